"""The stochastic advection ensemble on the GPU: dgmr_spectral_ar (csrc/spectral_ar.hip) and dgmr_advect_series (csrc/advect.hip) against
the float64 specifications of stochastic.py / advection.py on the same arrays, the nowcaster end to end against its CPU path, and its
members in the three verifiers.  No test has a time threshold."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import advection_recipe as AR
import stochastic_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/stochastic_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "stochastic_accuracy.json")
ADVECT_C = 22  # rounded fp32 operations per step in the position arithmetic of dgmr_advect[_series], both axes (include/dgmr_hip.h)
SENTINEL = -77.0


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _bits(t):
    return t.contiguous().view(torch.int32)


def _strided_planes(x, extra=64):
    """x [P, H, W] on the device, its planes H * W + extra elements apart"""
    p, h, w = x.shape
    buf = torch.full((p, h * w + extra), SENTINEL, device="cuda")
    view = buf[:, :h * w].view(p, h, w)
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def _run(z0, white, rho, window, **kw):
    from skillful_nowcasting_amd.stochastic import spectral_ar

    out = spectral_ar(z0 if torch.is_tensor(z0) else torch.from_numpy(np.array(z0)).cuda(),
                      white if torch.is_tensor(white) else torch.from_numpy(np.array(white)).cuda(),
                      rho if torch.is_tensor(rho) else torch.from_numpy(np.array(rho)).cuda(), window, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(R.AR_CASES))
def test_spectral_ar_against_the_reference(name):
    """Radar-like dB fields with strided planes, Gaussian noise, `out` a view into a sentinel-filled buffer.  Per L/2 x L/2 cell the
    2-norm of device - reference is at most K eps(L) times the summed majorants of the windows over the cell, K = 1/64 from the fp32
    CPU implementation (stochastic_recipe.K); the buffer is untouched outside the view; unaligned pointers (the 4-byte path) give
    the same bits."""
    window, h, w, p, m, steps = R.AR_CASES[name]
    z0, white, rho, ref, cells = R.ar_case(name)
    buf = torch.full((p, m, steps + 2, h, w), SENTINEL, device="cuda")
    view = buf[:, :, 1:-1]
    got = _run(_strided_planes(z0), white, rho, window, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert (buf[:, :, 0] == SENTINEL).all() and (buf[:, :, -1] == SENTINEL).all()
    dev = R.cell_ratio(view.cpu().numpy(), ref, cells, window)
    cpu = R.cell_ratio(R.spectral_ar_fp32(z0, white, rho, window), ref, cells, window)
    print(f"{name}: worst cell error / (eps(L) majorant): device {dev:.3e}, fp32 CPU implementation {cpu:.3e}; K = {R.K:.3e}")
    _log_accuracy("spectral_ar " + name, {"device_ratio": dev, "fp32_cpu_ratio": cpu, "K": R.K, "eps": R.eps(window)})
    assert np.isfinite(view.cpu().numpy()).all()
    assert dev <= R.K
    # every pointer one float off a 16-byte boundary: 4-byte loads and stores, the same arithmetic
    n = p * m * steps * h * w
    flat_z, flat_w, flat_o = (torch.full((k + 1,), SENTINEL, device="cuda") for k in (p * h * w, n, n))
    flat_z[1:].copy_(torch.from_numpy(np.array(z0)).reshape(-1))
    flat_w[1:].copy_(torch.from_numpy(np.array(white)).reshape(-1))
    odd = _run(flat_z[1:].view(p, h, w), flat_w[1:].view(p, m, steps, h, w), rho, window, out=flat_o[1:].view(p, m, steps, h, w))
    assert odd.data_ptr() % 16 == 4 and flat_o[0] == SENTINEL
    assert torch.equal(_bits(odd), _bits(view))


@pytest.mark.parametrize("window,h,w", [(32, 64, 96), (64, 128, 64), (128, 128, 256)])
def test_round_trip_and_nyquist(window, h, w):
    """rho = 1 returns the blended z0 at every lead time: the checkerboards (-1)^x and (-1)^y live in the Nyquist column and row;
    a constant comes back within 4 ulp at every pixel (the weights sum to one, also in the outer L / 2); the noise gain is exactly 0,
    so two members with different noise are bit-identical."""
    from skillful_nowcasting_amd.stochastic import spectral_ar_reference

    z0 = R.checkerboards(h, w, 3.0)
    white = R.white_field((4, 2, 2, h, w), seed=7)
    one = np.ones(window, np.float32)
    ref, maj = spectral_ar_reference(z0, white, one, window)
    got = _run(z0, white, one, window)
    ratio = R.cell_ratio(got.cpu().numpy(), ref, R.cell_majorant(maj, h, w, window), window)
    print(f"L={window} round trip: worst cell error / (eps(L) majorant) {ratio:.3e}")
    assert ratio <= R.K
    assert np.abs(ref - z0[:, None, None]).max() <= 8 * 2.0 ** -24 * np.abs(z0).max()  # the reference itself returns z0
    assert torch.equal(_bits(got[:, 0]), _bits(got[:, 1]))
    const = got[2].cpu().numpy()
    ulp = np.spacing(np.float32(3.0))
    assert np.abs(const.astype(np.float64) - 3.0).max() <= 4 * ulp, np.abs(const.astype(np.float64) - 3.0).max() / ulp
    err = np.abs(got.cpu().numpy() - z0[:, None, None]).max()
    assert err <= 1e-4, err  # the checkerboards come back: a lost Nyquist column would leave an error of 1


def test_memoryless_case_ignores_other_steps():
    """rho[r > 0] = 0: lead t depends on white[..., t - 1] alone - changing the other steps' noise changes no bit of it."""
    name = "L32 64x96"
    window, h, w, p, m, steps = R.AR_CASES[name]
    z0, white = R.ar_case(name)[:2]
    rho = np.zeros(window, np.float32)
    rho[0] = 1.0
    base = _run(z0, white, rho, window)
    for t in range(steps):
        other = R.white_field(white.shape, seed=100 + t)
        other[:, :, t] = white[:, :, t]
        got = _run(z0, other, rho, window)
        assert torch.equal(_bits(got[:, :, t]), _bits(base[:, :, t]))
        assert not torch.equal(_bits(got), _bits(base))


@pytest.mark.parametrize("name", ["L32 64x96", "L128 128x256"])
def test_repeatability_and_member_independence(name):
    """Two calls give equal bits; a call on M = 2 equals two calls on M = 1."""
    window = R.AR_CASES[name][0]
    z0, white, rho = R.ar_case(name)[:3]
    a, b = _run(z0, white, rho, window), _run(z0, white, rho, window)
    assert torch.equal(_bits(a), _bits(b))
    for member in range(2):
        single = _run(z0, np.ascontiguousarray(white[:, member:member + 1]), rho, window)
        assert torch.equal(_bits(single[:, 0]), _bits(a[:, member]))


def test_argument_errors_leave_the_output_untouched():
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.stochastic import spectral_ar

    lib = _lib.load()
    h, w, steps = 64, 96, 3
    z0 = torch.zeros(1, h, w, device="cuda")
    white = torch.zeros(1, 2, steps, h, w, device="cuda")
    rho = torch.ones(32, device="cuda")
    out = torch.full((1, 2, steps, h, w), SENTINEL, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(L=32, H=h, W=w, T=steps, z=z0.data_ptr(), wh=white.data_ptr(), r=rho.data_ptr(), o=out.data_ptr()):
        return lib.dgmr_spectral_ar(z, H * W, wh, T * H * W, H * W, r, 1, 2, T, H, W, L, o, T * H * W, H * W, st)

    for kw in ({"L": 16}, {"L": 256}, {"H": 80}, {"W": 100}, {"T": 0}, {"T": 65}, {"z": None}, {"wh": None}, {"r": None}, {"o": None}):
        assert raw(**kw) < 0 and b"dgmr_spectral_ar" in lib.dgmr_last_error(), kw
    for bad in (dict(window=16), dict(window=256)):
        with pytest.raises(ValueError):
            spectral_ar(z0, white, rho, out=out, **bad)
    with pytest.raises(ValueError):
        spectral_ar(z0[:, :, :80], white[..., :80], rho, 32)
    with pytest.raises(ValueError):
        spectral_ar(z0, white[:, :, :0], rho, 32, out=out[:, :, :0])
    with pytest.raises(ValueError):
        spectral_ar(z0, torch.zeros(1, 1, 65, h, w, device="cuda"), rho, 32)
    with pytest.raises(ValueError):
        spectral_ar(z0, white, rho[:16], 32, out=out)
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- advect_series -----------------------------------------------------------------------------------------------------------------
def _source(h, w, n):
    x = np.stack([AR.rain_field(5 + i, h, w) for i in range(n)])
    x[:, 3, 5] = np.nan
    x[:, h - 2, w - 3] = -1.0
    return x


def _rotating_field(n, gy, gx, h, w, origin, spacing, omega):
    f = np.empty((n, gy, gx, 2), np.float32)
    py = origin + spacing * np.arange(gy)[:, None]
    px = origin + spacing * np.arange(gx)[None, :]
    for i in range(n):
        om = omega * (1 + i)
        f[i, ..., 0] = om * (px - w / 2) + 0.3 * (i + 1)
        f[i, ..., 1] = -om * (py - h / 2) - 0.7
    return f


def test_advect_series_with_step_stride_zero_is_advect():
    """48 x 81 (the 4-byte path), T = 18: an expanded view of one source per plane gives `advect`'s bits."""
    from skillful_nowcasting_amd.advection import advect, advect_series

    h, w, steps = 48, 81, 18
    x = torch.from_numpy(_source(h, w, 2)).cuda()
    origin, spacing = 7.5, min((h - 16) / 2.0, (w - 16) / 4.0)
    field = torch.from_numpy(_rotating_field(2, 3, 5, h, w, origin, spacing, 0.004)).cuda()
    want = advect(x, field, steps, origin, spacing)
    got = advect_series(x[:, None].expand(2, steps, h, w), field, origin, spacing)
    torch.cuda.synchronize()
    assert got.shape == want.shape and torch.equal(_bits(got), _bits(want))
    x4 = torch.from_numpy(_source(48, 80, 2)).cuda()  # and the 16-byte path
    assert torch.equal(_bits(advect_series(x4[:, None].expand(2, steps, 48, 80), field, origin, spacing)),
                       _bits(advect(x4, field, steps, origin, spacing)))


@pytest.mark.parametrize("h,w", [(48, 80), (48, 81)])
def test_advect_series_uniform_integer_field_shifts_each_source(h, w):
    """A uniform integer field: lead t is ITS OWN source shifted by t v, zeros shifted in, bit for bit; negative values read as 0."""
    from skillful_nowcasting_amd.advection import advect_series

    steps, v = 5, (2, -3)
    x = np.stack([np.stack([AR.rain_field(20 + 7 * i + t, h, w) for t in range(steps)]) for i in range(2)])  # [2, T, h, w]
    x[:, :, 3, 5] = np.nan
    x[:, :, 7, 9] = -4.0
    x[1, 2][x[1, 2] > 1.0] *= -1.0  # a source with many negative values: all read as dry
    clean = np.where(x >= 0, x, 0).astype(np.float32)
    want = np.zeros_like(clean)
    for t in range(steps):
        dy, dx = v[0] * (t + 1), v[1] * (t + 1)
        want[:, t, dy:, :w + dx] = clean[:, t, :h - dy, -dx:]
    field = torch.tensor([float(v[0]), float(v[1])], device="cuda").view(1, 1, 1, 2)
    got = advect_series(torch.from_numpy(x).cuda(), field)
    torch.cuda.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)
    assert (got >= 0).all()


def test_advect_series_rotating_field_against_the_reference():
    """The rotating field of the advection test, a source per step, two members per field plane (field_group = 2), written through
    strides.  |device - reference| <= c T max(H, W) 2^-24 A + 4 * 2^-24 max|x|, A and max|x| over all steps' sources."""
    from skillful_nowcasting_amd.advection import advect_series, advect_series_reference

    h, w, steps, planes, group = 48, 80, 18, 2, 2
    n = planes * group
    base = _source(h, w, n)
    x = np.stack([base * np.float32(1.0 + 0.05 * t) for t in range(steps)], axis=1)  # [n, T, h, w]
    x[0, 4, 10:20, 10:30] = -3.0
    origin, spacing = 7.5, min((h - 16) / 2.0, (w - 16) / 4.0)
    field = _rotating_field(planes, 3, 5, h, w, origin, spacing, 0.004)
    ref = advect_series_reference(x, field, origin, spacing, group)
    buf = torch.full((n, steps, 2, h, w), -7.0, device="cuda")
    got = advect_series(torch.from_numpy(x).cuda(), torch.from_numpy(field).cuda(), origin, spacing, field_group=group, out=buf[:, :, 1])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[:, :, 1].data_ptr() and (buf[:, :, 0] == -7.0).all()
    clean = np.where(x >= 0, x, 0).astype(np.float64)
    adjacent = max(np.abs(np.diff(clean, axis=-1)).max(), np.abs(np.diff(clean, axis=-2)).max())
    bound = ADVECT_C * steps * max(h, w) * 2.0 ** -24 * adjacent + 4 * 2.0 ** -24 * clean.max()
    err = np.abs(buf[:, :, 1].cpu().numpy().astype(np.float64) - ref).max()
    print(f"advect_series {h} x {w}, T = {steps}: worst error {err:.3e}, bound {bound:.3e} (ratio {err / bound:.3e})")
    _log_accuracy(f"advect_series {h}x{w} T={steps} field_group={group}",
                  {"worst_abs_error": float(err), "bound": float(bound), "error_over_bound": float(err / bound), "c": ADVECT_C})
    assert np.abs(ref[2] - ref[0]).max() > 0.1  # the two field planes differ
    assert err <= bound


# ---- the nowcaster -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translating():
    seq = R.translating_db_context()  # [5, 128, 128]
    return seq, torch.from_numpy(seq[:4])[..., None], torch.from_numpy(seq[4:])[:, None]


def test_nowcast_on_the_device_equals_the_cpu_path(translating):
    """The same explicit white field through the kernels and through the references, 128 x 128, M = 2, T = 3, window 64: motion
    fields within 8 match_eps; the dB fields after spectral_ar within the cell bound; rain rates compared where the reference's
    advected z is further from `pad` than the dB tolerance (elsewhere wet / dry may flip) - at most 1 % of the pixels are left out."""
    from skillful_nowcasting_amd.advection import advect_series_reference, lattice_geometry
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, spectral_ar, spectral_ar_reference, to_db

    seq, frames, _ = translating
    m, steps, window, size = 2, 3, 64, 128
    rho = torch.from_numpy(R.case_rho(window))
    cpu = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=rho)
    dev = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=rho)
    white = torch.from_numpy(R.white_field((1, m, steps, size, size), seed=3))
    want = cpu.nowcast(frames, m, white=white)
    got = dev.nowcast(frames.cuda(), m, white=white.cuda())
    torch.cuda.synchronize()
    assert got.is_cuda and tuple(got.shape) == tuple(want.shape) == (m, steps, 1, size, size)
    field_gap = (dev.last_field.cpu() - cpu.last_field).abs().max().item()
    assert field_gap <= 8 * AR.match_eps(32), field_gap
    # the dB fields after spectral_ar, from the same z0
    z0 = to_db(torch.from_numpy(seq[3])[None])
    ref, maj = spectral_ar_reference(z0.numpy(), white.numpy(), rho.numpy(), window)
    cells = R.cell_majorant(maj, size, size, window)
    z_dev = spectral_ar(z0.cuda(), white.cuda(), rho.cuda(), window)
    ratio = R.cell_ratio(z_dev.cpu().numpy(), ref, cells, window)
    assert ratio <= R.K, ratio
    # per pixel the dB fields differ by at most a cell's 2-norm bound; advection interpolates (a convex combination) and adds its
    # own bound and the field difference times the adjacent difference
    tol_z = float((R.K * R.eps(window) * cells).max())
    clean = np.where(ref >= 0, ref, 0.0)
    adjacent = max(np.abs(np.diff(np.pad(clean, [(0, 0)] * 3 + [(1, 1)] * 2), axis=-1)).max(),
                   np.abs(np.diff(np.pad(clean, [(0, 0)] * 3 + [(1, 1)] * 2), axis=-2)).max())
    tol = tol_z + (ADVECT_C * steps * size * 2.0 ** -24 + 2 * steps * field_gap) * adjacent + 5 * 2.0 ** -24 * clean.max()
    origin, spacing = lattice_geometry(32, 16)
    moved = advect_series_reference(ref.reshape(m, steps, size, size).astype(np.float32), cpu.last_field.numpy(), origin, spacing, m)
    moved = moved.reshape(1, m, steps, size, size).transpose(1, 2, 0, 3, 4)  # [M, T, C, H, W]
    compared = np.abs(moved - dev.pad) > tol
    left_out = 1.0 - compared.mean()
    rate_ref = want.numpy().astype(np.float64)
    # d rain / d z = rain ln(10) / 10; tol in z is small, so first order with a factor 2 of room, plus fp32 rounding of pow and log
    tol_rate = 2.0 * np.log(10.0) / 10.0 * tol * np.maximum(rate_ref, dev.threshold) + 16 * 2.0 ** -24 * np.maximum(rate_ref, dev.threshold)
    err = np.abs(got.cpu().numpy().astype(np.float64) - rate_ref)
    worst = float((err / tol_rate)[compared].max())
    print(f"nowcast device against CPU: field gap {field_gap:.3e} px, dB cell ratio {ratio:.3e}, z tolerance {tol:.3e}, "
          f"{left_out * 100:.3f} % of the pixels within it of pad and left out, worst rate error / tolerance {worst:.3e}")
    _log_accuracy("nowcast 128x128 M=2 T=3 L=64", {"field_gap_px": field_gap, "db_cell_ratio": ratio, "z_tolerance": tol,
                                                   "left_out_share": float(left_out), "worst_rate_error_over_tolerance": worst})
    assert left_out <= 0.01
    assert (err <= tol_rate)[compared].all()


def test_members_in_the_verifiers(translating):
    """M = 4 members through NowcastVerifier, SpectrumVerifier and ValueVerifier; the members differ, with rho = 1 they do not."""
    from skillful_nowcasting_amd.spectra import SpectrumVerifier
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster
    from skillful_nowcasting_amd.value import ValueVerifier
    from skillful_nowcasting_amd.verification import NowcastVerifier

    seq, frames, _ = translating
    m, steps = 4, 2
    observed = torch.from_numpy(np.stack([seq[4], seq[4]]))[:, None].cuda()  # [T, C, H, W]
    nc = EnsembleAdvectionNowcaster(forecast_steps=steps, window=64, rho=torch.from_numpy(R.case_rho(64)))
    fc = nc.nowcast(frames.cuda(), m, seed=4)
    assert tuple(fc.shape) == (m, steps, 1, 128, 128) and torch.isfinite(fc).all() and (fc >= 0).all()
    for a in range(m):
        for b in range(a + 1, m):
            assert not torch.equal(fc[a], fc[b])
    ver, spec, val = NowcastVerifier(m, steps), SpectrumVerifier(m, steps, window=64), ValueVerifier(m, steps)
    for v in (ver, spec, val):
        v.update(fc, observed)
    res, res_spec, res_val = ver.compute(), spec.compute(), val.compute()
    ranks = np.asarray(res["rank_histogram"], dtype=np.float64)
    assert np.allclose(ranks.sum(axis=-1), 1.0) and ranks.shape[-1] == m + 1
    assert np.isfinite(res_spec["psd_forecast"]).all() and np.isfinite(res_val["brier"]).all()
    same = EnsembleAdvectionNowcaster(forecast_steps=steps, window=64, rho=torch.ones(64)).nowcast(frames.cuda(), m, seed=4)
    for a in range(1, m):
        assert torch.equal(_bits(same[a]), _bits(same[0]))
    batch = nc.nowcast_batch(torch.from_numpy(np.stack([seq[:4], seq[1:5]]))[:, :, None].cuda(), 2, seed=1)
    assert tuple(batch.shape) == (2, 2, steps, 1, 128, 128) and tuple(nc.last_field.shape) == (2, 7, 7, 2)
