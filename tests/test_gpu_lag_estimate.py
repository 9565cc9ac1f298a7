"""rho(r) estimated from the context frames, on the GPU: dgmr_lag_spectra (csrc/spectrum.hip) against the float64 specification of
stochastic.py on the same arrays, single-mode inputs, sign and identity, determinism, `estimate_rho` against its CPU path and the
nowcaster with rho="estimate".  No test has a time threshold."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import lag_recipe as LR
import stochastic_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/lag_estimate_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "lag_estimate_accuracy.json")
SENTINEL = -77.0
SHAPES = [(32, 64, 96), (64, 128, 64), (128, 128, 256)]


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
    return t.contiguous().view(torch.int64)


def _strided_planes(x, extra):
    """x [N, H, W] on the device, its planes H * W + extra elements apart"""
    n, h, w = x.shape
    buf = torch.full((n, h * w + extra), SENTINEL, device="cuda")
    view = buf[:, :h * w].view(n, h, w)
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def _odd(x):
    """x [N, H, W] on the device, its first element one float past a 16-byte boundary"""
    flat = torch.full((x.size + 1,), SENTINEL, device="cuda")
    flat[1:].copy_(torch.from_numpy(np.array(x)).reshape(-1))
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == 4
    return view


def _run(a, b, window, **kw):
    from skillful_nowcasting_amd.stochastic import lag_spectra

    out = lag_spectra(a if torch.is_tensor(a) else torch.from_numpy(np.array(a)).cuda(),
                      b if torch.is_tensor(b) else torch.from_numpy(np.array(b)).cuda(), window, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(LR.LAG_CASES))
def test_lag_spectra_against_the_reference(name):
    """Radar-like dB planes with two different plane strides, `out` a view into a sentinel-filled buffer.  Per window, q and bin
    |device - reference| <= K 2 eps(L) L^2 n_q, K = 1/128 from the fp32 CPU implementation (lag_recipe.K); the all-zero window gives
    exact zeros (lag_ratio asserts it); the buffer is untouched outside the view; pointers one float off a 16-byte boundary (the
    4-byte loads) give the same bits."""
    window, h, w, n = LR.LAG_CASES[name]
    a, b, ref, norms = LR.lag_case(name)
    buf = torch.full((n + 2,) + ref.shape[1:], SENTINEL, dtype=torch.float64, device="cuda")
    view = buf[1:-1]
    got = _run(_strided_planes(a, 64), _strided_planes(b, 128), window, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert (buf[0] == SENTINEL).all() and (buf[-1] == SENTINEL).all()
    res = view.cpu().numpy()
    assert np.isfinite(res).all() and (res[0, 0] == 0).all()
    dev = LR.lag_ratio(res, ref, norms, window)
    cpu = LR.lag_ratio(LR.lag_spectra_fp32(a, b, window), ref, norms, window)
    print(f"{name}: worst |error| / (2 eps(L) L^2 n_q): device {dev:.3e}, fp32 CPU implementation {cpu:.3e}; K = {LR.K:.3e}")
    _log_accuracy("lag_spectra " + name, {"device_ratio": dev, "fp32_cpu_ratio": cpu, "K": LR.K, "eps": R.eps(window)})
    assert dev <= LR.K
    odd = _run(_odd(a), _odd(b), window)
    assert torch.equal(_bits(odd), _bits(view))
    mixed = _run(_odd(a), _strided_planes(b, 128), window)  # one pointer misaligned is enough for the 4-byte path
    assert torch.equal(_bits(mixed), _bits(view))


@pytest.mark.parametrize("window,h,w", SHAPES)
def test_single_mode_inputs(window, h, w):
    """A constant puts all of q = 0 into bin 0; (-1)^x and (-1)^y into bin L / 2 with value L^4 (the Nyquist column doubled, or lost,
    shows here); (-1)^(x + y) into bin round(L / sqrt 2) (a dropped corner bin shows here).  Everything within the criterion."""
    from skillful_nowcasting_amd.stochastic import lag_spectra_reference

    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    planes = np.stack([np.full((h, w), 3.0), 1.0 - 2.0 * (x % 2), 1.0 - 2.0 * (y % 2), 1.0 - 2.0 * ((x + y) % 2)]).astype(np.float32)
    ref = lag_spectra_reference(planes, planes, window)
    norms = LR.window_norms(planes, planes, window)
    got = _run(planes, planes, window).cpu().numpy()
    ratio = LR.lag_ratio(got, ref, norms, window)
    print(f"L={window} single modes: worst |error| / (2 eps(L) L^2 n_q) = {ratio:.3e}")
    assert ratio <= LR.K
    tol = LR.K * 2.0 * R.eps(window) * float(window) ** 4  # n_q = L^2 for the +-1 planes
    l4 = float(window) ** 4
    for plane, r, value in ((0, 0, 9.0 * l4), (1, window // 2, l4), (2, window // 2, l4), (3, int(round(window / np.sqrt(2.0))), l4)):
        scale = value / l4
        assert (np.abs(got[plane, :, :, r] - value) <= tol * scale).all(), (plane, r, got[plane, 0, :, r])
        rest = np.delete(got[plane], r, axis=-1)
        assert (np.abs(rest) <= tol * scale).all(), (plane, np.abs(rest).max())
        assert (np.abs(ref[plane, :, :, r] - value) <= 1e-9 * value).all()


@pytest.mark.parametrize("name", sorted(LR.LAG_CASES))
def test_sign_and_identity(name):
    """b = a gives three bit-equal rows; b = -a gives q = 2 equal to -(q = 0), bit for bit, and q = 1 equal to q = 0."""
    window = LR.LAG_CASES[name][0]
    a = torch.from_numpy(np.array(LR.lag_case(name)[0])).cuda()
    same = _run(a, a.clone(), window)
    assert torch.equal(_bits(same[:, :, 0]), _bits(same[:, :, 1])) and torch.equal(_bits(same[:, :, 0]), _bits(same[:, :, 2]))
    assert (same[:, :, 0].sum(dim=(1, 2)) > 0).all()
    neg = _run(a, -a, window)
    assert torch.equal(_bits(neg[:, :, 0]), _bits(same[:, :, 0])) and torch.equal(_bits(neg[:, :, 1]), _bits(same[:, :, 0]))
    assert torch.equal(neg[:, :, 2], -same[:, :, 0])  # by value: an all-zero window and an empty bin give +0, not -0


@pytest.mark.parametrize("name", ["L32 64x96", "L64 128x64"])
def test_determinism_and_plane_independence(name):
    """Two calls give equal bits; a call on N planes equals N calls on one plane."""
    window = LR.LAG_CASES[name][0]
    a, b = LR.lag_case(name)[:2]
    one, two = _run(a, b, window), _run(a, b, window)
    assert torch.equal(_bits(one), _bits(two))
    for i in range(2):
        single = _run(np.ascontiguousarray(a[i:i + 1]), np.ascontiguousarray(b[i:i + 1]), window)
        assert torch.equal(_bits(single[0]), _bits(one[i]))


def test_argument_errors_leave_the_output_untouched():
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.stochastic import lag_spectra

    lib = _lib.load()
    h, w = 64, 96
    a, b = torch.zeros(2, h, w, device="cuda"), torch.zeros(2, h, w, device="cuda")
    out = torch.full((2, 15, 3, 32), SENTINEL, dtype=torch.float64, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(L=32, H=h, W=w, N=2, pa=a.data_ptr(), pb=b.data_ptr(), o=out.data_ptr(), sa=h * w, sb=h * w):
        return lib.dgmr_lag_spectra(pa, sa, pb, sb, N, H, W, L, o, st)

    for kw in ({"L": 16}, {"L": 256}, {"H": 80}, {"W": 100}, {"N": 0}, {"pa": None}, {"pb": None}, {"o": None}, {"sa": h * w - 4},
               {"sb": h * w - 1}):
        assert raw(**kw) < 0 and b"dgmr_lag_spectra" in lib.dgmr_last_error(), kw
    for bad in (lambda: lag_spectra(a, b, 16, out=out), lambda: lag_spectra(a[:, :, :80], b[:, :, :80], 32),
                lambda: lag_spectra(a, b[:1], 32, out=out), lambda: lag_spectra(a, b.cpu(), 32, out=out),
                lambda: lag_spectra(a, b, 32, out=out[:, :14]), lambda: lag_spectra(a, b, 32, out=out.float())):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- the estimator and the nowcaster -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translating():
    seq = R.translating_db_context()  # [5, 128, 128], v = (2, -3) pixels per frame
    return seq, torch.from_numpy(seq[:4])[:, None].contiguous()


def test_estimate_rho_on_the_device_against_the_cpu_path(translating):
    """An explicit uniform integer field: the alignment is a bit-exact copy on both paths, so the kernel is the only source of a
    difference.  With E_q = sum over the pooled windows and pairs of K 2 eps(L) L^2 n_q, gamma = C / sqrt(Pa Pb) and |gamma| <= 1:
    |device - CPU| <= (E_c / sqrt(Pa Pb) + (E_a / Pa + E_b / Pb) / 2) (1 + 1e-2) + 2^-23  (first order; the last terms: the second
    order and the rounding of both results to fp32)."""
    from skillful_nowcasting_amd.stochastic import estimate_rho, lag_spectra_reference, lagrangian_frames, to_db, window_table

    window, size = 64, 128
    # the translating context plus an independent radar-like field per frame: coherences well inside (0, 1)
    z = to_db(translating[1]) + 0.5 * torch.from_numpy(R.db_field(4, size, size, seed=40))[:, None]
    field = torch.tensor([2.0, -3.0]).view(1, 1, 1, 2)
    lf = lagrangian_frames(z, field)
    lf_dev = lagrangian_frames(z.cuda(), field.cuda())
    assert torch.equal(lf_dev.cpu(), lf)
    cpu = estimate_rho(z, field, 0.0, 1.0, window)
    dev = estimate_rho(z.cuda(), field.cuda(), 0.0, 1.0, window)
    torch.cuda.synchronize()
    assert dev.rho.is_cuda and dev.rho.dtype == torch.float32 and tuple(dev.rho.shape) == (1, window)
    assert cpu.windows[0] == 1 and dev.windows.cpu()[0] == 1  # margin ceil(3 * 3) + 1 = 10: the window at (32, 32)
    a, b = lf[:-1, 0].numpy(), lf[1:, 0].numpy()
    table = window_table(size, size, window)
    used = np.minimum(np.minimum(table[:, 2], table[:, 3]), size - window - np.maximum(table[:, 2], table[:, 3])) >= 10
    assert used.sum() == 1
    pooled = lag_spectra_reference(a, b, window)[:, used].sum(axis=(0, 1))  # [3, L]
    err = (LR.K * 2.0 * R.eps(window) * window * window * LR.window_norms(a, b, window)[:, used]).sum(axis=(0, 1))  # [3]
    have = pooled[0] * pooled[1] > 0
    root = np.sqrt(np.where(have, pooled[0] * pooled[1], 1.0))
    tol = (err[2] / root + 0.5 * (err[0] / np.where(have, pooled[0], 1.0) + err[1] / np.where(have, pooled[1], 1.0))) * 1.01 + 2.0 ** -23
    gap = np.abs(dev.rho.cpu().numpy()[0].astype(np.float64) - cpu.rho.numpy()[0])
    worst = float((gap / tol)[have].max())
    print(f"estimate_rho device against CPU: worst gap {gap.max():.3e}, worst gap / tolerance {worst:.3e}")
    _log_accuracy("estimate_rho 128x128 L=64 uniform field", {"worst_gap": float(gap.max()), "worst_gap_over_tolerance": worst})
    assert (gap[have] <= tol[have]).all() and (gap[~have] == 0).all()
    inner = cpu.rho[0].numpy()[have][1:]
    # most bins are not clipped: the comparison is of the coherences themselves (the clip is 1-Lipschitz, so the bound holds for the rest)
    assert ((inner > 0) & (inner < 0.999)).sum() >= len(inner) // 2


def test_translation_is_persistence_on_the_device(translating):
    from skillful_nowcasting_amd.advection import lattice_geometry, motion_field
    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import estimate_rho, to_db

    ctx = translating[1].cuda()
    field = motion_field(ctx)
    origin, spacing = lattice_geometry(32, 16)
    est = estimate_rho(to_db(ctx), field, origin, spacing, 64)
    holds = np.bincount(_radial_bins(64).reshape(-1), minlength=64) > 0
    rho = est.rho.cpu().numpy()[0]
    print(f"translation on the device: min rho over the bins with modes = {rho[holds].min():.6f}")
    assert est.windows.cpu()[0] == 1 and rho[0] == 1 and (rho[holds] >= 0.99).all() and (rho <= 1).all()
    low = estimate_rho(to_db(ctx), field, origin, spacing, 64, margin=0).rho.cpu().numpy()[0][holds].min()
    assert low < 0.9


def test_nowcaster_with_estimated_rho(translating):
    """rho="estimate" on two cases: last_rho is [P, L] in [0, 1] with column 0 one; the nowcast is bit-identical to the one of a
    nowcaster that is given each plane's row; the members pass through the three verifiers."""
    from skillful_nowcasting_amd.spectra import SpectrumVerifier
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster
    from skillful_nowcasting_amd.value import ValueVerifier
    from skillful_nowcasting_amd.verification import NowcastVerifier

    seq = translating[0]
    m, steps, window = 4, 2, 64
    images = torch.from_numpy(np.stack([seq[:4], seq[1:5][::-1].copy()]))[:, :, None].cuda()  # [B = 2, T_in, C = 1, H, W]
    nc = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho="estimate")
    white = nc.white_noise(2, m, 128, 128, "cuda", seed=4)
    fc = nc.nowcast_batch(images, m, white=white)
    rho = nc.last_rho
    assert tuple(fc.shape) == (m, 2, steps, 1, 128, 128) and torch.isfinite(fc).all() and (fc >= 0).all()
    assert rho.is_cuda and rho.dtype == torch.float32 and tuple(rho.shape) == (2, window)
    assert (rho >= 0).all() and (rho <= 1).all() and (rho[:, 0] == 1).all() and (nc.last_windows == 1).all()
    for p in range(2):
        explicit = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=rho[p].cpu())
        got = explicit.nowcast_batch(images[p:p + 1], m, white=white[p:p + 1])
        assert torch.equal(got[:, 0].contiguous().view(torch.int32), fc[:, p].contiguous().view(torch.int32))
        assert explicit.last_rho is None
    for a in range(m):
        for b in range(a + 1, m):
            assert not torch.equal(fc[a], fc[b])
    observed = torch.from_numpy(np.stack([seq[4], seq[4]]))[:, None].cuda()  # [T, C, H, W]
    member_fc = fc[:, 0]  # [M, T, C, H, W]
    ver, spec, val = NowcastVerifier(m, steps), SpectrumVerifier(m, steps, window=64), ValueVerifier(m, steps)
    for v in (ver, spec, val):
        v.update(member_fc, observed)
    res, res_spec, res_val = ver.compute(), spec.compute(), val.compute()
    ranks = np.asarray(res["rank_histogram"], dtype=np.float64)
    assert np.allclose(ranks.sum(axis=-1), 1.0) and ranks.shape[-1] == m + 1
    assert np.isfinite(res_spec["psd_forecast"]).all() and np.isfinite(res_val["brier"]).all()
