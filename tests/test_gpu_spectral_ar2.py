"""The AR(2) recursion of the stochastic ensemble on the GPU: dgmr_spectral_ar2 (csrc/spectral_ar.hip) against the float64 specification
of stochastic.py on the same arrays, its reductions to the AR(1) kernel and to a swap of its two states, determinism, `estimate_ar2`
against its CPU path and the nowcaster with order=2 end to end.  No test has a time threshold."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import advection_recipe as AR
import ar2_recipe as A
import lag_recipe as LR
import stochastic_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/spectral_ar2_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "spectral_ar2_accuracy.json")
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


def _dev(x):
    return x.cuda() if torch.is_tensor(x) else torch.from_numpy(np.array(x)).cuda()


def _strided_planes(x, extra=64):
    """x [P, H, W] on the device, its planes H * W + extra elements apart"""
    p, h, w = x.shape
    buf = torch.full((p, h * w + extra), SENTINEL, device="cuda")
    view = buf[:, :h * w].view(p, h, w)
    view.copy_(torch.from_numpy(np.array(x)))
    return view


def _odd(x):
    """x on the device, its first element one float past a 16-byte boundary"""
    x = np.array(x)
    flat = torch.full((x.size + 1,), SENTINEL, device="cuda")
    flat[1:].copy_(torch.from_numpy(x).reshape(-1))
    view = flat[1:].view(x.shape)
    assert view.data_ptr() % 16 == 4
    return view


def _run(z0, zm1, white, coef, window, **kw):
    from skillful_nowcasting_amd.stochastic import spectral_ar2

    out = spectral_ar2(_dev(z0), _dev(zm1), _dev(white), _dev(coef), window, **kw)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", sorted(A.AR2_CASES))
def test_spectral_ar2_against_the_reference(name):
    """Radar-like dB fields with strided planes (two different strides), Gaussian noise, coefficients with both clips phi2 = +-1 (and a
    set per plane at L = 32), `out` a view into a sentinel-filled buffer.  Per L/2 x L/2 cell the 2-norm of device - reference is at
    most K2 eps(L) times the summed majorants of the windows over the cell, K2 = 1/64 from the fp32 CPU implementation
    (ar2_recipe.K2); the buffer is untouched outside the view; every pointer one float off a 16-byte boundary (the 4-byte path) gives
    the same numbers (the sign of a zero does not count)."""
    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white, coef, ref, cells = A.ar2_case(name)
    buf = torch.full((p, m, steps + 2, h, w), SENTINEL, device="cuda")
    view = buf[:, :, 1:-1]
    got = _run(_strided_planes(z0), _strided_planes(zm1, 128), white, coef, window, out=view)
    assert got.data_ptr() == view.data_ptr()
    assert (buf[:, :, 0] == SENTINEL).all() and (buf[:, :, -1] == SENTINEL).all()
    dev = R.cell_ratio(view.cpu().numpy(), ref, cells, window)
    cpu = R.cell_ratio(A.spectral_ar2_fp32(z0, zm1, white, coef, window), ref, cells, window)
    print(f"{name}: worst cell error / (eps(L) majorant): device {dev:.3e}, fp32 CPU implementation {cpu:.3e}; K2 = {A.K2:.3e}")
    _log_accuracy("spectral_ar2 " + name, {"device_ratio": dev, "fp32_cpu_ratio": cpu, "K2": A.K2, "eps": R.eps(window)})
    assert np.isfinite(view.cpu().numpy()).all()
    assert dev <= A.K2
    flat_o = torch.full((p * m * steps * h * w + 1,), SENTINEL, device="cuda")
    odd = _run(_odd(z0), _odd(zm1), _odd(white), _odd(coef), window, out=flat_o[1:].view(p, m, steps, h, w))
    assert odd.data_ptr() % 16 == 4 and flat_o[0] == SENTINEL
    assert torch.equal(odd, view)


@pytest.mark.parametrize("name", sorted(A.AR2_CASES))
def test_phi2_zero_ignores_the_second_state(name):
    """phi2 = 0 in every bin: two different finite zm1 give equal outputs - as numbers: 0 * X2 is a zero of X2's sign, which can flip the
    sign of a zero of an all-dry window."""
    from skillful_nowcasting_amd.stochastic import ar2_coefficients

    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white = A.ar2_case(name)[:3]
    rho1 = torch.from_numpy(A.case_rhos(window)[0])
    coef = ar2_coefficients(rho1, torch.full_like(rho1, float("nan")))
    assert (coef[1] == 0).all()
    a = _run(z0, zm1, white, coef, window)
    b = _run(z0, -3.0 * R.db_field(p, h, w, seed=77), white, coef, window)
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("name", sorted(A.AR2_CASES))
def test_pure_second_lag_alternates_the_two_states(name):
    """coef = (0, 1, 0): lead t (0-based) is the blended zm1 for even t and z0 for odd t, within the round trip's tolerance - the cell
    criterion against the reference, which itself returns the planes within 8 * 2^-24 of their largest value.  Swapped lags show here."""
    from skillful_nowcasting_amd.stochastic import spectral_ar2_reference

    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white = A.ar2_case(name)[:3]
    coef = np.stack([np.zeros(window), np.ones(window), np.zeros(window)]).astype(np.float32)
    ref, maj = spectral_ar2_reference(z0, zm1, white, coef, window)
    for t in range(steps):
        want = (zm1 if t % 2 == 0 else z0).astype(np.float64)[:, None]
        assert np.abs(ref[:, :, t] - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max()
    got = _run(z0, zm1, white, coef, window)
    ratio = R.cell_ratio(got.cpu().numpy(), ref, R.cell_majorant(maj, h, w, window), window)
    print(f"{name} alternation: worst cell error / (eps(L) majorant) {ratio:.3e}")
    assert ratio <= A.K2
    assert torch.equal(_bits(got[:, 0]), _bits(got[:, 1]))  # the gain is exactly 0: the noise does not enter


@pytest.mark.parametrize("name", ["L32 64x96", "L128 128x256"])
def test_repeatability_and_independence(name):
    """Two calls give equal bits; a call on M = 2 equals two calls on M = 1; with a set of coefficients per plane, plane 1 equals a
    one-plane call with its own set (the coefficient stride is honoured)."""
    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white, coef = A.ar2_case(name)[:4]
    a, b = _run(z0, zm1, white, coef, window), _run(z0, zm1, white, coef, window)
    assert torch.equal(_bits(a), _bits(b))
    for member in range(2):
        single = _run(z0, zm1, np.ascontiguousarray(white[:, member:member + 1]), coef, window)
        assert torch.equal(_bits(single[:, 0]), _bits(a[:, member]))
    if p > 1:
        assert coef.shape == (p, 3, window) and not np.array_equal(coef[0], coef[1])
        for plane in range(p):
            alone = _run(z0[plane:plane + 1], zm1[plane:plane + 1], white[plane:plane + 1], coef[plane], window)
            assert torch.equal(_bits(alone[0]), _bits(a[plane]))
        shared = _run(z0, zm1, white, coef[0], window)  # one set for all planes: stride 0
        assert torch.equal(_bits(shared[0]), _bits(a[0])) and not torch.equal(shared[1], a[1])


@pytest.mark.parametrize("name", sorted(R.AR_CASES))
def test_ar1_coefficients_against_the_ar1_kernel(name):
    """coef = (rho, 0, fp32 sqrt(1 - rho^2)) is the AR(1) recursion term for term: dgmr_spectral_ar2 and dgmr_spectral_ar are each
    within their own bound of the AR(1) reference.  Whether they are bit-equal is printed and logged, not asserted (two kernels may
    be contracted differently)."""
    from skillful_nowcasting_amd.stochastic import spectral_ar

    window, h, w, p, m, steps = R.AR_CASES[name]
    z0, white, rho, ref, cells = R.ar_case(name)
    zm1 = R.db_field(p, h, w, seed=60)
    two = _run(z0, zm1, white, A.ar1_as_ar2(rho), window)
    one = spectral_ar(_dev(z0), _dev(white), _dev(rho), window)
    torch.cuda.synchronize()
    r2, r1 = R.cell_ratio(two.cpu().numpy(), ref, cells, window), R.cell_ratio(one.cpu().numpy(), ref, cells, window)
    same_bits, same_numbers = bool(torch.equal(_bits(two), _bits(one))), bool(torch.equal(two, one))
    print(f"{name}: against the AR(1) reference, spectral_ar2 {r2:.3e} (K2 = {A.K2:.3e}), spectral_ar {r1:.3e} (K = {R.K:.3e}); "
          f"bit-equal: {same_bits}, equal as numbers: {same_numbers}")
    _log_accuracy("ar1 through spectral_ar2 " + name, {"spectral_ar2_ratio": r2, "spectral_ar_ratio": r1, "bit_equal": same_bits,
                                                        "equal_as_numbers": same_numbers})
    assert r2 <= A.K2 and r1 <= R.K


def test_argument_errors_leave_the_output_untouched():
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.stochastic import spectral_ar2

    lib = _lib.load()
    h, w, steps = 64, 96, 3
    z0, zm1 = torch.zeros(1, h, w, device="cuda"), torch.zeros(1, h, w, device="cuda")
    white = torch.zeros(1, 2, steps, h, w, device="cuda")
    coef = torch.ones(3, 32, device="cuda")
    out = torch.full((1, 2, steps, h, w), SENTINEL, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def raw(L=32, H=h, W=w, T=steps, P=1, M=2, z=z0.data_ptr(), zm=zm1.data_ptr(), wh=white.data_ptr(), c=coef.data_ptr(), o=out.data_ptr(),
            cs=0, zs=None):
        return lib.dgmr_spectral_ar2(z, H * W if zs is None else zs, zm, H * W, wh, T * H * W, H * W, c, cs, P, M, T, H, W, L, o, T * H * W,
                                     H * W, st)

    for kw in ({"L": 16}, {"L": 256}, {"H": 80}, {"W": 100}, {"T": 0}, {"T": 65}, {"P": 0}, {"M": 0}, {"z": None}, {"zm": None}, {"wh": None},
               {"c": None}, {"o": None}, {"cs": -96}, {"cs": 8}, {"zs": -4}):
        assert raw(**kw) < 0 and b"dgmr_spectral_ar2" in lib.dgmr_last_error(), kw
    for bad in (dict(window=16), dict(window=256)):
        with pytest.raises(ValueError):
            spectral_ar2(z0, zm1, white, coef, out=out, **bad)
    for bad in (lambda: spectral_ar2(z0[:, :, :80], zm1[:, :, :80], white[..., :80], coef, 32),
                lambda: spectral_ar2(z0, zm1, white[:, :, :0], coef, 32, out=out[:, :, :0]),
                lambda: spectral_ar2(z0, zm1, torch.zeros(1, 1, 65, h, w, device="cuda"), coef, 32),
                lambda: spectral_ar2(z0, zm1, white, coef[:, :16], 32, out=out), lambda: spectral_ar2(z0, zm1, white, coef[0], 32, out=out),
                lambda: spectral_ar2(z0, zm1.cpu(), white, coef, 32, out=out), lambda: spectral_ar2(z0, zm1[:, :32], white, coef, 32, out=out),
                lambda: spectral_ar2(z0, zm1, white, coef.cpu(), 32, out=out)):
        with pytest.raises(ValueError):
            bad()
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()


# ---- the estimator and the nowcaster -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translating():
    seq = R.translating_db_context()  # [5, 128, 128], v = (2, -3) pixels per frame
    return seq, torch.from_numpy(seq[:4])[:, None].contiguous()


def test_estimate_ar2_on_the_device_against_the_cpu_path(translating):
    """An explicit uniform integer field: the alignment is a bit-exact copy on both paths, so the kernel is the only source of a
    difference.  Per lag, with E_q = sum over the pooled windows and pairs of K 2 eps(L) L^2 n_q (lag_recipe.K, the criterion of
    dgmr_lag_spectra), gamma = C / sqrt(Pa Pb) and |gamma| <= 1:
    |device - CPU| <= (E_c / sqrt(Pa Pb) + (E_a / Pa + E_b / Pb) / 2) (1 + 1e-2) + 2^-23  (first order; the last terms: the second
    order and the rounding of both results to fp32).  rho is compared, not phi: near rho1 = 1 Yule-Walker is ill-conditioned."""
    from skillful_nowcasting_amd.stochastic import estimate_ar2, estimate_rho, lag_spectra_reference, lagrangian_frames, to_db, window_table

    window, size = 64, 128
    # the translating context plus an independent radar-like field per frame: coherences well inside (0, 1)
    z = to_db(translating[1]) + 0.5 * torch.from_numpy(R.db_field(4, size, size, seed=40))[:, None]
    field = torch.tensor([2.0, -3.0]).view(1, 1, 1, 2)
    lf = lagrangian_frames(z, field)
    cpu = estimate_ar2(z, field, 0.0, 1.0, window)
    dev = estimate_ar2(z.cuda(), field.cuda(), 0.0, 1.0, window)
    torch.cuda.synchronize()
    assert torch.equal(dev.previous.cpu(), lf[2]) and torch.equal(cpu.previous, lf[2])
    assert torch.equal(dev.rho1, estimate_rho(z.cuda(), field.cuda(), 0.0, 1.0, window).rho)
    assert cpu.windows[0] == 1 and dev.windows.cpu()[0] == 1  # margin ceil(3 * 3) + 1 = 10: the window at (32, 32)
    table = window_table(size, size, window)
    used = np.minimum(np.minimum(table[:, 2], table[:, 3]), size - window - np.maximum(table[:, 2], table[:, 3])) >= 10
    assert used.sum() == 1
    for lag, got_dev, got_cpu in ((1, dev.rho1, cpu.rho1), (2, dev.rho2, cpu.rho2)):
        assert got_dev.is_cuda and got_dev.dtype == torch.float32 and tuple(got_dev.shape) == (1, window)
        a, b = lf[:-lag, 0].numpy(), lf[lag:, 0].numpy()
        pooled = lag_spectra_reference(a, b, window)[:, used].sum(axis=(0, 1))  # [3, L]
        err = (LR.K * 2.0 * R.eps(window) * window * window * LR.window_norms(a, b, window)[:, used]).sum(axis=(0, 1))  # [3]
        have = pooled[0] * pooled[1] > 0
        root = np.sqrt(np.where(have, pooled[0] * pooled[1], 1.0))
        tol = (err[2] / root + 0.5 * (err[0] / np.where(have, pooled[0], 1.0) + err[1] / np.where(have, pooled[1], 1.0))) * 1.01 + 2.0 ** -23
        d, c = got_dev.cpu().numpy()[0].astype(np.float64), got_cpu.numpy()[0].astype(np.float64)
        if lag == 2:  # no fallback: NaN where the pool is empty, on both paths
            assert np.array_equal(np.isnan(d), ~have) and np.array_equal(np.isnan(c), ~have)
        else:
            assert (d[~have] == c[~have]).all()
        gap = np.abs(d - c)[have]
        worst = float((gap / tol[have]).max())
        print(f"estimate_ar2 device against CPU, lag {lag}: worst gap {gap.max():.3e}, worst gap / tolerance {worst:.3e}")
        _log_accuracy(f"estimate_ar2 128x128 L=64 uniform field, lag {lag}", {"worst_gap": float(gap.max()), "worst_gap_over_tolerance": worst})
        assert (gap <= tol[have]).all()
        inner = c[have][1:]
        assert ((inner > -0.999) & (inner < 0.999)).sum() >= len(inner) // 2  # most bins are not clipped
    assert tuple(dev.coef.shape) == (1, 3, window) and torch.isfinite(dev.coef).all()


def test_nowcast_order2_on_the_device_equals_the_cpu_path(translating):
    """order=2 with explicit (rho1, rho2), the same white field through the kernels and through the references, 128 x 128, M = 2,
    T = 3, window 64.  The tolerances are those of the order=1 test (test_gpu_stochastic.py): motion fields within 8 match_eps; the dB
    fields after the recursion within the cell bound; rain rates compared where the reference's advected z is further from `pad`
    than the dB tolerance.  The recursion has one more input, zm1, which each path advects for itself: the two zm1 differ by at most
    dgmr_advect's bound (asserted), and because the recursion is linear in zm1 the effect of that difference on z is the difference
    of two float64 references, one per zm1 - its largest value is added to the dB tolerance."""
    from skillful_nowcasting_amd.advection import advect, advect_series_reference, lattice_geometry
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, ar2_coefficients, spectral_ar2, spectral_ar2_reference, to_db
    from skillful_nowcasting_amd.verification import NowcastVerifier

    seq, _ = translating
    frames = torch.from_numpy(seq[:4])[..., None]
    m, steps, window, size = 2, 3, 64, 128
    rhos = torch.from_numpy(np.stack(A.case_rhos(window)))
    cpu = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=rhos, order=2)
    dev = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=rhos, order=2)
    white = torch.from_numpy(R.white_field((1, m, steps, size, size), seed=3))
    want = cpu.nowcast(frames, m, white=white)
    got = dev.nowcast(frames.cuda(), m, white=white.cuda())
    torch.cuda.synchronize()
    assert got.is_cuda and tuple(got.shape) == tuple(want.shape) == (m, steps, 1, size, size)
    assert torch.isfinite(got).all() and (got >= 0).all()
    coef = ar2_coefficients(rhos[0], rhos[1])
    assert torch.equal(dev.last_coef.cpu(), coef) and torch.equal(cpu.last_coef, coef)
    field_gap = (dev.last_field.cpu() - cpu.last_field).abs().max().item()
    assert field_gap <= 8 * AR.match_eps(32), field_gap
    origin, spacing = lattice_geometry(32, 16)
    z0, zprev = to_db(torch.from_numpy(seq[3])[None]), to_db(torch.from_numpy(seq[2])[None])
    zm1_cpu = advect(zprev, cpu.last_field, 1, origin, spacing)[:, -1]
    zm1_dev = advect(zprev.cuda(), dev.last_field, 1, origin, spacing)[:, -1]
    # one step of advection on each path: dgmr_advect's bound with T = 1, plus the field difference times the adjacent difference
    prev = zprev.numpy().astype(np.float64)
    adjacent_prev = max(np.abs(np.diff(np.pad(prev, [(0, 0)] + [(1, 1)] * 2), axis=-1)).max(),
                        np.abs(np.diff(np.pad(prev, [(0, 0)] + [(1, 1)] * 2), axis=-2)).max())
    zm1_gap = float((zm1_dev.cpu() - zm1_cpu).abs().max())
    zm1_bound = (ADVECT_C * size * 2.0 ** -24 + 2 * field_gap) * adjacent_prev + 5 * 2.0 ** -24 * prev.max()
    assert zm1_gap <= zm1_bound, (zm1_gap, zm1_bound)
    # the dB fields after spectral_ar2, from the same z0 and the CPU path's zm1
    ref, maj = spectral_ar2_reference(z0.numpy(), zm1_cpu.numpy(), white.numpy(), coef.numpy(), window)
    cells = R.cell_majorant(maj, size, size, window)
    z_dev = spectral_ar2(z0.cuda(), zm1_cpu.cuda(), white.cuda(), coef.cuda(), window)
    ratio = R.cell_ratio(z_dev.cpu().numpy(), ref, cells, window)
    assert ratio <= A.K2, ratio
    ref_other, _ = spectral_ar2_reference(z0.numpy(), zm1_dev.cpu().numpy(), white.numpy(), coef.numpy(), window)
    tol_zm1 = float(np.abs(ref_other - ref).max())
    # per pixel the dB fields differ by at most a cell's 2-norm bound and the effect of the other zm1; advection interpolates (a
    # convex combination) and adds its own bound and the field difference times the adjacent difference
    tol_z = float((A.K2 * R.eps(window) * cells).max()) + tol_zm1
    clean = np.where(ref >= 0, ref, 0.0)
    adjacent = max(np.abs(np.diff(np.pad(clean, [(0, 0)] * 3 + [(1, 1)] * 2), axis=-1)).max(),
                   np.abs(np.diff(np.pad(clean, [(0, 0)] * 3 + [(1, 1)] * 2), axis=-2)).max())
    tol = tol_z + (ADVECT_C * steps * size * 2.0 ** -24 + 2 * steps * field_gap) * adjacent + 5 * 2.0 ** -24 * clean.max()
    moved = advect_series_reference(ref.reshape(m, steps, size, size).astype(np.float32), cpu.last_field.numpy(), origin, spacing, m)
    moved = moved.reshape(1, m, steps, size, size).transpose(1, 2, 0, 3, 4)  # [M, T, C, H, W]
    compared = np.abs(moved - dev.pad) > tol
    left_out = 1.0 - compared.mean()
    rate_ref = want.numpy().astype(np.float64)
    # d rain / d z = rain ln(10) / 10; tol in z is small, so first order with a factor 2 of room, plus fp32 rounding of pow and log
    tol_rate = 2.0 * np.log(10.0) / 10.0 * tol * np.maximum(rate_ref, dev.threshold) + 16 * 2.0 ** -24 * np.maximum(rate_ref, dev.threshold)
    err = np.abs(got.cpu().numpy().astype(np.float64) - rate_ref)
    worst = float((err / tol_rate)[compared].max())
    print(f"order=2 nowcast device against CPU: field gap {field_gap:.3e} px, zm1 gap {zm1_gap:.3e} (bound {zm1_bound:.3e}, effect on z "
          f"{tol_zm1:.3e}), dB cell ratio {ratio:.3e}, z tolerance {tol:.3e}, {left_out * 100:.3f} % of the pixels within it of pad and "
          f"left out, worst rate error / tolerance {worst:.3e}")
    _log_accuracy("nowcast order=2 128x128 M=2 T=3 L=64", {"field_gap_px": field_gap, "zm1_gap": zm1_gap, "zm1_bound": float(zm1_bound),
                                                           "zm1_effect_on_z": tol_zm1, "db_cell_ratio": ratio, "z_tolerance": tol,
                                                           "left_out_share": float(left_out), "worst_rate_error_over_tolerance": worst})
    assert left_out <= 0.01
    assert (err <= tol_rate)[compared].all()
    # the members in the verifier, as a batch of one: [M, B, T, C, H, W]
    batch = dev.nowcast_batch(torch.from_numpy(seq[:4])[None, :, None].cuda(), m, white=white.cuda())
    assert tuple(batch.shape) == (m, 1, steps, 1, size, size) and torch.equal(_bits(batch[:, 0]), _bits(got))
    ver = NowcastVerifier(m, steps)
    ver.update(got, torch.from_numpy(np.stack([seq[4]] * steps))[:, None].cuda())
    ranks = np.asarray(ver.compute()["rank_histogram"], dtype=np.float64)
    assert np.allclose(ranks.sum(axis=-1), 1.0) and ranks.shape[-1] == m + 1


def test_nowcaster_order2_with_estimated_coefficients(translating):
    """rho="estimate", order=2, two cases: the nowcast is, bit for bit, the pieces called by hand on the device - `estimate_ar2`,
    one `spectral_ar2` with `last_coef` and `previous`, `advect_series`, `from_db`; `last_rho` is what an order=1 estimating nowcaster
    reports for the same context."""
    from skillful_nowcasting_amd.advection import advect_series, lattice_geometry
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, estimate_ar2, from_db, spectral_ar2, to_db

    seq = translating[0]
    m, steps, window = 2, 3, 64
    images = torch.from_numpy(np.stack([seq[:4], seq[1:5][::-1].copy()]))[:, :, None].cuda()  # [B = 2, T_in, C = 1, H, W]
    nc = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho="estimate", order=2)
    white = nc.white_noise(2, m, 128, 128, "cuda", seed=4)
    fc = nc.nowcast_batch(images, m, white=white)
    assert tuple(fc.shape) == (m, 2, steps, 1, 128, 128) and torch.isfinite(fc).all() and (fc >= 0).all()
    assert tuple(nc.last_rho.shape) == tuple(nc.last_rho2.shape) == (2, window) and tuple(nc.last_coef.shape) == (2, 3, window)
    assert (nc.last_windows == 1).all() and torch.isfinite(nc.last_coef).all() and (nc.last_coef[:, 1].abs() <= 1).all()
    context = images.permute(1, 0, 2, 3, 4).reshape(4, 2, 128, 128).contiguous()
    origin, spacing = lattice_geometry(32, 16)
    est = estimate_ar2(to_db(context), nc.last_field, origin, spacing, window)
    assert torch.equal(est.coef, nc.last_coef) and torch.equal(est.rho1, nc.last_rho)
    assert torch.equal(torch.nan_to_num(est.rho2, nan=7.0), torch.nan_to_num(nc.last_rho2, nan=7.0))
    z = spectral_ar2(to_db(context[-1]), est.previous, white, nc.last_coef, window)
    moved = advect_series(z.view(2 * m, steps, 128, 128), nc.last_field, origin, spacing, field_group=m)
    by_hand = from_db(moved).view(2, 1, m, steps, 128, 128).permute(2, 0, 3, 1, 4, 5)
    assert torch.equal(_bits(by_hand), _bits(fc))
    first = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho="estimate")
    other = first.nowcast_batch(images, m, white=white)
    assert torch.equal(first.last_rho, nc.last_rho) and first.last_rho2 is None and first.last_coef is None
    assert not torch.equal(other, fc)
