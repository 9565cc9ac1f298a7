"""The AR(2) recursion of the stochastic ensemble on the CPU: the coefficients against the Yule-Walker identities, the float64
specification against the AR(1) specification and against a pure swap of its two states, the accuracy factor of the device
criterion, the estimator's second lag, the nowcaster's order switch and the C ABI."""
import ctypes

import numpy as np
import pytest
import torch

import ar2_recipe as A
import stochastic_recipe as R
from skillful_nowcasting_amd import stochastic as S
from skillful_nowcasting_amd.spectra import _radial_bins


def test_coefficients_satisfy_yule_walker():
    """phi1 + phi2 r1 = r1 and g^2 = (1 - phi2^2)(1 - r1^2) to fp32 rounding everywhere; phi1 r1 + phi2 = r2 where the clip is
    inactive; r1 = 1 gives (1, 0, 0); a NaN rho2 gives phi2 = 0 and the AR(1) gain; both clips are reached."""
    window = 64
    rho1, rho2 = (torch.from_numpy(v) for v in A.case_rhos(window))
    coef = S.ar2_coefficients(rho1, rho2)
    assert coef.dtype == torch.float32 and tuple(coef.shape) == (3, window)
    phi1, phi2, g = (coef[i].double().numpy() for i in range(3))
    r1, r2 = rho1.double().numpy(), rho2.double().numpy()
    ulp = 2.0 ** -23
    assert (phi1[0], phi2[0], g[0]) == (1.0, 0.0, 0.0)
    assert phi2[1] == -1.0 and phi2[2] == 1.0 and g[1] == 0.0 and g[2] == 0.0  # both clips
    assert (np.abs(phi2) <= 1).all() and (g >= 0).all() and (g <= 1).all()
    rest = slice(1, None)
    # three rounded values enter each identity: |phi1| <= 2, |phi2| <= 1, g <= 1
    assert np.abs(phi1 + phi2 * r1 - r1)[rest].max() <= 3 * ulp
    assert np.abs(g * g - (1 - phi2 * phi2) * (1 - r1 * r1))[rest].max() <= 3 * ulp
    free = np.abs(phi2) < 1
    free[0] = False
    assert free.sum() == window - 3
    assert np.abs(phi1 * r1 + phi2 - r2)[free].max() <= 4 * ulp
    # no second lag measured: the AR(1) of r1
    nan = S.ar2_coefficients(rho1, torch.full_like(rho2, float("nan")))
    assert (nan[1] == 0).all() and torch.equal(nan[0], rho1) and np.array_equal(nan.numpy(), A.ar1_as_ar2(rho1.numpy()))
    # the input clips: rho1 below 0 or above 1, rho2 beyond +-1
    edge = S.ar2_coefficients(torch.tensor([-0.5, 1.5, 0.5, 0.5]), torch.tensor([0.3, 0.3, 7.0, -7.0]))
    assert np.allclose(edge[:, 0].numpy(), [0.0, 0.3, np.sqrt(1 - 0.09)]) and tuple(edge[:, 1].tolist()) == (1.0, 0.0, 0.0)
    assert tuple(edge[1, 2:].tolist()) == (1.0, -1.0) and tuple(edge[0, 2:].tolist()) == (0.0, 1.0)
    batch = S.ar2_coefficients(torch.stack([rho1, rho1]), torch.stack([rho2, rho2]))
    assert tuple(batch.shape) == (2, 3, window) and torch.equal(batch[1], coef)
    with pytest.raises(ValueError):
        S.ar2_coefficients(rho1, rho2[:-1])


@pytest.mark.parametrize("name", sorted(R.AR_CASES))
def test_phi2_zero_is_the_ar1_reference(name):
    """coef = (rho, 0, fp32 sqrt(1 - rho^2)) and any finite zm1: spectral_ar_reference's result up to the fp32 rounding of the gain -
    a relative 2^-24 on the drive terms against eps(L) = 32 log2 L 2^-24, so cell_ratio with the AR(1) majorant <= 1 / (32 log2 L)."""
    window, h, w, p, m, steps = R.AR_CASES[name]
    z0, white, rho, ref, cells = R.ar_case(name)
    coef = A.ar1_as_ar2(rho)
    worst = 0.0
    for seed in (50, 51):
        zm1 = R.db_field(p, h, w, seed=seed) * np.float32(3.0)
        got, _ = S.spectral_ar2_reference(z0, zm1, white, coef, window)
        worst = max(worst, R.cell_ratio(got, ref, cells, window))
    print(f"{name}: AR(2) reference with phi2 = 0 against the AR(1) reference, worst cell ratio {worst:.3e}, "
          f"bound {1.0 / (32.0 * np.log2(window)):.3e}")
    assert worst <= 1.0 / (32.0 * np.log2(window))


@pytest.mark.parametrize("name", sorted(A.AR2_CASES))
def test_pure_second_lag_alternates_the_two_states(name):
    """coef = (0, 1, 0): X_t = X_(t-2), so lead t (0-based) is the blended zm1 for even t and z0 for odd t - swapped lags show here.
    The weights sum to one: the reference returns the planes within 8 * 2^-24 of their largest value."""
    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white = A.ar2_case(name)[:3]
    coef = np.stack([np.zeros(window), np.ones(window), np.zeros(window)]).astype(np.float32)
    out, maj = S.spectral_ar2_reference(z0, zm1, white, coef, window)
    assert all((mj > 0).all() for mj in maj if mj.size)
    for t in range(steps):
        want = (zm1 if t % 2 == 0 else z0).astype(np.float64)[:, None]
        assert np.abs(out[:, :, t] - want).max() <= 8 * 2.0 ** -24 * np.abs(want).max(), t
    assert np.abs(z0 - zm1).max() > 1.0


def test_accuracy_factor_is_the_smallest_power_of_two():
    """The fp32 CPU implementation stays within half the bound with K2 and not with K2 / 2, on the inputs of the GPU test; those
    inputs give a finite reference and a positive majorant in every cell, the clipped bins phi2 = +-1 included."""
    worst = 0.0
    for name, case in A.AR2_CASES.items():
        z0, zm1, white, coef, ref, cells = A.ar2_case(name)
        assert np.isfinite(ref).all() and (cells > 0).all()
        flat = coef.reshape(-1, 3, case[0])
        assert (flat[0, 1, 1], flat[0, 1, 2]) == (-1.0, 1.0)
        ratio = R.cell_ratio(A.spectral_ar2_fp32(z0, zm1, white, coef, case[0]), ref, cells, case[0])
        print(f"{name}: fp32 CPU implementation, worst cell error / (eps(L) majorant) = {ratio:.3e}")
        worst = max(worst, ratio)
    assert A.K2 / 4.0 < worst <= A.K2 / 2.0
    assert np.frexp(A.K2)[0] == 0.5


def test_reference_and_cpu_path_shapes_and_refusals():
    name = "L32 64x96"
    window, h, w, p, m, steps = A.AR2_CASES[name]
    z0, zm1, white, coef, ref, _ = A.ar2_case(name)
    tz, tm, tw, tc = (torch.from_numpy(np.array(v)) for v in (z0, zm1, white, coef))
    got = S.spectral_ar2(tz, tm, tw, tc, window)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), ref.astype(np.float32))
    # a set per plane: plane 1 alone with its own row is plane 1 of the joint call
    alone, _ = S.spectral_ar2_reference(z0[1:], zm1[1:], white[1:], coef[1], window)
    assert np.array_equal(alone[0], ref[1]) and not np.array_equal(coef[0], coef[1])
    buf = torch.full((p, m, steps + 2, h, w), -7.0)
    view = S.spectral_ar2(tz, tm, tw, tc, window, out=buf[:, :, 1:-1])
    assert view.data_ptr() == buf[:, :, 1:-1].data_ptr() and torch.equal(buf[:, :, 1:-1], got) and (buf[:, :, 0] == -7).all()
    for bad in (lambda: S.spectral_ar2(tz, tm, tw, tc, 48), lambda: S.spectral_ar2(tz, tm[:1], tw, tc, window),
                lambda: S.spectral_ar2(tz, tm, tw, tc[:, :2], window), lambda: S.spectral_ar2(tz, tm, tw, tc.double(), window),
                lambda: S.spectral_ar2(tz, tm, tw[:, :, :0], tc, window), lambda: S.spectral_ar2(tz, tm.double(), tw, tc, window),
                lambda: S.spectral_ar2(tz, tm, tw, tc, window, out=buf[:, :, 1:]),
                lambda: S.spectral_ar2_reference(z0, zm1[:1], white, coef, window),
                lambda: S.spectral_ar2_reference(z0, zm1, white, coef[:, :, :16], window),
                lambda: S.spectral_ar2_reference(z0, zm1, white, coef, 256)):
        with pytest.raises(ValueError):
            bad()


def test_symbol_resolves_and_refuses_bad_arguments():
    """dgmr_spectral_ar2 is in the ctypes table and reports argument errors before any launch (no GPU here)."""
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    lib = _lib.load()
    assert "dgmr_spectral_ar2" in _lib.SIGNATURES and lib.dgmr_abi_version() == _lib.ABI_VERSION
    buf = (ctypes.c_float * 8)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def ar2(L=32, H=64, W=96, T=3, P=1, M=2, z0=p, zm1=p, white=p, coef=p, out=p, zs=None, cs=0, wms=None):
        plane = H * W
        return lib.dgmr_spectral_ar2(z0, plane if zs is None else zs, zm1, plane, white, T * plane if wms is None else wms, plane, coef, cs,
                                     P, M, T, H, W, L, out, T * plane, plane, None)

    for kw, word in (({"L": 16}, b"window"), ({"L": 256}, b"window"), ({"L": 48}, b"window"), ({"H": 80}, b"multiples"),
                     ({"W": 100}, b"multiples"), ({"H": 0}, b"multiples"), ({"T": 0}, b"lead times"), ({"T": 65}, b"lead times"),
                     ({"P": 0}, b"planes"), ({"M": 0}, b"planes"), ({"M": -1}, b"planes"), ({"z0": None}, b"null"), ({"zm1": None}, b"null"),
                     ({"white": None}, b"null"), ({"coef": None}, b"null"), ({"out": None}, b"null"), ({"zs": -4}, b"plane_stride"),
                     ({"cs": -96}, b"coef_plane_stride"), ({"cs": 95}, b"coef_plane_stride"), ({"wms": -1}, b"white_member_stride")):
        assert ar2(**kw) < 0 and word in lib.dgmr_last_error() and b"dgmr_spectral_ar2" in lib.dgmr_last_error(), kw


@pytest.fixture(scope="module")
def translating():
    """(dB context [4, 1, 128, 128], the matched field, origin, spacing) of the translating recipe, v = (2, -3) pixels per frame"""
    from skillful_nowcasting_amd.advection import lattice_geometry, motion_field

    ctx = torch.from_numpy(R.translating_db_context()[:4])[:, None].contiguous()
    field = motion_field(ctx)
    return (S.to_db(ctx), field) + lattice_geometry(32, 16)


def test_estimate_ar2_on_a_translation(translating):
    """rho1 is `estimate_rho`'s result, exactly; a field that only moves keeps its second lag too: rho2 >= 0.999 in every bin that holds
    modes (the float64 reference: >= 0.99945); `previous` is the Lagrangian frame before the last; K = 2 has no second lag - rho2 is
    NaN and phi2 = 0 everywhere."""
    z, field, origin, spacing = translating
    window = 64
    holds = np.bincount(_radial_bins(window).reshape(-1), minlength=window) > 0
    one = S.estimate_rho(z, field, origin, spacing, window)
    est = S.estimate_ar2(z, field, origin, spacing, window)
    assert est._fields == ("rho1", "rho2", "coef", "windows", "previous")
    assert torch.equal(est.rho1, one.rho) and torch.equal(est.windows, one.windows) and est.windows[0] == 1
    assert est.rho2.dtype == torch.float32 and tuple(est.rho2.shape) == (1, window) and tuple(est.coef.shape) == (1, 3, window)
    rho2 = est.rho2[0].numpy()
    print(f"translation: min rho2 over the bins with modes = {rho2[holds].min():.6f}, min rho1 = {est.rho1[0].numpy()[holds].min():.6f}")
    assert (rho2[holds] >= 0.999).all() and (rho2[holds] <= 1).all() and np.isnan(rho2[~holds]).all()
    assert torch.equal(est.coef, S.ar2_coefficients(est.rho1, est.rho2)) and torch.isfinite(est.coef).all()
    assert torch.equal(est.previous, S.lagrangian_frames(z, field, origin, spacing)[2]) and tuple(est.previous.shape) == (1, 128, 128)
    two = S.estimate_ar2(z[-2:], field, origin, spacing, window)
    assert torch.isnan(two.rho2).all() and (two.coef[:, 1] == 0).all()
    assert torch.equal(two.rho1, S.estimate_rho(z[-2:], field, origin, spacing, window).rho)
    assert torch.equal(two.coef[0], S.ar2_coefficients(two.rho1[0], two.rho2[0]))
    for bad in (dict(window=48), dict(window=64, margin=-1), dict(window=64, fallback=torch.ones(32))):
        with pytest.raises(ValueError):
            S.estimate_ar2(z, field, origin, spacing, **bad)
    with pytest.raises(ValueError):
        S.estimate_ar2(z[-1:], field, origin, spacing, 64)


def test_nowcaster_order_switch_on_the_cpu():
    """order=2 needs a second lag: rho=None raises; a [2, L] tensor and "estimate" run, the latter from the pieces called by hand;
    order=1 objects give what they gave (the default and an explicit order=1 are one code path) and keep no AR(2) state."""
    from skillful_nowcasting_amd.advection import advect_series, lattice_geometry

    seq = R.translating_db_context(size=64, frames=4)
    frames = torch.from_numpy(seq)[..., None]  # [T_in, H, W, C]
    kw = dict(forecast_steps=2, block=16, stride=16, radius=4, window=32)
    with pytest.raises(ValueError, match="second lag"):
        S.EnsembleAdvectionNowcaster(order=2, **kw)
    for bad in (3, 0, True):  # a bool is a positional probability_matching of a caller from before `order`: refused, not reinterpreted
        with pytest.raises(ValueError):
            S.EnsembleAdvectionNowcaster(order=bad, **kw)
    with pytest.raises(ValueError):
        S.EnsembleAdvectionNowcaster(order=2, rho=torch.ones(32), **kw)
    with pytest.raises(ValueError):
        S.EnsembleAdvectionNowcaster(order=1, rho=torch.ones(2, 32), **kw)
    old, new = S.EnsembleAdvectionNowcaster(**kw), S.EnsembleAdvectionNowcaster(order=1, **kw)
    white = old.white_noise(1, 2, 64, 64, "cpu", seed=1)
    base = old.nowcast(frames, 2, white=white)
    assert torch.equal(base, new.nowcast(frames, 2, white=white))
    assert old.order == 1 and old.last_rho2 is None and old.last_coef is None and old.last_rho is None
    rhos = torch.from_numpy(np.stack(A.case_rhos(32)))
    explicit = S.EnsembleAdvectionNowcaster(order=2, rho=rhos, **kw)
    out = explicit.nowcast(frames, 2, white=white)
    assert tuple(out.shape) == (2, 2, 1, 64, 64) and torch.isfinite(out).all() and (out >= 0).all() and not torch.equal(out, base)
    assert torch.equal(explicit.last_coef, S.ar2_coefficients(rhos[0], rhos[1])) and explicit.last_rho is None
    est = S.EnsembleAdvectionNowcaster(order=2, rho="estimate", **kw)
    got = est.nowcast(frames, 2, white=white)
    first = S.EnsembleAdvectionNowcaster(rho="estimate", **kw)
    first.nowcast(frames, 2, white=white)
    assert torch.equal(est.last_rho, first.last_rho) and torch.equal(est.last_windows, first.last_windows)
    assert tuple(est.last_rho2.shape) == (1, 32) and tuple(est.last_coef.shape) == (1, 3, 32)
    origin, spacing = lattice_geometry(16, 16)
    from skillful_nowcasting_amd.verification import observed_from_frames

    ctx = observed_from_frames(frames, 1.0, 0.0).contiguous()  # [T_in, C, H, W]
    parts = S.estimate_ar2(S.to_db(ctx), est.last_field, origin, spacing, 32)
    assert torch.equal(parts.coef, est.last_coef) and torch.allclose(parts.rho2, est.last_rho2, rtol=0, atol=0, equal_nan=True)
    z = S.spectral_ar2(S.to_db(ctx[-1]), parts.previous, white, parts.coef, 32)
    moved = advect_series(z.view(2, 2, 64, 64), est.last_field, origin, spacing, field_group=2)
    assert torch.equal(S.from_db(moved).view(1, 2, 2, 64, 64).permute(1, 2, 0, 3, 4), got)
