"""Velocity perturbations of the stochastic advection ensemble, host side: the float64 specification of
dgmr_advect_series_perturbed, unit_directions, velocity_perturbation_scale and EnsembleAdvectionNowcaster's CPU path with
`perturb_velocities`.  No GPU."""
import numpy as np
import pytest
import torch

import velocity_recipe as R
from skillful_nowcasting_amd import advection as A
from skillful_nowcasting_amd import stochastic as S


# ---- the specification -----------------------------------------------------------------------------------------------------------------
def test_zero_amplitude_is_the_unperturbed_reference():
    h, w, steps, n = 48, 81, 5, 4
    x = R.series_source(h, w, n, steps)
    origin, spacing = R.geometry(h, w)
    field = R.rotating_field(2, 3, 5, h, w, origin, spacing, 0.004)
    want = A.advect_series_reference(x, field, origin, spacing, 2)
    got = A.advect_series_perturbed_reference(x, field, R.unit(field), np.zeros((n, steps, 2), np.float32), origin, spacing, 2)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert np.abs(want[:, -1] - np.where(x[:, -1] >= 0, x[:, -1], 0)).max() > 0.1


def _uniform(v, shape):
    return np.broadcast_to(np.array(v, np.float32), shape + (2,)).copy()


@pytest.mark.parametrize("lattice", [(1, 1), (3, 5)])
def test_parallel_integer_amplitudes_shift_along_the_direction(lattice):
    """v = (2, -3), direction (1, 0), a_par[t] integers: lead t (0-based) is its own source shifted by (2 (t + 1) + sum a_par, -3 (t + 1))."""
    h, w, steps = 48, 80, 6
    x = R.series_source(h, w, 2, steps)
    clean = np.where(x >= 0, x, 0).astype(np.float64)
    a_par = np.array([[1, 0, -2, 3, 0, 1], [-1, -1, 0, 2, 0, 0]], np.float32)
    amp = np.stack([a_par, np.zeros_like(a_par)], axis=-1)
    got = A.advect_series_perturbed_reference(x, _uniform((2, -3), (1,) + lattice), _uniform((1, 0), (1,) + lattice), amp, 7.5, 16.0)
    for n in range(2):
        for t in range(steps):
            want = R.shifted(clean[n, t], 2 * (t + 1) + int(a_par[n, :t + 1].sum()), -3 * (t + 1))
            assert np.array_equal(got[n, t], want), (n, t)


def test_perpendicular_of_uy_ux_is_minus_ux_uy():
    """direction (0, 1) with a_perp: the perpendicular is (-1, 0), so the shift in y is 2 (t + 1) - sum a_perp and x is untouched by it."""
    h, w, steps = 48, 80, 4
    x = R.series_source(h, w, 1, steps)
    clean = np.where(x >= 0, x, 0).astype(np.float64)
    a_perp = np.array([[2, 1, 0, 3]], np.float32)
    amp = np.stack([np.zeros_like(a_perp), a_perp], axis=-1)
    got = A.advect_series_perturbed_reference(x, _uniform((2, -3), (1, 1, 1)), _uniform((0, 1), (1, 1, 1)), amp)
    for t in range(steps):
        assert np.array_equal(got[0, t], R.shifted(clean[0, t], 2 * (t + 1) - int(a_perp[0, :t + 1].sum()), -3 * (t + 1))), t
    # and direction (1, 0): the perpendicular is (0, 1), a shift in +x
    got = A.advect_series_perturbed_reference(x, _uniform((2, -3), (1, 1, 1)), _uniform((1, 0), (1, 1, 1)), amp)
    for t in range(steps):
        assert np.array_equal(got[0, t], R.shifted(clean[0, t], 2 * (t + 1), -3 * (t + 1) + int(a_perp[0, :t + 1].sum()))), t


def test_reference_and_wrapper_refusals():
    x = np.zeros((2, 3, 8, 8), np.float32)
    f = np.zeros((1, 1, 1, 2), np.float32)
    amp = np.zeros((2, 3, 2), np.float32)
    with pytest.raises(ValueError):
        A.advect_series_perturbed_reference(x, f, np.zeros((1, 2, 1, 2), np.float32), amp)
    with pytest.raises(ValueError):
        A.advect_series_perturbed_reference(x, f, f, amp[:, :2])
    xt, ft, at = torch.from_numpy(x), torch.from_numpy(f), torch.from_numpy(amp)
    assert tuple(A.advect_series_perturbed(xt, ft, ft, at).shape) == (2, 3, 8, 8)
    with pytest.raises(ValueError):
        A.advect_series_perturbed(xt, ft, ft.expand(1, 2, 1, 2), at)
    with pytest.raises(ValueError):
        A.advect_series_perturbed(xt, ft, ft.double(), at)
    with pytest.raises(ValueError):
        A.advect_series_perturbed(xt, ft, ft, at[:1])
    with pytest.raises(ValueError):
        A.advect_series_perturbed(xt, ft, ft, at.double())
    with pytest.raises(ValueError):
        A.advect_series_perturbed(xt, ft, ft, at, field_group=3)


def test_the_cpu_wrapper_is_the_reference_rounded_and_writes_views():
    name = "48x81 T=18"
    x, field, direction, amp, origin, spacing, ref, _ = R.rotating_case(name)
    n, steps, h, w = x.shape
    buf = torch.full((n, steps, 2, h, w), -7.0)
    got = A.advect_series_perturbed(torch.from_numpy(np.array(x)), torch.from_numpy(np.array(field)), torch.from_numpy(np.array(direction)),
                                    torch.from_numpy(np.array(amp)), origin, spacing, R.FIELD_GROUP, out=buf[:, :, 1])
    assert got.data_ptr() == buf[:, :, 1].data_ptr() and (buf[:, :, 0] == -7.0).all()
    assert np.array_equal(buf[:, :, 1].numpy(), ref.astype(np.float32))


def test_symbol_header_and_table_agree():
    from skillful_nowcasting_amd import _lib

    lib = _lib.load()
    assert "dgmr_advect_series_perturbed" in _lib.SIGNATURES and hasattr(lib, "dgmr_advect_series_perturbed")
    assert len(_lib.SIGNATURES["dgmr_advect_series_perturbed"]) == len(_lib.SIGNATURES["dgmr_advect_series"]) + 3
    assert lib.dgmr_abi_version() == _lib.ABI_VERSION


def test_argument_errors_come_before_any_launch():
    """Null direction or amplitude, bad T, field_group = 0, a negative direction stride: rc < 0 and a message, with no device at all."""
    from skillful_nowcasting_amd import _lib

    lib = _lib.load()
    fn = lib.dgmr_advect_series_perturbed
    ok = dict(x=8, xs=64, xt=64, f=8, fs=0, d=8, ds=0, a=8, g=1, n=1, h=8, w=8, gy=1, gx=1, o=0.0, s=1.0, t=2, out=8, ops=128, oss=64)

    def rc(**kw):
        v = dict(ok, **kw)
        return fn(v["x"], v["xs"], v["xt"], v["f"], v["fs"], v["d"], v["ds"], v["a"], v["g"], v["n"], v["h"], v["w"], v["gy"], v["gx"],
                  v["o"], v["s"], v["t"], v["out"], v["ops"], v["oss"], None)

    for kw, word in (({"d": None}, "direction"), ({"a": None}, "amplitude"), ({"t": 0}, "T=0"), ({"t": 65}, "T=65"), ({"g": 0}, "field_group"),
                     ({"ds": -1}, "direction_plane_stride"), ({"x": None}, "null"), ({"s": 0.0}, "spacing")):
        assert rc(**kw) < 0, kw
        assert word in lib.dgmr_last_error().decode(), (kw, lib.dgmr_last_error())


# ---- unit_directions ---------------------------------------------------------------------------------------------------------------------
def test_unit_directions():
    f = torch.tensor([[[[3.0, -4.0], [0.0, 0.0]], [[float("nan"), 1.0], [1e-3, 0.0]]],
                      [[[0.0, 2.0], [float("inf"), 1.0]], [[-1e-20, 1e-20], [5.0, 12.0]]]])
    u = A.unit_directions(f)
    assert u.dtype == torch.float32 and u.shape == f.shape and u.is_contiguous()
    assert torch.equal(u[0, 0, 0], torch.tensor([0.6, -0.8]))
    for idx in ((0, 0, 1), (0, 1, 0), (1, 0, 1)):  # zero, NaN, inf
        assert torch.equal(u[idx], torch.zeros(2)), idx
    assert torch.equal(u[0, 1, 1], torch.tensor([1.0, 0.0])) and torch.equal(u[1, 0, 0], torch.tensor([0.0, 1.0]))
    moving = [(0, 0, 0), (0, 1, 1), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
    for idx in moving:
        assert abs(float(u[idx].double().norm()) - 1.0) <= 2.0 ** -23, idx
    v = A.unit_directions(f, floor=0.01)
    assert torch.equal(v[0, 1, 1], torch.zeros(2)) and torch.equal(v[1, 1, 0], torch.zeros(2)) and torch.equal(v[0, 0, 0], u[0, 0, 0])
    assert torch.isfinite(u).all()
    with pytest.raises(ValueError):
        A.unit_directions(torch.zeros(3, 3))
    with pytest.raises(ValueError):
        A.unit_directions(f, floor=-1.0)


# ---- velocity_perturbation_scale -----------------------------------------------------------------------------------------------------
def test_scale_shape_dtype_formula_and_units():
    s = S.velocity_perturbation_scale(6)
    assert s.dtype == torch.float32 and tuple(s.shape) == (6, 2)
    p_par, p_perp = (3.0, 0.5, -1.0), (2.0, 0.25, 0.5)
    got = S.velocity_perturbation_scale(4, 10.0, 2.0, p_par, p_perp).numpy()
    t = (np.arange(4) + 1.0) * 10.0
    want = np.stack([np.maximum(a * t ** b + c, 0.0) for a, b, c in (p_par, p_perp)], axis=1) * 10.0 / 60.0 / 2.0
    assert np.array_equal(got, want.astype(np.float32))
    # units: with b = 0 the law does not depend on t, and sigma scales as timestep / km_per_pixel
    flat = ((4.0, 0.0, 1.0), (2.0, 0.0, 0.0))
    a = S.velocity_perturbation_scale(3, 5.0, 1.0, *flat).double()
    b = S.velocity_perturbation_scale(3, 10.0, 4.0, *flat).double()
    assert torch.allclose(b, a * (10.0 / 5.0) / 4.0, rtol=2.0 ** -22, atol=0) and (a[:, 0] == a[0, 0]).all()


def test_scale_clips_a_non_monotone_law_at_zero():
    s = S.velocity_perturbation_scale(5, 5.0, 1.0, (-1.0, 1.0, 12.0), (1.0, 1.0, -12.0)).numpy()  # 12 - t and t - 12, t = 5 ... 25
    assert (s >= 0).all()
    assert (s[:2, 0] > 0).all() and (s[2:, 0] == 0).all()
    assert (s[:2, 1] == 0).all() and (s[2:, 1] > 0).all()
    with pytest.raises(ValueError):
        S.velocity_perturbation_scale(0)
    with pytest.raises(ValueError):
        S.velocity_perturbation_scale(3, timestep=0.0)
    with pytest.raises(ValueError):
        S.velocity_perturbation_scale(3, p_par=(1.0, 2.0))


# ---- the nowcaster on the CPU ----------------------------------------------------------------------------------------------------------
M, T, SIZE, WINDOW = 3, 3, 64, 32
KW = dict(forecast_steps=T, block=16, stride=16, radius=4, window=WINDOW)


@pytest.fixture(scope="module")
def frames():
    return torch.from_numpy(R.translating_context(SIZE, 4))[..., None]  # [T_in, H, W, C]


@pytest.fixture(scope="module")
def plain(frames):
    nc = S.EnsembleAdvectionNowcaster(**KW)
    return nc, nc.nowcast(frames, M, seed=7)


def test_zero_velocity_noise_gives_the_bits_of_no_perturbation(frames, plain):
    nc = S.EnsembleAdvectionNowcaster(**KW).perturb_velocities("steps")
    out = nc.nowcast(frames, M, seed=7, velocity_noise=torch.zeros(1, M, 2))
    assert torch.equal(out.view(torch.int32), plain[1].view(torch.int32))
    assert torch.equal(nc.last_velocity_noise, torch.zeros(1, M, 2)) and plain[0].last_velocity_noise is None
    assert tuple(nc.velocity_scale.shape) == (T, 2) and torch.equal(nc.velocity_scale, S.velocity_perturbation_scale(T))


def test_a_seed_gives_the_same_noise_and_result(frames, plain):
    a = S.EnsembleAdvectionNowcaster(**KW).perturb_velocities("steps")
    b = S.EnsembleAdvectionNowcaster(**KW).perturb_velocities()
    ra, rb = a.nowcast(frames, M, seed=7), b.nowcast(frames, M, seed=7)
    assert a.last_velocity_noise.dtype == torch.float32 and tuple(a.last_velocity_noise.shape) == (1, M, 2)
    assert torch.equal(a.last_velocity_noise, b.last_velocity_noise) and torch.equal(ra.view(torch.int32), rb.view(torch.int32))
    assert torch.equal(a.last_velocity_noise, a.velocity_noise(1, M, 7))
    assert not torch.equal(a.velocity_noise(1, M, 7), a.velocity_noise(1, M, 8))
    assert not torch.equal(ra, plain[1])  # the perturbation does something
    batch = a.nowcast_batch(frames.permute(0, 3, 1, 2)[None].contiguous(), M, seed=7)
    assert tuple(batch.shape) == (M, 1, T, 1, SIZE, SIZE) and torch.equal(batch[:, 0].view(torch.int32), ra.view(torch.int32))


def test_the_white_noise_of_a_seed_does_not_change(plain):
    before = plain[0].white_noise(1, M, SIZE, SIZE, torch.device("cpu"), seed=11)
    on = S.EnsembleAdvectionNowcaster(**KW).perturb_velocities("steps")
    on.velocity_noise(1, M, 11)
    after = on.white_noise(1, M, SIZE, SIZE, torch.device("cpu"), seed=11)
    gen = torch.Generator().manual_seed(11)
    parent = torch.randn((1, M, T, SIZE, SIZE), generator=gen, dtype=torch.float32)  # the draw as it was before the feature
    assert torch.equal(before, after) and torch.equal(before, parent)


def test_parallel_noise_moves_the_rain_along_the_motion(frames):
    """rho = 1: the members are one field before the advection.  eps_par = +2, 0, -2: at the last lead time member 0's rain centroid
    lies further along the motion than member 1's, and member 2's less far."""
    nc = S.EnsembleAdvectionNowcaster(**KW, rho=torch.ones(WINDOW)).perturb_velocities("steps")
    eps = torch.tensor([[[2.0, 0.0], [0.0, 0.0], [-2.0, 0.0]]])
    out = nc.nowcast(frames, M, seed=3, velocity_noise=eps).numpy()
    v = nc.last_field.double().mean(dim=(0, 1, 2)).numpy()
    assert np.linalg.norm(v) > 1.0  # the context moves by (2, -3) per frame
    along = [float(R.centroid(out[m, -1, 0]) @ v / np.linalg.norm(v)) for m in range(M)]
    sigma = nc.velocity_scale[:, 0].double().sum().item()  # pixels of displacement per unit eps_par at the last lead time
    assert sigma > 0.1
    assert along[0] > along[1] > along[2], along


def test_the_device_tests_nowcast_case_is_sound_on_the_cpu():
    """The case of test_gpu_velocity's device-against-CPU nowcast, without a device: the float64 chain against the CPU path (the same
    chain with every stage rounded to fp32; no motion-field or direction gap) leaves at most 1 % of the pixels out and is within the
    criterion everywhere else."""
    case = R.nowcast_case()
    compared, tol_rate, tol = R.nowcast_tolerances(case, 0.0, 0.0)
    left_out = 1.0 - compared.mean()
    rate = S.from_db(torch.from_numpy(case["moved"]), case["threshold"], case["pad"]).numpy()
    err = np.abs(case["want"] - rate)
    print(f"z tolerance {tol:.3e}, {left_out * 100:.3f} % left out, worst rate error / tolerance {(err / tol_rate)[compared].max():.3e}")
    assert left_out <= 0.01
    assert (err <= tol_rate)[compared].all()
    assert np.abs(case["amplitude"]).max() > 0.5  # the members' velocities differ by more than half a pixel per step


def test_refusals(frames, plain):
    with pytest.raises(ValueError):
        S.EnsembleAdvectionNowcaster(**KW).perturb_velocities("bowler")
    for bad in (((1.0, 2.0, 3.0),), ((1.0, 2.0), (1.0, 2.0, 3.0)), ((1.0, 2.0, 3.0), (1.0, "x", 3.0)), 5.0,
                ((1.0, 2.0, float("nan")), (1.0, 2.0, 3.0))):
        with pytest.raises(ValueError):
            S.EnsembleAdvectionNowcaster(**KW).perturb_velocities(bad)
    with pytest.raises(TypeError):  # the constructor's arguments end with the mask's
        S.EnsembleAdvectionNowcaster(T, 16, 16, 4, 0.1, None, 2, WINDOW, 0.1, 5.0, None, 1, False, None, 0.0, "steps")
    nc = S.EnsembleAdvectionNowcaster(**KW).perturb_velocities(((1.0, 0.5, 0.0), (1.0, 0.5, 0.0)), timestep=10.0, km_per_pixel=2.0)
    assert nc.perturb_velocities(None) is nc and nc.velocity_scale is None  # and off again
    nc.perturb_velocities(((1.0, 0.5, 0.0), (1.0, 0.5, 0.0)), timestep=10.0, km_per_pixel=2.0)
    assert torch.equal(nc.velocity_scale, S.velocity_perturbation_scale(T, 10.0, 2.0, (1.0, 0.5, 0.0), (1.0, 0.5, 0.0)))
    for bad in (torch.zeros(1, M + 1, 2), torch.zeros(1, M, 3), torch.zeros(M, 2), torch.zeros(1, M, 2, dtype=torch.float64)):
        with pytest.raises(ValueError):
            nc.nowcast(frames, M, velocity_noise=bad)
    with pytest.raises(ValueError):  # nothing to apply it to
        plain[0].nowcast(frames, M, velocity_noise=torch.zeros(1, M, 2))
