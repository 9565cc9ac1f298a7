"""Velocity perturbations on the GPU: dgmr_advect_series_perturbed (csrc/advect.hip) against dgmr_advect_series, against shifted
sources and against the float64 specification of advection.py on the same arrays; the nowcaster after `perturb_velocities` end to
end against its CPU path, and its spread in NowcastVerifier.  No test has a time threshold."""
import json
import os

import numpy as np
import pytest
import torch

import advection_recipe as AR
import velocity_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/velocity_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "velocity_accuracy.json")


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("h,w", [(48, 81), (96, 128)])
def test_zero_amplitude_is_advect_series_bit_for_bit(h, w):
    """T = 18, a rotating 3 x 5 lattice per group of two planes and its unit directions: with all amplitudes 0 the perturbed kernel
    gives dgmr_advect_series' bits (W = 81: the 4-byte-store kernels, 96 x 128: the 16-byte ones)."""
    from skillful_nowcasting_amd.advection import advect_series, advect_series_perturbed, unit_directions

    n, steps, group = 4, 18, 2
    origin, spacing = R.geometry(h, w)
    x = _dev(R.series_source(h, w, n, steps))
    field = _dev(R.rotating_field(n // group, 3, 5, h, w, origin, spacing, 0.004))
    direction = unit_directions(field)
    assert float(direction.abs().min()) > 0 and not torch.equal(direction[0], direction[1])  # no trivial direction
    want = advect_series(x, field, origin, spacing, group)
    got = advect_series_perturbed(x, field, direction, torch.zeros(n, steps, 2, device="cuda"), origin, spacing, group)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, steps, h, w) and torch.equal(_bits(got), _bits(want))
    assert (want[:, -1] - torch.where(x[:, -1] >= 0, x[:, -1], torch.zeros_like(x[:, -1]))).abs().max().item() > 0.1


def _integer_amplitudes(n, steps):
    t, i = np.meshgrid(np.arange(steps), np.arange(n))
    return (((t * 7 + i * 3) % 5) - 2).astype(np.float32)  # -2 ... 2, another sequence per plane


@pytest.mark.parametrize("h,w", [(48, 80), (96, 128), (48, 81)])
@pytest.mark.parametrize("steps", [1, 18])
def test_uniform_integer_field_with_integer_amplitudes_is_bit_exact(h, w, steps):
    """v = (2, -3) as a 1 x 1 lattice shared by the planes and as a constant 3 x 5 lattice per plane.  Direction (1, 0) with integer
    a_par: lead t (0-based) is its own source shifted by (2 (t + 1) + sum a_par, -3 (t + 1)).  Direction (0, 1) with integer a_perp
    only: shifted by (2 (t + 1) - sum a_perp, -3 (t + 1)), the perpendicular of (uy, ux) being (-ux, uy).  Zeros shifted in, negative
    and NaN sources read as 0, bit for bit."""
    from skillful_nowcasting_amd.advection import advect_series_perturbed

    n = 2
    x = R.series_source(h, w, n, steps)
    clean = np.where(x >= 0, x, 0).astype(np.float32)
    xt = _dev(x)
    a = _integer_amplitudes(n, steps)
    total = np.cumsum(a, axis=1).astype(np.int64)
    zero = np.zeros_like(a)
    for kind, udir, amp, sign in (("parallel", (1.0, 0.0), np.stack([a, zero], axis=-1), 1), ("perpendicular", (0.0, 1.0), np.stack([zero, a], axis=-1), -1)):
        want = np.stack([np.stack([R.shifted(clean[i, t], 2 * (t + 1) + sign * int(total[i, t]), -3 * (t + 1)) for t in range(steps)])
                         for i in range(n)])
        for shape, origin, spacing in (((1, 1, 1), 0.0, 1.0), ((n, 3, 5), 7.5, 16.0)):
            field = torch.tensor([2.0, -3.0], device="cuda").expand(shape + (2,)).contiguous()
            direction = torch.tensor(udir, device="cuda").expand(shape + (2,)).contiguous()
            got = advect_series_perturbed(xt, field, direction, _dev(amp), origin, spacing)
            torch.cuda.synchronize()
            assert got.shape == (n, steps, h, w) and np.array_equal(got.cpu().numpy(), want), (kind, shape)


@pytest.mark.parametrize("name", sorted(R.ROTATING_CASES))
def test_rotating_field_against_the_reference(name):
    """A smooth rotating field on a 3 x 5 lattice per group of three planes (or one for all), its unit directions, amplitudes per plane
    that differ in sign and grow with t up to about 0.5 pixels per step, written into a [B, T, C, H, W] buffer through the two
    strides; nothing outside the channel is touched.  |device - float64 reference| <= c' T max(H, W) 2^-24 max|adjacent difference
    of x| + 4 * 2^-24 max|x|, c' = 50."""
    from skillful_nowcasting_amd.advection import advect_series_perturbed

    h, w, steps, shared = R.ROTATING_CASES[name]
    x, field, direction, amp, origin, spacing, ref, plain = R.rotating_case(name)
    n, c = x.shape[0], 2
    buf = torch.full((n, steps, c, h, w), -7.0, device="cuda")
    got = advect_series_perturbed(_dev(x), _dev(field), _dev(direction), _dev(amp), origin, spacing, R.FIELD_GROUP, out=buf[:, :, 1])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[:, :, 1].data_ptr() and (buf[:, :, 0] == -7.0).all()
    bound, clean = R.bound(x, steps, h, w)
    err = np.abs(buf[:, :, 1].cpu().numpy().astype(np.float64) - ref).max()
    moved = np.abs(ref[:, -1] - clean[:, -1]).max()
    perturbed = np.abs(amp).sum(axis=(1, 2)) > 0
    gap = np.abs(ref - plain).reshape(n, -1).max(axis=1)
    print(f"{name}: worst error {err:.3e}, bound {bound:.3e} (ratio {err / bound:.3e}); the field moved the frame by {moved:.2f}, the "
          f"perturbation by {gap[perturbed].min():.2f} at least")
    _log_accuracy(f"advect_series_perturbed {name}", {"worst_abs_error": float(err), "bound": float(bound), "error_over_bound": float(err / bound),
                                                      "c": R.PERTURBED_C, "least_effect_of_the_perturbation": float(gap[perturbed].min())})
    assert moved > 0.1  # the case does something
    assert perturbed.sum() == 4 and (gap[perturbed] > 0.1).all() and (gap[~perturbed] == 0).all()
    assert err <= bound


def test_repeatability_and_plane_independence():
    """Two calls give the same bits; plane n of the N = 6 call is the N = 1 call on that plane with its field plane and amplitude row."""
    from skillful_nowcasting_amd.advection import advect_series_perturbed

    x, field, direction, amp, origin, spacing, _ref, _plain = R.rotating_case("48x80 T=18")
    x, field, direction, amp = _dev(x), _dev(field), _dev(direction), _dev(amp)
    a = advect_series_perturbed(x, field, direction, amp, origin, spacing, R.FIELD_GROUP)
    b = advect_series_perturbed(x, field, direction, amp, origin, spacing, R.FIELD_GROUP)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))
    for n in range(x.shape[0]):
        g = n // R.FIELD_GROUP
        one = advect_series_perturbed(x[n:n + 1], field[g:g + 1], direction[g:g + 1], amp[n:n + 1], origin, spacing)
        assert torch.equal(_bits(one[0]), _bits(a[n])), n


def test_argument_errors_leave_the_output_untouched():
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.advection import _stream

    lib = _lib.load()
    n, steps, h, w = 2, 3, 16, 16
    x = torch.rand(n, steps, h, w, device="cuda")
    field = torch.ones(1, 1, 1, 2, device="cuda")
    amp = torch.ones(n, steps, 2, device="cuda")
    out = torch.full((n, steps, h, w), -7.0, device="cuda")

    def rc(direction=field.data_ptr(), amplitude=amp.data_ptr(), t=steps, group=1):
        return lib.dgmr_advect_series_perturbed(x.data_ptr(), steps * h * w, h * w, field.data_ptr(), 0, direction, 0, amplitude, group, n, h, w,
                                                1, 1, 0.0, 1.0, t, out.data_ptr(), steps * h * w, h * w, _stream(x.device))

    for kw, word in (({"direction": None}, "direction"), ({"amplitude": None}, "amplitude"), ({"t": 0}, "T=0"), ({"t": 65}, "T=65"),
                     ({"group": 0}, "field_group")):
        assert rc(**kw) < 0, kw
        assert word in lib.dgmr_last_error().decode(), (kw, lib.dgmr_last_error())
    torch.cuda.synchronize()
    assert (out == -7.0).all()
    assert rc() == 0  # and the same call with nothing wrong writes every element
    torch.cuda.synchronize()
    assert (out >= 0).all()


def test_nowcast_on_the_device_equals_the_cpu_path():
    """The same explicit white field and velocity noise through the kernels and through the references, 128 x 128, M = 2, T = 3,
    window 64: test_gpu_stochastic's criterion - motion fields within 8 match_eps, rain rates compared where the reference's advected
    dB value is further from `pad` than the dB tolerance, at most 1 % of the pixels left out - with the advection term extended by
    the direction lattices' gap times the sum of the amplitudes."""
    from skillful_nowcasting_amd.advection import unit_directions
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster

    case = R.nowcast_case()
    dev = EnsembleAdvectionNowcaster(forecast_steps=R.NC_T, window=R.NC_WINDOW, rho=case["rho"]).perturb_velocities("steps")
    got = dev.nowcast(case["frames"].cuda(), R.NC_M, white=case["white"].cuda(), velocity_noise=case["eps"])
    torch.cuda.synchronize()
    assert got.is_cuda and tuple(got.shape) == (R.NC_M, R.NC_T, 1, R.NC_SIZE, R.NC_SIZE) and dev.last_velocity_noise.is_cuda
    assert torch.equal(dev.last_velocity_noise.cpu(), case["eps"])
    field_gap = (dev.last_field.cpu() - case["field"]).abs().max().item()
    assert field_gap <= 8 * AR.match_eps(32), field_gap
    direction_gap = (unit_directions(dev.last_field).cpu() - unit_directions(case["field"])).abs().max().item()
    assert direction_gap <= R.largest_direction_gap(case["field"].numpy(), field_gap), direction_gap
    compared, tol_rate, tol = R.nowcast_tolerances(case, field_gap, direction_gap)
    left_out = 1.0 - compared.mean()
    err = np.abs(got.cpu().numpy().astype(np.float64) - case["want"])
    worst = float((err / tol_rate)[compared].max())
    print(f"perturbed nowcast device against CPU: field gap {field_gap:.3e} px, direction gap {direction_gap:.3e}, z tolerance {tol:.3e}, "
          f"{left_out * 100:.3f} % of the pixels within it of pad and left out, worst rate error / tolerance {worst:.3e}")
    _log_accuracy("nowcast 128x128 M=2 T=3 L=64 perturbed", {"field_gap_px": field_gap, "direction_gap": direction_gap, "z_tolerance": tol,
                                                             "left_out_share": float(left_out), "worst_rate_error_over_tolerance": worst})
    assert left_out <= 0.01
    assert (err <= tol_rate)[compared].all()


def test_velocity_perturbations_give_spread_that_grows_with_lead_time():
    """M = 4 with rho = 1 (the members are one field before the advection) through NowcastVerifier: without perturbations the members
    are identical and the CRPS' spread term sum |x_i - x_j| / (2 M^2) is 0; with "steps" it is positive at every lead time and larger
    at the last than at the first."""
    import stochastic_recipe as SR
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster
    from skillful_nowcasting_amd.verification import NowcastVerifier

    m, steps, window = 4, 3, 64
    seq = SR.translating_db_context(frames=4 + steps)
    frames = torch.from_numpy(seq[:4])[..., None].cuda()
    observed = torch.from_numpy(seq[4:])[:, None].cuda()  # [T, C, H, W]
    spread = {}
    for key, law in (("off", None), ("steps", "steps")):
        nc = EnsembleAdvectionNowcaster(forecast_steps=steps, window=window, rho=torch.ones(window)).perturb_velocities(law)
        fc = nc.nowcast(frames, m, seed=4)
        assert tuple(fc.shape) == (m, steps, 1, 128, 128) and torch.isfinite(fc).all() and (fc >= 0).all()
        ver = NowcastVerifier(m, steps)
        ver.update(fc, observed)
        res = ver.compute()
        # crps = |err| - pair / M^2, crps_fair = |err| - pair / (M (M - 1)): the spread term pair / M^2 is (M - 1) (crps - crps_fair)
        spread[key] = (m - 1) * (res["crps"]["avg"][1] - res["crps_fair"]["avg"][1])
        if key == "off":
            assert all(torch.equal(fc[0], fc[i]) for i in range(1, m))
        else:
            assert all(not torch.equal(fc[0], fc[i]) for i in range(1, m))
    print(f"CRPS spread term per lead time: off {spread['off']}, steps {spread['steps']}")
    assert (spread["off"] == 0).all()
    assert (spread["steps"] > 0).all() and spread["steps"][-1] > spread["steps"][0]
