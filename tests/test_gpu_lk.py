"""dgmr_lk_refine (csrc/advect.hip) on the GPU against the float64 specification advection.lk_refine_reference on the same arrays and
the same block match, its determinism, and motion_field(subpixel="lk") and both nowcasters on HIP tensors against the parabola.
Tiny frames only; no test has a time threshold."""
import json
import os

import numpy as np
import pytest
import torch

import lk_recipe as R
from conftest import BAND_LOG
from skillful_nowcasting_amd import advection as A

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/lk_refine_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "lk_refine_accuracy.json")
EIG_BOUND = 16 * 2.0 ** -24  # of lambda_max: one rounding in each difference, three in the square, at most four fp32 partial adds
# The largest deviations from the float64 specification measured on an MI355X over all parity cases (profiles/lk_refine_accuracy.json);
# the tests allow four times as much, for other boxes of the pool and another contraction of a * b + c.
V_MEASURED = 7.1e-7         # pixels (7.01e-7 at 84x100 32/16, 4 iterations); 4 x is far below 1e-3, a twentieth of the method's own error
RESIDUAL_MEASURED = 0.24    # in units of residual_unit() below (0.236, the same case)


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _device_match(match):
    """The float64 reference's block match as `block_match` returns it on the device: the refinement starts from the same d0."""
    return A.BlockMatch(torch.from_numpy(match.disp).cuda(), torch.from_numpy(match.cost.astype(np.float32)).cuda(),
                        torch.from_numpy(match.wet).cuda())


def _refine(prev, nxt, match, block, stride, iterations):
    res = A.lk_refine(prev, nxt, _device_match(match), block, stride, iterations)
    torch.cuda.synchronize()
    return res


def residual_unit(ref_residual, block, q_max):
    """What one rounding of r per pixel does to sum r^2 over the n = (block - 2)^2 pixels: with |dr| <= u = 2^-24 q_max,
    |sum (r + dr)^2 - sum r^2| <= 2 sqrt(n sum r^2) u + n u^2."""
    n, u = (block - 2) ** 2, 2.0 ** -24 * q_max
    return 2.0 * np.sqrt(n * ref_residual) * u + n * u * u


@pytest.mark.parametrize("iterations", [1, 4])
@pytest.mark.parametrize("name", sorted(R.PARITY_CASES))
def test_lk_refine_against_the_reference(name, iterations):
    """Every block of every plane: dry blocks as specified, the same blocks conditioned, eig within 16 * 2^-24 lambda_max, v and the
    residual within four times the largest deviation measured."""
    block, stride = R.PARITY_CASES[name][:2]
    prev, nxt = R.parity_case(name)
    match, ref = R.parity_reference(name, iterations)
    wet = np.isfinite(match.cost[..., 0])
    ratio = R.eig_ratio_of(ref.eig)
    stripe = prev.shape[0] - 1
    assert (ratio[:stripe][wet[:stripe]] >= R.MIN_RATIO).all() and (ref.eig[stripe][..., 0] == 0).all() and wet[stripe].all()
    if block == 32:
        assert (~wet[2]).any()  # the dry quarter
    got = _refine(torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(nxt)).cuda(), match, block, stride, iterations)
    assert got.v.dtype == torch.float32 and got.eig.dtype == torch.float64 and got.residual.dtype == torch.float64
    v, eig, residual = got.v.cpu().numpy().astype(np.float64), got.eig.cpu().numpy(), got.residual.cpu().numpy()
    assert v.shape == ref.v.shape and eig.shape == ref.eig.shape and residual.shape == ref.residual.shape
    assert (v[~wet] == 0).all() and (eig[~wet] == 0).all() and np.isposinf(residual[~wet]).all()
    cond = A.lk_conditioned(ref.eig)
    assert np.array_equal(A.lk_conditioned(eig), cond) and cond[:stripe][wet[:stripe]].all() and not cond[stripe].any()
    assert (v[stripe] == match.disp[stripe]).all()  # not conditioned: the integer match, bit for bit
    eig_dev = (np.abs(eig - ref.eig).max(axis=-1) / np.where(wet, ref.eig[..., 1], 1.0))[wet].max()
    v_dev = np.abs(v - ref.v)[wet].max()
    q_max = float(np.nanmax(nxt))
    res_dev = (np.abs(residual[wet] - ref.residual[wet]) / residual_unit(ref.residual[wet], block, q_max)).max()
    print(f"{name}, {iterations} iterations: eig {eig_dev / 2.0 ** -24:.2f} * 2^-24 lambda_max, v {v_dev:.3e} px, residual {res_dev:.2f} units")
    _log_accuracy(f"{name} iterations={iterations}", {"eig_over_2^-24_lambda_max": eig_dev / 2.0 ** -24, "v_px": v_dev,
                                                       "residual_units": res_dev, "blocks": int(wet.sum())})
    assert eig_dev <= EIG_BOUND
    assert 4 * V_MEASURED < 1e-3
    assert v_dev <= 4 * V_MEASURED
    assert res_dev <= 4 * RESIDUAL_MEASURED


def test_views_of_one_tensor_are_taken_in_place_and_two_launches_give_the_same_bits():
    name = "84x100 32/16"
    prev, nxt = R.parity_case(name)
    match, _ref = R.parity_reference(name, 4)
    both = torch.from_numpy(np.stack([prev, nxt])).cuda()  # [T, N, H, W]
    first = _refine(both[0], both[1], match, 32, 16, 4)
    second = _refine(both[0], both[1], match, 32, 16, 4)
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                           b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))
    # planes of one case in a [N, T, H, W] tensor: the plane stride is 2 H W, nothing is copied, the same bits
    apart = torch.from_numpy(np.stack([prev, nxt], axis=1)).cuda()
    assert apart[:, 0].stride(0) == 2 * 84 * 100
    third = _refine(apart[:, 0], apart[:, 1], match, 32, 16, 4)
    for a, b in zip(first, third):
        assert torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a.view(torch.int32),
                           b.view(torch.int64) if b.dtype == torch.float64 else b.view(torch.int32))


def _device_refine(prev, nxt):
    p, q = torch.from_numpy(prev).cuda(), torch.from_numpy(nxt).cuda()
    match = A.block_match(p, q, 32, 16, 8)
    lk = A.lk_refine(p, q, match, 32, 16)
    return A.BlockMatch(*(t.cpu().numpy() for t in match)), lk


def _device_vectors(prev, nxt):
    match, lk = _device_refine(prev, nxt)
    return match, lk.v.cpu().numpy(), lk.eig.cpu().numpy()


def test_integer_translation_is_returned_bit_for_bit():
    prev, nxt = R.field(7, 128, 128, R.CUT[32])[None], R.field(7, 128, 128, R.CUT[32], (1, -2))[None]
    match, lk = _device_refine(prev, nxt)
    usable = R.usable_blocks(match)
    assert usable.sum() >= 25 and (match.disp[usable] == np.array([1, -2])).all()
    assert (lk.v.cpu().numpy()[usable] == match.disp[usable]).all() and (lk.residual.cpu().numpy()[usable] == 0).all()


@pytest.mark.parametrize("shift", [(2.3, -1.6), (0.5, 0.5), (-3.75, 4.25)])
def test_subpixel_translation_beats_the_parabola_fourfold(shift):
    err_lk, err_par = R.subpixel_errors(_device_vectors, shift)
    _log_accuracy(f"per-block error, shift {shift}", {"lk_px": err_lk, "parabola_px": err_par})
    assert err_lk <= 0.25 * err_par
    assert err_lk <= 0.03


def test_forecast_error_at_lead_18_is_a_quarter_of_the_parabolas():
    errors = R.e2e_errors("cuda")
    _log_accuracy("forecast MAE, 192 x 192 moving by (2.3, -1.6), central 64 x 64",
                  {m: {f"lead {t}": float(errors[m][0][t - 1]) for t in (1, 9, 18)} for m in errors})
    R.check_e2e(errors)


def test_striped_blocks_do_not_vote_in_the_motion_field():
    frames = torch.from_numpy(R.half_striped_frames())[:, None].cuda()
    R.check_aperture(A.motion_field(frames, subpixel="lk")[0].cpu().numpy(), A.motion_field(frames, subpixel="parabola")[0].cpu().numpy())


def test_the_default_is_the_parabola_bit_for_bit():
    frames = torch.from_numpy(R.sequence(7, 128, 128, 3, (2.3, -1.6), R.CUT[32]))[:, None].cuda()
    default, parabola = A.motion_field(frames), A.motion_field(frames, subpixel="parabola")
    assert torch.equal(default.view(torch.int32), parabola.view(torch.int32))
    assert not torch.equal(default, A.motion_field(frames, subpixel="lk"))
