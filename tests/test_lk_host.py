"""Lucas-Kanade refinement of the block match without a GPU: the float64 specification (advection.lk_refine_reference) against planted
sub-pixel translations and the parabola it replaces, stripes (the aperture problem), motion_field and both nowcasters on the CPU
path, and the C entry point's refusals."""
import ctypes

import numpy as np
import pytest
import torch

import lk_recipe as R
from skillful_nowcasting_amd import advection as A
from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster

SUBPIXEL_SHIFTS = [(2.3, -1.6), (0.5, 0.5), (-3.75, 4.25)]


def _match_and_refine(prev, nxt, block=32, stride=16, radius=8, iterations=4):
    match = A.block_match_reference(prev, nxt, block, stride, radius, 0.1, block * block // 16)
    return match, A.lk_refine_reference(prev, nxt, match.disp, match.cost, block, stride, iterations)


def test_integer_translation_is_returned_exactly():
    prev, nxt = R.field(7, 128, 128, R.CUT[32])[None], R.field(7, 128, 128, R.CUT[32], (1, -2))[None]
    match, lk = _match_and_refine(prev, nxt)
    usable = R.usable_blocks(match)
    assert usable.sum() >= 25
    assert (R.eig_ratio_of(lk.eig)[np.isfinite(match.cost[..., 0])] >= R.MIN_RATIO).all()
    assert (match.disp[usable] == np.array([1, -2])).all()
    assert (lk.v[usable] == match.disp[usable]).all() and (lk.residual[usable] == 0).all()
    assert lk.v.dtype == np.float64 and lk.eig.shape == (1, 7, 7, 2) and lk.residual.shape == (1, 7, 7)


def _reference_refine(prev, nxt):
    match, lk = _match_and_refine(prev, nxt)
    return match, lk.v, lk.eig


@pytest.mark.parametrize("shift", SUBPIXEL_SHIFTS)
def test_subpixel_translation_beats_the_parabola_fourfold(shift):
    err_lk, err_par = R.subpixel_errors(_reference_refine, shift)
    assert err_lk <= 0.25 * err_par
    assert err_lk <= 0.03


def test_four_iterations_have_converged():
    prev, nxt = R.field(7, 128, 128, R.CUT[32])[None], R.field(7, 128, 128, R.CUT[32], (2.3, -1.6))[None]
    match, four = _match_and_refine(prev, nxt, iterations=4)
    eight = A.lk_refine_reference(prev, nxt, match.disp, match.cost, 32, 16, 8)
    usable = R.usable_blocks(match)
    change = np.abs(four.v - eight.v)[usable].max()
    print(f"4 against 8 iterations: {change:.2e} px")
    assert change < 1e-3


def test_stripes_are_not_conditioned():
    prev, nxt = R.stripes(64, 96, 1.4)[None], R.stripes(64, 96)[None]
    match, lk = _match_and_refine(prev, nxt)
    wet = np.isfinite(match.cost[..., 0])
    assert wet.all()
    assert (lk.eig[..., 0] == 0).all() and (lk.eig[..., 1] > 0).all()
    assert not A.lk_conditioned(lk.eig).any()
    assert (lk.v == match.disp).all() and np.isfinite(lk.residual).all()
    assert (match.disp[..., 0] == 0).all()  # block matching's tie rule: no motion along the stripes


def test_striped_blocks_do_not_vote_in_the_motion_field():
    frames = torch.from_numpy(R.half_striped_frames())[:, None]
    field_lk = A.motion_field(frames, subpixel="lk")[0]
    field_par = A.motion_field(frames, subpixel="parabola")[0]
    R.check_aperture(field_lk.numpy(), field_par.numpy())


def test_forecast_error_at_lead_18_is_a_quarter_of_the_parabolas():
    R.check_e2e(R.e2e_errors())


def test_the_default_is_the_parabola_bit_for_bit_and_other_methods_are_refused():
    frames = torch.from_numpy(R.sequence(7, 128, 128, 3, (2.3, -1.6), R.CUT[32]))[:, None]
    assert torch.equal(A.motion_field(frames), A.motion_field(frames, subpixel="parabola"))
    assert not torch.equal(A.motion_field(frames), A.motion_field(frames, subpixel="lk"))
    with pytest.raises(ValueError):
        A.motion_field(frames, subpixel="farneback")
    with pytest.raises(ValueError):
        A.AdvectionNowcaster(subpixel="farneback")
    with pytest.raises(ValueError):
        EnsembleAdvectionNowcaster().refine_motion("lk", lk_iterations=0)
    with pytest.raises(TypeError):
        A.AdvectionNowcaster(18, 32, 16, 8, 0.1, None, 2, "lk")  # keyword-only
    assert A.AdvectionNowcaster().params["subpixel"] == "parabola" and EnsembleAdvectionNowcaster().params["subpixel"] == "parabola"
    assert EnsembleAdvectionNowcaster().refine_motion().params["subpixel"] == "lk"


def test_lk_refine_on_cpu_tensors_is_the_reference():
    prev, nxt = R.parity_case("84x100 32/16")
    match, ref = R.parity_reference("84x100 32/16", 4)
    tm = A.block_match(torch.from_numpy(prev.copy()), torch.from_numpy(nxt.copy()), 32, 16, 8)
    got = A.lk_refine(torch.from_numpy(prev.copy()), torch.from_numpy(nxt.copy()), tm, 32, 16)
    assert got.v.dtype == torch.float32 and got.eig.dtype == torch.float64 and got.residual.dtype == torch.float64
    assert (tm.disp.numpy() == match.disp).all()
    dry = ~np.isfinite(match.cost[..., 0])
    assert dry.any() and (ref.v[dry] == 0).all() and (ref.eig[dry] == 0).all() and np.isinf(ref.residual[dry]).all()
    # block_match rounds its costs to fp32, which only says which blocks are dry: the same blocks, the same values
    assert (got.v.numpy() == ref.v.astype(np.float32)).all() and (got.eig.numpy() == ref.eig).all()
    assert (got.residual.numpy() == ref.residual).all()
    with pytest.raises(ValueError):
        A.lk_refine(torch.from_numpy(prev.copy()), torch.from_numpy(nxt.copy()), tm, 32, 32)  # another lattice than the match's
    with pytest.raises(ValueError):
        A.lk_refine_reference(prev, nxt, match.disp, match.cost, 32, 16, iterations=17)
    with pytest.raises(ValueError):
        A.lk_refine_reference(prev, nxt, match.disp, match.cost, 32, 16, eig_ratio=-0.1)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_symbol_is_declared_exported_and_the_abi_version_stays(lib):
    from skillful_nowcasting_amd import _lib

    assert "dgmr_lk_refine" in _lib.SIGNATURES and len(_lib.SIGNATURES["dgmr_lk_refine"]) == 16
    assert hasattr(lib, "dgmr_lk_refine")
    assert lib.dgmr_abi_version() == 13 and _lib.ABI_VERSION == 13


def test_refusals_without_a_gpu(lib):
    buf = (ctypes.c_float * 16)()
    ibuf = (ctypes.c_int32 * 16)()
    dbuf = (ctypes.c_double * 16)()

    def lk(prev=buf, nxt=buf, n=1, h=64, w=64, block=32, stride=16, disp=ibuf, cost=buf, iterations=4, eig_ratio=0.01, v=buf, eig=dbuf,
           residual=dbuf):
        return lib.dgmr_lk_refine(prev, nxt, h * w, n, h, w, block, stride, disp, cost, iterations, eig_ratio, v, eig, residual, None)

    for kwargs, word in [(dict(prev=None), b"null pointer"), (dict(nxt=None), b"null pointer"), (dict(disp=None), b"null pointer"),
                         (dict(cost=None), b"null pointer"), (dict(v=None), b"null pointer"), (dict(eig=None), b"null pointer"),
                         (dict(residual=None), b"null pointer"), (dict(block=24), b"block=24"), (dict(stride=0), b"stride=0"),
                         (dict(stride=33), b"stride=33"), (dict(h=31), b"at least block"), (dict(w=16), b"at least block"),
                         (dict(iterations=0), b"iterations=0"), (dict(iterations=17), b"iterations=17"),
                         (dict(eig_ratio=-0.5), b"eig_ratio"), (dict(eig_ratio=float("nan")), b"eig_ratio"),
                         (dict(eig_ratio=float("inf")), b"eig_ratio"), (dict(n=0), b"N=0")]:
        assert lk(**kwargs) < 0, kwargs
        message = lib.dgmr_last_error()
        assert message.startswith(b"dgmr_lk_refine") and word in message, (kwargs, message)
