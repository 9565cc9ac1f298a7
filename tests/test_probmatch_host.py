"""Probability matching and the precipitation mask without a GPU: the fp32 specification (`probability_match_reference`) against
exact rank matching, its edge rules, the mask, the C ABI's refusals and the nowcaster's new arguments."""
import ctypes

import numpy as np
import pytest
import torch

import probmatch_recipe as PR
import stochastic_recipe as R


def _ref(z, target, mask=None, **kw):
    from skillful_nowcasting_amd.stochastic import probability_match_reference

    z = np.asarray(z, np.float32)
    target = np.asarray(target, np.float32)
    return probability_match_reference(z, np.sort(target.reshape(target.shape[0], -1), axis=1), mask, **kw)


def _tie_free(h, w, seed=0):
    """fp32 [h, w] inside the range, no two values equal"""
    rng = np.random.Generator(np.random.PCG64([seed, 61]))
    z = (rng.standard_normal(h * w) * 9.0).astype(np.float32)
    assert np.unique(z).size == z.size and np.abs(z).max() < 60
    return z.reshape(h, w)


def test_ranks_are_within_a_bin_of_the_exact_ranks():
    """target = 0, 1, ..., N - 1, so the output IS the rank: on a plane without ties every rank differs from argsort(argsort) by less
    than the occupancy of its element's bin, the ranks of a bin stay inside the bin's span, and bins of one element are exact."""
    from skillful_nowcasting_amd.stochastic import PM_BINS

    assert PM_BINS == PR.BINS
    h, w = 96, 80
    z = _tie_free(h, w)
    ranks = _ref(z[None, None, None], np.arange(h * w, dtype=np.float32).reshape(1, h, w))[0, 0, 0].astype(np.int64).ravel()
    exact = PR.exact_ranks(z)
    b = PR.bins_of(z).ravel()
    occ = PR.occupancy(z)
    gap = np.abs(ranks - exact)
    print(f"worst rank gap {gap.max()} with occupancies up to {occ.max()}")
    assert (gap < occ[b]).all()
    before = np.cumsum(occ) - occ
    assert (ranks >= before[b]).all() and (ranks < before[b] + occ[b]).all()
    assert (gap[occ[b] == 1] == 0).all() and (occ == 1).any()


def test_the_map_is_monotone_and_stays_within_the_target():
    z0, z = PR.member_case("128 L32")
    out = _ref(z, z0)
    assert out.dtype == np.float32 and out.shape == z.shape
    values = np.unique(z0)
    for plane_z, plane_o in zip(z.reshape(-1, z0.size), out.reshape(-1, z0.size)):
        order = np.argsort(plane_z, kind="stable")
        assert (np.diff(plane_o[order]) >= 0).all()
        assert np.isin(plane_o, values).all()
    # ties in z get one value
    tied = np.round(z[:, :1, :1] * 4) / 4
    got = _ref(tied, z0).ravel()
    for v in np.unique(tied)[::50]:
        assert np.unique(got[tied.ravel() == v]).size == 1


@pytest.mark.parametrize("name", sorted(PR.MEMBER_CASES))
def test_matching_restores_the_exceedance_counts(name):
    """At 5 / 15 / 21 / 25 dB the count of a matched plane differs from the target's by at most the largest occupancy of a bin other
    than bin 0 and the bin of exact zeros; the unmatched members are far off (what the matching is for)."""
    z0, z = PR.member_case(name)
    out = _ref(z, z0)
    want = PR.exceedances(z0)
    n = z0.size
    worst_bound = 0
    for plane_z, plane_o in zip(z.reshape(-1, n), out.reshape(-1, n)):
        bound = PR.exceedance_bound(plane_z)
        worst_bound = max(worst_bound, bound)
        assert (np.abs(PR.exceedances(plane_o) - want) <= bound).all(), (PR.exceedances(plane_o), want, bound)
    before = np.array([PR.exceedances(q) for q in z.reshape(-1, n)]).mean(axis=0)
    print(f"{name}: observed shares {(want / n).round(4).tolist()}, unmatched members {(before / n).round(4).tolist()}, largest "
          f"occupancy of a bin {worst_bound} of {n}")
    assert worst_bound < n // 100
    assert before[0] > 1.4 * want[0] and before[2] < 0.5 * want[2]  # the straw man: too much drizzle, too little heavy rain


def test_edge_rules():
    h, w = 16, 24
    n = h * w
    target = np.arange(n, dtype=np.float32).reshape(1, h, w) + 100.0
    z = _tie_free(h, w, seed=1).copy()
    z.ravel()[:6] = [np.nan, -np.inf, -64.5, np.inf, 64.0, 1.0e30]
    z.ravel()[6] = -64.0  # the first value inside the range: bin 0 too, f = 0
    out = _ref(z[None, None, None], target)[0, 0, 0].ravel()
    assert (out[:3] == 100.0).all() and out[6] == 100.0  # NaN and below the range: rank 0
    top = PR.occupancy(z)[PR.BINS - 1]
    assert top == 3 and (out[3:6] == 100.0 + n - top).all()  # above the range: the top bin's first rank (f = 0)
    # a constant plane: one bin, f the same for all - one rank
    const = np.full((1, 1, 1, h, w), 7.3, np.float32)
    got = np.unique(_ref(const, target))
    u = (np.float32(7.3) - PR.LO) * PR.SCALE
    assert got.size == 1 and got[0] == 100.0 + min(int((u - np.floor(u)) * np.float32(n)), n - 1)
    # an all-dry target gives zeros, whatever the input
    assert not _ref(z[None, None, None], np.zeros((1, h, w), np.float32)).any()
    # another origin and bin width
    coarse = _ref(z[None, None, None], target, lo=-32.0, scale=0.5)[0, 0, 0].ravel()
    assert (np.diff(coarse[np.argsort(z.ravel()[6:], kind="stable") + 6]) >= 0).all()
    for bad in (dict(scale=3.0), dict(scale=0.0), dict(scale=-2.0), dict(lo=np.nan), dict(scale=np.inf)):
        with pytest.raises(ValueError):
            _ref(z[None, None, None], target, **bad)
    with pytest.raises(ValueError):
        _ref(z[None, None, None], target, mask=np.ones((1, 2, h, w), np.uint8))
    with pytest.raises(ValueError):
        _ref(np.zeros((1, 1, 65, h, w), np.float32), target)


def test_masked_elements_are_dry_and_the_rest_shares_the_top_ranks():
    """A masked-out element counts in bin 0 and comes out 0.0; with the half-dry input no wet pixel lies outside the mask, and matching
    alone (what the mask is for) puts many there."""
    from skillful_nowcasting_amd.stochastic import precipitation_mask

    z0, z = PR.half_dry_case()
    pad = 5.0
    dry = np.broadcast_to((z0 < pad)[:, None, None], z.shape)
    unmasked = _ref(z, z0)
    leaked = int(((unmasked >= pad) & dry)[0, 0, 0].sum())
    print(f"wet pixels on the dry side without a mask: {leaked}")
    assert leaked > 500
    for radius in (0, 2, 8):
        mask = precipitation_mask(torch.from_numpy(np.array(z0)), pad, radius).numpy()
        assert mask.dtype == np.uint8 and mask.shape == (1, 1) + z0.shape[1:]
        out = _ref(z, z0, mask)
        allowed = np.broadcast_to((mask != 0)[:, None], z.shape)
        assert not (out[~allowed] != 0).any() and (np.signbit(out[~allowed]) == 0).all()
        assert not ((out >= pad) & ~allowed).any()
        # the plane's wet area is still the observation's (the mask allows at least the observed wet set): up to the bin bound
        for plane_z, plane_o, plane_a in zip(z.reshape(-1, z0.size), out.reshape(-1, z0.size), allowed.reshape(-1, z0.size)):
            bound = PR.exceedance_bound(np.where(plane_a, plane_z, np.float32(-1000)))
            assert (np.abs(PR.exceedances(plane_o) - PR.exceedances(z0)) <= bound).all()
    # a mask per lead time equals per-step calls with one plane
    masks = precipitation_mask(torch.from_numpy(np.array(z0)), pad, 1, growth=3.0, steps=2).numpy()
    assert masks.shape == (1, 2) + z0.shape[1:]
    both = _ref(z, z0, masks)
    for t in range(2):
        assert np.array_equal(PR.bits(both[:, :, t:t + 1]), PR.bits(_ref(z[:, :, t:t + 1], z0, masks[:, t:t + 1])))


def test_precipitation_mask_is_a_square_dilation():
    from skillful_nowcasting_amd.stochastic import precipitation_mask

    z0 = np.zeros((2, 20, 30), np.float32)
    z0[0, 5, 7], z0[0, 19, 0], z0[1, 10, 29], z0[1, 3, 3] = 9.0, 5.0, 6.0, 4.99
    for radius, growth, steps in ((0, 0.0, 1), (2, 0.0, 3), (1, 1.5, 3)):
        got = precipitation_mask(torch.from_numpy(z0), 5.0, radius, growth, steps).numpy()
        assert got.shape == (2, steps if growth else 1, 20, 30) and set(np.unique(got)) <= {0, 1}
        for t in range(got.shape[1]):
            k = radius + int(round(growth * (t + 1)))
            want = np.zeros((2, 20, 30), np.uint8)
            for p, y, x in ((0, 5, 7), (0, 19, 0), (1, 10, 29)):
                want[p, max(y - k, 0):y + k + 1, max(x - k, 0):x + k + 1] = 1
            assert np.array_equal(got[:, t], want), (radius, growth, t)
    for bad in (dict(radius=-1), dict(radius=1, growth=-0.5), dict(radius=1, steps=0), dict(radius=1, steps=65)):
        with pytest.raises(ValueError):
            precipitation_mask(torch.from_numpy(z0), 5.0, **bad)


def test_cpu_tensors_go_through_the_reference():
    from skillful_nowcasting_amd.stochastic import probability_match

    z0, z = PR.member_case("128 L32")
    zt, target = torch.from_numpy(np.array(z)), torch.from_numpy(np.array(z0))
    want = _ref(z, z0)
    got = probability_match(zt, target)
    assert np.array_equal(PR.bits(got.numpy()), PR.bits(want)) and torch.equal(zt, torch.from_numpy(np.array(z)))
    buf = torch.full((1, 4, 4, 128, 128), -7.0)
    view = buf[:, :, 1:3]
    view.copy_(zt)
    assert probability_match(view, target, out=view).data_ptr() == view.data_ptr()  # in place, through strides
    assert np.array_equal(PR.bits(view.numpy()), PR.bits(want)) and (buf[:, :, 0] == -7.0).all() and (buf[:, :, 3] == -7.0).all()
    for bad in (dict(scale=3.0), dict(out=torch.zeros(1, 4, 2, 128, 128).transpose(3, 4)), dict(mask=torch.ones(1, 3, 128, 128, dtype=torch.uint8)),
                dict(mask=torch.ones(1, 1, 128, 128))):
        with pytest.raises(ValueError):
            probability_match(zt, target, **bad)
    with pytest.raises(ValueError):
        probability_match(zt, target[:, :64])
    with pytest.raises(ValueError):
        probability_match(zt.double(), target)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_the_c_abi_refuses_bad_arguments_without_a_gpu(lib):
    """Every refusal happens before anything is enqueued, so none of these calls needs a device; the pointers are host buffers that a
    refused call never touches."""
    h, w, p, m, steps = 8, 12, 1, 2, 3
    n = h * w
    need = lib.dgmr_probability_match_workspace(p, m, steps)
    assert need == p * m * steps * 2 * 4096 * 4 + 16 and lib.dgmr_probability_match_workspace(5, 1, 1) == 5 * 2 * 4096 * 4 + 32
    assert lib.dgmr_probability_match_workspace(0, 1, 1) < 0 and lib.dgmr_probability_match_workspace(1, 0, 1) < 0
    assert lib.dgmr_probability_match_workspace(1, 1, 0) < 0 and lib.dgmr_probability_match_workspace(1, 1, 65) < 0
    z = (ctypes.c_float * (p * m * steps * n))()
    out = (ctypes.c_float * (p * m * steps * n))(*([-7.0] * (p * m * steps * n)))
    target = (ctypes.c_float * n)()
    mask = (ctypes.c_uint8 * (steps * n))()
    ws = (ctypes.c_uint8 * (need + 16))()
    ws_ptr = (ctypes.addressof(ws) + 15) & ~15
    base = dict(z=z, ms=steps * n, ss=n, target=target, ts=n, mask=None, mps=0, mss=0, P=p, M=m, T=steps, H=h, W=w, lo=-64.0, scale=32.0,
                ws=ws_ptr, wsb=need, out=out, oms=steps * n, oss=n)

    def raw(**kw):
        a = dict(base, **kw)
        return lib.dgmr_probability_match(a["z"], a["ms"], a["ss"], a["target"], a["ts"], a["mask"], a["mps"], a["mss"], a["P"], a["M"],
                                          a["T"], a["H"], a["W"], a["lo"], a["scale"], a["ws"], a["wsb"], a["out"], a["oms"], a["oss"], None)

    cases = [({"z": None}, b"null"), ({"target": None}, b"null"), ({"ws": None}, b"null"), ({"out": None}, b"null"),
             ({"scale": 3.0}, b"power of two"), ({"scale": 0.0}, b"power of two"), ({"scale": -32.0}, b"power of two"),
             ({"scale": float("nan")}, b"power of two"), ({"scale": float("inf")}, b"power of two"), ({"lo": float("nan")}, b"finite"),
             ({"H": 4097, "W": 4096}, b"2^24"), ({"H": 0}, b"2^24"),
             ({"ms": n - 1}, b"member_stride"), ({"ss": n - 1}, b"step_stride"), ({"oms": n - 1}, b"out_member_stride"),
             ({"oss": 0}, b"out_step_stride"), ({"ts": n - 1}, b"target_stride"),
             ({"mask": mask, "mps": n - 1, "mss": 0}, b"mask_plane_stride"), ({"mask": mask, "mps": steps * n, "mss": 1}, b"mask_step_stride"),
             ({"T": 0}, b"T=0"), ({"T": 65}, b"T=65"), ({"P": 0}, b"P=0"), ({"M": 0}, b"M=0"),
             ({"wsb": need - 1}, b"workspace"), ({"ws": ws_ptr + 4}, b"workspace")]
    for kw, word in cases:
        assert raw(**kw) < 0, kw
        msg = lib.dgmr_last_error()
        assert b"dgmr_probability_match" in msg and word in msg, (kw, msg)
    assert all(v == -7.0 for v in out)


def test_the_nowcaster_has_the_new_arguments():
    import inspect

    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster

    sig = inspect.signature(EnsembleAdvectionNowcaster.__init__).parameters
    assert sig["probability_matching"].default is False and sig["mask_radius"].default is None and sig["mask_growth"].default == 0.0
    assert list(sig)[-3:] == ["probability_matching", "mask_radius", "mask_growth"]  # appended: positional callers keep their meaning
    nc = EnsembleAdvectionNowcaster(forecast_steps=2, window=32)
    assert nc.probability_matching is False and nc.mask_radius is None and nc.mask_growth == 0.0
    with pytest.raises(ValueError, match="probability_matching"):
        EnsembleAdvectionNowcaster(forecast_steps=2, window=32, mask_radius=2)
    with pytest.raises(ValueError):
        EnsembleAdvectionNowcaster(forecast_steps=2, window=32, probability_matching=True, mask_radius=-1)
    with pytest.raises(ValueError):
        EnsembleAdvectionNowcaster(forecast_steps=2, window=32, probability_matching=True, mask_growth=1.0)
    nc = EnsembleAdvectionNowcaster(forecast_steps=2, window=32, probability_matching=True, mask_radius=4, mask_growth=0.5)
    assert nc.probability_matching and nc.mask_radius == 4 and nc.mask_growth == 0.5


def test_the_cpu_nowcast_with_matching_keeps_the_observed_wet_area():
    """The translating field on the CPU path, one white field, with and without matching: without it the first lead time rains over
    far more than the observed area, with it the wet-area ratio is close to the observation's - the inputs of the GPU test give the
    effect that it asserts.  The default arguments change no bit of the unmatched nowcast."""
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster

    seq = R.translating_db_context()
    frames = torch.from_numpy(seq[:4])[..., None]
    m, steps, window = 2, 2, 64
    white = torch.from_numpy(R.white_field((1, m, steps, 128, 128), seed=3))
    kw = dict(forecast_steps=steps, window=window)
    plain = EnsembleAdvectionNowcaster(**kw).nowcast(frames, m, white=white)
    again = EnsembleAdvectionNowcaster(**kw, probability_matching=False, mask_radius=None, mask_growth=0.0).nowcast(frames, m, white=white)
    assert torch.equal(PR.bits(plain), PR.bits(again))
    matched = EnsembleAdvectionNowcaster(**kw, probability_matching=True).nowcast(frames, m, white=white)
    masked = EnsembleAdvectionNowcaster(**kw, probability_matching=True, mask_radius=2).nowcast(frames, m, white=white)
    observed = PR.wet_area(seq[4], 0.1)
    gaps = {k: abs(PR.wet_area(v[:, 0], 0.1) - observed) for k, v in (("plain", plain), ("matched", matched), ("masked", masked))}
    print(f"wet-area ratio at the first lead time: observed {observed:.4f}, |member - observed| {gaps}")
    assert gaps["matched"] < 0.5 * gaps["plain"] and gaps["masked"] < 0.5 * gaps["plain"]
    assert tuple(matched.shape) == (m, steps, 1, 128, 128) and torch.isfinite(matched).all() and (matched >= 0).all()
