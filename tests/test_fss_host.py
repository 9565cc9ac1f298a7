"""Fractions skill score on the host: the numpy specification (fss.fss_sums_reference) against a brute-force loop and closed forms,
FractionsVerifier.compute on hand-made accumulators, its bookkeeping on CPU tensors, and the C entry point's argument checks (no
launch: there is no GPU here)."""
import ctypes
from fractions import Fraction

import numpy as np
import pytest
import torch

from fss_recipe import brute_force
from spectra_recipe import THRESHOLDS, make_ensemble

from skillful_nowcasting_amd import fss as F


def test_reference_against_a_brute_force_loop():
    f, o = make_ensemble(3, 2, 16, 32, "radar", seed=2, missing=False)
    o[0, 1, 2], o[0, 5, 5], o[1, 2, 30] = -1.0, np.nan, -np.inf
    o[1, 8:, :4] = -0.5
    f[1, 0, 3, 3] = np.nan
    radii = (0, 1, 5, 32)
    sums, events = F.fss_sums_reference(f, o, THRESHOLDS, radii)
    assert sums.shape == (2, 3, 4, 4) and events.shape == (2, 3, 2) and sums.dtype == np.int64 and events.dtype == np.int64
    want_sums, want_events = brute_force(f, o, THRESHOLDS, radii)
    assert np.array_equal(sums, want_sums) and np.array_equal(events, want_events)
    assert (sums[:, 0] > 0).all() and (events[:, 0] > 0).all()
    # at radius 0 the box sum is the indicator: oo is the observed event count, mm the members'
    assert np.array_equal(sums[:, :, 0, 1], events[:, :, 1]) and np.array_equal(sums[:, :, 0, 3], events[:, :, 0])
    # the radii may come in any order
    swapped, _ = F.fss_sums_reference(f, o, THRESHOLDS, (32, 0, 5, 1))
    assert np.array_equal(swapped, sums[:, :, [3, 0, 2, 1]])


def _fss(sums, m):
    """[..., 4] integers -> exact Fractions 2 (fo / M) / (ff / M^2 + oo)"""
    ff, oo, fo, _ = (int(v) for v in sums)
    return Fraction(2 * fo, m) / (Fraction(ff, m * m) + oo)


def test_a_displaced_pixel_has_the_closed_form():
    """One wet pixel, displaced by d = 7 columns, far from the border: FSS = max(0, 1 - d / (2r + 1))."""
    f = np.zeros((1, 1, 96, 96), np.float32)
    o = np.zeros((1, 96, 96), np.float32)
    f[0, 0, 40, 40], o[0, 40, 47] = 5.0, 5.0
    radii = (0, 1, 3, 4, 8)
    sums, events = F.fss_sums_reference(f, o, (4.0,), radii)
    assert events.tolist() == [[[1, 1]]]
    got = [_fss(sums[0, 0, s], 1) for s in range(len(radii))]
    assert got == [0, 0, 0, Fraction(2, 9), Fraction(10, 17)]
    v = F.FractionsVerifier(1, 1, (4.0,), radii)
    v.update(torch.from_numpy(f).view(1, 1, 1, 96, 96), torch.from_numpy(o).view(1, 1, 96, 96))
    res = v.compute()
    assert np.allclose(res["fss"][0, :, 0], [0.0, 0.0, 0.0, 2 / 9, 10 / 17], rtol=1e-15, atol=0)
    assert np.array_equal(res["fss"], res["fss_members"])  # one member: the classical deterministic score


def test_identical_forecast_and_observation_score_exactly_one():
    _, o = make_ensemble(1, 2, 32, 48, "radar", seed=4)
    f = np.repeat(o[None], 3, axis=0)
    v = F.FractionsVerifier(3, 2, THRESHOLDS, (0, 2, 8, 32))
    v.update(torch.from_numpy(f).view(3, 2, 1, 32, 48), torch.from_numpy(o).view(2, 1, 32, 48))
    res = v.compute()
    assert (res["fss"][:, :, 0] == 1.0).all() and (res["fss_members"][:, :, 0] == 1.0).all()
    assert np.isnan(res["fss"][:, :, 1]).all()  # lead time 1 is the wholly missing plane: no event anywhere, 0 / 0
    assert (res["frequency_bias"][:, 0] == 1.0).all() and (res["skilful_side"][:, 0] == 1.0).all()


def test_a_window_that_contains_the_plane():
    f, o = make_ensemble(4, 1, 16, 16, "radar", seed=6)
    sums, events = F.fss_sums_reference(f, o, THRESHOLDS, (32,))
    ef, eo = events[0, :, 0], events[0, :, 1]
    assert (ef > 0).all()
    assert np.array_equal(sums[0, :, 0, 0], 256 * ef ** 2) and np.array_equal(sums[0, :, 0, 1], 256 * eo ** 2)
    assert np.array_equal(sums[0, :, 0, 2], 256 * ef * eo)


def _verifier_with(sums, events, pixels, m, radii):
    """sums [T, K, S, 4], events [T, K, 2], pixels [T]"""
    sums = np.asarray(sums, dtype=np.float64)
    v = F.FractionsVerifier(m, sums.shape[0], THRESHOLDS[:sums.shape[1]], radii)
    v._sums, v._events, v._pixels = (torch.from_numpy(np.asarray(a, dtype=np.float64).copy()) for a in (sums, events, pixels))
    return v


def test_compute_from_hand_made_accumulators():
    """M = 2, one threshold, radii (8, 0, 2), three lead times: a scored one, one without forecast events, one without anything."""
    m = 2
    lead0 = [[40.0, 30.0, 28.0, 26.0], [8.0, 6.0, 2.0, 4.0], [16.0, 9.0, 10.0, 9.0]]   # (ff, oo, fo, mm) per radius
    lead1 = [[0.0, 30.0, 0.0, 0.0], [0.0, 6.0, 0.0, 0.0], [0.0, 9.0, 0.0, 0.0]]
    lead2 = [[0.0] * 4] * 3
    sums = [[lead0], [lead1], [lead2]]
    events = [[[8.0, 6.0]], [[0.0, 6.0]], [[0.0, 0.0]]]
    res = _verifier_with(sums, events, [100.0, 100.0, 0.0], m, (8, 0, 2)).compute()
    assert res["sides"].tolist() == [17, 1, 5] and res["fss"].shape == (1, 3, 3) and res["base_rate"].shape == (1, 3)
    want = [2 * (fo / m) / (ff / m ** 2 + oo) for ff, oo, fo, _ in lead0]
    want_members = [2 * (fo / m) / (mm / m + oo) for _, oo, fo, mm in lead0]
    assert np.allclose(res["fss"][0, :, 0], want, rtol=1e-15) and np.allclose(res["fss_members"][0, :, 0], want_members, rtol=1e-15)
    assert res["fss"][0, :, 1].tolist() == [0.0, 0.0, 0.0]           # observed events, no forecast events: a score of 0
    assert np.isnan(res["fss"][0, :, 2]).all() and np.isnan(res["fss_members"][0, :, 2]).all()  # 0 / 0
    assert res["base_rate"][0, :2].tolist() == [0.06, 0.06] and np.isnan(res["base_rate"][0, 2])
    assert res["forecast_rate"][0, :2].tolist() == [0.04, 0.0] and np.isnan(res["forecast_rate"][0, 2])
    assert np.isclose(res["frequency_bias"][0, 0], 0.04 / 0.06) and res["frequency_bias"][0, 1] == 0.0 and np.isnan(res["frequency_bias"][0, 2])
    assert np.array_equal(res["fss_random"], res["base_rate"], equal_nan=True)
    assert np.allclose(res["fss_useful"][0, :2], 0.53, rtol=1e-15) and np.isnan(res["fss_useful"][0, 2])
    # lead 0: fss = 0.7, 0.25, 0.769... at sides 17, 1, 5 against a useful level of 0.53: the smallest skilful side is 5
    assert res["skilful_side"][0, 0] == 5.0 and np.isnan(res["skilful_side"][0, 1]) and np.isnan(res["skilful_side"][0, 2])
    assert res["thresholds"].tolist() == [THRESHOLDS[0]]
    empty = F.FractionsVerifier(3, 2).compute()  # nothing accumulated: NaN, not an exception
    assert empty["fss"].shape == (3, 4, 2) and np.isnan(empty["fss"]).all() and np.isnan(empty["skilful_side"]).all()
    assert empty["sides"].tolist() == [1, 5, 17, 65]


def _verifier_inputs(b=3, t=2, c=2, m=4, seed=5):
    f, o = make_ensemble(m, b * t * c, 32, 32, "radar", seed=seed)
    o[-1] = o[0]
    return torch.from_numpy(f).view(m, b, t, c, 32, 32), torch.from_numpy(o).view(b, t, c, 32, 32)


def test_verifier_weights_and_cpu_tensors_go_through_the_reference():
    f, o = _verifier_inputs()
    w = np.array([2.0, 0.5, 4.0])
    radii = (0, 2, 8)
    v = F.FractionsVerifier(4, 2, THRESHOLDS, radii)
    v.update(f, o, weights=w)
    sums, events = F.fss_sums_reference(f.reshape(4, 12, 32, 32).numpy(), o.reshape(12, 32, 32).numpy(), THRESHOLDS, radii)
    want = (sums.reshape(3, 2, 2, 3, 3, 4) * w[:, None, None, None, None, None]).sum(axis=(0, 2))
    want_events = (events.reshape(3, 2, 2, 3, 2) * w[:, None, None, None, None]).sum(axis=(0, 2))
    assert v._sums.dtype == torch.float64 and np.array_equal(v._sums.numpy(), want)  # (half-integer products: exact)
    assert np.array_equal(v._events.numpy(), want_events) and v._pixels.tolist() == [6.5 * 2 * 1024] * 2
    got_sums, got_events = F.fss_sums(f, o, THRESHOLDS, radii)
    assert got_sums.dtype == torch.int64 and np.array_equal(got_sums.numpy(), sums) and np.array_equal(got_events.numpy(), events)
    one, batch = F.FractionsVerifier(4, 2, THRESHOLDS, radii), F.FractionsVerifier(4, 2, THRESHOLDS, radii)
    one.update(f[:, 1], o[1])
    batch.update(f[:, 1:2], o[1:2], weights=[1.0])
    assert torch.equal(one._sums, batch._sums) and torch.equal(one._events, batch._events) and torch.equal(one._pixels, batch._pixels)
    res = v.compute()
    assert res["fss"].shape == (3, 3, 2) and res["fss_members"].shape == (3, 3, 2) and res["skilful_side"].shape == (3, 2)
    ok = np.isfinite(res["fss"])
    assert ok.any() and (res["fss"][ok] >= 0).all() and (res["fss"][ok] <= 1).all()
    # the members' pooled score never exceeds the ensemble probability's: ff / M^2 <= mm / M (Cauchy-Schwarz)
    assert (res["fss_members"][ok] <= res["fss"][ok]).all()


def test_verifier_merge_reset_and_skill_score():
    f, o = _verifier_inputs(b=4)
    w = np.array([1.0, 3.0, 0.25, 2.0])
    whole, left, right = (F.FractionsVerifier(4, 2, THRESHOLDS, (0, 8)) for _ in range(3))
    whole.update(f[:, :2], o[:2], w[:2])
    whole.update(f[:, 2:], o[2:], w[2:])
    left.update(f[:, :2], o[:2], w[:2])
    right.update(f[:, 2:], o[2:], w[2:])
    left.merge(right)
    for a, b in ((whole._sums, left._sums), (whole._events, left._events), (whole._pixels, left._pixels)):
        assert torch.equal(a, b)
    fresh = F.FractionsVerifier(4, 2, THRESHOLDS, (0, 8))
    fresh.merge(F.FractionsVerifier(4, 2, THRESHOLDS, (0, 8)))  # nothing on either side
    assert fresh._sums is None
    fresh.merge(whole)
    assert torch.equal(fresh._sums, whole._sums) and torch.equal(fresh._pixels, whole._pixels)
    res, base = whole.compute(), right.compute()
    skill = F.skill_score_fss(res, base)
    assert np.array_equal(skill["fss"], res["fss"] - base["fss"], equal_nan=True) and skill["sides"].tolist() == [1, 17]
    assert np.array_equal(skill["fss_members"], res["fss_members"] - base["fss_members"], equal_nan=True)
    with pytest.raises(ValueError):
        F.skill_score_fss(res, F.FractionsVerifier(4, 2, THRESHOLDS, (0, 2)).compute())
    with pytest.raises(ValueError):
        F.skill_score_fss(res, F.FractionsVerifier(4, 2, (1.0, 4.0, 16.0), (0, 8)).compute())
    with pytest.raises(ValueError):
        F.skill_score_fss(res, F.FractionsVerifier(4, 3, THRESHOLDS, (0, 8)).compute())
    left.reset()
    assert (left._sums == 0).all() and (left._events == 0).all() and (left._pixels == 0).all()
    for other in (F.FractionsVerifier(4, 3, THRESHOLDS, (0, 8)), F.FractionsVerifier(4, 2, (1.0,), (0, 8)),
                  F.FractionsVerifier(4, 2, THRESHOLDS, (8, 0)), F.FractionsVerifier(3, 2, THRESHOLDS, (0, 8))):
        with pytest.raises(ValueError):
            left.merge(other)


@pytest.mark.parametrize("kwargs,shape", [
    (dict(), (33, 1, 16, 16)),
    (dict(), (2, 1, 24, 16)),
    (dict(), (2, 1, 16, 40)),
    (dict(thresholds=tuple(range(9))), (2, 1, 16, 16)),
    (dict(thresholds=()), (2, 1, 16, 16)),
    (dict(radii=()), (2, 1, 16, 16)),
    (dict(radii=tuple(range(9))), (2, 1, 16, 16)),
    (dict(radii=(0, 33)), (2, 1, 16, 16)),
    (dict(radii=(-1,)), (2, 1, 16, 16)),
    (dict(radii=(2, 8, 2)), (2, 1, 16, 16)),
    (dict(radii=(1.5,)), (2, 1, 16, 16)),
])
def test_bad_arguments_raise_value_error(kwargs, shape):
    f = torch.zeros(shape)
    with pytest.raises(ValueError):
        F.fss_sums(f, torch.zeros(shape[1:]), **kwargs)
    with pytest.raises(ValueError):
        F.fss_sums_reference(f.numpy(), np.zeros(shape[1:], np.float32), **kwargs)


def test_more_bad_arguments():
    with pytest.raises(ValueError):
        F.fss_sums(torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(ValueError):
        F.fss_sums(torch.zeros(2, 1, 16, 16, dtype=torch.float64), torch.zeros(1, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        F.FractionsVerifier(33, 2)
    with pytest.raises(ValueError):
        F.FractionsVerifier(2, 0)
    with pytest.raises(ValueError):
        F.FractionsVerifier(2, 2, radii=(0, 0))
    with pytest.raises(ValueError, match="2\\^63"):  # the conservative bound M^2 (2R + 1)^4 H W, before anything is touched
        F.fss_sums(torch.zeros(1).expand(32, 1, 32768, 32768), torch.zeros(1).expand(1, 32768, 32768), (1.0,), (32,))
    v = F.FractionsVerifier(2, 2)
    with pytest.raises(ValueError):
        v.update(torch.zeros(3, 2, 1, 16, 16), torch.zeros(2, 1, 16, 16))
    with pytest.raises(ValueError):
        v.update(torch.zeros(2, 2, 2, 1, 16, 16), torch.zeros(2, 2, 1, 16, 16), weights=[1.0, 2.0, 3.0])


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_the_symbol_is_new_and_the_abi_version_is_not(lib):
    from skillful_nowcasting_amd import _lib

    assert hasattr(lib, "dgmr_fss_sums") and lib.dgmr_abi_version() == 13 == _lib.ABI_VERSION
    assert "dgmr_fss_sums" in _lib.SIGNATURES


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """Every refusal of dgmr_fss_sums: nothing is enqueued (host buffers, never dereferenced)."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def go(m=2, n=1, h=16, w=16, k=3, stride=256, fc=base, obs=base, thr=base, radii=(0, 2, 8, 32), s=None, sums=base, events=base):
        rad = None if radii is None else (ctypes.c_int * max(len(radii), 1))(*radii)
        return lib.dgmr_fss_sums(fc, stride, obs, m, n, h, w, thr, k, rad, len(radii) if s is None else s, sums, events, None)

    for bad, text in [(dict(m=33), b"members"), (dict(m=0), b"members"), (dict(h=24), b"multiples of 16"), (dict(w=8), b"multiples of 16"),
                      (dict(h=0), b"multiples of 16"), (dict(k=9), b"thresholds"), (dict(k=0), b"thresholds"), (dict(k=-1), b"thresholds"),
                      (dict(radii=(), s=0), b"radii"), (dict(radii=tuple(range(9))), b"radii"), (dict(s=-1), b"radii"),
                      (dict(radii=(0, 33)), b"radius 33"), (dict(radii=(-1, 2)), b"radius -1"), (dict(radii=(2, 8, 2)), b"given twice"),
                      (dict(stride=258), b"member_stride"), (dict(stride=-4), b"member_stride"),
                      (dict(fc=base + 4), b"16-byte aligned"), (dict(obs=base + 8), b"16-byte aligned"),
                      (dict(sums=base + 4), b"8-byte aligned"), (dict(events=base + 4), b"8-byte aligned"),
                      (dict(fc=None), b"null pointer"), (dict(obs=None), b"null pointer"), (dict(thr=None), b"null pointer"),
                      (dict(radii=None, s=2), b"null pointer"), (dict(sums=None), b"null pointer"), (dict(events=None), b"null pointer"),
                      (dict(n=0), b"planes"), (dict(m=32, h=32768, w=32768, radii=(0, 32)), b"2^63"),
                      (dict(h=65536, w=65536), b"out of range")]:
        assert go(**bad) < 0, bad
        assert b"dgmr_fss_sums" in lib.dgmr_last_error() and text in lib.dgmr_last_error(), (bad, lib.dgmr_last_error())
