"""Exceedance tables and what is derived from them, on the host: the numpy specification (value.exceedance_table_reference) against
direct statements, ValueVerifier.compute on hand-made tables, its bookkeeping on CPU tensors, and the C entry point's argument checks
(no launch: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

from spectra_recipe import THRESHOLDS, make_ensemble

from skillful_nowcasting_amd import value as V
from skillful_nowcasting_amd.verification import ensemble_scores_reference


def test_reference_against_a_per_pixel_loop():
    f, o = make_ensemble(5, 2, 16, 16, "radar", seed=1, missing=False)
    o[0, 1, 2], o[0, 5, 5], o[1, 2, 3] = -1.0, np.nan, -np.inf
    o[1, 8:, :4] = -0.5
    table = V.exceedance_table_reference(f, o, THRESHOLDS)
    assert table.shape == (2, 3, 6, 2) and table.dtype == np.int64
    want = np.zeros_like(table)
    for n in range(2):
        for y in range(16):
            for x in range(16):
                if not o[n, y, x] >= 0:
                    continue
                for k, t in enumerate(THRESHOLDS):
                    j = sum(1 for m in range(5) if f[m, n, y, x] >= np.float32(t))
                    want[n, k, j, int(o[n, y, x] >= np.float32(t))] += 1
    assert np.array_equal(table, want)
    assert (table.sum(axis=(2, 3)) == (o >= 0).sum(axis=(1, 2))[:, None]).all()  # every present pixel once per threshold
    assert table[:, :, 1:].sum() > 0 and table[..., 1].sum() > 0


def test_one_member_table_is_the_contingency_table():
    f, o = make_ensemble(1, 3, 32, 48, "radar", seed=3)
    table = V.exceedance_table_reference(f, o, THRESHOLDS)
    cont = ensemble_scores_reference(f, o, (1,), THRESHOLDS).contingency  # [N, K, 1, (hits, misses, false alarms)]
    assert np.array_equal(table[:, :, 1, 1], cont[:, :, 0, 0]) and np.array_equal(table[:, :, 0, 1], cont[:, :, 0, 1])
    assert np.array_equal(table[:, :, 1, 0], cont[:, :, 0, 2])
    assert (table[-1] == 0).all()  # the all-missing plane
    assert V.exceedance_table_reference(f, o, ()).shape == (3, 0, 2, 2)


def test_values_at_a_threshold_reach_it_and_nan_members_do_not():
    f = np.full((2, 1, 16, 16), 4.0, np.float32)
    f[1, 0, :8] = np.nan
    o = np.full((1, 16, 16), 4.0, np.float32)
    t = V.exceedance_table_reference(f, o, (4.0, np.nextafter(np.float32(4.0), np.float32(5.0))))
    assert t[0, 0].tolist() == [[0, 0], [0, 128], [0, 128]] and t[0, 1].tolist() == [[256, 0], [0, 0], [0, 0]]


def _verifier_with_table(table, m):
    """table: [T, K, M + 1, 2]"""
    table = np.asarray(table, dtype=np.float64)
    v = V.ValueVerifier(m, table.shape[0], THRESHOLDS[:table.shape[1]])
    v._acc = torch.from_numpy(table.copy())
    return v


def test_value_anchors_perfect_always_never():
    """One member, s = 0.2.  A perfect forecast is worth 1 at every cost/loss ratio; "always act" is worth 0 where a < s (and less than
    that above); "never act" is worth 0 where a > s."""
    wet, dry = 200.0, 800.0
    perfect = [[[dry, 0.0], [0.0, wet]]]
    always = [[[0.0, 0.0], [dry, wet]]]
    never = [[[dry, wet], [0.0, 0.0]]]
    res = _verifier_with_table([perfect, always, never], 1).compute()
    alpha = res["cost_loss"]
    assert alpha.shape == (99,) and np.isclose(alpha[0], 0.01) and np.isclose(alpha[-1], 0.99)
    val = res["value"][THRESHOLDS[0]]
    assert val.shape == (3, 99)
    assert np.allclose(res["base_rate"][0], 0.2)
    assert np.allclose(val[0], 1.0, rtol=1e-13)
    assert np.allclose(val[1][alpha < 0.2], 0.0, atol=1e-13) and (val[1][alpha > 0.2 + 1e-9] < 0).all()
    assert np.allclose(val[2][alpha > 0.2], 0.0, atol=1e-13) and (val[2][alpha < 0.2 - 1e-9] < 0).all()
    assert res["hit_rate"][0, 0].tolist() == [1.0, 1.0, 0.0] and res["false_alarm_rate"][0, 0].tolist() == [0.0, 1.0, 0.0]
    assert res["brier"][0].tolist() == [0.0, 0.8, 0.2]


def test_two_member_toy():
    """M = 2, one threshold, one lead time; counts [j][o]: j = 0: (50, 10), j = 1: (20, 20), j = 2: (5, 45)."""
    tab = [[[[50.0, 10.0], [20.0, 20.0], [5.0, 45.0]]]]
    res = _verifier_with_table(tab, 2).compute(cost_loss=[0.1, 0.5, 0.9])
    n, wet, dry = 150.0, 75.0, 75.0
    assert np.isclose(res["base_rate"][0, 0], wet / n)
    brier = (10 * 1.0 + 20 * 0.25 + 20 * 0.25 + 5 * 1.0) / n  # (j / 2 - o)^2: (0 - 1)^2, (1/2)^2 twice, (1 - 0)^2; the rest is 0
    assert np.isclose(res["brier"][0, 0], brier, rtol=1e-15)
    assert np.allclose(res["hit_rate"][0, :, 0], [65 / wet, 45 / wet]) and np.allclose(res["false_alarm_rate"][0, :, 0], [25 / dry, 5 / dry])
    assert np.allclose(res["reliability"]["observed_frequency"][0, :, 0], [10 / 60, 0.5, 0.9])
    assert res["reliability"]["count"][0, :, 0].tolist() == [60.0, 40.0, 50.0] and res["forecast_probability"].tolist() == [0.0, 0.5, 1.0]
    s = 0.5
    want = []
    for a in (0.1, 0.5, 0.9):
        vj = [(min(a, s) - F * a * (1 - s) + H * s * (1 - a) - s) / (min(a, s) - s * a) for H, F in ((65 / wet, 25 / dry), (45 / wet, 5 / dry))]
        want.append(max(vj))
    assert np.allclose(res["value"][THRESHOLDS[0]][0], want, rtol=1e-14)
    # at a = s the value of a rule is its hit rate minus its false-alarm rate
    assert np.isclose(want[1], max(65 / wet - 25 / dry, 45 / wet - 5 / dry), rtol=1e-14)


def test_value_is_nan_without_events_or_without_non_events():
    only_dry = [[[100.0, 0.0], [10.0, 0.0]]]
    only_wet = [[[0.0, 100.0], [0.0, 10.0]]]
    res = _verifier_with_table([only_dry, only_wet], 1).compute()
    assert np.isnan(res["value"][THRESHOLDS[0]]).all()
    assert res["base_rate"][0].tolist() == [0.0, 1.0] and np.isfinite(res["brier"]).all()


def _verifier_inputs(b=3, t=2, c=2, m=4, seed=5):
    f, o = make_ensemble(m, b * t * c, 32, 32, "radar", seed=seed)
    o[-1] = o[0]
    return torch.from_numpy(f).view(m, b, t, c, 32, 32), torch.from_numpy(o).view(b, t, c, 32, 32)


def test_verifier_weights_and_cpu_tensors_go_through_the_reference():
    f, o = _verifier_inputs()
    w = np.array([2.0, 0.5, 4.0])
    v = V.ValueVerifier(4, 2, THRESHOLDS)
    v.update(f, o, weights=w)
    ref = V.exceedance_table_reference(f.reshape(4, 12, 32, 32).numpy(), o.reshape(12, 32, 32).numpy(), THRESHOLDS)
    want = (ref.reshape(3, 2, 2, 3, 5, 2) * w[:, None, None, None, None, None]).sum(axis=(0, 2))
    assert v._acc.dtype == torch.float64 and np.array_equal(v._acc.numpy(), want)  # (quarter-integer products: exact)
    got = V.exceedance_table(f, o, THRESHOLDS)
    assert got.dtype == torch.int64 and np.array_equal(got.numpy(), ref)
    one, batch = V.ValueVerifier(4, 2, THRESHOLDS), V.ValueVerifier(4, 2, THRESHOLDS)
    one.update(f[:, 1], o[1])
    batch.update(f[:, 1:2], o[1:2], weights=[1.0])
    assert torch.equal(one._acc, batch._acc)
    res = v.compute()
    assert res["hit_rate"].shape == (3, 4, 2) and res["reliability"]["count"].shape == (3, 5, 2) and res["brier"].shape == (3, 2)
    assert res["value"][THRESHOLDS[1]].shape == (2, 99)
    # more members required -> fewer hits and fewer false alarms
    assert (np.diff(res["hit_rate"], axis=1) <= 0).all() and (np.diff(res["false_alarm_rate"], axis=1) <= 0).all()


def test_verifier_merge_reset_and_empty_compute():
    f, o = _verifier_inputs(b=4)
    w = np.array([1.0, 3.0, 0.25, 2.0])
    whole, left, right = (V.ValueVerifier(4, 2, THRESHOLDS) for _ in range(3))
    whole.update(f[:, :2], o[:2], w[:2])
    whole.update(f[:, 2:], o[2:], w[2:])
    left.update(f[:, :2], o[:2], w[:2])
    right.update(f[:, 2:], o[2:], w[2:])
    left.merge(right)
    assert torch.equal(whole._acc, left._acc)
    left.reset()
    assert (left._acc == 0).all()
    with pytest.raises(ValueError):
        left.merge(V.ValueVerifier(4, 3, THRESHOLDS))
    with pytest.raises(ValueError):
        left.merge(V.ValueVerifier(4, 2, (1.0,)))
    empty = V.ValueVerifier(3, 2, THRESHOLDS).compute()  # nothing accumulated: NaN, not an exception
    assert np.isnan(empty["brier"]).all() and np.isnan(empty["value"][THRESHOLDS[0]]).all() and np.isnan(empty["hit_rate"]).all()
    assert empty["value"][THRESHOLDS[0]].shape == (2, 99)


@pytest.mark.parametrize("kwargs,shape", [
    (dict(), (33, 1, 16, 16)),
    (dict(), (2, 1, 24, 16)),
    (dict(), (2, 1, 16, 40)),
    (dict(thresholds=tuple(range(9))), (2, 1, 16, 16)),
])
def test_bad_arguments_raise_value_error(kwargs, shape):
    f = torch.zeros(shape)
    with pytest.raises(ValueError):
        V.exceedance_table(f, torch.zeros(shape[1:]), **kwargs)
    with pytest.raises(ValueError):
        V.exceedance_table_reference(f.numpy(), np.zeros(shape[1:], np.float32), **kwargs)
    with pytest.raises(ValueError):
        V.exceedance_table(torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(ValueError):
        V.ValueVerifier(33, 2)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """The refusals of dgmr_ensemble_scores that apply: nothing is enqueued (host buffers, never dereferenced)."""
    assert hasattr(lib, "dgmr_exceedance_table") and lib.dgmr_abi_version() == 13
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def go(m=2, n=1, h=16, w=16, k=3, stride=256, fc=base, obs=base, thr=base, table=base):
        return lib.dgmr_exceedance_table(fc, stride, obs, m, n, h, w, thr, k, table, None)

    for bad, text in [(dict(m=33), b"members"), (dict(m=0), b"members"), (dict(h=24), b"multiples of 16"), (dict(w=8), b"multiples of 16"),
                      (dict(k=9), b"thresholds"), (dict(k=-1), b"thresholds"), (dict(stride=258), b"member_stride"),
                      (dict(fc=base + 4), b"16-byte aligned"), (dict(obs=base + 8), b"16-byte aligned"), (dict(fc=None), b"null pointer"),
                      (dict(obs=None), b"null pointer"), (dict(thr=None), b"null pointer"), (dict(table=None), b"null pointer"),
                      (dict(table=base + 4), b"8-byte aligned"), (dict(n=0), b"planes")]:
        assert go(**bad) < 0, bad
        assert b"dgmr_exceedance_table" in lib.dgmr_last_error() and text in lib.dgmr_last_error(), (bad, lib.dgmr_last_error())
    assert go(k=0, thr=None, table=None) == 0  # an empty table: nothing to enqueue
