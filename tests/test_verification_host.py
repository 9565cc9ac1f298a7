"""Ensemble verification on the host: the numpy specification (verification.ensemble_scores_reference) against independent
statements of the same quantities, NowcastVerifier's bookkeeping on CPU tensors, and the C entry point's argument checks (no launch:
there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

from verification_recipe import SCALES, THRESHOLDS, make_case

from skillful_nowcasting_amd import verification as V


def test_hand_computed_two_members():
    """M = 2 on one 16 x 16 plane: member 0 is 0 everywhere, member 1 is 3 everywhere, the observation 1 everywhere except y = 3 at
    (0, 0) and one missing pixel at (5, 9).  Every present cell, at every scale and pooling, has (|x_0 - y| + |x_1 - y|) / 2 = 1.5
    (y lies between the members) and |x_0 - x_1| = 3."""
    f = np.zeros((2, 1, 16, 16), np.float32)
    f[1] = 3.0
    o = np.ones((1, 16, 16), np.float32)
    o[0, 0, 0] = 3.0
    o[0, 5, 9] = np.nan
    r = V.ensemble_scores_reference(f, o, (1, 4, 16), (1.0, 2.0, 3.0))
    assert r.cells.tolist() == [[255, 15, 0]]
    assert r.abs_err.tolist() == [[[382.5, 22.5, 0.0]] * 2]
    assert r.pair.tolist() == [[[765.0, 45.0, 0.0]] * 2]
    # thresholds 1, 2, 3: (hits, misses, false alarms) of member 0 (always below) and member 1 (3 everywhere: at the threshold 3 too)
    assert r.contingency[0].tolist() == [[[0, 255, 0], [255, 0, 0]], [[0, 1, 0], [1, 0, 254]], [[0, 1, 0], [1, 0, 254]]]
    want = np.zeros((3, 3), np.int64)
    want[1, 0], want[1, 1] = 254, 1  # member 0 below; at (0, 0) member 1 ties
    assert np.array_equal(r.ranks[0], want)


def test_one_member_is_the_absolute_error():
    f, o = make_case(1, 3, 32, 64, "radar")
    r = V.ensemble_scores_reference(f, o, (1,), ())
    present = o >= 0
    want = np.where(present, np.abs(f[0].astype(np.float64) - o.astype(np.float64)), 0.0).reshape(3, -1).sum(axis=1)
    assert np.allclose(r.abs_err[:, 0, 0], want, rtol=1e-13, atol=0)
    assert (r.pair == 0).all() and r.contingency.shape == (3, 0, 1, 3)


def test_identical_members_have_no_spread():
    f, o = make_case(1, 2, 32, 32, "continuous")
    r = V.ensemble_scores_reference(np.repeat(f, 5, axis=0), o, (1, 2, 4, 8, 16), THRESHOLDS)
    assert (r.pair == 0).all() and (r.abs_err[0] > 0).all()


def test_member_permutation():
    f, o = make_case(6, 3, 32, 64, "radar")
    a = V.ensemble_scores_reference(f, o, SCALES, THRESHOLDS)
    perm = [4, 0, 5, 2, 1, 3]
    b = V.ensemble_scores_reference(f[perm], o, SCALES, THRESHOLDS)
    assert np.array_equal(a.cells, b.cells) and np.array_equal(a.ranks, b.ranks)
    assert np.array_equal(a.contingency[:, :, perm], b.contingency)
    assert np.allclose(a.abs_err, b.abs_err, rtol=1e-13, atol=0) and np.allclose(a.pair, b.pair, rtol=1e-13, atol=0)


def test_counts_against_direct_statements():
    f, o = make_case(6, 5, 96, 160, "radar")
    scales = (1, 2, 4, 8, 16)
    r = V.ensemble_scores_reference(f, o, scales, THRESHOLDS)
    present = o >= 0
    for si, s in enumerate(scales):
        direct = present.reshape(5, 96 // s, s, 160 // s, s).all(axis=(2, 4)).sum(axis=(1, 2))
        assert np.array_equal(r.cells[:, si], direct), s
    assert (r.cells[-1] == 0).all() and (r.abs_err[-1] == 0).all() and (r.pair[-1] == 0).all()  # the all-missing plane
    assert 0 < r.cells[0, -1] < 60  # one of plane 0's 60 cells of 16 x 16 is missing as a whole, scattered pixels take more
    assert np.array_equal(r.ranks.sum(axis=(1, 2)), r.cells[:, 0])
    for k, t in enumerate(THRESHOLDS):
        wet = (present & (o >= np.float32(t))).sum(axis=(1, 2))
        for m in range(6):
            assert np.array_equal(r.contingency[:, k, m, 0] + r.contingency[:, k, m, 1], wet)
    b, e = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
    assert (r.ranks[:, b + e > 6] == 0).all()
    assert np.array_equal(r.abs_err[:, 0, 0], r.abs_err[:, 1, 0]) and np.array_equal(r.pair[:, 0, 0], r.pair[:, 1, 0])


def test_values_at_a_threshold_reach_it():
    f = np.full((1, 1, 16, 16), 4.0, np.float32)
    o = np.full((1, 16, 16), 4.0, np.float32)
    r = V.ensemble_scores_reference(f, o, (1,), (4.0, np.nextafter(np.float32(4.0), np.float32(5.0))))
    assert r.contingency[0, 0, 0].tolist() == [256, 0, 0] and r.contingency[0, 1, 0].tolist() == [0, 0, 0]
    assert r.ranks[0, 0, 1] == 256


def test_nan_member_is_neither_hit_nor_miss():
    f = np.full((2, 1, 16, 16), 5.0, np.float32)
    f[1, 0, :8] = np.nan
    o = np.full((1, 16, 16), 5.0, np.float32)
    o[0, :, 8:] = 0.0
    r = V.ensemble_scores_reference(f, o, (1,), (1.0,))
    assert r.contingency[0, 0, 0].tolist() == [128, 0, 128]  # member 0: 5 everywhere
    assert r.contingency[0, 0, 1].tolist() == [64, 0, 64]    # member 1: NaN over half of the wet and half of the dry pixels
    assert r.ranks[0].sum() == 256 and r.ranks[0, 0, 2] == 64 and r.ranks[0, 0, 1] == 64  # NaN: not below, not tied
    assert np.isnan(r.abs_err).all() and np.isnan(r.pair).all()


def test_max_pooling_of_a_constant_field():
    """Members c_m, observation c_y, constant: every pooled value is the constant, so every cell has sum_m |c_m - c_y| / M, at every scale
    and under both poolings."""
    c = np.array([0.5, 2.0, 7.25], np.float32)
    f = np.broadcast_to(c[:, None, None, None], (3, 2, 32, 48)).copy()
    o = np.full((2, 32, 48), 3.0, np.float32)
    scales = (1, 2, 4, 8, 16)
    r = V.ensemble_scores_reference(f, o, scales, ())
    per_cell_abs = (2.5 + 1.0 + 4.25) / 3
    per_cell_pair = 1.5 + 6.75 + 5.25
    for si, s in enumerate(scales):
        n_cells = (32 // s) * (48 // s)
        assert r.cells[:, si].tolist() == [n_cells] * 2
        assert np.allclose(r.abs_err[:, :, si], per_cell_abs * n_cells, rtol=1e-14, atol=0)
        assert np.allclose(r.pair[:, :, si], per_cell_pair * n_cells, rtol=1e-14, atol=0)


def test_average_pooling_against_a_plain_mean():
    f, o = make_case(2, 1, 32, 32, "continuous", missing=False)
    r = V.ensemble_scores_reference(f, o, (4,), ())
    x = f.astype(np.float64).reshape(2, 8, 4, 8, 4).mean(axis=(2, 4))
    y = o.astype(np.float64).reshape(8, 4, 8, 4).mean(axis=(1, 3))
    assert np.isclose(r.abs_err[0, 0, 0], (np.abs(x - y).sum(axis=0) / 2).sum(), rtol=1e-13)
    assert np.isclose(r.pair[0, 0, 0], np.abs(x[0] - x[1]).sum(), rtol=1e-13)
    xm, ym = f.reshape(2, 8, 4, 8, 4).max(axis=(2, 4)).astype(np.float64), o.reshape(8, 4, 8, 4).max(axis=(1, 3)).astype(np.float64)
    assert np.isclose(r.abs_err[0, 1, 0], (np.abs(xm - ym).sum(axis=0) / 2).sum(), rtol=1e-13)


def test_rank_histogram_is_flat_for_a_calibrated_ensemble():
    """Observation and M = 7 members drawn from one continuous distribution, 5 planes of 96 x 160: every rank is equally likely, so
    every bin is within 5 standard errors sqrt(p (1 - p) / n) of p = 1 / 8, n the pixel count."""
    f, o = make_case(7, 5, 96, 160, "continuous", seed=3, missing=False)
    v = V.NowcastVerifier(7, 1, (1,), ())
    v.update(torch.from_numpy(f).view(7, 1, 5, 96, 160), torch.from_numpy(o).view(1, 5, 96, 160))
    hist = v.compute()["rank_histogram"]
    assert hist.shape == (1, 8) and abs(hist.sum() - 1.0) < 1e-12
    n, p = 5 * 96 * 160, 1.0 / 8
    se = np.sqrt(p * (1 - p) / n)
    print("bins", hist[0], "standard error", se)
    assert (np.abs(hist[0] - p) <= 5 * se).all()


def test_rank_histogram_spreads_ties():
    ranks = np.zeros((1, 3, 3))
    ranks[0, 0, 2], ranks[0, 1, 0], ranks[0, 1, 1] = 6, 2, 4  # all tied; one below; one below and one tied
    hist = V._rank_histogram(ranks)
    assert np.allclose(hist[0] * 12, [2, 2 + 2 + 2, 2 + 2])


def _verifier_inputs(b=3, t=2, c=2, m=4, seed=5):
    f, o = make_case(m, b * t * c, 32, 32, "radar", seed=seed)
    o[-1] = o[0]  # (no all-missing plane here)
    return torch.from_numpy(f).view(m, b, t, c, 32, 32), torch.from_numpy(o).view(b, t, c, 32, 32)


def test_verifier_weights_scale_contributions():
    f, o = _verifier_inputs()
    w = np.array([2.0, 0.5, 4.0])
    a = V.NowcastVerifier(4, 2, SCALES, THRESHOLDS)
    a.update(f, o, weights=w)
    want = None
    for case in range(3):
        one = V.NowcastVerifier(4, 2, SCALES, THRESHOLDS)
        one.update(f[:, case], o[case])
        part = [x * w[case] for x in one._acc]
        want = part if want is None else [u + v for u, v in zip(want, part)]
    for got, ref in zip(a._acc, want):
        assert torch.allclose(got, ref, rtol=1e-14, atol=0)
    # sums over cases and channels per lead time, straight from the reference
    ref = V.ensemble_scores_reference(f.reshape(4, 12, 32, 32).numpy(), o.reshape(12, 32, 32).numpy(), SCALES, THRESHOLDS)
    cells = (ref.cells.reshape(3, 2, 2, -1) * w[:, None, None, None]).sum(axis=(0, 2))
    assert np.allclose(a._acc.cells.numpy(), cells, rtol=1e-14, atol=0)


def test_verifier_merge_equals_one_verifier():
    f, o = _verifier_inputs(b=4)
    w = np.array([1.0, 3.0, 0.25, 2.0])
    whole, left, right = (V.NowcastVerifier(4, 2, SCALES, THRESHOLDS) for _ in range(3))
    whole.update(f[:, :2], o[:2], w[:2])
    whole.update(f[:, 2:], o[2:], w[2:])
    left.update(f[:, :2], o[:2], w[:2])
    right.update(f[:, 2:], o[2:], w[2:])
    left.merge(right)
    for u, v in zip(whole._acc, left._acc):
        assert torch.equal(u, v)
    a, b = whole.compute(), left.compute()
    assert np.array_equal(a["crps"]["avg"][4], b["crps"]["avg"][4]) and np.array_equal(a["rank_histogram"], b["rank_histogram"])
    left.reset()
    assert all((x == 0).all() for x in left._acc)
    with pytest.raises(ValueError):
        left.merge(V.NowcastVerifier(4, 3, SCALES, THRESHOLDS))


def test_verifier_compute():
    f, o = _verifier_inputs(b=2, t=2, c=1, m=4)
    o[:, 1] = -1.0  # lead time 1: nothing observed
    v = V.NowcastVerifier(4, 2, SCALES, THRESHOLDS)
    v.update(f, o)
    res = v.compute()
    ref = V.ensemble_scores_reference(f[:, :, 0].reshape(4, 2, 32, 32).numpy(), o[:, 0].reshape(2, 32, 32).numpy(), SCALES, THRESHOLDS)
    for pi, pool in enumerate(("avg", "max")):
        for si, s in enumerate(SCALES):
            n = ref.cells[:, si].sum()
            crps = ref.abs_err[:, pi, si].sum() / n - ref.pair[:, pi, si].sum() / (16 * n)
            fair = ref.abs_err[:, pi, si].sum() / n - ref.pair[:, pi, si].sum() / (12 * n)
            assert np.isclose(res["crps"][pool][s][0], crps, rtol=1e-13) and np.isclose(res["crps_fair"][pool][s][0], fair, rtol=1e-13)
            assert np.isnan(res["crps"][pool][s][1]) and np.isnan(res["crps_fair"][pool][s][1])
    cont = ref.contingency.sum(axis=0)  # [K, M, 3]
    for k, t in enumerate(THRESHOLDS):
        assert np.isclose(res["csi"][t][0], cont[k, :, 0].sum() / cont[k].sum(), rtol=1e-15) and np.isnan(res["csi"][t][1])
    assert res["csi_members"].shape == (3, 4, 2)
    assert np.allclose(res["csi_members"][:, :, 0], cont[..., 0] / cont.sum(axis=2), rtol=1e-15)
    assert res["rank_histogram"].shape == (2, 5) and np.isclose(res["rank_histogram"][0].sum(), 1.0)
    assert np.isnan(res["rank_histogram"][1]).all() and np.isnan(res["rank_histogram_wet"][1]).all()
    dry = ref.ranks.sum(axis=0)[0, 4]
    assert dry > 0 and np.isclose(res["rank_histogram_wet"][0].sum(), 1.0)
    assert res["rank_histogram_wet"][0][2] != res["rank_histogram"][0][2]
    assert np.array_equal(res["cells"][0], ref.cells.sum(axis=0)) and (res["cells"][1] == 0).all()


def test_fair_crps_needs_two_members():
    f, o = _verifier_inputs(b=1, t=2, c=1, m=1)
    v = V.NowcastVerifier(1, 2, (1,), ())
    v.update(f[:, 0], o[0])
    res = v.compute()
    assert np.isnan(res["crps_fair"]["avg"][1]).all() and np.isfinite(res["crps"]["avg"][1]).all()
    assert np.isnan(V.NowcastVerifier(3, 2).compute()["crps"]["max"][16]).all()  # nothing accumulated yet: NaN, not an exception


def test_ensemble_scores_on_cpu_tensors_is_the_reference():
    f, o = make_case(3, 4, 32, 48, "radar")
    ref = V.ensemble_scores_reference(f, o, (2, 8), (0.5,))
    got = V.ensemble_scores(torch.from_numpy(f).view(3, 2, 2, 32, 48), torch.from_numpy(o).view(2, 2, 32, 48), (2, 8), (0.5,))
    for u, v in zip(got, ref):
        assert isinstance(u, torch.Tensor) and np.array_equal(u.numpy(), v)
    out = V.EnsembleScores(*(torch.empty_like(u) for u in got))
    assert V.ensemble_scores(torch.from_numpy(f), torch.from_numpy(o), (2, 8), (0.5,), out=out) is out
    assert all(torch.equal(u, v) for u, v in zip(out, got))


def test_observed_from_frames_keeps_missing():
    raw = np.array([0, 5, -1, 320], np.int16).reshape(1, 2, 2, 1)
    got = V.observed_from_frames(raw, scale=1 / 32, offset=0.0)
    assert got.shape == (1, 1, 2, 2) and got.dtype == torch.float32 and got.is_contiguous()
    assert got.flatten().tolist() == [0.0, 5 / 32, -1 / 32, 10.0]
    assert torch.isnan(V.observed_from_frames(torch.full((2, 4, 4, 3), float("nan")), 2.0, 1.0)).all()


@pytest.mark.parametrize("kwargs,shape", [
    (dict(), (33, 1, 16, 16)),
    (dict(), (2, 1, 24, 16)),
    (dict(), (2, 1, 16, 40)),
    (dict(scales=(1, 3)), (2, 1, 16, 16)),
    (dict(scales=(4, 4)), (2, 1, 16, 16)),
    (dict(scales=()), (2, 1, 16, 16)),
    (dict(thresholds=tuple(range(9))), (2, 1, 16, 16)),
])
def test_bad_arguments_raise_value_error(kwargs, shape):
    f = torch.zeros(shape)
    with pytest.raises(ValueError):
        V.ensemble_scores(f, torch.zeros(shape[1:]), **kwargs)
    with pytest.raises(ValueError):
        V.ensemble_scores_reference(f.numpy(), np.zeros(shape[1:], np.float32), **kwargs)


def test_mismatched_inputs_raise():
    with pytest.raises(ValueError):
        V.ensemble_scores(torch.zeros(2, 3, 16, 16), torch.zeros(2, 16, 16))
    with pytest.raises(ValueError):
        V.ensemble_scores(torch.zeros(2, 3, 16, 16, dtype=torch.float64), torch.zeros(3, 16, 16, dtype=torch.float64))
    with pytest.raises(ValueError):
        V.NowcastVerifier(33, 2)
    with pytest.raises(ValueError):
        V.NowcastVerifier(4, 2).update(torch.zeros(4, 3, 1, 16, 16), torch.zeros(3, 1, 16, 16))


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_library_exports_the_new_symbols_under_the_same_abi(lib):
    assert hasattr(lib, "dgmr_ensemble_scores") and hasattr(lib, "dgmr_ensemble_scores_workspace")
    assert lib.dgmr_abi_version() == 13
    # 4096 workgroups' worth of 20 doubles at most for a few planes; one row per plane when there are many planes
    assert lib.dgmr_ensemble_scores_workspace(6, 18, 1536, 1280) == 18 * (4096 // 18) * 20 * 8
    assert lib.dgmr_ensemble_scores_workspace(6, 1, 16, 16) == 20 * 8
    assert lib.dgmr_ensemble_scores_workspace(6, 10000, 256, 256) == 10000 * 20 * 8
    assert lib.dgmr_ensemble_scores_workspace(33, 1, 16, 16) < 0 and lib.dgmr_ensemble_scores_workspace(2, 1, 24, 16) < 0


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """Every refusal comes from the argument checks at the top of dgmr_ensemble_scores: nothing is enqueued (there is no device here,
    and the pointers are host buffers that are never dereferenced)."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def go(m=2, n=1, h=16, w=16, scales=(1, 4, 16), k=3, stride=256, fc=base, ws_bytes=1 << 20, thr=base):
        arr = (ctypes.c_int * max(len(scales), 1))(*scales)
        return lib.dgmr_ensemble_scores(fc, stride, base, m, n, h, w, arr, len(scales), thr, k, base, ws_bytes, base, base, base, base,
                                        base, None)

    for bad, text in [(dict(m=33), b"members"), (dict(m=0), b"members"), (dict(h=24), b"multiples of 16"), (dict(w=8), b"multiples of 16"),
                      (dict(scales=(1, 3)), b"scale 3"), (dict(scales=(2, 2)), b"twice"), (dict(scales=()), b"scales"),
                      (dict(k=9), b"thresholds"), (dict(stride=258), b"member_stride"), (dict(fc=base + 4), b"16-byte aligned"),
                      (dict(fc=None), b"null pointer"), (dict(thr=None), b"null pointer"), (dict(ws_bytes=8), b"workspace"), (dict(n=0), b"planes")]:
        assert go(**bad) < 0, bad
        assert text in lib.dgmr_last_error(), (bad, lib.dgmr_last_error())
