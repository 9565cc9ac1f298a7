"""Exceedance tables on the GPU: dgmr_exceedance_table (csrc/verify.hip) against value.exceedance_table_reference on the same arrays,
exactly, and ValueVerifier's device accumulator.  No test has a time threshold."""
import functools

import numpy as np
import pytest
import torch

from spectra_recipe import THRESHOLDS, THRESHOLDS8, make_ensemble

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 16), (3, 32, 48), (1, 256, 256)]
THRESHOLD_SETS = {0: (), 3: THRESHOLDS, 8: THRESHOLDS8}


@functools.lru_cache(maxsize=None)
def _case(m, shape):
    f, o = make_ensemble(m, *shape, "radar")
    for a in (f, o):
        a.setflags(write=False)
    return f, o


def _table(f, o, thr):
    from skillful_nowcasting_amd.value import exceedance_table

    t = exceedance_table(f if isinstance(f, torch.Tensor) else torch.from_numpy(f.copy()).cuda(),
                         o if isinstance(o, torch.Tensor) else torch.from_numpy(o.copy()).cuda(), thr)
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("k", sorted(THRESHOLD_SETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("m", [1, 6, 32])
def test_table_equals_the_reference(m, shape, k):
    """The "radar" kind: 70 % zeros, values exactly on the thresholds 1, 4 and 8; scattered negatives / NaN / -inf, one missing 16 x 16
    cell and (N > 1) one whole missing plane in the observation."""
    from skillful_nowcasting_amd.value import exceedance_table_reference

    f, o = _case(m, shape)
    thr = THRESHOLD_SETS[k]
    ref = exceedance_table_reference(f, o, thr)
    got = _table(f, o, thr)
    assert got.dtype == torch.int64 and tuple(got.shape) == (shape[0], k, m + 1, 2)
    assert np.array_equal(got.cpu().numpy(), ref)
    if k:
        assert ref[0].sum() > 0 and ref[0, :, 1:].sum() > 0 and ref[0, ..., 1].sum() > 0
        if shape[0] > 1:
            assert (ref[-1] == 0).all()  # the all-missing plane


def test_nan_members_reach_no_threshold():
    from skillful_nowcasting_amd.value import exceedance_table_reference

    f, o = (a.copy() for a in _case(6, (3, 32, 48)))
    rng = np.random.Generator(np.random.PCG64(70))
    f[:, 0][rng.random(f[:, 0].shape) < 0.05] = np.nan
    f[3, 1] = np.inf
    ref = exceedance_table_reference(f, o, THRESHOLDS8)
    assert np.array_equal(_table(f, o, THRESHOLDS8).cpu().numpy(), ref)


def test_strided_members_and_unflattened_planes():
    """`full[:, 1]` of an [M, 3, N, H, W] tensor is read in place through the member stride."""
    from skillful_nowcasting_amd.value import exceedance_table_reference
    from skillful_nowcasting_amd.verification import _planes_contiguous

    f, o = _case(6, (3, 32, 48))
    ref = exceedance_table_reference(f, o, THRESHOLDS)
    full = torch.rand(6, 3, 3, 32, 48, generator=torch.Generator().manual_seed(0)).cuda()
    full[:, 1] = torch.from_numpy(f.copy()).cuda()
    view = full[:, 1]
    assert not view.is_contiguous() and _planes_contiguous(view)
    obs = torch.from_numpy(o.copy()).cuda()
    assert np.array_equal(_table(view, obs, THRESHOLDS).cpu().numpy(), ref)
    assert np.array_equal(_table(view.view(6, 3, 1, 32, 48), obs.view(3, 1, 32, 48), THRESHOLDS).cpu().numpy(), ref)
    members_innermost = view.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)  # a layout that has to be copied
    assert np.array_equal(_table(members_innermost, obs, THRESHOLDS).cpu().numpy(), ref)
    a, b = _table(view, obs, THRESHOLDS), _table(view, obs, THRESHOLDS)
    assert torch.equal(a, b)


def test_runs_on_the_callers_stream():
    from skillful_nowcasting_amd.value import exceedance_table, exceedance_table_reference

    f, o = _case(6, (3, 32, 48))
    fc, ob = torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = exceedance_table(fc, ob, THRESHOLDS)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), exceedance_table_reference(f, o, THRESHOLDS))


def test_value_verifier_on_the_device_against_cpu_tensors():
    """The same updates on device and on CPU tensors: the tables are integers and the weights small integers, so the accumulators are
    equal exactly and compute() agrees to float64 rounding."""
    from skillful_nowcasting_amd.value import ValueVerifier

    m, b, t, c = 6, 2, 2, 2
    f, o = make_ensemble(m, b * t * c, 32, 48, "radar", seed=11)
    o[-1] = o[1]
    f, o = f.reshape(m, b, t, c, 32, 48), o.reshape(b, t, c, 32, 48)
    w = [2.0, 5.0]
    dev, host = ValueVerifier(m, t, THRESHOLDS), ValueVerifier(m, t, THRESHOLDS)
    dev.update(torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda(), weights=w)
    host.update(torch.from_numpy(f), torch.from_numpy(o), weights=w)
    torch.cuda.synchronize()
    assert dev._acc.is_cuda and dev._acc.dtype == torch.float64 and torch.equal(dev._acc.cpu(), host._acc)
    a, h = dev.compute(), host.compute()
    for key in ("base_rate", "hit_rate", "false_alarm_rate", "brier"):
        assert np.allclose(a[key], h[key], rtol=1e-15, atol=0, equal_nan=True), key
    for key in ("observed_frequency", "count"):
        assert np.allclose(a["reliability"][key], h["reliability"][key], rtol=1e-15, atol=0, equal_nan=True), key
    for thr in THRESHOLDS:
        assert np.allclose(a["value"][thr], h["value"][thr], rtol=1e-15, atol=0, equal_nan=True)
        assert np.isfinite(h["value"][thr]).all() and (h["value"][thr] <= 1.0).all()
