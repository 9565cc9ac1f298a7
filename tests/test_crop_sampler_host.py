"""Importance-sampled crops from full frames, host side: the numpy specification of the score kernel against the definition, the
inclusion probability, ImportanceCropLoader(device=None) end to end, and the two new entry points at the C-ABI boundary.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import crop_sampler_recipe as R
from crop_sampler_recipe import collect, loader, make_rows, reference_selection
from skillful_nowcasting_amd.data import crop_scores, crop_scores_reference, gather_crops, inclusion_probability, row_to_sample


def hand_cropped(rows, scale, offset, origin, fill=0.0, clamp=True):
    index, y, x = origin
    images, future = row_to_sample(torch.from_numpy(rows[index][:, y:y + R.CROP, x:x + R.CROP, :]), R.N_IN, R.N_OUT)
    out = []
    for part in (images, future):
        v = part.float() * scale + offset
        out.append(torch.where(v >= 0, v, torch.full_like(v, fill)) if clamp else v)
    return out


# ---- the specification of the score kernel ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_reference_scores_match_the_definition(dtype):
    raw, scale, offset = R.recipe(dtype)
    scores, missing = crop_scores_reference(raw, scale, offset, 1.0, R.CELL, R.CROP)
    assert scores.dtype == np.float64 and missing.dtype == np.int64 and scores.shape == missing.shape == (R.GY, R.GX)
    want_s, want_m = R.brute_force(raw, scale, offset, 1.0, R.CELL, R.CROP)
    want_s, want_m = np.array(want_s), np.array(want_m)
    # the recipe spans the cases: wholly dry candidates, soaked ones, and missing counts from a handful to more than half a crop
    assert (want_s == 0.0).any() and want_s.max() > 100.0
    assert want_m.min() < 0.01 * R.N_ELEMENTS and want_m.max() > 0.5 * R.N_ELEMENTS
    assert np.array_equal(missing, want_m)
    assert np.all(np.abs(scores - want_s) <= 1e-12 * want_s)
    assert np.all(scores[want_s == 0.0] == 0.0)  # exactly


def test_reference_scores_other_sat_scale_and_cpu_wrapper():
    raw, scale, offset = R.recipe("int16")
    s, m = crop_scores_reference(raw, scale, offset, 3.5, R.CELL, R.CROP)
    want_s, want_m = R.brute_force(raw, scale, offset, 3.5, R.CELL, R.CROP)
    assert np.allclose(s, np.array(want_s), rtol=1e-12, atol=0.0) and np.array_equal(m, np.array(want_m))
    ts, tm = crop_scores(torch.from_numpy(raw), scale, offset, 3.5, R.CELL, R.CROP)  # a CPU tensor runs the reference
    assert ts.dtype == torch.float64 and tm.dtype == torch.int32
    assert np.array_equal(ts.numpy(), s) and np.array_equal(tm.numpy(), m)


def test_inclusion_probability():
    scores = np.array([[0.0, 10.0], [1536.0, 1e9]])
    q = inclusion_probability(scores, 1536, q_min=0.05, m=4.0)
    assert q.dtype == np.float64 and q.shape == scores.shape
    assert q[0, 0] == 0.05  # a dry crop keeps the floor
    assert q[0, 1] == 0.05 + 4.0 * 10.0 / 1536.0
    assert q[1, 0] == 1.0 and q[1, 1] == 1.0  # clamped
    assert np.array_equal(inclusion_probability(scores, 1536), np.minimum(1.0, 2e-4 + 0.1 * scores / 1536))  # the paper's defaults


def test_cpu_gather_matches_slicing():
    raw, scale, offset = R.recipe("uint8")
    origins = [(0, 0), (R.H - R.CROP, R.W - R.CROP), (3, 5)]
    got = gather_crops(torch.from_numpy(raw), origins, R.CROP, scale, offset)
    assert got.shape == (3, R.T, R.C, R.CROP, R.CROP) and got.dtype == torch.float32
    for k, (y, x) in enumerate(origins):
        want = torch.from_numpy(raw[:, y:y + R.CROP, x:x + R.CROP, :]).permute(0, 3, 1, 2).float() * scale + offset
        assert torch.equal(got[k], want)
    clamped = gather_crops(torch.from_numpy(raw), origins, R.CROP, scale, offset, clamp_missing=True, missing_fill=-1.0)
    assert torch.equal(clamped, torch.where(got >= 0, got, torch.full_like(got, -1.0))) and (clamped == -1.0).any()
    with pytest.raises(ValueError, match="origin"):
        gather_crops(torch.from_numpy(raw), [(R.H - R.CROP + 1, 0)], R.CROP, scale, offset)


# ---- the loader on the host ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_loader_yields_the_reference_selection(dtype):
    """Three rows, batches of three: every sample is the hand-cropped row through row_to_sample and the affine; origins and inclusion
    probabilities are the reference draw's, in its order; batches run across rows."""
    rows, scale, offset = make_rows(dtype)
    want_o, want_q, _ = reference_selection(rows, scale, offset)
    assert len(want_o) >= 7 and len(set(want_o[:, 0])) == 3, want_o  # several batches, every row contributes
    ld = loader(rows, scale, offset)
    batches = collect(ld)
    assert len(batches) == len(want_o) // 3
    assert any(len(set(o[:, 0])) > 1 for _, _, o, _ in batches), "no batch was assembled across rows"
    k = 0
    for images, future, origins, q in batches:
        assert images.shape == (3, R.N_IN, R.C, R.CROP, R.CROP) and future.shape == (3, R.N_OUT, R.C, R.CROP, R.CROP)
        assert images.dtype == future.dtype == torch.float32
        assert origins.shape == (3, 3) and q.shape == (3,) and q.dtype == np.float64
        for b in range(3):
            assert tuple(origins[b]) == tuple(want_o[k]) and q[b] == want_q[k]
            wi, wf = hand_cropped(rows, scale, offset, origins[b])
            assert torch.equal(images[b], wi) and torch.equal(future[b], wf)
            k += 1
    assert ld.stats == {"rows": 3, "candidates": 3 * R.GY * R.GX, "accepted": len(want_o), "rejected_missing": 0}


def test_loader_seed_and_drop_last():
    rows, scale, offset = make_rows("int16")
    a, b = collect(loader(rows, scale, offset, seed=5)), collect(loader(rows, scale, offset, seed=5))
    assert len(a) == len(b) > 0
    for x, y in zip(a, b):
        assert torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) and np.array_equal(x[2], y[2]) and np.array_equal(x[3], y[3])
    c = collect(loader(rows, scale, offset, seed=6))
    assert [o.tolist() for _, _, o, _ in c] != [o.tolist() for _, _, o, _ in a]
    # drop_last both ways, at a batch size that leaves a remainder
    want_o, _, _ = reference_selection(rows, scale, offset, seed=5)
    size = next(s for s in (4, 5, 3, 7) if len(want_o) % s)
    kept = collect(loader(rows, scale, offset, seed=5, batch_size=size, drop_last=False))
    dropped = collect(loader(rows, scale, offset, seed=5, batch_size=size, drop_last=True))
    assert len(dropped) == len(want_o) // size and len(kept) == len(dropped) + 1
    assert kept[-1][0].shape[0] == len(want_o) % size == len(kept[-1][2]) == len(kept[-1][3])
    assert np.array_equal(np.concatenate([o for _, _, o, _ in kept]), want_o)
    # the same row twice from one iterator object: iteration restarts the generator
    ld = loader(rows, scale, offset, seed=5)
    assert [o.tolist() for _, _, o, _ in collect(ld)] == [o.tolist() for _, _, o, _ in collect(ld)]


def test_loader_max_crops_per_row():
    rows, scale, offset = make_rows("uint8")
    full, _, _ = reference_selection(rows, scale, offset)
    assert max(np.bincount(full[:, 0])) > 2
    want_o, _, _ = reference_selection(rows, scale, offset, max_crops_per_row=2)
    assert len(want_o) == 6
    ld = loader(rows, scale, offset, max_crops_per_row=2, batch_size=2)
    got = np.concatenate([o for _, _, o, _ in collect(ld)])
    assert np.array_equal(got, want_o)
    # the cut keeps the head of the permuted accept list
    for r in range(3):
        assert np.array_equal(want_o[want_o[:, 0] == r], full[full[:, 0] == r][:2])
    assert ld.stats["accepted"] == 6


def test_loader_max_missing_excludes_exactly_the_holed_candidates():
    rows, scale, offset = make_rows("int16", n=1)
    _, miss = crop_scores_reference(rows[0][-R.T:], scale, offset, 1.0, R.CELL, R.CROP)
    over = miss.reshape(-1) > 0.25 * R.N_ELEMENTS
    assert over.any() and (~over).any()
    ld = loader(rows, scale, offset, q_min=1.0, max_missing=0.25, batch_size=1)
    got = np.concatenate([o for _, _, o, _ in collect(ld)])
    got_ids = sorted((got[:, 1] // R.CELL * R.GX + got[:, 2] // R.CELL).tolist())
    assert got_ids == np.flatnonzero(~over).tolist()
    assert ld.stats["rejected_missing"] == int(over.sum()) and ld.stats["accepted"] == int((~over).sum())
    assert np.all(ld.last_inclusion_prob == 1.0)


def test_loader_clamp_and_fill():
    rows, scale, offset = make_rows("float32", n=1)
    raw = collect(loader(rows, scale, offset, q_min=1.0, batch_size=1, clamp_missing=False))
    filled = collect(loader(rows, scale, offset, q_min=1.0, batch_size=1, missing_fill=-2.0))
    assert len(raw) == len(filled) == R.GY * R.GX
    seen = False
    for (ri, rf, ro, _), (fi, ff, fo, _) in zip(raw, filled):
        assert np.array_equal(ro, fo)
        wi, wf = hand_cropped(rows, scale, offset, ro[0], clamp=False)
        assert torch.equal(ri[0], wi) and torch.equal(rf[0], wf)  # -inf holes pass through
        wi, wf = hand_cropped(rows, scale, offset, ro[0], fill=-2.0)
        assert torch.equal(fi[0], wi) and torch.equal(ff[0], wf)
        seen = seen or bool((fi == -2.0).any())
    assert seen


def test_loader_refuses_bad_rows_and_geometry():
    rows, scale, offset = make_rows("int16", n=1)
    with pytest.raises(ValueError, match="frames"):
        next(iter(loader([rows[0][:R.T - 1]], scale, offset)))  # shorter than 2 + 4 frames
    with pytest.raises(ValueError, match="smaller than the crop"):
        next(iter(loader([rows[0][:, :R.CROP - 1]], scale, offset)))  # H < crop
    with pytest.raises(ValueError, match="multiple"):
        loader(rows, scale, offset, stride=5)  # crop % stride != 0
    with pytest.raises(ValueError, match="dtype"):
        next(iter(loader([rows[0].astype(np.float64)], scale, offset)))


# ---- the C-ABI boundary ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_symbols_are_exported_bound_and_declared(lib):
    from conftest import ROOT
    from skillful_nowcasting_amd import _lib

    src = open(os.path.join(ROOT, "include", "dgmr_hip.h")).read()
    for k, name in enumerate(("DGMR_DT_U8", "DGMR_DT_I16", "DGMR_DT_F16", "DGMR_DT_F32")):
        assert re.search(r"#define %s %d\b" % (name, k), src), name
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("dgmr_crop_scores", 16), ("dgmr_crop_gather", 15)):
        assert hasattr(lib, name), name
        assert len(_lib.SIGNATURES[name]) == nargs, name
        m = re.search(r"\bint %s\s*\((.*?)\);" % name, src, flags=re.S)
        assert m is not None, f"{name} is not declared in include/dgmr_hip.h"
        assert len(m.group(1).split(",")) == nargs, name
    assert lib.dgmr_abi_version() == 13 == _lib.ABI_VERSION  # new symbols only


def test_entry_points_report_argument_errors_without_a_gpu(lib):
    """Unknown dtype, crop % cell != 0, H < crop, W < crop and non-positive extents are refused before any launch."""
    buf = (ctypes.c_double * 16)()  # stands for any non-null pointer: a refused call reads nothing
    p = ctypes.cast(buf, ctypes.c_void_p)

    def scores(dtype=1, t=2, h=32, w=48, c=1, sat=1.0, cell=8, crop=16):
        return lib.dgmr_crop_scores(p, dtype, t, h, w, c, 1.0, 0.0, sat, cell, crop, p, p, p, p, None)

    def gather(dtype=1, t=2, h=32, w=48, c=1, n=1, crop=16):
        return lib.dgmr_crop_gather(p, dtype, t, h, w, c, p, n, crop, 1.0, 0.0, 0, 0.0, p, None)

    for fn, name in ((scores, b"dgmr_crop_scores"), (gather, b"dgmr_crop_gather")):
        for bad in (dict(dtype=4), dict(dtype=-1), dict(h=15), dict(w=15), dict(t=0), dict(c=0), dict(h=-32), dict(crop=0)):
            assert fn(**bad) < 0 and name in lib.dgmr_last_error(), (name, bad)
    assert scores(cell=5) < 0 and b"multiple" in lib.dgmr_last_error()
    assert scores(cell=0) < 0 and scores(sat=0.0) < 0 and scores(sat=float("nan")) < 0
    assert gather(n=-1) < 0
    assert lib.dgmr_crop_scores(None, 1, 2, 32, 48, 1, 1.0, 0.0, 1.0, 8, 16, p, p, p, p, None) < 0 and b"null" in lib.dgmr_last_error()
    assert lib.dgmr_crop_gather(p, 1, 2, 32, 48, 1, p, 1, 16, 1.0, 0.0, 0, 0.0, None, None) < 0 and b"null" in lib.dgmr_last_error()
    assert lib.dgmr_crop_gather(p, 1, 2, 32, 48, 1, None, 0, 16, 1.0, 0.0, 0, 0.0, None, None) == 0  # N == 0: nothing to do
