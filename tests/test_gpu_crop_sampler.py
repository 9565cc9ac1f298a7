"""Importance-sampled crops on the GPU: dgmr_crop_scores and dgmr_crop_gather against their numpy / torch specifications, the
device loader against the host loader by equality, and one training step fed from it."""
import ctypes
import gc

import numpy as np
import pytest
import torch

import crop_sampler_recipe as R
from crop_sampler_recipe import collect, loader, make_rows, reference_selection

pytestmark = pytest.mark.gpu

DEV = "cuda"
# (name, T, H, W, C, cell, crop): the recipe; ragged H and W (a remainder beyond the last full cell); two channels (the channel
# stride); several workgroups per band and several bands, the last workgroup of a band one cell short; and the two other reduction
# paths of pass 1 - a cell run of 24 elements (no power of two: added lane after lane) and one of 96 (wider than a wave).
GEOMETRIES = [("recipe", R.T, R.H, R.W, R.C, R.CELL, R.CROP), ("ragged", 3, 43, 61, 1, 8, 16), ("two_channels", 2, 32, 48, 2, 8, 16),
              ("bands", 5, 96, 160, 1, 32, 64), ("run24", 2, 32, 48, 3, 8, 16), ("run96", 2, 64, 96, 3, 32, 32)]


def score_bound(n_terms):
    """All terms are non-negative, so naive double summation in ANY order loses at most (n - 1) * 2^-53 relative; + 16 for a few ulp of
    the device's double expm1 per term and the cell / box regrouping."""
    return (n_terms + 16) * 2.0 ** -52


@pytest.fixture(scope="module")
def data():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import data as D

    return D


@pytest.fixture(scope="module")
def lib(data):
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def check_scores(D, raw, scale, offset, sat, cell, crop, what):
    t, h, w, c = raw.shape
    want_s, want_m = D.crop_scores_reference(raw, scale, offset, sat, cell, crop)
    dev = torch.from_numpy(raw).to(DEV)
    got_s, got_m = D.crop_scores(dev, scale, offset, sat, cell, crop)
    again_s, again_m = D.crop_scores(dev, scale, offset, sat, cell, crop)
    torch.cuda.synchronize()
    assert got_s.dtype == torch.float64 and got_m.dtype == torch.int32 and got_s.shape == want_s.shape == got_m.shape
    assert torch.equal(got_m.cpu().long(), torch.from_numpy(want_m)), what
    gs = got_s.cpu().numpy()
    err = np.abs(gs - want_s) / np.where(want_s > 0, want_s, 1.0)
    print(f"{what}: scores {want_s.min():.4g} ... {want_s.max():.4g}, missing {want_m.min()} ... {want_m.max()}, "
          f"max rel err {err.max():.3e} (bound {score_bound(t * c * crop * crop):.3e})")
    assert np.all(np.abs(gs - want_s) <= score_bound(t * c * crop * crop) * want_s), what
    assert np.all(gs[want_s == 0.0] == 0.0), what  # wholly dry candidates: exactly
    assert torch.equal(got_s, again_s) and torch.equal(got_m, again_m), what  # two launches: the same bits
    return want_s, want_m


# ---- scores ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_scores_on_the_recipe(data, dtype):
    raw, scale, offset = R.recipe(dtype)
    want_s, want_m = check_scores(data, raw, scale, offset, 1.0, R.CELL, R.CROP, f"recipe {dtype}")
    assert (want_s == 0.0).any() and want_s.max() > 100.0 and want_m.min() > 0 and want_m.max() > 0.5 * R.N_ELEMENTS


@pytest.mark.parametrize("geometry", GEOMETRIES[1:], ids=[g[0] for g in GEOMETRIES[1:]])
@pytest.mark.parametrize("dtype", ("int16", "float32"))
def test_scores_other_geometries(data, geometry, dtype):
    name, t, h, w, c, cell, crop = geometry
    v, holes = R.field(seed=21, t=t, h=h, w=w, c=c, centre=(h // 3, 2 * w // 3), widths=(h / 4.0, w / 4.0))  # rain in every band
    hc, wc = h // cell * cell, w // cell * cell
    if (hc, wc) != (h, w):  # the remainder beyond the last full cell belongs to no candidate: soak it and punch holes into it
        v[:, hc:], v[:, :, wc:] = 3000.0, 3000.0
        holes[:, hc:, ::2], holes[:, ::2, wc:] = True, True
    raw, scale, offset = R.encode(v, holes, dtype)
    check_scores(data, raw, scale, offset, 2.0, cell, crop, f"{name} {dtype}")


# ---- gather ----------------------------------------------------------------------------------------------------------------------
def gathered_reference(raw, scale, offset, origins, crop):
    x = torch.from_numpy(raw).float() * scale + offset
    return torch.stack([x[:, y:y + crop, xx:xx + crop, :].permute(0, 3, 1, 2) for y, xx in origins])


def check_gather(D, raw, scale, offset, origins, crop):
    want = gathered_reference(raw, scale, offset, origins, crop)
    dev = torch.from_numpy(raw).to(DEV)
    got = D.gather_crops(dev, origins, crop, scale, offset).cpu()
    assert got.shape == want.shape and got.dtype == torch.float32
    assert torch.equal(got.isnan(), want.isnan())  # NaNs by position ...
    assert torch.equal(got[~want.isnan()], want[~want.isnan()])  # ... everything else by value
    missing = ~(want >= 0)
    assert missing.any() and (~missing).any()
    clamped = D.gather_crops(dev, origins, crop, scale, offset, clamp_missing=True, missing_fill=-1.0).cpu()
    assert torch.equal(clamped == -1.0, missing)  # exactly the reference's missing positions hold the fill
    assert torch.equal(clamped[~missing], want[~missing])


@pytest.mark.parametrize("dtype", R.DTYPES)
def test_gather_on_the_recipe(data, dtype):
    raw, scale, offset = R.recipe(dtype)
    origins = [(0, 0), (R.H - R.CROP, R.W - R.CROP), (3, 5), (7, 39), (7, 39)]
    check_gather(data, raw, scale, offset, origins, R.CROP)


def test_gather_two_channels(data):
    raw, scale, offset = R.recipe("int16", seed=21, t=2, h=32, w=48, c=2)
    check_gather(data, raw, scale, offset, [(0, 0), (16, 32), (5, 3), (9, 27)], 16)
    raw, scale, offset = R.recipe("uint8", seed=22, t=2, h=32, w=48, c=2)
    check_gather(data, raw, scale, offset, [(16, 32), (1, 31)], 16)


def test_gather_nothing_and_bad_origins(data, lib):
    raw, scale, offset = R.recipe("int16")
    dev = torch.from_numpy(raw).to(DEV)
    out = torch.full((2, R.T, R.C, R.CROP, R.CROP), -123.0, device=DEV)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.dgmr_crop_gather(dev.data_ptr(), 1, R.T, R.H, R.W, R.C, None, 0, R.CROP, scale, offset, 0, 0.0, out.data_ptr(), stream)
    torch.cuda.synchronize()
    assert rc == 0 and bool((out == -123.0).all())
    empty = data.gather_crops(dev, np.zeros((0, 2), np.int64), R.CROP, scale, offset)
    assert empty.shape == (0, R.T, R.C, R.CROP, R.CROP)
    # the wrapper validates on the host and raises before anything is uploaded or launched
    for bad in [(R.H - R.CROP + 1, 0), (0, R.W - R.CROP + 1), (-1, 0), (0, -1)]:
        with pytest.raises(ValueError, match="origin"):
            data.gather_crops(dev, [(0, 0), bad], R.CROP, scale, offset, out=out)
    torch.cuda.synchronize()
    assert bool((out == -123.0).all())


# ---- the loader: device against host ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_loader_device_equals_host(data, dtype):
    rows, scale, offset = make_rows(dtype)
    # what makes equality a fair demand: no candidate's u lies within 1e-6 of its q (the kernel's tolerance moves q by < 1e-12)
    want_o, _, margin = reference_selection(rows, scale, offset, seed=3)
    print(f"{dtype}: {len(want_o)} crops, min |u - q| = {margin:.3e}")
    assert margin >= 1e-6 and len(want_o) >= 6
    host_loader, dev_loader = loader(rows, scale, offset, seed=3, missing_fill=-1.0), loader(rows, scale, offset, seed=3, missing_fill=-1.0, device=DEV)
    host, dev = collect(host_loader), collect(dev_loader)
    assert len(host) == len(dev) == len(want_o) // 3
    for (hi, hf, ho, hq), (di, df, do, dq) in zip(host, dev):
        assert di.is_cuda and df.is_cuda and di.dtype == torch.float32
        assert torch.equal(di.cpu(), hi) and torch.equal(df.cpu(), hf)
        assert np.array_equal(ho, do)
        # The inclusion probabilities are compared within a derived bound, not by `==`: q = q_min + m / n * score is formed in double
        # on both sides from scores that are only promised to agree to score_bound (another summation order, another expm1), so bit
        # equality of q cannot be demanded; what follows from the promise is the scores' bound and two roundings more.  Batches,
        # origins and stats ARE compared by equality, for every candidate.
        assert np.all(np.abs(hq - dq) <= (score_bound(R.N_ELEMENTS) + 2.0 ** -51) * hq)
    assert np.array_equal(np.concatenate([o for _, _, o, _ in dev]), want_o[:len(dev) * 3])
    assert host_loader.stats == dev_loader.stats
    # a final partial batch and the missing limit take the same way on both sides
    kw = dict(seed=3, batch_size=4, drop_last=False, max_missing=0.25, max_crops_per_row=5)
    host, dev = collect(loader(rows, scale, offset, **kw)), collect(loader(rows, scale, offset, device=DEV, **kw))
    assert len(host) == len(dev) > 0
    for (hi, hf, ho, hq), (di, df, do, dq) in zip(host, dev):
        assert torch.equal(di.cpu(), hi) and torch.equal(df.cpu(), hf) and np.array_equal(ho, do)


# ---- one training step fed from the loader ---------------------------------------------------------------------------------------
def test_training_step_from_the_loader(data):
    import skillful_nowcasting_amd as S

    rows = [R.recipe("int16", seed=31 + k, t=6, h=160, w=192)[0] for k in range(2)]
    ld = data.ImportanceCropLoader(rows, batch_size=2, device=DEV, crop=128, stride=32, q_min=0.5, m=4.0, scale=1.0 / 32.0,
                                   num_input_frames=4, num_target_frames=2)
    torch.manual_seed(0)
    model = S.DGMR(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2).to(DEV)
    images, future = next(iter(ld))
    assert images.shape == (2, 4, 1, 128, 128) and future.shape == (2, 2, 1, 128, 128)
    assert bool((images >= 0).all()) and bool((future >= 0).all())  # holes clamped to the fill
    losses = model.training_step((images, future), 0)
    torch.cuda.synchronize()
    vals = {k: float(v) for k, v in losses.items()}
    assert vals and all(np.isfinite(v) for v in vals.values()), vals
    del model, losses, images, future, ld  # (a model is cyclic garbage: leave none behind for the tests that count cache entries)
    gc.collect()
