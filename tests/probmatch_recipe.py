"""Inputs, the exact-rank comparison and the exceedance bound shared by the probability-matching tests
(tests/test_probmatch_host.py, tests/test_gpu_probmatch.py)."""
import functools

import numpy as np
import torch

import stochastic_recipe as R

LO, SCALE, BINS = np.float32(-64.0), np.float32(32.0), 4096
THRESHOLDS_DB = (5.0, 15.0, 21.0, 25.0)  # 0.1 / 1 / 4 / 10 mm/h in `to_db` units
# name -> (window, size): the radar field of spectra_recipe (seed 3) through spectral_ar_reference with lifetime_rho, 4 members
MEMBER_CASES = {"128 L32": (32, 128), "256 L64": (64, 256)}
# name -> (P, M, T, H, W): the smallest planes that reach every path of dgmr_probability_match
DEVICE_CASES = {
    "32x48": (2, 2, 3, 32, 48),       # a plane smaller than one workgroup's chunk, 16-byte path
    "33x47": (1, 2, 2, 33, 47),       # H W no multiple of 4: the 4-byte path by shape
    "256x320": (1, 1, 2, 256, 320),   # a plane of three chunks, the last one half full
}


def bins_of(z, lo=LO, scale=SCALE):
    """The bin of every element by the specification's rule, written out independently: fp32 (z - lo) * scale, clamped."""
    with np.errstate(invalid="ignore", over="ignore"):
        u = (np.asarray(z, np.float32) - np.float32(lo)) * np.float32(scale)
    b = np.zeros(u.shape, np.int64)
    inside = (u >= 0) & (u < BINS)
    b[inside] = np.floor(u[inside]).astype(np.int64)
    b[u >= BINS] = BINS - 1
    return b


def occupancy(z_plane, lo=LO, scale=SCALE):
    return np.bincount(bins_of(z_plane, lo, scale).ravel(), minlength=BINS)


def exceedance_bound(z_plane, lo=LO, scale=SCALE):
    """The largest occupancy of a bin that holds neither bin 0's clamped elements nor exact zeros: ranks are exact between bins, so
    the count of matched elements at or above a threshold differs from the target's by less than the occupancy of the ONE bin the
    threshold's rank falls into."""
    h = occupancy(z_plane, lo, scale).copy()
    h[0] = 0
    h[bins_of(np.zeros(1, np.float32), lo, scale)[0]] = 0
    return int(h.max())


def exceedances(x, thresholds=THRESHOLDS_DB):
    x = np.asarray(x)
    return np.array([int((x >= np.float32(t)).sum()) for t in thresholds])


def exact_ranks(plane):
    flat = np.asarray(plane).ravel()
    return np.argsort(np.argsort(flat, kind="stable"), kind="stable")


def radar_db(size, seed=3):
    """fp32 [size, size]: the radar field of the spectra tests in dB, about 72 % exact zeros"""
    return R.db_field(1, size, size, seed)[0]


@functools.lru_cache(maxsize=None)
def member_case(name):
    """-> (z0 fp32 [1, S, S], z fp32 [1, 4, 2, S, S]): the dB field and its unmatched members, computed once, read-only."""
    from skillful_nowcasting_amd.stochastic import lifetime_rho, spectral_ar_reference

    window, size = MEMBER_CASES[name]
    z0 = radar_db(size)[None]
    white = R.white_field((1, 4, 2, size, size), seed=11)
    z = spectral_ar_reference(z0, white, lifetime_rho(window).numpy(), window)[0].astype(np.float32)
    for a in (z0, z):
        a.setflags(write=False)
    return z0, z


@functools.lru_cache(maxsize=None)
def half_dry_case(h=128, w=192, window=32):
    """The partly dry field (right half dry) -> (z0 [1, h, w], z [1, 2, 2, h, w]), read-only."""
    from skillful_nowcasting_amd.stochastic import lifetime_rho, spectral_ar_reference

    z0 = R.db_field(1, h, w, 3).copy()
    z0[:, :, w // 2:] = 0.0
    white = R.white_field((1, 2, 2, h, w), seed=12)
    z = spectral_ar_reference(z0, white, lifetime_rho(window).numpy(), window)[0].astype(np.float32)
    for a in (z0, z):
        a.setflags(write=False)
    return z0, z


def device_input(p, m, steps, h, w, seed=0):
    """-> (z fp32 [P, M, T, H, W], target fp32 [P, H, W]): Gaussian dB values (sd 12) around 4, a fifth of them exact zeros in runs
    and scattered, a few NaN, infinities and values beyond both ends of the range; the target a radar-like dB field."""
    rng = np.random.Generator(np.random.PCG64([seed, p, m, steps, h, w, 23]))
    z = (rng.standard_normal((p, m, steps, h, w)) * 12.0 + 4.0).astype(np.float32)
    z[rng.random(z.shape) < 0.1] = 0.0
    z[..., : h // 4, :] = 0.0  # a run of exact zeros: whole waves on one bin
    odd = rng.random(z.shape)
    z[odd < 0.002] = np.nan
    z[(odd >= 0.002) & (odd < 0.004)] = np.inf
    z[(odd >= 0.004) & (odd < 0.006)] = -np.inf
    z[(odd >= 0.006) & (odd < 0.008)] = 500.0
    z[(odd >= 0.008) & (odd < 0.010)] = -500.0
    z[(odd >= 0.010) & (odd < 0.012)] = 63.99
    target = R.db_field(p, h, w, seed=seed + 1)
    return z, target


def blob_mask(p, steps, h, w, seed=0):
    """uint8 [P, steps, H, W]: a disc per plane whose radius grows with the step, values 0 and (to test `nonzero`) 1 or 255"""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    out = np.zeros((p, steps, h, w), np.uint8)
    for i in range(p):
        for t in range(steps):
            inside = (y - h * 0.4) ** 2 + (x - w * (0.4 + 0.1 * i)) ** 2 <= (min(h, w) * (0.3 + 0.05 * t)) ** 2
            out[i, t][inside] = 255 if (i + t) % 2 else 1
    return out


@functools.lru_cache(maxsize=None)
def device_case(name, masked=0):
    """-> (z, target, mask or None, reference), computed once, read-only.  masked: 0 no mask, 1 one plane per case, 2 a plane per
    lead time."""
    from skillful_nowcasting_amd.stochastic import probability_match_reference

    p, m, steps, h, w = DEVICE_CASES[name]
    z, target = device_input(p, m, steps, h, w, seed=sorted(DEVICE_CASES).index(name))
    mask = None if not masked else blob_mask(p, 1 if masked == 1 else steps, h, w)
    ref = probability_match_reference(z, np.sort(target.reshape(p, -1), axis=1), mask)
    for a in (z, target, ref) + (() if mask is None else (mask,)):
        a.setflags(write=False)
    return z, target, mask, ref


def bits(a):
    """fp32 array or tensor -> int32 view: equality of bits, NaN and the sign of zero included"""
    if torch.is_tensor(a):
        return a.contiguous().view(torch.int32)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def wet_area(x, threshold):
    """share of elements at or above threshold"""
    x = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    return float((x >= threshold).double().mean())


def pooled_csi(forecast, observed, threshold):
    """forecast [M, ...], observed [...] -> hits / (hits + misses + false alarms) over all members and pixels (nan without events)"""
    forecast = forecast if torch.is_tensor(forecast) else torch.as_tensor(np.asarray(forecast))
    observed = (observed if torch.is_tensor(observed) else torch.as_tensor(np.asarray(observed))).to(forecast.device)
    f, o = forecast >= threshold, (observed >= threshold).expand_as(forecast)
    hits, misses, false = int((f & o).sum()), int((~f & o).sum()), int((f & ~o).sum())
    return hits / (hits + misses + false) if hits + misses + false else float("nan")
