"""Seeded cases and references shared by the fractions-skill-score tests (tests/test_fss_host.py, test_gpu_fss.py)."""
import functools

import numpy as np

from spectra_recipe import THRESHOLDS, THRESHOLDS8, make_ensemble

TILE = 64  # the tile of window centres csrc/fss.hip uses (FSS_TILE); LARGE and the seam positions below assume it
# one plane, the smallest multiple-of-16 shape with two whole tiles and a ragged one in both directions
LARGE = (1, 2 * TILE + 16, 3 * TILE + 16)
assert LARGE == (1, 144, 208)
SHAPES = [(2, 16, 16), (3, 32, 48), LARGE]
THRESHOLD_SETS = {1: (4.0,), 3: THRESHOLDS, 8: THRESHOLDS8}
RADII_SETS = {"r0": (0,), "default": (0, 2, 8, 32), "eight": (32, 0, 1, 2, 3, 5, 8, 16)}
MAX_RADIUS = 32


@functools.lru_cache(maxsize=None)
def case(m, shape):
    """The "radar" ensemble of spectra_recipe: 70 % zeros, values exactly on the thresholds 1, 4 and 8; scattered negatives / NaN / -inf,
    one missing 16 x 16 cell and (N > 1) one whole missing plane in the observation.  Read-only."""
    f, o = make_ensemble(m, *shape, "radar")
    for a in (f, o):
        a.setflags(write=False)
    return f, o


@functools.lru_cache(maxsize=None)
def _full_reference(m, shape):
    """The reference at all eight thresholds and all eight radii, once per case: every configured set is a subset of these."""
    from skillful_nowcasting_amd.fss import fss_sums_reference

    f, o = case(m, shape)
    sums, events = fss_sums_reference(f, o, THRESHOLDS8, RADII_SETS["eight"])
    for a in (sums, events):
        a.setflags(write=False)
    return sums, events


def reference(m, shape, k, radii_key):
    """-> (sums [N, K, S, 4], events [N, K, 2]) of `case(m, shape)` at THRESHOLD_SETS[k] and RADII_SETS[radii_key]."""
    sums, events = _full_reference(m, shape)
    ki = [THRESHOLDS8.index(t) for t in THRESHOLD_SETS[k]]
    si = [RADII_SETS["eight"].index(r) for r in RADII_SETS[radii_key]]
    return sums[:, ki][:, :, si], events[:, ki]


def brute_force(f, o, thresholds, radii):
    """The sums by a loop over planes, thresholds, radii and window centres; a window is the slice of the plane it overlaps."""
    m, n, h, w = f.shape
    sums = np.zeros((n, len(thresholds), len(radii), 4), np.int64)
    events = np.zeros((n, len(thresholds), 2), np.int64)
    for i in range(n):
        with np.errstate(invalid="ignore"):
            present = o[i] >= 0
        for k, t in enumerate(thresholds):
            with np.errstate(invalid="ignore"):
                im = [((f[j, i] >= np.float32(t)) & present).astype(np.int64) for j in range(m)]
                io = ((o[i] >= np.float32(t)) & present).astype(np.int64)
            events[i, k] = sum(int(a.sum()) for a in im), int(io.sum())
            for s, r in enumerate(radii):
                ff = oo = fo = mm = 0
                for y in range(h):
                    for x in range(w):
                        win = (slice(max(0, y - r), y + r + 1), slice(max(0, x - r), x + r + 1))
                        sm = [int(a[win].sum()) for a in im]
                        so, sf = int(io[win].sum()), sum(sm)
                        ff, oo, fo, mm = ff + sf * sf, oo + so * so, fo + sf * so, mm + sum(v * v for v in sm)
                sums[i, k, s] = ff, oo, fo, mm
    return sums, events


def seam_positions(shape=LARGE, tile=TILE, reach=MAX_RADIUS):
    """Pixel positions (y, x) of a plane: its four corners, the crossings of the rows and the columns next to every tile seam, and a
    pixel at every distance from a seam out to which the largest radius reaches (reach and reach + 1 on the low side, reach - 1 and
    reach on the high side: the last position whose window crosses the seam and the first whose window does not), each against
    coordinates that lie next to a seam of the other direction."""
    _, h, w = shape

    def near(size):
        seams = range(tile, size, tile)
        close = sorted({s + d for s in seams for d in (-1, 0)})
        far = sorted({s + d for s in seams for d in (-reach - 1, -reach, reach - 1, reach) if 0 <= s + d < size})
        return close, far

    ys_close, ys_far = near(h)
    xs_close, xs_far = near(w)
    pos = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
    pos += [(y, x) for y in ys_close for x in xs_close]
    pos += [(y, xs_close[i % len(xs_close)]) for i, y in enumerate(ys_far)]
    pos += [(ys_close[i % len(ys_close)], x) for i, x in enumerate(xs_far)]
    pos += [(y, xs_far[i % len(xs_far)]) for i, y in enumerate(ys_far)]
    return pos
