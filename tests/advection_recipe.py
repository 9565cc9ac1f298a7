"""Inputs of the advection tests (numpy only): a seeded smooth rain field cut from a larger canvas, so that a shift by an integer
(dy, dx) is an exact re-cut - no interpolation, nothing shifted in from outside."""
import numpy as np

MARGIN = 48  # canvas border around the cut: shifts of up to this many pixels stay inside


def _box(a, width, axis):
    k = np.ones(width) / width
    return np.apply_along_axis(lambda r: np.convolve(r, k, mode="same"), axis, a)


def rain_canvas(seed, h, w):
    """float32 [h + 2 MARGIN, w + 2 MARGIN]: white noise, box-smoothed three times with width 9 along both axes, rescaled to unit
    standard deviation, then max(4 a - 1, 0) rounded to multiples of 1 / 32."""
    a = np.random.default_rng(seed).standard_normal((h + 2 * MARGIN, w + 2 * MARGIN))
    for _ in range(3):
        a = _box(_box(a, 9, 0), 9, 1)
    a = a / a.std()
    return (np.round(np.maximum(4.0 * a - 1.0, 0.0) * 32.0) / 32.0).astype(np.float32)


def cut(canvas, h, w, dy=0, dx=0):
    """The h x w field after the echo moved by (dy, dx): out[y][x] = field[y - dy][x - dx]."""
    return np.ascontiguousarray(canvas[MARGIN - dy:MARGIN - dy + h, MARGIN - dx:MARGIN - dx + w])


def rain_field(seed, h, w, dy=0, dx=0):
    return cut(rain_canvas(seed, h, w), h, w, dy, dx)


def translating_sequence(seed, h, w, frames, v):
    """[frames, h, w]: frame t is the field moved by t * v (integer v = (vy, vx))."""
    canvas = rain_canvas(seed, h, w)
    assert max(abs(v[0]), abs(v[1])) * (frames - 1) <= MARGIN
    return np.stack([cut(canvas, h, w, t * v[0], t * v[1]) for t in range(frames)])


def stripes(h, w, period=4):
    """Integer-valued (at most 15), periodic along x with the given period, varying along y: several displacements cost exactly 0."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    return (((x % period) * 3 + (y * 7) % 5 + (y // 3) % 3) % 16).astype(np.float32)


def qualifying(h, w, block, stride, radius, d):
    """bool [By, Bx]: blocks for which the displacement d and its four neighbours are candidates."""
    by, bx = (h - block) // stride + 1, (w - block) // stride + 1
    y0, x0 = np.arange(by) * stride, np.arange(bx) * stride
    ok = np.ones((by, bx), bool)
    for dy, dx in ((d[0], d[1]), (d[0] - 1, d[1]), (d[0] + 1, d[1]), (d[0], d[1] - 1), (d[0], d[1] + 1)):
        oy = (abs(dy) <= radius) & (y0 - dy >= 0) & (y0 - dy + block <= h)
        ox = (abs(dx) <= radius) & (x0 - dx >= 0) & (x0 - dx + block <= w)
        ok &= oy[:, None] & ox[None, :]
    return ok


# ---- the block-matching cases shared by the host and the GPU tests -----------------------------------------------------------------
# name -> (H, W, block, stride, radius, shift of plane 0, shift of plane 2, growth); plane 1 is all missing
MATCH_CASES = {
    "48x80 16/16/4": (48, 80, 16, 16, 4, (2, -1), (-3, 3), False),            # non-square, 3 x 5 lattice
    "96x128 32/16/8": (96, 128, 32, 16, 8, (3, -2), (-5, 7), False),          # overlapping blocks
    "96x128 32/32/16": (96, 128, 32, 32, 16, (11, -13), (-7, 9), False),      # 1089 displacements: more than one per thread
    "100x132 32/16/8": (100, 132, 32, 16, 8, (3, -2), (0, 6), False),         # a remainder no block covers
    "96x128 32/16/8 growth": (96, 128, 32, 16, 8, (3, -2), (-5, 7), True),    # next = shifted * (1 + 0.1 noise)
}
_MATCH_CACHE = {}


def match_eps(block):
    """2 (block^2 + 2) 2^-24: the forward bound of an fp32 sum of block^2 non-negative terms each rounded once, doubled."""
    return 2.0 * (block * block + 2) * 2.0 ** -24


def match_case(name):
    """-> (prev, nxt) float32 [3, H, W], read-only: two planted shifts with scattered NaN and negative elements in both frames and an
    all-missing plane between them."""
    if name not in _MATCH_CACHE:
        h, w, _block, _stride, _radius, d0, d2, growth = MATCH_CASES[name]
        rng = np.random.default_rng(sorted(MATCH_CASES).index(name) + 11)
        prev, nxt = np.empty((3, h, w), np.float32), np.empty((3, h, w), np.float32)
        for plane, seed, d in ((0, 5, d0), (2, 6, d2)):
            canvas = rain_canvas(seed, h, w)
            prev[plane], nxt[plane] = cut(canvas, h, w), cut(canvas, h, w, *d)
            if growth:
                nxt[plane] = nxt[plane] * (1.0 + 0.1 * rng.standard_normal((h, w))).astype(np.float32)
            for a in (prev[plane], nxt[plane]):
                a[rng.random((h, w)) < 0.003] = np.nan
                a[rng.random((h, w)) < 0.003] = -1.0
        prev[1], nxt[1] = np.nan, -3.0
        prev.setflags(write=False)
        nxt.setflags(write=False)
        _MATCH_CACHE[name] = (prev, nxt)
    return _MATCH_CACHE[name]


def clear_minimum(costs, eps):
    """bool [N, By, Bx]: the second-best cost exceeds the minimum by more than eps * min + eps."""
    flat = np.sort(costs.reshape(*costs.shape[:3], -1), axis=-1)
    return flat[..., 1] - flat[..., 0] > eps * flat[..., 0] + eps


_REFERENCE_CACHE = {}


def match_reference(name):
    """-> (costs float64 [3, By, Bx, 2R + 1, 2R + 1], BlockMatch) of the float64 specification, computed once per process."""
    if name not in _REFERENCE_CACHE:
        from skillful_nowcasting_amd import advection as A

        _h, _w, block, stride, radius = MATCH_CASES[name][:5]
        prev, nxt = match_case(name)
        costs = A.block_costs_reference(prev, nxt, block, stride, radius)
        _REFERENCE_CACHE[name] = (costs, A.block_match_reference(prev, nxt, block, stride, radius, 0.1, block * block // 16, costs=costs))
    return _REFERENCE_CACHE[name]
