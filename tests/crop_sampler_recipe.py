"""The seeded full-frame rows shared by test_crop_sampler_host.py and test_gpu_crop_sampler.py (no test in here).

One rain field on a 40 x 56 frame, six frames long: a gamma-distributed intensity under a Gaussian envelope centred at (y=10, x=44),
dry outside it, so that the 4 x 6 candidate crops (crop 16, stride 8) run from wholly dry to soaked; "no data" holes at 1 % of the
pixels plus the block [:, 28:40, 0:12], so that missing counts run from a handful to more than half a crop.  The same field in the
four storage encodings the loaders stage, each with its own affine and its own way to say "missing"."""
import numpy as np

T, H, W, C = 6, 40, 56, 1
N_IN, N_OUT = 2, 4
CELL, CROP = 8, 16
GY, GX = (H - CROP) // CELL + 1, (W - CROP) // CELL + 1
N_ELEMENTS = T * C * CROP * CROP  # 1536
Q_MIN, M = 0.05, 4.0
DTYPES = ("int16", "uint8", "float16", "float32")


def field(seed=7, t=T, h=H, w=W, c=C, centre=(10, 44), widths=(9.0, 11.0)):
    """-> (v float64 [t, h, w, c] >= 0, holes bool [t, h, w, c]), drawn in this order from one generator."""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    env = np.exp(-0.5 * (((yy - centre[0]) / widths[0]) ** 2 + ((xx - centre[1]) / widths[1]) ** 2))[None, :, :, None]
    v = rng.gamma(0.5, 60.0, (t, h, w, c)) * (rng.random((t, h, w, c)) < 0.6) * env
    v = np.where(env < 0.02, 0.0, v)
    holes = rng.random((t, h, w, c)) < 0.01
    holes[:, 28:40, 0:12] = True
    return v, holes


def encode(v, holes, dtype):
    """-> (raw array in the storage dtype, scale, offset)"""
    if dtype == "int16":
        return np.where(holes, -1, np.minimum(v, 4000)).astype(np.int16), 1.0 / 32.0, 0.0
    if dtype == "uint8":
        return np.where(holes, 0, np.minimum(v, 253) + 1).astype(np.uint8), 0.5, -0.5
    if dtype == "float16":
        return np.where(holes, np.nan, v / 32.0).astype(np.float16), 1.0, 0.0
    if dtype == "float32":
        return np.where(holes, -np.inf, v / 32.0).astype(np.float32), 1.0, 0.0
    raise KeyError(dtype)


def recipe(dtype, seed=7, **shape):
    return encode(*field(seed, **shape), dtype)


def brute_force(raw, scale, offset, sat_scale, cell, crop):
    """The definition, one element at a time: -> (scores [Gy][Gx] float, missing [Gy][Gx] int) as nested lists."""
    import math

    t, h, w, c = raw.shape
    x = (raw.astype(np.float32) * np.float32(scale) + np.float32(offset)).tolist()
    gy_n, gx_n = (h - crop) // cell + 1, (w - crop) // cell + 1
    scores = [[0.0] * gx_n for _ in range(gy_n)]
    missing = [[0] * gx_n for _ in range(gy_n)]
    for gy in range(gy_n):
        for gx in range(gx_n):
            s, n = 0.0, 0
            for ti in range(t):
                for i in range(gy * cell, gy * cell + crop):
                    for j in range(gx * cell, gx * cell + crop):
                        for e in x[ti][i][j]:
                            if not e >= 0.0:
                                n += 1
                            else:
                                s += -math.expm1(-e / sat_scale)
            scores[gy][gx], missing[gy][gx] = s, n
    return scores, missing


# ---- the loader on these rows (shared by the host and the GPU file) --------------------------------------------------------------
def make_rows(dtype, n=3, frames=T + 1):
    """n full-frame rows one frame longer than the loader needs (it takes the last 2 + 4), with their affine."""
    rows = []
    for k in range(n):
        raw, scale, offset = recipe(dtype, seed=7 + k, t=frames)
        rows.append(raw)
    return rows, scale, offset


def loader(rows, scale, offset, **kw):
    from skillful_nowcasting_amd.data import ImportanceCropLoader

    args = dict(batch_size=3, crop=CROP, stride=CELL, q_min=Q_MIN, m=M, scale=scale, offset=offset, num_input_frames=N_IN,
                num_target_frames=N_OUT)
    args.update(kw)
    return ImportanceCropLoader(rows, **args)


def reference_selection(rows, scale, offset, seed=0, q_min=Q_MIN, m=M, max_missing=1.0, max_crops_per_row=None):
    """The loader's draw, restated: -> (origins [K, 3] (row, y, x), q [K], margin = min |u - q| over every candidate of every row)."""
    from skillful_nowcasting_amd.data import crop_scores_reference, inclusion_probability

    rng = np.random.Generator(np.random.PCG64(seed))
    origins, qs, margin = [], [], np.inf
    for index, row in enumerate(rows):
        s, miss = crop_scores_reference(row[-T:], scale, offset, 1.0, CELL, CROP)
        q = inclusion_probability(s, N_ELEMENTS, q_min, m).reshape(-1)
        u = rng.random(q.size)
        margin = min(margin, np.abs(u - q).min())
        keep = np.flatnonzero((u < q) & (miss.reshape(-1) <= max_missing * N_ELEMENTS))
        keep = keep[rng.permutation(keep.size)][:max_crops_per_row]
        for g in keep:
            origins.append((index, g // GX * CELL, g % GX * CELL))
            qs.append(q[g])
    return np.array(origins, np.int64).reshape(-1, 3), np.array(qs, np.float64), margin


def collect(ld):
    """Every batch of one iteration with the attributes the loader exposes after it: [(images, future, origins, q)]."""
    batches = []
    for images, future in ld:
        batches.append((images.clone(), future.clone(), ld.last_origins.copy(), ld.last_inclusion_prob.copy()))
    return batches
