"""Seeded inputs and the comparison rule shared by tests/test_verification_host.py and tests/test_gpu_verification.py."""
import functools

import numpy as np

SCALES = (1, 4, 16)
THRESHOLDS = (1.0, 4.0, 8.0)


def make_case(m, n, h, w, kind, seed=0, missing=True):
    """-> (forecast fp32 [m, n, h, w], observed fp32 [n, h, w]).

    kind "continuous": gamma-distributed rain rates, no ties.  kind "radar": multiples of 1/32, about 70 % zeros - ties dominate and
    values sit exactly on the thresholds 1, 4 and 8.  missing: scattered negatives, NaN and -inf in the observation (0.1 % each:
    about half of the 16 x 16 cells stay whole), one whole 16 x 16 cell of plane 0 and, with more than one plane, the whole last
    plane."""
    rng = np.random.Generator(np.random.PCG64([seed, m, n, h, w, 0 if kind == "continuous" else 1]))
    field = rng.gamma(0.6, 4.0, size=(m + 1, n, h, w))
    if kind == "radar":
        field = np.round(field * 32.0) / 32.0
        field[rng.random(field.shape) < 0.7] = 0.0
        on_thr = rng.random(field.shape) < 0.02
        field[on_thr] = rng.choice(np.array(THRESHOLDS), size=int(on_thr.sum()))
    field = field.astype(np.float32)
    forecast, observed = np.ascontiguousarray(field[:m]), np.ascontiguousarray(field[m])
    if missing:
        u = rng.random(observed.shape)
        observed[u < 0.001] = -1.0
        observed[(u >= 0.001) & (u < 0.002)] = np.nan
        observed[(u >= 0.002) & (u < 0.003)] = -np.inf
        cy, cx = (h // 16) // 2, (w // 16) // 2
        observed[0, cy * 16:cy * 16 + 16, cx * 16:cx * 16 + 16] = np.nan
        if n > 1:
            observed[-1] = -32.0
    return forecast, observed


@functools.lru_cache(maxsize=None)
def case_with_reference(m, n, h, w, kind, scales=SCALES, thresholds=THRESHOLDS):
    """The seeded case and `ensemble_scores_reference` on it, computed once per process and shared (read-only) between tests."""
    from skillful_nowcasting_amd.verification import ensemble_scores_reference

    forecast, observed = make_case(m, n, h, w, kind)
    ref = ensemble_scores_reference(forecast, observed, scales, thresholds)
    for a in (forecast, observed) + tuple(ref):
        a.setflags(write=False)
    return forecast, observed, ref


def check_against_reference(got, ref, m, scales, label=""):
    """`got`, `ref`: EnsembleScores of numpy arrays.  Counts are equal exactly; the two float64 sums obey |got - ref| <= gamma * ref,
    gamma = (n_cells + M^2 + s^2) * 2^-53 - the a-priori bound for any order of that many float64 additions of non-negative terms
    (n_cells: the cells of that plane and scale).  Prints the largest measured gap / bound ratio before it asserts."""
    assert np.array_equal(got.cells, ref.cells), f"{label}: cells differ"
    assert np.array_equal(got.contingency, ref.contingency), f"{label}: contingency differs"
    assert np.array_equal(got.ranks, ref.ranks), f"{label}: ranks differ"
    s2 = np.asarray([s * s for s in scales], dtype=np.float64)
    gamma = (ref.cells.astype(np.float64) + m * m + s2[None, :]) * 2.0 ** -53  # [N, S]
    worst = {}
    for name in ("abs_err", "pair"):
        g, r = getattr(got, name), getattr(ref, name)
        gap, bound = np.abs(g - r), gamma[:, None, :] * r
        rel = np.where(r > 0, gap / np.where(r > 0, r, 1.0), gap)
        worst[name] = (float(rel.max()), float(gamma.max()))
        print(f"{label} {name}: largest |device - reference| / reference {rel.max():.3e} (largest gamma {gamma.max():.3e})")
        assert (gap <= bound).all(), f"{label}: {name} beyond gamma * reference: gap {gap.max():.3e}, at {np.argwhere(gap > bound)[:4].tolist()}"
    if 1 in scales:
        si = scales.index(1)
        assert np.array_equal(got.abs_err[:, 0, si], got.abs_err[:, 1, si]) and np.array_equal(got.pair[:, 0, si], got.pair[:, 1, si])
    return worst
