"""Seeded inputs and the comparison rules shared by the spectra / value tests (tests/test_spectra_host.py, test_value_host.py,
test_gpu_spectra.py, test_gpu_value.py)."""
import functools

import numpy as np

THRESHOLDS = (1.0, 4.0, 8.0)
THRESHOLDS8 = (0.03125, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 64.0)


def make_field(n, h, w, kind="radar", seed=0):
    """-> fp32 [n, h, w] rain rates, nothing missing.  kind "continuous": gamma-distributed; kind "radar": multiples of 1/32, about
    70 % zeros, 2 % of the values exactly on the thresholds 1, 4 and 8."""
    rng = np.random.Generator(np.random.PCG64([seed, n, h, w, 0 if kind == "continuous" else 1, 77]))
    field = rng.gamma(0.6, 4.0, size=(n, h, w))
    if kind == "radar":
        field = np.round(field * 32.0) / 32.0
        field[rng.random(field.shape) < 0.7] = 0.0
        on_thr = rng.random(field.shape) < 0.02
        field[on_thr] = rng.choice(np.array(THRESHOLDS), size=int(on_thr.sum()))
    return np.ascontiguousarray(field.astype(np.float32))


def punch_holes(field, window, seed=0):
    """Scattered -1, NaN and -inf (0.1 % each) and, with more than one window, one whole missing window (the last of plane 0), in place."""
    rng = np.random.Generator(np.random.PCG64([seed, 5]))
    u = rng.random(field.shape)
    field[u < 0.001] = -1.0
    field[(u >= 0.001) & (u < 0.002)] = np.nan
    field[(u >= 0.002) & (u < 0.003)] = -np.inf
    h, w = field.shape[-2:]
    if field.shape[0] * (h // window) * (w // window) > 1:
        field[0, h - window:, w - window:] = -32.0
    return field


def make_ensemble(m, n, h, w, kind="radar", seed=0, missing=True):
    """-> (forecast fp32 [m, n, h, w], observed fp32 [n, h, w]); with `missing` the observation has scattered holes, one missing
    16 x 16 cell in plane 0 and, with more than one plane, a whole missing last plane."""
    field = make_field((m + 1) * n, h, w, kind, seed).reshape(m + 1, n, h, w)
    forecast, observed = np.ascontiguousarray(field[:m]), np.ascontiguousarray(field[m])
    if missing:
        if h * w > 256:
            punch_holes(observed, 16, seed)
        else:  # (a single cell per plane: scattered holes only)
            observed[0, 1, 2], observed[0, 5, 5], observed[0, 9, 14] = -1.0, np.nan, -np.inf
        if n > 1:
            observed[-1] = -32.0
    return forecast, observed


def windows_of(x, window):
    """[..., H, W] -> [..., H / L, W / L, L, L]"""
    h, w = x.shape[-2:]
    t = x.reshape(x.shape[:-2] + (h // window, window, w // window, window))
    return np.moveaxis(t, -3, -2)


def psd_bound(x, window):
    """The allowed |sqrt(got_r) - sqrt(ref_r)| per window, [..., H / L, W / L]: eps(L) * L * sqrt(sum x^2) over the zero-filled window,
    eps(L) = 16 * 2 log2(L) * 2^-24 - the norm-wise forward error of a radix-2 fp32 FFT of L^2 points with correctly rounded twiddles
    (Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2: log2(L^2) * eta, eta ~ 7 u), with about a factor two of room
    for the fp32 |F|^2 and other radices.  (|F| is bounded by the 2-norm of the spectrum, L * ||x||_2; a bin's sqrt(power) is the
    2-norm of its modes, so the norm-wise error bounds its change.)"""
    t = windows_of(np.asarray(x, dtype=np.float32), window).astype(np.float64)
    with np.errstate(invalid="ignore"):
        t = np.where(t >= 0, t, 0.0)
    eps = 16.0 * 2.0 * np.log2(window) * 2.0 ** -24
    return eps * window * np.sqrt((t * t).sum(axis=(-2, -1)))


def check_psd(got, ref, x, window, label=""):
    """got, ref: power [..., H / L, W / L, L / 2].  Prints the worst gap / bound ratio before it asserts; returns it."""
    bound = psd_bound(x, window)[..., None]
    gap = np.abs(np.sqrt(got) - np.sqrt(ref))
    ratio = float(np.max(gap / np.where(bound > 0, bound, 1.0)))
    print(f"{label} L={window}: largest |sqrt(device) - sqrt(reference)| / bound {ratio:.3e}")
    assert np.isfinite(got).all() and (got >= 0).all(), f"{label}: negative or non-finite power"
    assert (gap <= bound).all(), f"{label}: beyond the bound at {np.argwhere(gap > bound)[:4].tolist()}, ratio {ratio:.3e}"
    return ratio


@functools.lru_cache(maxsize=None)
def field_with_reference(n, h, w, window, kind="radar", seed=0):
    """The seeded field and `radial_psd_reference` on it, computed once per process and shared (read-only) between tests."""
    from skillful_nowcasting_amd.spectra import radial_psd_reference

    x = make_field(n, h, w, kind, seed)
    power, missing = radial_psd_reference(x, window)
    for a in (x, power, missing):
        a.setflags(write=False)
    return x, power, missing


def impulse(window, a=3.0, at=(5, 9)):
    x = np.zeros((1, window, window), np.float32)
    x[0, at[0], at[1]] = a
    return x


def plane_wave(window, a=2.0):
    """A (1 + cos(2 pi (3 i + 4 j) / L)): (A L^2)^2 in bin 0 and 2 (A L^2 / 2)^2 in bin 5 (modes (3, 4) and (-3, -4))."""
    i, j = np.meshgrid(np.arange(window), np.arange(window), indexing="ij")
    return (a * (1.0 + np.cos(2.0 * np.pi * (3 * i + 4 * j) / window))).astype(np.float32)[None]
