"""Inputs, the fp32 CPU implementation and the accuracy criterion shared by the tests of the rho(r) estimate
(tests/test_lag_estimate_host.py, tests/test_gpu_lag_estimate.py)."""
import functools

import numpy as np
import torch

import stochastic_recipe as R

# name -> (window, H, W, N): the smallest shapes with every class / without a cx = 1 class / without a cy = 1 class at the LDS limit
LAG_CASES = {
    "L32 64x96": (32, 64, 96, 3),
    "L64 128x64": (64, 128, 64, 2),
    "L128 128x256": (128, 128, 256, 1),
}
# The accuracy factor K of the criterion  |got - ref| <= K * 2 eps(L) * L^2 * n_q  per window, q and bin r, with n_q = ||a||^2, ||b||^2,
# ||a|| ||b|| over the patch (Parseval: the whole spectrum's sum is L^2 n_q; a relative error eps(L) of a transform is 2 eps(L) in a
# product of two) and eps(L) of stochastic_recipe.  K is the smallest power of two for which the fp32 CPU implementation
# (`lag_spectra_fp32`: torch.fft in complex64, float64 sums) stays within HALF the bound on every case of LAG_CASES - its worst ratios
# against 2 eps(L) L^2 n_q are 3.61e-3 (L32), 1.57e-3 (L64), 1.46e-3 (L128), so with 1/128 it stays below one half of the bound and
# with 1/256 it does not (tests/test_lag_estimate_host.py::test_accuracy_factor_is_the_smallest_power_of_two asserts exactly that).
# eps(L) is a worst-case bound of one transform; the errors of real data add like a random walk, hence a factor well below one.
K = 1.0 / 128.0


def window_norms(a, b, window):
    """float64 [N, Wn, 3]: ||a||^2, ||b||^2, ||a|| ||b|| over each patch of `window_table`'s order"""
    from skillful_nowcasting_amd.stochastic import window_table

    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    out = []
    for _cy, _cx, y0, x0 in window_table(a.shape[1], a.shape[2], window):
        na = (a[:, y0:y0 + window, x0:x0 + window] ** 2).sum(axis=(1, 2))
        nb = (b[:, y0:y0 + window, x0:x0 + window] ** 2).sum(axis=(1, 2))
        out.append(np.stack([na, nb, np.sqrt(na * nb)], axis=-1))
    return np.stack(out, axis=1)


def lag_ratio(got, ref, norms, window):
    """max over windows, q and r of |got - ref| / (2 eps(L) L^2 n_q): the criterion is ratio <= K.  Where n_q = 0 (an all-zero patch)
    the sums must be exact zeros."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    unit = 2.0 * R.eps(window) * window * window * norms[..., None]  # [N, Wn, 3, 1]
    dry = np.broadcast_to(unit == 0, got.shape)
    assert (got[dry] == 0).all() and (ref[dry] == 0).all()
    return float((np.abs(got - ref) / np.where(unit == 0, 1.0, unit)).max())


def lag_inputs(window, h, w, n, seed):
    """a: radar-like dB planes; b = 0.8 a + 0.6 (another such field), fp32; the first aligned window of plane 0 is zero in both."""
    a = R.db_field(n, h, w, seed=seed).copy()
    b = (np.float32(0.8) * a + np.float32(0.6) * R.db_field(n, h, w, seed=seed + 10)).astype(np.float32)
    a[0, :window, :window] = 0
    b[0, :window, :window] = 0
    return a, b


@functools.lru_cache(maxsize=None)
def lag_case(name):
    """-> (a, b [N, H, W] fp32, reference float64 [N, Wn, 3, L], norms [N, Wn, 3]), computed once, read-only."""
    from skillful_nowcasting_amd.stochastic import lag_spectra_reference

    window, h, w, n = LAG_CASES[name]
    a, b = lag_inputs(window, h, w, n, seed=20 + sorted(LAG_CASES).index(name))
    ref = lag_spectra_reference(a, b, window)
    norms = window_norms(a, b, window)
    for x in (a, b, ref, norms):
        x.setflags(write=False)
    return a, b, ref, norms


def lag_spectra_fp32(a, b, window):
    """The sums of lag_spectra_reference from fp32 transforms on the CPU, independent of the kernel: torch.fft in complex64, the
    three terms in fp32, float64 sums."""
    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import window_table

    a, b = torch.from_numpy(np.array(a, np.float32)), torch.from_numpy(np.array(b, np.float32))
    bins = _radial_bins(window).reshape(-1)
    out = []
    for _cy, _cx, y0, x0 in window_table(a.shape[1], a.shape[2], window):
        fa = torch.fft.fft2(a[:, y0:y0 + window, x0:x0 + window])
        fb = torch.fft.fft2(b[:, y0:y0 + window, x0:x0 + window])
        assert fa.dtype == torch.complex64
        terms = torch.stack([fa.real * fa.real + fa.imag * fa.imag, fb.real * fb.real + fb.imag * fb.imag,
                             fa.real * fb.real + fa.imag * fb.imag], dim=1).reshape(a.shape[0], 3, -1).numpy().astype(np.float64)
        out.append(np.stack([[np.bincount(bins, weights=terms[i, q], minlength=window) for q in range(3)] for i in range(a.shape[0])]))
    return np.stack(out, axis=1)


def direct_lag_spectra(a, b, window):
    """lag_spectra_reference's definition, window by window with np.fft.fft2 and np.bincount over spectra._radial_bins."""
    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import window_table

    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    bins = _radial_bins(window).reshape(-1)
    table = window_table(a.shape[1], a.shape[2], window)
    out = np.zeros((a.shape[0], len(table), 3, window))
    for i in range(a.shape[0]):
        for k, (_cy, _cx, y0, x0) in enumerate(table):
            fa = np.fft.fft2(a[i, y0:y0 + window, x0:x0 + window]).reshape(-1)
            fb = np.fft.fft2(b[i, y0:y0 + window, x0:x0 + window]).reshape(-1)
            for q, t in enumerate((np.abs(fa) ** 2, np.abs(fb) ** 2, (fa * np.conj(fb)).real)):
                out[i, k, q] = np.bincount(bins, weights=t, minlength=window)
    return out
