"""Inputs, the fp32 CPU implementation and the accuracy factor shared by the tests of the AR(2) recursion
(tests/test_spectral_ar2_host.py, tests/test_gpu_spectral_ar2.py).  The criterion is stochastic_recipe's: per L/2 x L/2 cell the
2-norm of the error against eps(L) times the summed majorants of the windows over the cell (cell_majorant, cell_ratio)."""
import functools

import numpy as np
import torch

import stochastic_recipe as R

# name -> (window, H, W, P, M, T)
AR2_CASES = {
    "L32 64x96": (32, 64, 96, 2, 2, 4),        # every class; coefficients per plane; T = 4: both registers have rotated twice
    "L64 128x64": (64, 128, 64, 1, 2, 3),      # no class with cx = 1
    "L128 128x256": (128, 128, 256, 1, 2, 3),  # no class with cy = 1; the LDS and register limit
}
# The accuracy factor K2 of  cell_ratio <= K2: the smallest power of two for which the fp32 CPU implementation (`spectral_ar2_fp32`:
# the same recursion with torch.fft in complex64) stays within HALF the bound on every case of AR2_CASES - its worst ratios against
# eps(L) * majorant are 6.8e-3 (L32), 5.5e-3 (L64), 5.8e-3 (L128), so with 1/64 it stays below one half of the bound and with 1/128 it
# does not (tests/test_spectral_ar2_host.py::test_accuracy_factor_is_the_smallest_power_of_two asserts exactly that).
K2 = 1.0 / 64.0


def case_rhos(window, plane=0):
    """(rho1, rho2) fp32 [L] each.  Plane 0: rho1 = 0.97^r with rho1[0] = 1 (the bin is kept); rho2 = 0.9^r except rho2[1] = -1, which
    clips to phi2 = -1, and rho2[2] = 1, which clips to phi2 = +1.  Any other plane: 0.95^r (rho1[0] = 1) and 0.93^r, no clip."""
    r = np.arange(window, dtype=np.float64)
    if plane == 0:
        rho1, rho2 = 0.97 ** r, 0.9 ** r
        rho2[1], rho2[2] = -1.0, 1.0
    else:
        rho1, rho2 = 0.95 ** r, 0.93 ** r
    rho1[0] = 1.0
    return rho1.astype(np.float32), rho2.astype(np.float32)


def case_coef(window, planes):
    """fp32 [3, L] for one plane, [P, 3, L] for more: ar2_coefficients of case_rhos"""
    from skillful_nowcasting_amd.stochastic import ar2_coefficients

    rows = [ar2_coefficients(*(torch.from_numpy(v) for v in case_rhos(window, i))).numpy() for i in range(planes)]
    return rows[0] if planes == 1 else np.stack(rows)


@functools.lru_cache(maxsize=None)
def ar2_case(name):
    """-> (z0, zm1 [P, H, W], white [P, M, T, H, W], coef, reference out float64, cell majorant), computed once, read-only."""
    from skillful_nowcasting_amd.stochastic import spectral_ar2_reference

    window, h, w, p, m, steps = AR2_CASES[name]
    idx = sorted(AR2_CASES).index(name)
    z0, zm1 = R.db_field(p, h, w, seed=idx), R.db_field(p, h, w, seed=idx + 20)
    white = R.white_field((p, m, steps, h, w), seed=idx)
    coef = case_coef(window, p)
    ref, maj = spectral_ar2_reference(z0, zm1, white, coef, window)
    cells = R.cell_majorant(maj, h, w, window)
    for a in (z0, zm1, white, coef, ref, cells):
        a.setflags(write=False)
    return z0, zm1, white, coef, ref, cells


def ar1_as_ar2(rho):
    """fp32 [3, L] = (rho, 0, fp32(sqrt(1 - rho^2))): the AR(1) of rho written as an AR(2)"""
    rho = np.asarray(rho, np.float32)
    return np.stack([rho, np.zeros_like(rho), np.sqrt(np.maximum(1.0 - rho.astype(np.float64) ** 2, 0.0)).astype(np.float32)])


def spectral_ar2_fp32(z0, zm1, white, coef, window):
    """The recursion of spectral_ar2_reference in fp32 on the CPU, independent of the kernel: torch.fft in complex64, fp32 weights."""
    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import axis_weights

    z0, zm1, white = (torch.from_numpy(np.array(v)) for v in (z0, zm1, white))
    p, m, steps, h, w = white.shape
    ck = torch.from_numpy(np.broadcast_to(np.asarray(coef, np.float32), (p, 3, window))[:, :, _radial_bins(window)].copy())
    phi1, phi2, gain = (ck[:, i, None, None, None] for i in range(3))  # [P, 1, 1, 1, L, L]
    (ay, hy), (ax, hx) = axis_weights(h, window), axis_weights(w, window)
    out = torch.zeros((p, m, steps, h, w), dtype=torch.float32)
    half = window // 2

    def windows(x, ny, nx, ys, xs):
        t = x[..., ys, xs]
        return t.reshape(x.shape[:-2] + (ny, window, nx, window)).movedim(-3, -2)

    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)
            wy = torch.from_numpy((hy if cy else ay)[ys])
            wx = torch.from_numpy((hx if cx else ax)[xs])
            u = torch.fft.fft2(windows(z0, ny, nx, ys, xs))[:, None]
            um = torch.fft.fft2(windows(zm1, ny, nx, ys, xs))[:, None]
            amp = gain * (u.abs() / window)
            wh = torch.fft.fft2(windows(white, ny, nx, ys, xs))
            x1 = u.expand(p, m, ny, nx, window, window).clone()
            x2 = um.expand(p, m, ny, nx, window, window).clone()
            assert x1.dtype == torch.complex64 and amp.dtype == torch.float32
            for t in range(steps):
                x1, x2 = (phi1 * x1 + phi2 * x2) + amp * wh[:, :, t], x1
                x = torch.fft.ifft2(x1).real.movedim(-2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * (wy[:, None] * wx[None, :])
    assert out.dtype == torch.float32
    return out.numpy()
