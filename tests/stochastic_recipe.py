"""Inputs, the fp32 CPU implementation and the accuracy criterion shared by the stochastic-ensemble tests
(tests/test_stochastic_host.py, tests/test_gpu_stochastic.py)."""
import functools

import numpy as np
import torch

import spectra_recipe as SR

# name -> (window, H, W, P, M, T)
AR_CASES = {
    "L32 64x96": (32, 64, 96, 2, 2, 3),      # every class, two or more windows in each except along cy
    "L64 128x64": (64, 128, 64, 1, 2, 2),    # no class with cx = 1
    "L128 128x256": (128, 128, 256, 1, 2, 2),  # no class with cy = 1; the LDS limit
}
# The accuracy factor K of the criterion below: the smallest power of two for which the fp32 CPU implementation (`spectral_ar_fp32`:
# the same recursion with torch.fft in complex64) stays within HALF the bound on every case of AR_CASES - its worst ratios against
# eps(L) * majorant are 6.5e-3 (L32), 5.6e-3 (L64), 5.0e-3 (L128), so with 1/64 it stays below one half of the bound and with 1/128
# it does not (tests/test_stochastic_host.py::test_accuracy_factor_is_the_smallest_power_of_two asserts exactly that).  eps(L) is a
# worst-case bound of one transform; the errors of real data add like a random walk, hence a factor well below one.
K = 1.0 / 64.0


def eps(window):
    """16 * 2 log2(L) * 2^-24, as in spectra_recipe.psd_bound."""
    return 16.0 * 2.0 * np.log2(window) * 2.0 ** -24


def case_rho(window):
    """fp32 [L]: rho[0] = 1, then 0.97^r - every value between 1 and nearly 0 occurs (no library default enters a test)."""
    rho = 0.97 ** np.arange(window, dtype=np.float64)
    rho[0] = 1.0
    return rho.astype(np.float32)


def db_field(n, h, w, seed=0):
    """The radar-like fields of spectra_recipe.make_field in dB (to_db with its defaults): fp32 [n, h, w], about 70 % zeros."""
    from skillful_nowcasting_amd.stochastic import to_db

    return to_db(torch.from_numpy(SR.make_field(n, h, w, "radar", seed))).numpy()


def white_field(shape, seed=0):
    return np.random.Generator(np.random.PCG64([seed, 41])).standard_normal(shape).astype(np.float32)


@functools.lru_cache(maxsize=None)
def ar_case(name):
    """-> (z0 [P, H, W], white [P, M, T, H, W], rho [L], reference out float64, cell majorant), computed once, read-only."""
    from skillful_nowcasting_amd.stochastic import spectral_ar_reference

    window, h, w, p, m, steps = AR_CASES[name]
    z0 = db_field(p, h, w, seed=sorted(AR_CASES).index(name))
    white = white_field((p, m, steps, h, w), seed=sorted(AR_CASES).index(name))
    rho = case_rho(window)
    ref, maj = spectral_ar_reference(z0, white, rho, window)
    cells = cell_majorant(maj, h, w, window)
    for a in (z0, white, rho, ref, cells):
        a.setflags(write=False)
    return z0, white, rho, ref, cells


def cell_majorant(maj, h, w, window):
    """The reference's per-window majorants (one array per class, [P, M, T, wins_y, wins_x]) -> float64 [P, M, T, 2 H / L, 2 W / L]: per
    L/2 x L/2 cell of the output, the sum over the at most four windows that cover it."""
    ny, nx = 2 * h // window, 2 * w // window
    out = np.zeros(maj[0].shape[:3] + (ny, nx))
    for c, mj in enumerate(maj):
        cy, cx = c >> 1, c & 1
        for i in range(mj.shape[3]):
            for j in range(mj.shape[4]):
                out[..., 2 * i + cy:2 * i + cy + 2, 2 * j + cx:2 * j + cx + 2] += mj[..., i, j, None, None]
    return out


def cell_ratio(got, ref, cells, window):
    """max over the L/2 x L/2 cells of ||got - ref||_2 / (eps(L) * cell majorant): the criterion is ratio <= K."""
    half = window // 2
    d = np.asarray(got, dtype=np.float64) - ref
    lead, (h, w) = d.shape[:-2], d.shape[-2:]
    d = d.reshape(lead + (h // half, half, w // half, half))
    norm = np.sqrt((d * d).sum(axis=(-3, -1)))
    assert (cells > 0).all()
    return float((norm / (eps(window) * cells)).max())


def spectral_ar_fp32(z0, white, rho, window):
    """The recursion of spectral_ar_reference in fp32 on the CPU, independent of the kernel: torch.fft in complex64, fp32 weights."""
    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import axis_weights

    z0, white = torch.from_numpy(np.array(z0)), torch.from_numpy(np.array(white))
    p, m, steps, h, w = white.shape
    rk = torch.from_numpy(np.asarray(rho, np.float32)[_radial_bins(window)])
    gain = torch.from_numpy(np.sqrt(1.0 - np.asarray(rho, np.float64)[_radial_bins(window)] ** 2).astype(np.float32))
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
            amp = gain * (u.abs() / window)
            wh = torch.fft.fft2(windows(white, ny, nx, ys, xs))
            state = u.expand(p, m, ny, nx, window, window).clone()
            for t in range(steps):
                state = rk * state + amp * wh[:, :, t]
                x = torch.fft.ifft2(state).real.movedim(-2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * (wy[:, None] * wx[None, :])
    assert out.dtype == torch.float32
    return out.numpy()


def checkerboards(h, w, constant=3.0):
    """fp32 [4, h, w]: (-1)^x, (-1)^y, a constant, and the sum of the three."""
    y, x = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cx, cy = 1.0 - 2.0 * (x % 2), 1.0 - 2.0 * (y % 2)
    return np.stack([cx, cy, np.full((h, w), constant), cx + cy + constant]).astype(np.float32)


def translating_db_context(seed=5, size=128, frames=5, v=(2, -3)):
    """[frames, size, size] rain rates of a translating field (advection_recipe), the last one the observation after the context."""
    import advection_recipe as AR

    return AR.translating_sequence(seed, size, size, frames, v)
