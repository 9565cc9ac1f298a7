"""A stochastic advection ensemble: the core of STEPS in one form (INTEGRATION.md "A probabilistic baseline").

  * the last observed frame in dB (`to_db`), cut into overlapping L x L windows;
  * per window and member an AR(1) process per Fourier mode, `X_t = rho X_(t-1) + sqrt(1 - rho^2) A Wh_t`, whose lag-1 correlation
    `rho` depends on the mode's radial wavenumber (`lifetime_rho`: small scales forget faster - a cascade with as many levels as radial
    bins) and whose noise is shaped by the window's own amplitude spectrum `A = |fft2(window)| / L` (the short-space idea of pysteps'
    SSFT generator): with unit white noise the expected power of every mode stays what the observation had, at every lead time;
  * the windows blended with sin^2 weights that sum to one (`spectral_ar`);
  * optionally (`probability_matching=True`) every member and lead time pulled back to the marginal distribution of the last
    observed frame (`probability_match`: the recursion keeps a window's spectrum, not its distribution - noise turns a field that
    is mostly exact zeros into a roughly Gaussian one, with almost twice the observed wet area and a quarter of its heavy rain),
    and rain kept to a dilated copy of the observed wet set (`precipitation_mask`: noise is shaped per window and spreads to the
    far side of one);
  * the evolved fields moved along the motion field of the context (`advection.motion_field`, `advection.advect_series`: Lagrangian
    coordinates first, advection last) and taken back to rain rates (`from_db`).

`spectral_ar_reference` is the specification in float64 numpy.  On a HIP device `spectral_ar` is `dgmr_spectral_ar`
(csrc/spectral_ar.hip) on the current stream, without synchronisation; CPU tensors go through the reference.
`probability_match_reference` is the specification of the matching in fp32 numpy, which `dgmr_probability_match`
(csrc/probmatch.hip) reproduces bit for bit: ranks from a 4096-bin histogram of each plane instead of a sort.

Matching and mask act in Lagrangian coordinates: the bilinear advection afterwards blurs the wet / dry edge over a pixel, as it does
for the deterministic baseline, so a moved member's distribution is the observed one only up to that interpolation.

`lifetime_rho` is a fixed power law.  `estimate_rho` measures rho[r] instead, as STEPS does, in Lagrangian coordinates: the context
frames are advected into the last frame's coordinates (`lagrangian_frames`), `lag_spectra` (`dgmr_lag_spectra`, csrc/spectrum.hip;
`lag_spectra_reference` is its float64 specification) forms per window and radial bin the sums of |A|^2, |B|^2 and Re(A conj B) of
consecutive frames over exactly the windows and bins the recursion evolves, and the pooled coherence C / sqrt(Pa Pb) of the windows
that stay clear of the advection's zero inflow is rho[r].  `EnsembleAdvectionNowcaster(rho="estimate")` does this per call and plane.

`spectral_ar2` (`dgmr_spectral_ar2`; `spectral_ar2_reference`) is the same recursion with a second lag, X_t = phi1 X_(t-1) +
phi2 X_(t-2) + g A Wh_t, started from the last two frames; `estimate_ar2` adds the pooled coherence of frames two apart and
`ar2_coefficients` solves Yule-Walker per bin (clipped so that the process stays bounded, keeps rho1 and has unit variance);
`EnsembleAdvectionNowcaster(order=2)` uses them.

`EnsembleAdvectionNowcaster(...).perturb_velocities("steps")` adds STEPS' perturbed motion vectors: every member draws one error
along and one across the local motion, which grow with lead time by `velocity_perturbation_scale`'s law, and moves along
`advection.advect_series_perturbed` instead of `advect_series`.

Limits: a member's velocity error is one pair of scalars along and across the local motion that grows by a fixed law of lead time -
not a spatially varying perturbation field, and the law is not fitted to this data; the AR(2) is per radial bin and from coherences, not per cascade level from pixel correlations
as in STEPS, its Yule-Walker solution is ill-conditioned near rho1 = 1, its second state carries the advection's zero inflow at
the border and its noise amplitude comes from the last frame alone; bilinear advection and motion error bias the estimate's high
wavenumbers low, and a frame too small to keep a window clear of the margin falls back to the law; the mask's dilation law is
fixed (radius + growth t), it does not follow the members.  The white field and the result each take M T H W floats: about
1.1 GB each for 8 members and 18 lead times of a 1536 x 1280 frame.
"""
from __future__ import annotations

import functools
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

from .advection import (CONTEXT_FRAMES, MAX_STEPS, AdvectionNowcaster, _planes, _stream, advect, advect_series, advect_series_perturbed,
                        lattice_geometry, motion_field, unit_directions)
from .spectra import _radial_bins

WINDOWS = (32, 64, 128)
PM_BINS = 4096  # bins of `probability_match`: with its defaults [-64, 64) dB in steps of 1/32 dB


def _check_window(window) -> int:
    if window not in WINDOWS:
        raise ValueError(f"window={window!r}: one of {WINDOWS} is required")
    return int(window)


def _check_plane(h: int, w: int, window: int):
    if h < window or w < window or h % window or w % window:
        raise ValueError(f"H={h} and W={w} must be positive multiples of the window {window}")


# ---- rain rate <-> dB ----------------------------------------------------------------------------------------------------------------
def to_db(x: torch.Tensor, threshold: float = 0.1, pad: float = 5.0) -> torch.Tensor:
    """z = 10 log10(x / threshold) + pad where x >= threshold; 0 everywhere else (dry and missing elements, `!(x >= threshold)`)."""
    wet = x >= threshold
    z = 10.0 * torch.log10(torch.where(wet, x, torch.full_like(x, threshold)) / threshold) + pad
    return torch.where(wet, z, torch.zeros_like(z))


def from_db(z: torch.Tensor, threshold: float = 0.1, pad: float = 5.0) -> torch.Tensor:
    """threshold * 10^((z - pad) / 10) where z >= pad, else 0: `to_db` undone on wet elements."""
    wet = z >= pad
    x = threshold * torch.pow(10.0, (torch.where(wet, z, torch.full_like(z, pad)) - pad) / 10.0)
    return torch.where(wet, x, torch.zeros_like(x))


def lifetime_rho(window: int, tau_ref: float = 12.0, lambda_ref: float = 64.0, beta: float = 1.0) -> torch.Tensor:
    """fp32 [L]: rho[0] = 1 (a window keeps its mean) and rho[r] = exp(-1 / tau(r)), tau(r) = tau_ref ((L / r) / lambda_ref)^beta steps:
    a structure of wavelength lambda_ref pixels decorrelates in tau_ref steps, shorter ones faster.  The defaults are this library's
    (PAPERS.md), not fitted to any data set."""
    window = _check_window(window)
    if not (tau_ref > 0 and lambda_ref > 0):
        raise ValueError(f"tau_ref={tau_ref} and lambda_ref={lambda_ref} must be positive")
    r = np.arange(1, window, dtype=np.float64)
    tau = tau_ref * ((window / r) / lambda_ref) ** beta
    return torch.from_numpy(np.concatenate([[1.0], np.exp(-1.0 / tau)]).astype(np.float32))


# ---- the specification -----------------------------------------------------------------------------------------------------------------
def axis_weights(n: int, window: int):
    """The blend weights along an axis of n pixels -> (a, h), fp32 [n]: h the weight of the offset window over a pixel,
    sin^2(pi (i + 1/2) / L) at its local index i, formed in double and rounded (0 in the outer L / 2, where there is none); a = 1 - h
    in fp32, the weight of the aligned window."""
    hw = (np.sin(np.pi * (np.arange(window) + 0.5) / window) ** 2).astype(np.float32)
    h = np.zeros(n, np.float32)
    if n > window:
        h[window // 2:n - window // 2] = np.tile(hw, n // window - 1)
    return np.float32(1) - h, h


def _class_windows(x: np.ndarray, window: int, cy: int, cx: int) -> np.ndarray:
    """[..., H, W] -> the windows of class (cy, cx), [..., H / L - cy, W / L - cx, L, L] (a view where numpy can make one)"""
    h, w = x.shape[-2:]
    ny, nx, half = h // window - cy, w // window - cx, window // 2
    t = x[..., cy * half:cy * half + ny * window, cx * half:cx * half + nx * window]
    return np.moveaxis(t.reshape(x.shape[:-2] + (ny, window, nx, window)), -3, -2)


def spectral_ar_reference(z0, white, rho, window: int):
    """The specification of `dgmr_spectral_ar`, in float64 numpy.

    z0: fp32 [P, H, W], any real values; white: fp32 [P, M, T, H, W]; rho: fp32 [L], L = window one of 32, 64, 128; H and W multiples of
    L, 1 <= T <= 64.  L x L windows in four classes (cy, cx), each index 0 or 1, with origins (i L + cy L / 2, j L + cx L / 2),
    i < H / L - cy, j < W / L - cx.  Per window and member: U = fft2(z0 patch), A = |U| / L, X_0 = U and, with Wh_t = fft2(white[p, m,
    t - 1] patch),  X_t(k) = rho[r(k)] X_(t-1)(k) + sqrt(1 - rho[r(k)]^2) A(k) Wh_t(k),  x_t = real(ifft2(X_t)),  r(k) the radial bin
    of `spectra` (r (r - 1) < kx^2 + ky^2 <= r (r + 1) over the signed frequencies in [-L/2, L/2)).  out[p, m, t - 1] is the sum of the
    at most four windows over a pixel, weighted per axis by `axis_weights` (h for an offset window, a for an aligned one).

    -> (out float64 [P, M, T, H, W], maj): maj is a tuple over the classes in the order (0,0), (0,1), (1,0), (1,1) of float64
    [P, M, T, H / L - cy, W / L - cx]:  maj_t = (||rho^t U||_2 + sum_(s <= t) ||rho^(t-s) sqrt(1 - rho^2) A Wh_s||_2) / L, which bounds
    the 2-norm of x_t term by term - the scale of the accuracy criterion."""
    window = _check_window(window)
    z0 = np.asarray(z0, dtype=np.float32).astype(np.float64)
    white = np.asarray(white, dtype=np.float32).astype(np.float64)
    rho = np.asarray(rho, dtype=np.float32).astype(np.float64)
    if z0.ndim != 3 or white.ndim != 5 or white.shape[0] != z0.shape[0] or white.shape[3:] != z0.shape[1:]:
        raise ValueError(f"z0 must be [P, H, W] and white [P, M, T, H, W], got {z0.shape} and {white.shape}")
    if rho.shape != (window,):
        raise ValueError(f"rho must hold {window} values, got shape {rho.shape}")
    p, m, steps, h, w = white.shape
    _check_plane(h, w, window)
    if not 1 <= steps <= MAX_STEPS or m < 1 or p < 1:
        raise ValueError(f"T={steps} must be 1 ... {MAX_STEPS}, P={p} and M={m} at least 1")
    rk = rho[_radial_bins(window)]  # [L, L], indexed like fft2's output
    gain = np.sqrt(np.maximum(1.0 - rk * rk, 0.0))
    (ay, hy), (ax, hx) = axis_weights(h, window), axis_weights(w, window)
    out = np.zeros((p, m, steps, h, w))
    majorants = []
    half = window // 2
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            maj = np.zeros((p, m, steps, ny, nx))
            majorants.append(maj)
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)
            wy = (hy if cy else ay)[ys].astype(np.float64)
            wx = (hx if cx else ax)[xs].astype(np.float64)
            u = np.fft.fft2(_class_windows(z0, window, cy, cx))[:, None]    # [P, 1, ny, nx, L, L]
            amp = gain * np.abs(u) / window
            wh = np.fft.fft2(_class_windows(white, window, cy, cx))          # [P, M, T, ny, nx, L, L]
            state = np.broadcast_to(u, (p, m) + u.shape[2:]).copy()
            terms = [state]  # rho^t U, then rho^(t-s) sqrt(1 - rho^2) A Wh_s for s = 1 ... t: the majorant adds their norms
            for t in range(steps):
                drive = amp * wh[:, :, t]
                state = rk * state + drive
                terms = [rk * e for e in terms] + [drive]
                maj[:, :, t] = sum(np.sqrt((np.abs(e) ** 2).sum(axis=(-2, -1))) for e in terms) / window
                x = np.fft.ifft2(state).real                                  # [P, M, ny, nx, L, L]
                x = np.moveaxis(x, -2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * wy[:, None] * wx[None, :]
    return out, tuple(majorants)


# ---- the device path -----------------------------------------------------------------------------------------------------------------
def _members_layout(t: torch.Tensor):
    """[P, M, T, H, W] with contiguous planes -> (member stride, step stride) if the (P, M) pairs are one stride apart in row-major
    order and nothing is negative; None otherwise."""
    p, m, steps, h, w = t.shape
    if (w > 1 and t.stride(4) != 1) or (h > 1 and t.stride(3) != w):
        return None
    ss = int(t.stride(2)) if steps > 1 else h * w
    ms = int(t.stride(1)) if m > 1 else (int(t.stride(0)) if p > 1 else max(steps * ss, h * w))
    if p > 1 and m > 1 and t.stride(0) != m * ms:
        return None
    if ss < h * w or ms < h * w:
        return None
    return ms, ss


def _check_white(z0: torch.Tensor, white: torch.Tensor, window: int):
    """white against z0 [P, H, W] (`_planes`' result) and the window -> (P, M, T, H, W)"""
    if white.dim() != 5 or white.dtype != torch.float32 or white.shape[0] != z0.shape[0] or tuple(white.shape[3:]) != tuple(z0.shape[1:]) \
            or white.device != z0.device:
        raise ValueError(f"white must be a float32 [{z0.shape[0]}, M, T, {z0.shape[1]}, {z0.shape[2]}] tensor on {z0.device}, got "
                         f"{white.dtype} {tuple(white.shape)} on {white.device}")
    p, m, steps, h, w = (int(v) for v in white.shape)
    _check_plane(h, w, window)
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if m < 1 or p < 1:
        raise ValueError(f"P={p} planes and M={m} members: at least one each is required")
    return p, m, steps, h, w


def _check_out(out: Optional[torch.Tensor], shape, device) -> torch.Tensor:
    """out as passed if it is an fp32 tensor or view of `shape` = (P, M, T, H, W) on `device` that `_members_layout` takes; a new
    tensor for None"""
    if out is None:
        return torch.empty(shape, dtype=torch.float32, device=device)
    if tuple(out.shape) != tuple(shape) or out.dtype != torch.float32 or out.device != device or _members_layout(out) is None:
        raise ValueError(f"out must be a float32 [{', '.join(str(v) for v in shape)}] tensor on {device} with contiguous planes and its "
                         "(P, M) pairs one stride apart")
    return out


def _strided(t: torch.Tensor):
    """[P, M, T, H, W] as the device entries read it -> (t, member stride, step stride): copied where `_members_layout` refuses it"""
    if _members_layout(t) is None:
        t = t.contiguous()
    return (t,) + _members_layout(t)


def spectral_ar(z0: torch.Tensor, white: torch.Tensor, rho: torch.Tensor, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`spectral_ar_reference`'s first result for torch tensors -> fp32 [P, M, T, H, W] on the inputs' device.

    z0: fp32 [P, H, W] (contiguous planes, any plane stride); white: fp32 [P, M, T, H, W]; rho: fp32 [L].  white and out (an fp32
    [P, M, T, H, W] tensor or view) must have contiguous planes, steps at least H * W apart and the (P, M) pairs one stride apart - a
    slice of a larger buffer over T, H-aligned rows or members is written in place; a white of another layout is copied, an out of
    another layout is refused.  On a HIP device one `dgmr_spectral_ar` on the current stream, nothing synchronised; 16-byte accesses
    where pointers and strides allow them.  On the CPU the float64 reference, rounded."""
    window = _check_window(window)
    z0, zs = _planes(z0, "z0")
    p, m, steps, h, w = _check_white(z0, white, window)
    if rho.dim() != 1 or rho.shape[0] != window or rho.dtype != torch.float32 or rho.device != z0.device:
        raise ValueError(f"rho must be a float32 [{window}] tensor on {z0.device}, got {rho.dtype} {tuple(rho.shape)} on {rho.device}")
    out = _check_out(out, (p, m, steps, h, w), z0.device)
    if not z0.is_cuda:
        ref, _ = spectral_ar_reference(z0.numpy(), white.numpy(), rho.numpy(), window)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    white, wms, wss = _strided(white)
    oms, oss = _members_layout(out)
    device = z0.device
    with torch.cuda.device(device):
        call("dgmr_spectral_ar", z0.data_ptr(), zs if p > 1 else 0, white.data_ptr(), wms, wss, rho.contiguous().data_ptr(), p, m, steps,
             h, w, window, out.data_ptr(), oms, oss, _stream(device))
    return out


# ---- rho(r) from the context frames ------------------------------------------------------------------------------------------------------
RhoEstimate = namedtuple("RhoEstimate", ["rho", "windows"])


def window_table(h: int, w: int, window: int) -> np.ndarray:
    """int64 [Wn, 4] = (cy, cx, y0, x0): the windows of `spectral_ar` on an H x W plane in `dgmr_lag_spectra`'s order - class by class
    in the order (0,0), (0,1), (1,0), (1,1), row-major inside a class; Wn = the sum over the classes of (H / L - cy) (W / L - cx)."""
    window = _check_window(window)
    _check_plane(h, w, window)
    half = window // 2
    rows = [(cy, cx, i * window + cy * half, j * window + cx * half) for cy in (0, 1) for cx in (0, 1)
            for i in range(h // window - cy) for j in range(w // window - cx)]
    return np.array(rows, dtype=np.int64).reshape(-1, 4)


@functools.lru_cache(maxsize=None)
def _bin_matrix(window: int) -> np.ndarray:
    """float64 [L * L, L]: row k is the indicator of the radial bin of mode k (fft2's order, flattened)"""
    m = np.zeros((window * window, window))
    m[np.arange(window * window), _radial_bins(window).reshape(-1)] = 1.0
    m.setflags(write=False)
    return m


def lag_spectra_reference(a, b, window: int) -> np.ndarray:
    """The specification of `dgmr_lag_spectra`, in float64 numpy -> float64 [N, Wn, 3, L].

    a, b: fp32 [N, H, W], any finite real values; H and W multiples of L = window, one of 32, 64, 128.  Per plane and window of
    `window_table(H, W, L)`, with A = fft2(a patch) and B = fft2(b patch), unnormalised, summed over ALL L^2 modes of radial bin r
    (`spectral_ar_reference`'s r(k), r < L; the corners and the Nyquist row and column are kept):
      [..., 0, r] = sum |A|^2,   [..., 1, r] = sum |B|^2,   [..., 2, r] = sum Re(A conj B);   0 for a bin without modes."""
    window = _check_window(window)
    a = np.asarray(a, dtype=np.float32).astype(np.float64)
    b = np.asarray(b, dtype=np.float32).astype(np.float64)
    if a.ndim != 3 or a.shape != b.shape or a.shape[0] < 1:
        raise ValueError(f"a and b must be [N >= 1, H, W] of one shape, got {a.shape} and {b.shape}")
    n, h, w = a.shape
    _check_plane(h, w, window)
    bins = _bin_matrix(window)
    blocks = []
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            if ny == 0 or nx == 0:
                continue
            fa = np.fft.fft2(_class_windows(a, window, cy, cx)).reshape(n, ny * nx, window * window)
            fb = np.fft.fft2(_class_windows(b, window, cy, cx)).reshape(n, ny * nx, window * window)
            terms = np.stack([fa.real ** 2 + fa.imag ** 2, fb.real ** 2 + fb.imag ** 2, fa.real * fb.real + fa.imag * fb.imag], axis=2)
            blocks.append(terms @ bins)  # [N, ny nx, 3, L]
    return np.concatenate(blocks, axis=1)


def lag_spectra(a: torch.Tensor, b: torch.Tensor, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`lag_spectra_reference` for torch tensors -> float64 [N, Wn, 3, L] on the inputs' device.

    a, b: fp32 [N, H, W] (contiguous planes, any plane stride each; anything else is copied).  out: a contiguous float64
    [N, Wn, 3, L] tensor or view.  On a HIP device one `dgmr_lag_spectra` on the current stream, nothing synchronised, no workspace;
    16-byte loads where both pointers and strides allow them.  On the CPU the float64 reference."""
    window = _check_window(window)
    if tuple(a.shape) != tuple(b.shape) or a.device != b.device:
        raise ValueError(f"a {tuple(a.shape)} on {a.device} and b {tuple(b.shape)} on {b.device} must match")
    a, sa = _planes(a, "a")
    b, sb = _planes(b, "b")
    n, h, w = (int(v) for v in a.shape)
    if n < 1:
        raise ValueError("a and b hold no plane")
    wn = window_table(h, w, window).shape[0]
    if out is None:
        out = torch.empty((n, wn, 3, window), dtype=torch.float64, device=a.device)
    elif tuple(out.shape) != (n, wn, 3, window) or out.dtype != torch.float64 or out.device != a.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous float64 [{n}, {wn}, 3, {window}] tensor on {a.device}")
    if not a.is_cuda:
        out.copy_(torch.from_numpy(lag_spectra_reference(a.numpy(), b.numpy(), window)))
        return out
    from ._lib import call

    device = a.device
    with torch.cuda.device(device):
        call("dgmr_lag_spectra", a.data_ptr(), sa, b.data_ptr(), sb, n, h, w, window, out.data_ptr(), _stream(device))
    return out


def lagrangian_frames(z: torch.Tensor, field: torch.Tensor, origin: float = 0.0, spacing: float = 1.0) -> torch.Tensor:
    """The context in the last frame's coordinates -> fp32 [K, P, H, W]: frame k of z (fp32 [K, P, H, W], time order) moved K - 1 - k
    steps along `field` ([P or 1, Gy, Gx, 2], pixels per step) - the last lead time of one `advect` call per frame -, the newest
    frame as it is.  `advect`'s rules hold: bilinear interpolation, a tap outside the frame is 0 (so a band of up to
    (K - 1) max|field| pixels along the inflow border is not the field moved but zeros), values below 0 read as 0 (dB fields of
    `to_db` have none)."""
    if z.dim() != 4 or z.dtype != torch.float32 or z.shape[0] < 1:
        raise ValueError(f"z must be a float32 [K >= 1, P, H, W] tensor, got {z.dtype} {tuple(z.shape)}")
    k = int(z.shape[0])
    out = torch.empty(tuple(z.shape), dtype=torch.float32, device=z.device)
    out[k - 1].copy_(z[k - 1])
    for i in range(k - 1):
        out[i].copy_(advect(z[i], field, k - 1 - i, origin, spacing)[:, -1])
    return out


def estimate_rho(z: torch.Tensor, field: torch.Tensor, origin: float, spacing: float, window: int, margin: Optional[int] = None,
                 fallback: Optional[torch.Tensor] = None) -> RhoEstimate:
    """The lag-1 correlation per radial bin from K context frames -> RhoEstimate(rho fp32 [P, L], windows float64 [P]).

    z: fp32 [K >= 2, P, H, W] in time order (dB fields); field, origin, spacing: the motion of `motion_field` / `lattice_geometry`.
    The frames are brought to the last frame's coordinates (`lagrangian_frames`), one `lag_spectra` call forms the sums of the K - 1
    consecutive pairs, and they are pooled in float64 over the pairs and over the windows that are used: a window is used iff
    min(y0, x0, H - y0 - L, W - x0 - L) >= margin - the zero inflow of the advection contaminates every window it reaches.  margin:
    None for ceil((K - 1) max|field|) + 1 per plane, computed and applied on the device (a 0 / 1 weight per window: nothing is
    synchronised); 0 uses every window.  With the pooled Pa = sum |A|^2, Pb = sum |B|^2, C = sum Re(A conj B) of a bin:
      rho[r] = clip(C / sqrt(Pa Pb), 0, 1);  rho[0] = 1 (a window keeps its mean, as in `lifetime_rho`);
      rho[r] = fallback[r] where Pa Pb == 0 - a bin without modes, a dry pool, a pool with no window left.
    fallback: fp32 [L], default `lifetime_rho(window)`.  windows: how many windows each plane's pool used.
    Lag 1 only; the bilinear advection and motion error bias high wavenumbers low."""
    frames, weight, fallback = _lagrangian_pool(z, field, origin, spacing, window, margin, fallback)
    return RhoEstimate(_lag1_rho(frames, weight, fallback, window), weight.sum(dim=1))


def _lagrangian_pool(z, field, origin, spacing, window, margin, fallback):
    """The checks of `estimate_rho` -> (the Lagrangian frames [K, P, H, W], the 0 / 1 weight of every window in the pool float64
    [P, Wn], the fallback fp32 [L])"""
    window = _check_window(window)
    if z.dim() != 4 or z.dtype != torch.float32 or z.shape[0] < 2:
        raise ValueError(f"z must be a float32 [K >= 2, P, H, W] tensor, got {z.dtype} {tuple(z.shape)}")
    k, p, h, w = (int(v) for v in z.shape)
    _check_plane(h, w, window)
    device = z.device
    fallback = lifetime_rho(window) if fallback is None else torch.as_tensor(fallback, dtype=torch.float32)
    if tuple(fallback.shape) != (window,):
        raise ValueError(f"fallback must hold {window} values, got shape {tuple(fallback.shape)}")
    frames = lagrangian_frames(z, field, origin, spacing)
    table = window_table(h, w, window)
    edge = np.minimum(np.minimum(table[:, 2], table[:, 3]), np.minimum(h - table[:, 2] - window, w - table[:, 3] - window))
    edge = torch.from_numpy(edge.astype(np.float64)).to(device)
    if margin is None:
        speed = field.abs().reshape(field.shape[0], -1).amax(dim=1).to(torch.float64)  # [P or 1]
        need = torch.ceil((k - 1) * speed) + 1.0
    else:
        if int(margin) < 0:
            raise ValueError(f"margin={margin} must not be negative")
        need = torch.full((1,), float(int(margin)), dtype=torch.float64, device=device)
    weight = (edge[None, :] >= need.expand(p)[:, None]).to(torch.float64)  # [P, Wn]
    return frames, weight, fallback


def _pooled_coherence(frames: torch.Tensor, lag: int, weight: torch.Tensor, window: int):
    """One `lag_spectra` call over the K - lag pairs of frames `lag` apart, pooled in float64 over the pairs and the weighted windows
    -> (gamma = C / sqrt(Pa Pb) float64 [P, L], ok = Pa Pb > 0 bool [P, L]; gamma is C where not ok)"""
    k, p, h, w = (int(v) for v in frames.shape)
    sums = lag_spectra(frames[:-lag].reshape((k - lag) * p, h, w), frames[lag:].reshape((k - lag) * p, h, w), window)
    pooled = (sums.view(k - lag, p, -1, 3, window) * weight[None, :, :, None, None]).sum(dim=(0, 2))  # [P, 3, L]
    den = pooled[:, 0] * pooled[:, 1]
    ok = den > 0
    return pooled[:, 2] / torch.sqrt(torch.where(ok, den, torch.ones_like(den))), ok


def _lag1_rho(frames: torch.Tensor, weight: torch.Tensor, fallback: torch.Tensor, window: int) -> torch.Tensor:
    p = int(frames.shape[1])
    gamma, ok = _pooled_coherence(frames, 1, weight, window)
    rho = torch.where(ok, gamma.clamp(0.0, 1.0).to(torch.float32), fallback.to(frames.device)[None, :].expand(p, window)).contiguous()
    rho[:, 0] = 1.0
    return rho


# ---- the second lag: AR(2) ---------------------------------------------------------------------------------------------------------------
Ar2Estimate = namedtuple("Ar2Estimate", ["rho1", "rho2", "coef", "windows", "previous"])


def ar2_coefficients(rho1: torch.Tensor, rho2: torch.Tensor) -> torch.Tensor:
    """The AR(2) recursion's coefficients per radial bin from the lag-1 and lag-2 correlations -> fp32 [..., 3, L] = (phi1, phi2, g)
    on the inputs' device; rho1, rho2: [..., L] of one shape.  Computed in float64, rounded once.  With r1 = clip(rho1, 0, 1) and
    r2 = clip(rho2, -1, 1):
      where r1 = 1: (1, 0, 0) - the mode is kept, as bin 0 is by `lifetime_rho`;
      elsewhere phi2 = clip((r2 - r1^2) / (1 - r1^2), -1, 1), and 0 where rho2 is NaN (no second lag measured);
                phi1 = r1 (1 - phi2);  g = sqrt((1 - phi2^2) (1 - r1^2)).
    Yule-Walker wherever the clip is inactive: the process X_t = phi1 X_(t-1) + phi2 X_(t-2) + g e_t with unit white e has lag-1
    autocorrelation r1 (whatever the clip does: phi1 / (1 - phi2) = r1), lag-2 autocorrelation phi1 r1 + phi2 = r2 and stationary
    variance 1 (g^2 = (1 - phi2^2)(1 - r1^2) is that variance's innovation).  r1 < 1 and |phi2| <= 1 keep every characteristic root
    in the closed unit disc, a root on the circle simple: the recursion is bounded.  phi2 = 0 is the AR(1) of r1 with its gain."""
    if tuple(rho1.shape) != tuple(rho2.shape) or rho1.dim() < 1 or rho1.device != rho2.device:
        raise ValueError(f"rho1 {tuple(rho1.shape)} on {rho1.device} and rho2 {tuple(rho2.shape)} on {rho2.device} must match, [..., L]")
    r1 = rho1.to(torch.float64).clamp(0.0, 1.0)
    r2 = rho2.to(torch.float64).clamp(-1.0, 1.0)
    kept = r1 >= 1.0
    rest = torch.where(kept, torch.ones_like(r1), 1.0 - r1 * r1)  # 1 - r1^2, and 1 where it is not used
    phi2 = ((r2 - r1 * r1) / rest).clamp(-1.0, 1.0)
    phi2 = torch.where(torch.isnan(rho2) | kept, torch.zeros_like(phi2), phi2)
    phi1 = torch.where(kept, torch.ones_like(r1), r1 * (1.0 - phi2))
    gain = torch.where(kept, torch.zeros_like(r1), torch.sqrt((1.0 - phi2 * phi2) * rest))
    return torch.stack([phi1, phi2, gain], dim=-2).to(torch.float32).contiguous()


def _plane_coefficients(coef: np.ndarray, p: int, window: int) -> np.ndarray:
    """coef [3, L] or [P, 3, L] -> float64 [P, 3, L, L]: every row spread over the modes of fft2's layout"""
    if coef.shape not in ((3, window), (p, 3, window)):
        raise ValueError(f"coef must be [3, {window}] or [{p}, 3, {window}], got shape {coef.shape}")
    return np.broadcast_to(coef, (p, 3, window))[:, :, _radial_bins(window)]


def spectral_ar2_reference(z0, zm1, white, coef, window: int):
    """The specification of `dgmr_spectral_ar2`, in float64 numpy: `spectral_ar_reference` with a second lag.

    z0, white, window, the windows, their classes, the radial bin r(k) and the blend: `spectral_ar_reference`'s.  zm1: fp32 [P, H, W],
    the frame before z0 in z0's coordinates; coef: fp32 [3, L] = (phi1, phi2, g) (`ar2_coefficients`), or [P, 3, L] for a set per
    plane, used as passed.  Per window and member: X_0 = fft2(z0 patch), X_-1 = fft2(zm1 patch), A = |X_0| / L and
      X_t(k) = (phi1[r] X_(t-1)(k) + phi2[r] X_(t-2)(k)) + g[r] A(k) Wh_t(k),   x_t = real(ifft2(X_t)),   t = 1 ... T.

    -> (out float64 [P, M, T, H, W], maj): maj in `spectral_ar_reference`'s layout, from the recursion a rounding error itself
    follows, per mode:  m_0 = |X_0|, m_-1 = |X_-1|, m_t = |phi1| m_(t-1) + |phi2| m_(t-2) + |g A Wh_t|;  maj_t = ||m_t||_2 / L per
    window.  (Signed impulse responses would cancel - an AR(2) oscillates - and under-bound the error.)"""
    window = _check_window(window)
    z0 = np.asarray(z0, dtype=np.float32).astype(np.float64)
    zm1 = np.asarray(zm1, dtype=np.float32).astype(np.float64)
    white = np.asarray(white, dtype=np.float32).astype(np.float64)
    coef = np.asarray(coef, dtype=np.float32).astype(np.float64)
    if z0.ndim != 3 or white.ndim != 5 or white.shape[0] != z0.shape[0] or white.shape[3:] != z0.shape[1:] or zm1.shape != z0.shape:
        raise ValueError(f"z0 and zm1 must be [P, H, W] and white [P, M, T, H, W], got {z0.shape}, {zm1.shape} and {white.shape}")
    p, m, steps, h, w = white.shape
    _check_plane(h, w, window)
    if not 1 <= steps <= MAX_STEPS or m < 1 or p < 1:
        raise ValueError(f"T={steps} must be 1 ... {MAX_STEPS}, P={p} and M={m} at least 1")
    ck = _plane_coefficients(coef, p, window)[:, :, None, None, None]  # [P, 3, 1, 1, 1, L, L]
    phi1, phi2, gain = ck[:, 0], ck[:, 1], ck[:, 2]
    (ay, hy), (ax, hx) = axis_weights(h, window), axis_weights(w, window)
    out = np.zeros((p, m, steps, h, w))
    majorants = []
    half = window // 2
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            maj = np.zeros((p, m, steps, ny, nx))
            majorants.append(maj)
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)
            wy = (hy if cy else ay)[ys].astype(np.float64)
            wx = (hx if cx else ax)[xs].astype(np.float64)
            u = np.fft.fft2(_class_windows(z0, window, cy, cx))[:, None]    # [P, 1, ny, nx, L, L]
            um = np.fft.fft2(_class_windows(zm1, window, cy, cx))[:, None]
            amp = gain * np.abs(u) / window
            wh = np.fft.fft2(_class_windows(white, window, cy, cx))          # [P, M, T, ny, nx, L, L]
            full = (p, m) + u.shape[2:]
            x1, x2 = np.broadcast_to(u, full).copy(), np.broadcast_to(um, full).copy()
            m1, m2 = np.abs(x1), np.abs(x2)
            for t in range(steps):
                drive = amp * wh[:, :, t]
                x1, x2 = (phi1 * x1 + phi2 * x2) + drive, x1
                m1, m2 = np.abs(phi1) * m1 + np.abs(phi2) * m2 + np.abs(drive), m1
                maj[:, :, t] = np.sqrt((m1 * m1).sum(axis=(-2, -1))) / window
                x = np.fft.ifft2(x1).real                                     # [P, M, ny, nx, L, L]
                x = np.moveaxis(x, -2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * wy[:, None] * wx[None, :]
    return out, tuple(majorants)


def spectral_ar2(z0: torch.Tensor, zm1: torch.Tensor, white: torch.Tensor, coef: torch.Tensor, window: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`spectral_ar2_reference`'s first result for torch tensors -> fp32 [P, M, T, H, W] on the inputs' device.

    z0, zm1: fp32 [P, H, W] (contiguous planes, any plane stride each); white, out: `spectral_ar`'s layouts and refusals; coef: fp32
    [3, L] for one set of coefficients, [P, 3, L] for one per plane (`ar2_coefficients`; copied if not contiguous).  On a HIP device one
    `dgmr_spectral_ar2` on the current stream - all planes in its four launches, also with coefficients per plane -, nothing
    synchronised; 16-byte accesses where pointers and strides allow them.  On the CPU the float64 reference, rounded."""
    window = _check_window(window)
    z0, zs = _planes(z0, "z0")
    if tuple(zm1.shape) != tuple(z0.shape) or zm1.device != z0.device:
        raise ValueError(f"zm1 {tuple(zm1.shape)} on {zm1.device} must match z0 {tuple(z0.shape)} on {z0.device}")
    zm1, zms = _planes(zm1, "zm1")
    p, m, steps, h, w = _check_white(z0, white, window)
    if tuple(coef.shape) not in ((3, window), (p, 3, window)) or coef.dtype != torch.float32 or coef.device != z0.device:
        raise ValueError(f"coef must be a float32 [3, {window}] or [{p}, 3, {window}] tensor on {z0.device}, got {coef.dtype} "
                         f"{tuple(coef.shape)} on {coef.device}")
    out = _check_out(out, (p, m, steps, h, w), z0.device)
    if not z0.is_cuda:
        ref, _ = spectral_ar2_reference(z0.numpy(), zm1.numpy(), white.numpy(), coef.numpy(), window)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    white, wms, wss = _strided(white)
    oms, oss = _members_layout(out)
    coef = coef.contiguous()
    device = z0.device
    with torch.cuda.device(device):
        call("dgmr_spectral_ar2", z0.data_ptr(), zs if p > 1 else 0, zm1.data_ptr(), zms if p > 1 else 0, white.data_ptr(), wms, wss,
             coef.data_ptr(), 3 * window if coef.dim() == 3 and p > 1 else 0, p, m, steps, h, w, window, out.data_ptr(), oms, oss,
             _stream(device))
    return out


def estimate_ar2(z: torch.Tensor, field: torch.Tensor, origin: float, spacing: float, window: int, margin: Optional[int] = None,
                 fallback: Optional[torch.Tensor] = None) -> Ar2Estimate:
    """`estimate_rho` with the second lag -> Ar2Estimate(rho1 fp32 [P, L], rho2 fp32 [P, L], coef fp32 [P, 3, L], windows float64 [P],
    previous fp32 [P, H, W]).

    The arguments, the Lagrangian frames, the pool of windows and rho1 are `estimate_rho`'s (the same code: rho1 is its result).
    rho2[r] = clip(C / sqrt(Pa Pb), -1, 1) from one more `lag_spectra` call, over the K - 2 pairs of frames two apart, pooled over
    the same windows; NaN where Pa Pb == 0 and everywhere when K = 2 - no fallback: `ar2_coefficients` reads NaN as "no second lag",
    phi2 = 0, the AR(1) of rho1.  coef = ar2_coefficients(rho1, rho2).  previous: the Lagrangian frame K - 2, the frame before the
    last moved one step along the field - the recursion's zm1 (a view of the frames).  Nothing synchronises.
    Near rho1 -> 1 the Yule-Walker solution is ill-conditioned: phi2 = (rho2 - rho1^2) / (1 - rho1^2) moves by d rho2 / (1 - rho1^2)."""
    frames, weight, fallback = _lagrangian_pool(z, field, origin, spacing, window, margin, fallback)
    rho1 = _lag1_rho(frames, weight, fallback, window)
    k, p = int(frames.shape[0]), int(frames.shape[1])
    if k > 2:
        gamma, ok = _pooled_coherence(frames, 2, weight, window)
        rho2 = torch.where(ok, gamma.clamp(-1.0, 1.0), torch.full_like(gamma, float("nan"))).to(torch.float32).contiguous()
    else:
        rho2 = torch.full((p, window), float("nan"), dtype=torch.float32, device=frames.device)
    return Ar2Estimate(rho1, rho2, ar2_coefficients(rho1, rho2), weight.sum(dim=1), frames[k - 2])


# ---- probability matching and the precipitation mask -----------------------------------------------------------------------------------
def _check_bins(lo: float, scale: float):
    lo, scale = float(lo), float(scale)
    if not (np.isfinite(lo) and np.isfinite(scale) and scale > 0 and np.frexp(scale)[0] == 0.5 and np.float32(scale) == scale):
        raise ValueError(f"lo={lo} must be finite and scale={scale} a power of two")
    return np.float32(lo), np.float32(scale)


def probability_match_reference(z, target_sorted, mask=None, lo: float = -64.0, scale: float = 32.0) -> np.ndarray:
    """The specification of `dgmr_probability_match`, in fp32 numpy -> fp32 [P, M, T, H, W]; the device reproduces it bit for bit.

    z: fp32 [P, M, T, H, W], dB fields in Lagrangian coordinates (`spectral_ar`'s output); target_sorted: fp32 [P, H W], per case the
    frame to match (the last observed dB frame, dry zeros included: matching over the whole plane restores the wet-area ratio too)
    sorted ascending; mask: None or uint8 [P, 1 or T, H, W], nonzero where rain is allowed.  PM_BINS = 4096 bins of 1 / scale dB from
    lo, scale a power of two; N = H W <= 2^24.  Per plane (p, m, t), every operation an fp32 operation rounded once:
      u = (z - lo) scale;  !(u >= 0) (below the range, NaN): b = 0, f = 0;  u >= 4096: b = 4095, f = 0;  else b = floor(u), f = u - b
      (exact);  a masked-out element: b = 0, f = 0;
      h[b] counts the plane's N elements, c[b] = sum of h[b'] over b' < b;
      r = c[b] + min(int(f float(h[b])), h[b] - 1);  out = target_sorted[p][r], and 0.0 for a masked-out element.
    r lies in [c[b], c[b] + h[b] - 1]: the map is monotone in z, every output is a value of the target, a rank differs from the exact
    one by less than its bin's occupancy, and all exact zeros of a member (entirely dry windows) share one rank."""
    lo32, scale32 = _check_bins(lo, scale)
    z = np.asarray(z, dtype=np.float32)
    target_sorted = np.asarray(target_sorted, dtype=np.float32)
    if z.ndim != 5 or target_sorted.ndim != 2 or target_sorted.shape != (z.shape[0], z.shape[3] * z.shape[4]):
        raise ValueError(f"z must be [P, M, T, H, W] and target_sorted [P, H W], got {z.shape} and {target_sorted.shape}")
    p, m, steps, h, w = z.shape
    n = h * w
    if not 1 <= steps <= MAX_STEPS or m < 1 or p < 1 or not 1 <= n <= 1 << 24:
        raise ValueError(f"T={steps} must be 1 ... {MAX_STEPS}, P={p} and M={m} at least 1, H W = {n} 1 ... 2^24")
    allowed = None
    if mask is not None:
        mask = np.asarray(mask)
        if mask.dtype != np.uint8 or mask.ndim != 4 or mask.shape[0] != p or mask.shape[1] not in (1, steps) or mask.shape[2:] != (h, w):
            raise ValueError(f"mask must be uint8 [{p}, 1 or {steps}, {h}, {w}], got {mask.dtype} {mask.shape}")
        allowed = np.broadcast_to((mask != 0)[:, None], z.shape)
    with np.errstate(invalid="ignore", over="ignore"):
        u = (z - lo32) * scale32
        inside = (u >= 0) & (u < PM_BINS)
        top = u >= PM_BINS
    if allowed is not None:
        inside, top = inside & allowed, top & allowed
    fl = np.floor(np.where(inside, u, np.float32(0)))  # fp32
    b = np.where(top, PM_BINS - 1, fl.astype(np.int64))
    f = np.where(inside, u, np.float32(0)) - fl
    assert u.dtype == f.dtype == np.float32
    planes = p * m * steps
    b = b.reshape(planes, n)
    hist = np.bincount((b + np.arange(planes)[:, None] * PM_BINS).ravel(), minlength=planes * PM_BINS).reshape(planes, PM_BINS)
    before = np.cumsum(hist, axis=1) - hist
    hb = np.take_along_axis(hist, b, axis=1)
    within = (f.reshape(planes, n) * hb.astype(np.float32)).astype(np.int64)
    rank = np.take_along_axis(before, b, axis=1) + np.minimum(within, hb - 1)
    case = np.repeat(np.arange(p), m * steps)[:, None]
    out = target_sorted[case, rank].reshape(z.shape)
    if allowed is not None:
        out = np.where(allowed, out, np.float32(0))
    return np.ascontiguousarray(out, dtype=np.float32)


def probability_match(z: torch.Tensor, target: torch.Tensor, mask: Optional[torch.Tensor] = None, lo: float = -64.0, scale: float = 32.0,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`probability_match_reference` for torch tensors -> fp32 [P, M, T, H, W] on the inputs' device: every plane of z takes the
    marginal distribution of its case's `target` plane, through binned ranks.

    z: fp32 [P, M, T, H, W]; target: fp32 [P, H, W], sorted here once per case (`torch.sort`: P planes); mask: None or uint8
    [P, 1 or T, H, W] (`precipitation_mask`).  The layouts of z and out are `spectral_ar`'s: contiguous planes, steps at least H W
    apart, the (P, M) pairs one stride apart; a z of another layout is copied, an out of another layout is refused.  out may be z (in
    place).  On a HIP device one `dgmr_probability_match` on the current stream, nothing synchronised; on the CPU the reference."""
    _check_bins(lo, scale)
    if z.dim() != 5 or z.dtype != torch.float32:
        raise ValueError(f"z must be a float32 [P, M, T, H, W] tensor, got {z.dtype} {tuple(z.shape)}")
    p, m, steps, h, w = (int(v) for v in z.shape)
    n = h * w
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if m < 1 or p < 1 or not 1 <= n <= 1 << 24:
        raise ValueError(f"P={p} planes and M={m} members: at least one each is required, and H W = {n} must be 1 ... 2^24")
    if tuple(target.shape) != (p, h, w) or target.dtype != torch.float32 or target.device != z.device:
        raise ValueError(f"target must be a float32 [{p}, {h}, {w}] tensor on {z.device}, got {target.dtype} {tuple(target.shape)} on "
                         f"{target.device}")
    if mask is not None and (mask.dim() != 4 or mask.dtype != torch.uint8 or mask.device != z.device or mask.shape[0] != p
                             or mask.shape[1] not in (1, steps) or tuple(mask.shape[2:]) != (h, w)):
        raise ValueError(f"mask must be a uint8 [{p}, 1 or {steps}, {h}, {w}] tensor on {z.device}, got {mask.dtype} {tuple(mask.shape)} on "
                         f"{mask.device}")
    out = _check_out(out, (p, m, steps, h, w), z.device)
    target_sorted = torch.sort(target.reshape(p, n), dim=1).values
    if not z.is_cuda:
        ref = probability_match_reference(z.numpy(), target_sorted.numpy(), None if mask is None else mask.numpy(), lo, scale)
        out.copy_(torch.from_numpy(ref))
        return out
    from ._lib import call, load

    z, zms, zss = _strided(z)
    oms, oss = _members_layout(out)
    mask_ptr = mask_ps = mask_ss = 0
    if mask is not None:
        mask = mask.contiguous()
        mask_ptr, mask_ps, mask_ss = mask.data_ptr(), int(mask.shape[1]) * n, n if mask.shape[1] > 1 else 0
    device = z.device
    with torch.cuda.device(device):
        need = int(load().dgmr_probability_match_workspace(p, m, steps))
        if need < 0:
            raise ValueError(f"P M T = {p * m * steps} planes are out of range")
        workspace = torch.empty(need, dtype=torch.uint8, device=device)
        call("dgmr_probability_match", z.data_ptr(), zms, zss, target_sorted.data_ptr(), n, mask_ptr or None, mask_ps, mask_ss, p, m, steps,
             h, w, float(lo), float(scale), workspace.data_ptr(), need, out.data_ptr(), oms, oss, _stream(device))
    return out


def precipitation_mask(z0: torch.Tensor, pad: float, radius: int, growth: float = 0.0, steps: int = 1) -> torch.Tensor:
    """Where an ensemble member may rain -> uint8 [P, 1 or steps, H, W] on z0's device: the wet set `z0 >= pad` of the last observed
    dB frame (fp32 [P, H, W]) dilated by a square of half-width radius + round(growth t) pixels at lead time t = 1 ... steps.
    growth = 0 gives ONE plane for all lead times.  Unlike pysteps' incremental mask the law is fixed: it does not follow what the
    members do.  torch (`max_pool2d`, one row and one column pass): it runs once per case and is not a hot path."""
    if z0.dim() != 3 or z0.dtype != torch.float32:
        raise ValueError(f"z0 must be a float32 [P, H, W] tensor, got {z0.dtype} {tuple(z0.shape)}")
    radius, steps, growth = int(radius), int(steps), float(growth)
    if radius < 0 or growth < 0 or not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"radius={radius} and growth={growth} must not be negative, steps={steps} must be 1 ... {MAX_STEPS}")
    wet = (z0 >= pad).to(torch.float32)[:, None]
    planes = []
    for t in range(1, steps + 1) if growth > 0 else (1,):
        k = radius + int(round(growth * t))
        grown = wet
        if k > 0:
            grown = torch.nn.functional.max_pool2d(grown, (2 * k + 1, 1), stride=1, padding=(k, 0))
            grown = torch.nn.functional.max_pool2d(grown, (1, 2 * k + 1), stride=1, padding=(0, k))
        planes.append(grown)
    return (torch.cat(planes, dim=1) > 0).to(torch.uint8)


# ---- velocity perturbations ------------------------------------------------------------------------------------------------------------
STEPS_P_PAR = (10.88, 0.23, -7.68)   # pysteps' fitted (a, b, c) of the error along the motion, km/h with t in minutes - quoted from memory
STEPS_P_PERP = (5.76, 0.31, -2.72)   # ... and across it
VELOCITY_SEED_OFFSET = 0x56454C  # "VEL": the velocity noise of seed s comes from a CPU generator seeded with s + this


def _law(p, what: str):
    try:
        a, b, c = (float(v) for v in p)
    except (TypeError, ValueError):
        raise ValueError(f"{what}={p!r}: three numbers (a, b, c) of a t^b + c are required") from None
    if not all(np.isfinite(v) for v in (a, b, c)):
        raise ValueError(f"{what}={p!r} must be finite")
    return a, b, c


def velocity_perturbation_scale(steps: int, timestep: float = 5.0, km_per_pixel: float = 1.0, p_par=STEPS_P_PAR,
                                p_perp=STEPS_P_PERP) -> torch.Tensor:
    """The standard deviation of a member's velocity error per lead time -> fp32 [steps, 2] = (sigma_par, sigma_perp) in pixels per step,
    computed in float64 and rounded once:  sigma[t] = max(a ((t + 1) timestep)^b + c, 0) timestep / 60 / km_per_pixel,  t = 0 ...
    steps - 1, with (a, b, c) = p_par along the motion and p_perp across it: STEPS' law a t^b + c in km/h with t in minutes
    (timestep: minutes per step), clipped at 0 and taken to pixels per step.  The defaults are pysteps' fitted constants quoted from
    memory, not fitted to any data set here."""
    steps = int(steps)
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps={steps}, 1 ... {MAX_STEPS} are supported")
    if not (float(timestep) > 0 and float(km_per_pixel) > 0 and np.isfinite(timestep) and np.isfinite(km_per_pixel)):
        raise ValueError(f"timestep={timestep} and km_per_pixel={km_per_pixel} must be positive and finite")
    minutes = (np.arange(steps, dtype=np.float64) + 1.0) * float(timestep)
    sigma = np.stack([np.maximum(a * minutes ** b + c, 0.0) for a, b, c in (_law(p_par, "p_par"), _law(p_perp, "p_perp"))], axis=1)
    with np.errstate(over="ignore"):
        sigma = (sigma * float(timestep) / 60.0 / float(km_per_pixel)).astype(np.float32)
    if not np.isfinite(sigma).all():
        raise ValueError(f"p_par={p_par!r}, p_perp={p_perp!r}: the law leaves fp32's range within {steps} steps")
    return torch.from_numpy(sigma)


class EnsembleAdvectionNowcaster(AdvectionNowcaster):
    """`AdvectionNowcaster` with `num_members` stochastic members: the last frame in dB evolves per window and Fourier mode by
    `spectral_ar` in Lagrangian coordinates, every member is then moved along the context's motion field (`advect_series`, the
    members of a case sharing its field) and taken back to rain rates.  window: L of `spectral_ar` (H and W must be multiples);
    threshold, pad: `to_db`'s; rho: fp32 [window] lag-1 correlations per radial wavenumber, None for `lifetime_rho(window)`, or
    "estimate": every call estimates them per plane from the dB transform of the context frames that give the motion (`estimate_rho`
    with its default margin, `lifetime_rho(window)` as the fallback), keeps them as `last_rho` (fp32 [planes, window]; `last_windows`:
    the windows each pool used) and runs one `spectral_ar` per plane.
    probability_matching: match every member and lead time to the last observed dB frame (`probability_match`, in place, before the
    advection); mask_radius (needs the matching): None for no mask, else `precipitation_mask`'s radius in pixels, mask_growth its
    growth in pixels per lead time.  The defaults leave all three off.
    order: 1 for the AR(1) above; 2 for an AR(2) per mode (`spectral_ar2`), whose second state is the dB frame before the last moved
    one step along the motion field.  order=2 takes rho="estimate" (`estimate_ar2` per call: `last_rho`, `last_rho2` fp32
    [planes, window], `last_coef` fp32 [planes, 3, window], `last_windows`) or an fp32 [2, window] tensor (rho1, rho2)
    (`ar2_coefficients` once: `last_coef` fp32 [3, window]); rho=None is refused - the law has no second lag.  Either way one
    `spectral_ar2` covers all planes.
    Velocity perturbations are off after construction - the members of a case all move along the one motion field (`advect_series`);
    `perturb_velocities("steps")` or `perturb_velocities((p_par, p_perp))` switches STEPS' perturbed motion vectors on: member m of
    a plane draws one pair (eps_par, eps_perp) of unit Gaussians, its velocity at lead time t is v + eps_par sigma_par[t] u +
    eps_perp sigma_perp[t] u_perp with u = `unit_directions(last_field)` and sigma = `velocity_scale` (fp32 [T, 2],
    `velocity_perturbation_scale`), and one `advect_series_perturbed` moves all members.  The pairs of the latest call are
    `last_velocity_noise` (fp32 [planes, M, 2]).
    `refine_motion("lk")` (`AdvectionNowcaster`'s; a method for `perturb_velocities`' reason) switches `motion_field`'s Lucas-Kanade
    refinement on - for the field that moves the members and that aligns the context frames for rho="estimate"."""

    def __init__(self, forecast_steps: int = 18, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                 min_wet: Optional[int] = None, smooth: int = 2, window: int = 128, threshold: float = 0.1, pad: float = 5.0,
                 rho: Optional[torch.Tensor] = None, order: int = 1, probability_matching: bool = False,
                 mask_radius: Optional[int] = None, mask_growth: float = 0.0):
        super().__init__(forecast_steps, block, stride, radius, wet_threshold, min_wet, smooth)
        self.velocity_scale = self.last_velocity_noise = None
        # order sits beside rho, which it qualifies; a bool here is a positional probability_matching from before it existed
        if isinstance(order, bool) or order not in (1, 2):
            raise ValueError(f"order={order!r}: 1 (an AR(1) per mode) or 2 (an AR(2)) is required; pass the arguments after rho by keyword")
        self.order = int(order)
        self.last_rho2 = self.last_coef = None
        self.probability_matching = bool(probability_matching)
        if mask_radius is not None and not self.probability_matching:
            raise ValueError("mask_radius needs probability_matching=True: a masked-out element is dry only after the matching")
        if (mask_radius is not None and int(mask_radius) < 0) or not mask_growth >= 0 or (mask_radius is None and mask_growth != 0):
            raise ValueError(f"mask_radius={mask_radius} and mask_growth={mask_growth} must not be negative, and a growth needs a radius")
        self.mask_radius = None if mask_radius is None else int(mask_radius)
        self.mask_growth = float(mask_growth)
        self.window = _check_window(window)
        self.threshold, self.pad = float(threshold), float(pad)
        self.estimate = isinstance(rho, str)
        if self.estimate and rho != "estimate":
            raise ValueError(f"rho={rho!r}: a tensor, None or \"estimate\" is required")
        if self.order == 2 and rho is None:
            raise ValueError("order=2 needs rho=\"estimate\" or a [2, window] tensor (rho1, rho2): the fixed law has no second lag, and "
                             "rho2 = rho1^2 would be the AR(1) at twice the state")
        rho = lifetime_rho(self.window) if rho is None or self.estimate else torch.as_tensor(rho, dtype=torch.float32)
        if self.order == 2 and not self.estimate:
            if tuple(rho.shape) != (2, self.window):
                raise ValueError(f"order=2: rho must be [2, {self.window}] = (rho1, rho2), got shape {tuple(rho.shape)}")
            self.coef = ar2_coefficients(rho[0], rho[1])  # fp32 [3, window]
        elif tuple(rho.shape) != (self.window,):
            raise ValueError(f"rho must hold {self.window} values, got shape {tuple(rho.shape)}")
        self.rho = rho  # with rho="estimate": the fallback of `estimate_rho`; with order=2 and a tensor: (rho1, rho2)
        self.last_rho = self.last_windows = None

    def white_noise(self, planes: int, num_members: int, h: int, w: int, device, seed: int = 0) -> torch.Tensor:
        """The unit Gaussian field `nowcast` draws for `seed`: fp32 [planes, M, T, H, W] from a seeded `torch.Generator` on `device`."""
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        return torch.randn((planes, int(num_members), self.forecast_steps, h, w), generator=gen, device=device, dtype=torch.float32)

    def perturb_velocities(self, velocity_perturbation="steps", timestep: float = 5.0, km_per_pixel: float = 1.0):
        """Switch the members' velocity perturbations on or off -> self, for `EnsembleAdvectionNowcaster(...).perturb_velocities()`.
        velocity_perturbation: None (off: `advect_series`, the members of a case move along one motion field), "steps" (the defaults of
        `velocity_perturbation_scale`) or a pair (p_par, p_perp) of (a, b, c) triples; timestep: minutes per step; km_per_pixel: the
        grid's.  Sets `velocity_scale` = `velocity_perturbation_scale(forecast_steps, timestep, km_per_pixel, p_par, p_perp)`, fp32
        [T, 2], or None.  (A method, not constructor arguments: the constructor's positional order ends with the mask's arguments.)"""
        if velocity_perturbation is None:
            self.velocity_scale = None
            return self
        if isinstance(velocity_perturbation, str):
            if velocity_perturbation != "steps":
                raise ValueError(f"velocity_perturbation={velocity_perturbation!r}: None, \"steps\" or a pair (p_par, p_perp) is required")
            laws = (STEPS_P_PAR, STEPS_P_PERP)
        else:
            try:
                laws = tuple(velocity_perturbation)
            except TypeError:
                laws = ()
            if len(laws) != 2:
                raise ValueError(f"velocity_perturbation={velocity_perturbation!r}: None, \"steps\" or a pair (p_par, p_perp) of "
                                 "(a, b, c) triples is required")
        self.velocity_scale = velocity_perturbation_scale(self.forecast_steps, timestep, km_per_pixel, laws[0], laws[1])
        return self

    def velocity_noise(self, planes: int, num_members: int, seed: int = 0) -> torch.Tensor:
        """The members' (eps_par, eps_perp) that `nowcast` draws for `seed`: fp32 [planes, M, 2] unit Gaussians on the CPU, from a
        second `torch.Generator` - a CPU one, seeded with (seed + VELOCITY_SEED_OFFSET) mod 2^63, so that a seed gives the same
        pairs for every device and the white-noise draw of `seed` is what it is without perturbations."""
        gen = torch.Generator()
        gen.manual_seed((int(seed) + VELOCITY_SEED_OFFSET) % (1 << 63))
        return torch.randn((int(planes), int(num_members), 2), generator=gen, dtype=torch.float32)

    def _members(self, context: torch.Tensor, num_members: int, seed: int, white: Optional[torch.Tensor],
                 velocity_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """context [T_in, P, H, W] -> rain rates fp32 [P, M, T, H, W]"""
        num_members = int(num_members)
        if num_members < 1:
            raise ValueError(f"num_members={num_members}: at least one member is required")
        planes, h, w = (int(v) for v in context.shape[1:])
        _check_plane(h, w, self.window)
        shape = (planes, num_members, self.forecast_steps, h, w)
        if self.velocity_scale is None:
            if velocity_noise is not None:
                raise ValueError("velocity_noise needs perturb_velocities(...) first")
        elif velocity_noise is None:
            velocity_noise = self.velocity_noise(planes, num_members, seed)
        elif not isinstance(velocity_noise, torch.Tensor) or tuple(velocity_noise.shape) != (planes, num_members, 2) or \
                velocity_noise.dtype != torch.float32:
            raise ValueError(f"velocity_noise must be a float32 [{planes}, {num_members}, 2] tensor, got "
                             f"{getattr(velocity_noise, 'dtype', type(velocity_noise))} {tuple(getattr(velocity_noise, 'shape', ()))}")
        self.last_velocity_noise = None if velocity_noise is None else velocity_noise.to(context.device)
        if white is None:
            white = self.white_noise(planes, num_members, h, w, context.device, seed)
        elif tuple(white.shape) != shape or white.dtype != torch.float32 or white.device != context.device:
            raise ValueError(f"white must be a float32 {shape} tensor on {context.device}, got {white.dtype} {tuple(white.shape)}")
        self.last_field = motion_field(context[-CONTEXT_FRAMES:], **self.params)
        origin, spacing = lattice_geometry(self.params["block"], self.params["stride"])
        z0 = to_db(context[-1], self.threshold, self.pad)
        if self.order == 2:
            if self.estimate:
                est = estimate_ar2(to_db(context[-CONTEXT_FRAMES:], self.threshold, self.pad), self.last_field, origin, spacing,
                                   self.window, fallback=self.rho)
                self.last_rho, self.last_rho2, self.last_coef, self.last_windows, zm1 = est
            else:
                self.last_coef = self.coef.to(context.device)
                zm1 = advect(to_db(context[-2], self.threshold, self.pad), self.last_field, 1, origin, spacing)[:, -1]
            z = spectral_ar2(z0, zm1, white, self.last_coef, self.window)  # one call for all planes, coefficients per plane or not
        elif self.estimate:
            est = estimate_rho(to_db(context[-CONTEXT_FRAMES:], self.threshold, self.pad), self.last_field, origin, spacing, self.window,
                               fallback=self.rho)
            self.last_rho, self.last_windows = est
            z = torch.empty(shape, dtype=torch.float32, device=context.device)
            for i in range(planes):  # a rho of its own per plane: one launch each, into views
                spectral_ar(z0[i:i + 1], white[i:i + 1], self.last_rho[i], self.window, out=z[i:i + 1])
        else:
            z = spectral_ar(z0, white, self.rho.to(context.device), self.window)
        if self.probability_matching:
            mask = None
            if self.mask_radius is not None:
                mask = precipitation_mask(z0, self.pad, self.mask_radius, self.mask_growth, self.forecast_steps)
            probability_match(z, z0, mask, out=z)
        if self.velocity_scale is None:
            moved = advect_series(z.view(planes * num_members, self.forecast_steps, h, w), self.last_field, origin, spacing,
                                  field_group=num_members)
        else:  # amplitude[n = plane M + m, t] = eps[plane, m] sigma[t], one fp32 product each
            amplitude = self.last_velocity_noise[:, :, None, :] * self.velocity_scale.to(context.device)[None, None, :, :]
            moved = advect_series_perturbed(z.view(planes * num_members, self.forecast_steps, h, w), self.last_field,
                                            unit_directions(self.last_field), amplitude.reshape(planes * num_members, self.forecast_steps, 2),
                                            origin, spacing, field_group=num_members)
        return from_db(moved, self.threshold, self.pad).view(shape)

    def nowcast(self, frames, num_members: int, seed: int = 0, white: Optional[torch.Tensor] = None, scale: float = 1.0,
                offset: float = 0.0, velocity_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames [T_in >= 2, H, W, C] as in `AdvectionNowcaster.nowcast` -> fp32 [M, forecast_steps, C, H, W] on the frames' device.
        seed: of the white noise; white: fp32 [C, M, T, H, W] to use instead (the same field gives the same members on every device).
        velocity_noise (after `perturb_velocities`): fp32 [C, M, 2] = the members' (eps_par, eps_perp) on any device, to use instead
        of `self.velocity_noise(C, M, seed)`; kept as `last_velocity_noise`."""
        from .verification import observed_from_frames

        x = observed_from_frames(frames, scale, offset)  # [T_in, C, H, W]
        if x.shape[0] < 2:
            raise ValueError(f"frames holds {x.shape[0]} frames, the motion needs 2")
        return self._members(x.contiguous(), num_members, seed, white, velocity_noise).permute(1, 2, 0, 3, 4).contiguous()

    def nowcast_batch(self, images: torch.Tensor, num_members: int, seed: int = 0, white: Optional[torch.Tensor] = None,
                      velocity_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images fp32 [B, T_in >= 2, C, H, W] -> fp32 [M, B, forecast_steps, C, H, W].  white: fp32 [B * C, M, T, H, W];
        velocity_noise: fp32 [B * C, M, 2] (`nowcast`)."""
        if images.dim() != 5 or images.shape[1] < 2 or images.dtype != torch.float32:
            raise ValueError(f"images must be a float32 [B, T_in >= 2, C, H, W] tensor, got {images.dtype} {tuple(images.shape)}")
        b, _, c, h, w = images.shape
        context = images[:, -CONTEXT_FRAMES:].permute(1, 0, 2, 3, 4).reshape(-1, b * c, h, w).contiguous()
        rain = self._members(context, num_members, seed, white, velocity_noise)  # [B * C, M, T, H, W]
        return rain.view(b, c, int(num_members), self.forecast_steps, h, w).permute(2, 0, 3, 1, 4, 5).contiguous()
