"""A stochastic advection ensemble: the core of STEPS in one form (INTEGRATION.md "A probabilistic baseline").

  * the last observed frame in dB (`to_db`), cut into overlapping L x L windows;
  * per window and member an AR(1) process per Fourier mode, `X_t = rho X_(t-1) + sqrt(1 - rho^2) A Wh_t`, whose lag-1 correlation
    `rho` depends on the mode's radial wavenumber (`lifetime_rho`: small scales forget faster - a cascade with as many levels as radial
    bins) and whose noise is shaped by the window's own amplitude spectrum `A = |fft2(window)| / L` (the short-space idea of pysteps'
    SSFT generator): with unit white noise the expected power of every mode stays what the observation had, at every lead time;
  * the windows blended with sin^2 weights that sum to one (`spectral_ar`);
  * the evolved fields moved along the motion field of the context (`advection.motion_field`, `advection.advect_series`: Lagrangian
    coordinates first, advection last) and taken back to rain rates (`from_db`).

`spectral_ar_reference` is the specification in float64 numpy.  On a HIP device `spectral_ar` is `dgmr_spectral_ar`
(csrc/spectrum.hip) on the current stream, without synchronisation; CPU tensors go through the reference.

Limits: no probability matching (the marginal distribution of the members is not pulled back to the observed one), no
precipitation mask (noise can create light rain just outside an echo), no velocity perturbations, and the lifetime law is a fixed
power law, not estimated from data.  The white field and the result each take M T H W floats: about 1.1 GB each for 8 members and 18
lead times of a 1536 x 1280 frame.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from .advection import CONTEXT_FRAMES, MAX_STEPS, AdvectionNowcaster, _planes, _stream, advect_series, lattice_geometry, motion_field
from .spectra import _radial_bins

WINDOWS = (32, 64, 128)


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


def spectral_ar(z0: torch.Tensor, white: torch.Tensor, rho: torch.Tensor, window: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`spectral_ar_reference`'s first result for torch tensors -> fp32 [P, M, T, H, W] on the inputs' device.

    z0: fp32 [P, H, W] (contiguous planes, any plane stride); white: fp32 [P, M, T, H, W]; rho: fp32 [L].  white and out (an fp32
    [P, M, T, H, W] tensor or view) must have contiguous planes, steps at least H * W apart and the (P, M) pairs one stride apart - a
    slice of a larger buffer over T, H-aligned rows or members is written in place; a white of another layout is copied, an out of
    another layout is refused.  On a HIP device one `dgmr_spectral_ar` on the current stream, nothing synchronised; 16-byte accesses
    where pointers and strides allow them.  On the CPU the float64 reference, rounded."""
    window = _check_window(window)
    z0, zs = _planes(z0, "z0")
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
    if rho.dim() != 1 or rho.shape[0] != window or rho.dtype != torch.float32 or rho.device != z0.device:
        raise ValueError(f"rho must be a float32 [{window}] tensor on {z0.device}, got {rho.dtype} {tuple(rho.shape)} on {rho.device}")
    if out is None:
        out = torch.empty((p, m, steps, h, w), dtype=torch.float32, device=z0.device)
    elif tuple(out.shape) != (p, m, steps, h, w) or out.dtype != torch.float32 or out.device != z0.device or _members_layout(out) is None:
        raise ValueError(f"out must be a float32 [{p}, {m}, {steps}, {h}, {w}] tensor on {z0.device} with contiguous planes and its "
                         "(P, M) pairs one stride apart")
    if not z0.is_cuda:
        ref, _ = spectral_ar_reference(z0.numpy(), white.numpy(), rho.numpy(), window)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    if _members_layout(white) is None:
        white = white.contiguous()
    wms, wss = _members_layout(white)
    oms, oss = _members_layout(out)
    device = z0.device
    with torch.cuda.device(device):
        call("dgmr_spectral_ar", z0.data_ptr(), zs if p > 1 else 0, white.data_ptr(), wms, wss, rho.contiguous().data_ptr(), p, m, steps,
             h, w, window, out.data_ptr(), oms, oss, _stream(device))
    return out


class EnsembleAdvectionNowcaster(AdvectionNowcaster):
    """`AdvectionNowcaster` with `num_members` stochastic members: the last frame in dB evolves per window and Fourier mode by
    `spectral_ar` in Lagrangian coordinates, every member is then moved along the context's motion field (`advect_series`, the
    members of a case sharing its field) and taken back to rain rates.  window: L of `spectral_ar` (H and W must be multiples);
    threshold, pad: `to_db`'s; rho: fp32 [window] lag-1 correlations per radial wavenumber, None for `lifetime_rho(window)`."""

    def __init__(self, forecast_steps: int = 18, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                 min_wet: Optional[int] = None, smooth: int = 2, window: int = 128, threshold: float = 0.1, pad: float = 5.0,
                 rho: Optional[torch.Tensor] = None):
        super().__init__(forecast_steps, block, stride, radius, wet_threshold, min_wet, smooth)
        self.window = _check_window(window)
        self.threshold, self.pad = float(threshold), float(pad)
        rho = lifetime_rho(self.window) if rho is None else torch.as_tensor(rho, dtype=torch.float32)
        if tuple(rho.shape) != (self.window,):
            raise ValueError(f"rho must hold {self.window} values, got shape {tuple(rho.shape)}")
        self.rho = rho

    def white_noise(self, planes: int, num_members: int, h: int, w: int, device, seed: int = 0) -> torch.Tensor:
        """The unit Gaussian field `nowcast` draws for `seed`: fp32 [planes, M, T, H, W] from a seeded `torch.Generator` on `device`."""
        gen = torch.Generator(device=device)
        gen.manual_seed(int(seed))
        return torch.randn((planes, int(num_members), self.forecast_steps, h, w), generator=gen, device=device, dtype=torch.float32)

    def _members(self, context: torch.Tensor, num_members: int, seed: int, white: Optional[torch.Tensor]) -> torch.Tensor:
        """context [T_in, P, H, W] -> rain rates fp32 [P, M, T, H, W]"""
        num_members = int(num_members)
        if num_members < 1:
            raise ValueError(f"num_members={num_members}: at least one member is required")
        planes, h, w = (int(v) for v in context.shape[1:])
        _check_plane(h, w, self.window)
        shape = (planes, num_members, self.forecast_steps, h, w)
        if white is None:
            white = self.white_noise(planes, num_members, h, w, context.device, seed)
        elif tuple(white.shape) != shape or white.dtype != torch.float32 or white.device != context.device:
            raise ValueError(f"white must be a float32 {shape} tensor on {context.device}, got {white.dtype} {tuple(white.shape)}")
        self.last_field = motion_field(context[-CONTEXT_FRAMES:], **self.params)
        origin, spacing = lattice_geometry(self.params["block"], self.params["stride"])
        z0 = to_db(context[-1], self.threshold, self.pad)
        z = spectral_ar(z0, white, self.rho.to(context.device), self.window)
        moved = advect_series(z.view(planes * num_members, self.forecast_steps, h, w), self.last_field, origin, spacing,
                              field_group=num_members)
        return from_db(moved, self.threshold, self.pad).view(shape)

    def nowcast(self, frames, num_members: int, seed: int = 0, white: Optional[torch.Tensor] = None, scale: float = 1.0,
                offset: float = 0.0) -> torch.Tensor:
        """frames [T_in >= 2, H, W, C] as in `AdvectionNowcaster.nowcast` -> fp32 [M, forecast_steps, C, H, W] on the frames' device.
        seed: of the white noise; white: fp32 [C, M, T, H, W] to use instead (the same field gives the same members on every device)."""
        from .verification import observed_from_frames

        x = observed_from_frames(frames, scale, offset)  # [T_in, C, H, W]
        if x.shape[0] < 2:
            raise ValueError(f"frames holds {x.shape[0]} frames, the motion needs 2")
        return self._members(x.contiguous(), num_members, seed, white).permute(1, 2, 0, 3, 4).contiguous()

    def nowcast_batch(self, images: torch.Tensor, num_members: int, seed: int = 0, white: Optional[torch.Tensor] = None) -> torch.Tensor:
        """images fp32 [B, T_in >= 2, C, H, W] -> fp32 [M, B, forecast_steps, C, H, W].  white: fp32 [B * C, M, T, H, W]."""
        if images.dim() != 5 or images.shape[1] < 2 or images.dtype != torch.float32:
            raise ValueError(f"images must be a float32 [B, T_in >= 2, C, H, W] tensor, got {images.dtype} {tuple(images.shape)}")
        b, _, c, h, w = images.shape
        context = images[:, -CONTEXT_FRAMES:].permute(1, 0, 2, 3, 4).reshape(-1, b * c, h, w).contiguous()
        rain = self._members(context, num_members, seed, white)  # [B * C, M, T, H, W]
        return rain.view(b, c, int(num_members), self.forecast_steps, h, w).permute(2, 0, 3, 1, 4, 5).contiguous()
