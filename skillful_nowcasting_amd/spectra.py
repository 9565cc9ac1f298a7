"""Radially averaged power spectral density of nowcasts and observations (the paper's spectral plot).

A generator that drifts towards the ensemble mean can improve its CRPS and CSI; what gives it away is the collapse of the power
spectrum at short wavelengths.  For one L x L window `x` (fp32, L a power of two out of 32 ... 512):

  * an element is missing when `!(x >= 0)` (the loader's rule); a missing element is read as 0 and counted;
  * `F = fft2(x)`, unnormalised, with NO window function and NO detrending - a window that is not periodic leaks;
  * with integer frequencies `kx, ky` in `-L/2 ... L/2 - 1`, a mode belongs to the radial bin `r = round(sqrt(kx^2 + ky^2))`, found
    in integers (`r (r - 1) < kx^2 + ky^2 <= r (r + 1)`; the square root of an integer is never `k + 1/2`, so there are no ties);
  * `power[r]` = sum of `|F|^2` over the modes of bin r, r = 0 ... L / 2 - 1, in float64; modes with r >= L / 2 (the corners, the
    Nyquist row and column) are dropped.  Sums, not means: divide by `radial_bin_counts(L)` for the mean per mode.

A plane [H][W], H and W multiples of L, is cut into (H / L) x (W / L) non-overlapping windows with one spectrum each (Welch-style
averaging over the windows of a full frame is the caller's sum).  `radial_psd_reference` is the specification in numpy / float64.  On
a HIP device `radial_psd` is `dgmr_radial_psd` (csrc/spectrum.hip): fp32 transforms in LDS that use the input's Hermitian symmetry.
`SpectrumVerifier` accumulates forecast and observed spectra per lead time on the device and has `NowcastVerifier`'s `update`, so
`DGMR.verify_batch(batch, SpectrumVerifier(...))` works.
"""
from __future__ import annotations

import ctypes
import functools
from typing import Optional

import numpy as np
import torch

WINDOWS = (32, 64, 128, 256, 512)


def _check_window(window: int) -> int:
    if window not in WINDOWS:
        raise ValueError(f"window={window}: one of {WINDOWS} is required")
    return int(window)


def _check_plane(h: int, w: int, window: int):
    if h < window or w < window or h % window or w % window:
        raise ValueError(f"H={h} and W={w} must be positive multiples of the window {window}")


@functools.lru_cache(maxsize=None)
def _radial_bins(window: int) -> np.ndarray:
    """[L, L] int64, indexed like `numpy.fft.fft2`'s output: the bin of every mode (>= L / 2 for the dropped ones)."""
    k = np.fft.fftfreq(window, 1.0 / window).astype(np.int64)  # 0 ... L/2 - 1, -L/2 ... -1
    d2 = k[:, None] ** 2 + k[None, :] ** 2
    r = np.arange(window, dtype=np.int64)  # (r (r - 1) < d2 <= r (r + 1)) for exactly one r <= L / sqrt(2) + 1
    bins = np.searchsorted(r * (r + 1), d2, side="left")  # the first r with d2 <= r (r + 1): r (r - 1) < d2 then holds as well
    bins.setflags(write=False)
    return bins


def radial_bin_counts(window: int) -> np.ndarray:
    """The number of modes per radial bin r = 0 ... L / 2 - 1 (1, 8, 12, 16, 32, 28, ...): it depends on L alone."""
    window = _check_window(window)
    return np.bincount(_radial_bins(window).reshape(-1), minlength=window)[:window // 2].astype(np.int64)


def radial_psd_reference(x, window: int):
    """The specification of `dgmr_radial_psd`, in numpy / float64.

    x: fp32 [..., H, W], H and W multiples of `window`.  -> (power float64 [..., H / L, W / L, L / 2], missing int64 [..., H / L, W / L])."""
    window = _check_window(window)
    x = np.asarray(x, dtype=np.float32)
    if x.ndim < 2:
        raise ValueError(f"x must be [..., H, W], got shape {x.shape}")
    h, w = x.shape[-2:]
    _check_plane(h, w, window)
    lead = x.shape[:-2]
    tiles = x.reshape(lead + (h // window, window, w // window, window))
    tiles = np.moveaxis(tiles, -3, -2)  # [..., H / L, W / L, L, L]
    with np.errstate(invalid="ignore"):
        present = tiles >= 0
    missing = (~present).sum(axis=(-2, -1)).astype(np.int64)
    spec = np.fft.fft2(np.where(present, tiles, np.float32(0)).astype(np.float64))
    mag = (spec.real ** 2 + spec.imag ** 2).reshape(-1, window * window)
    bins = _radial_bins(window).reshape(-1)
    keep = bins < window // 2
    power = np.zeros((mag.shape[0], window // 2), np.float64)
    for i in range(mag.shape[0]):
        power[i] = np.bincount(bins[keep], weights=mag[i][keep], minlength=window // 2)
    return power.reshape(lead + (h // window, w // window, window // 2)), missing


# ---- the device path -------------------------------------------------------------------------------------------------------------
def _plane_layout(x: torch.Tensor):
    """-> the plane stride (elements) if x [..., H, W] can be read in place: every plane a contiguous [H][W] block, the planes a
    constant stride apart in row-major order of the leading dimensions, stride % 4 == 0 and the first element 16-byte aligned;
    None otherwise."""
    h, w = x.shape[-2:]
    if (w != 1 and x.stride(-1) != 1) or (h != 1 and x.stride(-2) != w) or x.data_ptr() % 16:
        return None
    dims = [(int(s), int(st)) for s, st in zip(x.shape[:-2], x.stride()[:-2]) if s != 1]
    if not dims:
        return h * w
    stride = dims[-1][1]
    want = stride
    for size, st in reversed(dims):
        if st != want:
            return None
        want *= size
    return stride if stride >= h * w and stride % 4 == 0 else None


def radial_psd(x: torch.Tensor, window: int, workspace: Optional[torch.Tensor] = None):
    """`radial_psd_reference` as tensors on x's device: (power float64 [..., H / L, W / L, L / 2], missing int64 [..., H / L, W / L]).

    x: fp32 [..., H, W].  On a HIP device this is `dgmr_radial_psd` on the current stream, without synchronisation, reading x in
    place when every plane is one contiguous block and the planes are a constant multiple of 4 elements apart (a contiguous tensor,
    `ensemble[:, 1]`); any other layout is copied first.  CPU tensors go through the reference.  workspace: a uint8 tensor on x's
    device to use instead of the cached one (at least `dgmr_radial_psd_workspace(1, L, L, L)` bytes; its size only sets how many
    windows the two-pass path takes per round, never the result)."""
    try:
        window = _check_window(int(window))
    except TypeError:
        raise ValueError(f"window={window!r}: one of {WINDOWS} is required") from None
    if x.dim() < 2:
        raise ValueError(f"x must be [..., H, W], got shape {tuple(x.shape)}")
    if x.dtype != torch.float32:
        raise ValueError(f"x ({x.dtype}) must be float32")
    h, w = int(x.shape[-2]), int(x.shape[-1])
    _check_plane(h, w, window)
    lead = tuple(x.shape[:-2])
    n = int(np.prod(lead, dtype=np.int64))
    if n < 1:
        raise ValueError(f"x {tuple(x.shape)} holds no plane")
    if not x.is_cuda:
        power, missing = radial_psd_reference(x.numpy(), window)
        return torch.from_numpy(np.ascontiguousarray(power)), torch.from_numpy(np.ascontiguousarray(missing))
    from ._lib import call, load
    from .verification import _workspace  # one cached buffer per (device, stream), shared with ensemble_scores: the stream orders its users

    device = x.device
    with torch.cuda.device(device):
        stride = _plane_layout(x)
        if stride is None:
            x = x.contiguous()
            if x.data_ptr() % 16:
                x = x.clone(memory_format=torch.contiguous_format)
            stride = h * w
        nbytes = int(load().dgmr_radial_psd_workspace(n, h, w, window))
        if nbytes < 0:
            raise ValueError(f"dgmr_radial_psd_workspace refused N={n}, H={h}, W={w}, L={window}")
        ws = _workspace(device, nbytes) if workspace is None else workspace
        power = torch.empty(lead + (h // window, w // window, window // 2), dtype=torch.float64, device=device)
        missing = torch.empty(lead + (h // window, w // window), dtype=torch.int64, device=device)
        call("dgmr_radial_psd", x.data_ptr(), stride, n, h, w, window, ws.data_ptr(), ws.numel(), power.data_ptr(), missing.data_ptr(),
             ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return power, missing


class SpectrumVerifier:
    """Accumulate radial power spectra of forecasts and observations per lead time over cases (and channels and windows).

    num_members: M; lead_times: the number of forecast steps T (or a sequence of their labels); window: L; grid_km: the grid length,
    for `wavelength_km`.  The forecast power is the SUM OF THE MEMBERS' OWN SPECTRA (divided by M in `compute`), never the spectrum of
    the ensemble mean: the mean of an ensemble is smooth by construction, and the plot is there to show whether single nowcasts
    keep the observation's power at short wavelengths.  A window in which the observation has any missing element is left out of
    the forecast sum, the observed sum and the window count alike (a mask formed on the device: nothing is read back).  The
    accumulators are float64, on the device of the first `update`; frames larger than the window contribute all their windows
    (Welch-style averaging)."""

    def __init__(self, num_members: int, lead_times, window: int = 256, grid_km: float = 1.0):
        self.num_members = int(num_members)
        self.lead_times = int(lead_times) if isinstance(lead_times, (int, np.integer)) else len(tuple(lead_times))
        self.window = _check_window(int(window))
        self.grid_km = float(grid_km)
        if self.num_members < 1:
            raise ValueError(f"{num_members} ensemble members: at least one is required")
        if self.lead_times < 1:
            raise ValueError(f"lead_times={lead_times}: at least one lead time is required")
        self._acc = None  # (forecast power [T, L / 2], observed power [T, L / 2], windows [T])

    def _zeros(self, device):
        t, nb = self.lead_times, self.window // 2
        return tuple(torch.zeros(shape, dtype=torch.float64, device=device) for shape in ((t, nb), (t, nb), (t,)))

    def update(self, forecast: torch.Tensor, observed: torch.Tensor, weights=None) -> None:
        """forecast [M, T, C, H, W] with observed [T, C, H, W] (one case; `weights`: None or one value), or forecast [M, B, T, C, H, W]
        with observed [B, T, C, H, W] and `weights` [B] (None: ones), as in `NowcastVerifier.update`.  Two `radial_psd` calls; a
        window's spectra are multiplied by its case's weight.  Nothing is synchronised."""
        if forecast.dim() == 5:
            forecast, observed = forecast.unsqueeze(1), observed.unsqueeze(0)
        if forecast.dim() != 6 or observed.dim() != 5 or tuple(forecast.shape[1:]) != tuple(observed.shape):
            raise ValueError(f"forecast must be [M, T, C, H, W] or [M, B, T, C, H, W] and observed the same without M, got "
                             f"{tuple(forecast.shape)} and {tuple(observed.shape)}")
        m, b, t = (int(v) for v in forecast.shape[:3])
        if m != self.num_members or t != self.lead_times:
            raise ValueError(f"forecast {tuple(forecast.shape)}: {self.num_members} members and {self.lead_times} lead times are expected")
        device = forecast.device
        w = torch.ones(b, dtype=torch.float64) if weights is None else torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
        if w.numel() != b:
            raise ValueError(f"{w.numel()} weights for {b} cases")
        if w.device != device:
            w = w.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else w.to(device)
        obs_power, obs_missing = radial_psd(observed, self.window)  # [B, T, C, wy, wx, L / 2], [B, T, C, wy, wx]
        fc_power, _ = radial_psd(forecast, self.window)             # [M, B, T, C, wy, wx, L / 2]
        mask = (obs_missing == 0).to(torch.float64) * w.view(b, 1, 1, 1, 1)  # the weight of every window, 0 where anything is missing
        if self._acc is None:
            self._acc = self._zeros(device)
        fc_acc, obs_acc, win_acc = self._acc
        fc_acc.add_((fc_power * mask[None, ..., None]).sum(dim=(0, 1, 3, 4, 5)).to(fc_acc.device))
        obs_acc.add_((obs_power * mask[..., None]).sum(dim=(0, 2, 3, 4)).to(obs_acc.device))
        win_acc.add_(mask.sum(dim=(0, 2, 3, 4)).to(win_acc.device))

    def merge(self, other: "SpectrumVerifier") -> None:
        """Add another verifier's accumulators (another rank's, another shard's) to this one's."""
        if (other.num_members, other.lead_times, other.window) != (self.num_members, self.lead_times, self.window):
            raise ValueError("merge: the other verifier has a different configuration")
        if other._acc is None:
            return
        if self._acc is None:
            self._acc = self._zeros(other._acc[0].device)
        for mine, theirs in zip(self._acc, other._acc):
            mine.add_(theirs.to(mine.device))

    def reset(self) -> None:
        if self._acc is not None:
            for a in self._acc:
                a.zero_()

    def compute(self) -> dict:
        """The one call that brings results to the host.  -> dict of numpy arrays, T = lead times, L = window:
          psd_forecast -> [T, L / 2]   mean power per mode of a single member: sum / (M * windows * radial_bin_counts); NaN without windows
          psd_observed -> [T, L / 2]   the same for the observation
          wavenumber -> [L / 2]        r = 0 ... L / 2 - 1 (cycles per window)
          wavelength_km -> [L / 2]     L * grid_km / r, inf at r = 0
          windows -> [T]               the (weighted) number of windows"""
        acc = self._acc if self._acc is not None else self._zeros(torch.device("cpu"))
        fc, obs, windows = (a.cpu().numpy() for a in acc)
        counts = radial_bin_counts(self.window).astype(np.float64)
        r = np.arange(self.window // 2, dtype=np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            return {"psd_forecast": fc / (self.num_members * windows[:, None] * counts[None, :]),
                    "psd_observed": obs / (windows[:, None] * counts[None, :]),
                    "wavenumber": r.astype(np.int64),
                    "wavelength_km": self.window * self.grid_km / r,
                    "windows": windows.copy()}
