"""Fractions skill score (FSS; PAPERS.md: Roberts & Lean 2008) of ensemble nowcasts at neighbourhood scales.

For a threshold `thr`, a radius r and the present pixels of a plane (an observed element is missing when `!(y >= 0)`, as everywhere in
the verification; at a missing pixel neither the observation nor any member is an event), with `box_r` the sum over the (2r + 1)^2
square centred on a pixel of the zero-padded plane:

    I_m = present & (x_m >= thr),  I_o = present & (y >= thr),  S_m = box_r(I_m),  S_o = box_r(I_o),  S_f = sum_m S_m
    sums[N, K, S, 4] = sum over all pixels of the plane of (S_f^2, S_o^2, S_f S_o, sum_m S_m^2)            # ff, oo, fo, mm
    events[N, K, 2]  = (sum_m sum_pixels I_m, sum_pixels I_o)

All integers, nothing divided: the (2r + 1)^2 normalisation cancels in the scores.  The FSS of the ensemble's neighbourhood probability
(Schwartz et al. 2010) is 2 (fo / M) / (ff / M^2 + oo) = 1 - MSE / MSE_ref; the pooled FSS of the members as deterministic
forecasts is 2 (fo / M) / (mm / M + oo).

`fss_sums_reference` is the specification in numpy.  On a HIP device `fss_sums` is `dgmr_fss_sums` (csrc/fss.hip), equal to it bit for
bit.  `FractionsVerifier` accumulates the sums per lead time on the device, weighted by the cases' inverse inclusion probabilities, and
has `NowcastVerifier`'s `update`, so `DGMR.verify_batch(batch, FractionsVerifier(...))` works; `compute()` turns them into the scores
on the host.  Odd sides up to 65 px, zero padding at the border, no per-region masks.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from .verification import DEFAULT_THRESHOLDS, MAX_MEMBERS, MAX_THRESHOLDS, _check_shape, _device_thresholds, _planes_contiguous

DEFAULT_RADII = (0, 2, 8, 32)
MAX_RADII = 8
MAX_RADIUS = 32


def _check_config(thresholds, radii):
    thr = np.asarray(tuple(thresholds), dtype=np.float32).reshape(-1)
    if not 1 <= thr.size <= MAX_THRESHOLDS:
        raise ValueError(f"{thr.size} thresholds, 1 ... {MAX_THRESHOLDS} are supported")
    given = tuple(radii)
    if any(int(r) != r for r in given):
        raise ValueError(f"radii={given}: integers are required")
    rad = tuple(int(r) for r in given)
    if not 1 <= len(rad) <= MAX_RADII or any(not 0 <= r <= MAX_RADIUS for r in rad) or len(set(rad)) != len(rad):
        raise ValueError(f"radii={rad}: 1 ... {MAX_RADII} distinct values out of 0 ... {MAX_RADIUS} are required")
    return thr, rad


def _check_overflow(m: int, h: int, w: int, rad) -> None:
    """Every sum is at most M^2 (2R + 1)^4 H W (Python integers)."""
    if m * m * (2 * max(rad) + 1) ** 4 * h * w >= 2 ** 63:
        raise ValueError(f"M^2 (2R + 1)^4 H W with M={m}, R={max(rad)}, H={h}, W={w} reaches 2^63: the sums could overflow")


def _box_sum(a: np.ndarray, r: int) -> np.ndarray:
    """Sums over the (2r + 1)^2 squares centred on every pixel of the zero-padded planes a [..., H, W] (int64): a padded double cumsum."""
    if r == 0:
        return a
    side = 2 * r + 1
    p = np.pad(a, [(0, 0)] * (a.ndim - 2) + [(r + 1, r), (r + 1, r)])
    c = p.cumsum(axis=-2).cumsum(axis=-1)
    return c[..., side:, side:] - c[..., :-side, side:] - c[..., side:, :-side] + c[..., :-side, :-side]


def fss_sums_reference(forecast, observed, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, radii: Sequence[int] = DEFAULT_RADII):
    """The specification of `dgmr_fss_sums`, in numpy.

    forecast: fp32 [M, N, H, W]; observed: fp32 [N, H, W]; 1 <= M <= 32, H and W multiples of 16, 1 ... 8 thresholds (fp32
    comparisons), 1 ... 8 distinct radii 0 <= r <= 32 in any order.  -> (sums int64 [N, K, S, 4], events int64 [N, K, 2]), see the
    module's docstring."""
    thr, rad = _check_config(thresholds, radii)
    f = np.asarray(forecast, dtype=np.float32)
    o = np.asarray(observed, dtype=np.float32)
    if f.ndim != 4 or o.shape != f.shape[1:]:
        raise ValueError(f"forecast must be [M, N, H, W] and observed [N, H, W], got {f.shape} and {o.shape}")
    m, n, h, w = f.shape
    _check_shape(m, h, w)
    _check_overflow(m, h, w, rad)
    sums = np.zeros((n, thr.size, len(rad), 4), np.int64)
    events = np.zeros((n, thr.size, 2), np.int64)
    with np.errstate(invalid="ignore"):
        for i in range(n):
            present = o[i] >= 0
            for k, t in enumerate(thr):
                im = ((f[:, i] >= t) & present).astype(np.int64)  # [M, H, W]
                io = ((o[i] >= t) & present).astype(np.int64)
                events[i, k] = im.sum(), io.sum()
                for s, r in enumerate(rad):
                    sm, so = _box_sum(im, r), _box_sum(io, r)
                    sf = sm.sum(axis=0)
                    sums[i, k, s] = (sf * sf).sum(), (so * so).sum(), (sf * so).sum(), (sm * sm).sum()
    return sums, events


def fss_sums(forecast: torch.Tensor, observed: torch.Tensor, thresholds: Sequence[float] = DEFAULT_THRESHOLDS,
             radii: Sequence[int] = DEFAULT_RADII):
    """`fss_sums_reference` as int64 tensors (sums [N, K, S, 4], events [N, K, 2]) on the inputs' device.

    forecast: fp32 [M, N, H, W], or with the plane dimensions unflattened ([M, B, T, C, H, W], ...); observed: the forecast's shape
    without M; planes are numbered in row-major order.  On a HIP device this is `dgmr_fss_sums` on the current stream, without
    synchronisation; the forecast is read in place when each member is one contiguous block, whatever the member stride (any other
    layout is copied first).  CPU tensors go through the reference."""
    thr, rad = _check_config(thresholds, radii)
    if forecast.dim() < 3 or tuple(forecast.shape[1:]) != tuple(observed.shape):
        raise ValueError(f"forecast must be [M, ..., H, W] and observed [..., H, W], got {tuple(forecast.shape)} and {tuple(observed.shape)}")
    m, h, w = (int(v) for v in (forecast.shape[0], forecast.shape[-2], forecast.shape[-1]))
    _check_shape(m, h, w)
    _check_overflow(m, h, w, rad)
    n = int(np.prod(forecast.shape[1:-2], dtype=np.int64))
    if n < 1:
        raise ValueError(f"forecast {tuple(forecast.shape)} holds no plane")
    if forecast.dtype != torch.float32 or observed.dtype != torch.float32:
        raise ValueError(f"forecast ({forecast.dtype}) and observed ({observed.dtype}) must be float32")
    if forecast.device != observed.device:
        raise ValueError(f"forecast ({forecast.device}) and observed ({observed.device}) are on different devices")
    if not forecast.is_cuda:
        sums, events = fss_sums_reference(forecast.reshape(m, n, h, w).numpy(), observed.reshape(n, h, w).numpy(), thr, rad)
        return torch.from_numpy(sums), torch.from_numpy(events)
    from ._lib import call

    device = forecast.device
    with torch.cuda.device(device):
        if not _planes_contiguous(forecast) or forecast.data_ptr() % 16 or (m > 1 and forecast.stride(0) % 4):
            forecast = forecast.contiguous()
            if forecast.data_ptr() % 16:
                forecast = forecast.clone(memory_format=torch.contiguous_format)
        if not observed.is_contiguous() or observed.data_ptr() % 16:
            observed = observed.clone(memory_format=torch.contiguous_format)
        sums = torch.empty((n, int(thr.size), len(rad), 4), dtype=torch.int64, device=device)
        events = torch.empty((n, int(thr.size), 2), dtype=torch.int64, device=device)
        dev_thr = _device_thresholds(device, thr)
        call("dgmr_fss_sums", forecast.data_ptr(), forecast.stride(0) if m > 1 else 0, observed.data_ptr(), m, n, h, w,
             dev_thr.data_ptr(), int(thr.size), (ctypes.c_int * len(rad))(*rad), len(rad), sums.data_ptr(), events.data_ptr(),
             ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return sums, events


class FractionsVerifier:
    """Accumulate `fss_sums` per lead time over cases (and channels), on the device, and turn the sums into fractions skill scores.

    num_members: M (1: the classical deterministic FSS); lead_times: the number of forecast steps T (or a sequence of their labels);
    thresholds: 1 ... 8 rain rates; radii: 1 ... 8 distinct neighbourhood radii 0 ... 32 (side 2r + 1).  The accumulators (float64
    sums [T, K, S, 4], events [T, K, 2] and pixels [T]: a case's counts are multiplied by its weight) live on the device of the first
    `update`."""

    def __init__(self, num_members: int, lead_times, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, radii: Sequence[int] = DEFAULT_RADII):
        self.num_members = int(num_members)
        self.lead_times = int(lead_times) if isinstance(lead_times, (int, np.integer)) else len(tuple(lead_times))
        self._thr, self.radii = _check_config(thresholds, radii)
        self.thresholds = tuple(float(t) for t in self._thr)
        if not 1 <= self.num_members <= MAX_MEMBERS:
            raise ValueError(f"{num_members} ensemble members, 1 ... {MAX_MEMBERS} are supported")
        if self.lead_times < 1:
            raise ValueError(f"lead_times={lead_times}: at least one lead time is required")
        self._sums = self._events = self._pixels = None

    def _config(self):
        return self.num_members, self.lead_times, self.thresholds, self.radii

    def _allocate(self, device) -> None:
        t, k, s = self.lead_times, self._thr.size, len(self.radii)
        self._sums = torch.zeros((t, k, s, 4), dtype=torch.float64, device=device)
        self._events = torch.zeros((t, k, 2), dtype=torch.float64, device=device)
        self._pixels = torch.zeros((t,), dtype=torch.float64, device=device)

    def update(self, forecast: torch.Tensor, observed: torch.Tensor, weights=None) -> None:
        """forecast [M, T, C, H, W] with observed [T, C, H, W] (one case; `weights`: None or one value), or forecast [M, B, T, C, H, W]
        with observed [B, T, C, H, W] and `weights` [B] (None: ones), as in `NowcastVerifier.update`.  One `fss_sums` call over all
        B * T * C planes.  Nothing is synchronised."""
        if forecast.dim() == 5:
            forecast, observed = forecast.unsqueeze(1), observed.unsqueeze(0)
        if forecast.dim() != 6 or observed.dim() != 5:
            raise ValueError(f"forecast must be [M, T, C, H, W] or [M, B, T, C, H, W], got {tuple(forecast.shape)}")
        m, b, t, c, h, w_px = (int(v) for v in forecast.shape)
        if m != self.num_members or t != self.lead_times:
            raise ValueError(f"forecast {tuple(forecast.shape)}: {self.num_members} members and {self.lead_times} lead times are expected")
        device = forecast.device
        if weights is None:
            w = torch.ones(b, dtype=torch.float64, device=device)
        else:
            w = torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
            if w.numel() != b:
                raise ValueError(f"{w.numel()} weights for {b} cases")
            if w.device != device:
                w = w.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else w.to(device)
        sums, events = fss_sums(forecast, observed, self._thr, self.radii)
        if self._sums is None:
            self._allocate(device)
        acc = self._sums.device
        for dst, src in ((self._sums, sums), (self._events, events)):
            v = src.view(b, t, c, -1).to(torch.float64) * w.view(b, 1, 1, 1)
            dst.view(t, -1).add_(v.sum(dim=(0, 2)).to(acc))
        self._pixels.add_((w.sum() * float(c * h * w_px)).to(acc))

    def merge(self, other: "FractionsVerifier") -> None:
        """Add another verifier's accumulators (another rank's, another shard's) to this one's."""
        if other._config() != self._config():
            raise ValueError("merge: the other verifier has a different configuration")
        if other._sums is None:
            return
        if self._sums is None:
            self._allocate(other._sums.device)
        for dst, src in ((self._sums, other._sums), (self._events, other._events), (self._pixels, other._pixels)):
            dst.add_(src.to(dst.device))

    def reset(self) -> None:
        for a in (self._sums, self._events, self._pixels):
            if a is not None:
                a.zero_()

    def compute(self) -> dict:
        """The one call that brings results to the host.  -> dict of numpy arrays; K = thresholds, S = radii, T = lead times:
          fss -> [K, S, T]             2 (fo / M) / (ff / M^2 + oo): the FSS of the ensemble's neighbourhood probability
          fss_members -> [K, S, T]     2 (fo / M) / (mm / M + oo): the members as deterministic forecasts, pooled (not the mean of
                                       the members' scores)
          base_rate -> [K, T]          observed events / pixels (a missing pixel is a pixel without an event)
          forecast_rate -> [K, T]      forecast events / (M pixels)
          frequency_bias -> [K, T]     forecast_rate / base_rate
          fss_random -> [K, T]         base_rate: the score of a random forecast with the observed event share
          fss_useful -> [K, T]         0.5 + base_rate / 2
          skilful_side -> [K, T]       the smallest side 2r + 1 among the configured radii with fss >= fss_useful; NaN if none
          sides -> [S]                 2r + 1 in the configured order
          thresholds -> [K]
        Entries with a zero denominator are NaN."""
        m = float(self.num_members)
        t, k, s = self.lead_times, self._thr.size, len(self.radii)
        if self._sums is None:
            sums, events, pixels = np.zeros((t, k, s, 4)), np.zeros((t, k, 2)), np.zeros(t)
        else:
            sums, events, pixels = (a.cpu().numpy() for a in (self._sums, self._events, self._pixels))
        sums = np.transpose(sums, (1, 2, 3, 0))     # [K, S, 4, T]
        events = np.transpose(events, (1, 2, 0))    # [K, 2, T]
        ff, oo, fo, mm = (sums[:, :, q] for q in range(4))
        sides = np.asarray([2 * r + 1 for r in self.radii], dtype=np.int64)

        def ratio(num, den):
            ok = den != 0
            return np.where(ok, num / np.where(ok, den, 1.0), np.nan)

        fss = ratio(2.0 * fo / m, ff / (m * m) + oo)
        base = ratio(events[:, 1], pixels[None, :] * np.ones_like(events[:, 1]))
        rate = ratio(events[:, 0], m * pixels[None, :] * np.ones_like(events[:, 0]))
        useful = 0.5 + base / 2.0
        with np.errstate(invalid="ignore"):
            reached = fss >= useful[:, None, :]      # (False where either is NaN)
        side = np.where(reached, sides[None, :, None].astype(np.float64), np.inf).min(axis=1)
        return {"fss": fss, "fss_members": ratio(2.0 * fo / m, mm / m + oo), "base_rate": base, "forecast_rate": rate,
                "frequency_bias": ratio(rate, base), "fss_random": base.copy(), "fss_useful": useful,
                "skilful_side": np.where(np.isfinite(side), side, np.nan), "sides": sides,
                "thresholds": np.asarray(self.thresholds, dtype=np.float64)}


def skill_score_fss(metrics: dict, baseline_metrics: dict) -> dict:
    """A forecast's `FractionsVerifier.compute()` result against a baseline's over the same cases, thresholds and radii:
      fss, fss_members -> [K, S, T]   fss - fss_baseline: positive where the forecast beats the baseline
      sides -> [S]"""
    a, b = np.asarray(metrics["sides"]), np.asarray(baseline_metrics["sides"])
    if a.shape != b.shape or (a != b).any():
        raise ValueError(f"skill_score_fss: sides {a.tolist()} against the baseline's {b.tolist()}")
    ta, tb = np.asarray(metrics["thresholds"]), np.asarray(baseline_metrics["thresholds"])
    if ta.shape != tb.shape or (ta != tb).any():
        raise ValueError(f"skill_score_fss: thresholds {ta.tolist()} against the baseline's {tb.tolist()}")
    if np.shape(metrics["fss"]) != np.shape(baseline_metrics["fss"]):
        raise ValueError(f"skill_score_fss: fss {np.shape(metrics['fss'])} against the baseline's {np.shape(baseline_metrics['fss'])}")
    return {"fss": np.asarray(metrics["fss"]) - np.asarray(baseline_metrics["fss"]),
            "fss_members": np.asarray(metrics["fss_members"]) - np.asarray(baseline_metrics["fss_members"]), "sides": a.copy()}
