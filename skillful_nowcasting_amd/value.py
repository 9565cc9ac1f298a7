"""Reliability, Brier score, ROC points and economic value of ensemble nowcasts (the paper's decision-making argument).

All four derive from one table of counts.  For M members, a threshold `thr` and the present pixels of a plane (an observed element is
missing when `!(y >= 0)`, as everywhere in the verification), `table[j][o]` counts the pixels at which exactly j members are `>= thr`
and the observation is (`o = 1`) or is not (`o = 0`) `>= thr`.  The ensemble's forecast probability at such a pixel is j / M.

`exceedance_table_reference` is the specification in numpy.  On a HIP device `exceedance_table` is `dgmr_exceedance_table`
(csrc/verify.hip): one streaming read of the ensemble and the observation, integer counts, exact.  `ValueVerifier` accumulates the
tables per lead time on the device, weighted by the cases' inverse inclusion probabilities, and has `NowcastVerifier`'s `update`, so
`DGMR.verify_batch(batch, ValueVerifier(...))` works; `compute()` turns the sums into the metrics on the host.  Grid scale only: no
pooled-scale economic value.
"""
from __future__ import annotations

import ctypes
from typing import Sequence

import numpy as np
import torch

from .verification import DEFAULT_THRESHOLDS, MAX_MEMBERS, MAX_THRESHOLDS, _check_shape, _device_thresholds, _planes_contiguous


def _check_thresholds(thresholds) -> np.ndarray:
    thr = np.asarray(tuple(thresholds), dtype=np.float32).reshape(-1)
    if thr.size > MAX_THRESHOLDS:
        raise ValueError(f"{thr.size} thresholds, at most {MAX_THRESHOLDS} are supported")
    return thr


def exceedance_table_reference(forecast, observed, thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> np.ndarray:
    """The specification of `dgmr_exceedance_table`, in numpy.

    forecast: fp32 [M, N, H, W]; observed: fp32 [N, H, W]; 1 <= M <= 32, H and W multiples of 16, at most 8 thresholds, fp32
    comparisons.  -> table int64 [N, K, M + 1, 2]: per plane and threshold, the present pixels with exactly j members `>= thr` and the
    observation `>= thr` (o = 1) or not (o = 0)."""
    thr = _check_thresholds(thresholds)
    f = np.asarray(forecast, dtype=np.float32)
    o = np.asarray(observed, dtype=np.float32)
    if f.ndim != 4 or o.shape != f.shape[1:]:
        raise ValueError(f"forecast must be [M, N, H, W] and observed [N, H, W], got {f.shape} and {o.shape}")
    m, n, h, w = f.shape
    _check_shape(m, h, w)
    table = np.zeros((n, thr.size, m + 1, 2), np.int64)
    with np.errstate(invalid="ignore"):
        present = o >= 0
        for k, t in enumerate(thr):
            key = (f >= t).sum(axis=0) * 2 + (o >= t)
            for i in range(n):
                table[i, k] = np.bincount(key[i][present[i]], minlength=2 * (m + 1)).reshape(m + 1, 2)
    return table


def exceedance_table(forecast: torch.Tensor, observed: torch.Tensor, thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> torch.Tensor:
    """`exceedance_table_reference` as an int64 tensor [N, K, M + 1, 2] on the inputs' device.

    forecast: fp32 [M, N, H, W], or with the plane dimensions unflattened ([M, B, T, C, H, W], ...); observed: the forecast's shape
    without M; planes are numbered in row-major order.  On a HIP device this is `dgmr_exceedance_table` on the current stream, without
    synchronisation; the forecast is read in place when each member is one contiguous block, whatever the member stride (any other
    layout is copied first).  CPU tensors go through the reference."""
    thr = _check_thresholds(thresholds)
    if forecast.dim() < 3 or tuple(forecast.shape[1:]) != tuple(observed.shape):
        raise ValueError(f"forecast must be [M, ..., H, W] and observed [..., H, W], got {tuple(forecast.shape)} and {tuple(observed.shape)}")
    m, h, w = (int(v) for v in (forecast.shape[0], forecast.shape[-2], forecast.shape[-1]))
    _check_shape(m, h, w)
    n = int(np.prod(forecast.shape[1:-2], dtype=np.int64))
    if n < 1:
        raise ValueError(f"forecast {tuple(forecast.shape)} holds no plane")
    if forecast.dtype != torch.float32 or observed.dtype != torch.float32:
        raise ValueError(f"forecast ({forecast.dtype}) and observed ({observed.dtype}) must be float32")
    if forecast.device != observed.device:
        raise ValueError(f"forecast ({forecast.device}) and observed ({observed.device}) are on different devices")
    if not forecast.is_cuda:
        return torch.from_numpy(exceedance_table_reference(forecast.reshape(m, n, h, w).numpy(), observed.reshape(n, h, w).numpy(), thr))
    from ._lib import call

    device = forecast.device
    with torch.cuda.device(device):
        if not _planes_contiguous(forecast) or forecast.data_ptr() % 16 or (m > 1 and forecast.stride(0) % 4):
            forecast = forecast.contiguous()
            if forecast.data_ptr() % 16:
                forecast = forecast.clone(memory_format=torch.contiguous_format)
        if not observed.is_contiguous() or observed.data_ptr() % 16:
            observed = observed.clone(memory_format=torch.contiguous_format)
        table = torch.empty((n, int(thr.size), m + 1, 2), dtype=torch.int64, device=device)
        dev_thr = _device_thresholds(device, thr)
        call("dgmr_exceedance_table", forecast.data_ptr(), forecast.stride(0) if m > 1 else 0, observed.data_ptr(), m, n, h, w,
             dev_thr.data_ptr(), int(thr.size), table.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return table


DEFAULT_COST_LOSS = np.linspace(0.01, 0.99, 99)


class ValueVerifier:
    """Accumulate `exceedance_table` per lead time over cases (and channels), on the device, and turn the sums into reliability,
    Brier score, ROC points and relative economic value.

    num_members: M; lead_times: the number of forecast steps T (or a sequence of their labels); thresholds: at most 8 rain rates.  The
    accumulator (float64 [T, K, M + 1, 2]: a case's table is multiplied by its weight) lives on the device of the first `update`."""

    def __init__(self, num_members: int, lead_times, thresholds: Sequence[float] = DEFAULT_THRESHOLDS):
        self.num_members = int(num_members)
        self.lead_times = int(lead_times) if isinstance(lead_times, (int, np.integer)) else len(tuple(lead_times))
        self._thr = _check_thresholds(thresholds)
        self.thresholds = tuple(float(t) for t in self._thr)
        if not 1 <= self.num_members <= MAX_MEMBERS:
            raise ValueError(f"{num_members} ensemble members, 1 ... {MAX_MEMBERS} are supported")
        if self.lead_times < 1:
            raise ValueError(f"lead_times={lead_times}: at least one lead time is required")
        self._acc = None

    def _zeros(self, device) -> torch.Tensor:
        return torch.zeros((self.lead_times, self._thr.size, self.num_members + 1, 2), dtype=torch.float64, device=device)

    def update(self, forecast: torch.Tensor, observed: torch.Tensor, weights=None) -> None:
        """forecast [M, T, C, H, W] with observed [T, C, H, W] (one case; `weights`: None or one value), or forecast [M, B, T, C, H, W]
        with observed [B, T, C, H, W] and `weights` [B] (None: ones), as in `NowcastVerifier.update`.  One `exceedance_table` call
        over all B * T * C planes.  Nothing is synchronised."""
        if forecast.dim() == 5:
            forecast, observed = forecast.unsqueeze(1), observed.unsqueeze(0)
        if forecast.dim() != 6 or observed.dim() != 5:
            raise ValueError(f"forecast must be [M, T, C, H, W] or [M, B, T, C, H, W], got {tuple(forecast.shape)}")
        m, b, t, c = (int(v) for v in forecast.shape[:4])
        if m != self.num_members or t != self.lead_times:
            raise ValueError(f"forecast {tuple(forecast.shape)}: {self.num_members} members and {self.lead_times} lead times are expected")
        device = forecast.device
        w = None
        if weights is not None:
            w = torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
            if w.numel() != b:
                raise ValueError(f"{w.numel()} weights for {b} cases")
            if w.device != device:
                w = w.pin_memory().to(device, non_blocking=True) if device.type == "cuda" else w.to(device)
        table = exceedance_table(forecast, observed, self._thr)
        if self._acc is None:
            self._acc = self._zeros(device)
        v = table.view(b, t, c, -1).to(torch.float64)
        if w is not None:
            v = v * w.view(b, 1, 1, 1)
        self._acc.view(t, -1).add_(v.sum(dim=(0, 2)).to(self._acc.device))

    def merge(self, other: "ValueVerifier") -> None:
        """Add another verifier's accumulator (another rank's, another shard's) to this one's."""
        if (other.num_members, other.lead_times, other.thresholds) != (self.num_members, self.lead_times, self.thresholds):
            raise ValueError("merge: the other verifier has a different configuration")
        if other._acc is None:
            return
        if self._acc is None:
            self._acc = self._zeros(other._acc.device)
        self._acc.add_(other._acc.to(self._acc.device))

    def reset(self) -> None:
        if self._acc is not None:
            self._acc.zero_()

    def compute(self, cost_loss=DEFAULT_COST_LOSS) -> dict:
        """The one call that brings results to the host.  -> dict of numpy arrays; T = lead times, K = thresholds, A = cost/loss ratios:
          base_rate -> [K, T]                  s: the share of present pixels at which the observation reaches the threshold
          hit_rate, false_alarm_rate -> [K, M, T]   of the decision rules "act when at least j of M members exceed", j = 1 ... M (the
                                               ROC points; index j - 1)
          reliability -> {"observed_frequency": [K, M + 1, T], "count": [K, M + 1, T]}   per forecast probability j / M
          forecast_probability -> [M + 1]      j / M
          brier -> [K, T]                      sum_j sum_o table (j / M - o)^2 / sum table
          cost_loss -> [A]
          value[threshold] -> [T, A]           max over the rules j of
                                               V_j(a) = (min(a, s) - F a (1 - s) + H s (1 - a) - s) / (min(a, s) - s a);
                                               NaN where s is 0 or 1 (or nothing was accumulated)
        Entries without pixels are NaN."""
        acc = self._acc if self._acc is not None else self._zeros(torch.device("cpu"))
        tab = np.transpose(acc.cpu().numpy(), (1, 2, 3, 0))  # [K, M + 1, 2, T]
        m = self.num_members
        alpha = np.asarray(cost_loss, dtype=np.float64).reshape(-1)
        prob = np.arange(m + 1, dtype=np.float64) / m
        with np.errstate(divide="ignore", invalid="ignore"):
            total = tab.sum(axis=(1, 2))                       # [K, T]
            wet, dry = tab[:, :, 1].sum(axis=1), tab[:, :, 0].sum(axis=1)
            base = wet / total
            # rule j: act where at least j members exceed - the cumulative sums from the top
            acted = np.flip(np.cumsum(np.flip(tab, axis=1), axis=1), axis=1)[:, 1:]  # [K, M, 2, T], j = 1 ... M
            hit = acted[:, :, 1] / wet[:, None, :]
            far = acted[:, :, 0] / dry[:, None, :]
            count = tab.sum(axis=2)                            # [K, M + 1, T]
            brier = (tab[:, :, 0] * (prob ** 2)[None, :, None] + tab[:, :, 1] * ((prob - 1.0) ** 2)[None, :, None]).sum(axis=1) / total
            res = {"base_rate": base, "hit_rate": hit, "false_alarm_rate": far,
                   "reliability": {"observed_frequency": tab[:, :, 1] / count, "count": count},
                   "forecast_probability": prob, "brier": brier, "cost_loss": alpha.copy(), "value": {}}
            for k, t in enumerate(self.thresholds):
                s = base[k][None, :, None]                      # [1, T, 1]
                a = alpha[None, None, :]                        # [1, 1, A]
                h, f = hit[k][:, :, None], far[k][:, :, None]   # [M, T, 1]
                v = (np.minimum(a, s) - f * a * (1.0 - s) + h * s * (1.0 - a) - s) / (np.minimum(a, s) - s * a)
                best = np.max(v, axis=0)                        # (NaN wherever s is NaN, 0 or 1: hit or far are 0 / 0 there)
                best[np.broadcast_to(~((s[0] > 0) & (s[0] < 1)), best.shape)] = np.nan
                res["value"][t] = best
        return res
