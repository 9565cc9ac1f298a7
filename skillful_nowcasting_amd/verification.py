"""Verification of ensemble nowcasts: pooled CRPS, CSI and the rank table (how the paper judges DGMR).

`validation_step` returns the three GAN losses, which do not rank generators.  What does is computed here, per plane - a plane is one
`(case, lead time, channel)` - from M ensemble members and one observation:

  * `cells`, `abs_err`, `pair`: the two sums the ensemble CRPS is made of, at the grid scale and average- / max-pooled over
    non-overlapping s x s cells:  CRPS = abs_err / cells - pair / (M^2 cells),  fair CRPS = abs_err / cells - pair / (M (M - 1) cells);
  * `contingency`: hits, misses and false alarms per threshold and member (CSI = hits / (hits + misses + false alarms));
  * `ranks`: how many members lie below and how many tie with the observation, as an exact table (radar fields are mostly ties -
    zeros - and resolving them at random would make the result irreproducible; the rank histogram is derived from the table).

`ensemble_scores_reference` is the specification in numpy.  On a HIP device `ensemble_scores` is `dgmr_ensemble_scores` (csrc/verify.hip):
one streaming read of the ensemble and the observation for all scales, both poolings and all five outputs; nothing pooled and no
per-pair temporary goes to memory.  `NowcastVerifier` accumulates the per-plane results per lead time on the device, weighted by the
cases' inverse inclusion probabilities, and `compute()` turns them into the metrics on the host.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Optional, Sequence

import numpy as np
import torch

ALLOWED_SCALES = (1, 2, 4, 8, 16)
DEFAULT_SCALES = (1, 4, 16)
DEFAULT_THRESHOLDS = (1.0, 4.0, 8.0)  # mm/h
MAX_MEMBERS = 32
MAX_THRESHOLDS = 8
POOLS = ("avg", "max")

EnsembleScores = namedtuple("EnsembleScores", ["cells", "abs_err", "pair", "contingency", "ranks"])


def _check_config(scales, thresholds):
    scales = tuple(int(s) for s in scales)
    if not scales or any(s not in ALLOWED_SCALES for s in scales) or len(set(scales)) != len(scales):
        raise ValueError(f"scales={scales}: distinct values out of {ALLOWED_SCALES} are required")
    thr = np.asarray(tuple(thresholds), dtype=np.float32).reshape(-1)
    if thr.size > MAX_THRESHOLDS:
        raise ValueError(f"{thr.size} thresholds, at most {MAX_THRESHOLDS} are supported")
    return scales, thr


def _check_shape(m: int, h: int, w: int):
    if not 1 <= m <= MAX_MEMBERS:
        raise ValueError(f"{m} ensemble members, 1 ... {MAX_MEMBERS} are supported")
    if h < 16 or w < 16 or h % 16 or w % 16:
        raise ValueError(f"H={h} and W={w} must be positive multiples of 16")


def _down_sum(a):
    """One pooling level: (top-left + top-right) + (bottom-left + bottom-right), the order the kernel's butterflies use."""
    return (a[..., 0::2, 0::2] + a[..., 0::2, 1::2]) + (a[..., 1::2, 0::2] + a[..., 1::2, 1::2])


def _down_max(a):
    return np.maximum(np.maximum(a[..., 0::2, 0::2], a[..., 0::2, 1::2]), np.maximum(a[..., 1::2, 0::2], a[..., 1::2, 1::2]))


def _down_all(a):
    return a[..., 0::2, 0::2] & a[..., 0::2, 1::2] & a[..., 1::2, 0::2] & a[..., 1::2, 1::2]


def ensemble_scores_reference(forecast, observed, scales: Sequence[int] = DEFAULT_SCALES,
                              thresholds: Sequence[float] = DEFAULT_THRESHOLDS) -> EnsembleScores:
    """The specification of `dgmr_ensemble_scores`, in numpy.

    forecast: fp32 [M, N, H, W], M ensemble members of N planes; observed: fp32 [N, H, W] in the same unit.  An observed element is
    missing when `!(y >= 0)` (negative, -inf, NaN: the loader's rule); forecast values are taken as they are.  1 <= M <= 32; H and W
    multiples of 16.  Per plane, nothing divided or averaged over planes:

      cells[N, S]              int64    the non-overlapping s x s cells (stride s) whose s^2 observed elements are all present
      abs_err[N, 2, S]         float64  sum over those cells of (1 / M) sum_m |x_m - y|, x_m and y the pooled member and observation:
                                        [:, 0] average pooling (float64 sum of the s^2 fp32 values / s^2, kept in float64), [:, 1] max
      pair[N, 2, S]            float64  sum over those cells of sum_{m<k} |x_m - x_k|   (at s = 1 the two rows are the same numbers)
      contingency[N, K, M, 3]  int64    grid scale, present pixels: hits (x >= thr, y >= thr), misses (x < thr, y >= thr), false alarms
                                        (x >= thr, y < thr), compared in fp32
      ranks[N, M + 1, M + 1]   int64    grid scale, present pixels: [b, e] counts b = #{m: x_m < y}, e = #{m: x_m == y}
    """
    scales, thr = _check_config(scales, thresholds)
    f = np.asarray(forecast, dtype=np.float32)
    o = np.asarray(observed, dtype=np.float32)
    if f.ndim != 4 or o.shape != f.shape[1:]:
        raise ValueError(f"forecast must be [M, N, H, W] and observed [N, H, W], got {f.shape} and {o.shape}")
    m, n, h, w = f.shape
    _check_shape(m, h, w)
    s_n, k_n = len(scales), thr.size
    cells = np.zeros((n, s_n), np.int64)
    abs_err = np.zeros((n, 2, s_n), np.float64)
    pair = np.zeros((n, 2, s_n), np.float64)
    contingency = np.zeros((n, k_n, m, 3), np.int64)
    ranks = np.zeros((n, m + 1, m + 1), np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        present = o >= 0
        levels = [(f.astype(np.float64), o.astype(np.float64), f, o, present)]
        for _ in range(max(scales).bit_length() - 1):
            fa, oa, fm, om, pr = levels[-1]
            levels.append((_down_sum(fa), _down_sum(oa), _down_max(fm), _down_max(om), _down_all(pr)))
        for si, s in enumerate(scales):
            fa, oa, fm, om, pr = levels[s.bit_length() - 1]
            inv = 1.0 / (s * s)  # (a power of two: exact)
            cells[:, si] = pr.reshape(n, -1).sum(axis=1)
            for pool, (x, y) in enumerate(((fa * inv, oa * inv), (fm.astype(np.float64), om.astype(np.float64)))):
                if s == 1 and pool == 1:
                    abs_err[:, 1, si], pair[:, 1, si] = abs_err[:, 0, si], pair[:, 0, si]
                    continue
                a, p = np.zeros(y.shape, np.float64), np.zeros(y.shape, np.float64)
                for i in range(m):  # members in index order, pairs in (i, j) lexicographic order
                    a += np.abs(x[i] - y)
                    for j in range(i + 1, m):
                        p += np.abs(x[i] - x[j])
                abs_err[:, pool, si] = np.where(pr, a / m, 0.0).reshape(n, -1).sum(axis=1)
                pair[:, pool, si] = np.where(pr, p, 0.0).reshape(n, -1).sum(axis=1)
        for k, t in enumerate(thr):
            wet = present & (o >= t)
            dry = present & ~wet
            ge, lt = f >= t, f < t
            contingency[:, k, :, 0] = (ge & wet).reshape(m, n, -1).sum(axis=2).T
            contingency[:, k, :, 1] = (lt & wet).reshape(m, n, -1).sum(axis=2).T
            contingency[:, k, :, 2] = (ge & dry).reshape(m, n, -1).sum(axis=2).T
        key = (f < o).sum(axis=0) * (m + 1) + (f == o).sum(axis=0)
        for i in range(n):
            ranks[i] = np.bincount(key[i][present[i]], minlength=(m + 1) ** 2).reshape(m + 1, m + 1)
    return EnsembleScores(cells, abs_err, pair, contingency, ranks)


# ---- the device path -------------------------------------------------------------------------------------------------------------
# Both caches live as long as the process and never shrink: one workspace per (device, stream) that ever called - its largest size so
# far, a few hundred KB for the scores (spectra.radial_psd shares it: up to 64 MiB with 256- or 512-pixel windows) - and one tensor of at most 8 floats per (device, distinct thresholds).  A process uses a handful of either.
_WORKSPACES = {}  # (device index, stream) -> uint8 tensor; a launch sequence owns it until the stream has run it
_THRESHOLDS = {}  # (device index, threshold bytes) -> (device tensor, upload event, stream of the upload)


def _workspace(device, nbytes: int) -> torch.Tensor:
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WORKSPACES.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=device)
        _WORKSPACES[key] = ws
    return ws


def _device_thresholds(device, thr: np.ndarray) -> torch.Tensor:
    """The thresholds on the device: uploaded once per (device, values) from pinned memory, without a host wait."""
    key = (device.index, thr.tobytes())
    stream = torch.cuda.current_stream(device)
    hit = _THRESHOLDS.get(key)
    if hit is None:
        dev = torch.from_numpy(thr.copy() if thr.size else np.zeros(1, np.float32)).pin_memory().to(device, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
        hit = _THRESHOLDS[key] = (dev, ev, stream.cuda_stream)
    elif hit[2] != stream.cuda_stream:
        stream.wait_event(hit[1])
    return hit[0]


def _planes_contiguous(t: torch.Tensor) -> bool:
    """Are the dimensions behind the first laid out as one contiguous block (a member is [N][H][W] in memory)?"""
    want = 1
    for size, stride in zip(reversed(t.shape[1:]), reversed(t.stride()[1:])):
        if size != 1 and stride != want:
            return False
        want *= size
    return True


def _out_shapes(n, m, s_n, k_n):
    return EnsembleScores(((n, s_n), torch.int64), ((n, 2, s_n), torch.float64), ((n, 2, s_n), torch.float64),
                          ((n, k_n, m, 3), torch.int64), ((n, m + 1, m + 1), torch.int64))


def ensemble_scores(forecast: torch.Tensor, observed: torch.Tensor, scales: Sequence[int] = DEFAULT_SCALES,
                    thresholds: Sequence[float] = DEFAULT_THRESHOLDS, out: Optional[EnsembleScores] = None) -> EnsembleScores:
    """The five per-plane results of `ensemble_scores_reference` as tensors on the inputs' device.

    forecast: fp32 [M, N, H, W], or with the plane dimensions unflattened ([M, T, C, H, W], [M, B, T, C, H, W], ...); observed: fp32, the
    forecast's shape without M.  Planes are numbered in row-major order of the plane dimensions.  On a HIP device this is
    `dgmr_ensemble_scores` on the current stream, without synchronisation; the forecast is read in place when each member is one
    contiguous block - what `DGMR.sample`, `DGMR.nowcast_full_frame` and a view of one case `out[:, b]` give - whatever the member
    stride (any other layout is copied first).  The workspace is cached per (device, stream), the thresholds are uploaded once per
    (device, values).  CPU tensors go through the reference.  `out`: an `EnsembleScores` of a previous call with the same shapes."""
    scales, thr = _check_config(scales, thresholds)
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
    shapes = _out_shapes(n, m, len(scales), thr.size)
    if out is not None:
        for name, t, (shape, dtype) in zip(EnsembleScores._fields, out, shapes):
            if tuple(t.shape) != shape or t.dtype != dtype or not t.is_contiguous() or t.device != forecast.device:
                raise ValueError(f"out.{name} must be a contiguous {dtype} {shape} tensor on {forecast.device}")
    if not forecast.is_cuda:
        ref = ensemble_scores_reference(forecast.reshape(m, n, h, w).numpy(), observed.reshape(n, h, w).numpy(), scales, thr)
        res = EnsembleScores(*(torch.from_numpy(np.ascontiguousarray(a)) for a in ref))
        if out is None:
            return res
        for dst, src in zip(out, res):
            dst.copy_(src)
        return out
    from ._lib import call, load

    device = forecast.device
    with torch.cuda.device(device):
        if not _planes_contiguous(forecast) or forecast.data_ptr() % 16 or (m > 1 and forecast.stride(0) % 4):
            forecast = forecast.contiguous()
            if forecast.data_ptr() % 16:
                forecast = forecast.clone(memory_format=torch.contiguous_format)
        if not observed.is_contiguous() or observed.data_ptr() % 16:
            observed = observed.clone(memory_format=torch.contiguous_format)
        if out is None:
            out = EnsembleScores(*(torch.empty(shape, dtype=dtype, device=device) for shape, dtype in shapes))
        nbytes = int(load().dgmr_ensemble_scores_workspace(m, n, h, w))
        if nbytes < 0:
            raise ValueError(f"dgmr_ensemble_scores_workspace refused M={m}, N={n}, H={h}, W={w}")
        ws = _workspace(device, nbytes)
        dev_thr = _device_thresholds(device, thr)
        c_scales = (ctypes.c_int * len(scales))(*scales)
        call("dgmr_ensemble_scores", forecast.data_ptr(), forecast.stride(0) if m > 1 else 0, observed.data_ptr(), m, n, h, w, c_scales,
             len(scales), dev_thr.data_ptr(), int(thr.size), ws.data_ptr(), ws.numel(), out.cells.data_ptr(), out.abs_err.data_ptr(),
             out.pair.data_ptr(), out.contingency.data_ptr(), out.ranks.data_ptr(),
             ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream))
    return out


def observed_from_frames(frames, scale: float = 1.0, offset: float = 0.0) -> torch.Tensor:
    """Stored frames [T, H, W, C] (numpy or torch; uint8 / int16 / float16 / float32) -> the fp32 physical value [T, C, H, W] =
    `raw.float() * scale + offset` (two rounded fp32 operations, as the loaders and kernels form it), contiguous, on the frames'
    device.  Nothing is clamped: a missing element (`!(x >= 0)`) stays missing, which is what the verification needs to see."""
    if isinstance(frames, np.ndarray):
        frames = torch.from_numpy(np.ascontiguousarray(frames))
    if frames.dim() != 4:
        raise ValueError(f"frames must be [T, H, W, C], got shape {tuple(frames.shape)}")
    return (frames.permute(0, 3, 1, 2).float() * float(scale) + float(offset)).contiguous()


class NowcastVerifier:
    """Accumulate `ensemble_scores` per lead time over cases (and channels), on the device, and turn the sums into metrics.

    num_members: M; lead_times: the number of forecast steps T (or a sequence of their labels); scales / thresholds as in
    `ensemble_scores`.  The accumulators (float64: a case's contribution is multiplied by its weight) live on the device of the
    first `update` and are sums over cases and channels."""

    def __init__(self, num_members: int, lead_times, scales: Sequence[int] = DEFAULT_SCALES,
                 thresholds: Sequence[float] = DEFAULT_THRESHOLDS):
        self.num_members = int(num_members)
        self.lead_times = int(lead_times) if isinstance(lead_times, (int, np.integer)) else len(tuple(lead_times))
        self.scales, self._thr = _check_config(scales, thresholds)
        self.thresholds = tuple(float(t) for t in self._thr)
        if not 1 <= self.num_members <= MAX_MEMBERS:
            raise ValueError(f"{num_members} ensemble members, 1 ... {MAX_MEMBERS} are supported")
        if self.lead_times < 1:
            raise ValueError(f"lead_times={lead_times}: at least one lead time is required")
        self._acc: Optional[EnsembleScores] = None

    def _zeros(self, device) -> EnsembleScores:
        shapes = _out_shapes(self.lead_times, self.num_members, len(self.scales), self._thr.size)
        return EnsembleScores(*(torch.zeros(shape, dtype=torch.float64, device=device) for shape, _ in shapes))

    def update(self, forecast: torch.Tensor, observed: torch.Tensor, weights=None) -> None:
        """forecast [M, T, C, H, W] with observed [T, C, H, W] (one case; `weights`: None or one value), or forecast [M, B, T, C, H, W]
        with observed [B, T, C, H, W] and `weights` [B] (None: ones) - the paper's 1 / q, `1.0 / loader.last_inclusion_prob`.  One
        `ensemble_scores` call over all B * T * C planes; every plane's results are multiplied by its case's weight in float64 and
        added to the lead time's accumulators.  Nothing is synchronised."""
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
        scores = ensemble_scores(forecast, observed, self.scales, self._thr)
        if self._acc is None:
            self._acc = self._zeros(device)
        for acc, s in zip(self._acc, scores):
            v = s.view(b, t, c, -1).to(torch.float64)
            if w is not None:
                v = v * w.view(b, 1, 1, 1)
            acc.view(t, -1).add_(v.sum(dim=(0, 2)).to(acc.device))

    def merge(self, other: "NowcastVerifier") -> None:
        """Add another verifier's accumulators (another rank's, another shard's) to this one's."""
        if (other.num_members, other.lead_times, other.scales, other.thresholds) != (self.num_members, self.lead_times, self.scales,
                                                                                     self.thresholds):
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
        """The one call that brings results to the host.  -> dict of numpy arrays, T = lead times:
          crps[pool][scale] -> [T]        abs_err / cells - pair / (M^2 cells), pool in ("avg", "max"); NaN where a lead time has no cell
          crps_fair[pool][scale] -> [T]   abs_err / cells - pair / (M (M - 1) cells); NaN for M = 1
          csi[threshold] -> [T]           pooled over members: sum_m hits / sum_m (hits + misses + false alarms); NaN where that is 0
          csi_members -> [K, M, T]
          rank_histogram -> [T, M + 1]    every (b, e) count spread as 1 / (e + 1) over ranks b ... b + e, normalised
          rank_histogram_wet              the same without the all-dry entry (b = 0, e = M)
          cells -> [T, S]                 the (weighted) cell counts"""
        acc = self._acc if self._acc is not None else self._zeros(torch.device("cpu"))
        cells, abs_err, pair, cont, ranks = (a.cpu().numpy() for a in acc)
        m = self.num_members
        res = {"crps": {p: {} for p in POOLS}, "crps_fair": {p: {} for p in POOLS}, "csi": {}, "cells": cells.copy()}
        with np.errstate(divide="ignore", invalid="ignore"):
            for pi, p in enumerate(POOLS):
                for si, s in enumerate(self.scales):
                    mean_abs = abs_err[:, pi, si] / cells[:, si]
                    res["crps"][p][s] = mean_abs - pair[:, pi, si] / (m * m * cells[:, si])
                    res["crps_fair"][p][s] = (mean_abs - pair[:, pi, si] / (m * (m - 1) * cells[:, si]) if m > 1
                                              else np.full(self.lead_times, np.nan))
            for k, t in enumerate(self.thresholds):
                res["csi"][t] = cont[:, k, :, 0].sum(axis=1) / cont[:, k].sum(axis=(1, 2))
            res["csi_members"] = np.transpose(cont[..., 0] / cont.sum(axis=3), (1, 2, 0))
            res["rank_histogram"] = _rank_histogram(ranks)
            wet = ranks.copy()
            wet[:, 0, m] = 0.0
            res["rank_histogram_wet"] = _rank_histogram(wet)
        return res


def _rank_histogram(ranks: np.ndarray) -> np.ndarray:
    """[T, M + 1, M + 1] (b, e) table -> [T, M + 1]: a pixel with e ties lies at each of the ranks b ... b + e with probability
    1 / (e + 1) (the expectation of resolving the ties at random), rows normalised (NaN for an empty row)."""
    m1 = ranks.shape[1]
    hist = np.zeros((ranks.shape[0], m1), np.float64)
    for b in range(m1):
        for e in range(m1 - b):
            hist[:, b:b + e + 1] += (ranks[:, b, e] / (e + 1))[:, None]
    with np.errstate(divide="ignore", invalid="ignore"):
        return hist / hist.sum(axis=1, keepdims=True)


def skill_score(metrics: dict, baseline_metrics: dict) -> dict:
    """A forecast's `NowcastVerifier.compute()` result against a baseline's (advection.py: `AdvectionNowcaster`, `persistence_nowcast`)
    over the same cases, with the same scales and thresholds:
      crps[pool][scale] -> [T]   1 - crps / crps_baseline: positive where the forecast beats the baseline, 1 for a perfect one; NaN
                                 where the baseline's CRPS is 0 or either is NaN
      csi[threshold] -> [T]      csi - csi_baseline"""
    res = {"crps": {}, "csi": {}}
    with np.errstate(divide="ignore", invalid="ignore"):
        for pool, per_scale in metrics["crps"].items():
            base = baseline_metrics["crps"][pool]
            if set(base) != set(per_scale):
                raise ValueError(f"skill_score: scales {sorted(per_scale)} against the baseline's {sorted(base)}")
            res["crps"][pool] = {}
            for s, v in per_scale.items():
                b = np.asarray(base[s], dtype=np.float64)
                res["crps"][pool][s] = np.where(b != 0, 1.0 - np.asarray(v, dtype=np.float64) / np.where(b != 0, b, 1.0), np.nan)
        if set(metrics["csi"]) != set(baseline_metrics["csi"]):
            raise ValueError(f"skill_score: thresholds {sorted(metrics['csi'])} against the baseline's {sorted(baseline_metrics['csi'])}")
        for t, v in metrics["csi"].items():
            res["csi"][t] = np.asarray(v, dtype=np.float64) - np.asarray(baseline_metrics["csi"][t], dtype=np.float64)
    return res
