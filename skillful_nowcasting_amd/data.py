"""The data path on either side of the training step (mirror of train/run.py:114-158 of the reference).

The reference's `TFDataset.__getitem__` takes a dataset row's `radar_frames` ([T_all, H, W, C], channels last), keeps the LAST
4 + 18 frames (targets aligned to the end of the window, inputs right before them) and moves the channel axis:
[T, H, W, C] -> [T, C, H, W].  That is all the arithmetic there is; what matters on an MI355X is that the host side keeps up with
~300 frames/s/GPU without stalling the step:

  * rows are copied into PINNED staging buffers in their storage dtype (uint8 / int16 / float16 / float32 - a uint8 frame is a
    quarter of the PCIe bytes of fp32),
  * two staging slots alternate: while the step runs on batch k, batch k+1 is uploaded on a side stream
    (`non_blocking` copies from pinned memory), converted to fp32 and laid out [B, T, C, H, W] on the device,
  * the consumer only waits on an event, never on the host; the PRODUCER waits (on the host) for a slot's previous upload before
    it overwrites that slot - a `non_blocking` copy reads the pinned buffer asynchronously, and nothing else stops the host from
    running two batches ahead of the copy engine.

`RadarBatchLoader` involves no HIP kernel of ours: layout moves and dtype conversion are torch copy kernels (plumbing, not the hot
path).  `ImportanceCropLoader` does: training on FULL-FRAME composites (crops drawn with an inclusion probability that
grows with the rain they hold) needs one transcendental per pixel of every frame, ~30 x the pixels a crop contains, on data that has
to be uploaded anyway - `dgmr_crop_scores` scores every candidate crop of a sequence in one streaming read on the device and
`dgmr_crop_gather` cuts the accepted ones straight into the batch, converted and laid out for the model.
"""
from __future__ import annotations

from typing import Iterable, Iterator, Optional, Tuple

import numpy as np
import torch

NUM_INPUT_FRAMES = 4
NUM_TARGET_FRAMES = 18


def extract_input_and_target_frames(radar_frames, num_input_frames: int = NUM_INPUT_FRAMES, num_target_frames: int = NUM_TARGET_FRAMES):
    """train/run.py:118-123: targets are the last `num_target_frames` frames of the window, inputs the frames right before them."""
    input_frames = radar_frames[-num_target_frames - num_input_frames: -num_target_frames]
    target_frames = radar_frames[-num_target_frames:]
    return input_frames, target_frames


def to_model_layout(frames):
    """[T, H, W, C] -> [T, C, H, W] (train/run.py:156-158, `np.moveaxis(x, [0, 1, 2, 3], [0, 2, 3, 1])`); numpy or torch."""
    if isinstance(frames, np.ndarray):
        return np.moveaxis(frames, [0, 1, 2, 3], [0, 2, 3, 1])
    return frames.permute(0, 3, 1, 2)


def row_to_sample(row, num_input_frames: int = NUM_INPUT_FRAMES, num_target_frames: int = NUM_TARGET_FRAMES):
    """What `TFDataset.__getitem__` returns for a dataset row (a mapping with a `radar_frames` entry, or the array itself)."""
    frames = row["radar_frames"] if isinstance(row, dict) else row
    x, y = extract_input_and_target_frames(frames, num_input_frames, num_target_frames)
    return to_model_layout(x), to_model_layout(y)


class RadarBatchLoader:
    """Iterate `(images [B,4,C,H,W], future [B,T,C,H,W])` fp32 device batches from an iterable of rows (`radar_frames` arrays
    [T_all, H, W, C] of any real dtype), double-buffered through pinned memory and a copy stream.

    `scale` / `offset`: optional affine applied after the conversion to fp32 (e.g. 1/32 for the 1/32-mm/h integer encoding of the
    NIMROD composites).  `device=None` or a CPU device: same semantics without streams (used by the CPU tests).
    `drop_last`: discard a final partial batch (the reference's loader yields whatever the dataset yields).
    """

    def __init__(self, rows: Iterable, batch_size: int, device=None, num_input_frames: int = NUM_INPUT_FRAMES,
                 num_target_frames: int = NUM_TARGET_FRAMES, scale: float = 1.0, offset: float = 0.0, drop_last: bool = True):
        self.rows, self.batch_size = rows, int(batch_size)
        self.device = torch.device(device) if device is not None else torch.device("cpu")
        self.n_in, self.n_out = num_input_frames, num_target_frames
        self.scale, self.offset, self.drop_last = float(scale), float(offset), drop_last
        self._slots = [None, None]
        self._slot_uploaded = [None, None]  # event recorded right after the H2D copy out of each slot
        self._stream = torch.cuda.Stream(self.device) if self.device.type == "cuda" else None

    # -- host side: rows -> one staging slot ------------------------------------------------------------------------------
    def _stage(self, batch_rows, slot: int):
        t = self.n_in + self.n_out
        first = np.asarray(batch_rows[0]["radar_frames"] if isinstance(batch_rows[0], dict) else batch_rows[0])
        shape = (len(batch_rows), t) + tuple(first.shape[1:])  # [B, T, H, W, C] in the rows' dtype
        dtype = torch.from_numpy(first[:1]).dtype
        if self._slot_uploaded[slot] is not None:
            self._slot_uploaded[slot].synchronize()  # the previous upload from this slot has left the pinned buffer
            self._slot_uploaded[slot] = None
        buf = self._slots[slot]
        if buf is None or tuple(buf.shape) != shape or buf.dtype != dtype:
            buf = torch.empty(shape, dtype=dtype, pin_memory=self.device.type == "cuda")
            self._slots[slot] = buf
        for i, row in enumerate(batch_rows):
            frames = np.asarray(row["radar_frames"] if isinstance(row, dict) else row)
            if frames.shape[0] < t:
                raise ValueError(f"row {i}: {frames.shape[0]} frames, need at least {t}")
            buf[i].copy_(torch.from_numpy(np.ascontiguousarray(frames[-t:])))  # the last 4 + T frames of the window
        return buf

    # -- device side: staging slot -> fp32 [B, T, C, H, W] -----------------------------------------------------------------
    def _upload(self, buf, slot: int):
        if self._stream is None:
            dev = buf.to(self.device)
            return self._finish(dev), None
        with torch.cuda.stream(self._stream):
            dev = buf.to(self.device, non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(self._stream)
            self._slot_uploaded[slot] = copied
            out = self._finish(dev)
            ev = torch.cuda.Event()
            ev.record(self._stream)
        return out, ev

    def _finish(self, dev):
        x = dev.permute(0, 1, 4, 2, 3).float()  # [B, T, H, W, C] -> [B, T, C, H, W], fp32
        if self.scale != 1.0 or self.offset != 0.0:
            x = x * self.scale + self.offset
        x = x.contiguous()
        return x[:, :self.n_in], x[:, self.n_in:]

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        pending: Optional[tuple] = None
        chunk, slot = [], 0
        for row in self.rows:
            chunk.append(row)
            if len(chunk) < self.batch_size:
                continue
            nxt = self._upload(self._stage(chunk, slot), slot)
            chunk, slot = [], slot ^ 1
            if pending is not None:
                yield self._ready(pending)
            pending = nxt
        if chunk and not self.drop_last:
            nxt = self._upload(self._stage(chunk, slot), slot)
            if pending is not None:
                yield self._ready(pending)
            pending = nxt
        if pending is not None:
            yield self._ready(pending)

    def _ready(self, item):
        (images, future), ev = item
        if ev is not None:
            torch.cuda.current_stream(self.device).wait_event(ev)
            for t_ in (images, future):  # the tensors were produced on the copy stream: tell the allocator about their consumer
                t_.record_stream(torch.cuda.current_stream(self.device))
        return images, future


# ---- importance-sampled crops from full frames -----------------------------------------------------------------------------------
# storage dtype -> DGMR_DT_* (include/dgmr_hip.h): the dtypes the loaders stage
_STORAGE_DTYPES = {torch.uint8: 0, torch.int16: 1, torch.float16: 2, torch.float32: 3}


def _crop_geometry(shape, cell: int, crop: int):
    """(T, H, W, C, Gy, Gx) of a sequence [T, H, W, C] cut into `crop`-sized candidates on a `cell`-pixel lattice."""
    if len(shape) != 4:
        raise ValueError(f"frames must be [T, H, W, C], got shape {tuple(shape)}")
    t, h, w, c = (int(v) for v in shape)
    cell, crop = int(cell), int(crop)
    if min(t, h, w, c) < 1 or cell < 1 or crop < 1:
        raise ValueError(f"extents must be positive: frames {tuple(shape)}, cell {cell}, crop {crop}")
    if crop % cell != 0:
        raise ValueError(f"crop={crop} is not a multiple of the stride / cell {cell}")
    if h < crop or w < crop:
        raise ValueError(f"frame {h} x {w} is smaller than the crop {crop}")
    return t, h, w, c, (h - crop) // cell + 1, (w - crop) // cell + 1


def _physical(raw: np.ndarray, scale: float, offset: float) -> np.ndarray:
    """fp32 raw * scale, rounded, + offset, rounded: what torch's `raw.float() * scale + offset` and the kernels compute."""
    return raw.astype(np.float32) * np.float32(scale) + np.float32(offset)


def crop_scores_reference(frames, scale: float = 1.0, offset: float = 0.0, sat_scale: float = 1.0, cell: int = 32, crop: int = 256):
    """The specification of `dgmr_crop_scores`, in numpy: for every candidate crop (top-left (gy * cell, gx * cell)) of the sequence
    `frames` [T, H, W, C], the rain score  sum -expm1(-x / sat_scale)  over its T * C * crop^2 elements, in float64, and the number of
    missing elements (`!(x >= 0)`: negative, -inf, NaN; they add nothing to the score).  x is the fp32 value `raw * scale + offset`.
    Returns (scores float64 [Gy, Gx], missing int64 [Gy, Gx])."""
    frames = np.asarray(frames)
    t, h, w, c, gy, gx = _crop_geometry(frames.shape, cell, crop)
    if not sat_scale > 0:
        raise ValueError(f"sat_scale={sat_scale} must be positive")
    ch, cw, k = h // cell, w // cell, crop // cell
    x = _physical(frames[:, :ch * cell, :cw * cell], scale, offset)
    miss = ~(x >= 0)
    terms = -np.expm1(-np.where(miss, np.float32(0), x).astype(np.float64) / float(sat_scale))
    cells = terms.reshape(t, ch, cell, cw, cell, c).sum(axis=(0, 2, 4, 5))
    cmiss = miss.reshape(t, ch, cell, cw, cell, c).sum(axis=(0, 2, 4, 5), dtype=np.int64)
    scores, missing = np.zeros((gy, gx), np.float64), np.zeros((gy, gx), np.int64)
    for a in range(k):
        for b in range(k):
            scores += cells[a:a + gy, b:b + gx]
            missing += cmiss[a:a + gy, b:b + gx]
    return scores, missing


def inclusion_probability(scores, n_elements: int, q_min: float = 2e-4, m: float = 0.1):
    """q = min(1, q_min + m / n * score) in float64, n_elements = T * C * crop^2 the elements a crop holds."""
    return np.minimum(1.0, float(q_min) + float(m) * np.asarray(scores, dtype=np.float64) / float(n_elements))


def _storage_code(frames: torch.Tensor) -> int:
    if frames.dtype not in _STORAGE_DTYPES:
        raise ValueError(f"frames dtype {frames.dtype}: one of uint8, int16, float16, float32 is required")
    return _STORAGE_DTYPES[frames.dtype]


def _launch_stream():
    import ctypes

    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def crop_scores(frames: torch.Tensor, scale: float = 1.0, offset: float = 0.0, sat_scale: float = 1.0, cell: int = 32,
                crop: int = 256, out=None):
    """Scores and missing counts of every candidate crop of one sequence `frames` [T, H, W, C] (uint8 / int16 / float16 / float32,
    contiguous): (scores float64 [Gy, Gx], missing int32 [Gy, Gx]) on the frames' device.  On a HIP device this is
    `dgmr_crop_scores` on the current stream (no synchronisation); a CPU tensor goes through `crop_scores_reference`.
    `out`: optional (cell_sums, cell_missing, scores, missing) device buffers of a previous call with the same geometry."""
    t, h, w, c, gy, gx = _crop_geometry(frames.shape, cell, crop)
    code = _storage_code(frames)
    if not sat_scale > 0:
        raise ValueError(f"sat_scale={sat_scale} must be positive")
    if not frames.is_cuda:
        s, m = crop_scores_reference(frames.numpy(), scale, offset, sat_scale, cell, crop)
        return torch.from_numpy(s), torch.from_numpy(m.astype(np.int32))
    from ._lib import call

    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous [T, H, W, C]")
    if out is None:
        with torch.cuda.device(frames.device):
            out = (torch.empty((h // cell, w // cell), dtype=torch.float64, device=frames.device),
                   torch.empty((h // cell, w // cell), dtype=torch.int32, device=frames.device),
                   torch.empty((gy, gx), dtype=torch.float64, device=frames.device),
                   torch.empty((gy, gx), dtype=torch.int32, device=frames.device))
    cell_sums, cell_missing, scores, missing = out
    with torch.cuda.device(frames.device):
        call("dgmr_crop_scores", frames.data_ptr(), code, t, h, w, c, float(scale), float(offset), float(sat_scale), int(cell), int(crop),
             cell_sums.data_ptr(), cell_missing.data_ptr(), scores.data_ptr(), missing.data_ptr(), _launch_stream())
    return scores, missing


def _check_origins(origins, h: int, w: int, crop: int) -> np.ndarray:
    o = np.asarray(origins, dtype=np.int64).reshape(-1, 2)
    bad = (o[:, 0] < 0) | (o[:, 0] > h - crop) | (o[:, 1] < 0) | (o[:, 1] > w - crop)
    if bad.any():
        y, x = o[bad][0]
        raise ValueError(f"crop origin (y={y}, x={x}) outside [0, {h - crop}] x [0, {w - crop}]")
    return o


def gather_crops(frames: torch.Tensor, origins, crop: int = 256, scale: float = 1.0, offset: float = 0.0, clamp_missing: bool = False,
                 missing_fill: float = 0.0, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The crops of one sequence `frames` [T, H, W, C] with top-left corners `origins` ([N, 2] host integers (y, x), validated here:
    an origin outside the frame raises ValueError before anything is uploaded; or an int32 [N, 2] tensor already on the frames' HIP
    device, validated by its owner - nothing is uploaded then), as fp32 [N, T, C, crop, crop] = the model's layout, each
    element `raw.float() * scale + offset`; `clamp_missing`: elements with `!(x >= 0)` become `missing_fill`.  On a HIP device this is
    `dgmr_crop_gather` on the current stream, written into `out` if given (contiguous fp32 [N, T, C, crop, crop], e.g. a slice of a
    batch under assembly); a CPU tensor is sliced with torch, same arithmetic."""
    t, h, w, c, _, _ = _crop_geometry(frames.shape, crop, crop)
    code = _storage_code(frames)
    dev_o = origins if isinstance(origins, torch.Tensor) and origins.is_cuda else None
    if dev_o is not None:
        if dev_o.dtype != torch.int32 or dev_o.dim() != 2 or dev_o.shape[1] != 2 or not dev_o.is_contiguous() or dev_o.device != frames.device:
            raise ValueError(f"device origins must be a contiguous int32 [N, 2] tensor on {frames.device}")
        n = dev_o.shape[0]
    else:
        o = _check_origins(origins, h, w, crop)
        n = o.shape[0]
    shape = (n, t, c, crop, crop)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous float32 {shape} tensor on {frames.device}")
    if n == 0:
        return out
    if not frames.is_cuda:
        for i, (y, x) in enumerate(o):
            v = frames[:, y:y + crop, x:x + crop, :].permute(0, 3, 1, 2).float() * float(scale) + float(offset)
            if clamp_missing:
                v = torch.where(v >= 0, v, torch.full_like(v, float(missing_fill)))
            out[i].copy_(v)
        return out
    from ._lib import call

    if not frames.is_contiguous():
        raise ValueError("frames must be contiguous [T, H, W, C]")
    with torch.cuda.device(frames.device):
        if dev_o is None:
            dev_o = torch.from_numpy(o.astype(np.int32)).pin_memory().to(frames.device, non_blocking=True)
        call("dgmr_crop_gather", frames.data_ptr(), code, t, h, w, c, dev_o.data_ptr(), n, int(crop), float(scale), float(offset),
             int(bool(clamp_missing)), float(missing_fill), out.data_ptr(), _launch_stream())
    return out


class ImportanceCropLoader(RadarBatchLoader):
    """Iterate `(images [B,4,C,crop,crop], future [B,T,C,crop,crop])` fp32 batches of crops drawn from FULL-FRAME rows
    (`radar_frames` windows [T_all, H, W, C], uint8 / int16 / float16 / float32; the last 4 + T frames are used), each candidate crop
    on the `stride`-pixel lattice kept with probability  q = min(1, q_min + m / n * sum(1 - exp(-x / sat_scale)))  over its n = (4 + T)
    * C * crop^2 elements - so that a dry-dominated archive does not train the model on zeros.  It feeds `training_step`
    like `RadarBatchLoader`.

    `scale` / `offset`: the affine from the storage encoding to the physical value x (mm/h), applied in fp32 as `raw * scale +
    offset`.  An element is MISSING when `!(x >= 0)` (negative, -inf, NaN: NIMROD-style "no data"); missing elements add nothing to a
    crop's score, a candidate with more than `max_missing * n` of them is never drawn, and with `clamp_missing` they reach the model as
    `missing_fill`.  `max_crops_per_row`: at most that many of a row's accepted crops are used.  `seed`: one
    `numpy.random.Generator(PCG64(seed))` per iteration draws, per row, `u = rng.random(Gy * Gx)` in raster order and
    `rng.permutation` of the accepted candidates; crops of several rows fill one batch; `drop_last` discards a final partial batch.

    On a HIP device every row is staged into `RadarBatchLoader`'s pinned staging in its storage dtype, uploaded and scored on a copy
    stream (`dgmr_crop_scores`); the two small grids come back to pinned host memory and the host waits for THAT copy only - the number
    of accepted crops decides batching, so the host has to see it; the consumer's stream is never synchronised - and the accepted crops
    are cut straight into the batch under assembly (`dgmr_crop_gather`).  Because of that wait a row's upload has always finished
    before the next row is staged: the staging's two slots alternate as in `RadarBatchLoader`, but no two uploads overlap here; what
    overlaps is the consumer's step, queued on its own stream, with the loader's work on the next rows.  `device=None` or a CPU device: the same selection on
    `crop_scores_reference`.  The host and the device path draw the same crops from the same seed as long as no `u` lies within
    ~1e-12 of its `q` (the two scores agree to double summation order).

    After each yielded batch: `last_inclusion_prob` (float64 [B]: the paper weights evaluation by its inverse), `last_origins`
    (int64 [B, 3]: row index, y, x) and the running `stats` (`rows`, `candidates`, `accepted`, `rejected_missing`)."""

    def __init__(self, rows: Iterable, batch_size: int, device=None, crop: int = 256, stride: int = 32, q_min: float = 2e-4,
                 m: float = 0.1, sat_scale: float = 1.0, scale: float = 1.0, offset: float = 0.0, max_missing: float = 1.0,
                 clamp_missing: bool = True, missing_fill: float = 0.0, max_crops_per_row: Optional[int] = None, seed: int = 0,
                 num_input_frames: int = NUM_INPUT_FRAMES, num_target_frames: int = NUM_TARGET_FRAMES, drop_last: bool = True):
        super().__init__(rows, batch_size, device, num_input_frames, num_target_frames, scale, offset, drop_last)
        self.crop, self.stride = int(crop), int(stride)
        if self.batch_size < 1 or self.crop < 1 or self.stride < 1:
            raise ValueError(f"batch_size={batch_size}, crop={crop}, stride={stride} must be positive")
        if self.crop % self.stride != 0:
            raise ValueError(f"crop={crop} is not a multiple of stride={stride}")
        if not sat_scale > 0:
            raise ValueError(f"sat_scale={sat_scale} must be positive")
        if max_crops_per_row is not None and max_crops_per_row < 0:
            raise ValueError(f"max_crops_per_row={max_crops_per_row} is negative")
        self.q_min, self.m, self.sat_scale = float(q_min), float(m), float(sat_scale)
        self.max_missing, self.clamp_missing, self.missing_fill = float(max_missing), bool(clamp_missing), float(missing_fill)
        self.max_crops_per_row, self.seed = max_crops_per_row, seed
        self.last_inclusion_prob = np.zeros(0, np.float64)
        self.last_origins = np.zeros((0, 3), np.int64)
        self.stats = {"rows": 0, "candidates": 0, "accepted": 0, "rejected_missing": 0}
        self._grids = None  # per geometry: device workspace, pinned host copies of the two grids, pinned + device origin tables

    # -- the accept draw (host, both paths) ---------------------------------------------------------------------------------
    def _select(self, rng, scores: np.ndarray, missing: np.ndarray, n_elements: int):
        """-> (origins int64 [K, 2], q float64 [K]) of this row's crops, in the order they enter batches."""
        q = inclusion_probability(scores, n_elements, self.q_min, self.m).reshape(-1)
        u = rng.random(q.size)
        usable = missing.reshape(-1) <= self.max_missing * n_elements
        keep = np.flatnonzero((u < q) & usable)
        self.stats["rows"] += 1
        self.stats["candidates"] += q.size
        self.stats["rejected_missing"] += int((~usable).sum())
        keep = keep[rng.permutation(keep.size)]
        if self.max_crops_per_row is not None:
            keep = keep[:self.max_crops_per_row]
        self.stats["accepted"] += keep.size
        gx = scores.shape[1]
        return np.stack([keep // gx * self.stride, keep % gx * self.stride], axis=1).astype(np.int64), q[keep]

    # -- device side: one staged row -> its two grids on the host ------------------------------------------------------------------
    def _score(self, dev: torch.Tensor):
        """`dgmr_crop_scores` on the copy stream (the caller's current stream) and the grids' way back: only this copy is waited for."""
        _, h, w, _, gy, gx = _crop_geometry(dev.shape, self.stride, self.crop)
        key = (tuple(dev.shape), dev.dtype)
        if self._grids is None or self._grids[0] != key:
            ws = (torch.empty((h // self.stride, w // self.stride), dtype=torch.float64, device=dev.device),
                  torch.empty((h // self.stride, w // self.stride), dtype=torch.int32, device=dev.device),
                  torch.empty((gy, gx), dtype=torch.float64, device=dev.device),
                  torch.empty((gy, gx), dtype=torch.int32, device=dev.device))
            host = (torch.empty((gy, gx), dtype=torch.float64, pin_memory=True), torch.empty((gy, gx), dtype=torch.int32, pin_memory=True))
            origins = (torch.empty((gy * gx, 2), dtype=torch.int32, pin_memory=True),
                       torch.empty((gy * gx, 2), dtype=torch.int32, device=dev.device))
            self._grids = (key, ws, host, origins)
        _, ws, host, _ = self._grids
        crop_scores(dev, self.scale, self.offset, self.sat_scale, self.stride, self.crop, out=ws)
        host[0].copy_(ws[2], non_blocking=True)
        host[1].copy_(ws[3], non_blocking=True)
        back = torch.cuda.Event()
        back.record(self._stream)
        back.synchronize()  # the copy stream's event: the consumer's stream is not involved
        return host[0].numpy().copy(), host[1].numpy().astype(np.int64)

    def __iter__(self) -> Iterator[Tuple[torch.Tensor, torch.Tensor]]:
        rng = np.random.Generator(np.random.PCG64(self.seed))
        t = self.n_in + self.n_out
        on_gpu = self._stream is not None
        batch, filled, meta_o, meta_q, slot = None, 0, [], [], 0

        def finish(n):
            self.last_origins = np.concatenate(meta_o)[:n] if meta_o else np.zeros((0, 3), np.int64)
            self.last_inclusion_prob = np.concatenate(meta_q)[:n] if meta_q else np.zeros(0, np.float64)
            x = batch[:n]
            item = (x[:, :self.n_in], x[:, self.n_in:])
            if not on_gpu:
                return item
            ev = torch.cuda.Event()
            ev.record(self._stream)
            return self._ready((item, ev))

        for index, row in enumerate(self.rows):
            frames = np.asarray(row["radar_frames"] if isinstance(row, dict) else row)
            if frames.ndim != 4:
                raise ValueError(f"row {index}: radar_frames must be [T, H, W, C], got shape {frames.shape}")
            if frames.shape[0] < t:
                raise ValueError(f"row {index}: {frames.shape[0]} frames, need at least {t}")
            c = _crop_geometry((t,) + frames.shape[1:], self.stride, self.crop)[3]
            n_elements = t * c * self.crop * self.crop
            if on_gpu:
                staged = self._stage([frames], slot)[0]  # pinned, storage dtype; waits for this slot's previous upload
                with torch.cuda.stream(self._stream):
                    dev = staged.to(self.device, non_blocking=True)
                    copied = torch.cuda.Event()
                    copied.record(self._stream)
                    self._slot_uploaded[slot] = copied
                    scores, missing = self._score(dev)
                slot ^= 1
            else:
                dev = torch.from_numpy(np.ascontiguousarray(frames[-t:]))
                _storage_code(dev)
                scores, missing = crop_scores_reference(dev.numpy(), self.scale, self.offset, self.sat_scale, self.stride, self.crop)
            origins, q = self._select(rng, scores, missing, n_elements)
            if on_gpu and len(origins):
                # one upload per row through the loader's own tables.  The host may rewrite the pinned table for the next row: it has
                # waited for that row's grids by then, which the copy stream brings back after this upload
                pinned_o, dev_o = self._grids[3]
                pinned_o[:len(origins)].copy_(torch.from_numpy(_check_origins(origins, *frames.shape[1:3], self.crop).astype(np.int32)))
                with torch.cuda.stream(self._stream):
                    dev_o[:len(origins)].copy_(pinned_o[:len(origins)], non_blocking=True)
            done = 0
            while done < len(origins):
                if batch is None:
                    if on_gpu:
                        with torch.cuda.stream(self._stream):
                            batch = torch.empty((self.batch_size, t, c, self.crop, self.crop), dtype=torch.float32, device=self.device)
                    else:
                        batch = torch.empty((self.batch_size, t, c, self.crop, self.crop), dtype=torch.float32)
                    filled, meta_o, meta_q = 0, [], []
                n = min(self.batch_size - filled, len(origins) - done)
                part = origins[done:done + n]
                if on_gpu:
                    with torch.cuda.stream(self._stream):
                        gather_crops(dev, dev_o[done:done + n], self.crop, self.scale, self.offset, self.clamp_missing,
                                     self.missing_fill, out=batch[filled:filled + n])
                else:
                    gather_crops(dev, part, self.crop, self.scale, self.offset, self.clamp_missing, self.missing_fill,
                                 out=batch[filled:filled + n])
                meta_o.append(np.concatenate([np.full((n, 1), index, np.int64), part], axis=1))
                meta_q.append(q[done:done + n])
                done, filled = done + n, filled + n
                if filled == self.batch_size:
                    yield finish(filled)
                    batch = None
        if batch is not None and filled and not self.drop_last:
            yield finish(filled)
