"""The advection baseline: block-matching motion (TREC), semi-Lagrangian extrapolation, Eulerian persistence (what the
paper plots DGMR against; INTEGRATION.md "A baseline to beat").

  * `block_match`: per block of `next`, the integer displacement (dy, dx) of least squared difference against `prev` - the echo
    moved by +d between the two frames - with the costs of its four neighbours and the block's wet count;
  * `lk_refine`: per block, a few Gauss-Newton steps on the squared difference from the integer match (Lucas-Kanade on the block
    lattice, `dgmr_lk_refine`) with the structure tensor's eigenvalues, which say whether the block shows its motion at all;
  * `motion_field`: block matching over consecutive context frames, a parabola through the neighbour costs for the sub-pixel part
    (or, `subpixel="lk"`, the refinement above), the pairs averaged, the lattice smoothed and filled;
  * `advect`: the last frame extrapolated along the field for all lead times, each lead time interpolating the source once;
  * `advect_series`: the same with a source of its own per lead time and one field per group of planes (`dgmr_advect_series`) -
    what `stochastic.EnsembleAdvectionNowcaster` moves its members with;
  * `advect_series_perturbed`: `advect_series` with a velocity error per plane and lead time along and across the directions of
    `unit_directions` (`dgmr_advect_series_perturbed`) - the members' perturbed motion vectors;
  * `AdvectionNowcaster`, `persistence_nowcast`: forecasts in the layout of `DGMR.nowcast_full_frame` / `DGMR.sample` with one member,
    which `NowcastVerifier`, `SpectrumVerifier` and `ValueVerifier` take as they are (`num_members=1`).

`block_match_reference` and `advect_reference` are the specifications in float64 numpy.  On a HIP device the two are
`dgmr_block_match` and `dgmr_advect` (csrc/advect.hip) on the current stream, without synchronisation; CPU tensors go through the
references.  Everything else is torch on a lattice of a few thousand nodes, the same code for CPU and HIP tensors.
"""
from __future__ import annotations

import ctypes
from collections import namedtuple
from typing import Optional

import numpy as np
import torch

BLOCKS = (16, 32)
MAX_RADIUS = 16
MAX_STEPS = 64
CONTEXT_FRAMES = 4  # at most this many of the latest frames give the motion

LK_MAX_ITERATIONS = 16
SUBPIXEL = ("parabola", "lk")

BlockMatch = namedtuple("BlockMatch", ["disp", "cost", "wet"])
LkRefine = namedtuple("LkRefine", ["v", "eig", "residual"])


def _check_match(h: int, w: int, block: int, stride: int, radius: int, min_wet: int):
    if block not in BLOCKS:
        raise ValueError(f"block={block}, {BLOCKS} are supported")
    if not 1 <= stride <= block:
        raise ValueError(f"stride={stride} must be 1 ... block={block}")
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"radius={radius} must be 1 ... {MAX_RADIUS}")
    if min_wet < 0:
        raise ValueError(f"min_wet={min_wet} must not be negative")
    if h < block or w < block:
        raise ValueError(f"H={h} and W={w} must be at least block={block}")
    return (h - block) // stride + 1, (w - block) // stride + 1


def _tie_order(radius: int):
    """The candidates (dy, dx) in the order ties are resolved: smallest dy^2 + dx^2, then smallest dy, then smallest dx."""
    d = [(dy, dx) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]
    return sorted(d, key=lambda v: (v[0] * v[0] + v[1] * v[1], v[0], v[1]))


def block_costs_reference(prev, nxt, block: int, stride: int, radius: int) -> np.ndarray:
    """float64 [N, By, Bx, 2R + 1, 2R + 1]: the cost of every displacement (index dy + R, dx + R), +inf where it is no candidate."""
    p = np.asarray(prev, dtype=np.float32)
    q = np.asarray(nxt, dtype=np.float32)
    n, h, w = p.shape
    by, bx = (h - block) // stride + 1, (w - block) // stride + 1
    with np.errstate(invalid="ignore"):
        p = np.where(p >= 0, p, np.float32(0)).astype(np.float64)
        q = np.where(q >= 0, q, np.float32(0)).astype(np.float64)
    pad = np.zeros((n, h + 2 * radius, w + 2 * radius))
    pad[:, radius:radius + h, radius:radius + w] = p
    y0 = np.arange(by) * stride
    x0 = np.arange(bx) * stride
    d = 2 * radius + 1
    costs = np.full((n, by, bx, d, d), np.inf)
    view = np.lib.stride_tricks.sliding_window_view
    for dy in range(-radius, radius + 1):
        ok_y = (y0 - dy >= 0) & (y0 - dy + block <= h)
        for dx in range(-radius, radius + 1):
            ok_x = (x0 - dx >= 0) & (x0 - dx + block <= w)
            if not ok_y.any() or not ok_x.any():
                continue
            diff = q - pad[:, radius - dy:radius - dy + h, radius - dx:radius - dx + w]  # prev[y - dy][x - dx]
            sums = view(diff * diff, (block, block), axis=(1, 2))[:, ::stride, ::stride].sum(axis=(-1, -2))
            costs[:, :, :, dy + radius, dx + radius] = np.where(ok_y[None, :, None] & ok_x[None, None, :], sums, np.inf)
    return costs


def block_match_reference(prev, nxt, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                          min_wet: int = 64, costs: Optional[np.ndarray] = None) -> BlockMatch:
    """The specification of `dgmr_block_match`, in float64 numpy.

    prev, nxt: fp32 [N, H, W]; an element with `!(x >= 0)` is missing and read as 0.  Blocks of block x block pixels with top-left
    corners at (by stride, bx stride), By = (H - block) // stride + 1, Bx likewise.  Per plane and block:

      wet[N, By, Bx]      int32    elements of the `nxt` block (missing as 0) that are >= wet_threshold, compared in fp32
      disp[N, By, Bx, 2]  int32    (dy, dx), |dy|, |dx| <= radius, of least cost among the candidates - those whose displaced block
                                   prev[y0 - dy ...][x0 - dx ...] lies wholly inside the frame; cost = sum over the block of
                                   (nxt[y0 + i][x0 + j] - prev[y0 - dy + i][x0 - dx + j])^2.  Ties: the smallest dy^2 + dx^2, then
                                   the smallest dy, then the smallest dx
      cost[N, By, Bx, 5]  float64  the minimum and the costs at (dy - 1, dx), (dy + 1, dx), (dy, dx - 1), (dy, dx + 1); +inf where
                                   that neighbour is no candidate
    A block with wet < min_wet is dry: disp = (0, 0), all five costs +inf.  `costs`: a `block_costs_reference` result to reuse."""
    q = np.asarray(nxt, dtype=np.float32)
    if q.ndim != 3 or np.shape(prev) != q.shape:
        raise ValueError(f"prev and nxt must be [N, H, W] of one shape, got {np.shape(prev)} and {q.shape}")
    n, h, w = q.shape
    by, bx = _check_match(h, w, block, stride, radius, min_wet)
    with np.errstate(invalid="ignore"):
        q0 = np.where(q >= 0, q, np.float32(0))
        is_wet = q0 >= np.float32(wet_threshold)
    wet = np.lib.stride_tricks.sliding_window_view(is_wet, (block, block), axis=(1, 2))[:, ::stride, ::stride].sum(axis=(-1, -2))
    wet = wet.astype(np.int32)
    if costs is None:
        costs = block_costs_reference(prev, nxt, block, stride, radius)
    order = _tie_order(radius)
    oy = np.array([v[0] for v in order])
    ox = np.array([v[1] for v in order])
    ranked = costs[:, :, :, oy + radius, ox + radius]  # [N, By, Bx, candidates in tie order]
    first = np.argmin(ranked, axis=-1)                 # the first of equal minima: the tie rule
    dy, dx = oy[first], ox[first]
    big = np.full((n, by, bx, 2 * radius + 3, 2 * radius + 3), np.inf)
    big[:, :, :, 1:-1, 1:-1] = costs
    ii = np.indices((n, by, bx))
    cost = np.stack([big[ii[0], ii[1], ii[2], dy + radius + 1 + a, dx + radius + 1 + b]
                     for a, b in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))], axis=-1)
    dry = wet < min_wet
    disp = np.stack([dy, dx], axis=-1).astype(np.int32)
    disp[dry] = 0
    cost[dry] = np.inf
    return BlockMatch(disp, cost, wet)


def _lattice_axis(q, origin: float, spacing: float, g: int):
    gc = np.clip((q - origin) / spacing, 0.0, g - 1.0)
    i0 = np.minimum(np.floor(gc).astype(np.int64), max(g - 2, 0))
    return i0, np.minimum(i0 + 1, g - 1), gc - i0


def _field_at(field, py, px, origin, spacing):
    """Bilinear interpolation of field [Gy, Gx, 2] at pixel positions (py, px), clamped to the lattice's extent."""
    y0, y1, fy = _lattice_axis(py, origin, spacing, field.shape[0])
    x0, x1, fx = _lattice_axis(px, origin, spacing, field.shape[1])
    fy, fx = fy[..., None], fx[..., None]
    top = field[y0, x0] + fx * (field[y0, x1] - field[y0, x0])
    bot = field[y1, x0] + fx * (field[y1, x1] - field[y1, x0])
    return top + fy * (bot - top)


def _sample(x, sy, sx):
    """Bilinear interpolation of x [H, W] at (sy, sx); a tap outside the frame is 0."""
    h, w = x.shape
    sy = np.clip(sy, -2.0, h + 1.0)
    sx = np.clip(sx, -2.0, w + 1.0)
    iy, ix = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
    fy, fx = sy - iy, sx - ix
    pad = np.zeros((h + 6, w + 6))
    pad[3:3 + h, 3:3 + w] = x

    def tap(a, b):
        return pad[a + 3, b + 3]

    top = tap(iy, ix) + fx * (tap(iy, ix + 1) - tap(iy, ix))
    bot = tap(iy + 1, ix) + fx * (tap(iy + 1, ix + 1) - tap(iy + 1, ix))
    return top + fy * (bot - top)


def advect_reference(x, field, steps: int, origin: float = 0.0, spacing: float = 1.0) -> np.ndarray:
    """The specification of `dgmr_advect`, in float64 numpy -> float64 [N, steps, H, W].

    x: fp32 [N, H, W], missing elements (`!(x >= 0)`) read as 0.  field: [N or 1, Gy, Gx, 2] = (vy, vx) in pixels per step; node
    (gy, gx) sits at pixel (origin + gy spacing, origin + gx spacing); one plane is shared by all planes of x.  v(p): bilinear
    interpolation of the lattice with positions clamped to its extent (Gy = Gx = 1: a uniform field); s(p): bilinear interpolation
    of x, a tap outside the frame is 0, so the forecast ramps to zero over one pixel where nothing can be advected in.
    D_0 = 0;  D_t(p) = D_(t-1)(p) + v(p - D_(t-1)(p));  out[n, t - 1][p] = s(p - D_t(p)): every lead time interpolates the source once."""
    x = np.asarray(x, dtype=np.float32)
    field = np.asarray(field, dtype=np.float32).astype(np.float64)
    if x.ndim != 3 or field.ndim != 4 or field.shape[-1] != 2 or field.shape[0] not in (1, x.shape[0]):
        raise ValueError(f"x must be [N, H, W] and field [N or 1, Gy, Gx, 2], got {x.shape} and {field.shape}")
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps={steps}, 1 ... {MAX_STEPS} are supported")
    if not spacing > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    origin, spacing = float(np.float32(origin)), float(np.float32(spacing))
    n, h, w = x.shape
    with np.errstate(invalid="ignore"):
        x = np.where(x >= 0, x, np.float32(0)).astype(np.float64)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((n, steps, h, w))
    for i in range(n):
        f = field[i if field.shape[0] > 1 else 0]
        dy, dx = np.zeros((h, w)), np.zeros((h, w))
        for t in range(steps):
            v = _field_at(f, py - dy, px - dx, origin, spacing)
            dy, dx = dy + v[..., 0], dx + v[..., 1]
            out[i, t] = _sample(x[i], py - dy, px - dx)
    return out


def _check_lk(iterations, eig_ratio):
    """-> (iterations, eig_ratio rounded to fp32, as the kernel takes it)"""
    if isinstance(iterations, bool) or int(iterations) != iterations or not 1 <= int(iterations) <= LK_MAX_ITERATIONS:
        raise ValueError(f"iterations={iterations!r} must be an integer 1 ... {LK_MAX_ITERATIONS}")
    ratio = float(np.float32(eig_ratio))
    if not (ratio >= 0 and np.isfinite(ratio)):
        raise ValueError(f"eig_ratio={eig_ratio} must be finite and not negative")
    return int(iterations), ratio


def lk_conditioned(eig, eig_ratio: float = 0.01):
    """bool [...]: the blocks of eig [..., 2] = (lambda_min, lambda_max) whose motion `lk_refine` solves for: lambda_min > 0 and
    lambda_min >= eig_ratio lambda_max (eig_ratio rounded to fp32).  numpy arrays and torch tensors alike."""
    ratio = _check_lk(1, eig_ratio)[1]
    return (eig[..., 0] > 0) & (eig[..., 0] >= ratio * eig[..., 1])


def lk_refine_reference(prev, nxt, disp, cost, block: int = 32, stride: int = 16, iterations: int = 4,
                        eig_ratio: float = 0.01) -> LkRefine:
    """The specification of `dgmr_lk_refine`, in float64 numpy: the integer block match refined to sub-pixel motion by Gauss-Newton
    steps on the block's squared difference (Lucas-Kanade, forward-additive, with the template's gradient).

    prev, nxt: fp32 [N, H, W], missing elements read as 0; disp [N, By, Bx, 2], cost [N, By, Bx, 5]: `block_match_reference`'s.  Per
    plane and block with corner (y0, x0) = (by stride, bx stride) and integer match d0 = disp, over the interior I of the `nxt` block,
    (y0 + i, x0 + j) with 1 <= i, j <= block - 2, Q = nxt:

      g = (gy, gx)        central differences of Q, 0.5 (Q[y + 1][x] - Q[y - 1][x]) and the same along x: all taps inside the block
      G = sum_I g g^T;    eig = (lambda_min, lambda_max) = (tr -+ sqrt(max(tr^2 - 4 det, 0))) / 2
      conditioned:        lambda_min > 0 and lambda_min >= eig_ratio lambda_max (`lk_conditioned`; eig_ratio rounded to fp32)
      d = d0; `iterations` times, for a conditioned block:
          r(p) = Q(p) - s(p - d), s the bilinear interpolation of prev with zero taps outside the frame (`advect_reference`'s);
          b = -sum_I g r;  delta = G^-1 b;  d <- clip(d + delta, d0 - 1, d0 + 1) per axis
      v[N, By, Bx, 2]     float64  d; d0 for a block that is not conditioned
      eig[N, By, Bx, 2]   float64
      residual[N, By, Bx] float64  sum_I r^2 at the final d
    A dry block (cost[..., 0] not finite) gets v = (0, 0), eig = (0, 0), residual = +inf.  G is formed once, and the start is the block
    match, so there is no pyramid: motion beyond block matching's radius stays out of reach."""
    q = np.asarray(nxt, dtype=np.float32)
    p = np.asarray(prev, dtype=np.float32)
    if q.ndim != 3 or p.shape != q.shape:
        raise ValueError(f"prev and nxt must be [N, H, W] of one shape, got {p.shape} and {q.shape}")
    n, h, w = q.shape
    by, bx = _check_match(h, w, block, stride, 1, 0)
    iterations, ratio = _check_lk(iterations, eig_ratio)
    disp, cost = np.asarray(disp), np.asarray(cost)
    if disp.shape != (n, by, bx, 2) or cost.shape != (n, by, bx, 5):
        raise ValueError(f"disp and cost must be [{n}, {by}, {bx}, 2] and [{n}, {by}, {bx}, 5], got {disp.shape} and {cost.shape}")
    with np.errstate(invalid="ignore"):
        p = np.where(p >= 0, p, np.float32(0)).astype(np.float64)
        q = np.where(q >= 0, q, np.float32(0)).astype(np.float64)
    inner = np.arange(1, block - 1)
    yy = (np.arange(by) * stride)[:, None, None, None] + inner[None, None, :, None]  # [By, 1, m, 1]
    xx = (np.arange(bx) * stride)[None, :, None, None] + inner[None, None, None, :]  # [1, Bx, 1, m]
    v = np.zeros((n, by, bx, 2))
    eig = np.zeros((n, by, bx, 2))
    residual = np.full((n, by, bx), np.inf)
    for i in range(n):
        blocks = np.lib.stride_tricks.sliding_window_view(q[i], (block, block))[::stride, ::stride]  # [By, Bx, block, block]
        big_q = blocks[..., 1:-1, 1:-1]
        gy = 0.5 * (blocks[..., 2:, 1:-1] - blocks[..., :-2, 1:-1])
        gx = 0.5 * (blocks[..., 1:-1, 2:] - blocks[..., 1:-1, :-2])
        gyy, gxy, gxx = (gy * gy).sum(axis=(-1, -2)), (gy * gx).sum(axis=(-1, -2)), (gx * gx).sum(axis=(-1, -2))
        tr, det = gyy + gxx, gyy * gxx - gxy * gxy
        root = np.sqrt(np.maximum(tr * tr - 4.0 * det, 0.0))
        e = np.stack([0.5 * (tr - root), 0.5 * (tr + root)], axis=-1)
        wet = np.isfinite(cost[i, ..., 0])
        cond = wet & lk_conditioned(e, ratio)
        det = np.where(cond, det, 1.0)
        d0 = disp[i].astype(np.float64)
        d = d0.copy()

        def differences(d):
            return big_q - _sample(p[i], yy - d[..., 0, None, None], xx - d[..., 1, None, None])

        for _ in range(iterations):
            r = differences(d)
            b_y, b_x = -(gy * r).sum(axis=(-1, -2)), -(gx * r).sum(axis=(-1, -2))
            delta = np.stack([(gxx * b_y - gxy * b_x) / det, (gyy * b_x - gxy * b_y) / det], axis=-1)
            d = np.where(cond[..., None], np.clip(d + delta, d0 - 1.0, d0 + 1.0), d0)
        r = differences(d)
        v[i] = np.where(wet[..., None], d, 0.0)
        eig[i] = np.where(wet[..., None], e, 0.0)
        residual[i] = np.where(wet, (r * r).sum(axis=(-1, -2)), np.inf)
    return LkRefine(v, eig, residual)


# ---- the device path -------------------------------------------------------------------------------------------------------------
def _stream(device):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _planes(t: torch.Tensor, what: str):
    """[N, H, W] fp32 with contiguous planes -> (tensor, plane stride); any other layout is copied."""
    if t.dim() != 3 or t.dtype != torch.float32:
        raise ValueError(f"{what} must be a float32 [N, H, W] tensor, got {t.dtype} {tuple(t.shape)}")
    h, w = t.shape[1:]
    if (w > 1 and t.stride(2) != 1) or (h > 1 and t.stride(1) != w) or (t.shape[0] > 1 and t.stride(0) < 0):
        t = t.contiguous()
    return t, (int(t.stride(0)) if t.shape[0] > 1 else h * w)


def block_match(prev: torch.Tensor, nxt: torch.Tensor, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                min_wet: Optional[int] = None) -> BlockMatch:
    """`block_match_reference` for torch tensors, results on the inputs' device: disp int32 [N, By, Bx, 2], cost fp32 [N, By, Bx, 5],
    wet int32 [N, By, Bx].  prev, nxt: fp32 [N, H, W] whose planes are contiguous and equally far apart in both (views of one
    [T, N, H, W] tensor are; anything else is copied).  min_wet: default block^2 // 16.  On a HIP device one `dgmr_block_match` on
    the current stream, nothing synchronised; on the CPU the float64 reference, its costs rounded to fp32."""
    min_wet = block * block // 16 if min_wet is None else int(min_wet)
    if prev.shape != nxt.shape or prev.device != nxt.device:
        raise ValueError(f"prev {tuple(prev.shape)} on {prev.device} and nxt {tuple(nxt.shape)} on {nxt.device} must match")
    prev, ps = _planes(prev, "prev")
    nxt, ns = _planes(nxt, "nxt")
    n, h, w = (int(v) for v in prev.shape)
    by, bx = _check_match(h, w, block, stride, radius, min_wet)
    if not prev.is_cuda:
        ref = block_match_reference(prev.numpy(), nxt.numpy(), block, stride, radius, wet_threshold, min_wet)
        return BlockMatch(torch.from_numpy(ref.disp), torch.from_numpy(ref.cost.astype(np.float32)), torch.from_numpy(ref.wet))
    from ._lib import call

    if ps != ns:
        prev, nxt = prev.contiguous(), nxt.contiguous()
        ps = h * w
    device = prev.device
    with torch.cuda.device(device):
        disp = torch.empty((n, by, bx, 2), dtype=torch.int32, device=device)
        cost = torch.empty((n, by, bx, 5), dtype=torch.float32, device=device)
        wet = torch.empty((n, by, bx), dtype=torch.int32, device=device)
        call("dgmr_block_match", prev.data_ptr(), nxt.data_ptr(), ps, n, h, w, block, stride, radius, float(wet_threshold), min_wet,
             disp.data_ptr(), cost.data_ptr(), wet.data_ptr(), _stream(device))
    return BlockMatch(disp, cost, wet)


def lk_refine(prev: torch.Tensor, nxt: torch.Tensor, match: BlockMatch, block: int = 32, stride: int = 16, iterations: int = 4,
              eig_ratio: float = 0.01) -> LkRefine:
    """`lk_refine_reference` for torch tensors, results on the inputs' device: v fp32 [N, By, Bx, 2], eig float64 [N, By, Bx, 2],
    residual float64 [N, By, Bx].  prev, nxt: `block_match`'s layouts and rules; match: its result for the same frames, block and
    stride.  On a HIP device one `dgmr_lk_refine` on the current stream, nothing synchronised; on the CPU the float64 reference,
    v rounded to fp32."""
    if prev.shape != nxt.shape or prev.device != nxt.device:
        raise ValueError(f"prev {tuple(prev.shape)} on {prev.device} and nxt {tuple(nxt.shape)} on {nxt.device} must match")
    prev, ps = _planes(prev, "prev")
    nxt, ns = _planes(nxt, "nxt")
    n, h, w = (int(v) for v in prev.shape)
    by, bx = _check_match(h, w, block, stride, 1, 0)
    iterations, ratio = _check_lk(iterations, eig_ratio)
    disp, cost = match.disp, match.cost
    if (tuple(disp.shape) != (n, by, bx, 2) or disp.dtype != torch.int32 or tuple(cost.shape) != (n, by, bx, 5) or
            cost.dtype != torch.float32 or disp.device != prev.device or cost.device != prev.device):
        raise ValueError(f"match must hold block_match's int32 [{n}, {by}, {bx}, 2] disp and float32 [{n}, {by}, {bx}, 5] cost on "
                         f"{prev.device}, got {disp.dtype} {tuple(disp.shape)} and {cost.dtype} {tuple(cost.shape)}")
    if not prev.is_cuda:
        ref = lk_refine_reference(prev.numpy(), nxt.numpy(), disp.numpy(), cost.numpy(), block, stride, iterations, ratio)
        return LkRefine(torch.from_numpy(ref.v.astype(np.float32)), torch.from_numpy(ref.eig), torch.from_numpy(ref.residual))
    from ._lib import call

    if ps != ns:
        prev, nxt = prev.contiguous(), nxt.contiguous()
        ps = h * w
    disp, cost = disp.contiguous(), cost.contiguous()
    device = prev.device
    with torch.cuda.device(device):
        v = torch.empty((n, by, bx, 2), dtype=torch.float32, device=device)
        eig = torch.empty((n, by, bx, 2), dtype=torch.float64, device=device)
        residual = torch.empty((n, by, bx), dtype=torch.float64, device=device)
        call("dgmr_lk_refine", prev.data_ptr(), nxt.data_ptr(), ps, n, h, w, block, stride, disp.data_ptr(), cost.data_ptr(), iterations,
             ratio, v.data_ptr(), eig.data_ptr(), residual.data_ptr(), _stream(device))
    return LkRefine(v, eig, residual)


def advect(x: torch.Tensor, field: torch.Tensor, steps: int, origin: float = 0.0, spacing: float = 1.0,
           out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`advect_reference` for torch tensors -> fp32 [N, steps, H, W] on the inputs' device.

    x: fp32 [N, H, W] (contiguous planes, any plane stride); field: fp32 [N or 1, Gy, Gx, 2].  out: an fp32 [N, steps, H, W] tensor or
    view whose planes are contiguous, with any strides over N and steps - a permuted view of a [B, T, C, H, W] buffer is written in
    place.  On a HIP device one `dgmr_advect` on the current stream, nothing synchronised; on the CPU the float64 reference, rounded."""
    x, xs = _planes(x, "x")
    n, h, w = (int(v) for v in x.shape)
    if field.dim() != 4 or field.shape[-1] != 2 or field.shape[0] not in (1, n) or field.dtype != torch.float32 or field.device != x.device:
        raise ValueError(f"field must be a float32 [{n} or 1, Gy, Gx, 2] tensor on {x.device}, got {field.dtype} {tuple(field.shape)}")
    steps = int(steps)
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"steps={steps}, 1 ... {MAX_STEPS} are supported")
    if not float(spacing) > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    if out is None:
        out = torch.empty((n, steps, h, w), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (n, steps, h, w) or out.dtype != torch.float32 or out.device != x.device or (w > 1 and out.stride(3) != 1)
          or (h > 1 and out.stride(2) != w) or (n > 1 and out.stride(0) < 0) or (steps > 1 and out.stride(1) < h * w)):
        raise ValueError(f"out must be a float32 [{n}, {steps}, {h}, {w}] tensor on {x.device} with contiguous planes")
    if not x.is_cuda:
        ref = advect_reference(x.numpy(), field.numpy(), steps, origin, spacing)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    if not field[0].is_contiguous() or (field.shape[0] > 1 and field.stride(0) < 0):
        field = field.contiguous()
    fs = int(field.stride(0)) if field.shape[0] > 1 else 0
    device = x.device
    with torch.cuda.device(device):
        call("dgmr_advect", x.data_ptr(), xs if n > 1 else 0, field.data_ptr(), fs, n, h, w, int(field.shape[1]), int(field.shape[2]),
             float(origin), float(spacing), steps, out.data_ptr(), int(out.stride(0)) if n > 1 else 0,
             int(out.stride(1)) if steps > 1 else h * w, _stream(device))
    return out


def advect_series_reference(x, field, origin: float = 0.0, spacing: float = 1.0, field_group: int = 1) -> np.ndarray:
    """The specification of `dgmr_advect_series`, in float64 numpy -> float64 [N, T, H, W]: `advect_reference` with a source of its
    own per lead time.

    x: fp32 [N, T, H, W]; every value below 0 (and NaN) reads as 0.  field: [N / field_group or 1, Gy, Gx, 2]: plane n moves along
    field plane n // field_group.  D_t as in `advect_reference`;  out[n, t - 1][p] = s_t(p - D_t(p)), s_t interpolating x[n, t - 1]."""
    x = np.asarray(x, dtype=np.float32)
    field = np.asarray(field, dtype=np.float32).astype(np.float64)
    field_group = int(field_group)
    if x.ndim != 4 or field.ndim != 4 or field.shape[-1] != 2 or field_group < 1 or x.shape[0] % field_group or \
            field.shape[0] not in (1, x.shape[0] // field_group):
        raise ValueError(f"x must be [N, T, H, W] and field [N / {field_group} or 1, Gy, Gx, 2], got {x.shape} and {field.shape}")
    n, steps, h, w = x.shape
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if not spacing > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    origin, spacing = float(np.float32(origin)), float(np.float32(spacing))
    with np.errstate(invalid="ignore"):
        x = np.where(x >= 0, x, np.float32(0)).astype(np.float64)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((n, steps, h, w))
    for i in range(n):
        f = field[i // field_group if field.shape[0] > 1 else 0]
        dy, dx = np.zeros((h, w)), np.zeros((h, w))
        for t in range(steps):
            v = _field_at(f, py - dy, px - dx, origin, spacing)
            dy, dx = dy + v[..., 0], dx + v[..., 1]
            out[i, t] = _sample(x[i, t], py - dy, px - dx)
    return out


def advect_series(x: torch.Tensor, field: torch.Tensor, origin: float = 0.0, spacing: float = 1.0, field_group: int = 1,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`advect_series_reference` for torch tensors -> fp32 [N, T, H, W] on the inputs' device.

    x: fp32 [N, T, H, W] whose planes are contiguous, with any non-negative strides over N and T (stride 0 over T: one source for all
    lead times, which is `advect`); any other layout is copied.  field: fp32 [N / field_group or 1, Gy, Gx, 2].  out: as in `advect`.
    On a HIP device one `dgmr_advect_series` on the current stream, nothing synchronised; on the CPU the float64 reference, rounded."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"x must be a float32 [N, T, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    n, steps, h, w = (int(v) for v in x.shape)
    field_group = int(field_group)
    if field_group < 1 or n % field_group:
        raise ValueError(f"field_group={field_group} must divide N={n}")
    planes = n // field_group
    if field.dim() != 4 or field.shape[-1] != 2 or field.shape[0] not in (1, planes) or field.dtype != torch.float32 or field.device != x.device:
        raise ValueError(f"field must be a float32 [{planes} or 1, Gy, Gx, 2] tensor on {x.device}, got {field.dtype} {tuple(field.shape)}")
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if not float(spacing) > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    if out is None:
        out = torch.empty((n, steps, h, w), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (n, steps, h, w) or out.dtype != torch.float32 or out.device != x.device or (w > 1 and out.stride(3) != 1)
          or (h > 1 and out.stride(2) != w) or (n > 1 and out.stride(0) < 0) or (steps > 1 and out.stride(1) < h * w)):
        raise ValueError(f"out must be a float32 [{n}, {steps}, {h}, {w}] tensor on {x.device} with contiguous planes")
    if not x.is_cuda:
        ref = advect_series_reference(x.numpy(), field.numpy(), origin, spacing, field_group)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    if (w > 1 and x.stride(3) != 1) or (h > 1 and x.stride(2) != w) or (n > 1 and x.stride(0) < 0) or (steps > 1 and x.stride(1) < 0):
        x = x.contiguous()
    if not field[0].is_contiguous() or (field.shape[0] > 1 and field.stride(0) < 0):
        field = field.contiguous()
    fs = int(field.stride(0)) if field.shape[0] > 1 else 0
    device = x.device
    with torch.cuda.device(device):
        call("dgmr_advect_series", x.data_ptr(), int(x.stride(0)) if n > 1 else 0, int(x.stride(1)) if steps > 1 else 0, field.data_ptr(),
             fs, field_group, n, h, w, int(field.shape[1]), int(field.shape[2]), float(origin), float(spacing), steps, out.data_ptr(),
             int(out.stride(0)) if n > 1 else 0, int(out.stride(1)) if steps > 1 else h * w, _stream(device))
    return out


def advect_series_perturbed_reference(x, field, direction, amplitude, origin: float = 0.0, spacing: float = 1.0,
                                      field_group: int = 1) -> np.ndarray:
    """The specification of `dgmr_advect_series_perturbed`, in float64 numpy -> float64 [N, T, H, W]: `advect_series_reference` with
    a velocity error per plane and lead time, along and across the local motion.

    x, field: as in `advect_series_reference`.  direction: [field's shape] = (uy, ux), unit vectors or (0, 0) (`unit_directions`),
    interpolated like the field; amplitude: [N, T, 2] = (a_par, a_perp) in pixels per step.  All inputs are rounded to fp32 first.
    At q = p - D_(t-1)(p):  v' = v(q) + a_par[n, t] u(q) + a_perp[n, t] (-ux(q), uy(q));  D_t = D_(t-1) + v'(q);
    out[n, t - 1][p] = s_t(p - D_t(p))."""
    x = np.asarray(x, dtype=np.float32)
    field = np.asarray(field, dtype=np.float32).astype(np.float64)
    direction = np.asarray(direction, dtype=np.float32).astype(np.float64)
    amplitude = np.asarray(amplitude, dtype=np.float32).astype(np.float64)
    field_group = int(field_group)
    if x.ndim != 4 or field.ndim != 4 or field.shape[-1] != 2 or field_group < 1 or x.shape[0] % field_group or \
            field.shape[0] not in (1, x.shape[0] // field_group):
        raise ValueError(f"x must be [N, T, H, W] and field [N / {field_group} or 1, Gy, Gx, 2], got {x.shape} and {field.shape}")
    if direction.shape != field.shape:
        raise ValueError(f"direction must have the field's shape {field.shape}, got {direction.shape}")
    n, steps, h, w = x.shape
    if amplitude.shape != (n, steps, 2):
        raise ValueError(f"amplitude must be [{n}, {steps}, 2], got {amplitude.shape}")
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if not spacing > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    origin, spacing = float(np.float32(origin)), float(np.float32(spacing))
    with np.errstate(invalid="ignore"):
        x = np.where(x >= 0, x, np.float32(0)).astype(np.float64)
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((n, steps, h, w))
    for i in range(n):
        plane = i // field_group if field.shape[0] > 1 else 0
        f, d = field[plane], direction[plane]
        dy, dx = np.zeros((h, w)), np.zeros((h, w))
        for t in range(steps):
            v = _field_at(f, py - dy, px - dx, origin, spacing)
            u = _field_at(d, py - dy, px - dx, origin, spacing)
            a_par, a_perp = amplitude[i, t]
            dy = dy + (v[..., 0] + (a_par * u[..., 0] - a_perp * u[..., 1]))
            dx = dx + (v[..., 1] + (a_par * u[..., 1] + a_perp * u[..., 0]))
            out[i, t] = _sample(x[i, t], py - dy, px - dx)
    return out


def advect_series_perturbed(x: torch.Tensor, field: torch.Tensor, direction: torch.Tensor, amplitude: torch.Tensor, origin: float = 0.0,
                            spacing: float = 1.0, field_group: int = 1, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`advect_series_perturbed_reference` for torch tensors -> fp32 [N, T, H, W] on the inputs' device.

    x, field, out: `advect_series`'s layouts and rules.  direction: fp32 of the field's shape on its device (`unit_directions(field)`);
    amplitude: fp32 [N, T, 2] = (a_par, a_perp) in pixels per step on the device (copied if not contiguous).  On a HIP device one
    `dgmr_advect_series_perturbed` on the current stream, nothing synchronised; on the CPU the float64 reference, rounded."""
    if x.dim() != 4 or x.dtype != torch.float32:
        raise ValueError(f"x must be a float32 [N, T, H, W] tensor, got {x.dtype} {tuple(x.shape)}")
    n, steps, h, w = (int(v) for v in x.shape)
    field_group = int(field_group)
    if field_group < 1 or n % field_group:
        raise ValueError(f"field_group={field_group} must divide N={n}")
    planes = n // field_group
    if field.dim() != 4 or field.shape[-1] != 2 or field.shape[0] not in (1, planes) or field.dtype != torch.float32 or field.device != x.device:
        raise ValueError(f"field must be a float32 [{planes} or 1, Gy, Gx, 2] tensor on {x.device}, got {field.dtype} {tuple(field.shape)}")
    if tuple(direction.shape) != tuple(field.shape) or direction.dtype != torch.float32 or direction.device != x.device:
        raise ValueError(f"direction must be a float32 {tuple(field.shape)} tensor on {x.device} like the field, got {direction.dtype} "
                         f"{tuple(direction.shape)} on {direction.device}")
    if tuple(amplitude.shape) != (n, steps, 2) or amplitude.dtype != torch.float32 or amplitude.device != x.device:
        raise ValueError(f"amplitude must be a float32 [{n}, {steps}, 2] tensor on {x.device}, got {amplitude.dtype} "
                         f"{tuple(amplitude.shape)} on {amplitude.device}")
    if not 1 <= steps <= MAX_STEPS:
        raise ValueError(f"T={steps}, 1 ... {MAX_STEPS} are supported")
    if not float(spacing) > 0:
        raise ValueError(f"spacing={spacing} must be positive")
    if out is None:
        out = torch.empty((n, steps, h, w), dtype=torch.float32, device=x.device)
    elif (tuple(out.shape) != (n, steps, h, w) or out.dtype != torch.float32 or out.device != x.device or (w > 1 and out.stride(3) != 1)
          or (h > 1 and out.stride(2) != w) or (n > 1 and out.stride(0) < 0) or (steps > 1 and out.stride(1) < h * w)):
        raise ValueError(f"out must be a float32 [{n}, {steps}, {h}, {w}] tensor on {x.device} with contiguous planes")
    if not x.is_cuda:
        ref = advect_series_perturbed_reference(x.numpy(), field.numpy(), direction.numpy(), amplitude.numpy(), origin, spacing, field_group)
        out.copy_(torch.from_numpy(ref.astype(np.float32)))
        return out
    from ._lib import call

    if (w > 1 and x.stride(3) != 1) or (h > 1 and x.stride(2) != w) or (n > 1 and x.stride(0) < 0) or (steps > 1 and x.stride(1) < 0):
        x = x.contiguous()
    if not field[0].is_contiguous() or (field.shape[0] > 1 and field.stride(0) < 0):
        field = field.contiguous()
    if not direction[0].is_contiguous() or (direction.shape[0] > 1 and direction.stride(0) < 0):
        direction = direction.contiguous()
    amplitude = amplitude.contiguous()
    fs = int(field.stride(0)) if field.shape[0] > 1 else 0
    ds = int(direction.stride(0)) if direction.shape[0] > 1 else 0
    device = x.device
    with torch.cuda.device(device):
        call("dgmr_advect_series_perturbed", x.data_ptr(), int(x.stride(0)) if n > 1 else 0, int(x.stride(1)) if steps > 1 else 0,
             field.data_ptr(), fs, direction.data_ptr(), ds, amplitude.data_ptr(), field_group, n, h, w, int(field.shape[1]),
             int(field.shape[2]), float(origin), float(spacing), steps, out.data_ptr(), int(out.stride(0)) if n > 1 else 0,
             int(out.stride(1)) if steps > 1 else h * w, _stream(device))
    return out


def unit_directions(field: torch.Tensor, floor: float = 0.0) -> torch.Tensor:
    """The direction of motion per lattice node -> fp32 of `field`'s shape ([..., 2] = (vy, vx)): v / |v|, formed in float64 and rounded
    once; (0, 0) where |v| <= floor or a component is not finite - a calm or unusable node is not perturbed
    (`advect_series_perturbed`).  torch on the lattice, the same code for CPU and HIP tensors, like `motion_field`."""
    if field.dim() < 1 or field.shape[-1] != 2 or not field.dtype.is_floating_point:
        raise ValueError(f"field must be a floating-point [..., 2] tensor, got {field.dtype} {tuple(field.shape)}")
    if not float(floor) >= 0:
        raise ValueError(f"floor={floor} must not be negative")
    v = field.to(torch.float64)
    norm = torch.sqrt((v * v).sum(dim=-1, keepdim=True))
    ok = torch.isfinite(v).all(dim=-1, keepdim=True) & (norm > float(floor))
    u = torch.where(ok, v, torch.zeros_like(v)) / torch.where(ok, norm, torch.ones_like(norm))
    return u.to(torch.float32).contiguous()


# ---- motion field ----------------------------------------------------------------------------------------------------------------
def _box_sum(a: torch.Tensor, radius: int) -> torch.Tensor:
    """Sums over (2 radius + 1)^2 lattice nodes around every node of a [..., By, Bx] tensor (zeros beyond the edge), by prefix sums."""
    for dim in (-2, -1):
        size = a.shape[dim]
        pad = [0, 0] * a.dim()
        pad[2 * (-dim - 1)] = radius + 1
        pad[2 * (-dim - 1) + 1] = radius
        cs = torch.nn.functional.pad(a, pad).cumsum(dim)
        a = cs.narrow(dim, 2 * radius + 1, size) - cs.narrow(dim, 0, size)
    return a


def _subpixel(c0, cm, cp):
    """The minimum of the parabola through the costs at -1, 0, +1, clipped to +-0.5; 0 where the three do not curve upwards."""
    den = cm - 2.0 * c0 + cp
    ok = den > 0
    return torch.where(ok, (0.5 * (cm - cp) / torch.where(ok, den, torch.ones_like(den))).clamp(-0.5, 0.5), torch.zeros_like(den))


def motion_field(frames: torch.Tensor, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                 min_wet: Optional[int] = None, smooth: int = 2, subpixel: str = "parabola", lk_iterations: int = 4,
                 eig_ratio: float = 0.01) -> torch.Tensor:
    """Motion in pixels per frame on the block lattice: fp32 [N, By, Bx, 2] = (vy, vx); node (by, bx) stands for the block's centre,
    pixel ((block - 1) / 2 + by stride, (block - 1) / 2 + bx stride) - `advect`'s origin and spacing (`lattice_geometry`).

    frames: fp32 [T_in >= 2, N, H, W], the context in time order.  One `block_match` call over all T_in - 1 consecutive pairs and all
    planes.  A block of a pair is usable when it is not dry and its minimum is interior (all four neighbour costs finite); its
    vector is the integer displacement plus, per axis, clip(0.5 (c- - c+) / (c- - 2 c0 + c+), +-0.5) where that denominator is
    positive (else 0).  The pairs are averaged, weighted by usability; then a normalised box smoothing over (2 smooth + 1)^2 nodes,
    sum w v / sum w with w = 1 at nodes that had a usable pair; nodes with no usable neighbour take the plane's mean usable vector,
    (0, 0) if there is none.  All of this after `block_match` is torch in float64 on the lattice, on the frames' device.

    subpixel="lk" (the parabola is biased towards the integer by up to a third of a pixel; the lead time multiplies that): one
    `lk_refine` with lk_iterations and eig_ratio over the same pairs after the `block_match`; a block is usable when it is usable
    above AND conditioned (`lk_conditioned`: a block of stripes says nothing about the motion along them, and block matching's
    exact 0 there is no measurement), and its vector is the refinement's v.  Averaging, smoothing and fill are the same."""
    if frames.dim() != 4 or frames.shape[0] < 2 or frames.dtype != torch.float32:
        raise ValueError(f"frames must be a float32 [T_in >= 2, N, H, W] tensor, got {frames.dtype} {tuple(frames.shape)}")
    if smooth < 0:
        raise ValueError(f"smooth={smooth} must not be negative")
    if subpixel not in SUBPIXEL:
        raise ValueError(f"subpixel={subpixel!r}, {SUBPIXEL} are supported")
    frames = frames.contiguous()
    pairs, n, h, w = frames.shape[0] - 1, *(int(v) for v in frames.shape[1:])
    res = block_match(frames[:-1].reshape(pairs * n, h, w), frames[1:].reshape(pairs * n, h, w), block, stride, radius, wet_threshold,
                      min_wet)
    by, bx = res.wet.shape[1:]
    cost = res.cost.view(pairs, n, by, bx, 5).to(torch.float64)
    disp = res.disp.view(pairs, n, by, bx, 2).to(torch.float64)
    usable = torch.isfinite(cost).all(dim=-1)
    if subpixel == "lk":
        lk = lk_refine(frames[:-1].reshape(pairs * n, h, w), frames[1:].reshape(pairs * n, h, w), res, block, stride, lk_iterations,
                       eig_ratio)
        usable = usable & lk_conditioned(lk.eig, eig_ratio).view(pairs, n, by, bx)
        v = lk.v.view(pairs, n, by, bx, 2).to(torch.float64)
    else:
        c = torch.where(usable[..., None], cost, torch.zeros_like(cost))
        v = disp + torch.stack([_subpixel(c[..., 0], c[..., 1], c[..., 2]), _subpixel(c[..., 0], c[..., 3], c[..., 4])], dim=-1)
    u = usable.to(torch.float64)
    count = u.sum(dim=0)                                   # [N, By, Bx]
    have = count > 0
    mean = (v * u[..., None]).sum(dim=0) / count.clamp_min(1.0)[..., None]
    wgt = have.to(torch.float64)
    num = _box_sum((mean * wgt[..., None]).permute(0, 3, 1, 2), smooth).permute(0, 2, 3, 1)
    den = _box_sum(wgt, smooth)
    total = wgt.sum(dim=(1, 2))
    plane_mean = (mean * wgt[..., None]).sum(dim=(1, 2)) / total.clamp_min(1.0)[:, None]  # (0, 0) without a usable node
    near = den > 0.5
    field = torch.where(near[..., None], num / den.clamp_min(1.0)[..., None], plane_mean[:, None, None, :].expand_as(num))
    return field.to(torch.float32).contiguous()


def lattice_geometry(block: int, stride: int):
    """(origin, spacing) of `motion_field`'s lattice for `advect`: the block centres."""
    return (block - 1) / 2.0, float(stride)


def persistence_nowcast(last: torch.Tensor, forecast_steps: int) -> torch.Tensor:
    """Eulerian persistence: last [C, H, W] -> [1, T, C, H, W]; last [B, C, H, W] -> [1, B, T, C, H, W] - the last frame at every lead
    time, as an expanded VIEW of one copy in which missing elements (`!(x >= 0)`) are 0."""
    if last.dim() not in (3, 4):
        raise ValueError(f"last must be [C, H, W] or [B, C, H, W], got shape {tuple(last.shape)}")
    x = torch.where(last >= 0, last, torch.zeros_like(last)).float()
    if last.dim() == 3:
        return x[None, None].expand(1, int(forecast_steps), *x.shape)
    return x[None, :, None].expand(1, x.shape[0], int(forecast_steps), *x.shape[1:])


class AdvectionNowcaster:
    """Lagrangian persistence: the motion of the last (at most 4) context frames by `motion_field`, the last frame extrapolated along
    it by `advect` for `forecast_steps` lead times.  One member: no growth or decay, no perturbation.  `last_field`: the motion field
    of the latest call, [planes, By, Bx, 2] in pixels per frame, planes in (B, C) order.  subpixel, lk_iterations, eig_ratio
    (keyword-only, or `refine_motion` later): `motion_field`'s; the default "parabola" is the field of before, "lk" the Lucas-Kanade
    refinement."""

    def __init__(self, forecast_steps: int = 18, block: int = 32, stride: int = 16, radius: int = 8, wet_threshold: float = 0.1,
                 min_wet: Optional[int] = None, smooth: int = 2, *, subpixel: str = "parabola", lk_iterations: int = 4,
                 eig_ratio: float = 0.01):
        if not 1 <= int(forecast_steps) <= MAX_STEPS:
            raise ValueError(f"forecast_steps={forecast_steps}, 1 ... {MAX_STEPS} are supported")
        self.forecast_steps = int(forecast_steps)
        self.params = dict(block=block, stride=stride, radius=radius, wet_threshold=wet_threshold, min_wet=min_wet, smooth=smooth)
        self.refine_motion(subpixel, lk_iterations, eig_ratio)
        self.last_field = None

    def refine_motion(self, subpixel: str = "lk", lk_iterations: int = 4, eig_ratio: float = 0.01):
        """Choose `motion_field`'s sub-pixel method -> self, for `EnsembleAdvectionNowcaster(...).refine_motion()`: "lk" (the
        Lucas-Kanade refinement, with lk_iterations and eig_ratio) or "parabola" (the field of before).  Kept in `params`, which
        every `motion_field` call of the nowcaster takes.  (A method beside the constructor's keywords: a subclass whose positional
        order is fixed has no room for them.)"""
        if subpixel not in SUBPIXEL:
            raise ValueError(f"subpixel={subpixel!r}, {SUBPIXEL} are supported")
        _check_lk(lk_iterations, eig_ratio)
        self.params.update(subpixel=subpixel, lk_iterations=int(lk_iterations), eig_ratio=float(eig_ratio))
        return self

    def _run(self, context: torch.Tensor, out: torch.Tensor, planes_per_case: int) -> None:
        """context [T_in, B * C, H, W]; out [B, T, C, H, W]"""
        self.last_field = motion_field(context[-CONTEXT_FRAMES:], **self.params)
        origin, spacing = lattice_geometry(self.params["block"], self.params["stride"])
        b, c = out.shape[0], planes_per_case
        last = context[-1].view(b, c, *context.shape[2:])
        field = self.last_field.view(b, c, *self.last_field.shape[1:])
        for ch in range(c):  # planes of one channel are equally far apart in the output: one launch per channel
            advect(last[:, ch], field[:, ch], self.forecast_steps, origin, spacing, out=out[:, :, ch])

    def nowcast(self, frames, scale: float = 1.0, offset: float = 0.0) -> torch.Tensor:
        """frames [T_in >= 2, H, W, C] in a storage dtype (numpy or torch; converted as `verification.observed_from_frames` does,
        missing elements stay missing for the matching's rule) -> fp32 [1, forecast_steps, C, H, W] on the frames' device."""
        from .verification import observed_from_frames

        x = observed_from_frames(frames, scale, offset)  # [T_in, C, H, W]
        if x.shape[0] < 2:
            raise ValueError(f"frames holds {x.shape[0]} frames, the motion needs 2")
        out = torch.empty((1, self.forecast_steps) + tuple(x.shape[1:]), dtype=torch.float32, device=x.device)
        self._run(x, out, int(x.shape[1]))
        return out

    def nowcast_batch(self, images: torch.Tensor) -> torch.Tensor:
        """images fp32 [B, T_in >= 2, C, H, W] -> fp32 [1, B, forecast_steps, C, H, W]."""
        if images.dim() != 5 or images.shape[1] < 2 or images.dtype != torch.float32:
            raise ValueError(f"images must be a float32 [B, T_in >= 2, C, H, W] tensor, got {images.dtype} {tuple(images.shape)}")
        b, _, c, h, w = images.shape
        context = images[:, -CONTEXT_FRAMES:].permute(1, 0, 2, 3, 4).reshape(-1, b * c, h, w).contiguous()
        out = torch.empty((1, b, self.forecast_steps, c, h, w), dtype=torch.float32, device=images.device)
        self._run(context, out[0], int(c))
        return out
