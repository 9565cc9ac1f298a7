"""Full-frame ensemble nowcasts from a square model, by overlapping tiles that share one latent field.

The generator is trained (and parity-tested) on square crops; a radar composite is 1536 x 1280.  `nowcast_tiled` runs the model on
overlapping `tile`-sized tiles of the frame, every tile's context cut on the device by `dgmr_crop_gather`, and adds each tile's
forecast into the frame with separable weights that sum to one at every pixel (`dgmr_tile_blend`: one streaming launch per tile, no
weight-sum plane and no normalising pass).  Every ensemble member has ONE latent map for the whole frame (`latent_field`), and a
tile's latent is the part of it under the tile: tiles, strides and frame extents are multiples of 32 pixels, the latent's resolution,
so two tiles that overlap read the same noise in the cells they share.

What this does not do (INTEGRATION.md "Nowcasting a full frame"): the latent stack attends over its whole map, so two tiles' forecasts
are strongly correlated where they overlap but not identical, and a tile edge inside the frame sees zero padding where its neighbour
would be.  The ramps give those pixels the least weight: seams are reduced, not eliminated.
"""
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

LATTICE = 32  # pixels per latent cell (LatentConditioningStack: shape = (8 * C, size // 32, size // 32))


def tile_origins(extent: int, tile: int, stride: int) -> List[int]:
    """Top-left coordinates of the tiles along one axis: 0, stride, 2 * stride, ... while a tile starting there ends inside the
    extent, then one last tile shifted inwards so that it ends at the border.  `extent == tile` gives [0]."""
    for name, v in (("extent", extent), ("tile", tile), ("stride", stride)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v <= 0 or v % LATTICE != 0:
            raise ValueError(f"{name}={v!r} must be a positive multiple of {LATTICE}")
    extent, tile, stride = int(extent), int(tile), int(stride)
    if stride > tile:
        raise ValueError(f"stride={stride} exceeds tile={tile}: pixels between two tiles would get no forecast")
    if extent < tile:
        raise ValueError(f"extent={extent} is smaller than tile={tile}")
    return list(range(0, extent - tile, stride)) + [extent - tile]


def blend_weights(extent: int, tile: int, stride: int) -> Tuple[List[int], np.ndarray]:
    """(origins, w): w float32 [n_tiles, tile], the normalised blending weight of pixel i of tile a along one axis.

    Raw window of tile a: 1 in the interior; where the previous tile overlaps it by L > 0 pixels a ramp min(1, (i + 0.5) / L), where
    the next one overlaps it by R > 0 pixels the mirror image min(1, (tile - i - 0.5) / R), the minimum of the two where both apply;
    no ramp on a side that lies on the border.  w[a][i] = raw_a(i) / sum of raw_b over the tiles b that cover coordinate o_a + i, in
    float64, rounded to float32 once: every weight is > 0, a coordinate under one tile has weight exactly 1, and the tiles being the
    Cartesian product of row and column origins, wy[a][i] * wx[b][j] is the normalised 2-D weight."""
    origins = tile_origins(extent, tile, stride)
    n = len(origins)
    i = np.arange(tile, dtype=np.float64)
    raw = np.ones((n, tile), dtype=np.float64)
    for a, o in enumerate(origins):
        if a > 0 and origins[a - 1] + tile - o > 0:
            raw[a] = np.minimum(raw[a], np.minimum(1.0, (i + 0.5) / (origins[a - 1] + tile - o)))
        if a + 1 < n and o + tile - origins[a + 1] > 0:
            raw[a] = np.minimum(raw[a], np.minimum(1.0, (tile - i - 0.5) / (o + tile - origins[a + 1])))
    total = np.zeros(extent, dtype=np.float64)
    for a, o in enumerate(origins):
        total[o:o + tile] += raw[a]
    w = np.stack([raw[a] / total[o:o + tile] for a, o in enumerate(origins)])
    return origins, w.astype(np.float32)


def latent_field(num_samples: int, channels: int, h32: int, w32: int, generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """One latent map per ensemble member for the WHOLE frame, [num_samples, channels, h32, w32] standard normal on the CPU (the
    model's latents come from the CPU generator as well); channels = 8 * input_channels, h32 = H // 32, w32 = W // 32."""
    if min(int(num_samples), int(channels), int(h32), int(w32)) < 1:
        raise ValueError(f"latent_field: extents ({num_samples}, {channels}, {h32}, {w32}) must be positive")
    return torch.randn((int(num_samples), int(channels), int(h32), int(w32)), generator=generator)


def blend_tile(pred: torch.Tensor, out: torch.Tensor, wy: torch.Tensor, wx: torch.Tensor, oy: int, ox: int) -> torch.Tensor:
    """out[..., oy + i, ox + j] = fma(wy[i] * wx[j], pred[..., i, j], out[..., oy + i, ox + j]), the weight rounded to fp32 first.
    pred [..., tile, tile] and out [..., H, W] with the same leading extents, wy and wx [tile]; all contiguous float32 on one device.
    On a HIP device this is `dgmr_tile_blend` on the current stream; CPU tensors take the torch expression of the same arithmetic."""
    if not isinstance(out, torch.Tensor):
        raise ValueError(f"blend_tile: out must be a tensor, got {type(out).__name__}")
    for name, t in (("pred", pred), ("out", out), ("wy", wy), ("wx", wx)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != out.device:
            raise ValueError(f"blend_tile: {name} must be a contiguous float32 tensor on {out.device}")
    if pred.dim() < 2 or pred.dim() != out.dim() or pred.shape[-1] != pred.shape[-2] or pred.shape[:-2] != out.shape[:-2]:
        raise ValueError(f"blend_tile: pred {tuple(pred.shape)} is not [..., tile, tile] with the leading extents of out {tuple(out.shape)}")
    tile, (h, w) = int(pred.shape[-1]), (int(v) for v in out.shape[-2:])
    if tuple(wy.shape) != (tile,) or tuple(wx.shape) != (tile,):
        raise ValueError(f"blend_tile: wy {tuple(wy.shape)} and wx {tuple(wx.shape)} must both be [{tile}]")
    oy, ox = int(oy), int(ox)
    if tile < 1 or tile % 4 or ox % 4 or w % 4:
        raise ValueError(f"blend_tile: tile={tile}, ox={ox} and W={w} must be multiples of 4")
    if oy < 0 or ox < 0 or oy + tile > h or ox + tile > w:
        raise ValueError(f"blend_tile: tile {tile} at (oy={oy}, ox={ox}) is not inside the frame {h} x {w}")
    planes = pred.numel() // (tile * tile)
    if planes == 0:
        return out
    if not out.is_cuda:
        out[..., oy:oy + tile, ox:ox + tile] += (wy[:, None] * wx[None, :]) * pred
        return out
    from ._lib import call
    from .data import _launch_stream

    with torch.cuda.device(out.device):
        call("dgmr_tile_blend", pred.data_ptr(), out.data_ptr(), wy.data_ptr(), wx.data_ptr(), planes, tile, h, w, oy, ox, _launch_stream())
    return out


def nowcast_tiled(tile_fn: Callable, frames: torch.Tensor, zs: torch.Tensor, tile: int, stride: int, forecast_steps: int,
                  scale: float = 1.0, offset: float = 0.0, clamp_missing: bool = True, missing_fill: float = 0.0,
                  out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The tiled nowcast of one sequence -> fp32 [K, forecast_steps, C, H, W].

    frames: the context [T_in, H, W, C] in its storage dtype (uint8 / int16 / float16 / float32), as rows arrive; `scale`, `offset`,
    `clamp_missing`, `missing_fill` as in `data.gather_crops`, which cuts every tile's context.  zs: the latent field [K, 8 * C,
    H // 32, W // 32] on the frames' device.  Tiles are visited in raster order (row origins outer, column origins inner); for each,
    `tile_fn(context [1, T_in, C, tile, tile], z [K, 8 * C, tile // 32, tile // 32])` returns the K forecasts [K, forecast_steps, C,
    tile, tile], which `blend_tile` adds into `out` (zeroed once up front; allocated here unless given)."""
    from .data import gather_crops

    if frames.dim() != 4:
        raise ValueError(f"frames must be [T, H, W, C], got shape {tuple(frames.shape)}")
    t_in, h, w, c = (int(v) for v in frames.shape)
    ys, wy = blend_weights(h, tile, stride)
    xs, wx = blend_weights(w, tile, stride)
    tile, t_out = int(tile), int(forecast_steps)
    if t_out < 1:
        raise ValueError(f"forecast_steps={forecast_steps} must be positive")
    if zs.dim() != 4 or tuple(zs.shape[2:]) != (h // LATTICE, w // LATTICE) or zs.shape[0] < 1 or zs.device != frames.device:
        raise ValueError(f"zs {tuple(zs.shape)} on {zs.device} must be [K, channels, {h // LATTICE}, {w // LATTICE}] on {frames.device}")
    k = int(zs.shape[0])
    shape = (k, t_out, c, h, w)
    if out is None:
        out = torch.zeros(shape, dtype=torch.float32, device=frames.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != frames.device:
        raise ValueError(f"out must be a contiguous float32 {shape} tensor on {frames.device}")
    else:
        out.zero_()
    wy_dev, wx_dev = torch.from_numpy(wy).to(frames.device), torch.from_numpy(wx).to(frames.device)
    cells = tile // LATTICE
    for a, oy in enumerate(ys):
        for b, ox in enumerate(xs):
            context = gather_crops(frames, [(oy, ox)], tile, scale, offset, clamp_missing, missing_fill)
            z = zs[:, :, oy // LATTICE:oy // LATTICE + cells, ox // LATTICE:ox // LATTICE + cells].contiguous()
            pred = tile_fn(context, z)
            if tuple(pred.shape) != (k, t_out, c, tile, tile):
                raise ValueError(f"tile_fn returned {tuple(pred.shape)}, expected {(k, t_out, c, tile, tile)}")
            blend_tile(pred.float().contiguous(), out, wy_dev[a], wx_dev[b], oy, ox)
    return out
