"""Tiled full-frame nowcasts, host side: the tiling arithmetic (origins, blending weights, the latent field), the generic driver
`nowcast_tiled` on CPU tensors with stub models, and `dgmr_tile_blend` at the C-ABI boundary.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from skillful_nowcasting_amd.tiling import blend_tile, blend_weights, latent_field, nowcast_tiled, tile_origins

EPS = 2.0 ** -24
GEOMETRIES = [(1536, 256, 192), (1280, 256, 192), (224, 128, 96), (192, 64, 32), (128, 32, 32), (160, 96, 32)]


# ---- origins ---------------------------------------------------------------------------------------------------------------------
def test_tile_origins_examples():
    assert tile_origins(1536, 256, 192) == [0, 192, 384, 576, 768, 960, 1152, 1280]
    assert tile_origins(256, 256, 192) == [0]
    assert tile_origins(224, 128, 96) == [0, 96]
    assert tile_origins(128, 32, 32) == [0, 32, 64, 96]
    assert tile_origins(1280, 256, 192) == [0, 192, 384, 576, 768, 960, 1024]


@pytest.mark.parametrize("args", [
    (250, 128, 96), (256, 100, 96), (256, 128, 90),   # not on the 32-pixel lattice
    (0, 128, 96), (256, 0, 96), (256, 128, 0), (-256, 128, 96), (256, -128, 96), (256, 128, -96),  # not positive
    (256, 128, 160),                                    # stride > tile
    (96, 128, 96),                                      # extent < tile
    (256.0, 128, 96), (256, 128, True),                 # not integers
])
def test_tile_origins_refuses(args):
    with pytest.raises(ValueError):
        tile_origins(*args)
    with pytest.raises(ValueError):
        blend_weights(*args)


# ---- weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extent,tile,stride", GEOMETRIES)
def test_blend_weights_are_a_positive_partition_of_unity(extent, tile, stride):
    origins, w = blend_weights(extent, tile, stride)
    assert origins == tile_origins(extent, tile, stride)
    assert w.dtype == np.float32 and w.shape == (len(origins), tile)
    assert (w > 0).all()
    total = np.zeros(extent, dtype=np.float64)
    cover = np.zeros(extent, dtype=np.int64)
    for a, o in enumerate(origins):
        total[o:o + tile] += w[a].astype(np.float64)
        cover[o:o + tile] += 1
    assert cover.min() >= 1
    assert np.abs(total - 1.0).max() <= 4 * EPS
    for a, o in enumerate(origins):  # exactly 1 where a single tile covers
        single = cover[o:o + tile] == 1
        assert (w[a][single] == np.float32(1.0)).all()
    if (extent, tile, stride) == (128, 32, 32):
        assert cover.max() == 1 and (w == np.float32(1.0)).all()
    if (extent, tile, stride) == (160, 96, 32):
        assert cover.max() == 3  # three tiles cover some pixels


def test_blend_weights_follow_the_ramp_definition():
    """(224, 128, 96): two tiles that overlap by 32 pixels; in the overlap the raw windows are the ramp and its mirror image."""
    origins, w = blend_weights(224, 128, 96)
    assert origins == [0, 96]
    i = np.arange(32, dtype=np.float64)
    up, down = (i + 0.5) / 32, (32 - i - 0.5) / 32  # tile 1's left ramp, tile 0's right ramp over coordinates 96 ... 127
    assert np.array_equal(w[1][:32], (up / (up + down)).astype(np.float32))
    assert np.array_equal(w[0][96:], (down / (up + down)).astype(np.float32))
    assert (w[0][:96] == 1).all() and (w[1][32:] == 1).all()
    # the last tile of (1280, 256, 192) is shifted inwards: it overlaps its predecessor by 192 pixels, not by 64
    origins, w = blend_weights(1280, 256, 192)
    assert origins[-2:] == [960, 1024] and (w[-1][192:] == 1).all() and (w[-1][:192] < 1).all()


# ---- the latent field ------------------------------------------------------------------------------------------------------------
def test_latent_field_shape_and_seed():
    a = latent_field(3, 8, 7, 5, torch.Generator().manual_seed(11))
    b = latent_field(3, 8, 7, 5, torch.Generator().manual_seed(11))
    c = latent_field(3, 8, 7, 5, torch.Generator().manual_seed(12))
    assert a.shape == (3, 8, 7, 5) and a.dtype == torch.float32 and a.device.type == "cpu"
    assert torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(a, torch.randn((3, 8, 7, 5), generator=torch.Generator().manual_seed(11)))
    with pytest.raises(ValueError):
        latent_field(0, 8, 7, 5)


# ---- the driver on the CPU -------------------------------------------------------------------------------------------------------
K, T_OUT, C = 2, 3, 1


def _frames(h, w, t_in=4, dtype=torch.float32, seed=0):
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.int16:
        return torch.randint(-64, 1024, (t_in, h, w, C), generator=g, dtype=torch.int16)
    return torch.rand((t_in, h, w, C), generator=g)


def test_constant_model_gives_the_constant_everywhere():
    seen = []

    def tile_fn(context, z):
        seen.append((tuple(context.shape), tuple(z.shape)))
        return torch.full((K, T_OUT, C, 64, 64), 3.25)

    out = nowcast_tiled(tile_fn, _frames(128, 192), latent_field(K, 8, 4, 6), 64, 32, T_OUT)
    assert out.shape == (K, T_OUT, C, 128, 192) and out.dtype == torch.float32
    assert len(seen) == 3 * 5 and set(seen) == {((1, 4, C, 64, 64), (K, 8, 2, 2))}
    assert (out - 3.25).abs().max().item() <= 1e-6


def test_single_tile_is_the_models_output_exactly():
    frames, zs = _frames(64, 64), latent_field(K, 8, 2, 2, torch.Generator().manual_seed(3))
    pred = torch.randn(K, T_OUT, C, 64, 64, generator=torch.Generator().manual_seed(4))
    got = {}

    def tile_fn(context, z):
        got["context"], got["z"] = context, z
        return pred

    out = nowcast_tiled(tile_fn, frames, zs, 64, 32, T_OUT)
    assert torch.equal(out, pred)
    assert torch.equal(got["context"], frames.permute(0, 3, 1, 2).unsqueeze(0)) and torch.equal(got["z"], zs)
    # a caller's buffer is zeroed up front and returned
    buf = torch.full((K, T_OUT, C, 64, 64), 7.0)
    assert nowcast_tiled(tile_fn, frames, zs, 64, 32, T_OUT, out=buf) is buf and torch.equal(buf, pred)


def test_tiles_cut_one_latent_field_on_the_lattice():
    """A model that returns its latent upsampled 32x: where two tiles overlap both hold the SAME values (each tile's latent is the
    part of one full-frame field under it), so the blend reproduces the upsampled field."""
    h, w, tile, stride = 128, 224, 128, 96
    zs = latent_field(K, 8, h // 32, w // 32, torch.Generator().manual_seed(5))
    tiles = []

    def tile_fn(context, z):
        up = z[:, :1].repeat_interleave(32, dim=2).repeat_interleave(32, dim=3)  # [K, 1, tile, tile]
        pred = up.unsqueeze(1).expand(K, T_OUT, C, tile, tile).contiguous()
        tiles.append(pred)
        return pred

    out = nowcast_tiled(tile_fn, _frames(h, w), zs, tile, stride, T_OUT)
    assert len(tiles) == 2  # column origins 0 and 96: columns 96 ... 127 are covered by both
    assert torch.equal(tiles[0][..., 96:128], tiles[1][..., 0:32])
    full = zs[:, :1].repeat_interleave(32, dim=2).repeat_interleave(32, dim=3).unsqueeze(1).expand(K, T_OUT, C, h, w)
    assert (out - full).abs().max().item() <= 1e-6


def test_storage_dtype_path_equals_preconverted_frames():
    raw = _frames(96, 128, t_in=4, dtype=torch.int16, seed=6)
    assert (raw < 0).any()
    phys = raw.float() * (1 / 32)
    phys = torch.where(phys >= 0, phys, torch.zeros_like(phys))
    zs = latent_field(K, 8, 3, 4, torch.Generator().manual_seed(7))

    def tile_fn(context, z):  # depends on the context and on the latent
        return (context.mean(dim=1, keepdim=True) + z[:, :1].mean(dim=(2, 3), keepdim=True).unsqueeze(1)).expand(K, T_OUT, C, 64, 64)

    a = nowcast_tiled(tile_fn, raw, zs, 64, 32, T_OUT, scale=1 / 32, clamp_missing=True)
    b = nowcast_tiled(tile_fn, phys, zs, 64, 32, T_OUT)
    assert torch.equal(a, b)
    assert not torch.equal(a, nowcast_tiled(tile_fn, raw, zs, 64, 32, T_OUT, scale=1 / 32, clamp_missing=False))


def test_driver_and_blend_refuse_bad_arguments():
    def tile_fn(context, z):
        return torch.zeros(K, T_OUT, C, 64, 64)

    zs = latent_field(K, 8, 4, 4)
    with pytest.raises(ValueError):
        nowcast_tiled(tile_fn, _frames(120, 128), zs, 64, 32, T_OUT)  # height off the lattice
    with pytest.raises(ValueError):
        nowcast_tiled(tile_fn, _frames(128, 128), latent_field(K, 8, 4, 3), 64, 32, T_OUT)  # latent field of another frame
    with pytest.raises(ValueError):
        nowcast_tiled(tile_fn, _frames(128, 128), zs, 64, 32, T_OUT + 1)  # the model returns another number of steps
    with pytest.raises(ValueError):
        nowcast_tiled(tile_fn, _frames(128, 128), zs, 64, 32, T_OUT, out=torch.zeros(K, T_OUT, C, 128, 64))
    pred, out, wt = torch.zeros(2, 32, 32), torch.zeros(2, 64, 64), torch.ones(32)
    blend_tile(pred, out, wt, wt, 32, 32)
    for bad in (dict(pred=pred.double()), dict(pred=torch.zeros(3, 32, 32)), dict(pred=torch.zeros(2, 32, 64)[:, :, :32]),
                dict(wy=torch.ones(31)), dict(oy=33), dict(ox=36), dict(ox=30), dict(oy=-1), dict(out=None), dict(out=out.numpy())):
        kw = dict(pred=pred, out=out, wy=wt, wx=wt, oy=0, ox=0)
        kw.update(bad)
        with pytest.raises(ValueError):
            blend_tile(**kw)


def test_cpu_blend_is_the_formula():
    g = torch.Generator().manual_seed(8)
    pred, out = torch.randn(3, 32, 32, generator=g), torch.randn(3, 64, 96, generator=g)
    wy, wx = torch.rand(32, generator=g), torch.rand(32, generator=g)
    before = out.clone()
    blend_tile(pred, out, wy, wx, 32, 64)
    want = before.double()
    want[:, 32:, 64:] += (wy[:, None] * wx[None, :]).double() * pred.double()
    assert (out.double() - want).abs().max().item() <= 1e-6 * pred.abs().max().item()
    mask = torch.ones_like(out, dtype=torch.bool)
    mask[:, 32:, 64:] = False
    assert torch.equal(out[mask], before[mask])


# ---- the C-ABI boundary ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()  # hipcc cross-compiles gfx950 without a GPU
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_symbol_is_exported_bound_and_declared(lib):
    from conftest import ROOT
    from skillful_nowcasting_amd import _lib

    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dgmr_hip.h")).read(), flags=re.S)
    assert hasattr(lib, "dgmr_tile_blend")
    assert len(_lib.SIGNATURES["dgmr_tile_blend"]) == 11
    m = re.search(r"\bint dgmr_tile_blend\s*\((.*?)\);", src, flags=re.S)
    assert m is not None and len(m.group(1).split(",")) == 11
    assert lib.dgmr_abi_version() == _lib.ABI_VERSION


def test_tile_blend_reports_argument_errors_without_a_gpu(lib):
    """Null pointers, non-positive extents, tile / ox / W off the 16-byte grid and a tile outside the frame are refused before any
    launch: rc < 0 and a message."""
    buf = (ctypes.c_double * 16)()  # stands for any non-null pointer: a refused call reads nothing
    p = ctypes.cast(buf, ctypes.c_void_p)

    def blend(pred=p, out=p, wy=p, wx=p, planes=2, tile=32, h=64, w=96, oy=0, ox=0):
        return lib.dgmr_tile_blend(pred, out, wy, wx, planes, tile, h, w, oy, ox, None)

    for bad in (dict(pred=None), dict(out=None), dict(wy=None), dict(wx=None),
                dict(planes=0), dict(planes=-1), dict(tile=0), dict(tile=-32), dict(h=0), dict(w=0), dict(h=-64),
                dict(tile=30), dict(ox=2), dict(w=98),
                dict(oy=-1), dict(oy=33), dict(ox=-4), dict(ox=68), dict(tile=128), dict(oy=2 ** 31 - 16)):
        assert blend(**bad) < 0, bad
        assert b"dgmr_tile_blend" in lib.dgmr_last_error(), bad
    assert blend(pred=None) < 0 and b"null" in lib.dgmr_last_error()
    assert blend(tile=30) < 0 and b"multiples of 4" in lib.dgmr_last_error()
    assert blend(oy=33) < 0 and b"not inside" in lib.dgmr_last_error()
    if p.value % 16 == 0:
        off = ctypes.c_void_p(p.value + 4)
        assert blend(wx=off) < 0 and b"aligned" in lib.dgmr_last_error()
