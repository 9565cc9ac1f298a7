"""Tiled full-frame nowcasts on the GPU: dgmr_tile_blend against a float64 evaluation of its formula, and DGMR.nowcast_full_frame
against the generator's own forward_draws on the tiles it is made of."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KW = dict(forecast_steps=3, output_shape=128, latent_channels=256, context_channels=128)


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
def _blend_all(lead, tile, h, w, stride, seed):
    """Every tile of the frame blended on the device in raster order -> (out, [(oy, ox, wy, wx, pred)] on the host)."""
    from skillful_nowcasting_amd.tiling import blend_tile, blend_weights

    ys, wy = blend_weights(h, tile, stride)
    xs, wx = blend_weights(w, tile, stride)
    g = torch.Generator().manual_seed(seed)
    out = torch.zeros(*lead, h, w, device="cuda")
    wy_dev, wx_dev = torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda()
    tiles = []
    for a, oy in enumerate(ys):
        for b, ox in enumerate(xs):
            pred = torch.randn(*lead, tile, tile, generator=g) * 5.0
            blend_tile(pred.cuda(), out, wy_dev[a], wx_dev[b], oy, ox)
            tiles.append((oy, ox, wy[a], wx[b], pred.numpy()))
    torch.cuda.synchronize()
    return out.cpu().numpy(), tiles


@pytest.mark.parametrize("lead,tile,h,w,stride,cover", [
    ((6,), 64, 64, 128, 32, 2),       # three column tiles
    ((1, 3, 2), 64, 128, 128, 32, 4),  # K = 1, T = 3, C = 2: 3 x 3 tiles, four-fold coverage
    ((5,), 96, 96, 160, 32, 3),       # a 24-piece row (two rows per wave, idle lanes), three tiles over some pixels
    ((2,), 288, 288, 320, 32, 2),     # wider than 256 pixels: a lane takes two pieces of a row
])
def test_tile_blend_matches_the_formula_in_float64(lead, tile, h, w, stride, cover):
    """Bound 1e-6 * max|pred|: at most 4 covering tiles, at most 3 fp32 roundings of 2^-24 each per term, weights in [0, 1] that sum
    to 1 (within 4 * 2^-24 per axis)."""
    got, tiles = _blend_all(lead, tile, h, w, stride, seed=tile + w)
    want = np.zeros(got.shape, dtype=np.float64)
    count = np.zeros((h, w), dtype=np.int64)
    for oy, ox, wy, wx, pred in tiles:
        want[..., oy:oy + tile, ox:ox + tile] += (wy.astype(np.float64)[:, None] * wx.astype(np.float64)[None, :]) * pred.astype(np.float64)
        count[oy:oy + tile, ox:ox + tile] += 1
    assert count.min() >= 1 and count.max() == cover
    top = max(np.abs(t[4]).max() for t in tiles)
    err = np.abs(got.astype(np.float64) - want).max()
    print(f"tile_blend {lead} tile {tile} frame {h} x {w}: max error {err:.3e}, bound {1e-6 * top:.3e}")
    assert err <= 1e-6 * top


def test_tile_blend_without_overlap_copies_the_tiles_bit_for_bit():
    got, tiles = _blend_all((4,), 32, 96, 64, 32, seed=1)
    assert len(tiles) == 6
    want = np.zeros_like(got)
    for oy, ox, wy, wx, pred in tiles:
        assert (wy == 1).all() and (wx == 1).all()
        want[..., oy:oy + 32, ox:ox + 32] = pred
    assert np.array_equal(got, want)


def test_tile_blend_touches_nothing_outside_its_rectangle():
    from skillful_nowcasting_amd.tiling import blend_tile

    g = torch.Generator().manual_seed(2)
    out = torch.full((3, 96, 128), -777.0, device="cuda")
    pred = torch.randn(3, 32, 32, generator=g).cuda()
    wy, wx = torch.rand(32, generator=g).cuda(), torch.rand(32, generator=g).cuda()
    blend_tile(pred, out, wy, wx, 32, 64)
    torch.cuda.synchronize()
    inside = torch.zeros(96, 128, dtype=torch.bool, device="cuda")
    inside[32:64, 64:96] = True
    assert torch.equal(out[:, ~inside], torch.full_like(out[:, ~inside], -777.0))
    want = torch.addcmul(torch.full((3, 32, 32), -777.0, dtype=torch.float64), (wy[:, None] * wx[None, :]).double().cpu(), pred.double().cpu())
    assert (out[:, 32:64, 64:96].double().cpu() - want).abs().max().item() <= 1e-4  # (one fp32 rounding at magnitude 777)


def test_blend_tile_refuses_mixed_devices():
    from skillful_nowcasting_amd.tiling import blend_tile

    w = torch.ones(32)
    with pytest.raises(ValueError):
        blend_tile(torch.zeros(2, 32, 32), torch.zeros(2, 64, 64, device="cuda"), w.cuda(), w.cuda(), 0, 0)
    with pytest.raises(ValueError):
        blend_tile(torch.zeros(2, 32, 32, device="cuda"), torch.zeros(2, 64, 64, device="cuda"), w, w.cuda(), 0, 0)


# ---- the whole path --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    import skillful_nowcasting_amd as S

    torch.manual_seed(0)
    m = S.DGMR(**KW)
    with torch.no_grad():
        m.generator.latent_stack.att_block.gamma.fill_(0.4)
    return m.to("cuda").eval()


def _context(frames, ox=0, tile=128):
    """[T, H, W, C] fp32 frames -> the model's input for the tile at column ox: [1, 4, C, tile, tile]."""
    return frames[-4:, :tile, ox:ox + tile, :].permute(0, 3, 1, 2).unsqueeze(0).contiguous()


def test_single_tile_is_forward_draws(model):
    g = torch.Generator().manual_seed(3)
    frames = torch.rand(5, 128, 128, 1, generator=g).cuda()  # (five frames: the last four are the context)
    zs = torch.randn(3, 8, 4, 4, generator=g).cuda()
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        want = model.generator.forward_draws(_context(frames), 3, zs=zs)
    out = model.nowcast_full_frame(frames, 3, zs=zs)
    torch.cuda.synchronize()
    assert out.shape == (3, 3, 1, 128, 128) and out.dtype == torch.float32
    assert torch.equal(out, want.view(3, 3, 1, 128, 128))
    after = model.state_dict()
    assert set(after) == set(before)
    for k, v in before.items():
        assert torch.equal(after[k], v), k


def test_two_tiles_blend_between_their_own_forecasts(model):
    from skillful_nowcasting_amd.tiling import latent_field

    frames = torch.rand(4, 128, 224, 1, generator=torch.Generator().manual_seed(4)).cuda()
    out = model.nowcast_full_frame(frames, 2, stride=96, generator=torch.Generator().manual_seed(5))
    again = model.nowcast_full_frame(frames, 2, stride=96, generator=torch.Generator().manual_seed(5))
    other = model.nowcast_full_frame(frames, 2, stride=96, generator=torch.Generator().manual_seed(6))
    assert out.shape == (2, 3, 1, 128, 224)
    assert torch.equal(out, again) and not torch.equal(out, other)
    zs = latent_field(2, 8, 4, 7, torch.Generator().manual_seed(5)).cuda()
    with torch.no_grad():
        t0 = model.generator.forward_draws(_context(frames, 0), 2, zs=zs[..., 0:4].contiguous())
        t1 = model.generator.forward_draws(_context(frames, 96), 2, zs=zs[..., 3:7].contiguous())
    torch.cuda.synchronize()
    assert torch.equal(out[..., :96], t0[..., :96])        # weight exactly 1
    assert torch.equal(out[..., 128:], t1[..., 32:])
    a, b, mid = t0[..., 96:], t1[..., :32], out[..., 96:128]
    slack = 1e-6 * max(t0.abs().max().item(), t1.abs().max().item())
    assert (mid >= torch.minimum(a, b) - slack).all() and (mid <= torch.maximum(a, b) + slack).all()
    assert not torch.equal(a, b)  # (the two tiles do not agree in the overlap: the blend is doing something)


def test_storage_dtype_frames_equal_host_converted_frames(model):
    g = torch.Generator().manual_seed(7)
    raw = torch.randint(-64, 1024, (4, 128, 128, 1), generator=g, dtype=torch.int16)
    assert (raw < 0).any()
    phys = raw.float() * (1 / 32)
    phys = torch.where(phys >= 0, phys, torch.zeros_like(phys))
    zs = torch.randn(2, 8, 4, 4, generator=g).cuda()
    a = model.nowcast_full_frame(raw.cuda(), zs=zs, scale=1 / 32, clamp_missing=True)
    b = model.nowcast_full_frame(phys.cuda(), zs=zs)
    assert torch.equal(a, b)


def test_use_ema_nowcasts_from_the_averaged_generator(model):
    """use_ema=True is the nowcast made inside ema_scope(); the live weights are back afterwards."""
    g = torch.Generator().manual_seed(8)
    frames = torch.rand(4, 128, 128, 1, generator=g).cuda()
    zs = torch.randn(2, 8, 4, 4, generator=g).cuda()
    live = {n: p.detach().clone() for n, p in model.generator.named_parameters()}
    shadows = {n: (p * 0.75).cpu() for n, p in live.items()}
    shadows["num_updates"] = 1
    model.load_ema_state_dict(shadows)
    plain = model.nowcast_full_frame(frames, zs=zs)
    averaged = model.nowcast_full_frame(frames, zs=zs, use_ema=True)
    with model.ema_scope():
        inside = model.nowcast_full_frame(frames, zs=zs)
    assert torch.equal(averaged, inside) and not torch.equal(averaged, plain)
    assert torch.equal(model.nowcast_full_frame(frames, zs=zs), plain)
    for n, p in model.generator.named_parameters():
        assert torch.equal(p, live[n]), n


def test_refusals(model):
    frames = torch.rand(4, 128, 128, 1).cuda()
    model.train()
    try:
        with pytest.raises(RuntimeError, match="training mode"):
            model.nowcast_full_frame(frames, 2)
    finally:
        model.eval()
    with pytest.raises(ValueError, match="multiple of 32"):
        model.nowcast_full_frame(torch.rand(4, 120, 128, 1).cuda(), 2)
    with pytest.raises(ValueError):
        model.nowcast_full_frame(frames[:3], 2)
    with pytest.raises(ValueError):
        model.nowcast_full_frame(frames, 2, zs=torch.randn(3, 8, 4, 4).cuda())
    for bad in (torch.randn(2, 4, 4, 4).cuda(), torch.randn(2, 8, 4, 4).double().cuda(), torch.randn(2, 8, 4, 4)):  # channels, dtype, device
        with pytest.raises(ValueError):
            model.nowcast_full_frame(frames, zs=bad)
    with pytest.raises(ValueError, match="device"):
        model.nowcast_full_frame(frames.cpu(), 2)
