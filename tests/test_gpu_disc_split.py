"""Discriminator.forward_split - the generator pass's K discriminator calls run as their real half (no graph) and their generated
half - against Discriminator.forward on the joint batch cat(real, generated) that it replaces (dgmr/dgmr.py:186-193).

Nothing may differ, bit for bit: the scores of all rows, the gradient of the generated frames, every buffer the forward moves
(spectral-norm u / v, BatchNorm1d running statistics, num_batches_tracked) and the CPU RNG stream (the spatial discriminator's frame
draws).  That holds because every conv of either half is dispatched as the joint launch would be (dgmr_conv_args.plan_n,
tests/test_conv_plan_pin.py) and the BatchNorm1d heads run unchanged on the joint row order.  Both entries start from identical module
and RNG state, once while the spectral-norm requests are traced (first forward of a shape) and once served from the traced plan.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BUF = ("._u", "._v", "running_mean", "running_var", "num_batches_tracked")
GEOMETRIES = {"small": (128, 3), "paper": (256, 18)}  # frame size, forecast steps
# geometries where a structural requirement forces a half onto another kernel than the joint batch (the discriminator parity
# tolerance of test_gpu_draws.py would apply there): none - an odd B is not split at all (DGMR._gen_losses)
OTHER_KERNEL = ()


@pytest.fixture(scope="module")
def disc():
    import skillful_nowcasting_amd as S

    torch.manual_seed(3)
    d = S.Discriminator(input_channels=1)
    sd0 = {k: v.detach().clone() for k, v in d.state_dict().items()}
    d = d.to("cuda").train()
    for p in d.parameters():  # the generator pass freezes the discriminator (DGMR._training_step)
        p.requires_grad_(False)
    yield d, sd0
    S.ops.set_precision("f32")


def _joint(d, images, future, preds, k):
    """DGMR._gen_losses before the split: K calls on cat(real, draw) as one batch."""
    b = images.shape[0]
    pr = preds.view(k, b, *preds.shape[1:])
    real_sequence = torch.cat([images, future], dim=1)
    g_seq = torch.cat([images.unsqueeze(0).expand(k, *images.shape), pr], dim=2)
    x = torch.cat([real_sequence.unsqueeze(0).expand(k, *real_sequence.shape).unsqueeze(1), g_seq.unsqueeze(1)], dim=1)
    return d(x.reshape(2 * k * b, *real_sequence.shape[1:]), calls=k)


def _run(d, sd0, split, images, future, preds0, cot, k):
    import skillful_nowcasting_amd as S

    d.load_state_dict(sd0)
    S.ops.bump_weights_epoch()
    b = images.shape[0]
    preds = preds0.clone().requires_grad_(True)
    torch.manual_seed(17)
    out = d.forward_split(images, future, preds, calls=k) if split else _joint(d, images, future, preds, k)
    (out.view(k, 2, b, 2, 1)[:, 1] * cot).sum().backward()  # the generator's loss reads the generated rows only
    torch.cuda.synchronize()
    bufs = {n: v.detach().clone() for n, v in d.state_dict().items() if n.endswith(BUF)}
    return out.detach().clone(), preds.grad.clone(), bufs, torch.get_rng_state()


@pytest.mark.parametrize("precision", ["f32", "mixed"])
@pytest.mark.parametrize("k", [6, 1])
@pytest.mark.parametrize("geometry", ["small", "paper"])
def test_split_equals_joint(disc, geometry, k, precision):
    import skillful_nowcasting_amd as S
    from skillful_nowcasting_amd.nn import SNScope

    d, sd0 = disc
    size, steps = GEOMETRIES[geometry]
    b = 2
    S.ops.set_precision(precision)
    g = torch.Generator().manual_seed(5)
    images = torch.rand(b, 4, 1, size, size, generator=g).cuda()
    future = torch.rand(b, steps, 1, size, size, generator=g).cuda()
    preds0 = torch.rand(k * b, steps, 1, size, size, generator=g).cuda()
    cot = torch.randn(k, b, 2, 1, generator=g).cuda()
    for key in [key for key in SNScope._plans if key[0] == id(d)]:  # first pass of each entry: spectral-norm requests are traced
        del SNScope._plans[key]
    for mode in ("traced", "planned"):
        joint = _run(d, sd0, False, images, future, preds0, cot, k)
        if mode == "traced":
            for key in [key for key in SNScope._plans if key[0] == id(d)]:
                del SNScope._plans[key]
        split = _run(d, sd0, True, images, future, preds0, cot, k)
        what = f"{geometry} K={k} {precision} {mode}"
        assert geometry not in OTHER_KERNEL
        assert torch.equal(split[0], joint[0]), f"{what}: scores differ by {(split[0] - joint[0]).abs().max().item():.3e}"
        assert joint[1].abs().max().item() > 0
        assert torch.equal(split[1], joint[1]), f"{what}: gradient of the generated frames differs by {(split[1] - joint[1]).abs().max().item():.3e}"
        assert set(split[2]) == set(joint[2]) and len(joint[2]) > 40
        for n, v in joint[2].items():
            assert torch.equal(split[2][n], v), f"{what}: buffer {n} differs"
        assert torch.equal(split[3], joint[3]), f"{what}: CPU RNG state differs"
    assert any(key[0] == id(d) for key in SNScope._plans)  # (the second pass was served from a plan)


def test_frames_s2d_pair_is_the_gather_of_the_concatenation():
    """ops.frames_s2d_pair(context, following, ...) == ops.frames_s2d(cat(context[i % Bc], following[i % Bf]), ...), values and the
    gradient of the following frames, with and without drawn frame indices."""
    import skillful_nowcasting_amd as S

    ops = S.ops
    g = torch.Generator().manual_seed(1)
    bc, k, tc, tf, size = 2, 3, 4, 5, 32
    n = k * bc
    context = torch.rand(bc, tc, 1, size, size, generator=g).cuda()
    idx = torch.stack([torch.randint(0, tc + tf, (6,), generator=g) for _ in range(k)]).to(torch.int32).cuda()
    for bf in (n, bc):
        following = torch.rand(bf, tf, 1, size, size, generator=g).cuda()
        for kw in (dict(pool=True, frame_major=False, as_3d=True), dict(pool=True, frame_major=True, idx_group=bc), dict(pool=False, frame_major=True)):
            ix = idx if "idx_group" in kw else None
            f1 = following.clone().requires_grad_(bf == n)
            seq = torch.cat([context.repeat(n // bc, 1, 1, 1, 1), f1.repeat(n // bf, 1, 1, 1, 1)], dim=1)
            ref = ops.frames_s2d(seq, ix, **kw)
            f2 = following.clone().requires_grad_(bf == n)
            out = ops.frames_s2d_pair(context, f2, ix, n=n, **kw)
            assert out.shape == ref.shape and torch.equal(out, ref), kw
            if bf == n:
                cot = torch.randn(ref.shape, generator=g).cuda()
                (ref * cot).sum().backward()
                (out * cot).sum().backward()
                assert torch.equal(f2.grad, f1.grad), kw
