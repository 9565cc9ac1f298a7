"""What the FusedAdam tests on the GPU (test_gpu_grad_guard.py, test_gpu_ema.py) and tools/adam_digest.py share: the tensor set, its
seeded gradients, and one recipe that runs it in every mode and memory layout.

Tensor set: that of test_fused_adam_multi_tensor_equals_per_tensor_launches plus one that ends five elements past a chunk edge -
tensors shorter than a wave (3, 1) and longer than a workgroup's chunk (4096), one and five elements past a chunk edge (4097,
3 * 4096 + 5), whole chunks plus a tail (20000), a channels-last conv weight, a tensor without a gradient in two steps.
"""
import torch

SHAPES = [(3,), (4097,), (16, 8, 3, 3), (20000,), (1,), (129, 65), (3 * 4096 + 5,)]
NO_GRAD = (3, (1, 2))  # tensor 3 gets no gradient in steps 1 and 2
MODES = {"plain": dict(), "guarded": dict(max_grad_norm=30.0, skip_nonfinite=True), "ema": dict(ema_decay=0.9),
         "guarded+ema": dict(max_grad_norm=30.0, skip_nonfinite=True, ema_decay=0.9)}  # (30: clips the steps at gradient scale 10)
LAYOUTS = ("separate", "flat_grads", "flat_params")


def params(seed=12):
    torch.manual_seed(seed)
    ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in SHAPES]
    ps[2].data = ps[2].data.contiguous(memory_format=torch.channels_last)
    return ps


def grads(ps, steps, seed=100):
    """[step][tensor] -> gradient (None: no gradient), scaled 10 ** (step % 3 - 1)"""
    out = []
    for step in range(steps):
        torch.manual_seed(seed + step)
        row = []
        for i, p in enumerate(ps):
            g = torch.randn_like(p) * (10.0 ** (step % 3 - 1))
            row.append(None if i == NO_GRAD[0] and step in NO_GRAD[1] else g)
        out.append(row)
    return out


def set_grads(ps, row):
    for p, g in zip(ps, row):
        p.grad = None if g is None else g.clone(memory_format=torch.preserve_format)


def state(opt, ps):
    return [t.detach().clone() for p in ps for t in (p, opt.state[p]["exp_avg"], opt.state[p]["exp_avg_sq"])]


def odd_views(ps):
    """-> (flat, views): one zeroed buffer and, for every tensor of ps, a view with its shape and strides at an ODD element offset
    (4-byte aligned, never 16), the way ddp.FlatGrads lays gradients out."""
    offs, off = [], 1
    for p in ps:
        offs.append(off)
        off += p.numel()
        off += 1 - off % 2  # the next odd offset
    flat = torch.zeros(off, device="cuda")
    views = [flat[o:o + p.numel()].as_strided(p.shape, p.stride()) for o, p in zip(offs, ps)]
    assert all(v.data_ptr() % 16 != 0 and v.data_ptr() % 4 == 0 for v in views)
    return flat, views


def run(mode, layout, steps=5):
    """The recipe (lr 2e-3, betas (0.9, 0.99)) in MODES[mode] on one of LAYOUTS: separately allocated tensors; gradients as odd_views;
    parameters as (leaf) odd_views.  -> one snapshot after every step, one after swap_ema() and one after swapping back; a snapshot is
    [p, exp_avg, exp_avg_sq of every tensor] + [the shadows, EMA on] + [the guard's norm and coefficient, guard on]."""
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = params()
    rows = grads(ps, steps)
    g_views = odd_views(ps)[1] if layout == "flat_grads" else None
    if layout == "flat_params":
        views = odd_views(ps)[1]
        ps = [v.copy_(p.detach()).requires_grad_(True) for v, p in zip(views, ps)]
    kw = MODES[mode]
    opt = FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), **kw)

    def snapshot():
        out = state(opt, ps)
        if "ema_decay" in kw:
            out += [opt.ema(p).detach().clone() for p in ps]
        if "max_grad_norm" in kw:
            out += [opt.last_grad_norm.clone(), opt.last_clip_coef.clone()]
        return out

    shots = []
    for row in rows:
        if g_views is None:
            set_grads(ps, row)
        else:
            for p, v, g in zip(ps, g_views, row):
                p.grad = None if g is None else v.copy_(g)
        opt.step()
        shots.append(snapshot())
    for _ in range(2):
        opt.swap_ema()
        shots.append(snapshot())
    torch.cuda.synchronize()
    return shots
