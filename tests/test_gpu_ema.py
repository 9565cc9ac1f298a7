"""The weight EMA of optim.FusedAdam on the GPU: dgmr_adam_multi_ema (the Adam update of dgmr_adam_multi / dgmr_adam_multi_guarded plus
Tensor.lerp_ of a shadow towards the new parameter, one pass) and dgmr_swap_multi (the evaluation swap), from the kernels up to
DGMR.ema_scope().

Tensor set (adam_recipe.py): tensors shorter and longer than a workgroup's chunk (4096), one that ends five elements
past a chunk edge, a channels-last conv weight, a tensor without a gradient in two steps.  Five steps, gradients scaled
10 ** (step % 3 - 1).

The average is checked against the float64 recurrence e <- e + w (p_k - e), w = float32(1 - decay) as a double, fed with the fp32
parameter snapshots of each step (which test_training_is_not_perturbed pins against the path without EMA).  Bound after K updates:
|e - e64| <= K * 2^-22 * M, M the largest |p| or |e| of that tensor so far - at most four fp32 roundings per update, each at most
2^-24 * M (fma branch: p - e, the fma; other branch: p - e, 1 - w, the product, the difference; |p - e| <= 2 M is scaled by w < 0.5
resp. 1 - w <= 0.5), and carried errors are scaled by decay <= 1.
"""
import contextlib
import copy

import numpy as np
import pytest
import torch

import adam_recipe as R

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -22  # four fp32 roundings of 2^-24 each, per update and unit of magnitude


def _shadows(opt, ps):
    return [opt.ema(p).detach().clone() for p in ps]


def _run(steps=5, poison=None, **kw):
    """-> dict(p0: parameters before the first step, states: _state after every step, shadows: after every step (EMA on), opt, ps)"""
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = R.params()
    grads = R.grads(ps, steps)
    if poison is not None:
        step, tensor, index, value = poison
        grads[step][tensor].view(-1)[index] = value
    opt = FusedAdam(ps, lr=2e-3, **kw)
    rec = dict(p0=[p.detach().clone() for p in ps], states=[], shadows=[], grads=grads, opt=opt, ps=ps)
    for row in grads:
        R.set_grads(ps, row)
        opt.step()
        rec["states"].append(R.state(opt, ps))
        if opt.ema_decay is not None:
            rec["shadows"].append(_shadows(opt, ps))
    torch.cuda.synchronize()
    return rec


def _w(decay):
    """1 - decay formed in double and rounded to float once, as a double"""
    return float(np.float32(1.0 - decay))


def _check_recurrence(p0, snapshots, shadows, weights, stepped, what=""):
    """p0[i]: parameter i before its first update; snapshots[k][i]: after step k; shadows[k][i]: the shadow after step k;
    weights[k]: the double w of step k; stepped(k, i): did tensor i have a gradient in step k."""
    worst = 0.0
    for i in range(len(p0)):
        if shadows[-1][i] is None:  # (a parameter that never had a gradient: no shadow)
            assert all(s[i] is None for s in shadows), i
            continue
        e64 = p0[i].double()
        big = p0[i].abs().max().item()
        for k, w in enumerate(weights):
            if stepped(k, i):
                e64 = e64 + w * (snapshots[k][i].double() - e64)
            got = shadows[k][i]
            big = max(big, snapshots[k][i].abs().max().item(), got.abs().max().item())
            err = (got.double() - e64).abs().max().item()
            bound = (k + 1) * UNIT * big
            assert err <= bound, (what, "tensor", i, "step", k, err, bound)
            if bound > 0:
                worst = max(worst, err / bound)
    print(f"{what}: worst error / bound = {worst:.3f}")


def _stepped(k, i):
    return not (i == R.NO_GRAD[0] and k in R.NO_GRAD[1])


# ------------------------------------------------------------------------------------------------
# 1. training is not perturbed
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", [dict(), dict(max_grad_norm=30.0), dict(max_grad_norm=30.0, skip_nonfinite=True)],
                         ids=["plain", "clip", "clip+skip"])
@pytest.mark.parametrize("betas", [(0.0, 0.999), (0.9, 0.99)])
def test_training_is_not_perturbed(betas, guard):
    """p, exp_avg and exp_avg_sq after every step are the bits of the run without EMA (dgmr_adam_multi resp. dgmr_adam_multi_guarded;
    with the clip at 30 the coefficient is below 1 in the steps at gradient scale 10 and 1 in the others)."""
    off = _run(betas=betas, **guard)
    on = _run(betas=betas, ema_decay=0.999, **guard)
    for k, (a, b) in enumerate(zip(off["states"], on["states"])):
        bad = [(i // 3, ("p", "exp_avg", "exp_avg_sq")[i % 3]) for i, (u, v) in enumerate(zip(a, b)) if not torch.equal(u, v)]
        assert not bad, (betas, guard, "step", k, bad)
    if guard:
        assert torch.equal(off["opt"].last_grad_norm, on["opt"].last_grad_norm)
        assert torch.equal(off["opt"].last_clip_coef, on["opt"].last_clip_coef)
    assert on["opt"].ema_num_updates == 5 and off["opt"].ema_num_updates == 0
    assert all(off["opt"].ema(p) is None for p in off["ps"])
    assert set(on["opt"].state[on["ps"][0]]) == {"step", "exp_avg", "exp_avg_sq"}  # the shadows live outside self.state


# ------------------------------------------------------------------------------------------------
# 2. the average is right
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decay", [0.999, 0.3, 0.0])
def test_average_against_float64(decay):
    """0.999: at::lerp's w < 0.5 branch; 0.3: the other one; 0.0: w = 1, the shadow IS the parameter."""
    run = _run(betas=(0.9, 0.99), ema_decay=decay)
    snaps = [st[0::3] for st in run["states"]]
    for i, p in enumerate(run["ps"]):
        e = run["opt"].ema(p)
        assert e.shape == p.shape and e.stride() == p.stride() and e.data_ptr() != p.data_ptr(), i
    _check_recurrence(run["p0"], snaps, run["shadows"], [_w(decay)] * 5, _stepped, f"decay {decay}")
    if decay == 0.0:
        for k in range(5):
            for i in range(len(R.SHAPES)):
                if _stepped(k, i):
                    assert torch.equal(run["shadows"][k][i], snaps[k][i]), (k, i)
    else:  # the average is neither the parameter nor its starting point
        assert all(not torch.equal(e, p) and not torch.equal(e, p0) for e, p, p0 in zip(run["shadows"][-1], snaps[-1], run["p0"]))


def test_average_under_the_guard():
    """The shadow follows the parameter the GUARDED launch stores (g * clip_coef)."""
    run = _run(betas=(0.0, 0.999), ema_decay=0.3, max_grad_norm=30.0)
    snaps = [st[0::3] for st in run["states"]]
    _check_recurrence(run["p0"], snaps, run["shadows"], [_w(0.3)] * 5, _stepped, "decay 0.3, clip 30")


# ------------------------------------------------------------------------------------------------
# 3. warm-up
# ------------------------------------------------------------------------------------------------
def test_warmup_uses_the_ramp():
    run = _run(steps=2, betas=(0.9, 0.99), ema_decay=0.999, ema_warmup=True)
    snaps = [st[0::3] for st in run["states"]]
    weights = [_w(0.1), _w(2.0 / 11.0)]  # min(0.999, (1 + n) / (10 + n)) for n = 0, 1
    _check_recurrence(run["p0"], snaps, run["shadows"], weights, _stepped, "warm-up")
    assert run["opt"].ema_num_updates == 2
    # without the ramp the first shadow would sit 0.999 of the way back towards p0: far outside the bound
    e, p0, p1 = run["shadows"][0][1].double(), run["p0"][1].double(), snaps[0][1].double()
    assert ((e - p0).abs().max() > 0.5 * (p1 - p0).abs().max()).item()


# ------------------------------------------------------------------------------------------------
# 4. a skipped step
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_skipped_step_leaves_the_average(bad):
    run = _run(betas=(0.9, 0.99), ema_decay=0.9, skip_nonfinite=True, poison=(2, 1, 4096, bad))
    sh = run["shadows"]
    assert all(torch.equal(u, v) for u, v in zip(sh[1], sh[2])), "a skipped step stored something to a shadow"
    assert all(torch.equal(u, v) for u, v in zip(run["states"][1], run["states"][2]))
    assert run["opt"].skipped_steps.item() == 1
    assert run["opt"].ema_num_updates == 5  # attempted steps, like state["step"]
    for k in (3, 4):  # the next finite steps move every shadow again
        assert all(not torch.equal(u, v) for u, v in zip(sh[k - 1], sh[k])), k
    assert all(torch.isfinite(e).all().item() for e in sh[-1])


# ------------------------------------------------------------------------------------------------
# 5. a parameter without a gradient
# ------------------------------------------------------------------------------------------------
def test_shadow_of_a_parameter_without_gradient_does_not_move():
    run = _run(betas=(0.9, 0.99), ema_decay=0.9)
    i = R.NO_GRAD[0]
    sh = [s[i] for s in run["shadows"]]
    assert torch.equal(sh[0], sh[1]) and torch.equal(sh[1], sh[2])  # steps 1 and 2: not in the table
    assert not torch.equal(sh[2], sh[3]) and not torch.equal(sh[3], sh[4])
    assert not torch.equal(sh[0], run["p0"][i])  # step 0 did move it


# ------------------------------------------------------------------------------------------------
# 6. the swap
# ------------------------------------------------------------------------------------------------
def test_swap_exchanges_and_restores():
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = R.params()
    torch.manual_seed(5)
    lone = [torch.randn(5000, device="cuda").requires_grad_(True), torch.randn(7, device="cuda").requires_grad_(True)]
    every = [lone[0]] + ps + [lone[1]]  # parameters that never get a gradient: no shadow, at both ends of the list
    opt = FusedAdam(every, lr=2e-3, betas=(0.9, 0.99), ema_decay=0.5)
    for row in R.grads(ps, 3):
        R.set_grads(ps, row)
        opt.step()
    assert all(opt.ema(p) is None for p in lone)
    p_old = [p.detach().clone() for p in every]
    e_old = _shadows(opt, ps)
    tags = [ops._core.weight_tag(p) for p in every]
    swapped = opt.swap_ema()
    assert [id(p) for p in swapped] == [id(p) for p in ps]
    for i, p in enumerate(ps):
        assert torch.equal(p, e_old[i]), i
        assert torch.equal(opt.ema(p), p_old[1 + i]), i
        assert p.stride() == p_old[1 + i].stride()
    assert torch.equal(lone[0], p_old[0]) and torch.equal(lone[1], p_old[-1])
    now = [ops._core.weight_tag(p) for p in every]
    assert all(a != b for a, b in zip(tags[1:-1], now[1:-1]))  # the swapped weights' cached images are stale ...
    assert tags[0][:2] == now[0][:2] and tags[0][3:] == now[0][3:]  # ... through the per-parameter count, not the global epoch
    opt.swap_ema()
    for i, p in enumerate(every):
        assert torch.equal(p, p_old[i]), i
    for i, p in enumerate(ps):
        assert torch.equal(opt.ema(p), e_old[i]), i


def test_null_shadow_entries_are_skipped():
    """The C entry points with a table that has a NULL shadow in the middle: dgmr_adam_multi_ema updates that tensor like
    dgmr_adam_multi and averages the others; dgmr_swap_multi leaves it alone."""
    from skillful_nowcasting_amd import _lib, ops

    chunk = int(_lib.load().dgmr_adam_chunk())
    shapes = [(4096 + 3,), (2 * 4096,), (100,)]

    def make():
        torch.manual_seed(31)
        return [[torch.randn(s, device="cuda") for s in shapes] for _ in range(4)] + [[torch.rand(s, device="cuda") for s in shapes]]

    def table(p, g, m, v):
        tab = np.zeros(len(p), dtype=_lib.ADAM_DESC_DTYPE)
        block = 0
        for i in range(len(p)):
            tab[i] = (p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), p[i].numel(), block, np.float32(2e-3 / 0.1),
                      np.float32(0.1), 0)
            block += (p[i].numel() + chunk - 1) // chunk
        return torch.from_numpy(tab.view(np.uint8)).cuda(), block

    pa, ga, ma, e_unused, va = make()
    pb, gb, mb, eb, vb = make()
    e_old = [t.clone() for t in eb]
    ta, blocks = table(pa, ga, ma, va)
    tb, _ = table(pb, gb, mb, vb)
    ptrs = torch.tensor([eb[0].data_ptr(), 0, eb[2].data_ptr()], dtype=torch.int64, device="cuda")
    ops.call("dgmr_adam_multi", ta.data_ptr(), 3, blocks, 0.9, 0.99, 1e-8, ops._stream())
    ops.call("dgmr_adam_multi_ema", tb.data_ptr(), ptrs.data_ptr(), 3, blocks, 0.9, 0.99, 1e-8, 0.25, None, ops._stream())
    torch.cuda.synchronize()
    for i in range(3):
        assert torch.equal(pa[i], pb[i]) and torch.equal(ma[i], mb[i]) and torch.equal(va[i], vb[i]), i
    assert torch.equal(eb[1], e_old[1])
    for i in (0, 2):
        want = e_old[i].double() + _w(0.75) * (pb[i].double() - e_old[i].double())
        assert (eb[i].double() - want).abs().max().item() <= UNIT * max(pb[i].abs().max().item(), e_old[i].abs().max().item()), i
    p_old, e_now = [t.clone() for t in pb], [t.clone() for t in eb]
    ops.call("dgmr_swap_multi", tb.data_ptr(), ptrs.data_ptr(), 3, blocks, ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(pb[1], p_old[1]) and torch.equal(eb[1], e_now[1])
    for i in (0, 2):
        assert torch.equal(pb[i], e_now[i]) and torch.equal(eb[i], p_old[i]), i


def test_adam_multi_on_a_slice_of_a_table():
    """dgmr_adam_multi on descs + 1 of a three-row table (block0 of the slice's first row is not 0) against dgmr_adam_multi on a table
    built for those two rows alone; the row in front of the slice is left alone."""
    from skillful_nowcasting_amd import _lib, ops

    chunk = int(_lib.load().dgmr_adam_chunk())
    shapes = [(4096 + 3,), (2 * 4096,), (100,)]

    def make():
        torch.manual_seed(31)
        return [[torch.randn(s, device="cuda") for s in shapes] for _ in range(3)] + [[torch.rand(s, device="cuda") for s in shapes]]

    def table(rows, p, g, m, v):
        tab = np.zeros(len(rows), dtype=_lib.ADAM_DESC_DTYPE)
        block = 0
        for k, i in enumerate(rows):
            tab[k] = (p[i].data_ptr(), g[i].data_ptr(), m[i].data_ptr(), v[i].data_ptr(), p[i].numel(), block, np.float32(2e-3 / 0.1),
                      np.float32(0.1), 0)
            block += (p[i].numel() + chunk - 1) // chunk
        return torch.from_numpy(tab.view(np.uint8)).cuda(), block

    a, b = make(), make()
    first = [t[0].clone() for t in a]
    ta, blocks3 = table([0, 1, 2], *a)
    tb, blocks2 = table([1, 2], *b)
    assert blocks3 == 5 and blocks2 == 3  # the slice's first row starts at block 2
    ops.call("dgmr_adam_multi", ta.data_ptr() + _lib.ADAM_DESC_DTYPE.itemsize, 2, blocks2, 0.9, 0.99, 1e-8, ops._stream())
    ops.call("dgmr_adam_multi", tb.data_ptr(), 2, blocks2, 0.9, 0.99, 1e-8, ops._stream())
    torch.cuda.synchronize()
    for j, (u, v) in enumerate(zip(a, b)):  # p, g, m, v
        assert torch.equal(u[0], first[j]), j
        assert torch.equal(u[1], v[1]) and torch.equal(u[2], v[2]), j
    assert not torch.equal(a[0][1], make()[0][1])  # the slice was updated


@pytest.mark.parametrize("ema", [None, 0.9], ids=["plain", "ema"])
def test_two_groups_with_their_own_hyperparameters(ema):
    """Two parameter groups that differ in lr, betas and eps (one table, one launch per slice, each with its group's scalars) against
    one dgmr_adam launch per tensor: parameters and moments bit for bit after every step, with and without EMA; the shadows against
    the float64 recurrence."""
    from skillful_nowcasting_amd.optim import FusedAdam

    def make(**kw):
        ps = R.params()
        groups = [dict(params=ps[:3]), dict(params=ps[3:], lr=5e-3, betas=(0.5, 0.9), eps=1e-6)]
        return ps, FusedAdam(groups, lr=2e-3, betas=(0.9, 0.99), **kw)

    (pa, oa), (pb, ob) = make(ema_decay=ema), make()
    ob.multi_tensor = False
    p0 = [p.detach().clone() for p in pa]
    snaps, shadows = [], []
    for k, row in enumerate(R.grads(pa, 5)):
        R.set_grads(pa, row)
        R.set_grads(pb, row)
        oa.step()
        ob.step()
        sa, sb = R.state(oa, pa), R.state(ob, pb)
        bad = [i for i, (u, v) in enumerate(zip(sa, sb)) if not torch.equal(u, v)]
        assert not bad, (k, bad)
        snaps.append(sa[0::3])
        if ema is not None:
            shadows.append(_shadows(oa, pa))
    assert [oa.state[p]["step"] for p in pa] == [ob.state[p]["step"] for p in pb] == [5, 5, 5, 3, 5, 5, 5]
    if ema is not None:
        _check_recurrence(p0, snaps, shadows, [_w(ema)] * 5, _stepped, "two groups")


# ------------------------------------------------------------------------------------------------
# 7. flat gradient buffers
# ------------------------------------------------------------------------------------------------
def _run_layout(layout, steps=5):
    """separate: every gradient its own tensor (16-byte aligned).  flat: as_strided views at ODD element offsets into one buffer
    (4-byte aligned only), the way ddp.FlatGrads makes them; the buffer is opt.flat_grads, as under attach_data_parallel()."""
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = R.params()
    grads = R.grads(ps, steps)
    opt = FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), max_grad_norm=30.0, skip_nonfinite=True, ema_decay=0.9)
    views = None
    if layout == "flat":
        opt.flat_grads, views = R.odd_views(ps)
    for row in grads:
        opt.zero_grad()
        if views is None:
            R.set_grads(ps, row)
        else:
            for p, v, g in zip(ps, views, row):
                p.grad = None if g is None else v.copy_(g)
        opt.step()
    torch.cuda.synchronize()
    return R.state(opt, ps), _shadows(opt, ps)


def test_flat_gradient_buffers_give_the_same_bits():
    """The sixteen-byte path with a dword-aligned gradient (guard on, as under attach_data_parallel() with a clip norm): parameters,
    moments and shadows agree bit for bit with the run on separate, 16-byte aligned gradient tensors."""
    (sa, ea), (sb, eb) = _run_layout("separate"), _run_layout("flat")
    for i in range(len(R.SHAPES)):
        for j in range(3):
            assert torch.equal(sa[3 * i + j], sb[3 * i + j]), (i, j)
        assert torch.equal(ea[i], eb[i]), i
    (sc, ec) = _run_layout("flat")
    assert all(torch.equal(u, v) for u, v in zip(sb + eb, sc + ec))


@pytest.mark.parametrize("mode", list(R.MODES))
def test_misaligned_parameters_give_the_same_bits(mode):
    """Parameters that are leaf views at odd element offsets into one flat buffer (4-byte aligned only; moments and shadows are
    allocated on their own): the dword walk of every chunk, against the recipe on separately allocated parameters - bit for bit on
    every parameter, moment and shadow (and the guard's norm and coefficient) after each of five steps, after swap_ema() and after
    swapping back."""
    want, got = R.run(mode, "separate"), R.run(mode, "flat_params")
    assert len(want) == len(got) == 7
    for k, (a, b) in enumerate(zip(want, got)):
        assert len(a) == len(b) >= 3 * len(R.SHAPES)
        bad = [i for i, (u, v) in enumerate(zip(a, b)) if not torch.equal(u, v)]
        assert not bad, (mode, "snapshot", k, bad)
    n = len(R.SHAPES)
    if "ema" in mode:  # the swap did exchange parameters and shadows, and the second one put them back
        assert all(torch.equal(got[5][3 * i], got[4][3 * n + i]) and torch.equal(got[5][3 * n + i], got[4][3 * i]) for i in range(n))
        assert all(not torch.equal(got[5][3 * i], got[4][3 * i]) for i in range(n))
    assert all(torch.equal(u, v) for u, v in zip(got[6], got[4]))


# ------------------------------------------------------------------------------------------------
# 8. table reuse
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("guard", [dict(), dict(max_grad_norm=50.0, skip_nonfinite=True)], ids=["plain", "guarded"])
def test_ema_tables_survive_a_gpu_backlog(guard):
    """test_guarded_descriptor_tables_survive_a_gpu_backlog with EMA on: the shadows' pointer table shares the descriptors' pinned
    ring slot.  Two parameter groups, ~0.3 s of device work queued ahead and twelve steps without synchronisation, against the same
    settings synchronised after every step."""
    from skillful_nowcasting_amd.optim import FusedAdam

    shapes = [(5,), (4097,), (16, 8, 3, 3), (20000,), (1,), (129, 65)]

    def make():
        torch.manual_seed(21)
        ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
        return [dict(params=ps[:3], lr=1e-3), dict(params=ps[3:], lr=5e-3, betas=(0.5, 0.99))], ps

    (ga, pa), (gb, pb) = make(), make()
    oa = FusedAdam(ga, lr=1e-3, betas=(0.0, 0.999), ema_decay=0.9, **guard)
    ob = FusedAdam(gb, lr=1e-3, betas=(0.0, 0.999), ema_decay=0.9, **guard)
    torch.manual_seed(22)
    grads = [[torch.randn(s, device="cuda") * (10.0 ** (k % 3 - 1)) for s in shapes] for k in range(12)]
    big = torch.randn(8192, 8192, device="cuda")
    torch.cuda.synchronize()
    for _ in range(40):  # a backlog: the host runs far ahead of the device from here on
        big = torch.mm(big, big).clamp_(-1, 1)
    for k in range(12):
        for p, g in zip(pa, grads[k]):
            p.grad = g
        oa.step()
    torch.cuda.synchronize()
    for k in range(12):
        for p, g in zip(pb, grads[k]):
            p.grad = g
        ob.step()
        torch.cuda.synchronize()
    for i, (u, v) in enumerate(zip(R.state(oa, pa) + _shadows(oa, pa), R.state(ob, pb) + _shadows(ob, pb))):
        assert torch.equal(u, v), i
    assert all(not torch.equal(oa.ema(p), p) for p in pa)


def test_ema_state_dict_round_trip_on_the_device():
    """ema_state_dict() -> load_ema_state_dict() on an optimiser whose parameters are still on the host -> parameters moved: the
    shadows arrive at first use with the parameters' device and strides, and the next step continues bit for bit."""
    from skillful_nowcasting_amd.optim import FusedAdam

    run = _run(steps=3, betas=(0.9, 0.99), ema_decay=0.9)
    saved = run["opt"].ema_state_dict()
    adam = copy.deepcopy(run["opt"].state_dict())  # (state_dict() hands out the live moment tensors)
    assert saved["num_updates"] == 3 and sorted(saved["shadows"]) == list(range(len(R.SHAPES)))
    host = [torch.nn.Parameter(p.detach().cpu()) for p in run["ps"]]
    opt = FusedAdam(host, lr=2e-3, betas=(0.9, 0.99), ema_decay=0.9)
    opt.load_ema_state_dict({"num_updates": saved["num_updates"], "shadows": {i: t.cpu().contiguous() for i, t in saved["shadows"].items()}})
    assert not opt.ema(host[2]).is_cuda
    for p, q in zip(host, run["ps"]):
        p.data = torch.empty_like(q).copy_(p.data)  # to the device, channels-last where the original is
    opt.load_state_dict(adam)
    for p, q in zip(host, run["ps"]):
        e = opt.ema(p)
        assert e.is_cuda and e.stride() == q.stride() and torch.equal(e, run["opt"].ema(q))
    torch.manual_seed(77)
    row = [torch.randn_like(q) for q in run["ps"]]
    R.set_grads(run["ps"], row)
    R.set_grads(host, row)
    run["opt"].step()
    opt.step()
    assert opt.ema_num_updates == 4 == run["opt"].ema_num_updates
    for p, q in zip(host, run["ps"]):
        assert torch.equal(p, q) and torch.equal(opt.ema(p), run["opt"].ema(q))


# ------------------------------------------------------------------------------------------------
# 9. the whole model
# ------------------------------------------------------------------------------------------------
KW = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2, beta1=0.5)
DECAY = 0.5


@contextlib.contextmanager
def _mixed():
    import skillful_nowcasting_amd as S

    S.set_precision("mixed")
    try:
        yield
    finally:
        S.set_precision("f32")


def _train(ema):
    """Two seeded training steps (the guard tests' recipe) -> the model and what the tests below compare."""
    import skillful_nowcasting_amd as S

    with _mixed():
        torch.manual_seed(7)
        model = S.DGMR(**KW).to("cuda")
        if ema:
            model.gen_ema_decay = DECAY
        torch.manual_seed(8)
        x = torch.rand(2, 4, 1, 128, 128, device="cuda")
        y = torch.rand(2, 2, 1, 128, 128, device="cuda")
        torch.manual_seed(9)
        rec = dict(model=model, x=x, y=y, logged=[], gen=[[p.detach().clone() for p in model.generator.parameters()]])
        for i in range(2):
            model.training_step((x, y), i)
            torch.cuda.synchronize()
            rec["logged"].append({k: v.detach().clone() for k, v in model.logged_metrics.items()})
            rec["gen"].append([p.detach().clone() for p in model.generator.parameters()])
            if ema:
                g_opt = model.optimizers()[0]
                rec.setdefault("shadows", []).append([None if g_opt.ema(p) is None else g_opt.ema(p).detach().clone()
                                                      for p in model.generator.parameters()])
        rec["params"] = [p.detach().clone() for p in model.parameters()]
        rec["buffers"] = [b.detach().clone() for b in model.buffers()]
        return rec


@pytest.fixture(scope="module")
def whole():
    return _train(False), _train(True)


def _forward(model, x, seed=33):
    torch.manual_seed(seed)  # the latents
    with torch.no_grad():
        return model(x).clone()


def test_whole_step_is_not_perturbed(whole):
    off, on = whole
    assert len(off["params"]) == len(on["params"]) and len(off["buffers"]) == len(on["buffers"])
    bad = [i for i, (u, v) in enumerate(zip(off["params"], on["params"])) if not torch.equal(u, v)]
    assert not bad, f"{len(bad)} of {len(off['params'])} parameters differ with EMA on, e.g. {bad[:5]}"
    bad = [i for i, (u, v) in enumerate(zip(off["buffers"], on["buffers"])) if not torch.equal(u, v, )]
    assert not bad, f"{len(bad)} buffers differ with EMA on, e.g. {bad[:5]}"
    for a, b in zip(off["logged"], on["logged"]):
        assert set(a) == set(b) == {"train/d_loss", "train/g_loss", "train/grid_loss"}
        assert all(torch.equal(a[k], b[k]) for k in a)
    g_off, d_off = off["model"].optimizers()
    g_on, d_on = on["model"].optimizers()
    assert g_off.ema_decay is None and g_off.ema_num_updates == 0
    assert g_on.ema_decay == DECAY and g_on.ema_num_updates == 2
    assert d_on.ema_decay is None and all(d_on.ema(p) is None for p in on["model"].discriminator.parameters())  # never averaged


def test_whole_step_average_against_float64(whole):
    _, on = whole
    with_grad = [p.grad is not None for p in on["model"].generator.parameters()]
    assert [s is not None for s in on["shadows"][-1]] == with_grad and sum(with_grad) > 100  # a shadow for every stepped parameter
    _check_recurrence(on["gen"][0], on["gen"][1:], on["shadows"], [_w(DECAY)] * 2, lambda k, i: True, "generator, decay 0.5")


def test_ema_scope_swaps_weights_and_invalidates_the_caches(whole):
    """The stale-cache test: every weight image is warm from the forward outside the scope; inside, the forward must run the averaged
    weights - the output of a second model that was GIVEN them through load_state_dict - and afterwards the live ones again."""
    import skillful_nowcasting_amd as S

    _, on = whole
    model, x = on["model"], on["x"]
    with _mixed():
        model.eval()
        try:
            out_live = _forward(model, x)
            ema = model.ema_state_dict()
            with model.ema_scope():
                out_ema = _forward(model, x)
            out_live2 = _forward(model, x)
            sd = model.state_dict()
            replaced = 0
            for name, t in ema.items():
                if name == "num_updates":
                    continue
                assert "generator." + name in sd, name
                for key in ("generator." + name, name):  # (DGMR lists its generator parts under both)
                    if key in sd:
                        assert sd[key].shape == t.shape, key
                        sd[key] = t
                        replaced += 1
            assert replaced >= len(ema) - 1 > 0
            torch.manual_seed(1234)
            other = S.DGMR(**KW).to("cuda")
            other.load_state_dict(sd)
            other.eval()
            out_other = _forward(other, x)
        finally:
            model.train()
    assert not torch.equal(out_ema, out_live)
    assert torch.equal(out_ema, out_other)
    assert torch.equal(out_live2, out_live)


def test_state_dict_inside_the_scope_is_the_average(whole):
    _, on = whole
    model = on["model"]
    ema = model.ema_state_dict()
    assert ema["num_updates"] == 2
    live = {k: v.clone() for k, v in model.state_dict().items()}
    names = [n for n, p in model.generator.named_parameters() if p.grad is not None]  # (the stepped ones)
    assert set(ema) == set(names) | {"num_updates"}
    assert all(ema[n].is_contiguous() for n in names)
    with model.ema_scope():
        inside = {k: v.clone() for k, v in model.state_dict().items()}
    after = model.state_dict()
    assert set(inside) == set(live) == set(after)
    for n in names:
        assert torch.equal(inside["generator." + n], ema[n]), n
    assert sum(not torch.equal(inside["generator." + n], live["generator." + n]) for n in names) > len(names) // 2
    gen_keys = {"generator." + n for n in names} | set(names)
    for k in live:
        assert torch.equal(after[k], live[k]), k
        if k not in gen_keys:  # buffers and the discriminator: untouched by the scope
            assert torch.equal(inside[k], live[k]), k
    assert torch.equal(model.ema_state_dict()[names[0]], ema[names[0]])  # the shadows are back as well


def test_scope_refuses_training_and_nesting(whole):
    _, on = whole
    model, x, y = on["model"], on["x"], on["y"]
    live = [p.detach().clone() for p in model.parameters()]
    shadows = model.ema_state_dict()
    with pytest.raises(RuntimeError, match="ema_scope"):
        with model.ema_scope():
            model.training_step((x, y), 2)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), live)), "the scope did not put the live weights back"
    with pytest.raises(RuntimeError, match="ema_scope"):
        with model.ema_scope():
            with model.ema_scope():
                pass
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), live))
    with pytest.raises(RuntimeError, match="ema_scope"):
        with model.ema_scope():
            model.sample(x, 1, use_ema=True)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), live))
    now = model.ema_state_dict()
    assert all(torch.equal(now[k], shadows[k]) for k in shadows if k != "num_updates")
    assert model.optimizers()[0].ema_num_updates == 2  # nothing was stepped


def test_ema_state_dict_into_a_fresh_model(whole):
    """state_dict, then ema_state_dict into a model that is still on the host (the shadows wait there), then .to(device):
    sample(use_ema=True) draws the same bits from both."""
    import skillful_nowcasting_amd as S

    _, on = whole
    model, x = on["model"], on["x"]
    with _mixed():
        torch.manual_seed(4321)
        fresh = S.DGMR(**KW)
        fresh.load_state_dict({k: v.cpu() for k, v in model.state_dict().items()})
        fresh.load_ema_state_dict({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in model.ema_state_dict().items()})
        fresh = fresh.to("cuda")
        model.eval()
        fresh.eval()
        try:
            torch.manual_seed(55)
            a = model.sample(x, 2, use_ema=True).clone()
            torch.manual_seed(55)
            b = fresh.sample(x, 2, use_ema=True).clone()
            torch.manual_seed(55)
            c = model.sample(x, 2).clone()
        finally:
            model.train()
    assert a.shape == (2, 2, 2, 1, 128, 128)
    assert torch.equal(a, b)
    assert not torch.equal(a, c)
    assert fresh.optimizers()[0].ema_num_updates == 2
