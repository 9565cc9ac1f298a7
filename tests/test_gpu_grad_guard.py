"""The gradient guard of optim.FusedAdam on the GPU: dgmr_grad_norm_multi (global L2 norm in double, clip coefficient, skip flag;
deterministic, independent of the gradients' layout) and dgmr_adam_multi_guarded (Adam on g * clip_coef, nothing stored on a skipped
step), from the kernels up to DGMR.training_step.

Tensor set: adam_recipe.py.
"""
import pytest
import torch

import adam_recipe as R

pytestmark = pytest.mark.gpu

ULP2 = 2.0 ** -22  # two fp32 ulps: the squares are exact in double, the double sums add ~ n * 2^-53, one rounding to float


def _norm64(row):
    return torch.linalg.vector_norm(torch.cat([g.double().flatten() for g in row if g is not None])).item()


def test_norm_against_float64():
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = R.params()
    grads = R.grads(ps, 5)
    opt = FusedAdam(ps, lr=2e-3, betas=(0.0, 0.999), max_grad_norm=1.0)
    for step, row in enumerate(grads):
        R.set_grads(ps, row)
        opt.step()
        with_grad = [i for i, g in enumerate(row) if g is not None]
        assert [id(p) for p in opt.last_guarded_params] == [id(ps[i]) for i in with_grad], step  # grad None is left out, as torch does
        ref = _norm64(row)
        got = opt.last_grad_norm.item()
        print(f"step {step}: norm {got!r} float64 {ref!r} rel {abs(got - ref) / ref:.2e}")
        assert abs(got - ref) <= ULP2 * ref, (step, got, ref)
        per = opt.last_tensor_grad_norms
        assert per.dtype == torch.float64 and per.shape == (len(with_grad),)
        for k, i in enumerate(with_grad):
            r = torch.linalg.vector_norm(row[i].double().flatten()).item()
            assert abs(per[k].item() - r) <= ULP2 * r, (step, i, per[k].item(), r)
        coef = opt.last_clip_coef.item()
        want = min(1.0, 1.0 / (ref + 1e-6))
        assert abs(coef - want) <= 4 * ULP2 * want, (step, coef, want)
    assert opt.skipped_steps.item() == 0 and opt.nonfinite_parameters() == []


def _run_layout(layout, grads_of, steps=5):
    """separate: every gradient its own tensor.  flat: as_strided views at ODD element offsets into one buffer (4-byte aligned only),
    the way ddp.FlatGrads makes them."""
    from skillful_nowcasting_amd.optim import FusedAdam

    ps = R.params()
    grads = grads_of(ps)
    opt = FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), max_grad_norm=30.0, skip_nonfinite=True)
    views = None
    if layout == "flat":
        views = R.odd_views(ps)[1]
    seen = []
    for row in grads[:steps]:
        if views is None:
            R.set_grads(ps, row)
        else:
            for p, v, g in zip(ps, views, row):
                p.grad = None if g is None else v.copy_(g)
        opt.step()
        seen += [opt.last_grad_norm.clone(), opt.last_clip_coef.clone()]
    torch.cuda.synchronize()
    return seen + R.state(opt, ps)


def test_layout_independence_and_determinism():
    """Separate gradient tensors (16-byte aligned: the vector-load path) and odd-offset views into a flat buffer (dword loads) sum the
    same elements in the same order: norm, coefficient, parameters and moments agree bit for bit, and so do two runs of one layout."""
    a = _run_layout("separate", lambda ps: R.grads(ps, 5))
    b = _run_layout("flat", lambda ps: R.grads(ps, 5))
    a2 = _run_layout("separate", lambda ps: R.grads(ps, 5))
    b2 = _run_layout("flat", lambda ps: R.grads(ps, 5))
    coefs = [t.item() for t in a[1:10:2]]
    assert min(coefs) < 0.5 and max(coefs) == 1.0, coefs  # the clip is active in some steps, off in others
    for what, x, y in (("layouts", a, b), ("separate twice", a, a2), ("flat twice", b, b2)):
        bad = [i for i, (u, v) in enumerate(zip(x, y)) if not torch.equal(u, v)]
        assert not bad, (what, bad)


def test_inactive_clip_is_the_identity():
    from skillful_nowcasting_amd.optim import FusedAdam

    pa, pb = R.params(), R.params()
    grads = R.grads(pa, 5)
    oa = FusedAdam(pa, lr=2e-3, betas=(0.9, 0.99))
    ob = FusedAdam(pb, lr=2e-3, betas=(0.9, 0.99), max_grad_norm=1e30)
    for step, row in enumerate(grads):
        R.set_grads(pa, row)
        R.set_grads(pb, row)
        oa.step()
        ob.step()
        assert ob.last_clip_coef.item() == 1.0, step
        for i, (u, v) in enumerate(zip(R.state(oa, pa), R.state(ob, pb))):
            assert torch.equal(u, v), (step, i)
    assert oa.last_grad_norm is None  # the plain optimiser never ran the guard


@pytest.mark.parametrize("betas", [(0.0, 0.999), (0.9, 0.99)])
def test_active_clip_matches_torch(betas):
    """torch.nn.utils.clip_grad_norm_(params, max_norm) followed by torch.optim.Adam.step(), at test_fused_adam_matches_torch_adam's
    tolerances.  With beta1 = 0.9 and a coefficient below 0.2 an unclipped exp_avg is off by a factor of five on the clipped steps:
    the test cannot pass with the clip missing."""
    from skillful_nowcasting_amd.optim import FusedAdam

    p_ref, p_got = R.params(), R.params()
    grads = R.grads(p_ref, 6)
    norms = sorted(_norm64(row) for row in grads)
    max_norm = 1.5 * norms[3]  # above the four smaller norms, far below the two at gradient scale 10
    want = [min(1.0, max_norm / (_norm64(row) + 1e-6)) for row in grads]
    assert sum(c < 0.2 for c in want) >= 2 and sum(c == 1.0 for c in want) >= 2, want
    ref = torch.optim.Adam(p_ref, lr=3e-3, betas=betas)
    got = FusedAdam(p_got, lr=3e-3, betas=betas, max_grad_norm=max_norm)
    coefs = []
    for step, row in enumerate(grads):
        R.set_grads(p_ref, row)
        R.set_grads(p_got, row)
        torch.nn.utils.clip_grad_norm_(p_ref, max_norm)
        ref.step()
        got.step()
        coefs.append(got.last_clip_coef.item())
        for g, b in zip(row, p_got):
            assert g is None or torch.equal(b.grad, g), step  # p.grad is never rewritten
        for a, b in zip(p_ref, p_got):
            assert (a - b).abs().max().item() <= 2e-6 * max(1.0, a.abs().max().item()), (betas, step)
    assert sum(c < 0.2 for c in coefs) >= 2 and sum(c == 1.0 for c in coefs) >= 2, coefs
    for a, b in zip(p_ref, p_got):
        sa, sb = ref.state[a], got.state[b]
        assert int(sa["step"]) == sb["step"]
        assert torch.allclose(sa["exp_avg"], sb["exp_avg"], rtol=1e-5, atol=1e-7)
        assert torch.allclose(sa["exp_avg_sq"], sb["exp_avg_sq"], rtol=1e-5, atol=1e-9)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")])
def test_skip_on_nonfinite_gradient(bad):
    from skillful_nowcasting_amd.optim import FusedAdam

    def poisoned(ps):
        grads = R.grads(ps, 5)
        grads[2][1].view(-1)[4096] = bad  # step 3, the last element of tensor 1: alone in its chunk
        return grads

    ps = R.params()
    grads = poisoned(ps)
    opt = FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), max_grad_norm=30.0, skip_nonfinite=True)
    before = None
    for step, row in enumerate(grads):
        R.set_grads(ps, row)
        opt.step()
        now = R.state(opt, ps)
        if step == 2:
            assert all(torch.equal(u, v) for u, v in zip(before, now)), "a skipped step stored something"
            assert opt.skipped_steps.item() == 1
            assert not torch.isfinite(opt.last_grad_norm).item()
            offenders = opt.nonfinite_parameters()
            assert len(offenders) == 1 and offenders[0] is ps[1]
            assert opt.nonfinite_parameters(names=[(f"t{i}", p) for i, p in enumerate(ps)]) == ["t1"]
        elif before is not None:
            with_grad = [i for i, g in enumerate(row) if g is not None]
            assert all(not torch.equal(before[3 * i], now[3 * i]) for i in with_grad), step  # updates again
            assert opt.nonfinite_parameters() == []
        before = now
    assert opt.skipped_steps.item() == 1
    assert all(torch.isfinite(t).all().item() for t in before)
    assert [opt.state[p]["step"] for p in ps] == [5, 5, 5, 3, 5, 5, 5]  # the host counter follows attempted steps

    # the default is torch's: garbage in, garbage out
    ps = R.params()
    opt = FusedAdam(ps, lr=2e-3, betas=(0.9, 0.99), max_grad_norm=30.0)
    for row in poisoned(ps)[:3]:
        R.set_grads(ps, row)
        opt.step()
    assert opt.skipped_steps.item() == 0
    assert not torch.isfinite(ps[1]).all().item()


def test_guarded_descriptor_tables_survive_a_gpu_backlog():
    """test_fused_adam_descriptor_tables_survive_a_gpu_backlog with the guard on: two parameter groups (one table, one norm pass, one
    guarded launch per group's slice), ~0.3 s of device work queued ahead and twelve steps without synchronisation, against the same
    settings synchronised after every step."""
    from skillful_nowcasting_amd.optim import FusedAdam

    shapes = [(5,), (4097,), (16, 8, 3, 3), (20000,), (1,), (129, 65)]

    def make():
        torch.manual_seed(21)
        ps = [torch.randn(s, device="cuda").requires_grad_(True) for s in shapes]
        return [dict(params=ps[:3], lr=1e-3), dict(params=ps[3:], lr=5e-3, betas=(0.5, 0.99))], ps

    (ga, pa), (gb, pb) = make(), make()
    oa = FusedAdam(ga, lr=1e-3, betas=(0.0, 0.999), max_grad_norm=50.0, skip_nonfinite=True)
    ob = FusedAdam(gb, lr=1e-3, betas=(0.0, 0.999), max_grad_norm=50.0, skip_nonfinite=True)
    torch.manual_seed(22)
    grads = [[torch.randn(s, device="cuda") * (10.0 ** (k % 3 - 1)) for s in shapes] for k in range(12)]
    big = torch.randn(8192, 8192, device="cuda")
    torch.cuda.synchronize()
    for _ in range(40):  # a backlog: the host runs far ahead of the device from here on
        big = torch.mm(big, big).clamp_(-1, 1)
    norms_a, norms_b = [], []
    for k in range(12):
        for p, g in zip(pa, grads[k]):
            p.grad = g
        oa.step()
        norms_a.append(oa.last_grad_norm.clone())
    torch.cuda.synchronize()
    for k in range(12):
        for p, g in zip(pb, grads[k]):
            p.grad = g
        ob.step()
        torch.cuda.synchronize()
        norms_b.append(ob.last_grad_norm.clone())
    coefs = [min(1.0, 50.0 / n.item()) for n in norms_b]
    assert min(coefs) < 0.2 and max(coefs) == 1.0, coefs
    for k, (u, v) in enumerate(zip(norms_a, norms_b)):
        assert torch.equal(u, v), k
    for i, (u, v) in enumerate(zip(R.state(oa, pa), R.state(ob, pb))):
        assert torch.equal(u, v), i
    # group 2 has its own lr and betas: the slices were launched with their own hyper-parameters
    ref = torch.optim.Adam(make()[0], lr=1e-3, betas=(0.0, 0.999))
    pr = [p for g in ref.param_groups for p in g["params"]]
    for k in range(12):
        for p, g in zip(pr, grads[k]):
            p.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(pr, 50.0)
        ref.step()
    for a, b in zip(pr, pa):
        assert (a - b).abs().max().item() <= 2e-6 * max(1.0, a.abs().max().item())


# ------------------------------------------------------------------------------------------------
# the whole training step
# ------------------------------------------------------------------------------------------------
KW = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2, beta1=0.5)


def _grad_norm64(module):
    return torch.linalg.vector_norm(torch.cat([p.grad.double().flatten() for p in module.parameters() if p.grad is not None])).item()


def _train(clip=None, flat=False):
    """Two seeded training steps -> what the tests below compare.  clip: (generator, discriminator) clip norms."""
    import skillful_nowcasting_amd as S

    S.set_precision("mixed")
    try:
        torch.manual_seed(7)
        model = S.DGMR(**KW).to("cuda")
        if clip is not None:
            model.gen_grad_clip_norm, model.disc_grad_clip_norm = clip
        if flat:
            model.attach_data_parallel()  # no process group: world 1, on flat gradient buffers
        torch.manual_seed(8)
        x = torch.rand(2, 4, 1, 128, 128, device="cuda")
        y = torch.rand(2, 2, 1, 128, 128, device="cuda")
        torch.manual_seed(9)
        g_opt, d_opt = model.optimizers()
        big_name, big = max(model.discriminator.named_parameters(), key=lambda kv: kv[1].numel())  # the largest discriminator weight
        d_updates = []  # (exp_avg of that weight, clip coefficient, float64 norm of the gradients, the guard's norm) of every discriminator update
        plain_step = d_opt.step

        def recording_step():
            plain_step()
            coef = d_opt.last_clip_coef
            d_updates.append((d_opt.state[big]["exp_avg"].clone(), None if coef is None else coef.clone(), _grad_norm64(model.discriminator),
                              None if coef is None else d_opt.last_grad_norm.clone()))

        d_opt.step = recording_step
        rec = dict(steps=[], d_updates=d_updates, big_name=big_name)
        for i in range(2):
            model.training_step((x, y), i)
            torch.cuda.synchronize()
            rec["steps"].append(dict(logged={k: v.detach().clone() for k, v in model.logged_metrics.items()},
                                     g_norm64=_grad_norm64(model.generator), d_norm64=_grad_norm64(model.discriminator),
                                     g_coef=None if g_opt.last_clip_coef is None else g_opt.last_clip_coef.item()))
        rec["params"] = [p.detach().clone() for p in model.parameters()]
        return rec
    finally:
        S.set_precision("f32")


@pytest.fixture(scope="module")
def whole_step_runs():
    """Unguarded; guarded at 0.1 x the norms the unguarded run of the same seed measured in its first step; the same on flat gradient
    buffers.  The discriminator's norm is taken at its FIRST update: on these random frames the hinge loss of the second pass is
    exactly 0 (d_loss = 0, as in smoke()) and so are its gradients - a norm of 0 is no clip norm."""
    plain = _train()
    print("unguarded run: generator norms", [st["g_norm64"] for st in plain["steps"]], "discriminator norms per update",
          [u[2] for u in plain["d_updates"]])
    clip = (0.1 * plain["steps"][0]["g_norm64"], 0.1 * plain["d_updates"][0][2])
    assert clip[0] > 0 and clip[1] > 0, clip
    return plain, _train(clip), _train(clip, flat=True)


def test_whole_step_logs_the_norms_and_clips(whole_step_runs):
    plain, guarded, _ = whole_step_runs
    for i, st in enumerate(guarded["steps"]):
        logged = st["logged"]
        assert set(logged) == {"train/d_loss", "train/g_loss", "train/grid_loss", "train/g_grad_norm", "train/d_grad_norm",
                               "train/skipped_steps"}
        for key, ref in (("train/g_grad_norm", st["g_norm64"]), ("train/d_grad_norm", st["d_norm64"])):
            got = logged[key].item()
            print(f"step {i} {key}: {got!r} float64 of p.grad {ref!r} rel {abs(got - ref) / max(ref, 1e-300):.2e}")
            assert abs(got - ref) <= ULP2 * ref, (i, key, got, ref)
        assert logged["train/skipped_steps"].item() == 0
    # the first guarded step, where the states still match the unguarded run's: coefficients of about 0.1
    g_coef = guarded["steps"][0]["g_coef"]
    d_coef = guarded["d_updates"][0][1].item()  # (the clip norm was taken from the first discriminator update)
    print(f"first guarded step: generator coefficient {g_coef}, discriminator (first update) {d_coef}; all discriminator updates: "
          f"{[(u[1].item(), u[2]) for u in guarded['d_updates']]}")
    assert g_coef < 0.2 and d_coef < 0.2, (g_coef, d_coef)
    for _, _, ref, got in guarded["d_updates"]:  # (the logged norm is the second update's, 0 here: the first one's is not)
        assert abs(got.item() - ref) <= ULP2 * ref, (got.item(), ref)
    # The first discriminator update of the run sees bit-identical gradients in both runs (same seed, same state): with beta1 = 0.5
    # exp_avg = 0.5 * g without the guard and 0.5 * (g * coef) with it
    m_plain, m_clip = plain["d_updates"][0][0].double(), guarded["d_updates"][0][0].double()
    coef = guarded["d_updates"][0][1].double()
    assert coef.item() < 1.0, coef.item()
    assert m_plain.numel() >= 100_000 and m_plain.abs().max().item() > 0
    err = ((m_clip - coef * m_plain).abs().max() / (coef * m_plain).abs().max()).item()
    print(f"exp_avg of discriminator.{plain['big_name']} after the first update: coefficient {coef.item()}, relative deviation {err:.2e}")
    assert err <= 1e-5, err
    assert any(not torch.equal(u, v) for u, v in zip(guarded["params"], plain["params"]))


def test_whole_step_on_flat_gradient_buffers_is_bit_identical(whole_step_runs):
    _, guarded, flat = whole_step_runs
    bad = [i for i, (u, v) in enumerate(zip(guarded["params"], flat["params"])) if not torch.equal(u, v)]
    assert not bad, f"{len(bad)} of {len(guarded['params'])} parameters differ on flat gradient buffers, e.g. {bad[:5]}"
    for a, b in zip(guarded["steps"], flat["steps"]):
        for key in ("train/g_grad_norm", "train/d_grad_norm"):
            assert torch.equal(a["logged"][key], b["logged"][key]), key


def test_whole_step_with_the_guard_off_logs_what_it_always_did(whole_step_runs):
    plain, _, _ = whole_step_runs
    for st in plain["steps"]:
        assert set(st["logged"]) == {"train/d_loss", "train/g_loss", "train/grid_loss"}
        assert st["g_coef"] is None
    assert all(u[1] is None for u in plain["d_updates"])
