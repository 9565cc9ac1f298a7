"""GPU: the two kinds of per-call state that the library replays on the device in the reference's call order - the spectral-norm
power iteration (dgmr_spectral_sigma_seq_multi through nn.SNPlan, dgmr_spectral_sigma through ops.spectral_sigma) and BatchNorm's
running statistics (bn_finalize_kernel through ops.bn_prepare) - against a float64 reference of the same operation, call by call, at
the smallest shapes that cross every boundary of the kernels (tests/sn_sequence_recipe.py names them).  Every test takes seconds."""
import functools
import json
import os

import pytest
import torch

import sn_sequence_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

DEV = "cuda"
# 3 x the float32-torch yardstick (tests/test_sn_sequence_host.py holds the same inputs to 1e-6 on the CPU): the kernels sum in another
# order and form n^2 from a rounded A.  Ten times inside the 2e-5 a single conv block is held to - 1/sigma multiplies all its outputs.
SN_TOL = 2e-6
# the whole-forward tolerances of tests/test_gpu_precision.py::test_goldens_in_reduced_modes for the modes whose Gram matrix is not an
# fp32 product; "mixed" outside a discriminator forward is bf16x3, inside ops.discriminator_forward_precision() it is bf16x6
REDUCED_TOL = {"bf16x3": 1e-4, "bf16": 5e-2, "mixed": 1e-4, "mixed, discriminator forward": 2e-5}
BN_TOL = 1e-5  # of each tensor's max magnitude (tests/test_gpu_ops_vs_torch.py::test_batchnorm1d_groups_vs_torch)

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/call_sequence_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "call_sequence_accuracy.json")


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _set_mode(mode):
    """An arithmetic mode by the name ops.get_precision() gives it; cached Gram matrices and weight images are of the old mode."""
    from skillful_nowcasting_amd import ops

    if "+d:" in mode:
        ops.set_precision(*mode.split("+d:"))
    else:
        ops.set_precision(mode)
    ops.bump_weights_epoch()


class _Case:
    """One module of the table on the device, with the float64 sequence of 2 x calls iterations from its seeded start (two runs of the
    plan: the second continues where the first stopped), in CALL order.  Shared by the tests of a session and never modified."""

    def __init__(self, name, variant):
        m, self.calls, self.layout, self.w64, self.u0, self.v0 = R.build_case(name, variant)
        self.name, self.variant, self.eps = name, variant, R.CASES[name][5]
        self.module = m.to(DEV).train()
        self.vec = getattr(self.module.parametrizations.weight, "0")
        self.sigma, self.u, self.v = R.power_iterations(self.w64, self.u0, self.v0, 2 * self.calls, self.eps)
        self.yardstick = R.f32_yardstick(self.w64, self.u0, self.v0, 2 * self.calls, self.eps)
        self.u0_dev, self.v0_dev = self.u0.to(DEV), self.v0.to(DEV)

    def reset(self):
        with torch.no_grad():  # in place: the plans hold these buffers' addresses
            self.vec._u.copy_(self.u0_dev)
            self.vec._v.copy_(self.v0_dev)

    def entry(self):
        return (self.module, self.calls, self.layout)

    def reference(self, run):
        """(1/sigma, u, v) of run 0 or 1 in GROUP order, and the state the module is left in."""
        sl = slice(run * self.calls, (run + 1) * self.calls)
        grouped = tuple(R.to_group_order(t, self.layout) for t in (1.0 / self.sigma[sl], self.u[sl], self.v[sl]))
        return grouped, (self.u[sl][-1], self.v[sl][-1])


@functools.lru_cache(maxsize=None)
def _case(name, variant):
    return _Case(name, variant)


def _take(plan_out, case):
    """Copies of one module's record of a plan run (the record's tensors are views of the run's arena) and of its buffers."""
    rec, lay = plan_out[id(case.module)]
    assert rec.groups == case.calls and lay == case.layout
    assert tuple(rec.inv_sigma.shape) == (case.calls,) and tuple(rec.u.shape) == (case.calls, case.w64.shape[0])
    assert tuple(rec.v.shape) == (case.calls, case.w64.shape[1])
    torch.cuda.synchronize()
    return tuple(t.detach().cpu().clone() for t in (rec.inv_sigma, rec.u, rec.v, case.vec._u, case.vec._v))


def _errors(got, case, run):
    (ris, ru, rv), (ru_end, rv_end) = case.reference(run)
    gis, gu, gv, mu, mv = got
    return {"inv_sigma": R.rel_per_call(gis, ris), "u": R.rel_per_call(gu, ru), "v": R.rel_per_call(gv, rv),
            "module_u": R.rel_per_call(mu[None], ru_end[None]), "module_v": R.rel_per_call(mv[None], rv_end[None])}


def _solo(case):
    from skillful_nowcasting_amd.nn import SNPlan

    return SNPlan([case.entry()])


ALL = [(n, v) for n in sorted(R.CASES) for v in R.VARIANTS]


@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
@pytest.mark.parametrize("name,variant", ALL)
def test_sequence_parity_with_float64(name, variant, mode):
    """Every call's 1/sigma, u and v at the group slot its layout assigns, and the module's _u / _v afterwards, against the float64
    recipe from the same start; then a second run of the SAME plan against iterations calls + 1 ... 2 x calls (the state carries over).
    Per call, max error over max magnitude (so case f, whose sigma falls by 1e3 per call, is judged call by call).
    Measured (profiles/call_sequence_accuracy.json): worst 1.2e-6 (v of case e, plain weights, f32), 1/sigma within 2.5e-7."""
    from skillful_nowcasting_amd import ops

    case = _case(name, variant)
    prev = ops.get_precision()
    try:
        _set_mode(mode)
        case.reset()
        plan = _solo(case)
        runs = [_errors(_take(plan.run(), case), case, 0)]
        assert plan.valid()
        runs.append(_errors(_take(plan.run(), case), case, 1))
    finally:
        _set_mode(prev)
    ys = dict(zip(("sigma", "u", "v"), case.yardstick))
    _log_accuracy(f"sn/{name}/{variant}/{mode}", {"first_run": runs[0], "second_run": runs[1], "float32_torch": ys, "bound": SN_TOL})
    print(f"case {name} [{variant}, {mode}]: first run {runs[0]}\n  second run {runs[1]}\n  float32 torch on the CPU {ys}")
    for i, e in enumerate(runs):
        bad = {k: x for k, x in e.items() if not x <= SN_TOL}
        assert not bad, f"run {i + 1}: beyond {SN_TOL:.0e}: {bad} (float32 torch: {ys})"


@pytest.mark.parametrize("mode", ["f32", "bf16x6"])
@pytest.mark.parametrize("variant", R.VARIANTS)
def test_one_plan_of_seven_equals_seven_plans(variant, mode):
    """Cases a - g as one-module plans, then as ONE plan in the order d, c, a, g, b, f, e from the same starting u / v: every sum in
    these kernels has a fixed order, only the block -> module search, the per-module T and max_cout / max_T differ: the same bits."""
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd.nn import SNPlan

    cases = {n: _case(n, variant) for n in R.JOINT_ORDER}
    prev = ops.get_precision()
    try:
        _set_mode(mode)
        alone = {}
        for n, c in cases.items():
            c.reset()
            alone[n] = _take(_solo(c).run(), c)
        for c in cases.values():
            c.reset()
        joint = SNPlan([cases[n].entry() for n in R.JOINT_ORDER])
        assert joint.max_calls == 108 and joint.max_cout == 100
        out = joint.run()
        together = {n: _take(out, c) for n, c in cases.items()}
    finally:
        _set_mode(prev)
    names = ("1/sigma", "u", "v", "module _u", "module _v")
    bad = [(n, what) for n in R.JOINT_ORDER for what, a, b in zip(names, alone[n], together[n]) if not torch.equal(a, b)]
    assert not bad, f"the joint plan differs from the one-module plans in {bad}"
    for n, c in cases.items():  # ... and they are the right bits (the joint plan against float64, as above)
        e = _errors(together[n], c, 0)
        assert max(e.values()) <= SN_TOL, (n, e)


@pytest.mark.parametrize("variant", R.VARIANTS)
@pytest.mark.parametrize("name", ["a", "c", "g"])
def test_single_call_path(name, variant):
    """ops.spectral_sigma (three small kernels of its own): a train-mode call is one recipe iteration - record and buffers - and an
    eval-mode call behind it returns 1 / (u^T W v) of the state it finds and leaves u, v bit-unchanged."""
    from skillful_nowcasting_amd import ops

    case = _case(name, variant)
    m = case.module
    case.reset()
    rec = ops.spectral_sigma(m.weight_orig, case.vec._u, case.vec._v, m._scratch, m.eps, True)
    torch.cuda.synchronize()
    assert rec.groups == 1 and tuple(rec.u.shape) == (1, case.w64.shape[0]) and tuple(rec.v.shape) == (1, case.w64.shape[1])
    got = {"inv_sigma": rec.inv_sigma.cpu(), "u": rec.u.cpu(), "v": rec.v.cpu(), "module_u": case.vec._u.cpu()[None],
           "module_v": case.vec._v.cpu()[None]}
    ref = {"inv_sigma": 1.0 / case.sigma[:1], "u": case.u[:1], "v": case.v[:1], "module_u": case.u[:1], "module_v": case.v[:1]}
    errs = {k: R.rel_per_call(got[k], ref[k]) for k in got}
    print(f"case {name} [{variant}] single call, train: {errs}")
    assert max(errs.values()) <= SN_TOL, errs
    assert torch.equal(got["u"], got["module_u"]) and torch.equal(got["v"], got["module_v"])
    assert float(m._scratch.abs().max()) == 0.0
    # eval: no iteration; sigma = u^T W v of the converged-by-one-call state (no cancellation: it is ||W^T u|| up to rounding)
    u1, v1 = case.vec._u.clone(), case.vec._v.clone()
    ev = ops.spectral_sigma(m.weight_orig, case.vec._u, case.vec._v, m._scratch, m.eps, False)
    torch.cuda.synchronize()
    assert torch.equal(case.vec._u, u1) and torch.equal(case.vec._v, v1), "an eval-mode call moved u / v"
    assert torch.equal(ev.u[0], u1) and torch.equal(ev.v[0], v1)
    sig = torch.dot(u1.cpu().double(), torch.mv(case.w64, v1.cpu().double()))
    e = abs(ev.inv_sigma.item() * sig.item() - 1.0)
    print(f"  eval: 1/sigma off by {e:.2e}")
    assert e <= SN_TOL


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_one_call_plan_and_single_call_kernels_agree(variant):
    """Case g (one call) through the sequence kernels and through dgmr_spectral_sigma - different kernels - from the same start:
    both within the bound of the float64 value."""
    from skillful_nowcasting_amd import ops

    case = _case("g", variant)
    m = case.module
    case.reset()
    by_plan = _take(_solo(case).run(), case)
    case.reset()
    rec = ops.spectral_sigma(m.weight_orig, case.vec._u, case.vec._v, m._scratch, m.eps, True)
    by_call = _take({id(m): (rec, None)}, case)
    for what, got in (("plan", by_plan), ("single call", by_call)):
        e = _errors(got, case, 0)
        print(f"case g [{variant}] {what}: {e}")
        assert max(e.values()) <= SN_TOL, (what, e)


@pytest.mark.parametrize("mode", sorted(REDUCED_TOL))
def test_sequences_in_reduced_arithmetic(mode):
    """ops.weight_gram runs on the conv kernel in whatever mode set_precision holds, so in bf16x3, bf16 and mixed the A that the
    sequence iterates on is not an fp32 product.  Cases a, b, d (both weight variants), worst error of 1/sigma, u, v per mode.

    Which mode a Gram matrix is formed in under "mixed" follows from where it is refreshed: SNPlan.run() calls module._gram() in the
    mode in force when run() is CALLED.  Discriminator.forward / forward_split enter ops.discriminator_forward_precision() BEFORE
    SNScope, whose __enter__ runs the plan: a discriminator Gram is a bf16x6 product.  SNScope._prefetch only ever runs plans of the
    generator (SNScope.step brackets the generator alone), from a generator scope's __enter__: bf16x3, like the generator's forward."""
    from skillful_nowcasting_amd import ops

    prev = ops.get_precision()
    worst = {}
    try:
        _set_mode(mode.split(",")[0])
        for name in ("a", "b", "d"):
            for variant in R.VARIANTS:
                case = _case(name, variant)
                case.reset()
                if "discriminator" in mode:
                    assert ops.get_precision() == "mixed"
                    with ops.discriminator_forward_precision():
                        assert ops._PRECISION_CODE == ops.PRECISIONS["bf16x6"]
                        got = _take(_solo(case).run(), case)
                    assert ops._PRECISION_CODE == ops.PRECISIONS["bf16x3"]
                else:
                    got = _take(_solo(case).run(), case)
                e = _errors(got, case, 0)
                ys = dict(zip(("sigma", "u", "v"), case.yardstick))
                _log_accuracy(f"sn/{name}/{variant}/{mode}", {"first_run": e, "float32_torch": ys, "bound": REDUCED_TOL[mode]})
                print(f"case {name} [{variant}, {mode}]: {e}")
                for k, x in e.items():
                    worst[k] = max(worst.get(k, 0.0), x)
    finally:
        _set_mode(prev)
    _log_accuracy(f"sn/worst/{mode}", dict(worst, bound=REDUCED_TOL[mode]))
    bad = {k: x for k, x in worst.items() if not x <= REDUCED_TOL[mode]}
    assert not bad, f"{mode}: beyond {REDUCED_TOL[mode]:.0e}: {bad}"


def test_discriminator_gram_is_formed_in_its_forward_mode(monkeypatch):
    """What the docstring above reads from the code, observed: under "mixed" every W W^T that a discriminator forward refreshes -
    the first, traced pass (one-module plans from inside the forward) and the planned pass (SNScope.__enter__ -> SNPlan.run) - is
    computed with the library in bf16x6, and the global mode is bf16x3 again behind the forward."""
    import skillful_nowcasting_amd as S
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd.nn import SNScope

    torch.manual_seed(3)
    d = S.Discriminator(input_channels=1).to(DEV).train()
    x = torch.rand(2, 7, 1, 128, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    seen = []
    orig = ops.weight_gram

    def spy(w, out=None):
        seen.append(ops._PRECISION_CODE)
        return orig(w, out=out)

    monkeypatch.setattr(ops, "weight_gram", spy)
    prev = ops.get_precision()
    try:
        _set_mode("mixed")
        for planned in (False, True):
            del seen[:]
            ops.bump_weights_epoch()  # every cached Gram matrix is stale: this forward rebuilds them
            with torch.no_grad():
                torch.manual_seed(17)
                out = d(x)
            torch.cuda.synchronize()
            assert torch.isfinite(out).all()
            assert any(k[0] == id(d) for k in SNScope._plans)  # the first pass left a plan, the second was served from it
            # (traced: only modules with more than one call go through a plan; planned: every module of the forward)
            assert len(seen) >= (10 if planned else 1), f"{'planned' if planned else 'traced'} pass: {len(seen)} Gram matrices refreshed"
            assert set(seen) == {ops.PRECISIONS["bf16x6"]}, f"{'planned' if planned else 'traced'} pass: Gram matrices formed in modes {set(seen)}"
            assert ops._PRECISION_CODE == ops.PRECISIONS["bf16x3"] and ops.get_precision() == "mixed"
    finally:
        _set_mode(prev)
        for k in [k for k in SNScope._plans if k[0] == id(d)]:
            del SNScope._plans[k]


# ---- BatchNorm: running statistics in the reference's call order ---------------------------------------------------------------------------
def _bn_layout(g):
    from skillful_nowcasting_amd.ops import CallLayout

    return {108: CallLayout(6, 18, True, True), 24: CallLayout(6, 4, False, True)}.get(g)


@functools.lru_cache(maxsize=None)
def _bn_reference(g, c, h, w):
    """x = 100 + randn (mean^2 / var = 1e4, the ratio the kernels' header comment is about), float32 values; torch's BatchNorm2d in
    float64, called once per group in the reference's call order, from non-trivial weight, bias and running statistics."""
    gen = torch.Generator().manual_seed(10000 + 1000 * h * w + 10 * g + c)
    x = (100.0 + torch.randn(g, c, h, w, generator=gen)).float()
    start = {"weight": torch.rand(c, generator=gen) + 0.5, "bias": torch.randn(c, generator=gen),
             "running_mean": 100.0 + torch.randn(c, generator=gen), "running_var": torch.rand(c, generator=gen) + 0.5}
    bn = torch.nn.BatchNorm2d(c).double().train()
    with torch.no_grad():
        for k, t in start.items():
            getattr(bn, k).copy_(t)
        bn.num_batches_tracked.fill_(7)
    lay = _bn_layout(g)
    order = lay.slots() if lay is not None else list(range(g))
    with torch.no_grad():
        for q in order:
            bn(x[q:q + 1].double())
    xd = x.double()
    mean = xd.mean(dim=(2, 3))
    rstd = (xd.var(dim=(2, 3), unbiased=False) + bn.eps).rsqrt()
    a = bn.weight.detach() * rstd
    ref = {"a": a, "b": bn.bias.detach() - mean * a, "mean": mean, "rstd": rstd, "running_mean": bn.running_mean.clone(),
           "running_var": bn.running_var.clone()}
    return x, start, ref, int(bn.num_batches_tracked), bn.eps, bn.momentum


def _bn_run(g, c, h, w):
    from skillful_nowcasting_amd import ops

    x, start, _, _, eps, momentum = _bn_reference(g, c, h, w)
    xd = x.to(DEV).contiguous(memory_format=torch.channels_last)
    p = {k: t.float().to(DEV) for k, t in start.items()}
    nbt = torch.full((), 7, device=DEV, dtype=torch.int64)
    st = ops.bn_prepare(xd, p["weight"], p["bias"], p["running_mean"], p["running_var"], nbt, eps, momentum, True, g, _bn_layout(g))
    torch.cuda.synchronize()
    assert st.train and st.groups == g and st.group_size == 1
    got = {"a": st.a, "b": st.b, "mean": st.mean, "rstd": st.rstd, "running_mean": p["running_mean"], "running_var": p["running_var"]}
    return {k: t.cpu() for k, t in got.items()}, int(nbt)


def _bn_check(g, c, h, w):
    from skillful_nowcasting_amd import ops

    _, _, ref, nbt_ref, _, _ = _bn_reference(g, c, h, w)
    prev = ops.deterministic()
    try:
        for det in (True, False):
            ops.set_deterministic(det)
            got, nbt = _bn_run(g, c, h, w)
            errs = {k: (got[k].double() - ref[k]).abs().max().item() / ref[k].abs().max().item() for k in ref}
            _log_accuracy(f"bn/G{g}/C{c}/R{h * w}/deterministic={int(det)}", errs)
            print(f"G = {g}, C = {c}, R = {h * w}, deterministic = {det}: {errs}")
            assert all(tuple(got[k].shape) == tuple(ref[k].shape) for k in ref)
            bad = {k: e for k, e in errs.items() if not e <= BN_TOL}
            assert not bad, f"deterministic = {det}: beyond {BN_TOL:.0e}: {bad}"
            assert nbt == nbt_ref == 7 + g
            if det:
                again, _ = _bn_run(g, c, h, w)
                differ = [k for k in got if not torch.equal(got[k], again[k])]
                assert not differ, f"two deterministic runs differ in {differ}"
    finally:
        ops.set_deterministic(prev)


@pytest.mark.parametrize("c", [4, 48, 100, 260])
@pytest.mark.parametrize("g", [1, 17, 65, 108, 24])
def test_batchnorm_call_order_vs_torch(g, c):
    """ops.bn_prepare in train mode on [G, C, 2, 2] (R = 4): a, b, mean, rstd of every group, and the running statistics after G
    updates applied in the reference's call order (identity for G = 1, 17, 65 - a second BNF_Q chunk; the sampler's reversed
    time-major map for 108; the draw-major one for 24), in both deterministic modes; bit-identical reruns in deterministic mode.
    C = 260 crosses chan_reduce2's 256-column chunk with a 4-wide tail, 100 is ragged against BNF_C, 48 leaves 16 threads idle."""
    _bn_check(g, c, 2, 2)


def test_batchnorm_two_rows_per_group():
    """R = 2: Bessel's factor is 2 (and the largest the running variance ever sees)."""
    _bn_check(17, 48, 2, 1)
