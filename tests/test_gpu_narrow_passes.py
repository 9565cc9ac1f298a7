"""GPU: three single-purpose passes taken off the step's exposed stretches, through the C ABI and one sampler level.

  1. the streaming 1x1 conv kernel (conv1x1.h) writes the BatchNorm partial sums of its output from its epilogue (stats_out): one row
     [2][Cout] per 256-pixel tile, bit-reproducible, y untouched;
  2. SNConv 1x1 -> GBlock, forward and backward, with those statistics and with the separate statistics pass: two routes to the same
     sums, both held to the float64 oracle;
  3. dgmr_wgrad_reduce[_slice] on narrow weights: the groups' slab sums first, over the whole chip (wgrad_group_sum_kernel), then the
     reduce over one slab per group - the same bits as the single launch;
  4. dgmr_sn_wgrad_finalize through the LDS-tiled kernel: the same bits as the one-thread-per-element kernel.

The statistics of 1 are another rounding of the batch sums than the separate pass and are off by default: dgmr_debug_flags 512 switches
them on inside a process (DGMR_CONV1X1_STATS=1 for a whole process).  3 and 4 give the bits of the kernels they replace and are on;
flags 1024 / 2048 switch them off (DGMR_WGRAD_NARROW / DGMR_SN_FINALIZE_TILED = 0).  That the new kernels are what runs is checked by
what only they do: the group sums left in the consumed partial sums, and the tiled finalize's dispatch probe (flag 4096).
"""
import ctypes

import pytest
import torch

from conftest import rel_err

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24  # unit roundoff of fp32
STATS, NO_NARROW, NO_TILED, PROBE = 512, 1024, 2048, 4096


@pytest.fixture()
def flags():
    from skillful_nowcasting_amd._lib import call

    yield lambda f: call("dgmr_debug_flags", f)
    call("dgmr_debug_flags", 0)


@pytest.fixture()
def precision():
    import skillful_nowcasting_amd as S

    yield S.set_precision
    S.set_precision("f32")


# ------------------------------------------------------------------------------------------------------------------------------
# 1. statistics in the 1x1 kernel's epilogue
# ------------------------------------------------------------------------------------------------------------------------------
# The smallest launch the kernel takes: 131072 pixels (512 tiles of 256), here 128 maps of 32 x 32.
# (cin, cout, act_relu, scale groups): one full 96-column tile; a K tail (40 = 32 + 8) with a 64-column tile whose last 16 columns
# are dead; relu; four spectral-norm groups (= BatchNorm groups: 128 tiles each); two column tiles, the second one partly dead.
# A launch whose M is not a multiple of 256 while D*H*W is cannot exist: M = N * D*H*W, so the kernel's row bound m < M never cuts a
# tile short through the dispatch (the bound is still applied to the sums, as to the stores).
STATS_CASES = [(32, 96, False, 1), (40, 48, False, 1), (32, 96, True, 1), (40, 48, False, 4), (32, 160, False, 1)]
N1, H1 = 128, 32


@pytest.mark.parametrize("mode", ["bf16x3", "bf16"])
@pytest.mark.parametrize("cin,cout,relu,groups", STATS_CASES)
def test_conv1x1_statistics(precision, flags, mode, cin, cout, relu, groups):
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd._lib import ConvArgs, call, load

    precision(mode)
    lib = load()
    torch.manual_seed(cin + cout)
    m = N1 * H1 * H1
    x = torch.randn(m * cin, device=DEV)
    wt = torch.randn(cout * cin, device=DEV) * 0.2
    bias = torch.randn(cout, device=DEV)
    scale = torch.rand(groups, device=DEV) + 0.5
    planes = ops._PLANES[ops.PRECISIONS[mode]]
    wsp = torch.empty(planes * wt.numel(), device=DEV, dtype=torch.int16)
    call("dgmr_split_weights", wt.data_ptr(), wsp.data_ptr(), cout, cin, 0, 0, planes, 0, ops._stream())

    # the library picks the streaming 1x1 kernel for this launch, with and without stats_out (host arithmetic: nothing is launched)
    a = ConvArgs()
    a.x, a.w, a.y, a.scale, a.bias, a.w_split = x.data_ptr(), wt.data_ptr(), x.data_ptr(), scale.data_ptr(), bias.data_ptr(), wsp.data_ptr()
    a.N, a.D, a.H, a.W, a.Cin, a.Cout, a.KD, a.KH, a.KW = N1, 1, H1, H1, cin, cout, 1, 1, 1
    a.scale_group, a.pre_group, a.mask_group, a.act_relu = N1 // groups, 1, 1, int(relu)
    detail, ksplit = ctypes.c_uint32(0), ctypes.c_int32(0)
    assert lib.dgmr_conv_plan(ctypes.byref(a), ctypes.byref(detail), ctypes.byref(ksplit)) == 0, lib.dgmr_last_error()
    assert detail.value & 15 == 5, f"not the streaming 1x1 kernel: detail {detail.value:#x}"
    # off (the default): no rows, so a caller gets no partial sums and the BatchNorm behind the conv reads y
    assert lib.dgmr_conv_stats_rows(ctypes.byref(a)) == 0
    flags(STATS)
    assert lib.dgmr_conv_stats_rows(ctypes.byref(a)) == m // 256
    a.stats_out = x.data_ptr()
    assert lib.dgmr_conv_plan(ctypes.byref(a), ctypes.byref(detail), ctypes.byref(ksplit)) == 0, lib.dgmr_last_error()
    assert detail.value & 15 == 5, f"stats_out moves the conv off the streaming 1x1 kernel: detail {detail.value:#x}"

    def run(want):
        y = torch.full((m * cout,), float("nan"), device=DEV)
        part = ops._launch_conv(x, wt.data_ptr(), bias, scale, y, N1, 1, H1, H1, cin, cout, 1, 1, 1, scale_group=N1 // groups,
                                act_relu=relu, w_split=wsp, want_stats=want)
        torch.cuda.synchronize()
        return y, part

    y0, none = run(False)
    flags(0)
    assert run(True)[1] is None
    flags(STATS)
    y1, p1 = run(True)
    y2, p2 = run(True)
    assert none is None and p1 is not None and tuple(p1.shape) == (m // 256, 2, cout)
    assert not torch.isnan(y0).any()
    assert torch.equal(y0, y1), "stats_out changes y"
    assert torch.equal(p1, p2) and torch.equal(y1, y2), "two launches differ"
    # each row against the float64 sums of its own tile of y as stored: fp32 summation of 256 terms, 256 * 2^-24 * sum |term|
    t = y1.view(m // 256, 256, cout).double()
    worst = 0.0
    for which, terms in ((0, t), (1, t * t)):
        ref, mag = terms.sum(1), terms.abs().sum(1)
        err, bound = (p1[:, which, :].double() - ref).abs(), 256 * U * mag
        assert bool((err <= bound).all()), f"sum y^{which + 1}: worst err / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
        worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
    print(f"\nconv1x1 statistics [{mode}] cin {cin} cout {cout} relu {relu} groups {groups}: worst err / bound {worst:.4f}")


# ------------------------------------------------------------------------------------------------------------------------------
# 2. one sampler level: SNConv 1x1 -> GBlock
# ------------------------------------------------------------------------------------------------------------------------------
def test_sampler_level_statistics_routes(precision, flags):
    """GBlock.bn1's batch sums from the 1x1 conv's epilogue (fp32 per-tile partials, then double) against the separate statistics pass
    (double from the first element).  Both are rounding routes to the same sums.

    How far apart may they be?  A per-tile fp32 sum of 256 terms lies within 256 * 2^-24 * sum |term| of the exact one, so the batch
    mean and E[x^2] carry at most that relative error (of mean |x| and E[x^2]); they enter the block only through bn1's affine
    a = gamma * rstd, b = beta - mean * a, which moves a unit-variance element by at most about that much; behind it come relu
    (1-Lipschitz), spectral-normed convs (gain about 1) and a BatchNorm that normalises again.  So D = 256 * 2^-24 = 1.5e-5 of a
    tensor's largest entry bounds fused against separate, for the running statistics, the block output and - the same first-order
    argument, away from relu kinks - the gradients (roundings do not align: the expected distance is sqrt(256) * 2^-24, and 0.1 D
    was measured).  Asserted: that distance, per tensor.  And the band: the separate pass's error e_off against the float64 oracle
    of the same tensors is measured, and the fused route gets the same band - e_on <= e_off + D, no factor and no allowance for
    outliers (e_on <= e_off alone would fail a correct kernel half of the time: the two errors differ by rounding of either sign)."""
    import skillful_nowcasting_amd as S
    from oracle import dgmr_oracle as O
    from skillful_nowcasting_amd.common import GBlock
    from skillful_nowcasting_amd.nn import SNConv

    precision("bf16x3")
    c = 32
    torch.manual_seed(5)
    mods = torch.nn.ModuleDict({"c11": SNConv(c, c, 1), "g": GBlock(c, c)})
    sd0 = {k: v.detach().clone() for k, v in mods.state_dict().items()}
    x = torch.randn(N1, c, H1, H1)
    cot = torch.randn(N1, c, H1, H1)
    mods = mods.to(DEV)
    wkey = "c11.parametrizations.weight.original"
    keys = ("g.bn1.running_mean", "g.bn1.running_var", "g.bn2.running_mean")

    def run(flag):
        mods.load_state_dict(sd0)
        S.ops.bump_weights_epoch()
        mods.train()
        for p in mods.parameters():
            p.grad = None
        flags(flag)
        xg = x.to(DEV).requires_grad_(True)
        h, st = mods["c11"](xg, want_stats=True)
        assert (st is not None) == (flag == STATS), "the 1x1 kernel's statistics do not follow the switch"
        out = mods["g"](h, in_stats=st)
        out.backward(cot.to(DEV))
        torch.cuda.synchronize()
        sd1 = mods.state_dict()
        res = {"block output": out.detach(), "grad input": xg.grad, "grad 1x1 weight": dict(mods.named_parameters())[wkey].grad}
        res.update({"state " + k: sd1[k].detach() for k in keys})
        return {k: v.cpu().float().clone() for k, v in res.items()}

    on, off = run(STATS), run(0)
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = {k: (v.clone().double() if v.is_floating_point() else v.clone()) for k, v in sd0.items()}
    sd[wkey].requires_grad_(True)
    x64 = x.double().requires_grad_(True)
    out64 = O.gblock(sd, "g.", O.sn_conv(sd, "c11.", x64, True), True)
    out64.backward(cot.double())
    ref = {"block output": out64.detach(), "grad input": x64.grad, "grad 1x1 weight": sd[wkey].grad}
    ref.update({"state " + k: sd[k].detach() for k in keys})
    d_max = 256 * U
    bad = []
    print(f"\nSNConv 1x1 -> GBlock [bf16x3]: statistics from the conv epilogue (on) and from the separate pass (off); D = {d_max:.2e}")
    for k in ref:
        r64 = ref[k].double()
        e_on, e_off = rel_err(on[k].reshape(r64.shape), r64), rel_err(off[k].reshape(r64.shape), r64)
        dist = float((on[k].double() - off[k].double()).abs().max() / off[k].double().abs().max())
        ok = dist <= d_max and e_on <= e_off + d_max
        print(f"  {k:28s} on against float64 {e_on:.3e}  off against float64 {e_off:.3e}  on against off {dist:.2e}  {'ok' if ok else 'FAIL'}")
        if not ok:
            bad.append(k)
    assert not bad, f"fused statistics leave the separate pass's band: {bad}"


# ------------------------------------------------------------------------------------------------------------------------------
# 3. narrow weight-gradient reduces
# ------------------------------------------------------------------------------------------------------------------------------
def _reduce(partial, ns, groups, numel, w, scale, slice_=None):
    """One launch on a COPY of the partial sums (the narrow path consumes them) -> (g, dot[:groups], the copy after the launch)."""
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd._lib import call, load

    p = partial.clone()
    dot = torch.zeros(int(load().dgmr_wgrad_dot_floats(groups)), device=DEV)
    if slice_ is None:
        g = torch.full((numel,), float("nan"), device=DEV)
        call("dgmr_wgrad_reduce", p.data_ptr(), ns, groups, numel, w.data_ptr(), scale.data_ptr(), g.data_ptr(), dot.data_ptr(), ops._stream())
    else:
        cout, taps, cs, ct, coff = slice_
        g = torch.full((cout * taps * ct,), float("nan"), device=DEV)
        call("dgmr_wgrad_reduce_slice", p.data_ptr(), ns, groups, cout, taps, cs, ct, coff, w.data_ptr(), scale.data_ptr(), g.data_ptr(),
             dot.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    return g, dot[:groups].clone(), p


# (numel, groups, slabs per group, slice): the 4 x 48 weight of the sampler's output layer with its 108 call groups - one slab per group
# (nothing to pre-sum: the single launch), seven (the tail walk alone), 64 (eight rounds of the eight-load walk); three
# workgroups' worth with an odd slab count (four rounds and a tail of one); a true slice (cs = 8 of ct = 24 input channels at offset 8, 8 x 9 rows)
REDUCE_CASES = [(192, 108, 1, None), (192, 108, 7, None), (192, 108, 64, None), (576, 6, 33, None), (576, 6, 33, (8, 9, 8, 24, 8))]


@pytest.mark.parametrize("numel,groups,spg,slice_", REDUCE_CASES)
def test_narrow_wgrad_reduce(flags, numel, groups, spg, slice_):
    from skillful_nowcasting_amd._lib import load

    lib = load()
    torch.manual_seed(numel + spg)
    ns = groups * spg
    partial = torch.randn(ns * numel, device=DEV)
    scale = torch.rand(groups, device=DEV) + 0.5
    wlen = numel if slice_ is None else slice_[0] * slice_[1] * slice_[3]
    w = torch.randn(wlen, device=DEV)
    if slice_ is None:
        idx = torch.arange(numel, device=DEV)
    else:
        cout, taps, cs, ct, coff = slice_
        i = torch.arange(numel, device=DEV)
        idx = (i // cs) * ct + coff + i % cs  # (co, tap, ci) of the slab -> (co * taps + tap) * ct + coff + ci
    # float64 reference and the bounds n_terms * 2^-24 * sum |terms| per element of g and per dot
    p64 = partial.view(groups, spg, numel).double()
    g64 = (p64.sum(1) * scale.double()[:, None]).sum(0)
    g_bound = ns * U * (p64.abs().sum(1) * scale.double()[:, None]).sum(0)
    d64 = (p64.sum(1) * w.double()[idx]).sum(1)
    d_bound = spg * numel * U * (p64.abs().sum(1) * w.double()[idx].abs()).sum(1)
    was = lib.dgmr_get_deterministic()
    try:
        res = {}
        for det in (1, 0):
            lib.dgmr_set_deterministic(det)
            for flag in (0, NO_NARROW):
                flags(flag)
                g, d, used = _reduce(partial, ns, groups, numel, w, scale, slice_)
                g2, d2, _ = _reduce(partial, ns, groups, numel, w, scale, slice_)
                # which kernels ran: the two-stage path leaves each group's sum (slabs added in order, fp32) in the group's slab 0 and
                # nothing else changed; the single launch leaves the partial sums alone
                expect = partial.clone().view(groups, spg, numel)
                if flag == 0 and spg >= 4:
                    acc = torch.zeros(groups, numel, device=DEV)
                    for k in range(spg):
                        acc = acc + expect[:, k]
                    assert not torch.equal(acc, expect[:, 0])
                    expect[:, 0] = acc
                assert torch.equal(used.view(groups, spg, numel), expect), f"not the expected reduce path (det {det}, flag {flag})"
                assert torch.equal(g[idx], g2[idx]), (det, flag)
                # (without deterministic mode the workgroups' dots meet in float atomics: reproducible with one workgroup only)
                if det or numel <= 256:
                    assert torch.equal(d, d2), (det, flag)
                if slice_ is not None:
                    keep = torch.ones_like(g, dtype=torch.bool)
                    keep[idx] = False
                    assert bool(torch.isnan(g[keep]).all()), "the sliced reduce wrote outside its slice"
                ge, de = (g[idx].double() - g64).abs(), (d.double() - d64).abs()
                print(f"numel {numel} groups {groups} spg {spg} det {det} flag {flag}: g err / bound {float((ge / g_bound).max()):.4f}, "
                      f"dot err / bound {float((de / d_bound).max()):.4f}")
                assert bool((ge <= g_bound).all()) and bool((de <= d_bound).all()), (det, flag)
                res[det, flag] = (g, d)
        # g does not depend on the mode
        assert torch.equal(res[1, 0][0][idx], res[0, 0][0][idx]) and torch.equal(res[1, NO_NARROW][0][idx], res[0, NO_NARROW][0][idx])
        # the group sums are taken in the single launch's order: the two paths give the same bits (the dots where they are reproducible)
        for det in (1, 0):
            assert torch.equal(res[det, 0][0][idx], res[det, NO_NARROW][0][idx]), f"two-stage reduce differs from the single launch, det {det}"
            if det or numel <= 256:
                assert torch.equal(res[det, 0][1], res[det, NO_NARROW][1]), f"two-stage dots differ from the single launch, det {det}"
    finally:
        lib.dgmr_set_deterministic(was)


def test_wide_wgrad_reduce_is_untouched(flags):
    """1024 workgroups (numel = 262144): the single launch with the switch on or off, bit for bit."""
    numel, groups, spg = 1024 * 256, 2, 4
    torch.manual_seed(9)
    partial = torch.randn(groups * spg * numel, device=DEV)
    scale, w = torch.rand(groups, device=DEV) + 0.5, torch.randn(numel, device=DEV)
    flags(0)
    g_on, d_on, used = _reduce(partial, groups * spg, groups, numel, w, scale)
    assert torch.equal(used, partial), "a 1024-workgroup reduce took the two-stage path"
    flags(NO_NARROW)
    g_off, d_off, _ = _reduce(partial, groups * spg, groups, numel, w, scale)
    assert not torch.isnan(g_on).any()
    assert torch.equal(g_on, g_off) and torch.equal(d_on, d_off)


# ------------------------------------------------------------------------------------------------------------------------------
# 4. spectral-norm finalize
# ------------------------------------------------------------------------------------------------------------------------------
# (Cout, Cin, taps, groups): the issue's three; then ragged in every direction - 10 channels = one tile of 8 + 2, 36 input channels
# = a tile of 28 + 8, 17 groups = a chunk of 16 + 1
FINALIZE_CASES = [(48, 40, 9, 5), (4, 48, 1, 108), (96, 96, 27, 2), (10, 36, 9, 17)]


@pytest.mark.parametrize("accumulate", [1, 0])
@pytest.mark.parametrize("cout,cin,taps,groups", FINALIZE_CASES)
def test_sn_finalize_tiled_equals_elementwise(flags, cout, cin, taps, groups, accumulate):
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd._lib import call

    torch.manual_seed(cout + cin + taps)
    n = cout * cin * taps
    g, gw0 = torch.randn(n, device=DEV), torch.randn(n, device=DEV)
    dot0, inv_sigma = torch.randn(groups, device=DEV), torch.rand(groups, device=DEV) + 0.5
    u, v = torch.randn(groups * cout, device=DEV), torch.randn(groups * cin * taps, device=DEV)

    def run(flag, with_uv=True):
        flags(flag)
        gw, dot = gw0.clone(), dot0.clone()
        if with_uv:
            call("dgmr_sn_wgrad_finalize", g.data_ptr(), gw.data_ptr(), dot.data_ptr(), inv_sigma.data_ptr(), u.data_ptr(), v.data_ptr(),
                 cout, cin, taps, groups, accumulate, ops._stream())
        else:
            call("dgmr_sn_wgrad_finalize", g.data_ptr(), gw.data_ptr(), None, None, None, None, cout, cin, taps, 1, accumulate, ops._stream())
        torch.cuda.synchronize()
        return gw, dot

    new, dot_new = run(0)
    old, dot_old = run(NO_TILED)
    assert torch.equal(new, old), f"tiled finalize differs: max {float((new - old).abs().max()):.3e}"
    assert not bool(dot_new.any()) and not bool(dot_old.any()), "dot is not zeroed behind the finalize"
    # which kernel ran: under the dispatch probe the tiled kernel writes nothing, the one-thread-per-element kernel does not know it
    assert torch.equal(run(PROBE)[0], gw0), "the default path did not launch the tiled finalize"
    assert torch.equal(run(PROBE | NO_TILED)[0], old), "the switch did not reach the one-thread-per-element finalize"
    # against the expression itself in float64 (a wrong permutation of v would be equal in both kernels only by accident, but the
    # old kernel is the yardstick; this pins both): 2 * groups roundings of terms of size |coef v|
    coef = (-dot0.double() * inv_sigma.double() ** 2)[:, None] * u.view(groups, cout).double()
    vp = v.view(groups, cin, taps).double().permute(0, 2, 1).reshape(groups, taps * cin)  # (ci, t) -> (t, ci)
    terms = coef[:, :, None] * vp[:, None, :]
    ref = g.double().view(cout, -1) + terms.sum(0) + (gw0.double().view(cout, -1) if accumulate else 0.0)
    mag = g.double().abs().view(cout, -1) + terms.abs().sum(0) + gw0.double().abs().view(cout, -1)
    assert bool(((new.double().view(cout, -1) - ref).abs() <= (groups + 4) * 2 * U * mag).all())
    # u == NULL: the plain accumulate, one add (or a copy)
    for flag in (0, NO_TILED, PROBE):
        plain, _ = run(flag, with_uv=False)
        assert torch.equal(plain, gw0 + g if accumulate else g)
