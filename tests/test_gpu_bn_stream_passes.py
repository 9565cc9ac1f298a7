"""GPU: BatchNorm's stream passes with several rows in flight per lane, through the C ABI.

dgmr_bn_bwd_apply, dgmr_bn_stats, dgmr_bn_bwd_reduce, dgmr_colsum and the two serial walks behind them (reduce_rows_finish_kernel,
bn_param_grad_kernel) issue the loads of several rows before the arithmetic of the first; every sum keeps its chain and its order, so
the results are the bits of the one-row-in-flight kernels, which dgmr_debug_flags 8192 still launches on their former grids.  Each
default result is compared with that launch bit for bit (torch.equal) and, so that the pair cannot agree on a wrong answer, with the
float64 formula inside a rounding bound.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONE_ROW = 8192  # dgmr_debug_flags: one row in flight per lane, the former grids
ROWS = 2  # rows bn_bwd_apply4_kernel keeps in flight by default (batchnorm.hip: g_bn_rows), for the shapes below only
WGS = 256 * 8  # workgroups of its multi-pass grid (BN_APPLY_WGS)


@pytest.fixture()
def lib():
    """The library with flags 0 and the determinism mode restored behind the test."""
    from skillful_nowcasting_amd._lib import call, load

    lib = load()
    was = lib.dgmr_get_deterministic()
    call("dgmr_debug_flags", 0)
    yield lib
    call("dgmr_debug_flags", 0)
    lib.dgmr_set_deterministic(was)


def _stream():
    from skillful_nowcasting_amd import ops

    return ops._stream()


def _p(t):
    return None if t is None else t.data_ptr()


def _randn(shape, offset):
    """Seeded normal values plus a per-channel offset (the last dimension is the channel)."""
    return torch.randn(shape, device=DEV) + offset


# ------------------------------------------------------------------------------------------------------------------------------
# dgmr_bn_bwd_apply
# ------------------------------------------------------------------------------------------------------------------------------
def _apply_blocks(n4, c, g):
    """grid.x of the default launch (dgmr_bn_bwd_apply, batchnorm.hip)."""
    c4 = c // 4
    m = c4 // math.gcd(c4, 256)
    blocks = max((-(-n4 // (ROWS * 256)) + m - 1) // m * m, m)
    return min(blocks, max(WGS // g // m * m, m))


def _apply_rows(c, g, size):
    """R such that n4 = R * C / 4 is  'below': less than one pass of one workgroup;  'ragged': a few workgroups, not a multiple of
    ROWS x grid stride;  'passes': more than the multi-pass grid covers at once (2048 workgroups: 16 MiB per pass) - three whole
    passes and a ragged fourth at G = 3 (48 MiB per tensor), two and a half at G = 1 (40 MiB)."""
    c4 = c // 4
    if size == "below":
        return max(1, (ROWS * 256 - 37) // c4)
    if size == "ragged":
        r = (5 * ROWS * 256 + 3 * 256 + 77) // c4 + 1
        while r * c4 % (ROWS * 256 * _apply_blocks(r * c4, c, g)) == 0:
            r += 1
        return r
    m = c4 // math.gcd(c4, 256)
    one_pass = max(WGS // g // m * m, m) * 256 * ROWS
    n4 = 3 * one_pass + 1000 if g > 1 else 2 * one_pass + one_pass // 2 + 1000
    return -(-n4 // c4)


def _apply_check(lib, c, r, g, combos):
    from skillful_nowcasting_amd._lib import call

    torch.manual_seed(c * 1000 + g)
    n4 = r * c // 4
    blocks = _apply_blocks(n4, c, g)
    chan = torch.linspace(-1.5, 2.0, c, device=DEV)
    gy, x = _randn((g, r, c), chan), _randn((g, r, c), 0.5 * chan + 0.25)
    assert gy.numel() * 4 < 64 << 20
    mean = _randn((g, c), 0.5 * chan + 0.25) * 0.9
    rstd = torch.rand(g, c, device=DEV) + 0.5
    gamma = torch.rand(c, device=DEV) + 0.5
    sums = (torch.rand(g, 2, c, device=DEV, dtype=torch.float64) + 0.5) * r  # k0 / R and k1 / R in [0.5, 1.5)
    sums[:, :, ::2] *= -1.0
    add = _randn((g, r, c), 0.0)
    dpar0 = torch.randn(2, c, device=DEV)
    st = _stream()

    def run(flag, train, gm, ad):
        call("dgmr_debug_flags", flag)
        dx = torch.full((g, r, c), float("nan"), device=DEV)
        dpar = dpar0.clone()
        call("dgmr_bn_bwd_apply", _p(gy), _p(x), _p(mean), _p(rstd), _p(gm), _p(sums), _p(ad), _p(dx), _p(dpar[1]), _p(dpar[0]), g, r, c,
             train, st)
        torch.cuda.synchronize()
        return dx, dpar

    u24 = 2.0 ** -24
    gd, xh = gy.double(), (x.double() - mean.double()[:, None, :]) * rstd.double()[:, None, :]
    k0, k1 = sums[:, 0, None, :].float().double() / r, sums[:, 1, None, :].float().double() / r
    # dbeta / dgamma: the G doubles added in group order, rounded to float, added to what was there
    spar = sums.sum(0)
    par_bound = g * 2.0 ** -53 * sums.abs().sum(0) + 2 * u24 * (spar.abs() + dpar0.double().abs())
    worst = 0.0
    for train, with_gamma, with_add in combos:
        gm, ad = (gamma if with_gamma else None), (add if with_add else None)
        dx, dpar = run(0, train, gm, ad)
        dx1, dpar1 = run(ONE_ROW, train, gm, ad)
        tag = f"C {c} R {r} G {g} blocks {blocks} train {train} gamma {with_gamma} dx_add {with_add}"
        assert not torch.isnan(dx).any(), tag
        assert torch.equal(dx, dx1), f"{tag}: dx differs from the one-row launch in {int((dx != dx1).sum())} elements"
        assert torch.equal(dpar, dpar1), f"{tag}: dgamma / dbeta differ from the one-row launch"
        scale = (gamma.double() if with_gamma else 1.0) * rstd.double()[:, None, :]
        ref = (gd - k0 - xh * k1 if train else gd) * scale
        mag = (gd.abs() + k0.abs() + (xh * k1).abs() if train else gd.abs()) * scale.abs()
        bound = 8 * u24 * mag
        if with_add:  # one more rounding, of the sum with dx_add
            ref = ref + add.double()
            bound = bound + u24 * ref.abs()
        err = (dx.double() - ref).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max())
        worst = max(worst, ratio)
        assert bool((err <= bound).all()), f"{tag}: err / bound {ratio:.3f} against the float64 formula"
        assert bool(((dpar.double() - (dpar0.double() + spar)).abs() <= par_bound).all()), f"{tag}: dgamma / dbeta against float64"
    print(f"\nbn_bwd_apply C {c} R {r} G {g} ({blocks} x {g} workgroups, {n4 / (blocks * 256 * ROWS):.2f} passes): worst err / bound {worst:.3f}")


ALL_COMBOS = [(t, gm, ad) for t in (1, 0) for gm in (True, False) for ad in (False, True)]


@pytest.mark.parametrize("g", [1, 3])
@pytest.mark.parametrize("size", ["below", "ragged", "passes"])
@pytest.mark.parametrize("c", [4, 48, 96, 768])
def test_bn_bwd_apply_equals_one_row_launch(lib, c, size, g):
    r = _apply_rows(c, g, size)
    n4, stride = r * c // 4, _apply_blocks(r * c // 4, c, g) * 256
    if size == "below":
        assert n4 < ROWS * 256
    else:
        assert n4 % (ROWS * stride) != 0 and (size == "ragged" or n4 > ROWS * stride)
    # the large shapes: training with and without gamma and dx_add, and the plain evaluation launch; the small ones: every combination
    combos = ALL_COMBOS if size != "passes" else [(1, True, False), (1, False, True), (0, True, False)]
    _apply_check(lib, c, r, g, combos)


def test_bn_bwd_apply_many_groups(lib):
    """G = 108 at C = 96: bn_param_grad_kernel's walk over the groups is thirteen unrolled batches and a tail of four; the apply grid
    is 18 x 108 workgroups, four passes and a ragged fifth (63.3 MiB per tensor)."""
    _apply_check(lib, 96, 1600, 108, [(1, True, False)])


def test_bn_bwd_apply_misaligned_takes_scalar_kernel(lib):
    """dx offset by 4 bytes: the scalar kernel, which the switch does not touch."""
    from skillful_nowcasting_amd._lib import call

    c, r, g = 48, 301, 3
    torch.manual_seed(11)
    chan = torch.linspace(-1.5, 2.0, c, device=DEV)
    gy, x = _randn((g, r, c), chan), _randn((g, r, c), chan)
    mean, rstd, gamma = _randn((g, c), chan), torch.rand(g, c, device=DEV) + 0.5, torch.rand(c, device=DEV) + 0.5
    sums = (torch.rand(g, 2, c, device=DEV, dtype=torch.float64) + 0.5) * r
    res = []
    for flag in (0, ONE_ROW):
        call("dgmr_debug_flags", flag)
        buf = torch.full((g * r * c + 1,), float("nan"), device=DEV)
        call("dgmr_bn_bwd_apply", _p(gy), _p(x), _p(mean), _p(rstd), _p(gamma), _p(sums), None, buf.data_ptr() + 4, None, None, g, r, c, 1,
             _stream())
        torch.cuda.synchronize()
        assert bool(torch.isnan(buf[0]))
        res.append(buf[1:].view(g, r, c))
    assert torch.equal(res[0], res[1])
    scale = gamma.double() * rstd.double()[:, None, :]
    xh = (x.double() - mean.double()[:, None, :]) * rstd.double()[:, None, :]
    k0, k1 = sums[:, 0, None, :].float().double() / r, sums[:, 1, None, :].float().double() / r
    ref = (gy.double() - k0 - xh * k1) * scale
    bound = 8 * 2.0 ** -24 * (gy.double().abs() + k0.abs() + (xh * k1).abs()) * scale.abs()
    assert bool(((res[0].double() - ref).abs() <= bound).all())


# ------------------------------------------------------------------------------------------------------------------------------
# dgmr_bn_stats, dgmr_bn_bwd_reduce, dgmr_colsum
# ------------------------------------------------------------------------------------------------------------------------------
def _reductions(lib, c, r, g, det, flag):
    """The three entry points on seeded inputs -> {name: double sums}, and the float64 references with their bounds."""
    from skillful_nowcasting_amd._lib import call

    call("dgmr_debug_flags", flag)
    lib.dgmr_set_deterministic(det)
    torch.manual_seed(c * 100 + r + g)
    chan = torch.linspace(-1.5, 2.0, c, device=DEV)
    x, gy = _randn((g, r, c), chan), _randn((g, r, c), 0.5 - chan)
    mean, rstd = _randn((g, c), chan) * 0.9, torch.rand(g, c, device=DEV) + 0.5
    st = _stream()
    n = g * 2 * c

    def buffer(groups, rows):
        buf = torch.full((int(lib.dgmr_reduce_doubles(groups, rows, c)),), float("nan"), device=DEV, dtype=torch.float64)
        buf[:groups * 2 * c].zero_()
        return buf

    out = {}
    s = buffer(g, r)
    call("dgmr_bn_stats", _p(x), _p(s), g, r, c, st)
    out["bn_stats"] = s[:n].clone().view(g, 2, c)
    s = buffer(g, r)
    call("dgmr_bn_bwd_reduce", _p(gy), _p(x), _p(mean), _p(rstd), _p(s), g, r, c, st)
    out["bn_bwd_reduce"] = s[:n].clone().view(g, 2, c)
    tmp = torch.full((int(lib.dgmr_colsum_tmp_doubles(g * r, c)),), float("nan"), device=DEV, dtype=torch.float64)
    col = torch.zeros(c, device=DEV)
    call("dgmr_colsum", _p(x), _p(col), _p(tmp), g * r, c, 0, st)
    out["colsum"] = tmp[:c].clone()
    out["colsum out"] = col.double()
    torch.cuda.synchronize()

    u53 = 2.0 ** -53
    xd, gd = x.double(), gy.double()
    xh = ((x - mean[:, None, :]) * rstd[:, None, :]).double()  # x-hat is a float in the kernel: the same two float operations
    ref = {"bn_stats": (torch.stack([xd.sum(1), (xd * xd).sum(1)], 1), r * u53 * torch.stack([xd.abs().sum(1), (xd * xd).sum(1)], 1)),
           "bn_bwd_reduce": (torch.stack([gd.sum(1), (gd * xh).sum(1)], 1), r * u53 * torch.stack([gd.abs().sum(1), (gd * xh).abs().sum(1)], 1)),
           "colsum": (xd.sum((0, 1)), g * r * u53 * xd.abs().sum((0, 1)))}
    return out, ref


# 96 leaves 64 threads of a workgroup idle; 300 has a second column block of 44 channels.  Rows: fewer than row lanes; a tail shorter
# than the unroll; several unrolled passes (1000 rows: 16 workgroups' rows behind reduce_rows_finish_kernel - two unrolled batches;
# 700 rows: 11 - a batch and a tail of three)
@pytest.mark.parametrize("c", [4, 48, 96, 300, 768])
def test_reductions_equal_one_row_launch(lib, c):
    cases = [(r, g) for r in (1, 7, 130, 1000) for g in (1, 3)] + [(700, 3)]
    if c == 96:
        cases.append((700, 108))
    worst = 0.0
    for r, g in cases:
        new, ref = _reductions(lib, c, r, g, 1, 0)
        old, _ = _reductions(lib, c, r, g, 1, ONE_ROW)
        atomic, _ = _reductions(lib, c, r, g, 0, 0)
        for name in new:
            assert torch.equal(new[name], old[name]), f"{name} C {c} R {r} G {g}: differs from the one-row launch (deterministic mode)"
        for name, (want, bound) in ref.items():
            for mode, got in (("deterministic", new[name]), ("atomic", atomic[name])):
                err = (got - want).abs()
                assert bool((err <= bound).all()), f"{name} C {c} R {r} G {g} {mode}: err / bound {float((err / bound).max()):.3f}"
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
        # colsum's float output: the double sum rounded once
        assert torch.equal(new["colsum out"], new["colsum"].float().double())
    print(f"\nreductions C {c}: worst err / bound {worst:.3f} against float64 torch.sum")
