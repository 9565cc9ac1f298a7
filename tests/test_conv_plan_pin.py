"""dgmr_conv_args.plan_n / dgmr_conv_plan (ABI 12): a conv launched on half of a batch gets the kernel the whole batch gets.

CPU only: dgmr_conv_plan is host arithmetic (nothing is launched, no pointer is read).  The generator pass runs the discriminator as
two launch sets, the real and the generated sequences of every call (Discriminator.forward_split); each conv of either half passes
plan_n = the joint batch, and must then be dispatched exactly as the joint launch: same kernel class, tile, window plan and split-K
factor, hence the same summation order for every output element.  Checked here for every conv the two discriminators launch at the
paper configuration (256 x 256 frames, 4 + 18 frames per sequence), forward and data gradient, B in {16, 2}, K in {6, 1}, in the
arithmetic modes f32 (0), bf16x3 (1) and bf16 (2).  The argument sets mirror ops.ConvFn's launches (ops._launch_conv): which pointers
are given decides the dispatch, their values do not.
"""
import ctypes

import pytest

PTR = 0x10000  # any 16-byte aligned non-null address: never dereferenced by the query
T_SEQ, FRAMES_SPATIAL = 22, 8


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    lib = _lib.load()
    yield lib
    lib.dgmr_set_precision(0)


def _args(n, groups, d, h, w, cin, cout, k3d, k, *, prec, bias=False, split_c=None, residual=False, mask=False, pre_relu=False, pool2=False):
    from skillful_nowcasting_amd._core import SPLITK_WS_BYTES
    from skillful_nowcasting_amd._lib import ConvArgs

    a = ConvArgs()
    a.x = a.w = a.y = a.scale = PTR
    a.bias = PTR if bias else None
    a.residual = PTR if residual else None
    a.mask_src = PTR if mask else None
    a.splitk_ws, a.splitk_ws_bytes = PTR, SPLITK_WS_BYTES
    # ops._split_planes: bf16 planes exist in the bf16 modes for 1x1 / 3x3 weights whose contraction channels are a multiple of 8
    a.w_split = PTR if (prec != 0 and split_c % 8 == 0) else None
    a.N, a.D, a.H, a.W, a.Cin, a.Cout = n, d, h, w, cin, cout
    a.KD, a.KH, a.KW = (k if k3d else 1), k, k
    a.pre_relu = int(pre_relu)
    a.scale_group = n // groups
    a.pre_group = a.mask_group = 1
    if pool2:
        a.pool2, a.w_phase = 1, PTR
    return a


def _dblock(name, n, groups, d, h, w, cin, cout, is3d, first_relu, keep, prec, lib):
    """(name, ConvArgs) of every conv launch of one DBlock on a batch of n samples in `groups` spectral-norm calls: common.DBlock's
    forward (ops.ConvFn.forward / _forward_pooled) and its data gradients (ops._conv_data_grad)."""
    out = []
    dp, hp, wp = (d // 2 if is3d else d), h // 2, w // 2
    if cin != cout:
        dd, hh, ww = (d, h, w) if keep else (dp, hp, wp)  # the shortcut's 1x1 conv runs on the pooled map
        out.append((f"{name}.conv_1x1 fwd", _args(n, groups, dd, hh, ww, cin, cout, is3d, 1, prec=prec, bias=True, split_c=cin)))
        out.append((f"{name}.conv_1x1 dgrad", _args(n, groups, dd, hh, ww, cout, cin, is3d, 1, prec=prec, split_c=cout)))
    out.append((f"{name}.first fwd", _args(n, groups, d, h, w, cin, cout, is3d, 3, prec=prec, bias=True, split_c=cin, pre_relu=first_relu)))
    out.append((f"{name}.first dgrad", _args(n, groups, d, h, w, cout, cin, is3d, 3, prec=prec, split_c=cout, mask=first_relu)))
    if keep:
        out.append((f"{name}.last fwd", _args(n, groups, d, h, w, cout, cout, is3d, 3, prec=prec, bias=True, split_c=cout, pre_relu=True, residual=True)))
    else:
        pooled = None
        if prec != 0 and cout % 8 == 0 and h % 2 == 0 and w % 2 == 0:  # ops._pool2_fwd_planes
            pooled = _args(n, groups, d, h, w, cout, cout, is3d, 3, prec=prec, bias=True, split_c=cout, pre_relu=True, residual=not is3d, pool2=True)
            if not lib.dgmr_conv_pool2_supported(ctypes.byref(pooled)):
                pooled = None
        out.append((f"{name}.last fwd", pooled if pooled is not None else
                    _args(n, groups, d, h, w, cout, cout, is3d, 3, prec=prec, bias=True, split_c=cout, pre_relu=True)))
    out.append((f"{name}.last dgrad", _args(n, groups, d, h, w, cout, cout, is3d, 3, prec=prec, split_c=cout, mask=True)))
    return out


def _discriminator_launches(b, k, prec, lib):
    """Every conv launch of Discriminator.forward(x, calls=k) on the joint batch x = [k][real b | generated b] and of its backward."""
    n = 2 * k * b
    out = []
    # temporal: AvgPool + space-to-depth -> [n, 4, 22, 64, 64]; two 3-D blocks, then the remaining frames as a frame-major batch
    out += _dblock("t.d1", n, k, T_SEQ, 64, 64, 4, 48, True, False, False, prec, lib)
    out += _dblock("t.d2", n, k, T_SEQ // 2, 32, 32, 48, 96, True, True, False, prec, lib)
    frames = T_SEQ // 4
    c, s = 96, 16
    for i in range(3):
        out += _dblock(f"t.mid{i}", frames * n, frames * k, 1, s, s, c, 2 * c, False, True, False, prec, lib)
        c, s = 2 * c, s // 2
    out += _dblock("t.d_last", frames * n, frames * k, 1, s, s, c, c, False, True, True, prec, lib)
    # spatial: 8 drawn frames per call, frame-major
    frames = FRAMES_SPATIAL
    out += _dblock("s.d1", frames * n, frames * k, 1, 64, 64, 4, 48, False, False, False, prec, lib)
    c, s = 48, 32
    for i in range(4):
        out += _dblock(f"s.mid{i}", frames * n, frames * k, 1, s, s, c, 2 * c, False, True, False, prec, lib)
        c, s = 2 * c, s // 2
    out += _dblock("s.d6", frames * n, frames * k, 1, s, s, c, c, False, True, True, prec, lib)
    return out


def _plan(lib, a, n, plan_n, may_fail=False):
    from skillful_nowcasting_amd._lib import ConvArgs

    q = ConvArgs()
    ctypes.memmove(ctypes.byref(q), ctypes.byref(a), ctypes.sizeof(ConvArgs))
    groups = a.N // a.scale_group
    q.N, q.scale_group, q.plan_n = n, n // groups, plan_n
    detail, ksplit = ctypes.c_uint32(0), ctypes.c_int32(0)
    rc = lib.dgmr_conv_plan(ctypes.byref(q), ctypes.byref(detail), ctypes.byref(ksplit))
    if may_fail and rc != 0:  # (pool2 arguments on a batch too small for the window kernel: ops would launch conv + pooling instead)
        return None
    assert rc == 0, lib.dgmr_last_error()
    return detail.value, ksplit.value


def test_half_batch_launches_keep_the_joint_plan(lib):
    moved = []  # geometries where the pin does something: the unpinned half would get another kernel
    checked = 0
    for prec in (0, 1, 2):
        assert lib.dgmr_set_precision(prec) == 0
        for b in (16, 2):
            for k in (6, 1):
                for name, a in _discriminator_launches(b, k, prec, lib):
                    n = a.N
                    joint = _plan(lib, a, n, 0)
                    assert _plan(lib, a, n // 2, n) == joint, (prec, b, k, name, joint, _plan(lib, a, n // 2, n))
                    assert _plan(lib, a, n, n) == joint, (prec, b, k, name)
                    if _plan(lib, a, n // 2, 0, may_fail=True) != joint:
                        moved.append((prec, b, k, name))
                    checked += 1
    assert checked == 3 * 4 * 68, checked  # 12 blocks: 10 with a shortcut conv (6 launches each), 2 without (4)
    assert moved, "no discriminator conv changes its plan with the batch: the pin is not exercised"
    # the paper batch itself (B = 16, K = 6) has such layers in the benchmark's arithmetic (bf16x3)
    assert any(m[:3] == (1, 16, 6) for m in moved), moved


def test_pin_refuses_what_the_half_cannot_run(lib):
    """A structural requirement that holds for plan_n and fails for N is an argument error that names it: two-image tiles of 8x8
    maps need an even number of samples per spectral-norm call, which a half of an odd-B joint batch does not have."""
    from skillful_nowcasting_amd._lib import ConvArgs

    assert lib.dgmr_set_precision(1) == 0
    k, b, frames = 6, 1, 8
    n = frames * 2 * k * b
    a = _args(n, frames * k, 1, 8, 8, 192, 384, False, 3, prec=1, bias=True, split_c=192, pre_relu=True)
    detail, ksplit = ctypes.c_uint32(0), ctypes.c_int32(0)
    assert lib.dgmr_conv_plan(ctypes.byref(a), ctypes.byref(detail), ctypes.byref(ksplit)) == 0
    a.N, a.scale_group, a.plan_n = n // 2, 1, n
    assert lib.dgmr_conv_plan(ctypes.byref(a), ctypes.byref(detail), ctypes.byref(ksplit)) < 0
    msg = lib.dgmr_last_error()
    assert b"plan_n" in msg and b"even" in msg, msg
    # the launch entry refuses the same arguments (validation precedes the launch: no GPU needed)
    assert lib.dgmr_conv_fwd(ctypes.byref(a), None) < 0 and b"even" in lib.dgmr_last_error()
    # plan_n must be a whole number of launches
    a = _args(6, 1, 1, 16, 16, 96, 96, False, 3, prec=1, split_c=96)
    a.plan_n = 8
    assert lib.dgmr_conv_plan(ctypes.byref(a), ctypes.byref(detail), ctypes.byref(ksplit)) < 0
    assert b"multiple of N" in lib.dgmr_last_error()
    assert lib.dgmr_conv_plan(ctypes.byref(ConvArgs()), None, None) < 0
