"""The advection baseline without a GPU: the numpy specifications (advection.py), motion_field, the nowcaster on the CPU path against
the verifier, skill_score, and the two C entry points' refusals."""
import ctypes

import numpy as np
import pytest
import torch

import advection_recipe as R
from skillful_nowcasting_amd import advection as A
from skillful_nowcasting_amd.verification import NowcastVerifier, skill_score

# (H, W, block, stride, radius, shifts - one plane each, qualifying blocks as a prototype of the specification counted them, blocks per plane)
PLANTED = [(96, 128, 32, 16, 8, [(3, -2)], 23, 35), (96, 128, 32, 16, 8, [(0, 0)], 15, 35),
           (96, 128, 16, 16, 4, [(3, -2), (-3, 3)], 30, 48)]


@pytest.mark.parametrize("h,w,block,stride,radius,shifts,n_qual,n_blocks", PLANTED)
def test_planted_integer_shifts_are_found_exactly(h, w, block, stride, radius, shifts, n_qual, n_blocks):
    canvas = R.rain_canvas(5, h, w)
    prev = np.stack([R.cut(canvas, h, w)] * len(shifts))
    nxt = np.stack([R.cut(canvas, h, w, *d) for d in shifts])
    min_wet = block * block // 16
    res = A.block_match_reference(prev, nxt, block, stride, radius, 0.1, min_wet)
    total = qual_total = 0
    for i, d in enumerate(shifts):
        q = R.qualifying(h, w, block, stride, radius, d) & (res.wet[i] >= min_wet)
        total += q.size
        qual_total += int(q.sum())
        assert (res.disp[i][q] == np.array(d)).all(), (d, res.disp[i][q])
        assert (res.cost[i][q][:, 0] == 0).all()
        assert np.isfinite(res.cost[i][q]).all()
    print(f"{qual_total} of {total} blocks qualify (a prototype of the specification: {n_qual} of {n_blocks})")
    assert total == n_blocks * len(shifts)
    assert qual_total * 3 >= total, (qual_total, total)  # not vacuous


def test_recipe_statistics():
    f = R.rain_field(5, 96, 128)
    assert f.dtype == np.float32 and (f * 32 == np.round(f * 32)).all()
    assert 0.2 < (f > 0).mean() < 0.7 and 4.0 < f.max() < 40.0


def test_tie_rule_on_periodic_stripes():
    h, w = 48, 80
    s = R.stripes(h, w)
    assert s.max() <= 15 and (s == np.round(s)).all()
    prev = nxt = s[None]
    costs = A.block_costs_reference(prev, nxt, 16, 16, 4)
    res = A.block_match_reference(prev, nxt, 16, 16, 4, 0.5, 0, costs=costs)
    assert (costs == 0).sum(axis=(-1, -2)).min() >= 2  # several displacements cost exactly 0 in every block
    assert (res.disp == 0).all() and (res.cost[..., 0] == 0).all()  # ... and "no motion" wins
    # shifted by half a period the zero-cost candidates are dx = -2 and dx = +2 (and +-2 - 4 k): equal dy^2 + dx^2, the smaller dx wins
    nxt2 = np.roll(s, 2, axis=1)[None]
    costs2 = A.block_costs_reference(prev, nxt2, 16, 16, 4)
    res2 = A.block_match_reference(prev, nxt2, 16, 16, 4, 0.5, 0, costs=costs2)
    by, bx = res2.wet.shape[1:]
    inner = np.zeros((by, bx), bool)
    inner[:, 1:-1] = True  # both candidates exist
    assert (costs2[0][inner][:, 4, 2] == 0).all() and (costs2[0][inner][:, 4, 6] == 0).all()
    assert (res2.disp[0][inner] == np.array([0, -2])).all()
    # the general statement: the winner is the first minimum in (dy^2 + dx^2, dy, dx) order
    for c, r in ((costs, res), (costs2, res2)):
        for b in np.ndindex(*r.wet.shape):
            best = min((c[b][dy + 4, dx + 4], dy * dy + dx * dx, dy, dx) for dy in range(-4, 5) for dx in range(-4, 5))
            assert tuple(r.disp[b]) == best[2:]


def test_dry_blocks_missing_planes_and_min_wet():
    h, w = 48, 80
    f = R.rain_field(5, h, w)
    g = R.rain_field(5, h, w, 1, 1)
    g[:16, :16] = 0
    g[2, 3:10] = 1.0  # 7 wet elements: one short of min_wet
    g[16:32, 32:48] = 0
    g[20, 32:40] = 1.0  # 8: just not dry
    missing = np.full((h, w), np.nan, np.float32)
    prev = np.stack([f, missing, f, f])
    nxt = np.stack([g, missing, np.zeros_like(g), np.where(g > 0, g, -1).astype(np.float32)])
    res = A.block_match_reference(prev, nxt, 16, 16, 4, 0.1, 8)
    wet_true = np.stack([[(g[y:y + 16, x:x + 16] >= 0.1).sum() for x in range(0, 80, 16)] for y in range(0, 48, 16)])
    assert (res.wet[0] == wet_true).all() and (res.wet[3] == wet_true).all() and (res.wet[1] == 0).all() and (res.wet[2] == 0).all()
    dry = res.wet < 8
    assert dry[1].all() and dry[2].all() and dry[0, 0, 0] and res.wet[0, 0, 0] == 7 and not dry[0, 1, 2] and res.wet[0, 1, 2] == 8
    assert (res.disp[dry] == 0).all() and np.isinf(res.cost[dry]).all()
    assert np.isfinite(res.cost[~dry][:, 0]).all()
    assert (res.disp[3] == res.disp[0]).all() and (res.cost[3] == res.cost[0]).all()  # negative = missing = 0
    everything = A.block_match_reference(prev, nxt, 16, 16, 4, 0.1, 0)
    assert np.isfinite(everything.cost[..., 0]).all()  # min_wet = 0: no block is dry, an all-missing one matches at (0, 0) with cost 0
    assert (everything.disp[1] == 0).all() and (everything.cost[1][..., 0] == 0).all()
    nothing = A.block_match_reference(prev, nxt, 16, 16, 4, 0.1, 257)
    assert (nothing.disp == 0).all() and np.isinf(nothing.cost).all()


def _shifted(x, dy, dx):
    out = np.zeros_like(x)
    h, w = x.shape
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[yd, xd] = x[ys, xs]
    return out


def test_advect_uniform_integer_field_is_an_exact_shift():
    x = R.rain_field(5, 48, 80)
    x[3, 5] = np.nan
    x[7, 9] = -2.0
    clean = np.where(x >= 0, x, 0).astype(np.float32)
    uniform = np.array([2.0, -3.0], np.float32).reshape(1, 1, 1, 2)
    out = A.advect_reference(x[None], uniform, 4)
    for t in range(4):
        assert (out[0, t] == _shifted(clean, 2 * (t + 1), -3 * (t + 1))).all()
    lattice = np.broadcast_to(uniform, (1, 3, 5, 2))
    assert (A.advect_reference(x[None], lattice, 4, 7.5, 16.0) == out).all()
    assert (A.advect(torch.from_numpy(x[None]), torch.from_numpy(uniform), 4).numpy() == out.astype(np.float32)).all()


def test_advect_half_pixel_field_is_the_two_neighbour_mean():
    x = R.rain_field(5, 48, 80)
    out = A.advect_reference(x[None], np.array([0.0, 0.5], np.float32).reshape(1, 1, 1, 2), 1)[0, 0]
    x64 = x.astype(np.float64)
    want = 0.5 * (x64 + _shifted(x64, 0, 1))
    assert np.abs(out - want).max() <= 2.0 ** -22 * np.abs(want).max()


def test_advect_out_argument_and_strides_on_the_cpu_path():
    x = torch.from_numpy(np.stack([R.rain_field(5, 48, 80), R.rain_field(6, 48, 80)]))
    field = torch.tensor([1.25, -0.5]).view(1, 1, 1, 2)
    want = A.advect(x, field, 3)
    buf = torch.full((2, 3, 2, 48, 80), -7.0)
    got = A.advect(x, field, 3, out=buf[:, :, 1])
    assert got.data_ptr() == buf[:, :, 1].data_ptr() and (buf[:, :, 1] == want).all() and (buf[:, :, 0] == -7.0).all()
    with pytest.raises(ValueError):
        A.advect(x, field, 3, out=torch.empty(2, 3, 48, 81))
    with pytest.raises(ValueError):
        A.advect(x, field, 65)


def test_motion_field_recovers_a_planted_translation():
    seq = R.translating_sequence(5, 128, 160, 4, (2, -3))
    field = A.motion_field(torch.from_numpy(seq)[:, None])
    assert tuple(field.shape) == (1, 7, 9, 2) and field.dtype == torch.float32
    inner = field[0, 1:-1, 1:-1]
    assert (inner - torch.tensor([2.0, -3.0])).abs().max().item() <= 0.05, inner
    # nothing usable: a dry sequence gives a zero field
    assert (A.motion_field(torch.zeros(3, 2, 64, 64)) == 0).all()


@pytest.fixture(scope="module")
def translating_case():
    """4 context + 6 target frames, 128 x 160, moving by (2, -3) per frame; the CPU nowcast, persistence and both verifiers' results."""
    seq = R.translating_sequence(5, 128, 160, 10, (2, -3))
    frames = torch.from_numpy(seq[:4])[..., None]          # [T_in, H, W, C]
    observed = torch.from_numpy(seq[4:])[:, None]          # [T, C, H, W]
    nowcaster = A.AdvectionNowcaster(forecast_steps=6)
    fc = nowcaster.nowcast(frames)
    pers = A.persistence_nowcast(torch.from_numpy(seq[3])[None], 6)
    res = []
    for f in (fc, pers):
        ver = NowcastVerifier(1, 6)
        ver.update(f, observed)
        res.append(ver.compute())
    return seq, nowcaster, fc, pers, res


def test_nowcaster_beats_persistence_on_a_translating_sequence(translating_case):
    seq, nowcaster, fc, pers, (adv, per) = translating_case
    assert tuple(fc.shape) == (1, 6, 1, 128, 160) and fc.dtype == torch.float32
    assert tuple(pers.shape) == (1, 6, 1, 128, 160) and pers.stride(1) == 0  # a view
    assert tuple(nowcaster.last_field.shape) == (1, 7, 9, 2)
    print("grid-scale CRPS, advection:", adv["crps"]["avg"][1], "persistence:", per["crps"]["avg"][1])
    assert (adv["crps"]["avg"][1] < per["crps"]["avg"][1]).all()
    skill = skill_score(adv, per)
    assert (skill["crps"]["avg"][1] > 0).all() and set(skill["crps"]) == {"avg", "max"} and set(skill["crps"]["avg"]) == {1, 4, 16}
    for t in skill["csi"]:
        assert np.allclose(skill["csi"][t], adv["csi"][t] - per["csi"][t], equal_nan=True)
    same = skill_score(adv, adv)
    assert all((v == 0).all() for v in same["crps"]["avg"].values())


def test_nowcast_batch_matches_nowcast_and_missing_rules(translating_case):
    seq = translating_case[0]
    images = torch.from_numpy(np.stack([seq[:4], seq[1:5]]))[:, :, None]  # [B, T_in, C, H, W]
    nowcaster = A.AdvectionNowcaster(forecast_steps=3)
    out = nowcaster.nowcast_batch(images)
    assert tuple(out.shape) == (1, 2, 3, 1, 128, 160)
    one = nowcaster.nowcast(torch.from_numpy(seq[1:5])[..., None])
    assert (out[0, 1] == one[0]).all()
    raw = (seq[:4] * 32).astype(np.int16)
    raw[:, 5, 7] = -1
    scaled = A.AdvectionNowcaster(forecast_steps=3).nowcast(raw[..., None], scale=1 / 32)
    assert torch.isfinite(scaled).all() and (scaled >= 0).all()
    pers = A.persistence_nowcast(torch.tensor([[[1.0, -1.0], [float("nan"), 2.0]]]), 2)
    assert pers[0, 1, 0].tolist() == [[1.0, 0.0], [0.0, 2.0]]
    assert tuple(A.persistence_nowcast(torch.zeros(2, 1, 4, 4), 5).shape) == (1, 2, 5, 1, 4, 4)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_symbols_are_exported_and_the_abi_version_stays(lib):
    assert hasattr(lib, "dgmr_block_match") and hasattr(lib, "dgmr_advect")
    assert lib.dgmr_abi_version() == 13


def test_refusals_without_a_gpu(lib):
    buf = (ctypes.c_float * 16)()
    ibuf = (ctypes.c_int32 * 16)()

    def bm(prev=buf, nxt=buf, n=1, h=64, w=64, block=32, stride=16, radius=8, min_wet=0, disp=ibuf, cost=buf, wet=ibuf):
        return lib.dgmr_block_match(prev, nxt, h * w, n, h, w, block, stride, radius, 0.1, min_wet, disp, cost, wet, None)

    for kwargs, word in [(dict(prev=None), b"null pointer"), (dict(wet=None), b"null pointer"), (dict(block=24), b"block=24"),
                         (dict(stride=0), b"stride=0"), (dict(stride=33), b"stride=33"), (dict(radius=0), b"radius=0"),
                         (dict(radius=17), b"radius=17"), (dict(h=31), b"at least block"), (dict(w=16), b"at least block"),
                         (dict(n=0), b"N=0"), (dict(min_wet=-1), b"min_wet=-1")]:
        assert bm(**kwargs) < 0, kwargs
        assert word in lib.dgmr_last_error(), (kwargs, lib.dgmr_last_error())

    def adv(x=buf, field=buf, n=1, h=8, w=8, gy=1, gx=1, spacing=1.0, t=1, out=buf):
        return lib.dgmr_advect(x, h * w, field, 0, n, h, w, gy, gx, 0.0, spacing, t, out, t * h * w, h * w, None)

    for kwargs, word in [(dict(x=None), b"null pointer"), (dict(out=None), b"null pointer"), (dict(t=0), b"T=0"), (dict(t=65), b"T=65"),
                         (dict(spacing=0.0), b"spacing"), (dict(spacing=float("nan")), b"spacing"), (dict(gy=0), b"lattice"),
                         (dict(gx=0), b"lattice"), (dict(n=0), b"N=0"), (dict(h=0), b"plane")]:
        assert adv(**kwargs) < 0, kwargs
        assert word in lib.dgmr_last_error(), (kwargs, lib.dgmr_last_error())


@pytest.mark.parametrize("name", sorted(R.MATCH_CASES))
def test_gpu_cases_have_clear_minima_in_the_reference(name):
    """The premise of tests/test_gpu_advection.py, checked on the reference alone: in at least 90 % of the non-dry blocks the
    second-best cost exceeds the minimum by more than eps min + eps, so the device must find exactly the reference's displacement."""
    block = R.MATCH_CASES[name][2]
    costs, ref = R.match_reference(name)
    wet_blocks = ref.wet >= block * block // 16
    clear = R.clear_minimum(costs, R.match_eps(block)) & wet_blocks
    print(f"{name}: {int(clear.sum())} of {int(wet_blocks.sum())} non-dry blocks have a clear minimum")
    assert wet_blocks[0].any() and wet_blocks[2].any() and not wet_blocks[1].any()
    assert clear.sum() >= 0.9 * wet_blocks.sum()
