"""The advection baseline on the GPU: dgmr_block_match and dgmr_advect (csrc/advect.hip) against the float64 specifications of
advection.py on the same arrays, the nowcaster end to end against its CPU path, and its forecasts in the three verifiers.  No test
has a time threshold."""
import json
import os

import numpy as np
import pytest
import torch

import advection_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/advection_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "advection_accuracy.json")
ADVECT_C = 22  # rounded fp32 operations per step in dgmr_advect's position arithmetic, both axes (include/dgmr_hip.h, csrc/advect.hip)


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _match(prev, nxt, *args, **kw):
    from skillful_nowcasting_amd.advection import block_match

    res = block_match(torch.from_numpy(np.array(prev)).cuda(), torch.from_numpy(np.array(nxt)).cuda(), *args, **kw)
    torch.cuda.synchronize()
    return res


@pytest.mark.parametrize("name", sorted(R.MATCH_CASES))
def test_block_match_against_the_reference(name):
    """wet exact; dry blocks as specified; with eps = 2 (block^2 + 2) 2^-24: exactly the reference's displacement wherever its
    second-best cost exceeds the minimum by more than eps min + eps (at least 90 % of the non-dry blocks), everywhere a choice whose
    reference cost is <= min (1 + eps) + eps, and every finite cost within eps relative of the reference's cost at the device's
    displacement and its neighbours."""
    _h, _w, block, stride, radius = R.MATCH_CASES[name][:5]
    eps = R.match_eps(block)
    prev, nxt = R.match_case(name)
    costs, ref = R.match_reference(name)
    got = _match(prev, nxt, block, stride, radius)
    disp, cost, wet = got.disp.cpu().numpy(), got.cost.cpu().numpy().astype(np.float64), got.wet.cpu().numpy()
    assert disp.dtype == np.int32 and wet.dtype == np.int32 and disp.shape == ref.disp.shape and cost.shape == ref.cost.shape
    assert np.array_equal(wet, ref.wet)
    dry = ref.wet < block * block // 16
    assert dry[1].all() and not dry.all()
    assert (disp[dry] == 0).all() and np.isposinf(cost[dry]).all()
    clear = R.clear_minimum(costs, eps) & ~dry
    assert clear.sum() >= 0.9 * (~dry).sum()
    assert np.array_equal(disp[clear], ref.disp[clear])
    assert (np.abs(disp) <= radius).all()
    big = np.full(costs.shape[:3] + (2 * radius + 3, 2 * radius + 3), np.inf)
    big[..., 1:-1, 1:-1] = costs
    ii = np.indices(costs.shape[:3])
    at = np.stack([big[ii[0], ii[1], ii[2], disp[..., 0] + radius + 1 + a, disp[..., 1] + radius + 1 + b]
                   for a, b in ((0, 0), (-1, 0), (1, 0), (0, -1), (0, 1))], axis=-1)  # the reference's costs at the device's choice
    wetb = ~dry
    assert (at[wetb][:, 0] <= ref.cost[wetb][:, 0] * (1.0 + eps) + eps).all()
    finite = np.isfinite(at) & wetb[..., None]
    assert np.array_equal(np.isfinite(cost) & wetb[..., None], finite) and np.isposinf(cost[wetb[..., None] & ~finite]).all()
    rel = np.abs(cost[finite] - at[finite]) / np.where(at[finite] > 0, at[finite], 1.0)
    print(f"{name}: {int(clear.sum())} of {int(wetb.sum())} non-dry blocks with a clear minimum; worst relative cost error "
          f"{rel.max():.3e} (eps {eps:.3e})")
    _log_accuracy("block_match " + name, {"worst_relative_cost_error": float(rel.max()), "eps": eps, "clear_blocks": int(clear.sum()),
                                          "non_dry_blocks": int(wetb.sum())})
    assert (np.abs(cost[finite] - at[finite]) <= eps * at[finite]).all()


def test_block_match_ties_and_repeatability():
    """Integer-valued stripes of period 4: several displacements cost exactly 0, fp32 sums of small integers are exact, so disp and
    cost equal the reference exactly; and two launches give the same bits."""
    from skillful_nowcasting_amd.advection import block_match_reference

    s = R.stripes(48, 80)
    prev = np.stack([s, s])
    nxt = np.stack([s, np.roll(s, 2, axis=1)])
    ref = block_match_reference(prev, nxt, 16, 16, 4, 0.5, 0)
    got = _match(prev, nxt, 16, 16, 4, 0.5, 0)
    assert np.array_equal(got.disp.cpu().numpy(), ref.disp)
    assert np.array_equal(got.cost.cpu().numpy().astype(np.float64), ref.cost)
    assert np.array_equal(got.wet.cpu().numpy(), ref.wet)
    assert (ref.disp[1, :, 1:-1] == np.array([0, -2])).all()
    name = "96x128 32/32/16"
    a = _match(*R.match_case(name), 32, 32, 16)
    b = _match(*R.match_case(name), 32, 32, 16)
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32) if u.dtype == torch.float32 else u, v.view(torch.int32) if v.dtype == torch.float32 else v)


def test_block_match_min_wet_and_strided_planes():
    """min_wet = 0 searches every block (an all-missing one matches at (0, 0) with cost 0); views of one [T, N, H, W] tensor are read
    in place and give what contiguous copies give."""
    from skillful_nowcasting_amd.advection import block_match, block_match_reference

    prev, nxt = R.match_case("48x80 16/16/4")
    ref = block_match_reference(prev, nxt, 16, 16, 4, 0.1, 0)
    got = _match(prev, nxt, 16, 16, 4, 0.1, 0)
    assert np.array_equal(got.wet.cpu().numpy(), ref.wet)
    assert (got.disp[1] == 0).all() and (got.cost[1][..., 0] == 0).all() and torch.isfinite(got.cost[..., 0]).all()
    frames = torch.from_numpy(np.stack([prev, nxt, prev])).cuda()[:, :, :, :]
    wide = torch.zeros(3, 3, 48, 80 + 16, device="cuda")[..., :80]  # rows not contiguous: copied
    wide.copy_(frames)
    for src in (frames, wide):
        r = block_match(src[:-1].reshape(6, 48, 80), src[1:].reshape(6, 48, 80), 16, 16, 4)
        for p, (a, b) in enumerate(((prev, nxt), (nxt, prev))):
            one = _match(a, b, 16, 16, 4)
            assert torch.equal(r.disp[3 * p:3 * p + 3], one.disp) and torch.equal(r.wet[3 * p:3 * p + 3], one.wet)
            assert torch.equal(r.cost[3 * p:3 * p + 3].view(torch.int32), one.cost.view(torch.int32))


# ---- advect ------------------------------------------------------------------------------------------------------------------------
def _source(h, w, n):
    x = np.stack([R.rain_field(5 + i, h, w) for i in range(n)])
    x[:, 3, 5] = np.nan
    x[:, h - 2, w - 3] = -1.0
    return x


def _shifted(x, dy, dx):
    out = np.zeros_like(x)
    h, w = x.shape[-2:]
    if abs(dy) >= h or abs(dx) >= w:
        return out
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[..., yd, xd] = x[..., ys, xs]
    return out


@pytest.mark.parametrize("h,w", [(48, 80), (96, 128), (48, 81)])
@pytest.mark.parametrize("steps", [1, 18])
def test_advect_uniform_integer_field_is_bit_exact(h, w, steps):
    """A uniform integer field, as a 1 x 1 lattice shared by the planes and as a constant 3 x 5 lattice per plane: every lead time is
    the source shifted by t v with zeros shifted in, bit for bit (W = 81 takes the 4-byte-store kernel)."""
    from skillful_nowcasting_amd.advection import advect

    x = _source(h, w, 2)
    clean = np.where(x >= 0, x, 0).astype(np.float32)
    xt = torch.from_numpy(x).cuda()
    v = (2, -3)
    want = np.stack([_shifted(clean, v[0] * t, v[1] * t) for t in range(1, steps + 1)], axis=1)
    uniform = torch.tensor([float(v[0]), float(v[1])], device="cuda").view(1, 1, 1, 2)
    lattice = uniform.expand(2, 3, 5, 2).contiguous()
    for field, origin, spacing in ((uniform, 0.0, 1.0), (lattice, 7.5, 16.0)):
        got = advect(xt, field, steps, origin, spacing)
        torch.cuda.synchronize()
        assert got.shape == (2, steps, h, w) and np.array_equal(got.cpu().numpy(), want)


def _rotating_field(n, gy, gx, h, w, origin, spacing, omega):
    """Per plane a rigid rotation by omega_i radians per step about the frame's centre plus a drift, sampled on the lattice."""
    f = np.empty((n, gy, gx, 2), np.float32)
    py = origin + spacing * np.arange(gy)[:, None]
    px = origin + spacing * np.arange(gx)[None, :]
    for i in range(n):
        om = omega * (1 + i)
        f[i, ..., 0] = om * (px - w / 2) + 0.3 * (i + 1)
        f[i, ..., 1] = -om * (py - h / 2) - 0.7
    return f


@pytest.mark.parametrize("h,w,steps,shared", [(48, 80, 18, False), (96, 128, 18, True), (96, 128, 1, False), (48, 81, 18, False)])
def test_advect_rotating_field_against_the_reference(h, w, steps, shared):
    """A smooth rotating field on a 3 x 5 lattice, written into a [B, T, C, H, W] buffer through the two strides; nothing outside the
    channel is touched.  |device - float64 reference| <= c T max(H, W) 2^-24 max|adjacent difference of x| + 4 * 2^-24 max|x|, c = 22."""
    from skillful_nowcasting_amd.advection import advect, advect_reference

    b, c = 2, 2
    x = _source(h, w, b)
    origin, spacing = 7.5, min((h - 16) / 2.0, (w - 16) / 4.0)
    field = _rotating_field(1 if shared else b, 3, 5, h, w, origin, spacing, 0.004)
    ref = advect_reference(x, field, steps, origin, spacing)
    buf = torch.full((b, steps, c, h, w), -7.0, device="cuda")
    got = advect(torch.from_numpy(x).cuda(), torch.from_numpy(field).cuda(), steps, origin, spacing, out=buf[:, :, 1])
    torch.cuda.synchronize()
    assert got.data_ptr() == buf[:, :, 1].data_ptr() and (buf[:, :, 0] == -7.0).all()
    clean = np.where(x >= 0, x, 0).astype(np.float64)
    adjacent = max(np.abs(np.diff(clean, axis=-1)).max(), np.abs(np.diff(clean, axis=-2)).max())
    bound = ADVECT_C * steps * max(h, w) * 2.0 ** -24 * adjacent + 4 * 2.0 ** -24 * clean.max()
    err = np.abs(buf[:, :, 1].cpu().numpy().astype(np.float64) - ref).max()
    moved = np.abs(ref[:, -1] - clean).max()
    print(f"{h} x {w}, T = {steps}: worst error {err:.3e}, bound {bound:.3e} (ratio {err / bound:.3e}); the field moved the frame by {moved:.2f}")
    _log_accuracy(f"advect {h}x{w} T={steps} {'shared' if shared else 'per-plane'} field",
                  {"worst_abs_error": float(err), "bound": float(bound), "error_over_bound": float(err / bound), "c": ADVECT_C})
    assert moved > 0.1  # the case does something
    assert err <= bound


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translating():
    seq = R.translating_sequence(5, 128, 160, 10, (2, -3))
    return seq, torch.from_numpy(seq[:4])[..., None], torch.from_numpy(seq[4:])[:, None]


def test_nowcast_on_the_device_equals_the_cpu_path(translating):
    """The same nowcast through the kernels and through the references: the motion field within what an eps-relative cost error does
    to the sub-pixel parabola, the forecast within advect's bound plus that field difference times the adjacent difference."""
    from skillful_nowcasting_amd.advection import AdvectionNowcaster

    seq, frames, _ = translating
    cpu, dev = AdvectionNowcaster(forecast_steps=6), AdvectionNowcaster(forecast_steps=6)
    want = cpu.nowcast(frames).numpy().astype(np.float64)
    got = dev.nowcast(frames.cuda())
    torch.cuda.synchronize()
    assert got.is_cuda and tuple(got.shape) == (1, 6, 1, 128, 160) and dev.last_field.is_cuda
    field_gap = (dev.last_field.cpu() - cpu.last_field).abs().max().item()
    # the costs agree to eps relative; the parabola's offset is a ratio of cost differences of the costs' own size (the minimum is 0
    # here, its neighbours are not): 8 eps bounds the offset's change generously, the box smoothing only averages it
    eps = R.match_eps(32)
    assert field_gap <= 8 * eps, field_gap
    clean = np.pad(seq[3].astype(np.float64), 1)  # with the zeros outside: the field difference also moves the frame's edge
    adjacent = max(np.abs(np.diff(clean, axis=-1)).max(), np.abs(np.diff(clean, axis=-2)).max())
    bound = (ADVECT_C * 6 * 160 * 2.0 ** -24 + 2 * 6 * field_gap) * adjacent + 4 * 2.0 ** -24 * clean.max() + 2.0 ** -24 * clean.max()
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).max()
    print(f"device against CPU nowcast: field gap {field_gap:.3e} px, worst error {err:.3e}, bound {bound:.3e}")
    _log_accuracy("nowcast 128x160 T=6", {"field_gap_px": field_gap, "worst_abs_error": float(err), "bound": float(bound)})
    assert err <= bound


def test_nowcast_beats_persistence_in_the_verifiers(translating):
    from skillful_nowcasting_amd.advection import AdvectionNowcaster, persistence_nowcast
    from skillful_nowcasting_amd.spectra import SpectrumVerifier
    from skillful_nowcasting_amd.value import ValueVerifier
    from skillful_nowcasting_amd.verification import NowcastVerifier, skill_score

    seq, frames, observed = translating
    observed = observed.cuda()
    fc = AdvectionNowcaster(forecast_steps=6).nowcast(frames.cuda())
    pers = persistence_nowcast(torch.from_numpy(seq[3])[None].cuda(), 6)
    assert tuple(pers.shape) == tuple(fc.shape) and pers.stride(1) == 0
    res = []
    for f in (fc, pers):
        ver, spec, val = NowcastVerifier(1, 6), SpectrumVerifier(1, 6, window=32), ValueVerifier(1, 6)
        for v in (ver, spec, val):
            v.update(f, observed)
        res.append((ver.compute(), spec.compute(), val.compute()))
    (adv, adv_spec, adv_val), (per, _per_spec, per_val) = res
    assert (adv["crps"]["avg"][1] < per["crps"]["avg"][1]).all()
    assert (skill_score(adv, per)["crps"]["avg"][1] > 0).all()
    assert np.isfinite(adv_spec["psd_forecast"]).all() and (adv_spec["windows"] == 20).all()
    assert (adv_val["brier"] <= per_val["brier"]).all()
    # the batched entry: [B, T_in, C, H, W] -> [1, B, T, C, H, W]; case 1 of the batch is the single nowcast.  Both fields are one
    # float64 result rounded to fp32, summed in an order that may depend on the number of planes: one fp32 ulp of |v| < 4 apart at
    # most, which moves a lead time's source position by T ulps on each axis; the forecast's own rounding comes on top
    images = torch.from_numpy(np.stack([seq[1:5], seq[:4]]))[:, :, None].cuda()
    batched = AdvectionNowcaster(forecast_steps=6)
    batch = batched.nowcast_batch(images)
    assert tuple(batch.shape) == (1, 2, 6, 1, 128, 160) and tuple(batched.last_field.shape) == (2, 7, 9, 2)
    clean = np.pad(seq[3].astype(np.float64), 1)
    adjacent = max(np.abs(np.diff(clean, axis=-1)).max(), np.abs(np.diff(clean, axis=-2)).max())
    ulp = 2.0 ** -22
    assert (batch[0, 1] - fc[0]).abs().max().item() <= 2 * 6 * ulp * adjacent + 2.0 ** -23 * clean.max()
