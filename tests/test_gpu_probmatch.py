"""Probability matching on the GPU: dgmr_probability_match (csrc/probmatch.hip) against the fp32 specification of stochastic.py on
the same arrays, bit for bit (integer counts, singly rounded fp32 operations: there is no tolerance), and the nowcaster with the
matching and the mask switched on.  No test has a time threshold."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import probmatch_recipe as PR
import stochastic_recipe as R
from conftest import BAND_LOG

pytestmark = pytest.mark.gpu

# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/probmatch_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "probmatch_accuracy.json")
SENTINEL = -77.0


def _log_accuracy(key, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[key] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _dev(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _match(z, target, mask=None, **kw):
    from skillful_nowcasting_amd.stochastic import probability_match

    out = probability_match(z if torch.is_tensor(z) else _dev(z), target if torch.is_tensor(target) else _dev(target),
                            mask if torch.is_tensor(mask) else _dev(mask), **kw)
    torch.cuda.synchronize()
    return out


def _same_bits(got, ref):
    return np.array_equal(PR.bits(got.cpu().numpy()), PR.bits(ref))


@pytest.mark.parametrize("masked", [0, 1, 2], ids=["no mask", "one mask plane", "a mask per lead time"])
@pytest.mark.parametrize("name", sorted(PR.DEVICE_CASES))
def test_bits_against_the_reference(name, masked):
    """Gaussian dB values with runs of exact zeros, NaN, infinities and values beyond both ends; without a mask, with a mask of step
    stride 0 and with one plane per lead time.  The same call through views - z a slice over T of a larger buffer, out another, and
    then in place - gives the same bits and leaves the buffers' other planes alone; two calls give the same bits."""
    p, m, steps, h, w = PR.DEVICE_CASES[name]
    z, target, mask, ref = PR.device_case(name, masked)
    got = _match(z, target, mask)
    assert got.dtype == torch.float32 and tuple(got.shape) == z.shape and _same_bits(got, ref)
    assert torch.equal(PR.bits(_match(z, target, mask)), PR.bits(got))
    src = torch.full((p, m, steps + 2, h, w), SENTINEL, device="cuda")
    dst = torch.full((p, m, steps + 3, h, w), SENTINEL, device="cuda")
    src[:, :, 1:-1].copy_(_dev(z))
    out = _match(src[:, :, 1:-1], target, mask, out=dst[:, :, 2:-1])
    assert out.data_ptr() == dst[:, :, 2:-1].data_ptr() and _same_bits(dst[:, :, 2:-1], ref)
    assert (dst[:, :, :2] == SENTINEL).all() and (dst[:, :, -1] == SENTINEL).all()
    assert torch.equal(PR.bits(src[:, :, 1:-1]), PR.bits(_dev(z)))  # the input is only read
    _match(src[:, :, 1:-1], target, mask, out=src[:, :, 1:-1])  # in place
    assert _same_bits(src[:, :, 1:-1], ref) and (src[:, :, 0] == SENTINEL).all() and (src[:, :, -1] == SENTINEL).all()


@pytest.mark.parametrize("masked", [0, 2])
def test_four_byte_path_through_an_unaligned_view(masked):
    """32 x 36 planes that start one float past a 16-byte boundary (and a mask one byte past a 4-byte one): 4-byte loads and stores,
    the same bits as the reference and as the aligned call."""
    from skillful_nowcasting_amd.stochastic import probability_match_reference

    p, m, steps, h, w = 1, 2, 3, 32, 36
    z, target = PR.device_input(p, m, steps, h, w, seed=9)
    mask = PR.blob_mask(p, steps, h, w) if masked else None
    ref = probability_match_reference(z, np.sort(target.reshape(p, -1), axis=1), mask)
    n = z.size
    flat_z, flat_o = torch.full((n + 1,), SENTINEL, device="cuda"), torch.full((n + 1,), SENTINEL, device="cuda")
    flat_z[1:].copy_(_dev(z).reshape(-1))
    zv, ov = flat_z[1:].view(z.shape), flat_o[1:].view(z.shape)
    assert zv.data_ptr() % 16 == 4 and ov.data_ptr() % 16 == 4
    mv = None
    if masked:
        flat_m = torch.zeros(mask.size + 1, dtype=torch.uint8, device="cuda")
        flat_m[1:].copy_(_dev(mask).reshape(-1))
        mv = flat_m[1:].view(mask.shape)
        assert mv.data_ptr() % 4 == 1
    _match(zv, target, mv, out=ov)
    assert _same_bits(ov, ref) and flat_o[0] == SENTINEL
    assert torch.equal(PR.bits(_match(z, target, mask)), PR.bits(ov))  # the 16-byte path on the same values
    _match(zv, target, mv, out=zv)
    assert _same_bits(zv, ref) and flat_z[0] == SENTINEL


def test_half_exact_zeros_and_inputs_beyond_the_range():
    """Half of the plane exact zeros, scattered (the bin that a wave's lanes pile onto); planes entirely below and entirely above the
    range; a constant plane.  256 x 320: several workgroups per plane."""
    from skillful_nowcasting_amd.stochastic import probability_match_reference

    h, w = 256, 320
    rng = np.random.Generator(np.random.PCG64([5, 29]))
    z = (rng.standard_normal((1, 1, 5, h, w)) * 10.0).astype(np.float32)
    z[0, 0, 0][rng.random((h, w)) < 0.5] = 0.0
    z[0, 0, 1] = -100.0 - np.abs(z[0, 0, 1])
    z[0, 0, 2] = 64.0 + np.abs(z[0, 0, 2])
    z[0, 0, 3] = 7.3
    z[0, 0, 4][rng.random((h, w)) < 0.5] = -0.0
    target = R.db_field(1, h, w, seed=4)
    ts = np.sort(target.reshape(1, -1), axis=1)
    ref = probability_match_reference(z, ts)
    got = _match(z, target)
    assert _same_bits(got, ref)
    assert (got[0, 0, 1] == float(ts[0, 0])).all() and (got[0, 0, 2] == float(ts[0, 0])).all()  # one bin, f = 0: its first rank
    assert torch.unique(got[0, 0, 3]).numel() == 1
    # other bins: lo and scale reach the kernel
    assert _same_bits(_match(z, target, lo=-16.0, scale=128.0), probability_match_reference(z, ts, lo=-16.0, scale=128.0))
    assert _same_bits(_match(z, target, lo=0.0, scale=0.25), probability_match_reference(z, ts, lo=0.0, scale=0.25))


def test_targets_of_few_values_and_of_values_whose_bits_differ():
    """A bin whose ranks all read one target value takes it without the gather: an all-dry target, a target of three values, and -
    where equal values do not mean equal bits - targets with -0.0 and 0.0 mixed and with NaNs of two payloads; the reference runs
    on the very array the device sorted."""
    from skillful_nowcasting_amd.stochastic import probability_match_reference

    p, m, steps, h, w = 2, 2, 2, 32, 48
    z, _ = PR.device_input(p, m, steps, h, w, seed=13)
    rng = np.random.Generator(np.random.PCG64([6, 31]))
    three = rng.choice(np.array([0.0, 7.25, 30.0], np.float32), size=(p, h, w), p=[0.7, 0.2, 0.1])
    signed = np.where(rng.random((p, h, w)) < 0.5, np.float32(-0.0), three).astype(np.float32)
    nans = three.copy()
    nans.view(np.int32)[rng.random((p, h, w)) < 0.2] = 0x7fc00000
    nans.view(np.int32)[rng.random((p, h, w)) < 0.2] = 0x7fc00001
    nans[1] = three[1]  # a case without any beside one with
    for name, target in (("dry", np.zeros((p, h, w), np.float32)), ("three values", three), ("signed zeros", signed), ("NaNs", nans)):
        t = _dev(target)
        ts = torch.sort(t.reshape(p, -1), dim=1).values.cpu().numpy()
        assert np.array_equal(PR.bits(ts), PR.bits(torch.sort(t.reshape(p, -1), dim=1).values.cpu().numpy()))
        got = _match(z, t)
        assert _same_bits(got, probability_match_reference(z, ts)), name
        mask = PR.blob_mask(p, steps, h, w)
        assert _same_bits(_match(z, t, mask), probability_match_reference(z, ts, mask)), name
    assert not _match(z, np.zeros((p, h, w), np.float32)).any()


def test_a_refused_call_leaves_out_untouched():
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.stochastic import probability_match

    lib = _lib.load()
    p, m, steps, h, w = 1, 2, 3, 32, 48
    n = h * w
    z = torch.zeros(p, m, steps, h, w, device="cuda")
    target = torch.zeros(p, n, device="cuda")
    mask = torch.ones(p, steps, h, w, dtype=torch.uint8, device="cuda")
    out = torch.full((p, m, steps, h, w), SENTINEL, device="cuda")
    need = lib.dgmr_probability_match_workspace(p, m, steps)
    ws = torch.full((need,), 7, dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    base = dict(z=z.data_ptr(), ms=steps * n, ss=n, t=target.data_ptr(), ts=n, mk=None, mps=0, mss=0, P=p, M=m, T=steps, H=h, W=w, lo=-64.0,
                scale=32.0, ws=ws.data_ptr(), wsb=need, o=out.data_ptr(), oms=steps * n, oss=n)

    def raw(**kw):
        a = dict(base, **kw)
        return lib.dgmr_probability_match(a["z"], a["ms"], a["ss"], a["t"], a["ts"], a["mk"], a["mps"], a["mss"], a["P"], a["M"], a["T"],
                                          a["H"], a["W"], a["lo"], a["scale"], a["ws"], a["wsb"], a["o"], a["oms"], a["oss"], st)

    for kw in ({"z": None}, {"t": None}, {"ws": None}, {"o": None}, {"scale": 3.0}, {"scale": 0.0}, {"H": 4097, "W": 4096}, {"ms": n - 1},
               {"ss": n - 4}, {"oms": n - 1}, {"oss": n - 4}, {"ts": n - 1}, {"mk": mask.data_ptr(), "mps": n - 1},
               {"mk": mask.data_ptr(), "mps": steps * n, "mss": 4}, {"T": 0}, {"T": 65}, {"wsb": need - 1}):
        assert raw(**kw) < 0 and b"dgmr_probability_match" in lib.dgmr_last_error(), kw
    for bad in (dict(scale=3.0), dict(lo=float("inf")), dict(mask=mask[:, :2])):
        with pytest.raises(ValueError):
            probability_match(z, target.view(p, h, w), out=out, **bad)
    with pytest.raises(ValueError):
        probability_match(z, target.view(p, h, w), out=out.transpose(3, 4))
    torch.cuda.synchronize()
    assert (out == SENTINEL).all() and (ws == 7).all()
    assert raw() == 0  # and the same arguments, unchanged, are accepted
    torch.cuda.synchronize()
    assert (out == 0).all()


# ---- the nowcaster -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def translating():
    seq = R.translating_db_context()  # [5, 128, 128]
    return seq, torch.from_numpy(seq[:4])[..., None], torch.from_numpy(seq[4:])[:, None]


def test_nowcast_with_matching(translating):
    """128 x 128, M = 4, T = 2, window 64, the same white field with and without matching and with a mask.  Before the advection every
    member's exceedance counts at 5 / 15 / 21 / 25 dB are the last frame's within the bin bound of the host tests; the nowcaster's
    result is the hand-made chain spectral_ar -> probability_match -> advect_series -> from_db bit for bit; the first lead time's wet-area
    ratio is closer to the verifying observation's than the unmatched nowcast's; the members go through the three verifiers.  Wet-area
    ratios and CSI at 1 and 4 mm/h are recorded, not asserted."""
    from skillful_nowcasting_amd.advection import advect_series, lattice_geometry
    from skillful_nowcasting_amd.spectra import SpectrumVerifier
    from skillful_nowcasting_amd.stochastic import (EnsembleAdvectionNowcaster, from_db, precipitation_mask, probability_match, spectral_ar,
                                                    to_db)
    from skillful_nowcasting_amd.value import ValueVerifier
    from skillful_nowcasting_amd.verification import NowcastVerifier

    seq, frames, _ = translating
    m, steps, window, size = 4, 2, 64, 128
    kw = dict(forecast_steps=steps, window=window)
    white = torch.from_numpy(R.white_field((1, m, steps, size, size), seed=3)).cuda()
    plain_nc = EnsembleAdvectionNowcaster(**kw)
    plain = plain_nc.nowcast(frames.cuda(), m, white=white)
    matched_nc = EnsembleAdvectionNowcaster(**kw, probability_matching=True)
    matched = matched_nc.nowcast(frames.cuda(), m, white=white)
    masked = EnsembleAdvectionNowcaster(**kw, probability_matching=True, mask_radius=2, mask_growth=1.0).nowcast(frames.cuda(), m, white=white)
    torch.cuda.synchronize()
    # the chain by hand
    z0 = to_db(torch.from_numpy(seq[3])[None].cuda())
    z = spectral_ar(z0, white, matched_nc.rho.cuda(), window)
    zm = probability_match(z, z0)
    origin, spacing = lattice_geometry(32, 16)
    by_hand = from_db(advect_series(zm.view(m, steps, size, size), matched_nc.last_field, origin, spacing, field_group=m))
    assert torch.equal(PR.bits(by_hand.view(1, m, steps, size, size).permute(1, 2, 0, 3, 4)), PR.bits(matched))
    zk = probability_match(z, z0, precipitation_mask(z0, 5.0, 2, 1.0, steps))
    by_hand = from_db(advect_series(zk.view(m, steps, size, size), matched_nc.last_field, origin, spacing, field_group=m))
    assert torch.equal(PR.bits(by_hand.view(1, m, steps, size, size).permute(1, 2, 0, 3, 4)), PR.bits(masked))
    # exceedance counts before the advection
    want = PR.exceedances(z0.cpu().numpy())
    worst = 0
    for plane_z, plane_o in zip(z.cpu().numpy().reshape(-1, size * size), zm.cpu().numpy().reshape(-1, size * size)):
        bound = PR.exceedance_bound(plane_z)
        worst = max(worst, bound)
        assert (np.abs(PR.exceedances(plane_o) - want) <= bound).all(), (PR.exceedances(plane_o), want, bound)
    # wet-area ratio at the first lead time against the frame that verifies it
    observed = torch.from_numpy(seq[4]).cuda()
    areas = {k: PR.wet_area(v[:, 0], 0.1) for k, v in (("plain", plain), ("matched", matched), ("masked", masked))}
    areas["observed"] = PR.wet_area(observed, 0.1)
    print(f"wet-area ratios at the first lead time {areas}; largest occupancy of a bin {worst}")
    assert abs(areas["matched"] - areas["observed"]) < abs(areas["plain"] - areas["observed"])
    assert abs(areas["masked"] - areas["observed"]) < abs(areas["plain"] - areas["observed"])
    # the three verifiers
    obs = torch.from_numpy(np.stack([seq[4], seq[4]]))[:, None].cuda()  # [T, C, H, W]
    for fc in (matched, masked):
        assert tuple(fc.shape) == (m, steps, 1, size, size) and torch.isfinite(fc).all() and (fc >= 0).all()
        ver, spec, val = NowcastVerifier(m, steps), SpectrumVerifier(m, steps, window=64), ValueVerifier(m, steps)
        for v in (ver, spec, val):
            v.update(fc, obs)
        ranks = np.asarray(ver.compute()["rank_histogram"], dtype=np.float64)
        assert np.allclose(ranks.sum(axis=-1), 1.0) and ranks.shape[-1] == m + 1
        assert np.isfinite(spec.compute()["psd_forecast"]).all() and np.isfinite(val.compute()["brier"]).all()
    entry = {"shape": [m, steps, size, size], "window": window, "largest_bin_occupancy": worst, "wet_area_lead1": areas}
    for thr in (1.0, 4.0):
        entry[f"area_ge_{thr:g}_lead1"] = {k: PR.wet_area(v[:, 0], thr) for k, v in (("plain", plain), ("matched", matched), ("masked", masked))}
        entry[f"area_ge_{thr:g}_lead1"]["observed"] = PR.wet_area(observed, thr)
        entry[f"csi_{thr:g}_lead1"] = {k: PR.pooled_csi(v[:, 0, 0], observed, thr) for k, v in (("plain", plain), ("matched", matched),
                                                                                               ("masked", masked))}
    _log_accuracy("nowcast 128x128 M=4 T=2 L=64, translating field", entry)
