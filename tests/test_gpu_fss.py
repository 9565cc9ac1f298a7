"""Fractions skill score sums on the GPU: dgmr_fss_sums (csrc/fss.hip) against fss.fss_sums_reference on the same arrays, bit for bit
(every term is an integer count), FractionsVerifier's device accumulators and DGMR.verify_batch.  The kernel works on 64 x 64 tiles of
window centres (fss_recipe.TILE): the larger shape and the seam positions are chosen for that tile.  No test has a time threshold."""
import numpy as np
import pytest
import torch

from fss_recipe import LARGE, MAX_RADIUS, RADII_SETS, SHAPES, THRESHOLD_SETS, TILE, case, reference, seam_positions
from spectra_recipe import THRESHOLDS, THRESHOLDS8, make_ensemble

pytestmark = pytest.mark.gpu


def _sums(f, o, thr, radii):
    from skillful_nowcasting_amd.fss import fss_sums

    sums, events = fss_sums(f if isinstance(f, torch.Tensor) else torch.from_numpy(f.copy()).cuda(),
                            o if isinstance(o, torch.Tensor) else torch.from_numpy(o.copy()).cuda(), thr, radii)
    torch.cuda.synchronize()
    return sums, events


def _assert_equal(got, want):
    (gs, ge), (ws, we) = got, want
    assert gs.dtype == torch.int64 and ge.dtype == torch.int64
    assert np.array_equal(ge.cpu().numpy(), we), "events"
    assert np.array_equal(gs.cpu().numpy(), ws), "sums"


@pytest.mark.parametrize("radii_key", sorted(RADII_SETS))
@pytest.mark.parametrize("k", sorted(THRESHOLD_SETS))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(str(v) for v in s))
@pytest.mark.parametrize("m", [1, 6, 8, 12, 32])
def test_sums_equal_the_reference(m, shape, k, radii_key):
    """M = 1, 6, 8, 12 and 32 take the kernel's five member-loop instantiations; K = 8 with M = 32 and R = 32 needs four threshold groups,
    with M = 6 two; one threshold at one radius splits the tile rows into four chunks, one at several radii or several at one into
    fewer; the larger shape has two whole tiles and a ragged one in both directions."""
    assert TILE == 64 and shape[1] % 16 == 0 and shape[2] % 16 == 0
    f, o = case(m, shape)
    want = reference(m, shape, k, radii_key)
    got = _sums(f, o, THRESHOLD_SETS[k], RADII_SETS[radii_key])
    assert tuple(got[0].shape) == (shape[0], k, len(RADII_SETS[radii_key]), 4) and tuple(got[1].shape) == (shape[0], k, 2)
    _assert_equal(got, want)
    assert want[0][0, 0].sum() > 0 and want[1][0, 0].sum() > 0
    if shape[0] > 1:
        assert (want[0][-1] == 0).all() and (want[1][-1] == 0).all()  # the wholly missing plane


def test_saturated_windows_need_64_bit_products():
    """M = 32, one 96 x 80 plane, everything wet, r = 32: interior windows are full, one S_f^2 term is (32 * 65^2)^2 = 1.8e10."""
    m, h, w, r = 32, 96, 80, 32
    f = torch.full((m, 1, h, w), 9.0).cuda()
    o = torch.full((1, h, w), 9.0).cuda()
    sums, events = _sums(f, o, (1.0,), (r,))
    cy = [min(h - 1, y + r) - max(0, y - r) + 1 for y in range(h)]   # rows of the plane in the window of row y
    cx = [min(w - 1, x + r) - max(0, x - r) + 1 for x in range(w)]
    assert max(cy) * max(cx) == 65 * 65 and (m * 65 * 65) ** 2 > 2 ** 32
    q = sum(v * v for v in cy) * sum(v * v for v in cx)               # sum over centres of (cy cx)^2, Python integers
    assert sums.cpu().numpy().tolist() == [[[[m * m * q, q, m * q, m * q]]]]
    assert events.cpu().numpy().tolist() == [[[m * h * w, h * w]]]


def test_a_window_that_contains_the_plane():
    f, o = case(6, (2, 16, 16))
    sums, events = (a.cpu().numpy() for a in _sums(f, o, THRESHOLDS, (MAX_RADIUS,)))
    ef, eo = events[0, :, 0], events[0, :, 1]
    assert (ef > 0).all() and (eo > 0).all()
    assert np.array_equal(sums[0, :, 0, 0], 256 * ef ** 2) and np.array_equal(sums[0, :, 0, 1], 256 * eo ** 2)
    assert np.array_equal(sums[0, :, 0, 2], 256 * ef * eo)


@pytest.mark.parametrize("where", ["member", "observation", "both"])
def test_single_wet_pixels_at_corners_and_tile_seams(where):
    """One plane per position of fss_recipe.seam_positions (64 x 64 tiles): the four corners, both sides of every tile seam and the
    distances 32 and 33 / 31 and 32 from it, out to which the largest radius reaches.  The pixel is in member 1 of 2, in the
    observation, or in both at neighbouring positions of the list."""
    from skillful_nowcasting_amd.fss import fss_sums_reference

    pos = seam_positions()
    _, h, w = LARGE
    assert all(0 <= y < h and 0 <= x < w for y, x in pos)
    assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1), (63, 64), (64, 63), (127, 128), (128, 191), (64, 192)} <= set(pos)
    assert {y for y, _ in pos} >= {31, 32, 95, 96, 63, 64, 127, 128} and {x for _, x in pos} >= {31, 32, 159, 160, 191, 192}
    n = len(pos)
    f = np.zeros((2, n, h, w), np.float32)
    o = np.zeros((n, h, w), np.float32)
    for i, (y, x) in enumerate(pos):
        if where in ("member", "both"):
            f[1, i, y, x] = 5.0
        if where == "observation":
            o[i, y, x] = 5.0
        if where == "both":
            y2, x2 = pos[(i + 1) % n]
            o[i, y2, x2] = 5.0
    radii = (MAX_RADIUS, 0, 2, 8)
    want = fss_sums_reference(f, o, (4.0,), radii)
    assert want[1].sum() == (2 * n if where == "both" else n)
    _assert_equal(_sums(f, o, (4.0,), radii), want)


def test_nan_and_infinite_members_and_a_missing_plane():
    from skillful_nowcasting_amd.fss import fss_sums_reference

    f, o = (a.copy() for a in case(6, (3, 32, 48)))
    rng = np.random.Generator(np.random.PCG64(70))
    f[:, 0][rng.random(f[:, 0].shape) < 0.05] = np.nan
    f[3, 1] = np.inf
    f[4, 1] = -np.inf
    f[2, 2] = np.inf  # the missing plane: no event, whatever the members hold
    want = fss_sums_reference(f, o, THRESHOLDS8, RADII_SETS["default"])
    got = _sums(f, o, THRESHOLDS8, RADII_SETS["default"])
    _assert_equal(got, want)
    assert (got[0][2] == 0).all() and (got[1][2] == 0).all()
    assert (want[1][1, :, 0] >= want[1][1, 0, 1]).all()  # the +inf member reaches every threshold at every present pixel


def test_strided_members_and_unflattened_planes(monkeypatch):
    """`full[:, 1]` of an [M, 3, N, H, W] tensor is read in place through the member stride."""
    from skillful_nowcasting_amd import _lib
    from skillful_nowcasting_amd.verification import _planes_contiguous

    f, o = case(6, (3, 32, 48))
    want = reference(6, (3, 32, 48), 3, "default")
    full = torch.rand(6, 3, 3, 32, 48, generator=torch.Generator().manual_seed(0)).cuda() * 20.0
    full[:, 1] = torch.from_numpy(f.copy()).cuda()
    view = full[:, 1]
    assert not view.is_contiguous() and _planes_contiguous(view) and view.data_ptr() == full.data_ptr() + 4 * 3 * 32 * 48
    obs = torch.from_numpy(o.copy()).cuda()
    seen = []

    def spy(name, *args):
        seen.append((name, args[0], args[1]))
        return real_call(name, *args)

    real_call = _lib.call
    monkeypatch.setattr(_lib, "call", spy)  # (fss_sums looks `call` up when it runs)
    _assert_equal(_sums(view, obs, THRESHOLDS, RADII_SETS["default"]), want)
    monkeypatch.undo()
    assert seen == [("dgmr_fss_sums", view.data_ptr(), full.stride(0))]  # no copy: the view's own pointer and stride
    _assert_equal(_sums(view.view(6, 3, 1, 32, 48), obs.view(3, 1, 32, 48), THRESHOLDS, RADII_SETS["default"]), want)
    members_innermost = view.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)  # a layout that has to be copied
    _assert_equal(_sums(members_innermost, obs, THRESHOLDS, RADII_SETS["default"]), want)


def test_outputs_are_cleared_and_two_launches_give_the_same_bits():
    """Two launches give the same bits, and the call clears its outputs itself: the C entry point is given outputs pre-filled with
    garbage."""
    import ctypes

    from skillful_nowcasting_amd._lib import call
    from skillful_nowcasting_amd.verification import _device_thresholds

    f, o = case(6, LARGE)
    want = reference(6, LARGE, 3, "default")
    fc, ob = torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda()
    a = _sums(fc, ob, THRESHOLDS, RADII_SETS["default"])
    b = _sums(fc, ob, THRESHOLDS, RADII_SETS["default"])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    _assert_equal(a, want)
    sums = torch.full((1, 3, 4, 4), -0x0123456789ABCDEF, dtype=torch.int64, device="cuda")
    events = torch.full((1, 3, 2), 0x7EDCBA9876543210, dtype=torch.int64, device="cuda")
    thr = _device_thresholds(fc.device, np.asarray(THRESHOLDS, np.float32))
    call("dgmr_fss_sums", fc.data_ptr(), fc.stride(0), ob.data_ptr(), 6, 1, LARGE[1], LARGE[2], thr.data_ptr(), 3,
         (ctypes.c_int * 4)(*RADII_SETS["default"]), 4, sums.data_ptr(), events.data_ptr(),
         ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    _assert_equal((sums, events), want)


def test_runs_on_the_callers_stream():
    from skillful_nowcasting_amd.fss import fss_sums

    f, o = case(6, (3, 32, 48))
    fc, ob = torch.from_numpy(f.copy()).cuda(), torch.from_numpy(o.copy()).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = fss_sums(fc, ob, THRESHOLDS, RADII_SETS["default"])
    side.synchronize()
    _assert_equal(got, reference(6, (3, 32, 48), 3, "default"))


def test_fractions_verifier_on_the_device_against_cpu_tensors():
    """The same updates on device and on CPU tensors with power-of-two weights: every float64 product and sum is exact, so the
    accumulators and everything compute() derives from them are equal exactly.  merge across two verifiers."""
    from skillful_nowcasting_amd.fss import FractionsVerifier

    m, b, t, c = 6, 4, 2, 2
    f, o = make_ensemble(m, b * t * c, 32, 48, "radar", seed=11)
    o[-1] = o[1]
    f, o = f.reshape(m, b, t, c, 32, 48), o.reshape(b, t, c, 32, 48)
    w = [2.0, 0.5, 4.0, 1.0]
    radii = RADII_SETS["default"]
    host, dev, left, right = (FractionsVerifier(m, t, THRESHOLDS, radii) for _ in range(4))
    fd, od = torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda()
    host.update(torch.from_numpy(f), torch.from_numpy(o), weights=w)
    dev.update(fd, od, weights=w)
    left.update(fd[:, :2], od[:2], weights=w[:2])
    right.update(fd[:, 2:], od[2:], weights=torch.tensor(w[2:], dtype=torch.float64, device="cuda"))
    left.merge(right)
    torch.cuda.synchronize()
    for v in (dev, left):
        for name in ("_sums", "_events", "_pixels"):
            got = getattr(v, name)
            assert got.is_cuda and got.dtype == torch.float64 and torch.equal(got.cpu(), getattr(host, name)), name
    a, h = dev.compute(), host.compute()
    assert set(a) == set(h) >= {"fss", "fss_members", "base_rate", "forecast_rate", "frequency_bias", "fss_random", "fss_useful",
                                "skilful_side", "sides"}
    for key in a:
        assert np.array_equal(a[key], h[key], equal_nan=True), key
    assert np.isfinite(h["fss"]).all() and (h["fss"] > 0).all() and (h["fss"] <= 1).all() and (h["fss_members"] <= h["fss"]).all()
    one = FractionsVerifier(m, t, THRESHOLDS, radii)  # a single case without a batch dimension
    one.update(fd[:, 1], od[1], weights=0.5)
    torch.cuda.synchronize()
    ref = FractionsVerifier(m, t, THRESHOLDS, radii)
    ref.update(torch.from_numpy(f[:, 1:2]), torch.from_numpy(o[1:2]), weights=[0.5])
    assert torch.equal(one._sums.cpu(), ref._sums) and torch.equal(one._pixels.cpu(), ref._pixels)


KW = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)


def test_verify_batch_fills_a_fractions_verifier():
    import skillful_nowcasting_amd as S
    from skillful_nowcasting_amd.fss import FractionsVerifier, fss_sums_reference

    torch.manual_seed(0)
    model = S.DGMR(**KW).to("cuda")
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 4, 1, 128, 128, generator=g).cuda()
    y = torch.rand(2, 2, 1, 128, 128, generator=g).cuda()
    y[1, 0, 0, 3:40, 5] = -1.0  # some missing observations
    model.eval()
    thr, radii, w = (0.25, 0.5), (0, 2, 8), [2.0, 0.5]
    v = FractionsVerifier(3, 2, thr, radii)
    torch.manual_seed(5)
    out = model.verify_batch((x, y), v, num_samples=3, weights=w)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 2, 2, 1, 128, 128)
    sums, events = fss_sums_reference(out.reshape(3, 4, 128, 128).cpu().numpy(), y.reshape(4, 128, 128).cpu().numpy(), thr, radii)
    wn = np.asarray(w)
    want_sums = (sums.reshape(2, 2, 2, 3, 4) * wn[:, None, None, None, None]).sum(axis=0)      # [B, T, K, S, 4] -> [T, K, S, 4]
    want_events = (events.reshape(2, 2, 2, 2) * wn[:, None, None, None]).sum(axis=0)
    assert np.array_equal(v._sums.cpu().numpy(), want_sums) and np.array_equal(v._events.cpu().numpy(), want_events)
    assert v._pixels.cpu().tolist() == [2.5 * 128 * 128] * 2
    res = v.compute()
    assert res["fss"].shape == (2, 3, 2) and np.isfinite(res["fss"]).all() and (res["fss"] >= 0).all() and (res["fss"] <= 1).all()
    ff, oo, fo = (want_sums[..., q].transpose(1, 2, 0) for q in range(3))
    assert np.array_equal(res["fss"], 2.0 * fo / 3.0 / (ff / 9.0 + oo))
