"""Radial power spectra on the GPU: dgmr_radial_psd (csrc/spectrum.hip) against spectra.radial_psd_reference on the same arrays - the
in-LDS path (L <= 128) and the two-pass path (L >= 256) - SpectrumVerifier's device accumulators and DGMR.verify_batch.  No test has
a time threshold."""
import json
import os

import numpy as np
import pytest
import torch

from conftest import BAND_LOG
from spectra_recipe import check_psd, field_with_reference, impulse, make_field, plane_wave, psd_bound, punch_holes

pytestmark = pytest.mark.gpu

PLANES = {32: 3, 64: 3, 128: 3, 256: 2, 512: 1}
# beside the band tables of the run (conftest.BAND_LOG); the committed copy is profiles/radial_psd_accuracy.json
ACCURACY_LOG = os.path.join(os.path.dirname(BAND_LOG), "radial_psd_accuracy.json")


def _psd(x, window, **kw):
    from skillful_nowcasting_amd.spectra import radial_psd

    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).cuda()  # (a copy: the shared cases are read-only)
    power, missing = radial_psd(t, window, **kw)
    torch.cuda.synchronize()
    return power, missing


def _log_accuracy(window, entry):
    try:
        os.makedirs(os.path.dirname(ACCURACY_LOG), exist_ok=True)
        rec = json.load(open(ACCURACY_LOG)) if os.path.exists(ACCURACY_LOG) else {}
        rec[str(window)] = entry
        with open(ACCURACY_LOG, "w") as f:
            json.dump(rec, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("window", sorted(PLANES))
def test_psd_matches_the_reference(window):
    """Per window and bin |sqrt(got) - sqrt(ref)| <= eps(L) L sqrt(sum x^2), eps(L) = 16 * 2 log2(L) * 2^-24 (spectra_recipe.psd_bound).
    Printed and logged, not asserted: the worst per-bin relative error next to that of torch.fft.fft2 in fp32 on the CPU."""
    from skillful_nowcasting_amd.spectra import _radial_bins

    n = PLANES[window]
    x, ref, ref_missing = field_with_reference(n, window, window, window, "radar")
    power, missing = _psd(x, window)
    assert tuple(power.shape) == (n, 1, 1, window // 2) and power.dtype == torch.float64 and missing.dtype == torch.int64
    got = power.cpu().numpy()
    assert np.array_equal(missing.cpu().numpy(), ref_missing) and (ref_missing == 0).all()
    # torch's own fp32 transform of the same input, binned in float64
    spec = torch.fft.fft2(torch.from_numpy(x.copy())).numpy().astype(np.complex128)
    mag = (spec.real ** 2 + spec.imag ** 2).reshape(n, -1)
    bins = _radial_bins(window).reshape(-1)
    keep = bins < window // 2
    t32 = np.stack([np.bincount(bins[keep], weights=mag[i][keep], minlength=window // 2) for i in range(n)]).reshape(ref.shape)
    rel_dev, rel_t32 = float(np.max(np.abs(got - ref) / ref)), float(np.max(np.abs(t32 - ref) / ref))
    bound = psd_bound(x, window)[..., None]
    ratio_t32 = float(np.max(np.abs(np.sqrt(t32) - np.sqrt(ref)) / bound))
    print(f"L={window}: worst per-bin relative error device {rel_dev:.3e}, torch.fft.fft2 fp32 on the CPU {rel_t32:.3e} "
          f"(the latter at {ratio_t32:.3e} of the bound)")
    ratio = check_psd(got, ref, x, window, "parity")
    _log_accuracy(window, {"planes": n, "kind": "radar", "device_worst_relative_error": rel_dev, "torch_fp32_cpu_worst_relative_error": rel_t32,
                           "device_gap_over_bound": ratio, "torch_fp32_cpu_gap_over_bound": ratio_t32})


@pytest.mark.parametrize("window", [64, 256])
def test_exact_cases(window):
    from skillful_nowcasting_amd.spectra import radial_bin_counts

    counts = radial_bin_counts(window).astype(np.float64)
    wave = np.zeros(window // 2)
    wave[0], wave[5] = (2.0 * window * window) ** 2, 2.0 * (window * window) ** 2
    cases = {"impulse": (impulse(window, 3.0), 9.0 * counts),
             "constant": (np.full((1, window, window), 2.5, np.float32), np.r_[(2.5 * window * window) ** 2, np.zeros(window // 2 - 1)]),
             "plane wave": (plane_wave(window, 2.0), wave)}
    for name, (x, want) in cases.items():
        power, missing = _psd(x, window)
        assert int(missing.sum()) == 0
        # the closed form stands in for the reference (the plane wave's fp32 samples move it by 1e-7 relative: far below the bound)
        check_psd(power.cpu().numpy(), want.reshape(1, 1, 1, -1), x, window, name)


@pytest.mark.parametrize("window,h,w", [(32, 64, 96), (256, 256, 512)])
def test_window_grid_is_the_single_window_call(window, h, w):
    """Each window of a plane equals, bit for bit, the call on the sliced and copied window."""
    from spectra_recipe import windows_of

    x = punch_holes(make_field(2, h, w, "radar", seed=4), window)
    power, missing = _psd(x, window)
    singles = np.ascontiguousarray(windows_of(x, window).reshape(-1, window, window))
    p1, m1 = _psd(singles, window)
    assert torch.equal(power.reshape(-1, window // 2), p1.reshape(-1, window // 2)) and torch.equal(missing.reshape(-1), m1.reshape(-1))
    assert int(m1.reshape(-1)[h // window * (w // window) - 1]) == window * window  # plane 0's last window is missing as a whole


def test_strided_view_gives_the_bits_of_its_copy():
    """`ensemble[:, 1]` of an [M, 3, H, W] tensor is read in place through the plane stride."""
    from skillful_nowcasting_amd.spectra import _plane_layout

    full = torch.from_numpy(make_field(9, 64, 96, "radar", seed=6)).cuda().view(3, 3, 64, 96)
    view = full[:, 1]
    assert not view.is_contiguous() and _plane_layout(view) == 3 * 64 * 96
    a, am = _psd(view, 32)
    b, bm = _psd(view.contiguous(), 32)
    assert torch.equal(a, b) and torch.equal(am, bm)
    x, ref, _ = field_with_reference(3, 64, 64, 64, "radar")
    wide = torch.zeros(3, 64, 128).cuda()
    wide[:, :, 64:] = torch.from_numpy(x.copy()).cuda()
    c, _ = _psd(wide[:, :, 64:], 64)  # rows that are not contiguous: copied first
    check_psd(c.cpu().numpy(), ref, x, 64, "column slice")


@pytest.mark.parametrize("window,n", [(32, 5), (256, 3)])
def test_result_does_not_depend_on_the_workspace(window, n):
    from skillful_nowcasting_amd._lib import load

    x = torch.from_numpy(make_field(n, window, window, "radar", seed=8)).cuda()
    full, _ = _psd(x, window)
    again, _ = _psd(x, window)
    assert torch.equal(full, again)  # two identical calls
    one = int(load().dgmr_radial_psd_workspace(1, window, window, window))
    if window >= 256:  # the two-pass path then takes one window per round
        assert one < int(load().dgmr_radial_psd_workspace(n, window, window, window))
    small, sm = _psd(x, window, workspace=torch.empty(one, dtype=torch.uint8, device="cuda"))
    assert torch.equal(full, small) and int(sm.sum()) == 0
    x_ref = x.cpu().numpy()
    from skillful_nowcasting_amd.spectra import radial_psd_reference

    check_psd(small.cpu().numpy(), radial_psd_reference(x_ref, window)[0], x_ref, window, "one-window workspace")


@pytest.mark.parametrize("window,h,w", [(32, 64, 64), (128, 128, 256), (256, 512, 256)])
def test_missing_data(window, h, w):
    """Scattered -1, NaN, -inf and one whole missing window: the counts are exact, the power is that of the zero-filled field."""
    from skillful_nowcasting_amd.spectra import radial_psd_reference

    x = punch_holes(make_field(2, h, w, "radar", seed=9), window)
    ref, ref_missing = radial_psd_reference(x, window)
    assert ref_missing.max() == window * window and 0 < ref_missing[1].sum() < window * window
    power, missing = _psd(x, window)
    assert np.array_equal(missing.cpu().numpy(), ref_missing)
    got = power.cpu().numpy()
    check_psd(got, ref, x, window, "missing data")
    assert (got[ref_missing == window * window] == 0).all()


def _verifier_case():
    m, b, t = 3, 2, 2
    f = make_field(m * b * t, 64, 64, "radar", seed=12).reshape(m, b, t, 1, 64, 64)
    o = make_field(b * t, 64, 64, "radar", seed=13).reshape(b, t, 1, 64, 64)
    o[0, 1, 0, 40, 3] = np.nan     # window (1, 0) of case 0, lead time 1
    o[1, 0, 0, :32, 32:] = -1.0    # window (0, 1) of case 1, lead time 0
    return f, o


def test_spectrum_verifier_on_the_device_against_cpu_tensors():
    """The same updates on device and on CPU tensors (the reference).  Window counts exactly; a window's power may differ by
    |g - r| = |sqrt g - sqrt r| (sqrt g + sqrt r) <= b (2 sqrt r + b), b the bound of psd_bound, and the weighted sums by the weighted
    sum of that (+ 1e-12 relative for the float64 additions)."""
    from skillful_nowcasting_amd.spectra import SpectrumVerifier, radial_psd_reference

    f, o = _verifier_case()
    w = [2.0, 5.0]
    dev, host = SpectrumVerifier(3, 2, window=32), SpectrumVerifier(3, 2, window=32)
    dev.update(torch.from_numpy(f).cuda(), torch.from_numpy(o).cuda(), weights=w)
    host.update(torch.from_numpy(f), torch.from_numpy(o), weights=w)
    torch.cuda.synchronize()
    assert all(a.is_cuda and a.dtype == torch.float64 for a in dev._acc)
    assert torch.equal(dev._acc[2].cpu(), host._acc[2]) and host._acc[2].tolist() == [2.0 * 4 + 5.0 * 3, 2.0 * 3 + 5.0 * 4]
    _, om = radial_psd_reference(o, 32)
    keep = (om == 0) * np.asarray(w)[:, None, None, None, None]  # [B, T, C, 2, 2]
    for which, x, lead_axes in ((0, f, (0, 1, 3, 4, 5)), (1, o, (0, 2, 3, 4))):
        ref, _ = radial_psd_reference(x, 32)
        b = psd_bound(x, 32)[..., None]
        k = keep[None, ..., None] if which == 0 else keep[..., None]
        tol = (k * b * (2.0 * np.sqrt(ref) + b)).sum(axis=lead_axes)
        want = host._acc[which].numpy()
        gap = np.abs(dev._acc[which].cpu().numpy() - want)
        print(f"SpectrumVerifier accumulator {which}: largest gap / allowed {np.max(gap / (tol + 1e-12 * want)):.3e}")
        assert (gap <= tol + 1e-12 * want).all()
    a, h = dev.compute(), host.compute()
    assert np.array_equal(a["windows"], h["windows"]) and a["psd_forecast"].shape == h["psd_forecast"].shape == (2, 16)
    # excluded from forecast and observed sums alike: without the mask both would be larger
    unmasked = SpectrumVerifier(3, 2, window=32)
    unmasked.update(torch.from_numpy(f).cuda(), torch.from_numpy(np.where(o >= 0, o, 0.0).astype(np.float32)).cuda(), weights=w)
    assert (unmasked._acc[0] > dev._acc[0]).all() and (unmasked._acc[2] > dev._acc[2]).all()


KW = dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2)


@pytest.fixture(scope="module")
def model_and_batch():
    import skillful_nowcasting_amd as S

    torch.manual_seed(0)
    model = S.DGMR(**KW).to("cuda")
    g = torch.Generator().manual_seed(1)
    x = torch.rand(2, 4, 1, 128, 128, generator=g).cuda()
    y = torch.rand(2, 2, 1, 128, 128, generator=g).cuda()
    y[1, 0, 0, 3:40, 5] = -1.0  # some missing observations: windows (0, 0) and (1, 0) of case 1, lead time 0
    return model, x, y


def test_verify_batch_fills_a_spectrum_verifier(model_and_batch):
    from skillful_nowcasting_amd.spectra import SpectrumVerifier, radial_psd_reference

    model, x, y = model_and_batch
    model.eval()
    v = SpectrumVerifier(3, 2, window=32, grid_km=1.0)
    torch.manual_seed(5)
    out = model.verify_batch((x, y), v, num_samples=3)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (3, 2, 2, 1, 128, 128)
    res = v.compute()
    assert res["windows"].tolist() == [32.0 - 2.0, 32.0] and res["psd_forecast"].shape == (2, 16)
    assert np.isfinite(res["psd_forecast"]).all() and (res["psd_observed"] > 0).all()
    ref, missing = radial_psd_reference(y.cpu().numpy(), 32)
    keep = (missing == 0)[..., None]
    want = (ref * keep).sum(axis=(0, 2, 3, 4))
    b = psd_bound(y.cpu().numpy(), 32)[..., None]
    tol = (keep * b * (2.0 * np.sqrt(ref) + b)).sum(axis=(0, 2, 3, 4))  # as in the test above
    assert (np.abs(v._acc[1].cpu().numpy() - want) <= tol + 1e-12 * want).all()
