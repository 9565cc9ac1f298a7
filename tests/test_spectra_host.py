"""Radial power spectra on the host: the numpy specification (spectra.radial_psd_reference) against an independent statement and
closed forms, SpectrumVerifier's bookkeeping on CPU tensors, and the C entry point's argument checks (no launch: there is no GPU here)."""
import ctypes

import numpy as np
import pytest
import torch

from spectra_recipe import impulse, make_field, plane_wave, punch_holes

from skillful_nowcasting_amd import spectra as S

SIZES = (32, 64, 128, 256, 512)


def _bins_by_rounding(window):
    k = np.arange(window)
    k = np.where(k >= window // 2, k - window, k)
    return np.floor(np.sqrt((k[:, None] ** 2 + k[None, :] ** 2).astype(np.float64)) + 0.5).astype(np.int64)


def test_reference_against_a_brute_force_dft():
    """L = 32: fft2 as two float64 matrix products, bins from floor(sqrt(d2) + 0.5) - both formulated independently of the module."""
    L = 32
    x = make_field(2, L, L, "continuous", seed=1)
    x[1, 3, 4] = np.nan  # one missing element: read as 0
    x[1, 20, 7] = -2.0
    power, missing = S.radial_psd_reference(x, L)
    assert power.shape == (2, 1, 1, 16) and missing.tolist() == [[[0]], [[2]]]
    n = np.arange(L)
    dft = np.exp(-2j * np.pi * np.outer(n, n) / L)
    bins = _bins_by_rounding(L)
    for p in range(2):
        xz = np.where(x[p] >= 0, x[p], 0.0).astype(np.float64)
        spec = dft @ xz @ dft.T
        mag = np.abs(spec) ** 2
        want = np.array([mag[bins == r].sum() for r in range(L // 2)])
        assert np.allclose(power[p, 0, 0], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("window", SIZES)
def test_integer_bins_equal_rounded_radius_and_counts_add_up(window):
    bins = S._radial_bins(window)
    assert np.array_equal(bins, _bins_by_rounding(window))
    counts = S.radial_bin_counts(window)
    assert counts.shape == (window // 2,) and counts.sum() == (bins < window // 2).sum()
    assert counts[:6].tolist() == [1, 8, 12, 16, 32, 28]
    k = np.fft.fftfreq(window, 1.0 / window)
    nyquist = (np.abs(k[:, None]) == window // 2) | (np.abs(k[None, :]) == window // 2)
    assert (bins[nyquist] >= window // 2).all()  # the whole Nyquist row and column are dropped


def test_impulse_has_a_flat_spectrum():
    for window in (32, 128):
        power, missing = S.radial_psd_reference(impulse(window, 3.0), window)
        assert missing.sum() == 0
        assert np.allclose(power[0, 0, 0], 9.0 * S.radial_bin_counts(window), rtol=1e-12, atol=0)


def test_constant_field_is_all_in_bin_zero():
    window = 64
    power, _ = S.radial_psd_reference(np.full((1, window, window), 2.5, np.float32), window)
    total = (2.5 * window * window) ** 2
    assert np.isclose(power[0, 0, 0, 0], total, rtol=1e-14) and (power[0, 0, 0, 1:] <= 1e-24 * total).all()


def test_plane_wave_lands_in_bin_five():
    """A (1 + cos(2 pi (3 i + 4 j) / L)) in fp32 (the samples are rounded to 2^-24 relative, hence 1e-6)."""
    for window in (32, 256):
        power, _ = S.radial_psd_reference(plane_wave(window, 2.0), window)
        amp = 2.0 * window * window
        assert np.isclose(power[0, 0, 0, 0], amp ** 2, rtol=1e-6) and np.isclose(power[0, 0, 0, 5], 2 * (amp / 2) ** 2, rtol=1e-6)
        rest = np.delete(power[0, 0, 0], [0, 5])
        assert (rest <= 1e-12 * amp ** 2).all()


def test_window_grid_is_cut_row_major():
    x = make_field(2, 64, 96, "radar", seed=2)
    power, missing = S.radial_psd_reference(x, 32)
    assert power.shape == (2, 2, 3, 16) and missing.shape == (2, 2, 3)
    one, _ = S.radial_psd_reference(x[1, 32:64, 64:96], 32)
    assert np.array_equal(power[1, 1, 2], one[0, 0])


def test_radial_psd_on_cpu_tensors_is_the_reference():
    x = punch_holes(make_field(3, 64, 64, "radar", seed=3), 32)
    ref_p, ref_m = S.radial_psd_reference(x, 32)
    p, m = S.radial_psd(torch.from_numpy(x).view(3, 1, 64, 64), 32)
    assert p.dtype == torch.float64 and m.dtype == torch.int64 and tuple(p.shape) == (3, 1, 2, 2, 16) and tuple(m.shape) == (3, 1, 2, 2)
    assert np.array_equal(p.numpy().reshape(ref_p.shape), ref_p) and np.array_equal(m.numpy().reshape(ref_m.shape), ref_m)
    assert ref_m[0, 1, 1] == 32 * 32 and ref_p[0, 1, 1].sum() == 0


@pytest.mark.parametrize("shape,window", [((1, 64, 64), 48), ((1, 64, 64), 16), ((1, 64, 64), 1024), ((1, 64, 96), 64), ((1, 96, 64), 64),
                                          ((0, 64, 64), 32), ((64,), 32)])
def test_bad_shapes_raise_value_error(shape, window):
    with pytest.raises(ValueError):
        S.radial_psd(torch.zeros(shape), window)
    if 0 not in shape:
        with pytest.raises(ValueError):
            S.radial_psd_reference(np.zeros(shape, np.float32), window)
    with pytest.raises(ValueError):
        S.radial_psd(torch.zeros(1, 32, 32, dtype=torch.float64), 32)
    with pytest.raises(ValueError):
        S.SpectrumVerifier(3, 2, window=100)


def _verifier_inputs(b=3, t=2, c=2, m=3, seed=5):
    f = make_field(m * b * t * c, 64, 64, "radar", seed).reshape(m, b, t, c, 64, 64)
    o = make_field(b * t * c, 64, 64, "radar", seed + 1).reshape(b, t, c, 64, 64)
    o[0, 0, 0, 3, 40] = np.nan   # window (0, 1) of case 0, lead time 0
    o[1, 1, 1, 32:, :32] = -1.0  # window (1, 0) of case 1, lead time 1
    return torch.from_numpy(f), torch.from_numpy(o)


def test_verifier_sums_member_spectra_and_masks_missing_windows():
    f, o = _verifier_inputs()
    w = np.array([2.0, 0.5, 4.0])
    v = S.SpectrumVerifier(3, 2, window=32, grid_km=2.0)
    v.update(f, o, weights=w)
    fp, _ = S.radial_psd_reference(f.numpy(), 32)  # [M, B, T, C, 2, 2, 16]
    op, om = S.radial_psd_reference(o.numpy(), 32)
    keep = (om == 0) * w[:, None, None, None, None]
    assert (om > 0).sum() == 2
    want_f = (fp * keep[None, ..., None]).sum(axis=(0, 1, 3, 4, 5))
    want_o = (op * keep[..., None]).sum(axis=(0, 2, 3, 4))
    want_n = keep.sum(axis=(0, 2, 3, 4))
    assert want_n.tolist() == [(8 - 1) * 2.0 + 8 * 0.5 + 8 * 4.0, 8 * 2.0 + (8 - 1) * 0.5 + 8 * 4.0]
    fc_acc, obs_acc, win_acc = v._acc
    assert np.allclose(fc_acc.numpy(), want_f, rtol=1e-13, atol=0) and np.allclose(obs_acc.numpy(), want_o, rtol=1e-13, atol=0)
    assert np.array_equal(win_acc.numpy(), want_n)
    # the members' own spectra, not the spectrum of the ensemble mean (which is smoother: less power away from bin 0)
    mean_p, _ = S.radial_psd_reference(f.numpy().mean(axis=0), 32)
    assert (fc_acc.numpy()[:, 8:] / 3 > 1.5 * (mean_p * keep[..., None]).sum(axis=(0, 2, 3, 4))[:, 8:]).all()
    res = v.compute()
    counts = S.radial_bin_counts(32)
    assert np.allclose(res["psd_forecast"], want_f / (3 * want_n[:, None] * counts), rtol=1e-13)
    assert np.allclose(res["psd_observed"], want_o / (want_n[:, None] * counts), rtol=1e-13)
    assert res["wavenumber"].tolist() == list(range(16)) and np.isinf(res["wavelength_km"][0])
    assert np.allclose(res["wavelength_km"][1:], 64.0 / np.arange(1, 16)) and np.array_equal(res["windows"], want_n)
    # one case as [M, T, C, H, W] is a batch of one
    one, batch = S.SpectrumVerifier(3, 2, window=32), S.SpectrumVerifier(3, 2, window=32)
    one.update(f[:, 1], o[1])
    batch.update(f[:, 1:2], o[1:2], weights=[1.0])
    assert all(torch.equal(a, b_) for a, b_ in zip(one._acc, batch._acc))


def test_verifier_merge_reset_and_empty_compute():
    f, o = _verifier_inputs(b=4)
    w = np.array([1.0, 3.0, 0.25, 2.0])
    whole, left, right = (S.SpectrumVerifier(3, 2, window=32) for _ in range(3))
    whole.update(f[:, :2], o[:2], w[:2])
    whole.update(f[:, 2:], o[2:], w[2:])
    left.update(f[:, :2], o[:2], w[:2])
    right.update(f[:, 2:], o[2:], w[2:])
    left.merge(right)
    assert all(torch.equal(a, b) for a, b in zip(whole._acc, left._acc))
    left.reset()
    assert all((a == 0).all() for a in left._acc)
    with pytest.raises(ValueError):
        left.merge(S.SpectrumVerifier(3, 2, window=64))
    with pytest.raises(ValueError):
        left.update(f[:2], o)
    with pytest.raises(ValueError):
        left.update(f, o, weights=[1.0])
    empty = S.SpectrumVerifier(3, 2, window=32).compute()  # nothing accumulated: NaN, not an exception
    assert np.isnan(empty["psd_forecast"]).all() and np.isnan(empty["psd_observed"]).all() and (empty["windows"] == 0).all()
    assert empty["psd_forecast"].shape == (2, 16)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as ge

    ge.build()
    from skillful_nowcasting_amd import _lib

    return _lib.load()


def test_library_exports_the_new_symbols_under_the_same_abi(lib):
    assert hasattr(lib, "dgmr_radial_psd") and hasattr(lib, "dgmr_radial_psd_workspace") and hasattr(lib, "dgmr_exceedance_table")
    assert lib.dgmr_abi_version() == 13


def test_workspace_is_monotone_up_to_its_cap(lib):
    table = 2048
    for L in (32, 64, 128):
        assert lib.dgmr_radial_psd_workspace(1, L, L, L) == table == lib.dgmr_radial_psd_workspace(1000, 4 * L, 2 * L, L)
    for L, per_win in ((256, 4 * 256 * 256 + 4 * 128 * 8), (512, 4 * 512 * 512 + 16 * 256 * 8)):
        one = lib.dgmr_radial_psd_workspace(1, L, L, L)
        assert one == table + per_win
        sizes = [lib.dgmr_radial_psd_workspace(n, L, 2 * L, L) for n in (1, 2, 3, 10, 100, 1000, 100000)]
        assert sizes[0] == table + 2 * per_win and all(a <= b for a, b in zip(sizes, sizes[1:]))
        assert sizes[-1] == sizes[-2] <= table + (64 << 20) and (sizes[-1] - table) % per_win == 0
    # a full-frame ensemble of 6 x 18 frames of 1536 x 1280 stays at the cap
    assert lib.dgmr_radial_psd_workspace(6 * 18, 1536, 1280, 256) <= table + (64 << 20)
    for bad in ((1, 64, 64, 48), (1, 64, 64, 1024), (1, 64, 96, 64), (0, 64, 64, 64), (1, 0, 64, 64)):
        assert lib.dgmr_radial_psd_workspace(*bad) < 0, bad
    assert b"dgmr_radial_psd_workspace" in lib.dgmr_last_error()


def test_c_entry_point_refuses_bad_arguments_before_any_launch(lib):
    """Every refusal comes from the argument checks at the top of dgmr_radial_psd: nothing is enqueued (there is no device here, and
    the pointers are host buffers that are never dereferenced)."""
    buf = (ctypes.c_double * 64)()
    p = ctypes.addressof(buf)
    base = p + (-p % 16)

    def go(x=base, stride=256 * 256, n=1, h=256, w=256, L=256, ws=base, ws_bytes=1 << 30, power=base, missing=base):
        return lib.dgmr_radial_psd(x, stride, n, h, w, L, ws, ws_bytes, power, missing, None)

    one = lib.dgmr_radial_psd_workspace(1, 256, 256, 256)
    for bad, text in [(dict(x=None), b"null pointer"), (dict(ws=None), b"null pointer"), (dict(power=None), b"null pointer"),
                      (dict(missing=None), b"null pointer"), (dict(L=48), b"window L=48"), (dict(L=1024, h=1024, w=1024), b"window L=1024"),
                      (dict(L=16, h=16, w=16), b"window L=16"), (dict(h=384), b"multiples of the window"), (dict(w=128), b"multiples of the window"),
                      (dict(n=0), b"planes"), (dict(x=base + 4), b"16-byte aligned"), (dict(ws=base + 8), b"16-byte aligned"),
                      (dict(power=base + 4), b"8-byte aligned"), (dict(stride=256 * 256 + 2), b"plane_stride"),
                      (dict(stride=256 * 256 - 4), b"plane_stride"), (dict(ws_bytes=one - 1), b"workspace"),
                      (dict(L=32, h=32, w=32, stride=1024, ws_bytes=2047), b"workspace")]:
        assert go(**bad) < 0, bad
        assert text in lib.dgmr_last_error(), (bad, lib.dgmr_last_error())
