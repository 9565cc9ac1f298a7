"""Device time of the rho(r) estimate on a full 1536 x 1280 composite (skillful_nowcasting_amd/stochastic.py: lag_spectra,
estimate_rho; dgmr_lag_spectra in csrc/spectrum.hip).

    python tools/lag_estimate_timing.py [--repeats 7] [--out profiles/lag_estimate_timing.json]

Inputs: the rain-covered sequence of tools/advection_timing.py (a smooth field moving by (2, -3) pixels per frame), four context
frames - three consecutive pairs -, window 128.  HIP events bracket single calls on one stream; after a warm-up the median over
--repeats calls counts (minimum and maximum are listed).

  * dgmr_lag_spectra alone on the three pairs of aligned frames, with the bytes it must read (every pixel of both planes once per
    class that covers it) and its transform count;
  * the same sums by torch.fft on the same device (rfft2 over the windows of each class, the three terms, a matrix product with the
    bins' indicator in float64), for scale, and how far the two results are apart relative to the largest sum;
  * the whole estimate_rho (alignment, kernel, pooling) on the context's motion field;
  * one whole EnsembleAdvectionNowcaster.nowcast (M = 8, T = 18) with rho="estimate" against rho=None.
Numbers are recorded, not asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, T_OUT, MEMBERS, WINDOW = 1536, 1280, 18, 8, 128


def lag_spectra_torch(a, b, window):
    """stochastic.lag_spectra_reference with torch.fft in fp32 on the tensors' device (half spectra with the Hermitian weights)."""
    import numpy as np
    import torch

    from skillful_nowcasting_amd.spectra import _radial_bins

    n, h, w = a.shape
    half = window // 2
    bins = _radial_bins(window)[:, :half + 1].reshape(-1)
    weight = np.tile(np.where((np.arange(half + 1) == 0) | (np.arange(half + 1) == half), 1.0, 2.0), window)
    onehot = np.zeros((bins.size, window))
    onehot[np.arange(bins.size), bins] = weight
    onehot = torch.from_numpy(onehot).to(a.device)
    blocks = []
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)

            def spectra(x):
                t = x[:, ys, xs].reshape(n, ny, window, nx, window).movedim(-3, -2)
                return torch.fft.rfft2(t).reshape(n, ny * nx, -1)

            fa, fb = spectra(a), spectra(b)
            terms = torch.stack([fa.real * fa.real + fa.imag * fa.imag, fb.real * fb.real + fb.imag * fb.imag,
                                 fa.real * fb.real + fa.imag * fb.imag], dim=2)
            blocks.append(terms.double() @ onehot)
    return torch.cat(blocks, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from advection_timing import rain_sequence
    from skillful_nowcasting_amd.advection import lattice_geometry, motion_field
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, estimate_rho, lag_spectra, lagrangian_frames, to_db, window_table
    from stochastic_timing import timed

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    seq = rain_sequence(gen, dev, 4, (2, -3), False)  # [4, H, W]
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/lag_estimate_timing.py --repeats {a.repeats}", "frame": [H, W],
           "context_frames": 4, "pairs": 3, "window": WINDOW, "wet_pixel_share": float((seq > 0).double().mean())}
    field = motion_field(seq[:, None], 32, 16, 8)
    origin, spacing = lattice_geometry(32, 16)
    z = to_db(seq[:, None])  # [4, 1, H, W]
    frames = lagrangian_frames(z, field, origin, spacing)
    fa, fb = frames[:-1, 0], frames[1:, 0]
    table = window_table(H, W, WINDOW)
    sums = torch.empty((3, len(table), 3, WINDOW), dtype=torch.float64, device=dev)
    lag = timed(lambda: lag_spectra(fa, fb, WINDOW, out=sums), a.repeats)
    nbytes = 3 * 2 * len(table) * WINDOW * WINDOW * 4
    lag.update({"windows": 3 * len(table), "transforms_2d": 3 * 2 * len(table), "bytes_read": nbytes, "GB_per_s": nbytes / lag["ms"] / 1e6})
    rec["lag_spectra"] = lag
    print(f"lag_spectra  3 pairs L={WINDOW}: {lag['ms']:.3f} ms ({lag['min_ms']:.3f} - {lag['max_ms']:.3f}), {lag['windows']} windows, "
          f"{lag['GB_per_s']:.0f} GB/s read", flush=True)
    try:
        ref = lag_spectra_torch(fa, fb, WINDOW)
        gap = float((ref - sums).abs().max() / ref.abs().max())
        tf = timed(lambda: lag_spectra_torch(fa, fb, WINDOW), max(3, a.repeats // 2))
        tf["max_difference_to_kernel_over_largest_sum"] = gap
        tf["over_kernel"] = tf["ms"] / lag["ms"]
        rec["lag_spectra_torch_fft"] = tf
        print(f"torch.fft sums: {tf['ms']:.3f} ms ({tf['over_kernel']:.1f} x the kernel), largest relative difference {gap:.3e}", flush=True)
        del ref
    except RuntimeError as e:  # no FFT library on the device
        rec["lag_spectra_torch_fft"] = {"unavailable": str(e).splitlines()[0]}
        print(f"torch.fft on the device is not available: {rec['lag_spectra_torch_fft']['unavailable']}", flush=True)
    est = estimate_rho(z, field, origin, spacing, WINDOW)
    rec["estimate_rho"] = timed(lambda: estimate_rho(z, field, origin, spacing, WINDOW), a.repeats)
    rec["estimate_rho"].update({"windows_used": float(est.windows[0]), "windows_per_plane": len(table),
                                "min_rho_over_bins_with_modes": float(est.rho[0, :int(round(WINDOW / 2 ** 0.5)) + 1].min())})
    print(f"estimate_rho: {rec['estimate_rho']['ms']:.3f} ms, {rec['estimate_rho']['windows_used']:.0f} of {len(table)} windows used, "
          f"smallest rho {rec['estimate_rho']['min_rho_over_bins_with_modes']:.4f}", flush=True)
    del frames, sums
    context = seq[..., None].contiguous()
    for key, rho in (("nowcast", None), ("nowcast_estimated_rho", "estimate")):
        nc = EnsembleAdvectionNowcaster(forecast_steps=T_OUT, window=WINDOW, rho=rho)
        rec[key] = timed(lambda: nc.nowcast(context, MEMBERS, seed=1), a.repeats)
        print(f"whole {key}: {rec[key]['ms']:.3f} ms", flush=True)
    rec["nowcast_estimated_rho"]["over_fixed_law"] = rec["nowcast_estimated_rho"]["ms"] / rec["nowcast"]["ms"]
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
