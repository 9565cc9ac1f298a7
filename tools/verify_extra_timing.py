"""Device time of dgmr_radial_psd and dgmr_exceedance_table at the two shapes they are used at.

    python tools/verify_extra_timing.py [--repeats 11] [--out profiles/verify_extra_timing.json]

Inputs: a crop ensemble [6, 16, 18, 1, 256, 256] (453 MB + a 75 MB observation) and a full-frame ensemble [6, 18, 1, 1536, 1280]
(849 MB + 141 MB), window 256 for the spectra, thresholds (1, 4, 8) mm/h for the table, radar-like values (multiples of 1/32, ~70 %
zeros, 0.1 % of the observation missing).  HIP events bracket windows of back-to-back calls on one stream; after a warm-up the median
over --repeats windows counts (minimum and maximum are listed).  Both inputs are larger than the 256 MiB last-level cache.

Per call: the time, the bytes read once (elements * 4: the ensemble for the spectra, ensemble + observation for the table) and the
ratio of the time to that traffic at the measured 6.29 TB/s copy rate.  The two-pass spectra also write and re-read the half
spectrum (twice the input's bytes again), listed as `workspace_bytes_moved`.  For the spectra, the same quantity by
`torch.fft.rfft2` + `index_add_` on the same device is timed next to the kernel, alternating, if that route runs there, and the two
results are compared.  Numbers are recorded, not asserted; there is no earlier kernel to compare with."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WINDOW, THRESHOLDS = 256, (1.0, 4.0, 8.0)
SHAPES = {"crop_ensemble": (6, 16, 18, 1, 256, 256), "full_frame_ensemble": (6, 18, 1, 1536, 1280)}
COPY_BYTES_PER_S = 6.29e12  # measured device-to-device copy rate of the MI355X


def radar_like(shape, gen, device):
    import torch

    x = torch.empty(shape, device=device)
    for part in x.view(-1, *shape[-2:]).split(64):
        v = torch.empty(part.shape, device=device).exponential_(0.25, generator=gen)
        v = torch.round(v * 32.0) / 32.0
        v[torch.rand(part.shape, device=device, generator=gen) < 0.7] = 0.0
        part.copy_(v)
    return x


def torch_psd(x, window, bins, weight):
    """The same sums through torch.fft.rfft2: x [..., H, W] -> power float64 [windows, L / 2] (no missing-data rule: x has none)."""
    import torch

    h, w = x.shape[-2:]
    t = x.reshape(-1, h // window, window, w // window, window).permute(0, 1, 3, 2, 4).reshape(-1, window, window)
    out = torch.zeros(t.shape[0], window // 2 + 1, dtype=torch.float64, device=x.device)
    for part, dst in zip(t.split(512), out.split(512)):
        spec = torch.fft.rfft2(part)
        mag = (spec.real.double() ** 2 + spec.imag.double() ** 2) * weight
        dst.index_add_(1, bins, mag.reshape(part.shape[0], -1))
    return out[:, :window // 2]


def rfft_bins(window, device):
    """Bin (clamped to L / 2 for the dropped modes) and Hermitian weight of every entry of an rfft2 output [L, L / 2 + 1]."""
    import numpy as np
    import torch

    from skillful_nowcasting_amd.spectra import _radial_bins

    half = _radial_bins(window)[:, :window // 2 + 1]
    bins = np.minimum(half, window // 2).reshape(-1)
    weight = np.full((window, window // 2 + 1), 2.0)
    weight[:, 0] = 1.0
    weight[:, -1] = 0.0  # (the Nyquist column is dropped anyway)
    return torch.from_numpy(bins).to(device), torch.from_numpy(weight).to(device)


def timed(fns, repeats):
    """fns: {label: (callable, calls per window)} -> {label: [ms per call]}, alternating."""
    import torch

    times = {k: [] for k in fns}
    for _ in range(2):
        for fn, _n in fns.values():
            fn()
    torch.cuda.synchronize()
    for _ in range(repeats):
        for label, (fn, per) in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[label].append(t0.elapsed_time(t1) / per)
    return times


def summary(v, per):
    return {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v), "calls_per_window": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd.spectra import radial_psd
    from skillful_nowcasting_amd.value import exceedance_table

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/verify_extra_timing.py --repeats {a.repeats}",
           "window": WINDOW, "thresholds": list(THRESHOLDS), "assumed_rates": {"copy_bytes_per_s": COPY_BYTES_PER_S}, "shapes": {}}
    bins, weight = rfft_bins(WINDOW, dev)
    calls = 4
    for name, shape in SHAPES.items():
        f = radar_like(shape, gen, dev)
        o = radar_like(shape[1:], gen, dev)
        o[torch.rand(o.shape, device=dev, generator=gen) < 0.001] = -1.0
        row = {"shape": list(shape)}

        # ---- spectra of the ensemble ----
        nbytes = f.numel() * 4
        power, missing = radial_psd(f, WINDOW)
        fns = {"dgmr_radial_psd": (lambda: [radial_psd(f, WINDOW) for _ in range(calls)], calls)}
        torch_route = None
        try:
            want = torch_psd(f, WINDOW, bins, weight)
            torch.cuda.synchronize()
            gap = ((power.reshape(want.shape) - want).abs() / want.clamp_min(1e-300)).max()
            torch_route = {"max_rel_gap_to_kernel": float(gap), "missing_total": int(missing.sum())}
            del want
            fns["torch_rfft2_index_add"] = (lambda: torch_psd(f, WINDOW, bins, weight), 1)
        except Exception as e:  # (no FFT library for this device in the torch build, or not enough memory)
            torch_route = {"error": f"{type(e).__name__}: {e}"[:300]}
        times = timed(fns, a.repeats)
        psd = {"bytes_read_once": nbytes, "ms_at_copy_rate": nbytes / COPY_BYTES_PER_S * 1e3, "windows_of_256": int(missing.numel()),
               "workspace_bytes_moved": 2 * nbytes, "torch_route": torch_route}
        for label, v in times.items():
            psd[label] = summary(v, fns[label][1])
        psd["time_over_copy_rate_time"] = psd["dgmr_radial_psd"]["ms"] / psd["ms_at_copy_rate"]
        if "torch_rfft2_index_add" in psd:
            psd["torch_over_kernel"] = psd["torch_rfft2_index_add"]["ms"] / psd["dgmr_radial_psd"]["ms"]
        row["radial_psd"] = psd
        del power, missing

        # ---- exceedance table ----
        nbytes = (f.numel() + o.numel()) * 4
        times = timed({"dgmr_exceedance_table": (lambda: [exceedance_table(f, o, THRESHOLDS) for _ in range(calls)], calls)}, a.repeats)
        exc = {"bytes_read_once": nbytes, "ms_at_copy_rate": nbytes / COPY_BYTES_PER_S * 1e3,
               "dgmr_exceedance_table": summary(times["dgmr_exceedance_table"], calls)}
        exc["time_over_copy_rate_time"] = exc["dgmr_exceedance_table"]["ms"] / exc["ms_at_copy_rate"]
        exc["GB_per_s"] = nbytes / exc["dgmr_exceedance_table"]["ms"] / 1e6
        row["exceedance_table"] = exc
        rec["shapes"][name] = row
        print(f"{name:20s} {shape}: dgmr_radial_psd {psd['dgmr_radial_psd']['ms']:.3f} ms ({psd['time_over_copy_rate_time']:.1f} x the "
              f"{psd['ms_at_copy_rate']:.3f} ms of one read at the copy rate; torch route {psd.get('torch_rfft2_index_add', {}).get('ms')} ms, "
              f"{torch_route})   dgmr_exceedance_table {exc['dgmr_exceedance_table']['ms']:.3f} ms ({exc['time_over_copy_rate_time']:.1f} x, "
              f"{exc['GB_per_s']:.0f} GB/s)", flush=True)
        del f, o
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
