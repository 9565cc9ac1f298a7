"""Device time of dgmr_fss_sums at the two shapes the verifiers are used at, next to a torch expression of the same sums.

    python tools/fss_timing.py [--repeats 11] [--out profiles/fss_timing.json]

Inputs: a full-frame ensemble [8, 18, 1, 1536, 1280] (1.13 GB + a 141 MB observation) and a crop ensemble [6, 16, 18, 1, 256, 256]
(453 MB + 75 MB), thresholds (1, 4, 8) mm/h, radii (0, 2, 8, 32), radar-like values (multiples of 1/32, ~70 % zeros, 0.1 % of the
observation missing).  HIP events bracket windows of back-to-back calls on one stream; after a warm-up the median over --repeats
windows counts (minimum and maximum are listed).  Both inputs are larger than the 256 MiB last-level cache.

Per call: the time, the bytes of one read of the inputs (elements * 4) and the ratio of the time to that traffic at the measured
6.29 TB/s copy rate - the kernel is not expected to reach it: it stages a halo of 32 pixels around every 64 x 64 tile and does
K * S * (M + 1) box sums per pixel.  The torch route is the specification's own method on the device: indicator fields as int32, a
zero-padded double cumulative sum, four slices per radius, products and sums in int64, per threshold; it is timed alternating with
the kernel and its result is compared with the kernel's (both are exact).  Numbers are recorded, not asserted; there is no earlier
kernel to compare with."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

THRESHOLDS, RADII = (1.0, 4.0, 8.0), (0, 2, 8, 32)
SHAPES = {"full_frame_ensemble": (8, 18, 1, 1536, 1280), "crop_ensemble": (6, 16, 18, 1, 256, 256)}
COPY_BYTES_PER_S = 6.29e12  # measured device-to-device copy rate of the MI355X (tools/verify_extra_timing.py uses the same)


def radar_like(shape, gen, device):
    import torch

    x = torch.empty(shape, device=device)
    for part in x.view(-1, *shape[-2:]).split(64):
        v = torch.empty(part.shape, device=device).exponential_(0.25, generator=gen)
        v = torch.round(v * 32.0) / 32.0
        v[torch.rand(part.shape, device=device, generator=gen) < 0.7] = 0.0
        part.copy_(v)
    return x


def torch_fss(f, o, thresholds, radii, planes_per_pass=96):
    """The same sums with torch operators: f [M, N, H, W], o [N, H, W] -> (sums int64 [N, K, S, 4], events int64 [N, K, 2])."""
    import torch
    import torch.nn.functional as nnf

    m, n = f.shape[:2]
    sums = torch.zeros((n, len(thresholds), len(radii), 4), dtype=torch.int64, device=f.device)
    events = torch.zeros((n, len(thresholds), 2), dtype=torch.int64, device=f.device)
    for lo in range(0, n, planes_per_pass):
        fp, op = f[:, lo:lo + planes_per_pass], o[lo:lo + planes_per_pass]
        present = op >= 0
        for k, t in enumerate(thresholds):
            fields = torch.cat([((fp >= t) & present).to(torch.int32), ((op >= t) & present).to(torch.int32)[None]])  # [M + 1, n, H, W]
            events[lo:lo + planes_per_pass, k, 0] = fields[:m].sum(dim=(0, 2, 3))
            events[lo:lo + planes_per_pass, k, 1] = fields[m].sum(dim=(1, 2))
            for s, r in enumerate(radii):
                if r == 0:
                    box = fields
                else:
                    side = 2 * r + 1
                    c = nnf.pad(fields, (r + 1, r, r + 1, r)).cumsum(dim=-2, dtype=torch.int32).cumsum(dim=-1, dtype=torch.int32)
                    box = c[..., side:, side:] - c[..., :-side, side:] - c[..., side:, :-side] + c[..., :-side, :-side]
                box = box.to(torch.int64)
                sf, so = box[:m].sum(dim=0), box[m]
                dst = sums[lo:lo + planes_per_pass, k, s]
                dst[:, 0], dst[:, 1] = (sf * sf).sum(dim=(1, 2)), (so * so).sum(dim=(1, 2))
                dst[:, 2], dst[:, 3] = (sf * so).sum(dim=(1, 2)), (box[:m] * box[:m]).sum(dim=(0, 2, 3))
    return sums, events


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
    from skillful_nowcasting_amd.fss import fss_sums

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/fss_timing.py --repeats {a.repeats}",
           "thresholds": list(THRESHOLDS), "radii": list(RADII), "assumed_rates": {"copy_bytes_per_s": COPY_BYTES_PER_S}, "shapes": {}}
    calls = 4
    for name, shape in SHAPES.items():
        f = radar_like(shape, gen, dev)
        o = radar_like(shape[1:], gen, dev)
        o[torch.rand(o.shape, device=dev, generator=gen) < 0.001] = -1.0
        m, (h, w) = shape[0], shape[-2:]
        f4, o3 = f.view(m, -1, h, w), o.view(-1, h, w)
        nbytes = (f.numel() + o.numel()) * 4
        row = {"shape": list(shape), "planes": int(o3.shape[0]), "bytes_read_once": nbytes, "ms_at_copy_rate": nbytes / COPY_BYTES_PER_S * 1e3}
        sums, events = fss_sums(f, o, THRESHOLDS, RADII)
        fns = {"dgmr_fss_sums": (lambda: [fss_sums(f, o, THRESHOLDS, RADII) for _ in range(calls)], calls)}
        try:
            want_sums, want_events = torch_fss(f4, o3, THRESHOLDS, RADII)
            torch.cuda.synchronize()
            row["torch_route"] = {"equal_to_kernel": bool(torch.equal(want_sums, sums) and torch.equal(want_events, events)),
                                  "events_forecast": int(events[..., 0].sum()), "events_observed": int(events[..., 1].sum())}
            del want_sums, want_events
            fns["torch_cumsum"] = (lambda: torch_fss(f4, o3, THRESHOLDS, RADII), 1)
        except Exception as e:  # (not enough memory for the int32 / int64 copies)
            row["torch_route"] = {"error": f"{type(e).__name__}: {e}"[:300]}
        times = timed(fns, a.repeats)
        for label, v in times.items():
            row[label] = summary(v, fns[label][1])
        row["time_over_copy_rate_time"] = row["dgmr_fss_sums"]["ms"] / row["ms_at_copy_rate"]
        if "torch_cumsum" in row:
            row["torch_over_kernel"] = row["torch_cumsum"]["ms"] / row["dgmr_fss_sums"]["ms"]
        rec["shapes"][name] = row
        print(f"{name:20s} {shape}: dgmr_fss_sums {row['dgmr_fss_sums']['ms']:.3f} ms ({row['time_over_copy_rate_time']:.1f} x the "
              f"{row['ms_at_copy_rate']:.3f} ms of one read at the copy rate); torch route {row.get('torch_cumsum', {}).get('ms')} ms, "
              f"{row['torch_route']}", flush=True)
        del f, o, f4, o3, sums, events
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
