"""Device time of the advection baseline on a full 1536 x 1280 composite (skillful_nowcasting_amd/advection.py, csrc/advect.hip).

    python tools/advection_timing.py [--repeats 11] [--out profiles/advection_timing.json]

Inputs: four context frames of a smooth rain field (white noise box-smoothed on the device, max(4 a - 1, 0) in multiples of 1/32)
moving by (2, -3) pixels per frame, once as it is ("rain-covered": about 40 % wet pixels, nearly every block searched) and once
under a large-scale mask that leaves most blocks dry ("mostly dry"; the share of dry blocks is read from the kernel's wet counts and
recorded).  HIP events bracket windows of back-to-back calls on one stream; after a warm-up the median over --repeats windows counts
(minimum and maximum are listed).

  * dgmr_block_match on the 3 consecutive pairs at block 32, stride 16, radius 8 (one launch), for both inputs, with the fused
    multiply-adds of the searched blocks per second;
  * dgmr_advect for T = 18 with the bytes it stores (T H W 4 = 141 MB) and the store rate reached, against the measured 6.29 TB/s
    copy rate;
  * one whole AdvectionNowcaster.nowcast (conversion, block matching, the lattice arithmetic in torch, advection).
Numbers are recorded, not asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, W, T_OUT, BLOCK, STRIDE, RADIUS = 1536, 1280, 18, 32, 16, 8
COPY_BYTES_PER_S = 6.29e12  # measured device-to-device copy rate of the MI355X


def box(a, width):
    """Box smoothing of the last two dimensions by prefix sums (periodic: the canvas is cut afterwards)."""
    import torch

    for dim in (-2, -1):
        n = a.shape[dim]
        ext = torch.cat([a.narrow(dim, n - width, width), a], dim=dim).cumsum(dim)
        a = (ext.narrow(dim, width, n) - ext.narrow(dim, 0, n)) / width
    return a


def rain_sequence(gen, device, frames, v, masked):
    import torch

    m = 64
    a = torch.randn(H + 2 * m, W + 2 * m, device=device, generator=gen, dtype=torch.float64)
    for _ in range(3):
        a = box(a, 9)
    a = a / a.std()
    field = torch.round((4.0 * a - 1.0).clamp_min(0.0) * 32.0) / 32.0
    if masked:
        b = torch.randn(a.shape, device=device, generator=gen, dtype=torch.float64)
        for _ in range(3):
            b = box(b, 129)
        field = field * (b > b.flatten()[::97].quantile(0.75))
    field = field.float()
    return torch.stack([field[m - t * v[0]:m - t * v[0] + H, m - t * v[1]:m - t * v[1] + W] for t in range(frames)]).contiguous()


def timed(fn, per, repeats):
    import torch

    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1) / per)
    return {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "windows": len(times), "calls_per_window": per}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd.advection import AdvectionNowcaster, advect, block_match, lattice_geometry, motion_field

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/advection_timing.py --repeats {a.repeats}",
           "frame": [H, W], "block_stride_radius": [BLOCK, STRIDE, RADIUS], "lead_times": T_OUT,
           "assumed_rates": {"copy_bytes_per_s": COPY_BYTES_PER_S}, "inputs": {}}
    calls = 4
    for name, masked in (("rain_covered", False), ("mostly_dry", True)):
        seq = rain_sequence(gen, dev, 4, (2, -3), masked)  # [4, H, W]
        prev, nxt = seq[:-1], seq[1:]
        res = block_match(prev, nxt, BLOCK, STRIDE, RADIUS)
        blocks = res.wet.numel()
        searched = int((res.wet >= BLOCK * BLOCK // 16).sum())
        row = {"wet_pixel_share": float((seq > 0).double().mean()), "blocks": blocks, "dry_block_share": 1.0 - searched / blocks}
        bm = timed(lambda: [block_match(prev, nxt, BLOCK, STRIDE, RADIUS) for _ in range(calls)], calls, a.repeats)
        fma = searched * (2 * RADIUS + 1) ** 2 * BLOCK * BLOCK  # (an upper count: edge blocks have fewer candidates)
        bm["fma_per_call"] = fma
        bm["Tfma_per_s"] = fma / bm["ms"] / 1e9
        row["block_match_3_pairs"] = bm

        field = motion_field(seq[:, None], BLOCK, STRIDE, RADIUS)
        origin, spacing = lattice_geometry(BLOCK, STRIDE)
        out = torch.empty(1, T_OUT, H, W, device=dev)
        nbytes = out.numel() * 4
        adv = timed(lambda: [advect(seq[-1:], field, T_OUT, origin, spacing, out=out) for _ in range(calls)], calls, a.repeats)
        adv.update({"bytes_stored": nbytes, "GB_per_s": nbytes / adv["ms"] / 1e6, "ms_at_copy_rate": nbytes / COPY_BYTES_PER_S * 1e3,
                    "mean_speed_px_per_frame": float(field.norm(dim=-1).mean())})
        adv["time_over_copy_rate_time"] = adv["ms"] / adv["ms_at_copy_rate"]
        row["advect_T18"] = adv

        frames = seq[..., None].contiguous()  # [T_in, H, W, C]
        nowcaster = AdvectionNowcaster(forecast_steps=T_OUT, block=BLOCK, stride=STRIDE, radius=RADIUS)
        row["nowcast"] = timed(lambda: nowcaster.nowcast(frames), 1, a.repeats)
        rec["inputs"][name] = row
        print(f"{name:13s} dry blocks {row['dry_block_share']:.2f}: block_match (3 pairs) {bm['ms']:.3f} ms ({bm['Tfma_per_s']:.2f} Tfma/s)   "
              f"advect T=18 {adv['ms']:.3f} ms ({adv['GB_per_s']:.0f} GB/s stored, {adv['time_over_copy_rate_time']:.1f} x the copy-rate time)   "
              f"nowcast {row['nowcast']['ms']:.3f} ms", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
