"""Device time of dgmr_tile_blend at the operational shape, next to the torch expression it replaces, and what the tiling costs
inside one full-frame nowcast.

    python tools/tile_blend_timing.py [--repeats 21] [--out profiles/tile_blend_timing.json] [--no-nowcast]

Shape: K * T * C = 6 * 18 * 1 = 108 planes, a 256 x 256 tile into a 1536 x 1280 frame (stride 192: 8 x 7 = 56 tiles).  Two access
patterns, each timed for the kernel and for

    out[:, oy:oy + t, ox:ox + t] += (wy[:, None] * wx[None, :]) * pred

on the same device, alternating, with HIP events around a window of back-to-back launches on one stream; after a warm-up, the
median over --repeats windows of 3584 launches (60 - 120 ms each) counts (minimum and maximum are listed):

  * `sweep`: the 56 tiles of the frame in raster order, pred rotating through 8 buffers - what a nowcast does.  The frame's 849 MB
    do not stay in the 256 MiB last-level cache from one pass to the next.
  * `one_tile`: the same interior tile over and over (85 MB per launch: the cache-resident case, an upper bound).

Effective bandwidth = 3 * planes * tile^2 * 4 bytes (pred read, the covered part of out read and written) over the time.
Then one nowcast_full_frame at the paper configuration (default DGMR(), K = 6, on 4 x 1536 x 1280 x 1 int16 frames): its device and
host time, the summed device time of its 56 forward_draws calls, and the rest (context gathers, latent slices, blends) as the
tiling's share."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K, T_OUT, C, TILE, STRIDE, H, W = 6, 18, 1, 256, 192, 1536, 1280
PLANES = K * T_OUT * C
BYTES = 3 * PLANES * TILE * TILE * 4
HBM_BYTES_PER_S = 6.3e12  # achievable streaming rate (8 TB/s spec)
PRED_BUFFERS = 8
SWEEPS = 64  # passes over the frame per timed window: 3584 launches, 60 - 120 ms


def windows(fns, launches_per_call, repeats):
    """fns: {name: callable that issues `launches_per_call` launches}.  Warm-up, then `repeats` rounds in which every fn gets one
    event-bracketed window (alternating) -> {name: {"ms": median per launch, "min_ms", "max_ms", "windows"}}."""
    import torch

    for _ in range(3):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in fns}
    for _ in range(repeats):
        for name, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[name].append(t0.elapsed_time(t1) / launches_per_call)
    return {name: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v), "launches_per_window": launches_per_call}
            for name, v in times.items()}


def annotate(rec):
    for row in rec.values():
        row["bytes"] = BYTES
        row["GB_per_s"] = BYTES / row["ms"] / 1e6
        row["ms_at_hbm_rate"] = BYTES / HBM_BYTES_PER_S * 1e3
    rec["kernel_over_torch"] = rec["dgmr_tile_blend"]["ms"] / rec["torch_expression"]["ms"]
    rec["kernel_not_slower_than_torch"] = bool(rec["kernel_over_torch"] <= 1.0)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-nowcast", action="store_true")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd import tiling

    assert torch.cuda.is_available(), "needs a HIP device"
    ys, wy = tiling.blend_weights(H, TILE, STRIDE)
    xs, wx = tiling.blend_weights(W, TILE, STRIDE)
    wy, wx = torch.from_numpy(wy).cuda(), torch.from_numpy(wx).cuda()
    tiles = [(a_, oy, b_, ox) for a_, oy in enumerate(ys) for b_, ox in enumerate(xs)]
    gen = torch.Generator().manual_seed(0)
    preds = [torch.randn(PLANES, TILE, TILE, generator=gen).cuda() for _ in range(PRED_BUFFERS)]
    out = torch.zeros(PLANES, H, W, device="cuda")
    command = f"python tools/tile_blend_timing.py --repeats {a.repeats}" + (" --no-nowcast" if a.no_nowcast else "")  # (without --out)
    rec = {"device": torch.cuda.get_device_name(0), "command": command,
           "planes": PLANES, "tile": TILE, "stride": STRIDE, "frame": [H, W], "tiles": len(tiles), "bytes_per_launch": BYTES,
           "assumed_rates": {"hbm_bytes_per_s": HBM_BYTES_PER_S}}

    def kernel_sweep(sweeps=SWEEPS):
        for _ in range(sweeps):
            for n, (a_, oy, b_, ox) in enumerate(tiles):
                tiling.blend_tile(preds[n % PRED_BUFFERS], out, wy[a_], wx[b_], oy, ox)

    def torch_sweep(sweeps=SWEEPS):
        for _ in range(sweeps):
            for n, (a_, oy, b_, ox) in enumerate(tiles):
                out[:, oy:oy + TILE, ox:ox + TILE] += (wy[a_][:, None] * wx[b_][None, :]) * preds[n % PRED_BUFFERS]

    # the two forms agree (the torch expression rounds the product and the sum separately, the kernel fuses them: <= 1 ulp apart)
    kernel_sweep(1)
    want = out.clone()
    out.zero_()
    torch_sweep(1)
    rec["max_abs_difference_kernel_vs_torch"] = float((out - want).abs().max())
    rec["max_abs_pred"] = float(max(p.abs().max() for p in preds))
    del want
    rec["sweep"] = annotate(windows({"dgmr_tile_blend": kernel_sweep, "torch_expression": torch_sweep}, SWEEPS * len(tiles), a.repeats))
    a_, oy, b_, ox = tiles[len(xs) * 3 + 3]  # an interior tile: ramps on all four sides
    reps = SWEEPS * len(tiles)

    def kernel_one():
        for _ in range(reps):
            tiling.blend_tile(preds[0], out, wy[a_], wx[b_], oy, ox)

    def torch_one():
        for _ in range(reps):
            out[:, oy:oy + TILE, ox:ox + TILE] += (wy[a_][:, None] * wx[b_][None, :]) * preds[0]

    rec["one_tile"] = annotate(windows({"dgmr_tile_blend": kernel_one, "torch_expression": torch_one}, reps, a.repeats))
    for mode in ("sweep", "one_tile"):
        r = rec[mode]
        print(f"{mode:9s} dgmr_tile_blend {r['dgmr_tile_blend']['ms'] * 1e3:7.1f} us ({r['dgmr_tile_blend']['GB_per_s']:.0f} GB/s)   torch "
              f"{r['torch_expression']['ms'] * 1e3:7.1f} us ({r['torch_expression']['GB_per_s']:.0f} GB/s)   kernel / torch "
              f"{r['kernel_over_torch']:.3f}", flush=True)
    del preds, out
    torch.cuda.empty_cache()

    if not a.no_nowcast:
        import skillful_nowcasting_amd as S

        torch.manual_seed(0)
        model = S.DGMR().to("cuda").eval()
        frames = torch.randint(-32, 2048, (4, H, W, C), generator=gen, dtype=torch.int16).cuda()
        zs = tiling.latent_field(K, 8 * C, H // 32, W // 32, gen).cuda()
        buf = torch.empty(K, T_OUT, C, H, W, device="cuda")
        events = []

        def tile_fn(context, z):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            pred = model.generator.forward_draws(context, K, zs=z)
            t1.record()
            events.append((t0, t1))
            return pred

        runs = []
        with torch.no_grad():
            model.nowcast_full_frame(frames, zs=zs, scale=1 / 32, out=buf)  # warm-up through the public entry (kernel choices, caches)
            torch.cuda.synchronize()
            for _ in range(3):
                events.clear()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                h0 = time.perf_counter()
                t0.record()
                tiling.nowcast_tiled(tile_fn, frames, zs, TILE, STRIDE, T_OUT, 1 / 32, 0.0, True, 0.0, buf)
                t1.record()
                t1.synchronize()
                total = t0.elapsed_time(t1)
                fwd = sum(e0.elapsed_time(e1) for e0, e1 in events)
                runs.append({"device_ms": total, "host_ms": (time.perf_counter() - h0) * 1e3, "forward_draws_ms": fwd,
                             "forward_draws_calls": len(events), "tiling_ms": total - fwd, "tiling_share": (total - fwd) / total})
            h0 = time.perf_counter()
            model.nowcast_full_frame(frames, zs=zs, scale=1 / 32, out=buf)
            torch.cuda.synchronize()
            public_ms = (time.perf_counter() - h0) * 1e3
        runs.sort(key=lambda r: r["device_ms"])
        rec["nowcast_full_frame"] = {"config": "DGMR() defaults, K = 6, int16 frames 4 x 1536 x 1280 x 1, tile 256, stride 192",
                                     "median_run": runs[1], "runs": runs, "public_entry_host_ms_with_synchronise": public_ms,
                                     "finite": bool(torch.isfinite(buf).all())}
        m = runs[1]
        print(f"nowcast_full_frame: {m['device_ms']:.1f} ms on the device ({m['host_ms']:.1f} ms host), forward_draws x {m['forward_draws_calls']} "
              f"{m['forward_draws_ms']:.1f} ms, tiling {m['tiling_ms']:.1f} ms = {m['tiling_share']:.1%}; public entry {public_ms:.1f} ms", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
