"""Device time of the importance sampler's two kernels at the paper's full-frame size, next to the H2D copy they follow.

    python tools/crop_sampler_timing.py [--window-ms 400] [--out profiles/crop_sampler_timing.json] [--no-host]

One UK-size sequence (22 x 1536 x 1280 x 1, crop 256, stride 32: 41 x 33 candidates) in int16 (1/32 mm/h) and in uint8 (0.5 mm/h, 0 =
no data), as two fields: `radar` - rain under a few Gaussian systems, most of the frame dry, 1 % holes - and `soaked` - every pixel
wet, the score kernel's worst case (no element skips its exponential).  Timed with HIP events after a warm-up, each in a window of
at least --window-ms of back-to-back launches on one stream:

  * dgmr_crop_scores (both passes), with the bytes it must move (the sequence once; the grids are noise) and the fp64 work it must
    do (FP64_INSTR_PER_TERM instructions per wet element, counted in the kernel's ISA: the division, expm1's polynomial and the
    add), each as a time at the chip's rate - which of the two bounds the launch sits nearer to is the larger of them;
  * dgmr_crop_gather for 16 crops at spread-out origins (reads 16 crops in the storage dtype, writes them as fp32);
  * the H2D copy of the same sequence from pinned memory - the yardstick: the score kernel follows this copy for every row.

For orientation only, the numpy reference on the same host (one sequence, once), with the threads it really used (process CPU time
over wall time), not a core count."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, H, W, C, CROP, STRIDE, N_CROPS = 22, 1536, 1280, 1, 256, 32, 16
HBM_BYTES_PER_S = 6.3e12  # achievable streaming rate (8 TB/s spec)
FP64_INSTR_PER_S = 78.6e12 / 2  # spec vector FP64 rate, one fma = two flops
FP64_INSTR_PER_TERM = 40  # per wet element: 19 fma, 3 mul, 4 add, cvt / rndne / ldexp and the division's 6, in crop_cell_sums_kernel's ISA


def make_field(kind, rng):
    """-> mm/h, float32 [T, H, W, C]; holes as NaN."""
    if kind == "soaked":
        v = rng.gamma(0.5, 4.0, (T, H, W, C)).astype(np.float32) + 0.5
    else:
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        env = np.zeros((H, W), np.float32)
        for _ in range(5):
            cy, cx, sy, sx = rng.uniform(0, H), rng.uniform(0, W), rng.uniform(40, 160), rng.uniform(40, 160)
            env = np.maximum(env, np.exp(-0.5 * (((yy - cy) / sy) ** 2 + ((xx - cx) / sx) ** 2)))
        env = np.where(env < 0.1, 0.0, env)[None, :, :, None]
        v = (rng.gamma(0.5, 4.0, (T, H, W, C)) * (rng.random((T, H, W, C)) < 0.7)).astype(np.float32) * env
    v[rng.random((T, H, W, C)) < 0.01] = np.nan
    return v


def encode(v, dtype):
    hole = np.isnan(v)
    if dtype == "int16":
        return np.where(hole, -1, np.minimum(np.nan_to_num(v) * 32.0, 32000)).astype(np.int16), 1.0 / 32.0, 0.0
    return np.where(hole, 0, np.minimum(np.nan_to_num(v) * 2.0, 254) + 1).astype(np.uint8), 0.5, -0.5


def timed(fn, window_ms):
    """Warm up, size the repetition count to the window, then one pair of events around a whole window of back-to-back launches;
    three windows, the fastest counts (the others are listed)."""
    import torch

    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(5):
        fn()
    t1.record()
    t1.synchronize()
    reps = max(5, int(window_ms / max(t0.elapsed_time(t1) / 5, 1e-3)) + 1)
    windows = []
    for _ in range(3):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        windows.append(t0.elapsed_time(t1))
    return {"ms": min(windows) / reps, "launches_per_window": reps, "window_ms": windows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", type=float, default=400.0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd import data as D

    assert torch.cuda.is_available(), "needs a HIP device"
    gy, gx = (H - CROP) // STRIDE + 1, (W - CROP) // STRIDE + 1
    rec = {"device": torch.cuda.get_device_name(0), "sequence": [T, H, W, C], "crop": CROP, "stride": STRIDE, "candidates": [gy, gx],
           "gather_crops": N_CROPS, "assumed_rates": {"hbm_bytes_per_s": HBM_BYTES_PER_S, "fp64_instr_per_s": FP64_INSTR_PER_S,
                                                      "fp64_instr_per_wet_element": FP64_INSTR_PER_TERM}, "cases": {}}
    rng = np.random.default_rng(0)
    origins = np.stack([rng.integers(0, H - CROP + 1, N_CROPS), rng.integers(0, W - CROP + 1, N_CROPS)], axis=1)
    for kind in ("radar", "soaked"):
        v = make_field(kind, rng)
        for dtype in ("int16", "uint8"):
            raw, scale, offset = encode(v, dtype)
            x = raw.astype(np.float32) * np.float32(scale) + np.float32(offset)
            wet, missing = int((x > 0).sum()), int((~(x >= 0)).sum())
            pinned = torch.from_numpy(raw).pin_memory()
            dev = pinned.to("cuda", non_blocking=True)
            ws = (torch.empty((H // STRIDE, W // STRIDE), dtype=torch.float64, device="cuda"),
                  torch.empty((H // STRIDE, W // STRIDE), dtype=torch.int32, device="cuda"),
                  torch.empty((gy, gx), dtype=torch.float64, device="cuda"), torch.empty((gy, gx), dtype=torch.int32, device="cuda"))

            def scores():
                D.crop_scores(dev, scale, offset, 1.0, STRIDE, CROP, out=ws)

            dev_o = torch.from_numpy(origins.astype(np.int32)).to("cuda")
            out = torch.empty((N_CROPS, T, C, CROP, CROP), dtype=torch.float32, device="cuda")
            from skillful_nowcasting_amd._lib import call

            def gather():  # the entry point itself: the wrapper would add the origins' upload to every launch
                call("dgmr_crop_gather", dev.data_ptr(), {"uint8": 0, "int16": 1}[dtype], T, H, W, C, dev_o.data_ptr(), N_CROPS, CROP,
                     scale, offset, 1, 0.0, out.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))

            row = {"wet_elements": wet, "missing_elements": missing, "elements": int(raw.size), "sequence_bytes": int(raw.nbytes)}
            row["h2d_copy"] = timed(lambda: dev.copy_(pinned, non_blocking=True), a.window_ms)
            row["h2d_copy"]["GB_per_s"] = raw.nbytes / row["h2d_copy"]["ms"] / 1e6
            sc = row["crop_scores"] = timed(scores, a.window_ms)
            sc["bytes"] = int(raw.nbytes)
            sc["GB_per_s"] = raw.nbytes / sc["ms"] / 1e6
            sc["ms_at_hbm_rate"] = raw.nbytes / HBM_BYTES_PER_S * 1e3
            sc["ms_at_fp64_rate"] = wet * FP64_INSTR_PER_TERM / FP64_INSTR_PER_S * 1e3
            sc["nearer_bound"] = "fp64" if sc["ms_at_fp64_rate"] > sc["ms_at_hbm_rate"] else "hbm"
            sc["share_of_nearer_bound"] = max(sc["ms_at_fp64_rate"], sc["ms_at_hbm_rate"]) / sc["ms"]
            sc["ratio_to_h2d_copy"] = sc["ms"] / row["h2d_copy"]["ms"]
            ga = row["crop_gather"] = timed(gather, a.window_ms)
            ga["bytes"] = int(N_CROPS * T * C * CROP * CROP * (raw.itemsize + 4))
            ga["GB_per_s"] = ga["bytes"] / ga["ms"] / 1e6
            ga["ms_at_hbm_rate"] = ga["bytes"] / HBM_BYTES_PER_S * 1e3
            if not a.no_host and dtype == "int16":
                w0, c0 = time.perf_counter(), time.process_time()
                ref_s, ref_m = D.crop_scores_reference(raw, scale, offset, 1.0, STRIDE, CROP)
                w1, c1 = time.perf_counter(), time.process_time()
                row["host_reference"] = {"ms": (w1 - w0) * 1e3, "threads_measured": (c1 - c0) / (w1 - w0)}
                s, m = D.crop_scores(dev, scale, offset, 1.0, STRIDE, CROP)
                err = np.abs(s.cpu().numpy() - ref_s) / np.maximum(ref_s, 1e-300)
                row["host_reference"]["max_rel_difference_to_device"] = float(err.max())
                row["host_reference"]["missing_counts_equal"] = bool(np.array_equal(m.cpu().numpy(), ref_m))
            rec["cases"][f"{kind}.{dtype}"] = row
            print(f"{kind:6s} {dtype:5s} wet {wet / raw.size:5.1%}  h2d {row['h2d_copy']['ms']:7.3f} ms ({row['h2d_copy']['GB_per_s']:.1f} GB/s)  "
                  f"scores {sc['ms']:7.3f} ms ({sc['GB_per_s']:.0f} GB/s; hbm bound {sc['ms_at_hbm_rate']:.3f}, fp64 bound "
                  f"{sc['ms_at_fp64_rate']:.3f} ms; {sc['ratio_to_h2d_copy']:.3f} x the copy)  gather {ga['ms']:7.3f} ms ({ga['GB_per_s']:.0f} GB/s)"
                  + (f"  host reference {row['host_reference']['ms']:.0f} ms on {row['host_reference']['threads_measured']:.2f} threads"
                     if "host_reference" in row else ""), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
