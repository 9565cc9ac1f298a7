"""Device time of the Lucas-Kanade refinement beside the block matching it refines, on the frames of tools/advection_timing.py
(1536 x 1280, 3 pairs, block 32, stride 16, radius 8; skillful_nowcasting_amd/advection.py, csrc/advect.hip).

    python tools/lk_refine_timing.py [--repeats 11] [--out profiles/lk_refine_timing.json]

For the "rain-covered" and the "mostly dry" input of that tool, HIP events around windows of back-to-back calls on one stream, a
warm-up first, the median over --repeats windows (minimum and maximum listed):

  * dgmr_lk_refine alone (4 iterations, and 1 and 8 to separate the staging from the iterations), on the match of the same frames;
  * dgmr_block_match alone;
  * motion_field with subpixel="parabola" - the field of before, the yardstick - and with "lk";
  * one whole AdvectionNowcaster.nowcast (T = 18) with each.
The ratios lk / parabola and refinement / block matching are recorded.  Numbers are recorded, not asserted."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from advection_timing import BLOCK, H, RADIUS, STRIDE, T_OUT, W, rain_sequence, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd.advection import AdvectionNowcaster, block_match, lk_conditioned, lk_refine, motion_field

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/lk_refine_timing.py --repeats {a.repeats}",
           "frame": [H, W], "block_stride_radius": [BLOCK, STRIDE, RADIUS], "lead_times": T_OUT, "inputs": {}}
    calls = 4
    for name, masked in (("rain_covered", False), ("mostly_dry", True)):
        seq = rain_sequence(gen, dev, 4, (2, -3), masked)  # [4, H, W]
        prev, nxt = seq[:-1], seq[1:]
        match = block_match(prev, nxt, BLOCK, STRIDE, RADIUS)
        lk = lk_refine(prev, nxt, match, BLOCK, STRIDE)
        blocks = match.wet.numel()
        wet = torch.isfinite(match.cost[..., 0])
        row = {"blocks": blocks, "dry_block_share": 1.0 - int(wet.sum()) / blocks,
               "conditioned_share_of_wet": float(lk_conditioned(lk.eig)[wet].double().mean())}
        row["block_match_3_pairs"] = timed(lambda: [block_match(prev, nxt, BLOCK, STRIDE, RADIUS) for _ in range(calls)], calls, a.repeats)
        for it in (1, 4, 8):
            row[f"lk_refine_3_pairs_iterations_{it}"] = timed(
                lambda: [lk_refine(prev, nxt, match, BLOCK, STRIDE, it) for _ in range(calls)], calls, a.repeats)
        frames4 = seq[:, None]
        for method in ("parabola", "lk"):
            row[f"motion_field_{method}"] = timed(lambda: motion_field(frames4, BLOCK, STRIDE, RADIUS, subpixel=method), 1, a.repeats)
        frames = seq[..., None].contiguous()  # [T_in, H, W, C]
        for method in ("parabola", "lk"):
            nowcaster = AdvectionNowcaster(forecast_steps=T_OUT, block=BLOCK, stride=STRIDE, radius=RADIUS, subpixel=method)
            row[f"nowcast_{method}"] = timed(lambda: nowcaster.nowcast(frames), 1, a.repeats)
        row["ratios"] = {
            "lk_refine_over_block_match": row["lk_refine_3_pairs_iterations_4"]["ms"] / row["block_match_3_pairs"]["ms"],
            "motion_field_lk_over_parabola": row["motion_field_lk"]["ms"] / row["motion_field_parabola"]["ms"],
            "nowcast_lk_over_parabola": row["nowcast_lk"]["ms"] / row["nowcast_parabola"]["ms"]}
        rec["inputs"][name] = row
        print(f"{name:13s} dry blocks {row['dry_block_share']:.2f}: lk_refine {row['lk_refine_3_pairs_iterations_4']['ms']:.3f} ms, "
              f"block_match {row['block_match_3_pairs']['ms']:.3f} ms ({row['ratios']['lk_refine_over_block_match']:.3f} x)   "
              f"motion_field parabola {row['motion_field_parabola']['ms']:.3f} ms, lk {row['motion_field_lk']['ms']:.3f} ms "
              f"({row['ratios']['motion_field_lk_over_parabola']:.3f} x)   nowcast parabola {row['nowcast_parabola']['ms']:.3f} ms, "
              f"lk {row['nowcast_lk']['ms']:.3f} ms ({row['ratios']['nowcast_lk_over_parabola']:.3f} x)", flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
