"""Device time of dgmr_ensemble_scores at the two shapes it is used at, next to a straightforward torch expression of the same outputs.

    python tools/verification_timing.py [--repeats 11] [--out profiles/verification_timing.json]

Shapes: one full-frame nowcast [6, 18, 1, 1536, 1280] (849 MB + a 141 MB observation) and a crop batch [6, 16, 18, 1, 256, 256]
(453 MB + 75 MB), scales (1, 4, 16), thresholds (1, 4, 8) mm/h, radar-like values (multiples of 1/32, ~70 % zeros, 0.1 % missing).
The kernel and the torch expression alternate on the same device; HIP events bracket windows of back-to-back calls on one stream;
after a warm-up the median over --repeats windows counts (minimum and maximum are listed).  Both inputs are larger than the 256 MiB
last-level cache, so every call streams them from HBM.

Bytes the kernel must move = (M + 1) * N * H * W * 4: every element of forecast and observed once (the per-workgroup partials and the
outputs are < 1 MB).  The torch expression forms the same five outputs with pooling calls, one temporary per member pair and scale,
comparisons and a bincount: it is what a user would write, and it is the yardstick - there is no earlier kernel to compare with.
Numbers are recorded, not asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALES, THRESHOLDS = (1, 4, 16), (1.0, 4.0, 8.0)
SHAPES = {"full_frame": (6, 18, 1, 1536, 1280), "crop_batch": (6, 16, 18, 1, 256, 256)}
HBM_BYTES_PER_S = 6.3e12  # achievable streaming rate (8 TB/s spec)


def torch_scores(f, o, scales, thr):
    """The five outputs in plain torch on the inputs' device: f [M, N, H, W], o [N, H, W] -> (cells, abs_err, pair, contingency, ranks)."""
    import torch
    import torch.nn.functional as F

    m, n = f.shape[:2]
    present = o >= 0
    cells, abs_err, pair = [], [], []
    for s in scales:
        pr = present if s == 1 else F.avg_pool2d(present.double().unsqueeze(1), s).squeeze(1) == 1.0
        cells.append(pr.sum(dim=(1, 2)))
        rows_a, rows_p = [], []
        for pool in (F.avg_pool2d, F.max_pool2d):
            x = f.double() if s == 1 else pool(f.double(), s)
            y = o.double() if s == 1 else pool(o.double().unsqueeze(1), s).squeeze(1)
            a = (x - y).abs().sum(dim=0) / m
            p = torch.zeros_like(a)
            for i in range(m):
                for j in range(i + 1, m):
                    p += (x[i] - x[j]).abs()
            rows_a.append(torch.where(pr, a, torch.zeros_like(a)).sum(dim=(1, 2)))
            rows_p.append(torch.where(pr, p, torch.zeros_like(p)).sum(dim=(1, 2)))
        abs_err.append(torch.stack(rows_a, dim=1))
        pair.append(torch.stack(rows_p, dim=1))
    cont = []
    for t in thr:
        wet = present & (o >= t)
        dry = present & ~wet
        ge, lt = f >= t, f < t
        cont.append(torch.stack([(ge & wet).sum(dim=(2, 3)), (lt & wet).sum(dim=(2, 3)), (ge & dry).sum(dim=(2, 3))], dim=-1).transpose(0, 1))
    key = (f < o).sum(dim=0) * (m + 1) + (f == o).sum(dim=0) + torch.arange(n, device=f.device).view(n, 1, 1) * (m + 1) ** 2
    ranks = torch.bincount(key[present], minlength=n * (m + 1) ** 2).view(n, m + 1, m + 1)
    return torch.stack(cells, dim=1), torch.stack(abs_err, dim=2), torch.stack(pair, dim=2), torch.stack(cont, dim=1), ranks


def radar_like(shape, gen, device):
    import torch

    x = torch.empty(shape, device=device)
    for part in x.view(-1, *shape[-2:]).split(64):
        v = torch.empty(part.shape, device=device).exponential_(0.25, generator=gen)
        v = torch.round(v * 32.0) / 32.0
        v[torch.rand(part.shape, device=device, generator=gen) < 0.7] = 0.0
        part.copy_(v)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import __graft_entry__ as g

    g.build()
    from skillful_nowcasting_amd.verification import ensemble_scores

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    rec = {"device": torch.cuda.get_device_name(0), "command": f"python tools/verification_timing.py --repeats {a.repeats}",
           "scales": list(SCALES), "thresholds": list(THRESHOLDS), "assumed_rates": {"hbm_bytes_per_s": HBM_BYTES_PER_S}, "shapes": {}}
    for name, shape in SHAPES.items():
        f = radar_like(shape, gen, dev)
        o = radar_like(shape[1:], gen, dev)
        o[torch.rand(o.shape, device=dev, generator=gen) < 0.001] = -1.0
        m, h, w = shape[0], shape[-2], shape[-1]
        n = f.numel() // (m * h * w)
        nbytes = (m + 1) * n * h * w * 4
        f4, o3 = f.view(m, n, h, w), o.view(n, h, w)
        calls = 4

        def kernel():
            for _ in range(calls):
                ensemble_scores(f, o, SCALES, THRESHOLDS)

        def expression():
            torch_scores(f4, o3, SCALES, THRESHOLDS)

        got = ensemble_scores(f, o, SCALES, THRESHOLDS)
        want = torch_scores(f4, o3, SCALES, THRESHOLDS)
        torch.cuda.synchronize()
        agree = {"counts_equal": bool(all(torch.equal(u, v) for u, v in ((got.cells, want[0]), (got.contingency, want[3]), (got.ranks, want[4])))),
                 "abs_err_max_rel_gap": float(((got.abs_err - want[1]).abs() / want[1].clamp_min(1e-300)).max()),
                 "pair_max_rel_gap": float(((got.pair - want[2]).abs() / want[2].clamp_min(1e-300)).max())}
        del want
        times = {"dgmr_ensemble_scores": [], "torch_expression": []}
        for _ in range(2):
            kernel()
            expression()
        torch.cuda.synchronize()
        for _ in range(a.repeats):
            for label, fn, per in (("dgmr_ensemble_scores", kernel, calls), ("torch_expression", expression, 1)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fn()
                t1.record()
                t1.synchronize()
                times[label].append(t0.elapsed_time(t1) / per)
        row = {"shape": list(shape), "planes": n, "bytes_to_move": nbytes, "ms_at_hbm_rate": nbytes / HBM_BYTES_PER_S * 1e3,
               "agreement_with_torch_expression": agree}
        for label, v in times.items():
            row[label] = {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "windows": len(v),
                          "calls_per_window": calls if label == "dgmr_ensemble_scores" else 1}
        row["dgmr_ensemble_scores"]["GB_per_s"] = nbytes / row["dgmr_ensemble_scores"]["ms"] / 1e6
        row["torch_over_kernel"] = row["torch_expression"]["ms"] / row["dgmr_ensemble_scores"]["ms"]
        rec["shapes"][name] = row
        print(f"{name:10s} {shape}: dgmr_ensemble_scores {row['dgmr_ensemble_scores']['ms']:.3f} ms ({row['dgmr_ensemble_scores']['GB_per_s']:.0f} "
              f"GB/s of {nbytes / 1e6:.0f} MB; {row['ms_at_hbm_rate']:.3f} ms at the HBM rate)   torch {row['torch_expression']['ms']:.1f} ms   "
              f"torch / kernel {row['torch_over_kernel']:.1f}   agreement {agree}", flush=True)
        del f, o, f4, o3, got
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
