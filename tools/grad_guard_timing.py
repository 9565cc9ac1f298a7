"""Device time of FusedAdam.step() at the paper model's real parameter set, with and without the gradient guard.

    python tools/grad_guard_timing.py [--tree DIR] [--label NAME] [--reps 30] [--out FILE]
    python tools/grad_guard_timing.py --combine OUT.json RUN1.json RUN2.json ...

One run: DGMR() is built on the GPU, every parameter gets a random gradient (no forward), and step() of the generator's and of the
discriminator's optimiser is timed with HIP events in every state the tree under test offers - guard off; norm + clip; norm + clip +
skip - interleaved, state after state inside every repetition.  A ~10 ms matrix product is queued in front of every timed step so that
the host (which fills the descriptor table) is ahead of the device, as it is inside a training step: the events then bracket device
work only.  The norm pass (dgmr_grad_norm_multi) is also timed on its own, on the table of the last guarded step, and reported as
gradient bytes over time.  --tree: import the package from another checkout (a build of the parent commit, which has the first state
only); run the two trees alternately, process after process, and --combine the records (medians per state, ratios to the parent's
step).  Parameter counts are printed, not assumed.
"""
import argparse
import json
import os
import statistics
import sys


def combine(out, files):
    runs = [json.load(open(f)) for f in files]
    labels = sorted({r["label"] for r in runs})
    res = {"runs": runs, "summary": {}}
    for net in ("generator", "discriminator"):
        row = {"parameters": runs[0][net]["parameters"], "tensors": runs[0][net]["tensors"], "grad_bytes": runs[0][net]["grad_bytes"]}
        for label in labels:
            for state in ("off", "clip", "clip_skip", "norm_pass"):
                vals = [r[net][state]["median_us"] for r in runs if r["label"] == label and state in r[net]]
                if vals:
                    row[f"{label}.{state}.median_us"] = statistics.median(vals)
                    row[f"{label}.{state}.per_run_us"] = vals
        base = row.get("parent.off.median_us")
        if base:
            for state in ("off", "clip", "clip_skip"):
                if f"child.{state}.median_us" in row:
                    row[f"child.{state}.ratio_to_parent"] = row[f"child.{state}.median_us"] / base
        if "child.norm_pass.median_us" in row:
            row["norm_pass_TB_per_s"] = row["grad_bytes"] / (row["child.norm_pass.median_us"] * 1e-6) / 1e12
        res["summary"][net] = row
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res["summary"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="child")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=None)
    ap.add_argument("--combine", nargs="+", default=None)
    a = ap.parse_args()
    if a.combine:
        return combine(a.combine[0], a.combine[1:])
    sys.path.insert(0, os.path.abspath(a.tree))
    import inspect

    import torch

    import skillful_nowcasting_amd as S
    from skillful_nowcasting_amd.optim import FusedAdam

    assert torch.cuda.is_available(), "needs a HIP device"
    assert os.path.abspath(S.__file__).startswith(os.path.abspath(a.tree)), S.__file__
    guard = "max_grad_norm" in inspect.signature(FusedAdam.__init__).parameters
    torch.manual_seed(0)
    model = S.DGMR().to("cuda")
    g_opt, d_opt = model.optimizers()
    big = torch.randn(8192, 8192, device="cuda")
    rec = {"label": a.label, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    states = [("off", None, False)] + ([("clip", 1.0, False), ("clip_skip", 1.0, True)] if guard else [])
    for net, module, opt in (("generator", model.generator, g_opt), ("discriminator", model.discriminator, d_opt)):
        params = [p for p in module.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        n = sum(p.numel() for p in params)
        row = rec[net] = {"parameters": n, "tensors": len(params), "grad_bytes": 4 * n}
        print(f"{net}: {len(params)} tensors, {n} parameters, {4 * n / 2 ** 20:.1f} MiB of gradients")
        times = {s[0]: [] for s in states}

        def one(state):
            name, clip, skip = state
            if guard:
                opt.max_grad_norm, opt.skip_nonfinite = clip, skip
            torch.mm(big, big)  # the host gets ahead of the device
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            opt.step()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3

        for _ in range(5):  # warm-up: every state, every buffer allocated
            for s in states:
                one(s)
        for _ in range(a.reps):
            for s in states:
                times[s[0]].append(one(s))
        if guard:  # the norm pass alone, on the device table of the last guarded step
            from skillful_nowcasting_amd import ops

            d = opt.__dict__
            ring = d["_desc_ring"]
            table = ring[d["_desc_turn"] % len(ring)][1]
            chunk = d["_chunk"]
            blocks = sum((p.numel() + chunk - 1) // chunk for p in params)
            times["norm_pass"] = []
            for i in range(5 + a.reps):
                torch.mm(big, big)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                ops.call("dgmr_grad_norm_multi", table.data_ptr(), len(params), blocks, d["_partials"].data_ptr(), d["_tensor_sq"].data_ptr(),
                         1.0, 1, d["_guard"].data_ptr(), ops._stream())
                t1.record()
                t1.synchronize()
                if i >= 5:
                    times["norm_pass"].append(t0.elapsed_time(t1) * 1e3)
            row["norm_pass_TB_per_s"] = 4 * n / (statistics.median(times["norm_pass"]) * 1e-6) / 1e12
        for k, v in times.items():
            row[k] = {"median_us": statistics.median(v), "min_us": min(v), "max_us": max(v)}
            print(f"  {k:10s} median {row[k]['median_us']:8.1f} us  min {row[k]['min_us']:8.1f}  max {row[k]['max_us']:8.1f}")
        if guard:
            print(f"  norm pass: {row['norm_pass_TB_per_s']:.2f} TB/s of gradient bytes")
        for p in params:
            p.grad = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
