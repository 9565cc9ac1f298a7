"""Device time of FusedAdam.step() at the paper model's real parameter sets with the weight EMA off and on, and of swap_ema().

    python tools/ema_timing.py [--tree DIR] [--label NAME] [--reps 30] [--out FILE]
    python tools/ema_timing.py --combine OUT.json RUN1.json RUN2.json ...

One run, in the manner of tools/grad_guard_timing.py: DGMR() is built on the GPU, every parameter gets a random gradient (no forward),
and step() of the generator's and of the discriminator's optimiser is timed with HIP events in every state the tree under test offers -
`off` (dgmr_adam_multi, 28 bytes per element), `ema` (dgmr_adam_multi_ema, 36 bytes per element) and `swap` (swap_ema(): dgmr_swap_multi,
16 bytes per element) - interleaved, state after state inside every repetition.  A ~10 ms matrix product is queued in front of every
timed call so that the host (which fills the tables) is ahead of the device, as it is inside a training step: the events then bracket
device work only - ALL the device work of the call: the pinned table's copy (10 - 12 KB) and the kernel, with the gap between
them.  (The shadows are cloned in the warm-up repetitions, not in a timed one.)  --tree: import the package from another checkout (a build of the parent commit, which
has the `off` state only); run the two trees alternately, process after process, and --combine the records: medians per state, the
parent's own run-to-run spread of `off`, ratios to the parent's `off`, and achieved TB/s.  That figure is the bytes the KERNEL moves
over the median time of the whole CALL as bracketed above (table copy included), so it understates the kernel's own bandwidth a
little, by the same few microseconds in every state; the JSON says so under "TB_per_s_basis".  The two conditions a change of these
kernels has to meet are evaluated too: the child's `off` within the parent's spread, and the fused launch's TB/s not below the
child's plain launch's by more than that spread.  Parameter counts are printed, not assumed.
"""
import argparse
import json
import os
import statistics
import sys

TB_PER_S_BASIS = ("bytes moved by the kernel (28 / 36 / 16 per element) divided by the HIP-event time of the whole step() / swap_ema() call: "
                  "pinned table copy + kernel, not the kernel alone")
BYTES_PER_ELEMENT = {"off": 28, "ema": 36, "swap": 16}  # p m v read + written and g read; + the shadow read + written; p and shadow


def combine(out, files):
    runs = [json.load(open(f)) for f in files]
    labels = sorted({r["label"] for r in runs})
    res = {"TB_per_s_basis": TB_PER_S_BASIS, "runs": runs, "summary": {}}
    for net in ("generator", "discriminator"):
        n = runs[0][net]["parameters"]
        row = {"parameters": n, "tensors": runs[0][net]["tensors"]}
        for label in labels:
            for state, nbytes in BYTES_PER_ELEMENT.items():
                vals = [r[net][state]["median_us"] for r in runs if r["label"] == label and state in r[net]]
                if vals:
                    med = statistics.median(vals)
                    row[f"{label}.{state}.median_us"] = med
                    row[f"{label}.{state}.per_run_us"] = vals
                    row[f"{label}.{state}.TB_per_s"] = nbytes * n / (med * 1e-6) / 1e12
        base = row.get("parent.off.median_us")
        if base:
            per_run = row["parent.off.per_run_us"]
            row["parent.off.spread"] = (max(per_run) - min(per_run)) / base  # the parent's own run-to-run spread
            for state in BYTES_PER_ELEMENT:
                if f"child.{state}.median_us" in row:
                    row[f"child.{state}.ratio_to_parent_off"] = row[f"child.{state}.median_us"] / base
            if "child.off.median_us" in row:  # not SLOWER than the parent by more than the parent's own runs differ (faster is no regression)
                row["child.off.not_slower_than_parent_by_more_than_spread"] = row["child.off.median_us"] - base <= max(per_run) - min(per_run)
        if "child.ema.TB_per_s" in row and "child.off.TB_per_s" in row:
            row["ema_bandwidth_over_off"] = row["child.ema.TB_per_s"] / row["child.off.TB_per_s"]
            if "parent.off.spread" in row:
                row["ema_bandwidth_not_below_off_by_more_than_spread"] = row["ema_bandwidth_over_off"] >= 1.0 - row["parent.off.spread"]
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
    has_ema = "ema_decay" in inspect.signature(FusedAdam.__init__).parameters
    torch.manual_seed(0)
    model = S.DGMR().to("cuda")
    g_opt, d_opt = model.optimizers()
    big = torch.randn(8192, 8192, device="cuda")
    rec = {"label": a.label, "reps": a.reps, "TB_per_s_basis": TB_PER_S_BASIS, "device": torch.cuda.get_device_name(0)}
    states = ["off"] + (["ema", "swap"] if has_ema else [])
    for net, module, opt in (("generator", model.generator, g_opt), ("discriminator", model.discriminator, d_opt)):
        params = [p for p in module.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        n = sum(p.numel() for p in params)
        row = rec[net] = {"parameters": n, "tensors": len(params)}
        print(f"{net}: {len(params)} tensors, {n} parameters")
        times = {s: [] for s in states}

        def one(state):
            if has_ema:
                opt.ema_decay = 0.999 if state == "ema" else None
            torch.mm(big, big)  # the host gets ahead of the device
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            if state == "swap":
                opt.swap_ema()
            else:
                opt.step()
            t1.record()
            t1.synchronize()
            return t0.elapsed_time(t1) * 1e3

        for _ in range(6):  # warm-up: every state, every buffer and shadow allocated (an even number of swaps)
            for s in states:
                one(s)
        for _ in range(a.reps + a.reps % 2):
            for s in states:
                times[s].append(one(s))
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"median_us": med, "min_us": min(v), "max_us": max(v), "TB_per_s": BYTES_PER_ELEMENT[k] * n / (med * 1e-6) / 1e12}
            print(f"  {k:5s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  {row[k]['TB_per_s']:.2f} TB/s")
        for p in params:
            p.grad = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
