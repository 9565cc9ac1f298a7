"""Device time of FusedAdam.step() at the paper model's real parameter sets in every mode, and of swap_ema().

    python tools/adam_timing.py [--tree DIR] [--label NAME] [--reps 30] [--out FILE]
    python tools/adam_timing.py --combine OUT.json RUN1.json RUN2.json ...

One run: DGMR() is built on the GPU, every parameter gets a random gradient (no forward), and step() of the generator's and of the
discriminator's optimiser is timed with HIP events in every state the tree under test offers - `off` (dgmr_adam_multi, 28 bytes per
element), `guard` (norm pass + dgmr_adam_multi_guarded: clip and skip on, 32 bytes), `ema` (dgmr_adam_multi_ema, 36 bytes), `guard+ema`
(40 bytes) and `swap` (swap_ema(): dgmr_swap_multi, 16 bytes) - interleaved, state after state inside every repetition.  A ~10 ms
matrix product is queued in front of every timed call so that the host (which fills the tables) is ahead of the device, as it is
inside a training step: the events then bracket device work only - ALL the device work of the call: the pinned table's copy
(10 - 12 KB) and the kernels, with the gaps between them.  (Buffers and shadows are allocated in the warm-up repetitions, not in a
timed one.)  --tree: import the package from another checkout (a build of the parent commit, which may offer fewer states); run the
two trees alternately, process after process, and --combine the records: medians per state, the parent's own run-to-run spread of
each state, ratios to the parent's `off`, and achieved TB/s.  That figure is the bytes the KERNELS move over the median time of the
whole CALL as bracketed above (table copy included), so it understates the kernels' own bandwidth a little, by the same few
microseconds in every state; the JSON says so under "TB_per_s_basis".  The condition a change of these kernels has to meet is
evaluated for every state both trees offer: the child's median not above the parent's by more than the parent's own runs differ.
Parameter counts are printed, not assumed.
"""
import argparse
import json
import os
import statistics
import sys

TB_PER_S_BASIS = ("bytes moved by the kernels (28 / 32 / 36 / 40 / 16 per element) divided by the HIP-event time of the whole step() / "
                  "swap_ema() call: pinned table copy + kernels, not the kernels alone")
# p m v read + written and g read; + g read again by the norm pass; + the shadow read + written; swap: p and shadow
BYTES_PER_ELEMENT = {"off": 28, "guard": 32, "ema": 36, "guard+ema": 40, "swap": 16}


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
        for state in BYTES_PER_ELEMENT:
            base, per_run = row.get(f"parent.{state}.median_us"), row.get(f"parent.{state}.per_run_us")
            if not base:
                continue
            row[f"parent.{state}.spread"] = (max(per_run) - min(per_run)) / base  # the parent's own run-to-run spread
            if f"child.{state}.median_us" in row:  # not SLOWER than the parent by more than the parent's own runs differ (faster is no regression)
                row[f"child.{state}.not_slower_than_parent_by_more_than_spread"] = (
                    row[f"child.{state}.median_us"] - base <= max(per_run) - min(per_run))
                row[f"child.{state}.ratio_to_parent_off"] = row[f"child.{state}.median_us"] / row["parent.off.median_us"]
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
    options = inspect.signature(FusedAdam.__init__).parameters
    has_guard, has_ema = "max_grad_norm" in options, "ema_decay" in options
    torch.manual_seed(0)
    model = S.DGMR().to("cuda")
    g_opt, d_opt = model.optimizers()
    big = torch.randn(8192, 8192, device="cuda")
    rec = {"label": a.label, "reps": a.reps, "TB_per_s_basis": TB_PER_S_BASIS, "device": torch.cuda.get_device_name(0)}
    states = ["off"] + (["guard"] if has_guard else []) + (["ema"] if has_ema else []) + (
        ["guard+ema"] if has_guard and has_ema else []) + (["swap"] if has_ema else [])
    for net, module, opt in (("generator", model.generator, g_opt), ("discriminator", model.discriminator, d_opt)):
        params = [p for p in module.parameters() if p.requires_grad]
        for p in params:
            p.grad = torch.randn_like(p) * 1e-3
        n = sum(p.numel() for p in params)
        row = rec[net] = {"parameters": n, "tensors": len(params)}
        print(f"{net}: {len(params)} tensors, {n} parameters")
        times = {s: [] for s in states}

        def one(state):
            if has_guard and state != "swap":
                opt.max_grad_norm, opt.skip_nonfinite = (1.0, True) if "guard" in state else (None, False)
            if has_ema and state != "swap":
                opt.ema_decay = 0.999 if "ema" in state else None
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
            print(f"  {k:9s} median {med:8.1f} us  min {min(v):8.1f}  max {max(v):8.1f}  {row[k]['TB_per_s']:.2f} TB/s")
        for p in params:
            p.grad = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
