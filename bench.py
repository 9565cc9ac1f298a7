#!/usr/bin/env python
"""bench.py — radar frames/s of the DGMR training step on MI355X.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A "step" is one `DGMR.training_step` (2 discriminator passes + 1 generator pass over `generation_steps`
draws + both Adam updates) on one synthetic batch that is resident in HBM before the timed region.
Workload = BASELINE.json configs[2] ("paper config: 4 in -> 18 out, 256x256, latent=768"), the configuration the
metric "radar frames/sec (G+D step) 4->18 @256^2" is quoted on; per-GPU batch fixed (weak scaling).
Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line (headline, `ms_per_step`, config, memory).  `--full` adds
everything else the bench measures, after the timed steps: the live HIP-event roofline step, the other arithmetic modes and the
fast-semantics leg (`also`), the CPU baseline, and the full record in a side file (`--detail`).
`--dump-outputs DIR` writes what the last timed step computed - its losses and the model state it updated - as DIR/<name>.npy.
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
# (before anything initialises HIP: see skillful_nowcasting_amd/__init__.py - streams beyond the runtime's default of four hardware
#  queues share one, which serialised the weight-gradient stream with the main chain whenever a process group existed; one process per
#  GPU only - never where several processes share a device)
if int(os.environ.get("WORLD_SIZE", "1") or 1) > 1 or "--force-dist" in sys.argv:
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")

PEAK_F32_MFMA_TFLOPS = 157.3  # /opt/skills/guides/MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 dense peak
PEAK_BF16_MFMA_TFLOPS = 2500.0  # same guide: v_mfma_f32_32x32x16_bf16 dense peak
# algorithmic TFLOP of one training_step per sample, F_step = 20 F_g + 30 F_d
F_STEP_TFLOP = {"paper": 11.50, "cfg2": 1.20, "cfg5": 46.0}
DTYPE_TEXT = {
    "f32": "f32 (exact: v_mfma_f32_32x32x2_f32; the reference's arithmetic)",
    "bf16x6": "bf16x6 (fp32 tensors; operands split into three bf16 planes, six bf16 MFMAs per product: fp32-faithful products, fp32 accumulate)",
    "mixed": "mixed: bf16x3 (fp32 tensors; operands split into two bf16 planes, three MFMAs per product: products carry 16 significant "
             "bits, fp32 accumulate) for the generator and every backward pass, bf16x6 (fp32-faithful products) for the discriminator forward",
    "bf16x3": "bf16x3 (fp32 tensors; two bf16 planes per operand, three MFMAs per product: 16-bit products, NOT fp32 arithmetic; fp32 accumulate)",
    "bf16": "bf16 operands, fp32 accumulate",
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("DGMR_BENCH_BATCH", "16")), help="per-GPU batch")
    ap.add_argument("--workload", default="paper", choices=["paper", "cfg2", "cfg5", "smoke"])
    ap.add_argument("--fast", action="store_true", help="strict_reference_semantics=False (skip discarded work)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also measure the roofline, the `also` legs and the CPU baseline and write the detail "
                         "file (a plain run does none of these)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write the losses and the model state of the last timed step as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--cpu-baseline", default="sample", choices=["sample", "off", "only"],
                    help="with --full: sample = time the CPU baseline; only = the CPU baseline alone, no GPU (needs no --full)")
    ap.add_argument("--no-roofline", action="store_true", help="with --full: skip the roofline step")
    ap.add_argument("--tune", default="", help="A/B switch for kernel development: variant,ksplit,window,wgrad_window for "
                                               "dgmr_conv_tune (-1 = the library's own choice, the default)")
    ap.add_argument("--precision", default=os.environ.get("DGMR_PRECISION", "mixed"), choices=["f32", "bf16x6", "mixed", "bf16x3", "bf16"],
                    help="arithmetic of the conv contractions (tensors stay fp32 in HBM, fp32 accumulation): f32 exact | bf16x6 "
                         "fp32-faithful products on the bf16 pipe | mixed (default) = bf16x3 (16-bit products) with the discriminator "
                         "forward in bf16x6 | bf16x3 | bf16")
    ap.add_argument("--also", default="auto", choices=["auto", "on", "off"],
                    help="with --full: also time the same build in the other arithmetic modes and report them in an `also` block: exact "
                         "f32 (the reference's arithmetic: >= 10 steps after 3 warm-ups, with its own roofline block), bf16x6 and plain "
                         "bf16 (a few steps each); auto = on for single-GPU runs")
    ap.add_argument("--also-f32-steps", type=int, default=10)
    ap.add_argument("--detail", default="", help="with --full: side file for the full record (default bench_out/bench_detail.json, "
                                                 "relative to the repo)")
    ap.add_argument("--force-dist", action="store_true",
                    help="with --gpus 1: still create the RCCL process group (world 1), attach the gradient exchange with "
                         "force_exchange so that every bucket goes through ncclAllReduce and the buffers through ncclBroadcast")
    return ap.parse_args()


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` without a launcher: run N ranks (one per GPU, RCCL) under torch.distributed.run in a child process
    and exit with its status."""
    import socket

    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd))


WORKLOADS = {
    # name: (DGMR kwargs, H=W, T)
    "paper": (dict(forecast_steps=18, output_shape=256, latent_channels=768, context_channels=384, generation_steps=6), 256, 18),
    "cfg2": (dict(forecast_steps=4, output_shape=256, latent_channels=384, context_channels=192, generation_steps=6), 256, 4),
    "cfg5": (dict(forecast_steps=18, output_shape=512, latent_channels=768, context_channels=384, generation_steps=6), 512, 18),
    "smoke": (dict(forecast_steps=2, output_shape=128, latent_channels=384, context_channels=192, generation_steps=2), 128, 2),
}


def _cpu_threads():
    import torch

    # torch's CPU convolutions scale badly past a few tens of threads on these shapes: on the 2x EPYC 9575F GPU box one paper-config
    # generator forward takes 0.88 / 0.75 / 2.13 / 3.80 / 8.70 s at 8 / 16 / 32 / 64 / 128 threads (tools/cpu_threads_probe.py), so
    # the baseline runs at the best setting rather than at torch's default (all cores)
    threads = int(os.environ.get("DGMR_CPU_BASELINE_THREADS", "16"))
    torch.set_num_threads(max(1, min(threads, os.cpu_count() or 1)))
    return torch.get_num_threads()


def cpu_baseline_reference(kw, hw, T):
    """The UNMODIFIED reference (`oracle/_ref/dgmr`, staged byte for byte from /root/reference/dgmr by oracle/make_ref.py) timed on
    THIS host: whole `DGMR.training_step` calls (dgmr/dgmr.py:137-218) at the bench's model configuration and batch 1, through the
    stand-ins of oracle/_stubs.py for the three packages the image lacks (pytorch_lightning's LightningModule -> nn.Module with
    manual_backward / optimizers / log_dict, torchvision, pytorch_msssim: none of them does arithmetic on this path).  One step AS
    WRITTEN (torch.autograd.set_detect_anomaly(True), dgmr.py:130) runs first; a second, warmed-up one with anomaly detection off is `value`.
    Returns None when oracle/_ref is absent."""
    ref_root = os.path.join(ROOT, "oracle", "_ref")
    if not os.path.isdir(os.path.join(ref_root, "dgmr")):
        return None
    import torch

    from oracle import _stubs

    _stubs.install(ref_root)
    import dgmr as ref  # the reference's own package

    assert os.path.realpath(ref.__file__).startswith(os.path.realpath(ref_root)), ref.__file__
    cores = _cpu_threads()
    torch.manual_seed(0)
    model = ref.DGMR(**kw)  # (sets anomaly detection on, globally, as the reference does)
    model.train()
    x = torch.rand(1, 4, 1, hw, hw)
    y = torch.rand(1, T, 1, hw, hw)
    with torch.no_grad():
        model(x)  # warm-up: thread pool, oneDNN primitive caches (advances u / v like any forward)
    # "best setting" made checkable: the reference's generator forward (no grad) timed at a few thread counts on THIS host, second of two
    # calls each; the step below runs at the fastest of them (DGMR_CPU_BASELINE_THREADS pins one count and skips the probe)
    probe = {}
    if "DGMR_CPU_BASELINE_THREADS" not in os.environ:
        for n in (8, 16, 32, 64):
            if n > (os.cpu_count() or 1):
                break
            torch.set_num_threads(n)
            with torch.no_grad():
                model(x)
                t0 = time.perf_counter()
                model(x)
                probe[n] = round(time.perf_counter() - t0, 2)
        if probe:
            cores = min(probe, key=probe.get)
        torch.set_num_threads(cores)
    times = {}
    # the step AS WRITTEN (anomaly detection on, dgmr.py:130) runs first and absorbs what is left of the one-off warm-up; the warmed-up
    # step with anomaly detection off is the faster of the two and is `value` (the conservative baseline for any speed-up quoted)
    for label, anomaly in (("as_written_anomaly_on", True), ("anomaly_off", False)):
        torch.autograd.set_detect_anomaly(anomaly)
        t0 = time.perf_counter()
        model.training_step((x, y), 0)
        times[label] = time.perf_counter() - t0
    torch.autograd.set_detect_anomaly(False)
    t_step = times["anomaly_off"]
    return {
        "value": (4 + T) / t_step, "unit": "radar frames/s", "cores": cores, "kind": "reference", "host_cpus": os.cpu_count(),
        "seconds_per_step": {k: round(v, 2) for k, v in times.items()},
        "threads_probe_generator_forward_s": probe,
        "value_as_written_anomaly_on": (4 + T) / times["as_written_anomaly_on"],
        "sample": f"unmodified reference DGMR.training_step (dgmr/dgmr.py:137-218, staged by oracle/make_ref.py), torch-CPU fp32, batch 1, "
                  f"{cores} of {os.cpu_count()} host threads: 1 step as written (anomaly detection on, {times['as_written_anomaly_on']:.1f} s), "
                  f"then 1 warmed-up step with it off ({t_step:.1f} s) = value; no extrapolation",
    }


def cpu_baseline(kw, hw, T):
    """Oracle (CPU restatement of the reference, `kind: port`) timed on this host on a bounded sample: ONE whole
    `training_step` (oracle.training_step = dgmr/dgmr.py:137-218 as written: 17 generator forwards, 8 generator backwards, 16
    discriminator sequence forwards and backwards, both Adam updates) at the bench's model configuration and batch 1.
    frames/s = (4 + T) / t_step.  Used only when the staged reference (cpu_baseline_reference) is absent."""
    import torch

    import skillful_nowcasting_amd as S
    from oracle import dgmr_oracle as O

    cores = _cpu_threads()
    torch.manual_seed(0)
    model = S.DGMR(**kw)
    sd = {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(("generator.", "discriminator."))}
    del model
    x = torch.rand(1, 4, 1, hw, hw)
    y = torch.rand(1, T, 1, hw, hw)
    z = O.draw_latent((8, hw // 32, hw // 32))
    with torch.no_grad():
        O.generator(sd, "generator.", x, z, T, True)  # warm-up (thread pool, oneDNN primitive caches)
    hp = dict(forecast_steps=T, generation_steps=kw.get("generation_steps", 6), grid_lambda=20.0, gen_lr=5e-5, disc_lr=2e-4, beta1=0.0,
              beta2=0.999, precip_weight_cap=24.0, latent_shape=(8, hw // 32, hw // 32), num_spatial_frames=8)
    t0 = time.perf_counter()
    O.training_step(sd, x, y, hp, {"step": {}, "m": {}, "v": {}})
    t_step = time.perf_counter() - t0
    return {
        "value": (4 + T) / t_step, "unit": "radar frames/s", "cores": cores, "kind": "port",
        "host_cpus": os.cpu_count(),
        "sample": f"oracle.training_step (torch-CPU fp32 restatement of the reference's step, as written: 17 G fwd, 8 G bwd, 16 D "
                  f"seq fwd+bwd, 2 Adam) at its best thread count on this host, batch 1, ONE measured step of {t_step:.1f} s (no "
                  f"extrapolation); oracle/_ref (the staged reference package) was not present",
    }


# the UNMODIFIED reference (openclimatefix/skillful_nowcasting v1.4.4) timed in the build container, which is the only
# place /root/reference exists (it cannot travel to the GPU box); carried next to the oracle's `port` timing, labelled as such
REFERENCE_MEASURED = {
    "paper": {"value": 0.23, "range": [0.22, 0.24], "unit": "radar frames/s", "cores": 8, "batch": 1,
              "what": "unmodified reference DGMR.training_step, torch-CPU fp32, 90.5-98.6 s/step",
              "where": "build container, Intel Xeon 2.10 GHz 8 cores (BASELINE.md); not this host"},
    "cfg2": {"value": 0.30, "range": [0.28, 0.31], "unit": "radar frames/s", "cores": 8, "batch": 1,
             "what": "unmodified reference DGMR.training_step, torch-CPU fp32, 25.8-28.4 s/step",
             "where": "build container, Intel Xeon 2.10 GHz 8 cores (BASELINE.md); not this host"},
}


LINE_LIMIT = 6000  # bytes: the driver keeps an 8 KB tail of stdout; round 4's 52 KB line did not parse
DTYPE_SHORT = {
    "f32": "f32 (exact fp32 MFMA)",
    "bf16x6": "bf16x6 (fp32 tensors, 3 bf16 planes, 6 MFMAs/product, fp32 accumulate)",
    "mixed": "mixed (fp32 tensors + accumulate; bf16x3 = 2 bf16 planes, 3 MFMAs/product, 16-bit products; discriminator forward bf16x6)",
    "bf16x3": "bf16x3 (fp32 tensors, 2 bf16 planes, 3 MFMAs/product: 16-bit products, fp32 accumulate)",
    "bf16": "bf16 operands, fp32 accumulate",
}


def _r(v, sig=4):
    """floats to `sig` significant digits (the line is a summary; full precision lives in the detail file)"""
    if isinstance(v, float):
        return float(f"{v:.{sig}g}")
    if isinstance(v, dict):
        return {k: _r(x, sig) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [_r(x, sig) for x in v]
    return v


def _roof_compact(roof, top=8):
    if not roof:
        return None
    keep = ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic", "mfma_executed_frac", "mfma_util",
            "mfma_util_weighted", "valu_per_mfma", "launches_per_step", "avg_launch_us", "flops_per_launch")
    out = {k: roof.get(k) for k in keep if k in roof}
    for k in ("pmc_source", "mfma_util_weighted_source"):
        if roof.get(k):
            out[k] = roof[k]
    ws = roof.get("whole_step") or {}
    out["whole_step"] = {"tflops": ws.get("tflops"), "frac": ws.get("frac")}
    ack = roof.get("all_conv_kernels") or {}
    out["all_conv_kernels"] = {k: ack.get(k) for k in ("tflops", "ms_per_step", "executed_conv_tflop_per_step")}
    rows = sorted(roof.get("per_kernel") or [], key=lambda r: -r["total_ms"])[:top]
    out["top_rows"] = [[r["kernel"], r["launches"], r["total_ms"], r["tflops"]] for r in rows if r["launches"]]
    out["top_rows_cols"] = "kernel class, launches, total_ms, TFLOP/s"
    return out


def compact_line(full, detail_path=None, limit=LINE_LIMIT):
    """The ONE JSON line of the bench contract, bounded in size: headline, config, dominant-kernel roofline with the <= 8 biggest
    class rows, the other arithmetic modes as one number each, the CPU baseline.  Everything else (`per_kernel_detail`, per-step
    times, the PMC launch record) goes to the side file `detail_path`.  Optional blocks are dropped in a fixed order should the
    line still exceed `limit` bytes."""
    out = {k: full.get(k) for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "ms_per_step_median",
                                    "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "hbm") if k in full}
    for k in ("replicas_in_sync", "wgrad_tail_balance"):
        if k in full:
            out[k] = full[k]
    pg = full.get("process_group")
    if pg:
        out["process_group"] = {k: pg.get(k) for k in ("backend", "world_size_reported", "rccl_version", "forced_single_rank", "late_buckets_per_step",
                                                       "dist_overhead_ms") if k in pg}
        gs = pg.get("grad_sync")
        if isinstance(gs, dict):
            out["process_group"]["grad_sync"] = {k: v for k, v in gs.items() if isinstance(v, (int, float, str, bool))}
    if full.get("roofline"):
        out["roofline"] = _roof_compact(full["roofline"])
    if full.get("also"):
        out["also"] = {}
        for mode, leg in full["also"].items():
            c = {"ms_per_step": leg.get("ms_per_step"), "radar_frames_per_s": leg.get("radar_frames_per_s"), "steps": leg.get("steps")}
            rf = leg.get("roofline")
            if rf:
                c["roofline"] = {k: rf.get(k) for k in ("kernel", "achieved", "peak", "frac")}
            out["also"][mode] = c
    cb = full.get("cpu_baseline")
    if cb:
        out["cpu_baseline"] = {k: cb.get(k) for k in ("value", "unit", "cores", "kind", "host_cpus", "seconds_per_step",
                                                      "threads_probe_generator_forward_s", "value_as_written_anomaly_on", "sample") if k in cb}
    if detail_path:
        out["detail"] = detail_path
    out = _r(out)
    line = json.dumps(out, separators=(",", ":"))
    # bounded: drop optional blocks in a fixed order until the line fits
    for path in (("roofline", "top_rows"), ("cpu_baseline", "sample"), ("process_group",), ("also",), ("hbm",), ("roofline", "all_conv_kernels")):
        if len(line) <= limit:
            break
        d = out
        for k in path[:-1]:
            d = d.get(k) or {}
        if path[-1] == "top_rows" and d.get("top_rows"):
            d["top_rows"] = d["top_rows"][:4]
        else:
            d.pop(path[-1], None)
        line = json.dumps(out, separators=(",", ":"))
    assert len(line) <= limit, f"bench line is {len(line)} bytes"
    return line


def time_steps(model, batch, first_idx, n, barrier):
    """n training steps bracketed by barrier + device synchronisation; returns (seconds, per-step device ms from HIP events).
    time_steps.last: what the last step returned."""
    import torch

    evs = [torch.cuda.Event(enable_timing=True) for _ in range(n + 1)]
    barrier()
    t0 = time.perf_counter()
    evs[0].record()
    host = []
    step_sync = os.environ.get("DGMR_BENCH_STEP_SYNC") == "1"  # A/B switch: drain the device before every step (how much of a result is the host's lead)
    for i in range(n):
        if step_sync:
            torch.cuda.synchronize()
        h0 = time.perf_counter()
        time_steps.last = model.training_step(batch, first_idx + i)
        evs[i + 1].record()
        ms_ = torch.cuda.memory_stats()
        host.append((round(1e3 * (time.perf_counter() - h0), 1), round(torch.cuda.memory_reserved() / 2**30, 2),
                     ms_.get("num_device_alloc", 0), ms_.get("num_alloc_retries", 0)))
    barrier()
    dt = time.perf_counter() - t0
    time_steps.host = host  # per step: host ms inside training_step, reserved GB, device allocations so far, allocator retries
    return dt, [evs[i].elapsed_time(evs[i + 1]) for i in range(n)]


DUMP_SAMPLE = 4096  # elements kept per state tensor (a fixed, seeded sample of larger ones)
DUMP_LIMIT = 64 << 20  # bytes in all


def dump_outputs(out_dir, losses, model):
    """What the timed path hands its caller after its last step, as out_dir/<name>.npy: `loss.<name>` - the losses training_step
    returns (float64) - and `state.<key>` - every parameter and buffer of the model it updated in place (Adam steps, u / v, BatchNorm
    statistics; float32, integer buffers float64).  A tensor of more than DUMP_SAMPLE elements is reduced to DUMP_SAMPLE of them at
    sorted indices drawn from a generator seeded with the key, so that the same arguments dump the same positions in every run and
    build."""
    import zlib

    import numpy as np
    import torch

    os.makedirs(out_dir, exist_ok=True)
    arrays = {f"loss.{k}": np.asarray([float(v)], dtype=np.float64) for k, v in losses.items()}
    for k, v in model.state_dict().items():
        flat = v.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLE:
            idx = np.sort(np.random.default_rng(zlib.crc32(k.encode())).choice(flat.numel(), DUMP_SAMPLE, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
        flat = flat.cpu()
        arrays[f"state.{k}"] = (flat.float() if flat.is_floating_point() else flat.double()).numpy()
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_LIMIT, f"--dump-outputs: {total} bytes"
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)
    return len(arrays), total


def main():
    args = parse()
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        respawn_under_torchrun(args)
    if args.cpu_baseline == "only":  # (host-only check of the cpu_baseline leg; needs no GPU)
        kw, hw, T = WORKLOADS[args.workload]
        print(json.dumps(cpu_baseline_reference(kw, hw, T) or cpu_baseline(kw, hw, T)))
        return
    import torch
    import torch.distributed as dist

    import __graft_entry__ as ge

    # an up-to-date build is only loaded: build() takes a lock file beside the library, which a tree built by someone else (or
    # read-only) does not allow - and the benchmark needs nothing written
    if ge._needs_rebuild():
        ge.build()
    import skillful_nowcasting_amd as S
    from skillful_nowcasting_amd import _lib

    _lib.load()  # dlopen + check that every symbol of include/dgmr_hip.h is exported

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs a HIP device"
    backend = os.environ.get("DGMR_DIST_BACKEND", "nccl")  # "nccl" is RCCL on ROCm; "gloo" only for smoke-testing N ranks on one GPU
    if backend != "nccl":
        local_rank %= torch.cuda.device_count()
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    use_dist = world > 1 or args.force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # RCCL writes its version banner and its warnings to STDOUT by default: send them to stderr, stdout is for the ONE JSON line
        # (which is also printed last, after the process group is gone and C stdio has been flushed)
        os.environ.setdefault("NCCL_DEBUG_FILE", "/dev/stderr")
        if world == 1:  # --force-dist without a launcher: a one-rank RCCL group on this GPU
            import socket

            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                os.environ.setdefault("MASTER_PORT", str(sk.getsockname()[1]))
            os.environ.setdefault("RANK", "0")
            os.environ.setdefault("WORLD_SIZE", "1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)
    assert world == args.gpus, f"--gpus {args.gpus} but WORLD_SIZE {world}: launch one rank per GPU (bench.py re-execs itself under " \
                               "torch.distributed.run when started without a launcher)"

    kw, hw, T = WORKLOADS[args.workload]
    B = args.batch
    S.set_precision(args.precision)
    if args.tune:
        _lib.load().dgmr_conv_tune(*[int(v) for v in args.tune.split(",")])
    torch.manual_seed(0)
    model = S.DGMR(strict_reference_semantics=not args.fast, **kw).to(dev)
    if use_dist:
        model.attach_data_parallel(force_exchange=args.force_dist)
    torch.manual_seed(1000 + rank)
    images = torch.rand(B, 4, 1, hw, hw).to(dev)
    future = torch.rand(B, T, 1, hw, hw).to(dev)
    batch = (images, future)
    torch.manual_seed(2000 + rank)

    def barrier():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()

    for i in range(args.warmup):
        model.training_step(batch, i)
    dt, step_ms = time_steps(model, batch, args.warmup, args.steps, barrier)
    step_host = list(time_steps.host)
    if args.dump_outputs and rank == 0:  # before anything else runs a step on the model
        dump_outputs(args.dump_outputs, time_steps.last, model)
    # data parallel: every rank must hold bit-identical parameters after the timed steps (same all-reduced gradients, same Adam)
    replicas_in_sync = None
    if use_dist:
        cs = torch.stack([p.detach().double().sum() for p in model.parameters()]).sum().reshape(1)
        lo, hi = cs.clone(), cs.clone()
        if backend != "nccl":
            lo, hi = lo.cpu(), hi.cpu()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN)
        dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        replicas_in_sync = bool((lo == hi).all().item())
    pg_info = None
    if use_dist:
        # who is in the job: every rank reports (rank, device index, device name, PCI bus id); RCCL's version as torch reports it
        mine = {"rank": rank, "local_rank": local_rank, "device": torch.cuda.get_device_name(dev),
                "pci_bus_id": getattr(torch.cuda.get_device_properties(dev), "pci_bus_id", None)}
        seen = [None] * world
        try:  # (diagnostics only: nothing here may cost the bench line)
            dist.all_gather_object(seen, mine)
        except Exception as e:  # noqa: BLE001
            seen = [mine, f"all_gather_object failed: {type(e).__name__}: {e}"]
        try:
            ver = ".".join(str(v) for v in torch.cuda.nccl.version())
        except Exception:
            ver = None
        try:
            gs = dict(model.grad_sync.stats) if getattr(model, "grad_sync", None) is not None else None
        except Exception:
            gs = None
        pg_info = {"backend": backend, "world_size_reported": dist.get_world_size(), "rccl_version": ver, "ranks_seen": seen, "grad_sync": gs,
                   "forced_single_rank": bool(args.force_dist and world == 1)}
        if gs and (args.steps + args.warmup) > 1:
            # buckets that were NOT launched during the backward pass, per step, after the recording step (the first): the exchange's exposed part
            rec = gs.get("late_buckets_recording_step", 0)
            pg_info["late_buckets_per_step"] = round((gs.get("late_buckets", 0) - rec) / max(1, args.steps + args.warmup - 1), 2)
    if use_dist:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    ms_per_step = 1e3 * dt / args.steps
    frames = world * B * (4 + T)
    value = frames * args.steps / dt
    step_ms_sorted = sorted(step_ms)
    ms_median = step_ms_sorted[len(step_ms_sorted) // 2] if len(step_ms_sorted) % 2 else \
        0.5 * (step_ms_sorted[len(step_ms_sorted) // 2 - 1] + step_ms_sorted[len(step_ms_sorted) // 2])

    def measure_roofline(precision, ms_step, first_idx):
        """One extra step with HIP events around every conv launch (recorded on the launch stream inside the library)."""
        lib = _lib.load()
        # per-kernel durations must not include a co-running kernel: the weight gradients, which the timed steps run on a second
        # stream beside the data-gradient chain, are issued in line for this one instrumented step
        side = S.ops._WGRAD_STREAM
        S.ops._WGRAD_STREAM = False
        lib.dgmr_profile_enable(1)
        model.training_step(batch, first_idx)
        torch.cuda.synchronize()
        lib.dgmr_profile_enable(0)
        S.ops._WGRAD_STREAM = side
        # rows per INSTANTIATED kernel (tile, mode, launch size, arithmetic) - read before collect2, which clears the records
        need = lib.dgmr_profile_collect_detail(None, 0)
        dbuf = ctypes.create_string_buffer(need + 16)
        lib.dgmr_profile_collect_detail(dbuf, need + 16)
        detail = []
        for line in dbuf.value.decode().splitlines():
            name, n_l, ms_l, fl_l, ex_l = line.split("\t")
            n_l, ms_l, fl_l, ex_l = int(n_l), float(ms_l), float(fl_l), float(ex_l)
            pk = PEAK_F32_MFMA_TFLOPS if name.endswith("[f32]") else PEAK_BF16_MFMA_TFLOPS
            tf = fl_l / (ms_l * 1e-3) / 1e12 if ms_l > 0 else 0.0
            detail.append(dict(kernel=name, launches=n_l, total_ms=ms_l, avg_us=1e3 * ms_l / max(n_l, 1), flops_per_launch=fl_l / max(n_l, 1),
                               tflops=tf, mfma_executed_tflops=ex_l / (ms_l * 1e-3) / 1e12 if ms_l > 0 else 0.0, peak_tflops=pk, frac=tf / pk))
        detail.sort(key=lambda r: -r["total_ms"])
        nv = lib.dgmr_profile_variants()
        ms = (ctypes.c_double * nv)()
        fl = (ctypes.c_double * nv)()
        cnt = (ctypes.c_int64 * nv)()
        ex = (ctypes.c_double * nv)()
        lib.dgmr_profile_collect2(ms, fl, ex, cnt, nv)
        rows = [dict(kernel=lib.dgmr_profile_variant_name(i).decode(), launches=int(cnt[i]), total_ms=ms[i],
                     avg_us=(1e3 * ms[i] / cnt[i]) if cnt[i] else 0.0, tflops=(fl[i] / (ms[i] * 1e-3) / 1e12) if ms[i] > 0 else 0.0,
                     flops_per_launch=(fl[i] / cnt[i]) if cnt[i] else 0.0) for i in range(nv)]
        peak = PEAK_F32_MFMA_TFLOPS if precision == "f32" else PEAK_BF16_MFMA_TFLOPS
        for i_row, r in enumerate(rows):
            r["peak_tflops"] = peak
            # matrix-pipe work really issued (counted by the library per launch): x 3 / x 6 MFMAs per product in bf16x3 / bf16x6 launches,
            # x 16/36 for the phase / pooled launches of the upsampling convs
            r["mfma_executed_tflops"] = (ex[i_row] / (r["total_ms"] * 1e-3) / 1e12) if r["total_ms"] > 0 else 0.0
            r["frac"] = r["tflops"] / r["peak_tflops"]
        dom = max(rows, key=lambda r: r["total_ms"])
        tot_ms = sum(r["total_ms"] for r in rows)
        tot_fl = sum(fl[i] for i in range(nv))
        roof = {
            "bound": "mfma", "achieved": dom["tflops"], "peak": dom["peak_tflops"], "unit": "TFLOP/s",
            "frac": dom["tflops"] / dom["peak_tflops"], "traffic": None, "kernel": dom["kernel"],
            "mfma_executed_tflops": dom["mfma_executed_tflops"], "mfma_executed_frac": dom["mfma_executed_tflops"] / dom["peak_tflops"],
            "note": "achieved = algorithmic 2*M*K*Cout per launch / HIP-event time of that launch, summed over the step; a product "
                    "costs three bf16 MFMAs in bf16x3 and six in bf16x6 (mfma_executed_*), peak is the dense MFMA rate of the mode "
                    "(bf16 pipe 2.5 PF; exact f32 157.3 TF)",
            "launches_per_step": dom["launches"], "avg_launch_us": dom["avg_us"], "flops_per_launch": dom["flops_per_launch"],
            "all_conv_kernels": {"tflops": tot_fl / (tot_ms * 1e-3) / 1e12 if tot_ms else 0.0, "ms_per_step": tot_ms,
                                 "frac_of_step": tot_ms / ms_step,
                                 # algorithmic 2*M*K*Cout of every conv launch the step REALLY makes (strict semantics: the D-pass replay,
                                 # the logging forward, six recomputes), against whole_step's 20 F_g + 30 F_d
                                 "executed_conv_tflop_per_step": tot_fl / 1e12},
            "whole_step": {"algorithmic_tflop_per_sample": F_STEP_TFLOP.get(args.workload),
                           "tflops": (F_STEP_TFLOP[args.workload] * B / (ms_step * 1e-3)) if args.workload in F_STEP_TFLOP else None,
                           "frac": (F_STEP_TFLOP[args.workload] * B / (ms_step * 1e-3) / peak) if args.workload in F_STEP_TFLOP else None,
                           "note": "SURVEY.md §8(d): F_step = 20 F_g + 30 F_d per sample, over the whole step time"},
            "per_kernel": rows,
            "per_kernel_detail": detail,
            "per_kernel_detail_note": "the class rows of per_kernel split by instantiated kernel: output-channel block / pixels per workgroup, "
                                      "mode (plain 3x3 | phase = forward of an upsampling conv as four 2x2 convs | pooled = its data gradient), "
                                      "ConvGRU epilogue, split-K, 1x1, launch size (small = fewer than 1024 workgroups), arithmetic of the launch; "
                                      "tflops = flops_per_launch x launches / total_ms",
        }
        # HBM traffic of the dominant kernel from the committed PMC passes (separate rocprofv3 --pmc runs, FETCH_SIZE doubled per
        # MI355X_MICROARCH.md): measured on one representative launch of that kernel (tools/pmc_conv.sh), not inside this process
        import glob

        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_dominant.json")))
        pmc_path = cands[-1] if cands else ""
        if pmc_path:
            pmc = json.load(open(pmc_path))
            if pmc.get("precision") in (precision, {"mixed": "bf16x3"}.get(precision)) and dom["kernel"] in pmc.get("kernel", ""):
                # `traffic` belongs to ONE named launch of the dominant kernel (pmc_launch: its own duration, flops and bytes);
                # avg_launch_us / flops_per_launch above are the class averages over the step - two different things, both labelled
                roof["traffic"] = pmc["traffic_bytes"]
                roof["traffic_over_algorithmic"] = pmc.get("traffic_over_algorithmic")
                roof["pmc_source"] = f"profiles/{os.path.basename(pmc_path)}: committed rocprofv3 --pmc passes on one launch of this kernel (not this run)"
                roof["mfma_util"] = pmc.get("mfma_util")
                roof["valu_per_mfma"] = pmc.get("valu_per_mfma")
                roof["pmc_launch"] = {k: pmc.get(k) for k in ("kernel", "shape", "launch_us", "algorithmic_tflops", "mfma_executed_tflops",
                                                               "traffic_bytes", "algorithmic_bytes", "traffic_over_algorithmic", "hbm_gbps",
                                                               "mfma_util", "valu_per_mfma", "wave_cycles_split")}
                roof["traffic_detail"] = {k: pmc[k] for k in ("shape", "launch_us", "algorithmic_bytes", "traffic_over_algorithmic",
                                                              "hbm_gbps", "mfma_util", "valu_per_mfma", "traffic_note")}
                roof["traffic_detail"]["source"] = (f"profiles/{os.path.basename(pmc_path)} (+ raw counters in profiles/*_pmc_*.csv): "
                                                    "PMC passes cannot run inside this process; the number is the committed "
                                                    "measurement of one representative launch of this kernel, not of this run")
        # time-weighted matrix-pipe busy share over every 3x3 conv class (north star: >= 40 %), from the committed per-class PMC passes
        cands = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_classes.json")))
        if cands and precision != "f32":
            try:
                pc = json.load(open(cands[-1]))
                roof["mfma_util_weighted"] = pc.get("mfma_util_weighted")
                roof["mfma_util_weighted_source"] = (f"profiles/{os.path.basename(cands[-1])} (committed whole-step rocprofv3 --pmc pass"
                                                     + (f" of commit {pc['commit']}" if pc.get("commit") else "") + ", not this run)")
                roof["mfma_util_classes"] = {"source": f"profiles/{os.path.basename(cands[-1])}", "rows": pc.get("rows")}
            except (OSError, ValueError):
                pass
        return roof

    roofline = None
    if args.full and not args.no_roofline:
        roofline = measure_roofline(args.precision, ms_per_step, args.warmup + args.steps)

    # The same build in the other arithmetic modes, witnessed by the same run.  The exact-f32 leg is the reference's own arithmetic
    # (train/run.py:232 precision=32): a first-class line of >= 10 steps after 3 warm-ups with its own per-kernel roofline block
    # (peak 157.3 TF).  bf16x6 (fp32-faithful products on the bf16 pipe) and plain bf16 (BASELINE.json configs[1]'s dtype) ride along.
    also = None
    if args.full and (args.also == "on" or (args.also == "auto" and world == 1)) and not args.fast:
        also = {}
        legs = {"f32": (3, max(1, args.also_f32_steps)), "bf16x6": (2, 5), "bf16": (2, 5)}
        for mode, (w_m, n) in legs.items():
            if mode == args.precision:
                continue
            S.set_precision(mode)
            for i in range(w_m):
                model.training_step(batch, 10_000 + i)  # warm-up: weight planes / plans / allocator state of this mode
            dt_m, ms_m = time_steps(model, batch, 10_100, n, barrier)
            ms_sorted = sorted(ms_m)
            med = ms_sorted[n // 2] if n % 2 else 0.5 * (ms_sorted[n // 2 - 1] + ms_sorted[n // 2])
            also[mode] = {"ms_per_step": 1e3 * dt_m / n, "ms_per_step_median": med, "radar_frames_per_s": frames * n / dt_m,
                          "steps": n, "warmup": w_m, "step_ms": [round(v, 1) for v in ms_m], "dtype": DTYPE_TEXT[mode]}
            if mode == "f32" and not args.no_roofline:
                also[mode]["roofline"] = measure_roofline("f32", 1e3 * dt_m / n, 10_200)
        S.set_precision(args.precision)
        # what strictness costs: the same model with strict_reference_semantics=False (the D passes' state-only generator replay, the
        # logging forward and the checkpoint recomputes are skipped; losses and gradients of a step are the same, u / v / BatchNorm
        # state advance differently from the reference's) - NOT the headline, reported so that the price is visible
        model.strict_reference_semantics = False
        try:
            for i in range(2):
                model.training_step(batch, 20_000 + i)
            dt_m, ms_m = time_steps(model, batch, 20_100, 5, barrier)
            also["fast"] = {"ms_per_step": 1e3 * dt_m / 5, "radar_frames_per_s": frames * 5 / dt_m, "steps": 5, "warmup": 2,
                            "step_ms": [round(v, 1) for v in ms_m], "semantics": "strict_reference_semantics=False, same arithmetic mode as the headline"}
        finally:
            model.strict_reference_semantics = True

    if rank == 0:
        out = {
            "metric": "radar frames/sec (G+D step) 4->18 @256^2" if args.workload == "paper" else f"radar frames/sec (G+D step) [{args.workload}]",
            "value": value, "unit": "radar frames/s", "n_gpus": args.gpus, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "ms_per_step_median": ms_median, "step_ms": [round(v, 1) for v in step_ms], "step_host_ms__reserved_gb__device_allocs__retries": step_host,
            "hbm": {"max_allocated_gb": round(torch.cuda.max_memory_allocated() / 2**30, 1),
                    "reserved_gb": round(torch.cuda.memory_reserved() / 2**30, 1),
                    "alloc_retries": torch.cuda.memory_stats().get("num_alloc_retries", 0)},
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPE_SHORT[args.precision], "dtype_long": DTYPE_TEXT[args.precision],
            "data": "synthetic torch.rand frames, random-init weights",
            "config": {"workload": f"DGMR.training_step {args.workload}: " + ", ".join(f"{k}={v}" for k, v in kw.items()) + f", H=W={hw}",
                       "per_gpu_batch": B, "global_batch": world * B, "frames_per_sample": 4 + T, "parallelism": f"dp{world}",
                       "semantics": "fast (state-only forwards skipped)" if args.fast else
                                    "strict: every observable effect of the reference step (losses, both Adam updates, u/v, BN and RNG state)"},
        }
        try:  # tail balancing of the weight-gradient stream (_streams.py): per recurring backward pass, the share of its weight-gradient
            # cost that runs on the main stream and the last measured waits of the main stream at the join (ms; > 0: it waited)
            from skillful_nowcasting_amd import _streams as _st

            out["wgrad_tail_balance"] = [{"pass_calls": len(pr.costs), "inline_share": round(sh, 4), "join_wait_ms": hist}
                                         for (k_, (sh, hist)), pr in zip(_st.tail_stats().items(), _st._tail_profiles.values())]
        except Exception:  # noqa: BLE001
            pass
        if replicas_in_sync is not None:
            out["replicas_in_sync"] = replicas_in_sync  # parameter checksums agree bit for bit across the ranks after the timed steps
        if pg_info is not None:
            out["process_group"] = pg_info
        if roofline:
            out["roofline"] = roofline
        if also:
            out["also"] = also
        if args.full and args.cpu_baseline != "off" and world == 1:  # (the contract: on rank 0 at N = 1 only - the other ranks would sit in the final barrier)
            out["cpu_baseline"] = cpu_baseline_reference(kw, hw, T) or cpu_baseline(kw, hw, T)
            if args.workload in REFERENCE_MEASURED:
                out["cpu_baseline"]["reference_measured"] = REFERENCE_MEASURED[args.workload]
        # --full: the full record (per_kernel_detail, per-step times, the PMC launch records) goes to a side file; stdout gets ONE
        # bounded line
        detail_path = None
        if args.full:
            detail_path = args.detail or os.path.join("bench_out", "bench_detail.json")
            try:
                os.makedirs(os.path.dirname(os.path.join(ROOT, detail_path)) or ".", exist_ok=True)
                with open(os.path.join(ROOT, detail_path), "w") as f:
                    json.dump(out, f, indent=1)
            except OSError as e:  # (a read-only tree must not cost the bench line)
                detail_path = f"not written: {e}"
        final_line = compact_line(out, detail_path)
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the ONE line goes out LAST: RCCL prints a version banner through C stdio, which is flushed when it likes - seen behind the
        # JSON line in a --force-dist run; flush C stdio first, then print
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:  # noqa: BLE001
            pass
        sys.stdout.flush()
        print(final_line, flush=True)


if __name__ == "__main__":
    main()
