"""Device time of the stochastic advection ensemble on a full 1536 x 1280 composite (skillful_nowcasting_amd/stochastic.py;
dgmr_spectral_ar in csrc/spectral_ar.hip, dgmr_advect_series in csrc/advect.hip).

    python tools/stochastic_timing.py [--repeats 7] [--order 2] [--velocity] [--out profiles/stochastic_timing.json]
                                      [--match-out profiles/probability_match_timing.json]

Inputs: the rain-covered sequence of tools/advection_timing.py (a smooth field moving by (2, -3) pixels per frame), M = 8 members,
T = 18 lead times, window 128, the library's default lifetimes.  HIP events bracket single calls on one stream; after a warm-up the
median over --repeats calls counts (minimum and maximum are listed).

  * dgmr_spectral_ar alone (four launches), with the bytes it must move (white read once, out written by the first class and read
    and written by the other three) and its transform count;
  * the same recursion written with torch.fft (rfft2 / irfft2 over the windows of each class, the blend as slice updates) on the
    same device, for scale, and how far the two results are apart;
  * dgmr_advect_series for the M planes of T sources;
  * one whole EnsembleAdvectionNowcaster.nowcast (conversion, motion, dB, noise drawn on the device, recursion, advection, back).
With --match-out also (dgmr_probability_match in csrc/probmatch.hip), written to that file:
  * probability_match alone on the recursion's output (the target's sort and the workspace included), without and with a mask, with
    the rate it reaches on two reads and one write of M T H W floats;
  * the same ranks by a full sort on the device (argsort of every plane, the sorted target scattered through it), for scale, and
    how much of the two results differs (a binned rank is off by less than a bin's occupancy; ties are ordered arbitrarily by a sort);
  * the whole nowcast without matching, with it, and with it and a mask.
With --order 2 also (dgmr_spectral_ar2 in csrc/spectral_ar.hip), in the --out file:
  * spectral_ar2 beside spectral_ar on the same inputs (zm1: the frame before the last moved one step; rho2 = rho^3), and the
    same recursion written with torch.fft;
  * the whole nowcast at order 2 beside order 1, with explicit correlations and with rho="estimate".
With --velocity also (dgmr_advect_series_perturbed in csrc/advect.hip), under "velocity" in the --out file (default
profiles/velocity_perturbation_timing.json), every group timed in alternation, one call of each per round:
  * advect_series beside advect_series_perturbed with zero amplitudes (and whether the two results have the same bits) and with the
    amplitudes of perturb_velocities("steps") for seed 0;
  * the whole order-1 nowcast without and with perturb_velocities("steps").
Numbers are recorded, not asserted."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

H, W, T_OUT, MEMBERS, WINDOW = 1536, 1280, 18, 8, 128
COPY_BYTES_PER_S = 6.29e12  # measured device-to-device copy rate of the MI355X


def timed(fn, repeats):
    import torch

    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        t1.synchronize()
        times.append(t0.elapsed_time(t1))
    return {"ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times), "calls": len(times)}


def timed_alternating(fns, repeats):
    """`timed` for several calls that are to be compared: after a warm-up of each, `repeats` rounds that run every call once, one after
    the other, so that a drift of the machine reaches all of them alike -> {name: `timed`'s record}"""
    import torch

    for fn in fns.values():
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            times[k].append(t0.elapsed_time(t1))
    return {k: {"ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "calls": len(v)} for k, v in times.items()}


def spectral_ar_torch(z0, white, rho, window):
    """stochastic.spectral_ar_reference with torch.fft in fp32 on the tensors' device (half spectra: the fields are real)."""
    import numpy as np
    import torch

    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import axis_weights

    p, m, steps, h, w = white.shape
    dev = z0.device
    bins = torch.from_numpy(_radial_bins(window)[:, :window // 2 + 1].copy()).to(dev)
    rk = rho[bins]
    gain = torch.sqrt((1.0 - rk.double() ** 2).clamp_min(0.0)).float()
    (ay, hy), (ax, hx) = axis_weights(h, window), axis_weights(w, window)
    out = torch.zeros((p, m, steps, h, w), dtype=torch.float32, device=dev)
    half = window // 2
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)
            wgt = torch.from_numpy(np.outer((hy if cy else ay)[ys], (hx if cx else ax)[xs])).to(dev)

            def windows(x):
                t = x[..., ys, xs]
                return t.reshape(x.shape[:-2] + (ny, window, nx, window)).movedim(-3, -2)

            u = torch.fft.rfft2(windows(z0))[:, None]
            amp = gain * (u.abs() / window)
            state = u.expand(p, m, ny, nx, window, half + 1).clone()
            for t in range(steps):
                state = rk * state + amp * torch.fft.rfft2(windows(white[:, :, t]))
                x = torch.fft.irfft2(state, s=(window, window)).movedim(-2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * wgt
    return out


def spectral_ar2_torch(z0, zm1, white, coef, window):
    """stochastic.spectral_ar2_reference with torch.fft in fp32 on the tensors' device (half spectra: the fields are real)."""
    import numpy as np
    import torch

    from skillful_nowcasting_amd.spectra import _radial_bins
    from skillful_nowcasting_amd.stochastic import axis_weights

    p, m, steps, h, w = white.shape
    dev = z0.device
    bins = torch.from_numpy(_radial_bins(window)[:, :window // 2 + 1].copy()).to(dev)
    phi1, phi2, gain = coef[0][bins], coef[1][bins], coef[2][bins]
    (ay, hy), (ax, hx) = axis_weights(h, window), axis_weights(w, window)
    out = torch.zeros((p, m, steps, h, w), dtype=torch.float32, device=dev)
    half = window // 2
    for cy in (0, 1):
        for cx in (0, 1):
            ny, nx = h // window - cy, w // window - cx
            if ny == 0 or nx == 0:
                continue
            ys, xs = slice(cy * half, cy * half + ny * window), slice(cx * half, cx * half + nx * window)
            wgt = torch.from_numpy(np.outer((hy if cy else ay)[ys], (hx if cx else ax)[xs])).to(dev)

            def windows(x):
                t = x[..., ys, xs]
                return t.reshape(x.shape[:-2] + (ny, window, nx, window)).movedim(-3, -2)

            u = torch.fft.rfft2(windows(z0))[:, None]
            amp = gain * (u.abs() / window)
            x1 = u.expand(p, m, ny, nx, window, half + 1).clone()
            x2 = torch.fft.rfft2(windows(zm1))[:, None].expand(p, m, ny, nx, window, half + 1).clone()
            for t in range(steps):
                x1, x2 = (phi1 * x1 + phi2 * x2) + amp * torch.fft.rfft2(windows(white[:, :, t])), x1
                x = torch.fft.irfft2(x1, s=(window, window)).movedim(-2, -3).reshape(p, m, ny * window, nx * window)
                out[:, :, t, ys, xs] += x * wgt
    return out


def rank_match_torch(z, target):
    """Exact rank matching with torch: every plane sorted in full, the sorted target scattered through the order."""
    import torch

    p, m, steps, h, w = z.shape
    order = z.reshape(p, m * steps, h * w).argsort(dim=2)
    out = torch.empty((p, m * steps, h * w), dtype=torch.float32, device=z.device)
    out.scatter_(2, order, torch.sort(target.reshape(p, 1, h * w), dim=2).values.expand(p, m * steps, h * w))
    return out.view(z.shape)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--match-out", default=None)
    ap.add_argument("--order", type=int, default=1, choices=(1, 2))
    ap.add_argument("--velocity", action="store_true")
    a = ap.parse_args()
    if a.velocity and not a.out:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "velocity_perturbation_timing.json")
    import torch

    import __graft_entry__ as g

    g.build()
    from advection_timing import rain_sequence
    from skillful_nowcasting_amd.advection import advect_series, lattice_geometry, motion_field
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, lifetime_rho, spectral_ar, to_db

    assert torch.cuda.is_available(), "needs a HIP device"
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    seq = rain_sequence(gen, dev, 4, (2, -3), False)  # [4, H, W]
    rec = {"device": torch.cuda.get_device_name(0),
           "command": f"python tools/stochastic_timing.py --repeats {a.repeats}" + (" --order 2" if a.order == 2 else "")
           + (" --velocity" if a.velocity else ""), "frame": [H, W],
           "members": MEMBERS, "lead_times": T_OUT, "window": WINDOW, "assumed_rates": {"copy_bytes_per_s": COPY_BYTES_PER_S},
           "wet_pixel_share": float((seq > 0).double().mean())}
    nowcaster = EnsembleAdvectionNowcaster(forecast_steps=T_OUT, window=WINDOW)
    rho = lifetime_rho(WINDOW).to(dev)
    z0 = to_db(seq[-1:])
    white = nowcaster.white_noise(1, MEMBERS, H, W, dev, seed=0)
    out = torch.empty_like(white)
    plane = MEMBERS * T_OUT * H * W * 4
    windows = MEMBERS * sum((H // WINDOW - cy) * (W // WINDOW - cx) for cy in (0, 1) for cx in (0, 1))
    ar = timed(lambda: spectral_ar(z0, white, rho, WINDOW, out=out), a.repeats)
    # per class and covered pixel: white read once, out written (class (0,0)) or read and written (the other three)
    share = {(cy, cx): (H // WINDOW - cy) * (W // WINDOW - cx) / ((H // WINDOW) * (W // WINDOW)) for cy in (0, 1) for cx in (0, 1)}
    nbytes = int(plane * sum(f * (2 if c == (0, 0) else 3) for c, f in share.items()))
    ar.update({"windows": windows, "transforms_2d": windows * (2 * T_OUT + 1), "bytes_moved": nbytes, "GB_per_s": nbytes / ar["ms"] / 1e6,
               "ms_at_copy_rate": nbytes / COPY_BYTES_PER_S * 1e3})
    rec["spectral_ar"] = ar
    print(f"spectral_ar  M={MEMBERS} T={T_OUT} L={WINDOW}: {ar['ms']:.3f} ms ({ar['min_ms']:.3f} - {ar['max_ms']:.3f}), {windows} windows, "
          f"{ar['GB_per_s']:.0f} GB/s of its own traffic", flush=True)
    try:
        ref = spectral_ar_torch(z0, white, rho, WINDOW)
        gap = float((ref - out).abs().max())
        tf = timed(lambda: spectral_ar_torch(z0, white, rho, WINDOW), max(3, a.repeats // 2))
        tf["max_abs_difference_to_kernel"] = gap
        tf["over_kernel"] = tf["ms"] / ar["ms"]
        rec["spectral_ar_torch_fft"] = tf
        print(f"torch.fft recursion: {tf['ms']:.3f} ms ({tf['over_kernel']:.1f} x the kernel), largest difference {gap:.3e}", flush=True)
        del ref
    except RuntimeError as e:  # no FFT library on the device
        rec["spectral_ar_torch_fft"] = {"unavailable": str(e).splitlines()[0]}
        print(f"torch.fft on the device is not available: {rec['spectral_ar_torch_fft']['unavailable']}", flush=True)
    field = motion_field(seq[:, None], 32, 16, 8)
    origin, spacing = lattice_geometry(32, 16)
    rhos = None
    if a.order == 2:
        from skillful_nowcasting_amd.advection import advect
        from skillful_nowcasting_amd.stochastic import ar2_coefficients, spectral_ar2

        # a second lag that forgets faster than the AR(1) of rho would (rho2 = rho^3 < rho^2: phi2 < 0); the values do not enter the time
        rhos = torch.stack([rho, rho ** 3])
        coef = ar2_coefficients(rhos[0], rhos[1])
        zm1 = advect(to_db(seq[-2:-1]), field, 1, origin, spacing)[:, -1]
        out2 = torch.empty_like(out)
        ar2 = timed(lambda: spectral_ar2(z0, zm1, white, coef, WINDOW, out=out2), a.repeats)
        ar2.update({"windows": windows, "transforms_2d": windows * (2 * T_OUT + 2), "bytes_moved": nbytes, "GB_per_s": nbytes / ar2["ms"] / 1e6,
                    "over_spectral_ar": ar2["ms"] / ar["ms"]})
        rec["spectral_ar2"] = ar2
        print(f"spectral_ar2 M={MEMBERS} T={T_OUT} L={WINDOW}: {ar2['ms']:.3f} ms ({ar2['min_ms']:.3f} - {ar2['max_ms']:.3f}), "
              f"{ar2['over_spectral_ar']:.2f} x spectral_ar", flush=True)
        try:
            ref = spectral_ar2_torch(z0, zm1, white, coef, WINDOW)
            gap = float((ref - out2).abs().max())
            tf = timed(lambda: spectral_ar2_torch(z0, zm1, white, coef, WINDOW), max(3, a.repeats // 2))
            tf["max_abs_difference_to_kernel"] = gap
            tf["over_kernel"] = tf["ms"] / ar2["ms"]
            rec["spectral_ar2_torch_fft"] = tf
            print(f"torch.fft AR(2) recursion: {tf['ms']:.3f} ms ({tf['over_kernel']:.1f} x the kernel), largest difference {gap:.3e}", flush=True)
            del ref
        except RuntimeError as e:  # no FFT library on the device
            rec["spectral_ar2_torch_fft"] = {"unavailable": str(e).splitlines()[0]}
            print(f"torch.fft on the device is not available: {rec['spectral_ar2_torch_fft']['unavailable']}", flush=True)
        del out2, zm1
    moved = torch.empty(MEMBERS, T_OUT, H, W, device=dev)
    adv = timed(lambda: advect_series(out[0], field, origin, spacing, field_group=MEMBERS, out=moved), a.repeats)
    adv.update({"bytes_stored": plane, "GB_per_s_stored": plane / adv["ms"] / 1e6, "ms_at_copy_rate": 2 * plane / COPY_BYTES_PER_S * 1e3})
    rec["advect_series"] = adv
    print(f"advect_series {MEMBERS} x {T_OUT} planes: {adv['ms']:.3f} ms ({adv['GB_per_s_stored']:.0f} GB/s stored)", flush=True)
    if a.velocity:
        from skillful_nowcasting_amd.advection import advect_series_perturbed, unit_directions
        from skillful_nowcasting_amd.stochastic import velocity_perturbation_scale

        direction = unit_directions(field)
        sigma = velocity_perturbation_scale(T_OUT).to(dev)
        eps = nowcaster.velocity_noise(1, MEMBERS, 0).to(dev)
        amps = {"zero": torch.zeros(MEMBERS, T_OUT, 2, device=dev),
                "steps": (eps[:, :, None, :] * sigma[None, None]).reshape(MEMBERS, T_OUT, 2).contiguous()}
        moved_p = torch.empty_like(moved)
        advect_series(out[0], field, origin, spacing, field_group=MEMBERS, out=moved)
        advect_series_perturbed(out[0], field, direction, amps["zero"], origin, spacing, field_group=MEMBERS, out=moved_p)
        same = bool(torch.equal(moved.view(torch.int32), moved_p.view(torch.int32)))
        fns = {"advect_series": lambda: advect_series(out[0], field, origin, spacing, field_group=MEMBERS, out=moved)}
        for key, amp in amps.items():
            fns["advect_series_perturbed_" + key] = (lambda amp=amp: advect_series_perturbed(out[0], field, direction, amp, origin, spacing,
                                                                                           field_group=MEMBERS, out=moved_p))
        vel = timed_alternating(fns, a.repeats)
        for key in amps:
            vel["advect_series_perturbed_" + key]["over_advect_series"] = vel["advect_series_perturbed_" + key]["ms"] / vel["advect_series"]["ms"]
        vel["zero_amplitude_gives_advect_series_bits"] = same
        vel["largest_amplitude_px_per_step"] = float(amps["steps"].abs().max())
        rec["velocity"] = vel
        print(f"alternating: advect_series {vel['advect_series']['ms']:.3f} ms ({vel['advect_series']['min_ms']:.3f} - "
              f"{vel['advect_series']['max_ms']:.3f}); perturbed with zero amplitudes {vel['advect_series_perturbed_zero']['ms']:.3f} ms "
              f"({vel['advect_series_perturbed_zero']['over_advect_series']:.2f} x, the same bits: {same}), with \"steps\" amplitudes "
              f"{vel['advect_series_perturbed_steps']['ms']:.3f} ms ({vel['advect_series_perturbed_steps']['over_advect_series']:.2f} x)", flush=True)
        del moved_p
    del moved, white
    match = None
    if a.match_out:
        from skillful_nowcasting_amd.stochastic import precipitation_mask, probability_match

        match = {k: rec[k] for k in ("device", "frame", "members", "lead_times", "window", "wet_pixel_share")}
        match["command"] = f"python tools/stochastic_timing.py --repeats {a.repeats} --match-out {a.match_out}"
        matched = torch.empty_like(out)
        for key, mask in (("probability_match", None), ("probability_match_masked", precipitation_mask(z0, 5.0, 8))):
            pm = timed(lambda: probability_match(out, z0, mask, out=matched), a.repeats)
            pm.update({"bytes_moved": 3 * plane, "GB_per_s": 3 * plane / pm["ms"] / 1e6, "ms_at_copy_rate": 3 * plane / COPY_BYTES_PER_S * 1e3})
            match[key] = pm
            print(f"{key} {MEMBERS} x {T_OUT} planes: {pm['ms']:.3f} ms ({pm['min_ms']:.3f} - {pm['max_ms']:.3f}), {pm['GB_per_s']:.0f} GB/s "
                  "of two reads and a write", flush=True)
        probability_match(out, z0, out=matched)
        exact = rank_match_torch(out, z0)
        ts = timed(lambda: rank_match_torch(out, z0), max(3, a.repeats // 2))
        ts.update({"over_kernel": ts["ms"] / match["probability_match"]["ms"], "share_of_elements_that_differ": float((exact != matched).double().mean()),
                   "max_abs_difference_dB": float((exact - matched).abs().max())})
        match["rank_match_torch_sort"] = ts
        print(f"torch argsort + scatter: {ts['ms']:.3f} ms ({ts['over_kernel']:.1f} x the kernel), {ts['share_of_elements_that_differ']:.2e} of "
              f"the elements differ, by at most {ts['max_abs_difference_dB']:.3f} dB", flush=True)
        del exact, matched
    del out
    frames = seq[..., None].contiguous()
    rec["nowcast"] = timed(lambda: nowcaster.nowcast(frames, MEMBERS, seed=1), a.repeats)
    print(f"whole nowcast: {rec['nowcast']['ms']:.3f} ms", flush=True)
    if a.velocity:
        perturbed = EnsembleAdvectionNowcaster(forecast_steps=T_OUT, window=WINDOW).perturb_velocities("steps")
        both = timed_alternating({"nowcast": lambda: nowcaster.nowcast(frames, MEMBERS, seed=1),
                                  "nowcast_perturbed": lambda: perturbed.nowcast(frames, MEMBERS, seed=1)}, a.repeats)
        both["nowcast_perturbed"]["over_unperturbed"] = both["nowcast_perturbed"]["ms"] / both["nowcast"]["ms"]
        rec["velocity"].update(both)
        print(f"alternating: whole nowcast {both['nowcast']['ms']:.3f} ms ({both['nowcast']['min_ms']:.3f} - {both['nowcast']['max_ms']:.3f}), "
              f"with velocity perturbations {both['nowcast_perturbed']['ms']:.3f} ms ({both['nowcast_perturbed']['over_unperturbed']:.3f} x)",
              flush=True)
    if a.order == 2:
        for key, kw in (("nowcast_order2", {"rho": rhos.cpu(), "order": 2}), ("nowcast_estimate", {"rho": "estimate"}),
                        ("nowcast_order2_estimate", {"rho": "estimate", "order": 2})):
            nc = EnsembleAdvectionNowcaster(forecast_steps=T_OUT, window=WINDOW, **kw)
            rec[key] = timed(lambda: nc.nowcast(frames, MEMBERS, seed=1), a.repeats)
            print(f"whole {key}: {rec[key]['ms']:.3f} ms", flush=True)
        rec["nowcast_order2"]["over_order1"] = rec["nowcast_order2"]["ms"] / rec["nowcast"]["ms"]
        rec["nowcast_order2_estimate"]["over_order1"] = rec["nowcast_order2_estimate"]["ms"] / rec["nowcast_estimate"]["ms"]
    if match is not None:
        match["nowcast"] = rec["nowcast"]
        for key, kw in (("nowcast_matched", {}), ("nowcast_matched_masked", {"mask_radius": 8})):
            nc = EnsembleAdvectionNowcaster(forecast_steps=T_OUT, window=WINDOW, probability_matching=True, **kw)
            match[key] = timed(lambda: nc.nowcast(frames, MEMBERS, seed=1), a.repeats)
            match[key]["over_unmatched"] = match[key]["ms"] / rec["nowcast"]["ms"]
            print(f"whole {key}: {match[key]['ms']:.3f} ms ({match[key]['over_unmatched']:.2f} x the unmatched nowcast)", flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(a.match_out)), exist_ok=True)
        with open(a.match_out, "w") as fh:
            json.dump(match, fh, indent=1)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(rec, fh, indent=1)


if __name__ == "__main__":
    main()
