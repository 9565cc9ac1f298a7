"""Inputs, cases and the accuracy constant shared by the velocity-perturbation tests (tests/test_velocity_host.py,
tests/test_gpu_velocity.py).  The generators are this file's own copies of those in test_gpu_advection.py."""
import functools

import numpy as np

import advection_recipe as AR

# rounded fp32 operations per step in dgmr_advect_series_perturbed's position arithmetic, both axes (include/dgmr_hip.h,
# csrc/advect.hip): per axis the 10 of dgmr_advect, 2 x 6 for the two direction components' interpolations and 2 for the fmas, + 1
PERTURBED_C = 2 * (10 + 12 + 2 + 1)

# name -> (H, W, T, shared field): the shapes of the rotating-field accuracy test
ROTATING_CASES = {
    "48x80 T=18": (48, 80, 18, False),
    "96x128 T=18 shared": (96, 128, 18, True),
    "48x81 T=18": (48, 81, 18, False),
    "96x128 T=1": (96, 128, 1, False),
}
FIELD_GROUP = 3


def source(h, w, n):
    """fp32 [n, h, w] rain fields with one NaN and one negative element each."""
    x = np.stack([AR.rain_field(5 + i, h, w) for i in range(n)])
    x[:, 3, 5] = np.nan
    x[:, h - 2, w - 3] = -1.0
    return x


def series_source(h, w, n, steps):
    """fp32 [n, steps, h, w]: a source of its own per plane and lead time, with NaN and negative elements."""
    return source(h, w, n * steps).reshape(n, steps, h, w)


def shifted(x, dy, dx):
    """x moved by (dy, dx) with zeros shifted in: out[y][x] = x[y - dy][x - dx]."""
    out = np.zeros_like(x)
    h, w = x.shape[-2:]
    if abs(dy) >= h or abs(dx) >= w:
        return out
    ys, yd = (slice(0, h - dy), slice(dy, h)) if dy >= 0 else (slice(-dy, h), slice(0, h + dy))
    xs, xd = (slice(0, w - dx), slice(dx, w)) if dx >= 0 else (slice(-dx, w), slice(0, w + dx))
    out[..., yd, xd] = x[..., ys, xs]
    return out


def rotating_field(n, gy, gx, h, w, origin, spacing, omega):
    """Per plane a rigid rotation by omega_i radians per step about the frame's centre plus a drift, sampled on the lattice."""
    f = np.empty((n, gy, gx, 2), np.float32)
    py = origin + spacing * np.arange(gy)[:, None]
    px = origin + spacing * np.arange(gx)[None, :]
    for i in range(n):
        om = omega * (1 + i)
        f[i, ..., 0] = om * (px - w / 2) + 0.3 * (i + 1)
        f[i, ..., 1] = -om * (py - h / 2) - 0.7
    return f


def geometry(h, w):
    """(origin, spacing) of a 3 x 5 lattice over an h x w frame."""
    return 7.5, min((h - 16) / 2.0, (w - 16) / 4.0)


def unit(field):
    """`unit_directions` of a numpy lattice -> fp32 numpy"""
    import torch

    from skillful_nowcasting_amd.advection import unit_directions

    return unit_directions(torch.from_numpy(np.asarray(field, np.float32))).numpy()


def growing_amplitude(n, steps, peak=0.5):
    """fp32 [n, steps, 2]: per plane a pair of its own sign and size, growing linearly with t up to about `peak` pixels per step;
    every third plane is unperturbed."""
    t = (np.arange(steps, dtype=np.float64) + 1.0) / steps
    amp = np.zeros((n, steps, 2))
    for i in range(n):
        if i % 3 == 1:
            continue
        sign = 1.0 if i % 2 == 0 else -1.0
        amp[i, :, 0] = sign * peak * t * (1.0 - 0.1 * (i % 4))
        amp[i, :, 1] = -sign * 0.6 * peak * t
    return amp.astype(np.float32)


@functools.lru_cache(maxsize=None)
def rotating_case(name):
    """-> (x [N, T, H, W], field, direction, amplitude [N, T, 2], origin, spacing, reference float64 [N, T, H, W], unperturbed reference),
    N = 2 FIELD_GROUP planes, computed once, read-only."""
    from skillful_nowcasting_amd.advection import advect_series_perturbed_reference, advect_series_reference

    h, w, steps, shared = ROTATING_CASES[name]
    n = 2 * FIELD_GROUP
    x = series_source(h, w, n, steps)
    origin, spacing = geometry(h, w)
    field = rotating_field(1 if shared else n // FIELD_GROUP, 3, 5, h, w, origin, spacing, 0.004)
    direction = unit(field)
    amplitude = growing_amplitude(n, steps)
    ref = advect_series_perturbed_reference(x, field, direction, amplitude, origin, spacing, FIELD_GROUP)
    plain = advect_series_reference(x, field, origin, spacing, FIELD_GROUP)
    for a in (x, field, direction, amplitude, ref, plain):
        a.setflags(write=False)
    return x, field, direction, amplitude, origin, spacing, ref, plain


def bound(x, steps, h, w):
    """c' T max(H, W) 2^-24 A + 4 * 2^-24 max|x| over all steps' sources, missing elements as 0 -> (bound, clean x float64)"""
    with np.errstate(invalid="ignore"):
        clean = np.where(x >= 0, x, 0).astype(np.float64)
    adjacent = max(np.abs(np.diff(clean, axis=-1)).max(), np.abs(np.diff(clean, axis=-2)).max())
    return PERTURBED_C * steps * max(h, w) * 2.0 ** -24 * adjacent + 4 * 2.0 ** -24 * clean.max(), clean


def translating_context(size=64, frames=5, seed=5, v=(2, -3)):
    """[frames, size, size] rain rates of a translating field (advection_recipe)."""
    return AR.translating_sequence(seed, size, size, frames, v)


# ---- the nowcaster, device against CPU: 128 x 128, M = 2, T = 3, window 64 ---------------------------------------------------------------
NC_M, NC_T, NC_WINDOW, NC_SIZE = 2, 3, 64, 128
NC_EPS = ((1.5, -1.0), (-2.0, 0.5))  # the two members' (eps_par, eps_perp)


@functools.lru_cache(maxsize=None)
def nowcast_case():
    """The CPU nowcast with explicit white and velocity noise and what the criterion needs, computed once -> dict:
    frames [4, H, W, 1] torch, white, eps torch, rho torch, want (CPU rain rates, numpy float64 [M, T, 1, H, W]), field (the CPU path's
    motion field, torch), amplitude fp32 numpy [M, T, 2], z_ref / cells (spectral_ar_reference and its cell majorant), moved (the
    float64 reference advection of z_ref along the CPU field, [M, T, 1, H, W]), pad, threshold."""
    import torch

    import stochastic_recipe as SR
    from skillful_nowcasting_amd.advection import advect_series_perturbed_reference, lattice_geometry, unit_directions
    from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster, spectral_ar_reference, to_db

    seq = translating_context(NC_SIZE, 5)
    frames = torch.from_numpy(seq[:4])[..., None]
    rho = torch.from_numpy(SR.case_rho(NC_WINDOW))
    white = torch.from_numpy(SR.white_field((1, NC_M, NC_T, NC_SIZE, NC_SIZE), seed=3))
    eps = torch.tensor([NC_EPS], dtype=torch.float32)
    cpu = EnsembleAdvectionNowcaster(forecast_steps=NC_T, window=NC_WINDOW, rho=rho).perturb_velocities("steps")
    want = cpu.nowcast(frames, NC_M, white=white, velocity_noise=eps).numpy().astype(np.float64)
    amplitude = (eps[:, :, None, :] * cpu.velocity_scale[None, None]).reshape(NC_M, NC_T, 2).numpy()
    z0 = to_db(torch.from_numpy(seq[3])[None])
    z_ref, maj = spectral_ar_reference(z0.numpy(), white.numpy(), rho.numpy(), NC_WINDOW)
    cells = SR.cell_majorant(maj, NC_SIZE, NC_SIZE, NC_WINDOW)
    origin, spacing = lattice_geometry(32, 16)
    moved = advect_series_perturbed_reference(z_ref.reshape(NC_M, NC_T, NC_SIZE, NC_SIZE).astype(np.float32), cpu.last_field.numpy(),
                                              unit_directions(cpu.last_field).numpy(), amplitude, origin, spacing, NC_M)
    moved = moved.reshape(1, NC_M, NC_T, NC_SIZE, NC_SIZE).transpose(1, 2, 0, 3, 4)
    return dict(frames=frames, white=white, eps=eps, rho=rho, want=want, field=cpu.last_field, amplitude=amplitude, z_ref=z_ref, cells=cells,
                moved=moved, pad=cpu.pad, threshold=cpu.threshold)


def largest_direction_gap(field, field_gap):
    """What a field difference of `field_gap` per component can do to a component of v / |v|: |d(v / |v|)| <= 2 |dv| / |v| with
    |dv| <= sqrt(2) field_gap and the lattice's smallest speed, plus one fp32 rounding of a value of at most 1."""
    speed = float(np.sqrt((np.asarray(field, dtype=np.float64) ** 2).sum(axis=-1)).min())
    return 2.0 * np.sqrt(2.0) * field_gap / speed + 2.0 ** -24


def nowcast_tolerances(case, field_gap, direction_gap):
    """The criterion of test_gpu_stochastic's device-against-CPU nowcast, its advection term extended by the direction lattice's gap
    times the largest sum over lead times of |a_par| + |a_perp| -> (compared bool [M, T, 1, H, W], tolerance of the rain rates,
    z tolerance)."""
    import stochastic_recipe as SR

    steps, size = NC_T, NC_SIZE
    tol_z = float((SR.K * SR.eps(NC_WINDOW) * case["cells"]).max())
    clean = np.where(case["z_ref"] >= 0, case["z_ref"], 0.0)
    padded = np.pad(clean, [(0, 0)] * 3 + [(1, 1)] * 2)
    adjacent = max(np.abs(np.diff(padded, axis=-1)).max(), np.abs(np.diff(padded, axis=-2)).max())
    amp_sum = float(np.abs(case["amplitude"].astype(np.float64)).sum(axis=(1, 2)).max())
    tol = tol_z + (PERTURBED_C * steps * size * 2.0 ** -24 + 2 * steps * field_gap + 2 * direction_gap * amp_sum) * adjacent \
        + 5 * 2.0 ** -24 * clean.max()
    compared = np.abs(case["moved"] - case["pad"]) > tol
    floor = np.maximum(case["want"], case["threshold"])
    # d rain / d z = rain ln(10) / 10; tol in z is small, so first order with a factor 2 of room, plus fp32 rounding of pow and log
    tol_rate = 2.0 * np.log(10.0) / 10.0 * tol * floor + 16 * 2.0 ** -24 * floor
    return compared, tol_rate, tol


def centroid(rain):
    """(y, x) of the rain-weighted centre of an [H, W] field, float64"""
    rain = np.asarray(rain, dtype=np.float64)
    y, x = np.meshgrid(np.arange(rain.shape[0]), np.arange(rain.shape[1]), indexing="ij")
    return np.array([(rain * y).sum(), (rain * x).sum()]) / rain.sum()
