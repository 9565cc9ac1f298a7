"""Inputs and helpers of the Lucas-Kanade tests (numpy and the package's CPU paths): a band-limited field that a phase ramp
translates exactly by any (dy, dx), periodically; stripes, which show no motion along themselves; the per-block vectors of both
sub-pixel methods; the forecast error of a translating sequence."""
import numpy as np
import torch

from skillful_nowcasting_amd import advection as A
from skillful_nowcasting_amd.stochastic import EnsembleAdvectionNowcaster

CUT = {32: 0.05, 16: 0.1}  # block -> cut-off in cycles per pixel
MIN_RATIO = 0.05           # every wet block of the fields below has lambda_min / lambda_max above this (eig_ratio is 0.01)
_SPECTRA = {}


def _spectrum(seed, h, w, cut):
    """The filtered spectrum of the seeded noise and the standard deviation of its field, once per process."""
    key = (seed, h, w, cut)
    if key not in _SPECTRA:
        noise = np.random.default_rng(seed).standard_normal((h, w))
        ky, kx = np.fft.fftfreq(h)[:, None], np.fft.fftfreq(w)[None, :]
        spec = np.fft.fft2(noise) * np.exp(-((ky * ky + kx * kx) / (cut * cut)))
        _SPECTRA[key] = (spec, ky, kx, np.fft.ifft2(spec).real.std())
    return _SPECTRA[key]


def field(seed, h, w, cut, shift=(0.0, 0.0)):
    """float32 [h, w]: white noise of `default_rng(seed)` times exp(-(k / cut)^2) in Fourier space (k in cycles per pixel), moved by
    `shift` = (dy, dx) with a phase ramp (out[y][x] = field[y - dy][x - dx], exact and periodic), scaled by the unmoved field's
    standard deviation, then max(4 x + 2, 0)."""
    spec, ky, kx, std = _spectrum(seed, h, w, cut)
    a = np.fft.ifft2(spec * np.exp(-2j * np.pi * (ky * shift[0] + kx * shift[1]))).real / std
    return np.maximum(4.0 * a + 2.0, 0.0).astype(np.float32)


def sequence(seed, h, w, frames, v, cut):
    """[frames, h, w]: frame t is the field moved by t v."""
    return np.stack([field(seed, h, w, cut, (t * v[0], t * v[1])) for t in range(frames)])


def stripes(h, w, shift=0.0, period=23.0):
    """float32 [h, w]: 3 + 3 sin(2 pi (x - shift) / period), every row the same bits - no gradient along y at all."""
    row = (3.0 + 3.0 * np.sin(2.0 * np.pi * (np.arange(w) - shift) / period)).astype(np.float32)
    return np.ascontiguousarray(np.broadcast_to(row, (h, w)))


def usable_blocks(match):
    """bool [N, By, Bx]: `motion_field`'s rule - not dry and an interior minimum."""
    return np.isfinite(np.asarray(match.cost)).all(axis=-1)


def inner_blocks(shape):
    """bool [By, Bx]: the blocks that are not on the lattice's border."""
    m = np.zeros(shape, bool)
    m[1:-1, 1:-1] = True
    return m


def parabola_vectors(match):
    """float64 [N, By, Bx, 2]: the integer match plus `motion_field`'s parabola per axis (its own `_subpixel`); meaningful on usable blocks."""
    c = torch.as_tensor(np.nan_to_num(np.asarray(match.cost, dtype=np.float64), posinf=0.0))
    sub = torch.stack([A._subpixel(c[..., 0], c[..., 1], c[..., 2]), A._subpixel(c[..., 0], c[..., 3], c[..., 4])], dim=-1)
    return np.asarray(match.disp, dtype=np.float64) + sub.numpy()


def eig_ratio_of(eig):
    eig = np.asarray(eig)
    return eig[..., 0] / np.where(eig[..., 1] > 0, eig[..., 1], 1.0)


def central_mae(forecast, truth, size=64):
    """mean |forecast - truth| over the central size x size of [..., H, W] arrays, per leading index"""
    h, w = truth.shape[-2:]
    ys, xs = slice((h - size) // 2, (h + size) // 2), slice((w - size) // 2, (w + size) // 2)
    return np.abs(np.asarray(forecast, dtype=np.float64)[..., ys, xs] - np.asarray(truth, dtype=np.float64)[..., ys, xs]).mean(axis=(-1, -2))


# ---- the end-to-end case: 192 x 192 moving by (2.3, -1.6) per frame, 4 context frames, 18 lead times ---------------------------------
E2E = dict(seed=7, size=192, v=(2.3, -1.6), context=4, leads=18, cut=CUT[32])
_E2E = {}


def e2e_frames():
    """-> (context float32 [4, 192, 192], truth float32 [18, 192, 192]), read-only, once per process."""
    if not _E2E:
        c = E2E
        seq = sequence(c["seed"], c["size"], c["size"], c["context"] + c["leads"], c["v"], c["cut"])
        seq.setflags(write=False)
        _E2E["seq"] = seq
    seq = _E2E["seq"]
    return seq[:E2E["context"]], seq[E2E["context"]:]


def subpixel_errors(refine, shift):
    """-> (largest |v - shift| of the refinement, of the parabola) over the usable blocks off the lattice border, 128 x 128, block 32.
    refine(prev, nxt) -> (match, v [1, By, Bx, 2], eig [1, By, Bx, 2]), numpy or CPU tensors."""
    prev, nxt = field(7, 128, 128, CUT[32])[None], field(7, 128, 128, CUT[32], shift)[None]
    match, v, eig = refine(prev, nxt)
    assert (eig_ratio_of(eig)[np.isfinite(np.asarray(match.cost)[..., 0])] >= MIN_RATIO).all()
    blocks = usable_blocks(match)[0] & inner_blocks(match.disp.shape[1:3])
    assert blocks.sum() >= 20, blocks.sum()
    truth = np.array(shift)
    err_lk = np.abs(np.asarray(v, dtype=np.float64)[0][blocks] - truth).max()
    err_par = np.abs(parabola_vectors(match)[0][blocks] - truth).max()
    print(f"shift {shift}: {int(blocks.sum())} blocks, largest error lk {err_lk:.4f} px, parabola {err_par:.4f} px, ratio {err_lk / err_par:.3f}")
    return err_lk, err_par


def half_striped_frames():
    """[4, 128, 256]: the left half the isotropic field moving by (2.3, -1.6) per frame, the right half stripes moving by 1.4 in x."""
    iso = sequence(7, 128, 128, 4, (2.3, -1.6), CUT[32])
    return np.stack([np.concatenate([iso[t], stripes(128, 128, 1.4 * t)], axis=1) for t in range(4)])


def check_aperture(field_lk, field_par):
    """fields [By, Bx, 2] of the half-striped frames: nodes 9 ... are blocks of stripes only (x0 >= 144)"""
    striped = slice(9, None)
    vy_lk, vy_par = np.asarray(field_lk)[:, striped, 0], np.asarray(field_par)[:, striped, 0]
    print(f"along-stripe motion in the striped half: lk {vy_lk.mean():.3f}, parabola {vy_par.mean():.3f}; the isotropic half moves by 2.3")
    assert (np.abs(vy_par) < np.abs(vy_lk) - 1.0).all()  # the parabola's false zero against the neighbours' vector carried in


def e2e_errors(device="cpu"):
    """-> {method: (MAE at leads 1 ... 18 of AdvectionNowcaster, of an advection along EnsembleAdvectionNowcaster's last_field)}"""
    context, truth = e2e_frames()
    frames = torch.from_numpy(np.array(context))[..., None].to(device)  # [T_in, H, W, C]
    out = {}
    for method in ("parabola", "lk"):
        plain = A.AdvectionNowcaster(forecast_steps=E2E["leads"], subpixel=method)
        fc = plain.nowcast(frames)
        ens = EnsembleAdvectionNowcaster(forecast_steps=E2E["leads"], window=64).refine_motion(method)
        ens.nowcast(frames, 1)
        assert ens.params["subpixel"] == method and torch.equal(ens.last_field, plain.last_field)
        origin, spacing = A.lattice_geometry(32, 16)
        moved = A.advect(frames[-1, :, :, 0][None].contiguous(), ens.last_field, E2E["leads"], origin, spacing)
        out[method] = (central_mae(fc[0, :, 0].cpu().numpy(), truth), central_mae(moved[0].cpu().numpy(), truth))
        inner = plain.last_field[0, 1:-1, 1:-1].double().cpu()
        print(f"{method}: field mean {inner.mean(dim=(0, 1)).tolist()}, largest error "
              f"{(inner - torch.tensor(E2E['v'], dtype=torch.float64)).abs().max().item():.4f} px/frame; MAE lead 1 {out[method][0][0]:.4f}, "
              f"lead 9 {out[method][0][8]:.4f}, lead 18 {out[method][0][17]:.4f}")
    return out


def check_e2e(errors):
    for which in (0, 1):  # the nowcaster's forecast, the ensemble's field
        lk, par = errors["lk"][which], errors["parabola"][which]
        assert lk[17] <= 0.25 * par[17], (lk[17], par[17])
        assert lk[0] <= par[0], (lk[0], par[0])


# ---- the parity cases shared by the host and the GPU tests: name -> (block, stride, radius, H, W) --------------------------------------
PARITY_CASES = {"84x100 32/16": (32, 16, 8, 84, 100), "44x52 16/8": (16, 8, 4, 44, 52)}
_PARITY = {}


def parity_case(name):
    """-> (prev, nxt) float32 [N, H, W], read-only.  Planes: 0 a sub-pixel translation; 1 a translation whose match puts the +-1
    window of the blocks at a frame corner outside the frame, with a NaN / negative patch; 2 (block 32 only) a dry quarter;
    last: stripes, which are not conditioned."""
    if name not in _PARITY:
        block, _stride, _radius, h, w = PARITY_CASES[name]
        cut, seed = CUT[block], 7
        big = 128  # the periodic field is made at 128^2 and cut, so the frame's edge is no seam
        planes = [(field(seed, big, big, cut)[:h, :w], field(seed, big, big, cut, (1.3, -0.6))[:h, :w])]
        p, q = field(seed + 1, big, big, cut)[:h, :w].copy(), field(seed + 1, big, big, cut, (-0.25, 0.35))[:h, :w].copy()
        p[5:9, 7:12], q[6:8, 20:23] = np.nan, -1.0
        planes.append((p, q))
        if block == 32:
            p, q = field(seed + 2, big, big, cut)[:h, :w].copy(), field(seed + 2, big, big, cut, (2.0, 0.5))[:h, :w].copy()
            p[:h // 2, :w // 2], q[:h // 2, :w // 2] = 0.0, 0.0
            planes.append((p, q))
        planes.append((stripes(h, w, 1.4), stripes(h, w)))
        prev, nxt = np.stack([a for a, _ in planes]), np.stack([b for _, b in planes])
        prev.setflags(write=False)
        nxt.setflags(write=False)
        _PARITY[name] = (prev, nxt)
    return _PARITY[name]


_PARITY_REF = {}


def parity_reference(name, iterations):
    """-> (BlockMatch, LkRefine) of the float64 specifications, once per process."""
    key = (name, iterations)
    if key not in _PARITY_REF:
        block, stride, radius = PARITY_CASES[name][:3]
        prev, nxt = parity_case(name)
        match = A.block_match_reference(prev, nxt, block, stride, radius, 0.1, block * block // 16)
        _PARITY_REF[key] = (match, A.lk_refine_reference(prev, nxt, match.disp, match.cost, block, stride, iterations))
    return _PARITY_REF[key]
