import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """`gpu` tests are skipped (not failed) on hosts without a HIP device or without the built kernel library."""
    import torch

    lib = os.path.join(ROOT, "skillful_nowcasting_amd", "lib", "libdgmr_hip.so")
    if torch.cuda.is_available() and os.path.exists(lib):
        return
    why = "no HIP device" if not torch.cuda.is_available() else "libdgmr_hip.so not built"
    skip = pytest.mark.skip(reason=f"gpu test: {why}")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


def load_golden(name):
    """tests/golden/<name>.safetensors -> (tensors, metadata).  A fixture too large for one committed file is stored as
    consecutive byte ranges <name>.safetensors.part000, .part001, ... (oracle/gen_golden.py:save_file), joined here."""
    import glob
    import json
    import struct

    from safetensors.torch import load

    path = os.path.join(GOLDEN, name + ".safetensors")
    parts = [path] if os.path.exists(path) else sorted(glob.glob(path + ".part[0-9][0-9][0-9]"))
    assert parts, f"no golden fixture {path}"
    data = b"".join(open(p, "rb").read() for p in parts)
    meta = json.loads(data[8:8 + struct.unpack("<Q", data[:8])[0]]).get("__metadata__")
    return load(data), meta


def split_golden(rec):
    """-> (sd0, buf1, ins, outs, cots, grad_in, grad_p)"""
    sd0 = {k[4:]: v.clone() for k, v in rec.items() if k.startswith("sd0.")}
    buf1 = {k[5:]: v for k, v in rec.items() if k.startswith("buf1.")}
    n_in = len([k for k in rec if k.startswith("in.")])
    ins = [rec[f"in.{i}"] for i in range(n_in)]
    n_out = len([k for k in rec if k.startswith("out.")])
    outs = [rec[f"out.{i}"] for i in range(n_out)]
    cots = [rec[f"cot.{i}"] for i in range(n_out)]
    grad_in = {int(k.split(".")[-1]): v for k, v in rec.items() if k.startswith("grad.in.")}
    grad_p = {k[7:]: v for k, v in rec.items() if k.startswith("grad.p.")}
    return sd0, buf1, ins, outs, cots, grad_in, grad_p


import torch  # noqa: E402


def assert_init_fingerprints(got, ref, keys):
    """A seeded construction against the reference's fingerprints: rows (sum, abs-sum, first, last) in float64, one per key.
    Parameters and BatchNorm buffers come straight from the seeded generator / constants and must match element for element: first
    and last exactly, the sums to float64 summation order (1e-13 of the abs-sum).  The spectral-norm vectors `._u` / `._v` are the
    result of float32 power iterations (matrix-vector products, normalisations) whose rounding depends on the host CPU's vector code
    path - the reference's own values differ between hosts - so they must match to float32 rounding: the sums to 1e-5 of the abs-sum,
    single elements of these unit vectors to 1e-6."""
    bad = []
    for i, k in enumerate(keys):
        s, a, first, last = got[i].tolist()
        rs, ra, rfirst, rlast = ref[i].tolist()
        if k.endswith(("._u", "._v")):
            ok = abs(s - rs) <= 1e-5 * ra + 1e-7 and abs(a - ra) <= 1e-5 * ra + 1e-7 and abs(first - rfirst) <= 1e-6 and abs(last - rlast) <= 1e-6
        else:
            ok = first == rfirst and last == rlast and abs(s - rs) <= 1e-13 * ra and abs(a - ra) <= 1e-13 * ra
        if not ok:
            bad.append((k, got[i].tolist(), ref[i].tolist()))
    assert not bad, f"seeded construction differs from the reference's in {len(bad)} tensors, e.g. {bad[:3]}"


def rel_err(a, b):
    return (a.double() - b.double()).abs().max().item() / max(b.double().abs().max().item(), 1e-300)


def cos_sim(a, b):
    if b.numel() < 2:
        return 1.0
    return torch.nn.functional.cosine_similarity(a.flatten().double(), b.flatten().double(), dim=0).item()


BAND_LOG = os.environ.get("DGMR_BAND_LOG", os.path.join(ROOT, "gpurun_out", "band_tables.log"))


def _log_band(msg):
    """Every band table of a run is appended to one file (gpurun_out/ travels back from the GPU box; the final tree's copy is
    committed under profiles/): the measured errors are evidence whether or not a test fails."""
    try:
        os.makedirs(os.path.dirname(BAND_LOG), exist_ok=True)
        with open(BAND_LOG, "a") as f:
            f.write(msg + "\n\n")
    except OSError:
        pass


def band_check(what, precision, tol, rows, factor=None, flips_row=False):
    """rows: {name: (hip, ref32, ref64)}.  The HIP result must be within max(tol, 3 x the error of the reference's OWN fp32 arithmetic)
    of the float64 truth (max-abs error over the tensor's max magnitude; 1 - cosine within max(1e-4, 10 x fp32's)): where fp32
    itself is ill-conditioned (BatchNorm batch statistics over a handful of elements at B = 1, cancelling weight-gradient sums) a
    fixed 1e-3 would test the conditioning of the problem, not the kernels.  ref32 / ref64: the CPU oracle run in float32 (the
    reference's arithmetic) and in float64 on the same inputs and state.
    `factor` (default 3; 10 where 16-bit products are involved: "bf16x3", "mixed"): the exact-f32 kernels measure at 0.7 ... 1.7 x the
    fp32 oracle's own error everywhere; bf16x3 forms every product from 16 significant bits (2^-16 instead of 2^-24 per product),
    which an ill-conditioned backward amplifies to 2 ... 8 x the fp32 error on deep-layer gradients while the forward stays at 3e-4.
    Isolated ReLU-boundary flips: a pre-activation within ~1e-7 of zero falls on the other side of the kink under another fp32
    summation order and its whole gradient toggles; behind batch-statistics BatchNorm over a handful of samples the gradients are
    heavy-tailed, so ONE flipped element can move a max-abs comparison by 5e-2 while every other element agrees to 1e-6 (the
    unmodified reference shows the same between CPU thread counts, tests/golden/training_steps_adv `noise.*`).  They are accepted
    by COUNT, never by a norm: at most 0.1 % of a tensor's elements may exceed the bound (`flips_row`: or one output channel's worth -
    one bias element, one weight row - where the oracle cannot be aligned to the implementation's relu masks, see KinkAligner), none
    by more than 100 x, and the cosine criterion still applies - a uniform error of any size (every element beyond the bound) fails."""
    if factor is None:
        factor = 10.0 if precision in ("bf16x3", "mixed") else 3.0
    table, bad = [], []
    for k, (hip, r32, r64) in rows.items():
        e_hip, e_ref = rel_err(hip, r64), rel_err(r32, r64)
        c, c_ref = cos_sim(hip, r64), cos_sim(r32, r64)
        f_k = factor * (2.0 if r64.numel() == 1 else 1.0)  # a single element (attention gamma): nothing to take a max over
        bound = max(tol, f_k * e_ref)
        cbound = max(1e-4, 10.0 * factor * (1.0 - c_ref))
        scale = max(r64.double().abs().max().item(), 1e-300)
        over = ((hip.double() - r64.double()).abs() / scale > bound)
        n_over = int(over.sum().item())
        # one flipped activation reaches one output channel: one element of a bias gradient, one row of a weight gradient
        row = r64.numel() // r64.shape[0] if r64.dim() >= 2 else 1
        allowed = max(int(1e-3 * r64.numel()), row) if flips_row else int(1e-3 * r64.numel())
        l2 = ((hip.double() - r64.double()).pow(2).sum().sqrt() / r64.double().pow(2).sum().sqrt().clamp_min(1e-300)).item()
        within = e_hip <= bound
        flips = (not within) and n_over <= allowed and e_hip <= 100.0 * bound
        ok = (within or flips) and 1.0 - c <= cbound
        table.append(f"  {k:88s} hip {e_hip:.2e}  ref-fp32 {e_ref:.2e}  bound {bound:.2e}  1-cos {1 - c:.1e} (ref-fp32 {1 - c_ref:.1e})  l2 {l2:.1e}"
                     + ("" if within else f"  [{n_over} of {r64.numel()} elements beyond the bound" + (": accepted as isolated flips]" if ok else "]  FAIL")))
        if not ok:
            bad.append(k)
    msg = f"{what} [{precision}] errors against the float64 oracle:\n" + "\n".join(table)
    print("\n" + msg)
    _log_band(msg)
    assert not bad, f"beyond the bound: {bad}\n{msg}"


class KinkAligner:
    """Evaluate the oracle's discriminator on the linear piece the HIP forward was on.

    relu makes the discriminator piecewise linear.  Two correct fp32 implementations agree on the piece except where a
    pre-activation lies within rounding of zero; with millions of activations a handful always do.  On the 4 x 4 and 2 x 2 maps in
    front of the heads - and behind their BatchNorm1d, which divides by the batch spread - ONE such element moves every gradient below
    it by 1e-3 ... 1e-2 of its size, densely: no element-wise tolerance can tell that from a real defect.  So the comparison is made
    rigorous instead of tolerant: the implementation's own relu masks are captured (forward hooks on its D-blocks) and the oracle is
    run with `x * mask` in place of `relu(x)` at the same places (oracle.RELU_HOOK).  Both sides then evaluate the SAME smooth
    function and the float64-anchored band applies with no allowance for flips.  `report()` lists how many mask elements differ
    from the sign of the oracle's own pre-activations and how close to zero those are (they must be: a disagreement at a large
    pre-activation is a forward error, which the scores / the forward comparison would show).

    Usage:  with KinkAligner(model.discriminator) as ka:  out = model.discriminator(x) ...
            with ka.oracle(O):  ref = O.discriminator(sd, "", x, idxs, True)
    Only the FIRST call of the module that is seen is captured / aligned (`calls` discriminator calls of one step: the first)."""

    def __init__(self, disc, prefix=""):
        self.disc = disc
        self.prefix = prefix  # the discriminator's prefix in the oracle's state dict ("" or "discriminator.")
        self.masks = {}
        self.hooks = []
        self.mismatch = {}

    def __enter__(self):
        from skillful_nowcasting_amd.common import DBlock

        def keep(tag, t):
            tag = self.prefix + tag
            if tag not in self.masks:
                self.masks[tag] = (t.detach() > 0).cpu()

        for name, m in self.disc.named_modules():
            if not isinstance(m, DBlock):
                continue
            if m.first_relu:
                self.hooks.append(m.register_forward_pre_hook(lambda mod, args, n=name: keep(n + ".in", args[0])))
            self.hooks.append(m.first_conv_3x3.register_forward_hook(lambda mod, args, out, n=name: keep(n + ".mid", out)))
            if name.endswith((".d6", ".d_last")):  # the block in front of a head: its output is what relu_sum_hw sees
                head = name.rsplit(".", 1)[0]
                self.hooks.append(m.register_forward_hook(lambda mod, args, out, n=head: keep(n + ".head", out)))
        return self

    def __exit__(self, *exc):
        for h in self.hooks:
            h.remove()
        self.hooks = []

    def oracle(self, O):
        aligner = self

        class _Scope:
            def __enter__(self_):
                counters = {}

                def hook(x, tag):
                    mask = aligner.masks.get(tag)
                    if mask is None:
                        return torch.relu(x)
                    n = x.shape[0]
                    i = counters.get(tag, 0)
                    if (i + 1) * n > mask.shape[0]:
                        return torch.relu(x)  # a later call of the module: not aligned
                    counters[tag] = i + 1
                    m = mask[i * n:(i + 1) * n]
                    assert m.shape == x.shape, (tag, tuple(m.shape), tuple(x.shape))
                    own = x.detach() > 0
                    diff = own != m
                    if diff.any():
                        scale = x.detach().abs().max().item()
                        rec = aligner.mismatch.setdefault((tag, str(x.dtype)), [0, 0.0])
                        rec[0] += int(diff.sum().item())
                        rec[1] = max(rec[1], (x.detach().abs()[diff].max().item() / max(scale, 1e-300)))
                    return x * m.to(x.dtype)

                O.RELU_HOOK = hook
                return self_

            def __exit__(self_, *exc):
                O.RELU_HOOK = None

        return _Scope()

    def report(self):
        """[(tag, dtype, elements on the other side of the kink, their largest |pre-activation| / max|pre-activation|)]"""
        return sorted((t, d, n, r) for (t, d), (n, r) in self.mismatch.items())
