"""Float64 specification of the spectral-norm call sequences (csrc/spectral_norm.hip) and the table of cases that the host and the
GPU tests share.  Plain torch on the CPU; the arithmetic runs in the dtype of the weight matrix that is handed in, so the same two
functions give the float64 truth and the float32 yardstick.

A spectral-norm module advances its power iteration once per train-mode CALL (torch/nn/utils/parametrizations.py, _power_method):

    u = normalize(W v, eps),  v = normalize(W^T u, eps),  sigma = u^T W v          normalize(x, eps) = x / max(||x||, eps)

`power_iterations` states exactly that.  `gram_iterations` states what the sequence kernels compute instead (the comment blocks
above SN_TMAX and sn_iter_multi_kernel): with A = W W^T the chain never touches W between the first and the last launch,

    u_0 = W v / max(||W v||, eps)
    y_t = A u_t,  n_t^2 = u_t^T y_t,  d_t = max(n_t, eps),  v_t = W^T u_t / d_t,  sigma_t = n_t^2 / d_t,
    u_{t+1} = (y_t / d_t) / max(||y_t|| / d_t, eps)

Both return the values of every call in CALL order; `to_group_order` moves them to the group of the batched launch that each call
belongs to (ops.CallLayout.slots()), which is how nn.SNPlan.run() hands them out.
"""
import torch


def normalize(x, eps):
    """torch.nn.functional.normalize(x, dim=0, eps=eps) of a vector."""
    return x / x.norm().clamp_min(eps)


def power_iterations(W2d, u, v, calls, eps):
    """`calls` train-mode calls of torch's spectral_norm on the [Cout, K] matrix from the state (u, v).
    -> sigma [calls], u [calls, Cout], v [calls, K]: what call c computed its weight with (and left in the buffers)."""
    W = W2d
    u, v = u.to(W.dtype), v.to(W.dtype)
    sig, us, vs = [], [], []
    for _ in range(calls):
        u = normalize(torch.mv(W, v), eps)
        v = normalize(torch.mv(W.t(), u), eps)
        sig.append(torch.dot(u, torch.mv(W, v)))
        us.append(u)
        vs.append(v)
    return torch.stack(sig), torch.stack(us), torch.stack(vs)


def gram_iterations(W2d, u, v, calls, eps):
    """The same sequence in the Gram form of dgmr_spectral_sigma_seq_multi (`u` is not read: the first call overwrites it)."""
    W = W2d
    v = v.to(W.dtype)
    A = W @ W.t()
    t0 = torch.mv(W, v)
    u = t0 / t0.norm().clamp_min(eps)
    sig, us, vs = [], [], []
    for _ in range(calls):
        y = torch.mv(A, u)
        n2 = torch.dot(u, y)
        d = n2.clamp_min(0).sqrt().clamp_min(eps)
        sig.append(n2 / d)
        us.append(u)
        vs.append(torch.mv(W.t(), u) / d)
        u = (y / d) / (y.norm() / d).clamp_min(eps)
    return torch.stack(sig), torch.stack(us), torch.stack(vs)


def to_group_order(per_call, layout):
    """per_call[c] -> out[layout.slots()[c]] (layout None: call c is group c)."""
    if layout is None:
        return per_call.clone()
    slots = torch.tensor(layout.slots(), dtype=torch.long)
    assert sorted(slots.tolist()) == list(range(per_call.shape[0]))
    out = torch.empty_like(per_call)
    out[slots] = per_call
    return out


def rel_per_call(got, ref):
    """Worst over the calls of max |got - ref| / max |ref| within the call (a scalar per call: its relative error)."""
    got, ref = got.double().reshape(ref.shape[0], -1), ref.double().reshape(ref.shape[0], -1)
    return ((got - ref).abs().amax(1) / ref.abs().amax(1).clamp_min(1e-300)).max().item()


# ---- the cases: the smallest shapes that cross each boundary of the sequence kernels ------------------------------------------------------
# name -> (kind, constructor arguments, calls, call layout (outer, inner, time_major, reverse) or None, weight scale, eps)
CASES = {
    "a": ("conv", dict(in_channels=4, out_channels=33, kernel_size=3, ndim=3), 33, None, 1.0, 1e-12),  # SN_TMAX + 1, SN_RB + 1 rows, K = 108
    "b": ("conv", dict(in_channels=8, out_channels=72, kernel_size=1), 65, None, 1.0, 1e-12),  # chunks 32 | 32 | 1, 64 + 8 rows, K = 8
    "c": ("linear", dict(in_features=260), 5, None, 1.0, 1e-12),  # a one-row matrix
    "d": ("conv", dict(in_channels=36, out_channels=100, kernel_size=3), 108, (6, 18, True, True), 1.0, 1e-12),  # the sampler's own map
    "e": ("conv", dict(in_channels=36, out_channels=100, kernel_size=3), 24, (6, 4, False, True), 1.0, 1e-12),  # draw-major map
    "f": ("conv", dict(in_channels=8, out_channels=40, kernel_size=3), 2, None, 1e-5, 1e-4),  # both max(||.||, eps) clamps engaged
    "g": ("conv", dict(in_channels=8, out_channels=16, kernel_size=3), 1, None, 1.0, 1e-12),  # t > T early exit beside longer sequences
}
JOINT_ORDER = ("d", "c", "a", "g", "b", "f", "e")
# weights as _conv_init leaves them / with a planted rank-one part three times the largest singular value.  "plain" has close singular
# values: consecutive calls still move u by 7e-4 ... 1e-2 at the END of a run (d: call 108), so a call read at the wrong slot or a
# chunk walked in the wrong order shows anywhere in the sequence; "gap" converges within a dozen calls and is the well-conditioned case.
VARIANTS = ("plain", "gap")


def case_layout(name):
    from skillful_nowcasting_amd.ops import CallLayout

    lay = CASES[name][3]
    return None if lay is None else CallLayout(*lay)


def build_case(name, variant):
    """-> (module on the CPU in train mode, calls, layout, W2d float64, u0, v0 float32).  The module's weight is exactly W2d (values
    chosen in float32), and its _u / _v are seeded random unit vectors: after the constructor's 16 warm-up iterations the vectors are
    nearly converged and a skipped, repeated or reordered call would move them by less than the tolerance."""
    from skillful_nowcasting_amd import ops
    from skillful_nowcasting_amd.nn import SNConv, SNLinear1

    kind, kw, calls, _, scale, eps = CASES[name]
    seed = 1000 + 17 * sorted(CASES).index(name) + VARIANTS.index(variant)
    torch.manual_seed(seed)  # (the constructors draw from the global generator)
    g = torch.Generator().manual_seed(seed + 500)
    m = SNConv(eps=eps, **kw) if kind == "conv" else SNLinear1(eps=eps, **kw)
    w = m.weight_orig
    w2d = w.detach().flatten(1).clone()  # logical [Cout, Cin * taps] in OIHW order: the order of torch's own weight matrix and of _v
    cout, k = w2d.shape
    if variant == "gap":
        a = normalize(torch.randn(cout, generator=g), 0.0)
        b = normalize(torch.randn(k, generator=g), 0.0)
        top = torch.linalg.matrix_norm(w2d.double(), 2).item()
        w2d = w2d + float(3.0 * top) * torch.outer(a, b)
    w2d = (w2d * scale).float()
    with torch.no_grad():
        w.copy_(w2d.view(w.shape))
    ops.bump_weights_epoch()
    vec = getattr(m.parametrizations.weight, "0")
    u0 = normalize(torch.randn(cout, generator=g), 0.0).float()
    v0 = normalize(torch.randn(k, generator=g), 0.0).float()
    with torch.no_grad():
        vec._u.copy_(u0)
        vec._v.copy_(v0)
    assert torch.equal(m.weight_orig.detach().flatten(1), w2d)
    return m.train(), calls, case_layout(name), w2d.double(), u0, v0


def expected_clamps(W64, u0, v0, calls, eps):
    """How many of the 2 * calls normalisations of the sequence divide by eps instead of the norm (case f: all of them)."""
    n, u, v = 0, u0.double(), v0.double()
    for _ in range(calls):
        t = torch.mv(W64, v)
        n += int(t.norm().item() < eps)
        u = normalize(t, eps)
        s = torch.mv(W64.t(), u)
        n += int(s.norm().item() < eps)
        v = normalize(s, eps)
    return n


def f32_yardstick(W64, u0, v0, calls, eps):
    """Errors of the plain recurrence run in float32 torch on the CPU against float64: (sigma, u, v), each the worst over the calls."""
    s64, u64, v64 = power_iterations(W64, u0, v0, calls, eps)
    s32, u32, v32 = power_iterations(W64.float(), u0, v0, calls, eps)
    return rel_per_call(s32, s64), rel_per_call(u32, u64), rel_per_call(v32, v64)
