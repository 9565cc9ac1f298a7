"""Adam through the fused HIP kernel (torch.optim.Adam semantics as used at dgmr/dgmr.py:292-300)."""
import math

import torch

from . import ops


class FusedAdam(torch.optim.Optimizer):
    """Adam(lr, betas, eps=1e-8, weight_decay=0, amsgrad=False); one HIP launch per parameter GROUP (dgmr_adam_multi).

    State layout (``step``, ``exp_avg``, ``exp_avg_sq``) matches torch.optim.Adam so optimiser checkpoints
    interchange.  Parameters that received no gradient are skipped, like torch does.

    Every step() makes ONE descriptor table over every parameter with a gradient in ALL groups (one pinned upload) and one Adam launch
    per group on that group's slice of it: plain, guarded and EMA steps differ only in the entry point.  For an optimiser with one
    group - both of DGMR's - that is the upload and the launch it always issued; one with several groups makes one upload per step
    where it used to make one per group.

    Gradient guard (off by default; with both options at their defaults step() issues exactly the launches it always did):

    * ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_(all parameters of this optimiser, max_grad_norm)`` applied inside the Adam
      launch - the update uses ``g * clip_coef``, ``p.grad`` itself is never rewritten;
    * ``skip_nonfinite``: if any gradient element is NaN / Inf, this step stores nothing (``p``, ``exp_avg``, ``exp_avg_sq`` keep their
      values).  ``state[p]["step"]`` still advances, on the host, for a skipped step: the bias corrections follow ATTEMPTED steps
      (the step never waits for the device, so the host cannot know; a device-side counter per parameter is not worth it).

    Both are plain attributes (not ``param_groups`` keys: ``state_dict()`` stays interchangeable with torch.optim.Adam) and may be
    changed between steps.  With either set, step() adds one norm pass over the table (dgmr_grad_norm_multi: one extra read of the
    gradients, deterministic, no host synchronisation) and launches dgmr_adam_multi_guarded on the slices.  Results stay on the device, as views into the guard's scratch that the next guarded
    step overwrites: ``last_grad_norm``, ``last_clip_coef``, ``skipped_steps`` (running count), ``last_tensor_grad_norms`` (float64,
    in the order of ``last_guarded_params``).  ``nonfinite_parameters()`` is the only method that synchronises.

    Weight EMA (off by default; with ``ema_decay`` unset step() issues exactly the launches it issues without it):

    * ``ema_decay``: None or a float in [0, 1).  Every step also moves a shadow of each stepped parameter,
      ``ema.lerp_(p, 1 - decay)`` as ``torch.optim.swa_utils.get_ema_multi_avg_fn`` does it, INSIDE the Adam launch
      (dgmr_adam_multi_ema in place of dgmr_adam_multi / dgmr_adam_multi_guarded: still one launch per group, one table upload);
    * ``ema_warmup``: the step uses ``min(decay, (1 + n) / (10 + n))`` with ``n = ema_num_updates`` before the step.

    Plain attributes like the guard's, and like the guard they need ``multi_tensor = True``.  A shadow is created the first time its
    parameter is stepped with EMA on, as a copy of the parameter BEFORE that update (same shape and strides); it lives outside
    ``self.state`` (``state_dict()`` stays torch.optim.Adam's; ``ema_state_dict()`` / ``load_ema_state_dict()`` carry the shadows).
    A parameter without a gradient in a step is not in that step's table: its shadow does not move in that step.  A parameter that
    was never stepped has no shadow: its average is the parameter itself.  ``ema_num_updates`` counts ATTEMPTED steps on the host, like
    ``state[p]["step"]``: a step the guard skips stores nothing to the shadows and still counts.  ``swap_ema()`` exchanges parameters
    and shadows in one launch (evaluation with the averaged weights; twice restores every bit).
    """

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, skip_nonfinite=False, ema_decay=None,
                 ema_warmup=False):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps))
        self.max_grad_norm = max_grad_norm
        self.skip_nonfinite = skip_nonfinite
        self.ema_decay = ema_decay
        self.ema_warmup = ema_warmup
        self._guard_active()
        self._ema_active()

    flat_grads = None  # set by ddp.GradSync users: gradients then live in one flat buffer that is zeroed, not dropped

    def zero_grad(self, set_to_none: bool = True):
        if self.flat_grads is not None:
            self.flat_grads.zero_()
            return
        super().zero_grad(set_to_none=set_to_none)

    RING = 4  # pinned descriptor tables in flight (see _upload_table)
    multi_tensor = True  # every tensor of a parameter group in ONE launch (dgmr_adam_multi); False: one dgmr_adam launch per tensor
    skip_nonfinite = False  # (class default: an optimiser restored by pickle has the guard off)
    ema_warmup = False
    ema_num_updates = 0  # steps attempted with EMA on (host counter)

    @property
    def max_grad_norm(self):
        return self.__dict__.get("_max_grad_norm")

    @max_grad_norm.setter
    def max_grad_norm(self, value):
        if value is not None:
            value = float(value)
            if not (math.isfinite(value) and value > 0.0):
                raise ValueError(f"max_grad_norm must be None or a finite float > 0, got {value}")
        self.__dict__["_max_grad_norm"] = value

    def _guard_active(self) -> bool:
        on = self.max_grad_norm is not None or bool(self.skip_nonfinite)
        if on and not self.multi_tensor:
            raise ValueError("the gradient guard (max_grad_norm / skip_nonfinite) needs multi_tensor = True")
        return on

    @property
    def ema_decay(self):
        return self.__dict__.get("_ema_decay")

    @ema_decay.setter
    def ema_decay(self, value):
        if value is not None:
            value = float(value)
            if not (0.0 <= value < 1.0):  # (NaN fails both comparisons)
                raise ValueError(f"ema_decay must be None or a float with 0 <= decay < 1, got {value}")
        self.__dict__["_ema_decay"] = value

    def _ema_active(self) -> bool:
        on = self.ema_decay is not None
        if on and not self.multi_tensor:
            raise ValueError("the weight EMA (ema_decay) needs multi_tensor = True")
        return on

    @staticmethod
    def ema_decay_at(decay: float, num_updates: int, warmup: bool) -> float:
        """The decay of the update that follows `num_updates` earlier ones: min(decay, (1 + n) / (10 + n)) under warm-up."""
        return min(decay, (1.0 + num_updates) / (10.0 + num_updates)) if warmup else decay

    @torch.no_grad()
    def step(self, closure=None):
        guarded = self._guard_active()
        ema_w = None  # 1 - decay of this step, in double (the kernel rounds it once)
        if self._ema_active():
            ema_w = 1.0 - self.ema_decay_at(self.ema_decay, self.ema_num_updates, bool(self.ema_warmup))
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        written = []
        rows, slices = [], []  # one table over all groups, (first row, rows, b1, b2, eps) per group
        for group in self.param_groups:
            b1, b2 = group["betas"]
            first = len(rows)
            for p in group["params"]:
                if p.grad is None:
                    continue
                written.append(p)
                ops.require_hip(p, "parameter")
                st = self.state[p]
                if len(st) == 0:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p)
                    st["exp_avg_sq"] = torch.zeros_like(p)
                st["step"] += 1
                g = p.grad
                if g.stride() != p.stride():  # kernels index raw storage: bring the gradient to the parameter's layout
                    g = torch.empty_like(p).copy_(g)
                if self.multi_tensor:
                    rows.append((p, g, st, group["lr"], b1, b2))
                else:
                    ops.adam_update(p, g, st["exp_avg"], st["exp_avg_sq"], st["step"], group["lr"], b1, b2, group["eps"])
            if len(rows) > first:
                slices.append((first, len(rows) - first, b1, b2, group["eps"]))
        if rows:
            self._step_multi(rows, slices, guarded, ema_w)
        if ema_w is not None and written:
            self.ema_num_updates += 1
        ops._core.note_optimizer_step(written)  # (the images of THESE weights are stale; everything else keeps its caches)
        return loss

    def _ring_slot(self, nbytes, device):
        """-> (pinned host bytes, device bytes, event) of the next table slot, at least `nbytes` long and free to be rewritten."""
        # The upload is asynchronous and the step never synchronises the host: a pinned table must not be rewritten before the copy
        # that reads it has executed (two step() calls per training step, several parameter groups per call).  A ring of pinned
        # tables, each with the event of its last copy; a slot is reused only after that event.
        ring = self.__dict__.setdefault("_desc_ring", [])
        turn = self.__dict__["_desc_turn"] = self.__dict__.get("_desc_turn", -1) + 1
        if len(ring) < self.RING:
            ring.append(None)
        slot = turn % len(ring)
        ent = ring[slot]
        if ent is None or ent[0].numel() < nbytes:
            if ent is not None:
                ent[2].synchronize()
            ent = ring[slot] = (torch.empty(nbytes, dtype=torch.uint8).pin_memory(),
                                torch.empty(nbytes, dtype=torch.uint8, device=device), torch.cuda.Event())
        else:
            ent[2].synchronize()  # (long done in practice: RING - 1 other uploads lie in between)
        return ent

    def _upload_table(self, rows, ema=False):
        """One descriptor per tensor (pointers, length, first workgroup, the two step-dependent scalars - torch keeps a step counter per
        parameter), uploaded as one pinned-memory copy.  The scalars are formed in double and rounded once, like dgmr_adam does.
        ema: the shadows' pointers (one uint64 per row) follow the descriptors in the same slot and travel in the same copy, so the
        ring's reuse rule covers them.  Rows of a swap carry p only (g = st = None).
        -> (device table, first workgroup of every row + the total)"""
        import numpy as np

        from ._lib import ADAM_DESC_DTYPE, load

        chunk = self.__dict__.get("_chunk")
        if chunk is None:
            chunk = self.__dict__["_chunk"] = int(load().dgmr_adam_chunk())
        n = len(rows)
        desc_bytes = n * ADAM_DESC_DTYPE.itemsize  # (56 n: the pointer array behind it is 8-byte aligned)
        nbytes = desc_bytes + (8 * n if ema else 0)
        host, dev, done = self._ring_slot(nbytes, rows[0][0].device)
        tab = np.frombuffer(host.numpy(), dtype=ADAM_DESC_DTYPE, count=n)
        block = 0
        block0 = []
        for i, (p, g, st, lr, b1, b2) in enumerate(rows):
            numel = p.numel()
            if st is None:
                tab[i] = (p.data_ptr(), 0, 0, 0, numel, block, 0.0, 0.0, 0)
            else:
                step = st["step"]
                tab[i] = (p.data_ptr(), g.data_ptr(), st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), numel, block,
                          np.float32(lr / (1.0 - b1 ** step)), np.float32(math.sqrt(1.0 - b2 ** step)), 0)
            block0.append(block)
            block += (numel + chunk - 1) // chunk
        block0.append(block)
        if ema:
            ptrs = np.frombuffer(host.numpy(), dtype=np.uint64, count=n, offset=desc_bytes)
            for i, row in enumerate(rows):
                ptrs[i] = self._shadow(row[0]).data_ptr()
        dev[:nbytes].copy_(host[:nbytes], non_blocking=True)
        done.record()
        return dev, block0

    def _step_multi(self, rows, slices, guarded, ema_w):
        """One table over all groups (one upload), the norm pass over all of it if the guard is on, then ONE Adam launch on every
        group's slice."""
        from ._lib import ADAM_DESC_DTYPE

        dev, block0 = self._upload_table(rows, ema=ema_w is not None)
        stream = ops._stream()
        guard = self._norm_pass(dev, rows, block0[-1], stream) if guarded else None
        shadows = dev.data_ptr() + len(rows) * ADAM_DESC_DTYPE.itemsize  # (the shadows' pointers follow the descriptors)
        for first, count, b1, b2, eps in slices:
            descs = dev.data_ptr() + first * ADAM_DESC_DTYPE.itemsize
            args = (count, block0[first + count] - block0[first], float(b1), float(b2), float(eps))
            if ema_w is not None:
                ops.call("dgmr_adam_multi_ema", descs, shadows + 8 * first, *args, ema_w, guard, stream)
            elif guarded:
                ops.call("dgmr_adam_multi_guarded", descs, *args, guard, stream)
            else:
                ops.call("dgmr_adam_multi", descs, *args, stream)

    # ------------------------------------------------------------------------------------------
    # weight EMA
    # ------------------------------------------------------------------------------------------
    def _param_index(self):
        """parameter -> its index in state_dict()["state"] (position over all groups)"""
        return {p: i for i, p in enumerate(q for group in self.param_groups for q in group["params"])}

    def _shadow(self, p, create=True):
        """The shadow of `p`.  A loaded one waits on the host until its parameter is on the device, then takes the parameter's device and
        strides; otherwise (create) a copy of the parameter as it is now."""
        shadows = self.__dict__.setdefault("_ema_shadows", {})
        e = shadows.get(p)
        if e is not None:
            return e
        loaded = self.__dict__.get("_ema_loaded")  # parameter -> loaded tensor (keyed once, in load_ema_state_dict)
        if loaded and p in loaded:
            if not p.is_cuda:
                return loaded[p]
            src = loaded.pop(p)
            e = shadows[p] = torch.empty_like(p, memory_format=torch.preserve_format, requires_grad=False).copy_(src)
            return e
        if not create:
            return None
        e = shadows[p] = p.detach().clone(memory_format=torch.preserve_format)
        return e

    def ema(self, p):
        """The shadow (the averaged weights) of parameter `p`, or None if `p` was never stepped with EMA on."""
        return self._shadow(p, create=False)

    @torch.no_grad()
    def swap_ema(self):
        """Exchange every parameter that has a shadow with it: ONE dgmr_swap_multi launch, then the weight images of exactly those
        parameters are marked stale.  -> the parameters swapped.  Calling it again restores every bit."""
        from ._lib import ADAM_DESC_DTYPE

        rows = [(p, None, None, 0.0, 0.0, 0.0) for group in self.param_groups for p in group["params"]
                if self._shadow(p, create=False) is not None]
        if not rows:
            return []
        for row in rows:
            ops.require_hip(row[0], "parameter")
        dev, block0 = self._upload_table(rows, ema=True)
        ops.call("dgmr_swap_multi", dev.data_ptr(), dev.data_ptr() + len(rows) * ADAM_DESC_DTYPE.itemsize, len(rows), block0[-1],
                 ops._stream())
        params = [row[0] for row in rows]
        ops._core.note_optimizer_step(params)
        return params

    def ema_state_dict(self):
        """{"num_updates": int, "shadows": {index: tensor}}, indexed like state_dict()["state"]; the tensors are copies."""
        out = {}
        for p, i in self._param_index().items():
            e = self._shadow(p, create=False)
            if e is not None:
                out[i] = e.detach().clone(memory_format=torch.preserve_format)
        return {"num_updates": int(self.ema_num_updates), "shadows": out}

    def load_ema_state_dict(self, state):
        """Replaces every shadow and the update count.  The tensors are kept (as copies, wherever they are) until their parameter is
        first used on the device - the optimiser is usually restored before model.to(device)."""
        params = [p for group in self.param_groups for p in group["params"]]
        shadows = {int(i): t for i, t in state["shadows"].items()}
        bad = [i for i in shadows if not 0 <= i < len(params)]
        if bad:
            raise ValueError(f"EMA state names parameters {bad}, the optimiser has {len(params)}")
        for i, t in shadows.items():
            if t.shape != params[i].shape:
                raise ValueError(f"EMA shadow of parameter {i} has shape {tuple(t.shape)}, the parameter {tuple(params[i].shape)}")
        self.__dict__["_ema_shadows"] = {}
        self.__dict__["_ema_loaded"] = {params[i]: t.detach().clone() for i, t in shadows.items()}
        self.ema_num_updates = int(state["num_updates"])

    # ------------------------------------------------------------------------------------------
    # gradient guard
    # ------------------------------------------------------------------------------------------
    def _norm_pass(self, dev, rows, blocks, stream):
        """dgmr_grad_norm_multi over the whole table -> the device address of the guard record the Adam launches read."""
        n, device = len(rows), rows[0][0].device
        d = self.__dict__
        if d.get("_guard") is None:  # 16 bytes, dgmr_grad_guard; allocated once (skipped_total lives in it)
            d["_guard"] = torch.zeros(4, dtype=torch.int32, device=device)
        if d.get("_partials") is None or d["_partials"].numel() < blocks:
            d["_partials"] = torch.empty(blocks, dtype=torch.float64, device=device)
        if d.get("_tensor_sq") is None or d["_tensor_sq"].numel() < n:
            d["_tensor_sq"] = torch.empty(n, dtype=torch.float64, device=device)
        ops.call("dgmr_grad_norm_multi", dev.data_ptr(), n, blocks, d["_partials"].data_ptr(), d["_tensor_sq"].data_ptr(),
                 float(self.max_grad_norm or 0.0), int(bool(self.skip_nonfinite)), d["_guard"].data_ptr(), stream)
        d["_guarded_params"] = [r[0] for r in rows]
        return d["_guard"].data_ptr()

    @property
    def last_grad_norm(self):
        """Global L2 norm of the gradients of the last guarded step: 0-d float32 device tensor, a view (None before the first)."""
        g = self.__dict__.get("_guard")
        return None if g is None else g[:2].view(torch.float32)[0]

    @property
    def last_clip_coef(self):
        """min(1, max_grad_norm / (norm + 1e-6)) of the last guarded step (1 without max_grad_norm): 0-d float32 device view."""
        g = self.__dict__.get("_guard")
        return None if g is None else g[:2].view(torch.float32)[1]

    @property
    def skipped_steps(self):
        """How many guarded steps were skipped so far: 0-d int32 device view."""
        g = self.__dict__.get("_guard")
        return None if g is None else g[3]

    @property
    def last_guarded_params(self):
        """The parameters the last guarded step ran over (those with a gradient), in table order."""
        return list(self.__dict__.get("_guarded_params", ()))

    @property
    def last_tensor_grad_norms(self):
        """Per-tensor L2 norms of the last guarded step in the order of last_guarded_params: float64 device tensor, the square root
        of a view into the scratch (no synchronisation)."""
        sq = self.__dict__.get("_tensor_sq")
        return None if sq is None else sq[:len(self.__dict__["_guarded_params"])].sqrt()

    def nonfinite_parameters(self, names=None):
        """The parameters of the last guarded step whose gradient held NaN / Inf (their per-tensor norm is not finite).  SYNCHRONISES
        the host.  names: optional (name, parameter) pairs, e.g. ``module.named_parameters()`` - the offenders' names are returned
        instead of the parameters."""
        norms = self.last_tensor_grad_norms
        if norms is None:
            return []
        bad = (~torch.isfinite(norms)).nonzero().flatten().tolist()
        params = [self.__dict__["_guarded_params"][i] for i in bad]
        if names is None:
            return params
        by_id = {id(p): name for name, p in names}
        return [by_id.get(id(p), "?") for p in params]
