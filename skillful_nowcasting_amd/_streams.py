"""Second-stream scheduling of the backward pass: weight gradients beside the data-gradient chain, and the joins that order the main
stream behind them (no host synchronisation anywhere)."""
from __future__ import annotations

import os
from typing import List

import torch

# Weight gradients off the critical path: the backward chain only needs each conv's DATA gradient; its weight gradient (window /
# im2col kernel, slab reduce, spectral-norm finalize - latency-bound kernels at 20-30 % matrix-pipe occupancy) runs on a second
# stream beside the data-gradient convs of the layers below.  The main stream joins it when the backward pass ends
# (autograd engine callback), i.e. before anything can read a .grad.
_SIDE_STREAMS = {}  # device index -> the device's ONE weight-gradient stream
_SIDE_PENDING = {}  # device index -> the main stream that has to wait for it
_SIDE_KEEP = []  # (event after the side work, tensors it reads)


_DEFER_JOIN = [0]


class defer_side_join:
    """Inside: the end of a backward pass does NOT make the main stream wait for the weight-gradient stream; the caller does, with
    join_side_streams(), before it reads a .grad - after putting work that does not need the gradients in between
    (DGMR.training_step: the generator forward of the next discriminator iteration runs beside the tail of the weight gradients)."""

    def __enter__(self):
        _DEFER_JOIN[0] += 1

    def __exit__(self, *exc):
        _DEFER_JOIN[0] -= 1


def _device_index(dev) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def join_side_streams():
    """The current stream waits for everything issued on its device's weight-gradient stream (no host synchronisation): parameter
    gradients are written by the kernels, not handed to autograd, so its own end-of-backward stream synchronisation does not
    cover them."""
    cur = torch.cuda.current_stream()
    side = _SIDE_STREAMS.get(cur.device.index)
    _tail_end_of_pass(cur, side)
    if side is not None:
        cur.wait_stream(side)
    _SIDE_PENDING.clear()
    _SIDE_KEEP.clear()


def _join_side_streams():
    if _DEFER_JOIN[0]:
        return
    if _SIDE_PENDING:
        idx0, main0 = next(iter(_SIDE_PENDING.items()))
        _tail_end_of_pass(main0, _SIDE_STREAMS[idx0])
    for idx, main in list(_SIDE_PENDING.items()):
        main.wait_stream(_SIDE_STREAMS[idx])
    _SIDE_PENDING.clear()
    _SIDE_KEEP.clear()  # everything the main stream does from here on is ordered behind the side work


# Tail balancing (round 6).  The weight-gradient stream runs behind the data-gradient chain all through a backward pass; when the chain
# ends, the main stream sits at the join with nothing to do while the side stream works off its backlog alone - rocprofv3 of the bench
# step: ONE gap of 58 ms at the end of the generator pass, 6.6 % of the step (profiles/r06_tails_kernel_streams.txt).  So the LAST weight
# gradients of a pass are issued on the main stream instead, behind the chain, and the two streams finish together.  Which ones: every
# call carries a cost (its multiply-adds); a pass (the calls between two joins) is recognised by its first calls' costs; at each join
# the wait is MEASURED (two events: the main stream reaching the join, the side stream running dry) and the pass's inline budget moves by
# half of it - a few steps to settle, no model of kernel speeds.  Same kernels, same operands, same order of gradient-buffer touches:
# results are bit-identical wherever a call runs.  DGMR_WGRAD_TAIL=0 switches it off.
_TAIL_ON = os.environ.get("DGMR_WGRAD_TAIL", "1") != "0"
_TAIL_KEY = 4  # a pass is keyed by the costs of its first calls


class _TailPass:
    """One backward pass being issued: costs of its side-stream calls so far, how much went inline, the events of its first side launch."""

    def __init__(self):
        self.costs: List[float] = []
        self.inline_cost = 0.0
        self.first_ev = None


class _TailProfile:
    """What is known about a recurring pass: its call costs, and the cost budget of the trailing calls that run on the main stream."""

    def __init__(self):
        self.costs: List[float] = []
        self.budget = 0.0
        self.pending = None  # (event main-at-join, event side-dry, event first side launch, side cost of that pass)
        self.history: List[float] = []  # measured waits (ms), newest last


_tail_pass = _TailPass()
_tail_profiles = {}


def tail_stats():
    """{pass key: (inline budget as a share of the pass's weight-gradient cost, the last measured waits in ms)} - for bench.py / tests."""
    out = {}
    for k, pr in _tail_profiles.items():
        tot = sum(pr.costs) or 1.0
        out[k] = (pr.budget / tot, list(pr.history[-6:]))
    return out


def _tail_inline(cost: float, inline_ok: bool) -> bool:
    """Called for every weight-gradient job: True = run it on the current (main) stream.  inline_ok=False: the job may use a scratch
    buffer that the side stream's jobs share (stream order is what protects it): it never leaves that stream."""
    ps = _tail_pass
    i = len(ps.costs)
    ps.costs.append(float(cost))
    if not _TAIL_ON or not inline_ok or i < _TAIL_KEY:
        return False
    pr = _tail_profiles.get(tuple(ps.costs[:_TAIL_KEY]))
    if pr is None or i >= len(pr.costs) or pr.costs[i] != ps.costs[i]:
        return False  # unknown pass, or it no longer follows the recorded one
    if sum(pr.costs[i:]) <= pr.budget:
        ps.inline_cost += float(cost)
        return True
    return False


def _tail_end_of_pass(main, side):
    """At a join, BEFORE the main stream is made to wait: close the pass, read the previous measurement of its profile, start a new one."""
    global _tail_pass
    ps, _tail_pass = _tail_pass, _TailPass()
    if not _TAIL_ON or len(ps.costs) <= _TAIL_KEY or side is None:
        return
    key = tuple(ps.costs[:_TAIL_KEY])
    pr = _tail_profiles.get(key)
    if pr is None:
        pr = _tail_profiles[key] = _TailProfile()
    if pr.pending is not None:
        ev_main, ev_side, ev_first, side_cost = pr.pending
        pr.pending = None
        if ev_side.query() and ev_main.query():
            wait = ev_main.elapsed_time(ev_side)  # > 0: the main stream waited that long for the side stream; < 0: the side stream was done first
            span = max(ev_first.elapsed_time(ev_side), 1e-3) if ev_first is not None else 0.0
            pr.history.append(round(wait, 2))
            if span > 0 and abs(wait) > 1.0:
                rate = side_cost / span  # cost the side stream works off per ms over the pass
                pr.budget = min(max(pr.budget + 0.5 * wait * rate, 0.0), 0.5 * sum(ps.costs))
    pr.costs = list(ps.costs)
    ev_main, ev_side = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ev_main.record(main)
    ev_side.record(side)
    pr.pending = (ev_main, ev_side, ps.first_ev, sum(ps.costs) - ps.inline_cost)


def _on_side_stream(dev, fn, tensors, inline_ok=True, cost=0.0):
    """Run fn() (kernel launches through _stream()) on the device's weight-gradient stream, ordered after everything issued so far on
    the current stream; `tensors`: what fn reads that the caller may free right after (kept alive for the side stream's work).
    cost: the job's multiply-adds - the tail balancer (above) runs the last jobs of a pass on the current stream instead, unless
    inline_ok=False (see _tail_inline)."""
    if _tail_inline(cost, inline_ok):
        fn()  # on the main stream, behind the chain: nothing to order, nothing to keep alive
        torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)
        return
    idx = _device_index(dev)
    main = torch.cuda.current_stream(dev)
    side = _SIDE_STREAMS.get(idx)
    if side is None:
        side = _SIDE_STREAMS[idx] = torch.cuda.Stream(device=dev)
    while _SIDE_KEEP and _SIDE_KEEP[0][0].query():
        _SIDE_KEEP.pop(0)
    side.wait_stream(main)
    if _TAIL_ON and _tail_pass.first_ev is None:
        _tail_pass.first_ev = torch.cuda.Event(enable_timing=True)
        _tail_pass.first_ev.record(side)
    with torch.cuda.stream(side):
        fn()
    tensors = tuple(t for t in tensors if isinstance(t, torch.Tensor))
    for t in tensors:
        t.record_stream(side)
    # A reference is held until the side work is done: autograd accumulates a second gradient INTO a buffered one in place when
    # nobody else holds it (InputBuffer) - e.g. the gradient this conv hands to its residual - and would overwrite dy on the main
    # stream under the weight-gradient kernel still reading it here.
    _SIDE_KEEP.append((side.record_event(), tensors))
    # a callback per call (the first to run joins, the rest find nothing pending): a backward pass that died on an exception must
    # not leave a stale "callback already queued" state behind
    _SIDE_PENDING[idx] = main
    torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)


def side_streams(device) -> List["torch.cuda.Stream"]:
    """The weight-gradient stream of `device` if it exists so far (ddp: a collective must be ordered behind it)."""
    side = _SIDE_STREAMS.get(_device_index(device))
    return [] if side is None else [side]
