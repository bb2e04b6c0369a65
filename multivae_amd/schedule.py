"""The host step scheduler: which stream each launch of a training step goes to and which edges a captured step gets.

Two kinds of state live here and nowhere else.  What belongs to ONE step — the streams that hold late leaves, the postponed
closures, the loss assembly's ordering, the branch streams of the forward pass, the open OverlapPoint / Rotation — is a plain
attribute of that step's `deferred_reductions` scope, created on entry, registered in `_OPEN` and gone on exit: nothing a step
leaves behind reaches the next one.  What outlives a step (scratch, arenas, streams, constants whose addresses captured graphs
hold) is the block of device-lifetime caches below.  New step state goes on the scope, never into a module-level container.

kernels.py (the launch helpers and autograd Functions) calls into this module; this module launches no kernel of its own
beyond the deferred finishes.
"""
import ctypes as C
import os

import torch

from . import _lib
from ._lib import call, ptr, stream_ptr

# -----------------------------------------------------------------------------------------------------
# device-lifetime caches: made on first use and kept for the life of the process (captured graphs hold their addresses)
# -----------------------------------------------------------------------------------------------------
_WS = {}  # (device, stream) -> split-K slab scratch
_ARENA = {}  # device -> the deferred finishes' arena
_ARENA_RETIRED = []  # replaced arenas a captured graph points into
_ARENA_CAPTURED = set()  # data_ptr of every arena that was live during a stream capture
_SIDE = {}  # (device, i) -> dedicated side stream
_CONST_ROWS = {}  # (device, n, value) -> a tensor of n floats holding `value` (made in an eager pass, kept: captured graphs read it)
_TERMS_WS = {}  # (device, stream) -> the arrival counter + partials of mvk_reduce_terms_ws (zero between launches)

# ... and the one container of step state: device -> its open deferred_reductions scope
_OPEN = {}
scope = _OPEN.get  # scope(device): the open scope of a device, or None ("in a scope" is `scope(device) is not None`)

WS_FLOATS = 16 * 1024 * 1024  # 64 MB of split-K slab scratch per device (largest need on the path: 8.4M floats)


def _ws(like):
    """Caller-owned split-K scratch (see mvk.h): one persistent buffer per (device, stream), reused by every launch
    on that stream (launches are stream-ordered, so reuse is safe; two streams must not share one)."""
    key = (like.device, torch.cuda.current_stream(like.device).cuda_stream)
    t = _WS.get(key)
    if t is None:
        t = torch.empty(WS_FLOATS, dtype=torch.float32, device=like.device)
        _WS[key] = t
    return t


def _side_stream(device, i):
    key = (device, i)
    st = _SIDE.get(key)
    if st is None:
        # default priority: a priority -1 side stream costs +75 % step time (1.38 -> 2.4 ms, measured in round 2)
        st = _lib.new_stream(device)  # dedicated: never one of torch's 32 pooled streams (see _lib.new_stream)
        _SIDE[key] = st
    return st


def const_rows(device, n, value):
    key = (device, int(n), float(value))
    t = _CONST_ROWS.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            return None  # never allocate a cached buffer inside a capture (it would live in that graph's pool)
        t = torch.full((int(n),), float(value), dtype=torch.float32, device=device)
        _CONST_ROWS[key] = t
    return t


def terms_workspace(device, stream=None):
    """The loss assembly's workspace of (device, stream; default: the current one): eager memory, zeroed once, left zero by
    every launch.  Never made inside a capture (None then) — ADVICE r5: a workspace made there would live in the capturing
    graph's private pool, zero-filled by a node of that graph only, and then be handed to every later capture through this
    cache; trainers/graph.py makes it before torch.cuda.graph for the capture stream and the late-leaf stream."""
    key = (device, (torch.cuda.current_stream(device) if stream is None else stream).cuda_stream)
    ws = _TERMS_WS.get(key)
    if ws is None and not torch.cuda.is_current_stream_capturing():
        ws = _TERMS_WS[key] = torch.zeros(1 + 32 * 64, dtype=torch.float32, device=device)  # MVK_REDUCE_TERMS_WS_FLOATS
    return ws


def swap_arena(device, arena):
    """Replace a device's arena (None: the next scope makes a fresh one); returns the one it had (tests shrink it)."""
    old = _ARENA.pop(device, None)
    if arena is not None:
        _ARENA[device] = arena
    return old


def _tensors_of(obj):
    if torch.is_tensor(obj):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _tensors_of(v)
    elif isinstance(obj, (list, tuple)):
        for v in obj:
            yield from _tensors_of(v)


# -----------------------------------------------------------------------------------------------------
# deferred leaf reductions (mvk_defer_begin, include/mvk.h): the scope of one step
# -----------------------------------------------------------------------------------------------------
# Weight / bias gradients are leaves: between `deferred_reductions(flat)` and its exit the ordered finishes of every
# gradient that accumulates into the flat buffer (split-K slabs, column-sum partials, convolution weight-gradient slabs)
# are queued and run in ONE launch at exit instead of one small launch each in the middle of the backward chain.
DEFER = _lib.tune("MVK_DEFER", "1") != "0"
# The arena starts at 64 MB and grows between steps to what the last step asked for (mvk_defer_wanted), up to MVK_DEFER_MB
# (default 1024): an MLP model keeps 64 MB, the MnistSvhn models settle at ~200 MB, the ResNet configurations at the cap
# (a fixed 512 MB per device was wasteful for small models and too small for cfg5).  Grown only outside a stream
# capture; a replaced arena stays alive (a captured graph may hold its address).
DEFER_ARENA_CAP_FLOATS = int(os.environ.get("MVK_DEFER_MB", "1024")) * (1 << 18)
DEFER_ARENA_START_FLOATS = min(64 * (1 << 18), DEFER_ARENA_CAP_FLOATS)


class deferred_reductions:
    """with deferred_reductions(flat): forward + backward.  On exit the queued finishes run on the current stream; the
    gradient buffer is complete after that (before: NOT).  A no-op on CPU tensors or with MVK_DEFER=0 (no scope opens).

    The object is the step's scope: while it is open, `scope(device)` returns it and the helpers of this module read and write
    its attributes.  What the caller owns beyond the step is handed in: `prelude` (a closure with launches that depend on
    nothing of the step: run at the head of the first side branch run_branches opens, else by the caller's run_prelude()),
    `overlap` (the OverlapPoint of a data-parallel step), `rotation` (the Rotation of a rotated step)."""

    def __init__(self, flat, prelude=None, overlap=None, rotation=None):
        g = getattr(flat, "grad", None)
        self.on = DEFER and g is not None and g.is_cuda and g.numel() > 0
        self.grad = g
        self.prelude, self.overlap, self.rotation = prelude, overlap, rotation
        self.late_used = []  # streams that hold late leaves / partial flushes since mvk_defer_begin (joined at its end)
        self.late_calls = []  # (closure, tensors read): run on the late-leaf stream at exit, behind every other late leaf
        self.late_ready = None  # event where the postponed leaves may start
        # the loss assembly's ordering (ReconLossFn): None = ran on the caller's stream, nothing to wait for; a closure = the
        # launch, postponed among late_calls (assembly_last); an event = behind the launch on the stream it ran on
        self.loss = None
        self.big_late = False  # a backward node enqueued register-stationary late leaves
        self.tail_event = None  # event behind the SVHN decoder's image-layer backward
        self.branch_set = ()  # the streams of the last run_branches call (main first)

    def __enter__(self):
        if self.overlap is not None:
            self.overlap.begin()
        if self.on:
            dev = self.grad.device
            arena = _ARENA.get(dev)
            if arena is None:
                arena = torch.empty(DEFER_ARENA_START_FLOATS, dtype=torch.float32, device=dev)
                _ARENA[dev] = arena
            if torch.cuda.is_current_stream_capturing():
                _ARENA_CAPTURED.add(arena.data_ptr())  # a hipGraph holds pointers into it: it must outlive the graph
            call("mvk_defer_begin", ptr(arena), arena.numel(), ptr(self.grad), self.grad.numel())
            _OPEN[dev] = self
        return self

    def run_prelude(self):
        """The prelude, once, where the caller stands: run_branches at the head of its first side branch; the scope's owner
        behind the scope, in front of what needs it, when no branch took it."""
        fn, self.prelude = self.prelude, None
        if fn is not None:
            fn()

    def __exit__(self, et, ev, tb):
        if self.on:
            dev = self.grad.device
            late, self.late_calls = self.late_calls, []
            if late:  # postponed leaves: enqueued now, on the late-leaf stream, behind the other late leaves
                # Ordered behind a MAIN-stream event (late_ready: recorded where the posterior's backward starts, i.e. behind the
                # join of every decoder's backward), never behind the producer's branch stream itself: the partial flush on a branch
                # stream waits for the late-leaf stream, a late-leaf stream that waited for that branch stream made the two
                # "parallel capture streams" of each other and hip::Stream::EndCapture recursed until the stack overflowed; a
                # stream of its own changed the queue assignment of the replayed graph (the encoders' backward chain landed
                # behind the postponed launches: 1.10 -> 1.19 ms).
                st = _side_stream(dev, 30)
                ev = self.late_ready
                st.wait_event(ev if ev is not None else torch.cuda.current_stream(dev).record_event())
                self.late_used.append(st)
                with torch.cuda.stream(st):
                    for fn, reads in late:
                        for t in reads:
                            t.record_stream(st)
                        fn()
            _OPEN.pop(dev, None)
            cur = torch.cuda.current_stream(dev)
            for st in dict.fromkeys(self.late_used):  # the late leaves and sibling flushes end here
                if st != cur:
                    cur.wait_stream(st)
            call("mvk_defer_end", stream_ptr())
            wanted = int(_lib.load().mvk_defer_wanted())
            arena = _ARENA[dev]
            if wanted > arena.numel() and arena.numel() < DEFER_ARENA_CAP_FLOATS and not torch.cuda.is_current_stream_capturing():
                if arena.data_ptr() in _ARENA_CAPTURED:  # only an arena a captured graph points into is kept alive
                    _ARENA_RETIRED.append(arena)
                else:
                    arena.record_stream(cur)  # the finish launch above still reads it: no reuse before that has run
                grown = 1 << (wanted + wanted // 8 - 1).bit_length()  # powers of two: a creeping demand grows it log(n) times
                _ARENA[dev] = torch.empty(min(DEFER_ARENA_CAP_FLOATS, grown), dtype=torch.float32, device=dev)
        return False


# MVK_LATE_LEAVES=1: the weight gradients of the large decoder (two ~100 us launches that fill the chip) are enqueued AFTER
# its backward-data chain, on a stream that is joined only where the deferred finishes run: they execute beside the
# launch-latency-bound encoder backward (the ~300 us tail of the step in which the chip is mostly idle) instead of in
# front of it.
# MEASURED (headline step, same box, two pairs): 1.347 / 1.336 ms without vs 1.320 / 1.315 ms with; a smaller grid for the
# weight-gradient kernels (MVK_IMGWGRAD_GRID=224 / 192 / 128: compute units left free for the chain) does not help
# (1.331 / 1.348 / 1.414 ms).  MVK_LATE_LEAVES=0 disables.
LATE_LEAVES = _lib.tune("MVK_LATE_LEAVES", "1") != "0"


class late_leaves:
    """with late_leaves(device, *tensors_read): the enclosed launches go to the late-leaf stream, ordered behind what the
    current stream holds now; nothing waits for them until deferred_reductions ends.  Outside deferred_reductions (or with
    MVK_LATE_LEAVES=0, or on the CPU) the launches stay on the current stream."""

    def __init__(self, device, *reads):
        self.scope = scope(device) if LATE_LEAVES else None
        self.on = self.scope is not None
        self.device, self.reads, self._ctx = device, reads, None

    def __enter__(self):
        if self.on:
            st = _side_stream(self.device, 30)
            st.wait_event(torch.cuda.current_stream(self.device).record_event())
            for t in self.reads:
                t.record_stream(st)
            self.scope.late_used.append(st)
            self._ctx = torch.cuda.stream(st)
            self._ctx.__enter__()
        return self

    def __exit__(self, *exc):
        if self._ctx is not None:
            self._ctx.__exit__(*exc)
            self._ctx = None
        return False


# Of the MLP decoder's weight gradients only the first layer's (a split-K launch of 16 us alone, 50-60 us beside the convolutions)
# is postponed: autograd orders the posterior's backward behind EVERYTHING the decoder's backward node enqueued on its stream,
# leaves included.  MEASURED (three same-box pairs): 1.046 / 1.050 / 1.039 -> 1.042 / 1.040 / 1.032 ms.  Postponing ALL of them
# lost (1.099 / 1.093 / 1.094 ms without vs 1.114 / 1.104 / 1.106 ms with: the tail — the encoders' backward, a dependent chain of
# small kernels — slows down by what the decoder window gains).


def run_last(device, fn, *reads, params=()):
    """Inside deferred_reductions: run fn() on the late-leaf stream AFTER everything else the backward pass puts there (the
    enqueue itself is postponed to the end of the scope), i.e. in the launch-latency-bound tail of the step where the chip is
    mostly idle, instead of beside the decoders' backward-data chains whose window is throughput-bound.  Returns False when
    there is no such scope (the caller runs fn itself)."""
    sc = scope(device) if LATE_LEAVES else None
    if sc is None:
        return False
    sc.late_calls.append((fn, reads))
    if sc.overlap is not None:  # these gradients are written in the tail of the step: not part of the early collective
        sc.overlap.late_params.extend(params)
    return True


def late_ready(device):
    """Called on the main stream where every decoder's backward has been joined (the posterior's backward): the postponed
    leaves of run_last may start behind this point."""
    sc = scope(device)
    if sc is not None and sc.late_calls:
        sc.late_ready = torch.cuda.current_stream(device).record_event()


# -----------------------------------------------------------------------------------------------------
# the loss assembly's ordering (scope.loss)
# -----------------------------------------------------------------------------------------------------
# MVK_ASYNC_LOSS=0: the loss assembly stays on the caller's stream, between the last forward and the first backward launch
ASYNC_LOSS = _lib.tune("MVK_ASYNC_LOSS", "1") != "0"
# MVK_ASSEMBLY_LAST=0: the assembly launch at the head of the backward pass on the late-leaf stream (the round-5 place; A/B)
ASSEMBLY_LAST = _lib.tune("MVK_ASSEMBLY_LAST", "1") != "0"


def orders_behind_loss(rows):
    """True when the backward node that produced `rows` (a fused decoder tail's NLL row sums) is one of this package's, i.e.
    known to call wait_loss before it reads a row gradient the assembly launch fills (the Function says so: WAITS_FOR_LOSS).
    A user decoder may implement `reconstruction_nll` with ordinary autograd ops: its backward would read the row-gradient
    buffer with NO ordering against an assembly launch on the late-leaf stream — in a captured graph a missing dependency,
    silently wrong gradients.  Models set spec["async_ok"] only when this holds for every fused term."""
    fn = getattr(rows, "grad_fn", None)
    if fn is None:
        return not getattr(rows, "requires_grad", False)
    return getattr(getattr(fn, "_forward_cls", None), "WAITS_FOR_LOSS", False) is True


def wait_loss(device):
    """Order the current stream behind the loss assembly launch.  Every backward node that READS a gradient buffer the assembly
    fills (the KL rows' gradients, a fused tail's row gradients on its general path) calls this first; nodes that take the
    constant from `const_grad` do not wait for anything.  An assembly that was postponed to the end of the step (nobody was
    expected to read what it fills) runs HERE, on the caller's stream, when somebody does; the event recorded behind it orders
    every later reader of the scope, whatever stream it is on."""
    sc = scope(device)
    if sc is None or sc.loss is None:
        return
    cur = torch.cuda.current_stream(device)
    if callable(sc.loss):
        fn = sc.loss
        sc.late_calls[:] = [c for c in sc.late_calls if c[0] is not fn]
        fn()
        sc.loss = cur.record_event()
    else:
        cur.wait_event(sc.loss)


# -----------------------------------------------------------------------------------------------------
# where the backward pass says "this part of the gradient buffer is final" (overlapped data-parallel collective)
# -----------------------------------------------------------------------------------------------------
class OverlapPoint:
    """The reference's DDP reduces gradient buckets while loss.backward() still runs (trainers/base/base_trainer.py:116-117,359).
    Here the step is ONE replayed hipGraph, so the overlap needs a point INSIDE the graph that a stream OUTSIDE can wait for: an
    external event-record node (mvk_event_record(ev, 1, stream)), placed where the finishes of everything but the last backward
    node have run (defer_flush_sibling: the decoders', the posterior's and the short encoder's gradients are final there, the
    long encoder's backward chain — ~300 us of the headline step — is still ahead).  `late_params` collects the parameters whose
    gradients are NOT final at that point: the node that called defer_flush_sibling and every leaf postponed by run_last.
    Owned by trainers.graph.GraphedStep, handed to deferred_reductions(overlap=...) for every pass it enqueues / captures."""

    def __init__(self, device):
        self.device = device
        self.event = C.c_void_p()
        call("mvk_event_create", C.byref(self.event))
        self.late_params = []
        self.recorded = False

    def begin(self):
        self.late_params, self.recorded = [], False

    def __del__(self):
        try:
            if self.event:
                _lib.load().mvk_event_destroy(self.event)
        except Exception:
            pass


# When the LAST backward node of the step starts (the convolutional encoder: ~140 us of launch-latency-bound
# chain on its own stream), everything queued so far is finished on the other branch stream, which is idle by then, instead of
# in one launch behind the chain.
def defer_flush_sibling(device, node_params=()):
    """node_params: the parameters of the backward node that calls this (the LAST one of the step): with an OverlapPoint open,
    everything else's gradient is final behind the flush, and the point is recorded there."""
    sc = scope(device)
    if sc is None:
        return
    cur = torch.cuda.current_stream(device)
    sib = next((st for st in sc.branch_set if st != cur), None)
    if sib is None or _lib.load().mvk_defer_pending() == 0:
        return
    with torch.cuda.stream(sib):
        call("mvk_defer_flush", stream_ptr())
        op = sc.overlap
        if op is not None and not op.recorded:
            # the flush already waits for every stream a gradient producer RAN ON (csrc/igemm.hip defer_flush_locked); ordered
            # explicitly behind the caller's stream and the late-leaf streams as well: a gradient written straight into the
            # buffer by a launch that queued no finish would otherwise be unordered against the collective
            # (... and behind EVERY branch stream of the step, not only the caller's: a backward node of another branch
            # that is enqueued already must have written its gradients before the collective reads them)
            for st in dict.fromkeys([cur] + list(sc.branch_set) + sc.late_used):
                if st != sib:
                    sib.wait_event(st.record_event())
            call("mvk_event_record", op.event, 1, stream_ptr())
            op.late_params.extend(node_params)
            op.recorded = True  # from here on every gradient target handed out is late (kernels._grad_target): whatever node asks
    sc.late_used.append(sib)


# "auto" of MVK_HEADS_BWD_MLP (kernels.heads_bwd_mlp): whether a backward node of the open scope enqueued register-stationary
# late leaves
def big_late_leaves(device):
    sc = scope(device)
    if sc is not None:
        sc.big_late = True


def has_big_late_leaves(device):
    sc = scope(device)
    return sc is not None and sc.big_late


# -----------------------------------------------------------------------------------------------------
# the rotated step: leaf gradients of step N at the head of step N + 1 (trainers/graph.py GraphedStep(rotate=True))
# -----------------------------------------------------------------------------------------------------
# The reference's loop is strictly sequential (trainers/base/base_trainer.py:350-361: zero_grad, forward, backward, step), but
# nothing in its semantics ties a DECODER's weight gradients and their share of optimizer.step() of step N to anything before
# that decoder's forward pass of step N + 1.  In a rotated step the decoders' weight-gradient launches (leaves of the backward
# pass: nothing waits for them) are not enqueued by the backward pass; their closures are kept and run at the head of the
# next step on a branch of their own — beside the encoders' forward pass and the posterior, the launch-latency-bound head of
# the step in which the chip is mostly idle — followed by their ordered finishes, the Adam update of exactly those
# parameters (mvk_adam_step_dev with the scalars the step's main update published: mvk_adam_step_pub) and the weight packs
# that read them; the decoders' forward pass waits for that branch.  Every parameter is updated once per step, with the same
# gradient and the same scalars, before it is next read: the parameters after N steps + a drain are bit for bit those of N
# unrotated steps (tests/test_gpu_trainer.py).  What a leaf reads must survive into the next replay at a fixed address:
# `Rotation.buf` hands out persistent buffers, `Rotation.slots` persistent amax slots (zeroed by the branch behind the leaves).
# MVK_ROT_SVHN / MVK_ROT_MLP: 0 = that decoder's leaves stay in the step they belong to; 1 = all of its weight-gradient leaves are
# rotated (the large, register-stationary launches too); 2 = only its FIRST layer's (a split-K GEMM of 10-25 us whose workgroups
# fit beside anything: the kind of launch the head of the step has room for).
ROT_SVHN = int(_lib.tune("MVK_ROT_SVHN", "1"))
ROT_MLP = int(_lib.tune("MVK_ROT_MLP", "1"))


def rotation(device):
    """The Rotation of the device's open scope, or None."""
    sc = scope(device)
    return sc.rotation if sc is not None else None


class Rotation:
    """Owned by its GraphedStep (it lives from replay to replay), handed to deferred_reductions(rotation=...) for every pass."""

    def __init__(self, device):
        self.device = device
        self.bufs = {}
        self.amax = torch.zeros(64, dtype=torch.float32, device=device)
        self.amax_pos = 0
        self.leaves = []    # registered by the backward pass that is being enqueued: (closure, parameters, prepare)
        self.pending = []   # those of the previous pass: what the head of the next one runs
        self.cache = {}     # pack key -> what the head's `prepare` closures packed BEHIND the update of the rotated parameters
        self.event = None
        self.waited = set()
        self.stream = _side_stream(device, 29)
        self.open = False

    def buf(self, name, shape, dtype=torch.float32):
        """A buffer that keeps its address from pass to pass (and from replay to replay)."""
        t = self.bufs.get(name)
        if t is None or tuple(t.shape) != tuple(shape) or t.dtype != dtype:
            if t is not None and torch.cuda.is_current_stream_capturing():
                raise _lib.MvkError(f"rotated step: buffer {name} changes shape inside a capture")
            t = torch.zeros(tuple(shape), dtype=dtype, device=self.device)
            self.bufs[name] = t
        return t

    def slots(self, n):
        """n amax slots that are zero now and stay untouched until the head of the next step has run its leaves."""
        if self.amax_pos + n > self.amax.numel():
            raise _lib.MvkError("rotated step: out of amax slots")
        self.amax_pos += n
        return self.amax[self.amax_pos - n:self.amax_pos]

    @property
    def params(self):
        """The parameters whose gradients (and update) are rotated, in registration order."""
        out, seen = [], set()
        for _, ps, _ in self.pending:
            for q in ps:
                if id(q) not in seen:
                    seen.add(id(q))
                    out.append(q)
        return out

    def push(self, fn, params, prepare=None):
        self.leaves.append((fn, tuple(params), prepare))

    def begin_step(self, update=None):
        """Inside deferred_reductions, at the head of the forward pass: the branch of the previous step's leaves.  update: the
        closure that applies the optimizer to the rotated parameters (captured passes only; eager warm-up passes leave the
        parameters alone)."""
        cur = torch.cuda.current_stream(self.device)
        st = self.stream
        st.wait_event(cur.record_event())
        self.cache, self.waited, self.open = {}, set(), True
        with torch.cuda.stream(st):
            for fn, _, _ in self.pending:
                fn()
            if self.pending:
                call("mvk_defer_flush", stream_ptr())  # their ordered finishes: the gradients of the rotated parameters are final
                if update is not None:
                    update()
            self.amax.zero_()  # the slots the leaves read are free for this step's producers
            self.amax_pos = 0
            for _, _, prepare in self.pending:
                if prepare is not None:
                    prepare(self)
            self.event = st.record_event()
        self.leaves = []

    def wait(self):
        """Order the current stream behind the head branch (whoever reads a rotated parameter, or a pack of one, calls this)."""
        if not self.open or self.event is None:
            return
        cur = torch.cuda.current_stream(self.device)
        if cur.cuda_stream not in self.waited:
            cur.wait_event(self.event)
            self.waited.add(cur.cuda_stream)
            for t in _tensors_of(list(self.cache.values())):  # allocated on the branch's stream, read on this one
                t.record_stream(cur)
                if getattr(t, "mvk_frag", None) is not None:
                    t.mvk_frag.record_stream(cur)

    def end_step(self):
        """Behind the backward pass: the branch is joined (it is, transitively, when a decoder waited for it), the leaves the
        backward pass registered become the next head's."""
        if self.open:
            self.wait()
            self.open = False
        self.pending, self.leaves = self.leaves, []

    def run_pending(self):
        """The drain: the pending leaves on the current stream (inside deferred_reductions), no update, no packs."""
        for fn, _, _ in self.pending:
            fn()


# -----------------------------------------------------------------------------------------------------
# modality branches on separate HIP streams
# -----------------------------------------------------------------------------------------------------
# The encoders (and the decoders) of different modalities are independent until the posterior (resp. the
# reconstruction loss) joins them.  The small-modality branch is a string of short, launch-latency-bound
# kernels; on its own stream it runs beside the large modality's convolutions instead of in front of them.
# Autograd replays each node's backward on the stream its forward ran on, so the backward overlaps too.
BRANCH_STREAMS = _lib.tune("MVK_BRANCH_STREAMS", "1") != "0"


# The decoders' side branches are CREATED before the main one (run_branches(side_first=True)), so that autograd enqueues the main
# branch's backward first and a side branch's backward can be ordered behind the main branch's HBM-bound tail kernel
# (tail_bwd_done / wait_tail_bwd).  Two memory-heavy launches that share the chip are slower than the same two in a row:
# small_up_bwd_bf_kernel took 139 us beside the MLP decoder's backward-data GEMM (95 us), 82 and 32 us alone.  MEASURED (three
# same-box pairs): 1.087 / 1.080 / 1.095 ms -> 1.040 / 1.055 / 1.050 ms.
def tail_bwd_done(device):
    """SVHNDecoderFn.backward, right behind its image-layer launch."""
    sc = scope(device)
    if sc is not None:
        sc.tail_event = torch.cuda.current_stream(device).record_event()


def wait_tail_bwd(device):
    """A side branch's decoder backward: start behind the main branch's tail kernel when that one was enqueued first."""
    sc = scope(device)
    if sc is not None and sc.tail_event is not None:
        ev, sc.tail_event = sc.tail_event, None
        torch.cuda.current_stream(device).wait_event(ev)


def run_branches(names, fn, device, side_first=False):
    """{m: fn(m)} with every branch but the first on its own stream; joined before returning.  Inside a scope the stream set
    is recorded on it (defer_flush_sibling picks the idle sibling from it) and the first side branch takes the prelude."""
    names = list(names)
    if not BRANCH_STREAMS or len(names) < 2 or device.type != "cuda":
        return {m: fn(m) for m in names}
    main = torch.cuda.current_stream(device)
    streams = [main] + [_side_stream(device, i) for i in range(1, len(names))]
    sc = scope(device)
    if sc is not None:
        sc.branch_set = streams
    fork = main.record_event()
    # The first branch stays on the caller's stream and is enqueued FIRST: autograd runs backward nodes in reverse
    # creation order, so the side branches' backward is enqueued (and, in a captured graph, ordered) before the long
    # backward of the main branch instead of behind it.
    outs = {}
    if not side_first:
        outs[names[0]] = fn(names[0])
    for m, st in zip(names[1:], streams[1:]):
        st.wait_event(fork)
        with torch.cuda.stream(st):
            if sc is not None:
                sc.run_prelude()
            outs[m] = fn(m)
        for t in _tensors_of(outs[m]):
            t.record_stream(main)
    if side_first:
        outs[names[0]] = fn(names[0])
    for st in streams[1:]:
        main.wait_stream(st)
    return {m: outs[m] for m in names}
