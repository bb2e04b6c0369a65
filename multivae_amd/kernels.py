"""torch.autograd.Function wrappers over the C ABI of libmvk.so.

Every function here launches hand-written HIP kernels on the current PyTorch-ROCm stream; PyTorch is used
for device memory and autograd ordering only.  Whole networks (MLP / SVHN encoder and decoder) are single
autograd nodes so that a training step is a few dozen kernel launches with almost no Python in between,
and the backward passes use the producer-epilogue fusion of the engine (a layer's backward-data GEMM
multiplies by the previous layer's activation derivative and writes the pre-activation gradient directly).
"""
import ctypes as C
import math

import torch
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from . import _lib, schedule
from ._lib import ACT, DIST, FAMILY, PackDesc, ReconDesc, SeedDesc, TermDesc, call, ptr, ptr_array, stream_ptr

RELU, SIGMOID, NONE = ACT["relu"], ACT["sigmoid"], ACT["none"]

# bench.py sets PROFILE["recon_nll"] = [] to collect (start, end) HIP events around the fused reconstruction-NLL
# launch on the stream it is launched on (roofline measurement inside the timed region).
PROFILE = {}
# accumulate parameter gradients directly into pre-existing .grad buffers (see _grad_target)
DIRECT_GRAD = True
# The host scheduler (streams, the per-step scope, the switches that go with them) is schedule.py and is named as such here and
# by every caller: no second binding of a name somebody patches or assigns.  Two plain aliases: the scope, under the name the
# benchmark enters it by, and the scratch helper.
deferred_reductions = schedule.deferred_reductions
_ws = schedule._ws  # the per-stream split-K scratch every launch helper below hands to its kernel

# Device-lifetime caches of this module (like those of schedule.py: made on first use, kept for the life of the process; captured
# graphs hold their addresses).  Nothing of ONE step is kept here: that is the scope's (schedule.deferred_reductions).
_RNG = {}  # device -> [state tensor (3 x int64: seed, offset, ticket), torch seed it was built from, breadcrumb offset]
_UNIT_SEEDS = {}  # data_ptr -> tensor (kept alive): backward seeds known to hold exactly 1
_CONST_GRADS = {}  # data_ptr -> (weakref of the tensor, numel, value): gradient buffers known to hold ONE constant


def _c(t):
    """contiguous fp32 CUDA tensor (no copy when already so)."""
    _lib.require_gpu_tensor(t)
    return t if t.is_contiguous() else t.contiguous()


def _new(shape, like):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def _zeros(shape, like):
    return torch.zeros(shape, dtype=torch.float32, device=like.device)


FMT_IN_BF3 = 1  # mvk.h MVK_FMT_IN_BF3


def to_bf3(x):
    """fp32 tensor -> pre-split tensor [3, *x.shape] of bf16 (mvk_f32_to_bf3)."""
    x = x.contiguous()
    out = torch.empty((3,) + tuple(x.shape), dtype=torch.bfloat16, device=x.device)
    call("mvk_f32_to_bf3", ptr(x), x.numel(), out.data_ptr(), stream_ptr())
    return out


# =====================================================================================================
# thin launch helpers (no autograd)
# =====================================================================================================
def linear_fwd(x2, w, b, act):
    M, K = x2.shape
    N = w.shape[0]
    y = _new((M, N), x2)
    ws = _ws(x2)
    call("mvk_linear_fwd", ptr(x2), ptr(w), ptr(b), ptr(y), M, N, K, act, ptr(ws), ws.numel(), stream_ptr())
    return y


def _bias_target(bias_param):
    """(buffer the kernel accumulates the bias gradient into, what autograd gets for the bias)."""
    if bias_param is None:
        return None, None
    return _grad_target(bias_param)


def linear_bwd_data(dy, w, y_out=None, y_act=NONE, prev_out=None, prev_act=NONE, out=None, accumulate=False,
                    prev_bias=None):
    """dx (the previous layer's pre-activation gradient when prev_out is given).  prev_bias: that layer's bias
    parameter — its gradient (column sums of dx) is produced by the same launch; returns (dx, grad for autograd)."""
    M, N = dy.shape
    K = w.shape[1]
    dx = out if out is not None else _new((M, K), dy)
    ws = _ws(dy)
    tb, rb = _bias_target(prev_bias)
    call("mvk_linear_bwd_data", ptr(dy), ptr(w), ptr(dx), M, N, K, ptr(y_out), y_act, ptr(prev_out), prev_act,
         1 if accumulate else 0, ptr(tb), ptr(ws), ws.numel(), stream_ptr())
    return dx if prev_bias is None else (dx, rb)


def _grad_target(p):
    """Where a parameter's gradient is accumulated.  If the parameter already owns a contiguous fp32 .grad
    (e.g. a view of the flat gradient buffer of trainers.FlatParams) the kernels accumulate straight into it
    and autograd gets None for this input (no zero-fill, no extra add kernel); otherwise a fresh zero buffer is
    returned to autograd as usual.  Both ways the visible semantics are `p.grad += dL/dp`."""
    g = p.grad
    sc = schedule.scope(p.device)
    if sc is not None:
        op = sc.overlap
        if op is not None and op.recorded:
            # a gradient produced behind the overlap point — by the node that recorded it or by ANY node enqueued
            # later (a second SVHN-type encoder, an encoder on a side branch) — is not part of the early collective
            op.late_params.append(p)
    if DIRECT_GRAD and g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.shape == p.shape \
            and g.device == p.device:
        return g, None
    z = _zeros(p.shape, p)
    return z, z


def _is_direct(p):
    """_grad_target(p) accumulates straight into p.grad (autograd gets None)."""
    g = p.grad
    return bool(DIRECT_GRAD and g is not None and g.is_contiguous() and g.dtype == torch.float32 and g.shape == p.shape
                and g.device == p.device)


def linear_bwd_weight(dy, x2, w, b, y_out=None, y_act=NONE):
    """-> (grad to return for w, grad to return for b)"""
    M, N = dy.shape
    K = x2.shape[1]
    dw, rw = _grad_target(w)
    db, rb = _grad_target(b) if b is not None else (None, None)
    ws = _ws(dy)
    call("mvk_linear_bwd_weight", ptr(dy), ptr(x2), ptr(dw), ptr(db), M, N, K, ptr(y_out), y_act, ptr(ws),
         ws.numel(), stream_ptr())
    return rw, rb


def gemm(a, b, M, N, K, ta=False, tb=False, bias=None, bias_mod=0, act=NONE, out=None, accumulate=False,
         a_act_src=None, a_act=NONE, c_act_src=None, c_act=NONE):
    c = out if out is not None else _new((M, N), a)
    ws = _ws(a)
    call("mvk_gemm", ptr(a), ptr(b), ptr(c), M, N, K, int(ta), int(tb), ptr(bias), bias_mod, act,
         1 if accumulate else 0, ptr(a_act_src), a_act, ptr(c_act_src), c_act, ptr(ws), ws.numel(), stream_ptr())
    return c


def heads_fwd(h2, w_mu, b_mu, w_lv, b_lv, N, w_sk, w_sn):
    """(mu, lv) = h2 @ W_mu + b_mu, h2 @ W_lv + b_lv in one launch (mvk_heads_fwd); W(k, n) = W[k * w_sk + n * w_sn]."""
    M, K = h2.shape
    if N > 32 or K % 4 != 0:
        return None
    mu, lv = _new((M, N), h2), _new((M, N), h2)
    call("mvk_heads_fwd", ptr(h2), ptr(w_mu), ptr(b_mu), ptr(mu), ptr(w_lv), ptr(b_lv), ptr(lv), M, N, K, w_sk, w_sn,
         stream_ptr())
    return mu, lv


# The heads' backward in one launch (heads_bwd).
# MEASURED (headline step, one box, 3-4 rounds each): 1.355 ms with the six separate launches, 1.326 ms with the fused launch
# for the convolutional (SVHN) encoder only, 1.343 ms with the fused launch for the MLP encoder too (its chain is not the
# critical one and the fused launch delays the other stream's kernels).  RE-MEASURED at the end of round 2, with the partial
# finish on the sibling stream and a replayed graph that now spreads over three hardware queues: 1.2480 ms with the fused launch
# for the MLP encoder too vs 1.2569 ms without (four same-box pairs) — on by default now, MVK_HEADS_BWD_MLP=0 disables.
# RE-MEASURED in round 6, with the loss assembly at the end of the step and the convolutional encoder's weight-gradient pair: at the
# headline (K = 10: the large decoder's register-stationary weight gradients are late leaves of the tail, one 512-register wave
# per SIMD on every CU) the six separate launches for the MLP encoder are ahead again — 0.9262 / 0.9299 / 0.9272 ms against
# 0.9407 / 0.9370 / 0.9361 with the fused launch, second box 0.9565 / 0.9615 / 0.9606 against 0.9638 / 0.9713 / 0.9708, third
# 0.9487 / 0.9558 / 0.9508 against 0.9574 / 0.9612 / 0.9587 (-0.9 %, nine alternating pairs: the fused launch's 128 x 4
# workgroups with 48-62 KB of LDS wait for room beside those leaves) — while WITHOUT such leaves (decoder batch < 1024 rows:
# MMVAE MnistSvhn 0.516 / 0.533 fused against 0.560 / 0.559, MoPoE at K = 1 0.509 / 0.521 against 0.537 / 0.540) the fused launch
# wins by 5-8 %.  "auto" (default): fused unless a backward node of this scope enqueued register-stationary late leaves
# (schedule.big_late_leaves); MVK_HEADS_BWD_MLP=0 / 1 force one form.
_HEADS_BWD_MLP_MODE = _lib.tune("MVK_HEADS_BWD_MLP", "auto")


def heads_bwd_mlp(device):
    """Whether an MLP encoder's heads take the one-launch backward now."""
    if _HEADS_BWD_MLP_MODE in ("0", "1"):
        return _HEADS_BWD_MLP_MODE == "1"
    return not schedule.has_big_late_leaves(device)


def heads_bwd(x, x_act, dys, ws_, bs, w_sk, w_sn, flat_c=0, want_dx=True, prev_bias=None, dw_params=None):
    """Backward of 1 or 2 narrow heads that read x [M,K] (mvk_heads_bwd).  dys: gradients [M,N]; ws_: the weights as the
    kernel reads them (W(k, n) = W[k * w_sk + n * w_sn]); dw_params: the parameters whose .grad receives dY^T x (default:
    ws_); bs: bias parameters (or None).  Returns None when the shape is not covered, else
    (dx or None, [grad for autograd per weight], [grad per bias], grad for prev_bias)."""
    M, K = x.shape
    N = dys[0].shape[1]
    if N > 32 or K % 16 != 0 or len(dys) > 2 or M < 1 or (M + 127) // 128 > 64:
        return None
    dw_params = ws_ if dw_params is None else dw_params
    tw, rw = zip(*[_grad_target(p) for p in dw_params])
    tb, rb = zip(*[_grad_target(b) if b is not None else (None, None) for b in bs])
    tp, rp = _grad_target(prev_bias) if prev_bias is not None else (None, None)
    dx = _new((M, K), x) if want_dx else None
    two = len(dys) == 2
    ws = _ws(x)
    # slabs of the launch: N * K * ceil(M / 128) floats per head + the bias rows; what does not fit the deferred arena must fit
    # the per-stream scratch, else the separate launches take over (the C side declines with MVK_EINVAL)
    rgs = (M + 127) // 128
    if (len(dys) * (N * K + N) + K) * rgs + 64 > ws.numel():
        return None
    call("mvk_heads_bwd", ptr(x), x_act, ptr(dys[0]), ptr(dys[1]) if two else None, ptr(ws_[0]), ptr(ws_[1]) if two else None,
         w_sk, w_sn, flat_c, ptr(dx), ptr(tw[0]), ptr(tw[1]) if two else None, ptr(tb[0]), ptr(tb[1]) if two else None,
         ptr(tp), M, N, K, ptr(ws), ws.numel(), stream_ptr())
    return dx, list(rw), list(rb), rp


def colsum(dy2, b, y_out=None, y_act=NONE):
    """bias gradient: b.grad += column sums of dy2 [M,N]; returns what autograd should get for b."""
    M, N = dy2.shape
    db, rb = _grad_target(b)
    ws = _ws(dy2)
    call("mvk_colsum_acc", ptr(dy2), ptr(y_out), y_act, ptr(db), M, N, ptr(ws), ws.numel(), stream_ptr())
    return rb


def pack_conv(wref, want_down=True, want_up=True):
    """wref [Cv][Cu][4][4] -> (Wdown [16*Cu, Cv], Wup [4, 4*Cv, Cu])."""
    (wd, wu), = pack_weights([(wref, want_down, want_up)])
    return wd, wu


def _frag(like, Cu, Cv):
    """Buffer for the bf16-piece fragment pack of a 4x4/stride-2 layer the register-stationary kernels cover, else None."""
    nb = _lib.load().mvk_imgconv_frag_bytes(Cu, Cv)
    return torch.empty(nb, dtype=torch.uint8, device=like.device) if nb else None


def wfrag(w):
    """The fragment pack that travels with a packed weight (attached by pack_weights), or None."""
    return getattr(w, "mvk_frag", None)


PACK_MAX = 16  # MVK_PACK_MAX descriptors per launch
_PACK_SCOPE = None


class pack_scope:
    """with pack_scope(model): ONE weight-pack launch for the whole forward pass.  The first `pack_weights` call inside the
    scope also packs what every other sub-module of `model` announces through `pack_jobs()` (the decoder's pack used to sit on
    the critical chain between the posterior and the first decoder layer); later calls find their packs in the scope's cache.
    The cache dies with the scope: nothing packed here outlives the forward pass (the weights change at the next optimizer step)."""

    def __init__(self, model):
        self.model, self.own = model, False

    def __enter__(self):
        global _PACK_SCOPE
        if _PACK_SCOPE is None:
            _PACK_SCOPE = {"model": self.model, "cache": {}, "done": False}
            self.own = True
            # the zeroed arena of the amax protocol (AmaxPool, the pack launches): filled HERE, on the caller's stream and in front
            # of every fork of run_branches — a slot must be zero before ANY stream publishes into it, and the branch streams
            # are ordered behind the fork only, not behind what the first branch enqueues
            dev = next((p.device for p in self.model.parameters()), None)
            if (C3_F16 or IMG_F16) and dev is not None and dev.type == "cuda":
                _PACK_SCOPE["amax"], _PACK_SCOPE["amax_pos"] = torch.zeros(512, dtype=torch.float32, device=dev), 0
        return self

    def __exit__(self, *exc):
        global _PACK_SCOPE
        if self.own:
            _PACK_SCOPE = None
        return False


def _job_key(job):
    return (job[0].data_ptr(), tuple(job[0].shape)) + tuple(job[1:])


def pack_weights(jobs):
    """`_pack_launch(jobs)`, or inside a pack_scope: from the scope's cache / together with every announced job of the model."""
    sc = _PACK_SCOPE
    keys = [_job_key(j) for j in jobs]
    rot = schedule.rotation(jobs[0][0].device)
    if rot is not None and rot.cache:  # some (or all) of them packed by the head branch of a rotated step, behind their update
        hit = [k in rot.cache for k in keys]
        if any(hit):
            rot.wait()
            if all(hit):
                return [rot.cache[k] for k in keys]
            rest = iter(pack_weights([j for j, h in zip(jobs, hit) if not h]))
            return [rot.cache[k] if h else next(rest) for k, h in zip(keys, hit)]
    if sc is None:
        return _pack_launch(jobs)
    cache = sc["cache"]
    if all(k in cache for k in keys):
        return [cache[k] for k in keys]
    todo, tkeys = list(jobs), list(keys)
    if not sc["done"]:
        sc["done"] = True
        for mod in sc["model"].modules():
            announce = getattr(mod, "pack_jobs", None)
            if announce is None:
                continue
            for j in announce():
                k = _job_key(j)
                if rot is not None and k in rot.cache:
                    continue  # behind the rotated update of these weights, on the head branch
                if k not in tkeys and k not in cache and j[0].device == jobs[0][0].device and len(todo) < PACK_MAX:
                    todo.append(j)
                    tkeys.append(k)
    outs = []
    for i0 in range(0, len(todo), PACK_MAX):
        outs += _pack_launch(todo[i0:i0 + PACK_MAX])
    for k, o in zip(tkeys, outs):
        cache[k] = o
    return outs[:len(jobs)]


def _pack_launch(jobs, am=None):
    """All weight packs of a network in ONE launch.  jobs: list of (wref, want_down, want_up) for 4x4/stride-2
    layers ([Cv][Cu][4][4] -> (Wdown [16*Cu, Cv], Wup [4, 4*Cv, Cu])) or (wref, "unflatten") for the 1x1-spatial
    transposed convolution ([Cin][Cout][4][4] -> [Cin, 16*Cout]).  Returns the packed tensors in job order."""
    descs = (PackDesc * len(jobs))()
    outs = []
    # max |W| per convolution weight: the operand scale of the scaled-fp16 launches (mvk_conv3x3_s, mvk_conv4s2_down_s / _up_s)
    # (am given: zeroed slots of the caller's — the head branch of a rotated step packs outside the scope's arena)
    if am is None and ((C3_F16 and any(job[1] == "c3" for job in jobs))
                       or (IMG_F16 and any(job[1] not in ("c3", "unflatten") for job in jobs))):
        am = _amax_slots(jobs[0][0], len(jobs), create=True)
    for i, job in enumerate(jobs):
        wref = job[0]
        Cv, Cu = wref.shape[0], wref.shape[1]
        d = descs[i]
        d.Wref, d.Cv, d.Cu, d.ld_down, d.col_off = wref.data_ptr(), Cv, Cu, Cv, 0
        if job[1] == "unflatten":
            wp = _new((Cv, 16 * Cu), wref)
            d.kind, d.Wdown, d.Wup = 1, None, wp.data_ptr()
            outs.append(wp)
        elif job[1] == "c3":  # 3x3 convolution [Cout][Cin][3][3] -> (forward [9*Cin, Cout], backward-data [9*Cout, Cin])
            wf = _new((9 * Cu, Cv), wref) if job[2] else None
            wb = _new((9 * Cv, Cu), wref) if job[3] else None
            d.kind = 2
            d.Wdown = wf.data_ptr() if wf is not None else None
            d.Wup = wb.data_ptr() if wb is not None else None
            if am is not None:
                d.amax = am[i:i + 1].data_ptr()
                for t in (wf, wb):
                    if t is not None:
                        t.mvk_amax = am[i:i + 1]
            outs.append((wf, wb))
        else:
            wd = _new((16 * Cu, Cv), wref) if job[1] else None
            wu = _new((4, 4 * Cv, Cu), wref) if job[2] else None
            d.kind = 0
            d.Wdown = wd.data_ptr() if wd is not None else None
            d.Wup = wu.data_ptr() if wu is not None else None
            # bf16-piece MFMA fragments for the register-stationary kernels travel with the packs (same launch)
            if wd is not None:
                wd.mvk_frag = _frag(wref, Cu, Cv)
                d.Fdown = wd.mvk_frag.data_ptr() if wd.mvk_frag is not None else None
            if wu is not None:
                wu.mvk_frag = _frag(wref, Cu, Cv)
                d.Fup = wu.mvk_frag.data_ptr() if wu.mvk_frag is not None else None
            if am is not None:
                d.amax = am[i:i + 1].data_ptr()
                for t in (wd, wu):
                    if t is not None:
                        t.mvk_amax = am[i:i + 1]
            outs.append((wd, wu))
    call("mvk_pack_weights", descs, len(jobs), stream_ptr())
    return outs


def conv4s2_scaled_ok(n, h, w, Cu, Cv):
    """True when the `amax=` forms of conv_down / conv_up (mvk_conv4s2_down_s / _up_s) take this layer at this batch."""
    return bool(_lib.load().mvk_conv4s2_scaled_ok(n, h, w, Cu, Cv))


def conv_down(U, wdown, bias, n, h, w, Cu, Cv, act=NONE, u_nchw=False, u_act_src=None, u_act=NONE,
              v_act_src=None, v_act=NONE, out_bias=None, in_bf3=False, frag=None, amax=None, out=None):
    """out_bias: bias parameter whose gradient is the per-channel sum of the result (backward-data use): fused into
    the launch; returns (V, grad for autograd) then.  amax = (x_amax, w_amax, y_amax): the amax protocol (mvk_conv4s2_down_s;
    x and w bounds given = scaled fp16 pairs, y_amax = zeroed slot that receives max |V|).  out: the buffer V is written to."""
    V = out if out is not None else torch.empty((n, h, w, Cv), dtype=torch.float32, device=U.device)
    ws = _ws(V)
    tb, rb = _bias_target(out_bias)
    if amax is not None:
        if u_nchw or u_act_src is not None or in_bf3:
            raise _lib.MvkError("conv_down: the amax form takes NHWC fp32 input without a fused input activation")
        call("mvk_conv4s2_down_s", ptr(U), ptr(wdown), ptr(bias), ptr(V), n, h, w, Cu, Cv, act, ptr(v_act_src), v_act, ptr(tb),
             ptr(amax[0]), ptr(amax[1]), ptr(amax[2]), ptr(ws), ws.numel(), ptr(frag if frag is not None else wfrag(wdown)),
             stream_ptr())
        return V if out_bias is None else (V, rb)
    call("mvk_conv4s2_down", ptr(U), ptr(wdown), ptr(bias), ptr(V), n, h, w, Cu, Cv, act, int(u_nchw),
         ptr(u_act_src), u_act, ptr(v_act_src), v_act, ptr(tb), ptr(ws), ws.numel(), FMT_IN_BF3 if in_bf3 else 0,
         ptr(frag if frag is not None else wfrag(wdown)), stream_ptr())
    return V if out_bias is None else (V, rb)


def conv_up(V, wup, bias, n, h, w, Cu, Cv, act=NONE, u_nchw=False, u_act_src=None, u_act=NONE, out_bias=None,
            in_bf3=False, frag=None, amax=None, out=None):
    U = out if out is not None else torch.empty((n, Cu, 2 * h, 2 * w) if u_nchw else (n, 2 * h, 2 * w, Cu), dtype=torch.float32,
                                                device=V.device)
    ws = _ws(U)
    tb, rb = _bias_target(out_bias)
    if amax is not None:  # (x_amax, w_amax, y_amax): see conv_down
        if u_nchw or in_bf3:
            raise _lib.MvkError("conv_up: the amax form writes NHWC and reads fp32")
        call("mvk_conv4s2_up_s", ptr(V), ptr(wup), ptr(bias), ptr(U), n, h, w, Cu, Cv, act, ptr(u_act_src), u_act, ptr(tb),
             ptr(amax[0]), ptr(amax[1]), ptr(amax[2]), ptr(ws), ws.numel(), ptr(frag if frag is not None else wfrag(wup)),
             stream_ptr())
        return U if out_bias is None else (U, rb)
    call("mvk_conv4s2_up", ptr(V), ptr(wup), ptr(bias), ptr(U), n, h, w, Cu, Cv, act, int(u_nchw),
         ptr(u_act_src), u_act, ptr(tb), ptr(ws), ws.numel(), FMT_IN_BF3 if in_bf3 else 0,
         ptr(frag if frag is not None else wfrag(wup)), stream_ptr())
    return U if out_bias is None else (U, rb)


LEAKY = ACT["leaky_relu_0.2"]


def conv3x3(X, wpack, bias, n, H, W, Cin, Cout, act=NONE, y_act_src=None, y_src_act=NONE, out_bias=None, res=None,
            res_alpha=1.0, y_amax=None):
    """3x3/1/1 convolution on NHWC (forward with the forward pack; backward data with the backward pack and Cin/Cout
    swapped, y_act_src = the activation whose derivative multiplies the result, out_bias = the bias whose gradient is
    the channel sum of the result, res: the result becomes res + res_alpha * result in the same pass)."""
    Y = _new((n, H, W, Cout), X)
    ws = _ws(X)
    if res is not None:
        if out_bias is not None:
            raise _lib.MvkError("conv3x3: a residual and a fused bias gradient are exclusive")
        call("mvk_conv3x3_res", ptr(X), ptr(wpack), ptr(bias), ptr(Y), n, H, W, Cin, Cout, act, ptr(y_act_src), y_src_act,
             ptr(res), float(res_alpha), ptr(ws), ws.numel(), stream_ptr())
        return Y
    tb, rb = _bias_target(out_bias)
    if y_amax is not None:  # image on the input side + published maximum (mvk_conv3x3_y; MvkError when the shape is not covered)
        call("mvk_conv3x3_y", ptr(X), ptr(wpack), ptr(bias), ptr(Y), n, H, W, Cin, Cout, act, ptr(y_act_src), y_src_act,
             ptr(tb), ptr(y_amax), ptr(ws), ws.numel(), stream_ptr())
        return Y if out_bias is None else (Y, rb)
    call("mvk_conv3x3", ptr(X), ptr(wpack), ptr(bias), ptr(Y), n, H, W, Cin, Cout, act, ptr(y_act_src), y_src_act,
         ptr(tb), ptr(ws), ws.numel(), stream_ptr())
    return Y if out_bias is None else (Y, rb)


def conv3x3_wgrad(X, dY, wparam, n, H, W, Cin, Cout):
    dw, rw = _grad_target(wparam)
    ws = _ws(X)
    call("mvk_conv3x3_wgrad", ptr(X), ptr(dY), ptr(dw), n, H, W, Cin, Cout, ptr(ws), ws.numel(), stream_ptr())
    return rw


def conv3x3_fused_ok(n, H, W, Cin, Cout):
    """True when mvk_conv3x3_f / mvk_conv3x3_wgrad_f (the register-stationary kernels) take this problem: the elementwise
    passes of a ResnetBlock are then folded into the convolutions (ResnetStackFn)."""
    return bool(_lib.load().mvk_conv3x3_fused_ok(n, H, W, Cin, Cout))


def conv3x3_f(X, wpack, bias, n, H, W, Cin, Cout, act=NONE, y_act_src=None, y_src_act=NONE, res=None, res_alpha=1.0,
              out_bias=None, x_act=NONE, pre_scale=1.0):
    """Y = [res + res_alpha *] (act(pre_scale * conv(x_act(X)) + bias) * y_src_act'(y_act_src)); out_bias as in conv3x3."""
    Y = _new((n, H, W, Cout), X)
    ws = _ws(X)
    tb, rb = _bias_target(out_bias)
    call("mvk_conv3x3_f", ptr(X), ptr(wpack), ptr(bias), ptr(Y), n, H, W, Cin, Cout, act, ptr(y_act_src), y_src_act, ptr(res),
         float(res_alpha), ptr(tb), x_act, float(pre_scale), ptr(ws), ws.numel(), stream_ptr())
    return Y if out_bias is None else (Y, rb)


# ---- scaled-fp16 form of the register-stationary 3x3 kernels (csrc/bf3.hpp: 3 MFMAs per product instead of 6) --------------
# MVK_C3_F16=0 (under MVK_TUNE=1) keeps every 3x3 convolution on the bf16-piece kernels.
C3_F16 = _lib.tune("MVK_C3_F16", "1") != "0"
# the same product form for the 4x4 / stride-2 layers of the SVHN decoder (csrc/imgconv.hip NP = 2); MVK_IMG_F16=0: bf16 pieces
IMG_F16 = _lib.tune("MVK_IMG_F16", "1") != "0"
# decoder rows from which SVHNDecoderFn takes that form (below, the in-kernel conversion of the weights costs what the cheaper
# product saves); tests set 1 (with debug flag 0x200) so the small goldens meet these kernels too
IMG_F16_MIN_ROWS = 1024


def _amax_slots(like, n, create=False):
    """n zeroed device scalars.  Inside a pack_scope they are carved from the ONE arena the scope filled when it was entered
    (in front of every stream fork of the forward pass): one fill per forward pass instead of one per pool, all of them on
    the step's critical chain.  Outside a scope (backward passes): a fill on the current stream."""
    sc = _PACK_SCOPE
    if sc is not None:
        ar = sc.get("amax")
        if ar is not None and ar.device == like.device and sc["amax_pos"] + n <= ar.numel():
            sc["amax_pos"] += n
            return ar[sc["amax_pos"] - n:sc["amax_pos"]]
    return torch.zeros(n, dtype=torch.float32, device=like.device)


class AmaxPool:
    """Zeroed device scalars for the `amax` protocol (one fill launch per pool): a launch publishes max |Y| into a slot by
    atomic max, the launch that consumes Y takes its operand scale from it.  A slot is used by ONE producer."""

    def __init__(self, like, slots):
        self.t = _amax_slots(like, slots)
        self.i = 0

    def take(self):
        if self.i >= self.t.numel():
            self.t, self.i = torch.zeros_like(self.t), 0
        self.i += 1
        return self.t[self.i - 1:self.i]


def amax_of(x, slot):
    """slot <- max(slot, max |x|) (mvk_amax); returns the slot."""
    call("mvk_amax", ptr(x), x.numel(), ptr(slot), stream_ptr())
    return slot


def conv3x3_scaled_ok(n, H, W, Cin, Cout):
    """True when mvk_conv3x3_s takes this problem."""
    return C3_F16 and bool(_lib.load().mvk_conv3x3_scaled_ok(n, H, W, Cin, Cout))


def conv3x3_s(X, wpack, bias, n, H, W, Cin, Cout, x_amax, w_amax, y_amax=None, act=NONE, y_act_src=None, y_src_act=NONE,
              res=None, res_alpha=1.0, out_bias=None, x_act=NONE, pre_scale=1.0):
    """conv3x3_f on scaled fp16 pairs: x_amax / w_amax = device scalars bounding max |X| / max |wpack|, y_amax (optional,
    zeroed) receives max |Y|."""
    Y = _new((n, H, W, Cout), X)
    ws = _ws(X)
    tb, rb = _bias_target(out_bias)
    call("mvk_conv3x3_s", ptr(X), ptr(wpack), ptr(bias), ptr(Y), n, H, W, Cin, Cout, act, ptr(y_act_src), y_src_act, ptr(res),
         float(res_alpha), ptr(tb), x_act, float(pre_scale), ptr(x_amax), ptr(w_amax), ptr(y_amax), ptr(ws), ws.numel(),
         stream_ptr())
    return Y if out_bias is None else (Y, rb)


def conv3x3_s2(X, wpack, bias, n, H, W, Cin, Cout, x_amax, w_amax, y_amax, act, res, res_alpha):
    """conv3x3_s in its residual form with a second store -> (res + res_alpha * a, a), a = act(conv + bias)."""
    Y, A = _new((n, H, W, Cout), X), _new((n, H, W, Cout), X)
    ws = _ws(X)
    call("mvk_conv3x3_s2", ptr(X), ptr(wpack), ptr(bias), ptr(Y), ptr(A), n, H, W, Cin, Cout, act, ptr(res), float(res_alpha),
         ptr(x_amax), ptr(w_amax), ptr(y_amax), ptr(ws), ws.numel(), stream_ptr())
    return Y, A


def conv3x3_s_split(X, wpack, bias, n, H, W, Cin, Cout, x_amax, w_amax, y_amax=None, act=NONE, y_act_src=None, y_src_act=NONE,
                    out_bias=None, x_act=NONE, pre_scale=1.0):
    """conv3x3_s for a layer with 256 input channels: two launches over 128-channel slices (mvk_conv3x3_s_part) — the first leaves
    its partial sum, the second adds it in front of its bias / activation / mask and publishes max |Y|.  out_bias: the column
    sums of Y (the bias gradient of the layer below) come from a pass of their own."""
    half = Cin // 2
    part, Y = _new((n, H, W, Cout), X), _new((n, H, W, Cout), X)
    call("mvk_conv3x3_s_part", ptr(X), Cin, 0, ptr(wpack), None, ptr(part), n, H, W, half, Cout, NONE, None, NONE, None, 0, x_act,
         float(pre_scale), ptr(x_amax), ptr(w_amax), None, stream_ptr())
    call("mvk_conv3x3_s_part", ptr(X), Cin, half, ptr(wpack), ptr(bias), ptr(Y), n, H, W, half, Cout, act, ptr(y_act_src), y_src_act,
         ptr(part), 1, x_act, float(pre_scale), ptr(x_amax), ptr(w_amax), ptr(y_amax), stream_ptr())
    return Y if out_bias is None else (Y, colsum(Y.view(-1, Cout), out_bias))


def conv3x3_wgrad_scaled_ok(n, H, W, Cin, Cout):
    """True when mvk_conv3x3_wgrad_s takes this problem."""
    return C3_F16 and bool(_lib.load().mvk_conv3x3_wgrad_scaled_ok(n, H, W, Cin, Cout))


def conv3x3_wgrad_s(X, dY, wparam, bparam, n, H, W, Cin, Cout, x_amax, dy_amax, x_act=NONE, dy_scale=1.0):
    """conv3x3_wgrad_f on scaled fp16 pairs; x_amax / dy_amax: device scalars bounding max |X| / max |dY|."""
    dw, rw = _grad_target(wparam)
    tb, rb = _bias_target(bparam)
    ws = _ws(X)
    call("mvk_conv3x3_wgrad_s", ptr(X), ptr(dY), ptr(dw), ptr(tb), n, H, W, Cin, Cout, x_act, float(dy_scale), ptr(x_amax),
         ptr(dy_amax), ptr(ws), ws.numel(), stream_ptr())
    return rw, rb


def conv3x3_wgrad_f(X, dY, wparam, bparam, n, H, W, Cin, Cout, x_act=NONE, dy_scale=1.0):
    """dW += dy_scale * sum x_act(X) (x) dY and (bparam given) db += dy_scale * sum dY, one launch.  -> (dW ref, db ref)"""
    dw, rw = _grad_target(wparam)
    tb, rb = _bias_target(bparam)
    ws = _ws(X)
    call("mvk_conv3x3_wgrad_f", ptr(X), ptr(dY), ptr(dw), ptr(tb), n, H, W, Cin, Cout, x_act, float(dy_scale), ptr(ws),
         ws.numel(), stream_ptr())
    return rw, rb


def avgpool(x, n, H, W, C):
    y = _new((n, (H + 1) // 2, (W + 1) // 2, C), x)
    call("mvk_avgpool3s2_fwd", ptr(x), ptr(y), n, H, W, C, stream_ptr())
    return y


def avgpool_bwd(dy, n, H, W, C):
    dx = _new((n, H, W, C), dy)
    call("mvk_avgpool3s2_bwd", ptr(dy), ptr(dx), n, H, W, C, stream_ptr())
    return dx


def upsample2(x, n, H, W, C):
    y = _new((n, 2 * H, 2 * W, C), x)
    call("mvk_upsample2_fwd", ptr(x), ptr(y), n, H, W, C, stream_ptr())
    return y


def upsample2_bwd(dy, n, H, W, C):
    dx = _new((n, H, W, C), dy)
    call("mvk_upsample2_bwd", ptr(dy), ptr(dx), n, H, W, C, stream_ptr())
    return dx


# ---- noise with the generator state in device memory (mvk_device_rng) -------------------------------------------------
# (torch's generator would cost two extra host-issued fill launches per hipGraph replay)
def _rng_state(device):
    """The device-resident generator state, tied to torch's CUDA generator of that device: re-seeded from its seed whenever
    torch was re-seeded since the last draw.  A re-seed is seen as a changed seed or an offset that went backwards — every
    draw leaves a breadcrumb by advancing torch's (host-side) offset, so `torch.manual_seed(s)` twice with the same s and
    nothing drawn from torch in between is still noticed.  Not consulted while a stream is capturing (the launches inside
    a graph advance the state they find).

    The state tensor is allocated ONCE per device and re-seeded IN PLACE (a stream-ordered copy): a captured GraphedStep has
    its raw pointer baked into its mvk_device_rng launches, so the tensor must never be replaced — and a re-seed then also
    reaches every existing graph.  Draws must be stream-ordered with respect to each other (the {offset, ticket} protocol of
    device_rng_kernel serialises nothing): every caller in the package draws on the step's main stream or on a branch
    stream between that stream's fork and join."""
    ent = _RNG.get(device)
    if ent is not None and torch.cuda.is_current_stream_capturing():
        return ent[0]
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    seed, off = gen.initial_seed(), gen.get_offset()
    if ent is None or ent[1] != seed or off < ent[2]:
        if torch.cuda.is_current_stream_capturing():
            raise _lib.MvkError("the device generator state must exist before a graph capture starts (run one eager step)")
        fresh = torch.tensor([seed & 0x7FFFFFFFFFFFFFFF, off // 4, 0], dtype=torch.int64)
        if ent is None:
            ent = [torch.empty(3, dtype=torch.int64, device=device), seed, off]
            _RNG[device] = ent
        ent[0].copy_(fresh)  # pageable host source: the copy has read `fresh` when it returns; ordered on the current stream
        ent[1], ent[2] = seed, off
    ent[2] = off + 4
    gen.set_offset(ent[2])
    return ent[0]


def device_randn(shape, device, uniform=False, lo=0.0, hi=1.0):
    """N(0, 1) (or U[lo, hi)) noise of `shape` from the device-resident generator."""
    out = torch.empty(shape, dtype=torch.float32, device=device)
    call("mvk_device_rng", ptr(out), out.numel(), ptr(_rng_state(device)), 1 if uniform else 0, float(lo), float(hi), stream_ptr())
    return out


# Test hook (tests/relu_sites.py): a list that receives (node, first weight, activation tensors) from the forward of every
# network node, so a parity test can read which side of zero the HIP path put each ReLU / LeakyReLU unit on.  None = off (the default).
TAPS = None


def _tap(node, w, *acts):
    if TAPS is not None:
        TAPS.append((node, w, acts))


class TransposeActFn(Function):
    """y[b, c, r] = act(x[b, r, c]): NHWC <-> NCHW-flattened in ONE pass with the activation in front of the flatten
    (mvk_transpose_act); backward = the transposed gradient times act'(y)."""

    @staticmethod
    def forward(ctx, x, act):
        x = _c(x)
        b, r, c = x.shape
        y = _new((b, c, r), x)
        call("mvk_transpose_act", ptr(x), ptr(y), b, r, c, act, None, NONE, stream_ptr())
        ctx.act = act
        if act != NONE:
            ctx.save_for_backward(y)
            _tap("transpose_act", None, y)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        dy = _c(dy)
        b, c, r = dy.shape
        dx = _new((b, r, c), dy)
        y = ctx.saved_tensors[0] if ctx.act != NONE else None
        call("mvk_transpose_act", ptr(dy), ptr(dx), b, c, r, NONE, ptr(y), ctx.act, stream_ptr())
        return dx, None


def nhwc_to_flat_nchw(h, act=NONE):
    """[n, H, W, C] (NHWC) -> [n, C * H * W] in the reference's NCHW flatten order, with `act` applied on the way."""
    n, H, W, C = h.shape
    return TransposeActFn.apply(h.reshape(n, H * W, C), act).reshape(n, C * H * W)


def flat_nchw_to_nhwc(flat, C, H, W):
    """[n, C * H * W] (NCHW order) -> [n, H, W, C]."""
    n = flat.shape[0]
    return TransposeActFn.apply(flat.reshape(n, C, H * W), NONE).reshape(n, H, W, C)


def axpby(x, a, y, b, act=NONE, out=None):
    ref = x if x is not None else y
    out = torch.empty_like(ref) if out is None else out
    call("mvk_axpby", ptr(x), float(a), ptr(y), float(b), ref.numel(), act, ptr(out), stream_ptr())
    return out


def conv_wgrad(U, V, wparam, n, h, w, Cu, Cv, u_nchw=False, u_act_src=None, u_act=NONE, amax=None):
    """amax = (u_amax, v_amax): the scaled-fp16 launch (mvk_conv4s2_wgrad_s) where mvk_conv4s2_wgrad_scaled_ok says so."""
    dw, rw = _grad_target(wparam)
    ws = _ws(V)
    if (amax is not None and amax[0] is not None and amax[1] is not None and not u_nchw and u_act_src is None
            and _lib.load().mvk_conv4s2_wgrad_scaled_ok(n, h, w, Cu, Cv)):
        call("mvk_conv4s2_wgrad_s", ptr(U), ptr(V), ptr(dw), n, h, w, Cu, Cv, ptr(amax[0]), ptr(amax[1]), ptr(ws), ws.numel(),
             stream_ptr())
        return rw
    call("mvk_conv4s2_wgrad", ptr(U), ptr(V), ptr(dw), n, h, w, Cu, Cv, int(u_nchw), ptr(u_act_src), u_act,
         ptr(ws), ws.numel(), stream_ptr())
    return rw


# =====================================================================================================
# Encoder_VAE_MLP / Decoder_AE_MLP  (models/nn/default_architectures.py:21-72, 225-258)
# =====================================================================================================
class MLPEncoderFn(Function):
    """x -> [Linear+ReLU]*n -> (embedding, log_covariance).  params = (W0,b0, W1,b1, ..., We,be, Wl,bl)."""

    @staticmethod
    def forward(ctx, x, *params):
        n_layers = (len(params) - 4) // 2
        K0 = params[0].shape[1]
        x2 = _c(x.reshape(-1, K0))
        acts = [x2]
        h = x2
        for i in range(n_layers):
            h = linear_fwd(h, params[2 * i], params[2 * i + 1], RELU)
            acts.append(h)
        we, be, wl, bl = params[-4:]
        heads = heads_fwd(h, we, be, wl, bl, we.shape[0], 1, we.shape[1]) if we.shape == wl.shape else None
        if heads is not None:
            mu, lv = heads
        else:
            mu = linear_fwd(h, we, be, NONE)
            lv = linear_fwd(h, wl, bl, NONE)
        ctx.save_for_backward(*acts, *params)
        _tap("mlp_encoder", params[0], *acts[1:])
        ctx.n_layers = n_layers
        ctx.x_shape = x.shape
        return mu, lv

    @staticmethod
    @once_differentiable
    def backward(ctx, dmu, dlv):
        n = ctx.n_layers
        saved = ctx.saved_tensors
        acts, params = saved[: n + 1], saved[n + 1 :]
        we, be, wl, bl = params[-4:]
        dmu, dlv = _c(dmu), _c(dlv)
        h = acts[-1]
        grads = [None] * len(params)
        prev_src, prev_act = (h, RELU) if n > 0 else (None, NONE)
        need_dx = ctx.needs_input_grad[0]
        dh = None
        bias_done = False  # bias gradient of layer i already produced by the backward-data launch of layer i+1
        # both heads in one launch: weight / bias gradients, the gradient w.r.t. the last hidden layer's PRE-activation
        # (ReLU' applied) and, with hidden layers, that layer's bias gradient
        fused = heads_bwd(h, prev_act, [dmu, dlv], [we, wl], [be, bl], 1, h.shape[1], want_dx=n > 0 or need_dx,
                          prev_bias=params[2 * n - 1] if n > 0 else None) if we.shape == wl.shape and heads_bwd_mlp(h.device) else None
        if fused is not None:
            dh, (grads[-4], grads[-2]), (grads[-3], grads[-1]), gprev = fused
            if n > 0:
                grads[2 * n - 1], bias_done = gprev, True
        else:
            grads[-4], grads[-3] = linear_bwd_weight(dmu, h, we, be)
            grads[-2], grads[-1] = linear_bwd_weight(dlv, h, wl, bl)
            if n > 0 or need_dx:
                dh = linear_bwd_data(dmu, we, prev_out=prev_src, prev_act=prev_act)
                linear_bwd_data(dlv, wl, prev_out=prev_src, prev_act=prev_act, out=dh, accumulate=True)
        for i in range(n - 1, -1, -1):
            w, inp = params[2 * i], acts[i]
            gb = grads[2 * i + 1]
            grads[2 * i], gb2 = linear_bwd_weight(dh, inp, w, None if bias_done else params[2 * i + 1])
            grads[2 * i + 1] = gb if bias_done else gb2
            bias_done = False
            if i > 0:
                dh, grads[2 * i - 1] = linear_bwd_data(dh, w, prev_out=acts[i], prev_act=RELU, prev_bias=params[2 * i - 1])
                bias_done = True
            elif need_dx:
                dh = linear_bwd_data(dh, w)
        dx = dh.reshape(ctx.x_shape) if need_dx else None
        return (dx, *grads)


class MLPHeadsFn(Function):
    """x -> [Linear+ReLU]*n -> n_heads linear heads (Encoder_VAE_MLP_Style: embedding, log_var, style_embedding,
    style_log_var; default_architectures.py:75-141).  params = (W0,b0, ..., Wh1,bh1, ..., Whn,bhn)."""

    @staticmethod
    def forward(ctx, x, n_heads, *params):
        n_layers = (len(params) - 2 * n_heads) // 2
        K0 = params[0].shape[1]
        x2 = _c(x.reshape(-1, K0))
        acts = [x2]
        h = x2
        for i in range(n_layers):
            h = linear_fwd(h, params[2 * i], params[2 * i + 1], RELU)
            acts.append(h)
        outs = tuple(linear_fwd(h, params[2 * (n_layers + j)], params[2 * (n_layers + j) + 1], NONE)
                     for j in range(n_heads))
        ctx.save_for_backward(*acts, *params)
        _tap("mlp_heads", params[0], *acts[1:])
        ctx.n_layers, ctx.n_heads = n_layers, n_heads
        ctx.x_shape = x.shape
        return outs

    @staticmethod
    @once_differentiable
    def backward(ctx, *douts):
        n, nh = ctx.n_layers, ctx.n_heads
        saved = ctx.saved_tensors
        acts, params = saved[: n + 1], saved[n + 1 :]
        h = acts[-1]
        grads = [None] * len(params)
        prev_src, prev_act = (h, RELU) if n > 0 else (None, NONE)
        need_dx = ctx.needs_input_grad[0]
        dh = None
        fused = None
        if heads_bwd_mlp(h.device) and nh <= 2 and (n > 0 or need_dx):
            # every head in one launch; with hidden layers it also emits the last hidden layer's bias gradient
            hw = [params[2 * (n + j)] for j in range(nh)]
            fused = heads_bwd(h, prev_act, [_c(d) for d in douts[:nh]], hw, [params[2 * (n + j) + 1] for j in range(nh)],
                              1, h.shape[1], prev_bias=params[2 * n - 1] if n > 0 else None)
        if fused is not None:
            dh, gw, gb, gprev = fused
            for j in range(nh):
                grads[2 * (n + j)], grads[2 * (n + j) + 1] = gw[j], gb[j]
        for j in range(nh if fused is None else 0):
            w, b = params[2 * (n + j)], params[2 * (n + j) + 1]
            dy = _c(douts[j])
            grads[2 * (n + j)], grads[2 * (n + j) + 1] = linear_bwd_weight(dy, h, w, b)
            if n > 0 or need_dx:  # pre-activation gradient of the last hidden layer: all heads, ReLU' in the epilogue
                if dh is None:
                    dh = linear_bwd_data(dy, w, prev_out=prev_src, prev_act=prev_act)
                else:
                    linear_bwd_data(dy, w, prev_out=prev_src, prev_act=prev_act, out=dh, accumulate=True)
        for i in range(n - 1, -1, -1):
            w, inp = params[2 * i], acts[i]
            if fused is not None and i == n - 1:  # its bias gradient came with the heads' launch
                grads[2 * i], _ = linear_bwd_weight(dh, inp, w, None)
                grads[2 * i + 1] = gprev
            else:
                grads[2 * i], grads[2 * i + 1] = linear_bwd_weight(dh, inp, w, params[2 * i + 1])
            if i > 0:
                dh = linear_bwd_data(dh, w, prev_out=acts[i], prev_act=RELU)
            elif need_dx:
                dh = linear_bwd_data(dh, w)
        dx = dh.reshape(ctx.x_shape) if need_dx else None
        return (dx, None, *grads)


# The MLP decoder at the decoder batch on pre-split fp16 pair planes (csrc/dense16.hip): MVK_DENSE16=0 keeps the tiled engine
DENSE16 = _lib.tune("MVK_DENSE16", "1") != "0"
DENSE16_MIN_ROWS = 1024  # below, the tiled engine's latency-sized tiles win (tests set 1 to meet the small goldens)


def mlp_fused_tail_ok(n, L, H, D):
    """MLPDecoderFn's fused tail (mvk_dense16_*) takes z [n, L] -> Linear(L, H) + ReLU -> Linear(H, D) + Sigmoid."""
    return (DENSE16 and n >= DENSE16_MIN_ROWS and 4 <= L <= 32 and L % 4 == 0 and 16 <= H <= 1024 and H % 16 == 0
            and 256 % (H // 4) == 0 and D % 8 == 0 and bool(_lib.load().mvk_dense16_ok(n, D, H)))


def _planes(rows, cols, like):
    """An fp16 pair-planes buffer [2][rows][cols] (hi, lo): the bytes of the fp32 tensor it replaces."""
    t = torch.empty((2, rows, cols), dtype=torch.float16, device=like.device)
    return t, t[0], t[1]


def dense16_pack(w, raw=False):
    """Planes of a Linear weight [N][K] in both orientations + the per-row inverse scales; once per forward pass inside a
    pack_scope (the cache dies with the scope: the weights change at the next optimizer step).  raw: launch here, no cache."""
    sc = _PACK_SCOPE
    key = ("dense16", w.data_ptr(), tuple(w.shape))
    rot = schedule.rotation(w.device)
    if not raw and rot is not None and key in rot.cache:  # packed by the head branch of a rotated step, behind w's update
        rot.wait()
        return rot.cache[key]
    if not raw and sc is not None and key in sc["cache"]:
        return sc["cache"][key]
    N, K = w.shape
    nk, kn = _planes(N, K, w), _planes(K, N, w)
    nk_inv, kn_inv = _new((N,), w), _new((K,), w)
    call("mvk_dense16_pack", ptr(w), N, K, ptr(nk[1]), ptr(nk[2]), ptr(nk_inv), ptr(kn[1]), ptr(kn[2]), ptr(kn_inv), stream_ptr())
    out = (nk, nk_inv, kn, kn_inv)
    if sc is not None and not raw:
        sc["cache"][key] = out
    return out


def dense16_xamax(x):
    """Device scalar >= max |x| of a target batch, once per forward pass inside a pack_scope."""
    sc = _PACK_SCOPE
    key = ("dense16_xamax", x.data_ptr(), tuple(x.shape))
    if sc is not None and key in sc["cache"]:
        return sc["cache"][key]
    slot = _amax_slots(x, 1)
    call("mvk_amax", ptr(x), x.numel(), ptr(slot), stream_ptr())
    if sc is not None:
        sc["cache"][key] = slot
    return slot


def register_const_grad(t, value):
    """ReconLossFn.backward: `t` was filled with `value` by the forward launch (the unit-seed path)."""
    import weakref

    _CONST_GRADS[t.data_ptr()] = (weakref.ref(t), t.numel(), float(value))


def const_grad(t):
    """The constant every element of the gradient tensor `t` holds, when a producer registered it (None otherwise: read it on
    the device).  The registration dies with the tensor: a recycled address never matches."""
    e = _CONST_GRADS.get(t.data_ptr())
    if e is None:
        return None
    ref, numel, value = e
    src = ref()
    if src is None or numel != t.numel() or src.data_ptr() != t.data_ptr():
        _CONST_GRADS.pop(t.data_ptr(), None)
        return None
    return value


def _check_nll_weight(nll_x, nll_weight):
    """The fused tails store nll_weight * d NLL / d pre-activation and divide by it on their general backward path: a zero or
    non-finite weight has no such form (the decoders' `reconstruction_nll` return None for it and the caller takes the generic
    likelihood kernel)."""
    if nll_x is not None and not (math.isfinite(float(nll_weight)) and float(nll_weight) != 0.0):
        raise _lib.MvkError(f"fused decoder tail: nll_weight must be finite and non-zero, got {nll_weight}")


class MLPDecoderFn(Function):
    """z[...,L] -> Linear+ReLU -> Linear+Sigmoid -> reshape(*z.shape[:-1], *input_dim).

    nll_x [B, D] given: the FUSED TAIL on fp16 pair planes (csrc/dense16.hip; the caller checks `mlp_fused_tail_ok`) — the
    output layer scores its rows against nll_x[row % B] by a Normal(nll_scale) likelihood in its epilogue and the node returns
    PARTIAL NLL row sums [P, *z.shape[:-1]] (their sum over P is -log p(x | decoder(z)) per row) instead of the reconstruction;
    what is kept for the backward pass is nll_weight * d NLL / d pre-activation as planes.  nll_weight = the weight the rows
    are expected to enter the loss with (d loss / d rows): when the backward pass receives exactly that constant (const_grad)
    nothing is rescaled; any other upstream gradient takes the general path (planes -> fp32 times the row factor)."""

    WAITS_FOR_LOSS = True  # the backward calls schedule.wait_loss before it reads a row gradient (schedule.orders_behind_loss)

    @staticmethod
    def forward(ctx, z, w0, b0, w1, b1, input_dim, nll_x=None, nll_scale=1.0, nll_weight=1.0):
        _check_nll_weight(nll_x, nll_weight)
        L = w0.shape[1]
        z2 = _c(z.reshape(-1, L))
        ctx.fused = nll_x is not None
        ctx.z_shape = z.shape
        if ctx.fused:
            n, H, D = z2.shape[0], w0.shape[0], w1.shape[0]
            # rotated step (Rotation): the weight gradients of w1 / b1 / w0 run at the head of the NEXT step; what they read (z,
            # the planes of h and of the stored gradient, their bounds, the column-sum partials; dh in backward) is persistent
            rot = schedule.rotation(z2.device)
            if rot is not None:
                rot.wait()  # w0 is read as it is, w1 through planes packed behind its update
            if not (schedule.ROT_MLP and rot is not None and schedule.LATE_LEAVES and schedule.scope(z2.device) is not None
                    and all(_is_direct(t) for t in (w0, w1, b1))):
                rot = None
            ctx.rot, ctx.rot_mode = rot, schedule.ROT_MLP
            if rot is not None and schedule.ROT_MLP == 2:
                # mode 2 rotates the first layer's gradient only: z at a fixed address (copied HERE, on this branch's stream: the
                # late-leaf stream must never wait for a branch stream — hip::Stream::EndCapture recursion, see deferred_reductions)
                z2 = rot.buf(("mlp_dec", w0.data_ptr(), z2.shape[0], "z"), z2.shape).copy_(z2)
            if schedule.ROT_MLP != 1:
                rot = None
            rkey = ("mlp_dec", w0.data_ptr(), n)
            nk, nk_inv, kn, kn_inv = dense16_pack(w1)
            xam = dense16_xamax(nll_x)
            zam = _amax_slots(z2, 1)
            lib = _lib.load()
            P, CR = lib.mvk_dense16_fwd_nll_rows(D), lib.mvk_dense16_colsum_rows(n)
            if rot is None:
                hp = _planes(n, H, z2)
                gp = _planes(n, D, z2)
                bounds = _new((2,), z2)  # [bound of h, bound of G]
                cs = _new((CR, D), z2)
            else:
                z2 = rot.buf(rkey + ("z",), z2.shape).copy_(z2)
                hp = rot.buf(rkey + ("hp",), (2, n, H), torch.float16)
                hp = (hp, hp[0], hp[1])
                gp = rot.buf(rkey + ("gp",), (2, n, D), torch.float16)
                gp = (gp, gp[0], gp[1])
                bounds = rot.buf(rkey + ("bounds",), (2,))
                cs = rot.buf(rkey + ("cs",), (CR, D))
            rows = _new((P, n), z2)
            call("mvk_amax", ptr(z2), z2.numel(), ptr(zam), stream_ptr())
            call("mvk_dense16_first", ptr(z2), ptr(w0), ptr(b0), ptr(zam), ptr(hp[1]), ptr(hp[2]), ptr(bounds[0:1]), n, H, L,
                 RELU, stream_ptr())
            call("mvk_dense16_fwd_nll", ptr(hp[1]), ptr(hp[2]), ptr(bounds[0:1]), ptr(nk[1]), ptr(nk[2]), ptr(nk_inv), ptr(b1),
                 ptr(nll_x), nll_x.shape[0], ptr(xam), float(nll_scale), float(nll_weight), ptr(gp[1]), ptr(gp[2]),
                 ptr(bounds[1:2]), ptr(rows), ptr(cs), n, D, H, stream_ptr())
            ctx.save_for_backward(z2, hp[0], gp[0], bounds, kn[0], kn_inv, cs, w0, b0, w1, b1)
            ctx.nll_weight = float(nll_weight)
            if TAPS is not None:  # tests: the hidden activation as an fp32 tensor (the sign of h is the sign of its hi plane)
                h = _new((n, H), z2)
                call("mvk_dense16_unsplit", ptr(hp[1]), ptr(hp[2]), ptr(bounds[0:1]), None, 1.0, 0, n, H, ptr(h), stream_ptr())
                _tap("mlp_decoder", w0, h)
            return rows.view(P, *z.shape[:-1])
        h = linear_fwd(z2, w0, b0, RELU)
        out = linear_fwd(h, w1, b1, SIGMOID)
        ctx.save_for_backward(z2, h, out, w0, b0, w1, b1)
        _tap("mlp_decoder", w0, h)
        return out.view(*z.shape[:-1], *input_dim)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        if ctx.fused:
            return MLPDecoderFn._backward_fused(ctx, dout)
        z2, h, out, w0, b0, w1, b1 = ctx.saved_tensors
        dout = _c(dout).view(out.shape)
        # pre-activation gradient of the output layer + its bias gradient in one pass; the two GEMMs then read it
        # plainly (instead of re-deriving it from dout and out on every operand load, and a third time for the bias)
        dpre = torch.empty_like(dout)
        tb1, db1 = _grad_target(b1)
        ws = _ws(dout)
        call("mvk_act_bwd_colsum", ptr(dout), ptr(out), SIGMOID, dout.shape[0], dout.shape[1], ptr(dpre), ptr(tb1),
             ptr(ws), ws.numel(), stream_ptr())
        dw1, _ = linear_bwd_weight(dpre, h, w1, None)
        dh, db0 = linear_bwd_data(dpre, w1, prev_out=h, prev_act=RELU, prev_bias=b0)
        dw0, _ = linear_bwd_weight(dh, z2, w0, None)
        dz = None
        if ctx.needs_input_grad[0]:
            dz = linear_bwd_data(dh, w0).view(ctx.z_shape)
        return dz, dw0, db0, dw1, db1, None, None, None, None

    @staticmethod
    def _backward_fused(ctx, drows):
        z2, hp, gp, bounds, kn, kn_inv, cs, w0, b0, w1, b1 = ctx.saved_tensors
        schedule.wait_tail_bwd(z2.device)
        n, H, D = z2.shape[0], w0.shape[0], w1.shape[0]
        hb, gb = bounds[0:1], bounds[1:2]
        c = const_grad(drows)
        ws = _ws(z2)
        if c is not None and c == ctx.nll_weight:
            # the planes already hold d loss / d pre-activation: two GEMMs on planes, bias gradients out of their launches
            tw1, dw1 = _grad_target(w1)
            tb1, db1 = _grad_target(b1)
            tb0, db0 = _grad_target(b0)
            rot = ctx.rot if (ctx.rot is not None and schedule.rotation(z2.device) is ctx.rot and dw1 is None and db1 is None) else None
            rot0 = rot if (rot is not None and ctx.rot_mode == 2) else None
            dh = _new((n, H), z2) if rot is None else rot.buf(("mlp_dec", w0.data_ptr(), n, "dh"), (n, H))
            if rot0 is not None:
                rot = None
            call("mvk_dense16_bwd_data", ptr(gp[0]), ptr(gp[1]), ptr(gb), ptr(kn[0]), ptr(kn[1]), ptr(kn_inv), ptr(hp[0]), ptr(dh),
                 ptr(tb0), ptr(ws), ws.numel(), n, H, D, stream_ptr())
            # the gradient of z first (the posterior's backward waits for it), the weight gradients — leaves — behind it
            dz = None
            if ctx.needs_input_grad[0]:
                dz = linear_bwd_data(dh, w0).view(ctx.z_shape)

            def wgrad1():
                wsl = _ws(z2)
                call("mvk_dense16_wgrad", ptr(gp[0]), ptr(gp[1]), ptr(gb), ptr(hp[0]), ptr(hp[1]), ptr(hb), ptr(cs), cs.shape[0],
                     ptr(tw1), ptr(tb1), ptr(wsl), wsl.numel(), n, D, H, stream_ptr())

            if rot is not None:  # rotated step: both weight gradients are the head of the next step (Rotation.begin_step)
                def leaves():
                    wgrad1()
                    linear_bwd_weight(dh, z2, w0, None)

                def prepare(r):  # behind the update of w1: its planes for the next forward pass
                    r.cache[("dense16", w1.data_ptr(), tuple(w1.shape))] = dense16_pack(w1, raw=True)

                rot.push(leaves, (w1, b1, w0), prepare)
                return dz, None, db0, None, None, None, None, None, None

            wgrad1()
            # the first layer's weight gradient, a leaf: postponed into the tail of the step when its target is a view of the flat
            # gradient buffer (run_last)
            dw0 = None
            if rot0 is not None:  # mode 2: the first layer's weight gradient is the head of the next step (z2 is the fixed copy)
                rot0.push(lambda: linear_bwd_weight(dh, z2, w0, None), (w0,), None)
            elif not _is_direct(w0) or not schedule.run_last(z2.device, lambda: linear_bwd_weight(dh, z2, w0, None), dh, z2, params=(w0,)):
                dw0, _ = linear_bwd_weight(dh, z2, w0, None)
            return dz, dw0, db0, dw1, db1, None, None, None, None
        else:  # general upstream gradient: d pre = G * drows[column tile, row] / nll_weight as an fp32 tensor, then the tiled engine
            schedule.wait_loss(z2.device)
            drows = _c(drows).reshape(-1, n)
            dpre = _new((n, D), z2)
            h = _new((n, H), z2)
            call("mvk_dense16_unsplit", ptr(gp[0]), ptr(gp[1]), ptr(gb), ptr(drows), 1.0 / ctx.nll_weight, 128, n, D, ptr(dpre),
                 stream_ptr())
            call("mvk_dense16_unsplit", ptr(hp[0]), ptr(hp[1]), ptr(hb), None, 1.0, 0, n, H, ptr(h), stream_ptr())
            db1 = colsum(dpre, b1)
            dw1, _ = linear_bwd_weight(dpre, h, w1, None)
            dh, db0 = linear_bwd_data(dpre, w1, prev_out=h, prev_act=RELU, prev_bias=b0)
        dz = None
        if ctx.needs_input_grad[0]:
            dz = linear_bwd_data(dh, w0).view(ctx.z_shape)
        dw0, _ = linear_bwd_weight(dh, z2, w0, None)
        return dz, dw0, db0, dw1, db1, None, None, None, None


# =====================================================================================================
# Encoder_VAE_SVHN / Decoder_VAE_SVHN  (models/nn/svhn.py:7-70), NHWC activations inside
# =====================================================================================================
class SVHNEncoderFn(Function):
    """x[B,C,32,32] NCHW -> 3x(Conv 4/2/1 + ReLU) -> two Conv(4,2,0) heads -> (mu, lv) [B,L]."""

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, w2, b2, wc1, bc1, wc2, bc2):
        x = _c(x)
        B, C0, H, W = x.shape
        chans = [C0, w0.shape[0], w1.shape[0], w2.shape[0]]
        L = wc1.shape[0]
        if _lib.load().mvk_conv4s2_small_up_supported(H // 2, W // 2, chans[0], chans[1]):
            # the image-consuming layer reads the reference weight layout: no pack in front of the encoder's first kernel
            h1 = _new((B, H // 2, W // 2, chans[1]), x)
            call("mvk_conv4s2_small_down_fwd_wref", ptr(x), ptr(w0), ptr(b0), ptr(h1), B, H // 2, W // 2, chans[0], chans[1], RELU,
                 stream_ptr())
            (wd1, wu1), (wd2, wu2), (wdc1, _), (wdc2, _) = pack_weights(
                [(w1, True, True), (w2, True, True), (wc1, True, False), (wc2, True, False)])
        else:
            (wd0, _), (wd1, wu1), (wd2, wu2), (wdc1, _), (wdc2, _) = pack_weights(
                [(w0, True, False), (w1, True, True), (w2, True, True), (wc1, True, False), (wc2, True, False)])
            h1 = conv_down(x, wd0, b0, B, H // 2, W // 2, chans[0], chans[1], RELU, u_nchw=True)
        h2 = conv_down(h1, wd1, b1, B, H // 4, W // 4, chans[1], chans[2], RELU)
        h3 = conv_down(h2, wd2, b2, B, H // 8, W // 8, chans[2], chans[3], RELU)
        if (H // 8, W // 8) != (4, 4):
            raise _lib.MvkError("Encoder_VAE_SVHN expects 32x32 inputs (4x4 feature map before the heads)")
        Kf = 16 * chans[3]
        h3f = h3.view(B, Kf)
        heads = heads_fwd(h3f, wdc1, bc1, wdc2, bc2, L, L, 1)
        if heads is not None:
            mu, lv = heads
        else:
            mu = gemm(h3f, wdc1, B, L, Kf, bias=bc1, bias_mod=L)
            lv = gemm(h3f, wdc2, B, L, Kf, bias=bc2, bias_mod=L)
        ctx.save_for_backward(x, h1, h2, h3, wu1, wu2, wdc1, wdc2, w0, b0, w1, b1, w2, b2, wc1, bc1, wc2, bc2)
        _tap("svhn_encoder", w0, h1, h2, h3)  # NHWC
        ctx.frags = (wfrag(wu1), wfrag(wu2))  # saved tensors come back without Python attributes
        ctx.dims = (B, H, W, chans, L)
        return mu, lv

    @staticmethod
    @once_differentiable
    def backward(ctx, dmu, dlv):
        x, h1, h2, h3, wu1, wu2, wdc1, wdc2, w0, b0, w1, b1, w2, b2, wc1, bc1, wc2, bc2 = ctx.saved_tensors
        B, H, W, ch, L = ctx.dims
        dmu, dlv = _c(dmu).view(B, L), _c(dlv).view(B, L)
        Kf = 16 * ch[3]
        h3f = h3.view(B, Kf)
        schedule.defer_flush_sibling(x.device, node_params=(w0, b0, w1, b1, w2, b2, wc1, bc1, wc2, bc2))
        # heads: both weight gradients (in the Conv2d layout), both bias gradients, d h3 (pre-activation: dmu Wd1^T + dlv Wd2^T
        # with ReLU'(h3)) and its channel sums (the bias gradient of the layer below) in one launch
        fused = heads_bwd(h3f, RELU, [dmu, dlv], [wdc1, wdc2], [bc1, bc2], L, 1, flat_c=ch[3], prev_bias=b2,
                          dw_params=[wc1, wc2]) if (H // 8, W // 8) == (4, 4) else None
        if fused is not None:
            dh3, (dwc1, dwc2), (dbc1, dbc2), db2 = fused
        else:
            tw1, dwc1 = _grad_target(wc1)
            tw2, dwc2 = _grad_target(wc2)
            ws = _ws(x)
            call("mvk_flatten_wgrad", ptr(h3f), ptr(dmu), ptr(tw1), B, ch[3], L, ptr(ws), ws.numel(), stream_ptr())
            call("mvk_flatten_wgrad", ptr(h3f), ptr(dlv), ptr(tw2), B, ch[3], L, ptr(ws), ws.numel(), stream_ptr())
            dbc1, dbc2 = colsum(dmu, bc1), colsum(dlv, bc2)
            dh3 = gemm(dmu, wdc1, B, Kf, L, tb=True, c_act_src=h3f, c_act=RELU)
            gemm(dlv, wdc2, B, Kf, L, tb=True, c_act_src=h3f, c_act=RELU, out=dh3, accumulate=True)
        dh3 = dh3.view(B, H // 8, W // 8, ch[3])
        # The two inner layers' weight gradients as ONE launch behind both backward-data launches (mvk_conv4s2_wgrad_pair): at the
        # training batch each is a split-K GEMM of 256 workgroups and ~35 us, and the four launches were one dependent chain
        # (the step's last one).  Only where both targets are views of the flat gradient buffer inside deferred_reductions (the
        # pair's slabs live in the arena).
        pair = schedule.scope(x.device) is not None and _is_direct(w1) and _is_direct(w2) and x.device.type == "cuda"
        if not pair:
            dw2 = conv_wgrad(h2, dh3, w2, B, H // 8, W // 8, ch[2], ch[3])
        if fused is None:
            db2 = colsum(dh3.view(-1, ch[3]), b2)
        # each backward-data launch also emits the bias gradient of the layer it lands in (column sums of its output)
        dh2, db1 = conv_up(dh3, wu2, None, B, H // 8, W // 8, ch[2], ch[3], u_act_src=h2, u_act=RELU, out_bias=b1,
                           frag=ctx.frags[1])
        if not pair:
            dw1 = conv_wgrad(h1, dh2, w1, B, H // 4, W // 4, ch[1], ch[2])
        dh1, db0 = conv_up(dh2, wu1, None, B, H // 4, W // 4, ch[1], ch[2], u_act_src=h1, u_act=RELU, out_bias=b0,
                           frag=ctx.frags[0])
        if pair:
            ws = _ws(x)
            call("mvk_conv4s2_wgrad_pair", ptr(h2), ptr(dh3), ptr(_grad_target(w2)[0]), H // 8, W // 8, ch[2], ch[3],
                 ptr(h1), ptr(dh2), ptr(_grad_target(w1)[0]), H // 4, W // 4, ch[1], ch[2], B, ptr(ws), ws.numel(), stream_ptr())
            dw2 = dw1 = None
        dw0 = conv_wgrad(x, dh1, w0, B, H // 2, W // 2, ch[0], ch[1], u_nchw=True)
        dx = None
        if ctx.needs_input_grad[0]:
            raise _lib.MvkError("gradient w.r.t. the encoder input image is not implemented")
        return dx, dw0, db0, dw1, db1, dw2, db2, dwc1, dbc1, dwc2, dbc2


# MVK_TAIL_F16=0: the fused SVHN tail on bf16 pieces (small_up_fwd_bf_kernel) also where the scaled-fp16 chain runs
TAIL_F16 = _lib.tune("MVK_TAIL_F16", "1") != "0"


class SVHNDecoderFn(Function):
    """z[...,L] -> ConvT(4,1,0)+ReLU -> 2x ConvT(4,2,1)+ReLU -> ConvT(4,2,1)+Sigmoid -> [...,C,32,32] NCHW."""

    WAITS_FOR_LOSS = True  # the backward calls schedule.wait_loss before it reads a row gradient (schedule.orders_behind_loss)

    @staticmethod
    def forward(ctx, z, w0, b0, w1, b1, w2, b2, w3, b3, nll_x=None, nll_scale=1.0, nll_weight=1.0):
        """nll_x [B, C, 32, 32] given: the FUSED TAIL — the last layer scores its image against nll_x[row % B] by a
        Normal(nll_scale) likelihood in its epilogue (mvk_conv4s2_small_up_fwd_nll) and the node returns the NLL row sums
        [*z.shape[:-1]] instead of the images; the buffer that would hold the images holds d rows / d pre-activation for the
        backward pass.  The caller checks `svhn_fused_tail_ok` first."""
        _check_nll_weight(nll_x, nll_weight)
        L = w0.shape[0]
        z2 = _c(z.reshape(-1, L))
        n = z2.shape[0]
        C1, C2, C3, C4 = w0.shape[1], w1.shape[1], w2.shape[1], w3.shape[1]
        # [L][C1] unflatten pack; [Cv=C1][Cu=C2]; [Cv=C2][Cu=C3]; [Cv=C3][Cu=C4] — one launch
        wp0, (wd1, wu1), (wd2, wu2), (wd3, _) = pack_weights(
            [(w0, "unflatten"), (w1, True, True), (w2, True, True), (w3, True, False)])
        # scaled-fp16 form of the two 4x4/stride-2 layers (csrc/imgconv.hip NP = 2): every producer on the chain publishes the
        # maximum of what it writes, the consumer scales by it (amax protocol; no pass over a tensor)
        # (from 1024 images: below, the in-kernel conversion of the weights costs what the cheaper product saves — cfg2's decoder
        # batch of 512 measured 0.581 ms per step on bf16 pieces, 0.591 on fp16 pairs)
        f16 = (IMG_F16 and n >= IMG_F16_MIN_ROWS and conv4s2_scaled_ok(n, 4, 4, C2, C1) and conv4s2_scaled_ok(n, 8, 8, C3, C2)
               and all(getattr(t, "mvk_amax", None) is not None for t in (wu1, wu2, wd1, wd2)))
        ctx.f16 = f16
        # rotated step (Rotation): the three weight gradients of w0 / w1 / w2 run at the head of the NEXT step — what they read
        # (z, g1, g2 here; the three gradients in backward; the amax slots) lives in the rotation's persistent buffers
        rot = schedule.rotation(z2.device)
        if rot is not None:
            rot.wait()  # w0 / w1 / w2 (and their packs above) are final behind the head branch
        if not (schedule.ROT_SVHN and rot is not None and f16 and nll_x is not None and schedule.LATE_LEAVES
                and schedule.scope(z2.device) is not None and all(_is_direct(t) for t in (w0, w1, w2))):
            rot = None
        ctx.rot, ctx.rot_mode = rot, schedule.ROT_SVHN
        if schedule.ROT_SVHN != 1:
            rot = None  # mode 2 rotates the first layer's gradient only: nothing of the forward pass needs a fixed address
        rkey = ("svhn_dec", w0.data_ptr(), n)
        if rot is not None:
            z2 = rot.buf(rkey + ("z",), z2.shape).copy_(z2)
        if f16:
            pool = AmaxPool(z2, 6) if rot is None else AmaxPool.__new__(AmaxPool)
            if rot is not None:
                pool.t, pool.i = rot.slots(6), 0
            a1, a2 = pool.take(), pool.take()
            a3 = pool.take() if (TAIL_F16 and nll_x is not None) else None  # bound of g3 for the image layer's scaled form
            # bound of the fused tail's stored gradient: the image layer's backward scales it (small_up_bwd_h_kernel)
            ctx.a_dpre = pool.take() if a3 is not None else None
            ctx.a_g3 = a3
            ctx.bslots = (pool.take(), pool.take())  # the backward pass's two slots: no fill launch there
            g1 = _new((n, 16 * C1), z2) if rot is None else rot.buf(rkey + ("g1",), (n, 16 * C1))
            if L <= 32 and (16 * C1) % 4 == 0:
                call("mvk_gemm_smallk_amax", ptr(z2), ptr(wp0), ptr(g1), n, 16 * C1, L, 0, ptr(b0), C1, RELU, ptr(a1),
                     stream_ptr())
            else:
                gemm(z2, wp0, n, 16 * C1, L, bias=b0, bias_mod=C1, act=RELU, out=g1)
                amax_of(g1, a1)
            g2 = conv_up(g1, wu1, b1, n, 4, 4, C2, C1, RELU, amax=(a1, wu1.mvk_amax, a2),
                         out=None if rot is None else rot.buf(rkey + ("g2",), (n, 8, 8, C2)))  # [n,8,8,C2]
            g3 = conv_up(g2, wu2, b2, n, 8, 8, C3, C2, RELU, amax=(a2, wu2.mvk_amax, a3))  # [n,16,16,C3]
            ctx.wamax = (wd1.mvk_amax, wd2.mvk_amax)
            ctx.gamax = (a1, a2)  # bounds of g1, g2: the V operands of the two weight gradients
        else:
            a3 = None
            g1 = gemm(z2, wp0, n, 16 * C1, L, bias=b0, bias_mod=C1, act=RELU)  # [n,4,4,C1]
            g2 = conv_up(g1, wu1, b1, n, 4, 4, C2, C1, RELU)  # [n,8,8,C2]
            g3 = conv_up(g2, wu2, b2, n, 8, 8, C3, C2, RELU)  # [n,16,16,C3]
        out = _new((n, C4, 32, 32), z2)
        small = bool(_lib.load().mvk_conv4s2_small_up_supported(16, 16, C4, C3))
        ctx.fused = nll_x is not None
        if ctx.fused:
            rows = _new((n,), z2)
            # the stored gradient is pre-multiplied by nll_weight, the weight the rows are expected to enter the loss with
            ctx.nll_weight = float(nll_weight)
            if a3 is not None:  # scaled fp16 pairs under the bound the 64 -> 32 launch published (small_up_fwd_h_kernel), and the
                # maximum of the stored gradient published for the backward
                call("mvk_conv4s2_small_up_fwd_nll_sy", ptr(g3), ptr(w3), ptr(b3), ptr(nll_x), nll_x.shape[0], float(nll_scale),
                     float(nll_weight), ptr(out), ptr(rows), n, 16, 16, C4, C3, SIGMOID, ptr(a3), ptr(ctx.a_dpre), stream_ptr())
            else:
                call("mvk_conv4s2_small_up_fwd_nll_w", ptr(g3), ptr(w3), ptr(b3), ptr(nll_x), nll_x.shape[0], float(nll_scale),
                     float(nll_weight), ptr(out), ptr(rows), n, 16, 16, C4, C3, SIGMOID, stream_ptr())
        elif small:  # per-image MFMA column-matrix kernel (smallconv.hip)
            call("mvk_conv4s2_small_up_fwd", ptr(g3), ptr(w3), ptr(b3), ptr(out), n, 16, 16, C4, C3, SIGMOID,
                 stream_ptr())
        else:
            call("mvk_conv4s2_up_nchw_small", ptr(g3), ptr(w3), ptr(b3), ptr(out), n, 16, 16, C4, C3, SIGMOID,
                 stream_ptr())
        ctx.small = small
        ctx.frags = (wfrag(wd1), wfrag(wd2))
        ctx.save_for_backward(z2, g1, g2, g3, out, wp0, wd1, wd2, wd3, w0, b0, w1, b1, w2, b2, w3, b3)
        _tap("svhn_decoder", w0, g1.view(n, 4, 4, C1), g2, g3)  # NHWC
        ctx.dims = (n, L, C1, C2, C3, C4)
        ctx.z_shape = z.shape
        if ctx.fused:
            return rows.view(*z.shape[:-1])
        return out.view(*z.shape[:-1], C4, 32, 32)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        z2, g1, g2, g3, out, wp0, wd1, wd2, wd3, w0, b0, w1, b1, w2, b2, w3, b3 = ctx.saved_tensors
        n, L, C1, C2, C3, C4 = ctx.dims
        if ctx.fused:  # dout = d loss / d rows [n]; `out` holds nll_weight * d rows / d pre-activation
            c = const_grad(dout)
            if c is not None and c == ctx.nll_weight:
                drows = None  # exactly the weight folded into `out`: no row gradient is read (nor waited for)
            else:
                schedule.wait_loss(dout.device)
                drows = _c(dout).reshape(-1)
                if ctx.nll_weight != 1.0:
                    drows = drows * (1.0 / ctx.nll_weight)
            tw3, dw3 = _grad_target(w3)
            tb3, db3 = _grad_target(b3)
            rot = ctx.rot if (ctx.rot is not None and ctx.rot_mode == 1 and schedule.rotation(z2.device) is ctx.rot) else None
            rkey = ("svhn_dec", w0.data_ptr(), n)
            dg3 = _new((n, 16, 16, C3), z2) if rot is None else rot.buf(rkey + ("dg3",), (n, 16, 16, C3))
            ws = _ws(z2)
            tb2, db2 = _grad_target(b2)
            if ctx.f16:
                a_dg3 = ctx.bslots[0]
                if ctx.a_dpre is not None:  # scaled fp16 pairs: the gradient under the published bound x max |drows|, g3 under its own
                    call("mvk_conv4s2_small_up_bwd_pre_s", ptr(out), ptr(drows), ptr(g3), RELU, ptr(w3), ptr(dg3), ptr(tw3), ptr(tb3),
                         ptr(tb2), ptr(ws), ws.numel(), n, 16, 16, C4, C3, ptr(ctx.a_dpre), ptr(ctx.a_g3), ptr(a_dg3), stream_ptr())
                else:
                    call("mvk_conv4s2_small_up_bwd_pre_y", ptr(out), ptr(drows), ptr(g3), RELU, ptr(w3), ptr(dg3), ptr(tw3), ptr(tb3),
                         ptr(tb2), ptr(ws), ws.numel(), n, 16, 16, C4, C3, ptr(a_dg3), stream_ptr())
                schedule.tail_bwd_done(z2.device)
            else:
                call("mvk_conv4s2_small_up_bwd_pre", ptr(out), ptr(drows), ptr(g3), RELU, ptr(w3), ptr(dg3), ptr(tw3), ptr(tb3),
                     ptr(tb2), ptr(ws), ws.numel(), n, 16, 16, C4, C3, stream_ptr())
        else:
            dout = _c(dout).view(out.shape)
        # last layer: dpre = dout * out(1-out) applied while loading
        if ctx.fused:
            pass
        elif ctx.small:  # backward-data + backward-weight + bias gradient in ONE pass over dout / out / g3
            tw3, dw3 = _grad_target(w3)
            tb3, db3 = _grad_target(b3)
            dg3 = _new((n, 16, 16, C3), z2)
            ws = _ws(z2)
            tb2, db2 = _grad_target(b2)  # bias gradient of the layer below = channel sums of dg3: fused
            call("mvk_conv4s2_small_up_bwd", ptr(dout), ptr(out), SIGMOID, ptr(g3), RELU, ptr(w3), ptr(dg3), ptr(tw3),
                 ptr(tb3), ptr(tb2), ptr(ws), ws.numel(), n, 16, 16, C4, C3, stream_ptr())
        else:
            dw3 = conv_wgrad(dout, g3, w3, n, 16, 16, C4, C3, u_nchw=True, u_act_src=out, u_act=SIGMOID)
            tb3, db3 = _grad_target(b3)
            ws = _ws(dout)
            call("mvk_nchw_channel_sum_acc", ptr(dout), ptr(out), SIGMOID, ptr(tb3), n, C4, 32 * 32, ptr(ws), ws.numel(),
                 stream_ptr())
            dg3 = conv_down(dout, wd3, None, n, 16, 16, C4, C3, NONE, u_nchw=True, u_act_src=out, u_act=SIGMOID,
                            v_act_src=g3, v_act=RELU)
        am2 = am1 = wam2 = wam1 = None
        if ctx.f16:  # the bound of dg3 came with the fused-tail backward; without it the first launch stays on bf16 pieces
            if not ctx.fused:
                a_dg3 = None
            a_dg2 = ctx.bslots[1]
            am2 = (a_dg3, ctx.wamax[1] if a_dg3 is not None else None, a_dg2)
            am1 = (a_dg2, ctx.wamax[0], None)
            wam2, wam1 = (a_dg3, ctx.gamax[1]), (a_dg2, ctx.gamax[0])  # (max |U|, max |V|) of the two weight gradients
        if ctx.f16 and wam1 is not None and schedule.LATE_LEAVES and schedule.scope(z2.device) is not None:
            # register-stationary weight gradients are this step's late leaves (what an MLP encoder's backward asks: heads_bwd_mlp;
            # a rotated step decides the same way, so that it launches exactly the kernels of the unrotated one)
            schedule.big_late_leaves(z2.device)
        rot = ctx.rot if (ctx.fused and ctx.rot is not None and schedule.rotation(z2.device) is ctx.rot) else None
        rot0 = rot if (rot is not None and ctx.rot_mode == 2) else None  # mode 2: only the first layer's weight gradient
        if rot0 is not None:
            rot = None
        late = schedule.late_leaves(z2.device, dg3, g2, g1, z2)
        if not late.on:
            rot = rot0 = None
            dw2 = conv_wgrad(dg3, g2, w2, n, 8, 8, C3, C2, amax=wam2)
        if not ctx.small and not ctx.fused:
            db2 = colsum(dg3.view(-1, C3), b2)
        dg2, db1 = conv_down(dg3, wd2, None, n, 8, 8, C3, C2, NONE, v_act_src=g2, v_act=RELU, out_bias=b1,
                             frag=ctx.frags[1], amax=am2, out=None if rot is None else rot.buf(rkey + ("dg2",), (n, 8, 8, C2)))
        if not late.on:
            dw1 = conv_wgrad(dg2, g1, w1, n, 4, 4, C2, C1, amax=wam1)
        rany = rot if rot is not None else rot0
        dg1, db0 = conv_down(dg2, wd1, None, n, 4, 4, C2, C1, NONE, v_act_src=g1, v_act=RELU, out_bias=b0, frag=ctx.frags[0],
                             amax=am1, out=None if rany is None else rany.buf(("svhn_dec", w0.data_ptr(), n, "dg1"), (n, 4, 4, C1)))
        dg1f = dg1.view(n, 16 * C1)
        tw0, dw0 = _grad_target(w0)
        dz = None
        if rot is not None:  # rotated step: the three weight gradients are the head of the next step (Rotation.begin_step)
            if ctx.needs_input_grad[0]:
                dz = _svhn_dz(dg1f, wp0, n, L, C1).view(ctx.z_shape)

            def leaves():
                conv_wgrad(dg3, g2, w2, n, 8, 8, C3, C2, amax=wam2)
                conv_wgrad(dg2, g1, w1, n, 4, 4, C2, C1, amax=wam1)
                wsl = _ws(z2)
                call("mvk_unflatten_wgrad", ptr(z2), ptr(dg1f), ptr(_grad_target(w0)[0]), n, L, C1, ptr(wsl), wsl.numel(),
                     stream_ptr())

            def prepare(r):  # behind the update of w0 / w1 / w2: the packs the next forward pass asks for
                jobs = [(w0, "unflatten"), (w1, True, True), (w2, True, True), (w3, True, False)]
                for j, o in zip(jobs, _pack_launch(jobs, am=r.slots(len(jobs)))):
                    r.cache[_job_key(j)] = o

            rot.push(leaves, (w0, w1, w2), prepare)
            return dz, None, db0, None, db1, None, db2, dw3, db3, None, None, None
        if late.on:  # the backward-data chain first, then the weight gradients beside whatever follows it
            if ctx.needs_input_grad[0]:
                dz = _svhn_dz(dg1f, wp0, n, L, C1).view(ctx.z_shape)
            dg2.record_stream(schedule._side_stream(z2.device, 30))
            dg1.record_stream(schedule._side_stream(z2.device, 30))
            with late:
                dw2 = conv_wgrad(dg3, g2, w2, n, 8, 8, C3, C2, amax=wam2)
                dw1 = conv_wgrad(dg2, g1, w1, n, 4, 4, C2, C1, amax=wam1)
                if rot0 is not None:
                    # mode 2: the first layer's weight gradient (a split-K GEMM over z and dg1) is the head of the next step; z is
                    # copied to a buffer with a fixed address HERE, on the late-leaf stream (off the backward chain)
                    zp = rot0.buf(("svhn_dec", w0.data_ptr(), n, "z"), z2.shape).copy_(z2)

                    def leaf0():
                        wsl = _ws(zp)
                        call("mvk_unflatten_wgrad", ptr(zp), ptr(dg1f), ptr(_grad_target(w0)[0]), n, L, C1, ptr(wsl), wsl.numel(),
                             stream_ptr())

                    def prepare0(r):  # behind the update of w0: its pack for the next forward pass
                        job = (w0, "unflatten")
                        r.cache[_job_key(job)] = _pack_launch([job])[0]

                    rot0.push(leaf0, (w0,), prepare0)
                else:
                    ws = _ws(z2)
                    call("mvk_unflatten_wgrad", ptr(z2), ptr(dg1f), ptr(tw0), n, L, C1, ptr(ws), ws.numel(), stream_ptr())
            if dw0 is not None or dw1 is not None or dw2 is not None:  # a gradient autograd itself accumulates: join now
                torch.cuda.current_stream(z2.device).wait_stream(schedule._side_stream(z2.device, 30))
            return dz, dw0, db0, dw1, db1, dw2, db2, dw3, db3, None, None, None
        ws = _ws(z2)
        call("mvk_unflatten_wgrad", ptr(z2), ptr(dg1f), ptr(tw0), n, L, C1, ptr(ws), ws.numel(), stream_ptr())
        if ctx.needs_input_grad[0]:
            dz = _svhn_dz(dg1f, wp0, n, L, C1).view(ctx.z_shape)
        return dz, dw0, db0, dw1, db1, dw2, db2, dw3, db3, None, None, None


def _svhn_dz(dg1f, wp0, n, L, C1):
    """d z = d g1 W0^T of the SVHN decoder's first layer (wp0: the [L][16 C1] unflatten pack)."""
    return gemm(dg1f, wp0, n, L, 16 * C1, tb=True)


def svhn_fused_tail_ok(C4, C3):
    """The fused decoder tail of SVHNDecoderFn exists for this image layer (mvk_conv4s2_small_up_nll_supported)."""
    return bool(_lib.load().mvk_conv4s2_small_up_nll_supported(16, 16, C4, C3))


# =====================================================================================================
# ResNet stacks (models/nn/mmnist.py:214-366, models/nn/cub.py:144-293), NHWC activations
# =====================================================================================================
# =====================================================================================================
# PolyMNIST convolutional networks (models/nn/mmnist.py:36-206): 3x3 / stride 2 / pad 1 on 28 <-> 14 <-> 7 <-> 4 (csrc/polyconv.hip)
# =====================================================================================================
def conv3s2_ok(H, W, Cu, Cv):
    return bool(_lib.load().mvk_conv3s2_ok(int(H), int(W), int(Cu), int(Cv)))


def _conv3s2_check(H, W, Cu, Cv):
    if not conv3s2_ok(H, W, Cu, Cv):
        raise _lib.MvkError(f"no 3x3 / stride-2 kernel for a {H}x{W} map with channels ({Cu}, {Cv}): mvk_conv3s2_ok")


def conv3s2_down(U, wref, bias, n, H, W, Cu, Cv, act=NONE, u_nchw=False, v_act_src=None, v_act=NONE, out=None):
    """V [n, h, w, Cv] = act(conv(U) + bias) (* v_act'(v_act_src)); U [n, H, W, Cu], or the image [n, Cu, H, W] (u_nchw).  wref: the
    [Cv, Cu, 3, 3] parameter itself.  Conv2d forward, ConvTranspose2d backward-data."""
    _conv3s2_check(H, W, Cu, Cv)
    V = out if out is not None else _new((n, (H + 1) // 2, (W + 1) // 2, Cv), U)
    call("mvk_conv3s2_down", ptr(U), ptr(wref), ptr(bias), ptr(V), n, H, W, Cu, Cv, act, int(u_nchw), ptr(v_act_src), v_act,
         stream_ptr())
    return V


def conv3s2_up(V, wref, bias, n, H, W, Cu, Cv, act=NONE, u_nchw=False, u_act_src=None, u_act=NONE, out=None):
    """U [n, H, W, Cu] (u_nchw: [n, Cu, H, W]) = act(convT(V) + bias) (* u_act'(u_act_src)); V [n, (H+1)//2, (W+1)//2, Cv].  H, W are
    the output's: output_padding = H - (2 h - 1).  ConvTranspose2d forward, Conv2d backward-data."""
    _conv3s2_check(H, W, Cu, Cv)
    U = out if out is not None else _new((n, Cu, H, W) if u_nchw else (n, H, W, Cu), V)
    call("mvk_conv3s2_up", ptr(V), ptr(wref), ptr(bias), ptr(U), n, H, W, Cu, Cv, act, int(u_nchw), ptr(u_act_src), u_act,
         stream_ptr())
    return U


def conv3s2_wgrad(U, V, wparam, bparam, n, H, W, Cu, Cv, u_nchw=False, db_side=1):
    """wparam.grad += sum U(gathered) V, bparam.grad += the channel sums of V (db_side 1: Conv2d) or of U (db_side 2:
    ConvTranspose2d), straight into the flat gradient buffer where the trainer provides one -> (grad for w, grad for b)."""
    _conv3s2_check(H, W, Cu, Cv)
    dw, rw = _grad_target(wparam)
    db, rb = _grad_target(bparam) if bparam is not None else (None, None)
    ws = _ws(V)
    call("mvk_conv3s2_wgrad", ptr(U), ptr(V), ptr(dw), ptr(db), db_side if bparam is not None else 0, n, H, W, Cu, Cv,
         int(u_nchw), 1, ptr(ws), ws.numel(), stream_ptr())
    return rw, rb


POLYCONV_CHANS = (3, 32, 64, 128)
POLYCONV_MAPS = (28, 14, 7, 4)


def _polyconv_check(x_shape, ws, transposed):
    c = POLYCONV_CHANS
    want = [((c[i + 1], c[i], 3, 3), (c[i + 1],)) for i in range(3)]
    if transposed:
        want = [((c[3 - i], c[2 - i], 3, 3), (c[2 - i],)) for i in range(3)]
    got = [(tuple(ws[2 * i].shape), tuple(ws[2 * i + 1].shape)) for i in range(3)]
    if got != want:
        raise _lib.MvkError(f"PolyMNIST convolutional trunk: parameter shapes {got}, expected {want}")
    if tuple(x_shape[1:]) != ((4, 4, 128) if transposed else (3, 28, 28)):
        raise _lib.MvkError(f"PolyMNIST convolutional trunk: input {tuple(x_shape)}")


def polyenc_forward(x, w0, b0, w1, b1, w2, b2):
    """The no-grad encoder trunk in one launch (mvk_polyenc_fwd): x [n, 3, 28, 28] -> h3 [n, 4, 4, 128] (NHWC, after its ReLU)."""
    x = _c(x)
    _polyconv_check(x.shape, (w0, b0, w1, b1, w2, b2), False)
    h3 = _new((x.shape[0], 4, 4, 128), x)
    call("mvk_polyenc_fwd", ptr(x), x.shape[0], ptr(_c(w0)), ptr(_c(b0)), ptr(_c(w1)), ptr(_c(b1)), ptr(_c(w2)), ptr(_c(b2)),
         ptr(h3), stream_ptr())
    return h3


def polydec_forward(h0, w0, b0, w1, b1, w2, b2):
    """The no-grad decoder trunk in one launch (mvk_polydec_fwd): h0 [n, 4, 4, 128] (NHWC) -> [n, 3, 28, 28]."""
    h0 = _c(h0)
    _polyconv_check(h0.shape, (w0, b0, w1, b1, w2, b2), True)
    out = _new((h0.shape[0], 3, 28, 28), h0)
    call("mvk_polydec_fwd", ptr(h0), h0.shape[0], ptr(_c(w0)), ptr(_c(b0)), ptr(_c(w1)), ptr(_c(b1)), ptr(_c(w2)), ptr(_c(b2)),
         ptr(out), stream_ptr())
    return out


class PolyConvEncoderFn(Function):
    """x [n, 3, 28, 28] NCHW -> 3 x (Conv 3/2/1 + ReLU) -> h3 [n, 4, 4, 128] NHWC (the heads are the caller's).  Without a
    gradient to keep anything for, the whole trunk is one launch."""

    @classmethod
    def run(cls, x, *params):
        """`apply`, or the fused trunk under torch.no_grad() (grad mode is always off INSIDE forward: only the caller can look)."""
        return cls.apply(x, *params) if torch.is_grad_enabled() else polyenc_forward(x, *params)

    @staticmethod
    def forward(ctx, x, w0, b0, w1, b1, w2, b2):
        x = _c(x)
        params = (w0, b0, w1, b1, w2, b2)
        _polyconv_check(x.shape, params, False)
        if not any(ctx.needs_input_grad):  # nothing is kept for a backward pass
            return polyenc_forward(x, *params)
        n = x.shape[0]
        c, m = POLYCONV_CHANS, POLYCONV_MAPS
        h1 = conv3s2_down(x, w0, b0, n, m[0], m[0], c[0], c[1], RELU, u_nchw=True)
        h2 = conv3s2_down(h1, w1, b1, n, m[1], m[1], c[1], c[2], RELU)
        h3 = conv3s2_down(h2, w2, b2, n, m[2], m[2], c[2], c[3], RELU)
        ctx.save_for_backward(x, h1, h2, h3, *params)
        _tap("polyconv_encoder", w0, h1, h2, h3)  # NHWC
        return h3

    @staticmethod
    @once_differentiable
    def backward(ctx, dh3):
        x, h1, h2, h3, w0, b0, w1, b1, w2, b2 = ctx.saved_tensors
        if ctx.needs_input_grad[0]:
            raise _lib.MvkError("gradient w.r.t. the encoder input image is not implemented")
        n = x.shape[0]
        c, m = POLYCONV_CHANS, POLYCONV_MAPS
        schedule.defer_flush_sibling(x.device, node_params=(w0, b0, w1, b1, w2, b2))
        dp3 = torch.empty_like(h3)
        call("mvk_act_bwd_scaled", ptr(_c(dh3)), 1.0, ptr(h3), RELU, ptr(dp3), h3.numel(), stream_ptr())
        # each backward-data launch is followed by the weight gradient of the layer below it
        dw2, db2 = conv3s2_wgrad(h2, dp3, w2, b2, n, m[2], m[2], c[2], c[3])
        dp2 = conv3s2_up(dp3, w2, None, n, m[2], m[2], c[2], c[3], u_act_src=h2, u_act=RELU)
        dw1, db1 = conv3s2_wgrad(h1, dp2, w1, b1, n, m[1], m[1], c[1], c[2])
        dp1 = conv3s2_up(dp2, w1, None, n, m[1], m[1], c[1], c[2], u_act_src=h1, u_act=RELU)
        dw0, db0 = conv3s2_wgrad(x, dp1, w0, b0, n, m[0], m[0], c[0], c[1], u_nchw=True)
        return None, dw0, db0, dw1, db1, dw2, db2


class PolyConvDecoderFn(Function):
    """h0 [n, 4, 4, 128] NHWC (after the ReLU of the linear layer) -> ConvT(128, 64) + ReLU -> ConvT(64, 32, op 1) + ReLU ->
    ConvT(32, 3, op 1) -> [n, 3, 28, 28] NCHW.  Its backward reads the images' gradient only (there is no fused likelihood
    tail, so no row gradient of the loss assembly is read and nothing has to wait for it)."""

    @classmethod
    def run(cls, h0, *params):
        """`apply`, or the fused trunk under torch.no_grad()."""
        return cls.apply(h0, *params) if torch.is_grad_enabled() else polydec_forward(h0, *params)

    @staticmethod
    def forward(ctx, h0, w0, b0, w1, b1, w2, b2):
        h0 = _c(h0)
        params = (w0, b0, w1, b1, w2, b2)
        _polyconv_check(h0.shape, params, True)
        if not any(ctx.needs_input_grad):  # nothing is kept for a backward pass
            return polydec_forward(h0, *params)
        n = h0.shape[0]
        c, m = POLYCONV_CHANS, POLYCONV_MAPS
        d1 = conv3s2_up(h0, w0, b0, n, m[2], m[2], c[2], c[3], RELU)
        d2 = conv3s2_up(d1, w1, b1, n, m[1], m[1], c[1], c[2], RELU)
        out = conv3s2_up(d2, w2, b2, n, m[0], m[0], c[0], c[1], NONE, u_nchw=True)
        ctx.save_for_backward(h0, d1, d2, *params)
        _tap("polyconv_decoder", w0, d1, d2)  # NHWC
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        h0, d1, d2, w0, b0, w1, b1, w2, b2 = ctx.saved_tensors
        n = h0.shape[0]
        c, m = POLYCONV_CHANS, POLYCONV_MAPS
        dout = _c(dout)
        # the image layer has no activation: dout is its pre-activation gradient
        dw2, db2 = conv3s2_wgrad(dout, d2, w2, b2, n, m[0], m[0], c[0], c[1], u_nchw=True, db_side=2)
        dp2 = conv3s2_down(dout, w2, None, n, m[0], m[0], c[0], c[1], u_nchw=True, v_act_src=d2, v_act=RELU)
        dw1, db1 = conv3s2_wgrad(dp2, d1, w1, b1, n, m[1], m[1], c[1], c[2], db_side=2)
        dp1 = conv3s2_down(dp2, w1, None, n, m[1], m[1], c[1], c[2], v_act_src=d1, v_act=RELU)
        dw0, db0 = conv3s2_wgrad(dp1, h0, w0, b0, n, m[2], m[2], c[2], c[3], db_side=2)
        dh0 = conv3s2_down(dp1, w0, None, n, m[2], m[2], c[2], c[3]) if ctx.needs_input_grad[0] else None
        return dh0, dw0, db0, dw1, db1, dw2, db2


class PolyConvHeadsFn(Function):
    """The two Conv2d(128, L, 4, 2, 0) heads on the 4x4 map (mmnist.py:101-102): a window that covers the whole map is a linear layer
    over the map flattened in (c, h, w) order, which is the parameter's own layout [L, 128 * 16].  flat [n, 2048] -> (mu, lv) [n, L];
    the weight gradients land in the 4-d parameters' own gradient buffers."""

    @staticmethod
    def forward(ctx, flat, w_mu, b_mu, w_lv, b_lv):
        flat = _c(flat)
        L, Kf = w_mu.shape[0], flat.shape[1]
        if w_mu[0].numel() != Kf or w_lv.shape != w_mu.shape:
            raise _lib.MvkError(f"heads {tuple(w_mu.shape)} / {tuple(w_lv.shape)} on a flattened map of {Kf}")
        mu = linear_fwd(flat, w_mu.detach().view(L, Kf), b_mu, NONE)
        lv = linear_fwd(flat, w_lv.detach().view(L, Kf), b_lv, NONE)
        ctx.save_for_backward(flat, w_mu, b_mu, w_lv, b_lv)
        return mu, lv

    @staticmethod
    @once_differentiable
    def backward(ctx, dmu, dlv):
        flat, w_mu, b_mu, w_lv, b_lv = ctx.saved_tensors
        L, Kf = w_mu.shape[0], flat.shape[1]
        dys, w2 = [_c(dmu), _c(dlv)], [w_mu.detach().view(L, Kf), w_lv.detach().view(L, Kf)]
        need_dx = ctx.needs_input_grad[0]
        fused = heads_bwd(flat, NONE, dys, w2, [b_mu, b_lv], 1, Kf, want_dx=need_dx, dw_params=[w_mu, w_lv]) if need_dx else None
        if fused is not None:
            dflat, (dw_mu, dw_lv), (db_mu, db_lv), _ = fused
            return dflat, dw_mu, db_mu, dw_lv, db_lv
        dw_mu, db_mu = linear_bwd_weight(dys[0], flat, w_mu, b_mu)
        dw_lv, db_lv = linear_bwd_weight(dys[1], flat, w_lv, b_lv)
        dflat = None
        if need_dx:
            dflat = linear_bwd_data(dys[0], w2[0])
            linear_bwd_data(dys[1], w2[1], out=dflat, accumulate=True)
        return dflat, dw_mu, db_mu, dw_lv, db_lv


def _rs_conv(pool, X, xam, wpack, bias, n, H, W, Cin, Cout, **kw):
    """One 3x3 convolution of a ResNet stack -> (result of conv3x3 / conv3x3_f, amax slot of Y or None).  With a pool (the
    scaled-fp16 form is on) and a covered shape the launch is mvk_conv3x3_s: xam = the slot that bounds max |X| (None: it is
    computed here), the weight's bound came with its pack, and max |Y| lands in a fresh slot for the consumer of Y."""
    w_am = getattr(wpack, "mvk_amax", None)
    if (pool is not None and w_am is not None and kw.get("act", NONE) != SIGMOID and kw.get("y_src_act", NONE) != SIGMOID
            and conv3x3_scaled_ok(n, H, W, Cin, Cout)):
        xam = xam if xam is not None else amax_of(X, pool.take())
        yam = pool.take()
        return conv3x3_s(X, wpack, bias, n, H, W, Cin, Cout, xam, w_am, yam, **kw), yam
    if (pool is not None and w_am is not None and Cin == 256 and kw.get("res") is None
            and kw.get("act", NONE) != SIGMOID and kw.get("y_src_act", NONE) != SIGMOID and conv3x3_scaled_ok(n, H, W, 128, Cout)):
        # 256 input channels: more weights than a register-stationary wave holds — two launches over 128-channel slices
        xam = xam if xam is not None else amax_of(X, pool.take())
        yam = pool.take()
        kw2 = {k: v for k, v in kw.items() if k not in ("res", "res_alpha")}
        return conv3x3_s_split(X, wpack, bias, n, H, W, Cin, Cout, xam, w_am, yam, **kw2), yam
    if kw.get("x_act", NONE) != NONE or kw.get("pre_scale", 1.0) != 1.0:
        return conv3x3_f(X, wpack, bias, n, H, W, Cin, Cout, **kw), None
    kw.pop("x_act", None)
    kw.pop("pre_scale", None)
    if pool is not None and Cin <= 4 and Cout % 4 == 0 and kw.get("res") is None:
        # an image on the input side (conv_img of an encoder, the backward-data pass of a decoder's conv_img): the direct
        # kernel publishes max |Y| itself — the stack behind it takes the scaled-fp16 form without an amax pass over Y
        yam = pool.take()
        try:
            return conv3x3(X, wpack, bias, n, H, W, Cin, Cout, y_amax=yam, **kw), yam
        except _lib.MvkError:
            pass  # shape not covered by the direct kernel (MVK_EINVAL): the plain launch below
    return conv3x3(X, wpack, bias, n, H, W, Cin, Cout, **kw), None


def _rs_wgrad(pool, X, xam, dY, dyam, wparam, bparam, n, H, W, Cin, Cout, x_act=NONE, dy_scale=1.0, fused=False):
    """Weight (and bias) gradient of one 3x3 convolution of a ResNet stack -> (dW ref, db ref or None).  With a pool and a
    covered shape: mvk_conv3x3_wgrad_s (xam / dyam = slots bounding max |X| / max |dY|, computed here when unknown); else the
    bf16-piece launch (fused: bias gradient, x_act and dy_scale in it) or the plain one + a column-sum pass."""
    if pool is not None and conv3x3_wgrad_scaled_ok(n, H, W, Cin, Cout):
        xam = xam if xam is not None else amax_of(X, pool.take())
        dyam = dyam if dyam is not None else amax_of(dY, pool.take())
        return conv3x3_wgrad_s(X, dY, wparam, bparam, n, H, W, Cin, Cout, xam, dyam, x_act=x_act, dy_scale=dy_scale)
    if fused:
        return conv3x3_wgrad_f(X, dY, wparam, bparam, n, H, W, Cin, Cout, x_act=x_act, dy_scale=dy_scale)
    if x_act != NONE or dy_scale != 1.0:
        raise _lib.MvkError("_rs_wgrad: x_act / dy_scale need the fused launch")
    rw = conv3x3_wgrad(X, dY, wparam, n, H, W, Cin, Cout)
    return rw, (colsum(dY.view(-1, Cout), bparam) if bparam is not None else None)


class ResnetStackFn(Function):
    """x [n,H,W,C] NHWC -> a static program of layers -> y NHWC, one autograd node.

    program: list of tuples (static Python data; parameter references are indices into `params`)
      ("conv", iw, ib, act)                      3x3/1/1 convolution (+ bias, + activation)
      ("block", order, iw1, ib1, iw2, ib2, isc)  ResnetBlock; order "post": xs + 0.1*lrelu(conv2(lrelu(conv1(x))))
                                                 (mmnist.py:229-246), "pre": xs + 0.1*conv2(lrelu(conv1(lrelu(x))))
                                                 (cub.py:274-280); isc = 1x1 shortcut weight index or None
      ("pool",)                                  AvgPool2d(3, 2, 1)
      ("up",)                                    Upsample(scale_factor=2), nearest
      ("act", code)                              elementwise activation (cub.py: fc(actvn(out)), conv_img(actvn(out)))
    """

    @staticmethod
    def forward(ctx, x, program, *params):
        x = _c(x)
        n, H, W, C = x.shape
        tape = []  # per layer: what backward needs
        packs = {}
        jobs, order = [], []
        for op in program:
            idxs = [op[1]] if op[0] == "conv" else ([op[2], op[4]] if op[0] == "block" else [])
            for i in idxs:
                if i not in packs:
                    packs[i] = None
                    jobs.append((params[i], "c3", True, True))
                    order.append(i)
        for i0 in range(0, len(jobs), PACK_MAX):
            for i, pk in zip(order[i0:i0 + PACK_MAX], pack_weights(jobs[i0:i0 + PACK_MAX])):
                packs[i] = pk
        h = x
        sites = []  # sign sources of the activation sites in the reference's evaluation order (test hook, see TAPS)
        # scaled-fp16 form: ham = the slot that bounds max |h| (None: unknown, computed on demand)
        pool = AmaxPool(x, 4 * len(program) + 4) if C3_F16 else None
        ham = None
        for op in program:
            if op[0] == "conv":
                _, iw, ib, act = op
                Cout = params[iw].shape[0]
                y, yam = _rs_conv(pool, h, ham, packs[iw][0], params[ib] if ib is not None else None, n, H, W, C, Cout, act=act)
                tape.append((h, y, (H, W, C, Cout), ham))
                if act != NONE:
                    sites.append(y)
                h, C, ham = y, Cout, yam
            elif op[0] == "block":
                _, order_, iw1, ib1, iw2, ib2, isc = op
                Chid, Cout = params[iw1].shape[0], params[iw2].shape[0]
                b1 = params[ib1] if ib1 is not None else None
                b2 = params[ib2] if ib2 is not None else None
                if pool is not None and ham is None and conv3x3_scaled_ok(n, H, W, C, Chid):
                    ham = amax_of(h, pool.take())  # once: conv1 now, the weight gradient of conv1 in the backward pass
                # fused forms (register-stationary kernels): the leading LeakyReLU of a pre-activation block is applied while
                # conv1 stages its input (a0 is never written) and the backward pass folds the 0.1 and the bias gradients
                fused = (conv3x3_fused_ok(n, H, W, C, Chid) and conv3x3_fused_ok(n, H, W, Chid, Cout)
                         and conv3x3_fused_ok(n, H, W, Cout, Chid))  # conv1, conv2 and conv2's backward-data launch
                oam = y2am = None
                out = None
                if order_ == "post":
                    a0 = h
                    a1, a1am = _rs_conv(pool, a0, ham, packs[iw1][0], b1, n, H, W, C, Chid, act=LEAKY)
                    w2am = getattr(packs[iw2][0], "mvk_amax", None)
                    if pool is not None and a1am is not None and w2am is not None and conv3x3_scaled_ok(n, H, W, Chid, Cout):
                        # conv2, its LeakyReLU and the block's sum in one launch; y2 (the backward pass needs its signs) is the
                        # launch's second store, max |out| its published bound
                        xs = h if isc is None else linear_fwd(h.view(-1, C), params[isc].view(Cout, C), None, NONE).view(n, H, W, Cout)
                        oam = pool.take()
                        out, y2 = conv3x3_s2(a1, packs[iw2][0], b2, n, H, W, Chid, Cout, a1am, w2am, oam, LEAKY, xs, 0.1)
                    else:
                        y2, y2am = _rs_conv(pool, a1, a1am, packs[iw2][0], b2, n, H, W, Chid, Cout, act=LEAKY)
                elif fused:
                    a0 = None
                    a1, a1am = _rs_conv(pool, h, ham, packs[iw1][0], b1, n, H, W, C, Chid, act=LEAKY, x_act=LEAKY)
                    y2 = None
                else:
                    a0 = axpby(h, 1.0, None, 0.0, act=LEAKY)
                    a1, a1am = _rs_conv(pool, a0, ham, packs[iw1][0], b1, n, H, W, C, Chid, act=LEAKY)
                    y2 = None  # the block's sum is formed in conv2's epilogue; backward does not need conv2's output
                if out is None:
                    xs = h if isc is None else linear_fwd(h.view(-1, C), params[isc].view(Cout, C), None, NONE).view(n, H, W, Cout)
                if out is not None:
                    pass
                elif y2 is None:
                    out, oam = _rs_conv(pool, a1, a1am, packs[iw2][0], b2, n, H, W, Chid, Cout, act=NONE, res=xs, res_alpha=0.1)
                else:
                    out = axpby(xs, 1.0, y2, 0.1)
                    if isc is None and ham is not None and y2am is not None:
                        oam = torch.add(ham, y2am, alpha=0.1)  # |xs + 0.1 y2| <= max |xs| + 0.1 max |y2|: no pass over `out`
                tape.append((h, a0, a1, y2, (H, W, C, Chid, Cout), fused, ham, a1am))
                sites += [a1, y2] if order_ == "post" else [h, a1]
                h, C, ham = out, Cout, oam
            elif op[0] == "pool":
                y = avgpool(h, n, H, W, C)  # an average, a copy, a (leaky) ReLU: max |h| still bounds the result
                tape.append((H, W, C))
                h, H, W = y, (H + 1) // 2, (W + 1) // 2
            elif op[0] == "up":
                y = upsample2(h, n, H, W, C)
                tape.append((H, W, C))
                h, H, W = y, 2 * H, 2 * W
            elif op[0] == "act":
                y = axpby(h, 1.0, None, 0.0, act=op[1])
                tape.append((y,))
                sites.append(y)
                h = y
                ham = ham if op[1] in (LEAKY, RELU) else None
            else:
                raise _lib.MvkError(f"unknown ResNet op {op[0]!r}")
        ctx.tape, ctx.packs, ctx.program, ctx.n = tape, packs, program, n
        ctx.save_for_backward(*params)
        _tap("resnet_stack", params[0] if params else None, *sites)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        params = ctx.saved_tensors
        n, packs = ctx.n, ctx.packs
        grads = [None] * len(params)
        g = _c(dout)
        need_dx = ctx.needs_input_grad[0]
        pool = AmaxPool(g, 4 * len(ctx.program) + 4) if C3_F16 else None
        gam = None  # the slot that bounds max |g| (None: unknown)
        for li in range(len(ctx.program) - 1, -1, -1):
            op, rec = ctx.program[li], ctx.tape[li]
            first = li == 0
            if op[0] == "conv":
                _, iw, ib, act = op
                xin, y, (H, W, C, Cout), xam = rec
                dpre = g
                if act != NONE:
                    dpre = g.clone() if g is dout else g
                    call("mvk_act_bwd", ptr(dpre), ptr(y), dpre.numel(), act, stream_ptr())
                gam = gam if act in (NONE, LEAKY, RELU) else None  # |dpre| <= |g|: these derivatives are at most 1
                grads[iw], gb = _rs_wgrad(pool, xin, xam, dpre, gam, params[iw], params[ib] if ib is not None else None, n, H, W,
                                          C, Cout)
                if ib is not None:
                    grads[ib] = gb
                if not first or need_dx:
                    g, gam = _rs_conv(pool, dpre, gam, packs[iw][1], None, n, H, W, Cout, C)
            elif op[0] == "block":
                _, order_, iw1, ib1, iw2, ib2, isc = op
                xin, a0, a1, y2, (H, W, C, Chid, Cout), fused, xam, a1am = rec
                gout = g
                if gam is None and pool is not None:
                    gam = amax_of(gout, pool.take())  # three launches below take it
                if fused and order_ == "pre":
                    # d2 = 0.1 * gout is never formed: the 0.1 rides on the weight / bias gradient and on the backward-data
                    # sum; a0 = lrelu(x) is re-applied while the weight-gradient kernel stages x
                    grads[iw2], gb2 = _rs_wgrad(pool, a1, a1am, gout, gam, params[iw2], params[ib2] if ib2 is not None else None,
                                                n, H, W, Chid, Cout, dy_scale=0.1, fused=True)
                    if ib2 is not None:
                        grads[ib2] = gb2
                    if ib1 is not None:
                        (d1, grads[ib1]), d1am = _rs_conv(pool, gout, gam, packs[iw2][1], None, n, H, W, Cout, Chid, y_act_src=a1,
                                                          y_src_act=LEAKY, out_bias=params[ib1], pre_scale=0.1)
                    else:
                        d1, d1am = _rs_conv(pool, gout, gam, packs[iw2][1], None, n, H, W, Cout, Chid, y_act_src=a1,
                                            y_src_act=LEAKY, pre_scale=0.1)
                    grads[iw1], _ = _rs_wgrad(pool, xin, xam, d1, d1am, params[iw1], None, n, H, W, C, Chid, x_act=LEAKY, fused=True)
                    a0 = xin  # sign(lrelu(x)) == sign(x): the mask source of dx below
                else:
                    if order_ == "post":  # gradient w.r.t. conv2's pre-activation: 0.1 * gout * lrelu'(y2), one pass
                        d2 = _new(gout.shape, gout)
                        call("mvk_act_bwd_scaled", ptr(gout), 0.1, ptr(y2), LEAKY, ptr(d2), d2.numel(), stream_ptr())
                    else:
                        d2 = axpby(gout, 0.1, None, 0.0)  # gradient w.r.t. y2 (max |gout| bounds it)
                    grads[iw2], gb2 = _rs_wgrad(pool, a1, a1am, d2, gam, params[iw2], params[ib2] if ib2 is not None else None, n, H,
                                                W, Chid, Cout, fused=fused)  # fused: bias gradient with the weight gradient
                    if ib2 is not None:
                        grads[ib2] = gb2
                    # backward data of conv2 with lrelu'(a1) fused; its channel sums are conv1's bias gradient
                    if ib1 is not None:
                        (d1, grads[ib1]), d1am = _rs_conv(pool, d2, gam, packs[iw2][1], None, n, H, W, Cout, Chid, y_act_src=a1,
                                                          y_src_act=LEAKY, out_bias=params[ib1])
                    else:
                        d1, d1am = _rs_conv(pool, d2, gam, packs[iw2][1], None, n, H, W, Cout, Chid, y_act_src=a1, y_src_act=LEAKY)
                    grads[iw1], _ = _rs_wgrad(pool, a0, xam, d1, d1am, params[iw1], None, n, H, W, C, Chid)
                if isc is not None:
                    grads[isc], _ = linear_bwd_weight(gout.view(-1, Cout), xin.view(-1, C), params[isc].view(Cout, C), None)
                    if grads[isc] is not None:
                        grads[isc] = grads[isc].view(params[isc].shape)
                if not first or need_dx:
                    # the shortcut's gradient first, the convolution path adds itself to it in its epilogue
                    gsc = gout if isc is None else linear_bwd_data(gout.view(-1, Cout), params[isc].view(Cout, C)).view(n, H, W, C)
                    if order_ == "post":
                        dx, gam = _rs_conv(pool, d1, d1am, packs[iw1][1], None, n, H, W, Chid, C, res=gsc)
                    else:  # through the leading LeakyReLU: multiply by lrelu'(x) = lrelu'(a0)
                        dx, gam = _rs_conv(pool, d1, d1am, packs[iw1][1], None, n, H, W, Chid, C, y_act_src=a0, y_src_act=LEAKY,
                                           res=gsc)
                    g = dx
            elif op[0] == "pool":
                H, W, C = rec
                g = avgpool_bwd(g, n, H, W, C)  # every input position collects at most 4 window shares of 1/9: the bound holds
            elif op[0] == "act":
                g = g.clone() if g is dout else g
                call("mvk_act_bwd", ptr(g), ptr(rec[0]), g.numel(), op[1], stream_ptr())
            else:
                H, W, C = rec
                g = upsample2_bwd(g, n, H, W, C)
                gam = gam * 4.0 if gam is not None else None  # sums of 4 entries: a looser bound costs range, not precision
        return (g if need_dx else None, None, *grads)


# =====================================================================================================
# Fused posterior kernels
# =====================================================================================================
class MoPoEPosteriorFn(Function):
    """(mu_m, lv_m)_m -> z[K,B,L], kld_rows[B] (+ subset statistics); see mvk_mopoe_posterior_fwd.

    Inputs are given in PoE summation order (sorted modality names); subset_masks refer to that order.
    """

    @staticmethod
    def forward(ctx, eps, subset_masks, sel, weights, want_stats, *mus_lvs):
        M = len(mus_lvs) // 2
        mus = [_c(t) for t in mus_lvs[:M]]
        lvs = [_c(t) for t in mus_lvs[M:]]
        K, B, L = eps.shape
        S = subset_masks.numel()
        z = _new((K, B, L), eps)
        kld_rows = _new((B,), eps)
        mus_out = _new((S, B, L), eps) if want_stats else None
        lvs_out = _new((S, B, L), eps) if want_stats else None
        jmu = _new((B, L), eps) if want_stats else None
        jlv = _new((B, L), eps) if want_stats else None
        call("mvk_mopoe_posterior_fwd", ptr_array(mus), ptr_array(lvs), M, ptr(subset_masks), S, ptr(sel),
             ptr(weights), ptr(eps), K, B, L, ptr(z), ptr(kld_rows), ptr(mus_out), ptr(lvs_out), ptr(jmu), ptr(jlv),
             stream_ptr())
        ctx.save_for_backward(eps, subset_masks, sel, *mus, *lvs)
        ctx.weights = weights
        ctx.M = M
        if want_stats:
            ctx.mark_non_differentiable(mus_out, lvs_out, jmu, jlv)
            return z, kld_rows, mus_out, lvs_out, jmu, jlv
        return z, kld_rows

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dkld_rows, *unused):
        dev = ctx.saved_tensors[0].device
        # the gradient of the KL rows: ONE constant the host knows when the loss node registered it (const_grad: the unit-seed
        # path) — read from a kept buffer of that constant, and the assembly launch has no reader inside the step; else it comes
        # out of the assembly launch, which this node then waits for (or runs, when it was postponed)
        c = const_grad(dkld_rows) if dkld_rows is not None else None
        gk = schedule.const_rows(dev, dkld_rows.numel(), c) if c is not None else None
        if gk is None:
            schedule.wait_loss(dev)
            gk = _c(dkld_rows) if dkld_rows is not None else None
        schedule.late_ready(dev)
        saved = ctx.saved_tensors
        eps, subset_masks, sel = saved[:3]
        M = ctx.M
        mus, lvs = saved[3 : 3 + M], saved[3 + M :]
        K, B, L = eps.shape
        dz = _c(dz) if dz is not None else torch.zeros_like(eps)
        dmus = [_new((B, L), eps) for _ in range(M)]
        dlvs = [_new((B, L), eps) for _ in range(M)]
        call("mvk_mopoe_posterior_bwd", ptr_array(mus), ptr_array(lvs), M, ptr(subset_masks), subset_masks.numel(),
             ptr(sel), ptr(ctx.weights), ptr(eps), ptr(dz), K, B, L, ptr(gk), ptr_array(dmus), ptr_array(dlvs),
             stream_ptr())
        return (None, None, None, None, None, *dmus, *dlvs)


class MVTCAEPosteriorFn(Function):
    """(mu_m, lv_m)_m -> z[K,B,L], joint_kl_rows[B], cond_kl_rows[M,B], joint_mu, joint_lv."""

    @staticmethod
    def forward(ctx, eps, masks, *mus_lvs):
        M = len(mus_lvs) // 2
        mus = [_c(t) for t in mus_lvs[:M]]
        lvs = [_c(t) for t in mus_lvs[M:]]
        K, B, L = eps.shape
        z = _new((K, B, L), eps)
        jkl = _new((B,), eps)
        ckl = _new((M, B), eps)
        jmu, jlv = _new((B, L), eps), _new((B, L), eps)
        marr = ptr_array(masks) if masks is not None else None
        call("mvk_mvtcae_posterior_fwd", ptr_array(mus), ptr_array(lvs), marr, M, ptr(eps), K, B, L, ptr(z),
             ptr(jkl), ptr(ckl), ptr(jmu), ptr(jlv), stream_ptr())
        ctx.save_for_backward(eps, *mus, *lvs)
        ctx.masks = masks
        ctx.M = M
        ctx.mark_non_differentiable(jmu, jlv)
        return z, jkl, ckl, jmu, jlv

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, djkl, dckl, *unused):
        schedule.wait_loss(ctx.saved_tensors[0].device)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(ctx.saved_tensors[0].device)
        saved = ctx.saved_tensors
        eps = saved[0]
        M = ctx.M
        mus, lvs = saved[1 : 1 + M], saved[1 + M :]
        K, B, L = eps.shape
        dz = _c(dz) if dz is not None else torch.zeros_like(eps)
        gj = _c(djkl) if djkl is not None else None
        gc = _c(dckl) if dckl is not None else None
        dmus = [_new((B, L), eps) for _ in range(M)]
        dlvs = [_new((B, L), eps) for _ in range(M)]
        marr = ptr_array(ctx.masks) if ctx.masks is not None else None
        call("mvk_mvtcae_posterior_bwd", ptr_array(mus), ptr_array(lvs), marr, M, ptr(eps), ptr(dz), K, B, L,
             ptr(gj), ptr(gc), ptr_array(dmus), ptr_array(dlvs), stream_ptr())
        return (None, None, *dmus, *dlvs)


class JMVAEPosteriorFn(Function):
    """joint (mu, lv), unimodal (mu_m, lv_m)_m -> z[K,B,L], kld_rows[B], ljm_rows[B]  (jmvae_model.py:133-174)."""

    @staticmethod
    def forward(ctx, eps, jmu, jlv, *mus_lvs):
        M = len(mus_lvs) // 2
        jmu, jlv = _c(jmu), _c(jlv)
        mus = [_c(t) for t in mus_lvs[:M]]
        lvs = [_c(t) for t in mus_lvs[M:]]
        K, B, L = eps.shape
        z = _new((K, B, L), eps)
        kld, ljm = _new((B,), eps), _new((B,), eps)
        call("mvk_jmvae_posterior_fwd", ptr(jmu), ptr(jlv), ptr_array(mus), ptr_array(lvs), M, ptr(eps), K, B, L,
             ptr(z), ptr(kld), ptr(ljm), stream_ptr())
        ctx.save_for_backward(eps, jmu, jlv, *mus, *lvs)
        ctx.M = M
        return z, kld, ljm

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dkld, dljm):
        schedule.wait_loss(ctx.saved_tensors[0].device)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(ctx.saved_tensors[0].device)
        saved = ctx.saved_tensors
        eps, jmu, jlv = saved[:3]
        M = ctx.M
        mus, lvs = saved[3 : 3 + M], saved[3 + M :]
        K, B, L = eps.shape
        dz = _c(dz) if dz is not None else None
        gk = _c(dkld) if dkld is not None else None
        gj = _c(dljm) if dljm is not None else None
        djmu, djlv = _new((B, L), eps), _new((B, L), eps)
        dmus = [_new((B, L), eps) for _ in range(M)]
        dlvs = [_new((B, L), eps) for _ in range(M)]
        call("mvk_jmvae_posterior_bwd", ptr(jmu), ptr(jlv), ptr_array(mus), ptr_array(lvs), M, ptr(eps), ptr(dz), K, B,
             L, ptr(gk), ptr(gj), ptr(djmu), ptr(djlv), ptr_array(dmus), ptr_array(dlvs), stream_ptr())
        return (None, djmu, djlv, *dmus, *dlvs)


# =====================================================================================================
# Fused reconstruction NLL + scalar assembly (single autograd node producing the loss)
# =====================================================================================================
def unit_seed(like):
    """A ones tensor shaped like the loss `like`, registered as THE unit backward seed of its device: pass it as
    `loss.backward(gradient=...)` and ReconLossFn.backward needs no launch (autograd's own default seed is a fresh tensor
    whose value the host cannot know without a synchronisation)."""
    key = (like.device, tuple(like.shape))
    t = _UNIT_SEEDS.get(key)
    if t is None:
        t = torch.ones_like(like)
        _UNIT_SEEDS[key] = t
        _UNIT_SEEDS[t.data_ptr()] = t
    return t


def is_unit_seed(g):
    t = _UNIT_SEEDS.get(g.data_ptr())
    return t is not None and t.shape == g.shape and t.device == g.device


def _reduce_terms(terms, n_terms, loss_sum_scale, out, loss):
    """The scalar assembly on the current stream, on several workgroups where a term is long (mvk_reduce_terms_ws)."""
    ws = schedule.terms_workspace(out.device)
    if ws is None:
        # A capturing stream that has no workspace yet (schedule.terms_workspace makes none there).  The warm-up passes of
        # GraphedStep run on another stream than the capture: inside a capture the launch takes the one-workgroup form, which
        # needs no workspace (same sums in the same order per term; bit-identical results are tested for both forms)
        call("mvk_reduce_terms", terms, n_terms, loss_sum_scale, ptr(out), ptr(loss), stream_ptr())
        return
    call("mvk_reduce_terms_ws", terms, n_terms, loss_sum_scale, ptr(out), ptr(loss), ptr(ws), ws.numel(), stream_ptr())


class ReconLossFn(Function):
    """loss = sum_i lossw_i * coef_i * sum_{k,b} mask_i[b] rows_i[k,b] + sum_j lossw_j * coef_j * sum(extra_j).

    forward: ONE mvk_recon_nll_fwd launch for all modalities (row NLLs + d loss / d recon assuming an upstream
             gradient of 1) and ONE mvk_reduce_terms launch.  Returns (loss, terms[n_terms+2]) where terms holds
             every individual term, the loss and loss * loss_sum_scale (all detached: metrics).
    spec:    dict(K, B, x[], masks[], dist[], scale[], rescale[], coef[], lossw[], extra_coef[], extra_lossw[],
             extra_split[], loss_sum_scale).
    extras:  tensors (KL rows) whose sums enter the loss with a constant weight; with extra_split[j] = n the tensor is
             n equal chunks, one term each, and extra_coef[j] may be a list of n per-chunk coefficients.
    pairs:   optional spec["pairs"] = [(tensor index, slab)]: reconstruction term i scores ONE [B, D] slab of the
             decoder output tensors[tensor index] ([K_t, B, D]) against x[i] with its own mask / coefficient (MVAE: a
             decoder runs once over the samples of all its subsets, every (modality, subset) pair is a term).  The
             per-entry lists of spec are then indexed by pair; gradients are still one buffer per decoder output.
    """

    @staticmethod
    def forward(ctx, spec, n_mod, *tensors):
        recons = [_c(t) for t in tensors[:n_mod]]
        extras = [_c(t) for t in tensors[n_mod:]]
        xs, masks = spec["x"], spec["masks"]
        K, B = spec["K"], spec["B"]
        pairs = spec.get("pairs")
        ref = recons[0] if recons else extras[0]
        drecons = [torch.empty_like(r) if ctx.needs_input_grad[2 + i] else None for i, r in enumerate(recons)]
        if pairs is not None:  # every term is one slab: K = 1 launches; untouched slabs of a buffer get no gradient
            used = {}
            for j, k in pairs:
                used.setdefault(j, set()).add(k)
            for j, g in enumerate(drecons):
                if g is not None and len(used.get(j, ())) != g.shape[0]:
                    g.zero_()
        n_rec = len(pairs) if pairs is not None else n_mod
        descs = (ReconDesc * max(n_rec, 1))()
        rows = []
        for i in range(n_rec):
            j, k = pairs[i] if pairs is not None else (i, None)
            Kt = recons[j].shape[0] if pairs is not None else K
            D = recons[j].numel() // (Kt * B)
            off = 0 if k is None else 4 * k * B * D
            r = _new((1 if pairs is not None else K, B), ref)
            rows.append(r)
            d = descs[i]
            d.recon, d.x = recons[j].data_ptr() + off, xs[i].data_ptr()
            d.mask = masks[i].data_ptr() if masks[i] is not None else None
            d.rows = r.data_ptr()
            d.drecon = drecons[j].data_ptr() + off if drecons[j] is not None else None
            d.rowcoef = None
            d.D, d.dist, d.n_classes = D, spec["dist"][i], recons[j].shape[-1]
            d.scale, d.rescale = spec["scale"][i], spec["rescale"][i]
            d.coef = spec["coef"][i] * spec["lossw"][i]
        if n_rec:
            prof = PROFILE.get("recon_nll")
            if prof is not None:
                # measurement only: a short spin kernel ahead of the first event lets the host finish enqueueing the
                # launch while the GPU is busy, so the event pair brackets the kernel and not the launch latency
                if PROFILE.get("presleep_cycles"):
                    torch.cuda._sleep(int(PROFILE["presleep_cycles"]))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
            Kl = 1 if pairs is not None else K
            for i0 in range(0, n_rec, _lib.MAX_MODALITIES):  # MVK_MAX_MODALITIES descriptors per launch
                n = min(_lib.MAX_MODALITIES, n_rec - i0)
                call("mvk_recon_nll_fwd", C.cast(C.byref(descs[i0]), C.POINTER(ReconDesc)), n, Kl, B, stream_ptr())
            if prof is not None:
                e1.record()
                prof.append((e0, e1))
        splits = spec.get("extra_split") or [1] * len(extras)
        n_terms = n_rec + sum(splits)
        terms = (TermDesc * n_terms)()
        for i in range(n_rec):
            t = terms[i]
            t.v, t.n = rows[i].data_ptr(), rows[i].numel()
            t.mask = masks[i].data_ptr() if masks[i] is not None else None
            t.period, t.coef, t.lossw = B, spec["coef"][i], spec["lossw"][i]
        ti = n_rec
        extra_grad = []  # (byte offset, numel, coefficient) per chunk of every extra tensor
        # the gradients of the extra tensors for an upstream gradient of 1 are constants: mvk_reduce_terms writes them
        # (backward then launches nothing when its upstream gradient is the unit seed)
        dextras = [torch.empty_like(e) if ctx.needs_input_grad[2 + n_mod + j] else None for j, e in enumerate(extras)]
        for j, e in enumerate(extras):
            ns = splits[j]
            chunk = e.numel() // ns
            cj = spec["extra_coef"][j]
            for c in range(ns):  # one term per chunk (e.g. per-modality KL rows), one gradient per tensor
                t = terms[ti]
                cc = cj[c] if isinstance(cj, (list, tuple)) else cj
                t.v, t.n, t.mask, t.period = e.data_ptr() + 4 * c * chunk, chunk, None, 1
                t.coef, t.lossw = cc, spec["extra_lossw"][j]
                t.gfill = dextras[j].data_ptr() + 4 * c * chunk if dextras[j] is not None else None
                extra_grad.append((j, 4 * c * chunk, chunk, cc * spec["extra_lossw"][j]))
                ti += 1
        out = _new((n_terms + 2,), ref)
        loss = _new((), ref)
        # Every reconstruction term came from a fused decoder tail (n_rec == 0) and the model vouches for its backward nodes
        # (spec["async_ok"]: they call wait_loss before reading a gradient this launch fills): the assembly is a leaf of the
        # step — nothing on the backward chain needs the loss VALUE — so it runs on the late-leaf stream, joined where the
        # deferred finishes run, instead of between the last forward and the first backward launch of the critical chain.
        late = schedule.late_leaves(ref.device, *extras) if (schedule.ASYNC_LOSS and n_rec == 0 and spec.get("async_ok")) else None
        dev = ref.device
        if late is not None and late.on and schedule.ASSEMBLY_LAST and spec.get("assembly_last"):
            # The model vouches that NO backward node reads what this launch fills when the backward seed is the unit seed (its
            # posterior node takes the KL rows' constant gradient from const_grad): the launch is enqueued with the postponed
            # leaves at the end of the scope (run_last: the late-leaf stream, behind the large decoder's weight gradients) instead
            # of at the head of the backward pass, where its 18 workgroups wait 50-80 us for slots beside the image layer's 512
            # persistent workgroups — and delay them.  A node that does read (general seed, style latents) runs it first: wait_loss.
            keep = [out, loss] + [d for d in dextras if d is not None]

            def assemble():
                _reduce_terms(terms, n_terms, spec["loss_sum_scale"], out, loss)
                st = torch.cuda.current_stream(dev)
                for t in keep:
                    t.record_stream(st)

            if schedule.run_last(dev, assemble, *extras):
                late.scope.loss = assemble  # wait_loss runs it for whoever reads what it fills before the scope ends
            else:
                assemble()
        elif late is not None and late.on:
            # (postponing this launch behind the image layer's backward kernel — it competes with that kernel's persistent
            # workgroups for CU slots at the head of the backward pass — was measured: +60 us per step, the ninth cross-stream
            # edge inside the captured step that lost; profiles/NOTES_r05.md section 9)
            with late:
                _reduce_terms(terms, n_terms, spec["loss_sum_scale"], out, loss)
                st = torch.cuda.current_stream(ref.device)
                late.scope.loss = st.record_event()
                for t in [out, loss] + [d for d in dextras if d is not None]:
                    t.record_stream(st)
        else:
            _reduce_terms(terms, n_terms, spec["loss_sum_scale"], out, loss)
        ctx.drecons = drecons
        ctx.dextras = dextras
        ctx.extra_shapes = [e.shape for e in extras]
        ctx.extra_grad = extra_grad
        ctx.rows = rows  # keep alive: metrics / debugging
        if spec.get("rows_out") is not None:  # the caller's list receives the (unmasked) reconstruction rows: metrics
            spec["rows_out"].extend(rows)
        ctx.mark_non_differentiable(out)
        ctx.set_materialize_grads(False)  # no zero-fill launch for the gradient of `out` (never used)
        return loss, out

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss, gout):
        if gloss is None:  # only the (non-differentiable) terms were used
            return (None, None) + (None,) * (len(ctx.drecons) + len(ctx.extra_shapes))
        grads = list(ctx.drecons)
        if is_unit_seed(gloss):  # d loss = 1 exactly: every gradient below was written by the forward launches
            extras = list(ctx.dextras)
            # a single-term extra tensor's gradient is ONE constant the host knows: a fused decoder tail whose stored gradient
            # was pre-multiplied by it (MLPDecoderFn / SVHNDecoderFn `nll_weight`) then reads no row gradient at all
            per = {}
            for j, _off, _n, c in ctx.extra_grad:
                per.setdefault(j, []).append(c)
            for j, cs in per.items():
                if extras[j] is not None and len(set(cs)) == 1:
                    register_const_grad(extras[j], cs[0])
            ctx.drecons = ctx.dextras = None
            return (None, None, *grads, *extras)
        schedule.wait_loss(gloss.device)  # the seed launch below rewrites what the assembly launch filled
        gloss = _c(gloss.reshape(1))
        extras = [d if d is not None else _new(shape, gloss) for d, shape in zip(ctx.dextras, ctx.extra_shapes)]
        jobs = [(g.data_ptr(), g.numel(), 1.0, 0) for g in ctx.drecons if g is not None]
        jobs += [(extras[j].data_ptr() + off, n, c, 1) for j, off, n, c in ctx.extra_grad]
        for i0 in range(0, len(jobs), 12):  # MVK_SEED_MAX buffers per launch: normally ONE launch
            chunk = jobs[i0:i0 + 12]
            descs = (SeedDesc * len(chunk))()
            for d, (p, n, c, fill) in zip(descs, chunk):
                d.buf, d.n, d.coef, d.fill = p, n, float(c), fill
            call("mvk_loss_backward_seed", descs, len(chunk), ptr(gloss), stream_ptr())
        ctx.drecons = ctx.dextras = None
        return (None, None, *grads, *extras)


class GaussSampleKLFn(Function):
    """(mu, lv) [B,S], eps [K,B,S] -> w [K,B,S], kl_rows [B]  (mvk_gauss_sample_kl_fwd/bwd; MoPoE style latents)."""

    @staticmethod
    def forward(ctx, eps, mu, lv):
        eps, mu, lv = _c(eps), _c(mu), _c(lv)
        K, B, L = eps.shape
        w = torch.empty_like(eps)
        kl = _new((B,), eps)
        call("mvk_gauss_sample_kl_fwd", ptr(mu), ptr(lv), ptr(eps), K, B, L, ptr(w), ptr(kl), stream_ptr())
        ctx.save_for_backward(eps, mu, lv)
        return w, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, dw, dkl):
        schedule.wait_loss(ctx.saved_tensors[0].device)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(ctx.saved_tensors[0].device)
        eps, mu, lv = ctx.saved_tensors
        K, B, L = eps.shape
        dw = _c(dw) if dw is not None else None
        dkl = _c(dkl) if dkl is not None else None
        dmu, dlv = torch.empty_like(mu), torch.empty_like(lv)
        call("mvk_gauss_sample_kl_bwd", ptr(mu), ptr(lv), ptr(eps), ptr(dw), ptr(dkl), K, B, L, ptr(dmu), ptr(dlv),
             stream_ptr())
        return None, dmu, dlv


class TELBOLatentFn(Function):
    """TELBO stage two: eps [M,B,L], the joint encoder's log-variance [B,L], unimodal (mu_m, lv_m)_m -> kld_rows [M,B], z_0 [B,L],
    ..., z_{M-1} (the M slabs of the kernel's z [M,B,L]) with kld_rows[m,b] = -1/2 sum_l (1 + joint_lv - mu_m^2 - exp(lv_m))
    (telbo_model.py:110-120; mvk_telbo_latent_fwd/bwd).  joint_lv gets a gradient only when it asks for one (the model hands in
    a tensor without autograd: djoint_lv = NULL)."""

    @staticmethod
    def forward(ctx, eps, jlv, *mus_lvs):
        M = len(mus_lvs) // 2
        eps, jlv = _c(eps), _c(jlv)
        mus = [_c(t) for t in mus_lvs[:M]]
        lvs = [_c(t) for t in mus_lvs[M:]]
        Me, B, L = eps.shape
        if Me != M or len(mus_lvs) != 2 * M or M < 1:
            raise ValueError(f"TELBOLatentFn: eps holds {Me} modalities, {len(mus_lvs)} (mu, lv) tensors were given")
        for t in [jlv, *mus, *lvs]:
            if tuple(t.shape) != (B, L):
                raise ValueError(f"TELBOLatentFn: expected [{B}, {L}] for every mean and log-variance, got {tuple(t.shape)}")
        z = _new((M, B, L), eps)
        kld = _new((M, B), eps)
        call("mvk_telbo_latent_fwd", ptr(jlv), ptr_array(mus), ptr_array(lvs), M, ptr(eps), B, L, ptr(z), ptr(kld), stream_ptr())
        ctx.save_for_backward(eps, *mus, *lvs)
        ctx.M = M
        ctx.want_jlv = ctx.needs_input_grad[1]
        ctx.set_materialize_grads(False)
        return (kld, *z.unbind(0))  # one decoder input per modality: no slice node (zero-fill + copy in backward) per decoder

    @staticmethod
    @once_differentiable
    def backward(ctx, dkld, *dzs):
        schedule.wait_loss(ctx.saved_tensors[0].device)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(ctx.saved_tensors[0].device)
        saved = ctx.saved_tensors
        eps, M = saved[0], ctx.M
        mus, lvs = saved[1 : 1 + M], saved[1 + M :]
        _, B, L = eps.shape
        dz = None
        if any(g is not None for g in dzs):  # the decoders' input gradients, side by side again (one launch)
            dz = torch.stack([g if g is not None else torch.zeros_like(mus[0]) for g in dzs])
        gk = _c(dkld) if dkld is not None else None
        dmus = [_new((B, L), eps) for _ in range(M)]
        dlvs = [_new((B, L), eps) for _ in range(M)]
        djlv = _new((B, L), eps) if ctx.want_jlv else None
        call("mvk_telbo_latent_bwd", ptr_array(mus), ptr_array(lvs), M, ptr(eps), ptr(dz), ptr(gk), B, L, ptr_array(dmus),
             ptr_array(dlvs), ptr(djlv), stream_ptr())
        return (None, djlv, *dmus, *dlvs)


class CondLatentFn(Function):
    """(mu, lv) [B,L], prior (pmu, plv) [B,L] or (None, None) = N(0, I), eps [K,B,L], conditioning pieces [B, ...] ->
    zc [K,B,L+C] (the samples beside the flattened conditioning data: the conditional decoder's input), kl_rows [B]
    (mvk_cond_latent_fwd/bwd; CVAE).  want_kl=False: the sample only (kl_rows is None).  The pieces get no gradient."""

    @staticmethod
    def forward(ctx, eps, mu, lv, pmu, plv, want_kl, *cond):
        eps, mu, lv = _c(eps), _c(mu), _c(lv)
        if (pmu is None) != (plv is None):
            raise ValueError("CondLatentFn: the prior's mean and log-variance are given together or not at all")
        pmu, plv = (None, None) if pmu is None else (_c(pmu), _c(plv))
        K, B, L = eps.shape
        pieces = [_c(t.reshape(B, -1)) for t in cond]
        dims = (C.c_int * max(len(pieces), 1))(*[int(p.shape[1]) for p in pieces])
        Cc = sum(int(p.shape[1]) for p in pieces)
        zc = _new((K, B, L + Cc), eps)
        kl = _new((B,), eps) if want_kl else None
        call("mvk_cond_latent_fwd", ptr(mu), ptr(lv), ptr(pmu), ptr(plv), ptr(eps), ptr_array(pieces), dims, len(pieces), K, B, L,
             ptr(zc), ptr(kl), stream_ptr())
        ctx.save_for_backward(eps, mu, lv, *(() if pmu is None else (pmu, plv)))
        ctx.C = Cc
        ctx.n_cond = len(cond)
        if kl is None:
            return zc, None
        return zc, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, dzc, dkl):
        dev = ctx.saved_tensors[0].device
        schedule.wait_loss(dev)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(dev)
        eps, mu, lv = ctx.saved_tensors[:3]
        pmu, plv = ctx.saved_tensors[3:] if len(ctx.saved_tensors) > 3 else (None, None)
        K, B, L = eps.shape
        dzc = _c(dzc) if dzc is not None else None
        dkl = _c(dkl) if dkl is not None else None
        dmu, dlv = torch.empty_like(mu), torch.empty_like(lv)
        dpmu, dplv = (None, None) if pmu is None else (torch.empty_like(pmu), torch.empty_like(plv))
        call("mvk_cond_latent_bwd", ptr(mu), ptr(lv), ptr(pmu), ptr(plv), ptr(eps), ptr(dzc), ptr(dkl), K, B, L, ctx.C, ptr(dmu),
             ptr(dlv), ptr(dpmu), ptr(dplv), stream_ptr())
        return (None, dmu, dlv, dpmu, dplv, None) + (None,) * ctx.n_cond


class MHVAELevelFn(Function):
    """One level of the MHVAE hierarchy for all S subsets (mvk_mhvae_level_fwd/bwd): the product of each subset's available
    experts and the prior, one sample and the KL to the prior -> z [S,B,F], kl_rows [S,B].
    member: S bitmasks over the E experts; masks: None or E entries (bool [B] or None); eps [S,B,F] or None (z = the mean).
    shared=True: expert e is (mu, lv) of B F elements, the prior is N(0, I) (pmu = plv = None); shared=False: expert e holds S_e B F
    elements, one block per subset holding it in increasing subset order, the prior pmu, plv S B F.  experts = mu_0, lv_0, mu_1,
    lv_1, ...: any shape with that many elements; every one and the prior get a gradient of their own shape."""

    @staticmethod
    def forward(ctx, eps, member, shared, masks, B, F, pmu, plv, *experts):
        mus, lvs = [_c(t) for t in experts[0::2]], [_c(t) for t in experts[1::2]]
        E, S = len(mus), len(member)
        if len(lvs) != E or E < 1:
            raise ValueError("MHVAELevelFn: the experts are given as (mu, lv) pairs")
        if (pmu is None) != (plv is None) or (pmu is None) != bool(shared):
            raise ValueError("MHVAELevelFn: the shared layout takes no prior, the per-subset layout needs one")
        pmu, plv = (None, None) if pmu is None else (_c(pmu), _c(plv))
        eps = None if eps is None else _c(eps)
        for e in range(E):
            n = (1 if shared else sum(1 for m in member if m >> e & 1)) * B * F
            if mus[e].numel() != n or lvs[e].numel() != n:
                raise ValueError(f"MHVAELevelFn: expert {e} holds {mus[e].numel()} / {lvs[e].numel()} elements, expected {n}")
        for t in (pmu, plv, eps):
            if t is not None and t.numel() != S * B * F:
                raise ValueError(f"MHVAELevelFn: the prior and eps hold S B F = {S * B * F} elements")
        if masks is not None:
            masks = [None if m is None else m.to(torch.bool).contiguous() for m in masks]
        marr = ptr_array(masks) if masks is not None else None
        mem = (C.c_int32 * S)(*[int(m) for m in member])
        z = _new((S, B, F), mus[0])
        kl = _new((S, B), mus[0])
        call("mvk_mhvae_level_fwd", ptr_array(mus), ptr_array(lvs), marr, E, mem, S, int(bool(shared)), ptr(pmu), ptr(plv),
             ptr(eps), B, F, ptr(z), ptr(kl), stream_ptr())
        ctx.save_for_backward(*mus, *lvs, *(() if pmu is None else (pmu, plv)), *(() if eps is None else (eps,)))
        ctx.masks = masks
        ctx.cfg = (E, S, bool(shared), B, F, tuple(int(m) for m in member), pmu is not None, eps is not None)
        ctx.shapes = [t.shape for t in experts]
        return z, kl

    @staticmethod
    @once_differentiable
    def backward(ctx, dz, dkl):
        E, S, shared, B, F, member, has_prior, has_eps = ctx.cfg
        saved = ctx.saved_tensors
        dev = saved[0].device
        schedule.wait_loss(dev)  # the gradients of the KL rows come out of the loss assembly launch
        schedule.late_ready(dev)
        mus, lvs = list(saved[:E]), list(saved[E:2 * E])
        rest = list(saved[2 * E:])
        pmu, plv = (rest.pop(0), rest.pop(0)) if has_prior else (None, None)
        eps = rest.pop(0) if has_eps else None
        dz = _c(dz) if dz is not None else None
        dkl = _c(dkl) if dkl is not None else None
        dmus, dlvs = [torch.empty_like(t) for t in mus], [torch.empty_like(t) for t in lvs]
        dpmu, dplv = (None, None) if pmu is None else (torch.empty_like(pmu), torch.empty_like(plv))
        marr = ptr_array(ctx.masks) if ctx.masks is not None else None
        mem = (C.c_int32 * S)(*member)
        call("mvk_mhvae_level_bwd", ptr_array(mus), ptr_array(lvs), marr, E, mem, S, int(shared), ptr(pmu), ptr(plv), ptr(eps),
             ptr(dz), ptr(dkl), B, F, ptr_array(dmus), ptr_array(dlvs), ptr(dpmu), ptr(dplv), stream_ptr())
        grads = []
        for e in range(E):
            grads += [dmus[e].view(ctx.shapes[2 * e]), dlvs[e].view(ctx.shapes[2 * e + 1])]
        return (None, None, None, None, None, None, dpmu, dplv, *grads)


class NexusAggregateFn(Function):
    """msgs_m [B, D] -> (agg [B, D], keep [B, M]): the Nexus message mean over the kept modalities (mvk_nexus_aggregate_fwd/bwd,
    nexus_model.py:209-254).  Keep set: masks (list of M bool [B]), keep_in [B, M], or FPD from u [B, M + 1] uniforms on [0, 1)
    with drop probability p; keep is the set used (non-differentiable)."""

    @staticmethod
    def forward(ctx, masks, keep_in, u, p, *msgs):
        msgs = [_c(t) for t in msgs]
        M = len(msgs)
        B, D = msgs[0].shape
        agg = _new((B, D), msgs[0])
        keep = _new((B, M), msgs[0])
        marr = ptr_array(masks) if masks is not None else None
        call("mvk_nexus_aggregate_fwd", ptr_array(msgs), marr, ptr(keep_in), ptr(u), float(p), M, B, D, ptr(agg), ptr(keep),
             stream_ptr())
        ctx.save_for_backward(keep)
        ctx.mark_non_differentiable(keep)
        ctx.shape = (M, B, D)
        return agg, keep

    @staticmethod
    @once_differentiable
    def backward(ctx, g, gkeep):
        (keep,) = ctx.saved_tensors
        M, B, D = ctx.shape
        g = _c(g)
        d = [torch.empty((B, D), dtype=torch.float32, device=g.device) for _ in range(M)]
        call("mvk_nexus_aggregate_bwd", ptr(keep), ptr(g), M, B, D, ptr_array(d), stream_ptr())
        return (None, None, None, None, *d)


class NexusTopNLLFn(Function):
    """(z_m [B, D_m] detached, r_m [B, D_m])_m -> rows [M, B]: gamma_m mask_m sum_d -ln N(z_m | r_m, s_m), s_m = 1 or the adapted
    scale sqrt(mean((z_m - r_m)^2)) (mvk_nexus_top_nll_fwd/bwd, nexus_model.py:153-168).  Also returns s2 [M] (detached)."""

    @staticmethod
    def forward(ctx, masks, gammas, adapt, *zr):
        M = len(zr) // 2
        zs = [_c(t) for t in zr[:M]]
        rs = [_c(t) for t in zr[M:]]
        B = zs[0].shape[0]
        ref = zs[0]
        rows = _new((M, B), ref)
        q = _new((M, B), ref)
        s2 = _new((M,), ref)
        work = _new((M * ((B + 3) // 4),), ref)
        Ds = (C.c_int * M)(*[int(z.shape[1]) for z in zs])
        gam = (C.c_float * M)(*[float(g) for g in gammas])
        ad = (C.c_int * M)(*[1 if a else 0 for a in adapt])
        marr = ptr_array(masks) if masks is not None else None
        call("mvk_nexus_top_nll_fwd", ptr_array(zs), ptr_array(rs), marr, Ds, gam, ad, M, B, ptr_array(list(rows)), ptr(q),
             ptr(s2), ptr(work), stream_ptr())
        ctx.save_for_backward(*zs, *rs, q, s2)
        ctx.masks, ctx.cfg, ctx.work = masks, (Ds, gam, ad, M, B), work
        ctx.mark_non_differentiable(s2)
        return rows, s2

    @staticmethod
    @once_differentiable
    def backward(ctx, grows, gs2):
        Ds, gam, ad, M, B = ctx.cfg
        saved = ctx.saved_tensors
        zs, rs, q, s2 = saved[:M], saved[M:2 * M], saved[2 * M], saved[2 * M + 1]
        if grows is None:
            return (None, None, None) + (None,) * M + tuple(torch.zeros_like(r) for r in rs)
        schedule.wait_loss(grows.device)  # the rows' gradient may come out of the loss assembly launch
        grows = _c(grows)
        dr = [torch.empty_like(r) for r in rs]
        marr = ptr_array(ctx.masks) if ctx.masks is not None else None
        call("mvk_nexus_top_nll_bwd", ptr_array(zs), ptr_array(rs), marr, Ds, gam, ad, M, B, ptr_array(list(grows)), ptr(q),
             ptr(s2), ptr(ctx.work), ptr_array(dr), stream_ptr())
        return (None, None, None) + (None,) * M + tuple(dr)


class MVAEPosteriorFn(Function):
    """(mu_m, lv_m)_m, eps [S,B,L] -> z of every subset written into its modalities' decoder inputs zm[m] [K_m,B,L],
    kld_rows [S,B] (mvk_mvae_posterior_fwd/bwd; mvae_model.py:56-118)."""

    @staticmethod
    def forward(ctx, eps, masks, subset_bits, want_stats, *mus_lvs):
        M = len(mus_lvs) // 2
        mus = [_c(t) for t in mus_lvs[:M]]
        lvs = [_c(t) for t in mus_lvs[M:]]
        eps = _c(eps)
        S, B, L = eps.shape
        bits = (C.c_int32 * S)(*subset_bits)
        counts = [sum((b >> m) & 1 for b in subset_bits) for m in range(M)]
        zm = [_new((counts[m], B, L), eps) if counts[m] else None for m in range(M)]
        kld = _new((S, B), eps)
        smu = _new((S, B, L), eps) if want_stats else None
        slv = _new((S, B, L), eps) if want_stats else None
        marr = ptr_array(masks) if masks is not None else None
        call("mvk_mvae_posterior_fwd", ptr_array(mus), ptr_array(lvs), marr, M, bits, S, ptr(eps), B, L, ptr_array(zm),
             ptr(kld), ptr(smu) if want_stats else None, ptr(slv) if want_stats else None, stream_ptr())
        ctx.save_for_backward(eps, *mus, *lvs)
        ctx.masks, ctx.bits, ctx.M, ctx.n_z = masks, bits, M, sum(1 for t in zm if t is not None)
        ctx.has_z = [t is not None for t in zm]
        outs = [t for t in zm if t is not None] + [kld]
        if want_stats:
            outs += [smu, slv]
            ctx.mark_non_differentiable(smu, slv)
        return tuple(outs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        saved = ctx.saved_tensors
        eps, M = saved[0], ctx.M
        mus, lvs = list(saved[1:1 + M]), list(saved[1 + M:1 + 2 * M])
        S, B, L = eps.shape
        gz = iter(grads[:ctx.n_z])
        dzm = [(_c(next(gz)) if has else None) for has in ctx.has_z]
        gk = grads[ctx.n_z]
        gk = _c(gk) if gk is not None else None
        dmu = [torch.empty_like(t) for t in mus]
        dlv = [torch.empty_like(t) for t in lvs]
        marr = ptr_array(ctx.masks) if ctx.masks is not None else None
        call("mvk_mvae_posterior_bwd", ptr_array(mus), ptr_array(lvs), marr, M, ctx.bits, S, ptr(eps), ptr_array(dzm), B,
             L, ptr(gk) if gk is not None else None, ptr_array(dmu), ptr_array(dlv), stream_ptr())
        return (None, None, None, None, *dmu, *dlv)


def adam_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, grad_scale=1.0, vmax=None,
              zero_grad=False):
    """torch.optim.Adam on flat buffers, one launch; vmax = the amsgrad running maximum of exp_avg_sq (or None);
    zero_grad: g is cleared as it is consumed."""
    call("mvk_adam_step_fused", ptr(p), ptr(g), ptr(m), ptr(v), ptr(vmax), p.numel(), lr, beta1, beta2, eps,
         weight_decay, step, grad_scale, 1 if zero_grad else 0, stream_ptr())


# =====================================================================================================
# MMVAE: mixture-of-experts importance weights (IWAE / DReG)
# =====================================================================================================
class MMVAEStdFn(Function):
    """std = exp(lv/2) | softmax(lv)*L + 1e-6   (mmvae_model.py:66-74)."""

    @staticmethod
    def forward(ctx, lv, family):
        lv2 = _c(lv.reshape(-1, lv.shape[-1]))
        sd = torch.empty_like(lv2)
        call("mvk_mmvae_std_fwd", ptr(lv2), lv2.shape[0], lv2.shape[1], family, ptr(sd), stream_ptr())
        ctx.save_for_backward(lv2, sd)
        ctx.family = family
        ctx.shape = lv.shape
        return sd.view(lv.shape)

    @staticmethod
    @once_differentiable
    def backward(ctx, dsd):
        lv2, sd = ctx.saved_tensors
        dsd = _c(dsd).view(lv2.shape)
        dlv = torch.empty_like(lv2)
        call("mvk_mmvae_std_bwd", ptr(lv2), ptr(sd), ptr(dsd), lv2.shape[0], lv2.shape[1], ctx.family, ptr(dlv),
             stream_ptr())
        return dlv.view(ctx.shape), None


class MMVAEState:
    """Tensors shared between the latent node and the objective node of one forward pass."""

    def __init__(self):
        self.z = self.lpz = self.lqz = self.lq_all = None
        self.w = self.rowcoef = self.lw = None
        self.gloss = None
        self.lqw = None          # MMVAE+: log q_c(w_c) rows
        self.shared_dims = None  # MMVAE+: leading latent dims that enter the mixture (None = all)
        self.beta = 1.0          # MMVAE+: weight of the latent terms of lw
        self.resp = None         # CMVAE: q(cluster | u_c) rows [K,B,C]


# ---- shared by the two latent nodes (MMVAELatentFn, CMVAELatentFn) ----
def _latent_alloc(state, M, K, B, D, like, private):
    """The outputs of a latent forward launch into `state` (lqw only with private dims) -> the samples z_c [K,B,D]."""
    state.z = [_new((K, B, D), like) for _ in range(M)]
    state.lpz = [_new((K, B), like) for _ in range(M)]
    state.lqz = [_new((K, B), like) for _ in range(M)]
    state.lq_all = [_new((M, K, B), like) for _ in range(M)]
    state.lqw = [_new((K, B), like) for _ in range(M)] if private else None
    return state.z


def _mask_array(masks):
    return ptr_array(masks) if masks is not None else None


def _dz_or_zeros(dzs, zs):
    """The decoders' gradients of the samples, zeros where a sample reached no decoder."""
    return [(_c(d) if d is not None else torch.zeros_like(zs[i])) for i, d in enumerate(dzs)]


def _sum_rows(rows):
    """Per-batch-row terms [B, n] of a parameter gradient -> their sum [n], in a fixed order."""
    B, n = rows.shape
    out = _zeros((n,), rows)
    ws = _ws(rows)
    call("mvk_colsum_acc", ptr(rows), None, NONE, ptr(out), B, n, ptr(ws), ws.numel(), stream_ptr())
    return out


class MMVAELatentFn(Function):
    """(mu_c, std_c)_c, prior_std -> z_c [K,B,L] for every conditioning modality; also fills state.lpz / lqz."""

    @staticmethod
    def forward(ctx, state, noises, masks, prior_mean, family, dreg, prior_std, *mus_stds):
        M = len(mus_stds) // 2
        mus = [_c(t) for t in mus_stds[:M]]
        sds = [_c(t) for t in mus_stds[M:]]
        prior_std = _c(prior_std.reshape(-1))
        prior_mean = _c(prior_mean.reshape(-1))
        K, B, L = noises[0].shape
        Ls = L if state.shared_dims is None else int(state.shared_dims)
        zs = _latent_alloc(state, M, K, B, L, mus[0], private=Ls < L)
        call("mvk_mmvae_latent_fwd", ptr_array(mus), ptr_array(sds), ptr_array(noises), _mask_array(masks), ptr(prior_mean),
             ptr(prior_std), M, K, B, L, family, ptr_array(zs), ptr_array(state.lpz), ptr_array(state.lqz),
             ptr_array(state.lq_all), Ls, ptr_array(state.lqw) if state.lqw is not None else None, stream_ptr())
        ctx.save_for_backward(prior_mean, prior_std, *mus, *sds)
        ctx.state, ctx.noises, ctx.masks = state, noises, masks
        ctx.family, ctx.dreg, ctx.M = family, dreg, M
        return tuple(zs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dzs):
        saved = ctx.saved_tensors
        prior_mean, prior_std = saved[0], saved[1]
        M = ctx.M
        mus, sds = saved[2 : 2 + M], saved[2 + M :]
        st = ctx.state
        K, B, L = ctx.noises[0].shape
        dzs = _dz_or_zeros(dzs, st.z)
        dmus = [_new((B, L), mus[0]) for _ in range(M)]
        dsds = [_new((B, L), mus[0]) for _ in range(M)]
        dprior_rows = _new((B, L), mus[0])  # per-row terms of d loss / d prior_std
        call("mvk_mmvae_latent_bwd", ptr_array(mus), ptr_array(sds), ptr_array(ctx.noises), ptr_array(st.z),
             _mask_array(ctx.masks), ptr(prior_mean), ptr(prior_std), ptr_array(st.w), ptr_array(st.lq_all), ptr_array(st.lqz),
             ptr_array(dzs), M, K, B, L, ctx.family, ctx.dreg, ptr(st.gloss), ptr_array(dmus), ptr_array(dsds),
             ptr(dprior_rows), L if st.shared_dims is None else int(st.shared_dims), float(st.beta), stream_ptr())
        return (None, None, None, None, None, None, _sum_rows(dprior_rows).view(1, L), *dmus, *dsds)


class MMVAEPlusCrossLatentFn(Function):
    """z_c [K,B,D] (= [u_c, w_c]), the target modality's private prior std [S], noise [K,B,S] -> [u_c, w ~ prior_r]
    (mmvaePlus_model.py:152-172)."""

    @staticmethod
    def forward(ctx, z, prior_std, noise, Ls, family):
        z = _c(z)
        prior_std = _c(prior_std.reshape(-1))
        noise = _c(noise)
        K, B, D = z.shape
        zc = torch.empty_like(z)
        call("mvk_mmvaeplus_cross_latent_fwd", ptr(z), ptr(prior_std), ptr(noise), K * B, D, Ls, family, ptr(zc),
             stream_ptr())
        ctx.save_for_backward(noise)
        ctx.dims = (K, B, D, Ls, family)
        ctx.prior_shape = None
        return zc

    @staticmethod
    @once_differentiable
    def backward(ctx, dzc):
        (noise,) = ctx.saved_tensors
        K, B, D, Ls, family = ctx.dims
        dzc = _c(dzc)
        dz = torch.empty_like(dzc)
        dprior = _new((1, D - Ls), dzc)
        call("mvk_mmvaeplus_cross_latent_bwd", ptr(dzc), ptr(noise), K * B, D, Ls, family, ptr(dz), ptr(dprior),
             stream_ptr())
        return dz, dprior, None, None, None


class MMVAEObjectiveFn(Function):
    """recon[c][r] (M*M tensors, c-major) -> loss.  forward: row NLLs + IWAE/DReG objective; backward: the
    second reconstruction pass with the per-row weights d loss / d lw."""

    @staticmethod
    def forward(ctx, state, spec, M, dreg, *recons):
        recons = [_c(t) for t in recons]
        K, B = spec["K"], spec["B"]
        ref = recons[0]
        descs = (ReconDesc * M)()
        rows = []
        for c in range(M):
            for r in range(M):
                d = descs[r]
                rr = _new((K, B), ref)
                rows.append(rr)
                t = recons[c * M + r]
                d.recon, d.x = t.data_ptr(), spec["x"][r].data_ptr()
                d.mask, d.rows, d.drecon, d.rowcoef = None, rr.data_ptr(), None, None
                d.D, d.dist, d.n_classes = t.numel() // (K * B), spec["dist"][r], t.shape[-1]
                d.scale, d.rescale, d.coef = spec["scale"][r], spec["rescale"][r], 1.0
            call("mvk_recon_nll_fwd", descs, M, K, B, stream_ptr())
        state.lw = [_new((K, B), ref) for _ in range(M)]
        state.w = [_new((K, B), ref) for _ in range(M)]
        state.rowcoef = [_new((K, B), ref) for _ in range(M)]
        loss = _new((), ref)
        masks = spec["masks"]
        marr = ptr_array(masks) if masks[0] is not None else None
        call("mvk_mmvae_objective_fwd", ptr_array(rows), ptr_array(state.lpz), ptr_array(state.lqz), marr, M, K, B,
             int(dreg), ptr_array(state.lw), ptr_array(state.w), ptr_array(state.rowcoef), ptr(loss),
             ptr_array(state.lqw) if state.lqw is not None else None, float(state.beta), stream_ptr())
        ctx.save_for_backward(*recons)
        ctx.state, ctx.spec, ctx.M = state, spec, M
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, gloss):
        recons = ctx.saved_tensors
        st, spec, M = ctx.state, ctx.spec, ctx.M
        K, B = spec["K"], spec["B"]
        st.gloss = _c(gloss.reshape(1))
        grads = []
        descs = (ReconDesc * M)()
        for c in range(M):
            gs = []
            for r in range(M):
                d = descs[r]
                t = recons[c * M + r]
                g = torch.empty_like(t)
                gs.append(g)
                mk = spec["masks"][r]
                d.recon, d.x = t.data_ptr(), spec["x"][r].data_ptr()
                d.mask = mk.data_ptr() if mk is not None else None
                d.rows, d.drecon, d.rowcoef = None, g.data_ptr(), st.rowcoef[c].data_ptr()
                d.D, d.dist, d.n_classes = t.numel() // (K * B), spec["dist"][r], t.shape[-1]
                # lw contains +log p = -NLL, so d loss / d recon = rowcoef * (-1) * rescale * dNLL/drecon
                d.scale, d.rescale, d.coef = spec["scale"][r], spec["rescale"][r], -1.0
            call("mvk_recon_nll_bwd", descs, M, K, B, stream_ptr())
            for g in gs:
                call("mvk_scale_by_device_scalar", ptr(g), g.numel(), ptr(st.gloss), stream_ptr())
            grads += gs
        return (None, None, None, None, *grads)


# =====================================================================================================
# CMVAE: the MMVAE+ latent stage with a mixture over clusters as the prior of the shared latent
# =====================================================================================================
class CMVAELatentFn(Function):
    """(mu_c, std_c)_c, cluster means [C,Ls] and logits [C] -> z_c [K,B,D] for every conditioning modality; fills the
    MMVAEState (lpz with the mixture prior, lqz, lq_all, lqw) for MMVAEObjectiveFn and keeps the responsibilities for the
    backward launch.  Gradients: cluster means, logits, mu_c, std_c; none for the cluster stds and the private prior std
    (cmvae_model.py:100-105, :123-128 fix them)."""

    @staticmethod
    def forward(ctx, state, noises, masks, family, dreg, wprior_std, cluster_stds, cluster_means, cluster_logits, *mus_stds):
        M = len(mus_stds) // 2
        mus = [_c(t) for t in mus_stds[:M]]
        sds = [_c(t) for t in mus_stds[M:]]
        cmean, csd, clogit = _c(cluster_means), _c(cluster_stds), _c(cluster_logits.reshape(-1))
        wsd = _c(wprior_std.reshape(-1))
        K, B, D = noises[0].shape
        C, Ls = cmean.shape
        assert Ls == int(state.shared_dims) and wsd.numel() == D - Ls and csd.shape == cmean.shape and clogit.numel() == C
        zs = _latent_alloc(state, M, K, B, D, mus[0], private=True)
        state.resp = [_new((K, B, C), mus[0]) for _ in range(M)]
        call("mvk_cmvae_latent_fwd", ptr_array(mus), ptr_array(sds), ptr_array(noises), _mask_array(masks), ptr(cmean), ptr(csd),
             ptr(clogit), ptr(wsd), M, K, B, D, family, C, ptr_array(zs), ptr_array(state.lpz), ptr_array(state.lqz),
             ptr_array(state.lq_all), Ls, ptr_array(state.lqw), ptr_array(state.resp), stream_ptr())
        ctx.save_for_backward(cmean, csd, clogit, wsd, *mus, *sds)
        ctx.state, ctx.noises, ctx.masks = state, noises, masks
        ctx.family, ctx.dreg, ctx.M = family, dreg, M
        ctx.logit_shape = cluster_logits.shape
        return tuple(zs)

    @staticmethod
    @once_differentiable
    def backward(ctx, *dzs):
        saved = ctx.saved_tensors
        cmean, csd, clogit, wsd = saved[:4]
        M = ctx.M
        mus, sds = saved[4 : 4 + M], saved[4 + M :]
        st = ctx.state
        K, B, D = ctx.noises[0].shape
        C, Ls = cmean.shape
        dzs = _dz_or_zeros(dzs, st.z)
        dmus = [_new((B, D), mus[0]) for _ in range(M)]
        dsds = [_new((B, D), mus[0]) for _ in range(M)]
        rows = _new((B, C * Ls + C), mus[0])  # per-row terms of d loss / d (means, logits)
        call("mvk_cmvae_latent_bwd", ptr_array(mus), ptr_array(sds), ptr_array(ctx.noises), ptr_array(st.z),
             _mask_array(ctx.masks), ptr(cmean), ptr(csd), ptr(clogit), ptr(wsd), ptr_array(st.w), ptr_array(st.lq_all),
             ptr_array(st.lqz), ptr_array(st.resp), ptr_array(dzs), M, K, B, D, ctx.family, ctx.dreg, C, ptr(st.gloss),
             ptr_array(dmus), ptr_array(dsds), ptr(rows), Ls, float(st.beta), stream_ptr())
        dparams = _sum_rows(rows)
        return (None, None, None, None, None, None, None, dparams[: C * Ls].view(C, Ls), dparams[C * Ls :].view(ctx.logit_shape),
                *dmus, *dsds)


def cmvae_assign(z, cluster_means, cluster_stds, cluster_logits, family, want_lliks=False):
    """Rows z [R,Ls] -> pc_z [C,R], argmax [R] (int64, first maximum), norm_llik [R] or None (mvk_cmvae_assign)."""
    z, cmean, csd, clogit = _c(z), _c(cluster_means), _c(cluster_stds), _c(cluster_logits.reshape(-1))
    R, Ls = z.shape
    C = cmean.shape[0]
    pc = _new((C, R), z)
    amax = torch.empty(R, dtype=torch.int64, device=z.device)
    nll = _new((R,), z) if want_lliks else None
    call("mvk_cmvae_assign", ptr(z), ptr(cmean), ptr(csd), ptr(clogit), R, Ls, family, C, ptr(pc), ptr(amax), ptr(nll),
         stream_ptr())
    return pc, amax, nll


# =====================================================================================================
# Importance-sampled joint likelihood (compute_joint_nll)
# =====================================================================================================
IWAE_ROWS_BUDGET = 1 << 16  # decoder rows (K * data points) per pass of joint_nll


def std_from_logvar(lv, family=FAMILY["normal"]):
    """exp(lv/2) (or the MMVAE scale parametrisations) without an autograd node."""
    lv2 = _c(lv.reshape(-1, lv.shape[-1]))
    sd = torch.empty_like(lv2)
    call("mvk_mmvae_std_fwd", ptr(lv2), lv2.shape[0], lv2.shape[1], family, ptr(sd), stream_ptr())
    return sd.view(lv.shape)


def iwae_sample(loc, sd, noise, family=FAMILY["normal"]):
    """z [K,B,L] = loc + sd * t(noise)."""
    loc, sd, noise = _c(loc), _c(sd), _c(noise)
    K, B, L = noise.shape
    z = torch.empty_like(noise)
    call("mvk_iwae_sample", ptr(loc), ptr(sd), ptr(noise), K, B, L, family, ptr(z), stream_ptr())
    return z


def recon_nll_rows(recons, xs, dists, scales, K, B):
    """Unrescaled, unmasked NLL rows [K,B] of every modality in one mvk_recon_nll_fwd launch (no gradient)."""
    n = len(recons)
    recons = [_c(r) for r in recons]
    descs = (ReconDesc * n)()
    rows = []
    for i in range(n):
        r = _new((K, B), recons[i])
        rows.append(r)
        d = descs[i]
        d.recon, d.x, d.mask, d.rows, d.drecon, d.rowcoef = recons[i].data_ptr(), xs[i].data_ptr(), None, r.data_ptr(), None, None
        d.D, d.dist, d.scale, d.rescale, d.coef = recons[i].numel() // (K * B), dists[i], scales[i], 1.0, 1.0
        d.n_classes = recons[i].shape[-1]
    call("mvk_recon_nll_fwd", descs, n, K, B, stream_ptr())
    return rows


def iwae_logw(z, rows, locs, sds, family=FAMILY["normal"], prior_loc=None, prior_sd=None):
    """lw [K,B] = -sum rows + log p(z) - log mean_e q_e(z)   (mvk_iwae_logw)."""
    z = _c(z)
    K, B, L = z.shape
    locs, sds = [_c(t) for t in locs], [_c(t) for t in sds]
    lw = _new((K, B), z)
    pl = _c(prior_loc.reshape(-1)) if prior_loc is not None else None
    ps = _c(prior_sd.reshape(-1)) if prior_sd is not None else None
    call("mvk_iwae_logw", ptr(z), ptr_array(rows) if rows else None, len(rows), ptr_array(locs), ptr_array(sds),
         len(locs), ptr(pl) if pl is not None else None, ptr(ps) if ps is not None else None, K, B, L, family,
         ptr(lw), stream_ptr())
    return lw


def iwae_reduce(lws, out=None):
    """ll [B] = log-mean-exp over the K rows of every array in lws (mvk_iwae_reduce)."""
    lws = [_c(t) for t in lws]
    K, B = lws[0].shape
    ll = _new((B,), lws[0]) if out is None else out
    call("mvk_iwae_reduce", ptr_array(lws), len(lws), K, B, ptr(ll), stream_ptr())
    return ll


def joint_nll(decode_rows, z, locs, sds, family=FAMILY["normal"], prior_loc=None, prior_sd=None):
    """-sum_b log-mean-exp_k [ log p(x_b | z_kb) + log p(z_kb) - log mean_e q_e(z_kb | x_b) ].

    decode_rows(z_chunk [K,b,L], b0, b1) -> list of [K,b] NLL rows (decoders + recon_nll_rows on data rows b0:b1).
    The data axis is processed in chunks of IWAE_ROWS_BUDGET // K points so that the decoder activations of
    K = 1000 samples stay bounded; every chunk is independent (the estimate is per data point).
    """
    K, B, L = z.shape
    ll = _new((B,), z)
    step = max(1, IWAE_ROWS_BUDGET // max(K, 1))
    for b0 in range(0, B, step):
        b1 = min(B, b0 + step)
        zc = z[:, b0:b1].contiguous()
        rows = decode_rows(zc, b0, b1)
        lw = iwae_logw(zc, rows, [t[b0:b1] for t in locs], [t[b0:b1] for t in sds], family, prior_loc, prior_sd)
        iwae_reduce([lw], out=ll[b0:b1])
    return -ll.sum()


# =====================================================================================================
# Gaussian-mixture EM (samplers.GaussianMixtureSampler)
# =====================================================================================================
def gmm_scratch(L, n_comp, device):
    """The caller-owned scratch of the mvk_gmm_* entry points for (L, n_comp): its size does not depend on N."""
    n = C.c_int64(0)
    call("mvk_gmm_scratch_bytes", L, n_comp, C.byref(n))
    return torch.empty((n.value + 7) // 8, dtype=torch.float64, device=device)


def gmm_new_params(L, n_comp, device):
    """Uninitialised parameter buffers of one mixture: weights [C], means [C,L], covs, cov_chol, prec_chol [C,L,L], logdet [C]."""
    f = dict(dtype=torch.float32, device=device)
    return dict(weights=torch.empty(n_comp, **f), means=torch.empty(n_comp, L, **f), covs=torch.empty(n_comp, L, L, **f),
                cov_chol=torch.empty(n_comp, L, L, **f), prec_chol=torch.empty(n_comp, L, L, **f), logdet=torch.empty(n_comp, **f))


def gmm_estep(x, p, resp, scratch, row_out=None, lb=None):
    """resp [N,C] = responsibilities of the rows of x under the mixture p; row_out [N] = logsumexp rows, lb (1 double) = their
    mean (mvk_gmm_estep, soft)."""
    N, L = x.shape
    call("mvk_gmm_estep", ptr(x), N, L, p["means"].shape[0], ptr(p["weights"]), ptr(p["means"]), ptr(p["prec_chol"]),
         ptr(p["logdet"]), 0, ptr(resp), ptr(row_out), None, None, ptr(lb), ptr(scratch), stream_ptr())


def gmm_estep_hard(x, means, resp, scratch, row_out=None, labels=None, changed=None):
    """resp [N,C] = one-hot of the nearest of the rows of `means`; row_out [N] = that squared distance; labels [N] int32 in / out,
    changed (1 int32) = rows whose label changed (mvk_gmm_estep, hard)."""
    N, L = x.shape
    call("mvk_gmm_estep", ptr(x), N, L, means.shape[0], None, ptr(means), None, None, 1, ptr(resp), ptr(row_out), ptr(labels),
         ptr(changed), None, ptr(scratch), stream_ptr())


def gmm_mstep(x, resp, p, reg_covar, scratch, means_only=False):
    """The parameters p from the responsibilities (mvk_gmm_mstep); means_only: p["means"] alone (Lloyd's update)."""
    N, L = x.shape
    call("mvk_gmm_mstep", ptr(x), ptr(resp), N, L, p["means"].shape[0], float(reg_covar), int(means_only), ptr(p["weights"]),
         ptr(p["means"]), ptr(p["covs"]), ptr(p["cov_chol"]), ptr(p["prec_chol"]), ptr(p["logdet"]), ptr(scratch), stream_ptr())


def gmm_em_step(x, p, resp, state, reg_covar, tol, scratch):
    """One guarded EM iteration on the device state block (mvk_gmm_em_step): a no-op once state says converged or failed."""
    N, L = x.shape
    call("mvk_gmm_em_step", ptr(x), N, L, p["means"].shape[0], float(reg_covar), float(tol), ptr(p["weights"]), ptr(p["means"]),
         ptr(p["covs"]), ptr(p["cov_chol"]), ptr(p["prec_chol"]), ptr(p["logdet"]), ptr(resp), ptr(state), ptr(scratch),
         stream_ptr())


def gmm_new_state(device):
    """The state block before the first step: lower bound -inf, everything else 0."""
    st = torch.zeros(_lib.GMM_STATE_DOUBLES, dtype=torch.float64, device=device)
    st[_lib.GMM_STATE["lb"]] = -math.inf
    return st


def gmm_sample(means, cov_chol, comp, eps):
    """z [n,L] = means[comp] + cov_chol[comp] @ eps (mvk_gmm_sample); comp [n] int32."""
    n, L = eps.shape
    z = torch.empty_like(eps)
    call("mvk_gmm_sample", ptr(means), ptr(cov_chol), ptr(comp), ptr(eps), n, L, means.shape[0], ptr(z), stream_ptr())
    return z


# =====================================================================================================
# Batched k-means (metrics.Clustering)
# =====================================================================================================
def kmeans_scratch(L, n_clusters, n_runs, device):
    """The caller-owned scratch of the mvk_kmeans_* entry points for (L, n_clusters, n_runs): its size does not depend on N."""
    n = C.c_int64(0)
    call("mvk_kmeans_scratch_bytes", L, n_clusters, n_runs, C.byref(n))
    return torch.empty((n.value + 7) // 8, dtype=torch.float64, device=device)


def kmeans_new_state(n_runs, device):
    """The state blocks [R, 8] before the first step: all 0 (the labels of the first step are -1)."""
    return torch.zeros(n_runs, _lib.KMEANS_STATE_DOUBLES, dtype=torch.float64, device=device)


def kmeans_assign(x, centers, scratch=None, labels=None, d2=None, y=None, n_classes=0, table=None, majority=None, correct=None,
                  inertia=None):
    """Nearest centre of every row of x [N,L] for every run of centers [R,K,L] (mvk_kmeans_assign): labels [R,N] int32, d2 [R,N],
    inertia [R] float64 (needs scratch); with y [N] int32: table [R,K,n_classes+1] int64 += the contingency counts, correct [R]
    int64 += rows with majority[r, label] == y.  Every output is optional."""
    N, L = x.shape
    R, K, _ = centers.shape
    call("mvk_kmeans_assign", ptr(x), N, L, K, R, ptr(centers), ptr(labels), ptr(d2), ptr(y), int(n_classes), ptr(table),
         ptr(majority), ptr(correct), ptr(inertia), ptr(scratch), stream_ptr())


def kmeans_step(x, tol, centers, labels, state, scratch):
    """One guarded Lloyd iteration of every run (mvk_kmeans_step): a no-op for a run whose state says converged.  tol is a DEVICE
    float64 scalar."""
    N, L = x.shape
    R, K, _ = centers.shape
    call("mvk_kmeans_step", ptr(x), N, L, K, R, ptr(tol), ptr(centers), ptr(labels), ptr(state), ptr(scratch), stream_ptr())


def kmeans_vote(table, majority):
    """majority [R,K] int32 = the first maximum of table [R,K,n_classes+1] over the real classes; a cluster without a row in one
    maps to its own index (mvk_kmeans_vote)."""
    R, K, C1 = table.shape
    call("mvk_kmeans_vote", ptr(table), R, K, C1 - 1, ptr(majority), stream_ptr())


# =====================================================================================================
# SSIM / squared error of image batches (metrics.Reconstruction)
# =====================================================================================================
def ssim_tile():
    """The tile edge, in window positions, of the SSIM rows kernel (mvk_ssim_tile)."""
    return _lib.load().mvk_ssim_tile()


def ssim_scratch(B, Cc, H, W, device):
    """The caller-owned scratch of ssim_range / ssim_rows for a [B,Cc,H,W] update (mvk_ssim_scratch_bytes)."""
    n = C.c_int64(0)
    call("mvk_ssim_scratch_bytes", B, Cc, H, W, C.byref(n))
    return torch.empty((n.value + 7) // 8, dtype=torch.float64, device=device)


def ssim_new_acc(device):
    """The running {ssim_sum, sse_sum, rows} block of ssim_accumulate, zeroed."""
    return torch.zeros(_lib.SSIM_ACC_DOUBLES, dtype=torch.float64, device=device)


def ssim_range(preds, target, scratch, out=None):
    """The data range R of one update as a 1-element device tensor (mvk_ssim_range): no host read."""
    out = torch.empty(1, dtype=torch.float32, device=preds.device) if out is None else out
    call("mvk_ssim_range", ptr(preds), ptr(target), preds.numel(), ptr(out), ptr(scratch), stream_ptr())
    return out


def ssim_rows(preds, target, scratch, data_range=None, ssim_out=None, sse_out=None):
    """Per-image SSIM [B] and per-image sum of squared differences [B] of preds, target [B,Cc,H,W] (mvk_ssim_rows).  data_range:
    a 1-element device tensor (read on the device), a Python float (passed by value), or None (ssim_range is run first)."""
    B, Cc, H, W = preds.shape
    f = dict(dtype=torch.float32, device=preds.device)
    ssim_out = torch.empty(B, **f) if ssim_out is None else ssim_out
    sse_out = torch.empty(B, **f) if sse_out is None else sse_out
    if data_range is None:
        data_range = ssim_range(preds, target, scratch)
    by_value = not torch.is_tensor(data_range)
    call("mvk_ssim_rows", ptr(preds), ptr(target), B, Cc, H, W, None if by_value else ptr(data_range),
         float(data_range) if by_value else 0.0, 0, ptr(ssim_out), ptr(sse_out), ptr(scratch), stream_ptr())
    return ssim_out, sse_out


def sse_rows(preds, target, sse_out=None):
    """Per-row sum of squared differences [B] of two [B, ...] tensors: the window-free path of mvk_ssim_rows."""
    B = preds.shape[0]
    if preds.numel() // B >= 2 ** 31:
        raise _lib.MvkError("sse_rows: rows of 2^31 elements or more")
    sse_out = torch.empty(B, dtype=torch.float32, device=preds.device) if sse_out is None else sse_out
    call("mvk_ssim_rows", ptr(preds), ptr(target), B, 1, 1, preds.numel() // B, None, 0.0, 1, None, ptr(sse_out), None,
         stream_ptr())
    return sse_out


def ssim_accumulate(acc, sse, ssim=None):
    """acc += {sum of ssim, sum of sse, rows} in index order in fp64 on the device (mvk_ssim_accumulate)."""
    call("mvk_ssim_accumulate", ptr(ssim), ptr(sse), sse.shape[0], ptr(acc), stream_ptr())


# =====================================================================================================
# Streaming Frechet statistics (metrics.FIDEvaluator)
# =====================================================================================================
def fd_tile():
    """The tile edge of the second-moment matrix of the Frechet-statistics kernel (mvk_fd_tile)."""
    return _lib.load().mvk_fd_tile()


def fd_chunk():
    """The rows of a call that the Frechet-statistics kernel walks at a time (mvk_fd_chunk)."""
    return _lib.load().mvk_fd_chunk()


def fd_new_state(D, device):
    """The caller-owned state of the mvk_fd_* entry points for two streams of width D (mvk_fd_state_bytes); fd_begin zeroes it."""
    n = C.c_int64(0)
    call("mvk_fd_state_bytes", D, C.byref(n))
    return torch.empty((n.value + 7) // 8, dtype=torch.float64, device=device)


def fd_begin(state, x0, x1=None):
    """Zero the state and set each stream's shift to the column mean of its rows (mvk_fd_begin): x0, x1 [n,D] fp32 are the FIRST
    batch of the real and of the generated stream; no row is added.  x1 = None leaves stream 1 empty."""
    n, D = x0.shape
    call("mvk_fd_begin", ptr(x0), ptr(x1), n, D, ptr(state), stream_ptr())


def fd_update(state, x0, x1=None):
    """Add the n rows of x0 to stream 0 and of x1 (unless None) to stream 1 in one launch (mvk_fd_update): no host read."""
    n, D = x0.shape
    call("mvk_fd_update", ptr(x0), ptr(x1), n, D, ptr(state), stream_ptr())


def fd_finish(state, D, mean=None, cov=None, terms=None):
    """mean [2,D], cov [2,D,D] (np.cov(rowvar=False), exactly symmetric) and terms [5] = {|mean0 - mean1|^2, tr cov0, tr cov1,
    n0, n1}, all float64 on the device (mvk_fd_finish); the state is left as it was."""
    f = dict(dtype=torch.float64, device=state.device)
    mean = torch.empty(2, D, **f) if mean is None else mean
    cov = torch.empty(2, D, D, **f) if cov is None else cov
    terms = torch.empty(_lib.FD_TERMS, **f) if terms is None else terms
    call("mvk_fd_finish", ptr(state), D, ptr(mean), ptr(cov), ptr(terms), stream_ptr())
    return mean, cov, terms


# =====================================================================================================
# PolyMNIST classifier (metrics.classifiers.ClassifierPolyMNIST, metrics.CoherenceEvaluator)
# =====================================================================================================
POLYCLF_SHAPES = ((10, 3, 4, 4), (10,), (20, 10, 4, 4), (20,), (128, 980), (128,), (10, 128), (10,))


def polyclf_tile():
    """Images per workgroup of the fused classifier launch (mvk_polyclf_tile)."""
    return _lib.load().mvk_polyclf_tile()


def polyclf_forward(x, params, logits=None, pred=None, labels=None, counts=None):
    """The PolyMNIST classifier in eval mode on x [n,3,28,28] fp32 in one launch (mvk_polyclf_fwd).  params: the eight parameters
    (conv1 w, b, conv2 w, b, fc1 w, b, fc2 w, b) in PyTorch's layouts, read in place.  Outputs, each optional: logits [n,10] fp32,
    pred [n] int32 (torch.argmax), counts [11,2] int64 += the (correct, count) pairs of ClassCounts.update under
    labels[i % len(labels)] (int64).  With no output given, logits are allocated and returned."""
    _lib.require_gpu_tensor(x, "x")
    if x.dim() != 4 or tuple(x.shape[1:]) != (3, 28, 28) or not x.is_contiguous():
        raise ValueError(f"polyclf_forward: x must be a contiguous [n,3,28,28] tensor, got {tuple(x.shape)}")
    if len(params) != 8:
        raise ValueError("polyclf_forward: eight parameters (conv1, conv2, fc1, fc2: weight and bias)")
    for p, shape in zip(params, POLYCLF_SHAPES):
        _lib.require_gpu_tensor(p, "a classifier parameter")
        if tuple(p.shape) != shape or not p.is_contiguous() or p.device != x.device:
            raise ValueError(f"polyclf_forward: a contiguous parameter of shape {shape} on {x.device}, got {tuple(p.shape)} on {p.device}")
    n = x.shape[0]
    if logits is None and pred is None and counts is None:
        logits = torch.empty(n, 10, dtype=torch.float32, device=x.device)
    for t, name, dtype, shape in ((logits, "logits", torch.float32, (n, 10)), (pred, "pred", torch.int32, (n,)),
                                  (counts, "counts", torch.int64, (11, 2))):
        if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != x.device):
            raise ValueError(f"polyclf_forward: {name} must be a contiguous {dtype} tensor of shape {shape} on {x.device}")
    label_rows = 0
    if labels is not None:
        if labels.dtype != torch.int64 or labels.dim() != 1 or not labels.is_contiguous() or labels.device != x.device:
            raise ValueError(f"polyclf_forward: labels must be a contiguous 1-d int64 tensor on {x.device}")
        label_rows = labels.shape[0]
    if n == 0:  # nothing to classify (an empty tensor has no address to hand over)
        return logits
    call("mvk_polyclf_fwd", ptr(x), n, *[ptr(p) for p in params], ptr(logits), ptr(pred), ptr(labels), label_rows, ptr(counts),
         stream_ptr())
    return logits


# =====================================================================================================
# Masked autoregressive flows (models/nn/flows.py; JNF)
# =====================================================================================================
def maf_fused_ok(D, H, n_hidden, n_blocks, M=1):
    """The shapes mvk_maf_fwd/bwd/inverse take (mvk.h MVK_MAF_MAX_*): anything else runs the torch flow modules.  At the sizes that
    were timed (D = 20, H = 128: profiles/NOTES_jnf.md; D = 20 and 64 as a sampler's fit step and inverse:
    profiles/NOTES_flow_samplers.md) all three fused entries are ahead of the modules; other shapes were not timed, so the range is
    what the kernels can run."""
    return (2 <= D <= _lib.MAF_MAX_DIM and 1 <= H <= _lib.MAF_MAX_DIM and 1 <= n_hidden <= _lib.MAF_MAX_HIDDEN
            and 1 <= n_blocks <= _lib.MAF_MAX_BLOCKS and 1 <= M <= _lib.MAX_MODALITIES)


def _maf_check(dims, Ws, bs, M):
    n_blocks, n_hidden, D, H = dims
    if not maf_fused_ok(D, H, n_hidden, n_blocks, M):
        raise ValueError(f"maf: (D, H, hidden layers, blocks, flows) = {(D, H, n_hidden, n_blocks, M)} is outside the fused range")
    nl = n_hidden + 1
    if len(Ws) != M * n_blocks * nl or len(bs) != len(Ws):
        raise ValueError(f"maf: expected {M * n_blocks * nl} weights and biases, got {len(Ws)} and {len(bs)}")
    for i, (w, b) in enumerate(zip(Ws, bs)):
        l = i % nl
        shape = (H, D) if l == 0 else (2 * D, H) if l == n_hidden else (H, H)
        if tuple(w.shape) != shape or tuple(b.shape) != shape[:1]:
            raise ValueError(f"maf: layer {l} holds {tuple(w.shape)} / {tuple(b.shape)}, expected {shape} / {shape[:1]}")
        _lib.require_gpu_tensor(w)
        _lib.require_gpu_tensor(b)
        if not (w.is_contiguous() and b.is_contiguous()):
            raise ValueError("maf: weights and biases must be contiguous (they are read in place)")


def maf_forward(z, dims, Ws, bs, mus=None, lvs=None, keep=True):
    """All M flows of z [B,D] in one launch (mvk_maf_fwd).  dims = (n_blocks, n_hidden, D, H); Ws, bs: the M * n_blocks *
    (n_hidden + 1) masked-linear weights and biases, flow-major.  -> z0 [M,B,D], ladj [M,B], rows [M,B] (None without the
    posteriors mus / lvs), ws (what maf_backward needs; None with keep=False)."""
    n_blocks, n_hidden, D, H = dims
    M = len(Ws) // (n_blocks * (n_hidden + 1)) if n_blocks * (n_hidden + 1) else 0
    _maf_check(dims, Ws, bs, M)
    z = _c(z)
    B = z.shape[0]
    if tuple(z.shape) != (B, D):
        raise ValueError(f"maf_forward: z is {tuple(z.shape)}, expected [B, {D}]")
    if mus is not None:
        mus, lvs = [_c(t) for t in mus], [_c(t) for t in lvs]
        if len(mus) != M or len(lvs) != M or any(tuple(t.shape) != (B, D) for t in [*mus, *lvs]):
            raise ValueError(f"maf_forward: expected {M} means and log-variances of shape [{B}, {D}]")
    z0, ladj = _new((M, B, D), z), _new((M, B), z)
    rows = _new((M, B), z) if mus is not None else None
    ws = _new((M * n_blocks * B * (2 * D + n_hidden * H),), z) if keep else None
    call("mvk_maf_fwd", ptr(z), ptr_array(Ws), ptr_array(bs), M, n_blocks, n_hidden, D, H,
         None if mus is None else ptr_array(mus), None if mus is None else ptr_array(lvs), B, ptr(z0), ptr(ladj), ptr(rows),
         ptr(ws), stream_ptr())
    return z0, ladj, rows, ws


def maf_backward(dims, Ws, z0, ws, mus=None, lvs=None, grows=None, dz0=None, dladj=None, want_dz=False, dWs=None, dbs=None):
    """The backward of maf_forward (mvk_maf_bwd): one launch for the data gradients, one more when dWs / dbs (lists of
    accumulation targets, None entries skipped) are given.  -> dmus, dlvs (lists, None without posteriors), dz [B,D] or None."""
    n_blocks, n_hidden, D, H = dims
    M, B = z0.shape[0], z0.shape[1]
    dmus = dlvs = None
    if mus is not None:
        dmus, dlvs = [_new((B, D), z0) for _ in range(M)], [_new((B, D), z0) for _ in range(M)]
    dz = _new((B, D), z0) if want_dz else None
    want_w = dWs is not None and any(t is not None for t in [*dWs, *(dbs or [])])
    deltas = torch.empty_like(ws) if want_w else None
    call("mvk_maf_bwd", ptr_array(Ws), M, n_blocks, n_hidden, D, H, None if mus is None else ptr_array(mus),
         None if mus is None else ptr_array(lvs), ptr(z0), ptr(ws), ptr(grows), ptr(dz0), ptr(dladj), B,
         None if mus is None else ptr_array(dmus), None if mus is None else ptr_array(dlvs), ptr(dz), ptr(deltas),
         ptr_array(dWs) if want_w else None, ptr_array(dbs) if want_w else None, stream_ptr())
    return dmus, dlvs, dz


def maf_inverse(y, dims, Ws, bs, want_ladj=False):
    """x with flow(x) = y for ONE flow, y [R,D], in one launch (mvk_maf_inverse) -> x [R,D], ladj [R] or None."""
    n_blocks, n_hidden, D, H = dims
    _maf_check(dims, Ws, bs, 1)
    y = _c(y)
    R = y.shape[0]
    if tuple(y.shape) != (R, D):
        raise ValueError(f"maf_inverse: y is {tuple(y.shape)}, expected [R, {D}]")
    x = _new((R, D), y)
    ladj = _new((R,), y) if want_ladj else None
    call("mvk_maf_inverse", ptr(y), ptr_array(Ws), ptr_array(bs), n_blocks, n_hidden, D, H, R, ptr(x), ptr(ladj), stream_ptr())
    return x, ladj


class MAFFlowsFn(Function):
    """The M masked autoregressive flows of JNF on one shared input, forward in one launch and backward in two.
    apply(dims, with_post, z, *tensors): dims = (n_blocks, n_hidden, D, H); z [B,D]; tensors = with_post ? (mu0_0..mu0_{M-1},
    lv0_0..lv0_{M-1}) : (), then W, b of every layer, flow-major (the parameters themselves: their gradients accumulate the way
    linear_bwd_weight's do, _grad_target).  -> rows [M,B] (None without posteriors), z0 [M,B,D], ladj [M,B];
    rows[m,b] = -(sum_l log N(z0; mu0_m, exp(lv0_m / 2)) + ladj): the stage-two term of jnf_model.py:165-183."""

    @staticmethod
    def forward(ctx, dims, with_post, z, *tensors):
        n_blocks, n_hidden, D, H = dims
        nl = n_blocks * (n_hidden + 1)
        n_post = 0
        if with_post:
            M = len(tensors) // (2 + 2 * nl)
            n_post = 2 * M
        params = tensors[n_post:]
        Ws, bs = list(params[0::2]), list(params[1::2])
        mus = [_c(t) for t in tensors[: n_post // 2]] if with_post else None
        lvs = [_c(t) for t in tensors[n_post // 2 : n_post]] if with_post else None
        z = _c(z)
        z0, ladj, rows, ws = maf_forward(z, dims, Ws, bs, mus, lvs)
        ctx.dims, ctx.with_post, ctx.n_post = dims, with_post, n_post
        ctx.save_for_backward(z0, ws, *(mus or []), *(lvs or []), *params)
        ctx.set_materialize_grads(False)
        return rows, z0, ladj

    @staticmethod
    @once_differentiable
    def backward(ctx, grows, dz0, dladj):
        saved = ctx.saved_tensors
        z0, ws = saved[0], saved[1]
        schedule.wait_loss(z0.device)
        schedule.late_ready(z0.device)
        n_post = ctx.n_post
        M = z0.shape[0]
        mus = list(saved[2 : 2 + M]) if ctx.with_post else None
        lvs = list(saved[2 + M : 2 + n_post]) if ctx.with_post else None
        params = saved[2 + n_post :]
        need = ctx.needs_input_grad
        n_out = 3 + n_post + len(params)
        if grows is None and dz0 is None and dladj is None:
            return (None,) * n_out
        Ws = list(params[0::2])
        targets, rets = [], []
        for i, p in enumerate(params):
            t, r = _grad_target(p) if need[3 + n_post + i] else (None, None)
            targets.append(t)
            rets.append(r)
        dmus, dlvs, dz = maf_backward(ctx.dims, Ws, z0, ws, mus, lvs, None if grows is None else _c(grows),
                                      None if dz0 is None else _c(dz0), None if dladj is None else _c(dladj),
                                      want_dz=need[2], dWs=targets[0::2], dbs=targets[1::2])
        return (None, None, dz, *(dmus or []), *(dlvs or []), *rets)


# =====================================================================================================
# Inverse autoregressive flow (models/nn/flows.py; the flow samplers)
# =====================================================================================================
def iaf_fused_ok(D, H, n_hidden, n_blocks):
    """The shapes mvk_iaf_fwd/bwd/inverse take: those of maf_fused_ok for one flow; anything else runs the torch IAF module.  At the
    sizes that were timed (D = 20 and 64, H = 128, 3 hidden layers, 2 blocks: profiles/NOTES_flow_samplers.md) the fit step and the
    inverse are ahead of the module; other shapes were not timed, so the range is what the kernels can run."""
    return maf_fused_ok(D, H, n_hidden, n_blocks, 1)


def iaf_forward(x, dims, Ws, bs, want_rows=False, keep=True):
    """ONE inverse autoregressive flow of x [B,D] in one launch (mvk_iaf_fwd).  dims = (n_blocks, n_hidden, D, H); Ws, bs: the
    n_blocks * (n_hidden + 1) masked-linear weights and biases.  -> z0 [B,D], ladj [B], rows [B] (the NLL under N(0, I); None
    unless want_rows), ws (what iaf_backward needs; None with keep=False)."""
    n_blocks, n_hidden, D, H = dims
    _maf_check(dims, Ws, bs, 1)
    x = _c(x)
    B = x.shape[0]
    if tuple(x.shape) != (B, D):
        raise ValueError(f"iaf_forward: x is {tuple(x.shape)}, expected [B, {D}]")
    z0, ladj = _new((B, D), x), _new((B,), x)
    rows = _new((B,), x) if want_rows else None
    ws = _new((n_blocks * B * (2 * D + n_hidden * H),), x) if keep else None
    call("mvk_iaf_fwd", ptr(x), ptr_array(Ws), ptr_array(bs), n_blocks, n_hidden, D, H, B, ptr(z0), ptr(ladj), ptr(rows), ptr(ws),
         stream_ptr())
    return z0, ladj, rows, ws


def iaf_backward(dims, Ws, z0, ws, grows=None, dz0=None, dladj=None, want_dx=False, dWs=None, dbs=None, deltas=None):
    """The backward of iaf_forward (mvk_iaf_bwd): one launch for the data gradient and the layers' deltas, one more when dWs / dbs
    (lists of accumulation targets, None entries skipped) are given.  deltas: a buffer the size of ws to reuse.  -> dx [B,D] or
    None."""
    n_blocks, n_hidden, D, H = dims
    B = z0.shape[0]
    dx = _new((B, D), z0) if want_dx else None
    want_w = dWs is not None and any(t is not None for t in [*dWs, *(dbs or [])])
    if want_w and deltas is None:
        deltas = torch.empty_like(ws)
    call("mvk_iaf_bwd", ptr_array(Ws), n_blocks, n_hidden, D, H, ptr(z0), ptr(ws), ptr(grows), ptr(dz0), ptr(dladj), B, ptr(dx),
         ptr(deltas) if want_w else None, ptr_array(dWs) if want_w else None, ptr_array(dbs) if want_w else None, stream_ptr())
    return dx


def iaf_inverse(y, dims, Ws, bs, want_ladj=False):
    """x with flow(x) = y, y [R,D], in one launch and one MADE pass per block (mvk_iaf_inverse) -> x [R,D], ladj [R] or None."""
    n_blocks, n_hidden, D, H = dims
    _maf_check(dims, Ws, bs, 1)
    y = _c(y)
    R = y.shape[0]
    if tuple(y.shape) != (R, D):
        raise ValueError(f"iaf_inverse: y is {tuple(y.shape)}, expected [R, {D}]")
    x = _new((R, D), y)
    ladj = _new((R,), y) if want_ladj else None
    call("mvk_iaf_inverse", ptr(y), ptr_array(Ws), ptr_array(bs), n_blocks, n_hidden, D, H, R, ptr(x), ptr(ladj), stream_ptr())
    return x, ladj


class IAFFlowFn(Function):
    """One inverse autoregressive flow, forward in one launch and backward in two.  apply(dims, x, *params): dims = (n_blocks,
    n_hidden, D, H); x [B,D]; params = W, b of every layer in order (the parameters themselves: their gradients accumulate the way
    MAFFlowsFn's do, _grad_target).  -> rows [B] (the NLL under N(0, I)), z0 [B,D], ladj [B]."""

    @staticmethod
    def forward(ctx, dims, x, *params):
        Ws, bs = list(params[0::2]), list(params[1::2])
        z0, ladj, rows, ws = iaf_forward(x, dims, Ws, bs, want_rows=True)
        ctx.dims = dims
        ctx.save_for_backward(z0, ws, *params)
        ctx.set_materialize_grads(False)
        return rows, z0, ladj

    @staticmethod
    @once_differentiable
    def backward(ctx, grows, dz0, dladj):
        saved = ctx.saved_tensors
        z0, ws, params = saved[0], saved[1], saved[2:]
        schedule.wait_loss(z0.device)
        schedule.late_ready(z0.device)
        need = ctx.needs_input_grad
        if grows is None and dz0 is None and dladj is None:
            return (None,) * (2 + len(params))
        targets, rets = [], []
        for i, p in enumerate(params):
            t, r = _grad_target(p) if need[2 + i] else (None, None)
            targets.append(t)
            rets.append(r)
        dx = iaf_backward(ctx.dims, list(params[0::2]), z0, ws, None if grows is None else _c(grows),
                          None if dz0 is None else _c(dz0), None if dladj is None else _c(dladj), want_dx=need[1],
                          dWs=targets[0::2], dbs=targets[1::2])
        return (None, dx, *rets)


# =====================================================================================================
# CUB text encoder  (models/nn/cub.py CubTextEncoder; csrc/textenc.hip, include/mvk.h "CUB text encoder")
# =====================================================================================================
def text_encoder_ok(B, S, E, nhead, F):
    """Whether the fused text-encoder path covers this shape (mvk_txt_attn_*: S <= 64, head_dim <= 128)."""
    return bool(B >= 1 and 1 <= S <= _lib.TXT_MAX_SEQ and nhead >= 1 and E >= nhead and E % nhead == 0
                and E // nhead <= _lib.TXT_MAX_HEAD_DIM and F >= 1)


def text_noise_layout(B, S, E, nhead, F, n_layers):
    """(floats of one forward's dropout noise, offset of the positional site, [(attn, res1, ff, res2) offsets per layer]):
    pos [B,S,E], then per layer attn [B,nhead,S,S], res1 [B,S,E], ff [B,S,F], res2 [B,S,E] (include/mvk.h)."""
    off, layers = B * S * E, []
    for _ in range(n_layers):
        a = off
        r1 = a + B * nhead * S * S
        f = r1 + B * S * E
        r2 = f + B * S * F
        off = r2 + B * S * E
        layers.append((a, r1, f, r2))
    return off, 0, layers


def _txt_site(noise, off, n, p):
    """The noise of one dropout site (None: no dropout there)."""
    return None if noise is None or p == 0 else noise[off:off + n]


def txt_embed_fwd(tokens, emb, pe, noise=None, p=0.0):
    """drop(emb[tokens] * sqrt(E) + pe[:S]) -> [B,S,E] (mvk_txt_embed_fwd).  tokens int64 [B,S]; pe [>= S,E]."""
    B, S = tokens.shape
    V, E = emb.shape
    out = _new((B, S, E), emb)
    call("mvk_txt_embed_fwd", ptr(tokens), ptr(emb), ptr(pe), ptr(noise), float(p), ptr(out), B, S, E, V, stream_ptr())
    return out


def txt_embed_bwd(tokens, g, V, g2=None, noise=None, p=0.0, out=None):
    """The embedding table's gradient [V,E] (mvk_txt_embed_bwd); out: a buffer to accumulate into."""
    B, S = tokens.shape
    E = g.shape[-1]
    dE = out if out is not None else _new((V, E), g)
    call("mvk_txt_embed_bwd", ptr(tokens), ptr(g), ptr(g2), ptr(noise), float(p), ptr(dE), 1 if out is not None else 0, B, S, E, V,
         stream_ptr())
    return dE


def txt_attn_fwd(qkv, nhead, keymask=None, noise=None, p=0.0, keep=True):
    """Masked self-attention of every (sentence, head) from the packed qkv [B,S,3E] -> (ctx [B,S,E], P [B,nhead,S,S] before
    dropout, or None) (mvk_txt_attn_fwd).  keymask int32 [B,S], 1 = real key."""
    B, S, E3 = qkv.shape
    E = E3 // 3
    ctx = _new((B, S, E), qkv)
    P = _new((B, nhead, S, S), qkv) if keep else None
    call("mvk_txt_attn_fwd", ptr(qkv), ptr(keymask), ptr(noise), float(p), ptr(P), ptr(ctx), B, S, E, nhead, stream_ptr())
    return ctx, P


def txt_attn_bwd(qkv, P, dctx, nhead, noise=None, p=0.0):
    """dqkv [B,S,3E] (mvk_txt_attn_bwd)."""
    B, S, E3 = qkv.shape
    dqkv = _new((B, S, E3), qkv)
    call("mvk_txt_attn_bwd", ptr(qkv), ptr(P), ptr(dctx), ptr(noise), float(p), ptr(dqkv), B, S, E3 // 3, nhead, stream_ptr())
    return dqkv


def txt_add_ln_fwd(x, t, gamma, beta, eps, noise=None, p=0.0, rowmask=None, zero_pads=False, keep=True, z_in_t=False):
    """y = LN(x + drop(t)) gamma + beta over the last axis -> (y, z, mean, rstd) (mvk_txt_add_ln_fwd); z, mean, rstd are None
    without keep; z_in_t: z overwrites t."""
    E = x.shape[-1]
    rows = x.numel() // E
    y = _new(x.shape, x)
    z = (t if z_in_t else _new(x.shape, x)) if keep else None
    mean = _new((rows,), x) if keep else None
    rstd = _new((rows,), x) if keep else None
    call("mvk_txt_add_ln_fwd", ptr(x), ptr(t), ptr(noise), float(p), ptr(gamma), ptr(beta), float(eps), ptr(rowmask),
         1 if zero_pads else 0, ptr(y), ptr(z), ptr(mean), ptr(rstd), rows, E, stream_ptr())
    return y, z, mean, rstd


def txt_add_ln_bwd(dy, z, mean, rstd, gamma, dy2=None, noise=None, p=0.0, want_dt=True, dgamma=None, dbeta=None):
    """-> (dx, dt) of y = LN(x + drop(t)) gamma + beta for the upstream gradient dy + dy2; dgamma / dbeta (buffers or None)
    are accumulated into (mvk_txt_add_ln_bwd).  Without dropout dt is dx itself."""
    E = dy.shape[-1]
    rows = dy.numel() // E
    dx = _new(dy.shape, dy)
    dropped = noise is not None and p > 0
    dt = _new(dy.shape, dy) if want_dt and dropped else None
    ws = _new((2 * E * ((rows + 63) // 64),), dy) if dgamma is not None or dbeta is not None else None
    call("mvk_txt_add_ln_bwd", ptr(dy), ptr(dy2), ptr(z), ptr(mean), ptr(rstd), ptr(gamma), ptr(noise), float(p), ptr(dx), ptr(dt),
         ptr(dgamma), ptr(dbeta), ptr(ws), 0 if ws is None else ws.numel(), rows, E, stream_ptr())
    return dx, (dt if dropped or not want_dt else dx)


def txt_drop(x, noise=None, p=0.0):
    """x = keep * x / (1 - p) in place (mvk_txt_drop)."""
    call("mvk_txt_drop", ptr(x), ptr(noise), float(p), x.numel(), stream_ptr())
    return x


TXT_LAYER_PARAMS = 12  # in_proj w, b; out_proj w, b; linear1 w, b; linear2 w, b; norm1 w, b; norm2 w, b


class TextEncoderFn(Function):
    """tokens -> embedding + positions -> n post-norm transformer encoder layers -> [B,S,E], one node.
    apply(tokens, padding_mask, p, noise, zero_pads, nhead, eps, emb, pe, *layer params): tokens int64 [B,S]; padding_mask [B,S]
    (non-zero = real token) or None; p the dropout rate and noise the flat U[0,1) buffer of text_noise_layout (None: no dropout);
    zero_pads: the output is 0 at padded positions (evaluation without autograd only); eps the LayerNorm epsilon; emb [V,E];
    pe [>= S,E]; then TXT_LAYER_PARAMS parameters per layer.  The five GEMM sites of a layer are the tiled engine's, the other
    stages csrc/textenc.hip; the backward re-reads the noise and keeps no mask."""

    @staticmethod
    def forward(ctx, tokens, padding_mask, p, noise, zero_pads, nhead, eps, emb, pe, *params):
        n_layers = len(params) // TXT_LAYER_PARAMS
        B, S = tokens.shape
        V, E = emb.shape
        F = params[4].shape[0]
        if not text_encoder_ok(B, S, E, nhead, F) or len(params) != n_layers * TXT_LAYER_PARAMS:
            raise _lib.MvkError(f"TextEncoderFn: shape B={B} S={S} E={E} nhead={nhead} F={F} is not covered")
        _lib.require_gpu_tensor(emb, "emb")
        p = float(p)
        if noise is None or p == 0:
            noise, p = None, 0.0
        keep = any(ctx.needs_input_grad) and not zero_pads  # zero_pads: evaluation without autograd, nothing is kept
        total, pos_off, offs = text_noise_layout(B, S, E, nhead, F, n_layers)
        if noise is not None and (noise.numel() < total or noise.dtype != torch.float32 or not noise.is_contiguous()):
            raise _lib.MvkError(f"TextEncoderFn: noise must be a contiguous float32 buffer of {total} entries")
        tokens = tokens.contiguous()
        keymask = None if padding_mask is None else (padding_mask != 0).to(torch.int32).contiguous()
        M = B * S
        h = txt_embed_fwd(tokens, emb, pe, _txt_site(noise, pos_off, M * E, p), p).view(M, E)
        acts = []
        for l in range(n_layers):
            w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2 = params[l * TXT_LAYER_PARAMS:(l + 1) * TXT_LAYER_PARAMS]
            oa, or1, of, or2 = offs[l]
            qkv = linear_fwd(h, w_in, b_in, NONE)
            cx, P = txt_attn_fwd(qkv.view(B, S, 3 * E), nhead, keymask, _txt_site(noise, oa, B * nhead * S * S, p), p, keep=keep)
            cx = cx.view(M, E)
            a = linear_fwd(cx, w_o, b_o, NONE)
            y1, z1, m1, r1 = txt_add_ln_fwd(h, a, g1, be1, eps, _txt_site(noise, or1, M * E, p), p, keep=keep, z_in_t=True)
            f1 = txt_drop(linear_fwd(y1, w1, b1, RELU), _txt_site(noise, of, M * F, p), p)
            f2 = linear_fwd(f1, w2, b2, NONE)
            last = l == n_layers - 1
            y2, z2, m2, r2 = txt_add_ln_fwd(y1, f2, g2, be2, eps, _txt_site(noise, or2, M * E, p), p,
                                            rowmask=keymask if last and zero_pads else None, zero_pads=last and zero_pads,
                                            keep=keep, z_in_t=True)
            if keep:
                acts += [h, qkv, P, cx, z1, m1, r1, y1, f1, z2, m2, r2]
            h = y2
        if keep:
            ctx.save_for_backward(tokens, noise, emb, *params, *acts)
        ctx.cfg = (B, S, E, F, V, nhead, n_layers, p)
        return h.view(B, S, E)

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        B, S, E, F, V, nhead, n_layers, p = ctx.cfg
        saved = ctx.saved_tensors
        tokens, noise, emb = saved[:3]
        params = saved[3:3 + n_layers * TXT_LAYER_PARAMS]
        acts = saved[3 + n_layers * TXT_LAYER_PARAMS:]
        M = B * S
        _, pos_off, offs = text_noise_layout(B, S, E, nhead, F, n_layers)
        grads = [None] * len(params)
        dy, dy2 = _c(dout).view(M, E), None
        for l in range(n_layers - 1, -1, -1):
            w_in, b_in, w_o, b_o, w1, b1, w2, b2, g1, be1, g2, be2 = params[l * TXT_LAYER_PARAMS:(l + 1) * TXT_LAYER_PARAMS]
            h, qkv, P, cx, z1, m1, r1, y1, f1, z2, m2, r2 = acts[12 * l:12 * (l + 1)]
            oa, or1, of, or2 = offs[l]
            k = l * TXT_LAYER_PARAMS
            (tg2, grads[k + 10]), (tb2, grads[k + 11]) = _grad_target(g2), _grad_target(be2)
            dx2, dt2 = txt_add_ln_bwd(dy, z2, m2, r2, g2, dy2, _txt_site(noise, or2, M * E, p), p, dgamma=tg2, dbeta=tb2)
            grads[k + 6], grads[k + 7] = linear_bwd_weight(dt2, f1, w2, b2)
            # f1 is what linear2 read: relu(.) after the dropout, zero where dropped — its ReLU' carries the mask, the scale follows
            df1 = txt_drop(linear_bwd_data(dt2, w2, prev_out=f1, prev_act=RELU), _txt_site(noise, of, M * F, p), p)
            grads[k + 4], grads[k + 5] = linear_bwd_weight(df1, y1, w1, b1)
            dy1 = linear_bwd_data(df1, w1)
            (tg1, grads[k + 8]), (tb1, grads[k + 9]) = _grad_target(g1), _grad_target(be1)
            dx1, dt1 = txt_add_ln_bwd(dx2, z1, m1, r1, g1, dy1, _txt_site(noise, or1, M * E, p), p, dgamma=tg1, dbeta=tb1)
            grads[k + 2], grads[k + 3] = linear_bwd_weight(dt1, cx, w_o, b_o)
            dcx = linear_bwd_data(dt1, w_o)
            dqkv = txt_attn_bwd(qkv.view(B, S, 3 * E), P, dcx.view(B, S, E), nhead, _txt_site(noise, oa, B * nhead * S * S, p), p)
            dqkv = dqkv.view(M, 3 * E)
            grads[k], grads[k + 1] = linear_bwd_weight(dqkv, h, w_in, b_in)
            dy, dy2 = dx1, linear_bwd_data(dqkv, w_in)
        gemb = None
        if ctx.needs_input_grad[7]:
            te, gemb = _grad_target(emb)
            txt_embed_bwd(tokens, dy, V, dy2, _txt_site(noise, pos_off, M * E, p), p, out=te)
        return (None, None, None, None, None, None, None, gemb, None, *grads)


# =====================================================================================================
# The image grid of a set of modality tensors (metrics.Visualization, BaseTrainer.predict)
# =====================================================================================================
def image_grid_shape(shapes, nrow, padding=2):
    """(T, Hg, Wg) of the grid of image batches of shapes [(n, c, h, w), ...]: torchvision's make_grid geometry over tiles of the
    largest height and width (include/mvk.h, mvk_image_grid); a single tile has no border."""
    shapes = [s for s in shapes if s[0] > 0]
    T = sum(s[0] for s in shapes)
    if T == 0:
        return 0, 0, 0
    H, W = max(s[2] for s in shapes), max(s[3] for s in shapes)
    if T == 1:
        return 1, H, W
    xmaps = min(int(nrow), T)
    ymaps = (T + xmaps - 1) // xmaps
    return T, ymaps * (H + padding) + padding, xmaps * (W + padding) + padding


def _image_grid_torch(tensors, nrow, padding, pad_value, want):
    """The plain-torch path of image_grid (CPU tensors, other dtypes, strided tensors, more sources than the launch takes): adapt_shape,
    cat, the grid assembled from the padded cells in a handful of tensor operations, the quantisation of the reference."""
    from .data.datasets.utils import adapt_shape

    data, _ = adapt_shape({i: t.float() for i, t in enumerate(tensors)})
    x = torch.cat(list(data.values()))
    T, _, H, W = x.shape
    if T == 1:
        grid = x[0].clone()
    else:
        xmaps = min(int(nrow), T)
        ymaps = (T + xmaps - 1) // xmaps
        pad = torch.nn.functional.pad
        cells = pad(x, (0, padding, 0, padding), value=pad_value)  # every tile with the border to its right and below it
        cells = pad(cells, (0, 0, 0, 0, 0, 0, 0, ymaps * xmaps - T), value=pad_value)  # the empty cells of the last row
        body = cells.view(ymaps, xmaps, 3, H + padding, W + padding).permute(2, 0, 3, 1, 4)
        grid = pad(body.reshape(3, ymaps * (H + padding), xmaps * (W + padding)), (padding, 0, padding, 0), value=pad_value)
    image = None
    if "uint8" in want:
        q = torch.nan_to_num(grid.mul(255).add_(0.5), nan=0.0, posinf=255.0, neginf=0.0).clamp_(0, 255)
        image = q.permute(1, 2, 0).to(torch.uint8).contiguous()
    return (grid if "float" in want else None), image


def image_grid(tensors, nrow, padding=2, pad_value=0.0, want=("float", "uint8"), grid_out=None, image_out=None):
    """The picture of a list of modality tensors, each [n], [n, a], [n, a, b] or [n, c, h, w] as the models hand them out (NOT
    adapted): brought to three channels, centred in tiles of the largest height and width, tiled `nrow` to a row with `padding`
    pixels of `pad_value` around every tile -- adapt_shape, torch.cat and torchvision's make_grid of the reference -- and quantised
    as its `mul(255).add_(0.5).clamp_(0, 255).permute(1, 2, 0).to(uint8)`.  Returns (grid [3, Hg, Wg] fp32, image [Hg, Wg, 3] uint8)
    on the tensors' device; `want` names which of the two ("float", "uint8") are made, the other is None.

    Contiguous fp32 tensors on one GPU are ONE launch of mvk_image_grid that writes every element of both outputs once (grid_out /
    image_out: caller-owned outputs for that path, contiguous, any element offset).  Everything the launch declines -- CPU tensors,
    other dtypes (computed in fp32), strided tensors, more than GRID_MAX_SOURCES tensors, 3 Hg Wg >= 2^31 -- takes the plain-torch
    path."""
    from .data.datasets.utils import as_image_batch

    want = tuple(want)
    if not want or any(w not in ("float", "uint8") for w in want):
        raise ValueError(f'image_grid: want must name "float" and / or "uint8", got {want}')
    if int(nrow) <= 0 or int(padding) < 0:
        raise ValueError(f"image_grid: nrow must be positive and padding non-negative, got {nrow}, {padding}")
    srcs = [as_image_batch(t.detach()) for t in tensors]
    srcs = [t for t in srcs if t.shape[0] > 0]
    if not srcs:
        raise ValueError("image_grid: no image to show (the tensors hold no rows)")
    if any(t.numel() == 0 for t in srcs):
        raise ValueError("image_grid: a tensor with an empty channel, height or width")
    T, Hg, Wg = image_grid_shape([tuple(t.shape) for t in srcs], nrow, padding)
    dev = srcs[0].device
    fused = (dev.type == "cuda" and len(srcs) <= _lib.GRID_MAX_SOURCES and 3 * Hg * Wg < 2 ** 31
             and all(t.device == dev and t.dtype == torch.float32 and t.is_contiguous() for t in srcs))
    if not fused:
        if grid_out is not None or image_out is not None:
            raise ValueError("image_grid: grid_out / image_out belong to the fused launch, which declines these tensors")
        return _image_grid_torch(srcs, nrow, int(padding), float(pad_value), want)
    grid = image = None
    if "float" in want:
        grid = torch.empty(3, Hg, Wg, dtype=torch.float32, device=dev) if grid_out is None else grid_out
        if grid.dtype != torch.float32 or tuple(grid.shape) != (3, Hg, Wg) or not grid.is_contiguous() or grid.device != dev:
            raise ValueError(f"image_grid: grid_out must be a contiguous float32 tensor of shape {(3, Hg, Wg)} on {dev}")
    if "uint8" in want:
        image = torch.empty(Hg, Wg, 3, dtype=torch.uint8, device=dev) if image_out is None else image_out
        if image.dtype != torch.uint8 or tuple(image.shape) != (Hg, Wg, 3) or not image.is_contiguous() or image.device != dev:
            raise ValueError(f"image_grid: image_out must be a contiguous uint8 tensor of shape {(Hg, Wg, 3)} on {dev}")
    descs = (_lib.GridSrc * len(srcs))()
    for d, t in zip(descs, srcs):
        d.data, (d.n, d.c, d.h, d.w) = t.data_ptr(), t.shape
    call("mvk_image_grid", descs, len(srcs), int(nrow), int(padding), float(pad_value), ptr(grid), ptr(image), stream_ptr())
    return grid, image


# =====================================================================================================
# A batch of a device-resident dataset (data/datasets/cub.py, CUB.device_batcher)
# =====================================================================================================
def text_batch(tokens, lengths, index, vocab_size, want=("tokens", "padding_mask", "one_hot")):
    """The captions `index` (int64 [B], on the device, in [0, N): taken on trust) of a token store (`tokens` int32 [N, L],
    `lengths` int32 [N]) in ONE launch of mvk_text_batch: dict(tokens=int64 [B, L], padding_mask=fp32 [B, L], one_hot=fp32
    [B, L, V]) with the entries `want` names ("padding_mask" is always made)."""
    if tokens.dtype != torch.int32 or lengths.dtype != torch.int32 or index.dtype != torch.int64:
        raise ValueError("text_batch: tokens and lengths are int32, the index int64")
    if not (tokens.is_cuda and tokens.is_contiguous() and lengths.is_contiguous() and index.is_contiguous()
            and lengths.device == tokens.device and index.device == tokens.device):
        raise _lib.MvkError("text_batch: contiguous tensors on one GPU")
    N, L = tokens.shape
    B, V = index.numel(), int(vocab_size)
    out = {}
    if "tokens" in want:
        out["tokens"] = torch.empty(B, L, dtype=torch.int64, device=tokens.device)
    out["padding_mask"] = torch.empty(B, L, dtype=torch.float32, device=tokens.device)
    if "one_hot" in want:
        out["one_hot"] = torch.empty(B, L, V, dtype=torch.float32, device=tokens.device)
    call("mvk_text_batch", ptr(tokens), ptr(lengths), ptr(index), N, B, L, V, ptr(out.get("tokens")), ptr(out["padding_mask"]),
         ptr(out.get("one_hot")), stream_ptr())
    return out


def u8_image_batch(store, index, div=1):
    """Rows `index // div` (int64 [B], on the device: taken on trust) of a byte store [N, ...] as fp32 in [0, 1]: ONE launch of
    mvk_u8_image_batch, bit for bit `store[index // div].float().div(255)`."""
    if store.dtype != torch.uint8 or index.dtype != torch.int64:
        raise ValueError("u8_image_batch: a uint8 store and an int64 index")
    if not (store.is_cuda and store.is_contiguous() and index.is_contiguous() and index.device == store.device):
        raise _lib.MvkError("u8_image_batch: contiguous tensors on one GPU")
    N, B = store.shape[0], index.numel()
    E = store[0].numel() if N else 0
    out = torch.empty((B, *store.shape[1:]), dtype=torch.float32, device=store.device)
    call("mvk_u8_image_batch", ptr(store), ptr(index), N, B, E, int(div), ptr(out), stream_ptr())
    return out
