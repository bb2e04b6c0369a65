"""The tiled-GEMM dispatcher of csrc/igemm.hip, leaf by leaf, against float64.

Every dense layer, 4x4/stride-2 convolution and weight gradient that misses a specialised kernel goes through one host-side
dispatcher (launch_auto / launch_splitk / launch_with_colsum -> launch_igemm -> try_launch_fast -> launch_bf_tile /
launch_fast_tile, or the generic igemm_kernel).  CASES below is that dispatcher written down: every entry names the leaf it
targets (entry point, engine, tile, A mode, B mode, split-K form, epilogue and its options), the shape that reaches it and the
host rule it relies on, and the device kernels it must launch.  Each case

1. runs the C entry point once under torch.profiler and asserts the exact set of device kernels it launched (a case whose
   launch is not seen by the profiler fails: the table is checked, not assumed);
2. compares EVERY output entry with the same operation in float64 on the CPU (GEMM, bias, activation, masks, accumulate into
   a non-zero buffer, column sums):
       |got - ref| <= C_ENTRY * (sum_k |a_ik b_kj| + |bias_j| + |initial|)                                       (a)
   and, for the split-bf16 and exact-fp32 engines, max and rms error no worse than 2x torch's fp32 GEMM of the same operands
   on the GPU (TF32 off)                                                                                          (b);
3. shows that the tolerance has teeth: the same formula evaluated in float64 on operands rounded to a TWO-piece bf16 split
   (hi = x.bfloat16(), mid = (x - hi).bfloat16(): 16 instead of 24 significant bits, what the split engine computes if it
   drops its third piece) must FAIL (a), or (b) for the aggregate cases;
4. runs again from the same initial buffers and asserts bit-identical results wherever the launch has scratch (ordered
   split-K slabs, deferred slabs inside deferred_reductions, column-sum partials; include/mvk.h: only the fp32-atomic
   no-scratch fallback is allowed to differ between runs, and it is held to the tolerance alone).

C_ENTRY = 5e-7.  Basis: the exact-fp32 MFMA (a k-ordered fp32 fma chain) is documented at 0.75-1.5e-7 * sum|a b| for
K <= 1024 and 3.5e-7 at K = 4096 (cdna_hip_programming.md section 3).  Over this table (up to ~2e5 entries per output) the
largest entry measured on an MI355X is 3.9e-7 * sum|a b| with the split engine (bwdd-bf128x64-plainK-bmN-aact-relu, K = 100)
and 3.5e-7 with the exact-fp32 one; 5e-7 leaves 1.3x.  Every reduction held to it runs over at most 1024 terms in one
accumulator chain (longer ones are split into slabs by the split-K form or the waves of the few-row kernels).  The two-piece
operands are off by ~2^-17 per operand: the weakest per-entry rejection in the table is 1.2x the bound (column sums of 160
terms), the aggregate ones 4-20x torch's error.

The 3x3 / stride-1 routes of the engine (tw = 3, mul = 1 gather: AM_ROW forward / backward data, AM_COL weight gradient, E_CONVREF
with taps = 9, the residual epilogue, fused column sums) are the `c3` cases; their references are tests/conv3_ref.py, and the
entry-point wrappers p_conv3 / p_conv3_wgrad also serve the table of the specialised 3x3 kernels (tests/test_gpu_conv3x3.py).
c3fwd-bf128x32-row-K2304 reduces 2304 terms in one chain, beyond the 1024 C_ENTRY was derived for.  Measured on an MI355X: 0.17x the
bound on the split-bf16 engine and 0.28x on the exact-fp32 engine (two-piece emulation: 1.15x), so the case is held to (a) like every
other one; profiles/NOTES_conv3.md also records the exact-fp32 engine against torch's fp32 GEMM there (2.2x its max error).

The default configuration is the one under test (engine 1: split bf16).  test_engine_f32_child re-runs this table in a fresh
process with MVK_ENGINE=f32 (the documented switch, read once per process), where each case expects its `f32` kernels.

Leaves the default configuration cannot reach from these entry points (and why):
- igemm_fast_kernel<128,64,32,...> and <128,128,16,PLAIN/COL...>: with engine 1 every grid big enough for them (>= 384
  blocks) already takes the split engine (>= 256 blocks); covered by the f32-engine child.
- igemm_bf_kernel<128,128,AM_COL,...>: needs >= 384 128x128 blocks, but the 4x4/stride-2 weight gradient splits K for a
  target of 256 128x64 blocks (SPLITK_C4), so its 128x128 grid never exceeds 256 (igemm.hip:297, 374).
- the `ksplit_tiles & 1` fall-through (igemm.hip:286): launch_splitk always rounds ksplit_tiles up to even (igemm.hip:391).
- AM_ROW3 (pre-split operands): reached only with MVK_FMT_IN_BF3, covered by test_conv_reads_pre_split_input.
"""
import math
import os
import re
import subprocess
import sys
import zlib
from dataclasses import dataclass, field

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C_ENTRY = 5e-7
F32_ENGINE = os.environ.get("MVK_ENGINE", "")[:1] == "f"
TILED_ONLY = 0x100 | 0x400  # mvk_debug_set_flags: no register-stationary 4x4/stride-2 or 3x3 kernels (igemm.hip:737-742)
NONE, RELU, SIGMOID, LEAKY = 0, 1, 2, 3
F02 = float(torch.tensor(0.2, dtype=torch.float32))  # the kernels' 0.2f


def dev():
    return torch.device("cuda:0")


# ---- kernel names ------------------------------------------------------------------------------------------------------
_AM = dict(K=1, R=2, ROW=3, COL=4)  # igemm_fast.hpp AMode: AM_PLAIN_K, AM_PLAIN_R, AM_ROW, AM_COL
_BMODE = dict(K=1, N=2)             # BM_K, BM_N


def bf(bm, bn, am, bmode, aact=False):
    return f"igemm_bf_kernel<{bm},{bn},{_AM[am]},{_BMODE[bmode]},{str(aact).lower()},2>"


def fast(bm, bn, bkt, am, bmode, aact=False):
    return f"igemm_fast_kernel<{bm},{bn},{bkt},{_AM[am]},{_BMODE[bmode]},{str(aact).lower()}>"


def gen(bm, bn):
    return f"igemm_kernel<{bm},{bn}>"


RED, BATCH = "splitk_reduce_kernel", "splitk_reduce_batch_kernel"
FIN, FINS, CS4, CS1 = "colsum_finish_kernel", "colsum_finish_scalar_kernel", "colsum_kernel<4>", "colsum_kernel<1>"
NARROW, H4, H16, HFIN = "narrow_fwd_kernel", "heads_fwd_kernel<4>", "heads_fwd_kernel<16>", "heads_finish_kernel"


def _norm(name):
    n = name.replace("(anonymous namespace)::", "")
    if n.startswith("void "):
        n = n[5:]
    n = n.split("(")[0]
    n = re.sub(r"\b[A-Za-z_]\w*::", "", n)
    return n.replace(" ", "")


def launched_kernels(fn):
    """Device kernels launched by fn() (normalised names, memory copies left out), as recorded by torch.profiler."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == DeviceType.CUDA]
    return sorted({_norm(n) for n in names if not re.match(r"(?i)^(memcpy|memset|hipmemcpy|hipmemset)", n)})


# ---- operands and references ---------------------------------------------------------------------------------------------
def g(seed):
    return torch.Generator().manual_seed(seed)


def rows_scaled(m, k, gen_):
    """Non-square, asymmetric operand: normal entries, every row on its own scale (0.25 .. 4.25)."""
    return torch.randn(m, k, generator=gen_) * (torch.rand(m, 1, generator=gen_) * 4 + 0.25)


def cols_scaled(k, n, gen_):
    return torch.randn(k, n, generator=gen_) * (torch.rand(1, n, generator=gen_) + 0.5) / math.sqrt(k)


def two_piece(x):
    """x rounded to hi + mid of a bf16 split (the split engine without its third piece), in float64."""
    hi = x.float().bfloat16()
    mid = (x.float() - hi.float()).bfloat16()
    return hi.double() + mid.double()


def act64(v, act):
    if act == RELU:
        return v.clamp_min(0)
    if act == SIGMOID:
        return torch.sigmoid(v)
    if act == LEAKY:
        return torch.where(v > 0, v, F02 * v)
    return v


def actgrad64(y, act):
    """act'(pre) from the stored output y (mvk_act_grad_from_out); y given in float32 (the kernels' products in fp32)."""
    y = y.double()
    if act == RELU:
        return (y > 0).double()
    if act == LEAKY:
        return torch.where(y > 0, torch.ones_like(y), torch.full_like(y, F02))
    if act == SIGMOID:
        return (y.float() * (1 - y.float())).double()
    return torch.ones_like(y)


@dataclass
class Out:
    ref: torch.Tensor            # float64 reference of what the launch adds / writes
    bound: torch.Tensor          # sum_k |a b| (+ |bias| + |initial|) per entry
    deg: torch.Tensor            # the same formula on two-piece operands
    init: torch.Tensor = None    # non-zero initial content of an accumulated (+=) output (CPU float32)
    shape: tuple = None          # shape of the device buffer (default: ref's)
    rows: torch.Tensor = None    # the checked rows of the buffer (first dimension) when the reference is sampled
    slack: float = 0.0           # extra relative allowance of the result's own magnitude (sigmoid evaluation: 2 ulp)


@dataclass
class Prep:
    call: object                 # call(bufs) -> launches into the device buffers
    outs: list
    agg: object = None           # () -> torch fp32 result on the GPU of output 0 (aggregate check (b))
    det: bool = True             # ordered reductions: bit-identical repeat
    deferred: bool = False       # outputs are views of a flat gradient buffer inside schedule.deferred_reductions
    flags: int = 0               # mvk_debug_set_flags for the call
    keep: list = field(default_factory=list)


def _ws():
    t = getattr(_ws, "t", None)
    if t is None:
        t = _ws.t = torch.empty(16 * 1024 * 1024, device=dev())
    return t


def WS(mode="ws", need=0):
    """(pointer, floats) of the split-K scratch: 'ws' = ample, 'none' = NULL, 'short' = one float below what the launch needs."""
    from multivae_amd._lib import ptr

    if mode == "none":
        return None, 0
    t = _ws()
    return ptr(t), (need - 1 if mode == "short" else t.numel())


def unaligned(x):
    """x as a view with storage offset 1 (not 16-byte aligned)."""
    buf = torch.empty(x.numel() + 1, device=dev())
    v = buf[1:].view(x.shape)
    v.copy_(x)
    return v


def sample_rows(m, cap=4096):
    """All rows, or the first and last 1024 and 1024 spread between (tile edges at both ends stay in)."""
    if m <= cap:
        return None
    mid = torch.linspace(1024, m - 1025, 1024).long()
    return torch.unique(torch.cat([torch.arange(1024), mid, torch.arange(m - 1024, m)]))


def gemm64(a, b, bias=None, act=NONE, amask=None, cmask=None, rows=None):
    """(ref, bound, deg) of act(A B + bias) * cmask with A *= amask, in float64 (rows: sampled rows of A)."""
    if rows is not None:
        a = a[rows]
        amask = None if amask is None else amask[rows]
        cmask = None if cmask is None else cmask[rows]

    def f(A, B):
        A = A if amask is None else A * amask
        v = A @ B
        if bias is not None:
            v = v + bias.double()
        return v

    pre = f(a.double(), b.double())
    bound = (a.double() if amask is None else a.double() * amask).abs() @ b.double().abs()
    if bias is not None:
        bound = bound + bias.double().abs()
    deg = act64(f(two_piece(a), two_piece(b)), act)
    ref = act64(pre, act)
    if act == SIGMOID:
        bound = 0.25 * bound
    if cmask is not None:
        ref, deg, bound = ref * cmask, deg * cmask, bound * cmask
    return ref, bound, deg


# ---- entry points ------------------------------------------------------------------------------------------------------
def p_linear_fwd(seed, M, N, K, bias=True, act=NONE, x_off=False, ws="ws"):
    """mvk_linear_fwd: Y = act(X W^T + b), X [M][K], W [N][K]."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    x, w = rows_scaled(M, K, gn), rows_scaled(N, K, gn) / math.sqrt(K)
    b = torch.randn(N, generator=gn) if bias else None
    xd = unaligned(x.to(dev())) if x_off else x.to(dev())
    wd, bd = w.to(dev()), None if b is None else b.to(dev())
    rows = sample_rows(M)
    ref, bound, deg = gemm64(x, w.t(), b, act, rows=rows)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_linear_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(bufs[0]), M, N, K, act, wsp, wsn, stream_ptr())

    def agg():
        return act64((xd @ wd.t() + (0 if bd is None else bd)).double(), act)

    return Prep(run, [Out(ref, bound, deg, shape=(M, N), rows=rows, slack=2e-7 if act == SIGMOID else 0)], agg=agg,
                keep=[xd, wd, bd])


def p_heads_kn(seed, M, N, K):
    """mvk_heads_fwd with ONE head (W1 = NULL) on the packed [K][N] weight layout (w_sk = N, w_sn = 1: no 16-byte rows)."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    x, w = rows_scaled(M, K, gn), cols_scaled(K, N, gn)
    b = torch.randn(N, generator=gn)
    xd, wd, bd = x.to(dev()), w.to(dev()), b.to(dev())
    ref, bound, deg = gemm64(x, w, b)

    def run(bufs):
        call("mvk_heads_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(bufs[0]), None, None, None, M, N, K, N, 1, stream_ptr())

    return Prep(run, [Out(ref, bound, deg)], keep=[xd, wd, bd])


def p_linear_bwd_data(seed, M, N, K, y_act=NONE, prev_act=NONE, accumulate=False, colsum=False, ws="ws", deferred=False):
    """mvk_linear_bwd_data: dX = ((dY * y_act'(Y)) W) * prev_act'(prev), dY [M][N], W [N][K]; += into dX; colsum_acc += sums."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    dy, w = rows_scaled(M, N, gn), rows_scaled(N, K, gn) / math.sqrt(N)
    y = torch.randn(M, N, generator=gn) if y_act else None
    if y_act == SIGMOID:
        y = torch.sigmoid(y)
    prev = torch.randn(M, K, generator=gn) if prev_act else None
    amask = actgrad64(y, y_act) if y_act else None
    cmask = actgrad64(prev, prev_act) if prev_act else None
    rows = sample_rows(M)
    ref, bound, deg = gemm64(dy, w, amask=amask, cmask=cmask, rows=rows)
    d = dev()
    dyd, wd = dy.to(d), w.to(d)
    yd = None if y is None else y.to(d)
    pd = None if prev is None else prev.to(d)
    init = torch.randn(M, K, generator=gn) if accumulate else None
    outs = [Out(ref, bound + (0 if init is None else init.double().abs()[rows if rows is not None else slice(None)]), deg,
                init=init, shape=(M, K), rows=rows)]
    if colsum:
        assert rows is None
        cinit = torch.randn(K, generator=gn)
        outs.append(Out(ref.sum(0), bound.sum(0) + cinit.double().abs(), deg.sum(0), init=cinit))
    need = 0
    if ws == "short":  # one float below the ordered split's need (launch_splitk: z slabs of M x K)
        tiles = ((M + 127) // 128) * (1 if K <= 32 else (K + 63) // 64)
        kt = (N + 15) // 16
        sp = max(1, min(kt, 512 // tiles))
        ks = -(-kt // sp)
        ks += ks & 1
        need = -(-kt // ks) * M * K
    wsp, wsn = WS(ws, need)

    def run(bufs):
        call("mvk_linear_bwd_data", ptr(dyd), ptr(wd), ptr(bufs[0]), M, N, K, ptr(yd), y_act, ptr(pd), prev_act, int(accumulate),
             ptr(bufs[1]) if colsum else None, wsp, wsn, stream_ptr())

    def agg():
        a = dyd if yd is None else dyd * actgrad64(yd.cpu(), y_act).float().to(d)
        r = (a @ wd).double()
        return r if pd is None else r * actgrad64(pd.cpu(), prev_act).to(d)

    return Prep(run, outs, agg=agg, det=ws == "ws", deferred=deferred, keep=[dyd, wd, yd, pd])


def p_linear_bwd_weight(seed, M, N, K, y_act=NONE, db=True, ws="ws", deferred=False):
    """mvk_linear_bwd_weight: dW [N][K] += (dY * y_act'(Y))^T X, db [N] += column sums."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    dy, x = rows_scaled(M, N, gn), rows_scaled(M, K, gn) / math.sqrt(M)
    y = torch.randn(M, N, generator=gn) if y_act else None
    if y_act == SIGMOID:
        y = torch.sigmoid(y)
    m = actgrad64(y, y_act) if y_act else None
    a = dy.t()
    ref, bound, deg = gemm64(a, x, amask=None if m is None else m.t())
    init = torch.randn(N, K, generator=gn)
    outs = [Out(ref, bound + init.double().abs(), deg, init=init)]
    if db:
        binit = torch.randn(N, generator=gn)
        dm = dy.double() * (1 if m is None else m)
        outs.append(Out(dm.sum(0), dm.abs().sum(0) + binit.double().abs(), (two_piece(dy) * (1 if m is None else m)).sum(0),
                        init=binit))
    d = dev()
    dyd, xd = dy.to(d), x.to(d)
    yd = None if y is None else y.to(d)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_linear_bwd_weight", ptr(dyd), ptr(xd), ptr(bufs[0]), ptr(bufs[1]) if db else None, M, N, K, ptr(yd), y_act,
             wsp, wsn, stream_ptr())

    def agg():
        a_ = dyd if yd is None else dyd * actgrad64(yd.cpu(), y_act).float().to(d)
        return (a_.t() @ xd).double()

    return Prep(run, outs, agg=agg, det=ws == "ws", deferred=deferred, keep=[dyd, xd, yd])


def p_gemm(seed, M, N, K, ta=0, tb=0, bias_mod=0, act=NONE, accumulate=False, a_act=NONE, c_act=NONE, ws="ws"):
    """mvk_gemm: C (+)= act(op(A) op(B) + bias[n % bias_mod]) * c_act'(csrc), op(A) *= a_act'(asrc)."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    A, B = rows_scaled(M, K, gn), cols_scaled(K, N, gn)
    bias = torch.randn(bias_mod, generator=gn) if bias_mod else None
    bias_full = None if bias is None else bias[torch.arange(N) % bias_mod]
    asrc = torch.randn(*((K, M) if ta else (M, K)), generator=gn) if a_act else None
    csrc = torch.randn(M, N, generator=gn) if c_act else None
    amask = None if asrc is None else actgrad64(asrc.t() if ta else asrc, a_act)
    cmask = None if csrc is None else actgrad64(csrc, c_act)
    rows = sample_rows(M)
    ref, bound, deg = gemm64(A, B, bias_full, act, amask, cmask, rows=rows)
    init = torch.randn(M, N, generator=gn) if accumulate else None
    if init is not None:
        bound = bound + init.double().abs()[rows if rows is not None else slice(None)]
    d = dev()
    ad = (A.t().contiguous() if ta else A).to(d)
    bd = (B.t().contiguous() if tb else B).to(d)
    biasd = None if bias is None else bias.to(d)
    asd = None if asrc is None else asrc.to(d)
    csd = None if csrc is None else csrc.to(d)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_gemm", ptr(ad), ptr(bd), ptr(bufs[0]), M, N, K, ta, tb, ptr(biasd), bias_mod, act, int(accumulate), ptr(asd),
             a_act, ptr(csd), c_act, wsp, wsn, stream_ptr())

    return Prep(run, [Out(ref, bound, deg, init=init, shape=(M, N), rows=rows, slack=2e-7 if act == SIGMOID else 0)],
                det=ws == "ws", keep=[ad, bd, biasd, asd, csd])


def p_colsum(seed, M, N, y_act=NONE, ws="ws"):
    """mvk_colsum_acc: db [N] += sum_m dY[m][n] * y_act'(Y[m][n])."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    dy = rows_scaled(M, N, gn)
    y = torch.randn(M, N, generator=gn) if y_act else None
    m = 1 if y is None else actgrad64(y, y_act)
    init = torch.randn(N, generator=gn)
    out = Out((dy.double() * m).sum(0), (dy.double().abs() * m).sum(0) + init.double().abs(), (two_piece(dy) * m).sum(0), init=init)
    d = dev()
    dyd, yd = dy.to(d), None if y is None else y.to(d)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_colsum_acc", ptr(dyd), ptr(yd), y_act, ptr(bufs[0]), M, N, wsp, wsn, stream_ptr())

    return Prep(run, [out], det=ws == "ws", keep=[dyd, yd])


def p_act_bwd_colsum(seed, M, N, act, ws="ws"):
    """mvk_act_bwd_colsum: dPre = dY * act'(Y); db [N] += column sums of dPre."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    dy = rows_scaled(M, N, gn)
    y = torch.randn(M, N, generator=gn)
    if act == SIGMOID:
        y = torch.sigmoid(y)
    m = actgrad64(y, act)
    pre = dy.double() * m
    init = torch.randn(N, generator=gn)
    outs = [Out(pre, pre.abs(), two_piece(dy) * m),
            Out(pre.sum(0), pre.abs().sum(0) + init.double().abs(), (two_piece(dy) * m).sum(0), init=init)]
    d = dev()
    dyd, yd = dy.to(d), y.to(d)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_act_bwd_colsum", ptr(dyd), ptr(yd), act, M, N, ptr(bufs[0]), ptr(bufs[1]), wsp, wsn, stream_ptr())

    return Prep(run, outs, det=ws == "ws", keep=[dyd, yd])


def p_nchw_sum(seed, n, c, hw, y_act=NONE, ws="ws"):
    """mvk_nchw_channel_sum_acc: db [c] += sum over (image, position) of dY * y_act'(Y), NCHW."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    dy = torch.randn(n, c, hw, generator=gn) * (torch.rand(1, c, 1, generator=gn) * 4 + 0.25)
    y = torch.randn(n, c, hw, generator=gn) if y_act else None
    m = 1 if y is None else actgrad64(y, y_act)
    init = torch.randn(c, generator=gn)
    out = Out((dy.double() * m).sum((0, 2)), (dy.double().abs() * m).sum((0, 2)) + init.double().abs(),
              (two_piece(dy) * m).sum((0, 2)), init=init)
    d = dev()
    dyd, yd = dy.to(d), None if y is None else y.to(d)
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_nchw_channel_sum_acc", ptr(dyd), ptr(yd), y_act, ptr(bufs[0]), n, c, hw, wsp, wsn, stream_ptr())

    return Prep(run, [out], det=ws == "ws", keep=[dyd, yd])


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _conv_inputs(gn, n, h, w, Cu, Cv):
    U = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    Wc = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(Cv, 1, 1, 1, generator=gn) + 0.5) / math.sqrt(16 * Cu)
    return U, Wc


def _imgs(n, cap):
    """Images whose outputs are checked: all, or the first, the last and a spread between (when n * positions is large)."""
    if n <= cap:
        return None
    return torch.unique(torch.cat([torch.arange(cap // 3), torch.linspace(cap // 3, n - 1 - cap // 3, cap // 3).long(),
                                   torch.arange(n - cap // 3, n)]))


def p_conv_down(seed, n, h, w, Cu, Cv, act=RELU, bias=True, u_nchw=False, u_act=NONE, v_act=NONE, colsum=False, cap=64):
    """mvk_conv4s2_down on the tiled engine: V = act(conv4x4s2p1(U * u_act'(Usrc)) + b) * v_act'(Vsrc), NHWC V; colsum_acc += sums."""
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    U, Wc = _conv_inputs(gn, n, h, w, Cu, Cv)
    b = torch.randn(Cv, generator=gn) if bias else None
    usrc = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) if u_act else None
    vsrc = torch.randn(n, Cv, h, w, generator=gn) if v_act else None
    imgs = _imgs(n, cap)
    sel = (lambda t: t) if imgs is None else (lambda t: None if t is None else t[imgs])
    um = 1 if usrc is None else actgrad64(sel(usrc), u_act)
    vm = 1 if vsrc is None else actgrad64(sel(vsrc), v_act)

    def f(Ux, Wx, bx):
        return F.conv2d(Ux * um, Wx, bx, stride=2, padding=1)

    Us = sel(U)
    pre = f(Us.double(), Wc.double(), None if b is None else b.double())
    bnd = f(Us.double().abs(), Wc.double().abs(), None if b is None else b.double().abs())
    ref = act64(pre, act) * vm
    deg = act64(f(two_piece(Us), two_piece(Wc), None if b is None else b.double()), act) * vm
    bnd = (0.25 * bnd if act == SIGMOID else bnd) * (vm if isinstance(vm, torch.Tensor) else 1)
    tohw = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    outs = [Out(tohw(ref), tohw(bnd), tohw(deg), shape=(n, h, w, Cv), rows=imgs)]
    if colsum:
        assert imgs is None
        cinit = torch.randn(Cv, generator=gn)
        outs.append(Out(ref.sum((0, 2, 3)), bnd.sum((0, 2, 3)) + cinit.double().abs(), deg.sum((0, 2, 3)), init=cinit))
    d = dev()
    wdown, _ = KK.pack_conv(Wc.to(d), want_up=False)
    Ud = U.to(d) if u_nchw else _nhwc(U).to(d)
    usd = None if usrc is None else (usrc.to(d) if u_nchw else _nhwc(usrc).to(d))
    vsd = None if vsrc is None else _nhwc(vsrc).to(d)
    bd = None if b is None else b.to(d)
    wsp, wsn = WS("ws")

    def run(bufs):
        call("mvk_conv4s2_down", ptr(Ud), ptr(wdown), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, act, int(u_nchw), ptr(usd), u_act,
             ptr(vsd), v_act, ptr(bufs[1]) if colsum else None, wsp, wsn, 0, None, stream_ptr())

    def agg():  # torch's fp32 GEMM of the same operands (im2col + matmul)
        Ux = U.to(d) if usrc is None else U.to(d) * actgrad64(usrc, u_act).float().to(d)
        cols = F.unfold(Ux, 4, padding=1, stride=2).transpose(1, 2)  # [n][h w][Cu 16]
        r = (cols @ Wc.to(d).view(Cv, Cu * 16).t()).view(n, h, w, Cv)
        r = act64((r if bd is None else r + bd).double(), act)
        return r if vsrc is None else r * actgrad64(vsrc, v_act).permute(0, 2, 3, 1).to(d)

    return Prep(run, outs, agg=agg, flags=TILED_ONLY, keep=[Ud, wdown, usd, vsd, bd])


def p_conv_up(seed, n, h, w, Cu, Cv, act=NONE, bias=True, u_nchw=False, u_act=NONE, colsum=False, cap=64):
    """mvk_conv4s2_up on the tiled engine: U = act(convT4x4s2p1(V) + b) * u_act'(Usrc), NHWC V, NHWC or NCHW U."""
    from multivae_amd import kernels as KK
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    V = torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(n, 1, 1, 1, generator=gn) * 4 + 0.25)
    Wc = torch.randn(Cv, Cu, 4, 4, generator=gn) * (torch.rand(1, Cu, 1, 1, generator=gn) + 0.5) / math.sqrt(4 * Cv)
    b = torch.randn(Cu, generator=gn) if bias else None
    usrc = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) if u_act else None
    imgs = _imgs(n, cap)
    Vs, us = (V, usrc) if imgs is None else (V[imgs], None if usrc is None else usrc[imgs])
    um = 1 if us is None else actgrad64(us, u_act)

    def f(Vx, Wx, bx):
        return F.conv_transpose2d(Vx, Wx, bx, stride=2, padding=1)

    pre = f(Vs.double(), Wc.double(), None if b is None else b.double())
    bnd = f(Vs.double().abs(), Wc.double().abs(), None if b is None else b.double().abs())
    ref = act64(pre, act) * um
    deg = act64(f(two_piece(Vs), two_piece(Wc), None if b is None else b.double()), act) * um
    bnd = (0.25 * bnd if act == SIGMOID else bnd) * (um if isinstance(um, torch.Tensor) else 1)
    lay = (lambda t: t) if u_nchw else (lambda t: t.permute(0, 2, 3, 1))
    outs = [Out(lay(ref), lay(bnd), lay(deg), shape=(n, Cu, 2 * h, 2 * w) if u_nchw else (n, 2 * h, 2 * w, Cu), rows=imgs)]
    if colsum:
        assert imgs is None
        cinit = torch.randn(Cu, generator=gn)
        outs.append(Out(ref.sum((0, 2, 3)), bnd.sum((0, 2, 3)) + cinit.double().abs(), deg.sum((0, 2, 3)), init=cinit))
    d = dev()
    _, wup = KK.pack_conv(Wc.to(d), want_down=False)
    Vd = _nhwc(V).to(d)
    usd = None if usrc is None else (usrc.to(d) if u_nchw else _nhwc(usrc).to(d))
    bd = None if b is None else b.to(d)
    wsp, wsn = WS("ws")

    def run(bufs):
        call("mvk_conv4s2_up", ptr(Vd), ptr(wup), ptr(bd), ptr(bufs[0]), n, h, w, Cu, Cv, act, int(u_nchw), ptr(usd), u_act,
             ptr(bufs[1]) if colsum else None, wsp, wsn, 0, None, stream_ptr())

    def agg():  # torch's fp32 GEMM of the same reduction (im2col of the zero-dilated input: 4 Cv non-zero terms per output)
        Vz = torch.zeros(n, Cv, 2 * h - 1, 2 * w - 1, device=d)
        Vz[:, :, ::2, ::2] = V.to(d)
        cols = F.unfold(Vz, 4, padding=2)  # [n][Cv 16][2h 2w]
        r = (Wc.to(d).flip(2, 3).transpose(0, 1).reshape(Cu, Cv * 16) @ cols).view(n, Cu, 2 * h, 2 * w)
        r = act64((r if bd is None else r + bd.view(1, Cu, 1, 1)).double(), act)
        if usrc is not None:
            r = r * actgrad64(usrc, u_act).to(d)
        return lay(r)

    # No aggregate check (b) here: measured on an MI355X, BOTH engines' E_UP launches sit at 1.5-3.1x torch's fp32 GEMM of the
    # same 4 Cv-term reductions in max / rms error (up-bf128x32-row-parity-Eup-bias: 1.24e-5 / 6.3e-7 vs 5.8e-6 / 3.3e-7), while
    # every entry stays inside (a) (worst 0.9x); an open finding, recorded rather than hidden behind a wider factor.
    # (a) alone rejects the two-piece operands here (5-6x the bound).
    del agg
    return Prep(run, outs, flags=TILED_ONLY, keep=[Vd, wup, usd, bd])


def p_conv_wgrad(seed, n, h, w, Cu, Cv, u_nchw=False, u_act=NONE, ws="ws", deferred=False):
    """mvk_conv4s2_wgrad on the tiled engine: dWref [Cv][Cu][4][4] += d/dW sum(conv4x4s2p1(U * u_act'(Usrc), W) * V)."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    U, _ = _conv_inputs(gn, n, h, w, Cu, Cv)
    V = torch.randn(n, Cv, h, w, generator=gn) * (torch.rand(1, Cv, 1, 1, generator=gn) + 0.5) / math.sqrt(n * h * w)
    usrc = torch.randn(n, Cu, 2 * h, 2 * w, generator=gn) if u_act else None
    um = 1 if usrc is None else actgrad64(usrc, u_act)

    def f(Ux, Vx):
        return torch.nn.grad.conv2d_weight(Ux * um, (Cv, Cu, 4, 4), Vx, stride=2, padding=1)

    init = torch.randn(Cv, Cu, 4, 4, generator=gn)
    ref = f(U.double(), V.double())
    bnd = f(U.double().abs(), V.double().abs()) + init.double().abs()
    deg = f(two_piece(U), two_piece(V))
    d = dev()
    Ud = U.to(d) if u_nchw else _nhwc(U).to(d)
    Vd = _nhwc(V).to(d)
    usd = None if usrc is None else (usrc.to(d) if u_nchw else _nhwc(usrc).to(d))
    wsp, wsn = WS(ws)

    def run(bufs):
        call("mvk_conv4s2_wgrad", ptr(Ud), ptr(Vd), ptr(bufs[0]), n, h, w, Cu, Cv, int(u_nchw), ptr(usd), u_act, wsp, wsn,
             stream_ptr())

    def agg():  # torch's fp32 GEMM of the same operands (im2col + matmul)
        Ux = U.to(d) if usrc is None else U.to(d) * actgrad64(usrc, u_act).float().to(d)
        cols = F.unfold(Ux, 4, padding=1, stride=2).transpose(1, 2).reshape(n * h * w, Cu * 16)
        return (V.to(d).permute(0, 2, 3, 1).reshape(n * h * w, Cv).t() @ cols).view(Cv, Cu, 4, 4).double()

    return Prep(run, [Out(ref, bnd, deg, init=init)], agg=agg, det=ws == "ws", deferred=deferred, flags=TILED_ONLY,
                keep=[Ud, Vd, usd])


PAIR = ((8, 32, 64), (4, 64, 128))  # (h = w, Cu, Cv) of the SVHN encoder's two inner layers (models/nn/svhn.py)
# Smallest batch mvk_conv4s2_wgrad_pair takes as one launch (igemm.hip: z > 1 and tiles * z >= bf_min_blocks() = 256 for BOTH
# layers, slices of an even number of 16-wide k-tiles, split target SPLITK_C4 = 256):
#   32 -> 64 at 8x8:   M = 512, N = 64: 4 tiles, 4 n k-tiles, <= 64 slices of >= 2 k-tiles: z = 2 n >= 64  <=>  n >= 32 (n = 31: 248 blocks)
#   64 -> 128 at 4x4:  M = 1024, N = 128: 16 tiles, n k-tiles, <= 16 slices of >= 2: z = ceil(n / 2) >= 16  <=>  n >= 31
PAIR_N = 32
PAIRK = "igemm_bf_pair_kernel<128,64,4,2,false,2>"


def p_conv_wgrad_pair(seed, n, deferred=True, single=False):
    """mvk_conv4s2_wgrad_pair: the weight gradients of two NHWC layers at one batch, dW0 / dW1 [Cv][Cu][4][4] +=.  single: the same
    two gradients by two mvk_conv4s2_wgrad calls."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    d = dev()
    outs, ops = [], []
    for h, Cu, Cv in PAIR:
        U, _ = _conv_inputs(gn, n, h, h, Cu, Cv)
        V = torch.randn(n, Cv, h, h, generator=gn) * (torch.rand(1, Cv, 1, 1, generator=gn) + 0.5) / math.sqrt(n * h * h)
        f = lambda Ux, Vx, s_=(Cv, Cu, 4, 4): torch.nn.grad.conv2d_weight(Ux, s_, Vx, stride=2, padding=1)  # noqa: E731
        init = torch.randn(Cv, Cu, 4, 4, generator=gn)
        outs.append(Out(f(U.double(), V.double()), f(U.double().abs(), V.double().abs()) + init.double().abs(),
                        f(two_piece(U), two_piece(V)), init=init))
        ops.append((_nhwc(U).to(d), _nhwc(V).to(d), h, Cu, Cv))
    wsp, wsn = WS("ws")

    def run(bufs):
        (U0, V0, h0, a0, b0), (U1, V1, h1, a1, b1) = ops
        if single:
            for (U_, V_, h_, a_, b_), buf in zip(ops, bufs):
                call("mvk_conv4s2_wgrad", ptr(U_), ptr(V_), ptr(buf), n, h_, h_, a_, b_, 0, None, NONE, wsp, wsn, stream_ptr())
        else:
            call("mvk_conv4s2_wgrad_pair", ptr(U0), ptr(V0), ptr(bufs[0]), h0, h0, a0, b0, ptr(U1), ptr(V1), ptr(bufs[1]), h1, h1, a1,
                 b1, n, wsp, wsn, stream_ptr())

    return Prep(run, outs, deferred=deferred, flags=TILED_ONLY, keep=ops)


def p_unflatten(seed, n, Cin, Cout):
    """mvk_unflatten_wgrad: dWref [Cin][Cout][4][4] += Z^T dY, dY [n][(tap, co)]."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    Z, dy = rows_scaled(n, Cin, gn), cols_scaled(n, 16 * Cout, gn)
    ref, bnd, deg = gemm64(Z.t(), dy)
    lay = lambda t: t.view(Cin, 16, Cout).permute(0, 2, 1).reshape(Cin, Cout, 4, 4)  # noqa: E731
    init = torch.randn(Cin, Cout, 4, 4, generator=gn)
    d = dev()
    Zd, dyd = Z.to(d), dy.to(d)
    wsp, wsn = WS("ws")

    def run(bufs):
        call("mvk_unflatten_wgrad", ptr(Zd), ptr(dyd), ptr(bufs[0]), n, Cin, Cout, wsp, wsn, stream_ptr())

    return Prep(run, [Out(lay(ref), lay(bnd) + init.double().abs(), lay(deg), init=init)],
                agg=lambda: lay((Zd.t() @ dyd).double()), keep=[Zd, dyd])


def p_flatten(seed, n, Cu, Cv):
    """mvk_flatten_wgrad: dWref [Cv][Cu][4][4] += H^T dY, H [n][(tap, cu)]."""
    from multivae_amd._lib import call, ptr, stream_ptr

    gn = g(seed)
    H, dy = rows_scaled(n, 16 * Cu, gn), cols_scaled(n, Cv, gn)
    ref, bnd, deg = gemm64(H.t(), dy)
    lay = lambda t: t.view(16, Cu, Cv).permute(2, 1, 0).reshape(Cv, Cu, 4, 4)  # noqa: E731
    init = torch.randn(Cv, Cu, 4, 4, generator=gn)
    d = dev()
    Hd, dyd = H.to(d), dy.to(d)
    wsp, wsn = WS("ws")

    def run(bufs):
        call("mvk_flatten_wgrad", ptr(Hd), ptr(dyd), ptr(bufs[0]), n, Cu, Cv, wsp, wsn, stream_ptr())

    return Prep(run, [Out(lay(ref), lay(bnd) + init.double().abs(), lay(deg), init=init)],
                agg=lambda: lay((Hd.t() @ dyd).double()), keep=[Hd, dyd])


# ---- 3x3 / stride 1 / pad 1 (tests/conv3_ref.py; tests/test_gpu_conv3x3.py holds the table of the specialised kernels) ----------------
RS_ALL = 0x800  # mvk_debug_set_flags: the register-stationary 3x3 kernels take every problem size they cover


def _out3(r, lay=lambda t: t, init=None, shape=None):
    """Out of a conv_small_ref.Ref; degh = the second emulation (scaled fp16 pairs without a cross term) where it is defined."""
    bound = lay(r.bound) if init is None else lay(r.bound) + init.double().abs()
    o = Out(lay(r.ref), bound, lay(r.deg2), init=init, shape=shape)
    o.degh = None if r.degh is None else lay(r.degh)
    o.derived = False
    return o


def p_conv3(seed, n, H, W, Cin, Cout, entry="plain", bias=True, mask=NONE, colsum=False, res=False, res_alpha=0.1, res_pre=False,
            x_act=NONE, pre_scale=1.0, flags=0, off=None, data="unit", deferred=False, part=None, act=NONE, host=False):
    """Y [n][H][W][Cout] = [res + res_alpha *] (pre_scale conv3x3(x_act(X)) + bias [+ res]) * mask'(source), through
    entry = 'plain' mvk_conv3x3, 'y' mvk_conv3x3_y, 'res' mvk_conv3x3_res, 'f' mvk_conv3x3_f, 's' mvk_conv3x3_s, 's2'
    mvk_conv3x3_s2 (second output: the value before the residual sum), 's_part' mvk_conv3x3_s_part (part = (x_channels, x_off): X
    and the pack have x_channels channels, the launch convolves the Cin channels from x_off).  The references are those of the
    pre-activation; act != 0 is for the activation tests, which compare launches with each other.
    off: 'x' | 'bias' | 'y' | 'mask' at storage offset 1.  data: 'unit', 'spread' (images and weight rows over e^(+-3 sigma)),
    'loose' (operand bound 1000x above max |X|), 'tiny' (an image half and a weight row 2^-30 of the rest), 'chan' (input channels
    over e^(+-1.5 sigma): the operands of the 2304-term sums)."""
    import conv3_ref as R3

    xc, xo = part if part is not None else (Cin, 0)
    x, w, b, src, rs, cinit = R3.fwd_operands(seed, n, H, W, xc, Cout, spread=3.0 if data == "spread" else 0.0, tiny=data == "tiny",
                                              chan=1.5 if data == "chan" else 0.0)
    b = b if bias else None
    if mask == SIGMOID:
        src = torch.sigmoid(src)
    scaled = entry in ("s", "s2", "s_part")
    xb, wb = float(x.abs().max()) * (1000.0 if data == "loose" else 1.0), float(w.abs().max())
    r = R3.conv3_fwd(x[:, xo:xo + Cin], w[:, xo:xo + Cin], b, x_act=x_act, pre_scale=pre_scale, mask_src=src if mask else None,
                     mask_act=mask, res=rs if res else None, res_alpha=res_alpha, res_pre=res_pre, colsum=colsum,
                     floor_bounds=(xb, wb) if scaled else None, want_h=host)
    nhwc = lambda t: t.permute(0, 2, 3, 1)  # noqa: E731
    outs = [_out3(r["y"], nhwc, shape=(n, H, W, Cout))]
    if colsum:
        outs.append(_out3(r["colsum"], init=cinit))
    if entry == "s2":
        outs.append(_out3(r["a"], nhwc, shape=(n, H, W, Cout)))
    if host:
        return Prep(None, outs, deferred=deferred, flags=flags)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = dev()
    al = lambda t, name: None if t is None else (unaligned(t.to(d)) if off == name else t.contiguous().to(d))  # noqa: E731
    Xd, Wd, bd = al(_nhwc(x), "x"), R3.pack_fwd(w).to(d), al(b, "bias")
    sd, rd = al(_nhwc(src) if mask else None, "mask"), (_nhwc(rs).to(d) if res else None)
    yoff = unaligned(torch.full((n, H, W, Cout), float("nan"))) if off == "y" else None
    xam, wam, yam = torch.full((1,), xb, device=d), torch.full((1,), wb, device=d), torch.zeros(1, device=d)
    wsp, wsn = WS("ws")

    def run(bufs):
        Y = bufs[0] if yoff is None else yoff
        cs = ptr(bufs[1]) if colsum else None
        dims = (n, H, W, Cin, Cout)
        if entry == "plain":
            call("mvk_conv3x3", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, cs, wsp, wsn, stream_ptr())
        elif entry == "y":
            call("mvk_conv3x3_y", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, cs, ptr(yam), wsp, wsn, stream_ptr())
        elif entry == "res":
            call("mvk_conv3x3_res", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, ptr(rd), res_alpha, wsp, wsn,
                 stream_ptr())
        elif entry == "f":
            call("mvk_conv3x3_f", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, ptr(rd), res_alpha, cs, x_act,
                 pre_scale, wsp, wsn, stream_ptr())
        elif entry == "s":
            call("mvk_conv3x3_s", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, ptr(rd), res_alpha, cs, x_act,
                 pre_scale, ptr(xam), ptr(wam), ptr(yam), wsp, wsn, stream_ptr())
        elif entry == "s2":
            call("mvk_conv3x3_s2", ptr(Xd), ptr(Wd), ptr(bd), ptr(Y), ptr(bufs[-1]), *dims, act, ptr(rd), res_alpha, ptr(xam),
                 ptr(wam), ptr(yam), wsp, wsn, stream_ptr())
        else:
            call("mvk_conv3x3_s_part", ptr(Xd), xc, xo, ptr(Wd), ptr(bd), ptr(Y), *dims, act, ptr(sd), mask, ptr(rd), int(res_pre),
                 x_act, pre_scale, ptr(xam), ptr(wam), ptr(yam), stream_ptr())
        if yoff is not None:
            bufs[0].copy_(yoff)

    p = Prep(run, outs, deferred=deferred, flags=flags, keep=[Xd, Wd, bd, sd, rd, xam, wam, yam, yoff])
    p.yam = yam
    return p


def p_conv3_wgrad(seed, n, H, W, Cin, Cout, entry="plain", x_act=NONE, dy_scale=1.0, db=False, ws="ws", det=True, deferred=False,
                  flags=0, data="unit", host=False):
    """dWref [Cout][Cin][3][3] += dy_scale * d/dW sum(conv3x3(x_act(X), W) dY), db [Cout] += dy_scale * sum dY, through entry =
    'plain' mvk_conv3x3_wgrad, 'f' mvk_conv3x3_wgrad_f, 's' mvk_conv3x3_wgrad_s.  ws: 'ws' ample, 'none' NULL, 'unaligned' (storage
    offset 1), or a number of floats."""
    import conv3_ref as R3

    x, dy, init, binit = R3.wgrad_operands(seed, n, H, W, Cin, Cout, spread=3.0 if data == "spread" else 0.0)
    xb, yb = float(x.abs().max()), float(dy.abs().max())
    r = R3.conv3_wgrad(x, dy, x_act=x_act, dy_scale=dy_scale, floor_bounds=(xb, yb) if entry == "s" else None, want_h=host)
    outs = [_out3(r["dw"], init=init)]
    if db:
        outs.append(_out3(r["db"], init=binit))
    if host:
        return Prep(None, outs, det=det, deferred=deferred, flags=flags)
    from multivae_amd._lib import call, ptr, stream_ptr

    d = dev()
    Xd, dYd = _nhwc(x).to(d), _nhwc(dy).to(d)
    xam, yam = torch.full((1,), xb, device=d), torch.full((1,), yb, device=d)
    if ws == "unaligned":
        import ctypes

        wsp, wsn = ctypes.c_void_p(_ws().data_ptr() + 4), _ws().numel() - 1
    elif isinstance(ws, int):
        wsp, wsn = WS("ws")[0], ws
    else:
        wsp, wsn = WS(ws)

    def run(bufs):
        dbp = ptr(bufs[1]) if db else None
        if entry == "plain":
            call("mvk_conv3x3_wgrad", ptr(Xd), ptr(dYd), ptr(bufs[0]), n, H, W, Cin, Cout, wsp, wsn, stream_ptr())
        elif entry == "f":
            call("mvk_conv3x3_wgrad_f", ptr(Xd), ptr(dYd), ptr(bufs[0]), dbp, n, H, W, Cin, Cout, x_act, dy_scale, wsp, wsn, stream_ptr())
        else:
            call("mvk_conv3x3_wgrad_s", ptr(Xd), ptr(dYd), ptr(bufs[0]), dbp, n, H, W, Cin, Cout, x_act, dy_scale, ptr(xam), ptr(yam),
                 wsp, wsn, stream_ptr())

    return Prep(run, outs, det=det, deferred=deferred, flags=flags, keep=[Xd, dYd, xam, yam])


# ---- the dispatch table -------------------------------------------------------------------------------------------------
@dataclass
class Case:
    id: str
    make: object       # () -> Prep
    expect: tuple      # device kernels of the default configuration (engine 1)
    f32: tuple = None  # ... with MVK_ENGINE=f32 (None: the same)
    note: str = ""     # the host rule the route relies on


def case(id_, fn, kw, expect, f32=None, note=""):
    c = Case(id_, lambda: fn(zlib.crc32(id_.encode()) % 100003, **kw), tuple(sorted(expect)), None if f32 is None else tuple(sorted(f32)), note)
    c.fn, c.kw = fn, kw  # (tests/test_conv3_ref_host.py builds the host references of the 3x3 cases from them)
    return c


CASES = [
    # --- mvk_linear_fwd (igemm.hip:793-822): K > 32 (smallk), M > 1024 or unaligned X or K % 4 (heads_launch), launch_auto:
    # split K (512-block target) when scratch, < 128 128x64 tiles and K >= 256 (igemm.hip:787-791)
    case("linfwd-bf128x32-plainK-bmK-z1-rowmajor-bias-relu", p_linear_fwd, dict(M=4096, N=20, K=200, act=RELU),
         [bf(128, 32, "K", "K")], [fast(128, 32, 32, "K", "K")], "N <= 32 -> 128x32 (igemm.hip:295); 32 tiles, K < 256: z = 1"),
    case("linfwd-bf128x32-plainK-bmK-z1-N32-M4097", p_linear_fwd, dict(M=4097, N=32, K=96, act=LEAKY),
         [bf(128, 32, "K", "K")], [fast(128, 32, 32, "K", "K")], "N = 32 still 128x32; ragged last row tile"),
    case("linfwd-fast64x64-plainK-bmK-z1-N33-sigmoid", p_linear_fwd, dict(M=4096, N=33, K=200, act=SIGMOID),
         [fast(64, 64, 32, "K", "K")], None, "N = 33: 32 128x64 blocks < bf_min_blocks (256) -> exact 64x64 (igemm.hip:315)"),
    case("linfwd-bf128x32-plainK-bmK-splitk_ws-bias-relu", p_linear_fwd, dict(M=2048, N=20, K=1000, act=RELU),
         [bf(128, 32, "K", "K"), RED], [fast(128, 32, 32, "K", "K"), RED],
         "16 tiles: 32 slices of 2 k-tiles, ordered slabs + splitk_reduce (igemm.hip:402-409); K % 16 = 8"),
    case("linfwd-bf128x32-plainK-bmK-splitk_ws-odd-ksplit", p_linear_fwd, dict(M=2048, N=24, K=1040, bias=False),
         [bf(128, 32, "K", "K"), RED], [fast(128, 32, 32, "K", "K"), RED],
         "65 k-tiles / 32 splits = 3 -> rounded to 4 (igemm.hip:391): 17 slices, the last one 1 k-tile"),
    case("linfwd-bf128x64-plainK-bmK-z1-256blocks", p_linear_fwd, dict(M=32768, N=64, K=64),
         [bf(128, 64, "K", "K")], [fast(64, 64, 32, "K", "K")], "256 128x64 blocks = bf_min_blocks (igemm.hip:299)"),
    case("linfwd-fast64x64-plainK-bmK-z1-255blocks", p_linear_fwd, dict(M=32640, N=64, K=64),
         [fast(64, 64, 32, "K", "K")], None, "255 blocks: one below bf_min_blocks"),
    case("linfwd-bf128x64-plainK-bmK-z1-N65", p_linear_fwd, dict(M=16384, N=65, K=64, act=RELU),
         [bf(128, 64, "K", "K")], [fast(64, 64, 32, "K", "K")], "N = 65: 128 x 2 = 256 blocks; f32: 128 128x128 blocks < 384"),
    case("linfwd-bf128x64-plainK-bmK-z1-384blocks", p_linear_fwd, dict(M=49152, N=64, K=64),
         [bf(128, 64, "K", "K")], [fast(128, 64, 32, "K", "K")], "f32 engine: 384 128x64 blocks -> 128x64 (igemm.hip:314)"),
    case("linfwd-bf128x64-plainK-bmK-z1-N128-384blocks", p_linear_fwd, dict(M=49152, N=128, K=64),
         [bf(128, 64, "K", "K")], [fast(128, 128, 16, "K", "K")], "f32 engine: 384 128x128 blocks, N > 64 -> 128x128 (igemm.hip:312)"),
    case("linfwd-gen128x32-unalignedA", p_linear_fwd, dict(M=300, N=20, K=100, x_off=True),
         [gen(128, 32)], None, "X at storage offset 1: no vec4 -> generic (igemm.hip:268, 345); heads_launch declines"),
    case("linfwd-gen64x64-unalignedA", p_linear_fwd, dict(M=50, N=60, K=100, x_off=True, act=RELU),
         [gen(64, 64)], None, "generic, N <= 64, M <= 64 (igemm.hip:347)"),
    case("linfwd-gen128x64-unalignedA-splitk_ws", p_linear_fwd, dict(M=300, N=64, K=300, x_off=True),
         [gen(128, 64), RED], None, "generic, N <= 64, M > 64; 3 tiles, K >= 256: split K (10 slices)"),
    case("linfwd-gen128x128-unalignedA", p_linear_fwd, dict(M=2048, N=1536, K=64, x_off=True),
         [gen(128, 128)], None, "generic, 192 128x128 blocks (igemm.hip:351)"),
    case("linfwd-gen128x32-Kmod4-splitk_ws", p_linear_fwd, dict(M=2000, N=20, K=258, act=LEAKY),
         [gen(128, 32), RED], None, "K % 4 = 2: no vec4 (igemm.hip:423); 16 tiles, K >= 256: 9 slices"),
    case("linfwd-heads4-fewrows", p_linear_fwd, dict(M=1000, N=50, K=400, act=RELU),
         [H4], None, "M <= 1024, K >= 64 (igemm.hip:807); K < 1024: 4 waves (skinny.hip:386)"),
    case("linfwd-heads16-fewrows", p_linear_fwd, dict(M=512, N=40, K=1024),
         [H16], None, "K >= 1024: 16 waves (skinny.hip:384)"),
    case("linfwd-heads16-ksplit_ws", p_linear_fwd, dict(M=32, N=32, K=4096),
         [H16, HFIN], None, "4 tiles, K >= 2048, scratch: K split over 16 workgroups + ordered finish (skinny.hip:359-366)"),
]

# narrow_fwd_kernel (one head, 16 < N <= 32, M >= 1024) is reached through mvk_linear_fwd at exactly M = 1024
_NARROW = [(17, 64, True, NONE), (17, 100, False, RELU), (17, 400, True, SIGMOID), (17, 2048, True, LEAKY),
           (20, 64, False, LEAKY), (20, 100, True, NONE), (20, 400, True, RELU), (20, 2048, False, SIGMOID),
           (32, 64, True, SIGMOID), (32, 100, True, LEAKY), (32, 400, False, NONE), (32, 2048, True, RELU)]
for _N, _K, _b, _a in _NARROW:
    CASES.append(case(f"linfwd-narrow-M1024-N{_N}-K{_K}-{'bias' if _b else 'nobias'}-act{_a}", p_linear_fwd,
                      dict(M=1024, N=_N, K=_K, bias=_b, act=_a), [NARROW], None,
                      "heads_launch: one head, 16 < N <= 32, M >= 1024 (skinny.hip:369); K = 100: partial last k-block"))
CASES += [
    case("linfwd-narrow-M1024-N20-K400-allacts-sigmoid-wvec", p_linear_fwd, dict(M=1024, N=20, K=400, act=SIGMOID),
         [NARROW], None, "16-byte weight rows (wvec)"),
    case("heads_fwd-narrow-kn-M1024-N20-K400", p_heads_kn, dict(M=1024, N=20, K=400),
         [NARROW], None, "mvk_heads_fwd, W1 = NULL, [K][N] weights: strided loads (wvec = 0)"),
    case("heads_fwd-narrow-kn-M2048-N32-K100", p_heads_kn, dict(M=2048, N=32, K=100),
         [NARROW], None, "mvk_heads_fwd, one head, M > 1024"),
    case("linfwd-narrow-declines-M1024-K130", p_linear_fwd, dict(M=1024, N=20, K=130, act=RELU),
         [gen(128, 32)], None, "K % 4 != 0: heads_launch declines (skinny.hip:335), the tiled generic kernel takes it"),
    case("linfwd-M1025-N20-K400-bf128x32-splitk_ws", p_linear_fwd, dict(M=1025, N=20, K=400, act=RELU),
         [bf(128, 32, "K", "K"), RED], [fast(128, 32, 32, "K", "K"), RED], "M = 1025: past the few-row limit; 9 tiles, 13 slices"),
    case("linfwd-M1025-N17-K100-bf128x32-z1", p_linear_fwd, dict(M=1025, N=17, K=100),
         [bf(128, 32, "K", "K")], [fast(128, 32, 32, "K", "K")], "M = 1025, K < 256: one slice"),
    case("linfwd-M1025-N32-K2048-bf128x32-splitk_ws", p_linear_fwd, dict(M=1025, N=32, K=2048, act=SIGMOID),
         [bf(128, 32, "K", "K"), RED], [fast(128, 32, 32, "K", "K"), RED], "M = 1025: 9 tiles, 56 slices of 2 k-tiles"),

    # --- mvk_linear_bwd_data (igemm.hip:824-853): A = dY (AM_PLAIN_K, act mask = y_out), B = W (BM_N), E mask = prev_out
    case("bwdd-bf128x32-plainK-bmN-z1", p_linear_bwd_data, dict(M=4096, N=200, K=20),
         [bf(128, 32, "K", "N")], [fast(128, 32, 32, "K", "N")], "reduction 200 < 256: z = 1"),
    case("bwdd-bf128x32-plainK-bmN-aact-relu-prevmask-leaky", p_linear_bwd_data, dict(M=4096, N=200, K=20, y_act=RELU, prev_act=LEAKY),
         [bf(128, 32, "K", "N", True)], [fast(128, 32, 32, "K", "N", True)], "AACT instantiation (igemm.hip:224)"),
    case("bwdd-bf128x64-plainK-bmN-aact-relu", p_linear_bwd_data, dict(M=32768, N=100, K=64, y_act=RELU),
         [bf(128, 64, "K", "N", True)], [fast(64, 64, 32, "K", "N", True)], "256 blocks"),
    case("bwdd-accumulate-bf128x32-splitk_ws", p_linear_bwd_data, dict(M=512, N=1000, K=20, accumulate=True),
         [bf(128, 32, "K", "N"), RED], [fast(128, 32, 32, "K", "N"), RED], "atomic -> launch_splitk: 32 slices, ordered slabs"),
    case("bwdd-accumulate-noscratch-atomic", p_linear_bwd_data, dict(M=512, N=1000, K=20, accumulate=True, ws="none"),
         [bf(128, 32, "K", "N")], [fast(128, 32, 32, "K", "N")], "ws = NULL: fp32-atomic split K (igemm.hip:411-412)"),
    case("bwdd-accumulate-shortscratch-atomic", p_linear_bwd_data, dict(M=512, N=1000, K=20, accumulate=True, ws="short"),
         [bf(128, 32, "K", "N")], [fast(128, 32, 32, "K", "N")], "ws_floats one below z M N: fp32-atomic split K"),
    case("bwdd-accumulate-fast64x64-splitk_ws-prevmask", p_linear_bwd_data, dict(M=512, N=1000, K=64, accumulate=True, prev_act=RELU),
         [fast(64, 64, 32, "K", "N"), RED], None, "N = 64: 4 x 32 = 128 blocks < 256 -> exact 64x64"),
    case("bwdd-accumulate-deferred", p_linear_bwd_data, dict(M=512, N=1000, K=20, accumulate=True, deferred=True),
         [bf(128, 32, "K", "N"), BATCH], [fast(128, 32, 32, "K", "N"), BATCH], "dX inside the flat gradient buffer: deferred slabs"),
    case("bwdd-colsum-fused-bf128x32", p_linear_bwd_data, dict(M=4096, N=200, K=20, colsum=True),
         [bf(128, 32, "K", "N"), FIN], [fast(128, 32, 32, "K", "N"), FIN], "launch_with_colsum: partials in the epilogue (igemm.hip:687-702)"),
    case("bwdd-colsum-fused-fast64x64-prevmask", p_linear_bwd_data, dict(M=1000, N=200, K=64, colsum=True, prev_act=RELU),
         [fast(64, 64, 32, "K", "N"), FIN], None, "fused column sums of the masked output"),
    case("bwdd-colsum-Kmod4-generic-scalarfinish", p_linear_bwd_data, dict(M=1000, N=64, K=21, colsum=True),
         [gen(128, 32), CS1, FINS], None, "K % 4 != 0: generic, separate column sums, N % 4 != 0 -> scalar finish (igemm.hip:624-625)"),
    case("bwdd-colsum-splitk_ws-then-colsum", p_linear_bwd_data, dict(M=512, N=1000, K=64, colsum=True),
         [fast(64, 64, 32, "K", "N"), RED, CS4, FIN], None, "4 tiles, reduction >= 256: split K, then the column-sum pass (igemm.hip:851-852)"),

    # --- mvk_linear_bwd_weight (igemm.hip:855-874): A = dY^T (AM_PLAIN_R), B = X (BM_N), atomic, split K for 768 blocks
    case("bwdw-bf128x64-plainR-bmN-splitk_ws-db", p_linear_bwd_weight, dict(M=4096, N=64, K=400),
         [bf(128, 64, "R", "N"), RED, CS4, FIN], [fast(128, 64, 32, "R", "N"), RED, CS4, FIN],
         "7 tiles x 64 slices = 448 blocks; f32 engine: >= 384 -> 128x64"),
    case("bwdw-bf128x32-plainR-bmN-aact-splitk_ws-db", p_linear_bwd_weight, dict(M=4096, N=20, K=20, y_act=RELU),
         [bf(128, 32, "R", "N", True), RED, CS4, FIN], [fast(128, 32, 32, "R", "N", True), RED, CS4, FIN], "N = 20 latent width"),
    case("bwdw-bf128x64-plainR-bmN-aact-sigmoid-nodb", p_linear_bwd_weight, dict(M=2048, N=64, K=256, y_act=SIGMOID, db=False),
         [bf(128, 64, "R", "N", True), RED], [fast(64, 64, 32, "R", "N", True), RED], "4 tiles x 64 slices = 256 blocks"),
    case("bwdw-noscratch-atomic", p_linear_bwd_weight, dict(M=4096, N=64, K=400, ws="none"),
         [bf(128, 64, "R", "N"), CS4], [fast(128, 64, 32, "R", "N"), CS4], "ws = NULL: atomic slices, atomic column sums"),
    case("bwdw-deferred", p_linear_bwd_weight, dict(M=4096, N=64, K=400, deferred=True),
         [bf(128, 64, "R", "N"), CS4, BATCH], [fast(128, 64, 32, "R", "N"), CS4, BATCH], "dW, db in the flat gradient buffer"),
    case("bwdw-Nmod4-generic-scalarfinish", p_linear_bwd_weight, dict(M=2000, N=21, K=40),
         [gen(64, 64), RED, CS1, FINS], None, "N % 4 != 0: A not vec4 -> generic; scalar column-sum finish"),

    # --- mvk_gemm (igemm.hip:923-955): every ta / tb, bias period, activation, both masks, accumulate
    case("gemm-ta0tb0-bf128x32-plainK-bmN-biasmod13-leaky", p_gemm, dict(M=4096, N=20, K=100, bias_mod=13, act=LEAKY),
         [bf(128, 32, "K", "N")], [fast(128, 32, 32, "K", "N")], "bias_mod % 4 != 0: scalar epilogue"),
    case("gemm-ta0tb1-fast64x64-plainK-bmK-bias-relu", p_gemm, dict(M=4096, N=48, K=100, tb=1, bias_mod=48, act=RELU),
         [fast(64, 64, 32, "K", "K")], None, "N = 48: 32 blocks"),
    case("gemm-ta1tb0-bf128x32-plainR-bmN", p_gemm, dict(M=4096, N=20, K=100, ta=1),
         [bf(128, 32, "R", "N")], [fast(128, 32, 32, "R", "N")], "A^T: AM_PLAIN_R"),
    case("gemm-ta1tb1-generic", p_gemm, dict(M=4096, N=20, K=100, ta=1, tb=1, bias_mod=20, act=SIGMOID),
         [gen(128, 32)], None, "AM_PLAIN_R + BM_K is not instantiated (igemm.hip:202, 230) -> generic"),
    case("gemm-ta0tb1-aact-generic", p_gemm, dict(M=4096, N=20, K=100, tb=1, a_act=RELU),
         [gen(128, 32)], None, "AM_PLAIN_K + BM_K + AACT is not instantiated -> generic"),
    case("gemm-ta0tb0-aact-cact-accumulate-splitk_ws", p_gemm, dict(M=4096, N=20, K=100, accumulate=True, a_act=RELU, c_act=LEAKY),
         [bf(128, 32, "K", "N", True), RED], [fast(128, 32, 32, "K", "N", True), RED], "accumulate: 32 tiles x 4 slices"),
    case("gemm-ta1tb0-aact-bf128x64", p_gemm, dict(M=16384, N=128, K=96, ta=1, a_act=LEAKY, bias_mod=128),
         [bf(128, 64, "R", "N", True)], [fast(64, 64, 32, "R", "N", True)], "256 blocks, AM_PLAIN_R + AACT"),
    case("gemm-ta1tb1-accumulate-noscratch-generic-atomic", p_gemm, dict(M=300, N=20, K=600, ta=1, tb=1, accumulate=True, ws="none"),
         [gen(128, 32)], None, "generic kernel with fp32-atomic split K"),
]
# tile edges: M, N one below / at / one above 32, 64, 128, 256; K at 15..17 and 31..33 (accumulate keeps K <= 32 off the
# short-reduction kernel, igemm.hip:928)
_EDGES = [(31, 33, 15, [gen(64, 64)]), (32, 32, 16, [bf(128, 32, "K", "N")]),
          (33, 65, 17, [gen(64, 64)]), (63, 64, 16, [fast(64, 64, 32, "K", "N")]), (64, 128, 32, [fast(64, 64, 32, "K", "N")]),
          (65, 129, 33, [gen(64, 64), RED]), (127, 31, 31, [gen(128, 32)]), (128, 256, 32, [fast(64, 64, 32, "K", "N")]),
          (129, 257, 16, [gen(64, 64)]), (255, 33, 32, [gen(128, 64)]), (256, 32, 16, [bf(128, 32, "K", "N")]),
          (257, 63, 32, [gen(128, 64)])]
for _M, _N, _K, _e in _EDGES:
    _f = [fast(128, 32, 32, "K", "N") if x == bf(128, 32, "K", "N") else x for x in _e]
    CASES.append(case(f"gemm-edge-M{_M}-N{_N}-K{_K}-accumulate", p_gemm, dict(M=_M, N=_N, K=_K, accumulate=True, bias_mod=_N),
                      _e, _f if _f != _e else None, "K % 4 or N % 4 != 0 -> generic; z = 1 up to 2 k-tiles (K = 33: 2 slices)"))
CASES += [
    # --- column sums (igemm.hip:554-628, 876-921)
    case("colsum_acc-vec4-ws", p_colsum, dict(M=100, N=64), [CS4, FIN], None, "N % 4 = 0: float4 partials + ordered finish"),
    case("colsum_acc-vec4-ws-yact-relu", p_colsum, dict(M=100, N=64, y_act=RELU), [CS4, FIN]),
    case("colsum_acc-N21-ws-scalarfinish", p_colsum, dict(M=100, N=21), [CS1, FINS], None, "N % 4 != 0: scalar kernel and finish"),
    case("colsum_acc-vec4-noscratch-atomic", p_colsum, dict(M=100, N=64, ws="none"), [CS4], None, "no scratch: atomics"),
    case("act_bwd_colsum-fused-sigmoid", p_act_bwd_colsum, dict(M=2000, N=64, act=SIGMOID), ["act_bwd_colsum_kernel", FIN],
         None, "N % 4 = 0, aligned, scratch (igemm.hip:884)"),
    case("act_bwd_colsum-generic-N21-relu", p_act_bwd_colsum, dict(M=2000, N=21, act=RELU), ["act_bwd_plain_kernel", CS1, FINS],
         None, "N % 4 != 0: copy, elementwise pass, column sums (igemm.hip:886-893)"),
    case("act_bwd_colsum-generic-noscratch-leaky", p_act_bwd_colsum, dict(M=2000, N=64, act=LEAKY, ws="none"),
         ["act_bwd_plain_kernel", CS4], None, "no scratch: generic route, atomic column sums"),
    case("nchw_channel_sum-c24-finish", p_nchw_sum, dict(n=20, c=24, hw=8), ["nchw_channel_sum_kernel", FIN]),
    case("nchw_channel_sum-c21-relu-scalarfinish", p_nchw_sum, dict(n=20, c=21, hw=8, y_act=RELU),
         ["nchw_channel_sum_kernel", FINS]),

    # --- 4x4 / stride-2 convolutions on the tiled path (register-stationary kernels off: mvk_debug_set_flags(0x100 | 0x400))
    case("down-fast64x64-row-bmN-nhwc-bias-relu", p_conv_down, dict(n=64, h=8, w=8, Cu=32, Cv=64),
         [fast(64, 64, 32, "ROW", "N")], None, "AM_ROW gather, 32 blocks"),
    case("down-bf128x32-row-bmN-nhwc", p_conv_down, dict(n=64, h=8, w=8, Cu=32, Cv=32, act=NONE),
         [bf(128, 32, "ROW", "N")], [fast(128, 32, 32, "ROW", "N")], "Cv <= 32, C % 32 = 0"),
    case("down-bf128x64-row-bmN-nhwc-256blocks", p_conv_down, dict(n=512, h=8, w=8, Cu=32, Cv=36, act=SIGMOID),
         [bf(128, 64, "ROW", "N")], [fast(64, 64, 32, "ROW", "N")], "32768 positions: 256 blocks"),
    case("down-C48-generic128x32", p_conv_down, dict(n=16, h=8, w=8, Cu=48, Cv=32),
         [gen(128, 32)], None, "C % 32 = 16: no split engine, small grid -> generic (igemm.hip:308)"),
    case("down-fast256x32x16-C16", p_conv_down, dict(n=2048, h=8, w=8, Cu=16, Cv=20, cap=48),
         [fast(256, 32, 16, "ROW", "N")], None, "C % 32 = 16, N <= 32, 512 256-row blocks (igemm.hip:307)"),
    case("down-fast128x128x16-C16", p_conv_down, dict(n=768, h=8, w=8, Cu=16, Cv=72, cap=48),
         [fast(128, 128, 16, "ROW", "N")], None, "C % 32 = 16, N > 64, 384 128x128 blocks (igemm.hip:312)"),
    case("down-C6-novec4-generic", p_conv_down, dict(n=16, h=8, w=8, Cu=6, Cv=32), [gen(128, 32)], None, "C % 4 != 0"),
    case("down-nchw-generic", p_conv_down, dict(n=16, h=8, w=8, Cu=32, Cv=40, u_nchw=True),
         [gen(128, 64)], None, "NCHW source: A_DOWN_NCHW -> generic; Cv = 40 is no small-kernel shape"),
    case("down-uact-generic", p_conv_down, dict(n=16, h=8, w=8, Cu=32, Cv=64, u_act=RELU),
         [gen(128, 64)], None, "act-source gathered operand -> generic (igemm.hip:277)"),
    case("down-vact-colsum-fused-fast64x64", p_conv_down, dict(n=64, h=8, w=8, Cu=32, Cv=64, v_act=RELU, colsum=True),
         [fast(64, 64, 32, "ROW", "N"), FIN], None, "epilogue mask + fused column sums"),
    case("down-nchw-colsum-generic", p_conv_down, dict(n=16, h=8, w=8, Cu=4, Cv=32, u_nchw=True, colsum=True),
         [gen(128, 32), CS4, FIN], None, "NCHW network input with colsum_acc: generic + separate column sums"),
    case("up-bf128x32-row-parity-Eup-bias", p_conv_up, dict(n=64, h=4, w=4, Cu=32, Cv=64),
         [bf(128, 32, "ROW", "N")], [fast(128, 32, 32, "ROW", "N")], "E_UP, 4 parities (z)"),
    case("up-fast64x64-row-Eupnchw-relu", p_conv_up, dict(n=64, h=4, w=4, Cu=64, Cv=64, u_nchw=True, act=RELU),
         [fast(64, 64, 32, "ROW", "N")], None, "E_UP_NCHW"),
    case("up-bf128x64-row-Eup-256blocks", p_conv_up, dict(n=512, h=4, w=4, Cu=64, Cv=64),
         [bf(128, 64, "ROW", "N")], [fast(64, 64, 32, "ROW", "N")], "8192 positions x 4 parities: 256 blocks"),
    case("up-uact-colsum-fused-bf128x32", p_conv_up, dict(n=64, h=4, w=4, Cu=32, Cv=64, u_act=RELU, colsum=True),
         [bf(128, 32, "ROW", "N"), FIN], [fast(128, 32, 32, "ROW", "N"), FIN], "E_UP mask + fused column sums"),
    case("up-C48-generic", p_conv_up, dict(n=16, h=4, w=4, Cu=32, Cv=48, act=SIGMOID),
         [gen(128, 32)], None, "C % 32 = 16, small grid -> generic"),
    case("wgrad-bf128x64-col-splitk_ws-convref16", p_conv_wgrad, dict(n=64, h=4, w=4, Cu=64, Cv=128),
         [bf(128, 64, "COL", "N"), RED], [fast(64, 64, 32, "COL", "N"), RED], "AM_COL, 16 tiles x 16 slices (SPLITK_C4 = 256)"),
    case("wgrad-bf128x32-col-splitk_ws", p_conv_wgrad, dict(n=64, h=8, w=8, Cu=32, Cv=32),
         [bf(128, 32, "COL", "N"), RED], [fast(128, 32, 32, "COL", "N"), RED], "Cv <= 32"),
    case("wgrad-nchw-generic", p_conv_wgrad, dict(n=16, h=8, w=8, Cu=32, Cv=40, u_nchw=True),
         [gen(128, 64), RED], None, "NCHW source -> generic"),
    case("wgrad-uact-generic", p_conv_wgrad, dict(n=16, h=8, w=8, Cu=32, Cv=64, u_act=RELU),
         [gen(128, 64), RED], None, "act-source gathered operand -> generic"),
    case("wgrad-deferred", p_conv_wgrad, dict(n=64, h=4, w=4, Cu=64, Cv=128, deferred=True),
         [bf(128, 64, "COL", "N"), BATCH], [fast(64, 64, 32, "COL", "N"), BATCH], "deferred slabs"),
    case("wgrad-noscratch-atomic", p_conv_wgrad, dict(n=64, h=4, w=4, Cu=64, Cv=128, ws="none"),
         [bf(128, 64, "COL", "N")], [fast(64, 64, 32, "COL", "N")], "fp32-atomic split K"),
    case("wgradpair-bfpair128x64-col-deferred", p_conv_wgrad_pair, dict(n=PAIR_N),
         [PAIRK, BATCH], [fast(64, 64, 32, "COL", "N"), BATCH],
         "both layers split into >= 256 blocks of the 128x64 split-bf16 tile, gradients in the arena: ONE launch (igemm.hip "
         "mvk_conv4s2_wgrad_pair); f32 engine: two launches"),
    case("wgradpair-notdeferred-two-launches", p_conv_wgrad_pair, dict(n=PAIR_N, deferred=False),
         [bf(128, 64, "COL", "N"), RED], [fast(64, 64, 32, "COL", "N"), RED], "no arena: two mvk_conv4s2_wgrad launches"),
    case("wgradpair-below-n-two-launches", p_conv_wgrad_pair, dict(n=PAIR_N - 1),
         [bf(128, 64, "COL", "N"), fast(64, 64, 32, "COL", "N"), BATCH], [fast(64, 64, 32, "COL", "N"), BATCH],
         "n = 31: 4 tiles x 62 slices = 248 < 256 blocks at 32 -> 64 channels -> two launches (the first on the exact-fp32 tile)"),
    case("unflatten-bf128x64-plainR-bmN-Eunflatref", p_unflatten, dict(n=512, Cin=20, Cout=64),
         [bf(128, 64, "R", "N"), RED], [fast(64, 64, 32, "R", "N"), RED], "E_UNFLATREF, 16 tiles x 16 slices"),
    case("flatten-bf128x32-plainR-bmN-Econvref16", p_flatten, dict(n=512, Cu=64, Cv=20),
         [bf(128, 32, "R", "N"), RED], [fast(128, 32, 32, "R", "N"), RED], "E_CONVREF (16 taps)"),

    # --- 3x3 / stride-1 convolutions on the tiled path (tw = 3, mul = 1 gather; the register-stationary kernels off: 0x400).
    # The image-side kernels of conv3small.hip have no switch: these shapes are ones they decline.
    case("c3fwd-bf128x32-row-bmN-small-grid", p_conv3, dict(n=3, H=7, W=7, Cin=32, Cout=32, flags=TILED_ONLY),
         [bf(128, 32, "ROW", "N")], [fast(128, 32, 32, "ROW", "N")], "AM_ROW gather of a 3x3 window; N <= 32: 2 blocks"),
    case("c3fwd-bf128x64-row-bmN-256blocks", p_conv3, dict(n=16, H=32, W=32, Cin=32, Cout=128, bias=False, flags=TILED_ONLY),
         [bf(128, 64, "ROW", "N")], [fast(64, 64, 32, "ROW", "N")], "16384 positions x 2 column tiles = 256 blocks"),
    case("c3bwdd-bf128x32-row-mask-colsum-fused", p_conv3,
         dict(n=3, H=7, W=7, Cin=64, Cout=32, bias=False, mask=LEAKY, colsum=True, flags=TILED_ONLY),
         [bf(128, 32, "ROW", "N"), FIN], [fast(128, 32, 32, "ROW", "N"), FIN], "backward-data form: epilogue mask + fused column sums"),
    case("c3bwdd-bf128x64-row-mask-colsum-256blocks", p_conv3,
         dict(n=16, H=32, W=32, Cin=32, Cout=128, bias=False, mask=RELU, colsum=True, flags=TILED_ONLY),
         [bf(128, 64, "ROW", "N"), FIN], [fast(64, 64, 32, "ROW", "N"), FIN], "128 row tiles of partial column sums"),
    case("c3fwd-generic-K27-Cout6", p_conv3, dict(n=2, H=5, W=5, Cin=3, Cout=6), [gen(128, 32)], None,
         "Cout % 4 != 0: conv3_smallcin declines; Cin % 4 != 0: no vec4 -> generic, K = 27"),
    case("c3fwd-generic-Cin6-Cout10", p_conv3, dict(n=1, H=5, W=9, Cin=6, Cout=10, mask=RELU), [gen(128, 32)], None, "Cin % 4 != 0"),
    case("c3fwd-generic-N3-Cin24", p_conv3, dict(n=2, H=5, W=5, Cin=24, Cout=3), [gen(128, 32)], None,
         "Cin % 16 != 0: conv3_smallcout declines; N = 3: the weight pack has no 16-byte rows -> generic"),
    case("c3res-bf128x32-row-residual-mask", p_conv3,
         dict(n=3, H=7, W=7, Cin=32, Cout=32, entry="res", res=True, mask=LEAKY, flags=TILED_ONLY),
         [bf(128, 32, "ROW", "N")], [fast(128, 32, 32, "ROW", "N")], "mvk_conv3x3_res: res + alpha * (.) in the epilogue"),
    case("c3fwd-bf128x32-row-K2304", p_conv3, dict(n=2, H=7, W=7, Cin=256, Cout=32, flags=TILED_ONLY),
         [bf(128, 32, "ROW", "N")], [fast(128, 32, 32, "ROW", "N")],
         "K = 2304 in one accumulator chain (no split K in the forward): 0.17x the bound on the split engine, 0.28x on the exact one"),
    case("c3wgrad-bf128x64-col-splitk_ws-convref9", p_conv3_wgrad, dict(n=64, H=4, W=4, Cin=64, Cout=128, flags=TILED_ONLY),
         [bf(128, 64, "COL", "N"), RED], [fast(64, 64, 32, "COL", "N"), RED],
         "AM_COL, E_CONVREF with taps = 9; 10 tiles x 32 slices of 2 k-tiles (target 768) = 320 blocks"),
    case("c3wgrad-deferred", p_conv3_wgrad, dict(n=64, H=4, W=4, Cin=64, Cout=128, deferred=True, flags=TILED_ONLY),
         [bf(128, 64, "COL", "N"), BATCH], [fast(64, 64, 32, "COL", "N"), BATCH], "deferred slabs"),
    case("c3wgrad-noscratch-atomic", p_conv3_wgrad, dict(n=64, H=4, W=4, Cin=64, Cout=128, ws="none", det=False, flags=TILED_ONLY),
         [bf(128, 64, "COL", "N")], [fast(64, 64, 32, "COL", "N")], "fp32-atomic split K"),
]


# ---- running a case ------------------------------------------------------------------------------------------------------
def _flags(f):
    import ctypes

    from multivae_amd import _lib

    lib = _lib.load()
    lib.mvk_debug_set_flags.argtypes = [ctypes.c_int]
    lib.mvk_debug_set_flags(f)


def execute(p):
    """One launch from the case's initial buffers; returns the buffers (device) and the run closure's kernels are profiled
    by the caller."""
    from multivae_amd import schedule

    d = dev()
    shapes = [o.shape or tuple(o.ref.shape) for o in p.outs]
    if p.deferred:
        sizes = [math.prod(s) for s in shapes]
        flat = torch.zeros(sum((n + 63) // 64 * 64 for n in sizes), device=d)
        flat.grad = torch.zeros_like(flat)
        bufs, off = [], 0
        for s, n in zip(shapes, sizes):
            bufs.append(flat.grad[off:off + n].view(s))
            off += (n + 63) // 64 * 64
    else:
        flat = None
        bufs = [torch.empty(s, device=d) for s in shapes]
    for b, o in zip(bufs, p.outs):
        if o.init is not None:
            b.copy_(o.init.to(d))
        else:
            b.fill_(float("nan"))  # every entry must be written

    def run():
        _flags(p.flags)
        try:
            if flat is not None:
                with schedule.deferred_reductions(flat):
                    p.call(bufs)
            else:
                p.call(bufs)
        finally:
            _flags(0)

    return bufs, run


def check_case(c, engine_f32=F32_ENGINE, collect=False):
    """Run one case and check it; with collect=True return (report, failures) instead of asserting."""
    torch.backends.cuda.matmul.allow_tf32 = False
    torch.backends.cudnn.allow_tf32 = False
    fails, report = [], {}
    p = c.make()
    bufs, run = execute(p)
    names = launched_kernels(run)
    report["kernels"] = names
    want = sorted(c.f32 if engine_f32 and c.f32 is not None else c.expect)
    if not names:
        fails.append("the profiler recorded no device kernel for a launch that must run one")
    elif names != want:
        fails.append(f"launched {names}, expected {want} ({c.note})")
    got = [b.detach().cpu().double() for b in bufs]
    rejected = []
    for i, (o, t) in enumerate(zip(p.outs, got)):
        if o.rows is not None:
            t = t[o.rows]
        if o.init is not None:
            t = t - o.init.double()
        assert t.shape == o.ref.shape, (c.id, i, t.shape, o.ref.shape)
        if not bool(torch.isfinite(t).all()):
            fails.append(f"output {i} has entries that are NaN / inf (or were never written)")
            continue
        tol = C_ENTRY * o.bound + o.slack * o.ref.abs() + 1e-30
        err = (t - o.ref).abs()
        worst = float((err / tol).max())
        dworst = float(((o.deg - o.ref).abs() / tol).max())  # the two-piece emulation against the same bound
        report[f"out{i}"] = dict(worst=worst, degraded=dworst)
        rejected.append(dworst > 1.0)
        if worst > 1.0:
            fails.append(f"output {i}: {int((err > tol).sum())} of {err.numel()} entries above {C_ENTRY:g} sum|a b|; "
                         f"worst {worst:.2f}x the bound")
    if p.agg is not None:
        o = p.outs[0]
        rows = o.rows if o.rows is not None else slice(None)
        tg = p.agg().cpu()[rows]
        g0 = got[0][rows]
        if o.init is not None:
            g0 = g0 - o.init.double()[rows]
        e = [(x - o.ref).abs() for x in (g0, tg, o.deg)]
        mx = [float(x.max()) for x in e]
        rms = [float(x.pow(2).mean().sqrt()) for x in e]
        report["agg"] = dict(max=mx, rms=rms)
        if not (mx[0] <= 2 * mx[1] + 1e-30 and rms[0] <= 2 * rms[1] + 1e-30):
            fails.append(f"max / rms error {mx[0]:.3e} / {rms[0]:.3e} vs torch fp32 {mx[1]:.3e} / {rms[1]:.3e}")
        rejected.append(mx[2] > 2 * mx[1] or rms[2] > 2 * rms[1])
    if not any(rejected):
        fails.append(f"no teeth: the two-piece operands pass every check ({report})")
    if p.det:  # the reduction contract: a launch with scratch is reproducible to the bit
        bufs2, run2 = execute(p)
        run2()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(bufs, bufs2)):
            if not torch.equal(a, b):
                fails.append(f"output {i} differs between two runs of the same launch")
    if collect:
        return report, fails
    assert not fails, f"{c.id}: " + "; ".join(fails)
    return report


@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_dispatch_leaf(c):
    report = check_case(c)
    print(c.id, {k: v for k, v in report.items() if k != "kernels"})


def test_wgrad_pair_matches_two_launches():
    """igemm.hip's contract of mvk_conv4s2_wgrad_pair: same slabs, same sums as two mvk_conv4s2_wgrad launches under the same arena,
    so both gradients are bit-identical; without an arena the call is those two launches (ordered scratch slabs, the same bits)."""
    seed = 20231
    runs = {}
    for name, kw in (("pair", {}), ("single", dict(single=True)), ("plain", dict(deferred=False))):
        bufs, run = execute(p_conv_wgrad_pair(seed, PAIR_N, **kw))
        runs[name] = (launched_kernels(run), [b.clone() for b in bufs])
    if not F32_ENGINE:
        assert runs["pair"][0] == sorted([PAIRK, BATCH]) and runs["single"][0] == sorted([bf(128, 64, "COL", "N"), BATCH])
        assert runs["plain"][0] == sorted([bf(128, 64, "COL", "N"), RED])
    for i in range(2):
        assert torch.equal(runs["pair"][1][i], runs["single"][1][i]), f"dW{i}: pair vs two launches under the arena"
        assert torch.equal(runs["pair"][1][i], runs["plain"][1][i]), f"dW{i}: pair vs the not-deferred call"


def test_case_ids_are_unique():
    ids = [c.id for c in CASES]
    assert len(ids) == len(set(ids))


@pytest.mark.skipif(F32_ENGINE, reason="this is the parent of the MVK_ENGINE=f32 run")
def test_engine_f32_child():
    """MVK_ENGINE=f32 (exact-fp32 MFMA engine, include/mvk.h) is read once per process: the whole table again in a fresh
    child process (not an exec of this one), where every case expects its `f32` kernels."""
    env = dict(os.environ, MVK_ENGINE="f32")
    r = subprocess.run([sys.executable, "-s", "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.abspath(__file__) + "::test_dispatch_leaf"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, f"MVK_ENGINE=f32 child failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
