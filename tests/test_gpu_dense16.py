"""The MLP decoder on pre-split fp16 pair planes (csrc/dense16.hip), leaf by leaf, against float64.

The machinery is that of tests/test_gpu_gemm_dispatch.py (imported as D: launched_kernels, Prep, Out, execute, Case, C_ENTRY, WS); the
references, tolerances, degraded emulations and the restated launcher arithmetic are tests/dense16_ref.py, and
tests/test_dense16_ref_host.py shows on the CPU, for every case of CASES, that the case's degraded emulation leaves its tolerance,
that a float32 CPU evaluation stays inside it, that the exact value of the shipped three-product form stays at 0.8 of it and that the
regime the case names is the one its shape produces.  Each case

1. names its entry point and the exact set of device kernels it must launch (torch.profiler);
2. compares EVERY entry of every output with float64 of the DECODED planes the launch was given (operands of the GEMM kernels are
   planes built on the host by dense16_ref.split and uploaded, some under bounds 3.7x / 5.3x the true maxima):
   |got - ref| <= C_ENTRY (sum |a b| + |bias| + |initial|) + 2^-39 K a_bound rowmax_b, C_ENTRY = 5e-7; the NLL tail by the
   first-order rule of dense16_ref.nll_tail; d16_pack_kernel and d16_unsplit_kernel bit for bit;
3. carries the degraded emulation (the hi lo' cross term dropped; for plane outputs of fp32 arithmetic, the lo plane dropped), which
   must FAIL that check;
4. runs twice from the same buffers and must be bit-identical; every accumulating output (dW, db) starts from a non-zero buffer,
   every plain output from NaN; the G planes and rows_part carry a NaN guard behind row M - 1 that must stay NaN.

Chain lengths (basis of C_ENTRY: <= 1024 terms per fp32 accumulator chain): d16_first_kernel K <= 32 fmas; d16_nt_kernel K <= 784
per accumulator (a main and a cross one), bias gradient: <= 4 rows per thread, 16 row lanes, then <= 9 row tiles in order;
d16_tn_kernel <= 96 rows per slice (stated per case), then S <= 16 slabs in order.

Worst measured |got - ref| / tolerance per case on an MI355X, the degraded ratios, the yardstick of C_TAIL and the weakest rejection
of the table: profiles/NOTES_dense16.md.

Leaves of csrc/dense16.hip NOT reached here: mvk_dense16_debug flags 1 / 2 / 4 / 8 / 16 (probe switches of tools/dense16_probe.py
that skip loads, MFMAs, LDS writes or the epilogue: their results are wrong by design), the profiler slots (mvk_prof_slot: null
here), and MVK_DENSE16=0 (the generic path: test_gpu_kernels.py::test_mlp_decoder_fused_tail_matches_generic_path).  The 2^29
size limits of mvk_dense16_ok are not tested: a case would need buffers that large.
"""
import math
import os
import subprocess
import sys
import zlib

import pytest
import torch

import dense16_ref as R
import test_gpu_gemm_dispatch as D

pytestmark = pytest.mark.gpu

NONE, RELU, LEAKY = R.NONE, R.RELU, R.LEAKY
F16, F32, F64 = torch.float16, torch.float32, torch.float64
# MVK_D16_FWD_BM is read once per process (under MVK_TUNE=1): test_fwd_bm128_child re-runs the forward cases with 128-row tiles
FWD_BM = 128 if os.environ.get("MVK_TUNE") == "1" and os.environ.get("MVK_D16_FWD_BM") == "128" else 64
NT_FWD, NT_BWD, TN, SUM = f"d16_nt_kernel<{FWD_BM},0>", "d16_nt_kernel<64,1>", "d16_tn_kernel", "d16_sum_kernel"
PACK, UNSPLIT = "d16_pack_kernel", "d16_unsplit_kernel"
NAN = float("nan")


def _prep(call, checks, bufouts=(), deferred=False, **extra):
    """D.Prep of one launch.  checks: [(label, dict(ref, tol, deg, ...))] of EVERY checked output; bufouts: the labels that are fp32
    buffers of D.execute (in order), the others are side buffers that `collect` decodes after the run."""
    outs = []
    for label in bufouts:
        rd = dict(checks)[label]
        outs.append(D.Out(rd["ref"], rd["tol"] / D.C_ENTRY, rd["deg"], init=rd.get("init"), shape=rd.get("shape")))
    p = D.Prep(call, outs, deferred=deferred)
    p.checks, p.bufouts = checks, list(bufouts)
    p.reset = extra.pop("reset", lambda: None)        # refill the side buffers (NaN)
    p.collect = extra.pop("collect", lambda: {})      # () -> {label: float64 CPU tensor} of the side outputs
    p.exact = extra.pop("exact", lambda: [])          # () -> [(what, ok)] after the run
    p.raw = extra.pop("raw", lambda: [])              # () -> side buffers for the bit-identity of two runs
    p.meta = extra.pop("meta", {})
    p.keep = extra.pop("keep", [])
    assert not extra, extra
    return p


def _plain(name):
    """The function name of a kernel the profiler reports mangled (its demangler does not know _Float16 parameters): the last
    length-prefixed identifier of the nested name _ZN<len><id>...E; any other name as it is."""
    if not name.startswith("_ZN"):
        return name
    i, last = 3, name
    while i < len(name) and name[i].isdigit():
        j = i
        while name[j].isdigit():
            j += 1
        n = int(name[i:j])
        last, i = name[j:j + n], j + n
    return last


def launched(run):
    return sorted(_plain(n) for n in D.launched_kernels(run))


def _dev(*ts):
    return [None if t is None else t.to(D.dev()) for t in ts]


def _nanlike(shape, dtype=F32):
    return torch.full(shape, NAN, dtype=dtype, device=D.dev())


def _scalar(v):
    return torch.full((1,), float(v), device=D.dev())


def _biteq(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- mvk_dense16_pack ------------------------------------------------------------------------------------------------------------------
def p_pack(seed, N, K, host=False):
    W = R.pack_operand(seed, N, K)
    want = R.pack(W)
    meta = dict(W=W, want=want)
    if host:
        return _prep(None, [], meta=meta)
    from multivae_amd._lib import call, ptr, stream_ptr

    Wd, = _dev(W)
    shapes = dict(nk_hi=((N, K), F16), nk_lo=((N, K), F16), nk_inv=((N,), F32), kn_hi=((K, N), F16), kn_lo=((K, N), F16), kn_inv=((K,), F32))
    o = {}

    def reset():
        for k, (s, dt) in shapes.items():
            o[k] = _nanlike(s, dt)

    def run(bufs):
        call("mvk_dense16_pack", ptr(Wd), N, K, ptr(o["nk_hi"]), ptr(o["nk_lo"]), ptr(o["nk_inv"]), ptr(o["kn_hi"]), ptr(o["kn_lo"]),
             ptr(o["kn_inv"]), stream_ptr())

    def exact():
        res = [(f"{k} bit for bit", _biteq(o[k].cpu(), want[k])) for k in shapes]
        nk = R.decode(o["nk_hi"].cpu(), o["nk_lo"].cpu(), o["nk_inv"].cpu()[:, None])
        kn = R.decode(o["kn_hi"].cpu(), o["kn_lo"].cpu(), o["kn_inv"].cpu()[:, None])
        res.append(("the zero row and the zero column decode to 0", bool((nk[N // 2] == 0).all() and (nk[:, K // 3] == 0).all()
                                                                         and (kn[K // 3] == 0).all() and (kn[:, N // 2] == 0).all())))
        res.append(("a zero row carries 1 / 2^126", float(o["nk_inv"][N // 2]) == 2.0 ** -126 == float(o["kn_inv"][K // 3])))
        return res

    return _prep(run, [], reset=reset, exact=exact, raw=lambda: list(o.values()), meta=meta, keep=[Wd])


# ---- mvk_dense16_first -----------------------------------------------------------------------------------------------------------------
def p_first(seed, M, N, K, bias=True, act=RELU, loose=False, host=False):
    z, W, b = R.first_operands(seed, M, N, K)
    b = b if bias else None
    zam = float(z.abs().max()) * (R.LOOSE[1] if loose else 1.0)
    r = R.first(z, W, b, act, zam)
    pub = float(torch.tensor(r["bound_exact"], dtype=F32))  # the scale of the host emulations (the kernel publishes its own)
    cpu, ship, deg = R.first_emulations(r, pub)
    rd = dict(ref=r["ref"], tol=R.first_tol(r, r["bound_exact"]), deg=deg, ship=ship, cpu=cpu)
    meta = dict(cfg=R.first_cfg(M, N, K), bound_exact=r["bound_exact"], hmax=float(r["ref"].abs().max()), zam=zam, W=W, b=b)
    if host:
        return _prep(None, [("h", rd)], meta=meta)
    from multivae_amd._lib import call, ptr, stream_ptr

    zd, Wd, bd = _dev(z, W, b)
    zamd = _scalar(zam)
    o = {}

    def reset():
        o.update(hi=_nanlike((M, N), F16), lo=_nanlike((M, N), F16), bound=_nanlike((1,)))

    def run(bufs):
        call("mvk_dense16_first", ptr(zd), ptr(Wd), ptr(bd), ptr(zamd), ptr(o["hi"]), ptr(o["lo"]), ptr(o["bound"]), M, N, K, act,
             stream_ptr())

    def collect():
        return dict(h=R.decode(o["hi"].cpu(), o["lo"].cpu(), R.inv_of(o["bound"].cpu())))

    def exact():
        got = float(o["bound"])
        return [(f"published bound {got!r} >= max |h| {meta['hmax']!r}", got >= meta["hmax"]),
                (f"published bound {got!r} <= 1.001 x {r['bound_exact']!r}", got <= 1.001 * r["bound_exact"])]

    return _prep(run, [("h", rd)], reset=reset, collect=collect, exact=exact, raw=lambda: list(o.values()), meta=meta,
                 keep=[zd, Wd, bd, zamd])


# ---- the plane GEMM operands -----------------------------------------------------------------------------------------------------------
def _act_planes(gen, M, K, loose, relu=True, decades=1.0):
    """A GEMM's first operand [M][K] as planes under one tensor bound (loose: 3.7 x the maximum)."""
    a = R.spread_rows(M, K, gen, decades)
    a = a.clamp_min(0) if relu else a
    bound = float(a.abs().max()) * (R.LOOSE[0] if loose else 1.0)
    return R.tensor_planes(a, bound), bound


def _w_planes(gen, N, K, gain=0.3):
    """A weight operand [N][K]: rows over 10^+-2, one scale per row."""
    return R.row_planes(R.spread_rows(N, K, gen, 2.0) * (gain / math.sqrt(K)))


# ---- mvk_dense16_fwd_nll ---------------------------------------------------------------------------------------------------------------
def p_fwd(seed, M, N, K, xrows, bias=True, colsum=True, x_loose=False, h_loose=False, scale=0.75, sat=False, host=False, bm=None):
    bm = FWD_BM if bm is None else bm
    gen = R.g(seed)
    A, a_bound = _act_planes(gen, M, K, h_loose)
    B = _w_planes(gen, N, K)
    b = (torch.randn(N, generator=gen) * 0.5).float() if bias else None
    if sat:  # pre-activations pushed to +-12 in half of the columns
        b = torch.zeros(N) if b is None else b
        b[0::4] += 12.0
        b[1::4] -= 12.0
    X = (torch.rand(xrows, N, generator=gen) * 1.5 - 0.25).float()
    xam = float(X.abs().max()) * (R.LOOSE[1] if x_loose else 1.0)
    gw = 1.0 / M
    t = R.nll_tail(R.gemm_nt(A, B, a_bound), b, X, xrows, scale, gw, xam, bm=bm)
    P, CR = (N + 127) // 128, (M + bm - 1) // bm
    checks = [("G", t["G"]), ("rows", t["rows"])] + ([("colsum", t["colsum"])] if colsum else [])
    meta = dict(nt=R.nt_tiles(K), yard=t["yard"], g_bound=t["g_bound"], premax=float(t["pre"].abs().max()))
    if host:
        return _prep(None, checks, meta=meta)
    from multivae_amd import _lib
    from multivae_amd._lib import call, ptr, stream_ptr

    Ah, Al, Bh, Bl, binv, bd, Xd = _dev(A[0], A[1], B[0], B[1], B[2], b, X)
    ab, xamd = _scalar(a_bound), _scalar(xam)
    o = {}

    def reset():  # a NaN guard row behind G's planes, 64 NaN floats behind rows_part
        o.update(gh=_nanlike((M + 1, N), F16), gl=_nanlike((M + 1, N), F16), gb=_nanlike((1,)), rows=_nanlike((P * M + 64,)),
                 cs=_nanlike((CR, N)) if colsum else None)

    def run(bufs):
        call("mvk_dense16_fwd_nll", ptr(Ah), ptr(Al), ptr(ab), ptr(Bh), ptr(Bl), ptr(binv), ptr(bd), ptr(Xd), xrows, ptr(xamd), scale, gw,
             ptr(o["gh"]), ptr(o["gl"]), ptr(o["gb"]), ptr(o["rows"]), ptr(o["cs"]), M, N, K, stream_ptr())

    def collect():
        got = dict(G=R.decode(o["gh"][:M].cpu(), o["gl"][:M].cpu(), R.inv_of(o["gb"].cpu())), rows=o["rows"][:P * M].view(P, M).cpu().double())
        if colsum:
            got["colsum"] = o["cs"].cpu().double()
        return got

    def exact():
        gb, want = float(o["gb"]), t["g_bound"]
        return [("no row m >= M of G's planes or of rows_part is touched",
                 bool(torch.isnan(o["gh"][M]).all() and torch.isnan(o["gl"][M]).all() and torch.isnan(o["rows"][P * M:]).all())),
                (f"g_bound {gb!r} == gw (1 + x_amax) / (4 s^2) 1.0001 = {want!r} to 4 ulp",
                 abs(gb - want) <= 4 * float(R.ulp32(torch.tensor(want, dtype=F64)))),
                ("mvk_dense16_colsum_rows / _fwd_nll_rows", _lib.load().mvk_dense16_colsum_rows(M) == CR
                 and _lib.load().mvk_dense16_fwd_nll_rows(N) == P)]

    return _prep(run, checks, reset=reset, collect=collect, exact=exact, raw=lambda: [v for v in o.values() if v is not None], meta=meta,
                 keep=[Ah, Al, Bh, Bl, binv, bd, Xd, ab, xamd])


# ---- mvk_dense16_bwd_data --------------------------------------------------------------------------------------------------------------
MASK_BITS = (0x0000, 0x8000, 0x0001, 0x8001, 0x03FF, 0xBC00)  # +0, -0, smallest positive / negative subnormal, largest subnormal, -1


def _mask_plane(gen, M, N):
    """An fp16 hi plane of a hidden activation: normal values of both signs with the special bit patterns sprinkled in."""
    m = torch.randn(M, N, generator=gen).to(F16)
    bits = m.view(torch.int16).clone()
    pick = torch.randint(0, 3 * len(MASK_BITS), (M, N), generator=gen)
    for i, pat in enumerate(MASK_BITS):
        bits[pick == i] = pat - 0x10000 if pat >= 0x8000 else pat
    return bits.view(F16)


def p_bwd(seed, M, N, K, mask=True, db="ws", loose=False, host=False):
    """dA [M][N] = (G [M][K] planes) (W^T planes [N][K]) * ReLU'(mask); db [N] += column sums of dA ('off' | 'ws' | 'deferred')."""
    gen = R.g(seed)
    A, a_bound = _act_planes(gen, M, K, loose, relu=False)
    B = _w_planes(gen, N, K, gain=1.0)
    mk = _mask_plane(gen, M, N) if mask else None
    dbi = torch.randn(N, generator=gen).float()
    r, rdb = R.bwd_data(A, B, a_bound, mk, dbi)
    rdb["init"] = dbi
    checks = [("dA", r)] + ([("db", rdb)] if db != "off" else [])
    meta = dict(nt=R.nt_tiles(K), mask=mk)
    if host:
        return _prep(None, checks, meta=meta)
    from multivae_amd._lib import call, ptr, stream_ptr

    Ah, Al, Bh, Bl, binv, mkd = _dev(A[0], A[1], B[0], B[1], B[2], mk)
    ab = _scalar(a_bound)
    wsp, wsn = D.WS("ws")

    def run(bufs):
        call("mvk_dense16_bwd_data", ptr(Ah), ptr(Al), ptr(ab), ptr(Bh), ptr(Bl), ptr(binv), ptr(mkd), ptr(bufs[0]),
             ptr(bufs[1]) if db != "off" else None, wsp, wsn, M, N, K, stream_ptr())

    return _prep(run, checks, bufouts=[c[0] for c in checks], deferred=db == "deferred", meta=meta, keep=[Ah, Al, Bh, Bl, binv, mkd, ab])


# ---- mvk_dense16_wgrad -----------------------------------------------------------------------------------------------------------------
def p_wgrad(seed, M, N, K, finish="ws", cs=None, loose=False, host=False):
    """dW [N][K] += G^T H on planes G [M][N], H [M][K]; db [N] += the cs rows of colsum_part (cs None: db stays as it is)."""
    gen = R.g(seed)
    Dp, d_bound = _act_planes(gen, M, N, loose, relu=False)
    Hp, h_bound = _act_planes(gen, M, K, loose)
    dWi, dbi = torch.randn(N, K, generator=gen).float(), torch.randn(N, generator=gen).float()
    S, per, empty, mapping = R.wgrad_slices(M, N, K)
    r = R.gemm_tn(Dp, Hp, d_bound, h_bound, init=dWi, rows_per_slice=per * 32)
    r["init"] = dWi
    part = torch.randn(cs or 1, N, generator=gen).float()
    s64 = part.double().sum(0) if cs else torch.zeros(N, dtype=F64)
    rdb = dict(ref=s64, tol=R.C_ENTRY * (part.double().abs().sum(0) + dbi.double().abs()) if cs else torch.zeros(N, dtype=F64), deg=s64,
               ship=s64, cpu=(part.sum(0).double() if cs else s64), init=dbi)
    meta = dict(slices=(S, per, empty, mapping), chain=min(per * 32, M))
    checks = [("dW", r), ("db", rdb)]
    if host:
        return _prep(None, checks, meta=meta)
    from multivae_amd._lib import call, ptr, stream_ptr

    Dh, Dl, Hh, Hl, partd = _dev(Dp[0], Dp[1], Hp[0], Hp[1], part)
    db_, hb_ = _scalar(d_bound), _scalar(h_bound)
    wsp, wsn = D.WS("ws")

    def run(bufs):
        call("mvk_dense16_wgrad", ptr(Dh), ptr(Dl), ptr(db_), ptr(Hh), ptr(Hl), ptr(hb_), ptr(partd) if cs else None, cs or 0, ptr(bufs[0]),
             ptr(bufs[1]), wsp, wsn, M, N, K, stream_ptr())

    return _prep(run, checks, bufouts=["dW", "db"], deferred=finish == "deferred", meta=meta, keep=[Dh, Dl, Hh, Hl, partd, db_, hb_])


# ---- mvk_dense16_unsplit ---------------------------------------------------------------------------------------------------------------
def p_unsplit(seed, M, N, rowf=False, tile=0, host=False):
    gen = R.g(seed)
    x = R.spread_rows(M, N, gen, 2.0)
    bound = float(x.abs().max()) * R.LOOSE[0]
    hi, lo, _ = R.tensor_planes(x, bound)
    nt = (N + tile - 1) // tile if tile else 1
    rf = (torch.rand(nt, M, generator=gen) + 0.5).float() if rowf else None
    want = R.unsplit(hi, lo, bound, rf, 1.5, tile).double()
    rd = dict(ref=want, tol=torch.zeros_like(want), deg=R.unsplit(hi, torch.zeros_like(lo), bound, rf, 1.5, tile).double())
    if host:
        return _prep(None, [("out", rd)], meta=dict(x=x, bound=bound))
    from multivae_amd._lib import call, ptr, stream_ptr

    hid, lod, rfd = _dev(hi, lo, rf)
    bd = _scalar(bound)

    def run(bufs):
        call("mvk_dense16_unsplit", ptr(hid), ptr(lod), ptr(bd), ptr(rfd), 1.5, tile, M, N, ptr(bufs[0]), stream_ptr())

    return _prep(run, [("out", rd)], bufouts=["out"], keep=[hid, lod, rfd, bd])


# ---- the table -------------------------------------------------------------------------------------------------------------------------
def case(id_, fn, kw, expect, note=""):
    seed = zlib.crc32(id_.encode()) % 100003

    def make():
        p = fn(seed, **kw)
        if p.deferred:  # the arena grows between scopes to what the last one asked for: a first step sizes it
            p.reset()
            _, prime = D.execute(p)
            prime()
            torch.cuda.synchronize()
        return p

    c = D.Case(id_, make, tuple(sorted(expect)), None, note)
    c.host = lambda: fn(seed, host=True, **kw)
    c.fn, c.kw = fn, kw
    return c


def _opts(**kw):
    return "-".join(f"{k}{'' if v is True else ('0' if v is False else v)}" for k, v in kw.items())


CASES = [case(f"pack-n{N}-k{K}", p_pack, dict(N=N, K=K), [PACK]) for N, K in ((8, 16), (96, 48), (200, 256), (72, 64))]

# (M, N, K), bias, act, loose z_amax: K4 = 1, 1, 3, 5, 2, 1, 8, 5, 7; R = 8 up to M = 2048, 20 up to 5120, 40 above
FIRST = [((9, 8, 4), True, RELU, False), ((70, 16, 4), False, NONE, False), ((300, 64, 12), True, LEAKY, True),
         ((2048, 32, 20), False, RELU, False), ((2049, 16, 8), True, NONE, True), ((5121, 16, 4), False, LEAKY, False),
         ((5130, 1024, 32), True, RELU, False), ((131, 512, 20), False, LEAKY, True), ((40, 256, 28), True, NONE, False)]
for (_M, _N, _K), _b, _a, _l in FIRST:
    _k4, _r, _, _ = R.first_cfg(_M, _N, _K)
    CASES.append(case(f"first-m{_M}-n{_N}-k{_K}-K4_{_k4}-R{_r}-{_opts(bias=_b, act=_a, loose=_l)}", p_first,
                      dict(M=_M, N=_N, K=_K, bias=_b, act=_a, loose=_l), [f"d16_first_kernel<{_k4},{_r}>"], f"{_K} fmas per entry"))

# (M, N, K), xrows, options
FWD = [((1, 8, 8), 1, dict(bias=False, colsum=False, scale=1.0)),
       ((65, 8, 32), 65, dict(x_loose=True)),
       ((64, 128, 40), 7, dict(bias=False, scale=1.0, h_loose=True)),
       ((129, 136, 72), 200, dict(colsum=False, x_loose=True)),
       ((63, 264, 96), 9, dict(sat=True, scale=1.0)),
       ((200, 136, 200), 131, dict(bias=False, sat=True, h_loose=True)),
       ((70, 784, 512), 70, dict(x_loose=True, h_loose=True))]
for (_M, _N, _K), _x, _o in FWD:
    CASES.append(case(f"fwd_nll-m{_M}-n{_N}-k{_K}-x{_x}-nt{R.nt_tiles(_K)}{'-' if _o else ''}{_opts(**_o)}", p_fwd,
                      dict(M=_M, N=_N, K=_K, xrows=_x, **_o), [NT_FWD], f"{_K} products per accumulator"))

# (M, N, K), mask, db, loose
BWD = [((1, 8, 8), False, "off", False), ((65, 16, 8), True, "ws", True), ((129, 136, 72), True, "deferred", False),
       ((200, 64, 200), False, "ws", True), ((70, 512, 784), True, "deferred", True), ((129, 136, 72), True, "off", True)]
for (_M, _N, _K), _m, _d, _l in BWD:
    CASES.append(case(f"bwd_data-m{_M}-n{_N}-k{_K}-nt{R.nt_tiles(_K)}-{_opts(mask=_m, db=_d, loose=_l)}", p_bwd,
                      dict(M=_M, N=_N, K=_K, mask=_m, db=_d, loose=_l), [NT_BWD] + dict(off=[], ws=[SUM], deferred=[D.BATCH])[_d],
                      f"{_K} products per accumulator"))

# (M, N, K), finish, colsum rows, loose; the regime in the id comes from dense16_ref.wgrad_slices
WG = [((17, 8, 16), "ws", 1, False), ((150, 136, 136), "deferred", 5, True), ((300, 904, 904), "ws", None, False),
      ((300, 136, 72), "deferred", None, True), ((264, 784, 512), "ws", 5, True), ((520, 136, 72), "ws", 1, False),
      ((1024, 200, 256), "deferred", 5, True)]
for (_M, _N, _K), _f, _c, _l in WG:
    _S, _per, _empty, _map = R.wgrad_slices(_M, _N, _K)
    CASES.append(case(f"wgrad-m{_M}-n{_N}-k{_K}-S{_S}-per{_per}-empty{len(_empty)}-{_map}-{_opts(finish=_f, cs=_c or 0, loose=_l)}", p_wgrad,
                      dict(M=_M, N=_N, K=_K, finish=_f, cs=_c, loose=_l), [TN, D.BATCH if _f == "deferred" else SUM],
                      f"{min(_per * 32, _M)} products per accumulator, then {_S} slabs"))

CASES += [case(f"unsplit-{n}", p_unsplit, kw, [UNSPLIT]) for n, kw in (
    ("norowf", dict(M=70, N=136)), ("rowf-tile0", dict(M=70, N=136, rowf=True)), ("rowf-tile8", dict(M=33, N=72, rowf=True, tile=8)),
    ("rowf-tile128-n136", dict(M=70, N=136, rowf=True, tile=128)))]
IDS = [c.id for c in CASES]


# ---- running a case --------------------------------------------------------------------------------------------------------------------
def check(c, collect=False):
    """Run one case: the kernel set, every entry of every output, the degraded emulation, the exact properties, two runs bit for bit."""
    from multivae_amd import _lib

    fails, report = [], {}
    p = c.make()
    p.reset()
    bufs, run = D.execute(p)
    names = launched(run)
    report["kernels"] = names
    if names != sorted(c.expect):
        fails.append(f"launched {names}, expected {sorted(c.expect)}")
    if p.deferred and int(_lib.load().mvk_defer_pending()) != 0:
        fails.append("deferred reductions are still pending behind the scope")
    got = p.collect()
    for label, b in zip(p.bufouts, bufs):
        t = b.detach().cpu().double()
        init = dict(p.checks)[label].get("init")
        got[label] = t if init is None else t - init.double()
    rejected = []
    for label, rd in p.checks:
        t = got[label]
        assert t.shape == rd["ref"].shape, (c.id, label, t.shape, rd["ref"].shape)
        if not bool(torch.isfinite(t).all()):
            fails.append(f"{label} has entries that are NaN / inf (or were never written)")
            continue
        tol = rd["tol"] + 1e-30
        err = (t - rd["ref"]).abs()
        worst, dworst = float((err / tol).max()), float(((rd["deg"] - rd["ref"]).abs() / tol).max())
        report[label] = dict(worst=worst, degraded=dworst)
        rejected.append(dworst > 1.0)
        if worst > 1.0:
            fails.append(f"{label}: {int((err > tol).sum())} of {err.numel()} entries outside the tolerance; worst {worst:.2f}x")
    for what, ok in p.exact():
        if not ok:
            fails.append(what)
    if p.checks and not any(rejected):
        fails.append(f"no teeth: the degraded emulation passes every check ({report})")
    first = [t.clone() for t in list(bufs) + p.raw()]
    p.reset()
    bufs2, run2 = D.execute(p)
    run2()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(first, list(bufs2) + p.raw())):
        if not _biteq(a, b):
            fails.append(f"buffer {i} differs between two runs of the same launch")
    if collect:
        return report, fails
    assert not fails, f"{c.id}: " + "; ".join(fails)
    return report


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_dense16_leaf(c):
    report = check(c)
    print(c.id, {k: v for k, v in report.items() if k != "kernels"})


def test_case_ids_are_unique():
    assert len(IDS) == len(set(IDS))


# ---- one chain on device-produced planes -----------------------------------------------------------------------------------------------
def test_chain_on_device_planes():
    """pack -> first -> fwd_nll -> bwd_data -> wgrad at (M, L, H, D, B) = (136, 8, 64, 72, 17): every stage reads the planes the stage
    before it wrote, and is compared with float64 of exactly those planes (decoded on the host), at the leaf tolerances."""
    from multivae_amd import _lib
    from multivae_amd._lib import call, ptr, stream_ptr

    M, L, H, Dd, B = 136, 8, 64, 72, 17
    gen = R.g(136)
    z, W0, b0 = R.first_operands(1368, M, H, L)
    W1 = R.spread_rows(Dd, H, gen, 1.0) * (0.3 / math.sqrt(H))
    b1 = (torch.randn(Dd, generator=gen) * 0.5).float()
    X = (torch.rand(B, Dd, generator=gen) * 1.5 - 0.25).float()
    scale, gw = 0.75, 1.0 / M
    zam, xam = float(z.abs().max()), float(X.abs().max())
    dW1i, db1i, db0i = torch.randn(Dd, H, generator=gen).float(), torch.randn(Dd, generator=gen).float(), torch.randn(H, generator=gen).float()
    d = D.dev()
    zd, W0d, b0d, W1d, b1d, Xd = _dev(z, W0, b0, W1, b1, X)
    pk = dict(nk_hi=_nanlike((Dd, H), F16), nk_lo=_nanlike((Dd, H), F16), nk_inv=_nanlike((Dd,)), kn_hi=_nanlike((H, Dd), F16),
              kn_lo=_nanlike((H, Dd), F16), kn_inv=_nanlike((H,)))
    hh, hl, hb = _nanlike((M, H), F16), _nanlike((M, H), F16), _nanlike((1,))
    gh, gl, gb = _nanlike((M, Dd), F16), _nanlike((M, Dd), F16), _nanlike((1,))
    lib = _lib.load()
    P, CR = lib.mvk_dense16_fwd_nll_rows(Dd), lib.mvk_dense16_colsum_rows(M)
    rows, cs = _nanlike((P, M)), _nanlike((CR, Dd))
    dh, db0, dW1, db1 = _nanlike((M, H)), db0i.to(d), dW1i.to(d), db1i.to(d)
    wsp, wsn = D.WS("ws")
    zamd, xamd = _scalar(zam), _scalar(xam)

    def run():
        call("mvk_dense16_pack", ptr(W1d), Dd, H, ptr(pk["nk_hi"]), ptr(pk["nk_lo"]), ptr(pk["nk_inv"]), ptr(pk["kn_hi"]), ptr(pk["kn_lo"]),
             ptr(pk["kn_inv"]), stream_ptr())
        call("mvk_dense16_first", ptr(zd), ptr(W0d), ptr(b0d), ptr(zamd), ptr(hh), ptr(hl), ptr(hb), M, H, L, RELU, stream_ptr())
        call("mvk_dense16_fwd_nll", ptr(hh), ptr(hl), ptr(hb), ptr(pk["nk_hi"]), ptr(pk["nk_lo"]), ptr(pk["nk_inv"]), ptr(b1d), ptr(Xd), B,
             ptr(xamd), scale, gw, ptr(gh), ptr(gl), ptr(gb), ptr(rows), ptr(cs), M, Dd, H, stream_ptr())
        call("mvk_dense16_bwd_data", ptr(gh), ptr(gl), ptr(gb), ptr(pk["kn_hi"]), ptr(pk["kn_lo"]), ptr(pk["kn_inv"]), ptr(hh), ptr(dh),
             ptr(db0), wsp, wsn, M, H, Dd, stream_ptr())
        call("mvk_dense16_wgrad", ptr(gh), ptr(gl), ptr(gb), ptr(hh), ptr(hl), ptr(hb), ptr(cs), CR, ptr(dW1), ptr(db1), wsp, wsn, M, Dd, H,
             stream_ptr())

    names = launched(run)
    assert names == sorted([PACK, "d16_first_kernel<2,8>", NT_FWD, NT_BWD, SUM, TN]), names
    worst = {}

    def hold(label, got, rd):
        assert bool(torch.isfinite(got).all()), label
        worst[label] = (R.ratio(got, rd["ref"], rd["tol"] + 1e-30), R.ratio(rd["deg"], rd["ref"], rd["tol"] + 1e-30))

    want = R.pack(W1)
    for k in pk:
        assert _biteq(pk[k].cpu(), want[k]), k
    r1 = R.first(z, W0, b0, RELU, zam)
    hbv = float(hb)
    assert float(r1["ref"].max()) <= hbv <= 1.001 * r1["bound_exact"]
    Hp = (hh.cpu(), hl.cpu(), float(R.inv_of(hb.cpu())))
    hold("h", R.decode(*Hp), dict(ref=r1["ref"], tol=R.first_tol(r1, r1["bound_exact"]), deg=R.decode(Hp[0], torch.zeros_like(Hp[1]), Hp[2])))
    # fwd_nll on the planes of h and of W1 the device wrote
    gbv = float(gb)
    t = R.nll_tail(R.gemm_nt(Hp, (pk["nk_hi"].cpu(), pk["nk_lo"].cpu(), pk["nk_inv"].cpu()), hbv), b1, X, B, scale, gw, xam, bm=FWD_BM)
    assert abs(gbv - t["g_bound"]) <= 4 * float(R.ulp32(torch.tensor(t["g_bound"], dtype=F64)))
    Gp = (gh.cpu(), gl.cpu(), float(R.inv_of(gb.cpu())))
    hold("G", R.decode(*Gp), t["G"])
    hold("rows", rows.cpu().double(), t["rows"])
    hold("colsum", cs.cpu().double(), t["colsum"])
    # bwd_data on the planes of G and of W1^T, the ReLU mask from h's hi plane
    r3, rdb = R.bwd_data(Gp, (pk["kn_hi"].cpu(), pk["kn_lo"].cpu(), pk["kn_inv"].cpu()), gbv, Hp[0], db0i)
    hold("dh", dh.cpu().double(), r3)
    hold("db0", db0.cpu().double() - db0i.double(), rdb)
    # wgrad on the planes of G and h; db1 from the forward's partial column sums as the device wrote them
    r4 = R.gemm_tn(Gp, Hp, gbv, hbv, init=dW1i)
    hold("dW1", dW1.cpu().double() - dW1i.double(), r4)
    csd = cs.cpu().double()
    hold("db1", db1.cpu().double() - db1i.double(), dict(ref=csd.sum(0), tol=R.C_ENTRY * (csd.abs().sum(0) + db1i.double().abs()), deg=csd.sum(0)))
    print("chain", {k: (round(a, 3), round(b, 1)) for k, (a, b) in worst.items()})
    bad = {k: v for k, v in worst.items() if v[0] > 1.0}
    assert not bad, bad
    for k in ("h", "G", "dh", "dW1"):
        assert worst[k][1] > 1.0, f"no teeth at {k}: {worst[k]}"


# ---- the refusals ----------------------------------------------------------------------------------------------------------------------
def _refusal(name):
    """(entry, args, outputs that must stay as filled, keep) of one refused call: real, adequately sized buffers throughout."""
    from multivae_amd._lib import ptr, stream_ptr

    d = D.dev()
    M, N, K = 64, 24, 40  # buffers are sized for the largest of the shapes below
    f = lambda *s: torch.randn(*s, device=d)                    # noqa: E731
    h = lambda *s: torch.randn(*s, device=d).to(F16)            # noqa: E731
    one = torch.ones(1, device=d)
    outs, keep = [], [one]

    def out(*s, dtype=F32):
        t = _nanlike(s, dtype)
        outs.append(t)
        return t

    def inp(t):
        keep.append(t)
        return ptr(t)

    wsp, wsn = D.WS("ws")
    sp = stream_ptr()
    if name == "pack-k24":
        N, K = 16, 24
        return "mvk_dense16_pack", (inp(f(N, K)), N, K, ptr(out(N, K, dtype=F16)), ptr(out(N, K, dtype=F16)), ptr(out(N)),
                                    ptr(out(K, N, dtype=F16)), ptr(out(K, N, dtype=F16)), ptr(out(K)), sp), outs, keep
    if name.startswith("first-"):
        N, K = dict(k36=(16, 36), k6=(16, 6), n24=(24, 8))[name.split("-")[1]]
        return "mvk_dense16_first", (inp(f(M, K)), inp(f(N, K)), inp(f(N)), ptr(one), ptr(out(M, N, dtype=F16)), ptr(out(M, N, dtype=F16)),
                                     ptr(out(1)), M, N, K, RELU, sp), outs, keep
    if name.startswith("fwd_nll-"):
        what = name.split("-", 1)[1]
        N, K = (12, 16) if what == "n12" else (16, 16)
        scale = dict(scale0=0.0, scalenan=NAN).get(what, 0.75)
        xrows = 0 if what == "xrows0" else M
        X = f(M * N + 4)
        keep.append(X)
        xp = ptr(X[1:]) if what == "xoff1" else ptr(X)
        return "mvk_dense16_fwd_nll", (inp(h(M, K)), inp(h(M, K)), ptr(one), inp(h(N, K)), inp(h(N, K)), inp(f(N)), inp(f(N)), xp, xrows,
                                       ptr(one), scale, 1.0, ptr(out(M, N, dtype=F16)), ptr(out(M, N, dtype=F16)), ptr(out(1)),
                                       ptr(out(1, M)), ptr(out(1, N)), M, N, K, sp), outs, keep
    N, K = 16, 16
    if name == "bwd_data-ws-short":  # one row tile: the partials need 1 * N floats
        return "mvk_dense16_bwd_data", (inp(h(M, K)), inp(h(M, K)), ptr(one), inp(h(N, K)), inp(h(N, K)), inp(f(N)), None, ptr(out(M, N)),
                                        ptr(out(N)), wsp, N - 1, M, N, K, sp), outs, keep
    if name == "wgrad-ws-short":
        S = R.wgrad_slices(M, N, K)[0]
        return "mvk_dense16_wgrad", (inp(h(M, N)), inp(h(M, N)), ptr(one), inp(h(M, K)), inp(h(M, K)), ptr(one), None, 0, ptr(out(N, K)),
                                     ptr(out(N)), wsp, S * N * K - 1, M, N, K, sp), outs, keep
    if name == "wgrad-colsum-without-db":
        return "mvk_dense16_wgrad", (inp(h(M, N)), inp(h(M, N)), ptr(one), inp(h(M, K)), inp(h(M, K)), ptr(one), inp(f(1, N)), 1,
                                     ptr(out(N, K)), None, wsp, wsn, M, N, K, sp), outs, keep
    if name == "unsplit-tile6":
        return "mvk_dense16_unsplit", (inp(h(M, 24)), inp(h(M, 24)), ptr(one), inp(f(4, M)), 1.0, 6, M, 24, ptr(out(M, 24)), sp), outs, keep
    raise KeyError(name)


REFUSED = ["pack-k24", "first-k36", "first-k6", "first-n24", "fwd_nll-scale0", "fwd_nll-scalenan", "fwd_nll-xrows0", "fwd_nll-xoff1",
           "fwd_nll-n12", "bwd_data-ws-short", "wgrad-ws-short", "wgrad-colsum-without-db", "unsplit-tile6"]


@pytest.mark.parametrize("name", REFUSED)
def test_entries_refuse(name):
    """MVK_EINVAL (-1), no launch, and every NaN-filled output stays all NaN."""
    from multivae_amd import _lib

    lib = _lib.load()
    entry, args, outs, keep = _refusal(name)
    rc = []
    names = D.launched_kernels(lambda: rc.append(getattr(lib, entry)(*args)))
    assert rc == [-1] and names == [], (rc, names)
    for t in outs:
        assert bool(torch.isnan(t).all())


# ---- the 128-row forward tile ----------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(FWD_BM == 128, reason="this is the parent of the MVK_D16_FWD_BM=128 run")
def test_fwd_bm128_child():
    """MVK_D16_FWD_BM (under MVK_TUNE=1) is read once per process: the fwd_nll cases again in a fresh child process (not an exec of
    this one), where each expects d16_nt_kernel<128, 0> and mvk_dense16_colsum_rows gives ceil(M / 128)."""
    env = dict(os.environ, MVK_TUNE="1", MVK_D16_FWD_BM="128")
    r = subprocess.run([sys.executable, "-s", "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider", "-m", "gpu",
                        os.path.abspath(__file__) + "::test_dense16_leaf", "-k", "fwd_nll"],
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, f"MVK_D16_FWD_BM=128 child failed ({r.returncode}):\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert f"{len(FWD)} passed" in r.stdout, r.stdout[-2000:]
