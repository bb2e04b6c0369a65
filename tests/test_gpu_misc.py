"""The helper kernels of csrc/misc.hip called directly through the C ABI, entry by entry against tests/misc_ref.py: the weight packs
(mvk_pack_weights, mvk_pack_conv4s2_weight, mvk_pack_unflatten_weight), flat Adam in its seven entries, mvk_act_bwd,
mvk_act_bwd_scaled, mvk_axpby, the pre-split bf16 format (mvk_f32_to_bf3 / mvk_bf3_to_f32), the two layout changes, average pooling
and upsampling with their backward passes, and mvk_device_rng.

References, exact index / bit models, case tables (every case says which edge it is there for) and the error model live in
tests/misc_ref.py.  tests/test_misc_ref_host.py pins them to independent definitions on the CPU and runs every `check_*` routine
below with a stand-in backend (the plain fp32 CPU evaluation), so the tables and the bounds are proven before GPU time is spent.

Every output is allocated with a NaN (0xFFFF for 16-bit buffers) prefill and 64 sentinel floats on both sides; every output is
compared on EVERY entry; a NaN left anywhere or a touched sentinel fails; a second launch from the same inputs is bit-identical;
where a case exists to reach one leaf, the launched kernel's name is asserted (torch.profiler, test_gpu_gemm_dispatch.launched_kernels).
Permutations (packs, layouts, upsample forward), the bf16 split, the uniform draws at (0, 1) and the ReLU / LeakyReLU / NONE
forms are BIT-EXACT against their models; everything else is held per entry to C_STAGE[stage] * base (misc_ref's docstring).

Constants and what the HIP kernels showed on an MI355X (test_zz_report; `derived` = from the number of roundings):
    stage                   fp32 CPU   C        set by                         HIP     set by
    act_bwd.sigmoid         1.92       4 derived   act_bwd-n524291-act2           1.92    act_bwd-n524291-act2-off_dY
    act_bwd_scaled.sigmoid  2.11       5 derived   act_bwd_scaled-n1023-act2      2.11    act_bwd_scaled-n1023-act2
    axpby                   1.89       3 derived   axpby-n1028-xy                 1.89    axpby-n1028-xy
    pool.fwd                1.97      10 derived   pool.fwd-2x5x9x3               1.72    pool.fwd-2x7x7x20
    pool.bwd                1.71      10 derived   pool.bwd-2x7x7x20              1.89    pool.bwd-2x7x7x20
    up.bwd                  2.12       3 derived   up.bwd-3x3x7x6                 1.50    up.bwd-2x7x7x20
    rng.uniform (-2, 3.3)   1.17       3 derived   s1-o5-n65536                   0.83    s1-o5-n65536
    adam.m                  0.95       4           step-n524293-s1000-wd          0.96    step-n524293-s1000-wd
    adam.v                  3.88      16           step-n524293-s1000-wd          4.05    step-n524293-s1000-wd
    adam.vmax               3.02      13           fused-n1028-s1-wd-ams-zero     3.02    fused-n1028-s1-wd-ams-zero
    adam.p                  2.19       9           fused-n1028-s2-tiny            2.22    step-n524293-s1000-wd
    rng.normal              2.07       9           s1-o5-n65536                   2.48    s1-o5-n65536
i.e. at most 0.63 of C (axpby); the derived bounds are not tuned to these figures.  (adam.v: the fp32 casts of beta2 and 1 - beta2
alone are two roundings against the double scalars of the reference, and g' carries two more into its square.)
Wall time of this file on an MI355X: 2.6 s for the 82 tests (5.1 s with start-up and collection; the first profiler session
is 1.7 s of that); on the CPU with the stand-in backend (tests/test_misc_ref_host.py, 129 tests): 5 s.

Suspects read from the kernel text, each with the case that exercises it, and the verdict of the first run on an MI355X:
 1. pack_multi_kernel, tiled against element-per-thread: "the same values in the same places", bf16 fragments included; the
    element-per-thread branch with fragments runs only for an unaligned Wref (k0-cv64-cu32-frag-off, k0-cv128-cu64-frag-off:
    packs bit for bit, fragment buffers byte for byte equal to the tiled launch of the same weights, every byte written).
 2. pack_amax covers 8 x 32 x 256 = 65536 elements per round with 32 workgroups while the grid may be smaller or the weight larger,
    and the tiled branch publishes per workgroup of its tile loop (test_pack_amax_positions: the maximum at 0, last, 8191 / 8192,
    65535 / 65536 for all kinds and both branches; k2-cv128-cu128; presets above and below).
 3. 512 tiles on a grid capped at 256 workgroups, and 131072 elements on 256 x 256 threads (k0-cv256-cu128, k0-cv128-cu64-frag-off).
 4. ld_down / col_off: only the pack's columns are written (k0-cv8-cu16-ld2-co8 tiled, -co2 element-per-thread: the NaN prefill of
    the other columns stays), also through mvk_pack_conv4s2_weight.
 5. a launch sized by its largest descriptor hands idle workgroups to the small ones, whose amax / tile guards must hold
    (test_pack_one_launch_of_sixteen: the whole case table in one launch, every descriptor with the bits of its launch alone).
 6. adam_kernel's grid-stride loop past 2048 x 256 elements, and the one-lane second block of adam4_kernel (step-n524293-s1000-wd,
    *-n1028-*); each of p, g, m, v, vmax misaligned alone must select the scalar kernel (fused-n1028-s2-off_*: by name).
 7. adam4_dev_kernel and adam4_kernel instantiate adam_one separately: a different contraction would show as different bits
    (dev-*: bit-identical to mvk_adam_step_fused on every stage; the assertion stands unrelaxed).
 8. the identity scalars must also survive g = +-1e30, g subnormal and m = v = 0 (test_adam_identity); vmax is still raised to v where
    v > vmax, so "vmax keeps its bits" holds on the invariant vmax >= v that every amsgrad step leaves, which the test respects.
 9. adam_prepare_kernel's pow on the device against the host's (test_adam_prepare: within one ulp at steps 1, 2, 1000, 100000).
10. act_bwd_scaled_kernel's vector body and scalar tail in one kernel, chosen per lane (n = 1 .. 9, 1023 .. 1028, each pointer off:
    aligned and unaligned runs bit-identical); act_bwd_kernel's stride past the grid cap (act_bwd-n524291-*-off_dY).
11. f32_to_bf3_kernel's store guard at odd n: the last pair must not spill into the next plane (test_bf3[1], [3], [511], [513]: all
    three planes against the host split, sentinel behind plane 2).
12. device_rng_kernel: round constants and key schedule (test_rng_known_answer), the carry of offset + thread into the second
    counter word (hi-carry-n1024), a high key word, the (0, 1] map of u1 (s1-o5-n65536: u1 down to 2^-15), cosine before sine, the
    ticket: state[1] advances by gridDim x 256 and the ticket returns to 0 with two and with 64 workgroups.
13. the V = 1 leaf of pooling / upsampling at C % 4 == 0 (2x7x7x20 four bytes off: by name, bit-identical to the V = 4 leaf); maps
    with a dimension of 1 or 2, where every window is clipped (1x1x1x1, 2x1x5x4, 2x2x2x8).
Verdict: all thirteen cleared; csrc/misc.hip is unchanged.  Every stage is inside its bound on every case, no sentinel was touched,
no NaN was left, and both bit-identities that a contraction could have broken (7, 13) hold as bit-identities.

Entries of misc.hip that are tested entry-wise elsewhere and are not repeated here: mvk_reduce_terms(_ws), mvk_copy_batch,
mvk_transpose_act, mvk_amax, mvk_conv4s2_up_nchw_small (tests/test_gpu_kernels.py); mvk_loss_backward_seed and
mvk_scale_by_device_scalar (tests/test_gpu_recon_nll.py); their leaves are reached there (the several-workgroup form of
mvk_reduce_terms_ws and its one-workgroup fall-back, more than 16 terms, a transpose batch beyond gridDim.z = 65535).  The probes (mvk_probe_*) and the timestamp profiler (mvk_prof_*) are
measuring tools and stay out.  Leaves not covered: none of the entries above has a leaf that needs more than 2048 * 256 + 5 floats;
act_bwd4_kernel / adam4*_kernel / axpby4_kernel have no grid cap (one quad per lane), so they have no second sweep to reach.
"""
import time

import numpy as np
import pytest
import torch

import misc_ref as R
import test_gpu_gemm_dispatch as D

pytestmark = pytest.mark.gpu

GUARD = 64  # floats
EINVAL = -1  # MVK_EINVAL
SENTINEL = 12345.0
SENTINEL16 = 0x1234
MEASURED = {}
_T0 = time.time()
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def _lib():
    from multivae_amd import _lib as L

    return L


same_bits = R.same_bits


def note(measured, stage, ratio, name):
    if measured is not None and ratio > measured.get(stage, (-1.0, ""))[0]:
        measured[stage] = (ratio, name)


def hold(measured, stage, ratio, name):
    """Print, record and assert one stage's worst |err| / base."""
    print(f"{name}: {stage} {ratio:.3f}")
    note(measured, stage, ratio, name)
    assert ratio <= R.C_STAGE[stage], f"{name}: {stage} worst |err| / base = {ratio:.3g} > C = {R.C_STAGE[stage]}"


def no_nan(t, what):
    assert not bool(torch.isnan(t).any()), f"{what}: a NaN is left: an entry the kernel did not write"


# ---- guarded device buffers ---------------------------------------------------------------------------------------------------------------
class Guarded:
    """n elements (fp32, or int16 for the bf16 planes and fragments) with 64 floats' worth of sentinels before and after; `off`: the
    body starts 4 bytes past a 16-byte boundary.  Prefill: NaN (int16: 0xFFFF), or `src`."""

    def __init__(self, n, off=False, fill=NAN, src=None, dtype=torch.float32):
        per = 2 if dtype == torch.int16 else 1  # elements per 4 bytes
        self.n, self.g = n, GUARD * per
        self.lo = self.g + (per if off else 0)
        self.sent = SENTINEL16 if dtype == torch.int16 else SENTINEL
        self.buf = torch.full((self.lo + n + self.g,), self.sent, dtype=dtype, device=dev())
        self.body = self.buf[self.lo:self.lo + n]
        if src is not None:
            self.body.copy_(src.reshape(-1))
        else:
            self.body.fill_(-1 if dtype == torch.int16 else fill)
        assert self.body.data_ptr() % 16 == (4 if off else 0)

    @property
    def p(self):
        return self.body.data_ptr()

    def intact(self):
        b = self.buf.cpu()
        return bool((b[:self.lo] == self.sent).all()) and bool((b[self.lo + self.n:] == self.sent).all())

    def cpu(self, *shape):
        return self.body.cpu().reshape(*shape).clone()

    def untouched(self):
        b = self.body.cpu()
        return self.intact() and bool((b == -1).all() if b.dtype == torch.int16 else torch.isnan(b).all())


def _pack_shapes(kind, Cv, Cu, ld):
    T = R.pack_taps(kind)
    return dict(Wdown=(T * Cu, ld), Wup={0: (4, 4 * Cv, Cu), 1: (Cv, 16 * Cu), 2: (9 * Cv, Cu)}.get(kind, (-1,)))


# ---- the HIP backend: one method per C-ABI family, CPU tensors in, CPU tensors out ----------------------------------------------------------
class Hip:
    def _run(self, fn, names):
        if names:
            return [n.split("<")[0] if names == "base" else n for n in D.launched_kernels(fn)]
        fn()
        torch.cuda.synchronize()
        return None

    # descs: dicts with kind, W [Cv][Cu][taps], want (names of the outputs to pass; the others are NULL), off, ld, col_off, preset
    def pack(self, descs, via="multi", n_arg=None, may_fail=False):
        Lb = _lib()
        lib, sp = Lb.load(), Lb.stream_ptr
        arr = (Lb.PackDesc * max(len(descs), 1))()
        held = []
        for e, d in zip(arr, descs):
            W, kind, want = d["W"], d["kind"], d["want"]
            Cv, Cu, T = W.shape
            ld = d.get("ld") or Cv
            fb = int(lib.mvk_imgconv_frag_bytes(Cu, Cv)) // 2 or 16 * Cu * Cv * 3  # (uncovered pair: only for the argument checks)
            b = dict(W=Guarded(W.numel(), off=d.get("off", False), src=W))
            if "Wdown" in want:
                b["Wdown"] = Guarded(T * Cu * ld)
            if "Wup" in want:
                b["Wup"] = Guarded(W.numel())
            for k in ("Fdown", "Fup"):
                if k in want:
                    b[k] = Guarded(fb, dtype=torch.int16)
            if "amax" in want:
                b["amax"] = Guarded(1, fill=d.get("preset", 0.0))
            e.Wref, e.Cv, e.Cu, e.kind = b["W"].p, d.get("Cv", Cv), d.get("Cu", Cu), kind
            e.ld_down, e.col_off = d.get("ld") or 0, d.get("col_off", 0)
            for k in ("Wdown", "Wup", "Fdown", "Fup", "amax"):
                setattr(e, k, b[k].p if k in b else None)
            held.append(b)
        if via == "multi":
            self.rc = lib.mvk_pack_weights(arr, len(descs) if n_arg is None else n_arg, sp())
        else:
            assert len(descs) == 1
            e = arr[0]
            if descs[0]["kind"] == 0:
                self.rc = lib.mvk_pack_conv4s2_weight(e.Wref, e.Cv, e.Cu, e.Wdown, e.ld_down, e.col_off, e.Wup, sp())
            else:
                self.rc = lib.mvk_pack_unflatten_weight(e.Wref, e.Cv, e.Cu, e.Wup, sp())
        assert may_fail or self.rc == 0, f"pack call failed with code {self.rc}"
        torch.cuda.synchronize()
        outs = []
        for d, b in zip(descs, held):
            Cv, Cu, _ = d["W"].shape
            shp = _pack_shapes(d["kind"], Cv, Cu, d.get("ld") or Cv)
            o = dict(guards=all(g.intact() for g in b.values()), untouched=all(g.untouched() for k, g in b.items() if k not in ("W", "amax")))
            for k in ("Wdown", "Wup"):
                o[k] = b[k].cpu(*shp[k]) if k in b else None
            for k in ("Fdown", "Fup"):
                o[k] = b[k].cpu(-1) if k in b else None
            o["amax"] = b["amax"].cpu(1) if "amax" in b else None
            outs.append(o)
        return outs

    def adam(self, case, inp, names="base"):
        Lb = _lib()
        call, sp, n = Lb.call, Lb.stream_ptr, case.n
        B = {k: Guarded(n, off=case.off == k, src=inp[k]) for k in "pgmv"}
        if case.ams:
            B["vmax"] = Guarded(n, off=case.off == "vmax", src=inp["vmax"])
        pub = Guarded(8) if case.entry in ("pub", "dev") else None
        P = [B[k].p for k in "pgmv"]
        vm = B["vmax"].p if case.ams else None
        hyper = (case.lr, 0.9, 0.999, 1e-8, case.wd, case.step, case.gscale)

        def go():
            if case.entry == "step":
                call("mvk_adam_step", *P, n, *hyper, sp())
            elif case.entry == "amsgrad":
                call("mvk_adam_step_amsgrad", *P, vm, n, *hyper, sp())
            elif case.entry == "fused":
                call("mvk_adam_step_fused", *P, vm, n, *hyper, int(case.zero), sp())
            elif case.entry == "pub":
                call("mvk_adam_step_pub", *P, vm, n, *hyper, int(case.zero), pub.p, sp())
            else:  # the scalars from a publish-only call (n = 0), then the update that reads them from device memory
                call("mvk_adam_step_pub", *P, vm, 0, *hyper, int(case.zero), pub.p, sp())
                call("mvk_adam_step_dev", *P, vm, n, pub.p, int(case.zero), sp())

        kernels = self._run(go, names)
        out = {k: g.cpu(n) for k, g in B.items()}
        out.update(guards=all(g.intact() for g in B.values()) and (pub is None or pub.intact()), kernels=kernels,
                   pub=None if pub is None else pub.cpu(8))
        return out

    def _ew(self, ins, n_out, launch, names, off_out=False):
        """ins: name -> (tensor or None, off); launch(ptrs, out_ptr)."""
        G = {k: (None if t is None else Guarded(t.numel(), off=o, src=t)) for k, (t, o) in ins.items()}
        out = Guarded(n_out, off=off_out)
        ptrs = {k: (None if g is None else g.p) for k, g in G.items()}
        kernels = self._run(lambda: launch(ptrs, out.p), names)
        return dict(out=out.cpu(n_out), guards=out.intact() and all(g.intact() for g in G.values() if g is not None), kernels=kernels,
                    ins={k: (None if g is None else g.cpu(g.n)) for k, g in G.items()})

    def act_bwd(self, dY, Y, act, off=None, names=None):
        Lb = _lib()
        G = dict(dY=Guarded(dY.numel(), off=off == "dY", src=dY), Y=Guarded(Y.numel(), off=off == "Y", src=Y))
        kernels = self._run(lambda: Lb.call("mvk_act_bwd", G["dY"].p, G["Y"].p, dY.numel(), act, Lb.stream_ptr()), names)
        return dict(out=G["dY"].cpu(dY.numel()), guards=G["dY"].intact() and G["Y"].intact(), kernels=kernels,
                    Y_kept=same_bits(G["Y"].cpu(Y.numel()), Y))

    def act_bwd_scaled(self, g, a, Y, act, off=None, names=None):
        Lb, n = _lib(), g.numel()
        return self._ew(dict(g=(g, off == "g"), Y=(Y, off == "Y")), n,
                        lambda p, o: Lb.call("mvk_act_bwd_scaled", p["g"], a, p["Y"], act, o, n, Lb.stream_ptr()), names, off_out=off == "out")

    def axpby(self, x, a, y, b, act, n, off=None, names=None):
        Lb = _lib()
        return self._ew(dict(x=(x, off == "x"), y=(y, off == "y")), n,
                        lambda p, o: Lb.call("mvk_axpby", p["x"], a, p["y"], b, n, act, o, Lb.stream_ptr()), names, off_out=off == "out")

    def f32_to_bf3(self, x, off=False):
        Lb, n = _lib(), x.numel()
        src, pl = Guarded(n, off=off, src=x), Guarded(3 * n, dtype=torch.int16)
        Lb.call("mvk_f32_to_bf3", src.p, n, pl.p, Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(out=pl.cpu(3, n), guards=pl.intact() and src.intact())

    def bf3_to_f32(self, planes, off=False):
        Lb, n = _lib(), planes.shape[1]
        pl, out = Guarded(3 * n, src=planes, dtype=torch.int16), Guarded(n, off=off)
        Lb.call("mvk_bf3_to_f32", pl.p, n, out.p, Lb.stream_ptr())
        torch.cuda.synchronize()
        return dict(out=out.cpu(n), guards=pl.intact() and out.intact())

    def layout(self, x, to_nhwc):
        Lb = _lib()
        n, c, h, w = x.shape if to_nhwc else (x.shape[0], x.shape[3], x.shape[1], x.shape[2])
        fn = "mvk_nchw_to_nhwc" if to_nhwc else "mvk_nhwc_to_nchw"
        r = self._ew(dict(x=(x, False)), x.numel(), lambda p, o: Lb.call(fn, p["x"], o, n, c, h, w, Lb.stream_ptr()), None)
        r["out"] = r["out"].reshape(*((n, h, w, c) if to_nhwc else (n, c, h, w)))
        return r

    def pool(self, op, x, shape, off=False, names=None):
        Lb = _lib()
        n, H, W, C = shape
        OH, OW = (H + 1) // 2, (W + 1) // 2
        fn, oshape = {"pool.fwd": ("mvk_avgpool3s2_fwd", (n, OH, OW, C)), "pool.bwd": ("mvk_avgpool3s2_bwd", (n, H, W, C)),
                      "up.fwd": ("mvk_upsample2_fwd", (n, 2 * H, 2 * W, C)), "up.bwd": ("mvk_upsample2_bwd", (n, H, W, C))}[op]
        nout = oshape[0] * oshape[1] * oshape[2] * oshape[3]
        r = self._ew(dict(x=(x, off)), nout, lambda p, o: Lb.call(fn, p["x"], o, n, H, W, C, Lb.stream_ptr()), names, off_out=off)
        r["out"] = r["out"].reshape(*oshape)
        return r

    def rng(self, state, n, uniform, lo=0.0, hi=1.0, off=False):
        """state: (seed, offset, ticket) as Python ints -> out, the state after the launch."""
        Lb = _lib()
        st = torch.from_numpy(np.array(state, dtype=np.uint64).view(np.int64).copy()).to(dev())
        out = Guarded(n, off=off)
        Lb.call("mvk_device_rng", out.p, n, st.data_ptr(), int(uniform), lo, hi, Lb.stream_ptr())
        torch.cuda.synchronize()
        after = [int(v) for v in st.cpu().numpy().view(np.uint64)]
        return dict(out=out.cpu(n), guards=out.intact(), state=after)


HIP = Hip()


# ---- the comparison routines (also run on the CPU by tests/test_misc_ref_host.py with a stand-in backend) --------------------------------
def frag_triples(buf):
    """int16 fragment buffer [role * 16 + k-step][piece][lane * 8 + e] -> sorted int64 keys of the (p0, p1, p2) triples."""
    t = buf.reshape(-1, 3, 512).permute(0, 2, 1).reshape(-1, 3).to(torch.int64) & 0xFFFF
    return torch.sort((t[:, 0] << 32) | (t[:, 1] << 16) | t[:, 2])[0]


def pack_desc(case, W=None, want=None, off=None, preset=None):
    W = R.pack_weight(case) if W is None else W
    if want is None:
        want = ("Wup", "amax") if case.kind == 1 else ("Wdown", "Wup", "amax") + (("Fdown", "Fup") if case.frags else ())
    d = dict(kind=case.kind, W=W, want=tuple(want), off=case.off if off is None else off, ld=case.ld_mul * case.Cv if case.ld_mul > 1 else 0,
             col_off=case.col_off)
    if preset is not None:
        d["preset"] = preset
    return d


def check_pack_output(case, W, o, want, what):
    """One descriptor's outputs against the index model, bit for bit."""
    down, up = R.pack_ref(case.kind, W)
    assert o["guards"], f"{what}: a sentinel next to a buffer was overwritten"
    if "Wdown" in want:
        assert same_bits(o["Wdown"], R.place_down(down, case.ld_mul * case.Cv, case.col_off)), f"{what}: Wdown"
    if "Wup" in want:
        no_nan(o["Wup"], what)
        assert same_bits(o["Wup"], up), f"{what}: Wup"
    if "amax" in want:
        assert float(o["amax"]) == float(W.abs().max()), f"{what}: amax {float(o['amax'])} != max|W| {float(W.abs().max())}"
    for k in ("Fdown", "Fup"):
        if k in want:
            assert not bool((o[k] == -1).any()), f"{what}: {k} has bytes that were not written"
            host = R.bf3_split(W).t().to(torch.int64) & 0xFFFF
            keys = torch.sort((host[:, 0] << 32) | (host[:, 1] << 16) | host[:, 2])[0]
            assert torch.equal(frag_triples(o[k]), keys), f"{what}: the pieces of {k} are not those of the host split of Wref"


def check_pack(case, be):
    W = R.pack_weight(case)
    full = pack_desc(case)
    want = full["want"]
    got = be.pack([full])[0]
    check_pack_output(case, W, got, want, case.name)
    again = be.pack([full])[0]
    for k in want:
        assert same_bits(got[k], again[k]), f"{case.name}: {k} differs in a second launch"
    # each output NULL in turn: the others keep their bits
    for drop in want:
        rest = tuple(k for k in want if k != drop)
        if not rest or (case.kind == 1 and drop == "Wup") or rest == ("amax",):
            continue
        o = be.pack([pack_desc(case, want=rest)])[0]
        assert o["guards"], f"{case.name} without {drop}"
        for k in rest:
            assert same_bits(o[k], got[k]), f"{case.name}: {k} changes when {drop} is NULL"
    if case.frags and case.off:  # (c) the generic branch writes the fragment bytes of the tiled branch
        al = be.pack([pack_desc(case, off=False)])[0]
        for k in ("Fdown", "Fup", "Wdown", "Wup", "amax"):
            assert same_bits(al[k], got[k]), f"{case.name}: {k} of the tiled and of the element-per-thread branch differ"
    if case.kind in (0, 1):  # the single-layer entries
        w1 = ("Wup",) if case.kind == 1 else ("Wdown", "Wup")
        o = be.pack([pack_desc(case, want=w1)], via="single")[0]
        check_pack_output(case, W, o, w1, case.name + " (single-layer entry)")
        if case.kind == 0:
            for one in w1:
                o1 = be.pack([pack_desc(case, want=(one,))], via="single")[0]
                assert o1["guards"] and same_bits(o1[one], o[one]), f"{case.name}: single-layer entry with only {one}"


def expected_adam_kernels(case):
    if case.entry == "dev":
        return ["adam4_dev_kernel", "adam_publish_kernel"]
    return ["adam4_kernel" if case.n % 4 == 0 and not case.off else "adam_kernel"]


def check_adam(case, be, measured=None):
    inp = R.adam_inputs(case)
    got = be.adam(case, inp)
    ref, base = R.adam_ref(case, inp)
    assert got["guards"], f"{case.name}: a sentinel next to a buffer was overwritten"
    for k in ("p", "m", "v", "vmax", "g"):
        if k in ref:
            no_nan(got[k], f"{case.name}: {k}")
    for st, r in R.adam_ratios(case, got, ref, base).items():
        hold(measured, st, r, case.name)
    if got["kernels"] is not None:
        assert got["kernels"] == expected_adam_kernels(case), (case.name, got["kernels"])
    # the gradient: cleared to +0.0 exactly, or left bit for bit
    assert same_bits(got["g"], torch.zeros(case.n) if case.zero else inp["g"]), f"{case.name}: g"
    if case.regime == "zeros":
        assert same_bits(got["p"], inp["p"]), f"{case.name}: p moved although v = g = m = 0"
    if got["pub"] is not None:
        want = R.adam_scalars(case.lr, case.step, case.wd, case.gscale)
        w32 = torch.tensor(want, dtype=torch.float32)
        for i in (1, 2, 3, 4, 5, 7):
            assert same_bits(got["pub"][i], w32[i]), f"{case.name}: published scalar {i}"
        for i in (0, 6):  # pow of the C library against Python's
            assert abs(float(got["pub"][i]) - want[i]) <= 2.0 ** -23 * abs(want[i]), f"{case.name}: published scalar {i}"
    if case.entry == "dev":  # the same adam_one on float4 with the same eight floats: the bits of the host-scalar launch
        fz = be.adam(case._replace(entry="fused"), inp)
        for k in ("p", "m", "v", "vmax", "g"):
            if k in ref:
                assert same_bits(got[k], fz[k]), f"{case.name}: {k} of mvk_adam_step_dev and of mvk_adam_step_fused differ in their bits"
    again = be.adam(case, inp, names=None)
    for k in ("p", "m", "v", "vmax", "g"):
        if k in ref:
            assert same_bits(got[k], again[k]), f"{case.name}: {k} differs in a second launch"


def _prod32(a, b):
    return a * b


def check_act_bwd(n, act, off, be, measured=None, names=None):
    name = f"act_bwd-n{n}-act{act}" + (f"-off_{off}" if off else "")
    dY, Y = R.act_inputs(n, act)
    got = be.act_bwd(dY, Y, act, off, names)
    assert got["guards"] and got["Y_kept"], name
    no_nan(got["out"], name)
    if act == R.SIGMOID:
        ref = dY.double() * R.act_grad64(Y, act)
        hold(measured, "act_bwd.sigmoid", R.worst_ratio(got["out"], ref, R.U * ref.abs() + R.SUB), name)
    else:
        assert same_bits(got["out"], _prod32(dY, R.act_grad32(Y, act))), f"{name}: not the fp32 product"
    if got["kernels"] is not None:
        assert got["kernels"] == ["act_bwd4_kernel" if n % 4 == 0 and not off else "act_bwd_kernel"], (name, got["kernels"])
    assert same_bits(be.act_bwd(dY, Y, act, off)["out"], got["out"]), f"{name}: second launch"
    return got["out"]


def check_act_bwd_scaled(n, act, off, be, measured=None):
    name = f"act_bwd_scaled-n{n}-act{act}" + (f"-off_{off}" if off else "")
    g, Y = R.act_inputs(n, act, seed=1)
    a = R.f32(0.1)
    got = be.act_bwd_scaled(g, a, Y, act, off)
    assert got["guards"], name
    no_nan(got["out"], name)
    if act == R.SIGMOID:
        ref = a * g.double() * R.act_grad64(Y, act)
        hold(measured, "act_bwd_scaled.sigmoid", R.worst_ratio(got["out"], ref, R.U * ref.abs() + R.SUB), name)
    else:
        assert same_bits(got["out"], _prod32(torch.tensor(a) * g, R.act_grad32(Y, act))), f"{name}: not the fp32 product (a g) act'"
    if off:  # vector lanes and tail lanes compute one expression
        assert same_bits(be.act_bwd_scaled(g, a, Y, act, None)["out"], got["out"]), f"{name}: aligned and unaligned runs differ"
    assert same_bits(be.act_bwd_scaled(g, a, Y, act, off)["out"], got["out"]), f"{name}: second launch"


def check_axpby(n, mode, off, be, measured=None, names=None, sigmoid_yard=None):
    """mode: "xy", "x" (y NULL), "y" (x NULL)."""
    name = f"axpby-n{n}-{mode}" + (f"-off_{off}" if off else "")
    g_ = R.gen(n % 1000 + len(mode))
    x = torch.randn(n, generator=g_) * 3 if "x" in mode else None
    y = torch.randn(n, generator=g_) * 40 if "y" in mode else None
    a, b = R.f32(0.1), R.f32(-1.7)
    pre = be.axpby(x, a, y, b, R.NONE, n, off, names)
    assert pre["guards"], name
    no_nan(pre["out"], name)
    ref, mag = R.axpby_ref(x, a, y, b)
    hold(measured, "axpby", R.worst_ratio(pre["out"], ref, R.U * mag + R.SUB), name)
    if pre["kernels"] is not None:
        assert pre["kernels"] == ["axpby4_kernel" if n % 4 == 0 and not off else "axpby_kernel"], (name, pre["kernels"])
    v = pre["out"]
    relu = be.axpby(x, a, y, b, R.RELU, n, off)
    leaky = be.axpby(x, a, y, b, R.LEAKY, n, off)
    sig = be.axpby(x, a, y, b, R.SIGMOID, n, off)
    assert relu["guards"] and leaky["guards"] and sig["guards"], name
    assert same_bits(relu["out"], torch.where(v > 0, v, torch.zeros_like(v))), f"{name}: ReLU is not act(own pre-activation)"
    assert same_bits(leaky["out"], torch.where(v > 0, v, R.F02 * v)), f"{name}: LeakyReLU is not act(own pre-activation)"
    s64 = torch.sigmoid(v.double())
    mine = R.sigmoid_ulps(sig["out"], s64)
    yard = sigmoid_yard(v) if sigmoid_yard else R.sigmoid_ulps(torch.sigmoid(v), s64)
    print(f"{name}: sigmoid ulp kernel {mine:.3f}, torch fp32 {yard:.3f}")
    assert mine <= max(2 * yard, 1.0), (name, mine, yard)
    assert same_bits(be.axpby(x, a, y, b, R.NONE, n, off)["out"], v), f"{name}: second launch"


def check_bf3(n, be):
    x = R.bf3_input(n)
    host = R.bf3_split(x)
    got = be.f32_to_bf3(x)
    assert got["guards"], f"bf3 n={n}: a sentinel behind a plane was overwritten"
    assert got["out"].dtype == torch.int16 and torch.equal(got["out"], host), f"bf3 n={n}: the planes are not the host split"
    assert torch.equal(be.f32_to_bf3(x, off=True)["out"], host), f"bf3 n={n}: misaligned input"
    back = be.bf3_to_f32(got["out"])
    assert back["guards"] and same_bits(back["out"], x), f"bf3 n={n}: the round trip does not return the input"
    assert same_bits(be.bf3_to_f32(got["out"], off=True)["out"], x), f"bf3 n={n}: round trip into a misaligned output"


def check_layout(shape, be):
    n, c, h, w = shape
    x = torch.randn(n, c, h, w, generator=R.gen(sum(shape)))
    a = be.layout(x, True)
    assert a["guards"] and same_bits(a["out"], x.permute(0, 2, 3, 1).contiguous()), f"nchw_to_nhwc {shape}"
    b = be.layout(a["out"], False)
    assert b["guards"] and same_bits(b["out"], x), f"nhwc_to_nchw {shape}: not the inverse"
    y = torch.randn(n, h, w, c, generator=R.gen(sum(shape) + 1))
    c_ = be.layout(y, False)
    assert c_["guards"] and same_bits(c_["out"], y.permute(0, 3, 1, 2).contiguous()), f"nhwc_to_nchw {shape}"
    assert same_bits(be.layout(x, True)["out"], a["out"])


def pool_kernel(op, shape, off):
    base = {"pool.fwd": "avgpool3s2_fwd_kernel", "pool.bwd": "avgpool3s2_bwd_kernel", "up.fwd": "upsample2_fwd_kernel",
            "up.bwd": "upsample2_bwd_kernel"}[op]
    return [f"{base}<{4 if shape[3] % 4 == 0 and not off else 1}>"]


def check_pool(op, shape, be, measured=None, names=None):
    n, H, W, C = shape
    name = f"{op}-{R.pool_name(shape)}"
    x = R.pool_inputs(shape, op)
    got = be.pool(op, x, shape, False, names)
    assert got["guards"], name
    no_nan(got["out"], name)
    if op == "pool.fwd":
        ref, mag = R.pool_fwd_ref(x)
        hold(measured, op, R.worst_ratio(got["out"], ref, R.U * mag / 9 + R.SUB), name)
    elif op == "pool.bwd":
        ref, mag = R.pool_bwd_ref(x, H, W)
        hold(measured, op, R.worst_ratio(got["out"], ref, R.U * mag / 9 + R.SUB), name)
    elif op == "up.fwd":
        assert same_bits(got["out"], R.up_fwd_ref(x)), f"{name}: not the nearest-neighbour copy"
    else:
        ref, mag = R.up_bwd_ref(x)
        hold(measured, op, R.worst_ratio(got["out"], ref, R.U * mag + R.SUB), name)
    if got["kernels"] is not None:
        assert got["kernels"] == pool_kernel(op, shape, False), (name, got["kernels"])
    offr = be.pool(op, x, shape, True, names)  # the same data 4 bytes off: the V = 1 leaf, one order of summation
    assert offr["guards"], name + "-off"
    if offr["kernels"] is not None:
        assert offr["kernels"] == pool_kernel(op, shape, True), (name, offr["kernels"])
    assert same_bits(offr["out"], got["out"]), f"{name}: the V = 4 and the V = 1 leaves differ in their bits"
    assert same_bits(be.pool(op, x, shape, False)["out"], got["out"]), f"{name}: second launch"


def check_rng(case, be, measured=None):
    n, threads = case.n, (case.n + 3) // 4
    grid = (threads + 255) // 256
    words = R.rng_words(case.seed, case.offset, n)
    # uniform at (0, 1): every factor is a power of two or an integer below 2^24, so the draw is exact
    u = be.rng((case.seed, case.offset, 0), n, True, 0.0, 1.0, case.off)
    assert u["guards"], case.name
    no_nan(u["out"], case.name)
    ref, _ = R.rng_uniform_ref(words, n)
    assert same_bits(u["out"], ref.float()), f"{case.name}: uniform draws differ from the Philox emulation"
    assert bool((u["out"] >= 0).all()) and bool((u["out"] < 1).all())
    new_off = (case.offset + grid * 256) % 2 ** 64
    assert u["state"][0] == case.seed and u["state"][1] == new_off and u["state"][2] & 0xFFFFFFFF == 0, (case.name, u["state"])
    # the next launch continues behind the counters of this one
    u2 = be.rng(tuple(u["state"]), n, True, 0.0, 1.0, case.off)
    ref2, _ = R.rng_uniform_ref(R.rng_words(case.seed, new_off, n), n)
    assert same_bits(u2["out"], ref2.float()) and u2["state"][1] == (new_off + grid * 256) % 2 ** 64, f"{case.name}: second launch"
    assert n < 4 or not torch.equal(u2["out"], u["out"]), f"{case.name}: the second launch repeats the first"
    assert same_bits(be.rng((case.seed, case.offset, 0), n, True, 0.0, 1.0, case.off)["out"], u["out"])
    # a general interval: the roundings of (hi - lo), the product and the sum
    lo, hi = -2.0, R.f32(3.3)
    w = be.rng((case.seed, case.offset, 0), n, True, lo, hi, case.off)
    ref, mag = R.rng_uniform_ref(words, n, lo, hi)
    hold(measured, "rng.uniform", R.worst_ratio(w["out"], ref, R.U * mag), case.name)
    # normal draws: Box-Muller of the same words; cosine first, sine second
    z = be.rng((case.seed, case.offset, 0), n, False, 0.0, 1.0, case.off)
    assert z["guards"] and z["state"][1] == new_off, case.name
    no_nan(z["out"], case.name)
    ref, base = R.rng_normal_ref(words, n)
    hold(measured, "rng.normal", R.worst_ratio(z["out"], ref, R.U * base), case.name)
    assert same_bits(be.rng((case.seed, case.offset, 0), n, False, 0.0, 1.0, case.off)["out"], z["out"])


# ---- weight packs ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.PACK_CASES, ids=[c.name for c in R.PACK_CASES])
def test_pack(case):
    check_pack(case, HIP)


def test_pack_one_launch_of_sixteen():
    """MVK_PACK_MAX descriptors of all three kinds, both kind-0 branches, with and without fragments, in one launch: every
    descriptor has the bits of its launch alone (the grid is sized by the largest, so the small ones see idle workgroups)."""
    cases = R.PACK_CASES
    assert len(cases) == 16 and {c.kind for c in cases} == {0, 1, 2}
    descs = [pack_desc(c) for c in cases]
    alone = [HIP.pack([d])[0] for d in descs]
    both = HIP.pack(descs)
    for c, d, a, o in zip(cases, descs, alone, both):
        assert o["guards"], c.name
        for k in d["want"]:
            assert same_bits(o[k], a[k]), f"{c.name}: {k} differs from the descriptor launched alone"


AMAX_POS = [0, -1, 8191, 8192, 65535, 65536]


def test_pack_amax_positions():
    """The unique maximum at the first element, the last, and on both sides of the 8192-element sweep of 32 workgroups and of the
    65536-element round of pack_amax, for the tiled and the element-per-thread kind-0 branch, kind 1 and kind 2, as descriptors of
    two launches; its sign alternates.  A slot preset above the maximum keeps its value, one preset below is raised."""
    jobs = []
    for name, off in (("k0-cv128-cu64-frag", False), ("k0-cv128-cu64-frag", True), ("k1-cv20-cu128", False), ("k2-cv128-cu128", False)):
        case = R.PACK_BY_NAME[name]
        total = case.Cv * case.Cu * R.pack_taps(case.kind)
        for i, pos in enumerate(AMAX_POS):
            if pos >= total:
                continue
            W = torch.rand(total, generator=R.gen(pos % 97 + total % 89)) * 2 - 1
            W[pos] = 3.0 if i % 2 else -3.0
            jobs.append((case, off, pos, W.reshape(case.Cv, case.Cu, -1)))
    assert len(jobs) == 22
    presets = [0.0, 0.5, 7.0]
    for lo in (0, 16):
        part = jobs[lo:lo + 16]
        descs = [pack_desc(c, W=W, want=("Wup", "amax"), off=off, preset=presets[i % 3]) for i, (c, off, pos, W) in enumerate(part)]
        outs = HIP.pack(descs)
        for i, ((c, off, pos, W), o) in enumerate(zip(part, outs)):
            assert o["guards"] and same_bits(o["Wup"], R.pack_ref(c.kind, W)[1]), (c.name, pos)
            assert float(o["amax"]) == max(3.0, presets[i % 3]), f"{c.name} off={off}: maximum at {pos}, preset {presets[i % 3]}: {float(o['amax'])}"


def test_pack_argument_checks():
    """n = 0 and n = 17, jobs NULL, Wref NULL, Cv or Cu 0, kind 3, no output at all, kind 1 without Wup, fragments on an uncovered
    pair or on kind 2 -- alone and as the last of two descriptors: MVK_EINVAL before the launch, nothing written.  The single-layer
    entries: Wref NULL, no output, Cin 0."""
    Lb = _lib()
    lib, sp = Lb.load(), Lb.stream_ptr
    c8, c64 = R.PACK_BY_NAME["k0-cv8-cu8"], R.PACK_BY_NAME["k0-cv64-cu32-frag"]
    good = pack_desc(c8)
    bad = [dict(good, Cv=0), dict(good, Cu=-8), dict(good, kind=3), dict(good, kind=-1),
           dict(good, want=()), dict(good, want=("amax",)), dict(good, kind=1, want=("Wdown",)),
           dict(good, want=("Wdown", "Fdown")), dict(good, want=("Fup",)),
           dict(pack_desc(c64), kind=2, W=torch.zeros(64, 32, 9))]
    for i, b in enumerate(bad):
        for descs in ([b], [good, b]):
            outs = HIP.pack(descs, may_fail=True)
            assert HIP.rc == EINVAL, f"bad descriptor {i} was accepted"
            assert all(o["untouched"] for o in outs), f"bad descriptor {i}: something was written"
    outs = HIP.pack([good] * 16, n_arg=17, may_fail=True)
    assert HIP.rc == EINVAL and all(o["untouched"] for o in outs)
    outs = HIP.pack([good], n_arg=0, may_fail=True)
    assert HIP.rc == EINVAL and outs[0]["untouched"]
    assert lib.mvk_pack_weights(None, 1, sp()) == EINVAL
    w, out = Guarded(8 * 8 * 16, fill=1.0), Guarded(8 * 8 * 16)
    assert lib.mvk_pack_conv4s2_weight(None, 8, 8, out.p, 0, 0, out.p, sp()) == EINVAL
    assert lib.mvk_pack_conv4s2_weight(w.p, 8, 8, None, 0, 0, None, sp()) == EINVAL
    assert lib.mvk_pack_conv4s2_weight(w.p, 0, 8, out.p, 0, 0, None, sp()) == EINVAL
    assert lib.mvk_pack_unflatten_weight(None, 8, 8, out.p, sp()) == EINVAL
    assert lib.mvk_pack_unflatten_weight(w.p, 8, 8, None, sp()) == EINVAL
    assert lib.mvk_pack_unflatten_weight(w.p, 8, 0, out.p, sp()) == EINVAL
    torch.cuda.synchronize()
    assert out.untouched() and w.intact()


# ---- Adam -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ADAM_CASES, ids=[c.name for c in R.ADAM_CASES])
def test_adam(case):
    check_adam(case, HIP, MEASURED)


@pytest.mark.parametrize("ams,zero", [(False, False), (True, True)])
def test_adam_identity(ams, zero):
    """Under the scalars of mvk_adam_identity, mvk_adam_step_dev keeps p, m, v and vmax bit for bit for finite gradients up to
    1e30 (no -0.0 among the inputs: m = -0.0 legitimately becomes +0.0; vmax >= v, the invariant every amsgrad step leaves: the
    running maximum is still taken); with zero_grad the gradient is cleared."""
    Lb, n = _lib(), 1028
    g_ = R.gen(5)
    inp = dict(p=torch.randn(n, generator=g_), g=torch.randn(n, generator=g_) * torch.exp2(torch.randint(-60, 100, (n,), generator=g_).float()),
               m=torch.randn(n, generator=g_), v=torch.rand(n, generator=g_) + 1e-12)
    inp["g"] = inp["g"].clamp(-1e30, 1e30)
    inp["g"][:4] = torch.tensor([1e30, -1e30, 0.0, 1e-40])
    inp["m"][:2], inp["v"][:2] = torch.tensor([0.0, 1e-40]), torch.tensor([0.0, 1e-40])
    inp["vmax"] = inp["v"] * (1 + torch.arange(n) % 2)
    assert bool(torch.isfinite(inp["g"]).all()) and float(inp["g"].abs().max()) <= R.f32(1e30)
    B = {k: Guarded(n, src=inp[k]) for k in inp}
    sc = Guarded(8)
    Lb.call("mvk_adam_identity", sc.p, Lb.stream_ptr())
    Lb.call("mvk_adam_step_dev", B["p"].p, B["g"].p, B["m"].p, B["v"].p, B["vmax"].p if ams else None, n, sc.p, int(zero), Lb.stream_ptr())
    torch.cuda.synchronize()
    assert same_bits(sc.cpu(8), torch.tensor([0.0, 0.0, 1.0, 0.0, 1.0, 0.0, 1.0, 0.0])) and sc.intact()
    for k in ("p", "m", "v", "vmax"):
        assert B[k].intact() and same_bits(B[k].cpu(n), inp[k]), f"{k} changed under the identity scalars"
    assert B["g"].intact() and same_bits(B["g"].cpu(n), torch.zeros(n) if zero else inp["g"])


def test_adam_prepare():
    """The eight floats against the Python-double formulas at steps 1, 2, 1000 and 100000: 1 - b1, b2, 1 - b2, eps, wd and gscale
    bit for bit, step_size and sqrt(bc2) within one fp32 ulp (the device's pow); k calls leave state[6] == k; state[0] written
    between two calls changes the learning rate of the next; nothing else of the state changes."""
    Lb = _lib()
    lr, wd, gs = 1e-3, 0.01, 0.5
    for first, calls in ((0, 2), (999, 1), (99999, 1)):
        st0 = [lr, 0.9, 0.999, 1e-8, wd, gs, float(first), 42.0]
        st = torch.tensor(st0, dtype=torch.float64, device=dev())
        sc = Guarded(8)
        for k in range(1, calls + 1):
            if k == 2:
                st[0] = 5e-4  # a scheduler writes the learning rate between replays
            Lb.call("mvk_adam_prepare", st.data_ptr(), sc.p, Lb.stream_ptr())
            torch.cuda.synchronize()
            now = st.cpu().tolist()
            assert now[6] == first + k and now[1:6] == st0[1:6] and now[7] == 42.0
            want = R.adam_scalars(now[0], first + k, wd, gs)
            got, w32 = sc.cpu(8), torch.tensor(want, dtype=torch.float32)
            for i in (1, 2, 3, 4, 5, 7):
                assert same_bits(got[i], w32[i]), f"step {first + k}: scalar {i}: {float(got[i])} != {float(w32[i])}"
            for i in (0, 6):
                assert abs(float(got[i]) - want[i]) <= 2.0 ** -23 * abs(want[i]), f"step {first + k}: scalar {i}: {float(got[i])} vs {want[i]}"
            assert sc.intact()


def test_adam_argument_checks():
    """MVK_EINVAL without a write: a misaligned publish or scalars pointer; mvk_adam_step_dev with n % 4 != 0 or any buffer 4 bytes
    off; step 0; a NULL buffer.  n = 0: mvk_adam_step_pub publishes the scalars and writes nothing else, the others write nothing."""
    Lb = _lib()
    lib, sp, n = Lb.load(), Lb.stream_ptr, 8
    hyper = (1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1.0)
    B = {k: Guarded(n + 1) for k in ("p", "g", "m", "v", "vmax")}
    sc, st = Guarded(9), torch.zeros(8, dtype=torch.float64, device=dev())
    P = [B[k].p for k in ("p", "g", "m", "v", "vmax")]
    assert lib.mvk_adam_step_pub(*P, n, *hyper, 0, sc.p + 4, sp()) == EINVAL
    assert lib.mvk_adam_step_pub(*P, 0, *hyper, 0, sc.p + 4, sp()) == EINVAL
    assert lib.mvk_adam_identity(sc.p + 4, sp()) == EINVAL and lib.mvk_adam_identity(None, sp()) == EINVAL
    assert lib.mvk_adam_prepare(st.data_ptr(), sc.p + 4, sp()) == EINVAL and lib.mvk_adam_prepare(None, sc.p, sp()) == EINVAL
    assert lib.mvk_adam_prepare(st.data_ptr(), None, sp()) == EINVAL
    assert lib.mvk_adam_step_dev(*P, n - 1, sc.p, 0, sp()) == EINVAL
    for i in range(5):
        Q = list(P)
        Q[i] += 4
        assert lib.mvk_adam_step_dev(*Q, n, sc.p, 0, sp()) == EINVAL, f"mvk_adam_step_dev accepted buffer {i} 4 bytes off"
        if i < 4:
            Q[i] = None
            assert lib.mvk_adam_step_dev(*Q, n, sc.p, 0, sp()) == EINVAL
            assert lib.mvk_adam_step_fused(*Q, n, *hyper, 0, sp()) == EINVAL
    assert lib.mvk_adam_step_dev(*P, n, None, 0, sp()) == EINVAL
    assert lib.mvk_adam_step_fused(*P, n, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1.0, 0, sp()) == EINVAL  # step 0
    assert lib.mvk_adam_step_pub(*P, -1, *hyper, 0, None, sp()) == EINVAL
    assert lib.mvk_adam_step(*P[:4], 0, *hyper, sp()) == 0 and lib.mvk_adam_step_fused(*P, 0, *hyper, 1, sp()) == 0
    assert lib.mvk_adam_step_dev(*P, 0, sc.p, 1, sp()) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in B.values()) and sc.untouched() and bool((st == 0).all())
    assert lib.mvk_adam_step_pub(*P, 0, *hyper, 1, sc.p, sp()) == 0  # publishes, and only that
    torch.cuda.synchronize()
    assert all(b.untouched() for b in B.values()) and sc.intact()
    got = sc.cpu(9)
    assert same_bits(got[:8], torch.tensor(R.adam_scalars(1e-3, 1, 0.0, 1.0), dtype=torch.float32)) and bool(torch.isnan(got[8]))


# ---- element-wise helpers -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", R.ACTS)
def test_act_bwd(act):
    for n in R.ACT_BWD_N:
        check_act_bwd(n, act, None, HIP, MEASURED, names="base" if n in (4, 5) else None)
    for off in ("dY", "Y"):
        check_act_bwd(1028, act, off, HIP, MEASURED, names="base")
    check_act_bwd(R.BIG + 3, act, "dY", HIP, MEASURED)  # past the 2048-workgroup cap of the scalar kernel


@pytest.mark.parametrize("act", R.ACTS)
def test_act_bwd_scaled(act):
    for n in R.ACT_SCALED_N:
        check_act_bwd_scaled(n, act, None, HIP, MEASURED)
    for off in ("g", "Y", "out"):
        for n in (9, 1027, 1028):
            check_act_bwd_scaled(n, act, off, HIP, MEASURED)


def _gpu_sigmoid_ulps(v):
    return R.sigmoid_ulps(torch.sigmoid(v.to(dev())).cpu(), torch.sigmoid(v.double()))


@pytest.mark.parametrize("mode", ["xy", "x", "y"])
def test_axpby(mode):
    for n, off, names in ((1, None, None), (4, None, "base"), (5, None, "base"), (1023, None, None), (1028, None, None),
                          (1028, "out", "base"), (1028, "x" if "x" in mode else "y", "base"), (1028, "y" if "y" in mode else "x", None)):
        check_axpby(n, mode, off, HIP, MEASURED, names, _gpu_sigmoid_ulps)


@pytest.mark.parametrize("n", [1, 2, 3, 511, 512, 513])
def test_bf3(n):
    check_bf3(n, HIP)


@pytest.mark.parametrize("shape", R.LAYOUT_SHAPES, ids=[R.pool_name(s) for s in R.LAYOUT_SHAPES])
def test_layout(shape):
    check_layout(shape, HIP)


def test_elementwise_argument_checks():
    """Every MVK_EINVAL branch of the element-wise entries returns without a write, and n = 0 is MVK_OK and writes nothing."""
    Lb = _lib()
    lib, sp = Lb.load(), Lb.stream_ptr
    src, out, pl = Guarded(64, fill=0.5), Guarded(64), Guarded(192, dtype=torch.int16)
    st = torch.zeros(3, dtype=torch.int64, device=dev())
    E = EINVAL
    assert lib.mvk_act_bwd(None, src.p, 4, 1, sp()) == E and lib.mvk_act_bwd(out.p, None, 4, 1, sp()) == E
    assert lib.mvk_act_bwd(out.p, src.p, 0, 1, sp()) == 0
    for a in ((None, 1.0, src.p, 1, out.p, 4), (src.p, 1.0, None, 1, out.p, 4), (src.p, 1.0, src.p, 1, None, 4), (src.p, 1.0, src.p, 1, out.p, -1)):
        assert lib.mvk_act_bwd_scaled(*a, sp()) == E
    assert lib.mvk_act_bwd_scaled(src.p, 1.0, src.p, 1, out.p, 0, sp()) == 0
    assert lib.mvk_axpby(None, 1.0, None, 1.0, 4, 0, out.p, sp()) == E and lib.mvk_axpby(src.p, 1.0, src.p, 1.0, 4, 0, None, sp()) == E
    assert lib.mvk_axpby(src.p, 1.0, src.p, 1.0, -1, 0, out.p, sp()) == E and lib.mvk_axpby(src.p, 1.0, None, 1.0, 0, 0, out.p, sp()) == 0
    assert lib.mvk_f32_to_bf3(None, 4, pl.p, sp()) == E and lib.mvk_f32_to_bf3(src.p, 4, None, sp()) == E
    assert lib.mvk_f32_to_bf3(src.p, -1, pl.p, sp()) == E and lib.mvk_f32_to_bf3(src.p, 0, pl.p, sp()) == 0
    assert lib.mvk_bf3_to_f32(None, 4, out.p, sp()) == E and lib.mvk_bf3_to_f32(pl.p, 4, None, sp()) == E
    assert lib.mvk_bf3_to_f32(pl.p, -1, out.p, sp()) == E and lib.mvk_bf3_to_f32(pl.p, 0, out.p, sp()) == 0
    for fn in (lib.mvk_nchw_to_nhwc, lib.mvk_nhwc_to_nchw):
        assert fn(None, out.p, 1, 2, 2, 2, sp()) == E and fn(src.p, None, 1, 2, 2, 2, sp()) == E
        assert fn(src.p, out.p, 0, 2, 2, 2, sp()) == 0 and fn(src.p, out.p, 2, 2, 0, 2, sp()) == 0
    for fn in (lib.mvk_avgpool3s2_fwd, lib.mvk_avgpool3s2_bwd, lib.mvk_upsample2_fwd, lib.mvk_upsample2_bwd):
        for a in ((None, out.p, 1, 2, 2, 4), (src.p, None, 1, 2, 2, 4), (src.p, out.p, -1, 2, 2, 4), (src.p, out.p, 1, 0, 2, 4),
                  (src.p, out.p, 1, 2, 0, 4), (src.p, out.p, 1, 2, 2, 0)):
            assert fn(*a, sp()) == E
        assert fn(src.p, out.p, 0, 2, 2, 4, sp()) == 0
    assert lib.mvk_device_rng(None, 4, st.data_ptr(), 1, 0.0, 1.0, sp()) == E and lib.mvk_device_rng(out.p, 4, None, 1, 0.0, 1.0, sp()) == E
    assert lib.mvk_device_rng(out.p, -1, st.data_ptr(), 1, 0.0, 1.0, sp()) == E and lib.mvk_device_rng(out.p, 0, st.data_ptr(), 1, 0.0, 1.0, sp()) == 0
    torch.cuda.synchronize()
    assert out.untouched() and pl.untouched() and src.intact() and bool((src.body == 0.5).all()) and bool((st == 0).all())


# ---- pooling and upsampling -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["pool.fwd", "pool.bwd", "up.fwd", "up.bwd"])
def test_pool(op):
    for shape in R.POOL_SHAPES:
        check_pool(op, shape, HIP, MEASURED, names="full" if shape in ((2, 7, 7, 20), (2, 5, 9, 3)) else None)


# ---- the device-resident generator ----------------------------------------------------------------------------------------------------------
def test_rng_known_answer():
    """Philox4x32-10 with counter 0 and key 0 through the kernel: out * 2^24 are the four words of the published answer >> 8."""
    u = HIP.rng((0, 0, 0), 4, True, 0.0, 1.0)
    assert [int(v) for v in (u["out"].double() * 2.0 ** 24).tolist()] == [w >> 8 for w in R.PHILOX_KAT[0][2]]


@pytest.mark.parametrize("case", R.RNG_CASES, ids=[c.name for c in R.RNG_CASES])
def test_rng(case):
    check_rng(case, HIP, MEASURED)


def test_zz_report():
    """Prints the head-room the HIP kernels showed in this session (the largest |err| / base per stage, with the case) and the
    wall time of this file."""
    print("HIP_MEASURED", {k: (round(v, 3), n) for k, (v, n) in sorted(MEASURED.items())})
    print(f"WALL test_gpu_misc.py {time.time() - _T0:.1f} s")
