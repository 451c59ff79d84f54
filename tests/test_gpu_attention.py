"""Every attention kernel in every geometry the engine launches, one launch at a time through
capgen_debug_attention_geom (and the three fused fronts, and attention_head_mean) against the float64
restatement tests/attention_ref.py.  The cases are defined in test_attention_host.py, which also checks on
the CPU that each meets the conditions that make a wrong mask visible (a live key in every row, the
smallest live probability >= 1e-3, dropped share within 4 sd, mixed 16 x 16 dropout blocks at 64 x 64).
Inputs come from fixed-seed CPU generators scaled by 0.5; bf16 cases hand the reference the bf16-rounded
inputs.

Guards: every output buffer is wider and longer than the geometry and pre-filled with a sentinel; whatever
the geometry does not name must come back bit-unchanged (in the packed-qkv layout dq, dk and dv share one
buffer: each must leave the others' columns alone).  Slots the geometry must not read -- cache positions
> t, rows no kv_row entry names, keys >= Lk, the slab's other layer -- hold the finite poison 1e4.

Tolerances:
  probs (every path) and f32 outputs   |got - ref| <= k x 1e-5 x max|ref| of the tensor.  The restatement
      evaluated in float32 on the CPU is within 5.9e-7 max|ref| of float64 for every tensor of every case
      (probs 2.5e-7), below 1e-5 / 8 = 1.25e-6: k = 1 throughout (k_of() would raise it to 8 x the noise).
  bf16 outputs of the VALU and decode kernels (f32 accumulation, one output rounding)
      + 2^-8 |ref| elementwise
  bf16 MFMA outputs: + one rounding of the operand the kernel rounds to bf16 before its MFMA
      o  + 2^-8 sum_j Pd_ij |v_jd|        dv + 2^-8 sum_i Pd_ij |dO_id|
      dq + 2^-8 sum_j |dS_ij| |k_jd| / T  dk + 2^-8 sum_i |dS_ij| |q_id| / T
  attention_bwd_wo (dO = dA . Wo made inside the launch and rounded to bf16 there): the reference takes the
      bf16 rounding of the float64 product as dO, and the MFMA bound above holds as it stands.
With CAPGEN_ATTN_REPORT=<path> the module writes the worst err / bound per kernel family and tensor;
profiles/attention_kernel_tests.txt records them.
"""
import ctypes as C
import os

import pytest
import torch

import attention_ref as R
import test_attention_host as K
from test_attention_host import BF16, F32, TDT
from test_gpu_rowops import DEV, P, assert_same, call, gen

gpu = pytest.mark.gpu
SENT = -77.0


def ptr(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off * t.element_size())


class Launch:
    """one geometry on the device: inputs uploaded (a buffer shared by q / k / v once), outputs allocated
    with the sentinel"""

    def __init__(self, g, dtype, probs=True, backward=False):
        from capgen import _lib
        self.g, self.dtype, td = g, dtype, TDT[dtype]
        self.bufs = {}
        for t in (g.q, g.k, g.v):
            if id(t) not in self.bufs:
                self.bufs[id(t)] = t.to(DEV)
        self.aux = {n: (None if t is None else t.to(DEV)) for n, t in
                    (("kv_row", g.kv_row), ("key_valid", g.key_valid), ("key_ids", g.key_ids))}
        self.o = torch.full((g.extra["o_numel"],), SENT, dtype=td, device=DEV)
        n_p = g.B * g.H * g.Lq * g.Lk
        self.probs = torch.full((n_p + 64,), SENT, device=DEV) if probs else None
        self.dout = self.grads = None
        if backward:
            self.dout = g.extra["dout"].to(DEV)
            self.grads = {i: torch.full_like(b, SENT) for i, b in self.bufs.items()}
        c = _lib.capgen_attn_geom()
        c.B, c.H, c.Lq, c.Lk, c.dk = g.B, g.H, g.Lq, g.Lk, g.dk
        for n in "qkv":
            buf = self.bufs[id(getattr(g, n))]
            setattr(c, n, ptr(buf, getattr(g, n + "_off")))
            setattr(c, n + "_ld", getattr(g, n + "_ld"))
            setattr(c, n + "_bs", getattr(g, n + "_bs"))
        c.o_ld, c.o_bs, c.kv_bmod = g.o_ld, g.o_bs, g.kv_bmod
        c.kv_row, c.kv_row_ld = ptr(self.aux["kv_row"]), g.kv_row_ld
        c.key_valid, c.kv_bs = ptr(self.aux["key_valid"]), g.kv_bs
        c.key_ids, c.kid_bs, c.pad_idx = ptr(self.aux["key_ids"]), g.kid_bs, g.pad_idx
        c.causal, c.q_pos0, c.temperature = g.causal, g.q_pos0, g.temperature
        c.drop_p, c.drop_site, c.drop_seed = g.drop_p, g.drop_site, g.drop_seed
        self.c = c

    def args(self):
        g, gr = self.g, self.grads
        d = [None, None, None] if gr is None else [ptr(gr[id(getattr(g, n))], getattr(g, n + "_off")) for n in "qkv"]
        return (self.dtype, C.byref(self.c), P(self.o), P(self.probs), P(self.dout), *d, None)

    def run(self):
        call("capgen_debug_attention_geom", *self.args())
        return self

    # ---- results as the reference lays them out, and the guard regions ----
    def out(self, name):
        g = self.g
        if name == "probs":
            return self.probs.cpu()[:g.B * g.H * g.Lq * g.Lk].view(g.B, g.H, g.Lq, g.Lk)
        if name == "o":
            return self.o.cpu()[R.index(0, g.o_ld, g.o_bs, g.B, g.H, g.Lq, g.dk)]
        n = name[1]
        L = g.Lq if n == "q" else g.Lk
        idx = R.index(getattr(g, n + "_off"), getattr(g, n + "_ld"), getattr(g, n + "_bs"), g.B, g.H, L, g.dk)
        return self.grads[id(getattr(g, n))].cpu().flatten()[idx]

    def check_guards(self, tag):
        g = self.g
        sent = torch.tensor(SENT)
        w = torch.zeros(self.o.numel(), dtype=torch.bool)
        w[R.index(0, g.o_ld, g.o_bs, g.B, g.H, g.Lq, g.dk).flatten()] = True
        assert (~w).any()
        o = self.o.cpu()
        assert_same(o[~w], sent.to(o.dtype).expand(int((~w).sum())).contiguous(), tag + ": o guard")
        if self.probs is not None:
            tail = self.probs.cpu()[g.B * g.H * g.Lq * g.Lk:]
            assert_same(tail, torch.full_like(tail, SENT), tag + ": probs guard")
        if self.grads is None:
            return
        for i, gb in self.grads.items():
            w = torch.zeros(gb.numel(), dtype=torch.bool)
            for n in "qkv":
                if id(getattr(g, n)) == i:
                    L = g.Lq if n == "q" else g.Lk
                    w[R.index(getattr(g, n + "_off"), getattr(g, n + "_ld"), getattr(g, n + "_bs"), g.B, g.H, L,
                              g.dk).flatten()] = True
            assert (~w).any()
            gc = gb.cpu().flatten()
            assert_same(gc[~w], sent.to(gc.dtype).expand(int((~w).sum())).contiguous(), tag + ": gradient guard")


WORST = {}


def check(got, ref, k, out_bf16, extra, what, fam):
    """|got - ref| <= k 1e-5 max|ref| (+ 2^-8 |ref| for a bf16 output) (+ extra); returns err / bound"""
    got, ref = got.double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    bound = k * 1e-5 * ref.abs().max().clamp_min(1e-30) + torch.zeros_like(ref)
    if out_bf16:
        bound = bound + 2.0 ** -8 * ref.abs()
    if extra is not None:
        bound = bound + extra
    ratio = ((got - ref).abs() / bound).max().item()
    key = (fam, what.rsplit(" ", 1)[-1])
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    assert ratio <= 1.0, f"{what}: err / bound = {ratio:.3f} ({int(((got - ref).abs() > bound).sum())} of " \
                         f"{got.numel()} out)"
    return ratio


@pytest.fixture(scope="module", autouse=True)
def worst_record():
    """With CAPGEN_ATTN_REPORT=<path> the worst err / bound of every (kernel family, tensor) this module's tests
    reached is written there once, when the module is done, whatever the order of the tests (the source of
    profiles/attention_kernel_tests.txt)."""
    yield
    path = os.environ.get("CAPGEN_ATTN_REPORT")
    if path:
        with open(path, "w") as f:
            for (fam, t), v in sorted(WORST.items()):
                f.write(f"{fam}\t{t}\t{v:.3f}\n")


def compare(run, r, fam, fwd_mfma=False, bwd_mfma=False):
    g, bf = run.g, run.dtype == BF16
    tag = g.extra["tag"]
    ex = {t: e for t, e in R.mfma_extra(r).items() if (fwd_mfma if t == "o" else bwd_mfma)}
    names = ["o"] + (["probs"] if run.probs is not None else []) + (["dq", "dk", "dv"] if run.grads else [])
    for t in names:
        check(run.out(t), r[t], K.k_of(r["noise"][t]), bf and t != "probs", ex.get(t), f"{tag} {t}", fam)
    run.check_guards(tag)


# ---- A. the decode step ---------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("table", [0, 1])
@pytest.mark.parametrize("R_,H", K.DEC_RH)
@pytest.mark.parametrize("mode", sorted(K.MODES))
def test_decode_self(mode, R_, H, table):
    """dec_step's self attention (cache strides, key ids, causal with q_pos0 = t, the beam row table) at
    Lk on both sides of every LKM / NIT boundary, each with and without probs"""
    for Lk in K.DEC_LKS:
        g = K.dec_self_case(mode, R_, H, Lk, bool(table))
        fam = K.decode_kernel(g, mode)
        r = K.ref_of(g)
        a = Launch(g, K.MODES[mode], probs=True).run()
        b = Launch(g, K.MODES[mode], probs=False).run()
        compare(a, r, fam)
        compare(b, r, fam)
        assert_same(b.o.cpu(), a.o.cpu(), g.extra["tag"] + ": o differs with / without probs")


@gpu
@pytest.mark.parametrize("Rq,N", [(G * K.CROSS_BIMG, N) for G, N in K.CROSS_GN] + [(7, 36)])
@pytest.mark.parametrize("mode", sorted(K.MODES))
def test_decode_cross(set_knob, mode, Rq, N):
    """dec_step's cross attention (kv_bmod, key_valid, the slab's strides) over the G ladder, with and
    without probs; bf16: DECODE_GROUP_LDS on and off return the same bits"""
    g = K.dec_cross_case(mode, Rq, N)
    r = K.ref_of(g)
    outs = []
    for lds in ((1, 0) if mode == "bf16" else (1,)):
        set_knob("DECODE_GROUP_LDS", lds)
        fam = K.decode_kernel(g, mode, lds)
        for probs in (True, False):
            run = Launch(g, K.MODES[mode], probs=probs).run()
            compare(run, r, fam)
            outs.append((run.o.cpu(), run.probs.cpu() if probs else None))
    for o, p in outs[1:]:
        assert_same(o, outs[0][0], g.extra["tag"] + ": o differs between probs / LDS settings")
        if p is not None:
            assert_same(p, outs[0][1], g.extra["tag"] + ": probs differ between LDS settings")


# ---- B. the full kernels --------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("dtype,dk,H", K.KERNELS)
def test_full_kernels(dtype, dk, H):
    """forward + backward at every layout x (Lq, Lk), dropout off and at p = 0.1 / 0.5: the backward must
    drop exactly the elements the forward dropped (the bf16 MFMA backward recomputes the mask)"""
    for g in K.full_cases(dtype, dk, H):
        kern = K.full_kernel(g, dtype)
        bwd = None if g.extra.get("fwd_only") else K.bwd_kernel(g, dtype)
        fm, bm = "mfma" in kern or "wave" in kern, bwd is not None and "mfma" in bwd
        # (the MFMA backward never reads probs; every second MFMA case runs without them)
        probs = not (fm and bm and g.Lk % 2 == 1 and g.drop_p == 0)
        if kern == "decode":  # (Lq = 1, dk = 64, no dropout: the forward is the decode step's kernel)
            kern = K.decode_kernel(g, "f32" if dtype == F32 else "bf16")
        fam = kern + (f" + {bwd}" if bwd else "") + f" dk={g.dk}"
        compare(Launch(g, dtype, probs=probs, backward=bwd is not None).run(), K.ref_of(g), fam, fm, bm)


@gpu
def test_head_size_128_backward_is_rejected():
    """dk = 128 at Lq = Lk = 64: the backward's LDS need (168 KB) is over the budget; the hook returns the
    launcher's error before it launches anything (o and probs untouched too); forward alone, the case runs"""
    from capgen import _lib
    g = K.packed_case(F32, 128, 2, 64, "valid", B=2)
    run = Launch(g, F32, probs=True, backward=True)
    rc = getattr(_lib.load(), "capgen_debug_attention_geom")(*run.args())
    torch.cuda.synchronize()
    assert rc != 0
    assert b"LDS budget" in _lib.load().capgen_last_error()
    for gb in list(run.grads.values()) + [run.o, run.probs]:
        assert (gb == SENT).all(), "the rejected call wrote"
    r = K.ref_of(g)  # (the forward fits: 115 KB)
    run = Launch(g, F32, probs=True, backward=False).run()
    check(run.out("o"), r["o"], K.k_of(r["noise"]["o"]), False, None, "dk=128 L=64 o", "attn_fwd_kernel<float> dk=128")


# ---- C. attention_head_mean -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("Lk", [19, 36])
@pytest.mark.parametrize("Lq", [1, 5])
def test_head_mean(Lq, Lk):
    B, H = 3, 8
    probs = torch.softmax(torch.randn(B, H, Lq, Lk, generator=gen(Lq * 100 + Lk)), -1)
    pd = probs.to(DEV)
    for row in sorted({0, Lq - 1}):
        out = torch.full((B * Lk + 8,), SENT, device=DEV)
        call("capgen_debug_attention_head_mean", P(pd), B, H, Lq, Lk, row, P(out), None)
        check(out.cpu()[:B * Lk].view(B, Lk), R.head_mean_ref(probs, row), 1.0, False, None,
              f"head_mean Lq={Lq} Lk={Lk} row={row} out", "head_mean_kernel")
        assert (out[B * Lk:] == SENT).all()


# ---- D. the fused fronts with dropout ---------------------------------------------------------------------
FH, FD, FRONT_DROPS = K.FH, K.FD, K.FRONT_DROPS


def drop_c(drop):
    return C.c_float(drop[0]), drop[1], C.c_uint64(drop[2])


def front_compare(g, o, fam, tag, dout=None, grads=None, r=None):
    """the front's attention half against the restatement on the q / k / v the launch itself produced"""
    r = r or R.attention_ref(g, dout)
    r["noise"] = K.f32_noise(g, r, dout)
    R.check_conditions(g, r, tiles=(g.Lq == 64 and g.Lk == 64))
    ex = R.mfma_extra(r)
    if o is not None:
        got = o.cpu().flatten()[R.index(0, g.o_ld, g.o_bs, g.B, g.H, g.Lq, 64)]
        check(got, r["o"], K.k_of(r["noise"]["o"]), True, ex["o"], f"{tag} o", fam)
    for t, gt in (grads or {}).items():
        n = t[1]
        L = g.Lq if n == "q" else g.Lk
        idx = R.index(getattr(g, n + "_off"), getattr(g, n + "_ld"), getattr(g, n + "_bs"), g.B, g.H, L, 64)
        check(gt.cpu().flatten()[idx], r[t], K.k_of(r["noise"][t]), True, ex[t], f"{tag} {t}", fam)
    return r


@gpu
@pytest.mark.parametrize("drop", FRONT_DROPS, ids=["p0.1", "p0.5"])
@pytest.mark.parametrize("L,mask", K.QKV_FRONT)
def test_qkv_front_with_dropout(L, mask, drop):
    B = K.FRONT_B
    X, W, mk = K.qkv_front_inputs(L, mask)
    valid, ids = mk.get("key_valid"), mk.get("key_ids")
    Xd, Wd = X.to(DEV), W.to(DEV)
    qkv = torch.full((B * L + 1, 3 * FD), SENT, device=DEV, dtype=torch.bfloat16)
    o = torch.full((B * L + 1, FD), SENT, device=DEV, dtype=torch.bfloat16)
    vd, idd = (None if t is None else t.to(DEV) for t in (valid, ids))
    call("capgen_debug_qkv_attention", B, L, FH, P(Xd), P(Wd), P(qkv), P(o), P(vd), P(idd), K.PAD, 1, *drop_c(drop),
         None)
    got = qkv.cpu()
    ref = X.double() @ W.double().t()
    # each element the bf16 rounding of the product or its neighbour (the relation of the older front test)
    assert ((got[:B * L].double() - ref).abs() <= (ref.abs() * 2.0 ** -7).clamp_min(1e-5)).all()
    assert (got[B * L:] == SENT).all() and (o[B * L:] == SENT).all()
    g = K.qkv_front_geom(L, got[:B * L].contiguous(), mk, drop)
    front_compare(g, o[:B * L], "qkv_attn_kernel<*, 3> (self front)", f"qkv_front L={L} {mask} p={drop[0]}")


@gpu
@pytest.mark.parametrize("drop", FRONT_DROPS, ids=["p0.1", "p0.5"])
def test_cross_front_with_dropout(drop):
    B, Lq, Lk = K.FRONT_B, 19, 36
    X, Wq, KV, valid = K.cross_front_inputs(Lq, Lk)
    q = torch.full((B * Lq + 1, FD), SENT, device=DEV, dtype=torch.bfloat16)
    o = torch.full((B * Lq + 1, FD), SENT, device=DEV, dtype=torch.bfloat16)
    Xd, Wd, KVd, vd = (t.to(DEV) for t in (X, Wq, KV, valid))
    call("capgen_debug_cross_attention", B, Lq, Lk, FH, P(Xd), P(Wd), P(KVd), P(q), P(o), P(vd), *drop_c(drop), None)
    ref = X.double() @ Wq.double().t()
    got = q.cpu()
    assert ((got[:B * Lq].double() - ref).abs() <= (ref.abs() * 2.0 ** -7).clamp_min(1e-5)).all()
    assert (got[B * Lq:] == SENT).all() and (o[B * Lq:] == SENT).all()
    g = K.cross_front_geom(Lq, Lk, got[:B * Lq].contiguous(), KV, valid, drop)
    front_compare(g, o[:B * Lq], "qkv_attn_kernel<*, 1> (cross front)", f"cross_front p={drop[0]}")


@gpu
@pytest.mark.parametrize("drop", FRONT_DROPS, ids=["p0.1", "p0.5"])
@pytest.mark.parametrize("Lq,Lk,mask", K.BWD_WO)
def test_bwd_wo_front_with_dropout(Lq, Lk, mask, drop):
    """qkv_attn_bwd with dropout against the restatement, and against the pair it replaces (the input-gradient
    GEMM, then attention_bwd) with the same site and seed under the relation of
    test_fused_attention_bwd_wo_vs_separate: within 2e-2 of the tensor's max"""
    B = K.FRONT_B
    q, k, v, dA, Wo, valid = K.bwd_wo_inputs(Lq, Lk, mask)
    causal = int(mask == "causal")
    qd, kd, vd, dAd, Wod = (t.to(DEV) for t in (q, k, v, dA, Wo))
    vald = None if valid is None else valid.to(DEV)
    fused = [torch.full((B * L + 1, FD), SENT, device=DEV, dtype=torch.bfloat16) for L in (Lq, Lk, Lk)]
    call("capgen_debug_attention_bwd_wo", B, Lq, Lk, FH, P(qd), P(kd), P(vd), P(vald), causal, P(dAd), P(Wod),
         *(P(t) for t in fused), *drop_c(drop), None)
    for t, L in zip(fused, (Lq, Lk, Lk)):
        assert (t[B * L:] == SENT).all()
    g = K.bwd_wo_geom(Lq, Lk, q, k, v, valid, mask, drop)
    dO = (dA.double() @ Wo.double()).to(torch.bfloat16)  # as the launch stores it in its LDS image
    r = R.attention_ref(g, dO)
    fam = "qkv_attn_bwd_kernel (output-side front)"
    front_compare(g, None, fam, f"bwd_wo Lq={Lq} Lk={Lk} {mask} p={drop[0]}", dout=dO,
                  grads={"dq": fused[0][:B * Lq], "dk": fused[1][:B * Lk], "dv": fused[2][:B * Lk]},
                  r=r)
    # the separate pair, same site and seed
    dOd = torch.empty(B * Lq, FD, device=DEV, dtype=torch.bfloat16)
    call("capgen_debug_gemm", B * Lq, FD, FD, P(dAd), FD, 0, P(Wod), FD, 1, P(dOd), FD, 1, 1, None, C.c_float(1.0), 0, 0,
         None)
    g.extra["o_numel"] = B * Lq * FD
    g.extra["dout"] = dOd.cpu()
    run = Launch(g, BF16, probs=False, backward=True).run()
    for t, a1 in zip(("dq", "dk", "dv"), fused):
        L = Lq if t == "dq" else Lk
        a0 = run.out(t).double()
        a1 = a1.cpu()[:B * L].double().view(B, L, FH, 64).transpose(1, 2)
        assert (a1 - a0).abs().max().item() / (r[t].abs().max().item() + 1e-12) < 2e-2, t
