"""CPU: the float64 attention restatement (attention_ref.py) against torch.autograd in double, feature by
feature, and the conditions every case of test_gpu_attention.py must meet on the reference (live
keys, smallest live probability, dropped share, mixed 16 x 16 dropout blocks, float32 noise), so that a
bad choice of inputs fails here and not on the card.  The cases themselves are defined here; the GPU
module imports them."""

import numpy as np
import pytest
import torch

import attention_ref as R
from attention_ref import Geom
from test_gpu_rowops import SEEDS, gen

F32, BF16 = 0, 1
TDT = {F32: torch.float32, BF16: torch.bfloat16}
POISON = 1e4     # finite: a read of a slot the geometry must not read breaks the bound, nothing can fault
PAD = 2
# dtype modes: f32; bf16 with every stride a multiple of 8; bf16 with o_bs = H*64 + 4 (the decode step then
# takes the generic kernels attn_decode_kernel<bf16> / attn_decode_group_kernel<bf16>)
MODES = {"f32": F32, "bf16": BF16, "bf16u": BF16}


def randn(g, *shape):
    return torch.randn(*shape, generator=g) * 0.5


def site_of(layer):
    """an attention site id as the engine numbers them"""
    return (64 + layer) * 16 + 5


DROPS = [(0.0, 0, 0), (0.1, site_of(0), SEEDS[0]), (0.5, site_of(3), SEEDS[2])]


def with_drop(g, drop):
    g.drop_p, g.drop_site, g.drop_seed = drop
    return g


# ---- A. the decode step ---------------------------------------------------------------------------------
DEC_LKS = [1, 2, 24, 25, 32, 33, 40, 41, 63, 64]  # both sides of LKM 32 / 64 and NIT 3 / 5 / 8
DEC_RH = [(5, 8), (3, 3)]                         # (3, 3): B * H % 4 != 0
CROSS_GN = [(1, 36), (2, 32), (4, 33), (5, 24), (8, 64), (9, 5), (16, 41), (17, 36)]
CROSS_BIMG = 3


def out_layout(g, mode, rows_per_batch=1):
    """o wider and longer than the geometry: 8 (bf16u: 4) spare columns per batch, one spare batch"""
    d = g.H * g.dk
    g.o_ld = d + (4 if mode == "bf16u" else 8)
    g.o_bs = g.o_ld * rows_per_batch
    g.extra["o_numel"] = (g.B + 1) * g.o_bs
    return g


def dec_self_case(mode, R_, H, Lk, table):
    """dec_step's self attention at step t = Lk - 1: cache [R][Tc][2*dd] (k | v), key ids [R][Tc] with pad
    keys (never key 0), causal with q_pos0 = t, and the beam row table kv_row [R][Tc] (absolute rows)."""
    dt = TDT[MODES[mode]]
    dd, t, Tc = H * 64, Lk - 1, Lk + 2
    gg = gen(100000 + 1000 * Lk + 10 * R_ + H + (5 if table else 0))
    cache = randn(gg, R_, Tc, 2 * dd)
    ids = torch.randint(3, 50, (R_, Tc), generator=gg, dtype=torch.int32)
    for r in range(R_):
        for j in range(1, Lk):
            if (3 * j + r) % 7 == 0:
                ids[r, j] = PAD
    rows = None
    if table:
        rows = torch.randint(0, R_, (R_, Tc), generator=gg, dtype=torch.int32)
        named = torch.zeros(R_, Tc, dtype=torch.bool)
        named[rows[:, :Lk].long(), torch.arange(Lk).expand(R_, Lk)] = True
        cache[~named] = POISON          # rows no kv_row entry names
    cache[:, Lk:] = POISON              # positions > t
    q = randn(gg, R_, dd)
    g = Geom(B=R_, H=H, Lq=1, Lk=Lk, dk=64, q=q.to(dt), q_ld=dd, q_bs=dd,
             k=cache.to(dt), k_off=0, k_ld=2 * dd, k_bs=Tc * 2 * dd, kv_row=rows, kv_row_ld=Tc,
             key_ids=ids, kid_bs=Tc, pad_idx=PAD, causal=1, q_pos0=t, temperature=8.0)
    g.v, g.v_off, g.v_ld, g.v_bs = g.k, dd, g.k_ld, g.k_bs
    g.extra["tag"] = f"dec_self {mode} R={R_} H={H} Lk={Lk} table={int(table)}"
    return out_layout(g, mode)


def dec_cross_case(mode, Rq, N, Bimg=CROSS_BIMG):
    """dec_step's cross attention: rows r attend over image r % Bimg; K / V of layer 1 of a 2-layer slab
    [Bimg][N + 1][2*2*dd] (the other layer's columns and the key row behind the last are poison)."""
    dt = TDT[MODES[mode]]
    H, dd = 8, 512
    gg = gen(200000 + 100 * Rq + N)
    slab = torch.full((Bimg, N + 1, 4 * dd), POISON)
    slab[:, :N, 2 * dd:] = randn(gg, Bimg, N, 2 * dd)
    valid = torch.ones(Bimg, N, dtype=torch.uint8)
    for b in range(Bimg):
        for j in range(1, N):
            if (5 * j + b) % 11 == 3:
                valid[b, j] = 0
    q = randn(gg, Rq, dd)
    g = Geom(B=Rq, H=H, Lq=1, Lk=N, dk=64, q=q.to(dt), q_ld=dd, q_bs=dd,
             k=slab.to(dt), k_off=2 * dd, k_ld=4 * dd, k_bs=(N + 1) * 4 * dd, kv_bmod=Bimg,
             key_valid=valid, kv_bs=N, temperature=8.0)
    g.v, g.v_off, g.v_ld, g.v_bs = g.k, 3 * dd, g.k_ld, g.k_bs
    g.extra["tag"] = f"dec_cross {mode} R={Rq} Bimg={Bimg} N={N}"
    return out_layout(g, mode)


def dec_cases(mode):
    for R_, H in DEC_RH:
        for table in (False, True):
            for Lk in DEC_LKS:
                yield dec_self_case(mode, R_, H, Lk, table)
    for G, N in CROSS_GN:
        yield dec_cross_case(mode, G * CROSS_BIMG, N)
    yield dec_cross_case(mode, 7, 36)  # R % Bimg != 0: no grouping


def decode_kernel(g, mode, lds=1):
    """the instantiation launch_decode (attention.hip) picks, restated from its conditions"""
    G = g.B // g.kv_bmod if g.kv_bmod > 0 else 1
    grouped = (2 <= G <= 16 and g.B % g.kv_bmod == 0 and g.kv_row is None and not g.causal
               and g.key_ids is None)
    T = "float" if mode == "f32" else "bf16"
    if mode == "bf16":
        assert all(x % 8 == 0 for x in (g.q_bs, g.k_bs, g.v_bs, g.k_ld, g.v_ld, g.o_bs))
        nit = 3 if g.Lk <= 24 else 5 if g.Lk <= 40 else 8
        how = ("group+lds" if lds else "group") if grouped else "single"
        return f"attn_decode_bf16_kernel<{nit}> {how}"
    if mode == "bf16u":
        assert g.o_bs % 8 != 0
    lkm = 32 if g.Lk <= 32 else 64
    if grouped:
        return f"attn_decode_group_kernel<{T}, {lkm}, {4 if G <= 4 else 8 if G <= 8 else 16}>"
    return f"attn_decode_kernel<{T}, {lkm}>"


DECODE_INSTANTIATIONS = sorted(
    [f"attn_decode_kernel<{T}, {l}>" for T in ("float", "bf16") for l in (32, 64)]
    + [f"attn_decode_group_kernel<{T}, {l}, {gm}>" for T in ("float", "bf16") for l in (32, 64) for gm in (4, 8, 16)]
    + [f"attn_decode_bf16_kernel<{n}> {how}" for n in (3, 5, 8) for how in ("single", "group", "group+lds")])


# ---- B. the full kernels (Lq > 1, or dropout) ----------------------------------------------------------
# (dtype, dk, H): f32 VALU at head sizes 8 / 32 / 64, bf16 VALU at 32, bf16 MFMA at 64
KERNELS = [(F32, 8, 3), (F32, 32, 3), (F32, 64, 3), (BF16, 32, 3), (BF16, 64, 3)]
FB = 3  # batches


def key_mask_bytes(B, Lk):
    valid = torch.ones(B, Lk, dtype=torch.uint8)
    for b in range(B):
        valid[b, max(1, Lk - 3 * b - 2):] = 0
        if Lk > 4:
            valid[b, 2 + b] = 0  # (and one masked key in the middle: never key 0)
    return valid


def key_mask_ids(g_, B, Lk):
    ids = torch.randint(3, 100, (B, Lk), generator=g_, dtype=torch.int32)
    for b in range(B):
        ids[b, max(1, Lk - 2 * b - 1):] = PAD
        if Lk > 4:
            ids[b, 1 + b] = PAD
    return ids


def full_out(g):
    """o / dO: 8 spare columns per row, one spare row per batch, one spare batch"""
    g.o_ld = g.H * g.dk + 8
    g.o_bs = (g.Lq + 1) * g.o_ld
    g.extra["o_numel"] = (g.B + 1) * g.o_bs
    return g


def packed_case(dtype, dk, H, L, mask, B=FB):
    """a training self-attention site: one buffer [B][L + 1][3*d] (q | k | v, ld = 3*d; a spare row per batch
    and a spare batch), key_valid + causal (encoder with encode_mask) or key_ids + causal (decoder)."""
    d = H * dk
    gg = gen(300000 + 1000 * L + 10 * dk + dtype + (3 if mask == "ids" else 0))
    qkv = randn(gg, B + 1, L + 1, 3 * d).to(TDT[dtype])
    g = Geom(B=B, H=H, Lq=L, Lk=L, dk=dk, q=qkv, q_off=0, q_ld=3 * d, q_bs=(L + 1) * 3 * d,
             k=qkv, k_off=d, k_ld=3 * d, k_bs=(L + 1) * 3 * d, v=qkv, v_off=2 * d, v_ld=3 * d,
             v_bs=(L + 1) * 3 * d, causal=1, temperature=float(np.sqrt(dk)))
    if mask == "valid":
        g.key_valid, g.kv_bs = key_mask_bytes(B, L), L
    else:
        g.key_ids, g.kid_bs, g.pad_idx = key_mask_ids(gg, B, L), L, PAD
    g.extra["tag"] = f"packed_{mask} dtype={dtype} dk={dk} L={L}"
    g.extra["dout"] = randn(gg, (B + 1) * (L + 1) * (d + 8)).to(TDT[dtype])
    return full_out(g)


def cross_case(dtype, dk, H, Lq, Lk, causal=0, q_pos0=0, B=FB):
    """a training cross-attention site: dense q [B][Lq][d], K / V of layer 1 of the slab [B][Lk + 1][2*2*d]
    (the other layer and the spare key row are poison), key_valid"""
    d = H * dk
    gg = gen(400000 + 1000 * Lq + 10 * Lk + dk + dtype + q_pos0)
    slab = torch.full((B + 1, Lk + 1, 4 * d), POISON)
    slab[:B, :Lk, 2 * d:] = randn(gg, B, Lk, 2 * d)
    q = randn(gg, B + 1, Lq, d)
    g = Geom(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, q=q.to(TDT[dtype]), q_ld=d, q_bs=Lq * d,
             k=slab.to(TDT[dtype]), k_off=2 * d, k_ld=4 * d, k_bs=(Lk + 1) * 4 * d,
             key_valid=key_mask_bytes(B, Lk), kv_bs=Lk, causal=causal, q_pos0=q_pos0,
             temperature=float(np.sqrt(dk)))
    g.v, g.v_off, g.v_ld, g.v_bs = g.k, 3 * d, g.k_ld, g.k_bs
    g.extra["tag"] = f"cross dtype={dtype} dk={dk} Lq={Lq} Lk={Lk} causal={causal} q_pos0={q_pos0}"
    g.extra["dout"] = randn(gg, (B + 1) * (Lq + 1) * (d + 8)).to(TDT[dtype])
    return full_out(g)


def beam_block_case(dtype, kb, Lk=36, Bimg=3, H=8):
    """the beam's cross attention with an image's kb rows as one query block: q / o rows Bimg*dd apart,
    images dd apart (q_ld = Bimg*dd, q_bs = dd).  o: one spare image column per row, one spare row."""
    dd = H * 64
    gg = gen(500000 + 100 * kb + Lk + dtype)
    slab = torch.full((Bimg, Lk + 1, 4 * dd), POISON)
    slab[:, :Lk, 2 * dd:] = randn(gg, Bimg, Lk, 2 * dd)
    q = randn(gg, kb + 1, Bimg, dd)  # (a spare row: dq's guard)
    g = Geom(B=Bimg, H=H, Lq=kb, Lk=Lk, dk=64, q=q.to(TDT[dtype]), q_ld=Bimg * dd, q_bs=dd,
             k=slab.to(TDT[dtype]), k_off=2 * dd, k_ld=4 * dd, k_bs=(Lk + 1) * 4 * dd,
             key_valid=key_mask_bytes(Bimg, Lk), kv_bs=Lk, temperature=8.0)
    g.v, g.v_off, g.v_ld, g.v_bs = g.k, 3 * dd, g.k_ld, g.k_bs
    g.o_ld, g.o_bs = (Bimg + 1) * dd, dd
    g.extra["o_numel"] = (kb + 1) * g.o_ld
    g.extra["tag"] = f"beam_block dtype={dtype} kb={kb} Lk={Lk}"
    g.extra["dout"] = randn(gg, g.extra["o_numel"]).to(TDT[dtype])
    return g


def kv_row_full_case(dtype, dk=64, H=3, Lq=5, Lk=19, B=4):
    """kv_row with Lq > 1 (forward only: the VALU kernel's row map): cache [B][Lk + 1][2*d], key j of batch b
    in row kv_row[b][j]; causal with q_pos0 = Lk - Lq; slots no entry names are poison"""
    d = H * dk
    gg = gen(600000 + dtype)
    cache = randn(gg, B, Lk + 1, 2 * d)
    rows = torch.randint(0, B, (B, Lk + 1), generator=gg, dtype=torch.int32)
    named = torch.zeros(B, Lk + 1, dtype=torch.bool)
    named[rows[:, :Lk].long(), torch.arange(Lk).expand(B, Lk)] = True
    cache[~named] = POISON
    q = randn(gg, B, Lq, d)
    g = Geom(B=B, H=H, Lq=Lq, Lk=Lk, dk=dk, q=q.to(TDT[dtype]), q_ld=d, q_bs=Lq * d,
             k=cache.to(TDT[dtype]), k_off=0, k_ld=2 * d, k_bs=(Lk + 1) * 2 * d, kv_row=rows, kv_row_ld=Lk + 1,
             key_ids=key_mask_ids(gg, B, Lk), kid_bs=Lk, pad_idx=PAD, causal=1, q_pos0=Lk - Lq,
             temperature=float(np.sqrt(dk)))
    g.v, g.v_off, g.v_ld, g.v_bs = g.k, d, g.k_ld, g.k_bs
    g.extra["tag"] = f"kv_row_full dtype={dtype}"
    g.extra["fwd_only"] = True
    return full_out(g)


PACKED_L = {"valid": [36, 19, 64, 1], "ids": [36, 19, 64]}
CROSS_L = [(19, 36), (33, 17), (17, 64), (36, 36)]


def full_geoms(dtype, dk, H):
    """the layouts x (Lq, Lk) of one kernel family (dropout off; with_drop switches it on)"""
    for mask, Ls in PACKED_L.items():
        for L in Ls:
            yield packed_case(dtype, dk, H, L, mask)
    for Lq, Lk in CROSS_L:
        yield cross_case(dtype, dk, H, Lq, Lk)
    yield cross_case(dtype, dk, H, 19, 36, causal=1, q_pos0=3)
    if dk == 64:
        for kb in (2, 5, 16, 17):
            yield beam_block_case(dtype, kb)
        yield kv_row_full_case(dtype)


def full_cases(dtype, dk, H):
    for di, drop in enumerate(DROPS):
        for g in full_geoms(dtype, dk, H):
            if drop[0] > 0 and g.extra.get("fwd_only"):
                continue
            g.extra["tag"] += f" p={drop[0]}"
            yield with_drop(g, drop)
    if dtype == F32 and dk == 64:  # head size 128 at L = 48 (the backward's LDS: 117 KB)
        for drop in DROPS:
            g = packed_case(F32, 128, 2, 48, "valid")
            g.extra["tag"] += f" p={drop[0]}"
            yield with_drop(g, drop)


def full_kernel(g, dtype):
    """the forward kernel attention_fwd picks, restated from its conditions"""
    if g.Lq == 1 and g.dk == 64 and not g.drop_p > 0:
        return "decode"
    strides = (g.q_ld, g.k_ld, g.v_ld, g.o_ld, g.q_bs, g.k_bs, g.v_bs, g.o_bs)
    if dtype == BF16 and g.kv_row is None and g.dk == 64 and all(x % 8 == 0 for x in strides):
        return "attn_fwd_wave_kernel" if g.Lq <= 16 else "attn_fwd_mfma_kernel"
    return f"attn_fwd_kernel<{'float' if dtype == F32 else 'bf16'}>"


def bwd_kernel(g, dtype):
    """the backward kernel attention_bwd picks"""
    strides = (g.q_ld, g.k_ld, g.v_ld, g.o_ld, g.q_bs, g.k_bs, g.v_bs, g.o_bs)
    if dtype == BF16 and g.dk == 64 and all(x % 8 == 0 for x in strides):
        return "attn_bwd_mfma_kernel"
    return f"attn_bwd_kernel<{'float' if dtype == F32 else 'bf16'}>"


# ---- D. the fused fronts (bf16, H = 8, d = 512) with dropout ---------------------------------------------
FH, FD, FRONT_B = 8, 512, 3
FRONT_DROPS = [(0.1, site_of(1), SEEDS[0]), (0.5, site_of(2), SEEDS[1])]
QKV_FRONT = [(L, mask) for L in (19, 36, 64) for mask in ("valid_causal", "ids_causal")]
BWD_WO = [(19, 36, "valid"), (64, 64, "causal")]


def front_geom(B, Lq, Lk, q, k, v, strides, drop, **mask):
    (q_off, q_ld), (k_off, k_ld), (v_off, v_ld) = strides
    g = Geom(B=B, H=FH, Lq=Lq, Lk=Lk, dk=64, q=q, q_off=q_off, q_ld=q_ld, q_bs=Lq * q_ld, k=k, k_off=k_off,
             k_ld=k_ld, k_bs=Lk * k_ld, v=v, v_off=v_off, v_ld=v_ld, v_bs=Lk * v_ld, o_ld=FD, o_bs=Lq * FD,
             temperature=8.0, **mask)
    return with_drop(g, drop)


def qkv_front_inputs(L, mask):
    """X [B*L, 512], W [1536, 512] bf16 and the key mask of the self front"""
    B = FRONT_B
    gg = gen(B * 131 + L)
    X = randn(gg, B * L, FD).to(torch.bfloat16)
    W = (torch.randn(3 * FD, FD, generator=gg) / FD ** 0.5).to(torch.bfloat16)
    mk = dict(key_valid=key_mask_bytes(B, L), kv_bs=L) if mask == "valid_causal" else \
        dict(key_ids=key_mask_ids(gg, B, L), kid_bs=L, pad_idx=PAD)
    return X, W, mk


def qkv_front_geom(L, qkv, mk, drop):
    """the attention the self front runs on the qkv [B*L, 1536] it projected"""
    return front_geom(FRONT_B, L, L, qkv, qkv, qkv, ((0, 3 * FD), (FD, 3 * FD), (2 * FD, 3 * FD)), drop, causal=1, **mk)


def cross_front_inputs(Lq=19, Lk=36):
    B = FRONT_B
    gg = gen(77)
    X = randn(gg, B * Lq, FD).to(torch.bfloat16)
    Wq = (torch.randn(FD, FD, generator=gg) / FD ** 0.5).to(torch.bfloat16)
    KV = randn(gg, B * Lk, 2 * FD).to(torch.bfloat16)
    return X, Wq, KV, key_mask_bytes(B, Lk)


def cross_front_geom(Lq, Lk, q, KV, valid, drop):
    return front_geom(FRONT_B, Lq, Lk, q, KV, KV, ((0, FD), (0, 2 * FD), (FD, 2 * FD)), drop, key_valid=valid, kv_bs=Lk)


def bwd_wo_inputs(Lq, Lk, mask):
    B = FRONT_B
    gg = gen(B * 7 + Lq * 3 + Lk)
    q, k, v = (randn(gg, B * L, FD).to(torch.bfloat16) for L in (Lq, Lk, Lk))
    dA = randn(gg, B * Lq, FD).to(torch.bfloat16)
    Wo = (torch.randn(FD, FD, generator=gg) / FD ** 0.5).to(torch.bfloat16)
    return q, k, v, dA, Wo, (key_mask_bytes(B, Lk) if mask == "valid" else None)


def bwd_wo_geom(Lq, Lk, q, k, v, valid, mask, drop):
    mk = dict(key_valid=valid, kv_bs=Lk) if valid is not None else {}
    return front_geom(FRONT_B, Lq, Lk, q, k, v, ((0, FD), (0, FD), (0, FD)), drop, causal=int(mask == "causal"), **mk)


# ---- float32's own noise: the restatement once in float32 against float64 ----------------------------
TENSORS = ("probs", "o", "dq", "dk", "dv")


def f32_noise(g, r64=None, dout=None):
    """{tensor: max|ref32 - ref64| / max|ref64|}"""
    r64 = r64 or R.attention_ref(g, dout)
    r32 = R.attention_ref(g, dout, dtype=torch.float32)
    out = {}
    for t in TENSORS:
        if r64.get(t) is not None:
            out[t] = ((r32[t].double() - r64[t]).abs().max() / r64[t].abs().max().clamp_min(1e-30)).item()
    return out


def k_of(noise):
    """the factor k of the bound k x 1e-5 x max|ref|: 1, or 8 x the float32 noise where that is larger (the
    kernels sum sequentially, the CPU pairwise); never above the 1e-4 the older test asserts"""
    k = max(1.0, 8 * noise / 1e-5)
    assert k <= 10.0, noise
    return k


def ref_of(g):
    r = R.attention_ref(g, g.extra.get("dout"))
    r["noise"] = f32_noise(g, r, g.extra.get("dout"))
    return r


# ======================================= the CPU tests ===================================================
def loop_gather(buf, off, ld, bs, batches, H, L, dk):
    """[B, H, L, dk] through Python loops and slices (not attention_ref.index); batches[b][i] = stored batch"""
    flat = buf.flatten()
    return torch.stack([torch.stack([torch.stack([
        flat[off + batches[b][i] * bs + i * ld + h * dk: off + batches[b][i] * bs + i * ld + h * dk + dk]
        for i in range(L)]) for h in range(H)]) for b in range(len(batches))])


def autograd_check(g, dout=None):
    """attention through torch ops and autograd on double leaves laid out as the geometry says, the masks
    as constant factors"""
    r = R.attention_ref(g, dout)
    B, H, Lq, Lk, dk = g.B, g.H, g.Lq, g.Lk, g.dk
    same = g.q is g.k
    qb = g.q.double().flatten().clone().requires_grad_(True)
    kb = qb if same else g.k.double().flatten().clone().requires_grad_(True)
    own = [[b] * max(Lq, Lk) for b in range(B)]
    if g.kv_row is not None:
        kvb = [[int(g.kv_row.flatten()[b * g.kv_row_ld + j]) for j in range(Lk)] for b in range(B)]
    elif g.kv_bmod:
        kvb = [[b % g.kv_bmod] * Lk for b in range(B)]
    else:
        kvb = own
    q = loop_gather(qb, g.q_off, g.q_ld, g.q_bs, own, H, Lq, dk)
    k = loop_gather(kb, g.k_off, g.k_ld, g.k_bs, kvb, H, Lk, dk)
    v = loop_gather(kb, g.v_off, g.v_ld, g.v_bs, kvb, H, Lk, dk)
    live = torch.ones(B, 1, Lq, Lk, dtype=torch.float64)
    for b in range(B):
        bk = b % g.kv_bmod if g.kv_bmod else b
        for i in range(Lq):
            for j in range(Lk):
                dead = bool(g.causal and j > g.q_pos0 + i)
                dead |= g.key_valid is not None and int(g.key_valid.flatten()[bk * g.kv_bs + j]) == 0
                dead |= g.key_ids is not None and int(g.key_ids.flatten()[b * g.kid_bs + j]) == g.pad_idx
                live[b, 0, i, j] = 0.0 if dead else 1.0
    s = (q / float(np.float32(g.temperature))) @ k.transpose(-1, -2)
    e = torch.exp(s - s.detach().max()) * live
    p = e / e.sum(-1, keepdim=True)
    keep, scale = R.keep_mask(g)
    o = (p if keep is None else p * keep.double() * scale) @ v
    assert torch.allclose(p, r["probs"], rtol=0, atol=1e-13)
    assert torch.allclose(o, r["o"], rtol=0, atol=1e-12)
    if dout is None:
        return r
    dO = loop_gather(dout.double(), 0, g.o_ld, g.o_bs, own, H, Lq, dk)
    (o * dO).sum().backward()
    gq = qb.grad[R.index(g.q_off, g.q_ld, g.q_bs, B, H, Lq, dk)]
    assert torch.allclose(gq, r["dq"], rtol=0, atol=1e-12)
    if r["dk"] is not None:
        gk = kb.grad[R.index(g.k_off, g.k_ld, g.k_bs, B, H, Lk, dk)]
        gv = kb.grad[R.index(g.v_off, g.v_ld, g.v_bs, B, H, Lk, dk)]
        assert torch.allclose(gk, r["dk"], rtol=0, atol=1e-12)
        assert torch.allclose(gv, r["dv"], rtol=0, atol=1e-12)
        # (and nothing outside the q / k / v elements carries a gradient)
        used = torch.zeros(qb.numel() if same else kb.numel(), dtype=torch.bool)
        used[R.index(g.k_off, g.k_ld, g.k_bs, B, H, Lk, dk).flatten()] = True
        used[R.index(g.v_off, g.v_ld, g.v_bs, B, H, Lk, dk).flatten()] = True
        if same:
            used[R.index(g.q_off, g.q_ld, g.q_bs, B, H, Lq, dk).flatten()] = True
        assert (kb.grad[~used] == 0).all()
    return r


def small_dout(g, seed=9):
    return randn(gen(seed), g.extra["o_numel"])


@pytest.mark.parametrize("feature", ["packed_valid", "packed_ids", "cross_strided", "q_pos0", "beam_block",
                                     "kv_bmod", "kv_row", "kv_row_full", "dropout_0.1", "dropout_0.5"])
def test_restatement_matches_autograd(feature):
    if feature == "packed_valid":
        g = packed_case(F32, 8, 2, 7, "valid", B=2)
    elif feature == "packed_ids":
        g = packed_case(F32, 8, 2, 7, "ids", B=2)
    elif feature == "cross_strided":
        g = cross_case(F32, 8, 2, 5, 9, B=2)
    elif feature == "q_pos0":
        g = cross_case(F32, 8, 2, 5, 9, causal=1, q_pos0=3, B=2)
    elif feature == "beam_block":
        g = beam_block_case(F32, 3, Lk=6, Bimg=2, H=1)
    elif feature == "kv_bmod":
        g = dec_cross_case("f32", 4, 5, Bimg=2)
    elif feature == "kv_row":
        g = dec_self_case("f32", 3, 1, 6, True)
    elif feature == "kv_row_full":
        g = kv_row_full_case(F32, dk=8, H=2, Lq=3, Lk=7, B=3)
    else:
        g = with_drop(packed_case(F32, 8, 2, 9, "valid", B=2), (float(feature[8:]), site_of(1), SEEDS[1]))
    r = autograd_check(g, small_dout(g))
    if feature.startswith("dropout"):
        assert r["keep"] is not None and (~r["keep"]).any() and r["keep"].any()
        assert (r["Pd"][~r["keep"]] == 0).all()
    if feature in ("kv_bmod", "kv_row", "kv_row_full"):
        assert r["dk"] is None and r["dv"] is None
    if feature == "q_pos0":
        assert not r["masked"][0, 0, 0, 3] and r["masked"][0, 0, 0, 4]


def test_poison_is_never_read_by_the_reference():
    """the slots a geometry must not read hold 1e4: the reference's own operands stay small"""
    for g in list(dec_cases("f32")) + list(full_geoms(F32, 64, 3)):
        r = R.attention_ref(g)
        assert r["k"].abs().max() < 10 and r["v"].abs().max() < 10 and r["q"].abs().max() < 10, g.extra["tag"]
        assert (g.k.float() == POISON).any() or g.q is g.k, g.extra["tag"]


@pytest.mark.parametrize("mode", sorted(MODES))
def test_decode_cases_meet_the_conditions(mode):
    reached = set()
    pmin, noise = 1.0, 0.0
    for g in dec_cases(mode):
        r = ref_of(g)
        p, _ = R.check_conditions(g, r)
        pmin = min(pmin, p)
        noise = max(noise, max(r["noise"].values()))
        for t, n in r["noise"].items():
            k_of(n)
        reached.add(decode_kernel(g, mode, 1))
        if mode == "bf16":
            reached.add(decode_kernel(g, mode, 0))
        if g.key_ids is not None and g.Lk >= 8:
            assert (g.key_ids.flatten().view(g.B, -1)[:, :g.Lk] == PAD).any()
    want = [k for k in DECODE_INSTANTIATIONS if ("bf16_kernel" in k) == (mode == "bf16")
            and ("<float" in k) == (mode == "f32")]
    assert sorted(reached) == want, sorted(reached)
    assert pmin >= 5e-3 and noise <= 1e-6, (pmin, noise)


@pytest.mark.parametrize("dtype,dk,H", KERNELS)
def test_full_cases_meet_the_conditions(dtype, dk, H):
    pmin, noise, kmax = 1.0, {}, 1.0
    kernels = set()
    for g in full_cases(dtype, dk, H):
        r = ref_of(g)
        p, share = R.check_conditions(g, r, tiles=(g.drop_p > 0 and g.Lq == 64 and g.Lk == 64))
        pmin = min(pmin, p)
        for t, n in r["noise"].items():
            noise[t] = max(noise.get(t, 0.0), n)
            kmax = max(kmax, k_of(n))
        kernels.add(full_kernel(g, dtype))
    want = {f"attn_fwd_kernel<{'float' if dtype == F32 else 'bf16'}>"}
    if dk == 64:
        want |= {"decode"}
        if dtype == BF16:
            want |= {"attn_fwd_wave_kernel", "attn_fwd_mfma_kernel"}
    assert kernels == want, kernels
    assert {bwd_kernel(g, dtype) for g in full_cases(dtype, dk, H)} == \
        {"attn_bwd_mfma_kernel" if (dtype, dk) == (BF16, 64) else f"attn_bwd_kernel<{'float' if dtype == F32 else 'bf16'}>"}
    assert pmin >= 2e-3, pmin
    print("f32 noise", dtype, dk, {t: f"{n:.2e}" for t, n in noise.items()}, "k max", kmax)


def front_conditions(g, dout=None):
    r = R.attention_ref(g, dout)
    for n in f32_noise(g, r, dout).values():
        k_of(n)
    return R.check_conditions(g, r, tiles=(g.Lq == 64 and g.Lk == 64))[0]


@pytest.mark.parametrize("drop", FRONT_DROPS, ids=["p0.1", "p0.5"])
def test_front_cases_meet_the_conditions(drop):
    """the fronts' attention on the CPU's own projection (the card's differs by a rounding here and there)"""
    pmin = 1.0
    for L, mask in QKV_FRONT:
        X, W, mk = qkv_front_inputs(L, mask)
        qkv = (X.double() @ W.double().t()).to(torch.bfloat16)
        pmin = min(pmin, front_conditions(qkv_front_geom(L, qkv, mk, drop)))
    X, Wq, KV, valid = cross_front_inputs()
    q = (X.double() @ Wq.double().t()).to(torch.bfloat16)
    pmin = min(pmin, front_conditions(cross_front_geom(19, 36, q, KV, valid, drop)))
    for Lq, Lk, mask in BWD_WO:
        q, k, v, dA, Wo, valid = bwd_wo_inputs(Lq, Lk, mask)
        pmin = min(pmin, front_conditions(bwd_wo_geom(Lq, Lk, q, k, v, valid, mask, drop), dA.double() @ Wo.double()))
    assert pmin >= 2e-3, pmin


def test_rejected_case_meets_the_conditions():
    g = packed_case(F32, 128, 2, 64, "valid", B=2)
    R.check_conditions(g, ref_of(g))


def test_hook_passes_the_struct():
    """no GPU, null pointers only: the hooks check the shape first, then the pointers, so each refusal shows
    that the struct's fields arrive (and nothing can be launched)"""
    import ctypes as C
    from capgen import _lib
    lib = _lib.load()
    N = None
    c = _lib.capgen_attn_geom()
    call = lambda: lib.capgen_debug_attention_geom(0, C.byref(c), N, N, N, N, N, N, N)
    assert call() != 0 and b"bad shape" in lib.capgen_last_error()
    c.B, c.H, c.Lq, c.Lk, c.dk = 1, 1, 65, 3, 64
    assert call() != 0 and b"bad shape" in lib.capgen_last_error()
    c.Lq, c.Lk = 3, 65
    assert call() != 0 and b"bad shape" in lib.capgen_last_error()
    c.Lk = 3
    assert call() != 0 and b"are required" in lib.capgen_last_error()
    assert lib.capgen_debug_attention_geom(0, N, N, N, N, N, N, N, N) != 0
    assert lib.capgen_debug_attention_head_mean(N, 1, 1, 2, 3, 2, N, N) != 0  # row >= Lq
    assert b"bad shape" in lib.capgen_last_error()
    assert lib.capgen_debug_attention_head_mean(N, 1, 1, 2, 3, 1, N, N) != 0
    assert b"are required" in lib.capgen_last_error()


def test_front_hooks_accept_the_former_arity():
    """no GPU: a call of a front hook without drop_p, drop_site, drop_seed reaches the library (which refuses
    the bad shape) and means dropout off; with them it does the same"""
    from capgen import _lib
    lib = _lib.load()
    N = None
    former = {"capgen_debug_qkv_attention": (0, 1, 8, N, N, N, N, N, N, 0, 1),           # B = 0
              "capgen_debug_cross_attention": (0, 1, 1, 8, N, N, N, N, N, N),
              "capgen_debug_attention_bwd_wo": (1, 1, 1, 1, N, N, N, N, 0, N, N, N, N, N)}  # H * 64 != 512
    assert sorted(former) == sorted(_lib._DROP_HOOKS)
    for name, args in former.items():
        fn = getattr(lib, name)
        assert fn(*args, None) != 0 and b"bad shape" in lib.capgen_last_error(), name
        assert fn(*args, 0.0, 0, 0, None) != 0 and b"bad shape" in lib.capgen_last_error(), name
        with pytest.raises(TypeError):
            fn(*args)


def test_head_size_128_backward_is_over_the_lds_budget():
    """bwd_smem (attention.hip) at dk = 128, Lq = Lk = 64 is 168 KB > 160 KB; at L = 48 it fits"""
    def bwd_smem(Lq, Lk, dk):
        ldd, Lq2, Lk2 = dk + 4, (Lq + 1) & ~1, (Lk + 1) & ~1
        return 4 * (2 * Lq2 * ldd + 2 * Lk2 * ldd + 2 * Lq * (Lk + 1))
    assert bwd_smem(64, 64, 128) == 168448 > 160 * 1024
    assert bwd_smem(48, 48, 128) <= 160 * 1024


def test_head_mean_restatement():
    p = torch.rand(3, 8, 5, 19, generator=gen(3))
    out = R.head_mean_ref(p, 4)
    want = sum(p[:, h, 4, :].double() for h in range(8)) / 8
    assert torch.allclose(out, want, rtol=0, atol=1e-15) and out.shape == (3, 19)


def test_geom_struct_mirrors_the_header():
    """capgen_attn_geom (ctypes) has the fields of capgen_attn_geom_t, in the header's order"""
    import os
    import re
    from capgen import _lib
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "capgen.h")).read()
    body = re.search(r"typedef struct capgen_attn_geom \{(.*?)\} capgen_attn_geom_t;", src, re.S).group(1)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*").strip() for n in re.sub(r"^(const\s+)?(unsigned\s+)?\w+\s*\*?", "", decl).split(",")]
    assert names == [f[0] for f in _lib.capgen_attn_geom._fields_]
    assert set(names) >= {f for f in Geom.__dataclass_fields__ if not f.endswith("_off") and f != "extra"}
