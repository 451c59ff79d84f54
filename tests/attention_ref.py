"""Masked multi-head attention, forward and backward, restated in float64 on CPU tensors from the
comments of csrc/attention.h and modules.py:16-27 (s = (q / temperature) . k^T; masked_fill(-inf);
softmax; dropout; o = p . v) -- never the library.  It takes the geometry the hook
capgen_debug_attention_geom takes, field by field:

  row (b, i) of head h of q / k / v / o lives at  base + b*bs + i*ld + h*dk  of a flat buffer;
  kv_bmod > 0: K / V / key_valid of query batch b come from batch b % kv_bmod;
  kv_row: key j of query batch b is stored in batch kv_row[b*kv_row_ld + j] (an absolute cache row);
  key (b, j) is masked if key_valid[bk*kv_bs + j] == 0, or key_ids[b*kid_bs + j] == pad_idx,
  or causal and j > q_pos0 + i;
  dropout keeps element idx = ((b*H + h)*Lq + i)*Lk + j of the probabilities (drop_keep of
  test_gpu_rowops.py, the counter RNG of capgen_common.h) and scales it by 1 / (1 - p).

The backward is written out as attn_bwd_kernel's comments state it: d(p_dropped) = dO . V^T, through the
same dropout, dS = p (dP - rowsum(p dP)) (softmax backward), dq = (dS . K) / temperature,
dk = dS^T . (q / temperature), dv = Pd^T . dO.
"""
from dataclasses import dataclass, field

import numpy as np
import torch

from test_gpu_rowops import drop_keep


@dataclass
class Geom:
    B: int
    H: int
    Lq: int
    Lk: int
    dk: int
    q: torch.Tensor = None       # flat buffers (any dtype), with the element offset of (b=0, i=0, h=0)
    q_off: int = 0
    q_ld: int = 0
    q_bs: int = 0
    k: torch.Tensor = None
    k_off: int = 0
    k_ld: int = 0
    k_bs: int = 0
    v: torch.Tensor = None
    v_off: int = 0
    v_ld: int = 0
    v_bs: int = 0
    o_ld: int = 0
    o_bs: int = 0
    kv_bmod: int = 0
    kv_row: torch.Tensor = None  # int32, flat
    kv_row_ld: int = 0
    key_valid: torch.Tensor = None  # uint8, flat
    kv_bs: int = 0
    key_ids: torch.Tensor = None    # int32, flat
    kid_bs: int = 0
    pad_idx: int = 0
    causal: int = 0
    q_pos0: int = 0
    temperature: float = 1.0
    drop_p: float = 0.0
    drop_site: int = 0
    drop_seed: int = 0
    extra: dict = field(default_factory=dict)  # (the tests' own notes: tag, output buffers, ...)


def index(off, ld, bs, B, H, L, dk, batch_of=None):
    """flat element index [B, H, L, dk] of row (b, i), head h, column d; batch_of [B, L]: the stored batch"""
    b = torch.arange(B).view(B, 1, 1, 1) if batch_of is None else batch_of.long().view(B, 1, L, 1)
    h = torch.arange(H).view(1, H, 1, 1)
    i = torch.arange(L).view(1, 1, L, 1)
    d = torch.arange(dk).view(1, 1, 1, dk)
    return off + b * bs + i * ld + h * dk + d


def kv_batch(g):
    """[B, Lk]: the batch of the K / V buffer that holds key j of query batch b"""
    if g.kv_row is not None:
        b = torch.arange(g.B).view(g.B, 1)
        j = torch.arange(g.Lk).view(1, g.Lk)
        return g.kv_row.flatten().long()[b * g.kv_row_ld + j]
    b = torch.arange(g.B)
    if g.kv_bmod:
        b = b % g.kv_bmod
    return b.view(g.B, 1).expand(g.B, g.Lk)


def masked(g):
    """[B, Lq, Lk] bool: key j is masked for query (b, i)"""
    B, Lq, Lk = g.B, g.Lq, g.Lk
    b = torch.arange(B).view(B, 1, 1)
    i = torch.arange(Lq).view(1, Lq, 1)
    j = torch.arange(Lk).view(1, 1, Lk)
    m = torch.zeros(B, Lq, Lk, dtype=torch.bool)
    if g.causal:
        m = m | (j > g.q_pos0 + i)
    if g.key_valid is not None:
        bk = b % g.kv_bmod if g.kv_bmod else b
        m = m | (g.key_valid.flatten()[bk * g.kv_bs + j] == 0)
    if g.key_ids is not None:
        m = m | (g.key_ids.flatten()[b * g.kid_bs + j] == g.pad_idx)
    return m


def keep_mask(g):
    """(keep [B, H, Lq, Lk] bool, scale) of the dropout on the probabilities; (None, 1) when off"""
    if not g.drop_p > 0:
        return None, 1.0
    n = g.B * g.H * g.Lq * g.Lk
    keep = torch.from_numpy(drop_keep(g.drop_seed, g.drop_site, n, g.drop_p).reshape(g.B, g.H, g.Lq, g.Lk))
    return keep, float(np.float32(1.0) / (np.float32(1.0) - np.float32(g.drop_p)))


def attention_ref(g, dout=None, dtype=torch.float64):
    """dict of [B, H, L, dk] tensors (probs, Pd, dS: [B, H, Lq, Lk]) in `dtype` (float64: the reference;
    float32: the same formulas at the kernels' precision, to measure float32's own noise).
    dout: the flat dO buffer (layout o_ld / o_bs); dk / dv are None where K / V rows are shared
    (kv_bmod, kv_row: forward-only geometries)."""
    B, H, Lq, Lk, dk = g.B, g.H, g.Lq, g.Lk, g.dk
    kb = kv_batch(g)
    q = g.q.flatten()[index(g.q_off, g.q_ld, g.q_bs, B, H, Lq, dk)].to(dtype)
    k = g.k.flatten()[index(g.k_off, g.k_ld, g.k_bs, B, H, Lk, dk, kb)].to(dtype)
    v = g.v.flatten()[index(g.v_off, g.v_ld, g.v_bs, B, H, Lk, dk, kb)].to(dtype)
    T = torch.tensor(np.float32(g.temperature), dtype=dtype)
    m = masked(g).unsqueeze(1)
    s = (q / T) @ k.transpose(-1, -2)
    s = s.masked_fill(m, float("-inf"))
    e = torch.exp(s - s.max(-1, keepdim=True).values)
    p = e / e.sum(-1, keepdim=True)
    keep, scale = keep_mask(g)
    Pd = p if keep is None else torch.where(keep, p * scale, torch.zeros_like(p))
    out = {"q": q, "k": k, "v": v, "probs": p, "Pd": Pd, "o": Pd @ v, "masked": m, "keep": keep, "T": T}
    if dout is None:
        return out
    dO = dout.flatten()[index(0, g.o_ld, g.o_bs, B, H, Lq, dk)].to(dtype)
    dP = dO @ v.transpose(-1, -2)                       # d(p_dropped)
    if keep is not None:
        dP = torch.where(keep, dP * scale, torch.zeros_like(dP))
    dS = p * (dP - (p * dP).sum(-1, keepdim=True))      # softmax backward
    shared = g.kv_row is not None or g.kv_bmod > 0
    out.update({"dO": dO, "dS": dS, "dq": (dS @ k) / T,
                "dk": None if shared else dS.transpose(-1, -2) @ (q / T),
                "dv": None if shared else Pd.transpose(-1, -2) @ dO})
    return out


def head_mean_ref(probs, row):
    """out[b, j] = mean over heads of probs[b, :, row, j]  (model.py:123)"""
    return probs.double()[:, :, row, :].mean(1)


def mfma_extra(r):
    """The further elementwise error of the bf16 MFMA kernels: one bf16 rounding (2^-8 relative) of the
    operand they round before its product -- Pd in o and dv, dS in dq and dk."""
    u, T = 2.0 ** -8, r["T"]
    ex = {"o": u * (r["Pd"] @ r["v"].abs())}
    if "dS" in r:
        aS = r["dS"].abs()
        ex["dq"] = u * (aS @ r["k"].abs()) / T
        ex["dk"] = u * (aS.transpose(-1, -2) @ r["q"].abs()) / T
        ex["dv"] = u * (r["Pd"].transpose(-1, -2) @ r["dO"].abs())
    return ex


# ---- the conditions a case must meet ON THE REFERENCE so that a wrong mask cannot hide ---------------
MIN_LIVE_P = 1e-3


def check_conditions(g, r, tiles=False):
    """every query row has a live key; the smallest live probability is >= 1e-3 (one key wrongly masked
    or unmasked then moves probs by >= 100 x the tolerance); with dropout the dropped share is within 4
    binomial sd of p; tiles: every 16 x 16 (query tile, key tile) block holds kept and dropped elements.
    Returns (smallest live probability, dropped share or None)."""
    live = ~r["masked"].expand(g.B, g.H, g.Lq, g.Lk)
    assert live.any(-1).all(), "a query row without a live key"
    pmin = r["probs"][live].min().item()
    assert pmin >= MIN_LIVE_P, pmin
    assert (r["probs"][~live] == 0).all()
    share = None
    if r["keep"] is not None:
        n = r["keep"].numel()
        share = 1.0 - r["keep"].double().mean().item()
        sd = np.sqrt(g.drop_p * (1 - g.drop_p) / n)
        assert abs(share - g.drop_p) <= 4 * sd, (share, g.drop_p, sd)
        if tiles:
            assert g.Lq % 16 == 0 and g.Lk % 16 == 0
            t = r["keep"].view(g.B, g.H, g.Lq // 16, 16, g.Lk // 16, 16).permute(0, 1, 2, 4, 3, 5).reshape(
                g.B, g.H, g.Lq // 16, g.Lk // 16, 256)
            assert t.any(-1).all() and (~t).any(-1).all(), "a 16 x 16 block all kept or all dropped"
    return pmin, share
