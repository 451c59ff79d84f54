"""Float64 restatement of the nucleus (top-p) selection (sample_nucleus, csrc/select.hip), written from
the kernel's header comment on sampling_ref's hash, noise and candidate helpers.  It never calls the
library.

  z_v      = logits[r][v] * inv_tau                    (an f32 product)
  C0       = every v < V (top_k == 0), else the top_k columns under (logit descending, v ascending)
  M, P     = max over C0 of z_v,  sum_{u in C0} exp(z_u - M)
  above(v) = sum_{u in C0, z_u > z_v} exp(z_u - M)     (strict)
  C        = { v in C0 : above(v) < top_p * P };  C = C0 when top_p == 1, by definition
  token    = argmax over C of (z_v + g_v), first index on ties (g: sampling_ref.gumbel)
  logp     = z_token - M_C - log sum_{v in C} exp(z_v - M_C),  M_C = max over C of z_v
"""
import numpy as np

import sampling_ref as S


def ranking(logits):
    """the columns of each row under (logit descending, v ascending), as candidates() ranks them"""
    return np.argsort(-np.asarray(logits, dtype=np.float32).astype(np.float64), axis=1, kind="stable")


def masses(logits, inv_tau, top_k, cand=None, order=None):
    """what does not depend on top_p or the noise: dict(z [R, V] f64, C0 bool [R, V], above [R, V]
    (P outside C0), P [R], kgap [R]: candidates()'s gap).  cand / order: candidates(logits, top_k) /
    ranking(logits) where the caller has them (z is monotone in the logit and C0 a prefix of the
    ranking, so the ranking also sorts z over C0, ties in z adjacent)"""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    z = (x * np.float32(inv_tau)).astype(np.float32).astype(np.float64)
    C0, kgap = S.candidates(x, top_k) if cand is None else cand
    zc = np.where(C0, z, -np.inf)
    with np.errstate(invalid="ignore"):
        e = np.where(C0, np.exp(zc - zc.max(axis=1, keepdims=True)), 0.0)
    e = np.where(np.isnan(e), 0.0, e)  # (a row of C0 all -inf)
    P = e.sum(axis=1)
    order = np.argsort(-zc, axis=1, kind="stable") if order is None else order
    zs, es = np.take_along_axis(zc, order, 1), np.take_along_axis(e, order, 1)
    before = np.cumsum(es, axis=1) - es  # the mass ranked before each sorted column
    start = np.zeros((R, V), dtype=np.int64)  # where each column's group of equal z begins
    if V > 1:
        start[:, 1:] = np.where(zs[:, 1:] != zs[:, :-1], np.arange(1, V)[None, :], 0)
        start = np.maximum.accumulate(start, axis=1)
    above = np.empty((R, V))
    np.put_along_axis(above, order, np.take_along_axis(before, start, 1), axis=1)
    above = np.where(C0, above, P[:, None])
    return {"z": z, "C0": C0, "above": above, "P": P, "kgap": kgap}


def nucleus_set(m, top_p):
    """bool [R, V]: the candidate set C of masses() m at top_p (>= 1: C0)"""
    if top_p >= 1:
        return m["C0"].copy()
    return m["C0"] & (m["above"] < top_p * m["P"][:, None])


def logp_at(m, C, token):
    """[R]: the log-probability of token [R] under the softmax of z renormalised over C (-inf outside C)"""
    zc = np.where(C, m["z"], -np.inf)
    M = zc.max(axis=1)
    return zc[np.arange(zc.shape[0]), token] - M - np.log(np.exp(zc - M[:, None]).sum(axis=1))


def select(m, C, g):
    """token, logp, count and perturbed top-2 margin of the draw from candidate set C with noise g"""
    z = m["z"]
    R, V = z.shape
    score = np.where(C, z + g, -np.inf)
    token = score.argmax(axis=1)  # first index on ties
    if V > 1:
        top2 = -np.partition(-score, 1, axis=1)[:, :2]
        margin = top2[:, 0] - top2[:, 1]  # (inf with one candidate)
    else:
        margin = np.full(R, np.inf)
    return {"C": C, "token": token, "logp": logp_at(m, C, token), "count": C.sum(axis=1), "margin": margin}


def band(m, top_p, eps, g, margin):
    """The boundary rule of the GPU tests.  The kernel sums masses in f32, so a column whose above / P
    is within eps of top_p may fall on either side: with C_lo = C(top_p - eps) and C_hi = C(top_p + eps)
    (C0 from 1 on), a row is determined when the Gumbel winner over C_hi lies in C_lo and leads the
    runner-up in C_hi by at least margin.  -> dict(token [R]: the winner over C_hi, determined bool [R],
    C_lo, C_hi, count_lo, count_hi, logp_lo, logp_hi [R]: the token's logp under C_lo (the larger; -inf
    where it is not in C_lo) and under C_hi)"""
    p = float(np.float32(top_p))
    C_lo, C_hi = nucleus_set(m, p - eps), nucleus_set(m, p + eps)
    hi = select(m, C_hi, g)
    tok = hi["token"]
    determined = C_lo[np.arange(tok.size), tok] & (hi["margin"] >= margin)
    with np.errstate(invalid="ignore"):
        logp_lo = logp_at(m, C_lo, tok)
    return {"token": tok, "determined": determined, "C_lo": C_lo, "C_hi": C_hi, "count_lo": C_lo.sum(axis=1),
            "count_hi": C_hi.sum(axis=1), "logp_lo": logp_lo, "logp_hi": hi["logp"]}


def sample(logits, inv_tau, top_k, top_p, seed, site, g=None, m=None):
    """-> dict(C bool [R, V], token [R], logp [R], count [R] = |C|, margin [R]: the two best perturbed
    scores' gap within C (inf with one candidate)).  top_p is taken as the f32 the library receives.
    g / m: sampling_ref.gumbel(seed, site, R, V) / masses(logits, inv_tau, top_k) where the caller has them."""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    m = masses(x, inv_tau, top_k) if m is None else m
    g = S.gumbel(seed, site, R, V) if g is None else g
    return select(m, nucleus_set(m, float(np.float32(top_p))), g)
