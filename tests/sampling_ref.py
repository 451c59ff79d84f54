"""Float64 restatement of the sampled-decoding selection (sample_softmax, csrc/select.hip), written from
the kernel's header comment.  It never calls the library.

  z_v   = logits[r][v] * inv_tau                      (an f32 product)
  C     = every v < V (top_k == 0), else the top_k columns under (logit descending, v ascending)
  h     = mix32(seed, site, (uint32)(r * V + v)),  u = ((h >> 9) + 0.5) * 2^-23,  g = -log(-log(u))
  token = argmax over C of (z_v + g_v), first index on ties
  logp  = z_token - M - log sum_{v in C} exp(z_v - M),  M = max over C of z_v
"""
import numpy as np

M32 = 0xFFFFFFFF
SITE0 = 0x5A00  # capgen_sample draws position t at site SITE0 + t
SEEDS = (0x0123456789ABCDEF, 7, 0xFFFFFFFF00000001)


def lowbias32(x):
    """the 32-bit avalanche hash of the dropout masks (capgen_common.h), on uint64 arrays holding uint32"""
    x = np.asarray(x, dtype=np.uint64) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(M32)
    x = x ^ (x >> np.uint64(16))
    return x


def drop_key(seed, site):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    inner = ((seed >> 32) + 0x9E3779B9 * ((int(site) + 1) & M32)) & M32
    return int(lowbias32((seed & M32) ^ int(lowbias32(inner))))


def mix32(seed, site, idx):
    return lowbias32(np.asarray(idx, dtype=np.uint64) ^ np.uint64(drop_key(seed, site)))


def uniform(seed, site, idx):
    """u of counter idx: a multiple of 2^-24 strictly inside (0, 1), exact in f32 and in f64"""
    return ((mix32(seed, site, idx) >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(seed, site, R, V, row0=0):
    """g[r][v] of rows row0 .. row0 + R - 1 (float64)"""
    idx = (np.arange(row0, row0 + R, dtype=np.uint64)[:, None] * np.uint64(V) + np.arange(V, dtype=np.uint64)[None, :])
    return -np.log(-np.log(uniform(seed, site, idx & np.uint64(M32))))


def inv_tau_of(temperature):
    """1 / temperature as the engine forms it (one f32 division)"""
    return np.float32(1.0) / np.float32(temperature)


def candidates(logits, top_k):
    """bool [R, V]: the candidate set C; and the gap between logits top_k and top_k + 1 of the ranking
    (inf where there is no logit top_k + 1 or top_k == 0)"""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    if top_k == 0:
        return np.ones((R, V), dtype=bool), np.full(R, np.inf)
    order = np.argsort(-x.astype(np.float64), axis=1, kind="stable")  # logit descending, v ascending
    C = np.zeros((R, V), dtype=bool)
    np.put_along_axis(C, order[:, :top_k], True, axis=1)
    if top_k >= V:
        return C, np.full(R, np.inf)
    rows = np.arange(R)
    gap = x[rows, order[:, top_k - 1]].astype(np.float64) - x[rows, order[:, top_k]].astype(np.float64)
    return C, gap


def sample(logits, inv_tau, top_k, seed, site, g=None, cand=None):
    """-> dict(token [R], logp [R], margin [R]: the two best perturbed scores' gap (inf with one
    candidate), kgap [R]: candidates()'s gap).  g / cand: gumbel(seed, site, R, V) / candidates(logits,
    top_k) where the caller already has them."""
    x = np.asarray(logits, dtype=np.float32)
    R, V = x.shape
    z = (x * np.float32(inv_tau)).astype(np.float32).astype(np.float64)
    C, kgap = candidates(x, top_k) if cand is None else cand
    score = np.where(C, z + (gumbel(seed, site, R, V) if g is None else g), -np.inf)
    token = score.argmax(axis=1)  # first index on ties
    rows = np.arange(R)
    if V > 1:
        top2 = -np.partition(-score, 1, axis=1)[:, :2]
        margin = top2[:, 0] - top2[:, 1]
    else:
        margin = np.full(R, np.inf)
    zc = np.where(C, z, -np.inf)
    M = zc.max(axis=1)
    logp = z[rows, token] - M - np.log(np.exp(zc - M[:, None]).sum(axis=1))
    return {"token": token, "logp": logp, "margin": margin, "kgap": kgap}


def chi2(counts, expected):
    counts, expected = np.asarray(counts, dtype=np.float64), np.asarray(expected, dtype=np.float64)
    return float(((counts - expected) ** 2 / expected).sum())
