"""Float64 restatement of ensemble decoding (capgen_ensemble_beam_nbest / ensemble_combine), written from
the definition in include/capgen.h and csrc/select.hip.  It never calls the library.

  members k < K with weights w_k > 0, normalised to sum 1;  l_k = log_softmax(z_k)
  prob    : y[v] = log sum_k w_k exp(l_k[v]) = logsumexp_k(log w_k + l_k[v])
  logprob : y[v] = sum_k w_k l_k[v]
  y is the step's logits: the selection takes its log-softmax (beam_ref.step on beam_ref.log_softmax64(y))

`combine` is one step's fusion; `search` is beam_ref.search with every member's decoder run on the shared
hypotheses and their rows combined."""
import numpy as np
import torch

import beam_ref
from oracle import capgen_oracle as O

MODES = ("prob", "logprob")


def weights64(w, K):
    w = np.ones(K) if w is None else np.asarray(w, dtype=np.float64)
    assert w.shape == (K,) and (w > 0).all() and np.isfinite(w).all()
    return w / w.sum()


def combine_logsm(l, w, mode):
    """the members' float64 log-softmax rows l [K, R, V] -> y [R, V]"""
    w = weights64(w, l.shape[0])
    if mode == "logprob":
        return (w[:, None, None] * l).sum(axis=0)
    assert mode == "prob"
    a = np.log(w)[:, None, None] + l
    m = a.max(axis=0)
    return m + np.log(np.exp(a - m[None]).sum(axis=0))


def combine(logits, w, mode):
    """logits [K, R, V] -> y [R, V] f64"""
    return combine_logsm(beam_ref.log_softmax64(logits), w, mode)


def search(Ps, w, mode, cfg, feats, pos, k, end_id):
    """beam_ref.search over K members' float64 parameters Ps: the same state dict"""
    T, V, K = cfg.max_length, cfg.num_vocab, len(Ps)
    feats, pos = feats.double(), pos.double()
    with torch.no_grad():
        encs = [O.encode(P, cfg, feats, pos, False) for P in Ps]
        B = encs[0].size(0)
        seq = np.zeros((k, B, T), dtype=np.int64)
        seq[:, :, 0] = 1
        logp, fin, length = np.zeros((k, B)), np.zeros((k, B), np.int64), np.zeros((k, B), np.int64)
        step_margin, mixed = np.full(B, np.inf), np.zeros(B, dtype=bool)
        for t in range(T - 1):
            k_in = 1 if t == 0 else k
            ls = np.zeros((k_in, B, V))
            for j in range(k_in):
                prefix = torch.from_numpy(seq[j, :, :t + 1].copy())
                rows = []
                for P, enc in zip(Ps, encs):
                    dec, _, _ = O.decode(P, cfg, prefix, enc, O.context_mask(pos, t + 1), False)
                    rows.append((dec[:, t] @ P["classifer.weight"].t() + P["classifer.bias"]).numpy())
                ls[j] = beam_ref.log_softmax64(combine(np.stack(rows), w, mode))
            f_in = fin[:k_in]
            mixed |= f_in.any(axis=0) & ~f_in.all(axis=0)
            st = beam_ref.step(ls, logp[:k_in], f_in, length[:k_in], k, end_id)
            step_margin = np.minimum(step_margin, st["gaps"].min(axis=1))
            seq = np.take_along_axis(seq, st["src"][:, :, None], 0)
            seq[:, :, t + 1] = st["tok"]
            logp, fin, length = st["logp"], st["fin"], st["len"]
    return {"seq": seq, "logp": logp, "len": length, "fin": fin, "step_margin": step_margin, "mixed": mixed}


# the rows of the comparison: (fixture, member seeds, mode, weights, the alphas pinned, finished of k * B at k = 3)
TABLE = (
    ("c1", (0, 105), "prob", (.5, .5), ((0.0, 2.3e-3), (1.0, 2.0e-3)), (11, 24)),
    ("c1", (0, 105), "prob", (.7, .3), ((0.0, 2.9e-3), (1.0, 1.6e-3)), (10, 24)),
    ("c1", (0, 103), "logprob", (.5, .5), ((0.0, 2.6e-3), (1.0, 2.6e-3)), (19, 24)),
    ("c1", (0, 103), "logprob", (.7, .3), ((0.0, 6.1e-3), (1.0, 1.5e-3)), (17, 24)),
    ("c1", (0, 105, 103), "prob", (.5, .3, .2), ((0.0, 1.32e-3),), (10, 24)),
    ("c1", (0, 105, 103), "logprob", (.5, .3, .2), ((0.0, 1.18e-3),), (12, 24)),
    ("c2s", (3, 103), "prob", (.5, .5), ((0.0, 2.1e-2),), (5, 6)),
    ("c2s", (3, 103), "logprob", (.7, .3), ((0.0, 2.3e-3),), (4, 6)),
)
