"""Float64 restatement of the END-aware n-best beam search (capgen_beam_nbest), written from the definition
in csrc/select.hip's header comment.  It never calls the library.

  hypothesis = tokens, logp (sum of its token log-probabilities), len (tokens emitted while live, <END>
               included), fin;  start: <START>, logp = 0, len = 0, fin = 0; at step 0 only beam 0 is a source
  step       : a live source row j offers (logp_j + logsoftmax(logits[j, i])[v], flat index j * V + v) for
               every v, a finished one exactly (logp_j, j * V + 0); the k best under (score descending, flat
               index ascending)
  update     : from a finished source token 0 is appended and logp / len / fin are copied; from a live one
               token v, len + 1, fin = (v == end_id)
  end        : s = logp (alpha == 0) or logp / max(len, 1) ** alpha; per image the n_best under (s descending,
               beam ascending)

`step` is one selection from given logits (the kernel tests); `search` runs it over oracle.encode / decode /
context_mask with full-prefix recompute and no cache; `finish` is the end.  Both also return the margins a
comparison with an f32 implementation needs: the gaps between consecutive scores among the first k + 1
candidates of a step, and between consecutive final scores."""
import numpy as np
import torch

from oracle import capgen_oracle as O


def log_softmax64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def step(ls, logp, fin, length, k, end_id):
    """One selection.  ls [k_in, B, V] f64 log-softmax rows (rows of finished sources are never read), logp /
    fin / length [k_in, B].  -> dict(logp [k, B] f64, src, tok, fin, len [k, B] int64, gaps [B, k]: the gaps
    between consecutive scores among the first k + 1 candidates (inf where there is no such candidate))"""
    k_in, B, V = ls.shape
    out = {"logp": np.empty((k, B)), "src": np.zeros((k, B), np.int64), "tok": np.zeros((k, B), np.int64),
           "fin": np.zeros((k, B), np.int64), "len": np.zeros((k, B), np.int64), "gaps": np.full((B, k), np.inf)}
    for i in range(B):
        score, flat = [], []
        for j in range(k_in):
            if fin[j, i]:
                score.append(np.array([logp[j, i]], dtype=np.float64))
                flat.append(np.array([j * V], dtype=np.int64))
            else:
                score.append(logp[j, i] + ls[j, i])
                flat.append(j * V + np.arange(V, dtype=np.int64))
        score, flat = np.concatenate(score), np.concatenate(flat)
        assert score.size >= k, "a step needs at least k candidates"
        first = np.lexsort((flat, -score))[:k + 1]  # (score descending, flat index ascending)
        s = score[first]
        out["gaps"][i, :s.size - 1] = s[:-1] - s[1:]
        for r in range(k):
            j, v = divmod(int(flat[first[r]]), V)
            out["logp"][r, i], out["src"][r, i], out["tok"][r, i] = s[r], j, v
            if fin[j, i]:
                assert v == 0
                out["fin"][r, i], out["len"][r, i] = 1, length[j, i]
            else:
                out["fin"][r, i], out["len"][r, i] = int(v == end_id), length[j, i] + 1
    return out


def finish(logp, length, alpha, n_best):
    """-> dict(order [n_best, B]: the beam at each rank, score / logp [n_best, B] f64, len [n_best, B],
    final_margin [B]: the smallest gap between consecutive final scores of ALL k hypotheses (inf at k = 1))"""
    k, B = logp.shape
    logp = np.asarray(logp, dtype=np.float64)
    s = logp if alpha == 0 else logp / np.maximum(length, 1).astype(np.float64) ** float(alpha)
    order = np.stack([np.lexsort((np.arange(k), -s[:, i])) for i in range(B)], axis=1)  # [k, B]
    ss = np.take_along_axis(s, order, 0)
    margin = (ss[:-1] - ss[1:]).min(axis=0) if k > 1 else np.full(B, np.inf)
    top = order[:n_best]
    return {"order": top, "score": ss[:n_best], "logp": np.take_along_axis(logp, top, 0),
            "len": np.take_along_axis(np.asarray(length), top, 0), "final_margin": margin}


def search(P64, cfg, feats, pos, k, end_id):
    """The search on float64 parameters P64 (oracle.make_params(..., dtype=torch.float64)).  -> dict(seq
    [k, B, T] int64, logp [k, B] f64, len, fin [k, B], step_margin [B]: the smallest gap between consecutive
    scores among the first k + 1 candidates at any step, mixed [B]: the image held finished and live
    hypotheses together as sources of some step)"""
    T, V = cfg.max_length, cfg.num_vocab
    feats, pos = feats.double(), pos.double()
    with torch.no_grad():
        enc = O.encode(P64, cfg, feats, pos, False)
        B = enc.size(0)
        seq = np.zeros((k, B, T), dtype=np.int64)
        seq[:, :, 0] = 1
        logp, fin, length = np.zeros((k, B)), np.zeros((k, B), np.int64), np.zeros((k, B), np.int64)
        step_margin, mixed = np.full(B, np.inf), np.zeros(B, dtype=bool)
        for t in range(T - 1):
            k_in = 1 if t == 0 else k
            ls = np.zeros((k_in, B, V))
            for j in range(k_in):
                prefix = torch.from_numpy(seq[j, :, :t + 1].copy())
                dec, _, _ = O.decode(P64, cfg, prefix, enc, O.context_mask(pos, t + 1), False)
                logits = dec[:, t] @ P64["classifer.weight"].t() + P64["classifer.bias"]
                ls[j] = torch.log_softmax(logits, dim=1).numpy()
            f_in = fin[:k_in]
            mixed |= f_in.any(axis=0) & ~f_in.all(axis=0)
            st = step(ls, logp[:k_in], f_in, length[:k_in], k, end_id)
            step_margin = np.minimum(step_margin, st["gaps"].min(axis=1))
            seq = np.take_along_axis(seq, st["src"][:, :, None], 0)  # row (j, i) <- row (src[j, i], i)
            seq[:, :, t + 1] = st["tok"]
            logp, fin, length = st["logp"], st["fin"], st["len"]
    return {"seq": seq, "logp": logp, "len": length, "fin": fin, "step_margin": step_margin, "mixed": mixed}


def nbest(state, alpha, n_best):
    """finish on a search's state -> dict(ids [n_best, B, T], score, logp, len [n_best, B], margin [B] =
    min(step margin, final margin))"""
    f = finish(state["logp"], state["len"], alpha, n_best)
    ids = np.take_along_axis(state["seq"], f["order"][:, :, None], 0)
    return {"ids": ids, "score": f["score"], "logp": f["logp"], "len": f["len"],
            "margin": np.minimum(state["step_margin"], f["final_margin"])}


def structure_ok(ids, length, end_id, T):
    """the shape every result has: <START> first, zeros after the first end_id, len = tokens through it"""
    ids, length = np.asarray(ids), np.asarray(length)
    flat, ln = ids.reshape(-1, T), length.reshape(-1)
    for row, n in zip(flat, ln):
        assert row[0] == 1, row
        hit = np.nonzero(row[1:] == end_id)[0] if end_id >= 0 else np.array([], dtype=np.int64)
        if hit.size:
            assert n == hit[0] + 1 and (row[hit[0] + 2:] == 0).all(), (row, n)
        else:
            assert n == T - 1, (row, n)
