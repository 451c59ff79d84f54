"""Float64 restatement of diverse beam search (capgen_beam_diverse), written from the definition in
csrc/select.hip's header comment.  It never calls the library.

  k beams in G groups of k' = k / G, group g = beams g k' .. (g + 1) k' - 1, penalty lam >= 0.  A hypothesis is
  beam_ref's (tokens, logp, len, fin); logp never contains the penalty.
  step   : per image the groups in order.  c(v) = the hypotheses selected at this step for earlier groups of the
           image from a live source with token v.  Group g's candidates come from its own k' source rows (step
           0: beam 0): a live source j offers (logp_j + logsoftmax[j][v] - lam * c(v), flat index j * V + v), a
           finished one exactly (logp_j, j * V + 0), unpenalised.  The k' best under (penalised score
           descending, flat index ascending) become beams g k' + rank.
  update : beam_ref.step's, with the unpenalised logp_j + logsoftmax[j][v] as the new logp
  end    : beam_ref.finish per group; output row g * n_best + rank

`step` is one selection from given log-softmax rows, `search` runs it over a function that gives a source
beam's rows (the model, the constrained model, an ensemble: the three makers below), `nbest` is the end.  The
margins a comparison with an f32 implementation needs come back too: the gaps between consecutive penalised
scores among the first k' + 1 candidates of every group at every step, and the per-group final-score gaps."""
import numpy as np
import torch

import beam_ref as R
from oracle import capgen_oracle as O


def step(ls, logp, fin, length, k, G, lam, end_id):
    """One selection.  ls [k_in, B, V] f64 log-softmax rows with k_in = 1 (step 0) or k (rows of finished
    sources are never read), logp / fin / length [k_in, B].  -> dict(logp [k, B] f64 unpenalised, src, tok, fin,
    len [k, B] int64, count [k, B]: c of each selected candidate, gaps [B, G, k']: the gaps between consecutive
    penalised scores among the first k' + 1 candidates of each group (inf where there is no such candidate),
    cmax [B]: the largest c among the candidates selected or displaced (among the group's k' best unpenalised
    but not selected))"""
    k_in, B, V = ls.shape
    assert k % G == 0 and k_in in (1, k) and lam >= 0
    kg = k // G
    out = {"logp": np.empty((k, B)), "src": np.zeros((k, B), np.int64), "tok": np.zeros((k, B), np.int64),
           "fin": np.zeros((k, B), np.int64), "len": np.zeros((k, B), np.int64), "count": np.zeros((k, B), np.int64),
           "gaps": np.full((B, G, kg), np.inf), "cmax": np.zeros(B, np.int64)}
    for i in range(B):
        c = np.zeros(V, np.int64)
        for g in range(G):
            sources = [0] if k_in == 1 else range(g * kg, (g + 1) * kg)
            raw, pen, flat = [], [], []
            for j in sources:
                if fin[j, i]:
                    raw.append(np.array([logp[j, i]], dtype=np.float64))
                    pen.append(np.zeros(1, np.int64))
                    flat.append(np.array([j * V], dtype=np.int64))
                else:
                    raw.append(logp[j, i] + ls[j, i])
                    pen.append(c.copy())
                    flat.append(j * V + np.arange(V, dtype=np.int64))
            raw, pen, flat = np.concatenate(raw), np.concatenate(pen), np.concatenate(flat)
            assert raw.size >= kg, "a group needs at least k' candidates"
            score = raw - lam * pen
            first = np.lexsort((flat, -score))[:kg + 1]  # (penalised score descending, flat index ascending)
            s = score[first]
            out["gaps"][i, g, :s.size - 1] = s[:-1] - s[1:]
            plain = np.lexsort((flat, -raw))[:kg]
            looked_at = np.union1d(first[:kg], plain)
            out["cmax"][i] = max(out["cmax"][i], int(pen[looked_at].max()))
            chosen = []
            for r in range(kg):
                at, row = first[r], g * kg + r
                j, v = divmod(int(flat[at]), V)
                out["logp"][row, i], out["src"][row, i], out["tok"][row, i] = raw[at], j, v
                out["count"][row, i] = pen[at]
                if fin[j, i]:
                    assert v == 0
                    out["fin"][row, i], out["len"][row, i] = 1, length[j, i]
                else:
                    out["fin"][row, i], out["len"][row, i] = int(v == end_id), length[j, i] + 1
                    chosen.append(v)
            for v in chosen:  # (counted for the groups after this one only)
                c[v] += 1
    return out


def model_rows(P64, cfg, feats, pos, edit=None):
    """rows(seq_j [B, t + 1], t) -> [B, V] f64 log-softmax of the model's logits at position t, full-prefix
    recompute; edit (optional): (logits [B, V], histories, t) -> edited logits, before the log-softmax"""
    feats, pos = feats.double(), pos.double()
    with torch.no_grad():
        enc = O.encode(P64, cfg, feats, pos, False)

    def rows(seq_j, t):
        with torch.no_grad():
            dec, _, _ = O.decode(P64, cfg, torch.from_numpy(seq_j[:, :t + 1].copy()), enc, O.context_mask(pos, t + 1),
                                 False)
            z = dec[:, t] @ P64["classifer.weight"].t() + P64["classifer.bias"]
            if edit is None:  # (beam_ref.search's own arithmetic: one group is that search bit for bit)
                return torch.log_softmax(z, dim=1).numpy()
        return R.log_softmax64(edit(z.numpy(), seq_j, t))
    return rows


def constrained_rows(P64, cfg, feats, pos, c):
    """model_rows with constrain_ref's edit in front of the log-softmax"""
    import constrain_ref as CR
    return model_rows(P64, cfg, feats, pos, edit=lambda z, ids, t: CR.edit_rows(z, ids, t, c))


def ensemble_rows(Ps, w, mode, cfg, feats, pos):
    """the members' rows fused as ensemble_ref.combine_logsm fuses them, then the selection's log-softmax"""
    import ensemble_ref as E
    members = [model_rows(P, cfg, feats, pos) for P in Ps]
    return lambda seq_j, t: R.log_softmax64(E.combine_logsm(np.stack([m(seq_j, t) for m in members]), w, mode))


def search(rows, B, T, V, k, G, lam, end_id):
    """The search over rows(seq_j, t).  -> dict(seq [k, B, T] int64, logp [k, B] f64 (the sum of the unpenalised
    token log-probabilities), len, fin [k, B], step_margin [B]: the smallest gap of any group at any step,
    penalty [k, B]: lam * c summed over the hypothesis' own history, tok_logp [k, B, T - 1]: each appended
    token's unpenalised log-probability (0 where the source was finished), steps: the list of step dicts)"""
    seq = np.zeros((k, B, T), dtype=np.int64)
    seq[:, :, 0] = 1
    logp, fin, length = np.zeros((k, B)), np.zeros((k, B), np.int64), np.zeros((k, B), np.int64)
    penalty, tok_logp = np.zeros((k, B)), np.zeros((k, B, T - 1))
    step_margin, steps = np.full(B, np.inf), []
    for t in range(T - 1):
        k_in = 1 if t == 0 else k
        ls = np.stack([rows(seq[j], t) for j in range(k_in)])
        st = step(ls, logp[:k_in], fin[:k_in], length[:k_in], k, G, lam, end_id)
        steps.append(st)
        step_margin = np.minimum(step_margin, st["gaps"].min(axis=(1, 2)))
        src = st["src"]
        gain = st["logp"] - np.take_along_axis(logp[:k_in], src, 0)
        seq = np.take_along_axis(seq, src[:, :, None], 0)  # row (j, i) <- row (src[j, i], i)
        seq[:, :, t + 1] = st["tok"]
        tok_logp = np.take_along_axis(tok_logp, src[:, :, None], 0)
        tok_logp[:, :, t] = gain
        penalty = np.take_along_axis(penalty, src, 0) + lam * st["count"]
        logp, fin, length = st["logp"], st["fin"], st["len"]
    return {"seq": seq, "logp": logp, "len": length, "fin": fin, "step_margin": step_margin, "penalty": penalty,
            "tok_logp": tok_logp, "steps": steps}


def nbest(state, G, alpha, n_best):
    """beam_ref.finish per group on a search's state -> dict(ids [G * n_best, B, T], score, logp, len
    [G * n_best, B], penalty [G * n_best, B], margin [B] = min(step margin, every group's final margin))"""
    k, B, _ = state["seq"].shape
    kg = k // G
    parts = {"ids": [], "score": [], "logp": [], "len": [], "penalty": []}
    margin = state["step_margin"].copy()
    for g in range(G):
        sl = slice(g * kg, (g + 1) * kg)
        f = R.finish(state["logp"][sl], state["len"][sl], alpha, n_best)
        parts["ids"].append(np.take_along_axis(state["seq"][sl], f["order"][:, :, None], 0))
        parts["penalty"].append(np.take_along_axis(state["penalty"][sl], f["order"], 0))
        for name in ("score", "logp", "len"):
            parts[name].append(f[name])
        margin = np.minimum(margin, f["final_margin"])
    out = {name: np.concatenate(v, axis=0) for name, v in parts.items()}
    out["margin"] = margin
    return out
