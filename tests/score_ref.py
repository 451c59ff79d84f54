"""Float64 restatement of capgen_score_captions' read-out (pure torch, CPU): from the logits of a
teacher-forced forward and the targets, per row

    token_logp = logit[tgt] - logsumexp(logit)      (0 where tgt == pad)
    hit        = tgt != pad and logit[tgt] >= max(logit)   (the target is the argmax; ties count)

and per caption of Lq rows: logp = sum token_logp, length = #(tgt != pad), hits = sum hit."""
import torch


def score_rows_ref(logits, tgt, pad):
    """logits [M, V] (any float dtype; computed in float64), tgt [M] -> dict of [M] tensors:
    token_logp (f64), hit (int64), kept (bool), lse, tl (f64), margin (f64: the top-1 minus top-2 logit)"""
    x = logits.double()
    t = tgt.long()
    M = x.shape[0]
    lse = torch.logsumexp(x, 1)
    tl = x[torch.arange(M), t]
    kept = t != pad
    top = x.max(1).values
    token_logp = torch.where(kept, tl - lse, torch.zeros_like(lse))
    hit = (kept & (tl >= top)).long()
    if x.shape[1] > 1:
        top2 = torch.topk(x, 2, dim=1).values
        margin = top2[:, 0] - top2[:, 1]
    else:
        margin = torch.full_like(lse, float("inf"))
    return {"token_logp": token_logp, "hit": hit, "kept": kept, "lse": lse, "tl": tl, "margin": margin}


def score_ref(logits, tgt, pad, Lq):
    """logits [R * Lq, V] or [R, Lq, V], tgt [R * Lq] or [R, Lq] -> the rows' dict reshaped to [R, Lq], plus
    logp [R] (f64), length [R] and hits [R] (int64)"""
    V = logits.shape[-1]
    rows = score_rows_ref(logits.reshape(-1, V), tgt.reshape(-1), pad)
    out = {k: v.view(-1, Lq) for k, v in rows.items()}
    out["logp"] = out["token_logp"].sum(1)
    out["length"] = out["kept"].long().sum(1)
    out["hits"] = out["hit"].sum(1)
    return out
