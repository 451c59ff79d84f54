"""Float64 restatement of the decode constraints (constrain_logits, capgen_set_decode_constraints), written
from the definition in csrc/select.hip's header comment.  It never calls the library.

The step at position t predicts column t + 1.  A row's emitted tokens are e = ids[1 .. t] (<START> in column 0
is not counted).  From the logits z, in this order:

  1. repetition penalty theta (1 = off): every distinct word w of e: z[w] / theta if z[w] > 0 else z[w] * theta,
     once per word
  2. banned words: z[w] = -inf
  3. minimum length m (0 = off): z[end_id] = -inf while t + 1 < m
  4. no-repeat n-gram n (0 = off), when t >= n - 1: for every a with e[a .. a+n-2] == e[t-n+2 .. t] (and
     a + n - 1 <= t), z[e[a+n-1]] = -inf; n = 1 blocks every emitted word

`edit` is one row, `edit_rows` a [R, V] block, `search` is beam_ref.search's loop with `edit` applied before
the log-softmax (beam_ref.step / nbest / finish are reused as they are)."""
import numpy as np
import torch

import beam_ref as R
from oracle import capgen_oracle as O


def constraints(n=0, m=0, end_id=-1, theta=1.0, banned=()):
    """the settings as one dict (theta as the f32 the library receives)"""
    return {"n": int(n), "m": int(m), "end_id": int(end_id), "theta": float(np.float32(theta)),
            "banned": tuple(int(w) for w in banned)}


def touched(e, t, c, V):
    """(penalised, blocked): the distinct words of e[1 .. t] in [0, V) where theta != 1, and the set of
    blocked words of rules 2 to 4"""
    e = [int(w) for w in np.asarray(e).reshape(-1)[:t + 1]]
    pen = []
    if c["theta"] != 1.0:
        for w in e[1:t + 1]:
            if 0 <= w < V and w not in pen:
                pen.append(w)
    blk = set(c["banned"])
    if c["m"] > 0 and t + 1 < c["m"]:
        blk.add(c["end_id"])
    n = c["n"]
    if n > 0 and t >= n - 1:
        tail = e[t - n + 2:t + 1]  # n - 1 tokens (none for n = 1)
        for a in range(1, t - n + 2):  # a + n - 1 <= t
            if e[a:a + n - 1] == tail and 0 <= e[a + n - 1] < V:
                blk.add(e[a + n - 1])
    return pen, blk


def edit(z, e, t, c):
    """The constrained logits of one row, float64 [V].  A float32 z takes the penalty as one f32 division or
    product (what the kernel computes, exactly); a float64 z takes it in float64."""
    z = np.array(z)
    assert z.ndim == 1
    pen, blk = touched(e, t, c, z.size)
    theta = z.dtype.type(c["theta"])
    for w in pen:
        z[w] = z[w] / theta if z[w] > 0 else z[w] * theta
    z = z.astype(np.float64)
    for w in blk:
        z[w] = -np.inf
    return z


def edit_rows(x, ids, t, c):
    """edit on every row of x [R, V] with the histories ids [R, >= t + 1]"""
    return np.stack([edit(x[r], ids[r], t, c) for r in range(x.shape[0])])


def repeats(tokens, n):
    """the number of n-grams of the token list that occurred earlier in it"""
    tokens = [int(w) for w in tokens]
    seen, count = set(), 0
    for a in range(len(tokens) - n + 1):
        g = tuple(tokens[a:a + n])
        count += g in seen
        seen.add(g)
    return count


def search(P64, cfg, feats, pos, k, end_id, c):
    """beam_ref.search with the logits of every source row edited before the log-softmax.  -> its dict and
    blocked: the -inf entries the edits left in the source rows' logits over all steps (finished rows are
    edited like any other)"""
    T, V = cfg.max_length, cfg.num_vocab
    feats, pos = feats.double(), pos.double()
    with torch.no_grad():
        enc = O.encode(P64, cfg, feats, pos, False)
        B = enc.size(0)
        seq = np.zeros((k, B, T), dtype=np.int64)
        seq[:, :, 0] = 1
        logp, fin, length = np.zeros((k, B)), np.zeros((k, B), np.int64), np.zeros((k, B), np.int64)
        step_margin, mixed, blocked = np.full(B, np.inf), np.zeros(B, dtype=bool), 0
        for t in range(T - 1):
            k_in = 1 if t == 0 else k
            ls = np.zeros((k_in, B, V))
            for j in range(k_in):
                prefix = torch.from_numpy(seq[j, :, :t + 1].copy())
                dec, _, _ = O.decode(P64, cfg, prefix, enc, O.context_mask(pos, t + 1), False)
                logits = (dec[:, t] @ P64["classifer.weight"].t() + P64["classifer.bias"]).numpy()
                z = edit_rows(logits, seq[j], t, c)
                blocked += int(np.isinf(z).sum())
                ls[j] = R.log_softmax64(z)
            f_in = fin[:k_in]
            mixed |= f_in.any(axis=0) & ~f_in.all(axis=0)
            st = R.step(ls, logp[:k_in], f_in, length[:k_in], k, end_id)
            step_margin = np.minimum(step_margin, st["gaps"].min(axis=1))
            seq = np.take_along_axis(seq, st["src"][:, :, None], 0)
            seq[:, :, t + 1] = st["tok"]
            logp, fin, length = st["logp"], st["fin"], st["len"]
    return {"seq": seq, "logp": logp, "len": length, "fin": fin, "step_margin": step_margin, "mixed": mixed,
            "blocked": blocked}
