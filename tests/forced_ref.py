"""Float64 restatement of forced-word beam search (capgen_beam_forced), written from the definition in
csrc/select.hip's header comment.  It never calls the library.

  image i has W slots (word[i][s], group[i][s]), word = -1 an empty slot; bits_i(v) = OR of 1 << group over the
  slots of image i that hold v, full_i = the OR over all of its slots.  A hypothesis is beam_ref's plus met, a
  bitmask that starts at 0; logp is the sum of the model's token log-probabilities, nothing added.
  step   : a finished source j offers exactly (logp_j, j * V + 0) with met' = met_j; a live one (logp_j +
           logsoftmax[j][v], j * V + v) with met' = met_j | bits_i(v) for every v, except v == end_id while
           met_j != full_i.  bank = popcount(met'); rank = the position within the bank under (score descending,
           flat index ascending).  The k first under (rank ascending, bank descending) become beams 0 .. k - 1.
  update : beam_ref.step's, plus met = met'
  end    : per image the n_best under (popcount(met) descending, logp / max(len, 1)^alpha descending, beam
           ascending), met returned with them

`step` is one selection from given log-softmax rows, `search` runs it over a function that gives a source beam's
rows (diverse_ref.model_rows / constrained_rows / ensemble_rows), `finish` / `nbest` are the end.  The margin a
comparison with an f32 implementation needs is what decides the selection and nothing else: per step and image
the smallest gap between consecutive scores among the first (taken + 1) candidates of each bank, and at the end
the gaps between consecutive final scores of hypotheses with equal popcount(met)."""
import numpy as np

import beam_ref as R


def popcount(x):
    return np.vectorize(lambda m: bin(int(m)).count("1"), otypes=[np.int64])(np.asarray(x))


def slot_bits(word, group, V):
    """word / group [B, W] -> (bits [B, V] int64: bits_i(v), full [B])"""
    word, group = np.asarray(word), np.asarray(group)
    B = word.shape[0]
    bits = np.zeros((B, V), np.int64)
    for i in range(B):
        for w, g in zip(word[i], group[i]):
            if w >= 0:
                assert 0 <= w < V and 0 <= g < 16
                bits[i, w] |= 1 << int(g)
    return bits, np.bitwise_or.reduce(bits, axis=1) if V else np.zeros(B, np.int64)


def step(ls, logp, fin, length, met, k, end_id, word, group):
    """One selection.  ls [k_in, B, V] f64 log-softmax rows (rows of finished sources are never read), logp / fin
    / length / met [k_in, B], word / group [B, W].  -> dict(logp [k, B] f64, src, tok, fin, len, met [k, B]
    int64, bank [k, B]: popcount of the new met, advanced [k, B]: the selection met a new group, gap [B]: the
    smallest gap between consecutive scores among the first (taken + 1) candidates of any bank (inf where no
    bank has such a pair), banks [B]: the number of non-empty banks)"""
    k_in, B, V = ls.shape
    bits, full = slot_bits(word, group, V)
    out = {name: np.zeros((k, B), np.int64) for name in ("src", "tok", "fin", "len", "met", "bank", "advanced")}
    out.update(logp=np.empty((k, B)), gap=np.full(B, np.inf), banks=np.zeros(B, np.int64))
    for i in range(B):
        score, flat, new = [], [], []
        for j in range(k_in):
            if fin[j, i]:
                score.append(np.array([logp[j, i]], dtype=np.float64))
                flat.append(np.array([j * V], dtype=np.int64))
                new.append(np.array([met[j, i]], dtype=np.int64))
            else:
                keep = np.ones(V, bool)
                if 0 <= end_id < V and met[j, i] != full[i]:
                    keep[end_id] = False  # a hypothesis cannot end with a group unmet
                score.append((logp[j, i] + ls[j, i])[keep])
                flat.append((j * V + np.arange(V, dtype=np.int64))[keep])
                new.append((met[j, i] | bits[i])[keep])
        score, flat, new = np.concatenate(score), np.concatenate(flat), np.concatenate(new)
        assert score.size >= k, "a step needs at least k candidates"
        bank = popcount(new)
        lists = {}  # bank -> its candidates in order
        for b in np.unique(bank):
            at = np.nonzero(bank == b)[0]
            lists[int(b)] = at[np.lexsort((flat[at], -score[at]))]
        out["banks"][i] = len(lists)
        order, taken, rank = [], {b: 0 for b in lists}, 0
        while len(order) < k:
            for b in sorted(lists, reverse=True):
                if rank < lists[b].size and len(order) < k:
                    order.append(lists[b][rank])
                    taken[b] += 1
            rank += 1
        for b, n in taken.items():
            s = score[lists[b][:n + 1]]
            if s.size > 1:
                with np.errstate(invalid="ignore"):  # (-inf - -inf: two blocked words, no gap to speak of)
                    d = s[:-1] - s[1:]
                out["gap"][i] = min(out["gap"][i], np.nanmin(d) if not np.isnan(d).all() else np.inf)
        for r, at in enumerate(order):
            j, v = divmod(int(flat[at]), V)
            out["logp"][r, i], out["src"][r, i], out["tok"][r, i] = score[at], j, v
            out["met"][r, i], out["bank"][r, i] = new[at], bank[at]
            out["advanced"][r, i] = int(new[at] != met[j, i])
            if fin[j, i]:
                assert v == 0
                out["fin"][r, i], out["len"][r, i] = 1, length[j, i]
            else:
                out["fin"][r, i], out["len"][r, i] = int(v == end_id), length[j, i] + 1
    return out


def search(rows, B, T, V, k, end_id, word, group):
    """The search over rows(seq_j, t).  -> dict(seq [k, B, T] int64, logp [k, B] f64, len, fin, met [k, B],
    step_margin [B]: the smallest gap of any step, tok_logp [k, B, T - 1]: each appended token's
    log-probability (0 where the source was finished; NaN after a blocked word was forced), steps: the list of
    step dicts)"""
    seq = np.zeros((k, B, T), dtype=np.int64)
    seq[:, :, 0] = 1
    logp = np.zeros((k, B))
    fin, length, met = (np.zeros((k, B), np.int64) for _ in range(3))
    tok_logp, step_margin, steps = np.zeros((k, B, T - 1)), np.full(B, np.inf), []
    for t in range(T - 1):
        k_in = 1 if t == 0 else k
        ls = np.stack([rows(seq[j], t) for j in range(k_in)])
        st = step(ls, logp[:k_in], fin[:k_in], length[:k_in], met[:k_in], k, end_id, word, group)
        steps.append(st)
        step_margin = np.minimum(step_margin, st["gap"])
        src = st["src"]
        with np.errstate(invalid="ignore"):  # (a blocked forced word: -inf from then on, its gain NaN)
            gain = st["logp"] - np.take_along_axis(logp[:k_in], src, 0)
        seq = np.take_along_axis(seq, src[:, :, None], 0)  # row (j, i) <- row (src[j, i], i)
        seq[:, :, t + 1] = st["tok"]
        tok_logp = np.take_along_axis(tok_logp, src[:, :, None], 0)
        tok_logp[:, :, t] = gain
        logp, fin, length, met = st["logp"], st["fin"], st["len"], st["met"]
    return {"seq": seq, "logp": logp, "len": length, "fin": fin, "met": met, "step_margin": step_margin,
            "tok_logp": tok_logp, "steps": steps}


def finish(logp, length, met, alpha, n_best):
    """-> dict(order [n_best, B]: the beam at each rank, score / logp [n_best, B] f64, len, met [n_best, B],
    final_margin [B]: the smallest gap between consecutive final scores of hypotheses with equal popcount(met),
    over ALL k (inf where no two share a bank))"""
    k, B = logp.shape
    logp, length, met = np.asarray(logp, dtype=np.float64), np.asarray(length), np.asarray(met)
    s = logp if alpha == 0 else logp / np.maximum(length, 1).astype(np.float64) ** float(alpha)
    bank = popcount(met)
    order = np.stack([np.lexsort((np.arange(k), -s[:, i], -bank[:, i])) for i in range(B)], axis=1)  # [k, B]
    ss, bb = np.take_along_axis(s, order, 0), np.take_along_axis(bank, order, 0)
    margin = np.full(B, np.inf)
    for i in range(B):
        for r in range(k - 1):
            if bb[r, i] == bb[r + 1, i]:
                margin[i] = min(margin[i], ss[r, i] - ss[r + 1, i])
    top = order[:n_best]
    return {"order": top, "score": ss[:n_best], "logp": np.take_along_axis(logp, top, 0),
            "len": np.take_along_axis(length, top, 0), "met": np.take_along_axis(met, top, 0), "final_margin": margin}


def nbest(state, alpha, n_best):
    """finish on a search's state -> dict(ids [n_best, B, T], score, logp, len, met [n_best, B], margin [B] =
    min(step margin, final margin))"""
    f = finish(state["logp"], state["len"], state["met"], alpha, n_best)
    ids = np.take_along_axis(state["seq"], f["order"][:, :, None], 0)
    return {"ids": ids, "score": f["score"], "logp": f["logp"], "len": f["len"], "met": f["met"],
            "margin": np.minimum(state["step_margin"], f["final_margin"])}


def fixture_words(P64, cfg, feats, pos, k, W, C, end_id):
    """The fixture conditions' words: per image the model's step-0 log-softmax order (stable), without ids 0 and
    1, <END> and every id in the plain beam_ref search's k hypotheses of that image; the entries at positions
    3 .. 3 + W - 1 of what is left, slot s in group min(s, C - 1).  -> (word, group) int32 [B, W]"""
    import diverse_ref as D
    plain = R.search(P64, cfg, feats, pos, k, end_id)
    B, T = plain["seq"].shape[1], cfg.max_length
    start = np.ones((B, T), np.int64)
    ls0 = D.model_rows(P64, cfg, feats, pos)(start, 0)
    word, group = np.full((B, W), -1, np.int32), np.zeros((B, W), np.int32)
    for i in range(B):
        skip = {0, 1, end_id} | set(plain["seq"][:, i].reshape(-1).tolist())
        left = [int(v) for v in np.argsort(-ls0[i], kind="stable") if int(v) not in skip]
        word[i] = left[3:3 + W]
        group[i] = [min(s, C - 1) for s in range(W)]
    return word, group


def words_ok(ids, length, met, word, group, end_id):
    """every caption whose met is full contains a word of each group and ends no earlier than its last group
    was met; every met equals the mask rebuilt from the caption's own words (through len)"""
    ids, length, met = np.asarray(ids), np.asarray(length), np.asarray(met)
    n, B, T = ids.shape
    bits, full = slot_bits(word, group, int(max(ids.max(), np.asarray(word).max()) + 1))
    for r in range(n):
        for i in range(B):
            have = 0
            for t in range(1, int(length[r, i]) + 1):
                have |= int(bits[i, ids[r, i, t]])
                if ids[r, i, t] == end_id:
                    assert have == full[i], "ended with a group unmet"
            assert have == met[r, i], (r, i, have, met[r, i])
