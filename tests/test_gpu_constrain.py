"""The decode constraints on the GPU: constrain_logits through its C-ABI hook against the float64 restatement of
csrc/select.hip's definition (tests/constrain_ref.py) -- edited logits bit for bit, repaired slab stats --,
then the selection and sampling kernels on the edited logits, then capgen_beam_nbest / capgen_sample under
capgen_set_decode_constraints and the Python calls over them on the fixture weights.

Index results follow the project's margin rules: a selection is compared where the restatement alone says
that its candidates are far enough apart (asserted before the kernel runs); the conditions on the fixtures
are pinned in tests/test_constrain_host.py."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import constrain_ref as CR
import nucleus_ref as NU
import sampling_ref as S
from test_beam_host import C1_END, C2S_END
from test_constrain_host import BANNED, C1_SETTINGS, K, constrained_search
from test_gpu_beam_nbest import B, Tc, Tw, check_step, dev, fin_pattern, slab_stats, structural
from test_gpu_nucleus import check as check_nucleus, determined, run_nucleus
from test_gpu_sampling import DEV, MARGIN, P, call, engine

pytestmark = pytest.mark.gpu

ROWS = 6
ALPHABET = [5, 17, 18, 33, 2, 39, 20, 21, 9, 30, 12, 26]
END = 9  # the word that plays <END> in the kernel cases


def c_struct(c):
    from capgen import _lib
    return _lib.decode_constraints(c["n"], c["m"], c["end_id"], c["theta"], c["banned"])


def run_constrain(x, ids, t, c, stats=None):
    """the hook on logits x [R, V] (and stats [R, S, 2]) with histories ids [R, ld]; a guard row after every
    buffer must come back unchanged, and ids untouched.  -> (edited logits, stats or None), host f32"""
    R_, V = x.shape
    xg = np.concatenate([x, np.full((1, V), 7.5, np.float32)])
    ig = np.concatenate([ids, np.full((1, ids.shape[1]), -7, np.int32)])
    xd, idd, sd = dev(xg), dev(ig), None
    if stats is not None:
        sd = dev(np.concatenate([stats, np.full((1,) + stats.shape[1:], 7.5, np.float32)]))
    cs = c_struct(c)
    call("capgen_debug_constrain_logits", P(xd), P(sd), R_, V, P(idd), ids.shape[1], t, C.byref(cs), None)
    got = xd.cpu().numpy()
    assert (got[R_] == 7.5).all(), "the logits' guard row was written"
    assert np.array_equal(idd.cpu().numpy(), ig), "ids was written"
    out_s = None
    if sd is not None:
        out_s = sd.cpu().numpy()
        assert (out_s[R_] == 7.5).all(), "the stats' guard row was written"
        out_s = out_s[:R_]
    return got[:R_], out_s


@functools.lru_cache(maxsize=None)
def kernel_case(V, ld):
    """(logits f32 [6, V], histories int32 [6, ld]): small alphabets so that words repeat, row 0 holding
    word 5 three times, row 1 two words of slab 1, rows 3 to 5 words of the last (partial) slab, row 5 an id
    outside the vocabulary, and (ld = 80) row 2 every word of slab 1"""
    g = np.random.default_rng(1000 * ld + V)
    x = (3 * g.standard_normal((ROWS, V))).astype(np.float32)
    ids = np.zeros((ROWS, ld), np.int32)
    for r in range(ROWS):
        words = ALPHABET[:3 + 2 * r] + ([V - 1, V - 7] if r >= 3 else [])
        if r == 2 and ld == 80:
            words = list(range(16, 32)) + [5, 33]
        ids[r] = g.choice(words, size=ld)
    if ld == 80:
        ids[2, 1:17] = np.arange(16, 32)
    ids[0, 1:6] = [5, 17, 5, 17, 5]
    ids[1, 1:6] = [17, 18, 17, 33, 17]
    ids[5, 2] = V + 3
    ids[:, 0] = 1
    return x, ids


def banned_list(V, n_banned):
    if n_banned == 0:
        return ()
    if n_banned == 3:
        return (5, 17, 18)  # 5: also in the histories (penalised and blocked); 17, 18: one slab
    if V == 40:
        return tuple(list(range(16, 32)) * 6 + [3, 35, 3, 35])  # the middle slab, whole
    g = np.random.default_rng(V)
    return tuple([5] + g.choice(V, size=n_banned - 1).tolist())


def check_edit(x, ids, t, c, stats):
    R_, V = x.shape
    ref = CR.edit_rows(x, ids, t, c)
    got, got_s = run_constrain(x, ids, t, c, stats)
    what = f"V={V} ld={ids.shape[1]} t={t} {c}"
    # blocked = -inf, penalised = the f32 product or quotient, the rest untouched: all of it bit for bit
    assert np.array_equal(got.view(np.int32), ref.astype(np.float32).view(np.int32)), what
    plain, _ = run_constrain(x, ids, t, c, None)  # (stats == NULL: the same logits)
    assert np.array_equal(plain.view(np.int32), got.view(np.int32)), what
    n_touched = 0
    for r in range(R_):
        pen, blk = CR.touched(ids[r], t, c, V)
        slabs = {w >> 4 for w in list(pen) + list(blk)}
        n_touched += len(slabs)
        for s in range((V + 15) // 16):
            if s not in slabs:
                assert np.array_equal(got_s[r, s].view(np.int32), stats[r, s].view(np.int32)), (what, r, s)
                continue
            cols = ref[r, 16 * s:min(16 * s + 16, V)]
            mx = cols.max()
            if np.isneginf(mx):
                assert np.isneginf(got_s[r, s, 0]) and got_s[r, s, 1] == 0.0, (what, r, s, got_s[r, s])
            else:
                want = np.exp(cols - mx).sum()
                assert got_s[r, s, 0] == np.float32(mx), (what, r, s)
                assert abs(float(got_s[r, s, 1]) - want) <= 1e-6 * want, (what, r, s, got_s[r, s, 1], want)
    return ref, got_s, n_touched


@pytest.mark.parametrize("ld, t", [(7, 0), (7, 1), (7, 5), (80, 70)])
@pytest.mark.parametrize("V", [40, 1000])
def test_kernel_matches_restatement(V, ld, t):
    """constrain_logits_kernel: every combination of n in {0, 1, 2, 3}, m on / off, theta in {1, 1.3} and
    0 / 3 / 100 banned words; V = 40 has three slabs, the last one partial, ld = 80 makes the lanes stride"""
    x, ids = kernel_case(V, ld)
    stats = slab_stats(x)
    assert (ids[0, 1:6] == 5).sum() == 3
    touched = 0
    for n in (0, 1, 2, 3):
        for m in (0, 4):
            for theta in (1.0, 1.3):
                for n_banned in (0, 3, 100):
                    c = CR.constraints(n=n, m=m, end_id=END, theta=theta, banned=banned_list(V, n_banned))
                    ref, got_s, nt = check_edit(x, ids, t, c, stats)
                    touched += nt
                    if n_banned == 3:  # two blocked words in one slab, everywhere
                        assert np.isneginf(ref[:, [17, 18]]).all()
                    if n_banned == 3 and theta != 1.0 and t >= 1:  # penalised and blocked: it ends blocked
                        pen, blk = CR.touched(ids[0], t, c, V)
                        assert 5 in pen and 5 in blk and pen.count(5) == 1 and np.isneginf(ref[0, 5])
                    if m and t + 1 < m:
                        assert np.isneginf(ref[:, END]).all()
                    if V == 40 and (n_banned == 100 or (n == 1 and t == 70)):  # a slab with nothing left
                        assert np.isneginf(ref[2, 16:32]).all()
                        assert np.isneginf(got_s[2, 1, 0]) and got_s[2, 1, 1] == 0.0
    assert touched > 0


def test_kernel_rejects_bad_arguments():
    x, ids = kernel_case(40, 7)
    for kw, t, word in ((dict(n=-1), 2, "no_repeat_ngram"), (dict(m=-1, end_id=3), 2, "min_length"),
                        (dict(m=3), 2, "min_length"), (dict(end_id=40), 2, "end_id"), (dict(end_id=-2), 2, "end_id"),
                        (dict(theta=0.0), 2, "repetition_penalty"), (dict(theta=float("nan")), 2, "repetition_penalty"),
                        (dict(theta=float("inf")), 2, "repetition_penalty"), (dict(banned=(40,)), 2, "banned"),
                        (dict(banned=(-1,)), 2, "banned"), (dict(banned=(1,) * 1025), 2, "n_banned"),
                        (dict(n=2), 7, "ids_ld"), (dict(n=2), -1, "ids_ld")):
        with pytest.raises(RuntimeError, match=word):
            run_constrain(x, ids, t, CR.constraints(**kw))


# ---- the selection kernels on constrained logits -----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def step_case(V, k, pattern, t=3):
    """(logits f32 [k * B, V] (NaN rows where finished), histories, prev, fin, len, end_id, the settings, the
    restatement's step) of the first seed whose restatement has every gap >= 2e-4.  The histories are made of
    each row's own best words, so that the edits take candidates away from the selection."""
    fin = fin_pattern(pattern, k)
    for attempt in range(200):
        g = np.random.default_rng(7919 * attempt + 13 * V + 3 * k + len(pattern))
        x = (3 * g.standard_normal((k * B, V))).astype(np.float32)
        best = np.argsort(-x, axis=1)
        ids = np.zeros((k * B, Tc), np.int32)
        ids[:, 0] = 1
        ids[:, 1], ids[:, 2], ids[:, 3] = best[:, 0], best[:, 1], best[:, 0]  # after best[0] came best[1]
        ids[:, 4:] = g.integers(0, V, size=(k * B, Tc - 4))  # (past t: never read)
        prev = (-0.0437 * (np.arange(k * B) // B) - 0.0113 * g.random(k * B)).astype(np.float32)
        length = g.integers(0, 10, size=(k, B)).astype(np.int32)
        end_id = int(best[0, 2])
        c = CR.constraints(n=2, m=t + 2, end_id=end_id, theta=1.3, banned=tuple(int(w) for w in best[1, 3:6]))
        z = CR.edit_rows(x, ids, t, c)
        ls = R.log_softmax64(z.reshape(k, B, V))
        x[fin.reshape(-1) != 0] = np.nan
        ref = R.step(ls, prev.astype(np.float64).reshape(k, B), fin, length, k, end_id)
        if ref["gaps"].min() >= 2e-4:
            plain = R.step(R.log_softmax64(np.nan_to_num(x).reshape(k, B, V)), prev.astype(np.float64).reshape(k, B),
                           fin, length, k, end_id)
            assert (plain["tok"] != ref["tok"]).any(), "the edits change nothing"
            return x, ids, prev, fin, length, end_id, c, ref
    raise AssertionError(f"no draw with the margin for V={V} k={k} {pattern}")


@pytest.mark.parametrize("fused", [False, True], ids=["full_row", "fused_slab"])
@pytest.mark.parametrize("k", [3, 16])
@pytest.mark.parametrize("V", [40, 1000])
def test_step_on_constrained_logits(V, k, fused):
    """the hook, then capgen_debug_beam_step_ended on the edited logits (fused: and on the repaired stats):
    src / tok / fin / len exact and scores within 1e-5 of beam_ref.step on log_softmax64(edit(...))"""
    t, R_ = 3, k * B
    for pattern in ("none", "some"):
        x, ids, prev, fin, length, end_id, c, ref = step_case(V, k, pattern)
        assert ref["gaps"].min() >= 2e-4
        xd, idd, pd = dev(x), dev(ids), dev(prev)
        sd = dev(slab_stats(x)) if fused else None
        cs = c_struct(c)
        call("capgen_debug_constrain_logits", P(xd), P(sd), R_, V, P(idd), Tc, t, C.byref(cs), None)
        g = torch.Generator(device="cpu").manual_seed(V + k)
        seq_src = torch.randint(100, 10_000, (R_, Tw), generator=g, dtype=torch.int64).to(DEV)
        kv_src = torch.randint(100, 10_000, (R_, Tc), generator=g, dtype=torch.int32).to(DEV)
        seq_dst = torch.full((R_ + 1, Tw), -7, dtype=torch.int64, device=DEV)
        ids_dst = torch.full((R_ + 1, Tc), -7, dtype=torch.int32, device=DEV)
        kv_dst = torch.full((R_ + 1, Tc), -7, dtype=torch.int32, device=DEV)
        op = torch.full((R_ + 1,), 7.0, device=DEV)
        os_, ot, of, ol = (torch.full((R_ + 1,), -7, dtype=torch.int32, device=DEV) for _ in range(4))
        cv = torch.zeros(R_ * k, device=DEV)
        ci = torch.zeros(R_ * k, dtype=torch.int32, device=DEV)
        fd, ld = dev(fin.reshape(-1)), dev(length.reshape(-1))
        call("capgen_debug_beam_step_ended", P(xd), P(sd), P(pd), k, B, V, k, end_id, P(fd), P(ld), P(of), P(ol), P(cv),
             P(ci), P(op), P(os_), P(ot), P(seq_src), P(seq_dst), Tw, P(idd), P(ids_dst), P(kv_src), P(kv_dst), Tc, t,
             None)
        assert op[R_].item() == 7.0 and os_[R_].item() == -7 and ot[R_].item() == -7
        out = {"prob": op[:R_].cpu().numpy(), "src": os_[:R_].cpu().numpy(), "tok": ot[:R_].cpu().numpy(),
               "fin": of[:R_].cpu().numpy(), "len": ol[:R_].cpu().numpy()}
        check_step(f"V={V} k={k} fin={pattern} fused={fused}", out, ref, fin, k)
        live = fin[out["src"].reshape(k, B), np.arange(B)[None, :]] == 0
        z = CR.edit_rows(np.nan_to_num(x), ids, t, c).reshape(k, B, V)
        chosen = z[out["src"].reshape(k, B), np.arange(B)[None, :], out["tok"].reshape(k, B)]
        assert np.isfinite(chosen[live]).all(), "a blocked word was selected"
        if fused:  # the new rows' ids: the source row's history with the chosen token at column t + 1
            got_ids = ids_dst[:R_].cpu().numpy().reshape(k, B, Tc)
            assert np.array_equal(got_ids[:, :, t + 1], out["tok"].reshape(k, B))


# ---- the sampling kernels on constrained logits ------------------------------------------------------------
def edited_on_device(x, ids, t, c):
    xd, idd = dev(x), dev(ids)
    cs = c_struct(c)
    call("capgen_debug_constrain_logits", P(xd), None, x.shape[0], x.shape[1], P(idd), ids.shape[1], t, C.byref(cs), None)
    return xd


@pytest.mark.parametrize("V", [40, 1000])
def test_sampling_on_constrained_logits(V):
    """capgen_debug_sample_nucleus on the edited logits against sampling_ref / nucleus_ref fed the restatement's
    edited logits: tokens exact under the margin rules of test_gpu_sampling / test_gpu_nucleus, logp finite
    and within their bounds, no blocked word drawn"""
    x, ids = kernel_case(V, 7)
    t = 5
    c = CR.constraints(n=2, m=0, end_id=END, theta=1.3, banned=banned_list(V, 3))
    z = CR.edit_rows(x, ids, t, c)
    z32 = z.astype(np.float32)
    assert np.isneginf(z).any()
    xd = edited_on_device(x, ids, t, c)
    assert np.array_equal(xd.cpu().numpy().view(np.int32), z32.view(np.int32))
    noise = {}
    for top_k, top_p, temp in ((0, 1.0, 1.0), (5, 1.0, 0.7), (16, 1.0, 1.5), (0, 0.6, 1.0), (16, 0.9, 0.7)):
        inv_tau, site = S.inv_tau_of(temp), S.SITE0 + 2
        what = f"V={V} top_k={top_k} top_p={top_p} T={temp}"
        cand = S.candidates(z32, top_k)
        assert cand[1].min() >= MARGIN, what
        if top_p == 1.0:
            for seed in S.SEEDS:
                ref = S.sample(z32, inv_tau, top_k, seed, site, cand=cand)
                if ref["margin"].min() >= MARGIN:
                    break
            else:
                pytest.fail(what + ": no seed gives the margin")
            tok, lp, _ = run_nucleus(x, inv_tau, top_k, 1.0, seed, site, xd=xd)
            assert np.array_equal(tok, ref["token"]), what
            bound = 1e-5 * max(np.abs(ref["logp"]).max(), np.finfo(np.float32).tiny)
            assert np.abs(lp.astype(np.float64) - ref["logp"]).max() <= bound, what
        else:
            m = NU.masses(z32, inv_tau, top_k, cand=cand)
            seed, b = determined(z32, m, top_p, site, noise, what)
            tok, lp, cnt = run_nucleus(x, inv_tau, top_k, top_p, seed, site, xd=xd)
            check_nucleus(tok, lp, cnt, b, what)
        assert np.isfinite(lp).all() and (lp <= 0).all(), what
        assert np.isfinite(z[np.arange(ROWS), tok]).all(), what + ": a blocked word was drawn"


def test_constrained_draw_is_coupled_to_the_unconstrained_one():
    """theta = 1, top_k = 0, top_p = 1: the noise is the same, so wherever the unconstrained draw is not
    blocked the constrained draw is that token"""
    V, R_, t = 40, 37, 5
    g = np.random.default_rng(40)
    x = g.standard_normal((R_, V)).astype(np.float32)  # flat rows: the draws spread over the vocabulary
    ids = g.integers(0, V, size=(R_, 7)).astype(np.int32)
    c = CR.constraints(n=1, banned=(3, 4, 5, 6, 7, 8))
    z = CR.edit_rows(x, ids, t, c)
    xd = edited_on_device(x, ids, t, c)
    kept = dropped = 0
    for seed in S.SEEDS:
        for site in (S.SITE0, S.SITE0 + 7):
            plain = run_nucleus(x, 1.0, 0, 1.0, seed, site)[0]
            tok = run_nucleus(x, 1.0, 0, 1.0, seed, site, xd=xd)[0]
            free = np.isfinite(z[np.arange(R_), plain])
            assert np.array_equal(tok[free], plain[free])
            assert np.isfinite(z[np.arange(R_), tok]).all()
            kept, dropped = kept + int(free.sum()), dropped + int((~free).sum())
    assert kept > 0 and dropped > 0


# ---- the engine --------------------------------------------------------------------------------------------
# (test_gpu_sampling.engine keeps one engine per (fixture, dtype) for the whole run: the constraints are always
# switched off again)
@contextlib.contextmanager
def constrained(e, **kw):
    e.set_decode_constraints(**kw)
    try:
        yield
    finally:
        e.set_decode_constraints()


def violations(rows, n, m, end_id, banned):
    """rows: token lists (what a caption emitted).  -> how many break a constraint"""
    bad = 0
    for tok in rows:
        tok = [int(w) for w in tok]
        bad += bool((n and CR.repeats(tok, n)) or (m and end_id in tok[:m - 1]) or set(tok) & set(banned))
    return bad


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("name", sorted(C1_SETTINGS))
def test_engine_fp32_c1_matches_restatement(name, alpha):
    """beam_nbest under the settings of tests/test_constrain_host.py against constrain_ref.search + nbest, by
    the rule of test_gpu_beam_nbest.test_engine_fp32_c1_matches_restatement: m = max(1e-3, 4 delta), at most 2
    of 8 images left out, the rest exact on tokens / len and within 1e-3 on logp / score; no returned row of
    any image holds a repeated n-gram, an early <END> or a banned word"""
    e, cfg, f, p = engine("c1", "fp32")
    T = cfg.max_length
    _, c, st = constrained_search(name)
    ref = R.nbest(st, alpha, K)
    with constrained(e, no_repeat_ngram=c["n"], min_length=c["m"], end_id=C1_END, repetition_penalty=c["theta"],
                     banned=c["banned"]):
        ids, score, logp, length = structural(*e.beam_nbest(f, p, K, C1_END, alpha, K), C1_END, T)
    same = (ids == ref["ids"]).all(axis=2)
    delta = float(np.abs(logp - ref["logp"])[same].max()) if same.any() else float("inf")
    m = max(1e-3, 4 * delta)
    keep = ref["margin"] >= m
    print(f"{name} alpha={alpha}: delta {delta:.3e}, m {m:.3e}, smallest reference margin "
          f"{ref['margin'].min():.3e}, {int((~keep).sum())} of 8 images left out")
    assert (~keep).sum() <= 2
    assert np.array_equal(ids[:, keep], ref["ids"][:, keep])
    assert np.array_equal(length[:, keep], ref["len"][:, keep])
    assert np.abs(logp[:, keep] - ref["logp"][:, keep]).max() <= 1e-3
    assert np.abs(score[:, keep] - ref["score"][:, keep]).max() <= 1e-3
    rows = [ids[j, i, 1:1 + length[j, i]] for j in range(K) for i in range(8)]
    assert violations(rows, c["n"], c["m"], C1_END, c["banned"]) == 0


def test_engine_bf16_fused_step_equals_the_full_row_path(set_knob):
    """bf16, c2s, m = 5, n = 2, theta = 1.2: the fused slab step scores against the repaired slab stats, an
    engine created under CAPGEN_FUSED_BEAM_STEP=0 runs the full-row kernels on the same edited logits.
    Tokens, len and order equal, logp within 1e-4 (one exp-sum rounding per step against the restatement's
    margin 1.3e-3); every length is 5.  Fails if the stats repair is wrong or missing."""
    from capgen.engine import Engine
    from capgen.params import fixture_state_dict
    from golden_util import load_fixture
    kw = dict(no_repeat_ngram=2, min_length=5, end_id=C2S_END, repetition_penalty=1.2)
    e16, _, f, p = engine("c2s", "bf16")
    with constrained(e16, **kw):
        fused = e16.beam_nbest(f.bfloat16(), p, K, C2S_END, 1.0, K)
    cfg, seed, _ = load_fixture("c2s")
    set_knob("FUSED_BEAM_STEP", 0)
    e = Engine(cfg.replace(dtype="bf16"), DEV)
    try:
        e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
        e.set_training(False)
        e.set_decode_constraints(**kw)
        full = e.beam_nbest(f.bfloat16(), p, K, C2S_END, 1.0, K)
    finally:
        e.close()
    assert torch.equal(full[0], fused[0]) and torch.equal(full[3], fused[3])
    assert (full[2] - fused[2]).abs().max().item() <= 1e-4 and (full[1] - fused[1]).abs().max().item() <= 1e-4
    assert (fused[3] == 5).all()
    structural(*fused, C2S_END, cfg.max_length)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_engine_sample_respects_the_constraints(dtype):
    e, cfg, f, p = engine("c1", dtype)
    T = cfg.max_length
    x = f if dtype == "fp32" else f.bfloat16()
    plain = e.sample(x, p, n_samples=4, top_k=0, seed=21)
    with constrained(e, no_repeat_ngram=2, min_length=4, end_id=C1_END, banned=BANNED):
        a = e.sample(x, p, n_samples=4, top_k=0, seed=21)
        b = e.sample(x, p, n_samples=4, top_k=0, seed=21)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert torch.isfinite(a[1]).all() and (a[1] <= 0).all()
    # <END> is an ordinary word while sampling: the whole row is one history
    rows = a[0].view(-1, T + 1)[:, 1:T].cpu().numpy()
    assert violations(rows, 2, 4, C1_END, BANNED) == 0
    print(f"{dtype}: {violations(plain[0].view(-1, T + 1)[:, 1:T].cpu().numpy(), 2, 4, C1_END, BANNED)} of "
          f"{rows.shape[0]} unconstrained rows break a constraint")
    after = e.sample(x, p, n_samples=4, top_k=0, seed=21)
    assert torch.equal(after[0], plain[0]) and torch.equal(after[1].view(torch.int32), plain[1].view(torch.int32))


def test_constraints_off_and_unset_change_nothing():
    """a fresh engine: beam_nbest and sample after set(...) then set(NULL) equal the calls made before any
    setter call, bit for bit; greedy and beam are the same before, while constraints are set and after; the
    hazard log of a constrained beam_nbest holds no unordered conflicting pair"""
    from capgen import _lib
    from capgen.engine import Engine
    from capgen.params import fixture_state_dict
    from golden_util import load_fixture
    _, cfg, f, p = engine("c1", "fp32")
    _, seed, _ = load_fixture("c1")
    e = Engine(cfg.replace(dtype="fp32"), DEV)
    try:
        e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
        e.set_training(False)

        def everything():
            nb = e.beam_nbest(f, p, K, C1_END, 1.0, K)
            sm = e.sample(f, p, n_samples=2, seed=5)
            return [t.clone() for t in nb] + [sm[0].clone(), sm[1].clone().view(torch.int32)]

        def reference_decoders():
            return [e.greedy(f, p)[0].clone(), e.beam(f, p, K).clone()]

        before, ref_before = everything(), reference_decoders()
        e.set_decode_constraints(no_repeat_ngram=2, min_length=4, end_id=C1_END, repetition_penalty=1.2, banned=BANNED)
        assert all(torch.equal(x, y) for x, y in zip(reference_decoders(), ref_before))
        _lib.hazard_start()
        try:
            on = e.beam_nbest(f, p, K, C1_END, 1.0, K)
            torch.cuda.synchronize()
            n, report = _lib.hazard_check()
        finally:
            _lib.hazard_stop()
        assert n == 0, report
        assert not torch.equal(on[0], before[0])
        e.set_decode_constraints()
        assert all(torch.equal(x, y) for x, y in zip(everything(), before))
        assert all(torch.equal(x, y) for x, y in zip(reference_decoders(), ref_before))
    finally:
        e.close()


def test_python_api():
    from capgen.models import TRANSFORMER
    e, cfg, f, p = engine("c1", "fp32")
    words = {f"w{i}": i for i in range(cfg.num_vocab)}
    words.pop("w0"), words.pop("w1"), words.pop(f"w{C1_END}")
    words.update({"<NULL>": 0, "<START>": 1, "<END>": C1_END})
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=words, device=DEV, state_dict=e.state_dict())
    m.model.eval()
    banned_words = [f"w{w}" for w in BANNED] + ["<NULL>", "<START>"]
    banned = list(BANNED) + [0, 1]
    caps, score = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2, no_repeat_ngram=2, min_length=4,
                                  banned_words=banned_words)
    with constrained(e, no_repeat_ngram=2, min_length=4, end_id=C1_END, banned=banned):
        ids, want, _, length = e.beam_nbest(f, p, 3, C1_END, 1.0, 2)
    assert torch.equal(score.cpu(), want.cpu())
    assert caps[0] == m.decode_captions(ids[0].cpu().numpy()) and caps[1] == m.decode_captions(ids[1].cpu().numpy())
    assert (length >= 4).all()
    # nothing leaks into the next call, of the model or of its engine
    plain_caps, plain_score = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2)
    _, plain_want, _, _ = e.beam_nbest(f, p, 3, C1_END, 1.0, 2)
    assert torch.equal(plain_score.cpu(), plain_want.cpu()) and not torch.equal(plain_score.cpu(), score.cpu())
    with pytest.raises(ValueError, match="no_such_word"):
        m.beam_captions(f, p, beam_size=3, banned_words=["w5", "no_such_word"])
    with pytest.raises(RuntimeError, match="no_repeat_ngram"):  # the engine refuses: still switched off afterwards
        m.beam_captions(f, p, beam_size=3, no_repeat_ngram=cfg.max_length)
    again, _ = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2)
    assert again == plain_caps
    T = cfg.max_length
    s_caps, s_lp = m.sample_captions(f, p, n_samples=2, seed=3, no_repeat_ngram=2, banned_words=banned_words)
    with constrained(m.model.engine, no_repeat_ngram=2, banned=banned):
        c_ids, _ = m.model.sample_caption_vector(f, p, n_samples=2, seed=3)
    assert s_caps == [m.decode_captions(c_ids[j].cpu().numpy()) for j in range(2)]
    assert violations(c_ids.view(-1, T + 1)[:, 1:T].cpu().numpy(), 2, 0, C1_END, banned) == 0
    assert torch.isfinite(s_lp).all()


def test_bad_arguments_name_the_argument():
    e, cfg, f, p = engine("c1", "fp32")
    V, T = cfg.num_vocab, cfg.max_length
    cases = [(dict(no_repeat_ngram=-1), "no_repeat_ngram"), (dict(no_repeat_ngram=T), "no_repeat_ngram"),
             (dict(min_length=-1, end_id=5), "min_length"), (dict(min_length=T, end_id=5), "min_length"),
             (dict(min_length=3), "min_length"), (dict(no_repeat_ngram=2, end_id=V), "end_id"),
             (dict(no_repeat_ngram=2, end_id=-2), "end_id"), (dict(repetition_penalty=0.0), "repetition_penalty"),
             (dict(repetition_penalty=-1.0), "repetition_penalty"), (dict(repetition_penalty=float("nan")), "repetition_penalty"),
             (dict(repetition_penalty=float("inf")), "repetition_penalty"), (dict(banned=(V,)), "banned"),
             (dict(banned=(-1,)), "banned"), (dict(banned=(3,) * 1025), "n_banned"),
             (dict(banned=tuple(range(V - T - 15))), "num_vocab")]
    for kw, word in cases:
        with pytest.raises(RuntimeError, match=word):
            e.set_decode_constraints(**kw)
    try:
        e.set_decode_constraints(no_repeat_ngram=T - 1, min_length=T - 1, end_id=C1_END, banned=tuple(range(V - T - 16)))
        e.set_decode_constraints(min_length=4, end_id=C1_END)
        with pytest.raises(RuntimeError, match="end_id"):
            e.beam_nbest(f, p, K, 5, 0.0, 1)
        e.beam_nbest(f, p, K, C1_END, 0.0, 1)
        e.set_decode_constraints(no_repeat_ngram=2, end_id=C1_END)  # without min_length any end_id goes
        e.beam_nbest(f, p, K, 5, 0.0, 1)
    finally:
        e.set_decode_constraints()
