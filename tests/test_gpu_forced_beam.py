"""Forced-word beam search on the GPU: the forced step (beam_row_topk_kernel<ENDED, FORCED> with kf = min(16, k +
W + 1) finalists and the W slot-word scores per row, plus beam_forced_merge_kernel) through
capgen_debug_beam_forced_step against the float64 restatement of csrc/select.hip's definition
(tests/forced_ref.py), then capgen_beam_forced / capgen_ensemble_beam_forced and the Python calls over them on the
fixture weights.

Kernel cases are drawn from fixed seeds, tried in order until the restatement alone says that every two
consecutive scores among the first (taken + 1) candidates of every bank of every image lie at least 2e-4 apart;
1e-4, the project's margin for an f32 selection against an f64 one, is asserted before the kernel runs and no
image is ever left out."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import forced_ref as F
from test_beam_host import C1_END, C2S_END
from test_diverse_host import BANNED, CONSTRAINED, ENSEMBLE
from test_forced_host import BLOCKED_IMAGES, PINNED, fixture_slots, forced_search
from test_gpu_beam_nbest import B, dev, fin_pattern, run_step
from test_gpu_constrain import constrained, violations
from test_gpu_ensemble import members, same_bits
from test_gpu_sampling import DEV, MARGIN, P, call, engine

pytestmark = pytest.mark.gpu

KWC = ((3, 2, 2), (5, 4, 2), (8, 7, 3), (4, 11, 4), (14, 1, 1), (7, 8, 8))  # kf = 6, 10, 16, 16, 16, 16
VS = (40, 1000)
PATTERNS = ("none", "some", "all")
GROUP_ID = [(5 * c + 3) % 16 for c in range(16)]  # group c of a case sits at this bit: 3, 8, 13, 2, 7, ...


def kf_of(k, W):
    return min(16, k + W + 1)


def step_inputs(V, k, W, Cn, k_in, pattern, attempt):
    """test_gpu_beam_nbest.step_case's draw (logits, distinct prev per row, lengths, <END> = row 0's best word)
    plus the slots: image i's W words drawn from the best 3 W + 2 words of its row 0 (without <END>, 0 and 1) so
    that they compete, from W = 3 one word twice (two slots, two groups), image 1's last slot empty; met random
    within full_i for live rows, full_i for finished ones"""
    if pattern == "one":  # one finished row per image, row i % k_in: without prev it is alone at logp 0
        fin = (np.arange(k_in)[:, None] == np.arange(B)[None, :] % k_in).astype(np.int32)
    else:
        fin = fin_pattern(pattern, k_in)
    g = torch.Generator(device="cpu").manual_seed(7919 * attempt + 13 * V + 3 * k + k_in + len(pattern) + 101 * W)
    x = (3 * torch.randn(k_in * B, V, generator=g)).numpy()
    prev = (-0.0437 * (np.arange(k_in * B) // B) - 0.0113 * torch.rand(k_in * B, generator=g).numpy())
    prev = prev.astype(np.float32)
    length = torch.randint(0, 10, (k_in, B), generator=g).numpy().astype(np.int32)
    end_id = int(np.argmax(x[0]))
    rng = np.random.default_rng(1000 * attempt + 7 * V + k + W)
    word, group = np.full((B, W), -1, np.int32), np.zeros((B, W), np.int32)
    for i in range(B):
        pool = [int(v) for v in np.argsort(-x[i], kind="stable")[:3 * W + 2] if v not in (0, 1, end_id)]
        word[i] = rng.choice(pool, W, replace=False)
        group[i] = [GROUP_ID[c] for c in rng.integers(0, Cn, W)]
        group[i, :min(W, Cn)] = GROUP_ID[:min(W, Cn)]  # (every group of the case is used)
        if W >= 3:
            word[i, W - 2] = word[i, 0]
    word[1, W - 1] = -1
    _, full = F.slot_bits(word, group, V)
    met = (rng.integers(0, 1 << 16, (k_in, B)) & full[None]).astype(np.int32)
    met[fin != 0] = np.broadcast_to(full[None], (k_in, B))[fin != 0]
    return x, prev, fin, length, end_id, word, group, met


@functools.lru_cache(maxsize=None)
def step_case(V, k, W, Cn, k_in, pattern, with_prev=True):
    """(logits f32 [k_in * B, V] with NaN rows where finished, prev or None, fin, len, <END>, word, group, met,
    the restatement's step) of the first seed whose restatement has the margin"""
    for attempt in range(200):
        x, prev, fin, length, end_id, word, group, met = step_inputs(V, k, W, Cn, k_in, pattern, attempt)
        ls = R.log_softmax64(x.reshape(k_in, B, V))
        x[fin.reshape(-1) != 0] = np.nan
        p64 = prev.astype(np.float64).reshape(k_in, B) if with_prev else np.zeros((k_in, B))
        ref = F.step(ls, p64, fin, length, met, k, end_id, word, group)
        if ref["gap"].min() >= 2 * MARGIN:
            return x, (prev if with_prev else None), fin, length, end_id, word, group, met, ref
    raise AssertionError(f"no draw with the margin for V={V} k={k} W={W} C={Cn} k_in={k_in} {pattern}")


def step_cases(k):
    """(k_in, pattern, with_prev): one source row (step 0) is live"""
    yield 1, "none", True
    yield 1, "none", False
    for pattern in PATTERNS:
        yield k, pattern, True
    yield k, "none", False
    yield k, "one", False  # (several finished rows without prev would tie at logp 0: one per image does not)


def run_forced_step(x, prev, fin, length, met, word, group, k_in, V, k, end_id, W=None):
    """the hook with a guard element after every output; -> dict of host arrays"""
    W = word.shape[1] if W is None else W
    kf = kf_of(k, W) if W else k
    R_, Nv, Ni = k * B, k_in * B * (kf + W), k_in * B * kf
    op = torch.full((R_ + 1,), 7.0, device=DEV)
    os_, ot, of, ol, om = (torch.full((R_ + 1,), -7, dtype=torch.int32, device=DEV) for _ in range(5))
    cv = torch.full((Nv + 1,), 7.0, device=DEV)
    ci = torch.full((Ni + 1,), -7, dtype=torch.int32, device=DEV)
    xd, pd = dev(x), dev(prev)
    fd, ld, md = dev(fin.reshape(-1)), dev(length.reshape(-1)), dev(met.reshape(-1))
    wd, gd = dev(word.reshape(-1)), dev(group.reshape(-1))
    call("capgen_debug_beam_forced_step", P(xd), P(pd), k_in, B, V, k, end_id, P(wd), P(gd), W, P(fd), P(ld), P(md),
         P(of), P(ol), P(om), P(cv), P(ci), P(op), P(os_), P(ot), None)
    assert op[R_].item() == 7.0 and os_[R_].item() == -7 and ot[R_].item() == -7
    assert of[R_].item() == -7 and ol[R_].item() == -7 and om[R_].item() == -7
    assert cv[Nv].item() == 7.0 and ci[Ni].item() == -7
    assert torch.equal(fd.cpu(), torch.from_numpy(fin.reshape(-1))), "fin_src was written"
    assert torch.equal(ld.cpu(), torch.from_numpy(length.reshape(-1))), "len_src was written"
    assert torch.equal(md.cpu(), torch.from_numpy(met.reshape(-1))), "met_src was written"
    assert torch.equal(wd.cpu(), torch.from_numpy(word.reshape(-1))), "word was written"
    assert torch.equal(gd.cpu(), torch.from_numpy(group.reshape(-1))), "group was written"
    return {"prob": op[:R_].cpu().numpy(), "src": os_[:R_].cpu().numpy(), "tok": ot[:R_].cpu().numpy(),
            "fin": of[:R_].cpu().numpy(), "len": ol[:R_].cpu().numpy(), "met": om[:R_].cpu().numpy()}


def check_forced_step(tag, out, ref, fin, k):
    assert ref["gap"].min() >= MARGIN, tag + f": the restatement's own margin is {ref['gap'].min():.2e}"
    for name in ("src", "tok", "fin", "len", "met"):
        assert np.array_equal(out[name], ref[name].reshape(-1)), tag + " " + name
    err = np.abs(out["prob"].astype(np.float64) - ref["logp"].reshape(-1)).max()
    assert err <= 1e-5, tag + f": out_prob off the restatement's logp by {err:.2e}"
    from_fin = fin[out["src"].reshape(k, B), np.arange(B)[None, :]] != 0
    assert (out["tok"].reshape(k, B)[from_fin] == 0).all(), tag + ": a finished source appends token 0"


# ---- 1. the kernels against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("k, W, Cn", KWC)
@pytest.mark.parametrize("V", VS)
def test_forced_step_matches_restatement(V, k, W, Cn):
    """src / tok / fin / len / met exact, out_prob within 1e-5 of the restatement's logp; finished rows hold NaN
    logits; k_in = 1 and k, with and without prev"""
    for k_in, pattern, with_prev in step_cases(k):
        x, prev, fin, length, end_id, word, group, met, ref = step_case(V, k, W, Cn, k_in, pattern, with_prev)
        out = run_forced_step(x, prev, fin, length, met, word, group, k_in, V, k, end_id)
        check_forced_step(f"V={V} k={k} W={W} C={Cn} k_in={k_in} fin={pattern} prev={with_prev}", out, ref, fin, k)


def test_the_case_set_covers_advancing_selections_met_groups_and_four_banks():
    """on the restatement alone: some selection advances, some selected word belongs to a group its source had
    already met (and stays in its bank), and some image has at least 4 non-empty banks at once"""
    advanced, met_again, banks = 0, 0, 0
    for V in VS:
        for k, W, Cn in KWC:
            for k_in, pattern, with_prev in step_cases(k):
                _, _, fin, _, _, word, group, met, ref = step_case(V, k, W, Cn, k_in, pattern, with_prev)
                bits, _ = F.slot_bits(word, group, V)
                advanced += int(ref["advanced"].sum())
                banks = max(banks, int(ref["banks"].max()))
                for r in range(k):
                    for i in range(B):
                        j, v = ref["src"][r, i], ref["tok"][r, i]
                        if not fin[j, i] and bits[i, v] and not ref["advanced"][r, i]:
                            met_again += 1
    assert advanced > 0 and met_again > 0 and banks >= 4, (advanced, met_again, banks)


# ---- 2. the finalist bound ---------------------------------------------------------------------------------
def test_fourteen_beams_one_word_take_the_rows_ranks_three_to_fifteen():
    """k_in = 1, k = 14, W = 1, the word is the row's best and <END> its second: the selection is the word, then
    the row's ranks 3 to 15.  A kernel that keeps k finalists per row instead of k + W + 1 fails here."""
    k, W, word_id, end_id = 14, 1, 7, 5
    for V in VS:
        for attempt in range(200):
            g = torch.Generator(device="cpu").manual_seed(15485863 * attempt + V)
            x = (3 * torch.randn(B, V, generator=g)).numpy()
            for i in range(B):  # the row's best value to column 7, its second to column 5
                for rank, col in ((0, word_id), (1, end_id)):
                    at = int(np.argsort(-x[i], kind="stable")[rank])
                    x[i, at], x[i, col] = x[i, col], x[i, at]
            ls = R.log_softmax64(x)
            top = -np.sort(-ls, axis=1)[:, :17]
            if (top[:, :-1] - top[:, 1:]).min() >= 2 * MARGIN:
                break
        else:
            raise AssertionError("no draw with the margin")
        order = np.argsort(-ls, axis=1, kind="stable")
        assert (order[:, 0] == word_id).all() and (order[:, 1] == end_id).all()
        word, group = np.full((B, 1), word_id, np.int32), np.zeros((B, 1), np.int32)
        z = np.zeros((1, B), np.int32)
        ref = F.step(ls[None], np.zeros((1, B)), z, z, z, k, end_id, word, group)
        assert ref["gap"].min() >= MARGIN
        want = np.concatenate([order[:, :1], order[:, 2:15]], axis=1).T  # [rank, image]
        assert np.array_equal(ref["tok"], want) and (ref["met"][0] == 1).all() and not ref["met"][1:].any()
        out = run_forced_step(x.astype(np.float32), None, z, z, z, word, group, 1, V, k, end_id)
        check_forced_step(f"V={V} finalists", out, ref, z, k)
        assert np.array_equal(out["tok"].reshape(k, B), want)


# ---- 3. no words is the existing step and the existing call ------------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 8, 16])
def test_no_words_is_the_ended_step_bit_for_bit(k):
    """every slot -1 (W = 2), and no slot at all (W = 0): the hook takes the END-aware step's launches -- the
    row kernel's block size, and with it the order of its exp-sum, depends on the number of finalists -- at any
    k <= 16, and met comes back 0"""
    from test_gpu_beam_nbest import step_case as ended_case
    for V, W in ((V, W) for V in VS for W in (2, 0)):
        for k_in, pattern in ((1, "none"), (k, "some"), (k, "all")):
            x, prev, fin, length, end_id, _ = ended_case(V, k, k_in, pattern)
            word, group = np.full((B, 2), -1, np.int32), np.zeros((B, 2), np.int32)
            met = np.zeros((k_in, B), np.int32)
            a = run_forced_step(x, prev, fin, length, met, word, group, k_in, V, k, end_id, W=W)
            b = run_step(x, prev, fin, length, k_in, V, k, end_id, False)
            assert np.array_equal(a["prob"].view(np.int32), b["prob"].view(np.int32)), (V, k, k_in, pattern)
            for name in ("src", "tok", "fin", "len"):
                assert np.array_equal(a[name], b[name]), (V, k, k_in, pattern, name)
            assert not a["met"].any()


@pytest.mark.parametrize("k", [3, 5, 8])
def test_forced_kernels_on_images_without_words_select_what_the_ended_step_selects(k):
    """image 0 holds a word, so the hook launches the forced kernels; images 1 and 2 have every slot empty, and an
    image's selection reads only its own rows: their src / tok / fin / len are the END-aware step's and their
    out_prob its to 2e-6 (not bit for bit: the row kernel's exp-sum order follows the number of finalists), met 0"""
    from test_gpu_beam_nbest import step_case as ended_case
    for V in VS:
        for k_in, pattern in ((1, "none"), (k, "some"), (k, "all")):
            x, prev, fin, length, end_id, _ = ended_case(V, k, k_in, pattern)
            word, group = np.full((B, 2), -1, np.int32), np.zeros((B, 2), np.int32)
            word[0, 0] = 2 if end_id != 2 else 3
            met = np.zeros((k_in, B), np.int32)
            a = run_forced_step(x, prev, fin, length, met, word, group, k_in, V, k, end_id)
            b = run_step(x, prev, fin, length, k_in, V, k, end_id, False)
            empty = np.tile(np.arange(B) > 0, k)  # rows sel * B + i of images 1, 2
            for name in ("src", "tok", "fin", "len"):
                assert np.array_equal(a[name][empty], b[name][empty]), (V, k, k_in, pattern, name)
            assert np.abs(a["prob"][empty] - b["prob"][empty]).max() <= 2e-6, (V, k, k_in, pattern)  # (4 ulp at |score| < 8)
            assert not a["met"][empty].any()


def no_words(Bn, W=2):
    return np.full((Bn, W), -1, np.int32), np.zeros((Bn, W), np.int32)


@pytest.mark.parametrize("tag, dtype", [("c1", "fp32"), ("c2s", "fp32"), ("c2s", "bf16")])
def test_engine_without_words_is_beam_nbest_bit_for_bit(tag, dtype):
    e, cfg, f, p = engine(tag, dtype)
    end = C1_END if tag == "c1" else C2S_END
    f = f.bfloat16() if dtype == "bf16" else f
    want = e.beam_nbest(f, p, 5, end, 0.7, 3)
    for word, group in (no_words(f.shape[0]), no_words(f.shape[0], 0)):
        got = e.beam_forced(f, p, 5, end, word, group, 0.7, 3)
        assert same_bits(got[:4], want)
        assert all(x.shape == y.shape for x, y in zip(got, want))
        assert got[4].shape == want[3].shape and got[4].dtype == torch.int32 and not got[4].any()


# ---- 4. the engine against the restatement ---------------------------------------------------------------
def host(out):
    return [t.cpu().numpy() for t in out]


def structural(out, nb, end_id, T, word, group):
    ids, score, logp, length, met = host(out)
    R.structure_ok(ids, length, end_id, T)
    Bn = ids.shape[1]
    assert ids.shape == (nb, Bn, T) and score.shape == logp.shape == length.shape == met.shape == (nb, Bn)
    bank = F.popcount(met)
    assert (np.diff(bank, axis=0) <= 0).all(), "groups met increase down the list"
    with np.errstate(invalid="ignore"):
        down = np.diff(score, axis=0)
    assert (down[(np.diff(bank, axis=0) == 0) & ~np.isnan(down)] <= 0).all(), "scores increase within a bank"
    # every met is the mask of the caption's own words; one that is full ends no earlier than its last group
    F.words_ok(ids, length, met, word, group, end_id)
    return ids, score, logp, length, met


def absdiff(a, b):
    """|a - b| with equal infinities 0 apart"""
    with np.errstate(invalid="ignore"):
        d = np.abs(a - b)
    return np.where(a == b, 0.0, d)


def check_against(tag, got, ref, left_out=1):
    """the rule of test_gpu_diverse_beam.check_against, plus met"""
    ids, score, logp, length, met = got
    same = (ids == ref["ids"]).all(axis=2) & np.isfinite(ref["logp"])
    delta = float(absdiff(logp, ref["logp"])[same].max()) if same.any() else float("inf")
    m = max(1e-3, 4 * delta)
    keep = ref["margin"] >= m
    print(f"{tag}: delta {delta:.3e}, m {m:.3e}, smallest reference margin {ref['margin'].min():.3e}, "
          f"{int((~keep).sum())} of {keep.size} images left out")
    assert (~keep).sum() <= left_out
    assert np.array_equal(ids[:, keep], ref["ids"][:, keep])  # (tokens and their order down the list)
    assert np.array_equal(length[:, keep], ref["len"][:, keep])
    assert np.array_equal(met[:, keep], ref["met"][:, keep])
    assert absdiff(logp[:, keep], ref["logp"][:, keep]).max() <= 1e-3
    assert absdiff(score[:, keep], ref["score"][:, keep]).max() <= 1e-3


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("k, W, Cn", [key[1:] for key in sorted(PINNED) if key[0] == "c1"])
def test_engine_fp32_c1_matches_restatement(k, W, Cn, alpha):
    e, cfg, f, p = engine("c1", "fp32")
    _, word, group, st = forced_search("c1", k, W, Cn)
    ref = F.nbest(st, alpha, k)
    got = structural(e.beam_forced(f, p, k, C1_END, word, group, alpha, k), k, C1_END, cfg.max_length, word, group)
    check_against(f"k={k} W={W} C={Cn} alpha={alpha}", got, ref)
    _, full = F.slot_bits(word, group, cfg.num_vocab)
    assert (got[4][0] == full).all()  # the best caption of every image met every group


# ---- 5. logp is the model's ----------------------------------------------------------------------------------
def test_logp_is_the_models_log_probability():
    """score_captions of the returned ids gives the returned logp within 1e-3 (the bound the engine tests put on
    logp against float64) and the same len, at c1 (5, 2, 2): 16 of the 40 returned hypotheses met every group
    and all but the plain beam's were pulled up by their bank, yet nothing was added to logp"""
    e, cfg, f, p = engine("c1", "fp32")
    k, Bn = 5, f.shape[0]
    word, group = fixture_slots("c1", 5, 2, 2)
    ids, _, logp, length, met = e.beam_forced(f, p, k, C1_END, word, group, 0.0, k)
    assert int((F.popcount(met.cpu().numpy()) == 2).sum()) == PINNED[("c1", 5, 2, 2)][3]
    caps = ids.reshape(k * Bn, -1)
    idx = torch.arange(Bn, dtype=torch.int32, device=DEV).repeat(k)
    _, scored, slen, _ = e.score_captions(f, p, caps, img_idx=idx)
    err = (scored - logp.reshape(-1)).abs().max().item()
    print(f"c1 (5, 2, 2): returned logp against score_captions {err:.3e}")
    assert err <= 1e-3
    assert torch.equal(slen.cpu(), length.reshape(-1).cpu())


# ---- 6. bf16 ----------------------------------------------------------------------------------------------
def test_engine_bf16_c2s_finishes_like_fp32_and_repeats():
    """bf16, c2s, (3, 2, 2): structure always; tokens, len, met and order equal the fp32 engine's only if the
    measured bf16 error eps (2 x the largest bf16 - fp32 logit difference teacher-forced on the fp32 engine's
    sequences, as test_gpu_beam_nbest measures it) is below the restatement's margin 2.11e-3.
    This test's own print on an MI355X: "eps 6.811e-02, restatement margin 2.110e-03, tokens / len / met / order
    equal: False", so the equality is not asserted there.  Two bf16 calls must give the same bits."""
    e32, cfg, f, p = engine("c2s", "fp32")
    e16, _, _, _ = engine("c2s", "bf16")
    T, k = cfg.max_length, 3
    _, word, group, st = forced_search("c2s", 3, 2, 2)
    margin = float(F.nbest(st, 0.0, k)["margin"].min())
    assert abs(margin - PINNED[("c2s", 3, 2, 2)][0][0]) <= 1e-4
    r32 = e32.beam_forced(f, p, k, C2S_END, word, group, 0.0, k)
    r16 = e16.beam_forced(f.bfloat16(), p, k, C2S_END, word, group, 0.0, k)
    again = e16.beam_forced(f.bfloat16(), p, k, C2S_END, word, group, 0.0, k)
    assert same_bits(r16, again), "two calls differ"
    ids32, _, _, len32, met32 = structural(r32, k, C2S_END, T, word, group)
    ids16, _, _, len16, met16 = structural(r16, k, C2S_END, T, word, group)
    live = int(len32.max())
    eps = 0.0
    for j in range(k):  # teacher-forced on the fp32 engine's sequences (0 = <NULL> after <END>)
        caps = r32[0][j].to(torch.int32).contiguous()
        e32.forward(f, p, caps)
        l32 = e32.logits(caps.shape[0], T)[:, :live]
        e16.forward(f.bfloat16(), p, caps)
        l16 = e16.logits(caps.shape[0], T)[:, :live]
        eps = max(eps, 2.0 * (l16 - l32).abs().max().item())
    equal = np.array_equal(ids16, ids32) and np.array_equal(len16, len32) and np.array_equal(met16, met32)
    print(f"bf16 c2s: eps {eps:.3e}, restatement margin {margin:.3e}, tokens / len / met / order equal: {equal}")
    if eps < margin:
        assert equal


# ---- 7. constraints and ensembles ---------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_engine_under_constraints_matches_restatement(alpha):
    """CONSTRAINED bans the first forced word of images 4 and 7 (test_forced_host.BLOCKED_IMAGES): the blocked word
    scores -inf and still leads its bank, in the engine as in the restatement"""
    e, cfg, f, p = engine("c1", "fp32")
    k = 3
    _, word, group, st = forced_search("c1", 3, 2, 2, "constrained")
    ref = F.nbest(st, alpha, k)
    with constrained(e, no_repeat_ngram=CONSTRAINED["n"], end_id=C1_END, banned=CONSTRAINED["banned"]):
        got = structural(e.beam_forced(f, p, k, C1_END, word, group, alpha, k), k, C1_END, cfg.max_length, word, group)
    check_against(f"constrained alpha={alpha}", got, ref)
    ids, _, logp, length, _ = got
    assert tuple(np.nonzero(np.isneginf(logp).any(axis=0))[0]) == BLOCKED_IMAGES
    rows = [ids[j, i, 1:1 + length[j, i]] for j in range(k) for i in range(ids.shape[1]) if np.isfinite(logp[j, i])]
    assert violations(rows, CONSTRAINED["n"], 0, C1_END, BANNED) == 0


def test_one_member_ensemble_is_the_single_engine():
    from capgen.engine import ensemble_beam_forced
    e, cfg, f, p = engine("c1", "fp32")
    word, group = fixture_slots("c1", 3, 2, 2)
    want = e.beam_forced(f, p, 3, C1_END, word, group, 0.7, 3)
    for mode in ("prob", "logprob"):
        got = ensemble_beam_forced([e], f, p, 3, C1_END, word, group, 0.7, 3, mode=mode)
        assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3]) and torch.equal(got[4], want[4])
        assert (got[2] - want[2]).abs().max().item() <= 1e-4 and (got[1] - want[1]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_two_member_ensemble_matches_restatement(alpha):
    from capgen.engine import ensemble_beam_forced
    seeds, mode, w = ENSEMBLE
    es, cfg, f, p = members("c1", seeds)
    k = 3
    _, word, group, st = forced_search("c1", 3, 2, 2, "ensemble")
    ref = F.nbest(st, alpha, k)
    out = ensemble_beam_forced(es, f, p, k, C1_END, word, group, alpha, k, weights=w, mode=mode)
    check_against(f"ensemble alpha={alpha}", structural(out, k, C1_END, cfg.max_length, word, group), ref)


# ---- 8. arguments, hazards, the Python layer ------------------------------------------------------------
def test_bad_arguments_name_the_argument():
    from capgen import _lib
    lib = _lib.load()
    x, prev, fin, length, end_id, word, group, met, _ = step_case(40, 5, 4, 2, 5, "none")
    with pytest.raises(RuntimeError, match="beam_size \\+ words must be <= 15"):
        run_forced_step(x, prev, fin, length, met, np.tile(word, (1, 3)), np.tile(group, (1, 3)), 5, 40, 5, end_id)
    with pytest.raises(RuntimeError, match="words"):
        run_forced_step(x, prev, fin, length, met, word, group, 5, 40, 5, end_id, W=-1)
    with pytest.raises(RuntimeError, match="num_vocab"):
        run_forced_step(x[:, :9].copy(), prev, fin, length, met, word, group, 5, 9, 5, 3)
    with pytest.raises(RuntimeError, match="end_id"):
        run_forced_step(x, prev, fin, length, met, word, group, 5, 40, 5, 40)
    with pytest.raises(RuntimeError, match="k_in"):
        run_forced_step(x, prev, fin, length, met, word, group, 5, 40, 4, end_id)
    e, cfg, f, p = engine("c1", "fp32")
    Bi, N, T = f.shape[0], f.shape[1], cfg.max_length
    out = torch.zeros(16 * Bi, T, dtype=torch.int64, device=DEV)
    wd = torch.full((Bi, 16), -1, dtype=torch.int32, device=DEV)
    gd = torch.zeros((Bi, 16), dtype=torch.int32, device=DEV)

    def engine_err(k=5, W=2, end_id=5, alpha=0.0, n_best=1, n=N, word=wd, group=gd):
        rc = lib.capgen_beam_forced(e.h, P(f), _lib.F32, P(p), Bi, n, k, end_id, C.c_float(alpha), n_best,
                                    P(word) if word is not None else None, P(group) if group is not None else None, W,
                                    P(out), None, None, None, None, None)
        assert rc != 0
        return lib.capgen_last_error().decode()

    assert "beam_size" in engine_err(k=0) and "beam_size" in engine_err(k=17, W=0)
    assert "beam_forced: beam_size + words must be <= 15" in engine_err(k=5, W=11)
    assert "beam_size + words" in engine_err(k=14, W=2) and "words" in engine_err(W=-1)
    assert "word" in engine_err(word=None) and "group" in engine_err(group=None)
    assert "n_best" in engine_err(n_best=0) and "n_best" in engine_err(n_best=6)
    assert "end_id" in engine_err(end_id=-2) and "end_id" in engine_err(end_id=cfg.num_vocab)
    assert "length_penalty" in engine_err(alpha=-1.0) and "length_penalty" in engine_err(alpha=float("nan"))
    assert "N " in engine_err(n=65)
    with constrained(e, min_length=3, end_id=C1_END):
        assert "end_id" in engine_err(end_id=5)
    word, group = fixture_slots("c1", 3, 2, 2)
    with pytest.raises(ValueError, match="beam_size \\+ words"):
        e.beam_forced(f, p, 14, C1_END, word, group)
    with pytest.raises(ValueError, match="n_best"):
        e.beam_forced(f, p, 3, C1_END, word, group, n_best=4)
    with pytest.raises(ValueError, match="word"):
        e.beam_forced(f, p, 3, C1_END, np.where(word == word[0, 0], C1_END, word), group)
    with pytest.raises(ValueError, match="group"):
        e.beam_forced(f, p, 3, C1_END, word, group + 16)
    with pytest.raises(ValueError, match="word"):
        e.beam_forced(f, p, 3, C1_END, word[:4], group[:4])


def test_hazard_free_repeatable_and_python_api():
    e, cfg, f, p = engine("c1", "fp32")
    word, group = fixture_slots("c1", 3, 2, 2)
    a = e.beam_forced(f, p, 3, C1_END, word, group, 0.7, 2)
    from capgen import _lib
    _lib.hazard_start()
    try:
        b = e.beam_forced(f, p, 3, C1_END, word, group, 0.7, 2)
        torch.cuda.synchronize()
        n, report = _lib.hazard_check()
    finally:
        _lib.hazard_stop()
    assert n == 0, report
    assert same_bits(a, b)
    from capgen.ensemble import Ensemble
    from capgen.models import TRANSFORMER
    words = {f"w{i}": i for i in range(cfg.num_vocab)}
    words.pop("w0"), words.pop("w1"), words.pop(f"w{C1_END}")
    words.update({"<NULL>": 0, "<START>": 1, "<END>": C1_END})
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=words, device=DEV, state_dict=e.state_dict())
    m.model.eval()
    # slot s of the fixture sits in group s: one alternative per group; image 1 with both words in ONE group
    must = [[f"w{w}" for w in word[i]] for i in range(8)]
    caps, score = m.beam_captions(f, p, beam_size=3, length_penalty=0.7, n_best=2, must_include=must)
    assert len(caps) == 2 and all(len(c) == 8 and all(isinstance(s, str) for s in c) for c in caps)
    assert score.shape == (2, 8) and torch.equal(score.cpu(), a[1].cpu())
    assert caps[0] == m.decode_captions(a[0][0].cpu().numpy()) and caps[1] == m.decode_captions(a[0][1].cpu().numpy())
    for i in range(8):  # the best caption says both words
        assert all(f"w{w}" in caps[0][i].split() for w in word[i]), (i, caps[0][i])
    ids, _, _, _, met = m.model.beam_search_forced(f, p, 3, C1_END, word, group, length_penalty=0.7, n_best=2)
    assert torch.equal(ids, a[0]) and torch.equal(met, a[4])
    alt = [[tuple(f"w{w}" for w in word[i])] if i == 1 else must[i] for i in range(8)]
    alt[2] = []
    acaps, _ = m.beam_captions(f, p, beam_size=3, length_penalty=0.7, n_best=2, must_include=alt)
    w2, g2 = word.copy(), group.copy()
    g2[1], w2[2] = 0, -1
    want = e.beam_forced(f, p, 3, C1_END, w2, g2, 0.7, 2)
    assert acaps[0] == m.decode_captions(want[0][0].cpu().numpy())
    assert want[4][0, 1].item() == 1 and want[4][0, 2].item() == 0
    # the defaults are today's call: shapes and bits
    plain = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2)
    for none in (None, [[] for _ in range(8)]):
        same = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2, must_include=none)
        assert plain[0] == same[0] and torch.equal(plain[1], same[1]) and plain[1].shape == (2, 8)
    assert torch.equal(plain[1].cpu(), e.beam_nbest(f, p, 3, C1_END, 1.0, 2)[1].cpu())
    with pytest.raises(ValueError, match="must_include"):
        m.beam_captions(f, p, beam_size=3, must_include=[["nope"]] * 8)
    with pytest.raises(ValueError, match="must_include"):
        m.beam_captions(f, p, beam_size=6, num_groups=3, must_include=must)
    ens = Ensemble([m])
    ecaps, escore = ens.beam_captions(f, p, beam_size=3, length_penalty=0.7, n_best=2, must_include=must)
    assert ecaps == caps and (escore - score).abs().max().item() <= 1e-4
    with pytest.raises(ValueError, match="must_include"):
        ens.beam_captions(f, p, beam_size=3, must_include=must[:7])
