"""Diverse beam search on the GPU: the group step (beam_row_topk_kernel<ENDED> with k finalists per row plus
beam_group_merge_kernel) through capgen_debug_beam_group_step against the float64 restatement of
csrc/select.hip's definition (tests/diverse_ref.py), then capgen_beam_diverse / capgen_ensemble_beam_diverse and
the Python calls over them on the fixture weights.

Kernel cases are drawn from fixed seeds, tried in order until the restatement alone says that every two
consecutive penalised scores among the first k' + 1 candidates of every group of every image lie at least 2e-4
apart; 1e-4, the project's margin for an f32 selection against an f64 one, is asserted before the kernel runs and
no image is ever left out."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import diverse_ref as D
from test_beam_host import C1_END, C2S_END
from test_diverse_host import BANNED, CONSTRAINED, ENSEMBLE, PINNED, div_search
from test_gpu_beam_nbest import B, dev, fin_pattern, run_step
from test_gpu_constrain import constrained, violations
from test_gpu_ensemble import members, same_bits
from test_gpu_sampling import DEV, MARGIN, P, call, engine

pytestmark = pytest.mark.gpu

KGS = ((4, 2), (6, 3), (10, 2), (15, 3), (16, 2), (16, 16))  # every list width KM; k' = 2, 2, 5, 5, 8, 1
VS = (40, 1000)
LAMBDAS = (0.0, 0.3, 100.0)
PATTERNS = ("none", "some", "all")


def step_inputs(V, k, k_in, pattern, attempt):
    """test_gpu_beam_nbest.step_case's draw: logits, distinct prev per row, lengths, <END> = row 0's best word"""
    fin = fin_pattern(pattern, k_in)
    g = torch.Generator(device="cpu").manual_seed(7919 * attempt + 13 * V + 3 * k + k_in + len(pattern))
    x = (3 * torch.randn(k_in * B, V, generator=g)).numpy()
    prev = (-0.0437 * (np.arange(k_in * B) // B) - 0.0113 * torch.rand(k_in * B, generator=g).numpy())
    prev = prev.astype(np.float32)
    length = torch.randint(0, 10, (k_in, B), generator=g).numpy().astype(np.int32)
    return x, prev, fin, length, int(np.argmax(x[0]))


@functools.lru_cache(maxsize=None)
def step_case(V, k, G, lam, k_in, pattern, with_prev=True):
    """(logits f32 [k_in * B, V] with NaN rows where finished, prev or None, fin, len, <END>, the restatement's
    step) of the first seed whose restatement has the margin"""
    for attempt in range(200):
        x, prev, fin, length, end_id = step_inputs(V, k, k_in, pattern, attempt)
        ls = R.log_softmax64(x.reshape(k_in, B, V))
        x[fin.reshape(-1) != 0] = np.nan
        p64 = prev.astype(np.float64).reshape(k_in, B) if with_prev else np.zeros((k_in, B))
        ref = D.step(ls, p64, fin, length, k, G, float(np.float32(lam)), end_id)
        if ref["gaps"].min() >= 2 * MARGIN:
            return x, (prev if with_prev else None), fin, length, end_id, ref
    raise AssertionError(f"no draw with the margin for V={V} k={k} G={G} lam={lam} k_in={k_in} {pattern}")


def step_cases(k):
    """(k_in, pattern, with_prev): one source row (step 0) is live"""
    yield 1, "none", True
    yield 1, "none", False
    for pattern in PATTERNS:
        yield k, pattern, True
    yield k, "none", False  # (finished rows without prev would tie at logp 0)


def run_group_step(x, prev, fin, length, k_in, V, k, G, lam, end_id):
    """the hook with a guard element after every output; -> dict of host arrays"""
    R_, Nc = k * B, k_in * B * k
    op = torch.full((R_ + 1,), 7.0, device=DEV)
    os_, ot, of, ol = (torch.full((R_ + 1,), -7, dtype=torch.int32, device=DEV) for _ in range(4))
    cv = torch.full((Nc + 1,), 7.0, device=DEV)
    ci = torch.full((Nc + 1,), -7, dtype=torch.int32, device=DEV)
    xd, pd = dev(x), dev(prev)
    fd, ld = dev(fin.reshape(-1)), dev(length.reshape(-1))
    call("capgen_debug_beam_group_step", P(xd), P(pd), k_in, B, V, k, G, float(lam), end_id, P(fd), P(ld), P(of),
         P(ol), P(cv), P(ci), P(op), P(os_), P(ot), None)
    assert op[R_].item() == 7.0 and os_[R_].item() == -7 and ot[R_].item() == -7
    assert of[R_].item() == -7 and ol[R_].item() == -7 and cv[Nc].item() == 7.0 and ci[Nc].item() == -7
    assert torch.equal(fd.cpu(), torch.from_numpy(fin.reshape(-1))), "fin_src was written"
    assert torch.equal(ld.cpu(), torch.from_numpy(length.reshape(-1))), "len_src was written"
    return {"prob": op[:R_].cpu().numpy(), "src": os_[:R_].cpu().numpy(), "tok": ot[:R_].cpu().numpy(),
            "fin": of[:R_].cpu().numpy(), "len": ol[:R_].cpu().numpy()}


def check_group_step(tag, out, ref, fin, k):
    assert ref["gaps"].min() >= MARGIN, tag + f": the restatement's own margin is {ref['gaps'].min():.2e}"
    for name in ("src", "tok", "fin", "len"):
        assert np.array_equal(out[name], ref[name].reshape(-1)), tag + " " + name
    err = np.abs(out["prob"].astype(np.float64) - ref["logp"].reshape(-1)).max()
    assert err <= 1e-5, tag + f": out_prob off the unpenalised logp by {err:.2e}"
    from_fin = fin[out["src"].reshape(k, B), np.arange(B)[None, :]] != 0
    assert (out["tok"].reshape(k, B)[from_fin] == 0).all(), tag + ": a finished source appends token 0"


# ---- 1. the kernels against the restatement --------------------------------------------------------------
@pytest.mark.parametrize("k, G", KGS)
@pytest.mark.parametrize("V", VS)
def test_group_step_matches_restatement(V, k, G):
    """src / tok / fin / len exact, out_prob within 1e-5 of the restatement's unpenalised logp; finished rows
    hold NaN logits; k_in = 1 and k, with and without prev"""
    for lam in LAMBDAS:
        for k_in, pattern, with_prev in step_cases(k):
            x, prev, fin, length, end_id, ref = step_case(V, k, G, lam, k_in, pattern, with_prev)
            out = run_group_step(x, prev, fin, length, k_in, V, k, G, lam, end_id)
            check_group_step(f"V={V} k={k} G={G} lam={lam} k_in={k_in} fin={pattern} prev={with_prev}", out, ref, fin, k)
            if lam == 100.0 and k_in == 1 and k // G == 1:
                assert len(set(out["tok"].reshape(k, B)[:, 0].tolist())) == k


def test_the_case_set_covers_counts_of_two_and_a_finished_group():
    """on the restatement alone: some selected or displaced candidate has c >= 2, some selected candidate was
    penalised, and some group has only finished sources"""
    cmax, cnt, fin_group = 0, 0, False
    for V in VS:
        for k, G in KGS:
            for lam in LAMBDAS:
                for k_in, pattern, with_prev in step_cases(k):
                    _, _, fin, _, _, ref = step_case(V, k, G, lam, k_in, pattern, with_prev)
                    cmax, cnt = max(cmax, int(ref["cmax"].max())), max(cnt, int(ref["count"].max()))
                    if k_in == k:
                        fin_group |= bool(fin.reshape(G, k // G, B).all(axis=1).any())
    assert cmax >= 2 and cnt >= 2 and fin_group, (cmax, cnt, fin_group)


# ---- 2. the top-(k' + |S|) bound is tight ----------------------------------------------------------------------
def test_sixteen_groups_on_equal_rows_take_the_rows_sixteen_best_in_order():
    """k = G = 16, lambda = 100, all 16 source rows of an image hold the same logits and distinct prev: group g
    takes the row's rank-g token from its own source.  A kernel that keeps fewer than k finalists per row
    fails here, and nowhere smaller."""
    k = G = 16
    for V in VS:
        for attempt in range(200):
            g = torch.Generator(device="cpu").manual_seed(104729 * attempt + V)
            row = (3 * torch.randn(B, V, generator=g)).numpy()
            ls = R.log_softmax64(row)
            top = -np.sort(-ls, axis=1)[:, :17]
            if (top[:, :-1] - top[:, 1:]).min() >= 2 * MARGIN:
                break
        else:
            raise AssertionError("no draw with the margin")
        assert (top[:, :-1] - top[:, 1:]).min() >= MARGIN
        x = np.tile(row, (k, 1)).astype(np.float32)  # rows j * B + i = image i's row, for every j
        prev = (-0.05 * np.arange(k * B)).astype(np.float32)
        fin, length = np.zeros((k, B), np.int32), np.full((k, B), 2, np.int32)
        ref = D.step(np.tile(ls[None], (k, 1, 1)), prev.astype(np.float64).reshape(k, B), fin, length, k, G, 100.0, -1)
        assert ref["gaps"].min() >= MARGIN
        want = np.argsort(-ls, axis=1, kind="stable")[:, :16].T  # [rank, image]
        assert np.array_equal(ref["tok"], want) and np.array_equal(ref["src"], np.arange(k)[:, None].repeat(B, 1))
        out = run_group_step(x, prev, fin, length, k, V, k, G, 100.0, -1)
        check_group_step(f"V={V} tight", out, ref, fin, k)
        assert np.array_equal(out["tok"].reshape(k, B), want)


# ---- 3. one group is the existing step and the existing call ----------------------------------------------
@pytest.mark.parametrize("k", [3, 5, 8, 16])
def test_one_group_is_the_ended_step_bit_for_bit(k):
    from test_gpu_beam_nbest import step_case as ended_case
    for V in VS:
        for k_in, pattern in ((1, "none"), (k, "some"), (k, "all")):
            x, prev, fin, length, end_id, _ = ended_case(V, k, k_in, pattern)
            a = run_group_step(x, prev, fin, length, k_in, V, k, 1, 0.7, end_id)
            b = run_step(x, prev, fin, length, k_in, V, k, end_id, False)
            assert np.array_equal(a["prob"].view(np.int32), b["prob"].view(np.int32)), (V, k, k_in, pattern)
            for name in ("src", "tok", "fin", "len"):
                assert np.array_equal(a[name], b[name]), (V, k, k_in, pattern, name)


@pytest.mark.parametrize("tag, dtype", [("c1", "fp32"), ("c2s", "fp32"), ("c2s", "bf16")])
def test_engine_with_one_group_is_beam_nbest_bit_for_bit(tag, dtype):
    e, cfg, f, p = engine(tag, dtype)
    end = C1_END if tag == "c1" else C2S_END
    f = f.bfloat16() if dtype == "bf16" else f
    want = e.beam_nbest(f, p, 5, end, 0.7, 3)
    got = e.beam_diverse(f, p, 5, 1, 0.7, end, 0.7, 3)
    assert same_bits(got, want)
    assert all(x.shape == y.shape for x, y in zip(got, want))


# ---- 4. the engine against the restatement ---------------------------------------------------------------
def host(out):
    return [t.cpu().numpy() for t in out]


def structural(out, G, nb, end_id, T):
    ids, score, logp, length = host(out)
    R.structure_ok(ids, length, end_id, T)
    Bn = ids.shape[1]
    assert ids.shape == (G * nb, Bn, T) and score.shape == logp.shape == length.shape == (G * nb, Bn)
    assert (np.diff(score.reshape(G, nb, Bn), axis=1) <= 0).all(), "scores increase down a group's list"
    return ids, score, logp, length


def check_against(tag, got, ref, left_out=2):
    """the rule of test_gpu_beam_nbest.test_engine_fp32_c1_matches_restatement"""
    ids, score, logp, length = got
    same = (ids == ref["ids"]).all(axis=2)
    delta = float(np.abs(logp - ref["logp"])[same].max()) if same.any() else float("inf")
    m = max(1e-3, 4 * delta)
    keep = ref["margin"] >= m
    print(f"{tag}: delta {delta:.3e}, m {m:.3e}, smallest reference margin {ref['margin'].min():.3e}, "
          f"{int((~keep).sum())} of {keep.size} images left out")
    assert (~keep).sum() <= left_out
    assert np.array_equal(ids[:, keep], ref["ids"][:, keep])  # (tokens and their order down each group's list)
    assert np.array_equal(length[:, keep], ref["len"][:, keep])
    assert np.abs(logp[:, keep] - ref["logp"][:, keep]).max() <= 1e-3
    assert np.abs(score[:, keep] - ref["score"][:, keep]).max() <= 1e-3


@pytest.mark.parametrize("alpha", [0.0, 1.0])
@pytest.mark.parametrize("k, G, lam", [key[1:] for key in sorted(PINNED) if key[0] == "c1"])
def test_engine_fp32_c1_matches_restatement(k, G, lam, alpha):
    e, cfg, f, p = engine("c1", "fp32")
    kg = k // G
    ref = D.nbest(div_search("c1", k, G, lam)[1], G, alpha, kg)
    got = structural(e.beam_diverse(f, p, k, G, lam, C1_END, alpha, kg), G, kg, C1_END, cfg.max_length)
    check_against(f"k={k} G={G} lam={lam} alpha={alpha}", got, ref)


# ---- 5. logp is the model's ----------------------------------------------------------------------------------
@pytest.mark.parametrize("k, G, lam", [(4, 4, 1.0), (6, 3, 0.5)])
def test_logp_is_the_models_log_probability(k, G, lam):
    """score_captions of the returned ids gives the returned logp within 1e-3 (the bound the engine tests put on
    logp against float64).  At (6, 3, 0.5) 20 of the 48 returned hypotheses were penalised at some step (the
    restatement, pinned in test_diverse_host.PINNED): a penalised sum would be off by >= 0.5.  At (4, 4, 1.0)
    the restatement finds no returned hypothesis that was: on these weights no word leads its row by 1.0."""
    e, cfg, f, p = engine("c1", "fp32")
    kg, Bn = k // G, f.shape[0]
    nb = D.nbest(div_search("c1", k, G, lam)[1], G, 0.0, kg)
    n_pen = int((nb["penalty"] > 0).sum())
    assert n_pen == PINNED[("c1", k, G, lam)][5]
    if (k, G, lam) == (6, 3, 0.5):
        assert n_pen > 0 and nb["penalty"][nb["penalty"] > 0].min() >= lam
    ids, _, logp, length = e.beam_diverse(f, p, k, G, lam, C1_END, 0.0, kg)
    caps = ids.reshape(k * Bn, -1)
    idx = torch.arange(Bn, dtype=torch.int32, device=DEV).repeat(k)
    _, scored, slen, _ = e.score_captions(f, p, caps, img_idx=idx)
    err = (scored - logp.reshape(-1)).abs().max().item()
    print(f"k={k} G={G} lam={lam}: returned logp against score_captions {err:.3e}; penalised in the restatement {n_pen}")
    assert err <= 1e-3
    assert torch.equal(slen.cpu(), length.reshape(-1).cpu())


# ---- 6. bf16 ----------------------------------------------------------------------------------------------
def test_engine_bf16_c2s_finishes_like_fp32_and_repeats():
    """bf16, c2s, (6, 3, 1.0): structure always; tokens, len and order equal the fp32 engine's only if the
    measured bf16 error eps (2 x the largest bf16 - fp32 logit difference teacher-forced on the fp32 engine's
    sequences, as test_gpu_beam_nbest measures it) is below the restatement's margin 0.0154.
    Measured on an MI355X: eps 6.8e-2 against the margin 1.54e-2, so the equality is not asserted there (the
    two engines' tokens, len and order were nevertheless equal).  Two bf16 calls must give the same bits."""
    e32, cfg, f, p = engine("c2s", "fp32")
    e16, _, _, _ = engine("c2s", "bf16")
    T, k, G, lam = cfg.max_length, 6, 3, 1.0
    kg = k // G
    margin = float(D.nbest(div_search("c2s", k, G, lam)[1], G, 0.0, kg)["margin"].min())
    assert abs(margin - PINNED[("c2s", k, G, lam)][1]) <= 1e-3
    r32 = e32.beam_diverse(f, p, k, G, lam, C2S_END, 0.0, kg)
    r16 = e16.beam_diverse(f.bfloat16(), p, k, G, lam, C2S_END, 0.0, kg)
    again = e16.beam_diverse(f.bfloat16(), p, k, G, lam, C2S_END, 0.0, kg)
    assert same_bits(r16, again), "two calls differ"
    ids32, _, _, len32 = structural(r32, G, kg, C2S_END, T)
    ids16, _, _, len16 = structural(r16, G, kg, C2S_END, T)
    live = int(len32.max())
    eps = 0.0
    for j in range(k):  # teacher-forced on the fp32 engine's sequences (0 = <NULL> after <END>)
        caps = r32[0][j].to(torch.int32).contiguous()
        e32.forward(f, p, caps)
        l32 = e32.logits(caps.shape[0], T)[:, :live]
        e16.forward(f.bfloat16(), p, caps)
        l16 = e16.logits(caps.shape[0], T)[:, :live]
        eps = max(eps, 2.0 * (l16 - l32).abs().max().item())
    equal = np.array_equal(ids16, ids32) and np.array_equal(len16, len32)
    print(f"bf16 c2s: eps {eps:.3e}, restatement margin {margin:.3e}, tokens / len / order equal: {equal}")
    if eps < margin:
        assert equal


# ---- 7. constraints and ensembles ---------------------------------------------------------------------
@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_engine_under_constraints_matches_restatement(alpha):
    e, cfg, f, p = engine("c1", "fp32")
    k, G, lam, kg = 4, 2, 0.5, 2
    ref = D.nbest(div_search("c1", k, G, lam, "constrained")[1], G, alpha, kg)
    with constrained(e, no_repeat_ngram=CONSTRAINED["n"], end_id=C1_END, banned=CONSTRAINED["banned"]):
        got = structural(e.beam_diverse(f, p, k, G, lam, C1_END, alpha, kg), G, kg, C1_END, cfg.max_length)
    check_against(f"constrained alpha={alpha}", got, ref)
    ids, _, _, length = got
    rows = [ids[j, i, 1:1 + length[j, i]] for j in range(k) for i in range(ids.shape[1])]
    assert violations(rows, CONSTRAINED["n"], 0, C1_END, BANNED) == 0


def test_one_member_ensemble_is_the_single_engine():
    from capgen.engine import ensemble_beam_diverse
    e, cfg, f, p = engine("c1", "fp32")
    want = e.beam_diverse(f, p, 6, 3, 0.5, C1_END, 0.7, 2)
    for mode in ("prob", "logprob"):
        got = ensemble_beam_diverse([e], f, p, 6, 3, 0.5, C1_END, 0.7, 2, mode=mode)
        assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
        assert (got[2] - want[2]).abs().max().item() <= 1e-4 and (got[1] - want[1]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("alpha", [0.0, 1.0])
def test_two_member_ensemble_matches_restatement(alpha):
    from capgen.engine import ensemble_beam_diverse
    seeds, mode, w = ENSEMBLE
    es, cfg, f, p = members("c1", seeds)
    k, G, lam, kg = 4, 2, 0.5, 2
    ref = D.nbest(div_search("c1", k, G, lam, "ensemble")[1], G, alpha, kg)
    out = ensemble_beam_diverse(es, f, p, k, G, lam, C1_END, alpha, kg, weights=w, mode=mode)
    check_against(f"ensemble alpha={alpha}", structural(out, G, kg, C1_END, cfg.max_length), ref)


# ---- 8. arguments, hazards, the Python layer ------------------------------------------------------------
def test_bad_arguments_name_the_argument():
    from capgen import _lib
    lib = _lib.load()
    x, prev, fin, length, end_id, _ = step_case(40, 6, 3, 0.3, 6, "none")
    for G, lam, word in ((0, 0.3, "num_groups"), (4, 0.3, "num_groups"), (7, 0.3, "num_groups"),
                         (3, -0.1, "diversity_penalty"), (3, float("nan"), "diversity_penalty"),
                         (3, float("inf"), "diversity_penalty")):
        with pytest.raises(RuntimeError, match=word):
            run_group_step(x, prev, fin, length, 6, 40, 6, G, lam, end_id)
    with pytest.raises(RuntimeError, match="end_id"):
        run_group_step(x, prev, fin, length, 6, 40, 6, 3, 0.3, 40)
    with pytest.raises(RuntimeError, match="k_in"):
        run_group_step(x[:3 * B], prev[:3 * B], fin[:3], length[:3], 3, 40, 6, 3, 0.3, end_id)
    e, cfg, f, p = engine("c1", "fp32")
    Bi, N, T = f.shape[0], f.shape[1], cfg.max_length
    out = torch.zeros(16 * Bi, T, dtype=torch.int64, device=DEV)

    def engine_err(k=6, G=3, lam=0.5, end_id=5, alpha=0.0, n_best=1, n=N):
        rc = lib.capgen_beam_diverse(e.h, P(f), _lib.F32, P(p), Bi, n, k, G, C.c_float(lam), end_id, C.c_float(alpha),
                                     n_best, P(out), None, None, None, None)
        assert rc != 0
        return lib.capgen_last_error().decode()

    assert "beam_size" in engine_err(k=0, G=1) and "beam_size" in engine_err(k=17, G=1)
    assert "num_groups" in engine_err(G=0) and "num_groups" in engine_err(G=4) and "num_groups" in engine_err(G=7)
    for lam in (-0.5, float("nan"), float("inf")):
        assert "diversity_penalty" in engine_err(lam=lam)
    assert "n_best" in engine_err(n_best=0) and "n_best" in engine_err(n_best=3)
    assert "end_id" in engine_err(end_id=-2) and "end_id" in engine_err(end_id=cfg.num_vocab)
    assert "length_penalty" in engine_err(alpha=-1.0) and "length_penalty" in engine_err(alpha=float("nan"))
    assert "N " in engine_err(n=65)
    with constrained(e, min_length=3, end_id=C1_END):
        assert "end_id" in engine_err(end_id=5)
    with pytest.raises(ValueError, match="num_groups"):
        e.beam_diverse(f, p, 6, 4, 0.5, C1_END)
    with pytest.raises(ValueError, match="n_best"):
        e.beam_diverse(f, p, 6, 3, 0.5, C1_END, n_best=3)
    with pytest.raises(ValueError, match="diversity_penalty"):
        e.beam_diverse(f, p, 6, 3, -1.0, C1_END)


def test_hazard_free_repeatable_and_python_api():
    e, cfg, f, p = engine("c1", "fp32")
    a = e.beam_diverse(f, p, 6, 3, 0.5, C1_END, 0.7, 2)
    from capgen import _lib
    _lib.hazard_start()
    try:
        b = e.beam_diverse(f, p, 6, 3, 0.5, C1_END, 0.7, 2)
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
    caps, score = m.beam_captions(f, p, beam_size=6, length_penalty=0.7, n_best=2, num_groups=3, diversity_penalty=0.5)
    assert len(caps) == 6 and all(len(c) == 8 and all(isinstance(s, str) for s in c) for c in caps)
    assert score.shape == (6, 8) and torch.equal(score.cpu(), a[1].cpu())
    assert caps[2] == m.decode_captions(a[0][2].cpu().numpy())  # (group 1's best: row 1 * n_best + 0)
    ids, _, _, _ = m.model.beam_search_diverse(f, p, 6, 3, 0.5, C1_END, length_penalty=0.7, n_best=2)
    assert torch.equal(ids, a[0])
    # the defaults are today's call: shapes and bits
    plain = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2)
    same = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2, num_groups=1, diversity_penalty=0.0)
    assert plain[0] == same[0] and torch.equal(plain[1], same[1]) and plain[1].shape == (2, 8)
    assert torch.equal(plain[1].cpu(), e.beam_nbest(f, p, 3, C1_END, 1.0, 2)[1].cpu())
    with pytest.raises(ValueError, match="num_groups"):
        m.beam_captions(f, p, beam_size=6, num_groups=4)
    ens = Ensemble([m])
    ecaps, escore = ens.beam_captions(f, p, beam_size=6, length_penalty=0.7, n_best=2, num_groups=3,
                                      diversity_penalty=0.5)
    assert ecaps == caps and (escore - score).abs().max().item() <= 1e-4
    with pytest.raises(ValueError, match="diversity_penalty"):
        ens.beam_captions(f, p, beam_size=6, num_groups=3, diversity_penalty=float("nan"))
