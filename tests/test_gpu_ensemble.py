"""Ensemble decoding on the GPU: the fusing kernel (ensemble_combine, through its C-ABI hook) against the
float64 restatement (tests/ensemble_ref.py), then capgen_ensemble_beam_nbest / capgen_ensemble_sample and the
Python calls over them on the fixture weights, members fixture_state_dict(cfg, seed=s).

The engine comparisons follow the rules of test_gpu_beam_nbest.py and test_gpu_sampling.py; the conditions they
rest on are pinned, on the restatement alone, in tests/test_ensemble_host.py."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import beam_ref as R
import ensemble_ref as E
import sampling_ref as S
from capgen.params import fixture_state_dict
from golden_util import load_fixture
from test_ensemble_host import END, ens_search
from test_gpu_constrain import constrained, violations
from test_gpu_sampling import DEV, P, engine

pytestmark = pytest.mark.gpu

CASES = [(1, 8), (5, 24), (3, 1003), (37, 1000), (9, 10000), (130, 10000), (6, 16384)]
KS = (1, 2, 3, 8)
GUARD = -123.25


def weights_of(K, equal):
    return None if equal else tuple(float(1 + (3 * k) % 5) for k in range(K))


@functools.lru_cache(maxsize=None)
def case_logits(Rn, V):
    """8 members' logits [8, R, V] f32: 3 * randn; member 1's row 0 scaled to |z| <= 80; column 5 far enough
    down that its log-probability is below -104 under every member"""
    g = torch.Generator(device="cpu").manual_seed(7000 * Rn + V)
    z = (3 * torch.randn(8, Rn, V, generator=g)).numpy()
    z[1, 0] *= np.float32(80.0 / np.abs(z[1, 0]).max())
    z[:, :, 5] = z.min(axis=2) - np.float32(130.0)
    return z, R.log_softmax64(z)  # (the float64 log-softmax rows: computed once per case)


def slab_ref(y):
    """(max f32 [R, S], float64 sum exp(v - max) [R, S]) of the stored f32 rows y, columns past V as -inf"""
    Rn, V = y.shape
    Sn = (V + 15) // 16
    yp = np.full((Rn, Sn * 16), -np.inf, dtype=np.float32)
    yp[:, :V] = y
    ys = yp.reshape(Rn, Sn, 16)
    mx = ys.max(axis=2)
    return mx, np.exp(ys.astype(np.float64) - mx[:, :, None].astype(np.float64)).sum(axis=2)


def run_combine(z, w, mode, want_stats, alias=False):
    """the hook on members z [K, R, V] with a guard row after out and after stats; -> (out f32 [R, V], stats f32
    [R, S, 2] or None) after checking that nothing else was written and no input changed"""
    K, Rn, V = z.shape
    Sn = (V + 15) // 16
    zd = [torch.from_numpy(np.ascontiguousarray(z[k])).to(DEV) for k in range(K)]
    if alias:  # out is member 0's buffer, with the guard row behind it
        out = torch.full((Rn + 1, V), GUARD, dtype=torch.float32, device=DEV)
        out[:Rn] = zd[0]
        zd[0] = out[:Rn]
    else:
        out = torch.full((Rn + 1, V), GUARD, dtype=torch.float32, device=DEV)
    st = torch.full((Rn + 1, Sn, 2), GUARD, dtype=torch.float32, device=DEV) if want_stats else None
    ptrs = (C.c_void_p * K)(*[t.data_ptr() for t in zd])
    wa = None if w is None else (C.c_float * K)(*w)
    from capgen import _lib
    _lib.check(_lib.load().capgen_debug_ensemble_combine(ptrs, wa, K, E.MODES.index(mode), Rn, V, P(out), P(st), None))
    torch.cuda.synchronize()
    guard = torch.tensor([GUARD]).view(torch.int32).item()
    assert (out[Rn].view(torch.int32) == guard).all(), "out written past its rows"
    if want_stats:
        assert (st[Rn].view(torch.int32) == guard).all(), "stats written past their rows"
    for k in range(1 if alias else 0, K):
        assert np.array_equal(zd[k].cpu().numpy().view(np.int32), z[k].view(np.int32)), f"member {k} was written"
    return out[:Rn].cpu().numpy(), (st[:Rn].cpu().numpy() if want_stats else None)


def check_combine(tag, z, l, w, mode, out, st):
    ref = E.combine_logsm(l, w, mode)
    bound = 1e-5 * np.maximum(1.0, np.abs(l).max(axis=(0, 2)))[:, None]
    err = np.abs(out.astype(np.float64) - ref)
    assert np.isfinite(out).all(), tag
    assert (err <= bound).all(), tag + f": off by {(err / bound).max():.2f} bounds"
    if mode == "prob":
        assert (l[:, :, 5] < -104).all() and np.isfinite(out[:, 5]).all(), tag
    if st is not None:
        mx, se = slab_ref(out)
        assert np.array_equal(st[:, :, 0].view(np.int32), mx.view(np.int32)), tag + ": slab maxima"
        rel = np.abs(st[:, :, 1].astype(np.float64) - se) / se
        assert rel.max() <= 1e-6, tag + f": slab sums off by {rel.max():.2e}"


@pytest.mark.parametrize("Rn, V", CASES)
def test_kernel_matches_restatement(Rn, V):
    """ensemble_combine_kernel<K, VEC>: out within 1e-5 * max(1, max |l_k| of the row); stats' maxima the
    stored outputs' bit for bit and their sums within 1e-6 relative; K in {1, 2, 3, 8}, both modes, equal and
    unequal weights; guard rows and the inputs untouched"""
    zall, lall = case_logits(Rn, V)
    n = 0
    for K in KS:
        for mode in E.MODES:
            for equal in (True, False):
                z, w = zall[:K], weights_of(K, equal)
                want_stats = V != 1003 and n % 4 != 3  # (3, 1003): stats null, the scalar tail
                n += 1
                out, st = run_combine(z, w, mode, want_stats)
                check_combine(f"R={Rn} V={V} K={K} {mode} w={w}", z, lall[:K], w, mode, out, st)


@pytest.mark.parametrize("Rn, V", [(5, 24), (3, 1003), (9, 10000)])
def test_kernel_out_may_be_member_0(Rn, V):
    z, l = (a[:3] for a in case_logits(Rn, V))
    for mode in E.MODES:
        a, sa = run_combine(z, (.5, .3, .2), mode, True)
        b, sb = run_combine(z, (.5, .3, .2), mode, True, alias=True)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
        check_combine(f"alias R={Rn} V={V} {mode}", z, l, (.5, .3, .2), mode, b, sb)


def test_kernel_scalar_form_writes_the_slab_stats_too():
    z, l = (a[:2] for a in case_logits(3, 1003))
    for mode in E.MODES:
        out, st = run_combine(z, None, mode, True)
        check_combine(f"V=1003 {mode}", z, l, None, mode, out, st)


def test_kernel_is_deterministic_and_rows_are_independent():
    """two launches give equal bits; a row's bits at R = 130 equal the same row launched alone"""
    z = case_logits(130, 10000)[0][:3]
    for mode in E.MODES:
        a, sa = run_combine(z, (.5, .3, .2), mode, True)
        b, sb = run_combine(z, (.5, .3, .2), mode, True)
        assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(sa.view(np.int32), sb.view(np.int32))
        for r in (0, 77, 129):
            one, s1 = run_combine(z[:, r:r + 1], (.5, .3, .2), mode, True)
            assert np.array_equal(one.view(np.int32), a[r:r + 1].view(np.int32)), (mode, r)
            assert np.array_equal(s1.view(np.int32), sa[r:r + 1].view(np.int32)), (mode, r)


def test_kernel_with_one_member_is_its_log_softmax():
    z, l = (a[:1] for a in case_logits(37, 1000))
    for mode in E.MODES:
        out, _ = run_combine(z, None, mode, False)
        assert (np.abs(out - l[0]) <= 1e-5 * np.abs(l[0]).max(axis=1, keepdims=True)).all()


def test_kernel_rejects_bad_arguments():
    from capgen import _lib
    lib = _lib.load()
    x = torch.zeros(2, 8, device=DEV)
    ptrs = (C.c_void_p * 9)(*[x.data_ptr()] * 9)

    def err(K, mode, w=None, p=ptrs, Rn=2):
        wa = None if w is None else (C.c_float * len(w))(*w)
        assert lib.capgen_debug_ensemble_combine(p, wa, K, mode, Rn, 8, P(x), None, None) != 0
        return lib.capgen_last_error().decode()

    assert "K " in err(0, 0) and "K " in err(9, 0) and "mode" in err(2, 2) and "mode" in err(2, -1)
    assert "weights[1]" in err(2, 0, (1.0, 0.0)) and "weights[0]" in err(2, 0, (float("nan"), 1.0))
    assert "weights[1]" in err(2, 0, (1.0, float("inf"))) and "R" in err(2, 0, Rn=0)
    assert "member 1" in err(2, 0, p=(C.c_void_p * 2)(x.data_ptr(), None))


# ---- the engines ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def member(tag, seed, dtype):
    """one engine per (fixture, weight seed, dtype) for the whole run (the fixture's own: test_gpu_sampling's)"""
    from capgen.engine import Engine
    cfg, fseed, _ = load_fixture(tag)
    if seed == fseed:
        return engine(tag, dtype)[0]
    e = Engine(cfg.replace(dtype=dtype), DEV)
    e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
    e.set_training(False)
    return e


def members(tag, seeds, dtypes="fp32"):
    dtypes = (dtypes,) * len(seeds) if isinstance(dtypes, str) else dtypes
    _, cfg, f, p = engine(tag, "fp32")
    return [member(tag, s, d) for s, d in zip(seeds, dtypes)], cfg, f, p


def host(out):
    return [t.cpu().numpy() for t in out]


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32) if x.dtype == torch.float32 else x,
                           y.view(torch.int32) if y.dtype == torch.float32 else y) for x, y in zip(a, b))


@pytest.mark.parametrize("row, alpha", [(i, a) for i, r in enumerate(E.TABLE) for a, _ in r[4]])
def test_engine_fp32_matches_restatement(row, alpha):
    """every row of ensemble_ref.TABLE, n_best = k = 3, by the rule of test_engine_fp32_c1_matches_restatement"""
    from capgen.engine import ensemble_beam_nbest
    tag, seeds, mode, w, _, _ = E.TABLE[row]
    es, cfg, f, p = members(tag, seeds)
    T, k, B = cfg.max_length, 3, f.shape[0]
    ref = R.nbest(ens_search(tag, seeds, mode, w)[1], alpha, k)
    out = ensemble_beam_nbest(es, f, p, k, END[tag], alpha, k, weights=w, mode=mode)
    ids, score, logp, length = host(out)
    R.structure_ok(ids, length, END[tag], T)
    assert (np.diff(score, axis=0) <= 0).all()
    assert ids.shape == (k, B, T) and score.shape == logp.shape == length.shape == (k, B)
    same = (ids == ref["ids"]).all(axis=2)
    delta = float(np.abs(logp - ref["logp"])[same].max()) if same.any() else float("inf")
    m = max(1e-3, 4 * delta)
    keep = ref["margin"] >= m
    print(f"{tag} {seeds} {mode} {w} alpha={alpha}: delta {delta:.3e}, m {m:.3e}, smallest reference margin "
          f"{ref['margin'].min():.3e}, {int((~keep).sum())} of {B} images left out")
    assert (~keep).sum() <= (2 if tag == "c1" else 0)
    assert np.array_equal(ids[:, keep], ref["ids"][:, keep])
    assert np.array_equal(length[:, keep], ref["len"][:, keep])
    assert np.abs(logp[:, keep] - ref["logp"][:, keep]).max() <= 1e-3
    assert np.abs(score[:, keep] - ref["score"][:, keep]).max() <= 1e-3


@pytest.mark.parametrize("mode", E.MODES)
@pytest.mark.parametrize("k", [3, 5])
def test_one_member_is_the_single_engine(k, mode):
    from capgen.engine import ensemble_beam_nbest
    e, cfg, f, p = engine("c1", "fp32")
    want = e.beam_nbest(f, p, k, END["c1"], 0.7, k)
    got = ensemble_beam_nbest([e], f, p, k, END["c1"], 0.7, k, mode=mode)
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
    assert (got[2] - want[2]).abs().max().item() <= 1e-4 and (got[1] - want[1]).abs().max().item() <= 1e-4


@pytest.mark.parametrize("tag, seeds, mode, w, n, temp", [
    ("c1", (0, 105), "prob", (.5, .5), 3, 1.0), ("c1", (0, 103), "logprob", (.7, .3), 2, 0.7),
    ("c2s", (3, 103), "prob", (.7, .3), 3, 1.0)])
def test_engine_sampling_fp32_matches_restatement(tag, seeds, mode, w, n, temp):
    """The sampled ids fed back teacher-forced through every member; the members' logits combined in float64 and
    every position restated by sampling_ref.sample: the rule of
    test_engine_fp32_matches_restatement_on_teacher_forced_logits"""
    from capgen.engine import ensemble_sample
    es, cfg, f, p = members(tag, seeds)
    seed, T, B = 1234, cfg.max_length, f.shape[0]
    ids, logp = ensemble_sample(es, f, p, n_samples=n, temperature=temp, top_k=0, seed=seed, top_p=1.0, weights=w,
                                mode=mode)
    Rn = n * B
    assert ids.shape == (n, B, T + 1) and logp.shape == (n, B, T - 1)
    flat = ids.view(Rn, T + 1)
    assert (flat[:, 0] == 1).all() and (flat[:, T] == 0).all()
    lg = []
    for e in es:
        e.forward(f.repeat(n, 1, 1), p.repeat(n, 1, 1), flat[:, :T])
        lg.append(e.logits(Rn, T).cpu().numpy())
    y = np.stack([E.combine(np.stack([x[:, t] for x in lg]), w, mode) for t in range(T - 1)], 1)  # [R, T-1, V]
    got_tok, got_lp = flat[:, 1:T].cpu().numpy(), logp.view(Rn, T - 1).cpu().numpy().astype(np.float64)
    refs = [S.sample(y[:, t], S.inv_tau_of(temp), 0, seed, S.SITE0 + t) for t in range(T - 1)]
    ref_tok = np.stack([r["token"] for r in refs], 1)
    ref_lp = np.stack([r["logp"] for r in refs], 1)
    margin = np.stack([r["margin"] for r in refs], 1)
    delta = np.abs(got_lp - ref_lp).max() * temp
    m = 1e-3
    if 4 * delta / 0.7 > m:
        m = math.ceil(4 * delta / 0.7 * 1e4) / 1e4
    keep = margin >= m
    left_out = int((~keep).sum())
    print(f"{tag} {seeds} {mode} n={n} T={temp}: delta = {delta:.3e}, m = {m:.1e}, left out {left_out} of {keep.size}")
    assert np.array_equal(got_tok[keep], ref_tok[keep])
    assert left_out <= 0.02 * keep.size
    assert np.abs(got_lp - ref_lp).max() <= 1e-3
    assert (got_lp <= 0).all()


@pytest.mark.parametrize("kw", [dict(top_p=0.9), dict(top_k=4)])
def test_engine_sampling_truncated(kw):
    from capgen.engine import ensemble_sample
    es, cfg, f, p = members("c1", (0, 105))
    a = ensemble_sample(es, f, p, n_samples=2, seed=1234, weights=(.5, .5), **kw)
    b = ensemble_sample(es, f, p, n_samples=2, seed=1234, weights=(.5, .5), **kw)
    assert same_bits(a, b)
    assert torch.isfinite(a[1]).all() and (a[1] <= 0).all()
    ids, none = ensemble_sample(es, f, p, n_samples=2, seed=1234, weights=(.5, .5), want_logp=False, **kw)
    assert none is None and torch.equal(ids, a[0])


def test_engine_bf16_full_row_path_equals_the_fused_step(set_knob):
    """members c2s (3, 103), both bf16, k = 3, prob: under CAPGEN_FUSED_BEAM_STEP=0 the full-row kernels read
    the fused logits themselves, the fused slab step the statistics ensemble_combine rebuilt: ids and len
    equal, logp within 1e-4 (the existing bf16 rule)"""
    from capgen.engine import Engine, ensemble_beam_nbest
    es, cfg, f, p = members("c2s", (3, 103), "bf16")
    fb = f.bfloat16()
    fused = ensemble_beam_nbest(es, fb, p, 3, END["c2s"], 1.0, 3, weights=(.5, .5))
    set_knob("FUSED_BEAM_STEP", 0)
    full_es = []
    try:
        for s in (3, 103):
            e = Engine(cfg.replace(dtype="bf16"), DEV)
            e.load_state_dict(fixture_state_dict(cfg, seed=s, with_buffer=False))
            e.set_training(False)
            full_es.append(e)
        full = ensemble_beam_nbest(full_es, fb, p, 3, END["c2s"], 1.0, 3, weights=(.5, .5))
        assert torch.equal(full[0], fused[0]) and torch.equal(full[3], fused[3])
        assert (full[2] - fused[2]).abs().max().item() <= 1e-4 and (full[1] - fused[1]).abs().max().item() <= 1e-4
        torch.cuda.synchronize()
    finally:
        for e in full_es:
            e.close()


def test_engine_mixed_dtypes():
    """an fp32 leader and a bf16 second member: the structure and finiteness only"""
    from capgen.engine import ensemble_beam_nbest
    es, cfg, f, p = members("c2s", (3, 103), ("fp32", "bf16"))
    ids, score, logp, length = host(ensemble_beam_nbest(es, f, p, 3, END["c2s"], 1.0, 3, weights=(.5, .5)))
    R.structure_ok(ids, length, END["c2s"], cfg.max_length)
    assert (np.diff(score, axis=0) <= 0).all() and np.isfinite(score).all() and np.isfinite(logp).all()


def test_engine_constraints_are_the_leaders():
    from capgen.engine import ensemble_beam_nbest
    es, cfg, f, p = members("c1", (0, 105))
    end, banned = END["c1"], (int(ens_search("c1", (0, 105), "prob", (.5, .5))[1]["seq"][0, 0, 1]),)
    free = ensemble_beam_nbest(es, f, p, 3, end, 0.0, 3, weights=(.5, .5))
    rows = lambda out: [r[1:1 + n] for r, n in zip(out[0].view(-1, cfg.max_length).tolist(), out[3].view(-1).tolist())]  # noqa: E731
    assert violations(rows(free), 2, 5, end, banned) > 0, "the unconstrained result breaks no constraint"
    with constrained(es[0], no_repeat_ngram=2, min_length=5, end_id=end, banned=banned):
        out = ensemble_beam_nbest(es, f, p, 3, end, 0.0, 3, weights=(.5, .5))
    R.structure_ok(out[0].cpu().numpy(), out[3].cpu().numpy(), end, cfg.max_length)
    assert violations(rows(out), 2, 5, end, banned) == 0
    assert torch.isfinite(out[1]).all()
    with constrained(es[1], no_repeat_ngram=2, min_length=5, end_id=end, banned=banned):  # a member's: ignored
        other = ensemble_beam_nbest(es, f, p, 3, end, 0.0, 3, weights=(.5, .5))
    assert same_bits(other, free)
    assert same_bits(ensemble_beam_nbest(es, f, p, 3, end, 0.0, 3, weights=(.5, .5)), free)


def _models(tag, seeds, dtype):
    from capgen.models import TRANSFORMER
    cfg, _, _ = load_fixture(tag)
    end = END[tag]
    words = {f"w{i}": i for i in range(cfg.num_vocab)}
    words.pop("w0"), words.pop("w1"), words.pop(f"w{end}")
    words.update({"<NULL>": 0, "<START>": 1, "<END>": end})
    out = []
    for s in seeds:
        m = TRANSFORMER(cfg.replace(dtype=dtype), word_to_idx=words, device=DEV,
                        state_dict=fixture_state_dict(cfg, seed=s, with_buffer=False))
        m.model.eval()
        out.append(m)
    return out


@pytest.mark.parametrize("tag, seeds, dtype", [("c1", (0, 105), "fp32"), ("c2s", (3, 103), "bf16")])
def test_ensemble_object_and_self_consistency_with_scoring(tag, seeds, dtype):
    """capgen.Ensemble: beam_captions / sample_captions return MODEL's shapes; score_captions of the captions
    beam_captions returned gives their logp within length * 1e-3 (fp32) -- bf16: within 1.25 x the same
    difference of a single bf16 engine on this fixture + 5e-3.  The single engine is the worse of the members:
    a token's ensemble log-probability is the log of a convex combination of the members' probabilities (prob
    mode), so between the decode path and the teacher-forced path it moves by at most the largest move of a
    member's own log-probability -- the worst member is the yardstick the ensemble can be held to, the leader
    alone is not"""
    from capgen import Ensemble
    from capgen.engine import ensemble_beam_nbest
    _, cfg, f, p = engine(tag, "fp32")
    fin = f.bfloat16() if dtype == "bf16" else f
    B, T, end = f.shape[0], cfg.max_length, END[tag]
    ms = _models(tag, seeds, dtype)
    ens = Ensemble(ms, weights=(.7, .3))
    caps, score = ens.beam_captions(fin, p, beam_size=3, n_best=3)
    assert len(caps) == 3 and all(len(c) == B and all(isinstance(s, str) for s in c) for c in caps)
    assert score.shape == (3, B) and score.dtype == torch.float32
    ids, want, blogp, blen = ensemble_beam_nbest([m.model.engine for m in ms], fin, p, 3, end, 0.0, 3, weights=(.7, .3))
    assert torch.equal(score, want) and caps[0] == ms[0].decode_captions(ids[0].cpu().numpy())
    sc = ens.score_captions(fin, p, ids)
    assert set(sc) == {"logp", "score", "token_logp", "length"} and sc["logp"].shape == (3, B)
    assert (sc["token_logp"][ids[..., 1:] == cfg.pad_idx] == 0).all()
    whole = sc["length"] == blen  # (a <NULL> inside a hypothesis is a masked target: that caption is left out)
    err = (sc["logp"] - blogp).abs()
    assert whole.sum() >= 2 * B
    if dtype == "fp32":
        print(f"{tag}: compared {int(whole.sum())} of {3 * B}, max |logp - beam's logp| {err[whole].max().item():.3e}")
        assert (err <= blen * 1e-3)[whole].all()
    else:
        singles = []
        for m in ms:
            sids, _, slogp, slen = m.model.engine.beam_nbest(fin, p, 3, end, 0.0, 3)
            one = m.score_captions(fin, p, sids)
            singles.append((one["logp"] - slogp).abs()[one["length"] == slen].max().item())
        single = max(singles)
        print(f"{tag} bf16: ensemble {err[whole].max().item():.3e}, single engines {singles}")
        assert err[whole].max().item() <= 1.25 * single + 5e-3
    scaps, slp = ens.sample_captions(fin, p, n_samples=2, seed=5)
    assert len(scaps) == 2 and all(len(c) == B for c in scaps) and slp.shape == (2, B) and (slp <= 0).all()
    with pytest.raises(ValueError, match="mode"):
        Ensemble(ms, mode="logprob").score_captions(fin, p, ids)


def test_hygiene_repeatable_hazard_free_and_members_unchanged():
    from capgen import _lib
    from capgen.engine import ensemble_beam_nbest, ensemble_sample
    es, cfg, f, p = members("c1", (0, 105, 103))
    end = END["c1"]
    before = [e.beam_nbest(f, p, 3, end, 0.7, 3) for e in es]
    a = ensemble_beam_nbest(es, f, p, 3, end, 0.7, 3, weights=(.5, .3, .2))
    assert same_bits(a, ensemble_beam_nbest(es, f, p, 3, end, 0.7, 3, weights=(.5, .3, .2)))
    s = ensemble_sample(es, f, p, n_samples=2, seed=9, mode="logprob")
    _lib.hazard_start()
    try:
        c = ensemble_beam_nbest(es, f, p, 3, end, 0.7, 3, weights=(.5, .3, .2))
        d = ensemble_sample(es, f, p, n_samples=2, seed=9, mode="logprob")
        after = [e.beam_nbest(f, p, 3, end, 0.7, 3) for e in es]  # (each member's own stream, behind the calls)
        torch.cuda.synchronize()
        n, report = _lib.hazard_check()
    finally:
        _lib.hazard_stop()
    assert n == 0, report
    assert same_bits(a, c) and same_bits(s, d)
    for x, y in zip(before, after):
        assert same_bits(x, y)


def test_bad_arguments_name_the_member_and_the_field():
    from capgen import _lib
    from capgen.engine import Engine, ensemble_beam_nbest
    lib = _lib.load()
    es, cfg, f, p = members("c1", (0, 105))
    B, N, T = f.shape[0], f.shape[1], cfg.max_length
    out = torch.zeros(3 * B, T, dtype=torch.int64, device=DEV)
    want = ensemble_beam_nbest(es, f, p, 3, END["c1"], 0.0, 3)
    others = {}
    for field, kw in (("num_vocab", dict(num_vocab=1016)), ("max_length", dict(max_length=T + 1)),
                      ("pad_idx", dict(pad_idx=2)),
                      ("dim_features", dict(encode_dim_features=cfg.encode_dim_features + 8)),
                      ("dim_positions", dict(encode_dim_positions=cfg.encode_dim_positions + 4))):
        others[field] = Engine(cfg.replace(**kw), DEV)

    def err(handles, weights=None, mode=0, n=None):
        e = _lib.ensemble(handles, weights, mode)
        if n is not None:
            e.n_members = n
        rc = lib.capgen_ensemble_beam_nbest(C.byref(e), P(f), _lib.F32, P(p), B, N, 3, END["c1"], C.c_float(0.0), 3,
                                            P(out), None, None, None, None)
        rs = lib.capgen_ensemble_sample(C.byref(e), P(f), _lib.F32, P(p), B, N, 1, C.c_float(1.0), 0, C.c_float(1.0), 1,
                                        P(out), None, None)
        assert rc != 0 and rs != 0
        return lib.capgen_last_error().decode()

    h = [e.h for e in es]
    assert "n_members" in err(h, n=0) and "n_members" in err(h, n=9)
    assert "member 1" in err([h[0], None]) and "null" in err([h[0], None])
    assert "member 1" in err([h[0], h[0]]) and "duplicate" in err([h[0], h[0]])
    for field, o in others.items():
        msg = err([h[0], o.h])
        assert "member 1" in msg and field in msg, msg
    for w in ((1.0, 0.0), (1.0, -1.0), (1.0, float("nan")), (1.0, float("inf"))):
        msg = err(h, weights=w)
        assert "member 1" in msg and "weights[1]" in msg, msg
    assert "mode" in err(h, mode=2) and "mode" in err(h, mode=-1)
    assert lib.capgen_ensemble_beam_nbest(None, P(f), _lib.F32, P(p), B, N, 3, END["c1"], C.c_float(0.0), 3, P(out), None,
                                          None, None, None) != 0
    for o in others.values():
        o.close()
    assert same_bits(ensemble_beam_nbest(es, f, p, 3, END["c1"], 0.0, 3), want)  # every member is still usable
    for e in es:
        assert torch.isfinite(e.beam_nbest(f, p, 3, END["c1"], 0.0, 1)[1]).all()
