"""Scoring given captions on the GPU (capgen_score_captions): the two read-out kernels through their
C-ABI hooks against the float64 restatement tests/score_ref.py, then the engine call against the float64
oracle and against the engine's own loss, weighted-loss and decode paths, then the Python calls.

    token_logp[r, t] = logit[tgt] - logsumexp(logit)   (0 at pad targets)
    hit              = tgt != pad and logit[tgt] >= max(logit)
    logp[r] = sum_t token_logp, length[r] = #(tgt != pad), hits[r] = sum_t hit

Kernel bounds: |token_logp - ref| <= 1e-5 (|lse| + |tl|) (assert_loss_rows' bound for the same quantity),
|logp - sum ref| <= the sum of the caption's row bounds, everything integer exact."""
import numpy as np
import pytest
import torch

from score_ref import score_ref
from test_beam_host import C1_END, C2S_END
from test_gpu_rollout import _dev, _engine, _params_close, _vocab, case, other_tokens
from test_gpu_rowops import CE_PAD, DEV, P, _lib_, call, ce_rows, dev, gen, slab_stats

gpu = pytest.mark.gpu
POOL_ROWS = 10
PAD_MID = 7  # index of the extra pad row in the pool: inside a caption for Lq = 3 and 19


def score_pool(V, seed):
    """10 logit rows and targets: test_gpu_rowops.ce_rows' six (columns 0, V-1, both sides of a float4
    boundary, a pad row, the +-60 row), then 6: the target is the strict argmax; 7: a pad row; 8: the
    target ties the maximum with another column (a hit); 9: the target is second, one f32 ulp under the
    maximum (no hit)."""
    x6, t6 = ce_rows(V, seed)
    x = torch.cat([x6, 2 * torch.randn(4, V, generator=gen(seed + 77))])
    tgt = torch.cat([t6, torch.zeros(4, dtype=torch.int32)])
    a, b = V // 3, (2 * V) // 3
    assert a != b and CE_PAD not in (a, b)
    tgt[6] = int(x[6].argmax())
    if tgt[6] == CE_PAD:
        x[6, a] = x[6].max() + 1
        tgt[6] = a
    tgt[PAD_MID] = CE_PAD
    top = x[8].max() + 1
    x[8, a] = x[8, b] = top
    tgt[8] = b
    top = (x[9].max() + 1).item()
    x[9, b] = top
    x[9, a] = float(np.nextafter(np.float32(top), np.float32(top + 1)))
    tgt[9] = b
    return x, tgt


def score_case(V, Lq):
    """(x [M, V] f32, tgt [M] int32): the pool cycled over whole captions of Lq rows, then one caption of
    pads only; M = (ceil(10 / Lq) + 1) Lq"""
    px, pt = score_pool(V, V)
    n = -(-POOL_ROWS // Lq) * Lq
    idx = torch.arange(n + Lq) % POOL_ROWS
    x, tgt = px[idx].contiguous(), pt[idx].clone()
    tgt[n:] = CE_PAD
    return x, tgt


def guarded(n, dtype, fill):
    return torch.full((n + 1,), fill, dtype=dtype, device=DEV)


def run_hook(launch, M, Lq):
    """launch(token_logp, hit, logp, length, hits) runs a hook; every output carries a guard word"""
    R = M // Lq
    out = [guarded(M, torch.float32, 7.0), guarded(M, torch.int32, -7), guarded(R, torch.float32, 7.0),
           guarded(R, torch.int32, -7), guarded(R, torch.int32, -7)]
    launch(*out)
    for o, n in zip(out, (M, M, R, R, R)):
        assert o[n].item() in (7.0, -7), "the guard word after an output buffer"
    return [o[:n].cpu() for o, n in zip(out, (M, M, R, R, R))]


def check_kernel(got, x, tgt, Lq, what):
    tok, hit, logp, length, hits = got
    ref = score_ref(x.double(), tgt, CE_PAD, Lq)
    kept = ref["kept"].reshape(-1)
    bound = 1e-5 * (ref["lse"].abs() + ref["tl"].abs()) * ref["kept"]  # [R, Lq], 0 on pad rows
    err = (tok.double().view(-1, Lq) - ref["token_logp"]).abs()
    lerr = (logp.double() - ref["logp"]).abs()
    print(f"{what}: token_logp err {err.max().item():.3e} (bound there {bound.flatten()[err.argmax()].item():.3e}), "
          f"logp err {lerr.max().item():.3e}")
    assert torch.isfinite(tok).all() and torch.isfinite(logp).all(), what
    assert (err <= bound).all(), (what, err.max().item())
    assert (lerr <= bound.sum(1)).all(), (what, lerr, bound.sum(1))
    assert torch.equal(hit.long(), ref["hit"].reshape(-1)), what
    assert torch.equal(length.long(), ref["length"]) and torch.equal(hits.long(), ref["hits"]), what
    assert (tok[~kept] == 0).all() and (hit[~kept] == 0).all(), what + ": pad rows are exactly zero"
    empty = ref["length"] == 0
    assert empty[-1] and (logp[empty] == 0).all() and (hits[empty] == 0).all(), what + ": the all-pad caption"
    # the pool's hit rows say what they were built to say
    pool_hit = ref["hit"].reshape(-1)[:POOL_ROWS].tolist()
    assert pool_hit[6] == 1 and pool_hit[8] == 1 and pool_hit[9] == 0 and pool_hit[PAD_MID] == 0, pool_hit


def same_bits(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


@gpu
@pytest.mark.parametrize("Lq", [1, 3, 19])
@pytest.mark.parametrize("V", [8, 1001, 10000, 16384])
def test_score_rows(V, Lq):
    """the register forms NV4 = 4 (8), 10 (10000), 16 (16384) and the generic one-pass form (1001)"""
    x, tgt = score_case(V, Lq)
    M = x.shape[0]
    xd, td = dev(x), dev(tgt)

    def launch(tok, hit, logp, length, hits):
        call("capgen_debug_score_rows", P(xd), P(td), M, V, CE_PAD, Lq, P(tok), P(hit), P(logp), P(length), P(hits),
             None)

    got = run_hook(launch, M, Lq)
    check_kernel(got, x, tgt, Lq, f"score_rows V={V} Lq={Lq}")
    assert same_bits(got, run_hook(launch, M, Lq)), "two runs give the same bits"


SCORE_FINISH_VS = [8, 12, 1000, 4104, 10000, 16392]


@gpu
@pytest.mark.parametrize("Lq", [1, 3, 19])
@pytest.mark.parametrize("wide_ld", [0, 1])
@pytest.mark.parametrize("V", SCORE_FINISH_VS)
def test_score_finish(V, wide_ld, Lq):
    """1 slab (8, 12: a partial one), 63 (1000: a partial last slab), 257, 625 and 1025 slabs: 1, 1, 5 (the
    8-pair form), 10 and 17 (the 32-pair form) pairs per lane; ld exact and ld + 3 with NaN behind the row's
    slabs.  The e rows are not an argument of the hook."""
    x, tgt = score_case(V, Lq)
    M = x.shape[0]
    stats, _ = slab_stats(x)
    S = stats.shape[1]
    ld = S + 3 * wide_ld
    st = torch.full((M, ld, 2), float("nan"))
    st[:, :S] = stats
    tl = x[torch.arange(M), tgt.long()].float()
    std, tld, td = dev(st), dev(tl), dev(tgt)

    def launch(tok, hit, logp, length, hits):
        call("capgen_debug_score_finish", P(std), ld, P(tld), P(td), M, V, CE_PAD, Lq, P(tok), P(hit), P(logp),
             P(length), P(hits), None)

    got = run_hook(launch, M, Lq)
    check_kernel(got, x, tgt, Lq, f"score_finish V={V} ld+{3 * wide_ld} Lq={Lq}")
    assert same_bits(got, run_hook(launch, M, Lq)), "two runs give the same bits"
    # the optional outputs left out: the required one is unchanged
    R = M // Lq
    logp = guarded(R, torch.float32, 7.0)
    call("capgen_debug_score_finish", P(std), ld, P(tld), P(td), M, V, CE_PAD, Lq, None, None, P(logp), None, None, None)
    assert logp[R].item() == 7.0 and torch.equal(logp[:R].cpu().view(torch.int32), got[2].view(torch.int32))


@gpu
def test_score_hooks_reject_bad_arguments():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(64, dtype=torch.int32, device=DEV)
    rows, fin = lib.capgen_debug_score_rows, lib.capgen_debug_score_finish

    def r(logits=P(z), tgt=P(zi), M=4, V=8, Lq=2, tok=P(z), hit=P(zi), logp=P(z)):
        assert rows(logits, tgt, M, V, 0, Lq, tok, hit, logp, P(zi), P(zi), None) == 1
        assert b"score_rows" in lib.capgen_last_error(), lib.capgen_last_error()

    def f(stats=P(z), ld=1, tlo=P(z), tgt=P(zi), M=4, V=8, Lq=2, logp=P(z)):
        assert fin(stats, ld, tlo, tgt, M, V, 0, Lq, P(z), P(zi), logp, P(zi), P(zi), None) == 1
        assert b"score_finish" in lib.capgen_last_error(), lib.capgen_last_error()

    r(logits=None), r(tgt=None), r(tok=None), r(hit=None), r(logp=None)
    r(Lq=0), r(Lq=-1), r(Lq=3), r(M=0)
    f(stats=None), f(tlo=None), f(tgt=None), f(logp=None)
    f(Lq=0), f(Lq=3), f(M=0)
    f(V=10), f(V=1001)          # V % 4 != 0
    f(V=32, ld=1), f(V=20, ld=1)  # ld below the row's slab count
    tok, hit, logp = torch.zeros(4, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV), torch.zeros(2, device=DEV)
    assert rows(P(z), P(zi), 4, 8, 0, 2, P(tok), P(hit), P(logp), None, None, None) == 0  # (length, hits are optional)
    torch.cuda.synchronize()


# ---- the engine ----------------------------------------------------------------------------------------
TOK_BOUND = 2e-3  # fp32: the logits are held within 1e-3 of the oracle; token_logp is a difference of two such terms
MARGIN = 4e-3     # hits are compared where the float64 top-2 margin is at least this


def oracle_score(cfg, seed, f, p, c):
    from capgen.params import fixture_state_dict
    from oracle import capgen_oracle as O
    Pm = O.make_params(fixture_state_dict(cfg, seed=seed, with_buffer=False), requires_grad=False, dtype=torch.float64)
    with torch.no_grad():
        lg = O.forward_logits(Pm, cfg, f.double(), p.double(), c, training=False)
    return score_ref(lg, c[:, 1:], cfg.pad_idx, c.shape[1] - 1)


def score_fixture(tag):
    """test_gpu_rollout.case(tag); on padcap the first word of caption 0 is another one: as stored, that
    position's two best logits are 2.9e-3 apart, under the margin the hit comparison needs"""
    cfg, seed, f, p, c = case(tag)
    if tag == "padcap":
        c = c.clone()
        c[0, 1] = (c[0, 1] + 7) % 900 + 3
    return cfg, seed, f, p, c


def cpu(*ts):
    return [t.cpu() for t in ts]


@gpu
@pytest.mark.parametrize("tag", ["c1", "padcap"])
def test_score_fp32_matches_float64_oracle(tag):
    """Every kept token_logp within 2e-3, logp within 2e-3 x the caption's kept tokens, length exact, hits
    exact on the rows whose float64 top-2 margin is >= 4e-3.  CPU pre-check (the float32 oracle against the
    float64 one, before the first GPU run): token_logp error 1.2e-6 on c1 and 1.3e-6 on padcap (a tenth of
    the bound is 2e-4), logp error per token <= 3e-7; kept rows under the margin: c1 1 of 55 (1.8 %, row
    (5, 2), margin 2.9e-3); padcap as stored 1 of 22 (4.5 %, row (0, 1), margin 2.9e-3), so the captions
    were chosen, not the cap widened: with caption 0's first word replaced (score_fixture) 0 of 22 (the
    smallest margin is 6.0e-3)."""
    cfg, seed, f, p, c = score_fixture(tag)
    ref = oracle_score(cfg, seed, f, p, c)
    e = _engine(cfg, seed)
    tok, logp, length, hits = cpu(*e.score_captions(*_dev(f, p, c)))
    kept = ref["kept"]
    err = (tok.double() - ref["token_logp"]).abs()
    lerr = (logp.double() - ref["logp"]).abs()
    sure = kept & (ref["margin"] >= MARGIN)
    print(f"{tag}: token_logp err {err[kept].max().item():.3e} (bound {TOK_BOUND}), logp err {lerr.max().item():.3e}, "
          f"{int((kept & ~sure).sum())} of {int(kept.sum())} kept rows under the margin, hits {hits.tolist()}")
    assert (err[kept] <= TOK_BOUND).all() and (tok[~kept] == 0).all()
    assert (lerr <= TOK_BOUND * ref["length"]).all()
    assert torch.equal(length.long(), ref["length"])
    assert (kept & ~sure).sum() <= 0.02 * kept.sum()
    if not (kept & ~sure).any():
        assert torch.equal(hits.long(), ref["hits"])
    assert (hits.long() - ref["hits"]).abs().le((kept & ~sure).sum(1)).all()
    if tag == "padcap":
        assert length[1] == 0 and logp[1] == 0 and hits[1] == 0


def sum_rule(e, fd, pd, cd):
    tok, logp, length, hits = e.score_captions(fd, pd, cd)
    mean = -(logp.double().sum() / length.sum()).item()
    return mean, e.compute_loss(fd, pd, cd).item(), logp.cpu().double(), length.cpu()


@gpu
@pytest.mark.parametrize("tag", ["c1", "padcap"])
def test_score_sums_to_the_loss_fp32(tag):
    cfg, seed, f, p, c = case(tag)
    mean, loss, _, _ = sum_rule(_engine(cfg, seed), *_dev(f, p, c))
    print(f"{tag}: -sum logp / sum length {mean:.7f}, compute_loss {loss:.7f}")
    assert abs(mean - loss) <= 1e-4, (mean, loss)


@gpu
@pytest.mark.parametrize("tag", ["c2s", "padcap_c2s"])
def test_score_sums_to_the_loss_bf16_both_ce_paths(tag, set_knob):
    """bf16 with the fused classifier (score_finish) and with FUSED_CE = 0 (score_rows on the f32 logits):
    each within 1e-4 of its own engine's compute_loss, and the two within 1e-4 per caption and token"""
    cfg, seed, f, p, c = case(tag)
    args = _dev(f, p, c)
    res = []
    for fused in (1, 0):
        set_knob("FUSED_CE", fused)
        mean, loss, logp, length = sum_rule(_engine(cfg, seed, dtype="bf16"), *args)
        print(f"{tag} FUSED_CE={fused}: -sum logp / sum length {mean:.7f}, compute_loss {loss:.7f}")
        assert abs(mean - loss) <= 1e-4, (fused, mean, loss)
        res.append((logp, length))
    (la, na), (lb, nb) = res
    assert torch.equal(na, nb)
    per = ((la - lb) / na.clamp(min=1)).abs()
    print(f"{tag}: fused against logits path, per caption and token {per.max().item():.3e}")
    assert (per <= 1e-4).all(), per


def per_caption_weighted(e, fd, pd, cd, count):
    """the parent's own per-caption sum: -train_step_weighted(w = onehot(r), train=False) x count"""
    B = cd.shape[0]
    out = []
    for r in range(B):
        w = torch.zeros(B, device=DEV)
        w[r] = 1.0
        out.append(-e.train_step_weighted(fd, pd, cd, w, train=False).item() * count)
    return torch.tensor(out, dtype=torch.float64)


@gpu
@pytest.mark.parametrize("tag,dtype", [("c1", "fp32"), ("padcap", "fp32"), ("c2s", "bf16"), ("padcap_c2s", "bf16")])
def test_score_per_caption_against_the_weighted_loss(tag, dtype):
    """fp32: logp[r] within twice the summed row bound (2 x 2e-3 x length) of the weighted loss's sum; bf16:
    its error against the float64 oracle is at most 1.25 x (+5e-3) that of the weighted loss's sum"""
    cfg, seed, f, p, c = case(tag)
    ref = oracle_score(cfg, seed, f, p, c)
    e = _engine(cfg, seed, dtype=dtype)
    fd, pd, cd = _dev(f, p, c)
    _, logp, length, _ = cpu(*e.score_captions(fd, pd, cd))
    old = per_caption_weighted(e, fd, pd, cd, int(ref["length"].sum()))
    e_new = (logp.double() - ref["logp"]).abs()
    e_old = (old - ref["logp"]).abs()
    print(f"{tag} {dtype}: |logp - oracle| {e_new.tolist()}, |weighted-loss sum - oracle| {e_old.tolist()}")
    if dtype == "fp32":
        assert ((logp.double() - old).abs() <= 2 * TOK_BOUND * ref["length"]).all(), (logp, old)
    else:
        assert (e_new <= 1.25 * e_old + 5e-3).all(), (e_new, e_old)
    assert (logp[ref["length"] == 0] == 0).all()


@gpu
@pytest.mark.parametrize("tag,dtype", [("c1", "fp32"), ("c2s", "bf16")])
def test_score_img_idx_equals_repeated_features(tag, dtype):
    cfg, seed, f, p, c = case(tag)
    B, n = c.shape[0], 3
    caps = torch.cat([c, c.roll(1, 0), other_tokens(c, 0, cfg.pad_idx)])  # three candidates per image
    idx = torch.arange(B, dtype=torch.int32).repeat(n)
    e = _engine(cfg, seed, dtype=dtype)
    fd, pd, cd, idxd = _dev(f, p, caps, idx)
    a = cpu(*e.score_captions(fd, pd, cd, img_idx=idxd))
    b = cpu(*e.score_captions(fd.repeat(n, 1, 1), pd.repeat(n, 1, 1), cd))
    assert same_bits(a, b)
    assert not torch.equal(a[1][:B], a[1][B:2 * B])  # (the candidates differ)


@gpu
@pytest.mark.parametrize("tag,end", [("c1", C1_END), ("c2s", C2S_END)])
def test_score_matches_the_decoders_own_logp_fp32(tag, end):
    """Engine.sample (n = 2, temperature 1, the whole vocabulary, seed 1234) -> rollout_captions ->
    score_captions: every kept position through <END> within 1e-3 of the sampler's own logp (a sampled
    <NULL> is a masked target: left out, counted); beam_nbest (3 beams, 3 best): logp within length x 1e-3."""
    from capgen.utils import rollout_captions
    cfg, seed, f, p, _ = case(tag)
    fd, pd = _dev(f, p)
    B, T = f.shape[0], cfg.max_length
    e = _engine(cfg, seed)
    ids, lp = e.sample(fd, pd, n_samples=2, temperature=1.0, top_k=0, top_p=1.0, seed=1234)
    caps = rollout_captions(ids, end, cfg.pad_idx)  # [2, B, T]
    idx = torch.arange(B, dtype=torch.int32, device=DEV).repeat(2)
    tok, logp, length, _ = e.score_captions(fd, pd, caps.view(2 * B, T), img_idx=idx)
    tgt = caps.view(2 * B, T)[:, 1:]
    kept = tgt != cfg.pad_idx
    drawn = ids.view(2 * B, T + 1)[:, 1:T]
    after = (((drawn == end).long().cumsum(1) - (drawn == end).long()) > 0)
    nulls = int(((drawn == cfg.pad_idx) & ~after).sum())
    err = (tok - lp.view(2 * B, T - 1)).abs()[kept]
    print(f"{tag}: sampled positions kept {int(kept.sum())}, sampled <NULL> left out {nulls}, "
          f"max |token_logp - sampler's logp| {err.max().item():.3e}")
    assert torch.equal(kept, ~after & (drawn != cfg.pad_idx)) and torch.equal(length.long(), kept.sum(1))
    assert kept.sum() >= B and (err <= 1e-3).all()
    bids, _, blogp, blen = e.beam_nbest(fd, pd, 3, end, 0.0, 3)
    bc = bids.view(3 * B, T).to(torch.int32)
    idx3 = torch.arange(B, dtype=torch.int32, device=DEV).repeat(3)
    _, slogp, slen, _ = e.score_captions(fd, pd, bc, img_idx=idx3)
    whole = slen == blen.view(-1)  # (a <NULL> inside a hypothesis is a masked target: that caption is left out)
    berr = (slogp - blogp.view(-1)).abs()
    print(f"{tag}: beam captions compared {int(whole.sum())} of {3 * B}, max |logp - beam's logp| "
          f"{berr[whole].max().item():.3e}, lengths {blen.view(-1).tolist()}")
    assert whole.sum() >= 2 * B and (slen <= blen.view(-1)).all()
    assert (berr <= blen.view(-1) * 1e-3)[whole].all()
    # the greedy caption's targets are the teacher-forced argmax (the decode and the teacher-forced logits
    # differ by ~1e-6, the fixtures' top-2 margins are >= 2.9e-3: at most a stray position may flip)
    gc = rollout_captions(e.greedy(fd, pd, want_attention=False)[0], end, cfg.pad_idx)
    _, _, glen, ghits = e.score_captions(fd, pd, gc)
    print(f"{tag}: greedy captions: hits {int(ghits.sum())} of {int(glen.sum())} kept targets")
    assert glen.sum() >= B and ghits.sum() >= 0.9 * glen.sum()


@gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_changes_nothing(dtype):
    cfg, seed, f, p, c = case("c2s")
    fd, pd, cd = _dev(f, p, c)
    e = _engine(cfg, seed, dtype)
    e.train_step(fd, pd, cd)  # (Adam moments that are not zero)
    before = e.state_dict(False)
    step0, m0, v0 = e.adam_state()
    l0 = e.compute_loss(fd, pd, cd).item()
    s0 = cpu(*e.score_captions(fd, pd, cd))
    after = e.state_dict(False)
    step1, m1, v1 = e.adam_state()
    for k in before:
        assert torch.equal(before[k], after[k]), k
        assert torch.equal(m0[k], m1[k]) and torch.equal(v0[k], v1[k]), k
    assert step0 == step1
    assert e.compute_loss(fd, pd, cd).item() == l0
    assert same_bits(s0, cpu(*e.score_captions(fd, pd, cd))), "two calls give the same bits"


@gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_ignores_training_mode_and_leaves_the_dropout_seed(dtype):
    cfg, seed, f, p, c = case("c2s")
    fd, pd, cd = _dev(f, p, c)
    e = _engine(cfg, seed, dtype, dropout=0.1, training=True)
    s_train = cpu(*e.score_captions(fd, pd, cd))
    losses = []
    for score_between in (False, False, True):
        e.set_rng_seed(99)
        if score_between:
            e.score_captions(fd, pd, cd)
        losses.append(e.forward(fd, pd, cd).item())
    assert losses[0] == losses[1], "set_rng_seed(s); forward repeats itself"
    assert losses[2] == losses[0], (losses, "a scoring call moved the dropout seed")
    e.set_training(False)
    assert losses[0] != e.forward(fd, pd, cd).item(), "dropout was on in the forwards above"
    assert same_bits(s_train, cpu(*e.score_captions(fd, pd, cd))), "training mode changes no score"
    ref = _engine(cfg, seed, dtype)  # (an engine without dropout in its config scores the same)
    assert same_bits(s_train, cpu(*ref.score_captions(fd, pd, cd)))


@gpu
@pytest.mark.parametrize("route", ["forward_graph", "step_graph"])
def test_score_between_graph_steps_fp32(route, set_knob):
    """train step -> score -> train step with the forward graph (then the direct route) or the whole-step
    graph: the scores equal, bit for bit, those of an eager engine loaded with the same state, and the later
    steps' losses and the parameters equal those of an engine that never scored within
    test_weighted_graph_routes_equal_eager_fp32's tolerances (gradient sums are not pinned bit for bit)."""
    cfg, seed, f, p, c = case("c1")
    fd, pd, cd = _dev(f, p, c)
    set_knob("FWD_GRAPH", 0)
    eager = _engine(cfg, seed)
    set_knob("FWD_GRAPH", 1)
    a, never = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, never):
        e.set_graph(route == "step_graph")
    for i in range(3):  # 0: captures; 1, 2: replays (the forward graph's direct route on the caller's stream)
        la, ln = a.train_step(fd, pd, cd).item(), never.train_step(fd, pd, cd).item()
        if i == 0:
            assert la == ln, (la, ln)
        else:
            assert abs(la - ln) < 2e-2 * abs(ln), (i, la, ln)
        eager.load_state_dict(a.state_dict(False))  # the same state, scored without any graph around
        sa, se = cpu(*a.score_captions(fd, pd, cd)), cpu(*eager.score_captions(fd, pd, cd))
        assert same_bits(sa, se), i
        assert (sa[1] < 0).all()
    _params_close(a, never, 5e-3)


@gpu
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_score_has_no_unordered_conflicts(dtype):
    from capgen import _lib
    cfg, seed, f, p, c = case("c2s")
    e = _engine(cfg, seed, dtype=dtype, dropout=0.3, training=True)
    B = c.shape[0]
    fd, pd, cd, idxd = _dev(f, p, c, torch.arange(B, dtype=torch.int32))
    e.train_step(fd, pd, cd)  # tune + warm outside the log
    e.score_captions(fd, pd, cd)
    torch.cuda.synchronize()
    _lib.hazard_start()
    try:
        e.train_step(fd, pd, cd)
        e.score_captions(fd, pd, cd, img_idx=idxd)
        e.train_step(fd, pd, cd)
        torch.cuda.synchronize()
        n, report = _lib.hazard_check()
    finally:
        _lib.hazard_stop()
    assert n == 0, f"{n} unordered conflicting launch pairs:\n{report}"


@gpu
def test_score_errors_leave_the_engine_usable():
    _lib, lib = _lib_()
    cfg, seed, f, p, c = case("c1")
    fd, pd, cd = _dev(f, p, c)
    idx = torch.zeros(c.shape[0], dtype=torch.int32, device=DEV)
    e = _engine(cfg, seed)
    B, N, T = c.shape[0], f.shape[1], c.shape[1]
    logp = torch.zeros(B, device=DEV)

    def err(R=B, n=N, t=T, n_images=0, img_idx=None, out=P(logp)):
        rc = lib.capgen_score_captions(e.h, P(fd), _lib.F32, P(pd), n_images, img_idx, P(cd), R, n, t, None, out, None,
                                       None, None)
        assert rc != 0
        return lib.capgen_last_error().decode()

    assert "R >= 1" in err(R=0)
    assert "T" in err(t=1) and "max_length" in err(t=cfg.max_length + 1)
    assert "empty store" in err(n_images=0, img_idx=P(idx)) and "empty store" in err(n_images=-1, img_idx=P(idx))
    assert "logp is null" in err(out=None)
    assert "N" in err(n=65)
    with pytest.raises(ValueError):
        e.score_captions(fd, pd, cd[0])
    with pytest.raises(ValueError):
        e.score_captions(fd, pd, cd, img_idx=idx[:-1])
    tok, lp, length, hits = e.score_captions(fd, pd, cd)  # the engine stays usable
    assert torch.isfinite(tok).all() and (lp < 0).all() and torch.isfinite(e.train_step(fd, pd, cd)).all()


# ---- the Python call -----------------------------------------------------------------------------------
@gpu
def test_model_score_captions_and_the_reranking_recipe():
    """MODEL.score_captions on [n, B, T] and [B, T]; length_penalty only rescales 'score'; the re-ranking
    recipe of INTEGRATION.md picks, per image, the candidate whose score is largest."""
    from capgen.models import TRANSFORMER
    from capgen.params import fixture_state_dict
    from capgen.utils import rollout_captions
    cfg, seed, f, p, _ = case("c1")
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=_vocab(cfg), device=DEV,
                    state_dict=fixture_state_dict(cfg, seed=seed, with_buffer=False))
    m.model.eval()
    B, T, n = f.shape[0], cfg.max_length, 4
    # the recipe: candidates -> teacher-forcing captions -> scores -> the best per image
    ids, _ = m.model.sample_caption_vector(object_features=f, position_features=p, n_samples=n, temperature=1.0,
                                           top_k=0, seed=7)
    caps = rollout_captions(ids, m.end_idx, cfg.pad_idx)          # [n, B, T]
    out = m.score_captions(f, p, caps, length_penalty=0.7)
    best = out["score"].argmax(0)                                  # [B]
    chosen = caps[best, torch.arange(B, device=caps.device)]       # [B, T]
    text = m.decode_captions(chosen.cpu().numpy())
    assert len(text) == B and all(isinstance(s, str) for s in text)
    assert set(out) == {"logp", "score", "token_logp", "length", "token_accuracy"}
    assert out["logp"].shape == out["score"].shape == out["length"].shape == out["token_accuracy"].shape == (n, B)
    assert out["token_logp"].shape == (n, B, T - 1) and all(v.is_cuda for v in out.values())
    assert out["length"].dtype == torch.int32 and out["logp"].dtype == torch.float32
    assert ((out["token_accuracy"] >= 0) & (out["token_accuracy"] <= 1)).all()
    assert torch.equal(out["score"].gather(0, best.view(1, B)).view(B), out["score"].max(0).values)
    den = out["length"].clamp(min=1).float()
    assert torch.equal(out["score"], out["logp"] / den ** 0.7)
    plain = m.score_captions(f, p, caps)  # length_penalty = 0: the log-probability itself
    assert torch.equal(plain["score"], plain["logp"])
    for k in ("logp", "token_logp", "length", "token_accuracy"):
        assert torch.equal(plain[k], out[k]), k
    # [B, T] (numpy ids): candidate 1 alone, each row with its own image
    one = m.score_captions(f, p, caps[1].cpu().numpy())
    assert one["logp"].shape == (B,) and one["token_logp"].shape == (B, T - 1)
    assert torch.equal(one["logp"], out["logp"][1]) and torch.equal(one["length"], out["length"][1])
