"""Nucleus (top-p) sampling on the GPU: the selection kernel (sample_nucleus, through its C-ABI hook)
against the float64 restatement of its header comment (tests/nucleus_ref.py), then
capgen_sample_nucleus and the Python calls over it on the fixture weights.

The kernel sums masses in f32 and the restatement in f64, so results are compared under the boundary
rule of nucleus_ref.band: eps = 1e-5 of the compared quantity's maximum (above / P <= 1), the
project's f32 rule, around top_p, and the project's 1e-4 margin between the two best perturbed scores.
A seed is taken only if it determines every row (asserted on the restatement alone, before the
kernel runs); no row is ever left out."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import nucleus_ref as N
import sampling_ref as S
from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture
from test_gpu_sampling import CASES, DEV, MARGIN, SITES, TEMPS, P, call, case_logits, engine, run_kernel

pytestmark = pytest.mark.gpu

EPS = 1e-5
TOP_PS = (0.25, 0.6, 0.9)
TOP_KS = (0, 5, 16)
MORE_TOP_KS = (1, 4, 8)  # the other register-list widths, at T = 1 and top_p = 0.6


def run_nucleus(x, inv_tau, top_k, top_p, seed, site, want_next=True, want_logp=True, want_count=True, xd=None):
    """the hook on logits x with guard columns and a guard row around every output; returns (tokens
    int64 [R], logp f32 [R] or None, count int32 [R] or None) after checking that nothing else was written"""
    R, V = x.shape
    xd = torch.from_numpy(x).to(DEV) if xd is None else xd
    ids = torch.full((R + 1, 5), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((R + 1, 3), -7, dtype=torch.int32, device=DEV) if want_next else None
    lp = torch.full((R + 1, 4), -123.25, dtype=torch.float32, device=DEV) if want_logp else None
    cnt = torch.full((R + 2,), -7, dtype=torch.int32, device=DEV) if want_count else None
    call("capgen_debug_sample_nucleus", P(xd), R, V, float(inv_tau), top_k, float(top_p), seed, site, P(ids), 5, 2,
         P(nxt), 3, P(lp), 4, 1, C.c_void_p(cnt.data_ptr() + 4) if want_count else None, None)
    ic = ids.cpu()
    assert (ic[:, [0, 1, 3, 4]] == -7).all() and (ic[R] == -7).all(), "ids written outside column `col`"
    if want_next:
        nc = nxt.cpu()
        assert (nc[:, 1:] == -7).all() and (nc[R] == -7).all(), "next_ids written outside column 0"
        assert torch.equal(ic[:R, 2], nc[:R, 0].long())
    out_lp = out_cnt = None
    if want_logp:
        bits = lp.cpu().view(torch.int32)
        guard = torch.tensor([-123.25]).view(torch.int32).item()
        assert (bits[:, [0, 2, 3]] == guard).all() and (bits[R] == guard).all(), "logp written outside its column"
        out_lp = lp.cpu()[:R, 1].numpy()
    if want_count:
        cc = cnt.cpu()
        assert cc[0] == -7 and cc[R + 1] == -7, "count written outside its R entries"
        out_cnt = cc[1:R + 1].numpy()
    return ic[:R, 2].numpy(), out_lp, out_cnt


def determined(x, m, top_p, site, noise, what):
    """(seed, nucleus_ref.band) of the first of sampling_ref.SEEDS that determines every row"""
    for seed in S.SEEDS:
        if noise.get((seed, site)) is None:
            noise[seed, site] = S.gumbel(seed, site, *x.shape)
        b = N.band(m, top_p, EPS, noise[seed, site], MARGIN)
        if b["determined"].all():
            return seed, b
    pytest.fail(f"{what}: no seed determines every row")


def check(tok, lp, cnt, b, what):
    assert np.array_equal(tok, b["token"]), what
    if cnt is not None:
        assert (b["count_lo"] <= cnt).all() and (cnt <= b["count_hi"]).all(), what
    if lp is not None:
        tol = 1e-5 * max(np.abs(b["logp_hi"]).max(), np.finfo(np.float32).tiny)
        lp = lp.astype(np.float64)
        assert (b["logp_hi"] - tol <= lp).all() and (lp <= b["logp_lo"] + tol).all(), what
        assert (lp[b["count_hi"] == 1] == 0).all(), what


@pytest.mark.parametrize("R, V", CASES)
def test_kernel_tokens_logp_and_count(R, V):
    """sample_kernel<40 | 0, KM 0/4/5/8/16, NUCLEUS = true>: exact tokens, |C_lo| <= count <= |C_hi|, logp
    between the restatement's under C_hi and under C_lo (1e-5 of max |logp|), nothing else written;
    next_ids, logp_out and count_out each given and null"""
    x = case_logits(R, V)
    xd = torch.from_numpy(x).to(DEV)
    noise, n, widened = {}, 0, 0
    grid = [(k, t, p) for k in TOP_KS for t in TEMPS for p in TOP_PS] + [(k, 1.0, 0.6) for k in MORE_TOP_KS]
    masses, cands, order = {}, {}, N.ranking(x)
    for top_k, temp, top_p in grid:
        if top_k > V:
            continue
        inv_tau = S.inv_tau_of(temp)
        if (top_k, temp) not in masses:
            if top_k not in cands:
                cands[top_k] = S.candidates(x, top_k)
            masses[top_k, temp] = N.masses(x, inv_tau, top_k, cand=cands[top_k], order=order)
            assert masses[top_k, temp]["kgap"].min() >= MARGIN, f"top_k={top_k}: logits {top_k} and {top_k + 1} tie"
        m = masses[top_k, temp]
        for site in SITES:
            what = f"R={R} V={V} top_k={top_k} T={temp} top_p={top_p} site={site:#x}"
            seed, b = determined(x, m, top_p, site, noise, what)
            widened = max(widened, int((b["count_hi"] - b["count_lo"]).max()))
            want = [n % 4 != 1, n % 4 != 2, n % 4 != 3]
            n += 1
            tok, lp, cnt = run_nucleus(x, inv_tau, top_k, top_p, seed, site, *want, xd=xd)
            check(tok, lp, cnt, b, f"{what} seed={seed:#x}")
    print(f"R={R} V={V}: {n} launches, C_hi \\ C_lo at most {widened} column(s)")


@pytest.mark.parametrize("R, V", CASES)
def test_kernel_top_p_1_is_sample_softmax(R, V):
    """top_p = 1: tokens and logp bit-identical to capgen_debug_sample_softmax, count = V or top_k"""
    x = case_logits(R, V)
    for top_k in (0, 1, 5, 16):
        if top_k > V:
            continue
        inv_tau = S.inv_tau_of(0.7)
        a = run_kernel(x, inv_tau, top_k, S.SEEDS[0], S.SITE0 + 3)
        b = run_nucleus(x, inv_tau, top_k, 1.0, S.SEEDS[0], S.SITE0 + 3)
        assert np.array_equal(a[0], b[0])
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        assert (b[2] == (top_k or V)).all()


@pytest.mark.parametrize("R, V", [(37, 1000), (6, 16388)])
def test_kernel_top_p_below_1_over_v_is_the_argmax(R, V):
    """top_p = 1e-6 < 1 / V: only the row's maximum is left (both kernel forms)"""
    x = case_logits(R, V)
    for top_k in (0, 5):
        for temp in (0.7, 1.5):
            tok, lp, cnt = run_nucleus(x, S.inv_tau_of(temp), top_k, 1e-6, S.SEEDS[1], S.SITE0)
            assert np.array_equal(tok, x.argmax(axis=1))
            assert (lp == 0).all() and (cnt == 1).all()


@pytest.mark.parametrize("R, V", [(37, 1000), (9, 10240), (6, 16388)])
def test_kernel_draw_is_coupled_to_the_untruncated_one(R, V):
    """same seed and site: where the top_p = 1 token lies in C_lo, the nucleus token equals it"""
    x = case_logits(R, V)
    hit = 0
    for top_k in (0, 16):
        m = N.masses(x, 1.0, top_k)
        for top_p in (0.6, 0.9):
            full = run_nucleus(x, 1.0, top_k, 1.0, S.SEEDS[0], S.SITE0)[0]
            cut = run_nucleus(x, 1.0, top_k, top_p, S.SEEDS[0], S.SITE0)[0]
            inside = N.nucleus_set(m, float(np.float32(top_p)) - EPS)[np.arange(R), full]
            hit += int(inside.sum())
            assert np.array_equal(cut[inside], full[inside])
    assert hit >= R, "too few rows whose untruncated token lies in the nucleus"


@pytest.mark.parametrize("V", [1000, 16388])
def test_kernel_tie_group_on_the_boundary_is_kept_whole(V):
    """five bit-identical logits in columns of several threads and waves, top_p set from the
    restatement to the middle of the group's mass: a cut of the sorted row would split the group;
    count holds all five and logp matches"""
    g = torch.Generator(device="cpu").manual_seed(V + 1)
    x = (2 * torch.randn(6, V, generator=g)).numpy()
    first = [3, 200, 255, 256, 700, V - 302]
    group = [[c, c + 1, c + 64, min(c + 300, V - 2), V - 1] for c in first]
    for r, cols in enumerate(group):
        x[r, cols] = 3.0 + 0.25 * r
    noise = {}
    for temp in (0.7, 1.0):
        inv_tau = S.inv_tau_of(temp)
        m = N.masses(x, inv_tau, 0)
        for r, cols in enumerate(group):
            e = math.exp(m["z"][r, cols[0]] - m["z"][r].max())
            top_p = (m["above"][r, cols[0]] + 2.5 * e) / m["P"][r]  # half of the group's mass 5 e
            assert 10 * EPS < top_p < 1 - 10 * EPS and 2.5 * e / m["P"][r] > 10 * EPS
            mr = {k: v[r:r + 1] for k, v in m.items()}
            xr = np.ascontiguousarray(x[r:r + 1])
            for site in SITES:
                seed, b = determined(xr, mr, top_p, site, noise, f"V={V} row {r}")
                assert b["count_lo"][0] == b["count_hi"][0] == int((xr[0] > xr[0, cols[0]]).sum()) + 5
                assert b["C_lo"][0, cols].all()
                tok, lp, cnt = run_nucleus(xr, inv_tau, 0, top_p, seed, site)
                check(tok, lp, cnt, b, f"V={V} row {r} T={temp}")
                assert cnt[0] == b["count_lo"][0]


@pytest.mark.parametrize("R, V", [(5, 24), (37, 1000), (6, 16388)])
def test_kernel_masked_vocabulary(R, V):
    """-inf columns (a masked vocabulary) are never selected; count and logp match the restatement"""
    x = case_logits(R, V).copy()
    masked = np.random.default_rng(V).random((R, V)) < 0.3
    masked[np.arange(R), x.argmax(axis=1)] = False
    x[masked] = -np.inf
    noise = {}
    for top_k in (0, 16):
        with np.errstate(invalid="ignore"):
            m = N.masses(x, 1.0, top_k)
        for top_p in (0.6, 0.999):
            seed, b = determined(x, m, top_p, S.SITE0, noise, f"V={V} top_k={top_k} top_p={top_p}")
            assert not (b["C_hi"] & masked).any()
            tok, lp, cnt = run_nucleus(x, 1.0, top_k, top_p, seed, S.SITE0)
            check(tok, lp, cnt, b, f"V={V} top_k={top_k} top_p={top_p}")
            assert not masked[np.arange(R), tok].any()


def test_kernel_determinism_and_seed_site_dependence():
    x = case_logits(37, 1000)
    for top_k in (0, 8):
        a = run_nucleus(x, 1.0, top_k, 0.9, S.SEEDS[0], S.SITE0)
        b = run_nucleus(x, 1.0, top_k, 0.9, S.SEEDS[0], S.SITE0)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
        assert np.array_equal(a[2], b[2])
        for seed, site in ((S.SEEDS[1], S.SITE0), (S.SEEDS[0], S.SITE0 + 1)):
            c = run_nucleus(x, 1.0, top_k, 0.9, seed, site)
            assert (c[0] != a[0]).any()
            assert np.array_equal(c[2], a[2])  # the candidate set does not depend on the noise


def test_kernel_rejects_bad_arguments():
    x = torch.zeros(2, 8, device=DEV)
    ids = torch.zeros(2, 1, dtype=torch.int64, device=DEV)
    for inv_tau, top_k, top_p, word in ((1.0, 0, 0.0, "top_p"), (1.0, 0, -0.1, "top_p"), (1.0, 4, 1.5, "top_p"),
                                        (1.0, 0, float("nan"), "top_p"), (0.0, 0, 0.9, "temperature"),
                                        (float("nan"), 0, 0.9, "temperature"), (float("inf"), 0, 1.0, "temperature"),
                                        (1.0, 17, 0.9, "top_k"), (1.0, 9, 0.9, "top_k"), (1.0, -1, 1.0, "top_k")):
        with pytest.raises(RuntimeError, match=word):
            call("capgen_debug_sample_nucleus", P(x), 2, 8, inv_tau, top_k, top_p, 1, S.SITE0, P(ids), 1, 0, None, 0,
                 None, 0, 0, None, None)


# ---- engine level ----------------------------------------------------------------------------------

@pytest.mark.parametrize("n, temp, top_k", [(3, 1.0, 0), (2, 0.7, 16)])
@pytest.mark.parametrize("tag", ["c1", "c2s"])
def test_engine_fp32_matches_restatement_on_teacher_forced_logits(tag, n, temp, top_k):
    """The engine's sampled ids (top_p = 0.9) fed back as captions; the restatement on those
    teacher-forced logits.  The decode logits differ from them by about 1e-6, so eps = 1e-4 here, the
    token margin is 1e-3 and logp is held within 1e-3: every token lies in C_hi and its logp between
    the restatement's under C_hi and (where it is in C_lo) under C_lo; every determined position's
    token is exact; at most 2 % of the positions may be undetermined."""
    e, cfg, f, p = engine(tag, "fp32")
    seed, T, top_p = 1234, cfg.max_length, 0.9
    ids, logp = e.sample(f, p, n_samples=n, temperature=temp, top_k=top_k, seed=seed, top_p=top_p)
    B = f.shape[0]
    R = n * B
    assert ids.shape == (n, B, T + 1) and logp.shape == (n, B, T - 1)
    flat = ids.view(R, T + 1)
    assert (flat[:, 0] == 1).all() and (flat[:, T] == 0).all()
    e.forward(f.repeat(n, 1, 1), p.repeat(n, 1, 1), flat[:, :T])
    lg = e.logits(R, T).cpu().numpy()
    got_tok, got_lp = flat[:, 1:T].cpu().numpy(), logp.view(R, T - 1).cpu().numpy().astype(np.float64)
    assert (got_lp <= 0).all()
    rows = np.arange(R)
    left_out = widened = cut = 0
    for t in range(T - 1):
        m = N.masses(np.ascontiguousarray(lg[:, t]), S.inv_tau_of(temp), top_k)
        b = N.band(m, top_p, 1e-4, S.gumbel(seed, S.SITE0 + t, R, cfg.num_vocab), 1e-3)
        solid = m["kgap"] >= 1e-4  # (the top_k set itself is the same on both sets of logits)
        keep = b["determined"] & solid
        left_out += int((~keep).sum())
        widened += int((b["count_hi"] != b["count_lo"]).sum())
        cut += int((b["count_hi"] < m["C0"].sum(axis=1)).sum())
        assert np.array_equal(got_tok[keep, t], b["token"][keep]), t
        assert b["C_hi"][rows, got_tok[:, t]][solid].all(), t
        assert (got_lp[:, t] >= N.logp_at(m, b["C_hi"], got_tok[:, t]) - 1e-3)[solid].all(), t
        in_lo = b["C_lo"][rows, got_tok[:, t]] & solid
        assert (got_lp[in_lo, t] <= N.logp_at(m, b["C_lo"], got_tok[:, t])[in_lo] + 1e-3).all(), t
    total = R * (T - 1)
    print(f"{tag} n={n} T={temp} top_k={top_k}: left out {left_out} of {total}, C_hi != C_lo at {widened}, "
          f"nucleus smaller than C0 at {cut}")
    assert cut > 0
    assert left_out <= 0.02 * total


@pytest.mark.parametrize("tag, dtype", [("c1", "fp32"), ("c2s", "fp32"), ("c2s", "bf16")])
def test_engine_top_p_1_and_tiny_top_p(tag, dtype):
    """top_p = 1.0: ids and logp bit-identical to the call without the keyword; top_p = 1e-6: the
    same engine's greedy caption in every sample row, logp all zero"""
    e, cfg, f, p = engine(tag, dtype)
    for top_k in (0, 8):
        a = e.sample(f, p, n_samples=2, temperature=0.8, top_k=top_k, seed=17)
        b = e.sample(f, p, n_samples=2, temperature=0.8, top_k=top_k, seed=17, top_p=1.0)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    want, _ = e.greedy(f, p, want_attention=False)
    ids, logp = e.sample(f, p, n_samples=2, temperature=0.8, seed=17, top_p=1e-6)
    assert torch.equal(ids[0], want) and torch.equal(ids[1], want)
    assert (logp == 0).all()


def test_engine_bf16_is_deterministic_per_seed():
    e, cfg, f, p = engine("c2s", "bf16")
    a = e.sample(f, p, n_samples=3, seed=5, top_p=0.9)
    b = e.sample(f, p, n_samples=3, seed=5, top_p=0.9)
    c = e.sample(f, p, n_samples=3, seed=6, top_p=0.9)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert (a[1] <= 0).all()
    assert not torch.equal(a[0], c[0])


@pytest.mark.parametrize("top_p", [0.0, -0.1, 1.5, float("nan")])
def test_engine_rejects_bad_top_p(top_p):
    e, cfg, f, p = engine("c1", "fp32")
    with pytest.raises(RuntimeError, match="top_p"):
        e.sample(f, p, top_p=top_p)
    ids, logp = e.sample(f, p, n_samples=1, seed=3, top_p=0.9)  # the engine stays usable
    assert ids.shape == (1, f.shape[0], cfg.max_length + 1) and torch.isfinite(logp).all()


def _vocab(cfg):
    w2i = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    w2i.update({f"w{i}": i for i in range(3, cfg.num_vocab)})
    return w2i


def test_python_sample_captions():
    from capgen.models import TRANSFORMER
    from capgen.utils import sequence_logprob
    cfg, seed, z = load_fixture("c1")
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=_vocab(cfg), device=DEV,
                    state_dict=fixture_state_dict(cfg, seed=seed, with_buffer=False))
    m.model.eval()
    f, p, _ = fixture_inputs(z)
    B, T = f.shape[0], cfg.max_length
    caps, lp = m.sample_captions(f, p, n_samples=3, temperature=0.9, seed=11, top_p=0.9)
    assert len(caps) == 3 and all(len(c) == B and all(isinstance(s, str) for s in c) for c in caps)
    assert lp.shape == (3, B) and (lp <= 0).all()
    ids, logp = m.model.sample_caption_vector(f, p, n_samples=3, temperature=0.9, seed=11, top_p=0.9)
    assert ids.shape == (3, B, T + 1) and logp.shape == (3, B, T - 1)
    assert torch.equal(lp, sequence_logprob(ids[..., 1:T], logp, 2))
    full, full_lp = m.model.sample_caption_vector(f, p, n_samples=3, temperature=0.9, seed=11)
    assert not torch.equal(ids, full)  # (the fixture's distribution is flat: the tail is drawn often)


def test_python_rollout_trainer_passes_top_p():
    from capgen.models import RolloutSelfCritic
    from test_gpu_rollout import case, low_id_share
    cfg, seed, f, p, c = case("c1")
    m = RolloutSelfCritic(cfg.replace(dtype="fp32"), word_to_idx=_vocab(cfg), device=DEV,
                          state_dict=fixture_state_dict(cfg, seed=seed, with_buffer=False), reward_fn=low_id_share,
                          n_samples=2, seed=4, top_p=0.9)
    m.model.eval()
    eng, seen = m.model.engine, []
    inner = eng.sample

    def spy(*a, **kw):
        out = inner(*a, **kw)
        seen.append((kw.get("top_p"), out[0].clone()))
        return out

    eng.sample = spy
    a, b = m.compute_loss(f, p, c), m.compute_loss(f, p, c)
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["reward"], b["reward"])
    fd, pd = f.to(DEV), p.to(DEV)
    assert torch.equal(seen[0][1], inner(fd, pd, 2, seed=4, want_logp=False, top_p=0.9)[0])
    assert not torch.equal(seen[0][1], inner(fd, pd, 2, seed=4, want_logp=False)[0])
    before = eng.state_dict(False)
    m.train_step(f, p, c)
    after = eng.state_dict(False)
    assert any(not torch.equal(before[k], after[k]) for k in before)
    assert [s[0] for s in seen] == [0.9, 0.9, 0.9]
    assert torch.equal(seen[0][1], seen[1][1]) and torch.equal(seen[0][1], seen[2][1])  # (seed 4 each time)
