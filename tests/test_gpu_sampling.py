"""Sampled decoding on the GPU: the selection kernel (sample_softmax, through its C-ABI hook)
against the float64 restatement of its header comment (tests/sampling_ref.py), then capgen_sample
and the Python calls over it on the fixture weights.

Index results follow the project's margin rule: a token is compared where the restatement's own
two best candidates are at least MARGIN apart (asserted on the restatement alone, before the kernel
runs), so f32 rounding in the kernel cannot reorder them."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import sampling_ref as S
from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MARGIN = 1e-4
SITES = (S.SITE0, S.SITE0 + 18)
TEMPS = (0.7, 1.0, 1.5)
TOP_KS = (0, 1, 4, 5, 8, 16)
# the first and last column counts of the register form (V <= 10240), the generic loop, more rows
# than one wave of workgroups
CASES = [(1, 8), (5, 24), (37, 1000), (9, 10240), (130, 10000), (6, 16388)]


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def call(name, *args):
    from capgen import _lib
    _lib.check(getattr(_lib.load(), name)(*args))
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def case_logits(R, V):
    g = torch.Generator(device="cpu").manual_seed(1000 * R + V)
    return (3 * torch.randn(R, V, generator=g)).numpy()


def run_kernel(x, inv_tau, top_k, seed, site, want_next=True, want_logp=True, xd=None):
    """the hook on logits x with guard columns and a guard row around every output; returns
    (tokens int64 [R], logp f32 [R] or None) after checking that nothing else was written"""
    R, V = x.shape
    xd = torch.from_numpy(x).to(DEV) if xd is None else xd
    ids = torch.full((R + 1, 5), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((R + 1, 3), -7, dtype=torch.int32, device=DEV) if want_next else None
    lp = torch.full((R + 1, 4), -123.25, dtype=torch.float32, device=DEV) if want_logp else None
    call("capgen_debug_sample_softmax", P(xd), R, V, float(inv_tau), top_k, seed, site, P(ids), 5, 2, P(nxt), 3,
         P(lp), 4, 1, None)
    ic = ids.cpu()
    assert (ic[:, [0, 1, 3, 4]] == -7).all() and (ic[R] == -7).all(), "ids written outside column `col`"
    if want_next:
        nc = nxt.cpu()
        assert (nc[:, 1:] == -7).all() and (nc[R] == -7).all(), "next_ids written outside column 0"
        assert torch.equal(ic[:R, 2], nc[:R, 0].long())
    out_lp = None
    if want_logp:
        bits = lp.cpu().view(torch.int32)
        guard = torch.tensor([-123.25]).view(torch.int32).item()
        assert (bits[:, [0, 2, 3]] == guard).all() and (bits[R] == guard).all(), "logp written outside its column"
        out_lp = lp.cpu()[:R, 1].numpy()
    return ic[:R, 2].numpy(), out_lp


@pytest.mark.parametrize("R, V", CASES)
def test_kernel_tokens_and_logp(R, V):
    """sample_kernel<40 | 0, KM 0/4/5/8/16, NUCLEUS = false>: exact tokens, logp within 1e-5 of max |logp|,
    nothing else written; next_ids and logp_out each given and null"""
    x = case_logits(R, V)
    xd = torch.from_numpy(x).to(DEV)
    noise = {(seed, site): None for seed in S.SEEDS for site in SITES}
    n = 0
    for top_k in TOP_KS:
        if top_k > V:
            continue
        cand = S.candidates(x, top_k)
        assert cand[1].min() >= MARGIN, f"top_k={top_k}: logits {top_k} and {top_k + 1} are {cand[1].min():.2e} apart"
        for temp in TEMPS:
            inv_tau = S.inv_tau_of(temp)
            for site in SITES:
                for seed in S.SEEDS:  # the first seed whose two best perturbed scores are MARGIN apart
                    if noise[seed, site] is None:
                        noise[seed, site] = S.gumbel(seed, site, R, V)
                    ref = S.sample(x, inv_tau, top_k, seed, site, g=noise[seed, site], cand=cand)
                    if ref["margin"].min() >= MARGIN:
                        break
                else:
                    pytest.fail(f"top_k={top_k} T={temp} site={site:#x}: no seed gives a {MARGIN} margin")
                want_next, want_logp = n % 3 != 1, n % 3 != 2
                n += 1
                tok, lp = run_kernel(x, inv_tau, top_k, seed, site, want_next, want_logp, xd=xd)
                what = f"R={R} V={V} top_k={top_k} T={temp} site={site:#x} seed={seed:#x}"
                assert np.array_equal(tok, ref["token"]), what
                if want_logp:
                    bound = 1e-5 * max(np.abs(ref["logp"]).max(), np.finfo(np.float32).tiny)
                    assert np.abs(lp.astype(np.float64) - ref["logp"]).max() <= bound, what
                    if top_k == 1:
                        assert (lp == 0).all(), what


@pytest.mark.parametrize("V", [1000, 16388])
def test_kernel_ties_take_the_first_index(V):
    """rows whose maximum appears bit-identically in several columns, top_k = 1: the first of them,
    logp exactly 0 (both kernel forms)"""
    g = torch.Generator(device="cpu").manual_seed(V)
    x = (2 * torch.randn(6, V, generator=g)).clamp(max=4.0)
    first = [3, 200, 255, 256, 700, V - 2]
    for r, c in enumerate(first):
        x[r, [c, c + 1, V - 1]] = 6.0
        x[r, min(c + 300, V - 1)] = 6.0
    for temp in (0.7, 1.0):
        tok, lp = run_kernel(x.numpy(), S.inv_tau_of(temp), 1, S.SEEDS[0], S.SITE0)
        assert tok.tolist() == first
        assert (lp == 0).all()


def test_kernel_determinism_and_seed_site_dependence():
    x = case_logits(37, 1000)
    a = run_kernel(x, 1.0, 0, S.SEEDS[0], S.SITE0)
    b = run_kernel(x, 1.0, 0, S.SEEDS[0], S.SITE0)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.int32), b[1].view(np.int32))
    ref = S.sample(x, 1.0, 0, S.SEEDS[0], S.SITE0)["token"]
    for seed, site in ((S.SEEDS[1], S.SITE0), (S.SEEDS[0], S.SITE0 + 1)):
        assert (S.sample(x, 1.0, 0, seed, site)["token"] != ref).any()
        assert (run_kernel(x, 1.0, 0, seed, site)[0] != a[0]).any()


def test_kernel_rejects_bad_arguments():
    x = torch.zeros(2, 8, device=DEV)
    ids = torch.zeros(2, 1, dtype=torch.int64, device=DEV)
    for inv_tau, top_k, word in ((0.0, 0, "temperature"), (float("nan"), 0, "temperature"),
                                 (float("inf"), 0, "temperature"), (1.0, 17, "top_k"), (1.0, 9, "top_k"),
                                 (1.0, -1, "top_k")):
        with pytest.raises(RuntimeError, match=word):
            call("capgen_debug_sample_softmax", P(x), 2, 8, inv_tau, top_k, 1, S.SITE0, P(ids), 1, 0, None, 0, None,
                 0, 0, None)


# ---- engine level ----------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def engine(tag, dtype):
    from capgen.engine import Engine
    cfg, seed, z = load_fixture(tag)
    e = Engine(cfg.replace(dtype=dtype), DEV)
    e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
    e.set_training(False)
    f, p, _ = (t.to(DEV) for t in fixture_inputs(z))
    return e, cfg, f, p


@pytest.mark.parametrize("n, temp", [(3, 1.0), (2, 0.7)])
@pytest.mark.parametrize("tag", ["c1", "c2s"])
def test_engine_fp32_matches_restatement_on_teacher_forced_logits(tag, n, temp):
    """The engine's sampled ids fed back as captions: from those teacher-forced logits the
    restatement reproduces every token whose perturbed top-2 margin is >= m, and every logp within
    1e-3 (the fp32 logit bound).  m = 1e-3 while the decode logits stay within delta of the
    teacher-forced ones with 4 delta / 0.7 <= m (delta from the logp comparison, printed); at most
    2 % of the positions may fall below m."""
    e, cfg, f, p = engine(tag, "fp32")
    seed, T = 1234, cfg.max_length
    ids, logp = e.sample(f, p, n_samples=n, temperature=temp, top_k=0, seed=seed)
    B = f.shape[0]
    R = n * B
    assert ids.shape == (n, B, T + 1) and logp.shape == (n, B, T - 1)
    flat = ids.view(R, T + 1)
    assert (flat[:, 0] == 1).all() and (flat[:, T] == 0).all()
    e.forward(f.repeat(n, 1, 1), p.repeat(n, 1, 1), flat[:, :T])
    lg = e.logits(R, T).cpu().numpy()
    got_tok, got_lp = flat[:, 1:T].cpu().numpy(), logp.view(R, T - 1).cpu().numpy().astype(np.float64)
    refs = [S.sample(lg[:, t], S.inv_tau_of(temp), 0, seed, S.SITE0 + t) for t in range(T - 1)]
    ref_tok = np.stack([r["token"] for r in refs], 1)
    ref_lp = np.stack([r["logp"] for r in refs], 1)
    margin = np.stack([r["margin"] for r in refs], 1)
    delta = np.abs(got_lp - ref_lp).max() * temp
    m = 1e-3
    if 4 * delta / 0.7 > m:
        m = math.ceil(4 * delta / 0.7 * 1e4) / 1e4
    keep = margin >= m
    left_out = int((~keep).sum())
    print(f"{tag} n={n} T={temp}: delta = {delta:.3e}, m = {m:.1e}, left out {left_out} of {keep.size}, "
          f"<NULL> sampled {int((got_tok == cfg.pad_idx).sum())}")
    assert np.array_equal(got_tok[keep], ref_tok[keep])
    assert left_out <= 0.02 * keep.size
    assert np.abs(got_lp - ref_lp).max() <= 1e-3
    assert (got_lp <= 0).all()


@pytest.mark.parametrize("tag, dtype", [("c1", "fp32"), ("c2s", "fp32"), ("c2s", "bf16")])
def test_engine_top_k_1_is_greedy(tag, dtype):
    """top_k = 1: every sample row is the same engine's greedy caption and logp is all zeros (bf16 at
    R = 2 B: the grouped cross-attention and the LayerNorm-fold row thresholds of a multi-row image)"""
    e, cfg, f, p = engine(tag, dtype)
    want, _ = e.greedy(f, p, want_attention=False)
    for temp in (1.0, 0.7):
        ids, logp = e.sample(f, p, n_samples=2, temperature=temp, top_k=1, seed=99)
        assert torch.equal(ids[0], want) and torch.equal(ids[1], want)
        assert (logp == 0).all()


def test_engine_bf16_is_deterministic_per_seed():
    e, cfg, f, p = engine("c2s", "bf16")
    a = e.sample(f, p, n_samples=3, seed=5)
    b = e.sample(f, p, n_samples=3, seed=5)
    c = e.sample(f, p, n_samples=3, seed=6)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    assert (a[1] <= 0).all()
    assert not torch.equal(a[0], c[0])
    ids, none = e.sample(f, p, n_samples=3, seed=5, want_logp=False)
    assert none is None and torch.equal(ids, a[0])


@pytest.mark.parametrize("kw, word", [
    ({"temperature": 0.0}, "temperature"), ({"temperature": -1.0}, "temperature"),
    ({"temperature": float("nan")}, "temperature"), ({"top_k": 17}, "top_k"), ({"top_k": -1}, "top_k"),
    ({"n_samples": 0}, "n_samples"), ({"n_samples": 17}, "n_samples")])
def test_engine_rejects_bad_arguments(kw, word):
    e, cfg, f, p = engine("c1", "fp32")
    with pytest.raises(RuntimeError, match=word):
        e.sample(f, p, **kw)
    ids, logp = e.sample(f, p, n_samples=1, seed=3)  # the engine stays usable
    assert ids.shape == (1, f.shape[0], cfg.max_length + 1) and torch.isfinite(logp).all()


def test_python_api():
    from capgen.models import TRANSFORMER
    from capgen.utils import sequence_logprob
    cfg, seed, z = load_fixture("c1")
    w2i = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    w2i.update({f"w{i}": i for i in range(3, cfg.num_vocab)})
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=w2i, device=DEV,
                    state_dict=fixture_state_dict(cfg, seed=seed, with_buffer=False))
    m.model.eval()
    f, p, _ = fixture_inputs(z)
    B, T = f.shape[0], cfg.max_length
    caps, lp = m.sample_captions(f, p, n_samples=3, temperature=0.9, top_k=8, seed=11)
    assert len(caps) == 3 and all(len(c) == B and all(isinstance(s, str) for s in c) for c in caps)
    ids, logp = m.model.sample_caption_vector(f, p, n_samples=3, temperature=0.9, top_k=8, seed=11)
    assert lp.shape == (3, B)
    assert torch.equal(lp, sequence_logprob(ids[..., 1:T], logp, 2))
    assert caps == [m.decode_captions(ids[j].cpu().numpy()) for j in range(3)]
    torch.manual_seed(77)
    a = m.model.sample_caption_vector(f, p, n_samples=2)
    b = m.model.sample_caption_vector(f, p, n_samples=2)
    torch.manual_seed(77)
    c = m.model.sample_caption_vector(f, p, n_samples=2)
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
    assert not torch.equal(a[0], b[0])
    greedy_caps, _ = m.generate_caption(f, p)  # unchanged beside the new call
    assert len(greedy_caps) == B
