"""The END-aware n-best beam search on the GPU: the step kernels and the finish kernel through their C-ABI
hooks against the float64 restatement of csrc/select.hip's definition (tests/beam_ref.py), then
capgen_beam_nbest and the Python calls over it on the fixture weights.

Kernel cases are drawn from fixed seeds, tried in order until the restatement alone says that every two
consecutive candidates among the first k + 1 of every image lie at least 1e-4 apart (the project's margin
for an f32 selection against an f64 one); the condition is asserted before the kernel runs and no image is
ever left out.  Exact ties are made on purpose, between finished rows only, and must resolve by beam."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
from test_beam_host import C1_END, C2S_END, ref_search
from test_gpu_sampling import DEV, P, call, engine

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
B = 3
KS = (3, 5, 8, 16)  # one per register-list width KM = 4, 5, 8, 16
VS = (40, 1000)     # 40: three slabs, the last one partial
PATTERNS = ("none", "some", "all")
Tw = Tc = 7


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def slab_stats(x):
    """{max, sum exp(v - max)} per row and 16 columns, f32 [rows, ceil(V / 16), 2] (NaN rows stay NaN)"""
    rows, V = x.shape
    S = (V + 15) // 16
    xp = np.full((rows, S * 16), -np.inf, dtype=np.float32)
    xp[:, :V] = x
    xs = xp.reshape(rows, S, 16)
    with np.errstate(invalid="ignore"):
        mx = xs.max(axis=2)
        se = np.exp(xs - mx[:, :, None]).sum(axis=2, dtype=np.float32)
    return np.stack([mx, se], axis=2).astype(np.float32)


def fin_pattern(name, k_in):
    j, i = np.meshgrid(np.arange(k_in), np.arange(B), indexing="ij")
    if name == "none":
        return np.zeros((k_in, B), np.int32)
    if name == "all":
        return np.ones((k_in, B), np.int32)
    return ((j + i) % 3 == 0).astype(np.int32)  # every image: finished and live rows together (k_in >= 3)


@functools.lru_cache(maxsize=None)
def step_case(V, k, k_in, pattern):
    """(logits f32 [k_in * B, V] with NaN rows where finished, prev, fin, len, the restatement's step) of the
    first seed whose restatement has the margin"""
    fin = fin_pattern(pattern, k_in)
    for attempt in range(200):
        g = torch.Generator(device="cpu").manual_seed(7919 * attempt + 13 * V + 3 * k + k_in + len(pattern))
        x = (3 * torch.randn(k_in * B, V, generator=g)).numpy()
        # distinct logp per row, close enough for finished and live rows of every beam to interleave
        prev = (-0.0437 * (np.arange(k_in * B) // B) - 0.0113 * torch.rand(k_in * B, generator=g).numpy())
        prev = prev.astype(np.float32)
        length = torch.randint(0, 10, (k_in, B), generator=g).numpy().astype(np.int32)
        end_id = int(np.argmax(x[0]))  # the best word of row 0: some selected candidates finish
        ls = R.log_softmax64(x.reshape(k_in, B, V))
        x[fin.reshape(-1) != 0] = np.nan
        ref = R.step(ls, prev.astype(np.float64).reshape(k_in, B), fin, length, k, end_id)
        if ref["gaps"].min() >= 2 * MARGIN:
            return x, prev, fin, length, end_id, ref
    raise AssertionError(f"no draw with the margin for V={V} k={k} k_in={k_in} {pattern}")


def step_cases(k):
    """(k_in, pattern): a step needs k candidates per image, so one source row (step 0) is live"""
    yield 1, "none"
    for pattern in PATTERNS:
        yield k, pattern


def run_step(x, prev, fin, length, k_in, V, k, end_id, fused, t=2, hook_ended=True):
    """the hook (or, hook_ended = False, the reference step's hook with logsm = 1) with a guard row after
    every output; -> dict of host arrays.  The fused form's gathers are checked against the sources."""
    R_, Rs = k * B, max(k, k_in) * B
    g = torch.Generator(device="cpu").manual_seed(V + k + t)
    seq_src = torch.randint(100, 10_000, (Rs, Tw), generator=g, dtype=torch.int64)
    ids_src = torch.randint(100, 10_000, (Rs, Tc), generator=g, dtype=torch.int32)
    kv_src = torch.randint(100, 10_000, (Rs, Tc), generator=g, dtype=torch.int32)
    seq_dst = torch.full((R_ + 1, Tw), -7, dtype=torch.int64, device=DEV)
    ids_dst = torch.full((R_ + 1, Tc), -7, dtype=torch.int32, device=DEV)
    kv_dst = torch.full((R_ + 1, Tc), -7, dtype=torch.int32, device=DEV)
    op = torch.full((R_ + 1,), 7.0, device=DEV)
    os_, ot, of, ol = (torch.full((R_ + 1,), -7, dtype=torch.int32, device=DEV) for _ in range(4))
    cv = torch.zeros(k_in * B * k, device=DEV)
    ci = torch.zeros(k_in * B * k, dtype=torch.int32, device=DEV)
    xd, pd = dev(x), dev(prev)
    sd = dev(slab_stats(x)) if fused else None
    fd, ld = dev(fin.reshape(-1)), dev(length.reshape(-1))
    ss, is_, ks = seq_src.to(DEV), ids_src.to(DEV), kv_src.to(DEV)
    if hook_ended:
        call("capgen_debug_beam_step_ended", P(xd), P(sd), P(pd), k_in, B, V, k, end_id, P(fd), P(ld), P(of), P(ol),
             P(cv), P(ci), P(op), P(os_), P(ot), P(ss), P(seq_dst), Tw, P(is_), P(ids_dst), P(ks), P(kv_dst), Tc, t, None)
    elif fused:
        call("capgen_debug_beam_slab_step", P(xd), P(sd), P(pd), k_in, B, V, k, 1, P(op), P(os_), P(ot), P(ss),
             P(seq_dst), Tw, P(is_), P(ids_dst), P(ks), P(kv_dst), Tc, t, None)
    else:
        call("capgen_debug_beam_step_topk", P(xd), None, P(pd), k_in, B, V, k, 1, P(cv), P(ci), P(op), P(os_), P(ot),
             None)
    assert op[R_].item() == 7.0 and os_[R_].item() == -7 and ot[R_].item() == -7
    assert of[R_].item() == -7 and ol[R_].item() == -7
    assert (seq_dst[R_] == -7).all() and (ids_dst[R_] == -7).all() and (kv_dst[R_] == -7).all()
    assert torch.equal(fd.cpu(), torch.from_numpy(fin.reshape(-1))), "fin_src was written"
    assert torch.equal(ld.cpu(), torch.from_numpy(length.reshape(-1))), "len_src was written"
    out = {"prob": op[:R_].cpu().numpy(), "src": os_[:R_].cpu().numpy(), "tok": ot[:R_].cpu().numpy(),
           "fin": of[:R_].cpu().numpy(), "len": ol[:R_].cpu().numpy(), "seq": seq_dst[:R_].cpu(),
           "ids": ids_dst[:R_].cpu(), "kv": kv_dst[:R_].cpu()}
    if fused:  # gathered exactly as capgen_debug_beam_slab_step gathers (test_gpu_rowops.run_slab_step)
        src, tok = out["src"], out["tok"]
        e_seq, e_ids, e_kv = seq_src[:R_].clone(), ids_src[:R_].clone(), kv_src[:R_].clone()
        for j in range(k):
            for i in range(B):
                r, srow = j * B + i, int(src[j * B + i]) * B + i
                e_seq[r], e_ids[r] = seq_src[srow], ids_src[srow]
                e_seq[r, t + 1] = e_ids[r, t + 1] = int(tok[r])
                e_kv[r] = 0
                e_kv[r, :t + 1] = kv_src[srow, :t + 1]
                e_kv[r, t + 1] = r
        assert torch.equal(out["seq"], e_seq) and torch.equal(out["ids"], e_ids) and torch.equal(out["kv"], e_kv)
        assert torch.equal(ss.cpu(), seq_src) and torch.equal(is_.cpu(), ids_src) and torch.equal(ks.cpu(), kv_src)
    else:
        assert (out["seq"] == -7).all() and (out["ids"] == -7).all() and (out["kv"] == -7).all()
    return out


def check_step(tag, out, ref, fin, k):
    assert ref["gaps"].min() >= MARGIN, tag + f": the restatement's own margin is {ref['gaps'].min():.2e}"
    assert np.array_equal(out["src"], ref["src"].reshape(-1)), tag + " source beams"
    assert np.array_equal(out["tok"], ref["tok"].reshape(-1)), tag + " tokens"
    assert np.array_equal(out["fin"], ref["fin"].reshape(-1)), tag + " fin"
    assert np.array_equal(out["len"], ref["len"].reshape(-1)), tag + " len"
    err = np.abs(out["prob"].astype(np.float64) - ref["logp"].reshape(-1)).max()
    assert err <= 1e-5, tag + f": scores off by {err:.2e}"
    from_fin = fin[out["src"].reshape(k, B), np.arange(B)[None, :]] != 0
    assert (out["tok"].reshape(k, B)[from_fin] == 0).all(), tag + ": a finished source appends token 0"


@pytest.mark.parametrize("fused", [False, True], ids=["full_row", "fused_slab"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", VS)
def test_step_matches_restatement(V, k, fused):
    """beam_row_topk_kernel<KM, 20, 512 | 40, 256, true> + beam_merge_ended_kernel, and
    beam_slab_step_kernel<KM, true>: selection, fin / len and (fused) the gathers exact, scores within 1e-5;
    finished rows hold NaN logits and NaN stats"""
    n_fin = 0
    for n, (k_in, pattern) in enumerate(step_cases(k)):
        x, prev, fin, length, end_id, ref = step_case(V, k, k_in, pattern)
        out = run_step(x, prev, fin, length, k_in, V, k, end_id, fused, t=(0, 3)[n % 2])
        check_step(f"V={V} k={k} k_in={k_in} fin={pattern}", out, ref, fin, k)
        n_fin += int(ref["fin"].sum() - (fin[ref["src"], np.arange(B)[None, :]] != 0).sum())
    assert n_fin > 0, "no case finished a hypothesis at this step"
    # no prev (the first step): the row's own scores
    x, _, fin, length, end_id, _ = step_case(V, k, 1, "none")
    ref = R.step(R.log_softmax64(x.reshape(1, B, V)), np.zeros((1, B)), fin, length, k, end_id)
    check_step(f"V={V} k={k} no prev", run_step(x, None, fin, length, 1, V, k, end_id, fused), ref, fin, k)


@pytest.mark.parametrize("fused", [False, True], ids=["full_row", "fused_slab"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("V", VS)
def test_step_with_nothing_finished_is_the_reference_step_bit_for_bit(V, k, fused):
    """fin all zero: out_prob / src / tok (and the fused form's gathers, checked inside run_step against the
    same expectation) equal capgen_debug_beam_step_topk(logsm = 1) / capgen_debug_beam_slab_step"""
    for k_in in (1, k):
        x, prev, fin, length, _, _ = step_case(V, k, k_in, "none")
        a = run_step(x, prev, fin, length, k_in, V, k, -1, fused)
        b = run_step(x, prev, fin, length, k_in, V, k, -1, fused, hook_ended=False)
        assert np.array_equal(a["prob"].view(np.int32), b["prob"].view(np.int32)), (V, k, k_in)
        assert np.array_equal(a["src"], b["src"]) and np.array_equal(a["tok"], b["tok"])
        assert torch.equal(a["seq"], b["seq"]) and torch.equal(a["ids"], b["ids"]) and torch.equal(a["kv"], b["kv"])
        assert (a["fin"] == 0).all() and np.array_equal(a["len"], (length[a["src"].reshape(k, B), np.arange(B)] + 1).reshape(-1))


@pytest.mark.parametrize("fused", [False, True], ids=["full_row", "fused_slab"])
def test_step_finished_rows_with_equal_logp_keep_beam_order(fused):
    V, k = 40, 3
    x, prev, _, length, end_id, _ = step_case(V, k, k, "none")
    x, prev = x.copy(), prev.copy()
    fin = np.array([[1, 0, 1], [0, 1, 1], [1, 1, 1]], np.int32)  # image 0: beams 0, 2; image 1: 1, 2; image 2: all
    prev[:] = np.float32(-0.25)  # bit-equal everywhere: finished rows lead, live ones follow
    ls = R.log_softmax64(x.reshape(k, B, V))
    x[fin.reshape(-1) != 0] = np.nan
    ref = R.step(ls, prev.astype(np.float64).reshape(k, B), fin, length, k, end_id)
    assert ref["src"][:, 0].tolist()[:2] == [0, 2] and ref["src"][:, 1].tolist()[:2] == [1, 2]
    assert ref["src"][:, 2].tolist() == [0, 1, 2] and ref["gaps"][2, 0] == 0.0
    assert ((ref["gaps"] == 0) | (ref["gaps"] >= MARGIN)).all()  # (nothing else is close)
    out = run_step(x, prev, fin, length, k, V, k, end_id, fused)
    for name in ("src", "tok", "fin", "len"):
        assert np.array_equal(out[name], ref[name].reshape(-1)), name
    finished = out["fin"].reshape(k, B)[:2] == 1
    assert (out["prob"].reshape(k, B)[:2][finished].view(np.int32) == np.float32(-0.25).view(np.int32)).all()


def run_finish(seq, logp, length, k, Bn, T, alpha, n_best, want=(True, True, True)):
    Ro = n_best * Bn
    ids = torch.full((Ro + 1, T), -7, dtype=torch.int64, device=DEV)
    sc = torch.full((Ro + 1,), 7.0, device=DEV) if want[0] else None
    lp = torch.full((Ro + 1,), 7.0, device=DEV) if want[1] else None
    ln = torch.full((Ro + 1,), -7, dtype=torch.int32, device=DEV) if want[2] else None
    sd, pd, ld = dev(seq), dev(logp), dev(length)  # (held until the call has run)
    call("capgen_debug_beam_finish", P(sd), P(pd), P(ld), k, Bn, T, float(alpha), n_best, P(ids), P(sc), P(lp), P(ln),
         None)
    assert (ids[Ro] == -7).all()
    for t_, guard in ((sc, 7.0), (lp, 7.0), (ln, -7)):
        assert t_ is None or t_[Ro].item() == guard
    host = lambda t_: None if t_ is None else t_[:Ro].cpu().numpy().reshape(n_best, Bn)  # noqa: E731
    return ids[:Ro].cpu().numpy().reshape(n_best, Bn, T), host(sc), host(lp), host(ln)


@functools.lru_cache(maxsize=None)
def finish_case(k):
    """k hypotheses of 5 images with lengths 0 and 1 among them and, from k = 3, one exact tie per image;
    the first seed whose other final scores are >= 1e-4 apart at every alpha"""
    Bn, T = 5, 9
    for attempt in range(200):
        g = torch.Generator(device="cpu").manual_seed(31 * attempt + k)
        logp = (-20 * torch.rand(k, Bn, generator=g)).numpy().astype(np.float32)
        length = torch.randint(0, 13, (k, Bn), generator=g).numpy().astype(np.int32)
        length[0, 0], length[min(1, k - 1), 1] = 0, 1
        if k >= 3:
            for i in range(Bn):  # beam a's (logp, len) copied to the last beam: one score bit for bit
                a = i % 2
                logp[k - 1, i], length[k - 1, i] = logp[a, i], length[a, i]
        seq = torch.randint(0, 1000, (k * Bn, T), generator=g, dtype=torch.int64).numpy()
        ok = True
        for alpha in (0.0, 0.7, 1.0):
            s = R.finish(logp, length, alpha, k)["score"]
            d = -np.diff(s, axis=0)
            ok &= bool(((d == 0) | (d >= MARGIN)).all())
        if ok:
            return seq, logp, length, Bn, T
    raise AssertionError(f"no draw with the margin for k={k}")


@pytest.mark.parametrize("alpha", [0.0, 0.7, 1.0])
@pytest.mark.parametrize("k", [1, 3, 16])
def test_finish_kernel(k, alpha):
    """beam_finish_kernel<NORM>: exact order (ties by beam index), score within 1e-6 relative, logp / len /
    tokens of the ranked hypothesis, alpha = 0 bit-equal to logp; every output given and null"""
    seq, logp, length, Bn, T = finish_case(k)
    for n, n_best in enumerate(sorted({1, k})):
        ref = R.finish(logp, length, alpha, n_best)
        if k >= 3:
            assert ref["final_margin"].min() == 0.0, "the case holds no exact tie"
        want = (n != 1, True, n != 1) if n else (True, True, True)
        ids, sc, lp, ln = run_finish(seq, logp, length, k, Bn, T, alpha, n_best, want)
        exp_ids = np.take_along_axis(seq.reshape(k, Bn, T), ref["order"][:, :, None], 0)
        assert np.array_equal(ids, exp_ids), (k, alpha, n_best)
        assert np.array_equal(lp.view(np.int32), np.take_along_axis(logp, ref["order"], 0).view(np.int32))
        if ln is not None:
            assert np.array_equal(ln, ref["len"])
        if sc is not None:
            rel = np.abs(sc.astype(np.float64) - ref["score"]) / np.abs(ref["score"])
            assert rel.max() <= 1e-6, (k, alpha, rel.max())
            if alpha == 0.0:
                assert np.array_equal(sc.view(np.int32), lp.view(np.int32))
    ids, sc, lp, ln = run_finish(seq, logp, length, k, Bn, T, alpha, 1, (False, False, False))
    assert np.array_equal(ids, np.take_along_axis(seq.reshape(k, Bn, T), R.finish(logp, length, alpha, 1)["order"][:, :, None], 0))


def test_bad_arguments_name_the_argument():
    from capgen import _lib
    lib = _lib.load()
    seq, logp, length, Bn, T = finish_case(3)
    sd, ld, nd = dev(seq), dev(logp), dev(length)
    ids = torch.zeros(3 * Bn, T, dtype=torch.int64, device=DEV)

    def finish_err(k, alpha, n_best):
        rc = lib.capgen_debug_beam_finish(P(sd), P(ld), P(nd), k, Bn, T, C.c_float(alpha), n_best, P(ids), None, None,
                                          None, None)
        assert rc != 0
        return lib.capgen_last_error().decode()

    assert "n_best" in finish_err(3, 0.0, 0) and "n_best" in finish_err(3, 0.0, 4)
    assert "beam_size" in finish_err(17, 0.0, 1)
    for alpha in (-0.5, float("nan"), float("inf")):
        assert "length_penalty" in finish_err(3, alpha, 1)
    x, prev, fin, length, _, _ = step_case(40, 3, 3, "none")
    for fused in (False, True):
        with pytest.raises(RuntimeError, match="end_id"):
            run_step(x, prev, fin, length, 3, 40, 3, 40, fused)
        with pytest.raises(RuntimeError, match="end_id"):
            run_step(x, prev, fin, length, 3, 40, 3, -2, fused)
    e, cfg, f, p = engine("c1", "fp32")
    Bi, N, T = f.shape[0], f.shape[1], cfg.max_length
    out = torch.zeros(16 * Bi, T, dtype=torch.int64, device=DEV)

    def engine_err(k, end_id, alpha, n_best, n=N):
        rc = lib.capgen_beam_nbest(e.h, P(f), _lib.F32, P(p), Bi, n, k, end_id, C.c_float(alpha), n_best, P(out), None,
                                   None, None, None)
        assert rc != 0
        return lib.capgen_last_error().decode()

    assert "beam_size" in engine_err(0, 5, 0.0, 1) and "beam_size" in engine_err(17, 5, 0.0, 1)
    assert "n_best" in engine_err(3, 5, 0.0, 0) and "n_best" in engine_err(3, 5, 0.0, 4)
    assert "end_id" in engine_err(3, -2, 0.0, 1) and "end_id" in engine_err(3, cfg.num_vocab, 0.0, 1)
    assert "length_penalty" in engine_err(3, 5, -1.0, 1) and "length_penalty" in engine_err(3, 5, float("nan"), 1)
    assert "N " in engine_err(3, 5, 0.0, 1, n=65)
    with pytest.raises(ValueError, match="n_best"):
        e.beam_nbest(f, p, 3, 5, n_best=4)


# ---- the engine ----------------------------------------------------------------------------------------
# (test_gpu_sampling.engine keeps one engine per (fixture, dtype) for the whole run: never closed here)
def structural(ids, score, logp, length, end_id, T):
    ids, length = ids.cpu().numpy(), length.cpu().numpy()
    R.structure_ok(ids, length, end_id, T)
    assert (np.diff(score.cpu().numpy(), axis=0) <= 0).all(), "scores increase down the list"
    return ids, score.cpu().numpy(), logp.cpu().numpy(), length


@pytest.mark.parametrize("k, alpha, n_best", [(3, 0.0, 3), (3, 1.0, 3), (5, 0.0, 5), (5, 0.7, 2)])
def test_engine_fp32_c1_matches_restatement(k, alpha, n_best):
    e, cfg, f, p = engine("c1", "fp32")
    T = cfg.max_length
    _, st = ref_search("c1", k, C1_END)
    ref = R.nbest(st, alpha, n_best)
    ids, score, logp, length = structural(*e.beam_nbest(f, p, k, C1_END, alpha, n_best), C1_END, T)
    assert ids.shape == (n_best, 8, T) and score.shape == logp.shape == length.shape == (n_best, 8)
    same = (ids == ref["ids"]).all(axis=2)
    delta = float(np.abs(logp - ref["logp"])[same].max()) if same.any() else float("inf")
    m = max(1e-3, 4 * delta)
    keep = ref["margin"] >= m
    print(f"k={k} alpha={alpha} n_best={n_best}: delta {delta:.3e}, m {m:.3e}, smallest reference margin "
          f"{ref['margin'].min():.3e}, {int((~keep).sum())} of 8 images left out")
    assert (~keep).sum() <= 2
    assert np.array_equal(ids[:, keep], ref["ids"][:, keep])  # (tokens and their order down the list)
    assert np.array_equal(length[:, keep], ref["len"][:, keep])
    assert np.abs(logp[:, keep] - ref["logp"][:, keep]).max() <= 1e-3
    assert np.abs(score[:, keep] - ref["score"][:, keep]).max() <= 1e-3


@pytest.mark.parametrize("tag, dtype", [("c1", "fp32"), ("c2s", "fp32"), ("c2s", "bf16")])
def test_engine_without_end_is_the_log_softmax_beam(tag, dtype):
    """end_id = -1, alpha = 0, n_best = 1: the same kernels on live rows as beam() after
    set_decode_log_softmax(True) -- equality, not a margin.  (The flag is switched off again before the new
    call: it must not matter.)"""
    e, cfg, f, p = engine(tag, dtype)
    k = 3
    e.set_decode_log_softmax(True)
    want = e.beam(f, p, k).cpu()
    e.set_decode_log_softmax(False)
    ids, score, logp, length = e.beam_nbest(f, p, k, -1, 0.0, 1)
    assert torch.equal(ids[0].cpu(), want)
    assert (length.cpu() == cfg.max_length - 1).all() and torch.equal(score.cpu(), logp.cpu())


def test_engine_bf16_c2s_finishes_like_fp32():
    """bf16, c2s, <END> = 840, k = 3: every hypothesis finishes by length 2.  Tokens, len and order equal the
    fp32 engine's if the restatement's margin (0.033) exceeds the measured bf16 error eps = 2 x the largest
    bf16 - fp32 logit difference teacher-forced on these sequences; otherwise only the structure is asserted.
    Measured on an MI355X: eps 6.8e-2 against the margin 3.3e-2, so the equality is not asserted there (the
    two engines' tokens, len and order were nevertheless equal)."""
    e32, cfg, f, p = engine("c2s", "fp32")
    e16, _, _, _ = engine("c2s", "bf16")
    T, k = cfg.max_length, 3
    _, st = ref_search("c2s", k, C2S_END)
    margin = float(R.nbest(st, 0.0, k)["margin"].min())
    r32 = e32.beam_nbest(f, p, k, C2S_END, 0.0, k)
    r16 = e16.beam_nbest(f.bfloat16(), p, k, C2S_END, 0.0, k)
    ids32, _, _, len32 = structural(*r32, C2S_END, T)
    ids16, _, _, len16 = structural(*r16, C2S_END, T)
    assert len16.max() <= 2 and len32.max() <= 2
    eps = 0.0
    for j in range(k):  # teacher-forced on the fp32 engine's sequences (0 = <NULL> after <END>)
        caps = r32[0][j].to(torch.int32).contiguous()
        e32.forward(f, p, caps)
        l32 = e32.logits(caps.shape[0], T)[:, :2]  # (the steps any hypothesis was live at)
        e16.forward(f.bfloat16(), p, caps)
        l16 = e16.logits(caps.shape[0], T)[:, :2]
        eps = max(eps, 2.0 * (l16 - l32).abs().max().item())
    equal = np.array_equal(ids16, ids32) and np.array_equal(len16, len32)
    print(f"bf16 c2s: eps {eps:.3e}, restatement margin {margin:.3e}, tokens / len / order equal: {equal}")
    if eps < margin:
        assert equal


def test_engine_bf16_full_row_path_equals_the_fused_step(set_knob):
    """CAPGEN_FUSED_BEAM_STEP=0: the bf16 engine's beam_nbest runs the full-row END-aware kernels on the
    same f32 logits the fused slab step reads.  The two differ by the f32 rounding of one exp-sum per step
    (different summation orders), far below c2s's 0.033 margin: tokens, len and order equal, logp within the
    project's f32 margin 1e-4."""
    from capgen.engine import Engine
    from capgen.params import fixture_state_dict
    from golden_util import load_fixture
    e16, _, f, p = engine("c2s", "bf16")
    fused = e16.beam_nbest(f.bfloat16(), p, 3, C2S_END, 1.0, 3)
    cfg, seed, _ = load_fixture("c2s")
    set_knob("FUSED_BEAM_STEP", 0)
    e = Engine(cfg.replace(dtype="bf16"), DEV)
    e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
    e.set_training(False)
    full = e.beam_nbest(f.bfloat16(), p, 3, C2S_END, 1.0, 3)
    assert torch.equal(full[0], fused[0]) and torch.equal(full[3], fused[3])
    assert (full[2] - fused[2]).abs().max().item() <= 1e-4 and (full[1] - fused[1]).abs().max().item() <= 1e-4
    e.close()


def test_engine_repeatable_and_python_api():
    e, cfg, f, p = engine("c1", "fp32")
    a = e.beam_nbest(f, p, 5, C1_END, 0.7, 5)
    b = e.beam_nbest(f, p, 5, C1_END, 0.7, 5)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    from capgen import _lib
    _lib.hazard_start()  # the launch log covers the new state arrays: no unordered conflicting pair
    try:
        c = e.beam_nbest(f, p, 5, C1_END, 0.7, 5)
        torch.cuda.synchronize()
        n, report = _lib.hazard_check()
    finally:
        _lib.hazard_stop()
    assert n == 0, report
    assert all(torch.equal(x, y) for x, y in zip(a, c))
    from capgen.models import TRANSFORMER
    words = {f"w{i}": i for i in range(cfg.num_vocab)}
    words.pop("w0"), words.pop("w1"), words.pop(f"w{C1_END}")
    words.update({"<NULL>": 0, "<START>": 1, "<END>": C1_END})
    m = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=words, device=DEV, state_dict=e.state_dict())
    m.model.eval()
    caps, score = m.beam_captions(f, p, beam_size=3, length_penalty=1.0, n_best=2)
    assert len(caps) == 2 and all(len(c) == 8 and all(isinstance(s, str) for s in c) for c in caps)
    assert score.shape == (2, 8) and score.dtype == torch.float32
    ids, want, _, _ = e.beam_nbest(f, p, 3, C1_END, 1.0, 2)
    assert torch.equal(score.cpu(), want.cpu())
    assert caps[0] == m.decode_captions(ids[0].cpu().numpy())
    assert any(s.endswith(".") for s in caps[0])  # (a finished caption decodes through <END>)
