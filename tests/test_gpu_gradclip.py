"""Run-time learning rate and global-norm gradient clipping (capgen_set_lr, capgen_set_grad_clip,
capgen_last_grad_norm), on the GPU.

Kernel level, through the capgen_debug_grad_norm / capgen_debug_adam_scaled hooks against float64 torch
on the CPU.  The sum of squares is accumulated in double (the square of an f32 is exact there; the
sum's own error ~ n 2^-53 is far below everything else), so the reported norm differs from the float64
norm by its final rounding to f32 plus one ulp for the sqrt: REL = 2 * 2^-23 relative.  The coefficient
min(1, max_norm / (norm + 1e-6)) inherits the norm's rounding and adds its own: the same bound.

Engine level: fp32 on the c2s / c1 fixtures with dropout off unless a case says otherwise; tolerances
are those of the tests each case is modelled on (named in its docstring)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from capgen.params import fixture_state_dict
from golden_util import load_fixture
from test_gpu_hazard import _engine as _bf16_engine
from test_gpu_hazard import _inputs as _bf16_inputs
from test_gpu_hazard import _logged_run
from test_gpu_parity import _engine, _inputs, _params_close, _sharded_update_check
from test_gpu_rollout import WEIGHTS, case
from test_gpu_rowops import (B1, B2, DEV, EPS, F32, LR, P, _lib_, adam_inputs, adam_ref, assert_close, assert_same,
                             call, dev, tiled_index)

pytestmark = pytest.mark.gpu

REL = 2 * 2.0 ** -23
INF = float("inf")


def f32(x):
    return float(np.float32(x))


# ---- kernel level: the norm --------------------------------------------------------------------------
def norm_slots(n, grid_cap):
    """workgroups of the sum-of-squares kernel: 4096 elements per pass, one per CU unless capped"""
    return min((n // 4 + 1023) // 1024, grid_cap if grid_cap > 0 else 256)


def run_norm(gd, max_norm, grid_cap=0):
    """{norm, coef} of the device tensor gd; the guard words after both buffers must survive"""
    n = gd.numel()
    cap = norm_slots(n, grid_cap)
    part = torch.full((cap + 2,), 7.0, dtype=torch.float64, device=DEV)
    out = torch.full((4,), 7.0, device=DEV)
    call("capgen_debug_grad_norm", P(gd), n, C.c_float(max_norm), grid_cap, P(part), cap, P(out), None)
    assert (part[cap:] == 7.0).all(), "a partial sum was written past the slots"
    assert (out[2:] == 7.0).all(), "written past {norm, coef}"
    return out[:2].cpu()


def norm_case(n, kind):
    g = adam_inputs(n, n)[1][2]
    if kind == "big":      # its square overflows f32, not double
        g[n // 2] = 1e20
    elif kind == "tiny":   # every square underflows f32
        g = torch.full((n,), 1e-30)
    elif kind == "inf":
        g[n - 3] = INF
    elif kind == "nan":
        g[n - 3] = float("nan")
    return g


def coef_formula(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


@pytest.mark.parametrize("kind", ["adam", "big", "tiny", "inf", "nan"])
@pytest.mark.parametrize("n", [4, 4100, 1_048_580])
def test_grad_norm_kernels(n, kind):
    """test_adam's sizes: one vector, a ragged last pass, 128 grid-stride passes (grid_cap = 2)"""
    g = norm_case(n, kind)
    gd = dev(g)
    cap = 2 if n > 100_000 else 0
    ref = g.double().norm().item()
    if kind in ("inf", "nan"):
        norm, coef = run_norm(gd, 1.0, cap).tolist()
        if kind == "inf":
            assert norm == INF and coef == 0.0, (norm, coef)  # torch: 1 / (inf + 1e-6)
        else:
            assert math.isnan(norm) and math.isnan(coef), (norm, coef)
        return
    assert math.isfinite(ref) and ref > 0
    if kind == "big":
        assert abs(ref - 1e20) < 1e-6 * 1e20
    if kind == "tiny":
        assert abs(ref - 2e-30 * math.sqrt(n / 4)) < 1e-6 * ref
    clip = f32(0.5 * ref)
    out = run_norm(gd, clip, cap)
    norm, coef = out.double().tolist()
    want = coef_formula(ref, clip)
    print(f"n={n} {kind}: norm {norm:.9e} ref {ref:.9e} rel {abs(norm - ref) / ref:.2e}; "
          f"coef {coef:.9e} ref {want:.9e} rel {abs(coef - want) / want:.2e}")
    assert abs(norm - ref) <= REL * ref, (norm, ref)
    assert want < 1.0 and abs(coef - want) <= REL * want, (coef, want)
    again = run_norm(gd, clip, cap)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)), "two runs over one buffer differ"
    # measure only, and a bound the norm does not reach: exactly 1.  "Does not reach" is max_norm >= norm +
    # 1e-6, the formula's (and torch's) own epsilon: with the all-1e-30 vector, max_norm = 2 norm = 4e-30
    # gives 4e-30 / (2e-30 + 1e-6) = 4e-24 under clip_grad_norm_ too
    for loose in (INF, f32(2.0 * ref + 1e-5)):
        assert coef_formula(ref, loose) == 1.0
        o = run_norm(gd, loose, cap)
        assert o[1].item() == 1.0 and o[0].item() == out[0].item(), (loose, o)


def test_grad_norm_rejects_bad_arguments():
    _lib, lib = _lib_()
    g = torch.ones(4096 * 3, device=DEV)
    part = torch.zeros(8, dtype=torch.float64, device=DEV)
    out = torch.full((2,), 7.0, device=DEV)
    fn = lib.capgen_debug_grad_norm
    one = C.c_float(1.0)
    assert fn(P(g), 6, one, 0, P(part), 8, P(out), None) == 1            # n % 4 != 0
    assert fn(None, 8, one, 0, P(part), 8, P(out), None) == 1            # null pointers
    assert fn(P(g), 8, one, 0, None, 8, P(out), None) == 1
    assert fn(P(g), 8, one, 0, P(part), 8, None, None) == 1
    assert fn(P(g), g.numel(), one, 0, P(part), 2, P(out), None) == 1    # 3 workgroups, 2 slots
    assert fn(P(g), 8, C.c_float(-1.0), 0, P(part), 8, P(out), None) == 1
    assert b"partials" in lib.capgen_last_error() or b"max_norm" in lib.capgen_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (part == 0).all()
    assert fn(P(g), g.numel(), one, 0, P(part), 3, P(out), None) == 0
    torch.cuda.synchronize()
    assert abs(out[0].item() - math.sqrt(g.numel())) <= REL * math.sqrt(g.numel())


# ---- kernel level: Adam with a gradient scale ---------------------------------------------------------
def adam_bufs(n, p0, n_shadow, tiles):
    pd = torch.cat([dev(p0), torch.full((4,), 7.0, device=DEV)])
    md, vd = torch.zeros(n + 4, device=DEV), torch.zeros(n + 4, device=DEV)
    sh = torch.full((n + 4,), 7.0, dtype=torch.bfloat16, device=DEV)
    step = torch.zeros(2, dtype=torch.int64, device=DEV)
    scal = torch.zeros(3, device=DEV)
    dsts = [torch.full((ln + 8,), 7.0, dtype=torch.bfloat16, device=DEV) for _, ln in tiles]
    return dict(p=pd, m=md, v=vd, sh=sh, step=step, scal=scal, dsts=dsts, n_shadow=n_shadow, tiles=tiles)


def adam_call(b, n, gd, grid_cap, gscale=None):
    tiles = b["tiles"]
    offs = (C.c_int64 * 4)(*[o for o, _ in tiles])
    lens = (C.c_int64 * 4)(*[ln for _, ln in tiles])
    ptrs = (C.c_void_p * 4)(*[d_.data_ptr() for d_ in b["dsts"]])
    args = [P(b["p"]), P(gd), P(b["m"]), P(b["v"]), n, C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(EPS),
            P(b["step"]), P(b["scal"]), P(b["sh"]) if b["n_shadow"] else None, b["n_shadow"], grid_cap, len(tiles),
            offs, lens, ptrs]
    if gscale is None:
        call("capgen_debug_adam", *args, None)
    else:
        call("capgen_debug_adam_scaled", *args, P(gscale), None)


@pytest.mark.parametrize("n", [4, 4100, 1_048_580])
def test_adam_scaled_by_one_is_bit_identical(n):
    """*gscale = 1.0f: p, m, v, the bf16 shadow and the tiled copies equal capgen_debug_adam's bit for
    bit over three steps (x * 1.0f == x), and nothing is written past a buffer."""
    p0, grads = adam_inputs(n, n)
    big = n > 100_000
    tiles = [(0, 16 * 512), (16 * 512 + 12, 32 * 512)] if big else []
    a, b = adam_bufs(n, p0, n, tiles), adam_bufs(n, p0, n, tiles)
    one = torch.ones(1, device=DEV)
    for t in range(3):
        gd = dev(grads[t])
        adam_call(a, n, gd, 2 if big else 0)
        adam_call(b, n, gd, 2 if big else 0, gscale=one)
        for k in ("p", "m", "v"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (t, k)
        assert torch.equal(a["sh"].view(torch.int16), b["sh"].view(torch.int16)), (t, "shadow")
        for x, y in zip(a["dsts"], b["dsts"]):
            assert torch.equal(x.view(torch.int16), y.view(torch.int16)), (t, "tiled copy")
        assert b["step"][0].item() == t + 1 and b["step"][1].item() == 0 and b["scal"][2].item() == 0
        assert (b["p"][n:] == 7.0).all() and (b["m"][n:] == 0).all() and (b["v"][n:] == 0).all()
    assert one.item() == 1.0


@pytest.mark.parametrize("n", [4, 4100, 1_048_580])
def test_adam_scaled_by_a_real_clip(n):
    """Three steps whose coefficient comes from capgen_debug_grad_norm with max_norm = 0.5 * norm, against
    adam_ref fed coef64 * g (coef64: the formula in float64), with test_adam's own bounds: parameters
    1e-6 max|p| + 1e-6 lr, moments 1e-5 max|ref|; the shadow is bf16 of the parameters written.

    What the one extra f32 multiplication costs, from restating the kernel's f32 arithmetic in torch on
    the CPU (before the first GPU run) once with the f32 product g * coef and once with the correctly
    rounded float64 product: the two differ by at most 0.0005 of the parameter bound, 0.013 of exp_avg's
    and 0.027 of exp_avg_sq's (n = 4, step 1; at n = 1_048_580 the coefficient is exactly 0.5 and the
    product exact), while the whole f32 restatement uses up to 0.11 of the parameter bound.  Under a
    tenth everywhere: the bounds stand as they are."""
    p0, grads = adam_inputs(n, n)
    big = n > 100_000
    b = adam_bufs(n, p0, n, [])
    scaled, coefs = [], []
    out = []
    for t in range(3):
        gd = dev(grads[t])
        ref_norm = grads[t].double().norm().item()
        clip = f32(0.5 * ref_norm)
        o = torch.zeros(2, device=DEV)
        part = torch.zeros(256, dtype=torch.float64, device=DEV)
        call("capgen_debug_grad_norm", P(gd), n, C.c_float(clip), 2 if big else 0, P(part), 256, P(o), None)
        adam_call(b, n, gd, 2 if big else 0, gscale=o[1:])
        c64 = coef_formula(ref_norm, clip)
        assert abs(o[1].item() - c64) <= REL * c64
        scaled.append(c64 * grads[t].double())
        coefs.append(c64)
        out.append((b["p"][:n].cpu().double(), b["m"][:n].cpu().double(), b["v"][:n].cpu().double(),
                    b["sh"].cpu(), b["p"].cpu()))
    ref = adam_ref(p0.double(), scaled)
    for t in range(3):
        rp, rm, rv = ref[t]
        got, gm, gv, sh, pall = out[t]
        bound = 1e-6 * rp.abs().max().item() + 1e-6 * LR
        err = (got - rp).abs().max().item()
        print(f"n={n} step {t + 1}: coef {coefs[t]:.6f}, parameter error {err:.3e} of bound {bound:.3e}")
        assert err <= bound, (t, err, bound)
        assert_close(gm, rm, F32, f"step {t + 1} exp_avg")
        assert_close(gv, rv, F32, f"step {t + 1} exp_avg_sq")
        assert_same(sh[:n], pall[:n].bfloat16(), "shadow")
        assert (sh[n:] == 7.0).all() and (pall[n:] == 7.0).all()
    assert torch.equal(b["p"][:n].cpu()[0::7], p0[0::7]), "a parameter whose gradient was always 0 moved"


def test_adam_scaled_rejects_bad_arguments():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    args = [C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(EPS), P(st), P(z)]
    fn = lib.capgen_debug_adam_scaled
    assert fn(P(z), P(z), P(z), P(z), 6, *args, None, 0, 0, 0, None, None, None, P(z), None) == 1
    assert fn(P(z), P(z), P(z), P(z), 8, *args, None, 0, 0, 5, None, None, None, P(z), None) == 1
    assert fn(P(z), P(z), P(z), P(z), 8, *args, None, 0, 0, 0, None, None, None, None, None) == 1  # null gscale
    torch.cuda.synchronize()
    assert st.item() == 0


# ---- engine level ------------------------------------------------------------------------------------
def _adam_arenas(e):
    """(step, exp_avg arena, exp_avg_sq arena) of an engine, as host arrays"""
    torch.cuda.synchronize()
    step = C.c_int64(0)
    m = np.empty(e.arena_elems, np.float32)
    v = np.empty(e.arena_elems, np.float32)
    _lib, lib = _lib_()
    _lib.check(lib.capgen_get_adam_state(e.h, C.byref(step), m.ctypes.data_as(C.c_void_p),
                                         v.ctypes.data_as(C.c_void_p), e.arena_elems))
    return step.value, m, v


def _host_norm(arena):
    return float(np.sqrt((arena.astype(np.float64) ** 2).sum()))


def _probe_norm(e, f, p, c):
    """the gradient norm of the engine's current state (forward + backward change nothing else)"""
    e.forward(f, p, c)
    e.backward()
    return _host_norm(e.grads_arena())


@pytest.mark.parametrize("tag", ["c2s", "c1"])
def test_unbucketed_clip_matches_torch(tag):
    """forward, backward, set_grad_clip(0.5 * norm), adam_step against float64 clip_grad_norm_ + Adam on
    the very gradients the kernel read: parameters within 1e-6 max|p| (_params_close's tolerance in
    test_gpu_parity.py), the reported norm within REL of the host norm of that arena."""
    cfg, seed, z = load_fixture(tag)
    e = _engine(cfg, seed)
    e.set_training(False)
    f, p, c = _inputs(z)
    e.forward(f, p, c)
    e.backward()
    g, p0 = e.grads_arena(), e.params_arena()
    host = _host_norm(g)
    clip = f32(0.5 * host)
    e.set_grad_clip(clip)
    e.adam_step()
    got = e.params_arena().astype(np.float64)
    norm = e.grad_norm()
    print(f"{tag}: norm {norm:.9e}, host {host:.9e}, rel {abs(norm - host) / host:.2e}")
    assert abs(norm - host) <= REL * host, (norm, host)
    q = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    q.grad = torch.tensor(g, dtype=torch.float64)
    total = torch.nn.utils.clip_grad_norm_([q], max_norm=clip)
    assert abs(total.item() - host) <= 1e-12 * host
    torch.optim.Adam([q], lr=f32(cfg.learning_rate), betas=(f32(cfg.beta1), f32(cfg.beta2)), eps=f32(cfg.eps)).step()
    want = q.detach().numpy()
    err = np.abs(got - want).max()
    print(f"{tag}: parameter error {err:.3e}, bound {1e-6 * np.abs(want).max():.3e}")
    assert err <= 1e-6 * np.abs(want).max(), err
    # the update is the clipped one: without the clip Adam's first step moves every parameter whose
    # gradient is not tiny by lr whatever the scale, so compare the second moment instead
    _, _, v = _adam_arenas(e)
    coef = coef_formula(host, clip)
    i = int(np.abs(g).argmax())
    assert abs(v[i] - (1 - f32(cfg.beta2)) * (coef * float(g[i])) ** 2) <= 1e-5 * v[i]


@pytest.mark.parametrize("tag", ["c2s", "c1"])
@pytest.mark.parametrize("graph", [False, True])
def test_bucketed_clipped_step_equals_unfused_fp32(graph, tag):
    """test_bucketed_train_step_equals_unfused_fp32 with the clip set on both engines: three steps of
    train_step (graph off and on) against forward -> backward -> adam_step; losses within 1e-5 relative,
    parameters within 1e-6.  The clip is a quarter of the first step's norm and must bite every step."""
    cfg, seed, z = load_fixture(tag)
    f, p, c = _inputs(z)
    a, b = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, b):
        e.set_training(False)
    clip = f32(0.25 * _probe_norm(b, f, p, c))
    a.set_graph(graph)
    for e in (a, b):
        e.set_grad_clip(clip)
    for i in range(3):
        la = a.train_step(f, p, c).clone()
        lb = b.forward(f, p, c).clone()
        b.backward()
        b.adam_step()
        torch.cuda.synchronize()
        assert abs(la.item() - lb.item()) < 1e-5 * abs(lb.item()), (i, la.item(), lb.item())
        na, nb = a.grad_norm(), b.grad_norm()
        print(f"{tag} graph={graph} step {i}: norm bucketed {na:.7e} unfused {nb:.7e} clip {clip:.7e}")
        assert na > clip and nb > clip, (i, na, nb, clip)
        assert abs(na - nb) <= 1e-5 * nb
    _params_close(a, b, 1e-6)


def _bf16_step(clip, delay):
    """one bucketed bf16 c2s step (dropout on) from the fixture state and RNG seed 11: (loss, weights)"""
    from capgen import _lib
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _bf16_inputs(z)
    e = _bf16_engine(cfg, seed)
    e.set_rng_seed(11)
    if clip is not None:
        e.set_grad_clip(clip)
    _lib.side_delay(delay)
    try:
        loss = e.train_step(f, p, c).item()
        torch.cuda.synchronize()
        w = e.state_dict(False)
        norm = e.grad_norm() if clip is not None else None
    finally:
        _lib.side_delay(0.0)
    return loss, w, norm


@pytest.fixture(scope="module")
def bf16_unclipped_step():
    return _bf16_step(None, 0.0)


@pytest.mark.parametrize("delay", [0.0, 40.0])
def test_measure_only_leaves_the_bf16_step_as_it_was(delay, bf16_unclipped_step):
    """max_norm = +inf: the coefficient is exactly 1, so after one step from equal state and RNG seed
    every Linear weight (deterministic GEMM gradients) is bit-identical to an engine with clipping off,
    and the other tensors (f32-atomic gradient sums) agree within 1e-5 -- the split of
    test_side_stream_delay_leaves_bf16_results_bit_identical; the same with a 40 us spin in front of
    every launch off the critical stream (the norm pass and the deferred Adam among them)."""
    l0, w0, _ = bf16_unclipped_step
    l1, w1, norm = _bf16_step(INF, delay)
    assert l0 == l1, (l0, l1)
    assert math.isfinite(norm) and norm > 0
    lin = [k for k in w0 if w0[k].dim() == 2 and k != "decoder.word_embedding.weight"]
    bad = [k for k in lin if not torch.equal(w0[k], w1[k])]
    assert not bad, bad[:8]
    for k in w0:
        torch.testing.assert_close(w0[k], w1[k], atol=1e-5, rtol=0, msg=k)


def test_set_lr_reaches_a_replayed_step_graph():
    """The whole-step graph is captured at the config's rate; set_lr(x) between steps, and the replayed
    step moves the parameters as a fresh engine created with learning_rate = x does from the same
    state (parameters, moments, step counter): 1e-6."""
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _inputs(z)
    a = _engine(cfg, seed)
    a.set_training(False)
    a.set_graph(True)
    a.train_step(f, p, c)
    a.train_step(f, p, c)  # (a replay at the old rate)
    x = f32(0.37 * cfg.learning_rate)
    b = _engine(cfg.replace(learning_rate=x), seed)
    b.set_training(False)
    step, m, v = _adam_arenas(a)
    assert step == 2
    b.set_params_arena(a.params_arena())
    b.set_adam_state(step, m, v)
    before = a.params_arena()
    assert a.lr == f32(cfg.learning_rate)
    a.set_lr(x)
    assert a.lr == x
    la = a.train_step(f, p, c).item()
    lb = b.train_step(f, p, c).item()
    assert abs(la - lb) <= 1e-6 * abs(lb), (la, lb)
    _params_close(a, b, 1e-6)
    # (a step at the old rate would sit ~(learning_rate - x) = 3e-4 away from b, far outside 1e-6)
    assert np.abs(a.params_arena() - before).max() > 0
    assert _adam_arenas(a)[0] == 3


def test_set_lr_zero_freezes_the_parameters():
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    e = _engine(cfg, seed)
    e.set_training(False)
    e.train_step(f, p, c)
    before = e.params_arena()
    e.set_lr(0.0)
    e.train_step(f, p, c)
    after = e.params_arena()
    assert np.array_equal(before.view(np.int32), after.view(np.int32)), "a parameter moved at lr = 0"
    assert _adam_arenas(e)[0] == 2, "the Adam step counter must still advance"
    e.set_lr(cfg.learning_rate)
    e.train_step(f, p, c)
    assert not np.array_equal(before, e.params_arena())


def test_set_lr_to_the_config_value_changes_nothing():
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _inputs(z)
    a, b = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, b):
        e.set_training(False)
    a.set_lr(cfg.learning_rate)
    la, lb = a.train_step(f, p, c).item(), b.train_step(f, p, c).item()
    assert la == lb, (la, lb)
    sa, sb = a.state_dict(False), b.state_dict(False)
    for k in sa:
        if sa[k].dim() == 2 and k != "decoder.word_embedding.weight":
            assert torch.equal(sa[k], sb[k]), k
        torch.testing.assert_close(sa[k], sb[k], atol=1e-6, rtol=0, msg=k)


def test_weighted_step_with_a_clip_equals_its_unfused_sequence():
    """train_step_weighted goes through the same backward, so this guards the wiring only: against the
    weighted step's own gradients (taken from an unclipped step) fed to the clipped adam_step from the
    same parameters and zero moments."""
    cfg, seed, f, p, c = case("c1")
    fd, pd, cd, wd = (t.to(DEV) for t in (f, p, c, WEIGHTS(c.shape[0])))
    a, b = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, b):
        e.set_training(False)
    p0 = b.params_arena()
    lb = b.train_step_weighted(fd, pd, cd, wd).item()
    g = b.grads_arena()
    host = _host_norm(g)
    clip = f32(0.5 * host)
    b.set_params_arena(p0)
    b.set_adam_state(0)
    b.set_grads_arena(g)
    b.set_grad_clip(clip)
    b.adam_step()
    a.set_grad_clip(clip)
    la = a.train_step_weighted(fd, pd, cd, wd).item()
    assert la == lb, (la, lb)
    assert abs(a.grad_norm() - host) <= 1e-5 * host and a.grad_norm() > clip
    _params_close(a, b, 1e-6)


def test_sharded_emulation_with_a_clip_fp32():
    """_sharded_update_check (world 2, fp32) with a finite clip on every engine: each emulated rank takes
    the norm over the whole arena, so all derive the reference's coefficient and the assembled
    parameters equal the reference engine's clipped bucketed step within its 1e-6."""
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _inputs(z)
    ref = _engine(cfg, seed)
    ref.set_training(False)
    clip = f32(0.25 * _probe_norm(ref, f, p, c))
    ranks = [_engine(cfg, seed) for _ in range(2)]
    for e in ranks + [ref]:
        e.set_grad_clip(clip)
    _sharded_update_check(cfg, ref, ranks, f, p, c, "fp32")
    want = ref.grad_norm()
    assert want > clip
    for e in ranks:
        assert abs(e.grad_norm() - want) <= 1e-5 * want


def test_dp_world1_sharded_clipped_step_equals_single_process(set_knob):
    """dp_init(..., 0, 1) with ZERO = 2 (reduce-scatter / all-gather and the norm's all-reduce over RCCL
    at world 1) and a clip equals the single-process clipped step: test_dp_world1_rccl_train_step_fp32's
    tolerances."""
    from capgen.engine import Engine
    set_knob("ZERO", 2)
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    a, b = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, b):
        e.set_training(False)
    clip = f32(0.25 * _probe_norm(b, f, p, c))
    a.dp_init(Engine.dp_unique_id(), 0, 1)
    for e in (a, b):
        e.set_grad_clip(clip)
    for _ in range(3):
        la = a.train_step(f, p, c).item()
        lb = b.train_step(f, p, c).item()
        assert abs(la - lb) < 1e-5 * abs(lb), (la, lb)
        assert a.grad_norm() > clip and abs(a.grad_norm() - b.grad_norm()) <= 1e-5 * b.grad_norm()
    _params_close(a, b, 1e-6)


def test_clipping_adds_one_collective_per_step(set_knob):
    """test_dp_ranks_with_different_batches_issue_identical_collectives with a clip: two world-1 RCCL
    engines with different batches log the same calls, exactly one more line per train step than with
    the clip off -- the 8-byte all-reduce of the norm's sum on the bucket stream."""
    from capgen.engine import Engine
    from capgen.synthetic import synthetic_batch
    set_knob("ZERO", 2)
    cfg, seed, z = load_fixture("c2s")
    batches = [_bf16_inputs(z)]
    fb, pb, cb = synthetic_batch(3, z["feats"].shape[1], cfg.encode_dim_features, cfg.encode_dim_positions,
                                 12, cfg.num_vocab, seed=5, min_valid=3)
    batches.append([t.to(DEV) for t in (fb, pb, cb)])
    steps = 2
    logs = {}
    for clip in (None, 1.0):
        for i, (f, p, c) in enumerate(batches):
            e = _bf16_engine(cfg, seed)
            e.dp_init(Engine.dp_unique_id(), 0, 1)
            if clip is not None:
                e.set_grad_clip(clip)
            e.collectives_log(1)
            for _ in range(steps):
                e.train_step(f, p, c)
            e.forward(f, p, c)
            e.backward()
            torch.cuda.synchronize()
            logs[clip, i] = e.collectives_log(2).splitlines()
            e.collectives_log(0)
    assert logs[1.0, 0] == logs[1.0, 1], (logs[1.0, 0][:40], logs[1.0, 1][:40])
    assert logs[None, 0] == logs[None, 1]
    extra = [ln for ln in logs[1.0, 0] if "gnorm" in ln]
    assert extra == ["allreduce(gnorm) 8 B on bucket"] * steps, extra
    # the other calls are those of the unclipped step (the all-gathers now follow the norm: another order)
    assert len(logs[1.0, 0]) == len(logs[None, 0]) + steps
    assert sorted(ln for ln in logs[1.0, 0] if "gnorm" not in ln) == sorted(logs[None, 0])
    assert not [ln for ln in logs[None, 0] if "gnorm" in ln]


@pytest.mark.parametrize("mode", ["default", "dp_world1_sharded"])
def test_clipped_step_has_no_unordered_conflicts(mode, set_knob):
    """the hazard checker over test_gpu_hazard's logged run, on a bf16 c2s engine with a finite clip"""
    if mode == "dp_world1_sharded":
        set_knob("ZERO", 2)
    cfg, seed, z = load_fixture("c2s")
    e = _bf16_engine(cfg, seed)
    if mode.startswith("dp_"):
        from capgen.engine import Engine
        e.dp_init(Engine.dp_unique_id(), 0, 1)
    e.set_grad_clip(1.0)
    n, report = _logged_run(e, *_bf16_inputs(z))
    assert n == 0, f"{n} unordered conflicting launch pairs:\n{report}"
    assert e.grad_norm() > 0


def test_switching_clipping_recaptures_the_step_graph():
    """Off -> on -> a new bound -> off with the whole-step graph on, against an eager engine given the
    same calls: the switch drops the captured step (its schedule changes), a new bound while on is read
    by the replay.  Tolerances of test_bucketed_train_step_equals_unfused_fp32."""
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    a, b = _engine(cfg, seed), _engine(cfg, seed)
    for e in (a, b):
        e.set_training(False)
    a.set_graph(True)
    clip = f32(0.25 * _probe_norm(b, f, p, c))
    for setting in (None, clip, f32(0.5 * clip), 0.0):  # capture, re-capture, replay, re-capture
        for e in (a, b):
            if setting is not None:
                e.set_grad_clip(setting)
        la, lb = a.train_step(f, p, c).item(), b.train_step(f, p, c).item()
        assert abs(la - lb) < 1e-5 * abs(lb), (setting, la, lb)
        if setting:
            assert a.grad_norm() > setting and abs(a.grad_norm() - b.grad_norm()) <= 1e-5 * b.grad_norm()
    _params_close(a, b, 1e-6)


def test_setter_errors():
    cfg, seed, z = load_fixture("c1")
    e = _engine(cfg, seed)
    e.set_training(False)
    f, p, c = _inputs(z)
    with pytest.raises(RuntimeError, match="last_grad_norm"):
        e.grad_norm()
    e.train_step(f, p, c)  # clipping off: still no norm
    with pytest.raises(RuntimeError, match="last_grad_norm"):
        e.grad_norm()
    for bad in (-1.0, float("nan"), -INF):
        with pytest.raises(RuntimeError, match="set_grad_clip"):
            e.set_grad_clip(bad)
    for bad in (-1e-3, float("nan"), INF, -INF):
        with pytest.raises(RuntimeError, match="set_lr"):
            e.set_lr(bad)
    assert e.lr == f32(cfg.learning_rate) and e.grad_clip is None
    e.set_grad_clip(INF)
    e.train_step(f, p, c)
    assert e.grad_norm() > 0
    e.set_grad_clip(0)  # off again: the last measured norm stays readable
    e.train_step(f, p, c)
    assert e.grad_norm() > 0
