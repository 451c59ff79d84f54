"""The update kernel's variants (decoupled weight decay, the averaged weights, each with and without the
clip scale) and the arena exchange, through capgen_debug_adam_ex / capgen_debug_arena_swap against the
float64 restatement of tests/optim_ref.py (anchored to torch.optim.AdamW + AveragedModel in
test_optim_host.py).

Sizes are test_adam's: one 16-byte vector, a ragged last pass, and 128 grid-stride passes under
grid_cap = 2.  wd = 0.1 and d = 0.9 put both effects far above the bounds (asserted: a restatement without
an option misses the kernel's result by more than 10x the bound).

Bounds.  Parameters: test_adam's 1e-6 max|ref| + 1e-6 lr, plus 3 * 2^-24 max|ref| with decay on -- one more
f32 rounding per step for the multiply by 1 - lr * wd.  Average: 1e-6 max|ref_e| + 1e-6 lr -- it inherits
(1 - d) of the parameter error and adds three roundings per step (the difference, the product, the sum),
each <= 2^-24 max|e| = 6e-8 max|e|: under the bound for three steps.  Moments: as test_adam (1e-5 max|ref|).
The float64 reference uses the f32 values of lr, wd and d."""
import ctypes as C
import itertools

import pytest
import torch

from optim_ref import adamw_ema_ref, f32
from test_gpu_gradclip import adam_bufs, adam_call
from test_gpu_rowops import (B1, B2, DEV, EPS, F32, LR, P, _lib_, adam_inputs, assert_close, assert_same, call, dev,
                             tiled_index)

pytestmark = pytest.mark.gpu

WD, D, GS = f32(0.1), f32(0.9), f32(0.37)
SIZES = [4, 4100, 1_048_580]
COMBOS = list(itertools.product([False, True], repeat=3))  # (gscale, decay, average)


def bufs(n, p0, ema):
    """adam_bufs at a partial shadow (and, at the largest size, test_adam's two tiled ranges), the 8-float
    scal of the _ex hook, and the average with its guard words"""
    big = n > 100_000
    n_shadow = (n // 2 + 3) // 4 * 4
    tiles = [(0, 16 * 512), (16 * 512 + 12, 32 * 512)] if big else []
    b = adam_bufs(n, p0, n_shadow, tiles)
    b["scal"] = torch.zeros(8, device=DEV)
    b["e"] = torch.cat([dev(p0), torch.full((4,), 7.0, device=DEV)]) if ema else None
    b["cap"] = 2 if big else 0
    return b


def ex_call(b, n, gd, gscale=None, wd=0.0, d=0.0):
    tiles = b["tiles"]
    offs = (C.c_int64 * 4)(*[o for o, _ in tiles])
    lens = (C.c_int64 * 4)(*[ln for _, ln in tiles])
    ptrs = (C.c_void_p * 4)(*[d_.data_ptr() for d_ in b["dsts"]])
    call("capgen_debug_adam_ex", P(b["p"]), P(gd), P(b["m"]), P(b["v"]), n, C.c_float(LR), C.c_float(B1),
         C.c_float(B2), C.c_float(EPS), P(b["step"]), P(b["scal"]), P(b["sh"]) if b["n_shadow"] else None,
         b["n_shadow"], b["cap"], len(tiles), offs, lens, ptrs, P(gscale), C.c_float(wd), P(b["e"]), C.c_float(d),
         None)


def check_guards_and_copies(b, n, what):
    """nothing written past a buffer; the shadow is bf16 of the parameters written, the tiles its re-layout"""
    assert (b["p"][n:] == 7.0).all() and (b["m"][n:] == 0).all() and (b["v"][n:] == 0).all(), what
    if b["e"] is not None:
        assert (b["e"][n:] == 7.0).all(), f"{what}: the average was written past n"
    ns = b["n_shadow"]
    shc = b["sh"].cpu()
    assert_same(shc[:ns], b["p"][:ns].cpu().bfloat16(), f"{what} shadow")
    assert (shc[ns:] == 7.0).all(), f"{what}: shadow written past n_shadow"
    for (off, ln), d_ in zip(b["tiles"], b["dsts"]):
        dc = d_.cpu()
        exp = torch.full((ln,), 7.0, dtype=torch.bfloat16)
        exp[torch.from_numpy(tiled_index(ln // 512))] = shc[off:off + ln]
        assert_same(dc[:ln], exp, f"{what} tiled copy of [{off}, {off + ln})")
        assert (dc[ln:] == 7.0).all(), f"{what}: tiled copy wrote past its range"


@pytest.fixture(scope="module")
def cases():
    """per size: the inputs and the float64 references of all eight combinations, computed once"""
    out = {}
    for n in SIZES:
        p0, grads = adam_inputs(n, n)
        g64 = [g.double() for g in grads]
        refs = {}
        for gs, wd, ema in COMBOS:
            refs[(gs, wd, ema)] = adamw_ema_ref(p0.double(), g64, LR, B1, B2, EPS, wd=WD if wd else 0.0,
                                                scales=[GS] * 3 if gs else None, d=D if ema else None)
        out[n] = (p0, grads, refs)
    return out


@pytest.mark.parametrize("gs,wd,ema", COMBOS)
@pytest.mark.parametrize("n", SIZES)
def test_adam_ex(n, gs, wd, ema, cases):
    p0, grads, refs = cases[n]
    ref = refs[(gs, wd, ema)]
    b = bufs(n, p0, ema)
    gsd = torch.full((1,), GS, device=DEV) if gs else None
    for t in range(3):
        ex_call(b, n, dev(grads[t]), gsd, WD if wd else 0.0, D if ema else 0.0)
        rp, rm, rv, re_ = ref[t]
        what = f"n={n} gscale={gs} decay={wd} average={ema} step {t + 1}"
        assert b["step"][0].item() == t + 1 and b["step"][1].item() == 0
        sc = b["scal"].cpu()
        if wd:
            assert sc[2].item() == f32(1.0 - float(LR) * float(WD)), "the factor: computed in double, rounded once"
        else:
            assert sc[2].item() == 0, "the plain prepare kernel writes two floats"
        assert sc[3].item() == 0 and sc[7].item() == 0
        bound = 1e-6 * rp.abs().max().item() + 1e-6 * LR + (3 * 2.0 ** -24 * rp.abs().max().item() if wd else 0.0)
        err = (b["p"][:n].cpu().double() - rp).abs().max().item()
        print(f"{what}: parameter error {err:.3e} of bound {bound:.3e}")
        assert err <= bound, (what, err, bound)
        assert_close(b["m"][:n], rm, F32, f"{what} exp_avg")
        assert_close(b["v"][:n], rv, F32, f"{what} exp_avg_sq")
        if ema:
            ebound = 1e-6 * re_.abs().max().item() + 1e-6 * LR
            eerr = (b["e"][:n].cpu().double() - re_).abs().max().item()
            print(f"{what}: average error {eerr:.3e} of bound {ebound:.3e}")
            assert eerr <= ebound, (what, eerr, ebound)
        check_guards_and_copies(b, n, what)
    if gsd is not None:
        assert gsd.item() == GS
    # non-vacuity: the restatement without each option that is on misses the kernel's result by > 10x the bound
    got_p, got_m = b["p"][:n].cpu().double(), b["m"][:n].cpu().double()
    if wd:
        other = refs[(gs, False, ema)][2][0]
        assert (got_p - other).abs().max().item() > 10 * bound
    if ema:
        got_e = b["e"][:n].cpu().double()
        assert (got_e - p0.double()).abs().max().item() > 10 * ebound, "the average never left its starting copy"
        # ... nor is it the parameters themselves (d = 0)
        assert (got_e - got_p).abs().max().item() > 10 * ebound
    if gs:  # (Adam's step is invariant to the gradient's scale but for eps: the first moment is not)
        other = refs[(False, wd, ema)][2][1]
        assert (got_m - other).abs().max().item() > 10 * 1e-5 * other.abs().max().item()
    if not wd:
        assert torch.equal(b["p"][:n].cpu()[0::7], p0[0::7]), "a parameter whose gradient was always 0 moved"


@pytest.mark.parametrize("gs", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_adam_ex_without_options_is_bit_identical(n, gs, cases):
    """decay and average off: p, m, v, the shadow and the tiles equal capgen_debug_adam's (with only gscale:
    capgen_debug_adam_scaled's) bit for bit over three steps -- the hook then launches the same
    instantiation after a prepare kernel of the same formula"""
    p0, grads, _ = cases[n]
    a, b = bufs(n, p0, False), bufs(n, p0, False)
    gsd = torch.full((1,), GS, device=DEV) if gs else None
    for t in range(3):
        gd = dev(grads[t])
        adam_call(a, n, gd, a["cap"], gscale=gsd)
        ex_call(b, n, gd, gsd)
        for k in ("p", "m", "v"):
            assert_same(b[k].view(torch.int32), a[k].cpu().view(torch.int32), f"step {t + 1} {k}")
        assert_same(b["sh"], a["sh"].cpu(), f"step {t + 1} shadow")
        for x, y in zip(a["dsts"], b["dsts"]):
            assert_same(y, x.cpu(), f"step {t + 1} tiled copy")
        assert b["scal"][2].item() == 0 and torch.equal(a["scal"][:2].cpu(), b["scal"][:2].cpu())


def test_adam_ex_rejects_bad_arguments():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    st = torch.zeros(1, dtype=torch.int64, device=DEV)
    args = [C.c_float(LR), C.c_float(B1), C.c_float(B2), C.c_float(EPS), P(st), P(z)]
    fn = lib.capgen_debug_adam_ex
    tail = [None, 0, 0, 0, None, None, None]
    zero, one = C.c_float(0.0), C.c_float(1.0)
    assert fn(P(z), P(z), P(z), P(z), 6, *args, *tail, None, zero, None, zero, None) == 1            # n % 4
    assert fn(P(z), P(z), P(z), P(z), 8, *args, *tail, None, C.c_float(-0.1), None, zero, None) == 1  # wd < 0
    assert fn(P(z), P(z), P(z), P(z), 8, *args, *tail, None, C.c_float(float("nan")), None, zero, None) == 1
    assert fn(P(z), P(z), P(z), P(z), 8, *args, *tail, None, zero, P(z), one, None) == 1              # d = 1
    assert fn(P(z), P(z), P(z), P(z), 8, *args, *tail, None, zero, P(z), zero, None) == 1             # d = 0
    torch.cuda.synchronize()
    assert st.item() == 0 and (z == 0).all()


@pytest.mark.parametrize("n", SIZES)
def test_arena_swap(n):
    g = torch.Generator().manual_seed(n)
    a0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)  # any bits: NaNs, -0
    b0 = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
    guard = torch.full((4,), 0x40E00000, dtype=torch.int32)  # 7.0f
    a = torch.cat([a0, guard]).to(DEV).view(torch.float32)
    b = torch.cat([b0, guard]).to(DEV).view(torch.float32)
    cap = 2 if n > 100_000 else 0
    call("capgen_debug_arena_swap", P(a), P(b), n, cap, None)
    assert torch.equal(a.view(torch.int32)[:n].cpu(), b0) and torch.equal(b.view(torch.int32)[:n].cpu(), a0)
    assert (a[n:] == 7.0).all() and (b[n:] == 7.0).all()
    call("capgen_debug_arena_swap", P(a), P(b), n, cap, None)
    assert torch.equal(a.view(torch.int32)[:n].cpu(), a0) and torch.equal(b.view(torch.int32)[:n].cpu(), b0)
    assert (a[n:] == 7.0).all() and (b[n:] == 7.0).all()


def test_arena_swap_rejects_bad_arguments():
    _lib, lib = _lib_()
    a = torch.full((16,), 1.0, device=DEV)
    b = torch.full((16,), 2.0, device=DEV)
    fn = lib.capgen_debug_arena_swap
    assert fn(P(a), P(b), 6, 0, None) == 1
    assert fn(None, P(b), 8, 0, None) == 1
    assert fn(P(a), None, 8, 0, None) == 1
    assert fn(P(a), P(b), -4, 0, None) == 1
    torch.cuda.synchronize()
    assert (a == 1.0).all() and (b == 2.0).all()
    assert fn(P(a), P(b), 8, 0, None) == 0
    torch.cuda.synchronize()
    assert (a[:8] == 2.0).all() and (a[8:] == 1.0).all() and (b[:8] == 1.0).all() and (b[8:] == 2.0).all()
