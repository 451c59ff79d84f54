"""The per-caption weight of the two row-wise cross-entropy launchers (csrc/ops.h: cross_entropy_rows,
ce_finish with row_w), through the capgen_debug_*_weighted hooks against the float64 restatement of
tests/test_gpu_rowops.py times the weight: row m uses w = row_w[m // rows_per_w],
loss_row = w (lse - logit[tgt]), dlogits = w (softmax - onehot), pad rows exactly zero.

Tolerances: those of test_cross_entropy_rows / test_ce_finish, every bound multiplied by |w| of the row
(the one extra f32 multiplication, 6e-8 relative, disappears in their two orders of headroom).  With
all weights 1.0 the weighted kernels must reproduce the unweighted ones bit for bit (x * 1.0f == x).
"""
import pytest
import torch

from test_gpu_rowops import (BF16, CE_PAD, DEV, F32, TDT, P, _lib_, call, ce_ref, ce_rows, dev, run_ce_finish,
                             slab_stats)

gpu = pytest.mark.gpu
M = 6
# one pool, fixed: the first M / rows_per_w entries are the weights of a case.  rows_per_w = 1: row 1 has
# w = 0, the pad row (3) has w = 1; rows_per_w = 2: rows 2 and 3 (pad) have w = 0; rows_per_w = 6: -0.75.
W_POOL = [-0.75, 0.0, 2.5, 1.0, 1.5, -2.0]
RPW = [1, 2, 6]


def weights(rpw):
    w = torch.tensor(W_POOL[:M // rpw], dtype=torch.float32)
    return w, w.double().repeat_interleave(rpw)  # [M / rpw] for the kernel, [M] per row for the reference


def check(lr, got, w_row, lse, tl, tgt, grad, elem_bound, what):
    """lr [M] loss rows, got [M, V] gradient; elem_bound [M, V]: the unweighted test's gradient bound"""
    lr, got = lr.cpu().double(), got.cpu().double()
    kept = tgt != CE_PAD
    aw = w_row.abs()
    print(f"{what}: loss err {(lr - w_row * (lse - tl))[kept].abs().max().item():.3e}, "
          f"grad err {(got - w_row.unsqueeze(1) * grad).abs().max().item():.3e}")
    assert torch.isfinite(lr).all() and torch.isfinite(got).all(), what
    assert ((lr - w_row * (lse - tl)).abs() <= aw * 1e-5 * (lse.abs() + tl.abs()))[kept].all(), (what, lr)
    err = (got - w_row.unsqueeze(1) * grad).abs()
    bound = aw.unsqueeze(1) * elem_bound
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} gradient entries out, max err {err.max():.3e}"
    zero = ~kept | (w_row == 0)
    assert (lr[zero] == 0).all() and (got[zero] == 0).all(), what + ": pad rows and w = 0 rows are exactly zero"


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def run_ce_rows(hook, x, tgt, w, rpw, V, dtype):
    lr = torch.full((M + 1,), 7.0, device=DEV)
    dl = torch.full((M * V + 8,), 7.0, dtype=TDT[dtype], device=DEV)
    xd, td = dev(x), dev(tgt)
    if w is None:
        call(hook, P(xd), P(td), M, V, CE_PAD, P(lr), P(dl), dtype, None)
    else:
        wd = dev(w)
        call(hook, P(xd), P(td), P(wd), rpw, M, V, CE_PAD, P(lr), P(dl), dtype, None)
    assert lr[M].item() == 7.0 and (dl[M * V:] == 7.0).all(), "the guard words after the buffers"
    return lr[:M], dl[:M * V].view(M, V)


@gpu
@pytest.mark.parametrize("rpw", RPW)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", [8, 10000, 16384, 1001])
def test_cross_entropy_rows_weighted(V, dtype, rpw):
    """NV4 = 4 (8), 10 (10000), 16 (16384) of the register-resident form and the generic form (1001)."""
    x, tgt = ce_rows(V, V)
    lse, tl, _, grad, _ = ce_ref(x.double(), tgt, CE_PAD)
    w, w_row = weights(rpw)
    lr, got = run_ce_rows("capgen_debug_cross_entropy_rows_weighted", x, tgt, w, rpw, V, dtype)
    bound = 1e-5 * grad.abs().max() + torch.zeros_like(grad)
    if dtype == BF16:
        bound = bound + 2.0 ** -8 * grad.abs()
    check(lr, got, w_row, lse, tl, tgt, grad, bound, f"V={V} dtype={dtype} rpw={rpw}")


@gpu
@pytest.mark.parametrize("rpw", RPW)
@pytest.mark.parametrize("dtype", [F32, BF16])
@pytest.mark.parametrize("V", [8, 10000, 16384, 1001])
def test_cross_entropy_rows_unit_weights_bit_identical(V, dtype, rpw):
    x, tgt = ce_rows(V, V)
    ones = torch.ones(M // rpw)
    lr1, g1 = run_ce_rows("capgen_debug_cross_entropy_rows_weighted", x, tgt, ones, rpw, V, dtype)
    lr0, g0 = run_ce_rows("capgen_debug_cross_entropy_rows", x, tgt, None, 1, V, dtype)
    assert torch.equal(bits(lr1), bits(lr0)) and torch.equal(bits(g1), bits(g0))


def run_ce_finish_weighted(stats, e, tl, tgt, w, rpw, V, ld):
    S = stats.shape[1]
    st = torch.full((M, ld, 2), float("nan"))
    st[:, :S] = stats
    dl = torch.full((M * V + 16,), 7.0, dtype=torch.bfloat16)
    dl[:M * V] = e.reshape(-1)
    lr = torch.full((M + 1,), 7.0, device=DEV)
    std, dld, tld, td, wd = dev(st), dev(dl), dev(tl.float()), dev(tgt), dev(w)
    call("capgen_debug_ce_finish_weighted", P(std), ld, P(tld), P(td), P(wd), rpw, M, V, CE_PAD, P(lr), P(dld), None)
    assert lr[M].item() == 7.0
    assert (dld[M * V:] == 7.0).all(), "ce_finish wrote past the last row"
    return lr[:M], dld[:M * V].view(M, V)


CE_FINISH_VS = [8, 1000, 4104, 10000, 16392, 12]
CE_FINISH_CASES = [(V, 1) for V in CE_FINISH_VS] + [(V, 0) for V in CE_FINISH_VS if V % 8 == 0]


@gpu
@pytest.mark.parametrize("rpw", RPW)
@pytest.mark.parametrize("wide_ld", [0, 1])
@pytest.mark.parametrize("V,vec8", CE_FINISH_CASES)
def test_ce_finish_weighted(V, vec8, wide_ld, rpw, set_knob):
    """SPT = 1 (8, 1000, 12), 2 (4104), 3 (10000), 8 (16392); the 16-byte and the 8-byte row accesses."""
    set_knob("CE_VEC8", vec8)
    x, tgt = ce_rows(V, V + 1)
    stats, e = slab_stats(x)
    lse, tl, _, grad, sm = ce_ref(x.double(), tgt, CE_PAD)
    w, w_row = weights(rpw)
    ld = stats.shape[1] + 3 * wide_ld
    lr, got = run_ce_finish_weighted(stats, e, tl, tgt, w, rpw, V, ld)
    onehot = torch.zeros_like(sm)
    onehot[torch.arange(M), tgt.long()] = 1
    bound = 1e-5 * grad.abs().max() + 2.0 ** -7 * sm + 2.0 ** -8 * onehot
    check(lr, got.float(), w_row, lse, tl, tgt, grad, bound, f"V={V} vec8={vec8} ld+{3 * wide_ld} rpw={rpw}")
    if rpw == 1:  # all-ones weights: the unweighted kernel's bits
        lr1, g1 = run_ce_finish_weighted(stats, e, tl, tgt, torch.ones(M), 1, V, ld)
        lr0, g0 = run_ce_finish(stats, e, tl, tgt, V, CE_PAD, ld)
        assert torch.equal(bits(lr1), bits(lr0)) and torch.equal(bits(g1), bits(g0))


@gpu
def test_weighted_hooks_reject_bad_arguments():
    _lib, lib = _lib_()
    z = torch.zeros(64, device=DEV)
    zi = torch.zeros(8, dtype=torch.int32, device=DEV)
    ce = lib.capgen_debug_cross_entropy_rows_weighted
    fin = lib.capgen_debug_ce_finish_weighted
    for bad in [dict(w=None, rpw=1, M=4), dict(w=P(z), rpw=3, M=4), dict(w=P(z), rpw=0, M=4)]:
        assert ce(P(z), P(zi), bad["w"], bad["rpw"], bad["M"], 8, 0, P(z), P(z), F32, None) == 1, bad
        assert b"cross_entropy_rows_weighted" in lib.capgen_last_error()
        assert fin(P(z), 1, P(z), P(zi), bad["w"], bad["rpw"], bad["M"], 8, 0, P(z), P(z), None) == 1, bad
        assert b"ce_finish_weighted" in lib.capgen_last_error()
    torch.cuda.synchronize()
