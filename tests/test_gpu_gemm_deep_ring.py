"""The deep-ring variants of the 8- and 16-wave GEMM tiles (gemm_bf16.hip variants 31-36: three and
four LDS stages, so more than one k-tile's DMA is in flight when a CU holds a single workgroup, as
in the capped weight-gradient grid).  A deeper ring changes only when a k-tile is fetched, never the
order it is accumulated in, so every check is against the f32 product of the bf16 operands within the
suite's GEMM bound 2e-3 * sqrt(K), or bit for bit against a 2-stage variant.

K values: 40 = one partial k-tile, fewer tiles than stages (the prologue's `p < nk` guard);
64 * (STAGES - 1) = the prologue fetches everything, the loop body issues no DMA; 64 * STAGES + 8 = one
full turn of the ring plus a masked tail tile (the case an off-by-one in the counted DMA wait breaks:
a variant waiting for one stage fewer than it issued reads a tile that has not landed); 1000 = the
value of test_gemm_every_variant_and_splitk.  M x N = 200 x 264: row and column tails and at least two
tiles each way for the 128-wide tiles; 300 x 264 for the 256-row tile -- 304 x 264 where A is transposed
(TN): the GEMM takes a transposed operand only with rows of whole 16-B vectors (M % 8 == 0) and refuses
M = 300, and 304 is the nearest size it takes (still two row tiles, the second a 48-row tail)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
STAGES = {31: 3, 32: 4, 33: 3, 34: 3, 35: 4, 36: 3}  # 128x128w16s3/s4, 128x128w8s3, 128x64w8s3/s4, 256x128w16s3
NEW = sorted(STAGES)
LAYOUTS = [(0, 1), (0, 0), (1, 1)]  # NN, NT, TN (gemm_bf16.hip header)
F32, BF16 = 0, 1


def _mn(variant, ta=0):
    return ((304 if ta else 300), 264) if variant == 36 else (200, 264)


@functools.lru_cache(maxsize=None)
def _problem(M, N, K):
    """bf16 operands, the bias and the f32 reference product: computed once per shape, never modified"""
    g = torch.Generator(device="cpu").manual_seed(M * 7 + K)
    A = torch.randn(M, K, generator=g).bfloat16()
    Bm = torch.randn(N, K, generator=g).bfloat16()
    bias = torch.randn(N, generator=g)
    return A, Bm, bias, A.float() @ Bm.float().t() + bias


def _run(variant, M, N, K, ta, tb, Ad, lda, Bd, ldb, out=F32, bias=None, repeats=1):
    """`repeats` launches of the forced variant into NaN-filled outputs; returns them on the CPU"""
    from capgen import _lib
    lib = _lib.load()
    outs = []
    _lib.check(lib.capgen_debug_gemm_variant(variant))
    try:
        for _ in range(repeats):
            Cd = torch.full((M, N), float("nan"), dtype=torch.float32 if out == F32 else torch.bfloat16, device=DEV)
            _lib.check(lib.capgen_debug_gemm(M, N, K, C.c_void_p(Ad.data_ptr()), lda, ta, C.c_void_p(Bd.data_ptr()), ldb,
                                             tb, C.c_void_p(Cd.data_ptr()), N, 1, out,
                                             C.c_void_p(bias.data_ptr()) if bias is not None else None, 1.0, 0, 0,
                                             None))
            torch.cuda.synchronize()
            outs.append(Cd.cpu())
    finally:
        _lib.check(lib.capgen_debug_gemm_variant(0))
    return outs


def _product(variant, M, N, K, ta, tb, out=F32, repeats=1):
    A, Bm, bias, _ = _problem(M, N, K)
    Ad = (A.t().contiguous() if ta else A).to(DEV)
    Bd = (Bm.t().contiguous() if tb else Bm).to(DEV)
    return _run(variant, M, N, K, ta, tb, Ad, M if ta else K, Bd, N if tb else K, out, bias.to(DEV), repeats)


@pytest.mark.parametrize("kcase", ["partial", "prologue_only", "ring_turn_tail", "long"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
@pytest.mark.parametrize("variant", NEW)
def test_deep_ring_variant_computes_the_product(variant, ta, tb, kcase):
    st = STAGES[variant]
    K = {"partial": 40, "prologue_only": 64 * (st - 1), "ring_turn_tail": 64 * st + 8, "long": 1000}[kcase]
    M, N = _mn(variant, ta)
    ref = _problem(M, N, K)[3]
    (got,) = _product(variant, M, N, K, ta, tb)
    err = (got - ref).abs().max().item()
    print(f"variant {variant} ta={ta} tb={tb} K={K}: max err {err:.3e} (bound {2e-3 * np.sqrt(K):.3e})")
    assert torch.isfinite(got).all()
    assert err <= 2e-3 * np.sqrt(K)


@pytest.mark.parametrize("variant", NEW)
def test_deep_ring_k_tail_never_reads_past_the_operands(variant):
    """K = 72 weight-gradient layout (TN) with NaN past each operand row's end and past the last row: the
    second k-tile is 8 deep and its masked rows must land as zeros whatever follows the operand."""
    M, N = _mn(variant, 1)
    K = 72
    A, Bm, _, _ = _problem(M, N, K)
    ref = A.float() @ Bm.float().t()

    def poisoned(x):  # x in a NaN-filled buffer with 128 spare rows and >= 64 spare columns (rows 16-B multiples)
        buf = torch.full((x.shape[0] + 128, (x.shape[1] + 71) // 8 * 8), float("nan"), dtype=torch.bfloat16,
                         device=DEV)
        buf[: x.shape[0], : x.shape[1]] = x.to(DEV)
        return buf

    Ad, Bd = poisoned(A.t().contiguous()), poisoned(Bm.t().contiguous())
    (got,) = _run(variant, M, N, K, 1, 1, Ad, Ad.shape[1], Bd, Bd.shape[1])
    assert torch.isfinite(got).all(), int((~torch.isfinite(got)).sum())
    assert (got - ref).abs().max().item() <= 2e-3 * np.sqrt(K)


@functools.lru_cache(maxsize=None)
def _two_stage_reference(which):
    """the 2-stage 16-wave tile's TN f32 product / the 4-wave 64x64 tile's NN bf16 product, 200 x 264 x 1000"""
    if which == "tn_f32":
        return _product(10, 200, 264, 1000, 1, 1, F32)[0]
    return _product(7, 200, 264, 1000, 0, 1, BF16)[0]


@pytest.mark.parametrize("variant", NEW)
def test_deep_ring_is_bit_identical_to_the_shallow_ring(variant):
    """Same k-tiles, same order, same MFMA sequence: the weight-gradient product (TN, f32) equals variant
    10's (128x128w16s2, the table's former choice) and the NN bf16 product variant 7's bit for bit, and
    three launches of the variant agree with each other."""
    tn = _product(variant, 200, 264, 1000, 1, 1, F32, repeats=3)
    assert torch.equal(tn[0], tn[1]) and torch.equal(tn[0], tn[2])
    assert torch.equal(tn[0], _two_stage_reference("tn_f32"))
    nn = _product(variant, 200, 264, 1000, 0, 1, BF16, repeats=3)
    assert torch.equal(nn[0].view(torch.int16), nn[1].view(torch.int16))
    assert torch.equal(nn[0].view(torch.int16), nn[2].view(torch.int16))
    assert torch.equal(nn[0].view(torch.int16), _two_stage_reference("nn_bf16").view(torch.int16))


@pytest.mark.parametrize("variant", NEW)
def test_grouped_weight_gradients_on_a_deep_ring_match_single_launches(variant, set_knob):
    """The scheme of test_grouped_weight_gradients_match_single_launches_bf16 on the c1 fixture with every
    GEMM forced onto one deep-ring variant (no split-K): a block's weight gradients from ONE grouped
    launch equal the per-weight launches (CAPGEN_GROUP_DW=0) bit for bit.  Compared: every Linear weight
    gradient (the GEMM outputs; the word embedding's scatter-add is not one)."""
    from capgen import _lib
    from capgen.engine import Engine
    lib = _lib.load()
    cfg, seed, z = load_fixture("c1")
    f, p, c = (t.to(DEV) for t in fixture_inputs(z))
    cfg16 = cfg.replace(dropout=0.3, attention_dropout=0.3, dtype="bf16")
    grads = []
    _lib.check(lib.capgen_debug_gemm_variant(variant))
    try:
        for group in (0, 1):
            set_knob("GROUP_DW", group)
            e = Engine(cfg16, DEV)
            e.load_state_dict(fixture_state_dict(cfg, seed=seed, with_buffer=False))
            e.set_training(True)
            e.set_rng_seed(5)
            e.forward(f, p, c)
            e.backward()
            torch.cuda.synchronize()
            grads.append(e.grads_state_dict())
    finally:
        _lib.check(lib.capgen_debug_gemm_variant(0))
    ga, gb = grads
    linear = [n for n in ga if ga[n].dim() == 2 and n != "decoder.word_embedding.weight"]
    assert len(linear) >= 10
    for n in linear:
        assert torch.isfinite(gb[n]).all(), n
        assert torch.equal(ga[n], gb[n]), (n, (ga[n].double() - gb[n].double()).abs().max().item())
