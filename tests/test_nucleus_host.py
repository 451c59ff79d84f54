"""Nucleus (top-p) sampling, host side: the exports, and the float64 restatement (tests/nucleus_ref.py
-- the GPU tests hold the kernel to it) against hand-worked rows and its own statistics.  All inputs
are fixed: nothing here can flake."""
import numpy as np
import pytest

import nucleus_ref as N
import sampling_ref as S

ROWS = 65536
# 0.999 quantiles of chi-square at 1 .. 15 degrees of freedom
CHI2_999 = (10.83, 13.82, 16.27, 18.47, 20.52, 22.46, 24.32, 26.12, 27.88, 29.59, 31.26, 32.91, 34.53, 36.12, 37.70)

# probabilities 0.15, 0.4, 0.01, 0.3, 0.04, 0.1 at columns 0 .. 5
PROBS = np.array([0.15, 0.4, 0.01, 0.3, 0.04, 0.1])
ROW6 = np.log(PROBS).astype(np.float32)[None, :]


def sets(x, top_k, top_p, inv_tau=1.0):
    return N.nucleus_set(N.masses(x, inv_tau, top_k), top_p)


def test_exports():
    from capgen import _lib
    assert "capgen_sample_nucleus" in _lib.EXPORTED
    assert "capgen_debug_sample_nucleus" in _lib.EXPORTED
    assert _lib.ABI_VERSION == 13


def test_hand_worked_row():
    """sorted masses 0.4, 0.3, 0.15, 0.1, 0.04, 0.01 have 0, 0.4, 0.7, 0.85, 0.95, 0.99 above them"""
    for top_p, cols in ((0.3, [1]), (0.5, [1, 3]), (0.8, [0, 1, 3]), (0.9, [0, 1, 3, 5]), (0.97, [0, 1, 3, 4, 5])):
        assert np.flatnonzero(sets(ROW6, 0, top_p)[0]).tolist() == cols, top_p
    r = N.sample(np.tile(ROW6, (64, 1)), 1.0, 0, 0.8, S.SEEDS[1], S.SITE0)
    assert (r["count"] == 3).all() and np.isin(r["token"], [0, 1, 3]).all()
    np.testing.assert_allclose(r["logp"], np.log(PROBS / 0.85)[r["token"]], atol=1e-6)  # (f32 logits)
    assert len(set(r["token"].tolist())) > 1
    # a temperature reshapes the masses before the cut: p^2 / sum = 0.565, 0.318, 0.079, ...
    assert np.flatnonzero(sets(ROW6, 0, 0.8, inv_tau=2.0)[0]).tolist() == [1, 3]


def test_tie_group_straddling_the_boundary_is_kept_whole():
    """masses 0.4, 0.2, 0.2, 0.1, 0.1: at top_p = 0.5 the first 0.2 alone reaches 0.6, and both stay"""
    x = np.log(np.array([0.1, 0.2, 0.4, 0.1, 0.2])).astype(np.float32)[None, :]
    assert x[0, 1] == x[0, 4]
    assert sets(x, 0, 0.5)[0].tolist() == [False, True, True, False, True]
    assert sets(x, 0, 0.3)[0].tolist() == [False, False, True, False, False]
    assert sets(x, 0, 0.85)[0].all()  # 0.8 above the 0.1 pair: both in
    assert sets(x[:, ::-1].copy(), 0, 0.5)[0].tolist() == [True, False, True, True, False]  # no column order


def test_top_p_1_is_the_base_set():
    g = np.random.default_rng(5).normal(size=(7, 50)).astype(np.float32) * 3
    g[3, 10:20] = -np.inf
    for top_k in (0, 5):
        m = N.masses(g, 1.0, top_k)
        assert np.array_equal(N.nucleus_set(m, 1.0), S.candidates(g, top_k)[0])
        a = N.sample(g, 1.0, top_k, 1.0, 7, S.SITE0)
        b = S.sample(g, 1.0, top_k, 7, S.SITE0)
        assert np.array_equal(a["token"], b["token"]) and np.array_equal(a["logp"], b["logp"])


def test_sets_are_nested_in_top_p_and_hold_the_maximum():
    x = np.random.default_rng(6).normal(size=(33, 200)).astype(np.float32) * 2
    for top_k in (0, 16):
        m = N.masses(x, S.inv_tau_of(0.7), top_k)
        prev = None
        for top_p in (1e-6, 0.1, 0.25, 0.6, 0.9, 0.99, 1.0):
            C = N.nucleus_set(m, top_p)
            assert C[np.arange(33), x.argmax(axis=1)].all()
            assert not (C & ~m["C0"]).any()
            if prev is not None:
                assert not (prev & ~C).any(), top_p
                assert (C.sum(axis=1) >= prev.sum(axis=1)).all()
            prev = C
        assert (N.nucleus_set(m, 1e-6).sum(axis=1) == 1).all()


def test_top_k_then_top_p_uses_the_renormalised_mass():
    """top_k = 2 leaves 0.4 and 0.3, P = 0.7: at top_p = 0.5 the 0.4 above the second is not under
    0.35 (it is under 0.5 of the whole row), at top_p = 0.6 it is under 0.42"""
    assert np.flatnonzero(sets(ROW6, 2, 0.5)[0]).tolist() == [1]
    assert np.flatnonzero(sets(ROW6, 0, 0.5)[0]).tolist() == [1, 3]
    assert np.flatnonzero(sets(ROW6, 2, 0.6)[0]).tolist() == [1, 3]
    r = N.sample(np.tile(ROW6, (32, 1)), 1.0, 2, 0.6, 7, S.SITE0)
    np.testing.assert_allclose(r["logp"], np.log(PROBS / 0.7)[r["token"]], atol=1e-6)


def test_logp_is_zero_with_one_candidate():
    r = N.sample(np.tile(ROW6, (16, 1)), S.inv_tau_of(0.7), 0, 0.3, 7, S.SITE0)
    assert (r["count"] == 1).all() and (r["token"] == 1).all()
    assert (r["logp"] == 0.0).all() and np.isinf(r["margin"]).all()


def test_minus_inf_columns_are_never_candidates_below_1():
    x = np.tile(ROW6, (3, 1))
    x[:, [2, 4]] = -np.inf
    with np.errstate(invalid="ignore"):  # (candidates()'s gap between two -inf logits)
        for top_k in (0, 5):
            for top_p in (0.5, 0.999999):
                C = sets(x, top_k, top_p)
                assert not C[:, [2, 4]].any()
            assert sets(x, top_k, 0.999999)[:, [0, 1, 3, 5]].all()
        assert sets(x, 5, 1.0).sum() == 15  # (top_p = 1 is the base set, -inf and all)


@pytest.mark.parametrize("site", [S.SITE0, S.SITE0 + 18])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_restatement_samples_the_truncated_softmax(seed, site):
    row = np.linspace(-3, 2, 16, dtype=np.float32)
    r = N.sample(np.tile(row, (ROWS, 1)), 1.0, 0, 0.8, seed, site)
    C = r["C"][0]
    assert (r["C"] == C).all() and C.sum() == 5 and C[11:].all()  # 0.740 above the 5th, 0.815 above the 6th
    q = np.where(C, np.exp(row.astype(np.float64)), 0.0)
    q /= q.sum()
    counts = np.bincount(r["token"], minlength=16)
    assert counts[~C].sum() == 0
    x2 = S.chi2(counts[C], ROWS * q[C])
    print(f"seed {seed:#x} site {site:#x}: |C| = {C.sum()}, chi2 = {x2:.2f}")
    assert x2 < CHI2_999[C.sum() - 2]
