"""Sampled decoding, host side: the exports, the float64 restatement's own statistics (tests/
sampling_ref.py -- the GPU tests hold the kernel to it, so it must itself draw from the right
distribution), and capgen.utils.sequence_logprob.  All inputs are fixed: nothing here can flake."""
import numpy as np
import pytest
import torch

import sampling_ref as S

ROWS = 65536
CHI2_15_999 = 37.70  # 0.999 quantile of chi-square at 15 degrees of freedom


def test_exports():
    from capgen import _lib
    assert "capgen_sample" in _lib.EXPORTED
    assert "capgen_debug_sample_softmax" in _lib.EXPORTED
    assert _lib.ABI_VERSION == 13


def test_uniform_is_strictly_inside_the_unit_interval():
    lo = ((0 >> 9) + 0.5) * 2.0 ** -23
    hi = ((0xFFFFFFFF >> 9) + 0.5) * 2.0 ** -23
    assert 0.0 < lo and hi < 1.0
    assert np.float32(lo) == lo and np.float32(hi) == hi  # exact in f32
    u = S.uniform(S.SEEDS[0], S.SITE0, np.arange(4096))
    assert ((u > 0) & (u < 1)).all() and (u.astype(np.float32) == u).all()


@pytest.mark.parametrize("site", [S.SITE0, S.SITE0 + 18])
@pytest.mark.parametrize("seed", S.SEEDS)
def test_restatement_samples_the_softmax(seed, site):
    row = np.linspace(-3, 2, 16, dtype=np.float32)
    p = np.exp(row.astype(np.float64))
    p /= p.sum()
    tok = S.sample(np.tile(row, (ROWS, 1)), 1.0, 0, seed, site)["token"]
    x2 = S.chi2(np.bincount(tok, minlength=16), ROWS * p)
    print(f"seed {seed:#x} site {site:#x}: chi2 = {x2:.2f}")
    assert x2 < CHI2_15_999


@pytest.mark.parametrize("seed", S.SEEDS)
def test_restatement_sites_and_rows_are_independent(seed):
    """4 uniform columns: the joint 4 x 4 table of one row's tokens at two sites, and of adjacent rows
    at one site, against the uniform table (15 degrees of freedom each)"""
    x = np.zeros((ROWS, 4), dtype=np.float32)
    a = S.sample(x, 1.0, 0, seed, S.SITE0 + 1)["token"]
    b = S.sample(x, 1.0, 0, seed, S.SITE0 + 2)["token"]
    sites = S.chi2(np.bincount(a * 4 + b, minlength=16), np.full(16, ROWS / 16))
    rows = S.chi2(np.bincount(a[:-1] * 4 + a[1:], minlength=16), np.full(16, (ROWS - 1) / 16))
    print(f"seed {seed:#x}: sites chi2 = {sites:.2f}, adjacent rows chi2 = {rows:.2f}")
    assert sites < CHI2_15_999
    assert rows < CHI2_15_999


def test_restatement_top_k_and_logp():
    x = np.array([[0.5, 3.0, 3.0, -1.0, 2.0, 2.5]], dtype=np.float32)
    C, gap = S.candidates(x, 3)
    assert C[0].tolist() == [False, True, True, False, False, True] and gap[0] == 0.5
    C, _ = S.candidates(x, 1)
    assert C[0].tolist() == [False, True, False, False, False, False]  # first index on ties
    r = S.sample(x, 1.0, 1, 7, S.SITE0)
    assert r["token"][0] == 1 and r["logp"][0] == 0.0
    for k in (0, 3):
        r = S.sample(np.tile(x, (64, 1)), S.inv_tau_of(0.7), k, 7, S.SITE0)
        C, _ = S.candidates(x, k)
        z = (x[0] * S.inv_tau_of(0.7)).astype(np.float64)
        lp = z - np.log(np.exp(z[C[0]]).sum())
        assert C[0][r["token"]].all()
        np.testing.assert_allclose(r["logp"], lp[r["token"]], atol=1e-12)


END = 2


@pytest.mark.parametrize("ids, want", [
    ([END, 5, 6, 7], -1.0),              # <END> first
    ([5, 6, 7, END], -1.0 - 2 - 4 - 8),  # <END> last
    ([5, 6, 7, 8], -1.0 - 2 - 4 - 8),    # no <END>
    ([5, END, 7, END], -1.0 - 2),        # <END> twice: the first one ends the caption
])
def test_sequence_logprob(ids, want):
    from capgen.utils import sequence_logprob
    logp = torch.tensor([-1.0, -2.0, -4.0, -8.0])
    assert sequence_logprob(torch.tensor(ids), logp, END).item() == want
    # batched [n, B, T], numpy in
    out = sequence_logprob(np.array(ids).reshape(1, 1, 4).repeat(3, 1), logp.view(1, 1, 4).repeat(1, 3, 1).numpy(), END)
    assert out.shape == (1, 3) and (out == want).all()


def test_sequence_logprob_shape_mismatch():
    from capgen.utils import sequence_logprob
    with pytest.raises(ValueError):
        sequence_logprob(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 4), END)
