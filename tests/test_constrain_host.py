"""The decode constraints without a device: the float64 restatement (tests/constrain_ref.py) on small
hand-made rows, and the conditions on the fixtures that the GPU comparison (tests/test_gpu_constrain.py)
rests on -- what the constrained searches finish, at which lengths, with no repeated n-gram, and with which
margins -- as tests/test_beam_host.py pins them for the unconstrained search."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
import constrain_ref as CR
from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture
from oracle import capgen_oracle as O
from test_beam_host import C1_END, C2S_END, ref_search

K = 3
BANNED = (575, 922, 75)
# name -> (fixture, <END>, settings, blocked entries, finished hypotheses of the 24, their lengths,
#          {alpha: smallest margin})
C1_SETTINGS = {
    "n2": ("c1", C1_END, dict(n=2), 84, 12, {1, 2, 3, 4, 5, 8, 9}, {0.0: 1.3e-3, 1.0: 1.1e-3}),
    "n3_m4": ("c1", C1_END, dict(n=3, m=4), 84, 8, {4, 5, 7, 9}, {0.0: 1.1e-3, 1.0: 1.0e-3}),
    "n2_m4_pen_ban": ("c1", C1_END, dict(n=2, m=4, theta=1.2, banned=BANNED), 699, 14, {4, 5, 6, 7, 8, 9},
                      {0.0: 1.6e-3, 1.0: 1.6e-3}),
}
C2S_SETTINGS = {
    "m5": ("c2s", C2S_END, dict(m=5), 1.3e-3),
    "n2_m5_pen": ("c2s", C2S_END, dict(n=2, m=5, theta=1.2), 1.3e-3),
}
MARGIN = 1e-3
ROUNDING = 0.05e-3 + 1e-9  # the smallest margins above are given to two digits


@functools.lru_cache(maxsize=None)
def fixture(tag):
    cfg, seed, z = load_fixture(tag)
    P = O.make_params(fixture_state_dict(cfg, seed=seed, with_buffer=False), requires_grad=False, dtype=torch.float64)
    f, p, _ = fixture_inputs(z)
    return cfg, P, f, p


@functools.lru_cache(maxsize=None)
def constrained_search(name):
    """(cfg, the settings, the restatement's state) of a named setting; computed once and shared (read only)"""
    tag, end, kw = (C1_SETTINGS.get(name) or C2S_SETTINGS[name])[:3]
    cfg, P, f, p = fixture(tag)
    c = CR.constraints(end_id=end, **kw)
    return cfg, c, CR.search(P, cfg, f, p, K, end, c)


def hypotheses(st):
    """every (tokens emitted while live, len) of a search state"""
    k, B, _ = st["seq"].shape
    return [(st["seq"][j, i, 1:1 + st["len"][j, i]], int(st["len"][j, i])) for j in range(k) for i in range(B)]


# ---- the definition on small rows ------------------------------------------------------------------------
def test_penalty_is_applied_once_per_word_and_by_sign():
    z = np.array([2.0, -2.0, 0.0, 3.0, 1.0, -1.0], dtype=np.float64)
    e = [1, 0, 1, 0, 0, 5]  # <START> = 1 in column 0 is not counted; word 0 three times, word 1 once, word 5
    c = CR.constraints(theta=2.0)
    got = CR.edit(z, e, 5, c)
    assert got.tolist() == [1.0, -4.0, 0.0, 3.0, 1.0, -2.0]
    assert CR.edit(z, e, 0, c).tolist() == z.tolist()  # no history at t = 0
    assert CR.touched(e, 5, c, 6) == ([0, 1, 5], set())
    z32 = np.array([0.7, -0.3], dtype=np.float32)
    got = CR.edit(z32, [1, 0, 1], 2, CR.constraints(theta=1.3))
    assert got[0] == float(np.float32(0.7) / np.float32(1.3)) and got[1] == float(np.float32(-0.3) * np.float32(1.3))


def test_blocked_wins_over_penalised_and_min_length_counts_end():
    z = np.ones(8)
    e = [1, 4, 5, 4]
    c = CR.constraints(n=2, m=5, end_id=6, theta=2.0, banned=(4, 7))
    got = CR.edit(z, e, 3, c)  # bigram (4, 5) seen and the history ends in 4: 5 is blocked; 4 banned and penalised
    assert np.isneginf(got[[4, 5, 6, 7]]).all() and got[[0, 1, 2, 3]].tolist() == [1.0] * 4
    # <END> at step t gives len = t + 1: allowed from t + 1 == m on
    assert np.isneginf(CR.edit(z, e, 3, CR.constraints(m=5, end_id=6))[6])
    assert CR.edit(z, [1, 4, 5, 4, 2], 4, CR.constraints(m=5, end_id=6))[6] == 1.0


def test_ngram_rule_edges():
    z = np.zeros(10)
    e = [1, 3, 4, 3, 4, 3]
    assert CR.touched(e, 5, CR.constraints(n=1), 10)[1] == {3, 4}           # every emitted word
    assert CR.touched(e, 5, CR.constraints(n=2), 10)[1] == {4}              # after 3 came 4 (twice)
    assert CR.touched(e, 5, CR.constraints(n=3), 10)[1] == {4}              # after (4, 3) came 4
    assert CR.touched(e, 4, CR.constraints(n=3), 10)[1] == {3}              # after (3, 4) came 3
    assert CR.touched(e, 1, CR.constraints(n=2), 10)[1] == set()            # one token: no bigram yet
    assert CR.touched(e, 1, CR.constraints(n=3), 10)[1] == set()            # t < n - 1
    assert CR.touched([1, 1, 1], 2, CR.constraints(n=2), 10)[1] == {1}      # <START>'s own id in column 0 is not history
    assert CR.touched([1, 12, 3], 2, CR.constraints(n=1), 10)[1] == {3}     # an id outside the vocabulary names no column
    assert np.isneginf(CR.edit(z, e, 5, CR.constraints(n=2))).sum() == 1
    assert CR.repeats([3, 4, 3, 4, 3], 2) == 2 and CR.repeats([3, 4, 3, 4, 3], 3) == 1 and CR.repeats([3, 4, 5], 1) == 0


# ---- the fixtures -------------------------------------------------------------------------------------------
def test_unconstrained_c1_repeats_itself():
    """what the constraints are for: the plain search's hypotheses repeat bigrams"""
    _, st = ref_search("c1", K, C1_END)
    reps = [CR.repeats(tok, 2) for tok, _ in hypotheses(st)]
    assert len(reps) == 24 and sum(r > 0 for r in reps) >= 1


@pytest.mark.parametrize("name", sorted(C1_SETTINGS))
def test_c1_conditions_of_the_gpu_comparison(name):
    _, _, kw, n_blocked, n_fin, lens, smallest = C1_SETTINGS[name]
    cfg, c, st = constrained_search(name)
    T = cfg.max_length
    assert st["blocked"] == n_blocked
    assert int(st["fin"].sum()) == n_fin and st["fin"].size == 24
    assert set(st["len"][st["fin"] == 1].tolist()) == lens
    assert (st["len"][st["fin"] == 0] == T - 1).all()
    for tok, ln in hypotheses(st):
        assert CR.repeats(tok, c["n"]) == 0, tok
        assert not set(tok.tolist()) & set(c["banned"]), tok
        assert C1_END not in tok[:max(c["m"] - 1, 0)].tolist(), tok
    _, plain = ref_search("c1", K, C1_END)
    for alpha, want in smallest.items():
        nb = R.nbest(st, alpha, K)
        R.structure_ok(nb["ids"], nb["len"], C1_END, T)
        assert (nb["margin"] >= MARGIN).all(), (name, alpha, nb["margin"])
        assert abs(nb["margin"].min() - want) <= ROUNDING, (name, alpha, nb["margin"].min())
        assert (np.diff(nb["score"], axis=0) <= 0).all()
        differs = (nb["ids"] != R.nbest(plain, alpha, K)["ids"]).any(axis=(0, 2))
        assert differs.any(), (name, alpha)


@pytest.mark.parametrize("name", sorted(C2S_SETTINGS))
def test_c2s_conditions_of_the_gpu_comparison(name):
    _, _, _, want = C2S_SETTINGS[name]
    cfg, c, st = constrained_search(name)
    assert st["fin"].all() and (st["len"] == 5).all()
    _, plain = ref_search("c2s", K, C2S_END)
    assert plain["len"].max() <= 2  # so every result differs from the unconstrained one
    for alpha in (0.0, 1.0):
        nb = R.nbest(st, alpha, K)
        R.structure_ok(nb["ids"], nb["len"], C2S_END, cfg.max_length)
        assert (nb["margin"] >= MARGIN).all() and abs(nb["margin"].min() - want) <= ROUNDING, (name, nb["margin"])
    for tok, _ in hypotheses(st):
        assert CR.repeats(tok, c["n"]) == 0 if c["n"] else True


def test_exports():
    from capgen import _lib
    for name in ("capgen_set_decode_constraints", "capgen_debug_constrain_logits"):
        assert name in _lib.EXPORTED
    assert _lib.ABI_VERSION == 13
    c = _lib.decode_constraints(2, 4, 7, 1.2, (5, 6))
    assert (c.no_repeat_ngram, c.min_length, c.end_id, c.n_banned) == (2, 4, 7, 2)
    assert [c.banned[i] for i in range(2)] == [5, 6] and abs(c.repetition_penalty - 1.2) < 1e-6
