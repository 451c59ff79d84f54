"""Ensemble decoding without a device: the float64 restatement (tests/ensemble_ref.py), the conditions on
the fixtures that the GPU comparison (tests/test_gpu_ensemble.py) relies on, the exports and the Python
layer's argument checking."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import beam_ref as R
import ensemble_ref as E
from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture
from oracle import capgen_oracle as O
from test_beam_host import C1_END, C2S_END, ref_search

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = {"c1": C1_END, "c2s": C2S_END}
NEW = ["capgen_ensemble_beam_nbest", "capgen_ensemble_sample", "capgen_debug_ensemble_combine"]


@functools.lru_cache(maxsize=None)
def params64(tag, seed):
    cfg, _, _ = load_fixture(tag)
    return O.make_params(fixture_state_dict(cfg, seed=seed, with_buffer=False), requires_grad=False,
                         dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def ens_search(tag, seeds, mode, w, k=3):
    """(cfg, the restatement's state) of the ensemble of fixture_state_dict(cfg, seed=s) for s in seeds on
    fixture `tag`'s inputs; computed once and shared (read only)"""
    cfg, _, z = load_fixture(tag)
    f, p, _ = fixture_inputs(z)
    return cfg, E.search([params64(tag, s) for s in seeds], w, mode, cfg, f, p, k, END[tag])


@pytest.mark.parametrize("row", range(len(E.TABLE)))
def test_conditions_of_the_gpu_comparison(row):
    """every row of the table: the smallest margin at each pinned alpha, no image below 1e-3, the number of
    finished hypotheses"""
    tag, seeds, mode, w, alphas, (n_fin, n_hyp) = E.TABLE[row]
    cfg, st = ens_search(tag, seeds, mode, w)
    assert st["fin"].size == n_hyp and int(st["fin"].sum()) == n_fin
    for alpha, smallest in alphas:
        nb = R.nbest(st, alpha, 3)
        R.structure_ok(nb["ids"], nb["len"], END[tag], cfg.max_length)
        assert (nb["margin"] >= 1e-3).all(), (alpha, nb["margin"])
        assert abs(nb["margin"].min() - smallest) <= 0.05 * smallest, (alpha, nb["margin"].min())
        assert (np.diff(nb["score"], axis=0) <= 0).all()


@pytest.mark.parametrize("mode, seeds", [("prob", (0, 105)), ("logprob", (0, 103))])
def test_the_ensemble_is_neither_member(mode, seeds):
    """the (.5, .5) rows of c1: the best caption differs from member 0's own search on 6 of the 8 images and
    from member 1's on all 8"""
    cfg, st = ens_search("c1", seeds, mode, (.5, .5))
    best = R.nbest(st, 0.0, 1)["ids"][0]
    _, s0 = ref_search("c1", 3, C1_END)
    _, s1 = ens_search("c1", seeds[1:], "prob", None)
    d0 = int((best != R.nbest(s0, 0.0, 1)["ids"][0]).any(axis=1).sum())
    d1 = int((best != R.nbest(s1, 0.0, 1)["ids"][0]).any(axis=1).sum())
    assert (d0, d1) == (6, 8), (d0, d1)


def test_one_member_is_the_single_search():
    _, st = ens_search("c1", (0,), "prob", None)
    _, ref = ref_search("c1", 3, C1_END)
    assert np.array_equal(st["seq"], ref["seq"]) and np.abs(st["logp"] - ref["logp"]).max() < 1e-12


@pytest.mark.parametrize("mode", E.MODES)
def test_combine_with_one_member_is_log_softmax(mode):
    g = np.random.default_rng(3)
    z = 3 * g.standard_normal((1, 5, 40))
    assert np.abs(E.combine(z, None, mode) - R.log_softmax64(z[0])).max() < 1e-12
    assert np.abs(E.combine(z, [7.0], mode) - R.log_softmax64(z[0])).max() < 1e-12


def test_combine_prob_is_the_mean_of_the_probabilities_and_logprob_of_the_logs():
    g = np.random.default_rng(4)
    z = 3 * g.standard_normal((3, 4, 24))
    w = np.array([.5, .3, .2])
    p = np.exp(R.log_softmax64(z))
    y = E.combine(z, w, "prob")
    assert np.abs(np.exp(y) - (w[:, None, None] * p).sum(0)).max() < 1e-14
    assert np.abs(np.exp(y).sum(-1) - 1).max() < 1e-12  # already normalised
    y = E.combine(z, w, "logprob")
    assert np.abs(y - (w[:, None, None] * np.log(p)).sum(0)).max() < 1e-12
    assert (np.exp(y).sum(-1) < 1).all()  # the geometric mean is not: the selection normalises it


def test_combine_weights_are_normalised():
    g = np.random.default_rng(5)
    z = 3 * g.standard_normal((2, 3, 16))
    for mode in E.MODES:
        assert np.abs(E.combine(z, [.7, .3], mode) - E.combine(z, [14.0, 6.0], mode)).max() < 1e-12
        assert np.abs(E.combine(z, None, mode) - E.combine(z, [2.0, 2.0], mode)).max() < 1e-12


def test_combine_prob_stays_finite_where_every_probability_underflows_in_f32():
    g = np.random.default_rng(6)
    z = 3 * g.standard_normal((2, 2, 32))
    z[:, :, 5] = -150.0  # exp(-104) is below the smallest f32 denormal
    l = R.log_softmax64(z)
    assert (l[:, :, 5] < -104).all()
    y = E.combine(z, [.5, .5], "prob")
    assert np.isfinite(y).all() and (y[:, 5] < -104).all()
    with np.errstate(divide="ignore"):
        naive = np.log((0.5 * np.exp(l.astype(np.float32))).sum(0))  # the form the definition rules out
    assert np.isneginf(naive[:, 5]).all()


def test_exports():
    from capgen import _lib
    header = open(os.path.join(REPO, "include", "capgen.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    assert "CAPGEN_ENS_PROB = 0" in header and "CAPGEN_ENS_LOGPROB = 1" in header
    assert _lib.ENS_MODES == {"prob": 0, "logprob": 1}
    assert _lib.ABI_VERSION == 13 and lib.capgen_abi_version() == 13  # the additions are backward compatible
    import capgen
    assert "Ensemble" in capgen.__all__ and capgen.Ensemble.__name__ == "Ensemble"


class _Member:
    """stands in for a MODEL: every check below must fire before an engine is asked for"""

    def __init__(self, words=("<NULL>", "<START>", "<END>", "a")):
        self.word_to_idx = {w: i for i, w in enumerate(words)}
        self.end_idx = self.word_to_idx.get("<END>")


@pytest.mark.parametrize("kw, word", [
    (dict(n=0), "engines"), (dict(n=9), "engines"), (dict(dup=True), "duplicate"), (dict(mode="mean"), "mode"),
    (dict(mode=0), "mode"), (dict(weights=(1.0,)), "weights"), (dict(weights=(1.0, 0.0)), r"weights\[1\]"),
    (dict(weights=(-1.0, 1.0)), r"weights\[0\]"), (dict(weights=(1.0, float("nan"))), r"weights\[1\]"),
    (dict(weights=(float("inf"), 1.0)), r"weights\[0\]"),
])
def test_python_argument_checks_name_the_argument(kw, word):
    from capgen.engine import check_ensemble_args
    members = [object() for _ in range(kw.get("n", 2))]
    if kw.get("dup"):
        members[1] = members[0]
    ok = check_ensemble_args([object(), object()], (2.0, 6.0), "logprob")
    assert ok[1] == [2.0, 6.0] and ok[2] == 1 and check_ensemble_args([object()], None, "prob")[1:] == (None, 0)
    with pytest.raises(ValueError, match=word):
        check_ensemble_args(members, kw.get("weights"), kw.get("mode", "prob"))


def test_ensemble_object_argument_checks():
    from capgen.ensemble import Ensemble
    a, b = _Member(), _Member()
    e = Ensemble([a, b], weights=(3.0, 1.0))
    assert e.leader is a and e.norm_weights == [0.75, 0.25] and Ensemble([a]).norm_weights == [1.0]
    with pytest.raises(ValueError, match="word_to_idx"):
        Ensemble([a, _Member(("<NULL>", "<START>", "<END>", "b"))])
    with pytest.raises(ValueError, match="duplicate"):
        Ensemble([a, a])
    with pytest.raises(ValueError, match="mode"):
        Ensemble([a, b], mode="geometric")
    with pytest.raises(ValueError, match=r"weights\[1\]"):
        Ensemble([a, b], weights=(1.0, -2.0))
    with pytest.raises(ValueError, match="mode"):  # the refusal comes before any member is asked to score
        Ensemble([a, b], mode="logprob").score_captions(None, None, None)
