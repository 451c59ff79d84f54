"""Diverse beam search without a device: the float64 restatement (tests/diverse_ref.py) against beam_ref at
one group, the properties the definition promises, the conditions on the fixtures that the GPU comparison
(tests/test_gpu_diverse_beam.py) relies on, the exports and the Python layer's argument checking."""
import functools
import os
import re

import numpy as np
import pytest

import beam_ref as R
import diverse_ref as D
from test_beam_host import C1_END, C2S_END, ref_search
from test_constrain_host import BANNED, fixture
from test_ensemble_host import params64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = {"c1": C1_END, "c2s": C2S_END}
NEW = ["capgen_beam_diverse", "capgen_ensemble_beam_diverse", "capgen_debug_beam_group_step"]
# (fixture, k, G, lambda) -> (finished of k * B, the smallest margin at alpha 0 and 1, the next one at alpha 0,
#  images below 1e-3, images whose G group-best captions are pairwise distinct at alpha 0 and at alpha 1,
#  returned hypotheses (n_best = k') that were penalised at some step)
PINNED = {
    ("c1", 4, 2, 0.5): (16, 2.06e-3, 3.34e-3, 0, (8, 8), 7),
    ("c1", 6, 3, 0.5): (25, 5.0e-4, 1.55e-3, 1, (7, 8), 20),
    ("c1", 4, 4, 1.0): (17, 3.4e-5, 1.60e-3, 1, (8, 8), 0),
    ("c2s", 6, 3, 1.0): (12, 0.0154, 0.0415, 0, None, 5),
}
CONSTRAINED = dict(n=2, banned=BANNED)        # the constrained engine comparison: c1 at (4, 2, 0.5)
ENSEMBLE = ((0, 105), "prob", (.5, .5))       # the two-member engine comparison: c1 at (4, 2, 0.5)


@functools.lru_cache(maxsize=None)
def div_search(tag, k, G, lam, variant="plain"):
    """(cfg, the restatement's state) of fixture `tag`; variant 'plain', 'constrained' (CONSTRAINED) or
    'ensemble' (ENSEMBLE); computed once and shared (read only)"""
    cfg, P, f, p = fixture(tag)
    if variant == "constrained":
        import constrain_ref as CR
        rows = D.constrained_rows(P, cfg, f, p, CR.constraints(end_id=END[tag], **CONSTRAINED))
    elif variant == "ensemble":
        seeds, mode, w = ENSEMBLE
        rows = D.ensemble_rows([params64(tag, s) for s in seeds], w, mode, cfg, f, p)
    else:
        rows = D.model_rows(P, cfg, f, p)
    return cfg, D.search(rows, f.shape[0], cfg.max_length, cfg.num_vocab, k, G, lam, END[tag])


def test_one_group_is_beam_ref_whatever_the_penalty():
    _, want = ref_search("c1", 3, C1_END)
    _, got = div_search("c1", 3, 1, 0.7)
    for name in ("seq", "logp", "len", "fin", "step_margin"):
        assert np.array_equal(got[name], want[name]), name
    assert not got["penalty"].any()
    a, b = D.nbest(got, 1, 0.7, 3), R.nbest(want, 0.7, 3)
    for name in ("ids", "score", "logp", "len", "margin"):
        assert np.array_equal(a[name], b[name]), name


def random_step(seed, k, k_in, V=40, Bn=3):
    g = np.random.default_rng(seed)
    ls = R.log_softmax64(3 * g.standard_normal((k_in, Bn, V)))
    logp = -g.random((k_in, Bn))
    return ls, logp, np.zeros((k_in, Bn), np.int64), g.integers(0, 5, (k_in, Bn))


@pytest.mark.parametrize("k_in", [1, 6])
def test_a_large_penalty_with_groups_of_one_gives_distinct_tokens(k_in):
    ls, logp, fin, length = random_step(11, 6, k_in)
    st = D.step(ls, logp, fin, length, 6, 6, 100.0, end_id=7)
    for i in range(3):
        assert len(set(st["tok"][:, i].tolist())) == 6
    assert not st["count"].any()  # nothing selected was penalised
    if k_in == 1:  # the row's six best, in order; every later group's own best was displaced
        assert (st["cmax"] == 1).all()
        assert np.array_equal(st["tok"], np.argsort(-ls[0], axis=1, kind="stable")[:, :6].T)


def test_zero_penalty_gives_identical_groups_and_counts_stay_below_k_minus_kprime():
    ls, logp, fin, length = random_step(12, 6, 1)
    st = D.step(ls, logp, fin, length, 6, 3, 0.0, end_id=7)
    assert np.array_equal(st["tok"][0:2], st["tok"][2:4]) and np.array_equal(st["tok"][0:2], st["tok"][4:6])
    assert np.array_equal(st["logp"][0:2], st["logp"][4:6])
    assert st["count"].max() == 2 and st["count"].max() <= 6 - 2
    _, s = div_search("c1", 4, 2, 0.0)
    assert np.array_equal(s["seq"][:2], s["seq"][2:]) and np.array_equal(s["logp"][:2], s["logp"][2:])
    _, half = ref_search("c1", 2, C1_END)  # each group is beam_ref's search at k'
    assert np.array_equal(s["seq"][:2], half["seq"]) and np.array_equal(s["logp"][:2], half["logp"])


def test_finished_sources_are_neither_penalised_nor_counted():
    ls, logp, fin, length = random_step(13, 4, 4)
    fin[0], fin[2] = 1, 1
    ls[0], ls[2] = np.nan, np.nan
    logp[0], logp[2] = 0.0, 0.0  # the finished source leads its group
    st = D.step(ls, logp, fin, length, 4, 2, 100.0, end_id=7)
    assert (st["src"][0] == 0).all() and (st["tok"][0] == 0).all() and (st["fin"][0] == 1).all()
    assert (st["src"][2] == 2).all() and (st["tok"][2] == 0).all() and (st["logp"][2] == 0.0).all()
    assert not st["count"].any()  # (token 0 of group 0's finished source did not count against group 1's)
    assert np.array_equal(st["len"][0], length[0]) and np.array_equal(st["len"][1], length[1] + 1)


@pytest.mark.parametrize("key", sorted(PINNED))
def test_logp_is_the_sum_of_unpenalised_token_log_probabilities(key):
    _, st = div_search(*key)
    assert np.abs(st["tok_logp"].sum(axis=2) - st["logp"]).max() < 1e-12
    assert (st["tok_logp"] <= 0).all()
    live = np.arange(st["tok_logp"].shape[2])[None, None, :] < st["len"][:, :, None]
    assert (st["tok_logp"][~live] == 0).all()


@pytest.mark.parametrize("key", sorted(PINNED))
def test_conditions_of_the_gpu_comparison(key):
    tag, k, G, lam = key
    n_fin, smallest, second, below, distinct, n_pen = PINNED[key]
    cfg, st = div_search(*key)
    kg = k // G
    assert int(st["fin"].sum()) == n_fin and st["fin"].size == k * st["seq"].shape[1]
    for a, alpha in enumerate((0.0, 1.0)):
        nb = D.nbest(st, G, alpha, kg)
        R.structure_ok(nb["ids"], nb["len"], END[tag], cfg.max_length)
        m = np.sort(nb["margin"])
        assert abs(m[0] - smallest) <= 0.05 * smallest, (alpha, m)
        assert int((nb["margin"] < 1e-3).sum()) == below, (alpha, m)
        if alpha == 0.0:
            assert abs(m[1] - second) <= 0.05 * second, m
        assert (np.diff(nb["score"].reshape(G, kg, -1), axis=1) <= 0).all()
        assert int((nb["penalty"] > 0).sum()) == n_pen
        if distinct is not None:
            best = D.nbest(st, G, alpha, 1)["ids"]
            n = sum(len({tuple(best[g, i]) for g in range(G)}) == G for i in range(best.shape[1]))
            assert n == distinct[a], (alpha, n)


def test_conditions_of_the_constrained_and_ensemble_comparisons():
    """c1 at (4, 2, 0.5): at most one image below 1e-3 at either alpha, and both differ from the plain search"""
    _, plain = div_search("c1", 4, 2, 0.5)
    for variant, smallest in (("constrained", (1.44e-3, 8.2e-4)), ("ensemble", (1.15e-3, 8.0e-4))):
        _, st = div_search("c1", 4, 2, 0.5, variant)
        assert (st["seq"] != plain["seq"]).any()
        for alpha, want in zip((0.0, 1.0), smallest):
            nb = D.nbest(st, 2, alpha, 2)
            assert abs(nb["margin"].min() - want) <= 0.05 * want, (variant, alpha, nb["margin"].min())
            assert int((nb["margin"] < 1e-3).sum()) <= 1
    import constrain_ref as CR
    _, st = div_search("c1", 4, 2, 0.5, "constrained")
    for j in range(4):
        for i in range(st["seq"].shape[1]):
            tok = st["seq"][j, i, 1:1 + st["len"][j, i]]
            assert CR.repeats(tok, 2) == 0 and not set(tok.tolist()) & set(BANNED)


def test_exports():
    from capgen import _lib
    header = open(os.path.join(REPO, "include", "capgen.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 13 and lib.capgen_abi_version() == 13  # the additions are backward compatible
    from capgen.engine import Engine, ensemble_beam_diverse  # noqa: F401
    from capgen.model import Transformer
    assert callable(Engine.beam_diverse) and callable(Transformer.beam_search_diverse)


@pytest.mark.parametrize("kw, word", [
    (dict(num_groups=0), "num_groups"), (dict(num_groups=7), "num_groups"), (dict(num_groups=4), "num_groups"),
    (dict(num_groups=2.0), "num_groups"), (dict(num_groups=True), "num_groups"),
    (dict(diversity_penalty=-0.1), "diversity_penalty"), (dict(diversity_penalty=float("nan")), "diversity_penalty"),
    (dict(diversity_penalty=float("inf")), "diversity_penalty"), (dict(n_best=0), "n_best"), (dict(n_best=3), "n_best"),
    (dict(n_best=1.0), "n_best"), (dict(beam_size=17, num_groups=1), "beam_size"), (dict(beam_size=0), "beam_size"),
    (dict(end_id=1000), "end_id"), (dict(length_penalty=-1.0), "length_penalty"),
])
def test_python_argument_checks_name_the_argument(kw, word):
    from capgen.engine import check_beam_diverse_args, check_diverse_call
    args = dict(beam_size=6, num_groups=3, diversity_penalty=0.5, end_id=5, length_penalty=0.0, n_best=2, num_vocab=1000)
    assert check_beam_diverse_args(**args) == (6, 3, 2)
    assert check_beam_diverse_args(**dict(args, num_groups=1, n_best=6, diversity_penalty=0)) == (6, 1, 6)
    assert check_diverse_call(**args) is True
    # the defaults leave beam_captions the call it was: nothing is checked here, beam_nbest's own checks follow
    assert check_diverse_call(**dict(args, num_groups=1, diversity_penalty=0.0, n_best=99)) is False
    args.update(kw)
    with pytest.raises((ValueError, TypeError), match=word):
        check_beam_diverse_args(**args)
    with pytest.raises((ValueError, TypeError), match=word):
        check_diverse_call(**args)


class _NoEngine:
    """stands in for MODEL.model: a call that reaches it means a check fired too late"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def test_beam_captions_refuses_bad_group_arguments_before_the_library():
    from capgen.models import MODEL_init
    m = MODEL_init.__new__(MODEL_init)
    m.model, m.word_to_idx, m.end_idx = _NoEngine(), {"<NULL>": 0, "<START>": 1, "<END>": 2}, 2
    m.config = type("Cfg", (), {"num_vocab": 1000})()
    with pytest.raises(ValueError, match="num_groups"):
        m.beam_captions(None, None, beam_size=6, num_groups=4)
    with pytest.raises(ValueError, match="diversity_penalty"):
        m.beam_captions(None, None, beam_size=6, num_groups=3, diversity_penalty=-1.0)
    with pytest.raises(ValueError, match="n_best"):
        m.beam_captions(None, None, beam_size=6, num_groups=3, n_best=3)
