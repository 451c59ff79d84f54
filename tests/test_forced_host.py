"""Forced-word beam search without a device: the float64 restatement (tests/forced_ref.py) against beam_ref with
no words, the properties the definition promises, the conditions on the fixtures that the GPU comparison
(tests/test_gpu_forced_beam.py) relies on, the exports and the Python layer's argument checking."""
import functools
import os
import re

import numpy as np
import pytest

import beam_ref as R
import diverse_ref as D
import forced_ref as F
from test_beam_host import C1_END, C2S_END, ref_search
from test_constrain_host import fixture
from test_diverse_host import CONSTRAINED, ENSEMBLE
from test_ensemble_host import params64

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = {"c1": C1_END, "c2s": C2S_END}
NEW = ["capgen_beam_forced", "capgen_ensemble_beam_forced", "capgen_debug_beam_forced_step"]
# (fixture, k, W, C) -> (the smallest margin at alpha 0 and 1, images below 1e-3 at alpha 0 and 1, images whose
#  best caption met every group, hypotheses (n_best = k) that met every group, finished of k * B).  The words:
#  forced_ref.fixture_words.  As the restatement finds them; they are the issue's table.
PINNED = {
    ("c1", 3, 2, 2): ((2.06e-3, 2.06e-3), (0, 0), 8, 8, 4),
    ("c1", 5, 2, 2): ((1.27e-3, 1.6e-4), (0, 1), 8, 16, 7),
    ("c1", 5, 3, 2): ((1.43e-3, 1.6e-4), (0, 1), 8, 16, 6),
    ("c1", 4, 4, 4): ((2.35e-3, 2.35e-3), (0, 0), 8, 8, 2),
    ("c2s", 3, 2, 2): ((2.11e-3, 2.11e-3), (0, 0), 2, 2, 2),
}
# the constrained and the two-member comparison, c1 at (3, 2, 2): the smallest margin at alpha 0 and 1
VARIANTS = {"constrained": (1.56e-3, 1.56e-3), "ensemble": (4.56e-4, 4.56e-4)}
# CONSTRAINED bans words 75 and 575, which the fixture conditions make the first word of images 4 and 7: there the
# top bank's only way on is the blocked word, and the best "caption" has logp -inf -- as the definition says
BLOCKED_IMAGES = (4, 7)


@functools.lru_cache(maxsize=None)
def fixture_slots(tag, k, W, C):
    cfg, P, f, p = fixture(tag)
    return F.fixture_words(P, cfg, f, p, k, W, C, END[tag])


@functools.lru_cache(maxsize=None)
def forced_search(tag, k, W, C, variant="plain"):
    """(cfg, word, group, the restatement's state) of fixture `tag` with the fixture conditions' words; variant
    'plain', 'constrained' (test_diverse_host.CONSTRAINED) or 'ensemble' (ENSEMBLE); computed once and shared
    (read only)"""
    cfg, P, f, p = fixture(tag)
    word, group = fixture_slots(tag, k, W, C)
    if variant == "constrained":
        import constrain_ref as CR
        rows = D.constrained_rows(P, cfg, f, p, CR.constraints(end_id=END[tag], **CONSTRAINED))
    elif variant == "ensemble":
        seeds, mode, w = ENSEMBLE
        rows = D.ensemble_rows([params64(tag, s) for s in seeds], w, mode, cfg, f, p)
    else:
        rows = D.model_rows(P, cfg, f, p)
    return cfg, word, group, F.search(rows, f.shape[0], cfg.max_length, cfg.num_vocab, k, END[tag], word, group)


@pytest.mark.parametrize("tag", ["c1", "c2s"])
def test_no_words_is_beam_ref_exactly(tag):
    cfg, P, f, p = fixture(tag)
    B = f.shape[0]
    _, want = ref_search(tag, 3, END[tag])
    got = F.search(D.model_rows(P, cfg, f, p), B, cfg.max_length, cfg.num_vocab, 3, END[tag],
                   np.full((B, 2), -1), np.zeros((B, 2), np.int64))
    for name in ("seq", "logp", "len", "fin", "step_margin"):
        assert np.array_equal(got[name], want[name]), name
    assert not got["met"].any()
    a, b = F.nbest(got, 0.7, 3), R.nbest(want, 0.7, 3)
    for name in ("ids", "score", "logp", "len", "margin"):
        assert np.array_equal(a[name], b[name]), name


def random_step(seed, k, k_in, W, C, V=40, Bn=3):
    g = np.random.default_rng(seed)
    ls = R.log_softmax64(3 * g.standard_normal((k_in, Bn, V)))
    logp = -g.random((k_in, Bn))
    word = np.stack([g.choice(np.arange(2, V), W, replace=False) for _ in range(Bn)])
    group = g.integers(0, C, (Bn, W))
    _, full = F.slot_bits(word, group, V)
    met = g.integers(0, 1 << 16, (k_in, Bn)) & full[None]
    return ls, logp, np.zeros((k_in, Bn), np.int64), g.integers(0, 5, (k_in, Bn)), met, word, group


@pytest.mark.parametrize("seed", range(6))
def test_round_robin_properties(seed):
    """the beams' banks come in rounds, each strictly descending over the banks that still have candidates; a
    bank's selections are its best in order; every selected met' is its source's met plus the token's bits; a
    high bank is served first however bad its score"""
    k, W, C, V = 6, 5, 4, 40
    ls, logp, fin, length, met, word, group = random_step(100 + seed, k, k if seed % 2 else 1, W, C, V)
    st = F.step(ls, logp, fin, length, met, k, 7, word, group)
    bits, full = F.slot_bits(word, group, V)
    for i in range(3):
        bank = st["bank"][:, i].tolist()
        assert bank[0] == max(bank)
        rounds = [[bank[0]]]  # the maximal strictly descending runs
        for b in bank[1:]:
            if b < rounds[-1][-1]:
                rounds[-1].append(b)
            else:
                rounds.append([b])
        for prev, cur in zip(rounds, rounds[1:]):  # a bank that has run out leaves, none joins later
            it = iter(prev)
            assert all(b in it for b in cur), rounds
        for b in set(bank):
            s = st["logp"][np.array(bank) == b, i]
            assert (np.diff(s) <= 0).all()
        for r in range(k):
            j, v = st["src"][r, i], st["tok"][r, i]
            assert st["met"][r, i] == met[j, i] | bits[i, v] and st["bank"][r, i] == bin(st["met"][r, i]).count("1")
            assert st["advanced"][r, i] == int(bool(bits[i, v] & ~met[j, i]))
        if k >= st["banks"][i]:
            assert len(set(bank[:st["banks"][i]])) == st["banks"][i]
    assert st["banks"].max() >= (3 if seed % 2 else 2)  # (one source row: its own bank and the next)


def test_scores_are_never_compared_across_banks():
    """one live row, word 5 (group 0) and word 6 (groups 0 and 3) far less likely than the rest: the two-group
    word leads, the one-group word follows, then the row's best; at the next visit of bank 0 its second"""
    x = np.array([[[5.0, 4.0, 3.0, 2.0, 1.0, -20.0, -30.0, 0.0]]])
    ls = R.log_softmax64(x)
    z = np.zeros((1, 1), np.int64)
    word, group = np.array([[5, 6, 6, -1]]), np.array([[0, 0, 3, 9]])
    st = F.step(ls, np.zeros((1, 1)), z, z, z, 4, -1, word, group)
    assert st["tok"][:, 0].tolist() == [6, 5, 0, 1] and st["met"][:, 0].tolist() == [9, 1, 0, 0]
    assert st["bank"][:, 0].tolist() == [2, 1, 0, 0] and st["banks"][0] == 3
    assert st["gap"][0] == 1.0  # only bank 0 has a pair among its first taken + 1: (5, 4), (4, 3)
    # the same row with group 0 already met: word 5 stays in its bank, word 6 still advances
    st = F.step(ls, np.zeros((1, 1)), z, z, z + 1, 4, -1, word, group)
    assert st["tok"][:, 0].tolist() == [6, 0, 1, 2] and st["met"][:, 0].tolist() == [9, 1, 1, 1]


def test_a_live_source_with_an_unmet_group_never_ends():
    k, W, C, V, end = 4, 3, 2, 40, 7
    ls, logp, fin, length, met, word, group = random_step(21, k, k, W, C, V)
    word[word == end] = 8
    x = ls.copy()
    x[:, :, end] += 50.0  # <END> is every row's best by far
    ls = R.log_softmax64(x)
    bits, full = F.slot_bits(word, group, V)
    met[:] = 0
    met[1] = full  # beam 1 has met everything: it may end
    st = F.step(ls, logp, fin, length, met, k, end, word, group)
    ended = st["tok"] == end
    assert ended.any() and (st["src"][ended] == 1).all() and (st["fin"][ended] == 1).all()
    assert (st["fin"][~ended] == 0).all()
    # with no slot at all every row may end
    none = F.step(ls, logp, fin, length, np.zeros_like(met), k, end, np.full((3, W), -1), np.zeros((3, W), np.int64))
    assert (none["tok"] == end).all()


def test_finished_sources_copy_met_and_offer_one_candidate():
    k, W, C, V = 4, 3, 3, 40
    ls, logp, fin, length, met, word, group = random_step(22, k, k, W, C, V)
    _, full = F.slot_bits(word, group, V)
    fin[0], fin[2] = 1, 1
    ls[0], ls[2] = np.nan, np.nan
    met[0], met[2] = full, full
    logp[0], logp[2] = 0.0, -0.5
    st = F.step(ls, logp, fin, length, met, k, 7, word, group)
    for i in range(3):
        from_fin = [r for r in range(k) if st["src"][r, i] in (0, 2)]
        assert sorted(st["src"][from_fin, i].tolist()) == [0, 2]  # each offers itself once
        for r in from_fin:
            j = st["src"][r, i]
            assert st["tok"][r, i] == 0 and st["fin"][r, i] == 1 and st["met"][r, i] == met[j, i]
            assert st["len"][r, i] == length[j, i] and st["logp"][r, i] == logp[j, i] and not st["advanced"][r, i]
    assert np.isfinite(st["logp"]).all()


@pytest.mark.parametrize("key", sorted(PINNED))
def test_logp_is_the_sum_of_its_tokens_log_probabilities(key):
    _, _, _, st = forced_search(*key)
    assert np.abs(st["tok_logp"].sum(axis=2) - st["logp"]).max() < 1e-12
    assert (st["tok_logp"] <= 0).all()
    live = np.arange(st["tok_logp"].shape[2])[None, None, :] < st["len"][:, :, None]
    assert (st["tok_logp"][~live] == 0).all()


def close(got, want):
    return abs(got - want) <= 0.05 * want


@pytest.mark.parametrize("key", sorted(PINNED))
def test_conditions_of_the_gpu_comparison(key):
    tag, k, W, C = key
    smallest, below, best_full, n_full, n_fin = PINNED[key]
    cfg, word, group, st = forced_search(*key)
    Bn = st["seq"].shape[1]
    _, full = F.slot_bits(word, group, cfg.num_vocab)
    assert (word >= 2).all() and (word != END[tag]).all() and (group == np.minimum(np.arange(W), C - 1)).all()
    assert int(st["fin"].sum()) == n_fin
    _, plain = ref_search(tag, k, END[tag])
    for a, alpha in enumerate((0.0, 1.0)):
        nb = F.nbest(st, alpha, k)
        R.structure_ok(nb["ids"], nb["len"], END[tag], cfg.max_length)
        F.words_ok(nb["ids"], nb["len"], nb["met"], word, group, END[tag])
        assert close(nb["margin"].min(), smallest[a]), (alpha, nb["margin"])
        assert int((nb["margin"] < 1e-3).sum()) == below[a], (alpha, nb["margin"])
        assert int((nb["met"][0] == full).sum()) == best_full and best_full == Bn
        assert int((nb["met"] == full[None]).sum()) == n_full
        bank = F.popcount(nb["met"])
        assert (np.diff(bank, axis=0) <= 0).all()
        assert (np.diff(nb["score"], axis=0)[np.diff(bank, axis=0) == 0] <= 0).all()
        best = R.nbest(plain, alpha, 1)["ids"][0]
        assert (nb["ids"][0] != best).any(axis=1).all()  # the words change the best caption of every image


@pytest.mark.parametrize("variant", sorted(VARIANTS))
def test_conditions_of_the_constrained_and_ensemble_comparisons(variant):
    """c1 at (3, 2, 2): at most one image below 1e-3 at either alpha, and the search differs from the plain one"""
    _, _, _, plain = forced_search("c1", 3, 2, 2)
    cfg, word, group, st = forced_search("c1", 3, 2, 2, variant)
    assert (st["seq"] != plain["seq"]).any()
    for alpha, want in zip((0.0, 1.0), VARIANTS[variant]):
        nb = F.nbest(st, alpha, 3)
        F.words_ok(nb["ids"], nb["len"], nb["met"], word, group, C1_END)
        assert close(nb["margin"].min(), want), (variant, alpha, nb["margin"].min())
        assert int((nb["margin"] < 1e-3).sum()) <= 1
    if variant == "constrained":
        import constrain_ref as CR
        from test_constrain_host import BANNED
        banned_forced = [i for i in range(word.shape[0]) if set(word[i].tolist()) & set(BANNED)]
        assert tuple(banned_forced) == BLOCKED_IMAGES
        blocked = np.isneginf(st["logp"])  # a forced word the constraints block scores -inf like any blocked word
        assert tuple(np.nonzero(blocked.any(axis=0))[0]) == BLOCKED_IMAGES and blocked.sum() == 2
        assert (F.popcount(st["met"])[blocked] == 2).all()  # ... and still leads: the only one that met both
        for j in range(3):
            for i in range(st["seq"].shape[1]):
                tok = st["seq"][j, i, 1:1 + st["len"][j, i]]
                if not blocked[j, i]:
                    assert CR.repeats(tok, 2) == 0 and not set(tok.tolist()) & set(BANNED)


def test_finish_ranks_by_groups_met_before_score():
    logp = np.array([[-1.0], [-9.0], [-2.0], [-3.0]])
    length = np.array([[2], [2], [1], [4]])
    met = np.array([[0], [3], [1], [4]])
    f = F.finish(logp, length, met, 0.0, 4)
    assert f["order"][:, 0].tolist() == [1, 2, 3, 0] and f["met"][:, 0].tolist() == [3, 1, 4, 0]
    assert f["final_margin"][0] == 1.0  # only beams 2 and 3 share a bank
    f = F.finish(logp, length, met, 1.0, 2)
    assert f["order"][:, 0].tolist() == [1, 3] and np.allclose(f["score"][:, 0], [-4.5, -0.75])


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
    from capgen.engine import Engine, ensemble_beam_forced  # noqa: F401
    from capgen.model import Transformer
    assert callable(Engine.beam_forced) and callable(Transformer.beam_search_forced)


GOOD = dict(beam_size=5, end_id=5, length_penalty=0.0, n_best=2, word=[[7, 9], [8, -1]], group=[[0, 1], [0, 0]], B=2,
            num_vocab=1000)


@pytest.mark.parametrize("kw, name", [
    (dict(beam_size=0), "beam_size"), (dict(beam_size=17), "beam_size"), (dict(n_best=6), "n_best"),
    (dict(end_id=1000), "end_id"), (dict(length_penalty=-1.0), "length_penalty"),
    (dict(beam_size=14), "beam_size \\+ words"), (dict(beam_size=5, num_vocab=7), "num_vocab"),
    (dict(word=[[7, 9]], group=[[0, 1]]), "word"), (dict(group=[[0, 1, 2], [0, 0, 0]]), "group"),
    (dict(word=[[7, 5], [8, -1]]), "word"), (dict(word=[[0, 9], [8, -1]]), "word"), (dict(word=[[1, 9], [8, -1]]), "word"),
    (dict(word=[[7, 1000], [8, -1]]), "word"), (dict(word=[[7, -2], [8, -1]]), "word"),
    (dict(group=[[0, 16], [0, 0]]), "group"), (dict(group=[[-1, 1], [0, 0]]), "group"),
    (dict(word=[[7.5, 9], [8, -1]]), "word"),
])
def test_python_argument_checks_name_the_argument(kw, name):
    from capgen.engine import check_beam_forced_args
    k, n, word, group = check_beam_forced_args(**GOOD)
    assert (k, n) == (5, 2) and word.dtype == np.int32 and group.dtype == np.int32 and word.shape == (2, 2)
    # no word on any image: nothing to force (whatever group holds)
    assert check_beam_forced_args(**dict(GOOD, word=[[-1, -1], [-1, -1]], group=[[99, 0], [0, 0]]))[2:] == (None, None)
    assert check_beam_forced_args(**dict(GOOD, word=np.zeros((2, 0), int), group=np.zeros((2, 0), int)))[2] is None
    with pytest.raises((ValueError, TypeError), match=name):
        check_beam_forced_args(**dict(GOOD, **kw))


WORDS = {"<NULL>": 0, "<START>": 1, "<END>": 2, "dog": 10, "dogs": 11, "puppy": 12, "frisbee": 13, "grass": 14}


def test_must_include_becomes_slots():
    from capgen.engine import must_include_slots
    assert must_include_slots(None, WORDS, 2, 5) is None
    assert must_include_slots([[], ()], WORDS, 2, 5) is None
    assert must_include_slots([[], None], WORDS, 2, 5, num_groups=5) is None  # nothing required: nothing refused
    word, group = must_include_slots([[("dog", "dogs", "puppy"), "frisbee"], []], WORDS, 2, 5)
    assert word.tolist() == [[10, 11, 12, 13], [-1, -1, -1, -1]] and group.tolist() == [[0, 0, 0, 1], [0, 0, 0, 0]]
    word, group = must_include_slots([["grass"], ["dog", ["frisbee"]]], WORDS, 2, 5)
    assert word.tolist() == [[14, -1], [10, 13]] and group.tolist() == [[0, 0], [0, 1]]


@pytest.mark.parametrize("mi, kw", [
    ([["cat"], []], {}), ([["<END>"], []], {}), ([["<NULL>"], []], {}), ([[("dog", "<START>")], []], {}),
    ([["dog"] * 17, []], {}), ([["dog", "dogs", "puppy", "frisbee", "grass"], []], dict(beam_size=11)),
    ([["dog"]], {}), ([["dog"], [], []], {}), ([["dog"], []], dict(num_groups=5)), (["dog", []], {}),
])
def test_must_include_refusals_name_it(mi, kw):
    from capgen.engine import must_include_slots
    args = dict(word_to_idx=WORDS, B=2, beam_size=5)
    args.update(kw)
    with pytest.raises(ValueError, match="must_include"):
        must_include_slots(mi, **args)


class _NoEngine:
    """stands in for MODEL.model: a call that reaches it means a check fired too late"""

    def __getattr__(self, name):
        raise AssertionError(f"the library was asked for {name}")


def test_beam_captions_refuses_bad_must_include_before_the_library():
    from capgen.ensemble import Ensemble
    from capgen.models import MODEL_init
    m = MODEL_init.__new__(MODEL_init)
    m.model, m.word_to_idx, m.end_idx = _NoEngine(), WORDS, 2
    m.config = type("Cfg", (), {"num_vocab": 1000})()
    feats = [None, None]
    with pytest.raises(ValueError, match="must_include.*unknown word 'cat'"):
        m.beam_captions(feats, None, beam_size=5, must_include=[["cat"], []])
    with pytest.raises(ValueError, match="must_include.*<END>"):
        m.beam_captions(feats, None, beam_size=5, must_include=[["<END>"], []])
    with pytest.raises(ValueError, match="must_include.*num_groups"):
        m.beam_captions(feats, None, beam_size=5, num_groups=5, must_include=[["dog"], []])
    with pytest.raises(ValueError, match="must_include.*one entry per image"):
        m.beam_captions(feats, None, beam_size=5, must_include=[["dog"]])
    with pytest.raises(ValueError, match="must_include.*too many words"):
        m.beam_captions(feats, None, beam_size=12, must_include=[["dog", "dogs", "puppy", "grass"], []])
    ens = Ensemble.__new__(Ensemble)
    ens.models, ens.leader = [m], m
    with pytest.raises(ValueError, match="must_include.*unknown word"):
        ens.beam_captions(feats, None, beam_size=5, must_include=[["cat"], []])
