"""The END-aware n-best beam search without a device: the float64 restatement (tests/beam_ref.py) against
the oracle's reference beam, the conditions on the fixtures that the GPU comparison
(tests/test_gpu_beam_nbest.py) relies on, and the Python layer's argument checking."""
import functools

import numpy as np
import pytest
import torch

import beam_ref as R
from capgen.params import fixture_state_dict
from golden_util import fixture_inputs, load_fixture
from oracle import capgen_oracle as O

C1_END, C2S_END = 887, 840  # the ids that play <END> on the fixtures (chosen for the conditions pinned below)


@functools.lru_cache(maxsize=None)
def ref_search(tag, k, end_id):
    """(cfg, the restatement's state) of fixture `tag`; computed once and shared (read only)"""
    cfg, seed, z = load_fixture(tag)
    sd = fixture_state_dict(cfg, seed=seed, with_buffer=False)
    P = O.make_params(sd, requires_grad=False, dtype=torch.float64)
    f, p, _ = fixture_inputs(z)
    return cfg, R.search(P, cfg, f, p, k, end_id)


def test_without_end_the_best_row_is_the_reference_beam():
    """end_id = -1, alpha = 0: nothing finishes and the best hypothesis is oracle.beam(log_softmax=True)'s"""
    cfg, seed, z = load_fixture("c1")
    P = O.make_params(fixture_state_dict(cfg, seed=seed, with_buffer=False), requires_grad=False)
    f, p, _ = fixture_inputs(z)
    want = O.beam(P, cfg, f, p, 3, log_softmax=True).numpy()
    _, st = ref_search("c1", 3, -1)
    assert not st["fin"].any() and (st["len"] == cfg.max_length - 1).all() and not st["mixed"].any()
    got = R.nbest(st, 0.0, 1)
    assert np.array_equal(got["ids"][0], want)
    # logp is the only order at alpha 0, and the search already keeps the hypotheses in it
    assert np.array_equal(R.finish(st["logp"], st["len"], 0.0, 3)["order"], np.arange(3)[:, None].repeat(8, 1))


def test_c1_conditions_of_the_gpu_comparison():
    cfg, s3 = ref_search("c1", 3, C1_END)
    _, s5 = ref_search("c1", 5, C1_END)
    T = cfg.max_length
    assert int(s3["fin"].sum()) == 10 and s3["fin"].size == 24
    assert int(s5["fin"].sum()) == 15 and s5["fin"].size == 40
    assert set(s3["len"][s3["fin"] == 1].tolist()) == {1, 2, 4, 5, 9}
    assert set(s5["len"][s5["fin"] == 1].tolist()) - set(s3["len"][s3["fin"] == 1].tolist()) == {3}
    assert (s3["len"][s3["fin"] == 0] == T - 1).all() and (s5["len"][s5["fin"] == 0] == T - 1).all()
    assert int(s3["mixed"].sum()) == 5 and int(s5["mixed"].sum()) == 5
    b0, b1 = R.nbest(s3, 0.0, 1)["ids"][0], R.nbest(s3, 1.0, 1)["ids"][0]
    assert int((b0 != b1).any(axis=1).sum()) == 2
    for st, k, alpha, smallest in ((s3, 3, 0.0, 2.06e-3), (s3, 3, 1.0, 1.01e-3), (s5, 5, 0.0, 2.06e-3),
                                   (s5, 5, 0.7, 2.06e-3)):
        nb = R.nbest(st, alpha, k)
        R.structure_ok(nb["ids"], nb["len"], C1_END, T)
        assert (nb["margin"] >= 1e-3).all(), (k, alpha, nb["margin"])
        assert abs(nb["margin"].min() - smallest) < 1e-5, (k, alpha, nb["margin"].min())
        assert (np.diff(nb["score"], axis=0) <= 0).all()


def test_c2s_conditions_of_the_gpu_comparison():
    cfg, st = ref_search("c2s", 3, C2S_END)
    assert st["fin"].all() and set(st["len"].reshape(-1).tolist()) == {1, 2}
    nb = R.nbest(st, 0.0, 3)
    R.structure_ok(nb["ids"], nb["len"], C2S_END, cfg.max_length)
    assert abs(nb["margin"].min() - 0.033) < 5e-4, nb["margin"]


def test_step_finished_rows_offer_one_candidate_and_keep_beam_order():
    """two finished rows with equal logp keep beam order; a finished row's scores are never read"""
    g = np.random.default_rng(5)
    ls = R.log_softmax64(3 * g.standard_normal((3, 1, 40)))
    ls[0], ls[2] = np.nan, np.nan
    logp = np.array([[-0.5], [-9.0], [-0.5]])
    st = R.step(ls, logp, np.array([[1], [0], [1]]), np.array([[2], [4], [3]]), 3, end_id=7)
    assert st["src"][:, 0].tolist() == [0, 2, 1] and st["tok"][:2, 0].tolist() == [0, 0]
    assert st["len"][:, 0].tolist() == [2, 3, 5] and st["fin"][:2, 0].tolist() == [1, 1]
    assert st["logp"][0, 0] == -0.5 and st["logp"][1, 0] == -0.5 and st["gaps"][0, 0] == 0.0


def test_finish_orders_by_score_then_beam():
    logp = np.array([[-4.0], [-2.0], [-4.0], [-6.0]])
    length = np.array([[2], [1], [2], [0]])
    f = R.finish(logp, length, 1.0, 4)  # scores -2, -2, -2, -6: the tie resolves by beam index
    assert f["order"][:, 0].tolist() == [0, 1, 2, 3] and f["final_margin"][0] == 0.0
    assert f["score"][:, 0].tolist() == [-2.0, -2.0, -2.0, -6.0]  # (len 0 divides by 1)
    f = R.finish(logp, length, 0.0, 2)
    assert f["order"][:, 0].tolist() == [1, 0] and f["score"][:, 0].tolist() == [-2.0, -4.0]


def test_exports():
    from capgen import _lib
    for name in ("capgen_beam_nbest", "capgen_debug_beam_step_ended", "capgen_debug_beam_finish"):
        assert name in _lib.EXPORTED
    assert _lib.ABI_VERSION == 13


@pytest.mark.parametrize("kw, word", [
    (dict(beam_size=0), "beam_size"), (dict(beam_size=17), "beam_size"), (dict(beam_size=4, num_vocab=3), "beam_size"),
    (dict(beam_size=2.0), "beam_size"), (dict(n_best=0), "n_best"), (dict(n_best=4), "n_best"),
    (dict(end_id=-2), "end_id"), (dict(end_id=1000), "end_id"), (dict(end_id=None), "end_id"),
    (dict(length_penalty=-0.1), "length_penalty"), (dict(length_penalty=float("nan")), "length_penalty"),
    (dict(length_penalty=float("inf")), "length_penalty"),
])
def test_python_argument_checks_name_the_argument(kw, word):
    from capgen.engine import check_beam_nbest_args
    args = dict(beam_size=3, end_id=5, length_penalty=0.0, n_best=1, num_vocab=1000)
    assert check_beam_nbest_args(**args) == (3, 1)
    assert check_beam_nbest_args(**dict(args, end_id=-1, n_best=3, length_penalty=1)) == (3, 3)
    args.update(kw)
    with pytest.raises((ValueError, TypeError), match=word):
        check_beam_nbest_args(**args)
