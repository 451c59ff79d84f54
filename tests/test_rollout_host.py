"""Roll-out self-critical training, host side: the exports, capgen.utils.rollout_captions against a
per-row Python loop, and the leave-one-out baseline's arithmetic.  All inputs are fixed."""
import os
import re

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["capgen_train_step_weighted", "capgen_debug_cross_entropy_rows_weighted", "capgen_debug_ce_finish_weighted"]


def test_exports():
    from capgen import _lib
    header = open(os.path.join(REPO, "include", "capgen.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in _lib.EXPORTED, name
        assert re.search(r"\b%s\s*\(" % name, header), name
    assert _lib.ABI_VERSION == 13  # the additions are backward compatible


START, END, NULL = 1, 2, 0
# [3, 4, 9]: <START>, 7 drawn tokens, the trailing 0 column of Engine.sample / Engine.greedy
IDS = torch.tensor([
    [[1, 5, 6, 7, 8, 9, 4, 3, 0],     # no <END>
     [1, 2, 6, 7, 8, 9, 4, 3, 0],     # <END> in the first drawn position
     [1, 5, 6, 7, 8, 9, 4, 2, 0],     # <END> in the last position
     [1, 5, 2, 7, 2, 9, 4, 3, 0]],    # two <END>s: the first one ends the caption
    [[1, 5, 0, 7, 2, 9, 4, 3, 0],     # a drawn <NULL> before <END> stays
     [1, 2, 2, 2, 2, 2, 2, 2, 0],
     [1, 5, 6, 2, 0, 0, 9, 9, 0],
     [1, 0, 0, 0, 0, 0, 0, 0, 0]],
    [[1, 9, 9, 9, 9, 9, 9, 9, 0],
     [1, 3, 4, 5, 6, 2, 7, 8, 0],
     [1, 1, 5, 2, 6, 7, 8, 9, 0],     # a drawn <START> is an ordinary token
     [1, 5, 6, 7, 8, 9, 2, 2, 0]],
], dtype=torch.int64)


def loop_ref(ids, end_id, pad_id):
    out = np.empty(ids.shape[:-1] + (ids.shape[-1] - 1,), dtype=np.int32)
    for idx in np.ndindex(*ids.shape[:-1]):
        row, ended = ids[idx], False
        for t in range(ids.shape[-1] - 1):
            out[idx + (t,)] = pad_id if ended else row[t]
            if t >= 1 and row[t] == end_id:
                ended = True
    return out


@pytest.mark.parametrize("pad_id", [NULL, 11])
def test_rollout_captions_matches_the_loop(pad_id):
    from capgen.utils import rollout_captions
    got = rollout_captions(IDS, END, pad_id)
    assert got.dtype == torch.int32 and got.shape == (3, 4, 8) and got.is_contiguous()
    np.testing.assert_array_equal(got.numpy(), loop_ref(IDS.numpy(), END, pad_id))
    # the cases by hand
    assert got[0, 0].tolist() == [1, 5, 6, 7, 8, 9, 4, 3]
    assert got[0, 1].tolist() == [1, 2] + [pad_id] * 6
    assert got[0, 2].tolist() == [1, 5, 6, 7, 8, 9, 4, 2]
    assert got[0, 3].tolist() == [1, 5, 2] + [pad_id] * 5
    assert got[1, 0].tolist() == [1, 5, 0, 7, 2] + [pad_id] * 3
    # a [B, T+1] tensor (Engine.greedy), and the input is left alone
    before = IDS.clone()
    assert torch.equal(rollout_captions(IDS[1], END, pad_id), got[1])
    assert torch.equal(IDS, before)


def test_rollout_captions_without_end_cuts_nothing():
    from capgen.utils import rollout_captions
    got = rollout_captions(IDS, None, NULL)
    assert got.dtype == torch.int32 and got.shape == (3, 4, 8)
    assert torch.equal(got, IDS[..., :-1].to(torch.int32))
    # an int32 input is not modified either
    ids32 = IDS.to(torch.int32)
    rollout_captions(ids32, END, 11)
    assert torch.equal(ids32, IDS.to(torch.int32))


R = np.array([[0.50, 1.00, 0.00],
              [0.25, 1.00, 0.75],
              [1.00, 1.00, 0.25],
              [0.25, 0.00, 1.00]])  # [n = 4, B = 3]


def test_leave_one_out_baseline():
    from capgen.utils import leave_one_out_baseline
    base = leave_one_out_baseline(R)
    assert base.shape == R.shape and base.dtype == np.float64
    for j in range(4):
        for b in range(3):
            others = [R[k, b] for k in range(4) if k != j]
            assert base[j, b] == pytest.approx(sum(others) / 3, abs=1e-15)
    adv = R - base
    np.testing.assert_allclose(adv.sum(0), 0.0, atol=1e-15)  # each row's advantages sum to zero
    np.testing.assert_allclose(adv[:, 1], [1 / 3, 1 / 3, 1 / 3, -1.0], atol=1e-15)  # rewards 1, 1, 1, 0
    with pytest.raises(ValueError):
        leave_one_out_baseline(R[:1])


def test_rollout_self_critic_rejects_mean_baseline_of_one_sample():
    from capgen.models import RolloutSelfCritic
    w2i = {"<NULL>": 0, "<START>": 1, "<END>": 2}
    with pytest.raises(ValueError):
        RolloutSelfCritic(word_to_idx=w2i, n_samples=1, baseline="mean")
    with pytest.raises(ValueError):
        RolloutSelfCritic(word_to_idx=w2i, baseline="median")
