"""Host-side text helpers of the boundary (core/utils.py:67-103)."""
from __future__ import annotations

import io
import json
import pickle

import numpy as np


def decode_captions(captions, index_to_word):
    """ids -> sentences: skip <START> at t=0, <END> -> '.' and stop, drop <NULL>
    (core/utils.py:67-103; its 'a'->'an' branch can never fire and is omitted)."""
    captions = np.asarray(captions)
    rows = captions[None] if captions.ndim == 1 else captions
    out = []
    for row in rows:
        words = []
        for t, idx in enumerate(row):
            w = index_to_word[int(idx)]
            if w == "<START>" and t == 0:
                continue
            if w == "<END>":
                words.append(".")
                break
            if w != "<NULL>":
                words.append(w)
        out.append(" ".join(words))
    return out


def sequence_logprob(ids, logp, end_id):
    """Log-probability of each sampled caption: the sum of its token log-probabilities up to and
    including the first <END> (all of them when there is none).  ids [..., T] are the sampled tokens
    aligned with logp [..., T] (Engine.sample's ids[..., 1:T+1] and logp); returns [...]."""
    import torch

    ids, logp = torch.as_tensor(ids), torch.as_tensor(logp)
    if ids.shape != logp.shape:
        raise ValueError("capgen: sequence_logprob needs ids and logp of one shape")
    ended = (ids == end_id).to(torch.int64).cumsum(-1)
    keep = (ended - (ids == end_id).to(torch.int64)) == 0  # no <END> strictly before this position
    return torch.where(keep, logp, torch.zeros_like(logp)).sum(-1)


def rollout_captions(ids, end_id, pad_id):
    """Decoded ids -> teacher-forcing captions for Engine.train_step_weighted.  ids [..., max_length+1]
    are Engine.sample's / Engine.greedy's; returns int32 [..., max_length]: <START>, the drawn tokens
    through the first <END> inclusive, pad_id at every position strictly after it.  end_id=None cuts
    nothing.  A drawn <NULL> (= pad_id) before <END> stays where it is: as a target it is masked like
    any pad, as in the reference.  Pure torch: works on CPU and device tensors."""
    import torch

    ids = torch.as_tensor(ids)
    caps = ids[..., :-1].to(torch.int32)
    if end_id is None:
        return caps.contiguous()
    is_end = (caps == end_id).to(torch.int64)
    is_end[..., 0] = 0  # position 0 is <START>, not a drawn token
    after = (is_end.cumsum(-1) - is_end) > 0  # an <END> strictly before this position
    return torch.where(after, torch.full_like(caps, pad_id), caps).contiguous()


def leave_one_out_baseline(rewards):
    """Baseline of the n-sample self-critical estimator: rewards [n, B] -> [n, B], entry (j, b) the
    mean of the OTHER samples of row b, (sum_k r[k, b] - r[j, b]) / (n - 1).  The advantages
    r - baseline of each row then sum to zero.  numpy, float64."""
    r = np.asarray(rewards, dtype=np.float64)
    if r.ndim != 2 or r.shape[0] < 2:
        raise ValueError("capgen: the leave-one-out baseline needs rewards [n, B] with n >= 2")
    return (r.sum(0, keepdims=True) - r) / (r.shape[0] - 1)


class _VocabUnpickler(pickle.Unpickler):
    """word_index.pkl holds a plain {str: int} dict; refuse anything that is not data."""

    def find_class(self, module, name):
        raise pickle.UnpicklingError(f"capgen: refusing to load {module}.{name} from a vocabulary file")


def load_word_to_idx(path):
    """Vocabulary file of core/models.py:22 ({word: index}); JSON or a data-only pickle."""
    with open(path, "rb") as f:
        raw = f.read()
    if path.endswith(".json"):
        return {str(k): int(v) for k, v in json.loads(raw.decode()).items()}
    d = _VocabUnpickler(io.BytesIO(raw)).load()
    if not isinstance(d, dict):
        raise ValueError("capgen: vocabulary file must hold a dict")
    return {str(k): int(v) for k, v in d.items()}
