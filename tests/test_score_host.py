"""Scoring given captions, host side: the exports, the float64 restatement (tests/score_ref.py) against
torch's own cross entropy and argmax, and MODEL.score_captions' argument checks (no device)."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from score_ref import score_ref, score_rows_ref

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["capgen_score_captions", "capgen_debug_score_rows", "capgen_debug_score_finish"]


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


@pytest.mark.parametrize("V", [8, 1001])
def test_score_ref_is_torch_cross_entropy_and_argmax(V):
    g = torch.Generator().manual_seed(V)
    R, Lq, pad = 5, 7, 0
    x = 3 * torch.randn(R * Lq, V, generator=g, dtype=torch.float64)
    tgt = torch.randint(1, V, (R * Lq,), generator=g)
    tgt[3] = pad               # a pad in the middle of caption 0
    tgt[2 * Lq:3 * Lq] = pad   # caption 2: pads only
    am = x.argmax(1)
    tgt[Lq:Lq + 3] = am[Lq:Lq + 3]  # three sure hits in caption 1
    ref = score_ref(x, tgt, pad, Lq)
    ce = F.cross_entropy(x, tgt, reduction="none", ignore_index=pad)
    assert torch.allclose(ref["token_logp"].reshape(-1), -ce, atol=1e-12, rtol=0)
    assert torch.equal(ref["hit"].reshape(-1), ((am == tgt) & (tgt != pad)).long())
    assert torch.allclose(ref["logp"], -ce.view(R, Lq).sum(1), atol=1e-11, rtol=0)
    assert ref["length"].tolist() == [(tgt.view(R, Lq)[r] != pad).sum().item() for r in range(R)]
    assert ref["hits"][1] >= 3 and ref["logp"][2] == 0 and ref["length"][2] == 0 and ref["hits"][2] == 0
    assert ref["token_logp"][0, 3] == 0 and (ref["token_logp"][ref["kept"]] < 0).all()


def test_score_ref_counts_ties_and_not_the_second_largest():
    x = torch.zeros(3, 6, dtype=torch.float32)
    x[0, 2] = x[0, 4] = 1.5                                  # the target ties the maximum: a hit
    x[1, 2] = 1.5
    x[1, 4] = float(np.nextafter(np.float32(1.5), np.float32(2)))  # one f32 ulp above the target: no hit
    x[2, 1] = 9.0                                            # a pad row whose argmax is the pad id
    rows = score_rows_ref(x, torch.tensor([2, 2, 1]), pad=1)
    assert rows["hit"].tolist() == [1, 0, 0]
    assert rows["kept"].tolist() == [True, True, False] and rows["token_logp"][2] == 0
    assert rows["margin"][0] == 0 and 0 < rows["margin"][1] < 2e-7


def _model(max_length=10):
    from capgen import preset
    from capgen.models import MODEL_init
    m = MODEL_init(word_to_idx={"<NULL>": 0, "<START>": 1, "<END>": 2})
    m.config = preset("C1").replace(max_length=max_length)
    return m  # no network: every check below must fire before the engine is asked for


def test_model_score_captions_argument_checks():
    m = _model()
    f, p = torch.zeros(4, 8, 512), torch.zeros(4, 8, 84)
    ok = torch.ones(4, 10, dtype=torch.int64)
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        m.score_captions(f, p, ok[0])                       # rank 1
    with pytest.raises(ValueError, match=r"\[B, T\]"):
        m.score_captions(f, p, ok.view(1, 1, 4, 10))        # rank 4
    with pytest.raises(ValueError, match="batch"):
        m.score_captions(f, p, ok[:3])                      # [3, T] against 4 images
    with pytest.raises(ValueError, match="batch"):
        m.score_captions(f, p, ok.view(4, 1, 10).numpy())   # [n = 4, B = 1, T] against 4 images
    with pytest.raises(ValueError, match="batch"):
        m.score_captions(f, p[:2], ok)
    with pytest.raises(ValueError, match="max_length"):
        m.score_captions(f, p, torch.ones(4, 11, dtype=torch.int64))
    with pytest.raises(ValueError, match="max_length"):
        m.score_captions(f, p, torch.ones(2, 4, 1, dtype=torch.int64))  # T < 2
    with pytest.raises(ValueError, match="object_features"):
        m.score_captions(f[0], p, ok)
    with pytest.raises(AttributeError):  # (a well-formed call gets as far as the missing network)
        m.score_captions(f, p, ok)
