"""Weight decay, the averaged weights and checkpoints without a device: the float64 restatement the GPU
tests use against torch's own AdamW + AveragedModel, the ema_warmup schedule, train()'s use of the new
arguments on a recording stand-in model, the C ABI's new symbols, and the checkpoint dict's round trip
through torch.save / torch.load(weights_only=True)."""
import contextlib
import os
import re
import types

import numpy as np
import pytest
import torch
from torch.optim.swa_utils import AveragedModel, get_ema_multi_avg_fn

from capgen import schedule
from optim_ref import adamw_ema_ref, f32
from test_gpu_rowops import B1, B2, EPS, LR, adam_inputs

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WD, D = f32(0.1), f32(0.9)

NEW_SYMBOLS = ["capgen_set_weight_decay", "capgen_set_ema", "capgen_ema_info", "capgen_get_ema",
               "capgen_set_ema_state", "capgen_ema_swap", "capgen_debug_adam_ex", "capgen_debug_arena_swap"]


def test_restatement_matches_torch_adamw_and_averaged_model():
    """anchors the reference of the GPU tests: three float64 steps of torch.optim.AdamW and
    AveragedModel(multi_avg_fn=get_ema_multi_avg_fn(d)) -- whose first update copies the parameters, the
    state the engine's off -> on leaves -- against optim_ref.  As test_adam_restatement_matches_torch:
    <= 1e-14."""
    p, grads = adam_inputs(64, 5)
    lin = torch.nn.Linear(64, 1, bias=False).double()
    with torch.no_grad():
        lin.weight.copy_(p.double().view(1, 64))
    opt = torch.optim.AdamW(lin.parameters(), lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD)
    avg = AveragedModel(lin, multi_avg_fn=get_ema_multi_avg_fn(D))
    avg.update_parameters(lin)  # the first update: a copy
    ref = adamw_ema_ref(p.double(), [g.double() for g in grads], LR, B1, B2, EPS, wd=WD, d=D)
    for t in range(3):
        lin.weight.grad = grads[t].double().view(1, 64).clone()
        opt.step()
        avg.update_parameters(lin)
        dp = (lin.weight.detach().view(-1) - ref[t][0]).abs().max().item()
        de = (avg.module.weight.detach().view(-1) - ref[t][3]).abs().max().item()
        print(f"step {t + 1}: parameters differ by {dp:.3e}, the average by {de:.3e}")
        assert dp <= 1e-14 and de <= 1e-14
    # both options do something at this size: far above the comparison's 1e-14
    plain = adamw_ema_ref(p.double(), [g.double() for g in grads], LR, B1, B2, EPS, d=D)
    assert (plain[2][0] - ref[2][0]).abs().max().item() > 1e-5
    assert (ref[2][3] - ref[2][0]).abs().max().item() > 1e-5


def test_restatement_without_options_is_adam_ref():
    from test_gpu_rowops import adam_ref
    p, grads = adam_inputs(64, 6)
    a = adam_ref(p.double(), [g.double() for g in grads])
    b = adamw_ema_ref(p.double(), [g.double() for g in grads], LR, B1, B2, EPS)
    for t in range(3):
        for x, y in zip(a[t], b[t][:3]):
            assert torch.equal(x, y)
        assert b[t][3] is None


def test_ema_warmup_values():
    w = schedule.ema_warmup(0.999)
    assert w(0) == pytest.approx(0.1, rel=1e-15)
    assert w(1) == pytest.approx(2 / 11, rel=1e-15)
    assert w(90) == pytest.approx(0.91, rel=1e-15)
    assert w(8990) == pytest.approx(8991 / 9000, rel=1e-15)      # 0.99900: the two branches meet at t = 8990
    assert w(8991) == 0.999 and w(10 ** 7) == 0.999
    assert all(w(t) <= w(t + 1) for t in range(0, 10000, 7))
    assert schedule.ema_warmup(0.5)(0) == pytest.approx(0.1) and schedule.ema_warmup(0.05)(0) == 0.05
    for bad in (0.0, 1.0, -0.1, 1.5):
        with pytest.raises(ValueError):
            schedule.ema_warmup(bad)


class StubEngine:
    def __init__(self, ema_updates=0):
        self.calls, self.n = [], ema_updates

    def set_weight_decay(self, wd):
        self.calls.append(("set_weight_decay", wd))

    def set_ema(self, d):
        self.calls.append(("set_ema", d))

    def ema_info(self):
        self.calls.append(("ema_info", None))
        return 0.5, self.n, False


def test_scheduled_steps_sets_decay_once_and_a_callable_ema_each_step():
    eng = StubEngine()
    s = schedule.ScheduledSteps(eng, weight_decay=0.01, ema_decay=0.99)
    s.before_step()
    s.before_step()
    assert eng.calls == [("set_weight_decay", 0.01), ("set_ema", 0.99)]
    eng = StubEngine(ema_updates=4)   # a resumed average: the schedule continues at its count
    w = schedule.ema_warmup(0.999)
    s = schedule.ScheduledSteps(eng, ema_decay=w)
    assert eng.calls == []
    for _ in range(3):
        s.before_step()
    assert eng.calls == [("ema_info", None), ("set_ema", w(4)), ("set_ema", w(5)), ("set_ema", w(6))]
    eng = StubEngine()
    schedule.ScheduledSteps(eng).before_step()
    assert eng.calls == []


class Rec:
    """a recording stand-in for a trainer (as test_train_loop_cadence_matches_main_py's)"""

    def __init__(self):
        self.calls, self.inside = [], False

    def _log(self, *c):
        self.calls.append(c + (self.inside,))

    def set_schedule(self, **k):
        self._log("set_schedule", tuple(sorted(k.items())))

    def train_step_resident(self, store, idx, caps):
        self._log("step", int(idx.shape[0]))

    def compute_loss(self, object_features, position_features, target_caption):
        self._log("loss", int(object_features.shape[0]))
        return {"loss": torch.tensor(float(target_caption.shape[0]))}

    def generate_caption(self, object_features, position_features, beam_size=None):
        self._log("gen", int(object_features.shape[0]))
        return [f"c{k}" for k in range(object_features.shape[0])], None

    def decode_captions(self, ids):
        return [str(r) for r in ids.tolist()]

    @contextlib.contextmanager
    def averaged(self):
        self._log("enter")
        self.inside = True
        try:
            yield self
        finally:
            self.inside = False
            self._log("exit")

    def _touch(self, kind, path):
        open(path, "wb").close()
        self._log(kind, os.path.basename(path))

    def save(self, path):
        self._touch("save", path)

    def save_checkpoint(self, path):
        self._touch("save_checkpoint", path)

    def load_checkpoint(self, path):
        self._log("load_checkpoint", os.path.basename(path))


def _split(n_img, n_cap, seed):
    r = np.random.default_rng(seed)
    return {"features": r.random((n_img, 3, 8), dtype=np.float32),
            "positions": r.random((n_img, 3, 5), dtype=np.float32),
            "captions": r.integers(1, 9, (n_cap, 6)).astype(np.int32),
            "image_idxs": r.integers(0, n_img, n_cap).astype(np.int32)}


def _train(tmp, **kw):
    from capgen.train import train
    m = Rec()
    train(m, _split(5, 23, 0), _split(4, 9, 1), num_epoch=2, batch_size=4, output_path=str(tmp), eval_every=2,
          sample_every=5, log=lambda *_: None, device="cpu", feature_dtype=torch.float32, **kw)
    return m


def test_train_defaults_change_nothing(tmp_path):
    """the new arguments at their defaults: the same calls in the same order as without them, and no
    file beyond model_{epoch}.pt"""
    a = _train(tmp_path / "a")
    b = _train(tmp_path / "b", weight_decay=None, ema_decay=None, eval_averaged=False, resume=None)
    assert a.calls == b.calls and len(a.calls) > 20
    assert not any(c[0] in ("set_schedule", "enter", "save_checkpoint", "load_checkpoint") for c in a.calls)
    assert sorted(os.listdir(tmp_path / "b" / "model")) == ["model_1.pt", "model_2.pt"]
    # grad_clip / lr_schedule alone are forwarded exactly as before
    c = _train(tmp_path / "c", grad_clip=1.0)
    assert c.calls[0] == ("set_schedule", (("grad_clip", 1.0), ("lr_schedule", None)), False)
    assert sorted(os.listdir(tmp_path / "c" / "model")) == ["model_1.pt", "model_2.pt"]


def test_train_eval_averaged(tmp_path):
    m = _train(tmp_path, weight_decay=0.01, ema_decay=0.99, eval_averaged=True, resume="checkpoint_7.pt")
    assert m.calls[0] == ("set_schedule", (("ema_decay", 0.99), ("grad_clip", None), ("lr_schedule", None),
                                           ("weight_decay", 0.01)), False)
    assert m.calls[1] == ("load_checkpoint", "checkpoint_7.pt", False)
    assert all(not c[-1] for c in m.calls if c[0] == "step"), "a train step ran on the averaged weights"
    for epoch in (1, 2):
        lo = m.calls.index(("enter", False)) if epoch == 1 else \
            m.calls.index(("enter", False), m.calls.index(("exit", False)) + 1)
        hi = m.calls.index(("exit", False), lo)
        block = m.calls[lo + 1:hi]
        # the epoch's evaluation: 3 zipped batches of 2 losses and one generation each, then the averaged save
        assert [c[0] for c in block] == ["loss", "loss", "gen"] * 3 + ["save"]
        assert all(c[-1] for c in block)
        assert block[-1][1] == f"model_{epoch}.ema.pt"
        after = m.calls[hi + 1:hi + 3]
        assert after == [("save", f"model_{epoch}.pt", False), ("save_checkpoint", f"checkpoint_{epoch}.pt", False)]
    # the cadence losses / samples between steps run on the raw weights
    assert any(c[0] == "loss" and not c[-1] for c in m.calls) and any(c[0] == "gen" and not c[-1] for c in m.calls)
    assert sorted(os.listdir(tmp_path / "model")) == ["checkpoint_1.pt", "checkpoint_2.pt", "model_1.ema.pt",
                                                      "model_1.pt", "model_2.ema.pt", "model_2.pt"]


def test_train_swaps_back_when_the_evaluation_raises(tmp_path):
    from capgen.train import train

    class Boom(Rec):
        def generate_caption(self, **k):
            raise KeyError("boom")

    m = Boom()
    with pytest.raises(KeyError):
        train(m, _split(5, 23, 0), _split(4, 9, 1), num_epoch=1, batch_size=4, output_path=str(tmp_path),
              eval_every=100, sample_every=100, log=lambda *_: None, device="cpu", feature_dtype=torch.float32,
              ema_decay=0.9, eval_averaged=True)
    assert m.calls[-1] == ("exit", False) and not m.inside


def test_eval_averaged_without_an_average_fails_before_the_first_step(tmp_path):
    from capgen.train import train

    class WithEngine(Rec):
        def __init__(self, decay):
            super().__init__()
            self.model = types.SimpleNamespace(engine=types.SimpleNamespace(ema_info=lambda: (decay, 0, False)))

    def run(m, **kw):
        train(m, _split(5, 23, 0), _split(4, 9, 1), num_epoch=1, batch_size=4, output_path=str(tmp_path),
              eval_every=100, sample_every=100, log=lambda *_: None, device="cpu", feature_dtype=torch.float32,
              eval_averaged=True, **kw)

    m = WithEngine(0.0)
    with pytest.raises(ValueError, match="eval_averaged"):
        run(m)
    assert not any(c[0] == "step" for c in m.calls)
    with pytest.raises(ValueError, match="eval_averaged"):      # a checkpoint without an average
        run(WithEngine(0.0), resume="checkpoint_3.pt")
    ok = WithEngine(D)                                           # one restored from a checkpoint will do
    run(ok, resume="checkpoint_3.pt")
    assert any(c[0] == "enter" for c in ok.calls)
    run(WithEngine(0.0), ema_decay=0.9)                          # (the trainer enables it)


def test_ema_decay_is_checked_as_the_f32_the_engine_stores():
    from capgen.engine import check_ema_decay
    assert check_ema_decay(None) == 0.0 and check_ema_decay(0) == 0.0
    assert check_ema_decay(0.9) == D and check_ema_decay(np.float32(0.999)) == f32(0.999)
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf"), 0.99999999, -1e-50 - 1.0):
        with pytest.raises(ValueError, match="decay"):
            check_ema_decay(bad)


def test_new_symbols_declared_and_bound():
    from capgen import _lib
    header = open(os.path.join(REPO, "include", "capgen.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint " + name + r"\(", header), f"{name} is not declared in include/capgen.h"
        assert name in _lib.EXPORTED, f"{name} is not bound in capgen/_lib.py"
        assert getattr(lib, name).argtypes == _lib._SIGS[name][1]
    assert re.search(r"#define\s+CAPGEN_ABI_VERSION\s+%d\b" % _lib.ABI_VERSION, header)
    for meth in ("set_weight_decay", "set_ema", "ema_info", "ema_arena", "ema_state_dict", "set_ema_arena",
                 "swap_ema", "averaged"):
        from capgen.engine import Engine
        assert callable(getattr(Engine, meth))


def test_checkpoint_dict_round_trips_with_weights_only(tmp_path, monkeypatch):
    """MODEL_init.save_checkpoint's dict, built from a stand-in engine: torch.load(weights_only=True)
    accepts it and returns what went in"""
    from capgen.models import CHECKPOINT_FORMAT, MODEL_init, checkpoint_dict
    n = 24
    r = np.random.default_rng(3)
    arenas = {k: r.standard_normal(n).astype(np.float32) for k in ("p", "m", "v", "e")}

    class Eng:
        device = torch.device("cpu")
        arena_elems, lr, grad_clip, weight_decay = n, f32(3e-4), 1.5, f32(0.01)

        def adam_step_count(self):
            return 17

        def adam_arenas(self, m, v):
            m[:], v[:] = arenas["m"], arenas["v"]
            return 17

        def ema_info(self):
            return D, 12, False

        def ema_arena(self):
            return arenas["e"].copy()

        def state_dict(self):
            return {"encoder.w": torch.from_numpy(arenas["p"][:16].reshape(4, 4).copy()),
                    "decoder.b": torch.from_numpy(arenas["p"][16:].copy())}

        def dp_comm_info(self):
            return 0, 0

    monkeypatch.setattr(torch.cuda, "current_stream",
                        lambda dev=None: types.SimpleNamespace(synchronize=lambda: None))
    ck = checkpoint_dict(Eng())
    t = MODEL_init.__new__(MODEL_init)
    t.model = types.SimpleNamespace(engine=Eng())
    t.save_checkpoint(str(tmp_path / "ck.pt"))
    back = torch.load(str(tmp_path / "ck.pt"), map_location="cpu", weights_only=True)
    assert set(back) == {"format", "model", "adam", "ema", "lr", "grad_clip", "weight_decay"}
    assert back["format"] == CHECKPOINT_FORMAT and back["lr"] == f32(3e-4) and back["grad_clip"] == 1.5
    assert back["weight_decay"] == f32(0.01) and back["adam"]["step"] == 17
    assert back["ema"]["decay"] == D and back["ema"]["n_updates"] == 12
    assert np.array_equal(back["ema"]["params"].numpy(), arenas["e"])
    assert np.array_equal(back["adam"]["exp_avg"].numpy(), arenas["m"])
    assert np.array_equal(back["adam"]["exp_avg_sq"].numpy(), arenas["v"])
    for k in ck["model"]:
        assert torch.equal(back["model"][k], ck["model"][k])
    # the model entry alone is what save() writes: reference-keyed tensors
    assert all(isinstance(v, torch.Tensor) for v in back["model"].values())
