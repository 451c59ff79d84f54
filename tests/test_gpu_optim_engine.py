"""Weight decay, the averaged weights, the swap and checkpoints at engine level, on the GPU: fp32 on the
c1 / c2s fixtures with dropout off unless a case says otherwise.

The step restatement takes everything from the engine's own state: parameters, Adam state and average
before a step, the gradient arena after it (single process: the gradients are whole; the clip scale is
applied inside the kernel, so the arena holds the unclipped gradients) and, with clipping on, the
coefficient from grad_norm().  One restated float64 update (tests/optim_ref.py) must then give the
engine's new parameters and average within the kernel tests' bounds (tests/test_gpu_optim_kernels.py)."""
import ctypes as C

import numpy as np
import pytest
import torch

from capgen.params import fixture_state_dict
from golden_util import load_fixture
from optim_ref import adamw_ema_step, f32
from test_gpu_gradclip import _adam_arenas, _probe_norm, coef_formula
from test_gpu_hazard import _engine as _bf16_engine
from test_gpu_hazard import _inputs as _bf16_inputs
from test_gpu_hazard import _logged_run
from test_gpu_parity import _engine, _inputs, _params_close, _sharded_update_check

pytestmark = pytest.mark.gpu

WD, D = f32(0.1), f32(0.9)
WD2, D2 = f32(0.3), f32(0.5)
OPTS = {"decay": (WD, None), "average": (None, D), "both": (WD, D)}


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def _p_bound(ref, lr, decay):
    m = np.abs(ref).max()
    return 1e-6 * m + 1e-6 * lr + (3 * 2.0 ** -24 * m if decay else 0.0)


def _e_bound(ref, lr):
    return 1e-6 * np.abs(ref).max() + 1e-6 * lr


def _restate(cfg, before, g, t, lr, wd, scale, d):
    """one float64 update from the f32 arrays before = (p, m, v, e or None): (p, e) as numpy float64"""
    p, m, v, e = (None if x is None else torch.from_numpy(x.astype(np.float64)) for x in before)
    rp, _, _, re_ = adamw_ema_step(p, torch.from_numpy(g.astype(np.float64)), m, v, t, lr, f32(cfg.beta1),
                                   f32(cfg.beta2), f32(cfg.eps), wd or 0.0, scale, e, d)
    return rp.numpy(), None if re_ is None else re_.numpy()


MODES = ["unfused", "step", "step_graph"]  # forward / backward / adam_step; the bucketed train_step, graph off / on
# every combination on c1 (1.3 M parameters, restated whole); on c2s (46.5 M, six blocks a side: more
# buckets) the full one -- clip, decay and average -- in each mode, restated on a sample of the arena
STEP_CASES = [("c1", m, cl, o) for m in MODES for cl in (False, True) for o in OPTS] + \
             [("c2s", m, True, "both") for m in MODES]


def _sample(n):
    """the elements a case restates (the update is elementwise): all of a small arena; of a large one
    every 13th -- every residue of the kernels' power-of-two strides -- and both ends"""
    if n <= 2_000_000:
        return slice(None)
    return np.unique(np.concatenate([np.arange(0, n, 13), np.arange(8192), np.arange(n - 8192, n)]))


@pytest.mark.parametrize("tag,mode,clip,opts", STEP_CASES)
def test_step_restated_from_engine_state(tag, mode, clip, opts):
    cfg, seed, z = load_fixture(tag)
    f, p, c = _inputs(z)
    e = _engine(cfg, seed)
    e.set_training(False)
    lr = f32(cfg.learning_rate)
    wd, d = OPTS[opts]
    max_norm = f32(0.25 * _probe_norm(e, f, p, c)) if clip else None
    if clip:
        e.set_grad_clip(max_norm)
    if wd:
        e.set_weight_decay(wd)
    if d:
        e.set_ema(d)
        assert e.ema_info() == (d, 0, False)
    e.set_graph(mode == "step_graph")
    sel = _sample(e.arena_elems)
    for t in range(1, 4):
        if mode == "step_graph" and t == 3:  # new values while on: read by the replay, nothing re-captured
            wd, d = (WD2 if wd else None), (D2 if d else None)
            if wd:
                e.set_weight_decay(wd)
            if d:
                e.set_ema(d)
        step, m0, v0 = _adam_arenas(e)
        assert step == t - 1
        before = (e.params_arena()[sel], m0[sel], v0[sel], e.ema_arena()[sel] if d else None)
        if mode == "unfused":
            e.forward(f, p, c)
            e.backward()
            e.adam_step()
        else:
            e.train_step(f, p, c)
        torch.cuda.synchronize()
        g = e.grads_arena()[sel]
        scale = 1.0
        if clip:
            norm = e.grad_norm()
            scale = coef_formula(norm, max_norm)
            assert norm > max_norm, "the clip must bite"
        rp, re_ = _restate(cfg, before, g, t, lr, wd, scale, d)
        got = e.params_arena()[sel].astype(np.float64)
        bound = _p_bound(rp, lr, wd)
        err = np.abs(got - rp).max()
        print(f"{tag} {mode} clip={clip} {opts} step {t}: parameter error {err:.3e} of bound {bound:.3e}")
        assert err <= bound, (t, err, bound)
        if wd:  # non-vacuity: the update without the decay is far outside
            other, _ = _restate(cfg, before, g, t, lr, None, scale, d)
            assert np.abs(got - other).max() > 10 * bound
        if d:
            got_e = e.ema_arena()[sel].astype(np.float64)
            ebound = _e_bound(re_, lr)
            eerr = np.abs(got_e - re_).max()
            print(f"{tag} {mode} clip={clip} {opts} step {t}: average error {eerr:.3e} of bound {ebound:.3e}")
            assert eerr <= ebound, (t, eerr, ebound)
            assert np.abs(got_e - before[3].astype(np.float64)).max() > 10 * ebound, "the average did not move"
            assert e.ema_info() == (d, t, False)
    assert _adam_arenas(e)[0] == 3


def test_enable_semantics():
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    e = _engine(cfg, seed)
    e.set_training(False)
    with pytest.raises(RuntimeError, match="never enabled"):
        e.ema_arena()
    e.train_step(f, p, c)
    assert e.ema_info() == (0.0, 0, False)
    e.set_ema(D)                                     # off -> on: a copy, the counter at 0
    assert _same_bits(e.ema_arena(), e.params_arena()) and e.ema_info() == (D, 0, False)
    e.train_step(f, p, c)
    e.train_step(f, p, c)
    avg = e.ema_arena()
    assert not _same_bits(avg, e.params_arena()) and e.ema_info()[1] == 2
    e.set_ema(D2)                                    # on -> on: only the decay
    assert _same_bits(e.ema_arena(), avg) and e.ema_info() == (D2, 2, False)
    w = e.params_arena()
    e.set_params_arena(w * np.float32(0.5))          # set_params while on: the average is left alone
    assert _same_bits(e.ema_arena(), avg)
    e.set_params_arena(w)
    e.set_ema(None)                                  # -> off: updating stops, the arena stays readable
    e.train_step(f, p, c)
    e.forward(f, p, c)
    e.backward()
    e.adam_step()
    assert _same_bits(e.ema_arena(), avg) and e.ema_info() == (0.0, 2, False)
    e.set_ema(D)                                     # on again: a fresh copy
    assert _same_bits(e.ema_arena(), e.params_arena()) and e.ema_info() == (D, 0, False)
    e.set_ema_arena(avg, n_updates=7)
    assert _same_bits(e.ema_arena(), avg) and e.ema_info() == (D, 7, False)


def test_swap_exchanges_the_arenas_fp32():
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    e = _engine(cfg, seed)
    e.set_training(False)
    e.set_ema(D)
    for _ in range(2):
        e.train_step(f, p, c)
    w, avg, ck = e.params_arena(), e.ema_arena(), e.params_checksum()
    assert not _same_bits(w, avg)
    e.swap_ema()
    assert _same_bits(e.params_arena(), avg) and _same_bits(e.ema_arena(), w) and e.ema_info()[2]
    assert e.params_checksum() != ck
    e.swap_ema()
    assert _same_bits(e.params_arena(), w) and _same_bits(e.ema_arena(), avg) and not e.ema_info()[2]
    assert e.params_checksum() == ck
    with pytest.raises(ZeroDivisionError):           # the context manager swaps back on an exception too
        with e.averaged():
            assert e.ema_info()[2]
            1 / 0
    assert not e.ema_info()[2] and e.params_checksum() == ck
    e.train_step(f, p, c)                            # and training goes on


def test_swap_bf16_decodes_and_scores_on_the_average():
    """after an earlier decode (its tiles and bf16 embedding copy would be stale), swap: greedy ids and
    compute_loss equal those of a fresh engine loaded with ema_state_dict() -- ids identical, the loss to
    rel 1e-5 (test_dp_check_world1_forced's tolerance)"""
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _bf16_inputs(z)
    e = _bf16_engine(cfg, seed, dropout=0.0)
    e.set_ema(f32(0.5))
    e.set_lr(f32(20 * cfg.learning_rate))            # so that three steps move the captions
    ids_first, _ = e.greedy(f, p)
    for _ in range(3):
        e.train_step(f, p, c)
    ids_raw, _ = e.greedy(f, p)
    loss_raw = e.compute_loss(f, p, c).item()
    fresh = _bf16_engine(cfg, seed, dropout=0.0)
    fresh.load_state_dict(e.ema_state_dict(with_buffer=False))
    want_ids, _ = fresh.greedy(f, p)
    want_loss = fresh.compute_loss(f, p, c).item()
    with e.averaged():
        ids, _ = e.greedy(f, p)
        loss = e.compute_loss(f, p, c).item()
        sd = e.state_dict(False)                     # capgen_get_params: the averaged weights
        for k, v in fresh.state_dict(False).items():
            assert torch.equal(sd[k], v), k
    assert torch.equal(ids.cpu(), want_ids.cpu())
    assert abs(loss - want_loss) <= 1e-5 * abs(want_loss), (loss, want_loss)
    assert abs(loss - loss_raw) > 1e-4 * abs(loss_raw), "the average and the raw weights score alike: vacuous"
    back, _ = e.greedy(f, p)                         # swapped back: the raw weights' captions again
    assert torch.equal(back.cpu(), ids_raw.cpu())
    assert abs(e.compute_loss(f, p, c).item() - loss_raw) <= 1e-5 * abs(loss_raw)


def test_refusals():
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    e = _engine(cfg, seed)
    e.set_training(False)
    with pytest.raises(RuntimeError, match="ema_swap"):
        e.swap_ema()                                 # never enabled
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="weight_decay"):
            e.set_weight_decay(bad)
        assert e.lib.capgen_set_weight_decay(e.h, C.c_float(bad)) == 1
        assert b"set_weight_decay: wd" in e.lib.capgen_last_error()
    for bad in (-0.1, 1.0, 1.5, float("nan")):
        with pytest.raises(ValueError, match="decay"):
            e.set_ema(bad)
        assert e.lib.capgen_set_ema(e.h, C.c_float(bad)) == 1
        assert b"set_ema: decay" in e.lib.capgen_last_error()
    assert e.weight_decay is None and e.ema_info() == (0.0, 0, False)
    e.set_ema(D)
    e.train_step(f, p, c)
    e.set_ema(None)
    with pytest.raises(RuntimeError, match="ema_swap"):
        e.swap_ema()                                 # off
    e.set_ema(D)
    e.train_step(f, p, c)
    e.rl_sample(f, p, c)
    e.swap_ema()
    w = e.params_arena()
    step, m, v = _adam_arenas(e)
    idx = torch.arange(f.shape[0], dtype=torch.int32, device=f.device)
    ones = torch.ones(f.shape[0], device=f.device)
    from capgen.engine import Engine
    updating = [lambda: e.train_step(f, p, c),
                lambda: e.train_step_indexed(f, p, idx, c),
                lambda: e.train_step_weighted(f, p, c, ones),
                lambda: e.rl_finish(ones, 0.5, train=True),
                lambda: e.adam_step(),
                lambda: e.set_params_arena(w),
                lambda: e.set_adam_state(step, m, v),
                lambda: e.dp_init(Engine.dp_unique_id(), 0, 1)]
    for call_ in updating:
        with pytest.raises(RuntimeError, match="ema_swap"):
            call_()
    with pytest.raises(RuntimeError, match="set_ema"):
        e.set_ema(None)                              # nor may the average be switched off in there
    torch.cuda.synchronize()
    assert _same_bits(e.params_arena(), w) and _adam_arenas(e)[0] == step
    # what reads works: forward, losses without an update, scoring, decoding
    e.forward(f, p, c)
    e.compute_loss(f, p, c)
    e.train_step_weighted(f, p, c, ones, train=False)
    e.score_captions(f, p, c)
    e.greedy(f, p)
    e.set_ema(D2)                                    # the decay alone may change
    assert _same_bits(e.params_arena(), w)
    e.swap_ema()
    e.train_step(f, p, c)


def test_sharded_emulation_updates_the_average_in_own_chunks():
    """_sharded_update_check (world 2, fp32) with decay and the average on everywhere: the parameters
    assemble to the reference's (the helper), each rank's average equals the reference engine's inside
    its own chunks within the step bound and the enable-time copy everywhere else"""
    cfg, seed, z = load_fixture("c2s")
    f, p, c = _inputs(z)
    ref = _engine(cfg, seed)
    ranks = [_engine(cfg, seed) for _ in range(2)]
    for e in ranks + [ref]:
        e.set_weight_decay(WD)
        e.set_ema(D)
    start = ref.ema_arena()
    _sharded_update_check(cfg, ref, ranks, f, p, c, "fp32")
    want = ref.ema_arena()
    assert np.abs(want - start).max() > 10 * _e_bound(want, f32(cfg.learning_rate))
    buckets = ref.dp_buckets()
    for r, e in enumerate(ranks):
        mine = np.zeros(want.size, bool)
        for off, n in buckets:
            ch = n // 2
            mine[off + r * ch: off + (r + 1) * ch] = True
        got = e.ema_arena()
        assert _same_bits(got[~mine], start[~mine])
        err = np.abs(got[mine].astype(np.float64) - want[mine]).max()
        ebound = _e_bound(want, f32(cfg.learning_rate))
        print(f"rank {r}: average error against the reference engine {err:.3e} of bound {ebound:.3e}")
        assert err <= ebound, (r, err, ebound)
        assert e.ema_info()[1] == 2
        with pytest.raises(RuntimeError, match="dp_sync_adam_state"):
            e.swap_ema()                             # stale outside its chunks


def test_step_with_everything_on_has_no_unordered_conflicts():
    cfg, seed, z = load_fixture("c2s")
    e = _bf16_engine(cfg, seed)
    e.set_grad_clip(1.0)
    e.set_weight_decay(WD)
    e.set_ema(D)
    n, report = _logged_run(e, *_bf16_inputs(z))
    assert n == 0, f"{n} unordered conflicting launch pairs:\n{report}"
    assert e.ema_info()[1] == 3
    from capgen import _lib
    _lib.hazard_start()
    try:
        e.swap_ema()
        e.forward(*_bf16_inputs(z))
        e.swap_ema()
        e.train_step(*_bf16_inputs(z))
        torch.cuda.synchronize()
        n, report = _lib.hazard_check()
    finally:
        _lib.hazard_stop()
    assert n == 0, f"{n} unordered conflicting launch pairs around the swap:\n{report}"


def _trainer(cfg, seed, **kw):
    from capgen.models import TRANSFORMER
    vocab = {f"w{i}": i for i in range(cfg.num_vocab)}
    t = TRANSFORMER(cfg.replace(dtype="fp32"), word_to_idx=vocab, device="cuda:0",
                    state_dict=fixture_state_dict(cfg, seed=seed, with_buffer=False), **kw)
    t.model.eval()  # dropout off (the seed is not part of a checkpoint)
    return t


def test_resume_from_a_checkpoint(tmp_path):
    """two steps, save_checkpoint, two more; a fresh trainer loads the checkpoint and runs two: the
    parameters and the average agree to 1e-6 (test_bucketed_train_step_equals_unfused_fp32's tolerance
    over three steps), the Adam step counts are equal and the lr_schedule continues"""
    from capgen import schedule
    cfg, seed, z = load_fixture("c1")
    f, p, c = _inputs(z)
    sched = lambda t: schedule.warmup_inverse_sqrt(t, f32(cfg.learning_rate), 3)  # noqa: E731
    kw = dict(grad_clip=5.0, lr_schedule=sched, weight_decay=WD, ema_decay=schedule.ema_warmup(D))
    a = _trainer(cfg, seed, **kw)
    for _ in range(2):
        a.train_step(f, p, c)
    path = str(tmp_path / "ck.pt")
    a.save_checkpoint(path)
    ck = torch.load(path, map_location="cpu", weights_only=True)
    assert ck["adam"]["step"] == 2 and ck["ema"]["n_updates"] == 2 and ck["weight_decay"] == WD
    assert ck["grad_clip"] == 5.0 and ck["lr"] == f32(sched(2)) and ck["ema"]["decay"] == f32(2 / 11)
    for _ in range(2):
        a.train_step(f, p, c)
    b = _trainer(cfg, seed + 1, **kw)               # other weights: everything must come from the file
    b.load_checkpoint(path)
    eb = b.model.engine
    assert _same_bits(eb.ema_arena(), ck["ema"]["params"].numpy()) and eb.ema_info()[:2] == (f32(2 / 11), 2)
    for _ in range(2):
        b.train_step(f, p, c)
    ea = a.model.engine
    _params_close(ea, eb, 1e-6)
    assert np.abs(ea.ema_arena() - eb.ema_arena()).max() <= 1e-6
    assert _adam_arenas(ea)[0] == _adam_arenas(eb)[0] == 4
    assert ea.lr == eb.lr == f32(sched(4)) and ea.ema_info() == eb.ema_info() == (f32(4 / 13), 4, False)
    # a plain trainer (no options) restores them from the file as well
    d = _trainer(cfg, seed + 2)
    d.load_checkpoint(path)
    assert d.model.engine.weight_decay == WD and d.model.engine.grad_clip == 5.0
    assert d.model.engine.ema_info()[:2] == (f32(2 / 11), 2) and d.model.engine.lr == f32(sched(2))
    # save() / load() stay what they were: the weights alone
    a.save(str(tmp_path / "w.pt"))
    assert set(torch.load(str(tmp_path / "w.pt"), weights_only=True)) == set(ck["model"])
