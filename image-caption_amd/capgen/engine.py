"""Python handle over one libcapgen engine (one process, one device).

Thin: argument checking, dtype/layout normalisation of torch tensors, the
state_dict <-> packed-arena mapping, and current-stream plumbing.  All compute is in
libcapgen.so.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
from collections import OrderedDict

import numpy as np
import torch

from . import _lib
from .config import CapgenConfig
from .params import PE_BUFFER, sinusoid_table


def _ptr(t: torch.Tensor | None):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream(device) -> C.c_void_p:
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check_beam_nbest_args(beam_size, end_id, length_penalty, n_best, num_vocab):
    """The argument rules of capgen_beam_nbest, checked before anything is allocated (the library checks
    them again); returns (beam_size, n_best) as ints.  Each message names its argument."""
    for name, v in (("beam_size", beam_size), ("end_id", end_id), ("n_best", n_best)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"capgen beam_nbest: {name} must be an int, not {type(v).__name__}")
    if not 1 <= beam_size <= min(16, num_vocab):
        raise ValueError(f"capgen beam_nbest: beam_size must be in [1, min(16, num_vocab)], not {beam_size}")
    if not 1 <= n_best <= beam_size:
        raise ValueError(f"capgen beam_nbest: n_best must be in [1, beam_size], not {n_best}")
    if not -1 <= end_id < num_vocab:
        raise ValueError(f"capgen beam_nbest: end_id must be in [-1, num_vocab), not {end_id}")
    alpha = float(length_penalty)
    if not (0.0 <= alpha < float("inf")):  # (false for a NaN)
        raise ValueError(f"capgen beam_nbest: length_penalty must be finite and >= 0, not {length_penalty}")
    return int(beam_size), int(n_best)


def check_beam_diverse_args(beam_size, num_groups, diversity_penalty, end_id, length_penalty, n_best, num_vocab):
    """The argument rules of capgen_beam_diverse, as check_beam_nbest_args; returns (beam_size, num_groups,
    n_best) as ints.  n_best counts per group."""
    if isinstance(num_groups, bool) or not isinstance(num_groups, (int, np.integer)):
        raise TypeError(f"capgen beam_diverse: num_groups must be an int, not {type(num_groups).__name__}")
    check_beam_nbest_args(beam_size, end_id, length_penalty, 1, num_vocab)  # (n_best: the per-group rule below)
    if not 1 <= num_groups <= beam_size or beam_size % num_groups:
        raise ValueError(f"capgen beam_diverse: num_groups must be in [1, beam_size] and divide it, not {num_groups}")
    lam = float(diversity_penalty)
    if not (0.0 <= lam < float("inf")):  # (false for a NaN)
        raise ValueError(f"capgen beam_diverse: diversity_penalty must be finite and >= 0, not {diversity_penalty}")
    if isinstance(n_best, bool) or not isinstance(n_best, (int, np.integer)):
        raise TypeError(f"capgen beam_diverse: n_best must be an int, not {type(n_best).__name__}")
    if not 1 <= n_best <= beam_size // num_groups:
        raise ValueError(f"capgen beam_diverse: n_best must be in [1, beam_size / num_groups], not {n_best}")
    return int(beam_size), int(num_groups), int(n_best)


def check_diverse_call(beam_size, num_groups, diversity_penalty, end_id, length_penalty, n_best, num_vocab) -> bool:
    """beam_captions' num_groups / diversity_penalty: False for the defaults (1, 0.0), which leave the call
    the beam_nbest call it was; else the arguments are checked as beam_diverse's (a ValueError names the
    offending one before the library is called) and True comes back."""
    if not isinstance(num_groups, bool) and isinstance(num_groups, (int, np.integer)) and num_groups == 1 \
            and float(diversity_penalty) == 0.0:
        return False
    check_beam_diverse_args(beam_size, num_groups, diversity_penalty, end_id, length_penalty, n_best, num_vocab)
    return True


def check_beam_forced_args(beam_size, end_id, length_penalty, n_best, word, group, B, num_vocab):
    """The argument rules of capgen_beam_forced, as check_beam_nbest_args, and those of its word / group slots
    (integer arrays [B, W]; word -1: an empty slot), which the library cannot check: it never reads the device
    arrays on the host.  Returns (beam_size, n_best, word, group) with word / group as int32 arrays, or None
    for both where no slot holds a word -- the call is then beam_nbest's."""
    try:
        beam_size, n_best = check_beam_nbest_args(beam_size, end_id, length_penalty, n_best, num_vocab)
    except (TypeError, ValueError) as e:
        raise type(e)(str(e).replace("beam_nbest", "beam_forced")) from None
    word, group = np.asarray(word), np.asarray(group)
    for name, a in (("word", word), ("group", group)):
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise TypeError(f"capgen beam_forced: {name} must hold integers, not {a.dtype}")
    if word.ndim != 2 or word.shape[0] != B:
        raise ValueError(f"capgen beam_forced: word must be [B = {B}, W], not {list(word.shape)}")
    if group.shape != word.shape:
        raise ValueError(f"capgen beam_forced: group must have word's shape {list(word.shape)}, not {list(group.shape)}")
    held = word != -1
    if not held.any():
        return beam_size, n_best, None, None
    W = word.shape[1]
    if beam_size + W > 15:
        raise ValueError(f"capgen beam_forced: beam_size + words must be <= 15, not {beam_size} + {W}")
    if beam_size + W + 1 > num_vocab:
        raise ValueError(f"capgen beam_forced: beam_size + words + 1 must be <= num_vocab, not {beam_size} + {W} + 1")
    bad = held & ((word < 0) | (word >= num_vocab) | (word == end_id) | (word == 0) | (word == 1))
    if bad.any():
        raise ValueError(f"capgen beam_forced: word must be -1 or in [0, num_vocab) and not end_id, 0 (<NULL>) or 1 "
                         f"(<START>), not {int(word[bad][0])}")
    if ((group < 0) | (group >= 16))[held].any():
        raise ValueError(f"capgen beam_forced: group must be in [0, 16), not {int(group[held & ((group < 0) | (group >= 16))][0])}")
    return beam_size, n_best, np.ascontiguousarray(word, np.int32), np.ascontiguousarray(group, np.int32)


def must_include_slots(must_include, word_to_idx, B, beam_size, num_groups=1):
    """beam_captions' must_include -> (word, group) int arrays [B, W] for beam_forced, or None where nothing is
    required (None, or every entry empty: the call stays what it was).  must_include has one entry per image,
    each a sequence of groups, each group a word or a sequence of alternative words.  A ValueError names
    must_include and what is wrong with it, before the library is called."""
    if must_include is None:
        return None
    per_image = list(must_include)
    if len(per_image) != B:
        raise ValueError(f"must_include must have one entry per image ({B}), not {len(per_image)}")
    slots = []
    for i, entry in enumerate(per_image):
        if isinstance(entry, str):
            raise ValueError(f"must_include[{i}] must be a sequence of groups, not the string {entry!r} "
                             f"(write [{entry!r}] for one required word)")
        groups = [] if entry is None else list(entry)
        if len(groups) > 16:
            raise ValueError(f"must_include[{i}]: at most 16 groups per image, not {len(groups)}")
        mine = []
        for g, alt in enumerate(groups):
            for w in ([alt] if isinstance(alt, str) else list(alt)):
                if w not in word_to_idx:
                    raise ValueError(f"must_include[{i}]: unknown word {w!r}")
                if w in ("<END>", "<NULL>", "<START>"):
                    raise ValueError(f"must_include[{i}]: {w} cannot be required")
                mine.append((int(word_to_idx[w]), g))
        slots.append(mine)
    W = max(len(s) for s in slots) if slots else 0
    if W == 0:
        return None
    if not isinstance(num_groups, bool) and isinstance(num_groups, (int, np.integer)) and num_groups > 1:
        raise ValueError("must_include cannot be combined with num_groups > 1")
    if isinstance(beam_size, (int, np.integer)) and beam_size + W > 15:
        raise ValueError(f"must_include: too many words for the beam: beam_size + words must be <= 15, not "
                         f"{beam_size} + {W}")
    word, group = np.full((B, W), -1, np.int32), np.zeros((B, W), np.int32)
    for i, mine in enumerate(slots):
        for s, (w, g) in enumerate(mine):
            word[i, s], group[i, s] = w, g
    return word, group


def check_ema_decay(decay) -> float:
    """Engine.set_ema's argument rule, on the f32 the engine stores (0.99999999 rounds to 1.0f): the value
    to pass on, 0.0 for off; a ValueError naming the argument otherwise."""
    d = 0.0 if decay is None else float(np.float32(decay))
    if not (d == 0.0 or 0.0 < d < 1.0):  # (false for a NaN)
        raise ValueError(f"capgen: ema decay must be None, 0 or in (0, 1) as an f32, not {decay}")
    return d


def check_ensemble_args(engines, weights, mode):
    """The argument rules of a capgen_ensemble that need no device (the library checks them again, and the
    members' configs): returns (engines as a list, weights as floats or None, the mode's number).  Each
    message names its argument."""
    engines = list(engines)
    if not 1 <= len(engines) <= 8:
        raise ValueError(f"capgen ensemble: engines must hold 1 to 8 members, not {len(engines)}")
    for k, e in enumerate(engines):
        if any(e is o for o in engines[:k]):
            raise ValueError(f"capgen ensemble: engines[{k}] is a duplicate member")
    if mode not in _lib.ENS_MODES:
        raise ValueError(f"capgen ensemble: mode must be 'prob' or 'logprob', not {mode!r}")
    if weights is not None:
        weights = [float(w) for w in weights]
        if len(weights) != len(engines):
            raise ValueError(f"capgen ensemble: weights must hold one value per member ({len(engines)}), "
                             f"not {len(weights)}")
        for k, w in enumerate(weights):
            if not (0.0 < w < float("inf")):  # (false for a NaN)
                raise ValueError(f"capgen ensemble: weights[{k}] must be finite and > 0, not {w}")
    return engines, weights, _lib.ENS_MODES[mode]


def _beam_nbest(lead, call, feats, pos, beam_size, end_id, length_penalty, n_best):
    """Engine.beam_nbest and ensemble_beam_nbest: lead's inputs and outputs; call(*arguments after the handle)
    issues the C call"""
    beam_size, n = check_beam_nbest_args(beam_size, end_id, length_penalty, n_best, lead.cfg.num_vocab)
    f, ft, p, _ = lead._inputs(feats, pos)
    B, N, _ = f.shape
    T = lead.cfg.max_length
    dev = lead.device
    ids = torch.empty(n * B, T, dtype=torch.int64, device=dev)
    score = torch.empty(n * B, dtype=torch.float32, device=dev)
    logp = torch.empty(n * B, dtype=torch.float32, device=dev)
    length = torch.empty(n * B, dtype=torch.int32, device=dev)
    _lib.check(call(_ptr(f), ft, _ptr(p), B, N, beam_size, int(end_id), float(length_penalty), n, _ptr(ids),
                    _ptr(score), _ptr(logp), _ptr(length), _stream(dev)))
    return ids.view(n, B, T), score.view(n, B), logp.view(n, B), length.view(n, B)


def _beam_diverse(lead, call, feats, pos, beam_size, num_groups, diversity_penalty, end_id, length_penalty, n_best):
    """Engine.beam_diverse and ensemble_beam_diverse, as _beam_nbest; n = num_groups * n_best rows per image"""
    beam_size, G, nb = check_beam_diverse_args(beam_size, num_groups, diversity_penalty, end_id, length_penalty,
                                               n_best, lead.cfg.num_vocab)
    f, ft, p, _ = lead._inputs(feats, pos)
    B, N, _ = f.shape
    T, n = lead.cfg.max_length, G * nb
    dev = lead.device
    ids = torch.empty(n * B, T, dtype=torch.int64, device=dev)
    score = torch.empty(n * B, dtype=torch.float32, device=dev)
    logp = torch.empty(n * B, dtype=torch.float32, device=dev)
    length = torch.empty(n * B, dtype=torch.int32, device=dev)
    _lib.check(call(_ptr(f), ft, _ptr(p), B, N, beam_size, G, float(diversity_penalty), int(end_id),
                    float(length_penalty), nb, _ptr(ids), _ptr(score), _ptr(logp), _ptr(length), _stream(dev)))
    return ids.view(n, B, T), score.view(n, B), logp.view(n, B), length.view(n, B)


def _beam_forced(lead, call, feats, pos, beam_size, end_id, word, group, length_penalty, n_best):
    """Engine.beam_forced and ensemble_beam_forced, as _beam_nbest, plus met [n_best, B] int32"""
    f, ft, p, _ = lead._inputs(feats, pos)
    B, N, _ = f.shape
    if isinstance(word, torch.Tensor):
        word = word.cpu().numpy()
    if isinstance(group, torch.Tensor):
        group = group.cpu().numpy()
    beam_size, n, word, group = check_beam_forced_args(beam_size, end_id, length_penalty, n_best, word, group, B,
                                                       lead.cfg.num_vocab)
    T = lead.cfg.max_length
    dev = lead.device
    W = 0 if word is None else word.shape[1]
    wd = None if word is None else torch.from_numpy(word).to(dev)
    gd = None if group is None else torch.from_numpy(group).to(dev)
    ids = torch.empty(n * B, T, dtype=torch.int64, device=dev)
    score = torch.empty(n * B, dtype=torch.float32, device=dev)
    logp = torch.empty(n * B, dtype=torch.float32, device=dev)
    length = torch.empty(n * B, dtype=torch.int32, device=dev)
    met = torch.empty(n * B, dtype=torch.int32, device=dev)
    _lib.check(call(_ptr(f), ft, _ptr(p), B, N, beam_size, int(end_id), float(length_penalty), n, _ptr(wd), _ptr(gd),
                    W, _ptr(ids), _ptr(score), _ptr(logp), _ptr(length), _ptr(met), _stream(dev)))
    return ids.view(n, B, T), score.view(n, B), logp.view(n, B), length.view(n, B), met.view(n, B)


def _sample(lead, call, feats, pos, n_samples, temperature, top_k, seed, want_logp, top_p):
    """Engine.sample and ensemble_sample, as _beam_nbest"""
    f, ft, p, _ = lead._inputs(feats, pos)
    B, N, _ = f.shape
    n, T = int(n_samples), lead.cfg.max_length
    rows = max(n, 0) * B
    dev = lead.device
    ids = torch.empty(rows, T + 1, dtype=torch.int64, device=dev)
    logp = torch.empty(rows, T - 1, dtype=torch.float32, device=dev) if want_logp else None
    _lib.check(call(_ptr(f), ft, _ptr(p), B, N, n, float(temperature), int(top_k), float(top_p),
                    int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(ids), _ptr(logp), _stream(dev)))
    return ids.view(n, B, T + 1), (logp.view(n, B, T - 1) if want_logp else None)


def ensemble_beam_nbest(engines, feats, pos, beam_size, end_id, length_penalty=0.0, n_best=1, weights=None,
                        mode="prob"):
    """Engine.beam_nbest over the averaged next-word distribution of several engines
    (capgen_ensemble_beam_nbest): engines[0] leads -- its hypotheses, decode constraints, stream and device --
    and every member decodes the same hypotheses with its own weights.  weights: one positive value per
    member, normalised to sum 1 (None: equal); mode 'prob' averages the probabilities, 'logprob' the
    log-probabilities.  Returns what Engine.beam_nbest returns, scored under the ensemble distribution."""
    engines, weights, m = check_ensemble_args(engines, weights, mode)
    lead, e = engines[0], _lib.ensemble([x.h for x in engines], weights, m)
    return _beam_nbest(lead, lambda *a: lead.lib.capgen_ensemble_beam_nbest(C.byref(e), *a), feats, pos, beam_size,
                       end_id, length_penalty, n_best)


def ensemble_beam_diverse(engines, feats, pos, beam_size, num_groups, diversity_penalty, end_id, length_penalty=0.0,
                          n_best=1, weights=None, mode="prob"):
    """Engine.beam_diverse over the averaged next-word distribution of several engines
    (capgen_ensemble_beam_diverse; members, weights and mode as ensemble_beam_nbest's)."""
    engines, weights, m = check_ensemble_args(engines, weights, mode)
    lead, e = engines[0], _lib.ensemble([x.h for x in engines], weights, m)
    return _beam_diverse(lead, lambda *a: lead.lib.capgen_ensemble_beam_diverse(C.byref(e), *a), feats, pos,
                         beam_size, num_groups, diversity_penalty, end_id, length_penalty, n_best)


def ensemble_beam_forced(engines, feats, pos, beam_size, end_id, word, group, length_penalty=0.0, n_best=1,
                         weights=None, mode="prob"):
    """Engine.beam_forced over the averaged next-word distribution of several engines
    (capgen_ensemble_beam_forced; members, weights and mode as ensemble_beam_nbest's)."""
    engines, weights, m = check_ensemble_args(engines, weights, mode)
    lead, e = engines[0], _lib.ensemble([x.h for x in engines], weights, m)
    return _beam_forced(lead, lambda *a: lead.lib.capgen_ensemble_beam_forced(C.byref(e), *a), feats, pos, beam_size,
                        end_id, word, group, length_penalty, n_best)


def ensemble_sample(engines, feats, pos, n_samples=1, temperature=1.0, top_k=0, seed=0, want_logp=True, top_p=1.0,
                    weights=None, mode="prob"):
    """Engine.sample from the averaged next-word distribution of several engines (capgen_ensemble_sample;
    members, weights and mode as ensemble_beam_nbest's).  Returns what Engine.sample returns; logp is each
    token's log-probability under the ensemble distribution it was drawn from."""
    engines, weights, m = check_ensemble_args(engines, weights, mode)
    lead, e = engines[0], _lib.ensemble([x.h for x in engines], weights, m)
    return _sample(lead, lambda *a: lead.lib.capgen_ensemble_sample(C.byref(e), *a), feats, pos, n_samples,
                   temperature, top_k, seed, want_logp, top_p)


class Engine:
    def __init__(self, cfg: CapgenConfig, device="cuda:0"):
        self.cfg = cfg
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("capgen: the engine runs on a HIP device (cuda:N under ROCm)")
        self.lib = _lib.load()
        self._c = _lib.to_c_config(cfg)
        self.table, self.arena_elems = _lib.param_table(cfg)
        h = C.c_void_p()
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        _lib.check(self.lib.capgen_create(C.byref(self._c), idx, C.byref(h)))
        self.h = h
        self.training = True
        self.grad_clip = None  # the max_norm set_grad_clip last set (None: clipping off)
        self.weight_decay = None  # the value set_weight_decay last set (None: decay off)
        self._loss = torch.zeros(1, dtype=torch.float32, device=self.device)

    def close(self):
        if getattr(self, "h", None):
            self.lib.capgen_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- module state -------------------------------------------------------------------
    def set_training(self, training: bool):
        self.training = bool(training)
        _lib.check(self.lib.capgen_set_training(self.h, int(self.training)))

    def set_decode_log_softmax(self, enable: bool):
        """PolicyNetwork decoding (model_RL.py:72,126,182): greedy / beam score with LogSoftmax and
        beams accumulate log-probabilities; False (default) = Transformer (Softmax, probabilities)."""
        _lib.check(self.lib.capgen_set_decode_log_softmax(self.h, int(enable)))

    def set_graph(self, enable: bool):
        _lib.check(self.lib.capgen_set_graph(self.h, int(enable)))

    # ---- run-time optimizer control --------------------------------------------------------
    def set_lr(self, lr: float):
        """The Adam learning rate of every update issued from now on (finite, >= 0; capgen_set_lr): a
        replayed step graph reads the new value, nothing is re-captured."""
        _lib.check(self.lib.capgen_set_lr(self.h, float(lr)))

    @property
    def lr(self) -> float:
        """The learning rate last set (cfg.learning_rate until the first set_lr), as the f32 the engine uses."""
        v = C.c_float(0)
        _lib.check(self.lib.capgen_get_lr(self.h, C.byref(v)))
        return v.value

    def set_grad_clip(self, max_norm: float | None):
        """Clip every update's gradients to the global L2 norm `max_norm`, as
        torch.nn.utils.clip_grad_norm_ does (capgen_set_grad_clip): None or 0 = off (default), a finite
        value > 0 clips, float('inf') only measures the norm (see grad_norm)."""
        _lib.check(self.lib.capgen_set_grad_clip(self.h, 0.0 if max_norm is None else float(max_norm)))
        self.grad_clip = None if not max_norm else float(max_norm)

    def grad_norm(self) -> float:
        """The global gradient L2 norm, before clipping, of the most recent update that ran with clipping
        or measuring on (synchronous; raises if there was none)."""
        v = C.c_float(0)
        _lib.check(self.lib.capgen_last_grad_norm(self.h, C.byref(v)))
        return v.value

    def set_weight_decay(self, weight_decay: float | None):
        """Decoupled weight decay as torch.optim.AdamW (capgen_set_weight_decay): every parameter is
        multiplied by 1 - lr * weight_decay before each update.  None or 0 = off (default); finite, >= 0."""
        wd = 0.0 if weight_decay is None else float(weight_decay)
        if not (math.isfinite(wd) and wd >= 0.0):
            raise ValueError(f"capgen: weight_decay must be finite and >= 0, not {weight_decay}")
        _lib.check(self.lib.capgen_set_weight_decay(self.h, wd))
        self.weight_decay = wd or None

    def set_ema(self, decay: float | None):
        """Keep an exponential moving average of the parameters inside the update kernel
        (capgen_set_ema; torch.optim.swa_utils.get_ema_multi_avg_fn(decay)): None or 0 = off (default),
        else 0 < decay < 1.  Off -> on starts the average as a copy of the parameters; on -> on changes
        the decay only; off keeps the arena readable."""
        _lib.check(self.lib.capgen_set_ema(self.h, check_ema_decay(decay)))

    def ema_info(self):
        """(decay as the f32 the engine uses, 0.0 = off; updates issued while on; swapped in?)."""
        d, n, s = C.c_float(0), C.c_int64(0), C.c_int(0)
        _lib.check(self.lib.capgen_ema_info(self.h, C.byref(d), C.byref(n), C.byref(s)))
        return d.value, n.value, bool(s.value)

    def ema_arena(self) -> np.ndarray:
        """The averaged weights' f32 arena as a host copy (the raw weights while swapped).  After sharded
        (ZeRO-1) steps: this rank's chunks only until dp_sync_adam_state."""
        torch.cuda.current_stream(self.device).synchronize()
        return self._arena_to_host(self.lib.capgen_get_ema)

    def ema_state_dict(self, with_buffer: bool = True):
        """ema_arena() as reference-named f32 CPU tensors (loadable like state_dict())."""
        sd = self._unpack(self.ema_arena())
        if with_buffer:
            sd[PE_BUFFER] = torch.from_numpy(sinusoid_table(self.cfg.max_length - 1, self.cfg.decode_input_size)[None])
        return sd

    def set_ema_arena(self, arena: np.ndarray, n_updates: int = 0):
        """Overwrite the average's arena and its update counter (checkpoint restore; the average must be on)."""
        a = np.ascontiguousarray(arena, dtype=np.float32)
        assert a.size == self.arena_elems
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_set_ema_state(self.h, a.ctypes.data_as(C.c_void_p), self.arena_elems,
                                                 int(n_updates)))

    def swap_ema(self):
        """Exchange the parameters and the average in place (capgen_ema_swap): forward, losses, scoring
        and every decoder then run on the averaged weights, and every updating call raises until the
        next swap_ema()."""
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_ema_swap(self.h))

    @contextlib.contextmanager
    def averaged(self):
        """with engine.averaged(): ... -- the averaged weights swapped in for the block, and back out
        after it, exceptions included."""
        self.swap_ema()
        try:
            yield self
        finally:
            self.swap_ema()

    def adam_step_count(self) -> int:
        """The number of Adam updates so far (the optimizer's step counter t; follows set_adam_state).
        Synchronous: the trainers read it once and count their own steps from there."""
        torch.cuda.current_stream(self.device).synchronize()
        step = C.c_int64(0)
        _lib.check(self.lib.capgen_get_adam_state(self.h, C.byref(step), None, None, self.arena_elems))
        return step.value

    def set_adam_state(self, step: int, exp_avg: np.ndarray | None = None, exp_avg_sq: np.ndarray | None = None):
        """Restore the optimizer (capgen_set_adam_state): the step counter and the two moment arenas
        (f32, the parameter arena's layout; None = zeros).  A trainer created afterwards continues its
        lr_schedule from `step`."""
        def arr(a):
            if a is None:
                return None, None
            a = np.ascontiguousarray(a, dtype=np.float32)
            assert a.size == self.arena_elems
            return a, a.ctypes.data_as(C.c_void_p)
        torch.cuda.current_stream(self.device).synchronize()
        m, mp = arr(exp_avg)
        v, vp = arr(exp_avg_sq)
        _lib.check(self.lib.capgen_set_adam_state(self.h, int(step), mp, vp, self.arena_elems))

    def _arena_to_host(self, fn) -> np.ndarray:
        buf = np.empty(self.arena_elems, dtype=np.float32)
        _lib.check(fn(self.h, buf.ctypes.data_as(C.c_void_p), self.arena_elems))
        return buf

    def _unpack(self, arena: np.ndarray) -> "OrderedDict[str, torch.Tensor]":
        sd = OrderedDict()
        for name, ndim, rows, cols, off, stride in self.table:
            view = np.lib.stride_tricks.as_strided(arena[off:], shape=(rows, cols), strides=(stride * 4, 4))
            a = np.array(view, dtype=np.float32)
            sd[name] = torch.from_numpy(a if ndim == 2 else a.reshape(cols))
        return sd

    def state_dict(self, with_buffer: bool = True):
        """Reference-named f32 CPU tensors (checkpoint-compatible with model.py's keys)."""
        torch.cuda.current_stream(self.device).synchronize()
        sd = self._unpack(self._arena_to_host(self.lib.capgen_get_params))
        if with_buffer:
            sd[PE_BUFFER] = torch.from_numpy(sinusoid_table(self.cfg.max_length - 1, self.cfg.decode_input_size)[None])
        return sd

    def grads_state_dict(self):
        torch.cuda.current_stream(self.device).synchronize()
        return self._unpack(self._arena_to_host(self.lib.capgen_get_grads))

    def set_grads_arena(self, arena: np.ndarray):
        """Overwrite the whole f32 gradient arena (layout: capgen_param_table) from host memory."""
        a = np.ascontiguousarray(arena, dtype=np.float32)
        assert a.size == self.arena_elems
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_set_grads(self.h, a.ctypes.data_as(C.c_void_p), self.arena_elems))

    def params_arena(self) -> np.ndarray:
        """The whole f32 parameter arena as a host copy."""
        torch.cuda.current_stream(self.device).synchronize()
        return self._arena_to_host(self.lib.capgen_get_params)

    def set_params_arena(self, arena: np.ndarray):
        """Overwrite the whole f32 parameter arena (and the bf16 shadow) from host memory."""
        a = np.ascontiguousarray(arena, dtype=np.float32)
        assert a.size == self.arena_elems
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_set_params(self.h, a.ctypes.data_as(C.c_void_p), self.arena_elems))

    def grads_arena(self) -> np.ndarray:
        """The whole f32 gradient arena as a host copy."""
        torch.cuda.current_stream(self.device).synchronize()
        return self._arena_to_host(self.lib.capgen_get_grads)

    def load_state_dict(self, sd, strict: bool = True):
        arena = np.zeros(self.arena_elems, dtype=np.float32)
        seen = set()
        for name, ndim, rows, cols, off, stride in self.table:
            if name not in sd:
                if strict:
                    raise KeyError(f"capgen: missing key {name!r} in state_dict")
                continue
            v = sd[name]
            v = v.detach().cpu().float().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float32)
            want = (rows, cols) if ndim == 2 else (cols,)
            if tuple(v.shape) != want:
                raise ValueError(f"capgen: {name}: shape {tuple(v.shape)} != {want}")
            view = np.lib.stride_tricks.as_strided(arena[off:], shape=(rows, cols), strides=(stride * 4, 4))
            view[...] = v.reshape(rows, cols)
            seen.add(name)
        if strict:
            extra = set(sd) - seen - {PE_BUFFER}
            if extra:
                raise KeyError(f"capgen: unexpected keys in state_dict: {sorted(extra)[:5]}")
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_set_params(self.h, arena.ctypes.data_as(C.c_void_p), self.arena_elems))

    def adam_state(self):
        step = C.c_int64(0)
        m = np.empty(self.arena_elems, np.float32)
        v = np.empty(self.arena_elems, np.float32)
        _lib.check(self.lib.capgen_get_adam_state(self.h, C.byref(step), m.ctypes.data_as(C.c_void_p),
                                                  v.ctypes.data_as(C.c_void_p), self.arena_elems))
        return step.value, self._unpack(m), self._unpack(v)

    def adam_arenas(self, exp_avg: np.ndarray, exp_avg_sq: np.ndarray) -> int:
        """Fill two host f32 arrays of arena size with the moment arenas; returns the step counter."""
        step = C.c_int64(0)
        assert exp_avg.size == exp_avg_sq.size == self.arena_elems
        torch.cuda.current_stream(self.device).synchronize()
        _lib.check(self.lib.capgen_get_adam_state(self.h, C.byref(step), exp_avg.ctypes.data_as(C.c_void_p),
                                                  exp_avg_sq.ctypes.data_as(C.c_void_p), self.arena_elems))
        return step.value

    # ---- inputs ----------------------------------------------------------------------
    def _inputs(self, feats, pos, caps=None):
        dev = self.device
        if feats.dtype not in (torch.float32, torch.bfloat16):
            feats = feats.float()
        feats = feats.to(dev, non_blocking=True).contiguous()
        pos = pos.to(dev, dtype=torch.float32, non_blocking=True).contiguous()
        if feats.dim() != 3 or pos.dim() != 3 or feats.shape[:2] != pos.shape[:2]:
            raise ValueError("capgen: object_features [B,N,F] and position_features [B,N,P] must agree")
        if feats.shape[2] != self.cfg.encode_dim_features or pos.shape[2] != self.cfg.encode_dim_positions:
            raise ValueError("capgen: feature widths do not match the config")
        ft = _lib.BF16 if feats.dtype == torch.bfloat16 else _lib.F32
        if caps is not None:
            caps = caps.to(dev, dtype=torch.int32, non_blocking=True).contiguous()
            if caps.dim() != 2 or caps.shape[0] != feats.shape[0]:  # model.py:203
                raise ValueError("capgen: target_caption must be [B, T] with the batch of the features")
        return feats, ft, pos, caps

    # ---- hot path --------------------------------------------------------------------
    def forward(self, feats, pos, caps, loss_out=None):
        f, ft, p, c = self._inputs(feats, pos, caps)
        B, N, _ = f.shape
        out = self._loss if loss_out is None else loss_out
        _lib.check(self.lib.capgen_forward(self.h, _ptr(f), ft, _ptr(p), _ptr(c), B, N, c.shape[1], _ptr(out),
                                           _stream(self.device)))
        return out

    def backward(self):
        _lib.check(self.lib.capgen_backward(self.h, _stream(self.device)))

    def adam_step(self):
        _lib.check(self.lib.capgen_adam_step(self.h, _stream(self.device)))

    def train_step(self, feats, pos, caps, loss_out=None):
        f, ft, p, c = self._inputs(feats, pos, caps)
        B, N, _ = f.shape
        out = self._loss if loss_out is None else loss_out
        _lib.check(self.lib.capgen_train_step(self.h, _ptr(f), ft, _ptr(p), _ptr(c), B, N, c.shape[1], _ptr(out),
                                              _stream(self.device)))
        return out

    def train_step_raw(self, f, ft, p, c, B, N, T, out):
        """Pre-normalised device tensors (bench loop): no checks, no copies."""
        _lib.check(self.lib.capgen_train_step(self.h, _ptr(f), ft, _ptr(p), _ptr(c), B, N, T, _ptr(out),
                                              _stream(self.device)))

    def train_step_indexed(self, feat_store, pos_store, img_idx, caps, out=None):
        """Training step reading features of images img_idx[b] from device-resident stores
        (capgen.data.DeviceFeatureStore): no per-step host->device copy of features."""
        assert feat_store.is_cuda and pos_store.is_cuda and img_idx.is_cuda and caps.is_cuda
        assert feat_store.dim() == 3 and pos_store.shape[:2] == feat_store.shape[:2]
        ft = _lib.BF16 if feat_store.dtype == torch.bfloat16 else _lib.F32
        idx = img_idx.to(torch.int32).contiguous()
        c = caps.to(torch.int32).contiguous()
        B, T = c.shape
        out = self._loss if out is None else out
        _lib.check(self.lib.capgen_train_step_indexed(self.h, _ptr(feat_store), ft, _ptr(pos_store),
                                                      feat_store.shape[0], _ptr(idx), _ptr(c), B,
                                                      feat_store.shape[1], T, _ptr(out), _stream(self.device)))
        return out

    def train_step_weighted(self, feats, pos, caps, weights, img_idx=None, train=True, out=None):
        """Teacher-forced step on caps [B, T] whose cross entropy is weighted per caption
        (capgen_train_step_weighted): loss = sum_b w_b sum_t [tgt != pad] CE_bt / count.  weights [B]
        f32, any sign (the advantages of sampled roll-outs give the self-critical policy gradient).
        img_idx [B] given: feats / pos are [n_images, N, .] and row b reads image img_idx[b], so n
        roll-outs per image share one copy of the features; None: feats / pos are [B, N, .].
        train=False: the weighted loss only, nothing changes.  Returns the loss tensor.  A weights
        tensor already on the device in f32 is read in place (its pointer keys the captured graphs)."""
        dev = self.device
        if weights is None:
            w = None
        else:
            w = torch.as_tensor(weights).to(dev, dtype=torch.float32).contiguous()
        c = caps.to(dev, dtype=torch.int32, non_blocking=True).contiguous()
        if c.dim() != 2 or (w is not None and w.shape != (c.shape[0],)):
            raise ValueError("capgen: captions must be [B, T] and weights [B]")
        B, T = c.shape
        if img_idx is None:
            f, ft, p, _ = self._inputs(feats, pos, c)
            idx, n_img = None, 0
        else:
            f, ft, p, _ = self._inputs(feats, pos)
            idx = img_idx.to(dev, dtype=torch.int32).contiguous()
            if idx.shape != (B,):
                raise ValueError("capgen: img_idx must be [B]")
            n_img = f.shape[0]
        out = self._loss if out is None else out
        _lib.check(self.lib.capgen_train_step_weighted(self.h, _ptr(f), ft, _ptr(p), n_img, _ptr(idx), _ptr(c),
                                                       _ptr(w), B, f.shape[1], T, _ptr(out), int(bool(train)),
                                                       _stream(self.device)))
        return out

    def compute_loss(self, feats, pos, caps):
        out = torch.zeros(1, dtype=torch.float32, device=self.device)
        f, ft, p, c = self._inputs(feats, pos, caps)
        B, N, _ = f.shape
        _lib.check(self.lib.capgen_compute_loss(self.h, _ptr(f), ft, _ptr(p), _ptr(c), B, N, c.shape[1], _ptr(out),
                                                _stream(self.device)))
        return out

    def score_captions(self, feats, pos, caps, img_idx=None):
        """Log-probabilities of given captions caps [R, T] under the model (capgen_score_captions): the
        teacher-forced forward with dropout off, read out per token.  Targets are caps[:, 1:]; a pad
        target scores exactly 0 and does not count.  img_idx [R] given: feats / pos are [n_images, N, .]
        and row r reads image img_idx[r], so several candidates per image share one copy of the
        features; None: feats / pos are [R, N, .].  Returns (token_logp [R, T-1] f32, logp [R] f32,
        length [R] int32, hits [R] int32) on the engine's device; hits counts the kept positions whose
        target is the teacher-forced argmax.  Nothing of the engine's training state changes."""
        dev = self.device
        c = torch.as_tensor(caps).to(dev, dtype=torch.int32, non_blocking=True).contiguous()
        if c.dim() != 2:
            raise ValueError("capgen: captions must be [R, T]")
        R, T = c.shape
        if img_idx is None:
            f, ft, p, _ = self._inputs(feats, pos, c)
            idx, n_img = None, 0
        else:
            f, ft, p, _ = self._inputs(feats, pos)
            idx = torch.as_tensor(img_idx).to(dev, dtype=torch.int32).contiguous()
            if idx.shape != (R,):
                raise ValueError("capgen: img_idx must be [R]")
            n_img = f.shape[0]
        tok = torch.empty(R, max(T - 1, 0), dtype=torch.float32, device=dev)
        logp = torch.empty(R, dtype=torch.float32, device=dev)
        length = torch.empty(R, dtype=torch.int32, device=dev)
        hits = torch.empty(R, dtype=torch.int32, device=dev)
        _lib.check(self.lib.capgen_score_captions(self.h, _ptr(f), ft, _ptr(p), n_img, _ptr(idx), _ptr(c), R,
                                                  f.shape[1], T, _ptr(tok), _ptr(logp), _ptr(length), _ptr(hits),
                                                  _stream(self.device)))
        return tok, logp, length, hits

    def logits(self, B, T):
        out = torch.empty(B * (T - 1), self.cfg.num_vocab, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.capgen_copy_logits(self.h, _ptr(out), out.numel(), _stream(self.device)))
        return out.view(B, T - 1, -1)

    def greedy(self, feats, pos, want_attention=True):
        f, ft, p, _ = self._inputs(feats, pos)
        B, N, _ = f.shape
        T = self.cfg.max_length
        ids = torch.empty(B, T + 1, dtype=torch.int64, device=self.device)
        attn = torch.empty(T - 1, B, N, dtype=torch.float32, device=self.device) if want_attention else None
        _lib.check(self.lib.capgen_greedy(self.h, _ptr(f), ft, _ptr(p), B, N, _ptr(ids), _ptr(attn),
                                          _stream(self.device)))
        return ids, attn

    def beam(self, feats, pos, beam_size):
        f, ft, p, _ = self._inputs(feats, pos)
        B, N, _ = f.shape
        ids = torch.empty(B, self.cfg.max_length, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.capgen_beam(self.h, _ptr(f), ft, _ptr(p), B, N, int(beam_size), _ptr(ids),
                                        _stream(self.device)))
        return ids

    def beam_nbest(self, feats, pos, beam_size, end_id, length_penalty=0.0, n_best=1):
        """The standard beam search (capgen_beam_nbest): a hypothesis stops at end_id (-1: never), finished
        ones compete with their log-probability frozen, and the n_best of the beam_size hypotheses per image
        come back ordered by score = logp / max(len, 1) ** length_penalty (0.0: logp itself).  Always scored
        with the log-softmax.  Returns (ids int64 [n, B, T] laid out as beam's, zeros after <END>; score f32
        [n, B]; logp f32 [n, B]; len int32 [n, B]: tokens through <END>, T - 1 where it never came)."""
        return _beam_nbest(self, lambda *a: self.lib.capgen_beam_nbest(self.h, *a), feats, pos, beam_size, end_id,
                           length_penalty, n_best)

    def beam_diverse(self, feats, pos, beam_size, num_groups, diversity_penalty, end_id, length_penalty=0.0, n_best=1):
        """Diverse beam search (capgen_beam_diverse): beam_nbest with the beams split into num_groups groups,
        each penalised by diversity_penalty per hypothesis of an earlier group that chose the same word at the
        same position.  n_best <= beam_size / num_groups counts per group.  Returns (ids [G * n_best, B,
        max_length] int64, score, logp f32 and len int32 [G * n_best, B]), group-major: row g * n_best + r is
        group g's r-th best; logp is the model's log-probability, without the penalty.  num_groups = 1 is
        beam_nbest."""
        return _beam_diverse(self, lambda *a: self.lib.capgen_beam_diverse(self.h, *a), feats, pos, beam_size,
                             num_groups, diversity_penalty, end_id, length_penalty, n_best)

    def beam_forced(self, feats, pos, beam_size, end_id, word, group, length_penalty=0.0, n_best=1):
        """Forced-word beam search (capgen_beam_forced): beam_nbest over captions that must contain given words.
        word / group: integer arrays [B, W], image i's slots (word -1: empty); a group in [0, 16) is a set of
        alternatives, met once the caption holds any of them; beam_size + W <= 15.  The search keeps, per
        position, the best hypotheses of every count of met groups in turn (highest count first) and never lets
        a hypothesis end with a group unmet; logp is the model's log-probability, nothing added.  Returns (ids
        [n_best, B, max_length] int64, score, logp f32, len and met int32 [n_best, B]), ordered by (groups met
        descending, score descending); met is the bitmask of the groups each caption met -- one that ran out of
        positions may miss some.  No word on any image is beam_nbest bit for bit, met all zero."""
        return _beam_forced(self, lambda *a: self.lib.capgen_beam_forced(self.h, *a), feats, pos, beam_size, end_id,
                            word, group, length_penalty, n_best)

    def set_decode_constraints(self, no_repeat_ngram=0, min_length=0, end_id=-1, repetition_penalty=1.0, banned=()):
        """What beam_nbest and sample may not say, from now on (capgen_set_decode_constraints; greedy and beam
        are never constrained): no n-gram twice (no_repeat_ngram = n, 0: off), no end_id before min_length
        tokens (0: off), every emitted word's logit divided (positive) or multiplied (negative) by
        repetition_penalty (1.0: off), and the word ids in banned never.  A blocked word has probability
        exactly 0 and every score, mass and logp is taken over what is left.  Called with no arguments:
        everything off (the default).  One more launch per decode step while anything is on."""
        banned = tuple(banned)
        if not (no_repeat_ngram or min_length or banned) and float(repetition_penalty) == 1.0:
            _lib.check(self.lib.capgen_set_decode_constraints(self.h, None))
            return
        c = _lib.decode_constraints(no_repeat_ngram, min_length, end_id, repetition_penalty, banned)
        _lib.check(self.lib.capgen_set_decode_constraints(self.h, C.byref(c)))

    def sample(self, feats, pos, n_samples=1, temperature=1.0, top_k=0, seed=0, want_logp=True, top_p=1.0):
        """n_samples captions per image drawn from softmax(logits / temperature) over the top_k largest
        logits (0: the whole vocabulary), KV-cached, one encoder pass (capgen_sample_nucleus).  top_p in
        (0, 1] cuts those candidates to the nucleus: the most likely words up to the one at which their
        mass reaches top_p, renormalised (1.0: no cut, exactly capgen_sample).  Returns
        (ids int64 [n, B, T+1] laid out as greedy's, logp f32 [n, B, T-1] or None): logp holds each
        token's log-probability under the distribution it was drawn from.  One (seed, inputs,
        weights) gives one result."""
        return _sample(self, lambda *a: self.lib.capgen_sample_nucleus(self.h, *a), feats, pos, n_samples, temperature,
                       top_k, seed, want_logp, top_p)

    # ---- SCST (SelfCriticNetwork) -------------------------------------------------------
    def rl_sample(self, feats, pos, caps):
        """Teacher-forced forward + PolicyNetwork.sample (model_RL.py:75-97): returns
        (sample int64 [B, T-1], per-image masked mean entropy f32 [B], LM CE loss f32 [1])."""
        f, ft, p, c = self._inputs(feats, pos, caps)
        B, N, _ = f.shape
        T = c.shape[1]
        seq = torch.empty(B, T - 1, dtype=torch.int64, device=self.device)
        ent = torch.empty(B, dtype=torch.float32, device=self.device)
        lm = torch.empty(1, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.capgen_rl_sample(self.h, _ptr(f), ft, _ptr(p), _ptr(c), B, N, T, _ptr(seq), _ptr(ent),
                                             _ptr(lm), _stream(self.device)))
        return seq, ent, lm

    def rl_finish(self, scores, structure_loss_weight: float, train: bool = True):
        """ReinforcementLearningLoss (loss.py:53-76) on the last rl_sample, with per-image total
        scores [B]; train=True also runs backward + Adam.  Returns {loss, lm, struct} [3]."""
        sc = torch.as_tensor(scores, dtype=torch.float32).to(self.device).contiguous()
        out = torch.empty(3, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.capgen_rl_finish(self.h, _ptr(sc), float(structure_loss_weight), _ptr(out), int(train),
                                             _stream(self.device)))
        return out

    def set_rng_seed(self, seed: int):
        _lib.check(self.lib.capgen_set_rng_seed(self.h, seed & 0xFFFFFFFFFFFFFFFF))

    # ---- data parallel -----------------------------------------------------------------
    @staticmethod
    def dp_unique_id() -> bytes:
        lib = _lib.load()
        buf = C.create_string_buffer(128)
        _lib.check(lib.capgen_dp_unique_id(buf))
        return buf.raw

    def dp_init(self, uid: bytes, rank: int, world: int):
        assert len(uid) == 128
        _lib.check(self.lib.capgen_dp_init(self.h, uid, rank, world))

    def dp_comm_info(self):
        """(communicator size, this rank) of the engine's RCCL communicator; (0, 0) before dp_init."""
        n, r = C.c_int(0), C.c_int(0)
        _lib.check(self.lib.capgen_dp_comm_info(self.h, C.byref(n), C.byref(r)))
        return n.value, r.value

    def dp_check(self, loss: torch.Tensor | None = None):
        """Run the data-parallel consistency check now (collective over the engine communicator, any
        world size): every rank's global non-pad count and loss must agree (max == min); raises
        RuntimeError otherwise.  `loss`: the [1] f32 device tensor the last step wrote (None = the
        engine's internal loss).  The step runs the same check once by itself at world > 1."""
        _lib.check(self.lib.capgen_dp_check(self.h, _ptr(loss), _stream(self.device)))

    def params_checksum(self) -> int:
        """Exact, order-independent checksum of the f32 parameters (equal on every rank of a DP run)."""
        v = C.c_uint64(0)
        _lib.check(self.lib.capgen_params_checksum(self.h, C.byref(v)))
        return v.value

    def dp_set_global_count(self, count: float):
        _lib.check(self.lib.capgen_dp_set_global_count(self.h, float(count)))

    def dp_sync_adam_state(self):
        """Collective (every rank): all-gather the sharded Adam moments (see capgen.h)."""
        _lib.check(self.lib.capgen_dp_sync_adam_state(self.h))

    def dp_buckets(self):
        """The last train step's gradient buckets as [(offset, count)] over the parameter arena."""
        cap = 256
        offs = np.zeros(cap, np.int64)
        cnts = np.zeros(cap, np.int64)
        n = C.c_int(0)
        _lib.check(self.lib.capgen_dp_buckets(self.h, offs.ctypes.data_as(C.c_void_p),
                                              cnts.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
        return [(int(offs[i]), int(cnts[i])) for i in range(n.value)]

    def collectives_log(self, op: int, cap: int = 1 << 16) -> str:
        """Test hook: 1 = start recording the engine's RCCL calls, 0 = stop, 2 = the recorded calls."""
        buf = C.create_string_buffer(cap)
        _lib.check(self.lib.capgen_debug_collectives(self.h, int(op), buf, cap))
        return buf.value.decode()

    def stamps(self, op: int):
        """Diagnostic un-profiled timeline (capgen_debug_stamps): op 1 on, 0 off, 3 arm; op 2 returns
        [(name, start_us, end_us)] of the last step's stamped launches (unlaunched slots: 0, 0)."""
        cap = 8192
        out = np.zeros(2 * cap, np.float64)
        names = C.create_string_buffer(1 << 20)
        n = self.lib.capgen_debug_stamps(self.h, int(op), out.ctypes.data_as(C.c_void_p), 2 * cap, names, 1 << 20)
        if n < 0:
            _lib.check(1)
        if op != 2:
            return None
        lines = names.value.decode().split("\n")
        return [(lines[i], out[2 * i], out[2 * i + 1]) for i in range(n)]

    def dp_debug_shard(self, rank: int, world: int):
        """Test hook: update as rank `rank` of `world` would under the sharded update, no collectives."""
        _lib.check(self.lib.capgen_dp_debug_shard(self.h, int(rank), int(world)))
