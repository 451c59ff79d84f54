"""`TRANSFORMER` — drop-in for core/models.py:18-135 (the object `main.py` drives).

main.py uses exactly: train_step, compute_loss, generate_caption, decode_captions, save,
load (main.py:65,70,73,85,112,116,124,151).  Inputs arrive as host tensors; the wrapper
stages them into persistent device buffers so the captured train-step hipGraph replays
with fixed pointers (the reference did a synchronous pageable `.to(DEVICE)` per step,
models.py:120-122).
"""
from __future__ import annotations

import contextlib

import numpy as np
import torch

from .config import CapgenConfig
from .engine import check_diverse_call, must_include_slots
from .model import PolicyNetwork, Transformer
from .schedule import ScheduledSteps
from .staging import HostBatchStager
from .utils import decode_captions, leave_one_out_baseline, load_word_to_idx, rollout_captions, sequence_logprob


def _on_device(t) -> bool:
    return isinstance(t, torch.Tensor) and t.is_cuda


class MODEL_init:
    def __init__(self, word_to_idx=None, word_to_idx_path=None):
        if word_to_idx is None:
            if word_to_idx_path is None:
                raise ValueError("capgen: pass word_to_idx or word_to_idx_path (models.py:22)")
            word_to_idx = load_word_to_idx(word_to_idx_path)
        self.num_vocab = len(word_to_idx)
        self.word_to_idx = dict(word_to_idx)
        self.idx_to_word = {i: w for w, i in word_to_idx.items()}
        self.end_idx = word_to_idx.get("<END>")
        self.model = None

    def train_step(self, *a, **k):
        raise NotImplementedError

    def compute_loss(self, *a, **k):
        raise NotImplementedError

    def generate_caption(self, object_features, position_features, beam_size=None):
        """models.py:34-56: None/1 -> greedy (+attention_list); int > 1 -> beam search."""
        if beam_size in [None, 1]:
            ids, attention_list = self.model.generate_caption_vector(object_features=object_features,
                                                                     position_features=position_features)
            return self.decode_captions(ids.cpu().numpy()), attention_list
        if isinstance(beam_size, int) and beam_size > 1:
            ids = self.model.beam_search(object_features=object_features, position_features=position_features,
                                         beam_size=beam_size)
            return self.decode_captions(ids.cpu().numpy()), None
        assert isinstance(beam_size, int)
        assert beam_size > 1 or beam_size in [None, 1]

    @contextlib.contextmanager
    def _constrained(self, no_repeat_ngram, min_length, repetition_penalty, banned_words):
        """The engine's decode constraints for one generation call: set on entry where any is asked for and
        switched off again on the way out, whatever happened, so that nothing leaks into a later call or a
        trainer's roll-outs.  banned_words are words of the vocabulary; <END> comes from it too."""
        banned = []
        for w in banned_words:
            if w not in self.word_to_idx:
                raise ValueError(f"capgen: banned word {w!r} is not in the vocabulary")
            banned.append(int(self.word_to_idx[w]))
        if min_length and self.end_idx is None:
            raise ValueError("capgen: min_length needs <END> in the vocabulary")
        on = bool(no_repeat_ngram or min_length or banned) or float(repetition_penalty) != 1.0
        engine = self.model.engine
        try:
            if on:
                engine.set_decode_constraints(no_repeat_ngram=no_repeat_ngram, min_length=min_length,
                                              end_id=-1 if self.end_idx is None else int(self.end_idx),
                                              repetition_penalty=repetition_penalty, banned=banned)
            yield
        finally:
            if on:
                engine.set_decode_constraints()

    def beam_captions(self, object_features, position_features, beam_size, length_penalty=0.0, n_best=1,
                      no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned_words=(), num_groups=1,
                      diversity_penalty=0.0, must_include=None):
        """The n_best captions per image of a beam search that stops at <END> (generate_caption keeps the
        reference's search, which does not): (captions, score) -- n_best lists of B strings, best first, and
        their scores [n_best, B] (f32, on the model's device): the caption's log-probability through <END>
        divided by its length ** length_penalty (0.0: the log-probability itself).  A vocabulary without
        <END> searches to max_length.  Constraints, for this call only (Engine.set_decode_constraints): no
        n-gram of no_repeat_ngram words twice, no <END> before min_length tokens, the logits of the words
        already said scaled down by repetition_penalty, and banned_words (e.g. "<NULL>", "<START>", "<UNK>")
        never; the scores are log-probabilities under the constrained distribution.
        num_groups > 1: diverse beam search -- the beams in num_groups groups, a later group penalised by
        diversity_penalty for each earlier hypothesis that chose the same word at the same position; n_best
        then counts per group (<= beam_size / num_groups) and num_groups * n_best lists come back, group-major
        (all of group 0's first), with scores [num_groups * n_best, B] that never contain the penalty.
        must_include: words the captions must contain (forced-word beam search, Engine.beam_forced) -- one entry
        per image, each a sequence of groups, each group a word or a sequence of alternative words ("dog", or
        ("dog", "dogs", "puppy")); an empty entry requires nothing of its image.  The captions come back ordered
        by the number of groups they contain, then by score; a caption that ran out of positions may miss a
        group.  At most 16 groups per image and beam_size + (the most words of any image) <= 15; not together
        with num_groups > 1.  None, or every entry empty, is the call as it was."""
        end = -1 if self.end_idx is None else int(self.end_idx)
        slots = None if must_include is None else must_include_slots(must_include, self.word_to_idx,
                                                                      len(object_features), beam_size, num_groups)
        diverse = check_diverse_call(beam_size, num_groups, diversity_penalty, end, length_penalty, n_best,
                                     self.config.num_vocab)
        with self._constrained(no_repeat_ngram, min_length, repetition_penalty, banned_words):
            if slots is not None:
                ids, score, _, _, _ = self.model.beam_search_forced(
                    object_features=object_features, position_features=position_features, beam_size=beam_size,
                    end_id=end, word=slots[0], group=slots[1], length_penalty=length_penalty, n_best=n_best)
            elif diverse:
                ids, score, _, _ = self.model.beam_search_diverse(
                    object_features=object_features, position_features=position_features, beam_size=beam_size,
                    num_groups=num_groups, diversity_penalty=diversity_penalty, end_id=end,
                    length_penalty=length_penalty, n_best=n_best)
            else:
                ids, score, _, _ = self.model.beam_search_nbest(object_features=object_features,
                                                                position_features=position_features,
                                                                beam_size=beam_size, end_id=end,
                                                                length_penalty=length_penalty, n_best=n_best)
        host = ids.cpu().numpy()
        return [self.decode_captions(host[j]) for j in range(host.shape[0])], score

    def sample_captions(self, object_features, position_features, n_samples=1, temperature=1.0, top_k=0, seed=None,
                        top_p=1.0, no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned_words=()):
        """n_samples captions per image drawn from the model's distribution (temperature / top-k /
        nucleus top_p sampling): (captions, logprob) -- n lists of B strings and each caption's log-probability
        [n, B] (f32, on the model's device: the sum of its token log-probabilities through <END>).
        no_repeat_ngram, min_length, repetition_penalty and banned_words constrain this call as they do
        beam_captions; the log-probabilities are then those of the constrained distribution, which is why
        the self-critical trainers' roll-outs never use them (they would be off-policy)."""
        with self._constrained(no_repeat_ngram, min_length, repetition_penalty, banned_words):
            ids, logp = self.model.sample_caption_vector(object_features=object_features,
                                                         position_features=position_features, n_samples=n_samples,
                                                         temperature=temperature, top_k=top_k, seed=seed,
                                                         top_p=top_p)
        host = ids.cpu().numpy()
        end = -1 if self.end_idx is None else self.end_idx  # (no <END> in the vocabulary: every token counts)
        logprob = sequence_logprob(ids[..., 1:logp.shape[-1] + 1], logp, end)
        return [self.decode_captions(host[j]) for j in range(host.shape[0])], logprob

    def score_captions(self, object_features, position_features, captions, length_penalty=0.0):
        """How likely are these captions for these images: the log-probability of given caption ids under
        the model (teacher-forced, temperature 1, unconstrained, dropout off whatever the train/eval state;
        nothing is updated).  captions: [B, T] ids, one per image, or [n, B, T], n candidates per image (the
        features are read through an image index: one copy serves all n); tensor or numpy, <START> first,
        padded with <NULL> after <END> (utils.rollout_captions turns decoded ids into this form).  Returns a
        dict of tensors on the model's device, shaped like the input without T: 'logp' (the sum of the
        token log-probabilities through <END>), 'score' = logp / max(length, 1) ** length_penalty
        (beam_captions' formula), 'token_logp' [..., T-1] (0 at pad targets), 'length' (non-pad targets,
        int32) and 'token_accuracy' = the share of them that are the teacher-forced argmax."""
        caps = torch.as_tensor(captions)
        if caps.dim() not in (2, 3):
            raise ValueError("capgen: captions must be [B, T] or [n, B, T] ids")
        if len(object_features.shape) != 3 or len(position_features.shape) != 3:
            raise ValueError("capgen: object_features [B, N, F] and position_features [B, N, P] are needed")
        B = int(object_features.shape[0])
        if caps.shape[-2] != B or int(position_features.shape[0]) != B:
            raise ValueError("capgen: captions must have the batch of the features")
        T = int(caps.shape[-1])
        if T < 2 or T > self.config.max_length:
            raise ValueError("capgen: captions need 2 <= T <= max_length")
        eng = self.model.engine
        if caps.dim() == 2:
            tok, logp, length, hits = eng.score_captions(object_features, position_features, caps)
        else:
            n = int(caps.shape[0])
            idx = torch.arange(B, dtype=torch.int32).repeat(n)
            tok, logp, length, hits = eng.score_captions(object_features, position_features, caps.reshape(n * B, T),
                                                         img_idx=idx)
            tok, logp, length, hits = tok.view(n, B, T - 1), logp.view(n, B), length.view(n, B), hits.view(n, B)
        denom = length.clamp(min=1).to(torch.float32)
        return {"logp": logp, "score": logp / denom ** float(length_penalty), "token_logp": tok, "length": length,
                "token_accuracy": hits.to(torch.float32) / denom}

    def decode_captions(self, caption_vector):
        return decode_captions(caption_vector, self.idx_to_word)

    def set_schedule(self, lr_schedule=None, grad_clip=None, weight_decay=None, ema_decay=None):
        """Replace the constructor's lr_schedule / grad_clip / weight_decay / ema_decay (capgen.train.train
        forwards its own here)."""
        self._sched = ScheduledSteps(self.model.engine, lr_schedule, grad_clip, weight_decay, ema_decay)

    def averaged(self):
        """with model.averaged(): ... -- evaluate and decode on the averaged weights (Engine.averaged)."""
        return self.model.engine.averaged()

    def save(self, path):
        torch.save(self.model.state_dict(), path)

    def load(self, path):
        sd = torch.load(path, map_location="cpu", weights_only=True)
        self.model.load_state_dict(sd)
        self.model.eval()

    def save_checkpoint(self, path):
        """Everything a stopped run needs to go on, as one torch.save dict that loads with
        weights_only=True: 'format'; 'model', the reference-keyed state dict (what save() writes, loadable
        by the reference); 'adam' = {step, exp_avg, exp_avg_sq}; 'ema' = None or {decay, n_updates,
        params}; 'lr'; 'grad_clip'; 'weight_decay'.  At world > 1 this first calls dp_sync_adam_state,
        a COLLECTIVE: every rank must call save_checkpoint (any one of them may keep the file).  The
        dropout seed is not part of the checkpoint (the engine has no getter for it): a resumed run
        draws other masks than the uninterrupted one."""
        eng = self.model.engine
        if eng.dp_comm_info()[0] > 1:
            eng.dp_sync_adam_state()
        torch.save(checkpoint_dict(eng), path)

    def load_checkpoint(self, path):
        """Restore what save_checkpoint wrote: weights, Adam state, the average, learning rate, clip bound
        and weight decay.  The trainer's lr_schedule / ema_decay schedules then continue from the restored
        counters (they are re-read at the next step).  The train / eval state is left as it is."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        if ck.get("format") != CHECKPOINT_FORMAT:
            raise ValueError(f"capgen: {path} is not a {CHECKPOINT_FORMAT} checkpoint")
        eng = self.model.engine
        self.model.load_state_dict(ck["model"])
        ad = ck["adam"]
        eng.set_adam_state(int(ad["step"]), ad["exp_avg"].numpy(), ad["exp_avg_sq"].numpy())
        eng.set_lr(float(ck["lr"]))
        eng.set_grad_clip(ck["grad_clip"])
        eng.set_weight_decay(ck["weight_decay"])
        if ck["ema"] is None:
            eng.set_ema(None)
        else:
            eng.set_ema(float(ck["ema"]["decay"]))
            eng.set_ema_arena(ck["ema"]["params"].numpy(), int(ck["ema"]["n_updates"]))
        sched = getattr(self, "_sched", None)
        if sched is not None:
            sched._done = sched._ema_done = None


CHECKPOINT_FORMAT = "capgen-checkpoint-1"


def checkpoint_dict(eng):
    """The checkpoint of MODEL_init.save_checkpoint from an engine (tensors, numbers, None: nothing
    that torch.load(weights_only=True) refuses)."""
    decay, n_updates, swapped = eng.ema_info()
    if swapped:
        raise RuntimeError("capgen: save_checkpoint inside averaged(): the parameters hold the average")
    m = np.empty(eng.arena_elems, np.float32)
    v = np.empty(eng.arena_elems, np.float32)
    step = eng.adam_arenas(m, v)
    ema = None
    if decay != 0.0:
        ema = {"decay": float(decay), "n_updates": int(n_updates), "params": torch.from_numpy(eng.ema_arena())}
    return {"format": CHECKPOINT_FORMAT, "model": eng.state_dict(),
            "adam": {"step": int(step), "exp_avg": torch.from_numpy(m), "exp_avg_sq": torch.from_numpy(v)},
            "ema": ema, "lr": float(eng.lr), "grad_clip": eng.grad_clip, "weight_decay": eng.weight_decay}


class TRANSFORMER(MODEL_init):
    """grad_clip: clip every update's gradients to this global L2 norm (torch's clip_grad_norm_;
    float('inf') only measures, engine.grad_norm()); lr_schedule: a callable t -> learning rate
    (capgen.schedule), applied before each train step with t the Adam step number of that update.
    weight_decay: decoupled decay as torch.optim.AdamW (Engine.set_weight_decay).  ema_decay: keep an
    exponential moving average of the weights (Engine.set_ema; evaluate on it inside averaged()) -- a
    float, or a callable of the average's update count such as capgen.schedule.ema_warmup(0.999).
    None (default) for all four: the engine is never told anything."""

    def __init__(self, config: CapgenConfig | None = None, word_to_idx=None, word_to_idx_path=None,
                 device="cuda:0", state_dict=None, grad_clip=None, lr_schedule=None, weight_decay=None,
                 ema_decay=None):
        super().__init__(word_to_idx, word_to_idx_path)
        cfg = (config or CapgenConfig()).replace(num_vocab=self.num_vocab)
        self.config = cfg
        self.device = torch.device(device)
        self.model = Transformer.from_config(cfg, self.device, state_dict=state_dict)
        self._sched = ScheduledSteps(self.model.engine, lr_schedule, grad_clip, weight_decay, ema_decay)
        self._stage = {}
        self._host_stager = None

    def _staged(self, name, t, dtype):
        buf = self._stage.get(name)
        if buf is None or buf.shape != t.shape or buf.dtype != dtype:
            buf = torch.empty(t.shape, dtype=dtype, device=self.device)
            self._stage[name] = buf
        buf.copy_(t, non_blocking=True)
        return buf

    def train_step(self, batch_features, batch_positions, batch_captions):
        """models.py:115-126: zero_grad + forward + backward + Adam, one engine call.

        Host (CPU / numpy) batches -- what main.py's DataLoader yields -- go through pinned,
        double-buffered staging with the copy on a side stream, overlapped with the previous
        step (capgen.staging.HostBatchStager); device tensors are staged by a D2D copy."""
        self._sched.before_step()
        if not _on_device(batch_features):
            st = self._host_stager
            if st is None or not st.fits(batch_features, batch_positions, batch_captions):
                B, N, F = batch_features.shape
                st = self._host_stager = HostBatchStager(self.device, B, N, F, batch_positions.shape[2],
                                                         batch_captions.shape[1])
            st.run(self.model.engine, batch_features, batch_positions, batch_captions)
            return
        fdt = torch.bfloat16 if self.config.dtype == "bf16" else torch.float32
        f = self._staged("f", batch_features, fdt)
        p = self._staged("p", batch_positions, torch.float32)
        c = self._staged("c", batch_captions, torch.int32)
        self.model.engine.train_step(f, p, c)

    def train_step_resident(self, store, img_idx, captions):
        """train_step over an HBM-resident split (capgen.data.DeviceFeatureStore / ResidentBatches):
        the batch names its images; nothing is copied from the host."""
        self._sched.before_step()
        self.model.engine.train_step_indexed(store.features, store.positions, img_idx, captions)

    def compute_loss(self, object_features, position_features, target_caption):
        """models.py:128-135 (no_grad; dropout follows train/eval state)."""
        with torch.no_grad():
            return self.model(object_features=object_features, position_features=position_features,
                              target_caption=target_caption)


class SelfCriticNetwork(MODEL_init):
    """Drop-in for core/models.py:137-211 (SCST, config C5): same network as TRANSFORMER
    (PolicyNetwork, model_RL.py:10-97 = Encoder/Decoder/classifer), trained on
    (1 - w) * CE + w * structure loss with CIDEr-D + BLEU-4 + entropy rewards (loss.py:31-220).

    One step = capgen_rl_sample (GPU) -> host scoring of the greedy-from-logits samples
    (capgen/scst.py, parity unpinned) -> capgen_rl_finish (GPU: loss, backward, Adam).

    df: CIDEr-D document frequencies.  The reference scores with CiderD(df='coco-val')
    (loss.py:112), a table computed from the COCO validation references that the reference does
    not ship; the default 'corpus' computes them from the references being scored (coco-caption's
    corpus mode) and warns.  Pass df=(document_frequency, ref_len) to use a precomputed table."""

    def __init__(self, config: CapgenConfig | None = None, word_to_idx=None, word_to_idx_path=None,
                 device="cuda:0", state_dict=None, structure_loss_weight=0.5, cider_reward_weight=1.0,
                 bleu_reward_weight=1.0, entropy_reward_weight=1.0, self_cider_reward_weight=1.0, df="corpus",
                 grad_clip=None, lr_schedule=None, weight_decay=None, ema_decay=None):
        super().__init__(word_to_idx, word_to_idx_path)
        from .scst import RewardScorer
        cfg = (config or CapgenConfig()).replace(num_vocab=self.num_vocab)
        self.config = cfg
        self.device = torch.device(device)
        # PolicyNetwork (model_RL.py): generate_caption then decodes with LogSoftmax scoring
        self.model = PolicyNetwork.from_config(cfg, self.device, state_dict=state_dict)
        self._sched = ScheduledSteps(self.model.engine, lr_schedule, grad_clip, weight_decay, ema_decay)  # (as TRANSFORMER's)
        if isinstance(df, str) and df == "corpus":
            import warnings
            warnings.warn("capgen SelfCriticNetwork: CIDEr-D document frequencies from the scored references "
                          "(df='corpus'); the reference uses CiderD(df='coco-val') (loss.py:112), whose table is "
                          "not shipped with it -- pass df=(document_frequency, ref_len) for that reward",
                          stacklevel=2)
        self.structure_loss_weight = float(structure_loss_weight)  # core/config.py:81-85
        self.scorer = RewardScorer(self.idx_to_word, cider_reward_weight, bleu_reward_weight, entropy_reward_weight,
                                   self_cider_reward_weight, df=df)

    def _step(self, object_features, position_features, target_caption, train):
        eng = self.model.engine
        sample, entropy, _ = eng.rl_sample(object_features, position_features, target_caption)
        target = torch.as_tensor(target_caption)[:, 1:].cpu().numpy()
        reward = np.broadcast_to(self.scorer.scores(target, sample.cpu().numpy()), (sample.shape[0],))
        total = self.scorer.total(reward, entropy.cpu().numpy())
        out = eng.rl_finish(total, self.structure_loss_weight, train=train)
        return out, reward

    def train_step(self, batch_features, batch_positions, batch_captions):
        """models.py:179-195: forward, sample, reward, loss.backward(), Adam step."""
        self._sched.before_step()
        self._step(batch_features, batch_positions, batch_captions, train=True)

    def compute_loss(self, object_features, position_features, target_caption):
        """models.py:198-211 -> {'loss', 'language_model_loss', 'structure_loss', 'reward'}
        (config.py:65-68 keys; reward [B, 1] as in loss.py:121)."""
        with torch.no_grad():
            out, reward = self._step(object_features, position_features, target_caption, train=False)
        return {"loss": out[0], "language_model_loss": out[1], "structure_loss": out[2],
                "reward": torch.as_tensor(np.array(reward), dtype=torch.float32).view(-1, 1)}


class RolloutSelfCritic(MODEL_init):
    """Self-critical sequence training on free-running samples (Rennie et al. 2017; the n-sample
    variant of Luo 2020) -- beside SelfCriticNetwork, the port of the reference's trainer, whose
    "sample" is the argmax of a teacher-forced forward.

    One step: engine.sample draws n_samples captions per image (one encoder pass, KV-cached); the
    host scores them against the ground truth (CIDEr-D / BLEU-4, capgen_scst_rewards, or reward_fn);
    the baseline is the greedy caption's reward ("greedy") or the mean of the row's other samples
    ("mean", n_samples >= 2); one engine.train_step_weighted on the n * B sampled captions with the
    advantages as per-caption weights ascends advantage * log p(sample).  The n * B caption rows
    share the B images through img_idx, and the bf16 step keeps the fused classifier + CE.
    temperature / top_k / top_p shape the behaviour policy only: the gradient is taken through the model's
    own log-probabilities.

    reward_fn(target_ids [B, L], sample_ids [B, L]) -> [B] (host numpy) replaces the scorer.
    seed: step i draws with seed + i; None takes each step's seed from torch's CPU generator."""

    def __init__(self, config: CapgenConfig | None = None, word_to_idx=None, word_to_idx_path=None,
                 device="cuda:0", state_dict=None, n_samples=5, temperature=1.0, top_k=0, baseline="greedy",
                 cider_reward_weight=1.0, bleu_reward_weight=0.0, df="corpus", reward_fn=None, seed=None,
                 grad_clip=None, lr_schedule=None, top_p=1.0, weight_decay=None, ema_decay=None):
        super().__init__(word_to_idx, word_to_idx_path)
        from .scst import RewardScorer
        if baseline not in ("greedy", "mean"):
            raise ValueError("capgen RolloutSelfCritic: baseline must be 'greedy' or 'mean'")
        if baseline == "mean" and int(n_samples) < 2:
            raise ValueError("capgen RolloutSelfCritic: baseline='mean' needs n_samples >= 2")
        cfg = (config or CapgenConfig()).replace(num_vocab=self.num_vocab)
        self.config = cfg
        self.device = torch.device(device)
        self.model = PolicyNetwork.from_config(cfg, self.device, state_dict=state_dict)
        self._sched = ScheduledSteps(self.model.engine, lr_schedule, grad_clip, weight_decay, ema_decay)  # (as TRANSFORMER's)
        self.n_samples, self.temperature, self.top_k = int(n_samples), float(temperature), int(top_k)
        self.top_p = float(top_p)
        self.baseline, self.reward_fn, self.seed = baseline, reward_fn, seed
        self.steps = 0
        self._stage = {}
        self.scorer = None
        if reward_fn is None:
            self.scorer = RewardScorer(self.idx_to_word, cider_reward_weight, bleu_reward_weight, 0.0, 0.0, df=df)

    _staged = TRANSFORMER._staged

    def _rewards(self, target, sample):
        fn = self.reward_fn if self.reward_fn is not None else self.scorer.scores
        return np.asarray(fn(target, sample), dtype=np.float64).reshape(target.shape[0])

    def _step(self, batch_features, batch_positions, batch_captions, train):
        eng, n, cfg = self.model.engine, self.n_samples, self.config
        if self.seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        else:
            seed = int(self.seed) + self.steps
        self.steps += int(train)  # (compute_loss draws with the next train step's seed and leaves it)
        f, _, p, _ = eng._inputs(batch_features, batch_positions)
        if not (_on_device(batch_features) and _on_device(batch_positions)):
            f, p = self._staged("f", f, f.dtype), self._staged("p", p, torch.float32)
        B = f.shape[0]
        ids, _ = eng.sample(f, p, n, self.temperature, self.top_k, seed, want_logp=False, top_p=self.top_p)
        caps = rollout_captions(ids, self.end_idx, cfg.pad_idx)  # [n, B, T]
        target = torch.as_tensor(batch_captions)[:, 1:].cpu().numpy()
        L = min(target.shape[1], caps.shape[-1] - 1)
        host = caps[..., 1:].cpu().numpy()
        r = np.stack([self._rewards(target[:, :L], host[j][:, :L]) for j in range(n)])  # [n, B]
        if self.baseline == "greedy":
            g = rollout_captions(eng.greedy(f, p, want_attention=False)[0], self.end_idx, cfg.pad_idx)
            base = np.broadcast_to(self._rewards(target[:, :L], g[:, 1:].cpu().numpy()[:, :L]), r.shape)
        else:
            base = leave_one_out_baseline(r)
        # persistent device buffers: the step's graphs are keyed by pointer and replay while these stay
        adv = self._staged("w", torch.as_tensor((r - base).reshape(n * B), dtype=torch.float32), torch.float32)
        c = self._staged("c", caps.view(n * B, -1), torch.int32)
        idx = self._staged("i", torch.arange(B, dtype=torch.int32).repeat(n), torch.int32)
        loss = eng.train_step_weighted(f, p, c, adv, img_idx=idx, train=train)
        self.last_reward = r  # [n, B] sample rewards of this step (host, float64): for logging
        return loss, r, base

    def train_step(self, batch_features, batch_positions, batch_captions):
        self._sched.before_step()
        self._step(batch_features, batch_positions, batch_captions, train=True)

    def compute_loss(self, object_features, position_features, target_caption):
        """{'loss', 'reward' [B, 1] (mean sample reward), 'baseline_reward' [B, 1]}; nothing is updated."""
        with torch.no_grad():
            loss, r, base = self._step(object_features, position_features, target_caption, train=False)
        as_col = lambda x: torch.as_tensor(np.array(x.mean(0)), dtype=torch.float32).view(-1, 1)  # noqa: E731
        return {"loss": loss[0].clone(), "reward": as_col(r), "baseline_reward": as_col(base)}
