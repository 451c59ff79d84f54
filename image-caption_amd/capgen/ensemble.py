"""`Ensemble` -- several trained models decoded as one: per step the members' next-word distributions are
averaged and one beam search (or one set of draws) runs over the average.  The usual way a captioner is
evaluated: several seeds, the cross-entropy and the self-critical checkpoint, or the raw and the averaged
weights.  Host code; the lock-step decoding and the fusing kernel are in libcapgen.so
(capgen_ensemble_beam_nbest / capgen_ensemble_sample)."""
from __future__ import annotations

import math

import torch

from .engine import (check_diverse_call, check_ensemble_args, ensemble_beam_diverse, ensemble_beam_forced,
                     ensemble_beam_nbest, ensemble_sample, must_include_slots)
from .utils import sequence_logprob


class Ensemble:
    """models: TRANSFORMER / SelfCriticNetwork / RolloutSelfCritic objects over one vocabulary, on one device;
    models[0] leads (its engine owns the hypotheses and the decode constraints).  weights: one positive value
    per model, normalised to sum 1 (None: equal).  mode 'prob' averages the members' probabilities,
    'logprob' their log-probabilities (the weighted geometric mean, renormalised)."""

    def __init__(self, models, weights=None, mode="prob"):
        models = list(models)
        _, weights, _ = check_ensemble_args(models, weights, mode)
        for k, m in enumerate(models[1:], 1):
            if m.word_to_idx != models[0].word_to_idx:
                raise ValueError(f"capgen ensemble: models[{k}].word_to_idx differs from models[0]'s")
        self.models = models
        self.mode = mode
        self.weights = weights
        total = math.fsum(weights) if weights is not None else float(len(models))
        self.norm_weights = [(w if weights is not None else 1.0) / total
                             for w in (weights if weights is not None else [1.0] * len(models))]
        self.leader = models[0]

    def _engines(self):
        return [m.model.engine for m in self.models]

    def beam_captions(self, object_features, position_features, beam_size, length_penalty=0.0, n_best=1,
                      no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned_words=(), num_groups=1,
                      diversity_penalty=0.0, must_include=None):
        """MODEL.beam_captions over the ensemble distribution: (captions, score), the same shapes (num_groups,
        diversity_penalty and must_include included); the constraints are the leader's, for this call only."""
        lead = self.leader
        end = -1 if lead.end_idx is None else int(lead.end_idx)
        slots = None if must_include is None else must_include_slots(must_include, lead.word_to_idx,
                                                                      len(object_features), beam_size, num_groups)
        diverse = check_diverse_call(beam_size, num_groups, diversity_penalty, end, length_penalty, n_best,
                                     lead.config.num_vocab)
        with lead._constrained(no_repeat_ngram, min_length, repetition_penalty, banned_words):
            if slots is not None:
                ids, score, _, _, _ = ensemble_beam_forced(self._engines(), object_features, position_features,
                                                           beam_size, end, slots[0], slots[1],
                                                           length_penalty=length_penalty, n_best=n_best,
                                                           weights=self.weights, mode=self.mode)
            elif diverse:
                ids, score, _, _ = ensemble_beam_diverse(self._engines(), object_features, position_features,
                                                         beam_size, num_groups, diversity_penalty, end,
                                                         length_penalty=length_penalty, n_best=n_best,
                                                         weights=self.weights, mode=self.mode)
            else:
                ids, score, _, _ = ensemble_beam_nbest(self._engines(), object_features, position_features,
                                                       beam_size, end, length_penalty=length_penalty, n_best=n_best,
                                                       weights=self.weights, mode=self.mode)
        host = ids.cpu().numpy()
        return [lead.decode_captions(host[j]) for j in range(host.shape[0])], score

    def sample_captions(self, object_features, position_features, n_samples=1, temperature=1.0, top_k=0, seed=None,
                        top_p=1.0, no_repeat_ngram=0, min_length=0, repetition_penalty=1.0, banned_words=()):
        """MODEL.sample_captions from the ensemble distribution: (captions, logprob), the same shapes."""
        lead = self.leader
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        with lead._constrained(no_repeat_ngram, min_length, repetition_penalty, banned_words):
            ids, logp = ensemble_sample(self._engines(), object_features, position_features, n_samples=n_samples,
                                        temperature=temperature, top_k=top_k, seed=seed, top_p=top_p,
                                        weights=self.weights, mode=self.mode)
        host = ids.cpu().numpy()
        end = -1 if lead.end_idx is None else lead.end_idx
        logprob = sequence_logprob(ids[..., 1:logp.shape[-1] + 1], logp, end)
        return [lead.decode_captions(host[j]) for j in range(host.shape[0])], logprob

    def score_captions(self, object_features, position_features, captions, length_penalty=0.0):
        """MODEL.score_captions under the ensemble distribution ('prob' mode only): each member scores the
        captions and the per-token read-outs are combined on the device, token_logp =
        logsumexp_k(log w_k + token_logp_k), exactly 0 at pad targets; logp is its sum and score =
        logp / max(length, 1) ** length_penalty.  The dict has no 'token_accuracy': the ensemble's argmax
        cannot be derived from the members' read-outs.  mode 'logprob' raises: its normaliser needs the
        members' whole rows, which scoring never materialises."""
        if self.mode != "prob":
            raise ValueError("capgen ensemble: score_captions needs mode 'prob' (mode 'logprob' renormalises "
                             "over whole rows)")
        outs = [m.score_captions(object_features, position_features, captions) for m in self.models]
        dev = outs[0]["token_logp"].device
        tok = torch.stack([o["token_logp"].to(dev) + math.log(w) for o, w in zip(outs, self.norm_weights)])
        length = outs[0]["length"]
        kept = torch.as_tensor(captions)[..., 1:].to(dev).ne(self.leader.config.pad_idx)  # the non-pad targets
        tok = torch.where(kept, torch.logsumexp(tok, 0), torch.zeros((), device=dev))
        logp = tok.sum(-1)
        denom = length.clamp(min=1).to(torch.float32)
        return {"logp": logp, "score": logp / denom ** float(length_penalty), "token_logp": tok, "length": length}
