/* capgen — C ABI of the MI355X-native caption-generator training engine (libcapgen.so).
 *
 * Drop-in boundary.  The reference has no FFI: its boundary is the
 * Python object API of core/models.py (TRANSFORMER, models.py:81-135) over
 * core/TRANSFORMER/model.py (Transformer, model.py:8-209).  Every entry point below
 * replaces one reference call; the Python mirror (image-caption_amd/capgen) binds them
 * with ctypes and keeps the reference method names, arguments and return types.
 *
 * Conventions: all functions return 0 on success, nonzero on failure, with a
 * thread-local message from capgen_last_error().  Device pointers are plain pointers
 * into the current HIP device's memory; `stream` is a hipStream_t passed as void*
 * (NULL = default stream).  Calls on one handle are not thread-safe and are
 * asynchronous on `stream` unless stated otherwise.  The library owns weights, grads,
 * optimizer state and workspaces; the caller owns input/output buffers.
 */
#ifndef CAPGEN_H
#define CAPGEN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CAPGEN_ABI_VERSION 13

typedef struct capgen_engine capgen_t;

enum capgen_dtype { CAPGEN_F32 = 0, CAPGEN_BF16 = 1 };

/* Model/solver shape.  Field meanings follow Transformer.__init__ (model.py:10-36) and
 * core/config.py:5-62; `max_length` is the Transformer's max_length (the decoder
 * positional table has max_length-1 rows, model.py:383-396). */
typedef struct capgen_config {
  int32_t num_vocab, max_length;
  int32_t dim_features, dim_positions;                 /* ENCODE_DIM_FEATURES / _POSITIONS */
  int32_t enc_d, enc_ff, enc_blocks, enc_heads;        /* encode_input_size(=q_k=v), hidden, blocks, heads */
  int32_t dim_word_embedding;
  int32_t dec_d, dec_ff, dec_blocks, dec_heads;
  float dropout;                                       /* DROPOUT (modules.py:64,106) */
  float attention_dropout;                             /* 0.1, hard-coded at modules.py:8 */
  int32_t pad_idx;                                     /* PAD_IDX */
  int32_t encode_mask;                                 /* ENCODE_MASK (model.py:311-328) */
  int32_t focal_loss;                                  /* 'FocalLoss' in OUTPUT_NAME (model.py:73-76) */
  int32_t split_position;                              /* SPLIT_POSITION (model.py:231-233, 297-303): the
                                                          position Linear split into Linear(4, d) over
                                                          the box columns and Linear(P-4, d) over the
                                                          class columns; the same arena columns, two
                                                          table entries (position_ / object_embedding) */
  int32_t split_image_objects;                         /* SPLIT_IMAGE_OBJECTS (model.py:237-244, 258-292): an
                                                          extra EncoderBlock (encoder.image_encoder) over
                                                          every (image row, region) pair, causal + key-pad
                                                          masked; its region token + the position
                                                          embedding feed the shared encoder norm */
  int32_t move_first_image_feature;                    /* MOVE_FIRST_IMAGE_FAETURE (model.py:400-407,
                                                          451-457): after the last decoder block,
                                                          LN(x + drop(FFN(x + enc_out[:, 0]))) */
  int32_t dtype;                                       /* capgen_dtype: compute/storage of activations */
  int32_t max_batch, max_regions;                      /* workspace sizing hints */
  float lr, beta1, beta2, eps;                         /* torch.optim.Adam (models.py:111-113) */
  uint64_t seed;                                       /* dropout RNG seed */
} capgen_config;

/* One reference state_dict tensor mapped into the packed parameter arena:
 * element (r, c) of the reference tensor lives at arena[offset + r*row_stride + c]. */
typedef struct capgen_param_info {
  char name[96];
  int32_t ndim;
  int64_t rows, cols;   /* 1-D tensors: rows = 1 */
  int64_t offset, row_stride;
} capgen_param_info;

const char* capgen_last_error(void);
int capgen_abi_version(void);
/* Run-time switches (csrc/knobs.cpp): name without the CAPGEN_ prefix (e.g. "FUSED_CE").  The
 * CAPGEN_<NAME> environment sets the process default when the library first asks; this call changes
 * it afterwards (engines read theirs when created).  Non-zero status for an unknown name or a
 * debug-build-only switch in the product library.  *old (may be null) receives the previous value.
 * capgen_debug_build: 1 in libcapgen_debug.so (-DCAPGEN_DEBUG), else 0. */
int capgen_set_knob(const char* name, int value, int* old);
int capgen_debug_build(void);

/* Host-only (no device needed): the parameter table for a config.  Writes up to `cap`
 * entries, sets *count to the total; *arena_elems = arena size in f32 elements. */
int capgen_param_table(const capgen_config* cfg, capgen_param_info* out, int cap, int* count,
                       int64_t* arena_elems);

/* Transformer(...).to(DEVICE) + Adam(...)  — models.py:86-113. */
int capgen_create(const capgen_config* cfg, int device, capgen_t** out);
int capgen_destroy(capgen_t* h);

/* state_dict()/load_state_dict() (models.py:62-68) go through these synchronous host
 * copies of the whole f32 arena (layout: capgen_param_table). */
int capgen_get_params(capgen_t* h, float* host_dst, int64_t n);
int capgen_set_params(capgen_t* h, const float* host_src, int64_t n);  /* also resets nothing else */
int capgen_get_grads(capgen_t* h, float* host_dst, int64_t n);
/* Overwrite the gradient arena (e.g. gradients reduced outside the engine), then capgen_adam_step
 * applies them: the host side of a custom data-parallel reduction. */
int capgen_set_grads(capgen_t* h, const float* host_src, int64_t n);
/* Adam state: step count and exp_avg / exp_avg_sq arenas (optional checkpoint interop). */
int capgen_get_adam_state(capgen_t* h, int64_t* step, float* exp_avg, float* exp_avg_sq, int64_t n);
int capgen_set_adam_state(capgen_t* h, int64_t step, const float* exp_avg, const float* exp_avg_sq, int64_t n);
/* Device pointers of the f32 parameter / gradient arenas (for zero-copy views). */
int capgen_arenas(capgen_t* h, float** params, float** grads, int64_t* n);

/* nn.Module.train()/eval(): dropout on/off (modules.py:12,64,106). */
int capgen_set_training(capgen_t* h, int training);

/* Transformer.forward (model.py:79-98) in training state: saves activations for
 * capgen_backward.  feats [B,N,F] (feats_dtype), pos [B,N,P] f32, caps [B,T] int32, all
 * device pointers.  loss_out: device f32 scalar (NULL = internal). */
int capgen_forward(capgen_t* h, const void* feats, int feats_dtype, const float* pos, const int32_t* caps,
                   int B, int N, int T, float* loss_out, void* stream);
/* loss.backward() (models.py:125): fills the gradient arena (overwrites, = zero_grad + backward). */
int capgen_backward(capgen_t* h, void* stream);
/* optimizer.step() (models.py:126). */
int capgen_adam_step(capgen_t* h, void* stream);
/* TRANSFORMER.train_step (models.py:115-126): forward + backward (+ DP gradient
 * all-reduce) + Adam, replayed from a captured hipGraph after the first call with a
 * given (shape, pointers). */
int capgen_train_step(capgen_t* h, const void* feats, int feats_dtype, const float* pos, const int32_t* caps,
                      int B, int N, int T, float* loss_out, void* stream);
int capgen_set_graph(capgen_t* h, int enable);
/* Run-time optimizer control (warm-up / decay schedules, the drop from the cross-entropy rate to the
 * self-critical one, gradient clipping).  Off by default: without these calls a step's launches, streams,
 * RCCL call sequence, captured graphs and arithmetic are unchanged.
 * capgen_set_lr: the Adam learning rate (finite, >= 0; capgen_config.lr until the first call) of every
 * update issued after the call and of none issued before.  The value lives in a device word written by an
 * ordered asynchronous copy, so a replayed step graph picks it up without re-capture (graph keys do not
 * change).  capgen_get_lr: the value last set (host side, no synchronisation).
 * capgen_set_grad_clip: torch.nn.utils.clip_grad_norm_(parameters, max_norm) (L2, error_if_nonfinite=False)
 * before every Adam update: 0 = off (default), finite > 0 clips, +inf only measures the norm (the
 * coefficient is exactly 1); negative or NaN fails.  The norm is the global L2 norm of the step's
 * gradients -- under data parallel of the summed gradients, one 8-byte all-reduce per step on the bucket
 * stream -- accumulated in double in a fixed order, so equal gradients give equal coefficients on every
 * rank and run.  In a train step every bucket's Adam then runs after the step's last bucket
 * (capgen_train_step, _indexed, _weighted, capgen_rl_finish); capgen_adam_step clips over the whole
 * arena.  Switching between off and on drops the captured whole-step graph (not the forward graph); a new
 * value while on is read by the replay.
 * capgen_last_grad_norm (synchronous): the norm, before clipping, of the most recent update issued with
 * clipping or measuring on, into the HOST float *host_out; fails if there was none.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_set_lr(capgen_t* h, float lr);
int capgen_get_lr(capgen_t* h, float* lr);
int capgen_set_grad_clip(capgen_t* h, float max_norm);
int capgen_last_grad_norm(capgen_t* h, float* host_out);
/* Decoupled weight decay (torch.optim.AdamW) and an exponential moving average of the parameters
 * (torch.optim.swa_utils.AveragedModel with get_ema_multi_avg_fn(decay)), both inside the update kernel and
 * both off by default: an engine that never calls these launches what it launched before and allocates
 * nothing more.  Each combines with capgen_set_grad_clip and runs in every update (capgen_train_step,
 * _indexed, _weighted, capgen_rl_finish, capgen_adam_step; under ZeRO-1 on this rank's chunks).
 * Switching either between off and on drops the captured whole-step graph (not the forward graph); a
 * new value while on lives in a device word and is read by the replay.
 * capgen_set_weight_decay: p *= 1 - lr * wd before the Adam update of the same step, with the learning rate
 * of that step; the factor is computed in double on the device and rounded once.  Decay covers every
 * element of the arena (torch.optim.AdamW over all parameters); padding elements have zero parameter and
 * zero gradient, so they stay zero.
 * capgen_set_ema: after each update e += (p_new - e) * (1 - decay).  off -> on: the average becomes a copy
 * of the current parameters and n_updates = 0 (AveragedModel's first update); the arena (one more f32
 * arena) is allocated at the first enable.  on -> on: only the decay changes.  -> off: updating stops and
 * the arena stays readable.  capgen_dp_init, which replaces the parameters by rank 0's,
 * restarts an enabled average in the same way (a copy of them, n_updates = 0).  n_updates counts the updates issued while the average is on: a host counter,
 * and graph replays count.  capgen_set_params while on and not swapped leaves the average alone.
 * capgen_ema_info: the decay (0 = off), n_updates and whether the average is swapped in.
 * capgen_get_ema (synchronous; fails only if the average was never enabled or on a size mismatch): the
 * average's arena, laid out as the parameters.  It never refuses for staleness: after sharded (ZeRO-1)
 * steps it holds this rank's chunks only until capgen_dp_sync_adam_state, which all-gathers the average
 * too while it is on (as capgen_get_params under capgen_dp_debug_shard).
 * capgen_set_ema_state: overwrite the arena and the counter of an enabled average (checkpoint restore).
 * capgen_ema_swap: exchange the parameters and the average in place and rebuild the bf16 shadow and the
 * weight tiles, so that forward, capgen_compute_loss, capgen_score_captions and every decoder run on the
 * averaged weights and capgen_get_params returns them; a second call swaps back.  No pointer moves:
 * cached graphs stay valid.  While swapped, every call that would update parameters fails before it
 * launches anything, naming capgen_ema_swap: capgen_train_step, _indexed, _weighted (train != 0),
 * capgen_rl_finish (train != 0), capgen_adam_step, capgen_set_params, capgen_set_adam_state,
 * capgen_dp_init; capgen_set_ema may then change the decay only.  capgen_ema_swap fails while the average
 * is off or was never enabled, and at world > 1 while this rank's average is stale (call
 * capgen_dp_sync_adam_state on every rank first).
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_set_weight_decay(capgen_t* h, float wd);  /* finite, >= 0; 0 = off (default) */
int capgen_set_ema(capgen_t* h, float decay);        /* 0 = off (default), else in (0, 1) */
int capgen_ema_info(capgen_t* h, float* decay, int64_t* n_updates, int* swapped);  /* any pointer may be null */
int capgen_get_ema(capgen_t* h, float* host_dst, int64_t n);
int capgen_set_ema_state(capgen_t* h, const float* host_src, int64_t n, int64_t n_updates);
int capgen_ema_swap(capgen_t* h);
/* TRANSFORMER.compute_loss (models.py:128-135): forward under no_grad. */
int capgen_compute_loss(capgen_t* h, const void* feats, int feats_dtype, const float* pos, const int32_t* caps,
                        int B, int N, int T, float* loss_out, void* stream);
/* Logits of the last forward/compute_loss, [B*(T-1), V] f32 device copy (test hook). */
int capgen_copy_logits(capgen_t* h, float* dst, int64_t n, void* stream);

/* Transformer.generate_caption_vector (model.py:101-132): greedy decode, bit-identical
 * to the reference's full-prefix recompute but KV-cached.  ids_out: [B, max_length+1]
 * int64 device; attn_out (nullable): [max_length-1, B, N] f32 device (attention_list). */
int capgen_greedy(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N,
                  int64_t* ids_out, float* attn_out, void* stream);
/* Transformer.beam_search (model.py:135-200): ids_out [B, max_length] int64 device. */
int capgen_beam(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N, int beam_size,
                int64_t* ids_out, void* stream);

/* The standard beam search: capgen_beam's loop (one encoder pass, KV-cached, the same launch sequence) with
 * <END> honoured.  A hypothesis is live until it emits end_id (-1: nothing ever finishes); a live hypothesis
 * offers logp + log-softmax of its logits for every word (always the log-softmax, whatever
 * capgen_set_decode_log_softmax says), a finished one offers itself once with its logp frozen and gets
 * token 0 appended; the beam_size best survive under (logp descending, flat index ascending).  At the end
 * score = logp when length_penalty == 0, else logp / max(len, 1)^length_penalty, with len the tokens
 * emitted while live (<END> included; max_length - 1 for a hypothesis that never finished), and the n_best
 * per image under (score descending, beam ascending) come back.  Pruning during the search uses the raw
 * logp; finished rows still run through the decoder; there is no early exit.  Definition: csrc/select.hip.
 * beam_size in [1, min(16, num_vocab)], n_best in [1, beam_size], end_id in [-1, num_vocab),
 * length_penalty finite and >= 0, N in [1, 64].  All outputs on the device.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_beam_nbest(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N,
                      int beam_size, int end_id, float length_penalty, int n_best,
                      int64_t* ids_out,   /* [n_best*B, max_length], row j*B+b = j-th best of image b, col 0 = <START> */
                      float* score_out,   /* [n_best*B] final score, nullable */
                      float* logp_out,    /* [n_best*B] raw log-probability, nullable */
                      int32_t* len_out,   /* [n_best*B], nullable */
                      void* stream);

/* Diverse beam search (Vijayakumar et al. 2016): capgen_beam_nbest with the beam_size beams split into
 * num_groups groups of k' = beam_size / num_groups, group g being beams g k' .. (g + 1) k' - 1.  At every
 * position the groups of an image are served in order; group g selects its k' best among its own k' source
 * rows' candidates (at step 0: beam 0's), a live source's candidate for word v scored logp + log-softmax[v] -
 * diversity_penalty * c(v), c(v) = the hypotheses the earlier groups selected at this position from a live
 * source with word v (<END> counts like any word); a finished source offers itself once, unpenalised.  The
 * penalty only orders candidates: logp stays the sum of the model's token log-probabilities.  At the end each
 * group returns its n_best by logp / max(len, 1)^length_penalty: output row (g * n_best + rank) * B + b.
 * num_groups = 1 is capgen_beam_nbest bit for bit (the same launches) whatever diversity_penalty;
 * diversity_penalty = 0 gives num_groups identical groups.  Decode constraints apply as to capgen_beam_nbest.
 * Either dtype selects with the full-row top-k, one group-merge launch and the three reorder launches per
 * token.  Definition: csrc/select.hip.
 * num_groups in [1, beam_size] and dividing it, diversity_penalty finite and >= 0, n_best in
 * [1, beam_size / num_groups], the rest as capgen_beam_nbest.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_beam_diverse(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N,
                        int beam_size, int num_groups, float diversity_penalty, int end_id, float length_penalty,
                        int n_best,
                        int64_t* ids_out,   /* [num_groups*n_best*B, max_length], group-major */
                        float* score_out,   /* [num_groups*n_best*B], nullable */
                        float* logp_out,    /* [num_groups*n_best*B], nullable */
                        int32_t* len_out,   /* [num_groups*n_best*B], nullable */
                        void* stream);

/* Forced-word beam search (constrained beam search, Anderson et al. 2017; the fixed-beam bank form of Post &
 * Vilar 2018 / Hu et al. 2019): capgen_beam_nbest over captions that must contain given words.  Image i has W
 * slots (word[i * W + s], group[i * W + s]); word = -1 is an empty slot, a group (in [0, 16)) is a set of
 * alternative words and is met once the hypothesis has appended any of them; a word may sit in several groups.
 * Every hypothesis carries met, the bitmask of the groups it has met.  A live hypothesis may not append <END>
 * while a group of its image is unmet.  At every position the candidates fall into banks by popcount(met') and
 * are ranked within their bank by (score descending, flat index ascending); the k first under (rank ascending,
 * bank descending) are kept: the best of the highest non-empty bank, the best of the next, ..., then the second
 * best of each.  Scores are never compared across banks, and logp stays the sum of the model's token
 * log-probabilities.  At the end the n_best per image under (popcount(met) descending, logp / max(len, 1)^
 * length_penalty descending, beam ascending) come back, with met in met_out: nothing is forced as max_length
 * approaches, so a returned hypothesis may have groups unmet -- met says which.  Decode constraints apply as to
 * capgen_beam_nbest.  Either dtype selects with the full-row top-k, one bank-merge launch and the three reorder
 * launches per token.  Definition: csrc/select.hip.
 * W = 0 (word / group unread) is capgen_beam_nbest bit for bit (the same launches), met_out zeroed.  Else
 * beam_size + W <= 15 and beam_size + W + 1 <= num_vocab; word in [0, num_vocab) or -1, and not end_id, 0 or 1
 * (the caller's rule: the arrays are on the device and are not read by the host; a slot out of range is taken
 * as empty); the rest as capgen_beam_nbest.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_beam_forced(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N,
                       int beam_size, int end_id, float length_penalty, int n_best,
                       const int32_t* word,   /* device [B, W] */
                       const int32_t* group,  /* device [B, W] */
                       int W,
                       int64_t* ids_out,   /* [n_best*B, max_length] */
                       float* score_out,   /* [n_best*B], nullable */
                       float* logp_out,    /* [n_best*B], nullable */
                       int32_t* len_out,   /* [n_best*B], nullable */
                       int32_t* met_out,   /* [n_best*B], nullable */
                       void* stream);

/* Sampled decoding: n_samples captions per image drawn from the model's distribution, one encoder
 * pass, KV-cached.  Position t draws token ~ softmax(logits / temperature) restricted to the top_k
 * largest logits (top_k = 0: the whole vocabulary) by Gumbel-max over the counter hash of (seed,
 * site 0x5A00 + t, row * num_vocab + column): a (seed, inputs, weights) triple names one result.
 * Tokens are drawn to the end (<END> is not special, as in capgen_greedy); capgen_set_decode_log_softmax
 * has no effect.  ids_out: [n_samples * B, max_length + 1] int64 device, laid out as capgen_greedy's
 * (<START> in column 0, last column 0), row j * B + b = sample j of image b; logp_out (nullable):
 * [n_samples * B, max_length - 1] f32 device, each token's log-probability under the distribution it
 * was drawn from (0 for top_k = 1).  n_samples in [1, 16], temperature > 0 and finite, top_k in
 * [0, min(16, num_vocab)], N in [1, 64], n_samples * B * num_vocab < 2^32. */
int capgen_sample(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N, int n_samples,
                  float temperature, int top_k, uint64_t seed, int64_t* ids_out, float* logp_out, void* stream);
/* capgen_sample with nucleus (top-p) truncation (Holtzman et al. 2020): position t draws from the
 * candidates of capgen_sample (the top_k largest logits, or all) cut to the columns whose strictly more
 * likely columns hold less than top_p of their softmax mass -- the smallest set of most likely words
 * that reaches top_p, ties kept whole -- and renormalised; logp_out is the log-probability under that
 * distribution (0 where one word is left).  Same noise, counters and sites as capgen_sample: a draw is
 * the untruncated draw whenever that lies in the nucleus.  top_p in (0, 1]; top_p = 1 is capgen_sample,
 * bit for bit (the same kernels).  Everything else as capgen_sample.  Definition: csrc/select.hip.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_sample_nucleus(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int B, int N,
                          int n_samples, float temperature, int top_k, float top_p, uint64_t seed, int64_t* ids_out,
                          float* logp_out, void* stream);

/* Decode constraints of capgen_beam_nbest and capgen_sample / capgen_sample_nucleus: before every step's
 * selection the row's logits are edited from its own emitted tokens e (everything after <START>), in this
 * order: (1) repetition_penalty theta: every distinct word w of e gets z[w] / theta if z[w] > 0, else
 * z[w] * theta, once; (2) every banned word gets -inf; (3) min_length m: end_id gets -inf while the caption
 * would end with fewer than m tokens (<END> included); (4) no_repeat_ngram n: every word that would complete
 * an n-gram already in e gets -inf (n = 1: every emitted word).  A blocked word has probability exactly 0;
 * softmax, log-softmax, top-k, nucleus mass and logp_out are taken over what is left.  One more launch per
 * step while any constraint is on, none otherwise; capgen_greedy and capgen_beam (the reference's decoders)
 * are never constrained.  Finished beam hypotheses are not affected; capgen_sample keeps drawing (and
 * blocking) after <END>.  Constraints make sampled roll-outs off-policy: the trainers leave them off.
 * Definition: csrc/select.hip.
 * The setter copies the struct and the banned list; NULL switches every constraint off (the default).  It
 * fails, naming the argument, outside the ranges below and unless num_vocab - n_banned - max_length >= 16
 * (every row keeps at least 16 finite logits, the most a selection takes).  capgen_beam_nbest fails while
 * min_length > 0 and the struct's end_id differs from its own.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
typedef struct capgen_decode_constraints {
  int32_t no_repeat_ngram;     /* 0 = off, else in [1, max_length) */
  int32_t min_length;          /* 0 = off, else in [1, max_length - 1]; needs end_id */
  int32_t end_id;              /* [-1, num_vocab) */
  float   repetition_penalty;  /* finite, > 0; 1 = off */
  const int32_t* banned;       /* HOST array, copied by the call */
  int32_t n_banned;            /* [0, 1024], every id in [0, num_vocab) */
} capgen_decode_constraints;
int capgen_set_decode_constraints(capgen_t* h, const capgen_decode_constraints* c);

/* Ensemble decoding: one search, or one set of draws, over the averaged next-word distribution of several
 * engines (seeds, cross-entropy and self-critical checkpoints, raw and averaged weights).  Member 0 leads:
 * it owns the hypotheses, the selection state, the decode constraints (the other members' are ignored) and
 * the outputs, and the call runs on its stream.  At every position each member runs its own decoder step --
 * own weights, encoder output and K/V cache -- on the leader's token histories, giving l_k = log-softmax of
 * member k's logits; one launch writes over the leader's logits
 *   CAPGEN_ENS_PROB:    y[v] = log sum_k w_k exp(l_k[v])   (finite even where every exp underflows in f32)
 *   CAPGEN_ENS_LOGPROB: y[v] = sum_k w_k l_k[v]            (the selection's own log-softmax normalises it)
 * and the constraints and the selection of the single-engine call read y as that step's logits; returned
 * scores and log-probabilities are the ensemble distribution's.  weights: HOST, n_members values, finite
 * and > 0, normalised to sum 1 in double and rounded to f32 once; NULL: equal.  n_members in [1, 8]; the
 * members are distinct engines on one device with equal num_vocab, max_length, pad_idx, dim_features and
 * dim_positions (depth, width and dtype may differ); a call that breaks a rule fails before anything is
 * launched, naming the member and the field.  With one member both modes are the single engine's call up
 * to f32 rounding.  The remaining arguments, their ranges and the output layouts are those of
 * capgen_beam_nbest / capgen_sample_nucleus after h.  Definition: csrc/select.hip (ensemble_combine).
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
enum { CAPGEN_ENS_PROB = 0, CAPGEN_ENS_LOGPROB = 1 };
typedef struct capgen_ensemble {
  capgen_t* const* members;  /* members[0] leads */
  int32_t n_members;
  const float* weights;      /* HOST, nullable */
  int32_t mode;
} capgen_ensemble;
int capgen_ensemble_beam_nbest(const capgen_ensemble* e, const void* feats, int feats_dtype, const float* pos, int B,
                               int N, int beam_size, int end_id, float length_penalty, int n_best, int64_t* ids_out,
                               float* score_out, float* logp_out, int32_t* len_out, void* stream);
int capgen_ensemble_sample(const capgen_ensemble* e, const void* feats, int feats_dtype, const float* pos, int B, int N,
                           int n_samples, float temperature, int top_k, float top_p, uint64_t seed, int64_t* ids_out,
                           float* logp_out, void* stream);
/* capgen_beam_diverse over the ensemble's distribution: its arguments after h.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_ensemble_beam_diverse(const capgen_ensemble* e, const void* feats, int feats_dtype, const float* pos, int B,
                                 int N, int beam_size, int num_groups, float diversity_penalty, int end_id,
                                 float length_penalty, int n_best, int64_t* ids_out, float* score_out,
                                 float* logp_out, int32_t* len_out, void* stream);

/* capgen_beam_forced over the ensemble's distribution: its arguments after h.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_ensemble_beam_forced(const capgen_ensemble* e, const void* feats, int feats_dtype, const float* pos, int B,
                                int N, int beam_size, int end_id, float length_penalty, int n_best, const int32_t* word,
                                const int32_t* group, int W, int64_t* ids_out, float* score_out, float* logp_out,
                                int32_t* len_out, int32_t* met_out, void* stream);

/* Decode scoring of capgen_greedy / capgen_beam: 0 (default) = Transformer (argmax of Softmax,
 * beams accumulate probabilities, model.py:124-128,183); 1 = PolicyNetwork, the SCST model
 * (argmax of LogSoftmax, beams accumulate log-probabilities, model_RL.py:72,126-127,157,182). */
int capgen_set_decode_log_softmax(capgen_t* h, int enable);

/* Reset the device-side dropout RNG state (test hook: replays a dropout mask). */
int capgen_set_rng_seed(capgen_t* h, uint64_t seed);
/* Kernel test hook: C[M,N] = alpha*opA.opB (+bias)(relu) (+C if beta) with the engine's GEMM.
 * ta: A stored [K][M]; tb: B stored [K][N] (else [N][K]).  in/out dtypes: capgen_dtype. */
int capgen_debug_gemm(int M, int N, int K, const void* A, int64_t lda, int ta, const void* B, int64_t ldb, int tb,
                      void* C, int64_t ldc, int in_dtype, int out_dtype, const float* bias, float alpha, int beta,
                      int relu, void* stream);

/* Kernel test hook for the register-B GEMM (gemm_breg.hip, the bf16 decode step's Linears): writes
 * B's MFMA fragment pieces into Bt (N * K bf16; B stored [K][N] if tb else [N][K]), then
 * C[M,N] = A[M,K] . B (+bias)(relu)(zeroed where aux <= 0)(+C if beta) on that kernel; fails if the
 * shape / epilogue is one the kernel does not take (N % 64, K % 256 -- K % 128 at N >= 1536, M >= 1024). */
int capgen_debug_gemm_tiled(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, int tb,
                            void* Bt, void* C, int64_t ldc, int out_dtype, const float* bias, int beta, int relu,
                            const void* aux, int64_t ldaux, void* stream);

/* Kernel test hook for the register-B GEMM with the decode step's folded LayerNorm (K = 512): as
 * capgen_debug_gemm_tiled (tb = 0) with LayerNorm inputs v = A (+ ln_res if non-null; both [M][512]
 * bf16); the kernel multiplies y = ((v - mean) * rstd * ln_gamma + ln_beta) * keep (eps 1e-6; keep = 0
 * for rows m with ln_ids[m * ln_ids_ld] == ln_pad when ln_ids is non-null) and also stores y into ln_y
 * ([M][512] bf16). */
int capgen_debug_gemm_tiled_ln(int M, int N, const void* A, const void* ln_res, const void* B, void* Bt, void* C,
                               int out_dtype, const float* bias, int beta, int relu, const float* ln_gamma,
                               const float* ln_beta, void* ln_y, const int32_t* ln_ids, int64_t ln_ids_ld, int ln_pad,
                               void* stream);

/* Experiment hook: force a GEMM tile/wave/pipeline variant (0 = production heuristic). */
int capgen_debug_gemm_variant(int variant);
/* Diagnostic hook: the in-launch split-K combine's hand-off protocol (0 = the production form:
 * sc1 slab stores, agent acquire + plain slab loads in the combining workgroup, tickets re-armed
 * by the last arriver's atomic exchange).  Bits: 1 adds a writer release fence, 2 drops the
 * reader acquire, 4 reads the slabs with sc1 loads, 8 zeroes the tickets with a memset before
 * every launch, 16 re-arms tickets with a relaxed atomic store (round 1 = 2|4|16;
 * tools/splitk_stress.py, tools/step_det_probe.py). */
int capgen_debug_splitk_protocol(int proto);
/* Diagnostic: split-K hand-off counters collected under protocol bit 64 (out4[0] = tickets found
 * out of range at arrival, out4[1] = tiles combined); synchronises the device; reset != 0 zeroes. */
int capgen_debug_splitk_diag(int* out4, int reset);
/* Diagnostic (GEMM ablation build only, protocol bit 4096): device buffer (>= 88 u64) that block 0 of
 * the next GEMM launches fills with per-phase s_memtime / s_memrealtime stamps (gemm_bf16.hip ABL_T). */
int capgen_debug_gemm_timing_buf(void* dev_buf);
/* Diagnostic: synchronous copy of an internal buffer to host: 0 tmp, 1 gOut, 2 gRes, 3 cross-K/V
 * gradient, 4-7 the last encoder block's FFN-hidden / FFN-LN / MHA-LN / QKV gradients; 32 + 8 l + j
 * encoder block l's gAf / gH / gA1 / gATT1 / gQKV; 80 + l the encoder activations X[l]; 128 + 8 l + j
 * encoder block l's saved forward tensors (att, v1, m1, r1, Y, v2, m2, r2); 200 + l / 216 + l the
 * encoder / decoder block l's FFN hidden activations (relu output, the backward's ReLU mask). */
int capgen_debug_copy_buffer(capgen_t* h, int which, void* host_dst, int64_t bytes);

/* Training step over an HBM-resident feature store (replaces TrainDataset.__getitem__ + the
 * DataLoader collate + `.to(DEVICE)`, dataset.py:12-18, main.py:37-43, models.py:120-122):
 * feat_store [n_images, N, F] and pos_store [n_images, N, P] stay on the device (a COCO split in
 * bf16 is ~17 GB); img_idx [B] (device int32) selects each caption's image, gathered inside the
 * encoder-input pack kernel; caps [B, T] device int32.  Otherwise as capgen_train_step. */
int capgen_train_step_indexed(capgen_t* h, const void* feat_store, int feats_dtype, const float* pos_store,
                              int n_images, const int32_t* img_idx, const int32_t* caps, int B, int N, int T,
                              float* loss_out, void* stream);

/* Teacher-forced step whose cross entropy is weighted per caption:
 *   loss = sum_b w_b sum_t [tgt_bt != pad] (lse_bt - logit_bt[tgt_bt]) / count,
 * count = the number of non-pad targets (the global number under data parallel), exactly as in
 * capgen_train_step.  With w_b = the advantage of a sampled caption this is the self-critical policy
 * gradient loss over roll-outs (capgen_sample / capgen_greedy ids, scored by capgen_scst_rewards); other
 * weights give example weighting.  weights: [B] f32 on the device, one per caption row, any sign, required;
 * the weight enters the two row-wise CE kernels, so the bf16 step keeps the fused classifier + CE (no
 * logits are written).  img_idx non-null: feats / pos are [n_images, N, .] stores and row b reads image
 * img_idx[b] (capgen_train_step_indexed: n B roll-outs share B images without a copy); img_idx null:
 * feats / pos are [B, N, .] and n_images is ignored.  train != 0: forward, backward and Adam, through every
 * route of capgen_train_step (forward graph, capgen_set_graph, data parallel -- the same RCCL call
 * sequence); the weights pointer is part of the graph key: a new pointer re-captures, new values behind
 * the same pointer are read by the replay.  train == 0: the weighted loss only (no gradient, parameter or
 * Adam-state change; dropout follows capgen_set_training).  Fails when the config has focal_loss (it
 * transforms an unweighted mean) or weights is null.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_train_step_weighted(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int n_images,
                               const int32_t* img_idx, const int32_t* caps, const float* weights, int B, int N,
                               int T, float* loss_out, int train, void* stream);

/* Score given captions: the teacher-forced forward of capgen_train_step over R caption rows caps [R, T]
 * (int32), read out as log-probabilities under the model in place of a loss.  Targets are caps[:, 1:];
 * with pad = pad_idx, Lq = T - 1 and row m = r Lq + t:
 *   token_logp[r, t] = logit[m, tgt] - logsumexp(logit[m, :]), exactly 0 where tgt == pad   ([R, T-1] f32, or null)
 *   logp[r]   = sum_t token_logp[r, t], added in a fixed order                              ([R] f32, required)
 *   length[r] = #{t : tgt != pad}                                                           ([R] int32, or null)
 *   hits[r]   = #{t : tgt != pad and the target's logit is >= every logit of the row}        ([R] int32, or null)
 * (the target is then the teacher-forced argmax; ties count).  A caption of pads only gives 0, 0, 0.
 * img_idx non-null: feats / pos are [n_images, N, .] stores and row r reads image img_idx[r] (n candidates
 * of one image share its features); img_idx null: feats / pos are [R, N, .] and n_images is ignored.
 * Temperature 1, never constrained (no decode-constraint state is read or cleared).  Dropout is never
 * applied and the dropout seed does not advance, whatever capgen_set_training says; no parameter, gradient,
 * Adam state, gradient scale or loss word is written, and the cached step graphs stay valid (the call runs
 * eagerly; it re-allocates the activations, as every call does, only when R, N or T exceed every earlier
 * shape).  Under data parallel the call is rank-local and issues no collective.  focal_loss configs are
 * scored like any other (the transform belongs to the loss).  Two calls give the same bits.
 * Added without a change of CAPGEN_ABI_VERSION: no existing entry changed (backward compatible). */
int capgen_score_captions(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int n_images,
                          const int32_t* img_idx, const int32_t* caps, int R, int N, int T, float* token_logp,
                          float* logp, int32_t* length, int32_t* hits, void* stream);

/* Self-critical sequence training (SelfCriticNetwork, models.py:137-211), in two calls with the
 * host scoring the samples in between (CIDEr-D / BLEU, capgen/scst.py):
 *  capgen_rl_sample  replaces PolicyNetwork.forward + .sample (model_RL.py:75-97) and the entropy
 *                    of StructureCriterion (loss.py:123-127): teacher-forced forward (dropout as
 *                    set by capgen_set_training), sample = argmax log_softmax [B, T-1] (int64),
 *                    per-image masked mean entropy [B] and the CrossEntropy LM loss [1];
 *  capgen_rl_finish  replaces ReinforcementLearningLoss.forward (loss.py:53-76, 131-152) and, when
 *                    train != 0, loss.backward() + Adam.step() (models.py:191-195).  scores [B]
 *                    (device) = per-image total score (cider_w*CIDEr-D + bleu_w*BLEU-4 +
 *                    entropy_w*entropy + self_cider_w*self-CIDEr); loss_out [3] (device) =
 *                    {loss, language_model_loss, structure_loss}.  Under DP, sum(mask) and the
 *                    structure numerator are all-reduced (global mean as in one process). */
int capgen_rl_sample(capgen_t* h, const void* feats, int feats_dtype, const float* pos, const int32_t* caps, int B,
                     int N, int T, int64_t* sample_out, float* entropy_out, float* lm_loss_out, void* stream);
int capgen_rl_finish(capgen_t* h, const float* scores, float structure_loss_weight, float* loss_out, int train,
                     void* stream);

/* Host rewards for self-critical training, natively (StructureCriterion.get_scores,
 * loss.py:154-181, as restated by capgen/scst.py): out[b] = cider_w * CIDEr-D(sample_b | target_b)
 * + bleu_w * BLEU-4(sample_b | target_b), CIDEr-D with document frequencies from the B targets
 * (coco-caption 'corpus' mode, sigma 6, x10), per-sentence BLEU-4 with coco-caption smoothing.
 * target / sample: host int64 [B][L] token ids (row strides target_ld / sample_ld), read as
 * decode_captions does (core/utils.py:67-103): <START> at t = 0 skipped, <END> ends the sentence
 * as the token dot_id ("."; pass -1 when the vocabulary has no "." word), <NULL> dropped.
 * Pure host code: no device, no handle. */
int capgen_scst_rewards(const int64_t* target, int64_t target_ld, const int64_t* sample, int64_t sample_ld, int B,
                        int L, int start_id, int end_id, int null_id, int64_t dot_id, double cider_w, double bleu_w,
                        double* out);

/* Test hook: one masked multi-head attention forward (+ backward when dout != NULL) on packed
 * [B, L, H*dk] tensors (row stride H*dk), dtype 0 = f32, 1 = bf16 (the kernels the engine uses
 * for modules.py:16-27 ScaledDotProductAttention).  key_valid: optional [B][Lk] bytes (0 =
 * masked key); causal masks keys j > i.  probs: optional [B,H,Lq,Lk] f32 output. */
int capgen_debug_attention(int dtype, int B, int H, int Lq, int Lk, int dk, const void* q, const void* k,
                           const void* v, const unsigned char* key_valid, int causal, float temperature, void* o,
                           float* probs, const void* dout, void* dq, void* dk_, void* dv, void* stream);

/* Test hook: one attention launch in any geometry the engine uses (csrc/attention.h AttnGeom, field by
 * field but for its scheduling members): row (b, i) of head h lives at base + b*bs + i*ld + h*dk (elements
 * of dtype); dq / dk / dv mirror q / k / v, dout mirrors o.  kv_bmod > 0: K / V / key_valid of query batch
 * b come from batch b % kv_bmod.  kv_row (Lq = 1 or the VALU forward): key j of batch b is stored in batch
 * kv_row[b*kv_row_ld + j], an absolute row of the K / V buffer.  Masks: key_valid[b*kv_bs + j] == 0,
 * key_ids[b*kid_bs + j] == pad_idx, causal keys j > q_pos0 + i.  drop_p <= 0 = no dropout, else as the
 * LayerNorm hooks below (element index ((b*H + h)*Lq + i)*Lk + j).  tests/test_gpu_attention.py compares
 * every kernel this reaches with the float64 restatement tests/attention_ref.py. */
typedef struct capgen_attn_geom {
  int32_t B, H, Lq, Lk, dk;
  const void* q; int64_t q_ld, q_bs;
  const void* k; int64_t k_ld, k_bs;
  const void* v; int64_t v_ld, v_bs;
  int64_t o_ld, o_bs;
  int32_t kv_bmod;
  const int32_t* kv_row; int64_t kv_row_ld;
  const unsigned char* key_valid; int64_t kv_bs;
  const int32_t* key_ids; int64_t kid_bs; int32_t pad_idx;
  int32_t causal, q_pos0;
  float temperature;
  float drop_p; int32_t drop_site; uint64_t drop_seed;
} capgen_attn_geom_t;
/* attention_fwd into o (and probs [B,H,Lq,Lk] f32, pre-dropout, optional), then attention_bwd when
 * dout != NULL (no kv_row / kv_bmod there; the f32 and head-size != 64 backward reads probs).  A backward
 * the launcher refuses (its LDS need over 160 KB) is an error before anything is launched. */
int capgen_debug_attention_geom(int dtype, const capgen_attn_geom_t* g, void* o, float* probs, const void* dout,
                                void* dq, void* dk, void* dv, void* stream);
/* out[b*Lk + j] = mean over heads of probs[b, :, row, j] (attention_head_mean). */
int capgen_debug_attention_head_mean(const float* probs, int B, int H, int Lq, int Lk, int row, float* out,
                                     void* stream);

/* The three hooks of the fused fronts below take the attention dropout as the LayerNorm hooks do:
 * drop_p <= 0 = off, else drop_seed goes to a device word for the launch.  (These test hooks gained the
 * three arguments without a change of CAPGEN_ABI_VERSION: no entry outside the test hooks changed.) */

/* Test hook: the fused self-attention front (qkv_attn.hip; modules.py:67-76 then 16-27), bf16:
 * qkv [B*L, 3*H*64] = X [B*L, H*64] . W^T (W = [q; k; v] weights [3*H*64, H*64]), then the masked
 * attention of every (image, head) into o [B*L, H*64].  key_valid [B][L] bytes / key_ids [B][L]
 * int32 (== pad_idx: masked) optional; causal masks keys j > i.  Head size 64, H*64 = 512 only. */
int capgen_debug_qkv_attention(int B, int L, int H, const void* X, const void* W, void* qkv, void* o,
                               const unsigned char* key_valid, const int32_t* key_ids, int pad_idx, int causal,
                               float drop_p, int drop_site, uint64_t drop_seed, void* stream);

/* Test hook: the fused cross-attention front (qkv_attn.hip cross mode; modules.py:195-197), bf16:
 * q [B*Lq, H*64] = X . Wq^T, then attention over K / V = KV [B*Lk, 2*H*64] (k | v per row) with the
 * key mask key_valid [B][Lk] (optional) into o [B*Lq, H*64].  Head size 64, H*64 = 512 only. */
int capgen_debug_cross_attention(int B, int Lq, int Lk, int H, const void* X, const void* Wq, const void* KV, void* q,
                                 void* o, const unsigned char* key_valid, float drop_p, int drop_site,
                                 uint64_t drop_seed, void* stream);

/* Test hook: the fused output side of an attention block's backward (qkv_attn.hip qkv_attn_bwd;
 * modules.py:77 o_linear + 16-27), bf16: dO = dA . Wo (dA [B*Lq, 512], Wo [512, 512] nn.Linear), then
 * the masked attention backward over packed q [B*Lq, 512], k / v [B*Lk, 512] (key_valid [B][Lk]
 * optional, causal) into dq / dk / dv.  Head size 64, H * 64 = 512. */
int capgen_debug_attention_bwd_wo(int B, int Lq, int Lk, int H, const void* q, const void* k, const void* v,
                                  const unsigned char* key_valid, int causal, const void* dA, const void* Wo, void* dq,
                                  void* dk, void* dv, float drop_p, int drop_site, uint64_t drop_seed, void* stream);

/* Test hooks: the row-wise, loss, optimizer, selection and SCST launchers (csrc/ops.h, csrc/select.h, csrc/rl.h),
 * one launcher per call on raw device pointers and the given stream; the arguments are the
 * launcher's own (see the formula comments there), optional pointers may be NULL, dtype 0 = f32,
 * 1 = bf16.  tests/test_gpu_rowops.py compares each with a float64 restatement.
 * layernorm_fwd: y = LN(drop(a + a_bias) + res + pe[m % pe_L]) * rowmask; v_save = the LN input;
 * drop_p <= 0 = no dropout, else the hook places drop_seed in a device word for the launch (and
 * waits for the launch before it frees the word).  Row mask: ids[m * ids_ld] == pad_idx or
 * valid[m] == 0 zero row m.
 * layernorm_bwd: d_res = grad wrt the LN input, d_a = that through the same dropout; dgamma / dbeta
 * / dbias (column sum of d_a) are ACCUMULATED, workgroup w into stripe (w % stripes) * stripe_stride. */
int capgen_debug_layernorm_fwd(int dtype, int M, int d, const void* a, const float* a_bias, float drop_p,
                               int drop_site, uint64_t drop_seed, const void* res, const float* pe, int pe_L,
                               const float* gamma, const float* beta, const int32_t* ids, int64_t ids_ld, int pad_idx,
                               const unsigned char* valid, void* y, void* v_save, float* mean, float* rstd,
                               void* stream);
int capgen_debug_layernorm_bwd(int dtype, int M, int d, const void* dy, const void* v, const float* mean,
                               const float* rstd, const float* gamma, const int32_t* ids, int64_t ids_ld, int pad_idx,
                               const unsigned char* valid, float drop_p, int drop_site, uint64_t drop_seed,
                               void* d_res, void* d_a, float* dgamma, float* dbeta, float* dbias, int stripes,
                               int64_t stripe_stride, void* stream);
/* db[s][n] += alpha (* *alpha_ptr) * sum_m X[m][n] (row stride ldx), rows spread over `stripes`
 * partial sums stripe_stride floats apart; stripe_reduce: dst[i] (+)= sum_s S[s * stride + i],
 * clear = zero the partials as they are read. */
int capgen_debug_column_sum(int dtype, const void* X, int M, int N, int64_t ldx, float alpha, const float* alpha_ptr,
                            float* db, int stripes, int64_t stripe_stride, void* stream);
int capgen_debug_stripe_reduce(float* S, int stripes, int64_t stride, int64_t n, float* dst, int accumulate, int clear,
                               void* stream);
/* out[m] = table[ids[m * ids_ld]] (f32 table -> dtype); grad[ids[m]] += dE[m] for ids[m] != pad. */
int capgen_debug_embedding_gather(const float* table, const int32_t* ids, int64_t ids_ld, int M, int d, void* out,
                                  int dtype, void* stream);
int capgen_debug_embedding_scatter_add(const void* dE, const int32_t* ids, int M, int d, int pad, float* grad,
                                       int dtype, void* stream);
/* out[m] = [feats[m] | pos[m] | 0] (width Kp), valid[m] = any(pos[m] != 0); with img_idx ([M / N]) the
 * rows of image img_idx[b] of an [n_img, N, .] store (out of range: a zero row, valid 0); seed_bump
 * (optional device u64) advances by 0x9E3779B97F4A7C15 once. */
int capgen_debug_pack_encoder_input(const void* feats, int feats_dtype, const float* pos, int M, int F, int P, int Kp,
                                    void* out, int out_dtype, unsigned char* valid, const int32_t* img_idx, int N,
                                    int n_img, uint64_t* seed_bump, void* stream);
/* caps [B][T] -> ids_in / tgt [B][T-1], count = #(tgt != pad) (f32), inv_count = 1 / count (optional). */
int capgen_debug_prepare_captions(const int32_t* caps, int B, int T, int pad, int32_t* ids_in, int32_t* tgt,
                                  float* count, uint64_t* seed_bump, float* inv_count, void* stream);
/* loss_row[m] = lse - logit[tgt], dlogits = softmax - onehot (dtype; 0 for tgt == pad).  ce_finish: the
 * same from the classifier epilogue's outputs (stats = {max, sum exp} float pairs per 16-column slab,
 * row stride ld pairs; dl bf16 holds exp(v - slab max) and is rewritten in place; V % 4 == 0).
 * loss_finalize: loss = sum(loss_row) / count, or (1 - e^-ce)^2 ce (focal), grad_scale = dloss / d(row
 * sum) (optional); ce_in = the mean is given; partial = write the mean only. */
int capgen_debug_cross_entropy_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, float* loss_row,
                                    void* dlogits, int dtype, void* stream);
int capgen_debug_ce_finish(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V,
                           int pad, float* loss_row, void* dl, void* stream);
/* The same two with a per-caption weight: row m uses w = row_w[m / rows_per_w] ([M / rows_per_w] f32),
 * loss_row[m] = w (lse - logit[tgt]), dlogits = w (softmax - onehot) rounded once to dtype; pad rows stay 0.
 * Fail when row_w is null, rows_per_w < 1 or M % rows_per_w != 0. */
int capgen_debug_cross_entropy_rows_weighted(const float* logits, const int32_t* tgt, const float* row_w,
                                             int rows_per_w, int M, int V, int pad, float* loss_row, void* dlogits,
                                             int dtype, void* stream);
int capgen_debug_ce_finish_weighted(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt,
                                    const float* row_w, int rows_per_w, int M, int V, int pad, float* loss_row,
                                    void* dl, void* stream);
/* The two read-outs of capgen_score_captions (ops.h: score_rows from f32 logits [M, V]; score_finish from the
 * fused classifier's slab statistics [M, ld] {max, sum exp} and target logits, V % 4 == 0, ld >= ceil(V / 16),
 * nothing at or beyond slab ceil(V / 16) of a row is read).  Per row: token_logp [M] f32, hit [M] int32; per
 * caption of rows_per_caption rows: logp [M / rows_per_caption] f32, length and hits int32.  length and hits
 * may be null, for score_finish token_logp and hit too; fail on any other null pointer, rows_per_caption < 1
 * or M % rows_per_caption != 0.  Neither takes a pointer to softmax / gradient rows. */
int capgen_debug_score_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, int rows_per_caption,
                            float* token_logp, int32_t* hit, float* logp, int32_t* length, int32_t* hits,
                            void* stream);
int capgen_debug_score_finish(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V,
                              int pad, int rows_per_caption, float* token_logp, int32_t* hit, float* logp,
                              int32_t* length, int32_t* hits, void* stream);
int capgen_debug_loss_finalize(const float* loss_row, int M, const float* count, int focal, float* loss_out,
                               float* grad_scale, const float* ce_in, int partial, void* stream);
/* One torch.optim.Adam step of a flat f32 arena (n % 4 == 0): adam_prepare (++*step, device int64; scal =
 * 2 device floats) then adam_update; shadow[i] = bf16(p[i]) for i < n_shadow (optional), grid_cap > 0
 * caps the workgroups, and n_tiles <= 4 ranges [tile_off, tile_off + tile_len) of the shadow (HOST
 * arrays; whole 16-row blocks of 512-wide rows) are also written to tile_dst[t] in the attention
 * fronts' tiled layout.  to_bf16: dst = bf16(src).  arena_checksum: sum bits(p[i]) (2 i + 1) mod 2^64
 * into the HOST word *out (synchronous). */
int capgen_debug_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                      float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                      int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                      void* stream);
/* capgen_debug_adam with every gradient multiplied by the device float *gscale (required) before both
 * moment updates: the clipped update.  capgen_debug_grad_norm: the sum-of-squares kernel over g[0, n)
 * (n % 4 == 0; grid_cap > 0 caps the workgroups) into the device doubles partials[0, cap), one per
 * workgroup, then the finish kernel: out2 (2 device floats) = {norm = (float)sqrt(sum), coef =
 * (float)min(1, max_norm / (norm + 1e-6))}; max_norm >= 0, +inf gives coef = 1 exactly.  Fails (1) when
 * n % 4 != 0, a pointer is null or cap is smaller than the grid. */
int capgen_debug_adam_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                             float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                             int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                             const float* gscale, void* stream);
/* capgen_debug_adam_scaled plus the optional parts of the update, each of which may be absent: gscale
 * (null), weight_decay (0) -- p *= 1 - lr * weight_decay first -- and ema (null), n device floats updated
 * as e += (p_new - e) * (1 - ema_decay).  scal holds 8 device floats here: the hook stores {lr,
 * weight_decay, 1 - ema_decay} in scal[4..6] (synchronously) for the kernels to read, and the prepare
 * kernel writes scal[2] only when weight_decay != 0.
 * capgen_debug_arena_swap: a[i] <-> b[i] over n device floats (the kernel of capgen_ema_swap; grid_cap > 0
 * caps the workgroups).  Fails (1), writing nothing, when n % 4 != 0, n < 0 or a pointer is null. */
int capgen_debug_adam_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                         float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                         int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                         const float* gscale, float weight_decay, float* ema, float ema_decay, void* stream);
int capgen_debug_arena_swap(float* a, float* b, int64_t n, int grid_cap, void* stream);
int capgen_debug_grad_norm(const float* g, int64_t n, float max_norm, int grid_cap, double* partials, int cap,
                           float* out2, void* stream);
int capgen_debug_to_bf16(const float* src, void* dst, int64_t n, void* stream);
int capgen_debug_arena_checksum(const float* p, int64_t n, uint64_t* out, void* stream);
/* Decode selection.  argmax_softmax: ids_out[b * ids_ld + col] (and next_ids[b * next_ld]) = argmax of
 * the softmax (logsm: log-softmax) of row b, first index on ties; slab_argmax: the same from the decode
 * classifier's slab stats.  beam_step_topk: per image i the k best prev[j*B+i] + (log-)softmax(row
 * j*B+i)[v] under (score desc, j*V + v asc) -> out_prob / out_src / out_tok [sel*B + i]; stats NULL =
 * the full-row kernels, else the slab kernels (V <= 16384); cand_v / cand_i: k_in*B*k scratch.
 * beam_slab_step: the slab step in one launch, plus the gather of the sequences [.][Tw] (int64), ids
 * and K/V row table [.][Tc] from the source beams with the token at column t + 1. */
int capgen_debug_argmax_softmax(const float* logits, int B, int V, int64_t* ids_out, int64_t ids_ld, int col,
                                int32_t* next_ids, int64_t next_ld, int logsm, void* stream);
/* The selection of capgen_sample, one row per workgroup (definition: csrc/select.hip): token of row r by
 * Gumbel-max over z = logits[r] * inv_tau on the row's top_k logits (0: all), noise from (seed, site,
 * r * V + v) -> ids_out[r * ids_ld + col], next_ids[r * next_ld] (nullable), and its log-probability
 * -> logp_out[r * logp_ld + logp_col] (nullable). */
int capgen_debug_sample_softmax(const float* logits, int R, int V, float inv_tau, int top_k, uint64_t seed,
                                uint32_t site, int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids,
                                int64_t next_ld, float* logp_out, int64_t logp_ld, int logp_col, void* stream);
/* The selection of capgen_sample_nucleus: as capgen_debug_sample_softmax with the candidates cut to the
 * nucleus of top_p in (0, 1] (1: the kernels of capgen_debug_sample_softmax); count_out (nullable):
 * int32 [R], the size of each row's candidate set. */
int capgen_debug_sample_nucleus(const float* logits, int R, int V, float inv_tau, int top_k, float top_p,
                                uint64_t seed, uint32_t site, int64_t* ids_out, int64_t ids_ld, int col,
                                int32_t* next_ids, int64_t next_ld, float* logp_out, int64_t logp_ld, int logp_col,
                                int32_t* count_out, void* stream);
int capgen_debug_slab_argmax(const float* logits, const void* stats, int B, int V, int64_t* ids_out, int64_t ids_ld,
                             int col, int32_t* next_ids, int64_t next_ld, void* stream);
int capgen_debug_beam_step_topk(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                int k, int logsm, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                int32_t* out_tok, void* stream);
int capgen_debug_beam_slab_step(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                int k, int logsm, float* out_prob, int32_t* out_src, int32_t* out_tok,
                                const int64_t* seq_src, int64_t* seq_dst, int Tw, const int32_t* ids_src,
                                int32_t* ids_dst, const int32_t* kv_src, int32_t* kv_dst, int Tc, int t, void* stream);
/* One step of capgen_beam_nbest's selection (definition: csrc/select.hip).  stats == NULL: the full-row
 * kernels plus merge (cand_v / cand_i as capgen_debug_beam_step_topk; seq / ids / kv and t unused); else the
 * one-launch slab step (as capgen_debug_beam_slab_step; cand_v / cand_i unused).  fin_src / len_src
 * [k_in * B] in, fin_dst / len_dst [k * B] out.  The step needs at least k candidates per image. */
int capgen_debug_beam_step_ended(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                 int k, int end_id, const int32_t* fin_src, const int32_t* len_src, int32_t* fin_dst,
                                 int32_t* len_dst, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                 int32_t* out_tok, const int64_t* seq_src, int64_t* seq_dst, int Tw,
                                 const int32_t* ids_src, int32_t* ids_dst, const int32_t* kv_src, int32_t* kv_dst,
                                 int Tc, int t, void* stream);
/* One step of capgen_beam_diverse's selection (definition: csrc/select.hip): the full-row END-aware top-k with
 * k finalists per row, then the group merge.  k_in = 1 (step 0: every group draws on beam 0) or k; the other
 * arguments as capgen_debug_beam_step_ended's full-row form.  num_groups = 1 launches that form itself. */
int capgen_debug_beam_group_step(const float* logits, const float* prev, int k_in, int B, int V, int k,
                                 int num_groups, float diversity_penalty, int end_id, const int32_t* fin_src,
                                 const int32_t* len_src, int32_t* fin_dst, int32_t* len_dst, float* cand_v,
                                 int32_t* cand_i, float* out_prob, int32_t* out_src, int32_t* out_tok, void* stream);
/* One step of capgen_beam_forced's selection (definition: csrc/select.hip): the full-row END-aware top-k with
 * kf = min(16, k + W + 1) finalists and the W slot words' scores per row, then the bank merge.  k_in <= k;
 * word / group: device [B][W]; met_src [k_in * B] / met_dst [k * B] like fin / len; cand_v: k_in * B * (kf + W)
 * floats, cand_i: k_in * B * kf.  With no word on any image (W = 0, or every slot -1: the hook reads the slots on the
 * host) it launches capgen_debug_beam_step_ended's full-row form, whatever k <= 16, and zeroes met_dst. */
int capgen_debug_beam_forced_step(const float* logits, const float* prev, int k_in, int B, int V, int k, int end_id,
                                  const int32_t* word, const int32_t* group, int W, const int32_t* fin_src,
                                  const int32_t* len_src, const int32_t* met_src, int32_t* fin_dst, int32_t* len_dst,
                                  int32_t* met_dst, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                  int32_t* out_tok, void* stream);
/* The end of capgen_beam_nbest: the n_best of the k hypotheses (rows j * B + i of seq [k * B][Tw], logp, len)
 * per image by logp / max(len, 1)^length_penalty -> ids_out [n_best * B][Tw], score / logp / len (nullable). */
int capgen_debug_beam_finish(const int64_t* seq, const float* logp, const int32_t* len, int k, int B, int Tw,
                             float length_penalty, int n_best, int64_t* ids_out, float* score_out, float* logp_out,
                             int32_t* len_out, void* stream);
/* The decode constraints' one launch on device logits [R][V] (edited in place) before the selection of
 * position t: row r's history is ids[r * ids_ld + 1 .. t] (device, t < ids_ld); stats (nullable): the rows'
 * slab stats [R][ceil(V / 16)] of capgen_debug_gemm_classifier, rebuilt for every slab an edit touched.
 * c as capgen_set_decode_constraints takes it (banned on the host), without the max_length ranges. */
int capgen_debug_constrain_logits(float* logits, void* stats, int R, int V, const int32_t* ids, int64_t ids_ld,
                                  int t, const capgen_decode_constraints* c, void* stream);
/* The ensemble's one launch per step (definition: csrc/select.hip): logits is a HOST array of K device
 * pointers to f32 [R][V]; weights HOST, K values > 0 (NULL: equal), normalised as capgen_ensemble's; mode
 * CAPGEN_ENS_PROB / CAPGEN_ENS_LOGPROB; out [R][V] f32 device, may be logits[0]; stats (nullable): out's slab
 * stats [R][ceil(V / 16)] float2 {max, sum exp(v - max)}, as capgen_debug_gemm_classifier writes them. */
int capgen_debug_ensemble_combine(const float* const* logits, const float* weights, int K, int mode, int R, int V,
                                  float* out, void* stats, void* stream);
/* SCST kernels (csrc/rl.hip): rows = sample (argmax log-softmax), lse, logp[sample], entropy per logit
 * row; image = per-image masked mean entropy, scal[0] = sum(mask); numer: scal[1] = -sum logp mask
 * score; loss: out = {(1-w) lm + w struct, lm, struct}; grad = the fully scaled d loss / d logits. */
int capgen_debug_rl_rows(const float* logits, int M, int V, int32_t* sample, float* lse, float* logp_s, float* ent,
                         void* stream);
int capgen_debug_rl_image(const int32_t* sample, const float* ent, int B, int L, float* ent_img, float* scal,
                          void* stream);
int capgen_debug_rl_numer(const int32_t* sample, const float* logp_s, const float* score, int B, int L, float* scal,
                          void* stream);
int capgen_debug_rl_loss(const float* scal, const float* lm, float w, float* out, float* grad_scale, void* stream);
int capgen_debug_rl_grad(const float* logits, const int32_t* tgt, const int32_t* sample, const float* lse,
                         const float* score, const float* count, const float* scal, int B, int L, int V, int pad,
                         float w, void* dl, int dtype, void* stream);
/* The classifier GEMM's fused epilogues (bf16 NT, v = A . B^T + bias, A [M][K], B [N][K], f32 bias):
 * ce_tgt given = the training form (C bf16 = exp(v - slab max), stats = {max, sum exp} per 16-column
 * slab, ce_tlogit[m] = v[ce_tgt[m]]); ce_tgt NULL = the decode form (C = the f32 logits + stats). */
int capgen_debug_gemm_classifier(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* Cp,
                                 int64_t ldc, const float* bias, void* stats, int64_t stats_ld, const int32_t* ce_tgt,
                                 float* ce_tlogit, void* stream);

/* Persisted GEMM autotune table (no reference counterpart: the reference's GEMMs are cuBLAS calls
 * of torch eager, models.py:120-126).  The bf16 GEMM picks a tile / wave / pipeline / split-K
 * variant per shape by timing; a table file fixes those choices so that every process (bench,
 * tests, profiles) runs the same kernels.  load merges a file (returns the entries read, or -1:
 * no file); save writes every choice known to this process; tune_live_count = shapes this
 * process had to tune itself (a complete table keeps it 0).  libcapgen loads
 * $CAPGEN_TUNE_TABLE (default: tune_gfx950.txt next to the library) at first use. */
int capgen_tune_load(const char* path);
int capgen_tune_save(const char* path);
int capgen_tune_live_count(void);

/* Diagnostics of the multi-stream step (hazard.h): op 1 = start logging every launch's stream and
 * device byte ranges and every event / host-sync edge (clears the log), 0 = stop, 2 = check the log:
 * *n_conflicts = unordered pairs of launches on different streams touching overlapping bytes (at
 * least one writing), report (cap bytes, NUL-terminated) = the first of them.  side_delay: a spin
 * kernel of `us` microseconds in front of every launch off the critical stream (0 = off). */
int capgen_debug_hazard(int op, char* report, int cap, int* n_conflicts);
int capgen_debug_side_delay(double us);
/* The engine's RCCL call sequence (op 1 = start recording + clear, 0 = stop, 2 = dump one line per
 * collective: name, bytes, stream role).  Every rank must issue the identical sequence whatever its
 * batch, or the ranks deadlock (test hook for the data-parallel step). */
int capgen_debug_collectives(capgen_t* h, int op, char* out, int cap);
/* Un-profiled per-kernel timeline: op 1 = give every GEMM / LayerNorm / attention launch of the
 * following steps a timestamp slot (drops the captured forward so it re-captures with them), 3 = arm
 * (zero the slots; device synchronised), 2 = read: out[2i], out[2i+1] = start / end (us, 100 MHz
 * real-time counter) of slot i of the last step, names = one line per slot ("crit|side|bucket
 * kernel shape"); returns the slot count (-1: error), 0 = off. */
int capgen_debug_stamps(capgen_t* h, int op, double* out, int cap, char* names, int names_cap);

/* Data parallel (one process per GPU, RCCL over xGMI).  Rank 0 creates the 128-byte
 * unique id; the host broadcasts it (torch.distributed store) and every rank calls
 * capgen_dp_init, which also broadcasts rank 0's parameters. */
int capgen_dp_unique_id(char out[128]);
int capgen_dp_init(capgen_t* h, const char id[128], int rank, int world);
/* Override the global non-pad target count used by the CE mean (<= 0: all-reduce it).  Waits for
 * the previous step's copy of the override (no race with an in-flight step).  Under DP every rank's
 * loss output is the GLOBAL mean (Focal) loss: the per-rank partial CE sums are all-reduced before
 * the FocalLoss transform and the gradient scale (model.py:73-76, loss.py:20-28). */
int capgen_dp_set_global_count(capgen_t* h, float count);

/* Sharded parameter update (ZeRO-1; replaces the per-bucket all-reduce + full Adam that
 * torch.optim.Adam.step over DDP-averaged gradients would be, core/models.py:111-113,124-125).
 * With world > 1 (default; CAPGEN_ZERO=0 disables) every gradient bucket is reduce-scattered,
 * each rank runs Adam on its 1/world chunk, and the updated f32 chunk is all-gathered in place.
 * Parameters stay replicated on every rank after each step; the Adam moments are current only
 * in this rank's chunks -- capgen_dp_sync_adam_state (collective, every rank) all-gathers them
 * before capgen_get_adam_state is used for a checkpoint.
 * capgen_dp_buckets: the last train step's bucket ranges [off, off + count) over the parameter
 * arena, in issue order (rank r owns [off + r*count/world, off + (r+1)*count/world) of each).
 * capgen_dp_debug_shard (test hook): without any collective, update as rank `rank` of `world`
 * would (Adam on this rank's chunks only); world <= 1 turns it off. */
int capgen_dp_sync_adam_state(capgen_t* h);
/* The engine communicator's size and this rank (ncclCommCount / ncclCommUserRank; 0 / 0 before
 * capgen_dp_init).  At world > 1 the FIRST capgen_train_step / capgen_train_step_indexed also checks,
 * once, that every rank holds the same global non-pad count and loss (max == min over the ranks; the
 * loss the step wrote to loss_out, or its internal loss when loss_out was null) and fails the step
 * otherwise.  capgen_dp_check runs that same exchange now, at any world size (collective: every rank
 * calls it; needs capgen_dp_init and a train step before it; loss null = the buffer the last forward
 * wrote its loss to) -- the world-1 rehearsal of the check. */
int capgen_dp_comm_info(capgen_t* h, int* nranks, int* rank);
int capgen_dp_check(capgen_t* h, const float* loss, void* stream);
/* Exact, order-independent checksum of the f32 parameter arena (sum of the bit patterns times
 * (2 i + 1), mod 2^64; synchronous): equal parameters give equal values on every rank. */
int capgen_params_checksum(capgen_t* h, uint64_t* out);
int capgen_dp_buckets(capgen_t* h, int64_t* offs, int64_t* counts, int cap, int* n);
int capgen_dp_debug_shard(capgen_t* h, int rank, int world);

#ifdef __cplusplus
}
#endif
#endif /* CAPGEN_H */
