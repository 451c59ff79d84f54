// capgen -- the C ABI (include/capgen.h) over the engine: each function is `guarded`, then the device
// (or a null-handle check), the argument checks, and one engine call.  The test hooks that take no
// engine handle are in hooks.hip.
#include "abi_util.h"
#include "engine.h"

namespace capgen {
thread_local std::string g_last_error;
void scst_rewards(const int64_t* target, int64_t target_ld, const int64_t* sample, int64_t sample_ld, int B, int L,
                  int start_id, int end_id, int null_id, int64_t dot_id, double cider_w, double bleu_w, double* out);
}  // namespace capgen

// an ensemble entry point: the checks, then body(leader, run) between ensemble_enter / ensemble_leave
template <class F>
static int ensemble_call(const capgen_ensemble* e, const char* who, void* stream, F&& body) {
  return guarded([&] {
    const EnsembleRun run = capgen_engine::checked_ensemble(e, who);
    capgen_engine* h = run.m[0];
    set_device(h);
    hipStream_t cs = (hipStream_t)stream;
    h->ensemble_enter(run, cs);
    body(h, run);
    h->ensemble_leave(run, cs);
  });
}

extern "C" {

const char* capgen_last_error(void) { return g_last_error.c_str(); }

int capgen_abi_version(void) { return CAPGEN_ABI_VERSION; }

int capgen_set_knob(const char* name, int value, int* old) {
  return guarded([&] {
    require(name != nullptr, "set_knob: null name");
    const int rc = knob_set(name, value, old);
    require(rc != -1, std::string("set_knob: unknown switch ") + name);
    require(rc != -2, std::string("set_knob: ") + name + " exists only in the debug build (libcapgen_debug.so)");
  });
}

int capgen_param_table(const capgen_config* cfg, capgen_param_info* out, int cap, int* count, int64_t* arena_elems) {
  return guarded([&] {
    require(cfg != nullptr, "null config");
    Layout L = make_layout(*cfg);
    if (count) *count = (int)L.table.size();
    if (arena_elems) *arena_elems = L.total;
    for (int i = 0; i < (int)L.table.size() && i < cap && out; ++i) out[i] = L.table[i];
  });
}

int capgen_create(const capgen_config* cfg, int device, capgen_t** out) {
  return guarded([&] {
    require(cfg && out, "null argument");
    *out = nullptr;
    int ndev = 0;
    CAPGEN_HIP(hipGetDeviceCount(&ndev));
    require(device >= 0 && device < ndev, "capgen_create: invalid device index");
    CAPGEN_HIP(hipSetDevice(device));
    *out = new capgen_engine(*cfg, device);
  });
}

int capgen_destroy(capgen_t* h) {
  return guarded([&] {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
  });
}

int capgen_get_params(capgen_t* h, float* dst, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "get_params: size mismatch");
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(dst, h->params, n * 4, hipMemcpyDeviceToHost));
  });
}

int capgen_set_params(capgen_t* h, const float* src, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "set_params: size mismatch");
    h->require_unswapped("set_params");
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(h->params, src, n * 4, hipMemcpyHostToDevice));
    h->refresh_shadow(h->es);
    hz::host_sync(h->es);
  });
}

int capgen_get_grads(capgen_t* h, float* dst, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "get_grads: size mismatch");
    require(!h->grads_sharded, "get_grads: after a sharded (ZeRO-1) step the gradient arena holds this rank's "
                               "reduce-scattered chunks only (CAPGEN_ZERO=0 keeps whole gradients)");
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(dst, h->grads, n * 4, hipMemcpyDeviceToHost));
  });
}

int capgen_set_grads(capgen_t* h, const float* src, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "set_grads: size mismatch");
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(h->grads, src, n * 4, hipMemcpyHostToDevice));
  });
}

int capgen_get_adam_state(capgen_t* h, int64_t* step, float* m, float* v, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "get_adam_state: size mismatch");
    require(!h->moments_sharded, "get_adam_state: the moments are sharded across ranks (ZeRO-1): call "
                                 "capgen_dp_sync_adam_state on every rank first");
    hz::host_sync(h->es);
    if (step) CAPGEN_HIP(hipMemcpy(step, h->step, 8, hipMemcpyDeviceToHost));
    if (m) CAPGEN_HIP(hipMemcpy(m, h->am, n * 4, hipMemcpyDeviceToHost));
    if (v) CAPGEN_HIP(hipMemcpy(v, h->av, n * 4, hipMemcpyDeviceToHost));
  });
}

int capgen_set_adam_state(capgen_t* h, int64_t step, const float* m, const float* v, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "set_adam_state: size mismatch");
    h->require_unswapped("set_adam_state");
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(h->step, &step, 8, hipMemcpyHostToDevice));
    if (m) CAPGEN_HIP(hipMemcpy(h->am, m, n * 4, hipMemcpyHostToDevice));
    else CAPGEN_HIP(hipMemset(h->am, 0, n * 4));
    if (v) CAPGEN_HIP(hipMemcpy(h->av, v, n * 4, hipMemcpyHostToDevice));
    else CAPGEN_HIP(hipMemset(h->av, 0, n * 4));
    hz::host_sync(nullptr);
  });
}

int capgen_arenas(capgen_t* h, float** params, float** grads, int64_t* n) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    if (params) *params = h->params;
    if (grads) *grads = h->grads;
    if (n) *n = h->L.total;
  });
}

int capgen_set_training(capgen_t* h, int training) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    h->training = training != 0;
  });
}

int capgen_set_decode_log_softmax(capgen_t* h, int enable) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    h->decode_logsm = enable != 0;
  });
}

int capgen_set_decode_constraints(capgen_t* h, const capgen_decode_constraints* c) {
  return guarded([&] {
    set_device(h);
    h->set_constraints(c);
  });
}

int capgen_set_graph(capgen_t* h, int enable) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    h->graph_on = enable != 0;
    if (!h->graph_on) h->drop_graph();
  });
}

int capgen_set_lr(capgen_t* h, float lr) {
  return guarded([&] {
    set_device(h);
    require(std::isfinite(lr) && lr >= 0.f, "set_lr: the learning rate must be finite and >= 0");
    h->set_lr(lr);
  });
}

int capgen_get_lr(capgen_t* h, float* lr) {
  return guarded([&] {
    require(h != nullptr && lr != nullptr, "get_lr: null argument");
    *lr = h->lr_cur;
  });
}

int capgen_set_grad_clip(capgen_t* h, float max_norm) {
  return guarded([&] {
    set_device(h);
    require(max_norm >= 0.f, "set_grad_clip: max_norm must be 0 (off), > 0 or +inf (measure only)");  // (NaN fails too)
    h->set_grad_clip(max_norm);
  });
}

int capgen_set_weight_decay(capgen_t* h, float wd) {
  return guarded([&] {
    set_device(h);
    require(std::isfinite(wd) && wd >= 0.f, "set_weight_decay: wd must be finite and >= 0 (0 = off)");
    h->set_weight_decay(wd);
  });
}

int capgen_set_ema(capgen_t* h, float decay) {
  return guarded([&] {
    set_device(h);
    require(decay == 0.f || (decay > 0.f && decay < 1.f), "set_ema: decay must be 0 (off) or in (0, 1)");  // (NaN fails too)
    h->set_ema(decay);
  });
}

int capgen_ema_info(capgen_t* h, float* decay, int64_t* n_updates, int* swapped) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    if (decay) *decay = h->ema_decay;
    if (n_updates) *n_updates = h->ema_updates;
    if (swapped) *swapped = h->ema_swapped ? 1 : 0;
  });
}

int capgen_get_ema(capgen_t* h, float* dst, int64_t n) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "get_ema: size mismatch");
    require(h->ema != nullptr, "get_ema: the average was never enabled (capgen_set_ema)");
    hz::host_sync(h->es);
    hz::host_sync(h->ec);
    CAPGEN_HIP(hipMemcpy(dst, h->ema, n * 4, hipMemcpyDeviceToHost));
  });
}

int capgen_set_ema_state(capgen_t* h, const float* src, int64_t n, int64_t n_updates) {
  return guarded([&] {
    set_device(h);
    require(n == h->L.total, "set_ema_state: size mismatch");
    require(src != nullptr && n_updates >= 0, "set_ema_state: null source or negative n_updates");
    require(h->ema_on(), "set_ema_state: the average is off (capgen_set_ema first)");
    h->require_unswapped("set_ema_state");
    h->set_ema_state(src, n_updates);
  });
}

int capgen_ema_swap(capgen_t* h) {
  return guarded([&] {
    set_device(h);
    h->ema_swap();
  });
}

int capgen_last_grad_norm(capgen_t* h, float* host_out) {
  return guarded([&] {
    set_device(h);
    require(host_out != nullptr, "last_grad_norm: null output");
    require(h->norm_valid, "last_grad_norm: no update has run with clipping or measuring enabled "
                           "(capgen_set_grad_clip)");
    hz::host_sync(h->es);
    hz::host_sync(h->ec);
    CAPGEN_HIP(hipMemcpy(host_out, h->opt + 2, sizeof(float), hipMemcpyDeviceToHost));
  });
}

int capgen_forward(capgen_t* h, const void* feats, int ft, const float* pos, const int32_t* caps, int B, int N, int T,
                   float* loss_out, void* stream) {
  return guarded([&] {
    set_device(h);
    h->forward_call(feats, dt(ft), pos, caps, B, N, T, loss_out, h->training, (hipStream_t)stream);
  });
}

int capgen_backward(capgen_t* h, void* stream) {
  return guarded([&] {
    set_device(h);
    hipStream_t cs = (hipStream_t)stream;
    h->enter(cs);
    h->backward(h->es);
    h->allreduce_grads(h->es);
    h->leave(cs);
  });
}

int capgen_adam_step(capgen_t* h, void* stream) {
  return guarded([&] {
    set_device(h);
    hipStream_t cs = (hipStream_t)stream;
    h->require_unswapped("adam_step");
    h->enter(cs);
    h->adam(h->es);
    h->leave(cs);
  });
}

int capgen_train_step(capgen_t* h, const void* feats, int ft, const float* pos, const int32_t* caps, int B, int N,
                      int T, float* loss_out, void* stream) {
  return guarded([&] {
    set_device(h);
    h->require_unswapped("train_step");
    h->train_step(feats, dt(ft), pos, caps, B, N, T, loss_out, (hipStream_t)stream);
    h->dp_check((hipStream_t)stream, loss_out);
  });
}

int capgen_compute_loss(capgen_t* h, const void* feats, int ft, const float* pos, const int32_t* caps, int B, int N,
                        int T, float* loss_out, void* stream) {
  // torch.no_grad() only: dropout follows the module's train/eval state (models.py:131-135)
  return capgen_forward(h, feats, ft, pos, caps, B, N, T, loss_out, stream);
}

int capgen_copy_logits(capgen_t* h, float* dst, int64_t n, void* stream) {
  return guarded([&] {
    set_device(h);
    h->copy_logits(dst, n, (hipStream_t)stream);
  });
}

int capgen_greedy(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int64_t* ids_out,
                  float* attn_out, void* stream) {
  return decode_call(h, stream, [&] { h->greedy(feats, dt(ft), pos, B, N, ids_out, attn_out, h->es); });
}

int capgen_beam(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int k, int64_t* ids_out,
                void* stream) {
  return decode_call(h, stream, [&] { h->beam(feats, dt(ft), pos, B, N, k, ids_out, h->es); });
}

int capgen_beam_nbest(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int k, int end_id,
                      float length_penalty, int n_best, int64_t* ids_out, float* score_out, float* logp_out,
                      int32_t* len_out, void* stream) {
  return decode_call(h, stream, [&] {
    h->beam_nbest(feats, dt(ft), pos, B, N, k, end_id, length_penalty, n_best, ids_out, score_out, logp_out, len_out,
                  h->es);
  });
}

int capgen_beam_diverse(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int k, int num_groups,
                        float diversity_penalty, int end_id, float length_penalty, int n_best, int64_t* ids_out,
                        float* score_out, float* logp_out, int32_t* len_out, void* stream) {
  return decode_call(h, stream, [&] {
    h->beam_diverse(feats, dt(ft), pos, B, N, k, num_groups, diversity_penalty, end_id, length_penalty, n_best, ids_out,
                    score_out, logp_out, len_out, h->es);
  });
}

int capgen_beam_forced(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int k, int end_id,
                       float length_penalty, int n_best, const int32_t* word, const int32_t* group, int W,
                       int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out, int32_t* met_out,
                       void* stream) {
  return decode_call(h, stream, [&] {
    h->beam_forced(feats, dt(ft), pos, B, N, k, end_id, length_penalty, n_best, word, group, W, ids_out, score_out,
                   logp_out, len_out, met_out, h->es);
  });
}

int capgen_sample(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int n_samples,
                  float temperature, int top_k, uint64_t sd, int64_t* ids_out, float* logp_out, void* stream) {
  return capgen_sample_nucleus(h, feats, ft, pos, B, N, n_samples, temperature, top_k, 1.f, sd, ids_out, logp_out,
                               stream);
}

int capgen_sample_nucleus(capgen_t* h, const void* feats, int ft, const float* pos, int B, int N, int n_samples,
                          float temperature, int top_k, float top_p, uint64_t sd, int64_t* ids_out, float* logp_out,
                          void* stream) {
  return decode_call(h, stream, [&] {
    h->sample(feats, dt(ft), pos, B, N, n_samples, temperature, top_k, top_p, sd, ids_out, logp_out, h->es);
  });
}

int capgen_ensemble_beam_nbest(const capgen_ensemble* e, const void* feats, int ft, const float* pos, int B, int N,
                               int k, int end_id, float length_penalty, int n_best, int64_t* ids_out,
                               float* score_out, float* logp_out, int32_t* len_out, void* stream) {
  return ensemble_call(e, "ensemble_beam_nbest", stream, [&](capgen_engine* h, const EnsembleRun& run) {
    h->beam_nbest(feats, dt(ft), pos, B, N, k, end_id, length_penalty, n_best, ids_out, score_out, logp_out, len_out,
                  h->es, &run);
  });
}

int capgen_ensemble_beam_diverse(const capgen_ensemble* e, const void* feats, int ft, const float* pos, int B, int N,
                                 int k, int num_groups, float diversity_penalty, int end_id, float length_penalty,
                                 int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out,
                                 void* stream) {
  return ensemble_call(e, "ensemble_beam_diverse", stream, [&](capgen_engine* h, const EnsembleRun& run) {
    h->beam_diverse(feats, dt(ft), pos, B, N, k, num_groups, diversity_penalty, end_id, length_penalty, n_best, ids_out,
                    score_out, logp_out, len_out, h->es, &run);
  });
}

int capgen_ensemble_beam_forced(const capgen_ensemble* e, const void* feats, int ft, const float* pos, int B, int N,
                                int k, int end_id, float length_penalty, int n_best, const int32_t* word,
                                const int32_t* group, int W, int64_t* ids_out, float* score_out, float* logp_out,
                                int32_t* len_out, int32_t* met_out, void* stream) {
  return ensemble_call(e, "ensemble_beam_forced", stream, [&](capgen_engine* h, const EnsembleRun& run) {
    h->beam_forced(feats, dt(ft), pos, B, N, k, end_id, length_penalty, n_best, word, group, W, ids_out, score_out,
                   logp_out, len_out, met_out, h->es, &run);
  });
}

int capgen_ensemble_sample(const capgen_ensemble* e, const void* feats, int ft, const float* pos, int B, int N,
                           int n_samples, float temperature, int top_k, float top_p, uint64_t sd, int64_t* ids_out,
                           float* logp_out, void* stream) {
  return ensemble_call(e, "ensemble_sample", stream, [&](capgen_engine* h, const EnsembleRun& run) {
    h->sample(feats, dt(ft), pos, B, N, n_samples, temperature, top_k, top_p, sd, ids_out, logp_out, h->es, &run);
  });
}

int capgen_set_rng_seed(capgen_t* h, uint64_t sd) {
  return guarded([&] {
    set_device(h);
    hz::host_sync(h->es);
    CAPGEN_HIP(hipMemcpy(h->seed, &sd, 8, hipMemcpyHostToDevice));
  });
}

int capgen_train_step_indexed(capgen_t* h, const void* feat_store, int feats_dtype, const float* pos_store,
                              int n_images, const int32_t* img_idx, const int32_t* caps, int B, int N, int T,
                              float* loss_out, void* stream) {
  return guarded([&] {
    set_device(h);
    require(n_images >= 1, "train_step_indexed: empty store");
    h->require_unswapped("train_step_indexed");
    {
      Scoped<StepIn> inputs(h->in, StepIn{img_idx, n_images, nullptr});
      h->train_step(feat_store, dt(feats_dtype), pos_store, caps, B, N, T, loss_out, (hipStream_t)stream);
    }
    h->dp_check((hipStream_t)stream, loss_out);
  });
}

int capgen_train_step_weighted(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int n_images,
                               const int32_t* img_idx, const int32_t* caps, const float* weights, int B, int N, int T,
                               float* loss_out, int train, void* stream) {
  return guarded([&] {
    set_device(h);
    require(weights != nullptr, "train_step_weighted: weights is null");
    require(!h->cfg.focal_loss, "train_step_weighted: focal_loss transforms an unweighted mean");
    require(!img_idx || n_images >= 1, "train_step_weighted: empty store");
    if (train) h->require_unswapped("train_step_weighted");
    hipStream_t cs = (hipStream_t)stream;
    const DType ft = dt(feats_dtype);
    Scoped<StepIn> inputs(h->in, StepIn{img_idx, img_idx ? n_images : 0, weights});
    if (train) {
      h->train_step(feats, ft, pos, caps, B, N, T, loss_out, cs);
      h->dp_check(cs, loss_out);
    } else {  // as capgen_compute_loss: the forward alone
      h->forward_call(feats, ft, pos, caps, B, N, T, loss_out, h->training, cs);
    }
  });
}

int capgen_score_captions(capgen_t* h, const void* feats, int feats_dtype, const float* pos, int n_images,
                          const int32_t* img_idx, const int32_t* caps, int R, int N, int T, float* token_logp,
                          float* logp, int32_t* length, int32_t* hits, void* stream) {
  return guarded([&] {
    set_device(h);
    require(feats && pos && caps, "score_captions: feats, pos or caps is null");
    require(logp != nullptr, "score_captions: logp is null");
    require(R >= 1 && N >= 1 && N <= 64, "score_captions: need R >= 1 and 1 <= N <= 64");
    require(T >= 2 && T <= h->L.maxlen, "score_captions: need 2 <= T <= max_length");
    require(!img_idx || n_images >= 1, "score_captions: empty store");
    hipStream_t cs = (hipStream_t)stream;
    StepIn si;
    si.idx = img_idx, si.n_img = img_idx ? n_images : 0;
    si.score = true, si.s_tok = token_logp, si.s_logp = logp, si.s_len = length, si.s_hits = hits;
    Scoped<StepIn> inputs(h->in, si);
    // eager, on the engine's stream: the cached training graphs (keyed without the mode) stay as they are;
    // a deferred loss of the previous step was issued by that step's backward, which es is ordered after
    h->forward_call(feats, dt(feats_dtype), pos, caps, R, N, T, nullptr, /*drop_on=*/false, cs);
  });
}

int capgen_rl_sample(capgen_t* h, const void* feats, int feats_dtype, const float* pos, const int32_t* caps, int B,
                     int N, int T, int64_t* sample_out, float* entropy_out, float* lm_loss_out, void* stream) {
  return guarded([&] {
    set_device(h);
    h->rl_sample(feats, dt(feats_dtype), pos, caps, B, N, T, sample_out, entropy_out, lm_loss_out, (hipStream_t)stream);
  });
}

int capgen_rl_finish(capgen_t* h, const float* scores, float structure_loss_weight, float* loss_out, int train,
                     void* stream) {
  return guarded([&] {
    set_device(h);
    if (train) h->require_unswapped("rl_finish");
    h->rl_finish(scores, structure_loss_weight, loss_out, train != 0, (hipStream_t)stream);
  });
}

int capgen_scst_rewards(const int64_t* target, int64_t target_ld, const int64_t* sample, int64_t sample_ld, int B,
                        int L, int start_id, int end_id, int null_id, int64_t dot_id, double cider_w, double bleu_w,
                        double* out) {
  return guarded([&] {
    scst_rewards(target, target_ld, sample, sample_ld, B, L, start_id, end_id, null_id, dot_id, cider_w, bleu_w, out);
  });
}

int capgen_debug_copy_buffer(capgen_t* h, int which, void* host_dst, int64_t bytes) {
  return guarded([&] {
    set_device(h);
    require(h->ws != nullptr, "debug_copy_buffer: no workspace yet");
    void* src = h->debug_buffer(which);
    require(src != nullptr,
            "debug_copy_buffer: which in 0..7, 32 + 8 l + 0..4, 80 + 0..Le, 128 + 8 l + 0..7, 200 + l, 216 + l");
    hz::host_sync(nullptr);
    CAPGEN_HIP(hipMemcpy(host_dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
  });
}

int capgen_tune_load(const char* path) {
  int n = -1;
  const int rc = guarded([&] {
    require(path != nullptr, "tune_load: null path");
    n = gemm_tune_load(path);
  });
  return rc ? -2 : n;
}

int capgen_tune_save(const char* path) {
  int n = -1;
  const int rc = guarded([&] {
    require(path != nullptr, "tune_save: null path");
    n = gemm_tune_save(path);
    require(n >= 0, std::string("tune_save: cannot write ") + path);
  });
  return rc ? -2 : n;
}

int capgen_tune_live_count(void) { return gemm_tune_live_count(); }

int capgen_debug_collectives(capgen_t* h, int op, char* out, int cap) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    require(op >= 0 && op <= 2, "debug_collectives: op 0 (off), 1 (on + clear) or 2 (dump)");
    copy_out(h->collectives(op), out, cap);
  });
}

int capgen_debug_stamps(capgen_t* h, int op, double* out, int cap, char* names, int names_cap) {
  int count = 0;
  const int rc = guarded([&] {
    require(h != nullptr, "null engine handle");
    require(op >= 0 && op <= 3, "debug_stamps: op 0 (off), 1 (on), 2 (read), 3 (arm)");
    set_device(h);
    copy_out(h->stamps(op, out, cap, count), names, names_cap);
  });
  return rc ? -1 : count;
}

int capgen_dp_unique_id(char out[128]) {
  return guarded([&] {
    ncclUniqueId id;
    NCCL_CHECK(ncclGetUniqueId(&id));
    std::memcpy(out, id.internal, 128);
  });
}

int capgen_dp_init(capgen_t* h, const char id[128], int rank, int world) {
  return guarded([&] {
    set_device(h);
    require(world >= 1 && rank >= 0 && rank < world, "dp_init: bad rank/world");
    h->require_unswapped("dp_init");
    h->dp_init(id, rank, world);
  });
}

int capgen_dp_comm_info(capgen_t* h, int* nranks, int* rank) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    int n = 0, r = 0;
    if (h->comm) {
      NCCL_CHECK(ncclCommCount(h->comm, &n));
      NCCL_CHECK(ncclCommUserRank(h->comm, &r));
    }
    if (nranks) *nranks = n;
    if (rank) *rank = r;
  });
}

int capgen_dp_check(capgen_t* h, const float* loss, void* stream) {
  return guarded([&] {
    set_device(h);
    require(h->comm != nullptr, "dp_check: no communicator (capgen_dp_init first)");
    h->dp_check((hipStream_t)stream, loss, /*force=*/true);
  });
}

int capgen_params_checksum(capgen_t* h, uint64_t* out) {
  return guarded([&] {
    set_device(h);
    require(out != nullptr, "params_checksum: null output");
    hz::host_sync(h->es);
    hz::host_sync(h->ec);
    *out = arena_checksum(h->params, (size_t)h->L.total, h->es);
  });
}

int capgen_dp_sync_adam_state(capgen_t* h) {
  return guarded([&] {
    set_device(h);
    h->dp_sync_adam_state();
  });
}

int capgen_dp_buckets(capgen_t* h, int64_t* offs, int64_t* counts, int cap, int* n) {
  return guarded([&] {
    require(h != nullptr && n != nullptr, "dp_buckets: null argument");
    require((int)h->zbuckets.size() <= cap, "dp_buckets: capacity too small");
    for (size_t i = 0; i < h->zbuckets.size(); ++i) offs[i] = h->zbuckets[i][0], counts[i] = h->zbuckets[i][1];
    *n = (int)h->zbuckets.size();
  });
}

int capgen_dp_debug_shard(capgen_t* h, int rank, int world) {
  return guarded([&] {
    require(h != nullptr, "null engine handle");
    require(world <= 1 || (rank >= 0 && rank < world), "dp_debug_shard: bad rank/world");
    require(world <= 1 || !h->comm, "dp_debug_shard: not with a communicator");
    h->zemu_rank = world > 1 ? rank : 0;
    h->zemu_world = world > 1 ? world : 1;
  });
}

int capgen_dp_set_global_count(capgen_t* h, float count) {
  return guarded([&] {
    set_device(h);
    h->dp_set_global_count(count);
  });
}

}  // extern "C"
