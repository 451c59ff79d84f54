// capgen — row-wise / elementwise / optimizer kernels (launcher interface).
#pragma once
#include "capgen_common.h"
#include "gemm.h"

namespace capgen {

// y = LN(drop(a + a_bias) + res + pe[m % pe_L]) * rowmask          (modules.py:86-90, 114-120)
struct LnFwd {
  int M = 0, d = 0;
  int prio = 0;  // 1: the critical-path kernel raises its waves' issue priority (s_setprio)
  const void* a = nullptr;
  const float* a_bias = nullptr;
  Drop drop{};
  const void* res = nullptr;
  const float* pe = nullptr;
  int pe_L = 1;
  const float* gamma = nullptr;
  const float* beta = nullptr;
  RowMask mask{};
  void* y = nullptr;
  void* v_save = nullptr;  // LN input (post residual add), saved for backward
  float* mean = nullptr;
  float* rstd = nullptr;
  uint64_t* stamp = nullptr;  // diagnostic timestamps (StampScope)
};
void layernorm_fwd(const LnFwd& a, DType t, hipStream_t s);

struct LnBwd {
  int M = 0, d = 0;
  int prio = 0;  // as LnFwd::prio
  const void* dy = nullptr;
  const void* v = nullptr;
  const float* mean = nullptr;
  const float* rstd = nullptr;
  const float* gamma = nullptr;
  RowMask mask{};
  Drop drop{};             // the dropout applied to `a` in the forward
  void* d_res = nullptr;   // grad wrt residual input (= grad wrt LN input), or null
  void* d_a = nullptr;     // grad wrt a (dropout mask applied), or null
  float* dgamma = nullptr;  // accumulated
  float* dbeta = nullptr;   // accumulated
  float* dbias = nullptr;   // accumulated column sum of d_a (bias of the producing Linear), or null
  // contention relief: workgroup w accumulates into dgamma/dbeta/dbias + (w % stripes) * stripe_stride
  int stripes = 1;
  int64_t stripe_stride = 0;
  uint64_t* stamp = nullptr;  // diagnostic timestamps (StampScope)
};
void layernorm_bwd(const LnBwd& a, DType t, hipStream_t s);

// out[m] = [feats[m] | pos[m] | 0] (width Kp), valid[m] = any(pos[m] != 0)  (model.py:202-209)
// img_idx (optional, [M/N]): rows of image img_idx[b] of a resident [n_img, N, F] / [.., P] store
// (indices outside [0, n_img) give all-padding rows)
void pack_encoder_input(const void* feats, DType feats_t, const float* pos, int M, int F, int P, int Kp,
                        void* out, DType out_t, uint8_t* valid, hipStream_t s, const int32_t* img_idx = nullptr,
                        int N = 0, int n_img = 0, uint64_t* seed_bump = nullptr);
// caps [B][T] -> ids_in [B][T-1], tgt [B][T-1]; count = #(tgt != pad) as f32   (model.py:88-89);
// inv_count (optional): 1 / count, the CE mean's gradient scale (model.py:96)
void prepare_captions(const int32_t* caps, int B, int T, int pad, int32_t* ids_in, int32_t* tgt,
                      float* count, hipStream_t s, uint64_t* seed_bump = nullptr, float* inv_count = nullptr);
// out[m] = table[ids[m]] (f32 table -> T)                                      (model.py:432)
// (table_rows: rows of the table, for the hazard checker's byte ranges only)
void embedding_gather(const float* table, const int32_t* ids, int64_t ids_ld, int M, int d, void* out, DType t,
                      hipStream_t s, int64_t table_rows = 0);
// grad[ids[m]] += dE[m] for ids[m] != pad  (nn.Embedding padding_idx)
void embedding_scatter_add(const void* dE, const int32_t* ids, int M, int d, int pad, float* grad, DType t,
                           hipStream_t s, int64_t table_rows = 0);
// db[n] += alpha (* *alpha_ptr) * sum_m X[m][n]
void column_sum(const void* X, int M, int N, int64_t ldx, float alpha, const float* alpha_ptr, float* db,
                DType t, hipStream_t s, int stripes = 1, int64_t stripe_stride = 0);
// dst[i] (+)= sum_s S[s * stride + i], i < n  (folds striped partial sums); clear: the partials
// are zeroed as they are read (the next backward then needs no memset of them)
void stripe_reduce(float* S, int stripes, int64_t stride, int64_t n, float* dst, int accumulate,
                   hipStream_t s, int clear = 0);
// per-row cross entropy: loss_row[m] = lse - logit[tgt], dlogits = softmax - onehot (unscaled, 0 for pad)
// row_w != null (both CE launchers): row m's loss and gradient are multiplied by the per-caption weight
// row_w[m / rows_per_w] ([M / rows_per_w] f32, any sign; rows_per_w >= 1 divides M); pad rows stay 0
void cross_entropy_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, float* loss_row,
                        void* dlogits, DType t, hipStream_t s, const float* row_w = nullptr, int rows_per_w = 1);
// fused classifier + CE, second half: dl holds exp(v - slab max) from the classifier GEMM's CE
// epilogue (GemmArgs::ce_stats); writes loss_row and rewrites dl as softmax - onehot (0 for pad)
void ce_finish(const float2* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V, int pad,
               float* loss_row, bf16* dl, hipStream_t s, const float* row_w = nullptr, int rows_per_w = 1);
// Scoring given captions (no backward): token_logp[m] = logit[m][tgt] - logsumexp(logit[m]) and hit[m] =
// (the target's logit is >= every logit of the row), both exactly 0 where tgt == pad; caption r = rows
// [r * rows_per_caption, (r + 1) * rows_per_caption): logp[r] = sum of its token_logp in a fixed order (no
// atomics), length[r] = its non-pad targets, hits[r] = sum of its hits.  Neither writes anything of size
// M x V.  length / hits may be null.
// score_rows: from f32 logits [M][V] (token_logp and hit [M] are required: the per-caption pass reads them)
void score_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, int rows_per_caption,
                float* token_logp, int32_t* hit, float* logp, int32_t* length, int32_t* hits, hipStream_t s);
// score_finish: from the fused classifier's slab statistics and target logits (GemmArgs::ce_stats, ce_tlogit;
// V % 4 == 0, ld >= ceil(V / 16), statistics at or beyond slab ceil(V / 16) of a row are not read); the e rows
// the GEMM left are no argument.  token_logp / hit may be null too.
void score_finish(const float2* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V, int pad,
                  int rows_per_caption, float* token_logp, int32_t* hit, float* logp, int32_t* length,
                  int32_t* hits, hipStream_t s);
// loss = sum(loss_row)/count (or FocalLoss of it); grad_scale = dloss/d(logit sums).
// ce_in: the mean CE is given (all-reduced partials); partial: write sum(loss_row)/count only;
// grad_scale null: the loss only (the scale was written elsewhere, e.g. by prepare_captions).
void loss_finalize(const float* loss_row, int M, const float* count, int focal, float* loss_out,
                   float* grad_scale, hipStream_t s, const float* ce_in = nullptr, int partial = 0);
// Adam (torch.optim.Adam semantics).  step_buf: int64 step counter (incremented here).
void adam_prepare(int64_t* step, float lr, float b1, float b2, float* scal, hipStream_t s);
// Ranges of the shadow (relative to p, element offsets) that adam_update also writes in the fused
// attention fronts' tiled layout (qkv_tile_weights) -- whole 16-row blocks of 512-wide rows
struct AdamTiles {
  static constexpr int kMax = 4;
  int n = 0;
  int64_t off[kMax] = {};
  int64_t len[kMax] = {};
  bf16* dst[kMax] = {};
};
// Optional parts of the update, each a device word so that a replayed graph reads new values.  decay: the
// factor 1 - lr * wd (adam_prepare with wd writes it to scal[2]) every parameter is multiplied by before
// its update (torch.optim.AdamW).  ema (n f32, beside p) with ema_rate = 1 - decay: the exponential
// moving average e += (p_new - e) * rate of the updated parameters.
struct AdamOpt {
  const float* decay = nullptr;
  float* ema = nullptr;
  const float* ema_rate = nullptr;
};
// gscale (optional, one device float): every gradient is multiplied by *gscale before both moment updates
void adam_update(float* p, const float* g, float* m, float* v, size_t n, float b1, float b2, float eps,
                 const float* scal, bf16* shadow, size_t n_shadow, hipStream_t s, int grid_cap = 0,
                 const AdamTiles& tiles = AdamTiles{}, const float* gscale = nullptr, const AdamOpt& x = AdamOpt{});
// the learning rate read from a device word (the same formula: an unchanged rate gives the same bits);
// wd given (a device word): also scal[2] = (float)(1 - lr * wd), computed in double (else two floats)
void adam_prepare(int64_t* step, const float* lr, float b1, float b2, float* scal, hipStream_t s,
                  const float* wd = nullptr);
// a[i] <-> b[i] over n f32 (n % 4 == 0, disjoint); grid_cap 0: 2048 workgroups at most
void arena_swap(float* a, float* b, size_t n, hipStream_t s, int grid_cap = 0);
// Global gradient norm (torch.nn.utils.clip_grad_norm_).  grad_sumsq: the sum of squares of g[0, n)
// (16-byte aligned, n % 4 == 0) in double, one double per workgroup into partials[0, grid) by plain
// stores (no atomics: the value depends on n and the grid only); returns grid = grad_sumsq_grid(n,
// grid_cap) <= slots_cap (grid_cap 0: one workgroup per CU).  grad_norm_finish (one workgroup): phase & 1
// adds partials[0, n_slots) in slot order into *sum (double; null with phase 3: not stored); phase & 2
// writes out2 = {norm = (float)sqrt(*sum), coef = (float)min(1, max_norm / (norm + 1e-6))}, max_norm =
// *max_norm_ptr if given, else max_norm_val (+inf: coef = 1 exactly).  Definitions: ops.hip.
int grad_sumsq_grid(size_t n, int grid_cap = 0);
int grad_sumsq(const float* g, size_t n, double* partials, int slots_cap, hipStream_t s, int grid_cap = 0);
void grad_norm_finish(const double* partials, int n_slots, double* sum, const float* max_norm_ptr,
                      float max_norm_val, float* out2, int phase, hipStream_t s);
void to_bf16(const float* src, bf16* dst, size_t n, hipStream_t s);
// exact, order-independent checksum of an f32 arena (sum of bit patterns x (2 i + 1) mod 2^64); synchronous
uint64_t arena_checksum(const float* p, size_t n, hipStream_t s);
void bump_seed(uint64_t* seed, hipStream_t s);

}  // namespace capgen
