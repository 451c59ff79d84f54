// capgen -- the test hooks that take no engine handle (capgen_debug_*, include/capgen.h): each drives
// one kernel launcher of the kernel headers below with the caller's buffers.
#include "abi_util.h"
#include "attention.h"
#include "gemm.h"
#include "hazard.h"
#include "ops.h"
#include "qkv_attn.h"
#include "rl.h"
#include "variants.h"

using namespace capgen;

extern "C" {

int capgen_debug_build(void) { return debug_build() ? 1 : 0; }

int capgen_debug_gemm(int M, int N, int K, const void* A, int64_t lda, int ta, const void* B, int64_t ldb, int tb,
                      void* Cp, int64_t ldc, int in_dtype, int out_dtype, const float* bias, float alpha, int beta,
                      int relu, void* stream) {
  return guarded([&] {
    gemm_init();
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = A, ga.lda = lda, ga.B = B, ga.ldb = ldb, ga.C = Cp, ga.ldc = ldc;
    ga.bias = bias, ga.alpha = alpha, ga.beta = beta, ga.relu = relu;
    gemm(ga, dt(in_dtype), dt(out_dtype), ta != 0, tb != 0, (hipStream_t)stream);
  });
}

int capgen_debug_gemm_tiled(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, int tb,
                            void* Bt, void* Cp, int64_t ldc, int out_dtype, const float* bias, int beta, int relu,
                            const void* aux, int64_t ldaux, void* stream) {
  return guarded([&] {
    gemm_init();
    const hipStream_t s = (hipStream_t)stream;
    gemm_tile_b(reinterpret_cast<const bf16*>(B), ldb, tb, N, K, reinterpret_cast<bf16*>(Bt), s);
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = A, ga.lda = lda, ga.B = B, ga.ldb = ldb, ga.C = Cp, ga.ldc = ldc;
    ga.bias = bias, ga.beta = beta, ga.relu = relu, ga.aux = aux, ga.ldaux = ldaux, ga.bt = Bt;
    require(gemm_breg_ok(ga), "debug_gemm_tiled: a shape / epilogue the register-B kernel does not take");
    gemm(ga, DType::BF16, dt(out_dtype), false, tb != 0, s);
  });
}

int capgen_debug_gemm_tiled_ln(int M, int N, const void* A, const void* ln_res, const void* B, void* Bt, void* Cp,
                               int out_dtype, const float* bias, int beta, int relu, const float* ln_gamma,
                               const float* ln_beta, void* ln_y, const int32_t* ln_ids, int64_t ln_ids_ld, int ln_pad,
                               void* stream) {
  return guarded([&] {
    gemm_init();
    const hipStream_t s = (hipStream_t)stream;
    const int K = 512;
    gemm_tile_b(reinterpret_cast<const bf16*>(B), K, 0, N, K, reinterpret_cast<bf16*>(Bt), s);
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = A, ga.lda = K, ga.B = B, ga.ldb = K, ga.C = Cp, ga.ldc = N;
    ga.bias = bias, ga.beta = beta, ga.relu = relu, ga.bt = Bt;
    ga.ln_res = ln_res, ga.ln_gamma = ln_gamma, ga.ln_beta = ln_beta, ga.ln_y = ln_y;
    ga.ln_ids = ln_ids, ga.ln_ids_ld = ln_ids_ld, ga.ln_pad = ln_pad;
    require(ln_gamma && gemm_breg_ok(ga), "debug_gemm_tiled_ln: a shape the folded-LayerNorm kernel does not take");
    gemm(ga, DType::BF16, dt(out_dtype), false, false, s);
  });
}

int capgen_debug_score_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, int rows_per_caption,
                            float* token_logp, int32_t* hit, float* logp, int32_t* length, int32_t* hits,
                            void* stream) {
  return guarded([&] {
    score_rows(logits, tgt, M, V, pad, rows_per_caption, token_logp, hit, logp, length, hits, (hipStream_t)stream);
  });
}

int capgen_debug_score_finish(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V,
                              int pad, int rows_per_caption, float* token_logp, int32_t* hit, float* logp,
                              int32_t* length, int32_t* hits, void* stream) {
  return guarded([&] {
    score_finish(reinterpret_cast<const float2*>(stats), ld, tlogit, tgt, M, V, pad, rows_per_caption, token_logp,
                 hit, logp, length, hits, (hipStream_t)stream);
  });
}

int capgen_debug_cross_entropy_rows_weighted(const float* logits, const int32_t* tgt, const float* row_w,
                                             int rows_per_w, int M, int V, int pad, float* loss_row, void* dlogits,
                                             int dtype, void* stream) {
  return guarded([&] {
    require(row_w != nullptr, "debug_cross_entropy_rows_weighted: row_w is null");
    require(rows_per_w >= 1 && M % rows_per_w == 0,
            "debug_cross_entropy_rows_weighted: rows_per_w must be >= 1 and divide M");
    cross_entropy_rows(logits, tgt, M, V, pad, loss_row, dlogits, dt(dtype), (hipStream_t)stream, row_w, rows_per_w);
  });
}

int capgen_debug_ce_finish_weighted(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt,
                                    const float* row_w, int rows_per_w, int M, int V, int pad, float* loss_row,
                                    void* dl, void* stream) {
  return guarded([&] {
    require(row_w != nullptr, "debug_ce_finish_weighted: row_w is null");
    require(rows_per_w >= 1 && M % rows_per_w == 0,
            "debug_ce_finish_weighted: rows_per_w must be >= 1 and divide M");
    ce_finish(reinterpret_cast<const float2*>(stats), ld, tlogit, tgt, M, V, pad, loss_row,
              reinterpret_cast<bf16*>(dl), (hipStream_t)stream, row_w, rows_per_w);
  });
}


namespace {
// the dropout descriptor of a hook: p <= 0 is dropout off; otherwise the 64-bit seed goes to a
// device word (as the engine's step seed) that lives until the launch has run
struct HookDrop {
  uint64_t* dev = nullptr;
  Drop d{};
  HookDrop(float p, int site, uint64_t seed, hipStream_t s) {
    if (!(p > 0.f)) return;
    require(p < 1.f, "debug hook: dropout p must be in [0, 1)");
    CAPGEN_HIP(hipMalloc(&dev, 8));
    CAPGEN_HIP(hipMemcpyAsync(dev, &seed, 8, hipMemcpyHostToDevice, s));
    CAPGEN_HIP(hipStreamSynchronize(s));  // (the source is a stack word)
    d.seed_ptr = dev, d.site = (uint32_t)site, d.thresh = drop_threshold(p), d.scale = 1.f / (1.f - p);
  }
  void finish(hipStream_t s) {
    if (!dev) return;
    CAPGEN_HIP(hipStreamSynchronize(s));
    uint64_t* p = dev;
    dev = nullptr;
    CAPGEN_HIP(hipFree(p));
  }
  ~HookDrop() {
    if (dev) (void)hipFree(dev);  // (error path: hipFree waits for the device)
  }
};
}  // namespace

int capgen_debug_attention(int dtype, int B, int H, int Lq, int Lk, int dk, const void* q, const void* k,
                           const void* v, const unsigned char* key_valid, int causal, float temperature, void* o,
                           float* probs, const void* dout, void* dq, void* dk_, void* dv, void* stream) {
  return guarded([&] {
    require(B >= 1 && H >= 1 && dk >= 1, "debug_attention: bad shape");
    const int64_t ld = (int64_t)H * dk;
    AttnGeom g = attn_dense(B, H, Lq, Lk, dk, q, ld, k, ld, v, ld, ld);
    g.key_valid = key_valid, g.kv_bs = Lk;
    g.causal = causal;
    g.temperature = temperature;
    hipStream_t s = (hipStream_t)stream;
    attention_fwd(g, o, probs, dt(dtype), s);
    if (dout) attention_bwd(g, probs, dout, dq, dk_, dv, dt(dtype), s);
  });
}

int capgen_debug_attention_geom(int dtype, const capgen_attn_geom_t* c, void* o, float* probs, const void* dout,
                                void* dq, void* dk_, void* dv, void* stream) {
  return guarded([&] {
    require(c != nullptr, "debug_attention_geom: no geometry");
    require(c->B >= 1 && c->H >= 1 && c->dk >= 1 && c->Lq >= 1 && c->Lq <= 64 && c->Lk >= 1 && c->Lk <= 64,
            "debug_attention_geom: bad shape (B, H, dk >= 1; Lq, Lk in [1, 64])");
    require(o && c->q && c->k && c->v, "debug_attention_geom: q, k, v and o are required");
    require(!c->kv_row || c->kv_row_ld >= c->Lk, "debug_attention_geom: kv_row_ld < Lk");
    const hipStream_t s = (hipStream_t)stream;
    HookDrop hd(c->drop_p, c->drop_site, c->drop_seed, s);
    AttnGeom g;
    g.B = c->B, g.H = c->H, g.Lq = c->Lq, g.Lk = c->Lk, g.dk = c->dk;
    g.q = c->q, g.q_ld = c->q_ld, g.q_bs = c->q_bs;
    g.k = c->k, g.k_ld = c->k_ld, g.k_bs = c->k_bs;
    g.v = c->v, g.v_ld = c->v_ld, g.v_bs = c->v_bs;
    g.o_ld = c->o_ld, g.o_bs = c->o_bs;
    g.kv_bmod = c->kv_bmod;
    g.kv_row = c->kv_row, g.kv_row_ld = c->kv_row_ld;
    g.key_valid = c->key_valid, g.kv_bs = c->kv_bs;
    g.key_ids = c->key_ids, g.kid_bs = c->kid_bs, g.pad_idx = c->pad_idx;
    g.causal = c->causal, g.q_pos0 = c->q_pos0;
    g.temperature = c->temperature;
    g.drop = hd.d;
    if (dout) {
      // (the backward kernels write dk / dv per query batch and know no row table)
      require(dq && dk_ && dv, "debug_attention_geom: dout needs dq, dk, dv");
      require(!g.kv_row && g.kv_bmod == 0, "debug_attention_geom: no backward with kv_row / kv_bmod");
      require(probs || (dt(dtype) == DType::BF16 && attention_mfma_ok(g)),
              "debug_attention_geom: this backward reads the saved probs");
      // (a backward the launcher would refuse is refused here, before the forward: nothing is launched)
      require(attention_bwd_lds(g, dt(dtype)) <= 160 * 1024,
              "debug_attention_geom: attention_bwd: LDS budget exceeded (head size too large)");
    }
    attention_fwd(g, o, probs, dt(dtype), s);
    if (dout) attention_bwd(g, probs, dout, dq, dk_, dv, dt(dtype), s);
    hd.finish(s);
  });
}

int capgen_debug_attention_head_mean(const float* probs, int B, int H, int Lq, int Lk, int row, float* out,
                                     void* stream) {
  return guarded([&] {
    require(B >= 1 && H >= 1 && Lq >= 1 && Lk >= 1 && row >= 0 && row < Lq, "debug_attention_head_mean: bad shape");
    require(probs && out, "debug_attention_head_mean: probs and out are required");
    attention_head_mean(probs, B, H, Lq, Lk, row, out, (hipStream_t)stream);
  });
}


// the test hooks' weights in the fronts' tiled layout (a per-process scratch, grown as needed)
static const bf16* debug_tiles(const bf16* W, int rows, hipStream_t s) {
  static bf16* buf = nullptr;
  static size_t cap = 0;
  const size_t need = (size_t)rows * 512 * 2;
  if (need > cap) {
    CAPGEN_HIP(hipDeviceSynchronize());  // (the previous scratch may still be read)
    if (buf) CAPGEN_HIP(hipFree(buf));
    CAPGEN_HIP(hipMalloc(&buf, need));
    cap = need;
  }
  qkv_tile_weights(W, rows, 512, buf, s);
  return buf;
}

int capgen_debug_qkv_attention(int B, int L, int H, const void* X, const void* W, void* qkv, void* o,
                               const unsigned char* key_valid, const int32_t* key_ids, int pad_idx, int causal,
                               float drop_p, int drop_site, uint64_t drop_seed, void* stream) {
  return guarded([&] {
    require(B >= 1 && L >= 1 && H >= 1, "debug_qkv_attention: bad shape");
    const int d = H * 64;
    HookDrop hd(drop_p, drop_site, drop_seed, (hipStream_t)stream);
    QkvAttn qa;
    AttnGeom& g = qa.g;
    g = attn_dense(B, H, L, L, 64, qkv, 3 * d, (const bf16*)qkv + d, 3 * d, (const bf16*)qkv + 2 * d, 3 * d, d);
    g.key_valid = key_valid, g.kv_bs = L, g.key_ids = key_ids, g.kid_bs = L, g.pad_idx = pad_idx, g.causal = causal;
    qa.X = (const bf16*)X, qa.ldx = d, qa.W = debug_tiles((const bf16*)W, 3 * d, (hipStream_t)stream), qa.d = d;
    qa.qkv = (bf16*)qkv, qa.ldqkv = 3 * d, qa.o = (bf16*)o;
    g.drop = hd.d;
    qkv_attn_fwd(qa, (hipStream_t)stream);
    hd.finish((hipStream_t)stream);
  });
}

int capgen_debug_cross_attention(int B, int Lq, int Lk, int H, const void* X, const void* Wq, const void* KV, void* q,
                                 void* o, const unsigned char* key_valid, float drop_p, int drop_site,
                                 uint64_t drop_seed, void* stream) {
  return guarded([&] {
    require(B >= 1 && Lq >= 1 && Lk >= 1 && H >= 1, "debug_cross_attention: bad shape");
    const int d = H * 64;
    HookDrop hd(drop_p, drop_site, drop_seed, (hipStream_t)stream);
    QkvAttn qa;
    qa.g = attn_dense(B, H, Lq, Lk, 64, q, d, KV, 2 * d, (const bf16*)KV + d, 2 * d, d);
    qa.g.key_valid = key_valid, qa.g.kv_bs = Lk;
    qa.cross = 1;
    qa.X = (const bf16*)X, qa.ldx = d, qa.W = debug_tiles((const bf16*)Wq, d, (hipStream_t)stream), qa.d = d;
    qa.qkv = (bf16*)q, qa.ldqkv = d, qa.o = (bf16*)o;
    qa.g.drop = hd.d;
    qkv_attn_fwd(qa, (hipStream_t)stream);
    hd.finish((hipStream_t)stream);
  });
}

int capgen_debug_attention_bwd_wo(int B, int Lq, int Lk, int H, const void* q, const void* k, const void* v,
                                  const unsigned char* key_valid, int causal, const void* dA, const void* Wo, void* dq,
                                  void* dk, void* dv, float drop_p, int drop_site, uint64_t drop_seed, void* stream) {
  return guarded([&] {
    require(B >= 1 && Lq >= 1 && Lk >= 1 && H * 64 == 512, "debug_attention_bwd_wo: bad shape (H * 64 = 512)");
    const int d = H * 64;
    const hipStream_t s = (hipStream_t)stream;
    HookDrop hd(drop_p, drop_site, drop_seed, s);
    static bf16* wt = nullptr;  // (the test hook's tiled Wo^T scratch)
    if (!wt) CAPGEN_HIP(hipMalloc(&wt, (size_t)512 * 512 * 2));
    qkv_tile_weights_t((const bf16*)Wo, 512, wt, s);
    QkvBwd qb;
    AttnGeom& g = qb.g;
    g = attn_dense(B, H, Lq, Lk, 64, q, d, k, d, v, d, d);
    if (key_valid) g.key_valid = key_valid, g.kv_bs = Lk;
    g.causal = causal;
    qb.dA = (const bf16*)dA, qb.ldda = d, qb.Wt = wt;
    qb.dq = (bf16*)dq, qb.dk = (bf16*)dk, qb.dv = (bf16*)dv;
    g.drop = hd.d;
    qkv_attn_bwd(qb, s);
    hd.finish(s);
  });
}

int capgen_debug_gemm_variant(int v) {
  return guarded([&] { gemm_set_variant(v); });
}

// ---- test hooks of the row-wise / loss / Adam / selection / SCST launchers (ops.h, rl.h) ----
int capgen_debug_layernorm_fwd(int dtype, int M, int d, const void* a, const float* a_bias, float drop_p,
                               int drop_site, uint64_t drop_seed, const void* res, const float* pe, int pe_L,
                               const float* gamma, const float* beta, const int32_t* ids, int64_t ids_ld, int pad_idx,
                               const unsigned char* valid, void* y, void* v_save, float* mean, float* rstd,
                               void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(a && gamma && beta && y, "debug_layernorm_fwd: a, gamma, beta, y are required");
    HookDrop hd(drop_p, drop_site, drop_seed, s);
    LnFwd f;
    f.M = M, f.d = d, f.a = a, f.a_bias = a_bias, f.drop = hd.d, f.res = res, f.pe = pe, f.pe_L = pe_L;
    f.gamma = gamma, f.beta = beta, f.mask.ids = ids, f.mask.ids_ld = ids_ld, f.mask.pad_idx = pad_idx;
    f.mask.valid = valid, f.y = y, f.v_save = v_save, f.mean = mean, f.rstd = rstd;
    layernorm_fwd(f, dt(dtype), s);
    hd.finish(s);
  });
}

int capgen_debug_layernorm_bwd(int dtype, int M, int d, const void* dy, const void* v, const float* mean,
                               const float* rstd, const float* gamma, const int32_t* ids, int64_t ids_ld, int pad_idx,
                               const unsigned char* valid, float drop_p, int drop_site, uint64_t drop_seed,
                               void* d_res, void* d_a, float* dgamma, float* dbeta, float* dbias, int stripes,
                               int64_t stripe_stride, void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(dy && v && mean && rstd && gamma, "debug_layernorm_bwd: dy, v, mean, rstd, gamma are required");
    require((dgamma == nullptr) == (dbeta == nullptr), "debug_layernorm_bwd: dgamma and dbeta go together");
    require(stripes >= 1 && (stripes == 1 || stripe_stride >= d), "debug_layernorm_bwd: stripes >= 1, stride >= d");
    HookDrop hd(drop_p, drop_site, drop_seed, s);
    LnBwd b;
    b.M = M, b.d = d, b.dy = dy, b.v = v, b.mean = mean, b.rstd = rstd, b.gamma = gamma;
    b.mask.ids = ids, b.mask.ids_ld = ids_ld, b.mask.pad_idx = pad_idx, b.mask.valid = valid, b.drop = hd.d;
    b.d_res = d_res, b.d_a = d_a, b.dgamma = dgamma, b.dbeta = dbeta, b.dbias = dbias;
    b.stripes = stripes, b.stripe_stride = stripe_stride;
    layernorm_bwd(b, dt(dtype), s);
    hd.finish(s);
  });
}

int capgen_debug_column_sum(int dtype, const void* X, int M, int N, int64_t ldx, float alpha, const float* alpha_ptr,
                            float* db, int stripes, int64_t stripe_stride, void* stream) {
  return guarded([&] {
    require(stripes >= 1 && ldx >= N, "debug_column_sum: stripes >= 1, ldx >= N");
    column_sum(X, M, N, ldx, alpha, alpha_ptr, db, dt(dtype), (hipStream_t)stream, stripes, stripe_stride);
  });
}

int capgen_debug_stripe_reduce(float* S, int stripes, int64_t stride, int64_t n, float* dst, int accumulate, int clear,
                               void* stream) {
  return guarded([&] { stripe_reduce(S, stripes, stride, n, dst, accumulate, (hipStream_t)stream, clear); });
}

int capgen_debug_embedding_gather(const float* table, const int32_t* ids, int64_t ids_ld, int M, int d, void* out,
                                  int dtype, void* stream) {
  return guarded([&] { embedding_gather(table, ids, ids_ld, M, d, out, dt(dtype), (hipStream_t)stream); });
}

int capgen_debug_embedding_scatter_add(const void* dE, const int32_t* ids, int M, int d, int pad, float* grad,
                                       int dtype, void* stream) {
  return guarded([&] { embedding_scatter_add(dE, ids, M, d, pad, grad, dt(dtype), (hipStream_t)stream); });
}

int capgen_debug_pack_encoder_input(const void* feats, int feats_dtype, const float* pos, int M, int F, int P, int Kp,
                                    void* out, int out_dtype, unsigned char* valid, const int32_t* img_idx, int N,
                                    int n_img, uint64_t* seed_bump, void* stream) {
  return guarded([&] {
    require(Kp >= F + P, "debug_pack_encoder_input: Kp >= F + P");
    require(img_idx == nullptr || (N > 0 && M % N == 0), "debug_pack_encoder_input: M must be whole images of N rows");
    pack_encoder_input(feats, dt(feats_dtype), pos, M, F, P, Kp, out, dt(out_dtype), valid, (hipStream_t)stream,
                       img_idx, N, n_img, seed_bump);
  });
}

int capgen_debug_prepare_captions(const int32_t* caps, int B, int T, int pad, int32_t* ids_in, int32_t* tgt,
                                  float* count, uint64_t* seed_bump, float* inv_count, void* stream) {
  return guarded([&] {
    require(B >= 1 && T >= 2, "debug_prepare_captions: B >= 1, T >= 2");
    prepare_captions(caps, B, T, pad, ids_in, tgt, count, (hipStream_t)stream, seed_bump, inv_count);
  });
}

int capgen_debug_cross_entropy_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, float* loss_row,
                                    void* dlogits, int dtype, void* stream) {
  return guarded([&] { cross_entropy_rows(logits, tgt, M, V, pad, loss_row, dlogits, dt(dtype), (hipStream_t)stream); });
}

int capgen_debug_ce_finish(const void* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V,
                           int pad, float* loss_row, void* dl, void* stream) {
  return guarded([&] {
    ce_finish(reinterpret_cast<const float2*>(stats), ld, tlogit, tgt, M, V, pad, loss_row,
              reinterpret_cast<bf16*>(dl), (hipStream_t)stream);
  });
}

int capgen_debug_loss_finalize(const float* loss_row, int M, const float* count, int focal, float* loss_out,
                               float* grad_scale, const float* ce_in, int partial, void* stream) {
  return guarded([&] { loss_finalize(loss_row, M, count, focal, loss_out, grad_scale, (hipStream_t)stream, ce_in, partial); });
}

int capgen_debug_adam(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                      float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                      int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                      void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(n >= 0 && n_shadow >= 0 && n_shadow <= n, "debug_adam: 0 <= n_shadow <= n");
    require(n % 4 == 0 && n_shadow % 4 == 0, "debug_adam: n and n_shadow must be multiples of 4");
    require(n_tiles >= 0 && n_tiles <= AdamTiles::kMax, "debug_adam: at most AdamTiles::kMax tiled ranges");
    AdamTiles tiles;
    tiles.n = n_tiles;
    for (int t = 0; t < n_tiles; ++t)
      tiles.off[t] = tile_off[t], tiles.len[t] = tile_len[t], tiles.dst[t] = reinterpret_cast<bf16*>(tile_dst[t]);
    adam_prepare(step, lr, b1, b2, scal, s);
    adam_update(p, g, m, v, (size_t)n, b1, b2, eps, scal, reinterpret_cast<bf16*>(shadow), (size_t)n_shadow, s,
                grid_cap, tiles);
  });
}

int capgen_debug_adam_scaled(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                             float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                             int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                             const float* gscale, void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(gscale != nullptr, "debug_adam_scaled: null gscale");
    require(n >= 0 && n_shadow >= 0 && n_shadow <= n, "debug_adam_scaled: 0 <= n_shadow <= n");
    require(n % 4 == 0 && n_shadow % 4 == 0, "debug_adam_scaled: n and n_shadow must be multiples of 4");
    require(n_tiles >= 0 && n_tiles <= AdamTiles::kMax, "debug_adam_scaled: at most AdamTiles::kMax tiled ranges");
    AdamTiles tiles;
    tiles.n = n_tiles;
    for (int t = 0; t < n_tiles; ++t)
      tiles.off[t] = tile_off[t], tiles.len[t] = tile_len[t], tiles.dst[t] = reinterpret_cast<bf16*>(tile_dst[t]);
    adam_prepare(step, lr, b1, b2, scal, s);
    adam_update(p, g, m, v, (size_t)n, b1, b2, eps, scal, reinterpret_cast<bf16*>(shadow), (size_t)n_shadow, s,
                grid_cap, tiles, gscale);
  });
}

int capgen_debug_adam_ex(float* p, const float* g, float* m, float* v, int64_t n, float lr, float b1, float b2,
                         float eps, int64_t* step, float* scal, void* shadow, int64_t n_shadow, int grid_cap,
                         int n_tiles, const int64_t* tile_off, const int64_t* tile_len, void* const* tile_dst,
                         const float* gscale, float weight_decay, float* ema, float ema_decay, void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(n >= 0 && n_shadow >= 0 && n_shadow <= n, "debug_adam_ex: 0 <= n_shadow <= n");
    require(n % 4 == 0 && n_shadow % 4 == 0, "debug_adam_ex: n and n_shadow must be multiples of 4");
    require(n_tiles >= 0 && n_tiles <= AdamTiles::kMax, "debug_adam_ex: at most AdamTiles::kMax tiled ranges");
    require(std::isfinite(weight_decay) && weight_decay >= 0.f, "debug_adam_ex: weight_decay must be finite and >= 0");
    require(!ema || (ema_decay > 0.f && ema_decay < 1.f), "debug_adam_ex: ema_decay must be in (0, 1)");
    AdamTiles tiles;
    tiles.n = n_tiles;
    for (int t = 0; t < n_tiles; ++t)
      tiles.off[t] = tile_off[t], tiles.len[t] = tile_len[t], tiles.dst[t] = reinterpret_cast<bf16*>(tile_dst[t]);
    const float words[3] = {lr, weight_decay, (float)(1.0 - (double)ema_decay)};
    CAPGEN_HIP(hipMemcpyAsync(scal + 4, words, sizeof words, hipMemcpyHostToDevice, s));
    CAPGEN_HIP(hipStreamSynchronize(s));  // (the words leave this frame before it returns)
    const bool decay = weight_decay != 0.f;
    adam_prepare(step, scal + 4, b1, b2, scal, s, decay ? scal + 5 : nullptr);
    adam_update(p, g, m, v, (size_t)n, b1, b2, eps, scal, reinterpret_cast<bf16*>(shadow), (size_t)n_shadow, s,
                grid_cap, tiles, gscale, AdamOpt{decay ? scal + 2 : nullptr, ema, scal + 6});
  });
}

int capgen_debug_arena_swap(float* a, float* b, int64_t n, int grid_cap, void* stream) {
  return guarded([&] {
    require(n >= 0, "debug_arena_swap: n must be >= 0");
    arena_swap(a, b, (size_t)n, (hipStream_t)stream, grid_cap);
  });
}

int capgen_debug_grad_norm(const float* g, int64_t n, float max_norm, int grid_cap, double* partials, int cap,
                           float* out2, void* stream) {
  return guarded([&] {
    const hipStream_t s = (hipStream_t)stream;
    require(g != nullptr && partials != nullptr && out2 != nullptr, "debug_grad_norm: null argument");
    require(n >= 0 && n % 4 == 0, "debug_grad_norm: n must be a non-negative multiple of 4");
    require(max_norm >= 0.f, "debug_grad_norm: max_norm must be >= 0 (+inf: measure only)");
    require(cap >= grad_sumsq_grid((size_t)n, grid_cap), "debug_grad_norm: the partials buffer is too small");
    const int slots = grad_sumsq(g, (size_t)n, partials, cap, s, grid_cap);
    grad_norm_finish(partials, slots, nullptr, nullptr, max_norm, out2, 3, s);
  });
}

int capgen_debug_to_bf16(const float* src, void* dst, int64_t n, void* stream) {
  return guarded([&] { to_bf16(src, reinterpret_cast<bf16*>(dst), (size_t)n, (hipStream_t)stream); });
}

int capgen_debug_arena_checksum(const float* p, int64_t n, uint64_t* out, void* stream) {
  return guarded([&] {
    require(out != nullptr && n >= 0, "debug_arena_checksum: null output");
    *out = arena_checksum(p, (size_t)n, (hipStream_t)stream);
  });
}

int capgen_debug_argmax_softmax(const float* logits, int B, int V, int64_t* ids_out, int64_t ids_ld, int col,
                                int32_t* next_ids, int64_t next_ld, int logsm, void* stream) {
  return guarded([&] { argmax_softmax(logits, B, V, ids_out, ids_ld, col, next_ids, next_ld, (hipStream_t)stream, logsm); });
}

int capgen_debug_sample_softmax(const float* logits, int R, int V, float inv_tau, int top_k, uint64_t sd, uint32_t site,
                                int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids, int64_t next_ld,
                                float* logp_out, int64_t logp_ld, int logp_col, void* stream) {
  return guarded([&] {
    sample_softmax(logits, R, V, inv_tau, top_k, sd, site, ids_out, ids_ld, col, next_ids, next_ld, logp_out, logp_ld,
                   logp_col, (hipStream_t)stream);
  });
}

int capgen_debug_sample_nucleus(const float* logits, int R, int V, float inv_tau, int top_k, float top_p, uint64_t sd,
                                uint32_t site, int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids,
                                int64_t next_ld, float* logp_out, int64_t logp_ld, int logp_col, int32_t* count_out,
                                void* stream) {
  return guarded([&] {
    sample_nucleus(logits, R, V, inv_tau, top_k, top_p, sd, site, ids_out, ids_ld, col, next_ids, next_ld, logp_out,
                   logp_ld, logp_col, count_out, (hipStream_t)stream);
  });
}

int capgen_debug_slab_argmax(const float* logits, const void* stats, int B, int V, int64_t* ids_out, int64_t ids_ld,
                             int col, int32_t* next_ids, int64_t next_ld, void* stream) {
  return guarded([&] {
    slab_argmax(logits, reinterpret_cast<const float2*>(stats), B, V, ids_out, ids_ld, col, next_ids, next_ld,
                (hipStream_t)stream);
  });
}

// the three beam-step hooks' descriptor: what every form takes
static BeamStep debug_beam_step(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                int k, int logsm, float* out_prob, int32_t* out_src, int32_t* out_tok) {
  BeamStep b;
  b.logits = logits, b.stats = reinterpret_cast<const float2*>(stats), b.prev = prev;
  b.k_in = k_in, b.B = B, b.V = V, b.k = k, b.logsm = logsm;
  b.out_prob = out_prob, b.out_src = out_src, b.out_tok = out_tok;
  return b;
}

int capgen_debug_beam_step_topk(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                int k, int logsm, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                int32_t* out_tok, void* stream) {
  return guarded([&] {
    BeamStep b = debug_beam_step(logits, stats, prev, k_in, B, V, k, logsm, out_prob, out_src, out_tok);
    b.cand_v = cand_v, b.cand_i = cand_i;
    beam_step(b, (hipStream_t)stream);
  });
}

int capgen_debug_beam_slab_step(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                int k, int logsm, float* out_prob, int32_t* out_src, int32_t* out_tok,
                                const int64_t* seq_src, int64_t* seq_dst, int Tw, const int32_t* ids_src,
                                int32_t* ids_dst, const int32_t* kv_src, int32_t* kv_dst, int Tc, int t, void* stream) {
  return guarded([&] {
    require(t >= 0, "debug_beam_slab_step: t >= 0");
    BeamReorder ro;
    ro.seq_src = seq_src, ro.seq_dst = seq_dst, ro.Tw = Tw, ro.ids_src = ids_src, ro.ids_dst = ids_dst;
    ro.kv_src = kv_src, ro.kv_dst = kv_dst, ro.Tc = Tc, ro.t = t;
    BeamStep b = debug_beam_step(logits, stats, prev, k_in, B, V, k, logsm, out_prob, out_src, out_tok);
    b.reorder = &ro;
    beam_step(b, (hipStream_t)stream);
  });
}

int capgen_debug_beam_step_ended(const float* logits, const void* stats, const float* prev, int k_in, int B, int V,
                                 int k, int end_id, const int32_t* fin_src, const int32_t* len_src, int32_t* fin_dst,
                                 int32_t* len_dst, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                 int32_t* out_tok, const int64_t* seq_src, int64_t* seq_dst, int Tw,
                                 const int32_t* ids_src, int32_t* ids_dst, const int32_t* kv_src, int32_t* kv_dst,
                                 int Tc, int t, void* stream) {
  return guarded([&] {
    const BeamEnd e{fin_src, len_src, fin_dst, len_dst, end_id};
    BeamReorder ro;
    ro.seq_src = seq_src, ro.seq_dst = seq_dst, ro.Tw = Tw, ro.ids_src = ids_src, ro.ids_dst = ids_dst;
    ro.kv_src = kv_src, ro.kv_dst = kv_dst, ro.Tc = Tc, ro.t = t;
    BeamStep b = debug_beam_step(logits, stats, prev, k_in, B, V, k, 1, out_prob, out_src, out_tok);
    b.cand_v = cand_v, b.cand_i = cand_i, b.end = &e;
    if (stats) {  // the one-launch slab step (cand_v / cand_i unused); else the full-row kernels plus merge
      require(t >= 0, "debug_beam_step_ended: t >= 0");
      b.reorder = &ro;
    }
    beam_step(b, (hipStream_t)stream);
  });
}

int capgen_debug_beam_group_step(const float* logits, const float* prev, int k_in, int B, int V, int k, int num_groups,
                                 float diversity_penalty, int end_id, const int32_t* fin_src, const int32_t* len_src,
                                 int32_t* fin_dst, int32_t* len_dst, float* cand_v, int32_t* cand_i, float* out_prob,
                                 int32_t* out_src, int32_t* out_tok, void* stream) {
  return guarded([&] {
    const BeamEnd e{fin_src, len_src, fin_dst, len_dst, end_id};
    const BeamGroups gr{num_groups, diversity_penalty};
    BeamStep b = debug_beam_step(logits, nullptr, prev, k_in, B, V, k, 1, out_prob, out_src, out_tok);
    b.cand_v = cand_v, b.cand_i = cand_i, b.end = &e, b.groups = &gr;
    beam_step(b, (hipStream_t)stream);
  });
}

int capgen_debug_beam_forced_step(const float* logits, const float* prev, int k_in, int B, int V, int k, int end_id,
                                  const int32_t* word, const int32_t* group, int W, const int32_t* fin_src,
                                  const int32_t* len_src, const int32_t* met_src, int32_t* fin_dst, int32_t* len_dst,
                                  int32_t* met_dst, float* cand_v, int32_t* cand_i, float* out_prob, int32_t* out_src,
                                  int32_t* out_tok, void* stream) {
  return guarded([&] {
    require(W >= 0 && W <= 16, "debug_beam_forced_step: words must be in [0, 16]");
    require(B >= 1 && k >= 1, "debug_beam_forced_step: B, k >= 1");
    require(W == 0 || word, "debug_beam_forced_step: null word");
    const hipStream_t s = (hipStream_t)stream;
    bool any = false;  // a word on any image?  (the hook may wait for the device; the engine never reads the slots)
    if (W > 0) {
      std::vector<int32_t> host((size_t)B * W);
      CAPGEN_HIP(hipStreamSynchronize(s));
      CAPGEN_HIP(hipMemcpy(host.data(), word, sizeof(int32_t) * host.size(), hipMemcpyDeviceToHost));
      for (int32_t w : host) any = any || w != -1;
    }
    const BeamEnd e{fin_src, len_src, fin_dst, len_dst, end_id};
    const BeamForced fo{word, group, W, met_src, met_dst};
    BeamStep b = debug_beam_step(logits, nullptr, prev, k_in, B, V, k, 1, out_prob, out_src, out_tok);
    b.cand_v = cand_v, b.cand_i = cand_i, b.end = &e;
    if (any) b.forced = &fo;
    else if (met_dst) CAPGEN_HIP(hipMemsetAsync(met_dst, 0, sizeof(int32_t) * k * B, s));  // no word: the END-aware step itself
    beam_step(b, s);
  });
}

int capgen_debug_beam_finish(const int64_t* seq, const float* logp, const int32_t* len, int k, int B, int Tw,
                             float length_penalty, int n_best, int64_t* ids_out, float* score_out, float* logp_out,
                             int32_t* len_out, void* stream) {
  return guarded([&] {
    beam_finish(seq, logp, len, k, B, Tw, length_penalty, n_best, ids_out, score_out, logp_out, len_out,
                (hipStream_t)stream);
  });
}

int capgen_debug_constrain_logits(float* logits, void* stats, int R, int V, const int32_t* ids, int64_t ids_ld, int t,
                                  const capgen_decode_constraints* c, void* stream) {
  return guarded([&] {
    require(c != nullptr, "debug_constrain_logits: null constraints");
    require(V >= 1, "debug_constrain_logits: V >= 1");
    DecodeConstraints d = checked_constraints(*c, V, 0, "debug_constrain_logits");
    const hipStream_t s = (hipStream_t)stream;
    int32_t* banned = nullptr;  // the list on the device for the one launch
    if (d.n_banned > 0) {
      CAPGEN_HIP(hipMalloc(&banned, sizeof(int32_t) * d.n_banned));
      (void)hipMemcpy(banned, c->banned, sizeof(int32_t) * d.n_banned, hipMemcpyHostToDevice);
    }
    d.banned = banned;
    try {
      constrain_logits(logits, reinterpret_cast<float2*>(stats), R, V, ids, ids_ld, t, d, s);
    } catch (...) {
      if (banned) (void)hipFree(banned);
      throw;
    }
    if (banned) {
      (void)hipStreamSynchronize(s);
      CAPGEN_HIP(hipFree(banned));
    }
  });
}

int capgen_debug_ensemble_combine(const float* const* logits, const float* weights, int K, int mode, int R, int V,
                                  float* out, void* stats, void* stream) {
  return guarded([&] {
    require(K >= 1 && K <= 8, "debug_ensemble_combine: K must be in [1, 8]");
    require(logits != nullptr, "debug_ensemble_combine: null logits");
    double sum = 0;
    for (int k = 0; k < K; ++k) {
      const float w = weights ? weights[k] : 1.f;
      require(std::isfinite(w) && w > 0.f, "debug_ensemble_combine: weights[" + std::to_string(k) + "] must be finite and > 0");
      sum += (double)w;
    }
    float log_w[8];
    for (int k = 0; k < K; ++k) log_w[k] = logf((float)((double)(weights ? weights[k] : 1.f) / sum));
    ensemble_combine(logits, log_w, K, mode, R, V, out, reinterpret_cast<float2*>(stats), (hipStream_t)stream);
  });
}

int capgen_debug_rl_rows(const float* logits, int M, int V, int32_t* sample, float* lse, float* logp_s, float* ent,
                         void* stream) {
  return guarded([&] {
    require(M >= 1 && V >= 1, "debug_rl_rows: M, V >= 1");
    rl_rows(logits, M, V, sample, lse, logp_s, ent, (hipStream_t)stream);
  });
}

int capgen_debug_rl_image(const int32_t* sample, const float* ent, int B, int L, float* ent_img, float* scal,
                          void* stream) {
  return guarded([&] { rl_image(sample, ent, B, L, ent_img, scal, (hipStream_t)stream); });
}

int capgen_debug_rl_numer(const int32_t* sample, const float* logp_s, const float* score, int B, int L, float* scal,
                          void* stream) {
  return guarded([&] { rl_numer(sample, logp_s, score, B, L, scal, (hipStream_t)stream); });
}

int capgen_debug_rl_loss(const float* scal, const float* lm, float w, float* out, float* grad_scale, void* stream) {
  return guarded([&] { rl_loss(scal, lm, w, out, grad_scale, (hipStream_t)stream); });
}

int capgen_debug_rl_grad(const float* logits, const int32_t* tgt, const int32_t* sample, const float* lse,
                         const float* score, const float* count, const float* scal, int B, int L, int V, int pad,
                         float w, void* dl, int dtype, void* stream) {
  return guarded([&] {
    require(B >= 1 && L >= 1 && V >= 1, "debug_rl_grad: B, L, V >= 1");
    rl_grad(logits, tgt, sample, lse, score, count, scal, B, L, V, pad, w, dl, dt(dtype), (hipStream_t)stream);
  });
}

int capgen_debug_gemm_classifier(int M, int N, int K, const void* A, int64_t lda, const void* B, int64_t ldb, void* Cp,
                                 int64_t ldc, const float* bias, void* stats, int64_t stats_ld, const int32_t* ce_tgt,
                                 float* ce_tlogit, void* stream) {
  return guarded([&] {
    require(stats != nullptr, "debug_gemm_classifier: stats is required");
    gemm_init();
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = A, ga.lda = lda, ga.B = B, ga.ldb = ldb, ga.C = Cp, ga.ldc = ldc;
    ga.bias = bias;
    if (ce_tgt) {  // training: C = exp(v - slab max) in bf16, the logits are not written
      ga.ce_stats = reinterpret_cast<float2*>(stats), ga.ce_ld = stats_ld, ga.ce_tgt = ce_tgt, ga.ce_tlogit = ce_tlogit;
      gemm(ga, DType::BF16, DType::BF16, false, false, (hipStream_t)stream);
    } else {  // decode: C = the f32 logits
      ga.dec_stats = reinterpret_cast<float2*>(stats), ga.dec_ld = stats_ld;
      gemm(ga, DType::BF16, DType::F32, false, false, (hipStream_t)stream);
    }
  });
}

int capgen_debug_gemm_timing_buf(void* dev_buf) {
  return guarded([&] { gemm_set_timing_buf(reinterpret_cast<uint64_t*>(dev_buf)); });
}

int capgen_debug_splitk_diag(int* out4, int reset) {
  return guarded([&] { gemm_splitk_diag(out4, reset != 0); });
}

int capgen_debug_splitk_protocol(int proto) {
  return guarded([&] {
    require(proto >= 0 && proto < 8192, "debug_splitk_protocol: bits 0..12 only (10-12: ablation build)");
    gemm_set_splitk_protocol(proto);
  });
}

int capgen_debug_hazard(int op, char* report, int cap, int* n_conflicts) {
  return guarded([&] {
    require(op >= 0 && op <= 2, "debug_hazard: op 0 (off), 1 (on + clear) or 2 (check)");
    if (op == 0) return hz::enable(false);
    if (op == 1) {
      hz::reset();
      return hz::enable(true);
    }
    std::string rep;
    const int n = hz::check(&rep);
    if (n_conflicts) *n_conflicts = n;
    copy_out(rep, report, cap);
  });
}

int capgen_debug_side_delay(double us) {
  return guarded([&] { hz::set_delay_us(us); });
}

}  // extern "C"
