// capgen — row-wise / elementwise / optimizer kernels for gfx950.
//
// LayerNorm: one wave64 per row (d/64 contiguous elements per lane, 16-B loads), the
// mean/var reductions are cross-lane shuffles; dropout/bias/residual/positional-encoding
// adds and the non-pad row mask are fused in.  Backward accumulates dgamma/dbeta per
// workgroup and issues one f32 atomic per column per workgroup.
// CE: one workgroup per row (V=10000 f32 logits stay in L2 for the 3 passes).
// Adam: 16-B vectorised streaming over the flat parameter arena (HBM bound).
#include <cstdlib>

#include "ops.h"
#include "select_dev.h"  // block reductions
#include "hazard.h"

namespace capgen {


constexpr int LN_THREADS = 256;  // 4 rows per workgroup
constexpr float LN_EPS = 1e-6f;  // modules.py:57,105


// target of the LayerNorm kernels' absent optional inputs (zeros: residual, bias, positional row)
struct LnDummy {
  float zero[1024];  // the widest row (d = 64 * 16)
  uint64_t seed;
  int32_t id;
  uint8_t valid;
};
__device__ LnDummy g_ln_dummy = {{}, 0, 0, 1};

// Every global load of the row (input, residual, bias, positional row, gamma, beta, row mask,
// dropout seed) is issued before the first store: the kernel pays ONE memory round trip (the
// stores could alias the parameter pointers, so the compiler would not hoist them itself).
template <int DPL>
__device__ __forceinline__ void load_f32(const float* p, float (&out)[DPL]) {
  load_f<float, DPL>(p, out);
}
template <typename T, int DPL>
__global__ void __launch_bounds__(LN_THREADS) ln_fwd_kernel(LnFwd a) {
  StampScope stamp_scope(a.stamp);
  if (a.prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * (LN_THREADS / 64) + (threadIdx.x >> 6);
  if (m >= a.M) return;
  const int d = a.d, c0 = lane * DPL;
  const int64_t base = (int64_t)m * d + c0;
  float x[DPL], r[DPL], bias[DPL], pe[DPL], gm[DPL], bt[DPL];
  // optional inputs through a pointer select (absent -> a device dummy of zeros), loaded
  // unconditionally: a load inside a branch is waited for at the branch's join (one more round
  // trip per optional input; the ISA of the branchy form had five)
  // (the uniform base pointers go through opaque() so hipcc cannot turn the select back into a branch)
  const T* res_p = opaque(a.res ? reinterpret_cast<const T*>(a.res) : reinterpret_cast<const T*>(g_ln_dummy.zero)) +
                   (a.res ? base : c0);
  const float* bias_p = opaque(a.a_bias ? a.a_bias : g_ln_dummy.zero) + c0;
  const float* pe_p = opaque(a.pe ? a.pe : g_ln_dummy.zero) + (a.pe ? (int64_t)(m % max(a.pe_L, 1)) * d : 0) + c0;
  const uint64_t* seed_p = opaque(a.drop.seed_ptr ? a.drop.seed_ptr : &g_ln_dummy.seed);
  const int32_t* ids_p = opaque(a.mask.ids ? a.mask.ids : &g_ln_dummy.id) + (a.mask.ids ? (int64_t)m * a.mask.ids_ld : 0);
  const uint8_t* val_p = opaque(a.mask.valid ? a.mask.valid : &g_ln_dummy.valid) + (a.mask.valid ? m : 0);
  const uint64_t seed_v = *seed_p;
  const int idv = *ids_p;
  const int vld = *val_p;
  load_f<T, DPL>(reinterpret_cast<const T*>(a.a) + base, x);
  load_f<T, DPL>(res_p, r);
  load_f32<DPL>(bias_p, bias);
  load_f32<DPL>(pe_p, pe);
  load_f32<DPL>(a.gamma + c0, gm);
  load_f32<DPL>(a.beta + c0, bt);
  const bool kept = !(a.mask.ids && idv == a.mask.pad_idx) && !(a.mask.valid && vld == 0);
  const uint64_t seed = a.drop.seed_ptr ? seed_v : 0;
  if (a.a_bias) {
#pragma unroll
    for (int e = 0; e < DPL; ++e) x[e] += bias[e];
  }
  if (a.drop.seed_ptr) {
#pragma unroll
    for (int e = 0; e < DPL; ++e)
      x[e] = drop_keep(seed, a.drop.site, (uint32_t)(base + e), a.drop.thresh) ? x[e] * a.drop.scale : 0.f;
  }
  if (a.res) {
#pragma unroll
    for (int e = 0; e < DPL; ++e) x[e] += r[e];
  }
  if (a.pe) {
#pragma unroll
    for (int e = 0; e < DPL; ++e) x[e] += pe[e];
  }
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < DPL; ++e) s += x[e];
  const float mean = wave_sum(s) / (float)d;
  float q = 0.f;
#pragma unroll
  for (int e = 0; e < DPL; ++e) {
    float t = x[e] - mean;
    q = fmaf(t, t, q);
  }
  const float var = wave_sum(q) / (float)d;
  const float rstd = 1.0f / sqrtf(var + LN_EPS);
  const float keep = kept ? 1.f : 0.f;
  float y[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) y[e] = ((x[e] - mean) * rstd * gm[e] + bt[e]) * keep;
  if (a.v_save) store_f<T, DPL>(reinterpret_cast<T*>(a.v_save) + base, x);
  store_f<T, DPL>(reinterpret_cast<T*>(a.y) + base, y);
  if (lane == 0) {
    if (a.mean) a.mean[m] = mean;
    if (a.rstd) a.rstd[m] = rstd;
  }
}

// One row per wave.  The row index is wave-uniform (readfirstlane), so the row statistics, the row
// mask and the dropout seed are scalar loads, issued together with the row's two 16-B vector loads
// (dy, v) and gamma before any use: one memory round trip per row.
//
// (Round 3 ran R = 2 rows per wave -- both rows' loads first -- and, under co-scheduling with the
// side streams, sometimes wrote the row it computed last shifted by a row-scalar-sized amount while
// every input was equal after the call: 12-14 of 30 two-engine comparisons, 0 of 30 at one row.
// Its ISA did not issue the loads together: hipcc drained row 0's dy / v loads with vmcnt(0)
// before loading mean / rstd as per-lane vector loads, then issued row 1's.  The mechanism was not
// isolated; the multi-row variant is deleted, not configured away.)
template <typename T, int DPL, int NT = LN_THREADS>
__global__ void __launch_bounds__(NT) ln_bwd_kernel(LnBwd a) {
  __shared__ float red[3][NT / 64][64 * DPL];
  StampScope stamp_scope(a.stamp);
  if (a.prio) __builtin_amdgcn_s_setprio(3);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int d = a.d, c0 = lane * DPL;
  const int m = blockIdx.x * (NT / 64) + wave;  // wave-uniform
  const bool on = m < a.M;
  const int64_t base = (int64_t)m * d + c0;
  float gm[DPL], dy[DPL], v[DPL];
  float mean = 0.f, rstd = 0.f;
  int idv = 0, vld = 1;
  // optional inputs are read through a pointer select (absent -> a device dummy), never inside a
  // branch: a load in a branch makes hipcc wait for it at the join, one more round trip each
  const uint64_t* seed_p = opaque(a.drop.seed_ptr ? a.drop.seed_ptr : &g_ln_dummy.seed);
  const int32_t* ids_p = opaque(a.mask.ids ? a.mask.ids : &g_ln_dummy.id) +
                         (a.mask.ids ? (int64_t)min(m, a.M - 1) * a.mask.ids_ld : 0);
  const uint8_t* val_p = opaque(a.mask.valid ? a.mask.valid : &g_ln_dummy.valid) + (a.mask.valid ? min(m, a.M - 1) : 0);
  const uint64_t seed_v = *seed_p;
  const int idv_v = *ids_p;
  const int vld_v = *val_p;
  load_f<float, DPL>(a.gamma + c0, gm);
  if (on) {
    load_f<T, DPL>(reinterpret_cast<const T*>(a.dy) + base, dy);
    load_f<T, DPL>(reinterpret_cast<const T*>(a.v) + base, v);
    mean = a.mean[m], rstd = a.rstd[m];
  }
  const uint64_t seed = a.drop.seed_ptr ? seed_v : 0;
  if (a.mask.ids) idv = idv_v;
  if (a.mask.valid) vld = vld_v;
  const bool kept = !(a.mask.ids && idv == a.mask.pad_idx) && vld != 0;
  float dg[DPL], db[DPL], dz[DPL];
#pragma unroll
  for (int e = 0; e < DPL; ++e) dg[e] = db[e] = dz[e] = 0.f;
  if (on) {
    const float keep = kept ? 1.f : 0.f;
    float g[DPL], xh[DPL], s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int e = 0; e < DPL; ++e) {
      const float y = dy[e] * keep;
      xh[e] = (v[e] - mean) * rstd;
      g[e] = y * gm[e];
      s1 += g[e];
      s2 = fmaf(g[e], xh[e], s2);
      dg[e] = y * xh[e];
      db[e] = y;
    }
    const float mg = wave_sum(s1) / (float)d, mgx = wave_sum(s2) / (float)d;
    float dv[DPL];
#pragma unroll
    for (int e = 0; e < DPL; ++e) dv[e] = rstd * (g[e] - mg - xh[e] * mgx);
    if (a.d_res) store_f<T, DPL>(reinterpret_cast<T*>(a.d_res) + base, dv);
    if (a.d_a) {
      if (a.drop.seed_ptr) {
#pragma unroll
        for (int e = 0; e < DPL; ++e)
          dv[e] = drop_keep(seed, a.drop.site, (uint32_t)(base + e), a.drop.thresh) ? dv[e] * a.drop.scale : 0.f;
      }
      store_f<T, DPL>(reinterpret_cast<T*>(a.d_a) + base, dv);
#pragma unroll
      for (int e = 0; e < DPL; ++e) dz[e] = dv[e];
    }
  }
  if (!a.dgamma && !a.dbias) return;
  const int64_t so = (int64_t)(blockIdx.x % a.stripes) * a.stripe_stride;
#pragma unroll
  for (int e = 0; e < DPL; ++e) {
    red[0][wave][c0 + e] = dg[e];
    red[1][wave][c0 + e] = db[e];
    red[2][wave][c0 + e] = dz[e];
  }
  __syncthreads();
  for (int c = threadIdx.x; c < d; c += NT) {
    float sg = 0.f, sb = 0.f, sz = 0.f;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
      sg += red[0][w][c];
      sb += red[1][w][c];
      sz += red[2][w][c];
    }
    if (a.dgamma) {
      atomicAdd(a.dgamma + so + c, sg);
      atomicAdd(a.dbeta + so + c, sb);
    }
    if (a.dbias) atomicAdd(a.dbias + so + c, sz);
  }
}

template <typename T>
static void ln_fwd_dispatch(const LnFwd& a, hipStream_t s) {
  dim3 grid((a.M + 3) / 4);
  switch (a.d / 64) {
    case 1: ln_fwd_kernel<T, 1><<<grid, LN_THREADS, 0, s>>>(a); break;
    case 2: ln_fwd_kernel<T, 2><<<grid, LN_THREADS, 0, s>>>(a); break;
    case 4: ln_fwd_kernel<T, 4><<<grid, LN_THREADS, 0, s>>>(a); break;
    case 8: ln_fwd_kernel<T, 8><<<grid, LN_THREADS, 0, s>>>(a); break;
    case 16: ln_fwd_kernel<T, 16><<<grid, LN_THREADS, 0, s>>>(a); break;
    default: throw Error("layernorm: width must be 64 * {1,2,4,8,16}");
  }
}
void layernorm_fwd(const LnFwd& a, DType t, hipStream_t s) {
  if (a.M <= 0 || (skip_mask() & 1)) return;
  if (hz::active()) {
    using namespace hz;
    const int64_t row = a.d * (int64_t)dsize(t);
    op(s, "ln_fwd", {rd(a.a, a.M * row), rd(a.a_bias, a.d * 4), rd(a.res, a.M * row), rd(a.pe, (int64_t)a.pe_L * a.d * 4),
                     rd(a.gamma, a.d * 4), rd(a.beta, a.d * 4), blk(a.mask.ids, a.M, 4, a.mask.ids_ld * 4, RD),
                     rd(a.mask.valid, a.M), rd(a.drop.seed_ptr, 8), wr(a.y, a.M * row), wr(a.v_save, a.M * row),
                     wr(a.mean, a.M * 4), wr(a.rstd, a.M * 4)});
  }
  if (t == DType::F32) ln_fwd_dispatch<float>(a, s);
  else ln_fwd_dispatch<bf16>(a, s);
  CAPGEN_HIP(hipGetLastError());
}

// 8 rows (waves) per workgroup: half the workgroups -- and half the striped gamma / beta / bias
// atomics -- of the 4-row form (round 5: 2.699-2.703 vs 2.726-2.757 ms/step, three alternating rounds;
// the class 119 vs 137 us/step; 16 rows per workgroup: 2.711-2.716 vs 2.678-2.707 ms, slower)
#ifndef CAPGEN_LNB_NT
#define CAPGEN_LNB_NT 512
#endif
template <typename T, int DPL>
static void ln_bwd_launch(const LnBwd& a, hipStream_t s) {
  // (the per-wave partial sums take 3 * NT * DPL floats of LDS: the widest rows keep 8 waves)
  constexpr int NT = DPL * CAPGEN_LNB_NT > 8 * 1024 ? 512 : CAPGEN_LNB_NT, W = NT / 64;  // one row per wave
  ln_bwd_kernel<T, DPL, NT><<<(a.M + W - 1) / W, NT, 0, s>>>(a);
}
template <typename T>
static void ln_bwd_dispatch(const LnBwd& a, hipStream_t s) {
  switch (a.d / 64) {
    case 1: ln_bwd_launch<T, 1>(a, s); break;
    case 2: ln_bwd_launch<T, 2>(a, s); break;
    case 4: ln_bwd_launch<T, 4>(a, s); break;
    case 8: ln_bwd_launch<T, 8>(a, s); break;
    case 16: ln_bwd_launch<T, 16>(a, s); break;
    default: throw Error("layernorm: width must be 64 * {1,2,4,8,16}");
  }
}
void layernorm_bwd(const LnBwd& a_in, DType t, hipStream_t s) {
  if (a_in.M <= 0 || (skip_mask() & 4)) return;
  LnBwd a = a_in;  // (the diagnostic skip below clears its sum pointers)
  if (hz::active()) {
    using namespace hz;
    const int64_t row = a.d * (int64_t)dsize(t), sb = a.d * 4, ss = std::max<int64_t>(a.stripe_stride * 4, sb);
    op(s, "ln_bwd", {rd(a.dy, a.M * row), rd(a.v, a.M * row), rd(a.mean, a.M * 4), rd(a.rstd, a.M * 4),
                     rd(a.gamma, a.d * 4), blk(a.mask.ids, a.M, 4, a.mask.ids_ld * 4, RD), rd(a.mask.valid, a.M),
                     rd(a.drop.seed_ptr, 8), wr(a.d_res, a.M * row), wr(a.d_a, a.M * row),
                     blk(a.dgamma, a.stripes, sb, ss, ACC), blk(a.dbeta, a.stripes, sb, ss, ACC),
                     blk(a.dbias, a.stripes, sb, ss, ACC)});
  }
  if (skip_mask() & 128) a.dgamma = a.dbeta = a.dbias = nullptr;  // diagnostic: no parameter-gradient sums
  if (t == DType::F32) ln_bwd_dispatch<float>(a, s);
  else ln_bwd_dispatch<bf16>(a, s);
  CAPGEN_HIP(hipGetLastError());
}

// ---------------------------------------------------------------------------------------
template <typename TI, typename TO>
__global__ void __launch_bounds__(256) pack_kernel(const TI* __restrict__ feats, const float* __restrict__ pos,
                                                   const int32_t* __restrict__ img_idx, int n_img, int N, int F, int P,
                                                   int Kp, int M, TO* __restrict__ out, uint8_t* __restrict__ valid,
                                                   uint64_t* seed_bump) {
  // one wave per row m = (b, n), four rows per workgroup (round 6: the row-per-workgroup form spent its
  // time on a workgroup barrier pair and an LDS atomic per position element; the region flag is now a
  // wave ballot).  Features: 16-B loads, every load of the row issued before its stores.
  constexpr int V = 16 / sizeof(TI);
  const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
  // the step's dropout seed advance rides along: nothing in this launch reads the seed
  if (seed_bump && blockIdx.x == 0 && threadIdx.x == 0) *seed_bump += 0x9E3779B97F4A7C15ull;
  if (m >= M) return;  // (whole waves; no workgroup barrier in this kernel)
  // with img_idx the features / positions of image img_idx[b] are read straight from an HBM-resident
  // store (dataset.py:12-18 + DataLoader collate, fused)
  int64_t src = m;
  TO* o = out + (int64_t)m * Kp;
  if (img_idx) {
    const int img = img_idx[m / N];
    if (img < 0 || img >= n_img) {  // out-of-range image: an all-padding row, never an OOB read
      for (int c = lane; c < Kp; c += 64) o[c] = from_f<TO>(0.f);
      if (lane == 0) valid[m] = 0;
      return;
    }
    src = (int64_t)img * N + m % N;
  }
  const TI* f = feats + src * F;
  const float* p = pos + src * P;
  typedef typename Vec16<TI>::type VT;
  constexpr int U = 4;  // 16-B loads in flight per lane
  for (int c0 = lane * V; c0 < F; c0 += 64 * V * U) {
    VT v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u * 64 * V;
      if (c < F) v[u] = *reinterpret_cast<const VT*>(f + c);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int c = c0 + u * 64 * V;
      if (c >= F) break;
      const TI* e = reinterpret_cast<const TI*>(&v[u]);
      float x[V];
#pragma unroll
      for (int j = 0; j < V; ++j) x[j] = to_f(e[j]);
      store_f<TO, V>(o + c, x);
    }
  }
  // positions, then zeros to Kp; a region is padding iff its position row is all zero (model.py:206)
  bool nz = false;
  for (int c = F + lane; c < Kp; c += 64) {
    float x = 0.f;
    if (c < F + P) {
      x = p[c - F];
      nz |= x != 0.f;
    }
    o[c] = from_f<TO>(x);
  }
  const bool any = __ballot(nz) != 0;
  if (lane == 0) valid[m] = any ? 1 : 0;
}

void pack_encoder_input(const void* feats, DType ft, const float* pos, int M, int F, int P, int Kp, void* out,
                        DType ot, uint8_t* valid, hipStream_t s, const int32_t* img_idx, int N, int n_img,
                        uint64_t* seed_bump) {
  if (M <= 0) return;
  require(F % 8 == 0 && ((uintptr_t)feats & 15) == 0, "pack: feature width must be a multiple of 8, 16-B aligned");
  require(img_idx == nullptr || N > 0, "pack: indexed gather needs N");
  if (hz::active()) {
    using namespace hz;
    const int64_t src_rows = img_idx ? (int64_t)n_img * N : M;
    op(s, "pack", {rd(feats, src_rows * F * (int64_t)dsize(ft)), rd(pos, src_rows * P * 4), rd(img_idx, img_idx ? M / N * 4 : 0),
                   wr(out, (int64_t)M * Kp * dsize(ot)), wr(valid, M), wr(seed_bump, 8)});
  }
  dim3 grid((M + 3) / 4);
  if (ft == DType::F32 && ot == DType::F32)
    pack_kernel<float, float><<<grid, 256, 0, s>>>((const float*)feats, pos, img_idx, n_img, N, F, P, Kp, M, (float*)out, valid, seed_bump);
  else if (ft == DType::F32 && ot == DType::BF16)
    pack_kernel<float, bf16><<<grid, 256, 0, s>>>((const float*)feats, pos, img_idx, n_img, N, F, P, Kp, M, (bf16*)out, valid, seed_bump);
  else if (ft == DType::BF16 && ot == DType::BF16)
    pack_kernel<bf16, bf16><<<grid, 256, 0, s>>>((const bf16*)feats, pos, img_idx, n_img, N, F, P, Kp, M, (bf16*)out, valid, seed_bump);
  else
    pack_kernel<bf16, float><<<grid, 256, 0, s>>>((const bf16*)feats, pos, img_idx, n_img, N, F, P, Kp, M, (float*)out, valid, seed_bump);
  CAPGEN_HIP(hipGetLastError());
}

__global__ void prep_caps_kernel(const int32_t* __restrict__ caps, int B, int T, int pad, int32_t* ids_in,
                                 int32_t* tgt, float* count, uint64_t* seed_bump, float* inv_count) {
  __shared__ int cnt;
  if (threadIdx.x == 0) cnt = 0;
  // the step's dropout seed advance (bump_seed) rides along: no kernel in this launch reads it
  if (seed_bump && threadIdx.x == 0) *seed_bump += 0x9E3779B97F4A7C15ull;
  __syncthreads();
  const int L = T - 1;
  int local = 0;
  for (int c = threadIdx.x; c < B * L; c += blockDim.x) {
    int b = c / L, t = c % L;
    ids_in[c] = caps[b * T + t];
    int y = caps[b * T + t + 1];
    tgt[c] = y;
    local += (y != pad);
  }
  atomicAdd(&cnt, local);
  __syncthreads();
  if (threadIdx.x == 0) *count = (float)cnt;
  if (inv_count && threadIdx.x == 0) *inv_count = 1.f / (float)cnt;  // as loss_finalize's 1.f / n
}

void prepare_captions(const int32_t* caps, int B, int T, int pad, int32_t* ids_in, int32_t* tgt, float* count,
                      hipStream_t s, uint64_t* seed_bump, float* inv_count) {
  if (hz::active()) {
    using namespace hz;
    op(s, "prep_captions", {rd(caps, (int64_t)B * T * 4), wr(ids_in, (int64_t)B * (T - 1) * 4),
                            wr(tgt, (int64_t)B * (T - 1) * 4), wr(count, 4), wr(seed_bump, 8), wr(inv_count, 4)});
  }
  prep_caps_kernel<<<1, 1024, 0, s>>>(caps, B, T, pad, ids_in, tgt, count, seed_bump, inv_count);
  CAPGEN_HIP(hipGetLastError());
}

template <typename T>
__global__ void gather_kernel(const float* __restrict__ table, const int32_t* __restrict__ ids, int64_t ids_ld,
                              int M, int d, T* __restrict__ out) {
  int64_t n = (int64_t)M * d;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = c / d;
    int col = c % d;
    out[c] = from_f<T>(table[(int64_t)ids[m * ids_ld] * d + col]);
  }
}
void embedding_gather(const float* table, const int32_t* ids, int64_t ids_ld, int M, int d, void* out, DType t,
                      hipStream_t s, int64_t table_rows) {
  if (M <= 0) return;
  if (hz::active())
    hz::op(s, "emb_gather", {hz::rd(table, table_rows * d * 4), hz::blk(ids, M, 4, ids_ld * 4, hz::RD),
                             hz::wr(out, (int64_t)M * d * dsize(t))});
  int64_t n = (int64_t)M * d;
  int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
  if (t == DType::F32) gather_kernel<float><<<grid, 256, 0, s>>>(table, ids, ids_ld, M, d, (float*)out);
  else gather_kernel<bf16><<<grid, 256, 0, s>>>(table, ids, ids_ld, M, d, (bf16*)out);
  CAPGEN_HIP(hipGetLastError());
}

template <typename T>
__global__ void scatter_kernel(const T* __restrict__ dE, const int32_t* __restrict__ ids, int M, int d, int pad,
                               float* __restrict__ grad) {
  int64_t n = (int64_t)M * d;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < n; c += (int64_t)gridDim.x * blockDim.x) {
    int64_t m = c / d;
    int id = ids[m];
    if (id == pad) continue;
    atomicAdd(grad + (int64_t)id * d + (c % d), to_f(dE[c]));
  }
}
void embedding_scatter_add(const void* dE, const int32_t* ids, int M, int d, int pad, float* grad, DType t,
                           hipStream_t s, int64_t table_rows) {
  if (M <= 0) return;
  if (hz::active())
    hz::op(s, "emb_scatter", {hz::rd(dE, (int64_t)M * d * dsize(t)), hz::rd(ids, (int64_t)M * 4),
                              hz::acc(grad, table_rows * d * 4)});
  int64_t n = (int64_t)M * d;
  int grid = (int)std::min<int64_t>((n + 255) / 256, 4096);
  if (t == DType::F32) scatter_kernel<float><<<grid, 256, 0, s>>>((const float*)dE, ids, M, d, pad, grad);
  else scatter_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)dE, ids, M, d, pad, grad);
  CAPGEN_HIP(hipGetLastError());
}

// db[n] += alpha * sum_m X[m][n]: 16-B loads (a workgroup covers 8 vectors x 32 row lanes x
// 8 rows per lane), rows reduced through LDS, one atomic per column per workgroup
template <typename T>
__global__ void __launch_bounds__(256) colsum_kernel(const T* __restrict__ X, int M, int N, int64_t ldx, float alpha,
                                                     const float* alpha_ptr, float* __restrict__ db, int stripes,
                                                     int64_t stripe_stride) {
  constexpr int V = 16 / sizeof(T);
  __shared__ float red[32][8 * V + 1];
  const int cv = threadIdx.x & 7, rl = threadIdx.x >> 3;
  const int n = (blockIdx.x * 8 + cv) * V;
  float acc[V];
#pragma unroll
  for (int e = 0; e < V; ++e) acc[e] = 0.f;
  if (n < N) {
    const int r0 = blockIdx.y * 256;
#pragma unroll 4
    for (int j = 0; j < 8; ++j) {
      const int m = r0 + rl + 32 * j;
      if (m < M) {
        float x[V];
        load_f<T, V>(X + (int64_t)m * ldx + n, x);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += x[e];
      }
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) red[rl][cv * V + e] = acc[e];
  __syncthreads();
  if (threadIdx.x < 8 * V) {
    const int c = threadIdx.x;
    const int nn = blockIdx.x * 8 * V + c;
    if (nn < N) {
      float sum = 0.f;
      for (int r = 0; r < 32; ++r) sum += red[r][c];
      const float a = alpha_ptr ? alpha * *alpha_ptr : alpha;
      atomicAdd(db + (int64_t)(blockIdx.y % stripes) * stripe_stride + nn, a * sum);
    }
  }
}
void column_sum(const void* X, int M, int N, int64_t ldx, float alpha, const float* alpha_ptr, float* db, DType t,
                hipStream_t s, int stripes, int64_t stripe_stride) {
  if (M <= 0 || N <= 0) return;
  const int V = t == DType::F32 ? 4 : 8;
  require(N % V == 0 && ldx % V == 0, "column_sum: N/ld must be multiples of 16 B");
  if (hz::active()) {
    using namespace hz;
    op(s, "column_sum", {blk(X, M, N * (int64_t)dsize(t), ldx * (int64_t)dsize(t), RD), rd(alpha_ptr, 4),
                         blk(db, stripes, N * 4, std::max<int64_t>(stripe_stride * 4, N * 4), ACC)});
  }
  dim3 grid((N + 8 * V - 1) / (8 * V), (M + 255) / 256);
  if (t == DType::F32) colsum_kernel<float><<<grid, 256, 0, s>>>((const float*)X, M, N, ldx, alpha, alpha_ptr, db, stripes,
                                                               stripe_stride);
  else colsum_kernel<bf16><<<grid, 256, 0, s>>>((const bf16*)X, M, N, ldx, alpha, alpha_ptr, db, stripes,
                                                              stripe_stride);
  CAPGEN_HIP(hipGetLastError());
}

__global__ void stripe_reduce_kernel(float* __restrict__ S, int stripes, int64_t stride, int64_t n,
                                     float* __restrict__ dst, int accumulate, int clear) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float acc = accumulate ? dst[i] : 0.f;
    for (int k = 0; k < stripes; ++k) acc += S[k * stride + i];
    dst[i] = acc;
    if (clear)
      for (int k = 0; k < stripes; ++k) S[k * stride + i] = 0.f;
  }
}
void stripe_reduce(float* S, int stripes, int64_t stride, int64_t n, float* dst, int accumulate, hipStream_t s,
                   int clear) {
  if (n <= 0) return;
  if (hz::active()) {
    using namespace hz;
    const int64_t ss = std::max<int64_t>(stride * 4, n * 4);
    op(s, "stripe_reduce", {blk(S, stripes, n * 4, ss, clear ? WR : RD), blk(S, stripes, n * 4, ss, RD), wr(dst, n * 4),
                            accumulate ? rd(dst, n * 4) : Rgn{}});
  }
  int grid = (int)std::min<int64_t>((n + 255) / 256, 1024);
  stripe_reduce_kernel<<<grid, 256, 0, s>>>(S, stripes, stride, n, dst, accumulate, clear);
  CAPGEN_HIP(hipGetLastError());
}

// WT (all three CE kernels): the row's loss and gradient are scaled by the per-caption weight
// row_w[m / rows_per_w] (capgen_train_step_weighted); WT = false is the unweighted code, row_w unread.
template <typename T, bool WT>
__global__ void __launch_bounds__(256) ce_kernel(const float* __restrict__ logits, const int32_t* __restrict__ tgt,
                                                 int V, int pad, float* __restrict__ loss_row, T* __restrict__ dl,
                                                 const float* __restrict__ row_w, int rows_per_w) {
  __shared__ float sh[4];
  const int m = blockIdx.x;
  const float* x = logits + (int64_t)m * V;
  T* g = dl + (int64_t)m * V;
  const int y = tgt[m];
  float w = 1.f;
  if constexpr (WT) w = row_w[m / rows_per_w];
  if (y == pad) {
    for (int c = threadIdx.x; c < V; c += 256) g[c] = from_f<T>(0.f);
    if (threadIdx.x == 0) loss_row[m] = 0.f;
    return;
  }
  float mx = -INFINITY;
  for (int c = threadIdx.x; c < V; c += 256) mx = fmaxf(mx, x[c]);
  mx = block_max(mx, sh);
  float se = 0.f;
  for (int c = threadIdx.x; c < V; c += 256) se += expf(x[c] - mx);
  se = block_sum_pairwise(se, sh);
  const float inv = 1.f / se;
  for (int c = threadIdx.x; c < V; c += 256) {
    float p = expf(x[c] - mx) * inv;
    float o = p - (c == y ? 1.f : 0.f);
    if constexpr (WT) o *= w;
    g[c] = from_f<T>(o);
  }
  if (threadIdx.x == 0) {
    const float l = (logf(se) + mx) - x[y];
    loss_row[m] = WT ? w * l : l;
  }
}
// Register-resident variant (V % 4 == 0, V <= 1024 * NV4): the row is loaded ONCE as float4s
// (every load in flight together: one memory round trip instead of three dependent passes),
// max / sum-exp / gradient are computed from registers.
template <typename T, int NV4, bool WT>
__global__ void __launch_bounds__(256) ce_reg_kernel(const float* __restrict__ logits, const int32_t* __restrict__ tgt,
                                                     int V, int pad, float* __restrict__ loss_row, T* __restrict__ dl,
                                                     const float* __restrict__ row_w, int rows_per_w) {
  __shared__ float sh[4];
  const int m = blockIdx.x, V4 = V >> 2;
  const float4* x = reinterpret_cast<const float4*>(logits + (int64_t)m * V);
  T* g = dl + (int64_t)m * V;
  const int y = tgt[m];
  float w = 1.f;
  if constexpr (WT) w = row_w[m / rows_per_w];
  if (y == pad) {
    for (int c = threadIdx.x; c < V; c += 256) g[c] = from_f<T>(0.f);
    if (threadIdx.x == 0) loss_row[m] = 0.f;
    return;
  }
  float4 v[NV4];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < NV4; ++u) {
    const int c4 = threadIdx.x + 256 * u;
    v[u] = c4 < V4 ? x[c4] : float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
  }
#pragma unroll
  for (int u = 0; u < NV4; ++u) mx = fmaxf(mx, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
  mx = block_max(mx, sh);
  float se = 0.f;
#pragma unroll
  for (int u = 0; u < NV4; ++u) {
    v[u].x = expf(v[u].x - mx), v[u].y = expf(v[u].y - mx), v[u].z = expf(v[u].z - mx), v[u].w = expf(v[u].w - mx);
    se += (v[u].x + v[u].y) + (v[u].z + v[u].w);
  }
  se = block_sum_pairwise(se, sh);
  const float inv = 1.f / se;
#pragma unroll
  for (int u = 0; u < NV4; ++u) {
    const int c4 = threadIdx.x + 256 * u;
    if (c4 >= V4) continue;
    const int c = 4 * c4;
    float o[4] = {v[u].x * inv, v[u].y * inv, v[u].z * inv, v[u].w * inv};
    if (y >= c && y < c + 4) o[y - c] -= 1.f;
    if constexpr (WT) o[0] *= w, o[1] *= w, o[2] *= w, o[3] *= w;
    store_f<T, 4>(g + c, o);
  }
  if (threadIdx.x == 0) {
    const float l = (logf(se) + mx) - logits[(int64_t)m * V + y];
    loss_row[m] = WT ? w * l : l;
  }
}

template <typename T, bool WT>
static void ce_launch(const float* logits, const int32_t* tgt, int M, int V, int pad, float* loss_row, T* dl,
                      const float* row_w, int rows_per_w, hipStream_t s) {
  if (V % 4 == 0 && V <= 1024 * 16) {
    const int nv4 = (V / 4 + 255) / 256;
    if (nv4 <= 4) ce_reg_kernel<T, 4, WT><<<M, 256, 0, s>>>(logits, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
    else if (nv4 <= 8) ce_reg_kernel<T, 8, WT><<<M, 256, 0, s>>>(logits, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
    else if (nv4 <= 10) ce_reg_kernel<T, 10, WT><<<M, 256, 0, s>>>(logits, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
    else ce_reg_kernel<T, 16, WT><<<M, 256, 0, s>>>(logits, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
  } else {
    ce_kernel<T, WT><<<M, 256, 0, s>>>(logits, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
  }
}
// row_w != null: row m is weighted by row_w[m / rows_per_w] (M / rows_per_w weights)
static void check_row_w(const char* who, const float* row_w, int rows_per_w, int M) {
  if (!row_w) return;
  require(rows_per_w >= 1 && M % rows_per_w == 0,
          std::string(who) + ": rows_per_w must be >= 1 and divide M");
}
void cross_entropy_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, float* loss_row, void* dl,
                        DType t, hipStream_t s, const float* row_w, int rows_per_w) {
  if (M <= 0) return;
  check_row_w("cross_entropy_rows", row_w, rows_per_w, M);
  if (hz::active()) {
    std::vector<hz::Rgn> r = {hz::rd(logits, (int64_t)M * V * 4), hz::rd(tgt, (int64_t)M * 4),
                                hz::wr(loss_row, (int64_t)M * 4), hz::wr(dl, (int64_t)M * V * dsize(t))};
    if (row_w) r.push_back(hz::rd(row_w, (int64_t)(M / rows_per_w) * 4));
    hz::op(s, "cross_entropy", r.data(), r.size());
  }
  if (t == DType::F32) {
    if (row_w) ce_launch<float, true>(logits, tgt, M, V, pad, loss_row, (float*)dl, row_w, rows_per_w, s);
    else ce_launch<float, false>(logits, tgt, M, V, pad, loss_row, (float*)dl, nullptr, 1, s);
  } else {
    if (row_w) ce_launch<bf16, true>(logits, tgt, M, V, pad, loss_row, (bf16*)dl, row_w, rows_per_w, s);
    else ce_launch<bf16, false>(logits, tgt, M, V, pad, loss_row, (bf16*)dl, nullptr, 1, s);
  }
  CAPGEN_HIP(hipGetLastError());
}

// Second half of the fused classifier + cross entropy (GemmArgs::ce_stats): the classifier GEMM
// left e = exp(v - mx_c) in bf16 and {mx_c, s_c} per 16-column slab c of each row.  One
// workgroup per row: lse = M + log sum_c s_c exp(mx_c - M), loss_row = lse - v[tgt], and the
// row is rewritten in place as softmax - onehot = e * exp(mx_c - lse) - onehot.  Every load of the
// row (stats + the thread's slabs) is issued up front: one memory round trip.
template <int SPT, int VW, bool WT>
__global__ void __launch_bounds__(256) ce_finish_kernel(const float2* __restrict__ stats, int64_t ld,
                                                        const float* __restrict__ tlogit,
                                                        const int32_t* __restrict__ tgt, int V, int pad,
                                                        float* __restrict__ loss_row, bf16* __restrict__ dl,
                                                        const float* __restrict__ row_w, int rows_per_w) {
  // VW = elements per access: 8 (16-B loads / stores, rows 16-B aligned: V % 8 == 0) or 4
  __shared__ float sh[4];
  typedef __attribute__((ext_vector_type(VW))) __bf16 bv;
  constexpr int NQ = 16 / VW;  // accesses per 16-column slab
  const int m = blockIdx.x, nsl = (V + 15) / 16;
  bf16* row = dl + (int64_t)m * V;
  // every load first -- target, target logit, caption weight, slab stats, the row's e values -- from
  // clamped in-range addresses with no branch around them (a load in a branch is waited for at its join):
  // one round trip
  const int y = tgt[m];
  const float tl = tlogit[m];
  float w = 1.f;
  if constexpr (WT) w = row_w[m / rows_per_w];
  float2 st[SPT];
  bv e[SPT][NQ];
#pragma unroll
  for (int u = 0; u < SPT; ++u) {
    const int c = threadIdx.x + 256 * u, cc = min(c, nsl - 1);
    st[u] = stats[(int64_t)m * ld + cc];
#pragma unroll
    for (int q = 0; q < NQ; ++q) e[u][q] = *reinterpret_cast<const bv*>(row + min(cc * 16 + q * VW, V - VW));
  }
#pragma unroll
  for (int u = 0; u < SPT; ++u)
    if (threadIdx.x + 256 * u >= nsl) st[u] = float2{-INFINITY, 0.f};
  if (y == pad) {  // (uniform per workgroup)
    for (int c = threadIdx.x * VW; c < V; c += 256 * VW) *reinterpret_cast<bv*>(row + c) = bv{};
    if (threadIdx.x == 0) loss_row[m] = 0.f;
    return;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < SPT; ++u) mx = fmaxf(mx, st[u].x);
  mx = block_max(mx, sh);
  float se = 0.f;
#pragma unroll
  for (int u = 0; u < SPT; ++u) se += st[u].y == 0.f ? 0.f : st[u].y * expf(st[u].x - mx);
  se = block_sum_pairwise(se, sh);
  const float lse = mx + logf(se);
#pragma unroll
  for (int u = 0; u < SPT; ++u) {
    const int c = threadIdx.x + 256 * u;
    if (c >= nsl) continue;
    const float f = expf(st[u].x - lse);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int col = c * 16 + q * VW;
      if (col >= V) continue;
      bv o;
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        float x = (float)e[u][q][i] * f;
        if (y == col + i) x -= 1.f;
        if constexpr (WT) x *= w;
        o[i] = (bf16)x;
      }
      *reinterpret_cast<bv*>(row + col) = o;
    }
  }
  if (threadIdx.x == 0) loss_row[m] = WT ? w * (lse - tl) : lse - tl;
}
void ce_finish(const float2* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V, int pad,
               float* loss_row, bf16* dl, hipStream_t s, const float* row_w, int rows_per_w) {
  if (M <= 0) return;
  require(V % 4 == 0 && ld >= (V + 15) / 16, "ce_finish: V must be a multiple of 4");
  check_row_w("ce_finish", row_w, rows_per_w, M);
  if (hz::active()) {
    using namespace hz;
    std::vector<Rgn> r = {blk(stats, M, (int64_t)((V + 15) / 16) * 8, ld * 8, RD), rd(tlogit, (int64_t)M * 4),
                            rd(tgt, (int64_t)M * 4), wr(loss_row, (int64_t)M * 4), wr(dl, (int64_t)M * V * 2)};
    if (row_w) r.push_back(rd(row_w, (int64_t)(M / rows_per_w) * 4));
    op(s, "ce_finish", r.data(), r.size());
  }
  const int spt = ((V + 15) / 16 + 255) / 256;
  // 16-B accesses when every row starts 16-B aligned (Knob::CeVec8 = 0: the 8-B form, bit-identity test)
  const bool v8 = knob(Knob::CeVec8) != 0 && V % 8 == 0 && ((uintptr_t)dl & 15) == 0;
  auto go = [&](auto spt_c) {
    constexpr int S = decltype(spt_c)::value;
    if (row_w) {
      if (v8) ce_finish_kernel<S, 8, true><<<M, 256, 0, s>>>(stats, ld, tlogit, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
      else ce_finish_kernel<S, 4, true><<<M, 256, 0, s>>>(stats, ld, tlogit, tgt, V, pad, loss_row, dl, row_w, rows_per_w);
    } else {
      if (v8) ce_finish_kernel<S, 8, false><<<M, 256, 0, s>>>(stats, ld, tlogit, tgt, V, pad, loss_row, dl, nullptr, 1);
      else ce_finish_kernel<S, 4, false><<<M, 256, 0, s>>>(stats, ld, tlogit, tgt, V, pad, loss_row, dl, nullptr, 1);
    }
  };
  if (spt <= 1) go(std::integral_constant<int, 1>{});
  else if (spt <= 2) go(std::integral_constant<int, 2>{});
  else if (spt <= 3) go(std::integral_constant<int, 3>{});
  else if (spt <= 4) go(std::integral_constant<int, 4>{});
  else if (spt <= 8) go(std::integral_constant<int, 8>{});
  else throw Error("ce_finish: V > 32768");
  CAPGEN_HIP(hipGetLastError());
}

// ---- scoring given captions: per-row log-probability and teacher-forced hit, per-caption sums ---------
// The forward's read-out without a backward: nothing of size M x V is written, no loss word.
// One workgroup per row, as the CE kernels: the row's max / sum-exp come from ONE pass (register form:
// the row loaded once as float4s, clamped addresses, no branch around a load; generic form: a running
// {max, sum} per thread), the target logit from one more 4-byte load issued with them.
__device__ __forceinline__ void score_row_write(int m, int y, int pad, float tl, float mx, float se,
                                                float* __restrict__ token_logp, int32_t* __restrict__ hit) {
  const bool kept = y != pad;
  token_logp[m] = kept ? tl - (mx + logf(se)) : 0.f;
  hit[m] = kept && tl >= mx ? 1 : 0;
}
template <int NV4>
__global__ void __launch_bounds__(256) score_reg_kernel(const float* __restrict__ logits, const int32_t* __restrict__ tgt,
                                                        int V, int pad, float* __restrict__ token_logp,
                                                        int32_t* __restrict__ hit) {
  __shared__ float sh[4];
  const int m = blockIdx.x, V4 = V >> 2;
  const float4* x = reinterpret_cast<const float4*>(logits + (int64_t)m * V);
  const int y = tgt[m];
  float4 v[NV4];
#pragma unroll
  for (int u = 0; u < NV4; ++u) v[u] = x[min((int)threadIdx.x + 256 * u, V4 - 1)];
  const float tl = logits[(int64_t)m * V + min(max(y, 0), V - 1)];
  float mx = -INFINITY;
#pragma unroll
  for (int u = 0; u < NV4; ++u) {
    if ((int)threadIdx.x + 256 * u >= V4) v[u] = float4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    mx = fmaxf(mx, fmaxf(fmaxf(v[u].x, v[u].y), fmaxf(v[u].z, v[u].w)));
  }
  mx = block_max(mx, sh);
  float se = 0.f;
#pragma unroll
  for (int u = 0; u < NV4; ++u)
    se += (expf(v[u].x - mx) + expf(v[u].y - mx)) + (expf(v[u].z - mx) + expf(v[u].w - mx));
  se = block_sum_pairwise(se, sh);
  if (threadIdx.x == 0) score_row_write(m, y, pad, tl, mx, se, token_logp, hit);
}
__global__ void __launch_bounds__(256) score_gen_kernel(const float* __restrict__ logits, const int32_t* __restrict__ tgt,
                                                        int V, int pad, float* __restrict__ token_logp,
                                                        int32_t* __restrict__ hit) {
  __shared__ float sh[4];
  const int m = blockIdx.x;
  const float* x = logits + (int64_t)m * V;
  const int y = tgt[m];
  const float tl = x[min(max(y, 0), V - 1)];
  float tm = -INFINITY, ts = 0.f;  // the thread's running max and sum exp(x - tm)
  for (int c = threadIdx.x; c < V; c += 256) {
    const float xv = x[c];
    if (xv > tm) ts = ts * expf(tm - xv) + 1.f, tm = xv;  // (tm = -inf: ts = 0 * 0 + 1)
    else if (xv > -INFINITY) ts += expf(xv - tm);
  }
  const float mx = block_max(tm, sh);
  const float se = block_sum_pairwise(ts == 0.f ? 0.f : ts * expf(tm - mx), sh);
  if (threadIdx.x == 0) score_row_write(m, y, pad, tl, mx, se, token_logp, hit);
}
// caption r = rows [r * Lq, (r + 1) * Lq): logp = their token_logp added in row order, length = kept
// rows, hits = their hits.  One thread per caption, a fixed order: two runs give the same bits.
__global__ void __launch_bounds__(256) score_caption_kernel(const float* __restrict__ token_logp,
                                                            const int32_t* __restrict__ hit,
                                                            const int32_t* __restrict__ tgt, int R, int Lq, int pad,
                                                            float* __restrict__ logp, int32_t* __restrict__ length,
                                                            int32_t* __restrict__ hits) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= R) return;
  float acc = 0.f;
  int n = 0, h = 0;
  for (int t = 0; t < Lq; ++t) {
    const int m = r * Lq + t;
    acc += token_logp[m];
    n += tgt[m] != pad;
    h += hit[m];
  }
  logp[r] = acc;
  if (length) length[r] = n;
  if (hits) hits[r] = h;
}
static void check_score_args(const char* who, const void* a, const void* b, const int32_t* tgt, int M, int V,
                             int rows_per_caption, const float* logp) {
  const std::string w(who);
  require(a && b && tgt && logp, w + ": a null input or logp");
  require(M >= 1 && V >= 1, w + ": M and V must be >= 1");
  require(rows_per_caption >= 1 && M % rows_per_caption == 0, w + ": rows_per_caption must be >= 1 and divide M");
}
void score_rows(const float* logits, const int32_t* tgt, int M, int V, int pad, int rows_per_caption,
                float* token_logp, int32_t* hit, float* logp, int32_t* length, int32_t* hits, hipStream_t s) {
  check_score_args("score_rows", logits, token_logp, tgt, M, V, rows_per_caption, logp);
  require(hit != nullptr, "score_rows: hit is null");
  const int R = M / rows_per_caption;
  if (hz::active()) {
    using namespace hz;
    op(s, "score_rows", {rd(logits, (int64_t)M * V * 4), rd(tgt, (int64_t)M * 4), wr(token_logp, (int64_t)M * 4),
                         wr(hit, (int64_t)M * 4)});
    op(s, "score_caption", {rd(token_logp, (int64_t)M * 4), rd(hit, (int64_t)M * 4), rd(tgt, (int64_t)M * 4),
                            wr(logp, (int64_t)R * 4), wr(length, (int64_t)R * 4), wr(hits, (int64_t)R * 4)});
  }
  if (V % 4 == 0 && V <= 1024 * 16) {  // ce_reg_kernel's condition and its register forms
    const int nv4 = (V / 4 + 255) / 256;
    if (nv4 <= 4) score_reg_kernel<4><<<M, 256, 0, s>>>(logits, tgt, V, pad, token_logp, hit);
    else if (nv4 <= 8) score_reg_kernel<8><<<M, 256, 0, s>>>(logits, tgt, V, pad, token_logp, hit);
    else if (nv4 <= 10) score_reg_kernel<10><<<M, 256, 0, s>>>(logits, tgt, V, pad, token_logp, hit);
    else score_reg_kernel<16><<<M, 256, 0, s>>>(logits, tgt, V, pad, token_logp, hit);
  } else {
    score_gen_kernel<<<M, 256, 0, s>>>(logits, tgt, V, pad, token_logp, hit);
  }
  score_caption_kernel<<<(R + 255) / 256, 256, 0, s>>>(token_logp, hit, tgt, R, rows_per_caption, pad, logp, length,
                                                      hits);
  CAPGEN_HIP(hipGetLastError());
}

// The fused classifier's read-out (GemmArgs::ce_stats): a row's log-probability needs only its V / 16
// {mx_c, s_c} pairs and the target logit -- the e rows are not an argument.  One workgroup per caption,
// one wave per row (waves stride the caption's rows): a lane holds SPT pairs (8-byte loads: with an odd
// ld, 625 at V = 10000, rows start 8-byte aligned only), every load of the row issued up front from
// clamped addresses below the row's slab count, then lse = mx + log sum_c s_c exp(mx_c - mx) by
// cross-lane shuffles.  Wave w adds its rows' log-probabilities in row order, thread 0 the waves' sums in
// wave order: a fixed order, no atomics.
constexpr int SCORE_WAVES = 8;
template <int SPT>
__global__ void __launch_bounds__(64 * SCORE_WAVES) score_finish_kernel(
    const float2* __restrict__ stats, int64_t ld, const float* __restrict__ tlogit, const int32_t* __restrict__ tgt,
    int V, int pad, int Lq, float* __restrict__ token_logp, int32_t* __restrict__ hit, float* __restrict__ logp,
    int32_t* __restrict__ length, int32_t* __restrict__ hits) {
  __shared__ float sh_lp[SCORE_WAVES];
  __shared__ int sh_n[SCORE_WAVES], sh_h[SCORE_WAVES];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6, nsl = (V + 15) / 16;
  float acc = 0.f;
  int n = 0, h = 0;
  for (int t = wv; t < Lq; t += SCORE_WAVES) {  // (uniform per wave)
    const int m = r * Lq + t;
    const int y = tgt[m];
    const float tl = tlogit[m];
    float2 st[SPT];
#pragma unroll
    for (int u = 0; u < SPT; ++u) st[u] = stats[(int64_t)m * ld + min(lane + 64 * u, nsl - 1)];
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < SPT; ++u) {
      if (lane + 64 * u >= nsl) st[u] = float2{-INFINITY, 0.f};
      mx = fmaxf(mx, st[u].x);
    }
    mx = wave_max(mx);
    float se = 0.f;
#pragma unroll
    for (int u = 0; u < SPT; ++u) se += st[u].y == 0.f ? 0.f : st[u].y * expf(st[u].x - mx);
    se = wave_sum(se);
    const bool kept = y != pad;
    const float lp = kept ? tl - (mx + logf(se)) : 0.f;
    const int hm = kept && tl >= mx ? 1 : 0;
    if (lane == 0) {
      if (token_logp) token_logp[m] = lp;
      if (hit) hit[m] = hm;
    }
    acc += lp, n += kept, h += hm;
  }
  if (lane == 0) sh_lp[wv] = acc, sh_n[wv] = n, sh_h[wv] = h;
  __syncthreads();
  if (threadIdx.x == 0) {
    float a = sh_lp[0];
    int nn = sh_n[0], hh = sh_h[0];
#pragma unroll
    for (int w = 1; w < SCORE_WAVES; ++w) a += sh_lp[w], nn += sh_n[w], hh += sh_h[w];
    logp[r] = a;
    if (length) length[r] = nn;
    if (hits) hits[r] = hh;
  }
}
void score_finish(const float2* stats, int64_t ld, const float* tlogit, const int32_t* tgt, int M, int V, int pad,
                  int rows_per_caption, float* token_logp, int32_t* hit, float* logp, int32_t* length,
                  int32_t* hits, hipStream_t s) {
  check_score_args("score_finish", stats, tlogit, tgt, M, V, rows_per_caption, logp);
  require(V % 4 == 0, "score_finish: V must be a multiple of 4");
  const int nsl = (V + 15) / 16, R = M / rows_per_caption;
  require(ld >= nsl, "score_finish: ld is smaller than the row's slab count");
  require(nsl <= 64 * 32, "score_finish: V > 32768");
  if (hz::active()) {
    using namespace hz;
    op(s, "score_finish", {blk(stats, M, (int64_t)nsl * 8, ld * 8, RD), rd(tlogit, (int64_t)M * 4),
                           rd(tgt, (int64_t)M * 4), wr(token_logp, (int64_t)M * 4), wr(hit, (int64_t)M * 4),
                           wr(logp, (int64_t)R * 4), wr(length, (int64_t)R * 4), wr(hits, (int64_t)R * 4)});
  }
  const int spt = (nsl + 63) / 64;
  auto go = [&](auto spt_c) {
    score_finish_kernel<decltype(spt_c)::value><<<R, 64 * SCORE_WAVES, 0, s>>>(
        stats, ld, tlogit, tgt, V, pad, rows_per_caption, token_logp, hit, logp, length, hits);
  };
  if (spt <= 1) go(std::integral_constant<int, 1>{});
  else if (spt <= 2) go(std::integral_constant<int, 2>{});
  else if (spt <= 4) go(std::integral_constant<int, 4>{});
  else if (spt <= 8) go(std::integral_constant<int, 8>{});
  else if (spt <= 10) go(std::integral_constant<int, 10>{});
  else if (spt <= 16) go(std::integral_constant<int, 16>{});
  else go(std::integral_constant<int, 32>{});
  CAPGEN_HIP(hipGetLastError());
}

// CE mean over the (global) non-pad count and the FocalLoss transform (model.py:73-76,
// loss.py:20-28, gamma = 2, applied to the already-averaged CE).  ce_in != null: the mean CE is
// given (the data-parallel path all-reduces the per-rank partial sums first); partial: only
// the per-rank partial mean sum(rows) / count is written to loss_out.
__global__ void loss_finalize_kernel(const float* __restrict__ loss_row, int M, const float* count, int focal,
                                     const float* ce_in, int partial, float* loss_out, float* grad_scale) {
  __shared__ float sh[4];
  float acc = 0.f;
  if (!ce_in)
    for (int c = threadIdx.x; c < M; c += 256) acc += loss_row[c];
  acc = block_sum_pairwise(acc, sh);
  if (threadIdx.x == 0) {
    const float n = *count;
    const float ce = ce_in ? *ce_in : acc / n;
    if (partial) {
      *loss_out = ce;
    } else if (focal) {
      const float pt = expf(-ce);
      const float om = 1.f - pt;
      *loss_out = om * om * ce;
      if (grad_scale) *grad_scale = (2.f * om * pt * ce + om * om) / n;
    } else {
      *loss_out = ce;
      if (grad_scale) *grad_scale = 1.f / n;
    }
  }
}
void loss_finalize(const float* loss_row, int M, const float* count, int focal, float* loss_out, float* grad_scale,
                   hipStream_t s, const float* ce_in, int partial) {
  if (hz::active())
    hz::op(s, "loss_finalize", {hz::rd(ce_in ? nullptr : loss_row, (int64_t)M * 4), hz::rd(count, 4), hz::rd(ce_in, 4),
                                hz::wr(loss_out, 4), hz::wr(partial ? nullptr : grad_scale, 4)});
  loss_finalize_kernel<<<1, 256, 0, s>>>(loss_row, M, count, focal, ce_in, partial, loss_out, grad_scale);
  CAPGEN_HIP(hipGetLastError());
}

// ---- Adam ---------------------------------------------------------------------------
__global__ void adam_prep_kernel(int64_t* step, float lr, float b1, float b2, float* scal) {
  const int64_t t = ++(*step);
  const double bc1 = 1.0 - pow((double)b1, (double)t);
  const double bc2 = 1.0 - pow((double)b2, (double)t);
  scal[0] = (float)(-(double)lr / bc1);  // value of addcdiv_ (= -step_size)
  scal[1] = (float)sqrt(bc2);            // bias_correction2_sqrt
}
void adam_prepare(int64_t* step, float lr, float b1, float b2, float* scal, hipStream_t s) {
  if (hz::active()) hz::op(s, "adam_prepare", {hz::wr(step, 8), hz::wr(scal, 8)});
  adam_prep_kernel<<<1, 1, 0, s>>>(step, lr, b1, b2, scal);
  CAPGEN_HIP(hipGetLastError());
}
// the same with the learning rate read from a device word (capgen_set_lr: a captured step sees a new
// value without re-capture); the same formula, so an unchanged rate gives the same bits
__global__ void adam_prep_dev_kernel(int64_t* step, const float* lr, float b1, float b2, float* scal) {
  const int64_t t = ++(*step);
  const double bc1 = 1.0 - pow((double)b1, (double)t);
  const double bc2 = 1.0 - pow((double)b2, (double)t);
  scal[0] = (float)(-(double)*lr / bc1);
  scal[1] = (float)sqrt(bc2);
}
// ... and, for the decoupled weight decay (torch.optim.AdamW: p *= 1 - lr * wd before the step's Adam
// update), scal[2] = that factor from the two device words: in double, rounded once
__global__ void adam_prep_wd_kernel(int64_t* step, const float* lr, const float* wd, float b1, float b2, float* scal) {
  const int64_t t = ++(*step);
  const double bc1 = 1.0 - pow((double)b1, (double)t);
  const double bc2 = 1.0 - pow((double)b2, (double)t);
  scal[0] = (float)(-(double)*lr / bc1);
  scal[1] = (float)sqrt(bc2);
  scal[2] = (float)(1.0 - (double)*lr * (double)*wd);
}
void adam_prepare(int64_t* step, const float* lr, float b1, float b2, float* scal, hipStream_t s, const float* wd) {
  require(lr != nullptr, "adam_prepare: null learning-rate word");
  if (wd) {
    if (hz::active()) hz::op(s, "adam_prepare", {hz::rd(lr, 4), hz::rd(wd, 4), hz::wr(step, 8), hz::wr(scal, 12)});
    adam_prep_wd_kernel<<<1, 1, 0, s>>>(step, lr, wd, b1, b2, scal);
  } else {
    if (hz::active()) hz::op(s, "adam_prepare", {hz::rd(lr, 4), hz::wr(step, 8), hz::wr(scal, 8)});
    adam_prep_dev_kernel<<<1, 1, 0, s>>>(step, lr, b1, b2, scal);
  }
  CAPGEN_HIP(hipGetLastError());
}

// Adam streams 30 B per parameter that nothing else in the step reads (f32 params, grads, moments:
// 16 B in, 12 B out) beside the critical chain, so (a) those streams use non-temporal loads and
// stores -- they should not push the chain's GEMM panels out of the L2 / Infinity Cache -- while the
// bf16 shadow and the tiled copies, which the next forward reads, keep the default policy; and (b)
// every thread keeps ADAM_U 16-B loads of each array in flight (4 x ADAM_U loads issued before the
// first use), so one workgroup per CU moves the stream at a useful rate (one load per array per
// iteration measured 3.1 TB/s, round 4).
constexpr int ADAM_U = 4;
typedef float adam_f4 __attribute__((ext_vector_type(4)));  // (the nontemporal builtins take clang vectors)
// Opt empty: the kernel as it was (the same parameters, the same code).  Opt holds const float*: every
// gradient is multiplied by *gscale (the clip coefficient of grad_norm_finish) once, before both
// moment updates.  AdamDecayArg: p *= *factor (the prepare kernel's 1 - lr * wd) before the update, as
// torch.optim.AdamW.  AdamEmaArg: after the update e += (p_new - e) * *rate (rate = 1 - decay:
// torch.optim.swa_utils.get_ema_multi_avg_fn, e.lerp_(p, 1 - decay)); e is one more stream of the
// same kind (16-B non-temporal loads issued with the others, 38 B per parameter instead of 30).
// The options are types of the pack in the order {gscale, decay, ema}: compile-time variants, and the
// two instantiations without them keep their names and their code.
struct AdamDecayArg {
  const float* factor;
};
struct AdamEmaArg {
  adam_f4* e;
  const float* rate;
};
template <class T, class... Opt>
constexpr bool adam_has = (std::is_same_v<T, Opt> || ...);
template <class T, class First, class... Rest>
__device__ __forceinline__ T adam_arg(First first, Rest... rest) {
  if constexpr (std::is_same_v<T, First>) return first;
  else return adam_arg<T>(rest...);
}
template <class... Opt>
__global__ void __launch_bounds__(256) adam_kernel(adam_f4* __restrict__ p, const adam_f4* __restrict__ g,
                                                   adam_f4* __restrict__ m, adam_f4* __restrict__ v, size_t n4,
                                                   float b1, float b2, float eps, const float* __restrict__ scal,
                                                   bf16* __restrict__ shadow, size_t n_shadow, AdamTiles tiles,
                                                   Opt... opt) {
  constexpr bool SCALED = adam_has<const float*, Opt...>, DECAY = adam_has<AdamDecayArg, Opt...>,
                 EMA = adam_has<AdamEmaArg, Opt...>;
  const float neg_step = scal[0], bc2s = scal[1];
  float gs = 1.f;
  if constexpr (SCALED) gs = *adam_arg<const float*>(opt...);
  float keep = 1.f, rate = 0.f;
  adam_f4* __restrict__ e = nullptr;
  if constexpr (DECAY) keep = *adam_arg<AdamDecayArg>(opt...).factor;
  if constexpr (EMA) e = adam_arg<AdamEmaArg>(opt...).e, rate = *adam_arg<AdamEmaArg>(opt...).rate;
  const float b1c = 1.f - b1, b2c = 1.f - b2;
  const size_t stride = (size_t)gridDim.x * 256 * ADAM_U;
  for (size_t base = blockIdx.x * (size_t)(256 * ADAM_U) + threadIdx.x; base < n4; base += stride) {
    adam_f4 pp[ADAM_U], gg[ADAM_U], mm[ADAM_U], vv[ADAM_U], ee[EMA ? ADAM_U : 1];
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      // (a lane past the end re-reads element base: in range, its results are not stored)
      const size_t i = base + (size_t)u * 256 < n4 ? base + (size_t)u * 256 : base;
      pp[u] = __builtin_nontemporal_load(p + i);
      gg[u] = __builtin_nontemporal_load(g + i);
      mm[u] = __builtin_nontemporal_load(m + i);
      vv[u] = __builtin_nontemporal_load(v + i);
      if constexpr (EMA) ee[u] = __builtin_nontemporal_load(e + i);
    }
    // every load above is issued before the first value is consumed (hipcc otherwise sinks each
    // group of loads to its use, leaving one array's load in flight at a time)
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) asm volatile("" : "+v"(pp[u]), "+v"(gg[u]), "+v"(mm[u]), "+v"(vv[u]));
    if constexpr (EMA) {
#pragma unroll
      for (int u = 0; u < ADAM_U; ++u) asm volatile("" : "+v"(ee[u]));
    }
#pragma unroll
    for (int u = 0; u < ADAM_U; ++u) {
      const size_t i = base + (size_t)u * 256;
      if (i >= n4) break;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        float pc = pp[u][c], mc = mm[u][c], vc = vv[u][c];
        float gc = gg[u][c];
        if constexpr (SCALED) gc *= gs;
        if constexpr (DECAY) pc *= keep;
        adam_one(pc, gc, mc, vc, b1c, b2, b2c, eps, neg_step, bc2s);
        pp[u][c] = pc, mm[u][c] = mc, vv[u][c] = vc;
        if constexpr (EMA) ee[u][c] += (pc - ee[u][c]) * rate;
      }
      if constexpr (EMA) __builtin_nontemporal_store(ee[u], e + i);
      __builtin_nontemporal_store(pp[u], p + i);
      __builtin_nontemporal_store(mm[u], m + i);
      __builtin_nontemporal_store(vv[u], v + i);
      if (shadow && 4 * i < n_shadow) {
        typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
        bf16x4 o = {(bf16)pp[u][0], (bf16)pp[u][1], (bf16)pp[u][2], (bf16)pp[u][3]};
        *reinterpret_cast<bf16x4*>(shadow + 4 * i) = o;
        // the fused attention fronts' tiled copy (qkv_tile_weights layout): 4 consecutive k of one
        // row land in one 8-B piece of the row's 16-B fragment slot
#pragma unroll
        for (int t = 0; t < AdamTiles::kMax; ++t) {
          const int64_t rel = (int64_t)(4 * i) - tiles.off[t];
          if (t < tiles.n && rel >= 0 && rel < tiles.len[t]) {
            const int64_t row = rel >> 9;
            const int k = (int)(rel & 511);
            const int64_t piece = (((row >> 4) * 16 + (k >> 5)) * 64 + (row & 15) + 16 * ((k >> 3) & 3)) * 8 + (k & 7);
            *reinterpret_cast<bf16x4*>(tiles.dst[t] + piece) = o;
          }
        }
      }
    }
  }
}
void adam_update(float* p, const float* g, float* m, float* v, size_t n, float b1, float b2, float eps,
                 const float* scal, bf16* shadow, size_t n_shadow, hipStream_t s, int grid_cap,
                 const AdamTiles& tiles, const float* gscale, const AdamOpt& x) {
  require(tiles.n >= 0 && tiles.n <= AdamTiles::kMax, "adam: at most kMax tiled ranges");
  for (int t = 0; t < tiles.n; ++t)
    // (the tile formula needs only the element offset from the matrix start; 4-aligned so a thread's
    // 4 elements stay in one row)
    require(shadow && tiles.off[t] % 4 == 0 && tiles.len[t] % (16 * 512) == 0 && tiles.off[t] >= 0 &&
                tiles.off[t] + tiles.len[t] <= (int64_t)n_shadow && tiles.dst[t],
            "adam: a tiled range must be whole 16-row blocks of 512-wide rows inside the shadow range");
  require(n % 4 == 0 && n_shadow % 4 == 0, "adam: arena size must be a multiple of 4");
  require(!x.ema || x.ema_rate, "adam: an average needs its rate word");
  if (skip_mask() & 32) return;
  if (hz::active())
    hz::op(s, "adam", {hz::rd(g, (int64_t)n * 4), hz::rd(scal, 8), hz::rd(gscale, 4), hz::rd(x.decay, 4),
                       hz::rd(x.ema ? x.ema_rate : nullptr, 4), hz::wr(x.ema, (int64_t)n * 4),
                       hz::wr(p, (int64_t)n * 4), hz::wr(m, (int64_t)n * 4),
                       hz::wr(v, (int64_t)n * 4), hz::wr(shadow, (int64_t)n_shadow * 2),
                       hz::wr(tiles.n > 0 ? tiles.dst[0] : nullptr, tiles.n > 0 ? tiles.len[0] * 2 : 0),
                       hz::wr(tiles.n > 1 ? tiles.dst[1] : nullptr, tiles.n > 1 ? tiles.len[1] * 2 : 0),
                       hz::wr(tiles.n > 2 ? tiles.dst[2] : nullptr, tiles.n > 2 ? tiles.len[2] * 2 : 0),
                       hz::wr(tiles.n > 3 ? tiles.dst[3] : nullptr, tiles.n > 3 ? tiles.len[3] * 2 : 0)});
  size_t n4 = n / 4;
  // Adam workgroups (grid-stride): one per CU leaves the other wave slots to the critical stream
  // (A/B over 4 runs each: 3.046 vs 3.070 ms/step with 8 per CU)
  constexpr int cap = 256;
  // grid_cap > 0: the caller's cap (an update on the step's critical path takes the whole chip)
  int grid = (int)std::min<size_t>((n4 + 256 * ADAM_U - 1) / (256 * ADAM_U), (size_t)(grid_cap > 0 ? grid_cap : cap));
  // the variant: one instantiation per set of options, the options in the pack's fixed order
  auto launch = [&](auto... opt) {
    adam_kernel<decltype(opt)...><<<grid, 256, 0, s>>>((adam_f4*)p, (const adam_f4*)g, (adam_f4*)m, (adam_f4*)v, n4, b1,
                                                       b2, eps, scal, shadow, n_shadow, tiles, opt...);
  };
  auto with_ema = [&](auto... opt) {
    if (x.ema) launch(opt..., AdamEmaArg{(adam_f4*)x.ema, x.ema_rate});
    else launch(opt...);
  };
  auto with_decay = [&](auto... opt) {
    if (x.decay) with_ema(opt..., AdamDecayArg{x.decay});
    else with_ema(opt...);
  };
  if (gscale) with_decay(gscale);
  else with_decay();
  CAPGEN_HIP(hipGetLastError());
}

// ---- arena exchange (the averaged weights in and out of the parameter arena) ---------------------
// a[i] <-> b[i] over n f32 (n % 4 == 0, 16-byte aligned): 16-B non-temporal accesses, grid-stride
__global__ void __launch_bounds__(256) arena_swap_kernel(adam_f4* __restrict__ a, adam_f4* __restrict__ b, size_t n4) {
  const size_t stride = (size_t)gridDim.x * 256;
  for (size_t i = blockIdx.x * (size_t)256 + threadIdx.x; i < n4; i += stride) {
    const adam_f4 x = __builtin_nontemporal_load(a + i), y = __builtin_nontemporal_load(b + i);
    __builtin_nontemporal_store(y, a + i);
    __builtin_nontemporal_store(x, b + i);
  }
}
void arena_swap(float* a, float* b, size_t n, hipStream_t s, int grid_cap) {
  require(a != nullptr && b != nullptr, "arena_swap: null array");
  require(n % 4 == 0, "arena_swap: the size must be a multiple of 4");
  require(a + n <= b || b + n <= a, "arena_swap: the arrays overlap");
  if (n == 0) return;
  if (hz::active()) hz::op(s, "arena_swap", {hz::wr(a, (int64_t)n * 4), hz::wr(b, (int64_t)n * 4)});
  const size_t n4 = n / 4;
  const int grid = (int)std::min<size_t>((n4 + 255) / 256, (size_t)(grid_cap > 0 ? grid_cap : 2048));
  arena_swap_kernel<<<grid, 256, 0, s>>>((adam_f4*)a, (adam_f4*)b, n4);
  CAPGEN_HIP(hipGetLastError());
}

// ---- gradient norm (global-norm clipping) ------------------------------------------------
// Sum of squares of a flat f32 range, accumulated in double: the square of an f32 is exact in
// double and the kernel is memory-bound (one f64 FMA per 4 bytes loaded), so neither a 1e20 element
// nor a range of 1e-30s is lost.  Loads as in adam_kernel: 16 B, non-temporal, GNORM_U of them in
// flight per thread before the first use.  The sum is reduced per wave by shuffle and per workgroup
// through LDS, and every workgroup writes ONE double into its own slot with a plain store: no
// float / double atomics, so the value depends on (n, grid) only -- equal on every run and on every
// data-parallel rank that holds equal gradients (an arrival-ordered sum would let the clip
// coefficient, and then the parameters, differ in the last bit between ranks).
constexpr int GNORM_U = 4;
__global__ void __launch_bounds__(256) grad_sumsq_kernel(const adam_f4* __restrict__ g, size_t n4,
                                                         double* __restrict__ partials) {
  __shared__ double sh[4];
  double acc = 0.0;
  const size_t stride = (size_t)gridDim.x * 256 * GNORM_U;
  for (size_t base = blockIdx.x * (size_t)(256 * GNORM_U) + threadIdx.x; base < n4; base += stride) {
    adam_f4 gg[GNORM_U];
#pragma unroll
    for (int u = 0; u < GNORM_U; ++u) {
      // (a lane past the end re-reads element base: in range, its value is not added)
      const size_t i = base + (size_t)u * 256 < n4 ? base + (size_t)u * 256 : base;
      gg[u] = __builtin_nontemporal_load(g + i);
    }
#pragma unroll
    for (int u = 0; u < GNORM_U; ++u) asm volatile("" : "+v"(gg[u]));
#pragma unroll
    for (int u = 0; u < GNORM_U; ++u) {
      if (base + (size_t)u * 256 >= n4) break;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const double x = (double)gg[u][c];
        acc = fma(x, x, acc);
      }
    }
  }
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
int grad_sumsq_grid(size_t n, int grid_cap) {
  constexpr int cap = 256;  // one workgroup per CU: the kernel runs beside the critical chain (as adam_update)
  const size_t n4 = n / 4;
  return (int)std::min<size_t>((n4 + 256 * GNORM_U - 1) / (256 * GNORM_U), (size_t)(grid_cap > 0 ? grid_cap : cap));
}
int grad_sumsq(const float* g, size_t n, double* partials, int slots_cap, hipStream_t s, int grid_cap) {
  require(n % 4 == 0, "grad_sumsq: the range must be a multiple of 4 elements");
  require(g != nullptr && ((uintptr_t)g & 15) == 0, "grad_sumsq: the range must be 16-byte aligned");
  const int grid = grad_sumsq_grid(n, grid_cap);
  require(partials != nullptr && grid <= slots_cap, "grad_sumsq: the partials buffer is too small");
  if (grid == 0) return 0;
  if (hz::active()) hz::op(s, "grad_sumsq", {hz::rd(g, (int64_t)n * 4), hz::wr(partials, (int64_t)grid * 8)});
  grad_sumsq_kernel<<<grid, 256, 0, s>>>((const adam_f4*)g, n / 4, partials);
  CAPGEN_HIP(hipGetLastError());
  return grid;
}

// One wave: lane l sums the contiguous slots [l k, (l + 1) k), k = ceil(n_slots / 64), in slot order, and
// lane 0 adds the 64 lane sums in lane order -- the slots left to right, in double, in an association
// fixed by n_slots alone.  phase & 1: *sum = that total (sum == null: kept in a register); phase & 2:
// out2 = {norm = (float)sqrt(sum), coef = (float)min(1, max_norm / (norm + 1e-6))}, the coefficient of
// torch.nn.utils.clip_grad_norm_ (error_if_nonfinite=False; a non-finite norm is passed through as
// torch does).  Two launches (phase 1, then 2) leave room for an all-reduce of *sum in between.
__global__ void __launch_bounds__(64) grad_norm_finish_kernel(const double* __restrict__ partials, int n_slots,
                                                              double* sum, const float* max_norm_ptr,
                                                              float max_norm_val, float* out2, int phase) {
  __shared__ double sh[64];
  double total = 0.0;
  if (phase & 1) {
    const int k = (n_slots + 63) / 64;
    double acc = 0.0;
    for (int i = threadIdx.x * k; i < min(n_slots, (int)(threadIdx.x + 1) * k); ++i) acc += partials[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
      for (int l = 0; l < 64; ++l) total += sh[l];
      if (sum) *sum = total;
    }
  } else if (threadIdx.x == 0) {
    total = *sum;
  }
  if ((phase & 2) && threadIdx.x == 0) {
    const float max_norm = max_norm_ptr ? *max_norm_ptr : max_norm_val;
    const float norm = (float)sqrt(total);
    out2[0] = norm;
    // torch: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 (max_norm = +inf: exactly 1)
    const double coef = (double)max_norm / ((double)norm + 1e-6);
    out2[1] = (float)(coef > 1.0 ? 1.0 : coef);  // (a NaN coefficient stays NaN, as torch.clamp leaves it)
  }
}
void grad_norm_finish(const double* partials, int n_slots, double* sum, const float* max_norm_ptr,
                      float max_norm_val, float* out2, int phase, hipStream_t s) {
  require(phase >= 1 && phase <= 3, "grad_norm_finish: phase 1 (slot sum), 2 (norm + coefficient) or 3 (both)");
  require(n_slots >= 0 && (!(phase & 1) || n_slots == 0 || partials), "grad_norm_finish: null partials");
  require(phase == 3 || sum, "grad_norm_finish: a split finish needs the sum word");
  require(!(phase & 2) || out2, "grad_norm_finish: null output");
  if (hz::active())
    hz::op(s, "grad_norm_finish",
           {hz::rd(phase & 1 ? partials : nullptr, (int64_t)n_slots * 8), hz::rd(phase & 1 ? nullptr : sum, 8),
            hz::wr(phase & 1 ? sum : nullptr, 8), hz::rd(phase & 2 ? max_norm_ptr : nullptr, 4),
            hz::wr(phase & 2 ? out2 : nullptr, 8)});
  grad_norm_finish_kernel<<<1, 64, 0, s>>>(partials, n_slots, sum, max_norm_ptr, max_norm_val, out2, phase);
  CAPGEN_HIP(hipGetLastError());
}

// Position-weighted sum of the f32 bit patterns, sum_i bits(x_i) * (2 i + 1) mod 2^64: exact and
// independent of summation order, so equal arenas give equal values on every rank / run.
__global__ void checksum_kernel(const uint32_t* __restrict__ x, size_t n, unsigned long long* out) {
  unsigned long long acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    acc += (unsigned long long)x[i] * (2ull * i + 1ull);
  for (int o = 32; o >= 1; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((threadIdx.x & 63) == 0) atomicAdd(out, acc);
}
uint64_t arena_checksum(const float* p, size_t n, hipStream_t s) {
  unsigned long long* d = nullptr;
  CAPGEN_HIP(hipMalloc(&d, sizeof *d));
  CAPGEN_HIP(hipMemsetAsync(d, 0, sizeof *d, s));
  checksum_kernel<<<1024, 256, 0, s>>>(reinterpret_cast<const uint32_t*>(p), n, d);
  CAPGEN_HIP(hipGetLastError());
  unsigned long long v = 0;
  CAPGEN_HIP(hipMemcpyAsync(&v, d, sizeof v, hipMemcpyDeviceToHost, s));
  CAPGEN_HIP(hipStreamSynchronize(s));
  CAPGEN_HIP(hipFree(d));
  return v;
}

__global__ void to_bf16_kernel(const float* __restrict__ src, bf16* __restrict__ dst, size_t n) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = (bf16)src[i];
}
// 4 elements per lane: one dwordx4 load, one 8-byte store (the sharded update's shadow re-cast)
__global__ void to_bf16x4_kernel(const float4* __restrict__ src, bf16* __restrict__ dst, size_t n4) {
  typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const float4 x = src[i];
    bf16x4 o = {(bf16)x.x, (bf16)x.y, (bf16)x.z, (bf16)x.w};
    *reinterpret_cast<bf16x4*>(dst + 4 * i) = o;
  }
}
void to_bf16(const float* src, bf16* dst, size_t n, hipStream_t s) {
  if (!n) return;
  if (hz::active()) hz::op(s, "to_bf16", {hz::rd(src, (int64_t)n * 4), hz::wr(dst, (int64_t)n * 2)});
  if (n % 4 == 0 && ((uintptr_t)src & 15) == 0 && ((uintptr_t)dst & 7) == 0) {
    const size_t n4 = n / 4;
    int grid = (int)std::min<size_t>((n4 + 255) / 256, 2048);
    to_bf16x4_kernel<<<grid, 256, 0, s>>>((const float4*)src, dst, n4);
    CAPGEN_HIP(hipGetLastError());
    return;
  }
  int grid = (int)std::min<size_t>((n + 255) / 256, 4096);
  to_bf16_kernel<<<grid, 256, 0, s>>>(src, dst, n);
  CAPGEN_HIP(hipGetLastError());
}

__global__ void bump_seed_kernel(uint64_t* seed) { *seed += 0x9E3779B97F4A7C15ull; }
void bump_seed(uint64_t* seed, hipStream_t s) {
  bump_seed_kernel<<<1, 1, 0, s>>>(seed);
  CAPGEN_HIP(hipGetLastError());
}

}  // namespace capgen
