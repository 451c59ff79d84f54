// capgen — device pieces shared by the row kernels: block reductions (ops.hip's CE kernels, rl.hip,
// select.hip) and the building blocks of decode selection (select.hip, rl.hip's row argmax).
// Every selection orders candidates by (value descending, index ascending): first index on ties.
#pragma once
#include "capgen_common.h"

namespace capgen {

// ---- block reductions: 64 W threads, sh = W words of LDS, every thread gets the result ----------
__device__ __forceinline__ int wave_sum(int v) {
  v += lane_xchg<1>(v);
  v += lane_xchg<2>(v);
  v += lane_xchg<4>(v);
  v += lane_xchg<8>(v);
  v += lane_xchg<16>(v);
  v += lane_xchg<32>(v);
  return v;
}
template <int W = 4>
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int w = 1; w < W; ++w) r = fmaxf(r, sh[w]);
  __syncthreads();
  return r;
}
// Two orders of adding the waves' sums, because an f32 sum depends on it and each kernel's results are
// pinned bit for bit: pairwise (CE, greedy, sampling, SCST rows; 4 waves) and in wave order (the beam
// row softmax, 4 or 8 waves).
template <typename T>
__device__ __forceinline__ T block_sum_pairwise(T v, T* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = (sh[0] + sh[1]) + (sh[2] + sh[3]);
  __syncthreads();
  return r;
}
template <int W>
__device__ __forceinline__ float block_sum_inorder(float v, float* sh) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int w = 0; w < W; ++w) r += sh[w];
  __syncthreads();
  return r;
}

// ---- one row of V f32 seen by a workgroup of NT threads ------------------------------------------
// NV > 0: the row (V <= NT * NV) is read once into registers, every load up front (one memory round
// trip instead of one per pass), -inf past V; NV = 0: every pass re-reads it from memory.  each(f) calls
// f(value, c, u) for the thread's columns c = tid + NT * u < V in ascending order -- the same order in
// both forms; value is a reference a pass may overwrite for the next one (it lasts only where NV > 0).
// each_slot(f) also visits the register slots past V (c >= V, value -inf; none where NV = 0), for a pass
// that keeps per-slot state and would rather neutralise those slots once than test c < V every time.
template <int NV, int NT>
struct RowRegs {
  const float* x;
  int V, tid;
  float xr[NV > 0 ? NV : 1];
  __device__ __forceinline__ RowRegs(const float* x_, int V_, int tid_) : x(x_), V(V_), tid(tid_) {
    if constexpr (NV > 0) {
#pragma unroll
      for (int u = 0; u < NV; ++u) {
        const int c = tid + NT * u;
        xr[u] = c < V ? x[c] : -INFINITY;
      }
    }
  }
  template <bool PAST_V, class F>
  __device__ __forceinline__ void visit(F&& f) {
    if constexpr (NV > 0) {
#pragma unroll
      for (int u = 0; u < NV; ++u)  // unrolled: no dynamic register indexing
        if (PAST_V || tid + NT * u < V) f(xr[u], tid + NT * u, u);
    } else {
      for (int c = tid; c < V; c += NT) {
        float xv = x[c];
        f(xv, c, 0);
      }
    }
  }
  template <class F>
  __device__ __forceinline__ void each(F&& f) {
    visit<false>(f);
  }
  template <class F>
  __device__ __forceinline__ void each_slot(F&& f) {
    visit<true>(f);
  }
};

// ---- sorted per-thread candidate lists and the wave rounds over them -----------------------------
template <int KM>
__device__ __forceinline__ void topk_clear(float (&tv)[KM], int (&ti)[KM]) {
#pragma unroll
  for (int u = 0; u < KM; ++u) tv[u] = -INFINITY, ti[u] = 0x7fffffff;
}
// sorted (desc) register top-KM insert of candidate (x, c)
template <int KM>
__device__ __forceinline__ void topk_insert(float (&tv)[KM], int (&ti)[KM], float x, int c) {
  if (!(x > tv[KM - 1] || (x == tv[KM - 1] && c < ti[KM - 1]))) return;
  float cv = x;
  int ci = c;
#pragma unroll
  for (int u = 0; u < KM; ++u) {  // unrolled: no dynamic register indexing
    const bool better = cv > tv[u] || (cv == tv[u] && ci < ti[u]);
    const float ov = tv[u];
    const int oi = ti[u];
    tv[u] = better ? cv : ov;
    ti[u] = better ? ci : oi;
    cv = better ? ov : cv;
    ci = better ? oi : ci;
  }
}
template <int KM>
__device__ __forceinline__ void pop_head(float (&tv)[KM], int (&ti)[KM]) {
#pragma unroll
  for (int u = 0; u + 1 < KM; ++u) tv[u] = tv[u + 1], ti[u] = ti[u + 1];
  tv[KM - 1] = -INFINITY, ti[KM - 1] = 0x7fffffff;
}

// (value, index) winner of a wave: value desc, index asc; pos rides along
template <int O>
__device__ __forceinline__ void best_step(float& best, int& bidx, int& bpos) {
  const float ov = lane_xchg<O>(best);
  const int oi = lane_xchg<O>(bidx);
  const int op = lane_xchg<O>(bpos);
  if (ov > best || (ov == best && oi < bidx)) best = ov, bidx = oi, bpos = op;
}
__device__ __forceinline__ void wave_best(float& best, int& bidx, int& bpos) {
  best_step<32>(best, bidx, bpos);
  best_step<16>(best, bidx, bpos);
  best_step<8>(best, bidx, bpos);
  best_step<4>(best, bidx, bpos);
  best_step<2>(best, bidx, bpos);
  best_step<1>(best, bidx, bpos);
}

// The k best of a wave's sorted lists, in order: k rounds of a wave argmax over the lanes' list heads,
// the winner pops its head.  emit(sel, value, index) runs in every lane with round sel's winner.
template <int KM, class Emit>
__device__ __forceinline__ void wave_topk_rounds(float (&tv)[KM], int (&ti)[KM], int k, int lane, Emit&& emit) {
  for (int sel = 0; sel < k; ++sel) {
    float best = tv[0];
    int bidx = ti[0], bpos = lane;
    wave_best(best, bidx, bpos);
    emit(sel, best, bidx);
    if (lane == bpos) pop_head<KM>(tv, ti);
  }
}
// One wave picks a row's k best of its W waves' k finalists each (wv / wi[wave][rank], W k <= 64): one
// finalist per lane, the same rounds over one-entry lists.
template <int W, class Emit>
__device__ __forceinline__ void wave_merge_finalists(const float (*wv)[16], const int (*wi)[16], int k, int lane,
                                                     Emit&& emit) {
  const bool on = lane < W * k;
  float v[1] = {on ? wv[lane / k][lane % k] : -INFINITY};
  int c[1] = {on ? wi[lane / k][lane % k] : 0x7fffffff};
  wave_topk_rounds<1>(v, c, k, lane, emit);
}

// The winner of a 256-thread workgroup's per-thread (value, index[, payload]) candidates.  sv: 4 floats
// and si: 4 (PAY: 8) ints of LDS.  Thread 0 ends with the winner in its arguments; true in that thread.
template <bool PAY>
__device__ __forceinline__ bool block_best_impl(float& best, int& bidx, int& pay, float* sv, int* si) {
  const int wave = threadIdx.x >> 6;
  wave_best(best, bidx, pay);
  if ((threadIdx.x & 63) == 0) {
    sv[wave] = best, si[wave] = bidx;
    if constexpr (PAY) si[4 + wave] = pay;
  }
  __syncthreads();
  if (threadIdx.x != 0) return false;
  for (int w = 1; w < 4; ++w)
    if (sv[w] > best || (sv[w] == best && si[w] < bidx)) {
      best = sv[w], bidx = si[w];
      if constexpr (PAY) pay = si[4 + w];
    }
  return true;
}
__device__ __forceinline__ bool block_best(float& best, int& bidx, int& pay, float* sv, int* si) {
  return block_best_impl<true>(best, bidx, pay, sv, si);
}
__device__ __forceinline__ bool block_best(float& best, int& bidx, float* sv, int* si) {
  int none = 0;
  return block_best_impl<false>(best, bidx, none, sv, si);
}

}  // namespace capgen
