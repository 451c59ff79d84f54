// capgen — decode selection kernels for gfx950: what turns a decode step's logits into tokens.
//
// Greedy argmax, the beam step's per-row top-k and per-image merge, temperature / top-k / nucleus
// sampling by Gumbel-max, the bf16 path's selection from the classifier's slab stats, the decode constraints
// that edit a step's logits in front of a selection, the kernel that fuses an ensemble's logits into one row distribution, and the beam bookkeeping of the generation loops.  Every selection orders candidates by (value descending, index
// ascending).  The pieces the kernels are built from -- the row in registers, the sorted per-thread
// lists and the wave rounds over them, the block winner and the block reductions -- are in select_dev.h.
#include <algorithm>
#include <type_traits>

#include "select.h"
#include "select_dev.h"
#include "hazard.h"

namespace capgen {

// k -> the per-thread list length KM in {4, 5, 8, 16} the selection kernels are built for (k <= 16):
// calls f(std::integral_constant<int, KM>)
template <class F>
static void with_km(int k, F&& f) {
  if (k <= 4) f(std::integral_constant<int, 4>{});
  else if (k == 5) f(std::integral_constant<int, 5>{});
  else if (k <= 8) f(std::integral_constant<int, 8>{});
  else f(std::integral_constant<int, 16>{});
}

// ---- greedy / beam helpers ---------------------------------------------------------
// logsm = 0: argmax of Softmax (Transformer, model.py:124-128); 1: of LogSoftmax
// (PolicyNetwork, model_RL.py:72,126-127) -- the same token except where the rounding of the
// two scores makes different near-ties
// NV > 0: the row (V <= 256 NV) is held in registers (RowRegs); the same per-thread order as NV = 0
template <int NV>
__global__ void __launch_bounds__(256) argmax_softmax_kernel(const float* __restrict__ logits, int V,
                                                             int64_t* ids_out, int64_t ids_ld, int col,
                                                             int32_t* next_ids, int64_t next_ld, int logsm) {
  __shared__ float sh[4];
  __shared__ float bv[4];
  __shared__ int bi[4];
  const int b = blockIdx.x;
  RowRegs<NV, 256> row(logits + (int64_t)b * V, V, threadIdx.x);
  float mx = -INFINITY;
  row.each([&](float xv, int, int) { mx = fmaxf(mx, xv); });
  mx = block_max(mx, sh);
  float se = 0.f;
  row.each([&](float xv, int, int) { se += expf(xv - mx); });
  se = block_sum_pairwise(se, sh);
  // argmax over the softmax probabilities, first index on ties (torch.argmax)
  float best = -INFINITY;
  int bidx = 0x7fffffff;
  const float lse = logf(se);
  row.each([&](float xv, int c, int) {
    const float p = logsm ? (xv - mx) - lse : expf(xv - mx) / se;
    if (p > best) {
      best = p;
      bidx = c;
    }
  });
  if (block_best(best, bidx, bv, bi)) {
    ids_out[(int64_t)b * ids_ld + col] = bidx;
    if (next_ids) next_ids[(int64_t)b * next_ld] = bidx;
  }
}
void argmax_softmax(const float* logits, int B, int V, int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids,
                    int64_t next_ld, hipStream_t s, int logsm) {
  if (V <= 256 * 40) argmax_softmax_kernel<40><<<B, 256, 0, s>>>(logits, V, ids_out, ids_ld, col, next_ids, next_ld, logsm);
  else argmax_softmax_kernel<0><<<B, 256, 0, s>>>(logits, V, ids_out, ids_ld, col, next_ids, next_ld, logsm);
  CAPGEN_HIP(hipGetLastError());
}

// ---- beam search step (model.py:183-190; PolicyNetwork model_RL.py:182-190 with logsm) ----
// Candidate (j, v) of image i scores prev[j][i] + p[j*B+i][v] (p: Softmax, or LogSoftmax with
// logsm); the k best under (score desc, flat index j*V + v asc) -- a strict total order, so the
// selection equals a full sort's first k.  Part 1, one workgroup per decoder row r = j*B + i:
// the row's softmax exactly as a separate softmax pass would compute it (same strided
// per-thread order and block reductions: the scores are bit-identical), the row held in
// registers (NV values per thread; NV = 0 re-reads it from memory), each thread's sorted
// top-KM, and the row's top k.  Part 2, one wave per image: top k of its k_in rows' k
// finalists each -- every image-level winner is in its row's top k.  Neither the [R, V]
// probabilities nor a [B, k*V] scan exist: one read of the logits per step.
//
// ---- the END-aware beam step (beam_nbest; the ENDED = true forms of the kernels below) and its finish ----
// T = max_length, V = num_vocab, k = beam_size; rows are j * B + i, beam j of image i.  A hypothesis is
// its tokens, logp (the f32 running sum of its token log-probabilities), len (int32: the tokens emitted
// while live, <END> included) and the flag fin.  It starts as <START> with logp = 0, len = 0, fin = 0;
// at step 0 only beam 0 is a source.
// - Candidates of image i at a step.  A live source row j offers (logp_j + logsoftmax(logits[j*B+i])[v],
//   flat index j * V + v) for every v: always the log-softmax, scored by the logsm = 1 arithmetic of the
//   reference step in the same order, so with nothing finished the results are bit-identical to it.  A
//   finished source row j offers exactly one candidate, (logp_j, j * V + 0); its logits and slab stats are
//   never read (they may be NaN).  The k best are taken under (score descending, flat index ascending) --
//   two finished rows with bit-equal logp keep their beam order.  Pruning uses the raw logp.
// - Update for the selected (j, v).  From a finished source: token 0 is appended and logp, len, fin are
//   copied.  From a live source: token v is appended, len + 1, fin = (v == end_id); end_id = -1: nothing
//   ever finishes.
// - Fewer than k candidates (only where a caller hands in fewer than k live sources' worth: the engine
//   never does): the slots left over get score -inf, source 0, token 0 and source 0's state copied.
// - Finish (beam_finish_kernel).  Final score s = logp when alpha == 0 (by definition: the launcher picks
//   the form that does not divide), else s = logp / powf((float)max(len, 1), alpha).  Per image the
//   hypotheses are ordered by (s descending, beam index ascending; a NaN s ranks as -inf) and the first
//   n_best are written: tokens, s, logp and len.  A hypothesis that never finished has len = T - 1.
//
// ---- diverse beam search (beam_diverse; Vijayakumar et al. 2016: beam groups, Hamming diversity) ----
// k = beam_size, G = num_groups (G divides k), k' = k / G; group g is beams g k' .. (g + 1) k' - 1; lambda =
// diversity_penalty, finite and >= 0.  A hypothesis is exactly beam_nbest's, and logp stays the f32 running sum
// of the model's token log-probabilities: the penalty orders candidates and is never added into logp.
// At a position, for image i, the groups are served in order g = 0 .. G - 1:
// - Count.  c_g(v) = the number of hypotheses selected at this position for groups h < g of image i that came
//   from a live source and appended token v.  <END> counts like any word; the token 0 appended to a finished
//   source does not count.
// - Candidates of group g: those of beam_nbest's step, restricted to the group's own k' source rows (at step 0
//   the only source is beam 0, for every group).  A live source j offers (logp_j + logsoftmax(row)[v] -
//   lambda * c_g(v), flat index j * V + v); a finished one exactly (logp_j, j * V + 0), unpenalised, its logits
//   never read.  The penalised score is the f32 candidate score minus the f32 product lambda * c (c = 0: the
//   score itself).
// - Selection.  The k' best under (penalised score descending, flat index ascending) become beams g k' + rank.
// - Update: beam_nbest's, src being the absolute source beam.  The new logp is the unpenalised
//   logp_j + logsoftmax[v] -- the very f32 the row kernel wrote as that finalist, not "penalised + lambda * c".
// - Finish: beam_finish per group, the n_best <= k' best of each by logp / max(len, 1)^alpha, output row
//   (g * n_best + rank) * B + i.  Decode constraints edit the logits before the selection and pruning uses
//   the raw logp, both as for beam_nbest.
// Consequences: G = 1 is beam_nbest bit for bit whatever lambda (it takes beam_nbest's launches); lambda = 0
// with G > 1 gives G groups that each run beam_nbest(k') on their own -- identical groups; a penalised token has
// c <= k - k'.
// The kernels.  Penalties lower at most |S| <= g k' distinct tokens (S: the tokens chosen so far), so a row's
// k' best penalised candidates lie among its k' + |S| <= k best unpenalised ones: a candidate outside them has
// k' + |S| candidates ordered before it, at most |S| of which a penalty can move behind it.  Hence
// beam_row_topk_kernel<ENDED> runs once over all k_in * B rows with k finalists per row, and
// beam_group_merge_kernel, one wave per image, walks the groups in order over the group's rows' finalists.
// The bound is tight: k = G = 16 with 16 equal rows takes each row's ranks 0 .. 15.
//
// ---- forced-word beam search (beam_forced; constrained beam search: Anderson et al. 2017, in the fixed-beam
// form of Post & Vilar 2018 / Hu et al. 2019: banks by the number of constraints met) ----
// Inputs.  Image i has W slots (word[i][s], group[i][s]), word = -1 for an empty slot.  A group is a set of
// alternatives ("dog", "dogs", "puppy") and is met by a hypothesis once it has appended any of the group's
// words.  bits_i(v) = the OR of 1 << group over the slots of image i that hold v, full_i = the OR over all of
// the image's slots; a word may sit in several groups.
// Hypothesis: beam_nbest's, plus met, a bitmask that starts at 0.  logp stays the f32 running sum of the model's
// token log-probabilities: nothing is renormalised or added to it.
// Candidates at a position, for image i:
// - a finished source j offers exactly (logp_j, j * V + 0), with met' = met_j;
// - a live source j offers (logp_j + logsoftmax(row_j)[v], j * V + v) with met' = met_j | bits_i(v) for every v,
//   except that v == end_id is no candidate while met_j != full_i: a hypothesis cannot end with a group unmet.
// The bank of a candidate is popcount(met'), its rank its position within its own bank under (score descending,
// flat index ascending).
// Selection.  The k first candidates under (rank ascending, bank descending) become beams 0 .. k - 1 in that
// order: the best of the highest non-empty bank, the best of the next non-empty bank and so on down, then the
// second-best of each, until k are taken.  Scores are never compared across banks.
// Update: beam_nbest's, plus met = met'.  Fewer than k candidates: the slots left over are beam_nbest's (score
// -inf, source 0's state copied, its met included).
// Finish: per image the n_best of the k hypotheses under (popcount(met) descending, logp / max(len, 1)^alpha
// descending, beam ascending), met returned with them.  There is no forcing near max_length: a hypothesis may
// run out of positions with a group unmet; it then ranks behind every hypothesis that met more groups, and met
// says so.
// Decode constraints edit the logits in front of the selection, as for beam_nbest; a forced word they block
// scores -inf like any blocked word.
// Consequences: with no word on any image the search is beam_nbest bit for bit (and takes its launches);
// score_captions of a returned caption gives its returned logp.
// Limits: W >= 1, k + W <= 15, k + W + 1 <= V, group in [0, 16), word in [0, V) or -1 and not end_id, 0 (<NULL>)
// or 1 (<START>); not combined with beam groups.  (The kernels take a slot whose word or group is out of range
// as empty; what word may not be is the callers' rule.)
// Why the limit makes the kernels exact.  Row j's candidates are of two classes: staying ones keep bank
// popcount(met_j), advancing ones are the words of its unmet groups -- at most W per row, enumerated explicitly.
// At most k staying candidates of a row are ever selected, and they lie among the row's k + W + 1 <= 16 best:
// the only candidates that can precede them in the row are its advancing words and a filtered <END>.  So
// beam_row_topk_kernel<ENDED, FORCED> runs with kf = min(16, k + W + 1) finalists per row and writes, behind
// them, the W scores prev + (x[w] - max) - lse of the image's slot words from the mx / lse it holds, in its own
// f32 arithmetic.  beam_forced_merge_kernel, one wave per image, drops from the finalists every entry that
// advances its row and a filtered <END>, and adds the row's advancing words from those W scores (a word held by
// several slots once, from its first slot): an advancing word's score always comes from this route, never from
// the finalist list, so there is nothing to de-duplicate.  That gives k_in (kf + W) <= 240 entries per image.

// lane 0 of a merge, slot sel of image i: the selected (score, flat index) -> outputs and the new state
__device__ __forceinline__ void beam_end_emit(const BeamEnd& e, int sel, int i, int B, int V, float best, int bidx,
                                              float* out_prob, int32_t* out_src, int32_t* out_tok, int& src,
                                              int& tok) {
  const bool none = bidx == 0x7fffffff;  // fewer than k candidates
  src = none ? 0 : bidx / V, tok = none ? 0 : bidx % V;
  const int srow = src * B + i, f = e.fin_src[srow], l = e.len_src[srow];
  out_prob[sel * B + i] = best;
  out_src[sel * B + i] = src;
  out_tok[sel * B + i] = tok;
  e.fin_dst[sel * B + i] = (f || none) ? f : (tok == e.end_id);
  e.len_dst[sel * B + i] = (f || none) ? l : l + 1;
}
// a finished source row's k finalists: (logp, j * V) and k - 1 empty slots; threads 0 .. k - 1 of its wave
__device__ __forceinline__ void beam_end_finalists(const float* prev, int r, int j, int V, int k, int lane,
                                                   float* out_v, int* out_i) {
  if (lane < k) {
    out_v[lane] = lane == 0 ? (prev ? prev[r] : 0.f) : -INFINITY;
    out_i[lane] = lane == 0 ? j * V : 0x7fffffff;
  }
}

// the last argument of a step kernel: the END-aware form's state, nothing in the reference form
struct NoBeamEnd {};
// the forced-word form's: the END-aware state plus the image's slots and the hypotheses' met masks
struct BeamEndForced : BeamEnd {
  BeamForced f;
};
template <bool ENDED, bool FORCED = false>
using BeamEndArg = std::conditional_t<FORCED, BeamEndForced, std::conditional_t<ENDED, BeamEnd, NoBeamEnd>>;

// NT threads per row (W = NT / 64 waves), NV values per thread in registers (V <= NT * NV)
// ENDED: e.fin_src [rows] marks the finished source rows (see above) and logsm is 1; false: the reference step
// FORCED (with ENDED; k is kf here): row r's scores take kf + W floats of cand_v -- behind its kf finalists the
// score of each of its image's W slot words (-inf for an empty slot or a finished row)
template <int KM, int NV, int NT = 256, bool ENDED = false, bool FORCED = false>
__global__ void __launch_bounds__(NT) beam_row_topk_kernel(const float* __restrict__ logits,
                                                            const float* __restrict__ prev, int B, int V, int k,
                                                            int logsm, float* __restrict__ cand_v,
                                                            int* __restrict__ cand_i, BeamEndArg<ENDED, FORCED> e) {
  constexpr int W = NT / 64;
  __shared__ float sh[W];
  __shared__ float wv[W][16];
  __shared__ int wi[W][16];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = r / B;
  int vs = k;  // row stride of cand_v
  if constexpr (FORCED) vs = k + e.f.W;
  if constexpr (ENDED) {
    if (e.fin_src[r]) {  // (the whole workgroup: no barrier is skipped by some threads only)
      if (wave == 0) beam_end_finalists(prev, r, j, V, k, lane, cand_v + (int64_t)r * vs, cand_i + (int64_t)r * k);
      if constexpr (FORCED)
        if (tid < e.f.W) cand_v[(int64_t)r * vs + k + tid] = -INFINITY;
      return;
    }
  }
  RowRegs<NV, NT> row(logits + (int64_t)r * V, V, tid);
  float mx = -INFINITY;
  row.each([&](float xv, int, int) { mx = fmaxf(mx, xv); });
  mx = block_max<W>(mx, sh);
  float se = 0.f;
  row.each([&](float& xv, int, int) {
    const float e = expf(xv - mx);
    se += e;
    if (NV > 0 && !logsm) xv = e;  // Softmax scores need only exp(x - max)
  });
  se = block_sum_inorder<W>(se, sh);
  const float lse = logf(se), add = prev ? prev[r] : 0.f;
  float tv[KM];
  int ti[KM];
  topk_clear<KM>(tv, ti);
  row.each([&](float xv, int c, int) {
    const float p = logsm ? (xv - mx) - lse : (NV > 0 ? xv : expf(xv - mx)) / se;
    topk_insert<KM>(tv, ti, p + add, j * V + c);
  });
  // the row's k best: each wave's k best, then wave 0 selects the row's k from the W k of them
  wave_topk_rounds<KM>(tv, ti, k, lane, [&](int sel, float v, int i) {
    if (lane == 0) wv[wave][sel] = v, wi[wave][sel] = i;
  });
  __syncthreads();
  if (wave == 0)
    wave_merge_finalists<W>(wv, wi, k, lane, [&](int sel, float v, int i) {
      if (lane == 0) cand_v[(int64_t)r * vs + sel] = v, cand_i[(int64_t)r * k + sel] = i;
    });
  if constexpr (FORCED) {  // the slot words' scores, as the pass above scores a column
    if (tid < e.f.W) {
      const int w = e.f.word[(int64_t)(r % B) * e.f.W + tid];
      float p = -INFINITY;
      if ((unsigned)w < (unsigned)V) p = ((logits[(int64_t)r * V + w] - mx) - lse) + add;
      cand_v[(int64_t)r * vs + k + tid] = p;
    }
  }
}

// One wave, one image: the k best of its n = k_in * k row finalists (n <= 256; entry e = (row j = e / k,
// rank e % k)).  load(e, v, c) reads entry e; emit(sel, score, flat index) runs in lane 0.
template <class Load, class Emit>
__device__ __forceinline__ void beam_merge_wave(int n, int k, int lane, Load&& load, Emit&& emit) {
  float v[4];
  int c[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    v[u] = -INFINITY, c[u] = 0x7fffffff;
    if (lane + 64 * u < n) load(lane + 64 * u, v[u], c[u]);
  }
  for (int sel = 0; sel < k; ++sel) {
    float best = -INFINITY;
    int bidx = 0x7fffffff, bpos = -1;
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (v[u] > best || (v[u] == best && c[u] < bidx)) best = v[u], bidx = c[u], bpos = lane + 64 * u;
    wave_best(best, bidx, bpos);
    if (lane == 0) emit(sel, best, bidx);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (bpos == lane + 64 * u) v[u] = -INFINITY, c[u] = 0x7fffffff;
  }
}

// one wave per image over the rows' finalists in cand_v / cand_i [k_in * B][k]; ENDED: the END-aware merge,
// the same selection, then the new rows' fin / len from their sources'
template <bool ENDED>
__global__ void __launch_bounds__(64) beam_merge_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                        int k_in, int B, int V, int k, float* __restrict__ out_prob,
                                                        int32_t* __restrict__ out_src, int32_t* __restrict__ out_tok,
                                                        BeamEndArg<ENDED> e) {
  const int i = blockIdx.x;
  beam_merge_wave(
      k_in * k, k, threadIdx.x,
      [&](int en, float& v, int& c) {
        const int64_t src = ((int64_t)(en / k) * B + i) * k + en % k;
        v = cand_v[src], c = cand_i[src];
      },
      [&](int sel, float best, int bidx) {
        if constexpr (ENDED) {
          int src, tok;
          beam_end_emit(e, sel, i, B, V, best, bidx, out_prob, out_src, out_tok, src, tok);
        } else {
          out_prob[sel * B + i] = best;
          out_src[sel * B + i] = bidx / V;
          out_tok[sel * B + i] = bidx % V;
        }
      });
}

// The group-sequential merge of diverse beam search (definition above): one wave per image over the rows'
// k finalists each in cand_v / cand_i [k_in * B][k], k_in = 1 (step 0: every group draws on beam 0) or k.
// Group g's n = k' k (step 0: k) <= 128 entries sit two per lane; the tokens chosen so far (<= k - k' <= 15)
// sit one per lane in `said`, lane q holding the q-th, and are read back by lane broadcasts -- no LDS, no
// atomics.  Each of the k' rounds is beam_merge_wave's round on the penalised scores, with the unpenalised
// score fetched from the winner's lane for out_prob.
__global__ void __launch_bounds__(64) beam_group_merge_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                              int k_in, int B, int V, int k, int G, float lambda,
                                                              float* __restrict__ out_prob, int32_t* __restrict__ out_src,
                                                              int32_t* __restrict__ out_tok, BeamEnd e) {
  const int i = blockIdx.x, lane = threadIdx.x, kg = k / G;
  const int n = (k_in == 1 ? 1 : kg) * k;
  int said = -1, n_said = 0;  // (n_said is the same in every lane)
  for (int g = 0; g < G; ++g) {
    const int j0 = k_in == 1 ? 0 : g * kg;
    float v[2], p[2];
    int c[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int en = lane + 64 * u;
      v[u] = -INFINITY, c[u] = 0x7fffffff;
      int tok = -1;  // the token a penalty looks at: none for an empty slot or a finished source
      if (en < n) {
        const int64_t r = (int64_t)(j0 + en / k) * B + i;
        v[u] = cand_v[r * k + en % k], c[u] = cand_i[r * k + en % k];
        if (c[u] != 0x7fffffff && !e.fin_src[r]) tok = c[u] % V;
      }
      int cnt = 0;  // (every lane runs the broadcasts)
      for (int q = 0; q < n_said; ++q) cnt += __shfl(said, q, 64) == tok ? 1 : 0;
      p[u] = __fsub_rn(v[u], __fmul_rn(lambda, (float)cnt));
    }
    for (int sel = 0; sel < kg; ++sel) {
      float best = -INFINITY;
      int bidx = 0x7fffffff, bpos = -1;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (p[u] > best || (p[u] == best && c[u] < bidx)) best = p[u], bidx = c[u], bpos = lane + 64 * u;
      wave_best(best, bidx, bpos);
      float mine = -INFINITY;
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (bpos == lane + 64 * u) mine = v[u], p[u] = -INFINITY, c[u] = 0x7fffffff;
      const bool none = bidx == 0x7fffffff;  // fewer than k' candidates
      const float score = __shfl(mine, none ? 0 : bpos & 63, 64);  // (-inf where none)
      if (!none && !e.fin_src[(bidx / V) * B + i]) {  // a live source's token counts against the later groups
        if (lane == n_said) said = bidx % V;
        ++n_said;
      }
      if (lane == 0) {
        int src, tok;
        beam_end_emit(e, g * kg + sel, i, B, V, score, bidx, out_prob, out_src, out_tok, src, tok);
      }
    }
  }
}

// The bank round-robin of forced-word beam search (definition above): one wave per image over its k_in <= k
// source rows' kf finalists (cand_v [k_in * B][kf + W], cand_i [k_in * B][kf]) and W slot-word scores each,
// n = k_in (kf + W) <= 240 entries, four per lane.  Lane s < W holds slot s of the image and every lane reads
// the slots back by lane broadcasts -- no LDS, no atomics.  An entry keeps its score, flat index, met' and bank,
// or is empty: a finalist that advances its row or is a filtered <END>, a slot word that does not advance the
// row, repeats an earlier slot's word or belongs to a finished row.  Then rounds over the non-empty banks from
// the highest down, each one beam_merge_wave's round restricted to a bank, until k are taken.
__global__ void __launch_bounds__(64) beam_forced_merge_kernel(const float* __restrict__ cand_v, const int* __restrict__ cand_i,
                                                               int k_in, int B, int V, int k, int kf,
                                                               float* __restrict__ out_prob, int32_t* __restrict__ out_src,
                                                               int32_t* __restrict__ out_tok, BeamEndForced e) {
  constexpr int kNone = 0x7fffffff;
  const int i = blockIdx.x, lane = threadIdx.x, W = e.f.W, S = kf + W, n = k_in * S;
  const int32_t* word = e.f.word + (int64_t)i * W;
  int sw = -1, sb = 0;  // lane s: slot s' word and group bit (an empty slot: -1, 0)
  if (lane < W) {
    const int w = word[lane], g = e.f.group[(int64_t)i * W + lane];
    if ((unsigned)w < (unsigned)V && (unsigned)g < 16u) sw = w, sb = 1 << g;
  }
  int full = sb;
  full |= lane_xchg<32>(full), full |= lane_xchg<16>(full), full |= lane_xchg<8>(full);
  full |= lane_xchg<4>(full), full |= lane_xchg<2>(full), full |= lane_xchg<1>(full);
  float v[4];
  int c[4], m[4], bank[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int en = lane + 64 * u, q = en % S;
    const bool tail = q >= kf;
    v[u] = -INFINITY, c[u] = kNone, m[u] = 0, bank[u] = -1;
    int tok = -2, fin = 1, mj = 0;  // tok: the word whose bits count (-2: none)
    if (en < n) {
      const int j = en / S;
      const int64_t r = (int64_t)j * B + i;
      fin = e.fin_src[r], mj = e.f.met_src[r];
      if (!tail) {
        v[u] = cand_v[r * S + q], c[u] = cand_i[r * kf + q];
        if (c[u] != kNone && !fin) tok = c[u] % V;
      } else if (!fin) {
        const int w = word[q - kf];
        bool first = (unsigned)w < (unsigned)V;
        for (int s = 0; s < q - kf; ++s) first = first && word[s] != w;
        if (first) v[u] = cand_v[r * S + q], c[u] = j * V + w, tok = w;
      }
    }
    int bits = 0;  // (every lane runs the broadcasts)
    for (int s = 0; s < W; ++s) {
      const int w = __shfl(sw, s, 64), b = __shfl(sb, s, 64);
      bits |= w == tok ? b : 0;
    }
    const bool advances = (bits & ~mj) != 0;
    bool keep = c[u] != kNone;
    if (tail) keep = keep && advances;
    else if (!fin) keep = keep && !advances && !(tok == e.end_id && mj != full);
    if (keep) {
      v[u] = v[u] == v[u] ? v[u] : -INFINITY;  // (a NaN score ranks last)
      m[u] = mj | bits, bank[u] = __popc((unsigned)m[u]);
    } else {
      v[u] = -INFINITY, c[u] = kNone;
    }
  }
  int taken = 0;
  for (int round = 0; round < k && taken < k; ++round) {  // (a round with a bank left takes at least one)
    int present = 0;
#pragma unroll
    for (int u = 0; u < 4; ++u) present |= bank[u] >= 0 ? 1 << bank[u] : 0;
    present |= lane_xchg<32>(present), present |= lane_xchg<16>(present), present |= lane_xchg<8>(present);
    present |= lane_xchg<4>(present), present |= lane_xchg<2>(present), present |= lane_xchg<1>(present);
    if (!present) break;  // (the same in every lane)
    while (present && taken < k) {
      const int b = 31 - __clz(present);
      present &= ~(1 << b);
      float best = -INFINITY;
      int bidx = kNone, bpos = -1;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (bank[u] == b && (v[u] > best || (v[u] == best && c[u] < bidx))) best = v[u], bidx = c[u], bpos = lane + 64 * u;
      wave_best(best, bidx, bpos);
      if (bidx == kNone) continue;
      int mine = 0;
#pragma unroll
      for (int u = 0; u < 4; ++u)
        if (bpos == lane + 64 * u) mine = m[u], bank[u] = -1;
      const int met = __shfl(mine, bpos & 63, 64);
      if (lane == 0) {
        int src, tok;
        beam_end_emit(e, taken, i, B, V, best, bidx, out_prob, out_src, out_tok, src, tok);
        e.f.met_dst[taken * B + i] = met;
      }
      ++taken;
    }
  }
  if (lane == 0)
    for (; taken < k; ++taken) {  // fewer than k candidates
      int src, tok;
      beam_end_emit(e, taken, i, B, V, -INFINITY, kNone, out_prob, out_src, out_tok, src, tok);
      e.f.met_dst[taken * B + i] = e.f.met_src[i];
    }
}

template <int KM, bool ENDED = false, bool FORCED = false>
static void beam_row_topk(const float* logits, const float* prev, int rows, int B, int V, int k, int logsm,
                          float* cand_v, int32_t* cand_i, hipStream_t s, BeamEndArg<ENDED, FORCED> e = {}) {
  // 512 threads per row where the row fits 20 values per thread (42 vs 50 us per token at B = 1280
  // with 256 threads, round 2)
  if (V <= 512 * 20 && KM * 8 <= 64)
    beam_row_topk_kernel<KM, 20, 512, ENDED, FORCED><<<rows, 512, 0, s>>>(logits, prev, B, V, k, logsm, cand_v, cand_i, e);
  else if (V <= 256 * 40)
    beam_row_topk_kernel<KM, 40, 256, ENDED, FORCED><<<rows, 256, 0, s>>>(logits, prev, B, V, k, logsm, cand_v, cand_i, e);
  else beam_row_topk_kernel<KM, 0, 256, ENDED, FORCED><<<rows, 256, 0, s>>>(logits, prev, B, V, k, logsm, cand_v, cand_i, e);
}

static void require_beam_end(const char* who, int V, const BeamEnd& e) {
  const std::string w(who);
  require(e.fin_src && e.len_src && e.fin_dst && e.len_dst, w + ": null fin / len");
  require(e.fin_src != e.fin_dst && e.len_src != e.len_dst, w + ": fin / len must be double-buffered");
  require(e.end_id >= -1 && e.end_id < V, w + ": end_id must be in [-1, num_vocab)");
}

// ---- sampled decoding: temperature / top-k / nucleus sampling by Gumbel-max, with the log-probability ----
// One launch per decode position, one 256-thread workgroup per row r of logits [R][V] (f32); one kernel
// template, the lines marked [nucleus] hold for NUCLEUS = true (sample_nucleus with top_p < 1) only:
// - Scaled logits.  z_v = logits[r][v] * inv_tau (one f32 product), with inv_tau = 1 / temperature.
// - Base set C0.  Every v < V when top_k == 0.  Otherwise the top_k columns of the row under
//   (logit descending, v ascending), with 1 <= top_k <= min(16, V).
// - Candidate set C.  C = C0, or
//   [nucleus] C = { v in C0 : above(v) < top_p * P }, with M = max over C0 of z_v, P = sum_{u in C0}
//   exp(z_u - M) and above(v) = sum_{u in C0, z_u > z_v} exp(z_u - M); the inequality is strict and top_p
//   lies in (0, 1).  A word is kept exactly when the words strictly more likely than it do not already
//   hold top_p of the mass.  C always holds the row's maximum and is nested in top_p.  Columns with
//   bit-equal z are in or out together, so the set does not depend on column order (top_k may still cut
//   a tie group by index).  With top_k > 0 the mass is the one renormalised over C0: top-k first, nucleus
//   within it.
//   [nucleus] top_p == 1 means C = C0 by definition, not by arithmetic: the launcher then launches the
//   NUCLEUS = false kernel itself, so tokens and log-probabilities are bit-identical to sample_softmax.
// - Noise.  h = mix32(seed, site, (uint32_t)(r * V + v)), then u = ((h >> 9) + 0.5f) * 2^-23, then
//   g = -logf(-logf(u)).  u is exact in f32 and lies strictly inside (0, 1).  logf, not the __logf
//   intrinsic: the winning column usually has u close to 1, where -log u is 1e-4 ... 6e-8, and the
//   intrinsic's absolute error is of that size.  r is the row index within the launch; the launcher
//   requires R * V < 2^32.
// - Token.  token = argmax over v in C of (z_v + g_v), first index on ties.  With top_k == 1 this is
//   the argmax of the logits, first index on ties.  A row of NaNs has no winner: token 0.
//   [nucleus] The noise does not depend on top_p, so the draw is coupled to the untruncated one:
//   whenever the top_p = 1 winner lies in C, it is also the nucleus winner.
// - Log-probability.  logp = z_token - M - log sum_{v in C} exp(z_v - M), with M = max over C of z_v
//   (= max over C0, since C holds the maximum): the log-probability under the distribution actually
//   sampled.  Exactly 0 when |C| = 1.
// - Stores.  ids_out[r * ids_ld + col] = token (int64); next_ids[r * next_ld] = token (int32,
//   optional); logp_out[r * logp_ld + logp_col] = logp (optional);
//   [nucleus] count_out[r] = |C| (int32, optional).  Nothing else is written.
// Gumbel-max rather than an inverse-CDF scan: one pass, a result that does not depend on the
// summation order, and an index a float64 restatement predicts exactly wherever the two best
// perturbed scores are not within rounding of each other.  The slab statistics of the bf16 greedy /
// beam selection are not used: their per-slab exp-sums hold at temperature 1 only.
// NV > 0: the row (V <= 256 NV) is held in registers (as argmax_softmax_kernel).
// KM > 0 (top_k <= KM): C0 is found as beam_row_topk_kernel finds a row's k best, wave 0 ending with one
// column of C0 per lane.  [nucleus] above(v) is then top_k lane broadcasts, summed in lane order.
// KM = 0 (top_k == 0): one pass for M and the Gumbel winner, a second for the exp-sum.
// [nucleus] KM = 0: C is { v : key(z_v) >= k* } for the order-preserving integer key of the f32 z
// (-0 counted as +0); k* is the smallest key with mass_above(k*) < top_p * P, found by bisection of the
// 32-bit key range in exactly 32 steps, each one fixed-order block sum (no atomics: one result per seed,
// bit for bit).  mass_above is a sum of non-negative terms in a fixed order with some of them zeroed, so
// it is monotone in the key, and mass_above(key(-inf)) is P bit for bit: a column whose exp underflows is
// never in C.  The register form (NV = 40) keeps the row's keys and exponentials (80 VGPRs); the generic
// form recomputes them from memory in every step.  Every trip count is a constant or V / 256.  A row of
// NaNs or infinities leaves a NaN mass, every comparison false, and no winner: token 0.
__device__ __forceinline__ float gumbel_noise(uint32_t key, uint32_t idx) {
  const uint32_t h = lowbias32(idx ^ key);  // mix32(seed, site, idx), the key hoisted
  const float u = ((float)(h >> 9) + 0.5f) * 0x1p-23f;
  return -logf(-logf(u));
}
__device__ __forceinline__ uint32_t z_key(float z) {
  const uint32_t b = (uint32_t)__float_as_int(z + 0.f);  // -0 -> +0
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float key_z(uint32_t k) {
  return __int_as_float((int)(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)));
}

// where a row's token, next decoder input and log-probability go
struct SampleOut {
  int64_t* ids;
  int64_t ids_ld;
  int col;
  int32_t* next_ids;
  int64_t next_ld;
  float* logp;
  int64_t logp_ld;
  int logp_col;
};
// the winner (column bidx, scaled logit z) of row r under the candidates' max mx and exp-sum se
__device__ __forceinline__ void write_sample(const SampleOut& o, int r, int V, int bidx, float z, float mx, float se) {
  const int token = (unsigned)bidx < (unsigned)V ? bidx : 0;  // (a row of NaNs has no winner)
  o.ids[(int64_t)r * o.ids_ld + o.col] = token;
  if (o.next_ids) o.next_ids[(int64_t)r * o.next_ld] = token;
  if (o.logp) o.logp[(int64_t)r * o.logp_ld + o.logp_col] = (z - mx) - logf(se);
}

// (top_p and count_out are read by the NUCLEUS form only)
template <int NV, int KM, bool NUCLEUS>
__global__ void __launch_bounds__(256) sample_kernel(const float* __restrict__ logits, int V, float inv_tau, int top_k,
                                                     float top_p, uint64_t seed, uint32_t site, SampleOut out,
                                                     int32_t* count_out) {
  __shared__ float sh[4];
  __shared__ float wv[4][16];
  __shared__ int wi[4][16];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t key = drop_key(seed, site), base = (uint32_t)r * (uint32_t)V;
  RowRegs<NV, 256> row(logits + (int64_t)r * V, V, tid);
  // the winner's (perturbed score, column, bits of its z); M, the exp-sum over C and |C|
  float best = -INFINITY, mx = -INFINITY, se = 0.f;
  int bidx = 0x7fffffff, bz = 0, cnt = 0;
  bool writer = false;
  auto offer = [&](float z, int c) {
    const float sc = z + gumbel_noise(key, base + (uint32_t)c);
    if (sc > best) best = sc, bidx = c, bz = __float_as_int(z);
  };
  if constexpr (KM == 0 && !NUCLEUS) {
    row.each([&](float xv, int c, int) {
      const float z = __fmul_rn(xv, inv_tau);  // (not contracted into the add: z is an f32)
      mx = fmaxf(mx, z);
      offer(z, c);
    });
    mx = block_max(mx, sh);
    row.each([&](float xv, int, int) { se += expf(__fmul_rn(xv, inv_tau) - mx); });
    se = block_sum_pairwise(se, sh);
    writer = block_best(best, bidx, bz, wv[0], wi[0]);
  } else if constexpr (KM == 0) {
    uint32_t kr[NV > 0 ? NV : 1];  // NV > 0: key(z) of the thread's columns; 0 past the row's end
    float er[NV > 0 ? NV : 1];     // NV > 0: exp(z - M) of the thread's columns; 0 past the row's end
    row.each_slot([&](float xv, int c, int u) {
      const float z = __fmul_rn(xv, inv_tau);
      mx = fmaxf(mx, z);  // (-inf past the row's end)
      if constexpr (NV > 0) kr[u] = c < V ? z_key(z) : 0u, er[u] = 0.f;
    });
    mx = block_max(mx, sh);
    float pe = 0.f;
    row.each([&](float xv, int, int u) {
      float z;
      if constexpr (NV > 0) z = key_z(kr[u]);
      else z = __fmul_rn(xv, inv_tau);
      const float e = expf(z - mx);
      if constexpr (NV > 0) er[u] = e;
      pe += e;
    });
    const float thr = __fmul_rn(top_p, block_sum_pairwise(pe, sh));  // top_p * P
    // a column's (key(z), exp(z - M)): kept in registers, or recomputed from the logit
    auto key_exp = [&](float xv, int u, uint32_t& kz, float& e) {
      if constexpr (NV > 0) {
        kz = kr[u], e = er[u];
      } else {
        const float z = __fmul_rn(xv, inv_tau);
        kz = z_key(z), e = expf(z - mx);
      }
    };
    // the mass of the columns whose key is above k: the same per-thread order and block sum as P
    auto mass_above = [&](uint32_t k) {
      float a = 0.f;
      row.each_slot([&](float xv, int, int u) {
        uint32_t kz;
        float e;
        key_exp(xv, u, kz, e);
        a += kz > k ? e : 0.f;
      });
      return block_sum_pairwise(a, sh);
    };
    // k* = the smallest key k with mass_above(k) < top_p * P: [lo, hi] halves exactly 32 times
    uint32_t lo = 0u, hi = 0xFFFFFFFFu;
    for (int it = 0; it < 32; ++it) {
      const uint32_t mid = lo + ((hi - lo) >> 1);
      if (mass_above(mid) < thr) hi = mid;
      else lo = mid + 1u;
    }
    row.each([&](float xv, int c, int u) {
      uint32_t kz;
      float e;
      key_exp(xv, u, kz, e);
      if (kz < lo) return;
      se += e;
      ++cnt;
      offer(key_z(kz), c);
    });
    se = block_sum_pairwise(se, sh);
    cnt = block_sum_pairwise(cnt, wi[0]);
    writer = block_best(best, bidx, bz, wv[0], wi[0]);
  } else {
    float tv[KM];
    int ti[KM];
    topk_clear<KM>(tv, ti);
    row.each([&](float xv, int c, int) { topk_insert<KM>(tv, ti, xv, c); });
    wave_topk_rounds<KM>(tv, ti, top_k, lane, [&](int sel, float v, int i) {
      if (lane == 0) wv[wave][sel] = v, wi[wave][sel] = i;
    });
    __syncthreads();
    if (wave == 0) {  // the row's top_k of the waves' 4 top_k: lane sel keeps candidate sel
      float cx = -INFINITY;
      int cc = 0x7fffffff;
      wave_merge_finalists<4>(wv, wi, top_k, lane, [&](int sel, float v, int i) {
        if (lane == sel) cx = v, cc = i;
      });
      const bool in_c0 = lane < top_k;
      const float z = in_c0 ? __fmul_rn(cx, inv_tau) : -INFINITY;
      mx = wave_max(z);
      const float e = in_c0 ? expf(z - mx) : 0.f;
      bool in_c = in_c0;
      if constexpr (NUCLEUS) {
        // P and above(v) in one lane order, so that above(v) is P bit for bit under a column of no mass
        float pe = 0.f, above = 0.f;
#pragma unroll
        for (int j = 0; j < KM; ++j) {  // lanes >= top_k hold z = -inf, e = 0
          const float zj = __shfl(z, j, 64), ej = __shfl(e, j, 64);
          pe += ej;
          above += zj > z ? ej : 0.f;
        }
        in_c = in_c0 && above < __fmul_rn(top_p, pe);
        cnt = __popcll(__ballot(in_c));
      }
      se = wave_sum(in_c ? e : 0.f);
      best = in_c ? z + gumbel_noise(key, base + (uint32_t)cc) : -INFINITY;
      bidx = in_c ? cc : 0x7fffffff, bz = __float_as_int(z);
      wave_best(best, bidx, bz);
      writer = lane == 0;
    }
  }
  if (writer) {
    write_sample(out, r, V, bidx, __int_as_float(bz), mx, se);
    if constexpr (NUCLEUS)
      if (count_out) count_out[r] = cnt;
  }
}

template <bool NUCLEUS>
static void launch_sample(const char* who, const float* logits, int R, int V, float inv_tau, int top_k, float top_p,
                          uint64_t seed, uint32_t site, const SampleOut& out, int32_t* count_out, hipStream_t s) {
  const std::string w(who);
  require(R >= 1 && V >= 1 && (int64_t)R * V < ((int64_t)1 << 32), w + ": need R, V >= 1 and R * V < 2^32");
  require(inv_tau > 0.f && inv_tau < INFINITY, w + ": temperature must be > 0 and finite");
  require(top_k >= 0 && top_k <= 16 && top_k <= V, w + ": top_k must be in [0, min(16, num_vocab)]");
  require(logits && out.ids && out.col >= 0 && out.logp_col >= 0, w + ": null logits / ids_out or a negative column");
  auto go = [&](auto km) {
    constexpr int KM = decltype(km)::value;
    if (V <= 256 * 40) sample_kernel<40, KM, NUCLEUS><<<R, 256, 0, s>>>(logits, V, inv_tau, top_k, top_p, seed, site, out, count_out);
    else sample_kernel<0, KM, NUCLEUS><<<R, 256, 0, s>>>(logits, V, inv_tau, top_k, top_p, seed, site, out, count_out);
  };
  if (top_k == 0) go(std::integral_constant<int, 0>{});
  else with_km(top_k, go);
  CAPGEN_HIP(hipGetLastError());
}

void sample_softmax(const float* logits, int R, int V, float inv_tau, int top_k, uint64_t seed, uint32_t site,
                    int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids, int64_t next_ld, float* logp_out,
                    int64_t logp_ld, int logp_col, hipStream_t s) {
  launch_sample<false>("sample_softmax", logits, R, V, inv_tau, top_k, 1.f, seed, site,
                       SampleOut{ids_out, ids_ld, col, next_ids, next_ld, logp_out, logp_ld, logp_col}, nullptr, s);
}

__global__ void fill_i32_kernel(int32_t* p, int n, int32_t v) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) p[i] = v;
}

void sample_nucleus(const float* logits, int R, int V, float inv_tau, int top_k, float top_p, uint64_t seed,
                    uint32_t site, int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids, int64_t next_ld,
                    float* logp_out, int64_t logp_ld, int logp_col, int32_t* count_out, hipStream_t s) {
  require(top_p > 0.f && top_p <= 1.f, "sample_nucleus: top_p must be in (0, 1]");  // (false for a NaN)
  if (top_p == 1.f) {  // C = C0 by definition: sample_softmax's own kernels
    sample_softmax(logits, R, V, inv_tau, top_k, seed, site, ids_out, ids_ld, col, next_ids, next_ld, logp_out, logp_ld,
                   logp_col, s);
    if (count_out) {
      fill_i32_kernel<<<(R + 255) / 256, 256, 0, s>>>(count_out, R, top_k == 0 ? V : top_k);
      CAPGEN_HIP(hipGetLastError());
    }
    return;
  }
  launch_sample<true>("sample_nucleus", logits, R, V, inv_tau, top_k, top_p, seed, site,
                      SampleOut{ids_out, ids_ld, col, next_ids, next_ld, logp_out, logp_ld, logp_col}, count_out, s);
}

// ---- bf16 decode selection from slab stats (GemmArgs::dec_stats) ----------------------------
// One wave per row, 4 rows per workgroup.  The row's ceil(V/16) slab stats (8 B each, 1/8 of the
// f32 logits) sit NS per lane in registers: one pass gives the row max M and the exp-sum
// se = sum_c s_c exp(m_c - M) (the softmax of the selected elements is exp(x - M) / se), and each
// lane's sorted best slabs.  Any element of the row's top k (value desc, index asc) lies in one of
// the k best slabs under (max desc, slab asc): every slab ranked before the slab of the k-th best
// element holds, as its maximum, a distinct element ranked before it.  So only k * 16 logits are
// read back.  (The softmax is monotone in the logit; two logits rounding to one probability could
// order by index differently than a full scan would -- the bf16 path is held to the fp32 engine by
// the top-2-margin tests, the fp32 parity path keeps the exact full-row kernels above.)
constexpr int kSlabNS = 16;  // slabs per lane: V <= 64 * 16 * 16 = 16384
bool slab_select_ok(int V) { return V >= 1 && (V + 15) / 16 <= 64 * kSlabNS; }

struct SlabRow {
  float M, se;
};
// the row max and exp-sum from the stats; every lane ends with both
__device__ __forceinline__ SlabRow slab_row_stats(const float2* __restrict__ st, int S, int lane, float (&mx)[kSlabNS]) {
  float2 x[kSlabNS];
  float M = -INFINITY;
#pragma unroll
  for (int u = 0; u < kSlabNS; ++u) {
    const int c = lane + 64 * u;
    x[u] = c < S ? st[c] : float2{-INFINITY, 0.f};
    mx[u] = x[u].x;
    M = fmaxf(M, x[u].x);
  }
  M = wave_max(M);
  float se = 0.f;
#pragma unroll
  for (int u = 0; u < kSlabNS; ++u)
    if (lane + 64 * u < S) se += x[u].y * __expf(x[u].x - M);
  return SlabRow{M, wave_sum(se)};
}

__global__ void __launch_bounds__(256) slab_argmax_kernel(const float* __restrict__ logits,
                                                          const float2* __restrict__ stats, int B, int V,
                                                          int64_t* __restrict__ ids_out, int64_t ids_ld, int col,
                                                          int32_t* __restrict__ next_ids, int64_t next_ld) {
  const int lane = threadIdx.x & 63, b = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (b >= B) return;  // (whole waves)
  const int S = (V + 15) / 16;
  const float2* st = stats + (int64_t)b * S;
  // best slab of this lane (max desc, slab asc), then of the wave
  float best = -INFINITY;
  int bidx = 0x7fffffff, bpos = lane;
#pragma unroll
  for (int u = 0; u < kSlabNS; ++u) {
    const int c = lane + 64 * u;
    if (c < S) {
      const float m = st[c].x;
      if (m > best) best = m, bidx = c;  // c ascends: ties keep the first
    }
  }
  wave_best(best, bidx, bpos);
  // the slab's 16 logits: the first column holding the maximum
  const int c = bidx * 16 + lane;
  float v = -INFINITY;
  int vi = 0x7fffffff, vp = lane;
  if (lane < 16 && c < V) v = logits[(int64_t)b * V + c], vi = c;
  wave_best(v, vi, vp);
  if (lane == 0) {
    ids_out[(int64_t)b * ids_ld + col] = vi;
    if (next_ids) next_ids[(int64_t)b * next_ld] = vi;
  }
}
void slab_argmax(const float* logits, const float2* stats, int B, int V, int64_t* ids_out, int64_t ids_ld, int col,
                 int32_t* next_ids, int64_t next_ld, hipStream_t s) {
  require(slab_select_ok(V), "slab_argmax: V must be in [1, 16384]");
  slab_argmax_kernel<<<(B + 3) / 4, 256, 0, s>>>(logits, stats, B, V, ids_out, ids_ld, col, next_ids, next_ld);
  CAPGEN_HIP(hipGetLastError());
}

// one row's k best (value desc, index asc) from its slab stats: a wave per row, lane 0 leaves them in
// (out_v, out_i)[0 .. k); chosen = this wave's KM-entry LDS scratch (row j = beam index)
// ENDED: a finished row (done, the END-aware step above) offers its one candidate and reads nothing else
template <int KM, bool ENDED = false>
__device__ __forceinline__ void slab_row_topk_wave(const float* __restrict__ logits, const float2* __restrict__ stats,
                                                   const float* __restrict__ prev, int r, int j, int V, int k,
                                                   int logsm, int* chosen, int lane, float* out_v, int* out_i,
                                                   bool done = false) {
  if constexpr (ENDED) {
    if (done) return beam_end_finalists(prev, r, j, V, k, lane, out_v, out_i);  // (the whole wave)
  }
  const int S = (V + 15) / 16;
  float mx[kSlabNS];
  const SlabRow rs = slab_row_stats(stats + (int64_t)r * S, S, lane, mx);
  // each lane's best KM slabs, sorted; then k wave rounds pick the row's k best slabs
  float tv[KM];
  int ti[KM];
  topk_clear<KM>(tv, ti);
#pragma unroll
  for (int u = 0; u < kSlabNS; ++u) {
    const int c = lane + 64 * u;
    if (c < S) topk_insert<KM>(tv, ti, mx[u], c);
  }
  wave_topk_rounds<KM>(tv, ti, k, lane, [&](int sel, float, int slab) {
    if (lane == 0) chosen[sel] = slab;  // (0x7fffffff when S < k: no such slab)
  });
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // lane 0's LDS writes before the reads below
  // the k * 16 candidate logits, scored exactly as the full-row kernel scores them
  const float lse = __logf(rs.se), add = prev ? prev[r] : 0.f;
  topk_clear<KM>(tv, ti);
  const float* x = logits + (int64_t)r * V;
  for (int e = lane; e < k * 16; e += 64) {
    const int sl = chosen[e >> 4];
    if (sl == 0x7fffffff) continue;
    const int c = sl * 16 + (e & 15);
    if (c >= V) continue;
    const float xv = x[c];
    topk_insert<KM>(tv, ti, (logsm ? (xv - rs.M) - lse : __expf(xv - rs.M) / rs.se) + add, j * V + c);
  }
  wave_topk_rounds<KM>(tv, ti, k, lane, [&](int sel, float v, int i) {
    if (lane == 0) out_v[sel] = v, out_i[sel] = i;
  });
}

template <int KM>
__global__ void __launch_bounds__(256) slab_row_topk_kernel(const float* __restrict__ logits,
                                                            const float2* __restrict__ stats,
                                                            const float* __restrict__ prev, int rows, int B, int V,
                                                            int k, int logsm, float* __restrict__ cand_v,
                                                            int* __restrict__ cand_i) {
  __shared__ int chosen[4][KM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = blockIdx.x * 4 + wave;
  if (r >= rows) return;  // (whole waves; no workgroup barrier below)
  slab_row_topk_wave<KM>(logits, stats, prev, r, r / B, V, k, logsm, chosen[wave], lane, cand_v + (int64_t)r * k,
                         cand_i + (int64_t)r * k);
}

// The whole beam step of one image in ONE workgroup (round 6): wave j takes beam row j * B + i's k best
// (slab_row_topk_wave) into LDS, wave 0 merges the k_in * k finalists (beam_merge_wave, as
// beam_merge_kernel), and every thread then moves the image's k new rows -- sequences and ids gathered
// from their source beams with the chosen token at column t + 1, and the beam K/V row table
// (model.py:186-198) -- which took four more launches (merge, two gathers, the row table) per token.
// ENDED: the END-aware step (above): finished rows offer one candidate, lane 0 of the merge also writes the
// new rows' fin / len (e: double-buffered like the other arrays) and logsm is 1; false: the reference step
template <int KM, bool ENDED = false>
__global__ void __launch_bounds__(1024) beam_slab_step_kernel(
    const float* __restrict__ logits, const float2* __restrict__ stats, const float* __restrict__ prev, int k_in,
    int B, int V, int k, int logsm, float* __restrict__ out_prob, int32_t* __restrict__ out_src,
    int32_t* __restrict__ out_tok, const int64_t* __restrict__ seq_src, int64_t* __restrict__ seq_dst, int Tw,
    const int32_t* __restrict__ ids_src, int32_t* __restrict__ ids_dst, const int32_t* __restrict__ kv_src,
    int32_t* __restrict__ kv_dst, int Tc, int t, BeamEndArg<ENDED> e) {
  __shared__ int chosen[16][KM];
  __shared__ float cv[256];
  __shared__ int ci[256];
  __shared__ int bsrc[16], btok[16];
  const int i = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (wave < k_in) {
    bool done = false;
    if constexpr (ENDED) done = e.fin_src[wave * B + i] != 0;
    slab_row_topk_wave<KM, ENDED>(logits, stats, prev, wave * B + i, wave, V, k, logsm, chosen[wave], lane,
                                  cv + wave * k, ci + wave * k, done);
  }
  __syncthreads();
  if (wave == 0)
    beam_merge_wave(
        k_in * k, k, lane, [&](int en, float& v, int& c) { v = cv[en], c = ci[en]; },
        [&](int sel, float best, int bidx) {
          if constexpr (ENDED) {
            beam_end_emit(e, sel, i, B, V, best, bidx, out_prob, out_src, out_tok, bsrc[sel], btok[sel]);
          } else {
            out_prob[sel * B + i] = best;
            out_src[sel * B + i] = bsrc[sel] = bidx / V;
            out_tok[sel * B + i] = btok[sel] = bidx % V;
          }
        });
  __syncthreads();
  // the image's k new rows r = j * B + i from their source rows bsrc[j] * B + i (double-buffered arrays)
  for (int e = threadIdx.x; e < k * (Tw + 2 * Tc); e += blockDim.x) {
    const int j = e / (Tw + 2 * Tc), q = e % (Tw + 2 * Tc);
    const int64_t r = (int64_t)j * B + i, srow = (int64_t)bsrc[j] * B + i;
    if (q < Tw) {
      seq_dst[r * Tw + q] = q == t + 1 ? (int64_t)btok[j] : seq_src[srow * Tw + q];
    } else if (q < Tw + Tc) {
      const int cc = q - Tw;
      ids_dst[r * Tc + cc] = cc == t + 1 ? btok[j] : ids_src[srow * Tc + cc];
    } else {
      const int cc = q - Tw - Tc;
      kv_dst[r * Tc + cc] = cc <= t ? kv_src[srow * Tc + cc] : (cc == t + 1 ? (int32_t)r : 0);
    }
  }
}

// The launches of a checked BeamStep (the table in select.h); ea: the kernels' last argument
template <bool ENDED>
static void beam_step_launch(const BeamStep& b, BeamEndArg<ENDED> ea, hipStream_t s) {
  const BeamReorder* ro = b.reorder;
  const BeamGroups* gr = b.groups && b.groups->G > 1 ? b.groups : nullptr;
  const int k = b.k, k_in = b.k_in, B = b.B, V = b.V, rows = k_in * B, logsm = ENDED ? 1 : b.logsm;
  if constexpr (ENDED) {
    if (b.forced) {  // kf finalists and the slot words' scores per row, then the bank round-robin
      const int kf = std::min(16, k + b.forced->W + 1);
      BeamEndForced ef;
      static_cast<BeamEnd&>(ef) = ea, ef.f = *b.forced;
      with_km(kf, [&](auto km) {
        beam_row_topk<decltype(km)::value, true, true>(b.logits, b.prev, rows, B, V, kf, 1, b.cand_v, b.cand_i, s, ef);
      });
      CAPGEN_HIP(hipGetLastError());
      beam_forced_merge_kernel<<<B, 64, 0, s>>>(b.cand_v, b.cand_i, k_in, B, V, k, kf, b.out_prob, b.out_src, b.out_tok, ef);
      CAPGEN_HIP(hipGetLastError());
      return;
    }
  }
  with_km(k, [&](auto km) {
    constexpr int KM = decltype(km)::value;
    if (ro)
      beam_slab_step_kernel<KM, ENDED><<<B, 64 * k_in, 0, s>>>(
          b.logits, b.stats, b.prev, k_in, B, V, k, logsm, b.out_prob, b.out_src, b.out_tok, ro->seq_src, ro->seq_dst,
          ro->Tw, ro->ids_src, ro->ids_dst, ro->kv_src, ro->kv_dst, ro->Tc, ro->t, ea);
    else if (b.stats)
      slab_row_topk_kernel<KM><<<(rows + 3) / 4, 256, 0, s>>>(b.logits, b.stats, b.prev, rows, B, V, k, logsm, b.cand_v,
                                                              b.cand_i);
    else beam_row_topk<KM, ENDED>(b.logits, b.prev, rows, B, V, k, logsm, b.cand_v, b.cand_i, s, ea);
  });
  if constexpr (ENDED) {
    if (gr) {
      beam_group_merge_kernel<<<B, 64, 0, s>>>(b.cand_v, b.cand_i, k_in, B, V, k, gr->G, gr->lambda, b.out_prob,
                                               b.out_src, b.out_tok, ea);
      CAPGEN_HIP(hipGetLastError());
      return;
    }
  }
  if (!ro) beam_merge_kernel<ENDED><<<B, 64, 0, s>>>(b.cand_v, b.cand_i, k_in, B, V, k, b.out_prob, b.out_src, b.out_tok, ea);
  CAPGEN_HIP(hipGetLastError());
}

void beam_step(const BeamStep& b, hipStream_t s) {
  const BeamEnd* e = b.end;
  const BeamReorder* ro = b.reorder;
  const int k = b.k, k_in = b.k_in, V = b.V;
  require(k >= 1 && k <= 16 && k_in >= 1 && k_in * k <= 256, "beam_step: k in [1, 16], k_in * k in [1, 256]");
  if (b.groups) {
    require(b.groups->G >= 1 && b.groups->G <= k && k % b.groups->G == 0,
            "beam_step: num_groups must be in [1, beam_size] and divide it");
    require(b.groups->lambda >= 0.f && b.groups->lambda < INFINITY,
            "beam_step: diversity_penalty must be finite and >= 0");  // (false for a NaN)
  }
  const BeamGroups* gr = b.groups && b.groups->G > 1 ? b.groups : nullptr;  // (one group: no groups)
  require(!gr || (e && !b.stats && !ro), "beam_step: groups need end and take neither stats nor reorder");
  require(!gr || k_in == 1 || k_in == k, "beam_step: k_in must be 1 or k with groups");
  const BeamForced* fo = b.forced;
  if (fo) {
    require(e && !b.stats && !ro && !b.groups, "beam_step: forced needs end and takes none of stats, reorder and groups");
    require(fo->W >= 1 && k + fo->W <= 15, "beam_step: beam_size + words must be <= 15, words >= 1");
    require(k + fo->W + 1 <= V, "beam_step: beam_size + words + 1 must be <= num_vocab");
    require(k_in <= k, "beam_step: k_in must be <= k with forced");
    require(fo->word && fo->group && fo->met_src && fo->met_dst, "beam_step: null word / group / met");
    require(fo->met_src != fo->met_dst, "beam_step: met must be double-buffered");
  }
  require(!ro || b.stats, "beam_step: reorder without stats (the one-launch form selects from the slab stats)");
  require(!e || !b.stats || ro, "beam_step: end with stats but without reorder (no END-aware two-launch slab form)");
  require(!b.stats || slab_select_ok(V), "beam_step: V must be in [1, 16384] with stats");
  require(!ro || k_in <= 16, "beam_step: k_in in [1, 16] with reorder");
  require(!ro || (ro->t + 1 < ro->Tw && ro->t + 1 < ro->Tc), "beam_step: t + 1 < width (Tw, Tc)");
  if (e) require_beam_end("beam_step", V, *e);
  if (hz::active() && (ro || e)) {  // (the two-launch reference forms record nothing)
    using namespace hz;
    const int64_t Rin = (int64_t)k_in * b.B, R = (int64_t)k * b.B, S = (V + 15) / 16;
    const BeamEnd n = e ? *e : BeamEnd{};  // (null arrays: no region)
    if (ro)
      op(s, e ? "beam_slab_step_ended" : "beam_slab_step",
         {rd(b.logits, Rin * V * 4), rd(b.stats, Rin * S * 8), rd(b.prev, b.prev ? Rin * 4 : 0), rd(n.fin_src, Rin * 4),
          rd(n.len_src, Rin * 4), wr(n.fin_dst, R * 4), wr(n.len_dst, R * 4), wr(b.out_prob, R * 4),
          wr(b.out_src, R * 4), wr(b.out_tok, R * 4), rd(ro->seq_src, R * ro->Tw * 8), wr(ro->seq_dst, R * ro->Tw * 8),
          rd(ro->ids_src, R * ro->Tc * 4), wr(ro->ids_dst, R * ro->Tc * 4), rd(ro->kv_src, R * ro->Tc * 4),
          wr(ro->kv_dst, R * ro->Tc * 4)});
    else if (fo) {
      const int64_t Wn = fo->W, kf = std::min<int64_t>(16, k + Wn + 1);
      op(s, "beam_row_topk_forced", {rd(b.logits, Rin * V * 4), rd(b.prev, b.prev ? Rin * 4 : 0), rd(n.fin_src, Rin * 4),
                                     rd(fo->word, b.B * Wn * 4), wr(b.cand_v, Rin * (kf + Wn) * 4),
                                     wr(b.cand_i, Rin * kf * 4)});
      op(s, "beam_forced_merge",
         {rd(b.cand_v, Rin * (kf + Wn) * 4), rd(b.cand_i, Rin * kf * 4), rd(n.fin_src, Rin * 4), rd(n.len_src, Rin * 4),
          rd(fo->word, b.B * Wn * 4), rd(fo->group, b.B * Wn * 4), rd(fo->met_src, Rin * 4), wr(b.out_prob, R * 4),
          wr(b.out_src, R * 4), wr(b.out_tok, R * 4), wr(n.fin_dst, R * 4), wr(n.len_dst, R * 4),
          wr(fo->met_dst, R * 4)});
    } else {
      op(s, "beam_row_topk_ended", {rd(b.logits, Rin * V * 4), rd(b.prev, b.prev ? Rin * 4 : 0), rd(n.fin_src, Rin * 4),
                                    wr(b.cand_v, Rin * k * 4), wr(b.cand_i, Rin * k * 4)});
      op(s, gr ? "beam_group_merge" : "beam_merge_ended",
         {rd(b.cand_v, Rin * k * 4), rd(b.cand_i, Rin * k * 4), rd(n.fin_src, Rin * 4), rd(n.len_src, Rin * 4),
          wr(b.out_prob, R * 4), wr(b.out_src, R * 4), wr(b.out_tok, R * 4), wr(n.fin_dst, R * 4),
          wr(n.len_dst, R * 4)});
    }
  }
  if (e) beam_step_launch<true>(b, *e, s);
  else beam_step_launch<false>(b, NoBeamEnd{}, s);
}

// The end of the END-aware search (definition above), one wave per image, lane j = hypothesis j (k <= 16):
// the final scores, each hypothesis' rank by counting the ones ordered before it, then the n_best rows.
// NORM = false: alpha == 0, the score is logp itself.
// MET: beam_forced's finish -- popcount(met) ranks before the score, met_out (nullable) gets the masks.
template <bool NORM, bool MET = false>
__global__ void __launch_bounds__(64) beam_finish_kernel(const int64_t* __restrict__ seq, const float* __restrict__ logp,
                                                         const int32_t* __restrict__ len, int k, int B, int Tw,
                                                         float alpha, int n_best, int64_t* __restrict__ ids_out,
                                                         float* __restrict__ score_out, float* __restrict__ logp_out,
                                                         int32_t* __restrict__ len_out,
                                                         const int32_t* __restrict__ met = nullptr,
                                                         int32_t* __restrict__ met_out = nullptr) {
  __shared__ int order[16];  // order[rank] = hypothesis
  const int i = blockIdx.x, lane = threadIdx.x;
  const bool on = lane < k;
  const float lp = on ? logp[lane * B + i] : 0.f;
  const int ln = on ? len[lane * B + i] : 0;
  float sc = lp;
  if constexpr (NORM) sc = lp / powf((float)max(ln, 1), alpha);
  const float key = sc == sc ? sc : -INFINITY;  // (a NaN ranks last among equals, by beam index)
  int rank = 0, mt = 0;
  if constexpr (MET) {
    mt = on ? met[lane * B + i] : 0;
    const int bank = __popc((unsigned)mt);
    for (int j = 0; j < k; ++j) {
      const float kj = __shfl(key, j, 64);
      const int bj = __shfl(bank, j, 64);
      rank += (bj > bank || (bj == bank && (kj > key || (kj == key && j < lane)))) ? 1 : 0;
    }
  } else {
    for (int j = 0; j < k; ++j) {
      const float kj = __shfl(key, j, 64);
      rank += (kj > key || (kj == key && j < lane)) ? 1 : 0;
    }
  }
  if (on && rank < n_best) {
    if constexpr (MET)
      if (met_out) met_out[rank * B + i] = mt;
    order[rank] = lane;
    if (score_out) score_out[rank * B + i] = sc;
    if (logp_out) logp_out[rank * B + i] = lp;
    if (len_out) len_out[rank * B + i] = ln;
  }
  __syncthreads();
  for (int en = lane; en < n_best * Tw; en += 64) {
    const int rk = en / Tw, q = en % Tw;
    ids_out[((int64_t)rk * B + i) * Tw + q] = seq[((int64_t)order[rk] * B + i) * Tw + q];
  }
}
void beam_finish(const int64_t* seq, const float* logp, const int32_t* len, int k, int B, int Tw, float alpha,
                 int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out, hipStream_t s,
                 const int32_t* met, int32_t* met_out) {
  require(k >= 1 && k <= 16, "beam_finish: beam_size must be in [1, 16]");
  require(n_best >= 1 && n_best <= k, "beam_finish: n_best must be in [1, beam_size]");
  require(alpha >= 0.f && alpha < INFINITY, "beam_finish: length_penalty must be finite and >= 0");  // (false for a NaN)
  require(B >= 1 && Tw >= 1 && seq && logp && len && ids_out, "beam_finish: need B, width >= 1 and non-null arrays");
  require(met || !met_out, "beam_finish: met_out without met");
  if (hz::active()) {
    using namespace hz;
    const int64_t R = (int64_t)k * B, Ro = (int64_t)n_best * B;
    op(s, "beam_finish", {rd(seq, R * Tw * 8), rd(logp, R * 4), rd(len, R * 4), wr(ids_out, Ro * Tw * 8),
                          wr(score_out, score_out ? Ro * 4 : 0), wr(logp_out, logp_out ? Ro * 4 : 0),
                          wr(len_out, len_out ? Ro * 4 : 0), rd(met, met ? R * 4 : 0),
                          wr(met_out, met_out ? Ro * 4 : 0)});
  }
  if (met) {
    if (alpha == 0.f)
      beam_finish_kernel<false, true><<<B, 64, 0, s>>>(seq, logp, len, k, B, Tw, alpha, n_best, ids_out, score_out, logp_out, len_out, met, met_out);
    else
      beam_finish_kernel<true, true><<<B, 64, 0, s>>>(seq, logp, len, k, B, Tw, alpha, n_best, ids_out, score_out, logp_out, len_out, met, met_out);
    CAPGEN_HIP(hipGetLastError());
    return;
  }
  if (alpha == 0.f)
    beam_finish_kernel<false><<<B, 64, 0, s>>>(seq, logp, len, k, B, Tw, alpha, n_best, ids_out, score_out, logp_out, len_out);
  else
    beam_finish_kernel<true><<<B, 64, 0, s>>>(seq, logp, len, k, B, Tw, alpha, n_best, ids_out, score_out, logp_out, len_out);
  CAPGEN_HIP(hipGetLastError());
}

// ---- decode constraints: repetition penalty, banned words, minimum length, no-repeat n-grams ----
// One launch between a decode step and its selection (beam_nbest and sample; greedy and beam are the
// reference's decoders and are never constrained).  The step at position t predicts column t + 1.  Row r's
// emitted tokens are e = ids[r][1 .. t]; <START> in column 0 is not counted.  From the classifier's logits z
// the constrained logits are built in this order:
// 1. Repetition penalty theta (1 = off).  For each distinct word w in e: z[w] <- z[w] / theta if z[w] > 0,
//    else z[w] * theta (one f32 division or product).  Once per word, however often the word occurred.
// 2. Banned words.  z[w] <- -inf for every w in the list.
// 3. Minimum length m (0 = off).  z[end_id] <- -inf while t + 1 < m.  An <END> emitted at step t gives
//    len = t + 1, as beam_nbest counts it.
// 4. No-repeat n-gram n (0 = off), when t >= n - 1.  For every a with e[a .. a+n-2] equal to e[t-n+2 .. t],
//    z[e[a+n-1]] <- -inf (a + n - 1 <= t).  With n = 1 every emitted word is blocked.
// - "Blocked" is a logit of -inf, and a slab with nothing left has the stats {-inf, 0}.  Every selection kernel
//   above takes both as absent: exp(-inf - M) and __expf(-inf - M) are 0 for the finite row maximum M, so a
//   blocked word adds nothing to an exp-sum or to a nucleus mass and has probability exactly 0; its score
//   (-inf - M) - lse, its Gumbel score -inf + g and its nucleus key (below every finite logit's) are -inf or
//   last, and topk_insert / wave_best put a -inf candidate behind every finite one.  So a blocked word is
//   selected only where a row has fewer finite words than the selection takes; the engine keeps at least 16
//   (num_vocab - n_banned - max_length >= 16, the most any selection takes from a row).
// - Softmax, log-softmax, top-k, nucleus mass and logp are all taken over what is left: logp_out stays the
//   log-probability under the distribution the token was drawn from.
// - Finished beam rows are edited like any other row: the END-aware step never reads their logits.  In
//   sample <END> stays an ordinary word, so blocking goes on after it.
// - A history entry outside [0, V) names no column and is skipped.
// The kernel: one wave per row, the lanes striding over the history positions and the banned list (either
// may be longer than 64), in three phases: (1) the penalty's read-modify-writes, on distinct columns since
// only a word's first occurrence applies it; (2) the -inf stores, idempotent, so a word both penalised and
// blocked ends blocked; (3) with stats, {max, sum __expf(v - max)} of every touched slab from its (up to 16,
// the last slab of a row fewer) stored logits, summed in the classifier epilogue's order; two lanes repairing
// one slab write the same value.  Between the phases the row's stores must be visible to the other lanes'
// loads: every lane waits for its own stores (vmcnt counts stores on gfx9), then the workgroup barrier; the
// waves of a workgroup share one CU and its write-through L1, so no cache invalidate is needed.
__device__ __forceinline__ void workgroup_stores_visible() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// pen(w) for the first occurrence of every word in e[1 .. t], blk(w) for every blocked word (some twice)
template <class Pen, class Blk>
__device__ __forceinline__ void constrain_visit(const int32_t* __restrict__ e, int V, int t,
                                                const DecodeConstraints& c, int lane, Pen&& pen, Blk&& blk) {
  auto word = [&](int w) { return (unsigned)w < (unsigned)V; };
  if (c.repetition_penalty != 1.f)
    for (int p = 1 + lane; p <= t; p += 64) {
      const int w = e[p];
      bool first = word(w);
      for (int q = 1; q < p && first; ++q) first = e[q] != w;
      if (first) pen(w);
    }
  for (int i = lane; i < c.n_banned; i += 64) {
    const int w = c.banned[i];
    if (word(w)) blk(w);
  }
  if (lane == 0 && c.min_length > 0 && t + 1 < c.min_length && word(c.end_id)) blk(c.end_id);
  const int n = c.no_repeat_ngram;
  if (n > 0 && t >= n - 1)
    for (int a = 1 + lane; a + n - 1 <= t; a += 64) {
      bool match = true;
      for (int i = 0; i < n - 1 && match; ++i) match = e[a + i] == e[t - n + 2 + i];
      const int w = e[a + n - 1];
      if (match && word(w)) blk(w);
    }
}

__global__ void __launch_bounds__(64) constrain_logits_kernel(float* logits, float2* stats, int V, const int32_t* ids,
                                                              int64_t ids_ld, int t, DecodeConstraints c) {
  const int r = blockIdx.x, lane = threadIdx.x;
  float* x = logits + (int64_t)r * V;
  const int32_t* e = ids + (int64_t)r * ids_ld;
  const float theta = c.repetition_penalty;
  auto nothing = [](int) {};
  constrain_visit(
      e, V, t, c, lane,
      [&](int w) {
        const float z = x[w];
        x[w] = z > 0.f ? __fdiv_rn(z, theta) : __fmul_rn(z, theta);
      },
      nothing);
  workgroup_stores_visible();
  constrain_visit(e, V, t, c, lane, nothing, [&](int w) { x[w] = -INFINITY; });
  if (!stats) return;  // (the whole workgroup)
  workgroup_stores_visible();
  float2* st = stats + (int64_t)r * ((V + 15) / 16);
  auto repair = [&](int w) {
    const int sl = w >> 4, c0 = sl * 16;
    float v[16], mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      v[u] = c0 + u < V ? x[c0 + u] : -INFINITY;
      mx = fmaxf(mx, v[u]);
    }
    float q[4];  // the epilogue's order: four columns per lane, then the two xor-shuffles
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      q[g] = 0.f;
#pragma unroll
      for (int u = 4 * g; u < 4 * g + 4; ++u) q[g] += mx > -INFINITY ? __expf(v[u] - mx) : 0.f;  // (never NaN)
    }
    st[sl] = float2{mx, (q[0] + q[1]) + (q[2] + q[3])};
  };
  constrain_visit(e, V, t, c, lane, repair, repair);
}

void constrain_logits(float* logits, float2* stats, int R, int V, const int32_t* ids, int64_t ids_ld, int t,
                      const DecodeConstraints& c, hipStream_t s) {
  require(logits && ids && R >= 1 && V >= 1, "constrain_logits: need logits, ids and R, V >= 1");
  require(t >= 0 && t < ids_ld, "constrain_logits: t must be in [0, ids_ld)");
  require(c.no_repeat_ngram >= 0, "constrain_logits: no_repeat_ngram must be >= 0");
  require(c.end_id >= -1 && c.end_id < V, "constrain_logits: end_id must be in [-1, num_vocab)");
  require(c.min_length >= 0 && (c.min_length == 0 || c.end_id >= 0),
          "constrain_logits: min_length must be >= 0 and needs an end_id");
  require(c.repetition_penalty > 0.f && c.repetition_penalty < INFINITY,
          "constrain_logits: repetition_penalty must be finite and > 0");  // (false for a NaN)
  require(c.n_banned >= 0 && c.n_banned <= 1024 && (c.n_banned == 0 || c.banned),
          "constrain_logits: n_banned must be in [0, 1024], with a banned list");
  if (hz::active()) {
    using namespace hz;
    op(s, "constrain_logits", {rd(ids, (int64_t)R * ids_ld * 4), rd(c.banned, (int64_t)c.n_banned * 4),
                               wr(logits, (int64_t)R * V * 4), wr(stats, stats ? (int64_t)R * ((V + 15) / 16) * 8 : 0)});
  }
  constrain_logits_kernel<<<R, 64, 0, s>>>(logits, stats, V, ids, ids_ld, t, c);
  CAPGEN_HIP(hipGetLastError());
}

// ---- ensemble decoding: K members' logits of a step fused into one row distribution ----------
// One launch between the members' decode steps and the leader's constraints / selection.  Members k < K
// (1 <= K <= 8) hold logits z_k [R][V] of the same R hypotheses; l_k = z_k - logsumexp(z_k) is member k's
// log-softmax row and lw_k = log w_k the log of its (normalised, positive) weight.  Row r of out gets
// - mode 0 (prob, the arithmetic mean of the probabilities): y[v] = log sum_k w_k exp(l_k[v]), evaluated as
//   a = lw_k + l_k[v], m = max_k a, y = m + log(sum_k exp(a - m)): the largest term contributes exactly 1, so
//   y is finite wherever one member's logit is, however far every exp(l_k[v]) itself underflows;
// - mode 1 (logprob, the weighted geometric mean): y[v] = sum_k w_k l_k[v] with w_k = exp(lw_k), summed in
//   member order.  Not normalised: the selection's own log-softmax does that.
// y = -inf only where a member logit is -inf (mode 0: every member's), so -inf keeps its meaning of "blocked"
// for everything downstream, which reads y as the step's logits.  out may be member 0's buffer: every
// element is read (in both passes) by the thread that later stores it, and the second pass starts behind a
// workgroup barrier.
// stats (nullable): {max, sum __expf(y - max)} of every 16-column slab of the STORED y, the form of the
// classifier epilogue (GemmArgs::dec_stats) and in its order -- four columns per lane in column order, then
// the xor-1 and xor-2 exchanges -- with columns at or past V counting as -inf and an empty slab {-inf, 0}.
// The kernel: one workgroup of 256 threads per row, nothing shared between rows, so a row's bits do not
// depend on R or the grid.  Pass 1 reads each member row once, every thread keeping an online (max, sum
// __expf) per member over its columns 4 (tid + 256 u) .. + 3, merged over the wave by xor exchanges (both
// partners compute the same commutative merge) and over the four waves in wave order: lse_k.  Pass 2 reads
// the rows again -- the same workgroup, back to back, so from L2 -- and stores y.  16-byte loads and stores
// where V % 4 == 0 (a lane's four columns are a quarter slab, four neighbouring lanes a slab); otherwise a
// scalar form of the same two passes, and the slab stats from the stored row in a third step, as
// constrain_logits repairs them.
struct EnsembleArgs {
  const float* z[8];
  float lw[8];
};

// (m, s) <- the online-softmax merge of (m, s) and (m2, s2); an empty side has m = -inf, s = 0
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
  const float M = fmaxf(m, m2);
  const float a = m > -INFINITY ? s * expf(m - M) : 0.f, b = m2 > -INFINITY ? s2 * expf(m2 - M) : 0.f;
  m = M, s = a + b;
}
// the fused value of one column from the members' logits zk and log-normalisers
template <int K>
__device__ __forceinline__ float ensemble_one(const float (&zk)[K], const float (&lse)[K], const float (&lw)[K],
                                              const float (&w)[K], int mode) {
  if (mode == 1) {
    float y = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) y += w[k] * (zk[k] - lse[k]);
    return y;
  }
  float a[K], m = -INFINITY;
#pragma unroll
  for (int k = 0; k < K; ++k) a[k] = lw[k] + (zk[k] - lse[k]), m = fmaxf(m, a[k]);
  if constexpr (K == 1) return m;
  // the terms are <= 1 and their sum is in [1, K]: the fast exp and log are good to a few 1e-7 absolute here.
  // Every member blocked: the sum is 0 and its log -inf (no branch, never NaN)
  const float mm = m > -INFINITY ? m : 0.f;
  float se = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) se += __expf(a[k] - mm);
  return mm + __logf(se);
}

template <int K, bool VEC>
__global__ void __launch_bounds__(256) ensemble_combine_kernel(EnsembleArgs A, int mode, int V, float* out,
                                                               float2* stats) {
  __shared__ float sm[K][4], ss[K][4];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row = (int64_t)r * V;
  constexpr int W = VEC ? 4 : 1;  // columns per thread and round
  const int rounds = (V + 256 * W - 1) / (256 * W);  // (uniform: every lane takes part in the exchanges)
  float m[K], s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) m[k] = -INFINITY, s[k] = 0.f;
  for (int u = 0; u < rounds; ++u) {
    const int c = W * (tid + 256 * u);
    if (c >= V) continue;
    float x[K][W];
#pragma unroll
    for (int k = 0; k < K; ++k) load_f<float, W>(A.z[k] + row + c, x[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      float mx = x[k][0];
#pragma unroll
      for (int i = 1; i < W; ++i) mx = fmaxf(mx, x[k][i]);
      // (branch-free: while everything so far is -inf the shift is 0, and exp(-inf) adds 0)
      const float M = fmaxf(m[k], mx), Ms = M > -INFINITY ? M : 0.f;
      float q = s[k] * __expf(m[k] - Ms);
#pragma unroll
      for (int i = 0; i < W; ++i) q += __expf(x[k][i] - Ms);
      m[k] = M, s[k] = q;
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) {
    lse_merge(m[k], s[k], lane_xchg<1>(m[k]), lane_xchg<1>(s[k]));
    lse_merge(m[k], s[k], lane_xchg<2>(m[k]), lane_xchg<2>(s[k]));
    lse_merge(m[k], s[k], lane_xchg<4>(m[k]), lane_xchg<4>(s[k]));
    lse_merge(m[k], s[k], lane_xchg<8>(m[k]), lane_xchg<8>(s[k]));
    lse_merge(m[k], s[k], lane_xchg<16>(m[k]), lane_xchg<16>(s[k]));
    lse_merge(m[k], s[k], lane_xchg<32>(m[k]), lane_xchg<32>(s[k]));
    if (lane == 0) sm[k][wave] = m[k], ss[k][wave] = s[k];
  }
  __syncthreads();  // (also: every read of pass 1 is done before a store of pass 2 -- out may be z[0])
  float lse[K], lw[K], w[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    float mk = sm[k][0], sk = ss[k][0];
#pragma unroll
    for (int v = 1; v < 4; ++v) lse_merge(mk, sk, sm[k][v], ss[k][v]);
    lse[k] = mk + logf(sk);
    lw[k] = A.lw[k], w[k] = expf(A.lw[k]);
  }
  float* y = out + row;
  float2* st = stats ? stats + (int64_t)r * ((V + 15) / 16) : nullptr;
  for (int u = 0; u < rounds; ++u) {
    const int c = W * (tid + 256 * u);
    const bool on = c < V;
    float o[W];
    if (on) {
      float x[K][W];
#pragma unroll
      for (int k = 0; k < K; ++k) load_f<float, W>(A.z[k] + row + c, x[k]);
#pragma unroll
      for (int i = 0; i < W; ++i) {
        float zk[K];
#pragma unroll
        for (int k = 0; k < K; ++k) zk[k] = x[k][i];
        o[i] = ensemble_one<K>(zk, lse, lw, w, mode);
      }
      store_f<float, W>(y + c, o);
    } else {
#pragma unroll
      for (int i = 0; i < W; ++i) o[i] = -INFINITY;
    }
    if constexpr (VEC) {
      if (st) {  // (uniform) the slab of lanes 4 j .. 4 j + 3
        float mx = fmaxf(fmaxf(o[0], o[1]), fmaxf(o[2], o[3]));
        mx = fmaxf(mx, lane_xchg<1>(mx));
        mx = fmaxf(mx, lane_xchg<2>(mx));
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) q += mx > -INFINITY ? __expf(o[i] - mx) : 0.f;  // (never NaN)
        q += lane_xchg<1>(q);
        q += lane_xchg<2>(q);
        if (on && (lane & 3) == 0) st[c >> 4] = float2{mx, q};
      }
    }
  }
  if constexpr (!VEC) {
    if (!st) return;  // (the whole workgroup)
    workgroup_stores_visible();
    for (int sl = tid; sl < (V + 15) / 16; sl += 256) {
      const int c0 = sl * 16;
      float v[16], mx = -INFINITY;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        v[i] = c0 + i < V ? y[c0 + i] : -INFINITY;
        mx = fmaxf(mx, v[i]);
      }
      float q[4];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        q[g] = 0.f;
#pragma unroll
        for (int i = 4 * g; i < 4 * g + 4; ++i) q[g] += mx > -INFINITY ? __expf(v[i] - mx) : 0.f;
      }
      st[sl] = float2{mx, (q[0] + q[1]) + (q[2] + q[3])};
    }
  }
}

void ensemble_combine(const float* const* logits, const float* log_w, int K, int mode, int R, int V, float* out,
                      float2* stats, hipStream_t s) {
  require(K >= 1 && K <= 8, "ensemble_combine: K must be in [1, 8]");
  require(mode == 0 || mode == 1, "ensemble_combine: mode must be 0 (prob) or 1 (logprob)");
  require(logits && log_w && out && R >= 1 && V >= 1, "ensemble_combine: need logits, weights, out and R, V >= 1");
  EnsembleArgs A{};
  bool vec = V % 4 == 0 && (uintptr_t)out % 16 == 0;
  for (int k = 0; k < K; ++k) {
    require(logits[k] != nullptr, "ensemble_combine: null logits of member " + std::to_string(k));
    require(std::isfinite(log_w[k]), "ensemble_combine: log weight of member " + std::to_string(k) + " is not finite");
    A.z[k] = logits[k], A.lw[k] = log_w[k];
    vec = vec && (uintptr_t)logits[k] % 16 == 0;
  }
  if (hz::active()) {
    using namespace hz;
    Rgn rg[10];
    for (int k = 0; k < K; ++k) rg[k] = rd(logits[k], (int64_t)R * V * 4);
    rg[K] = wr(out, (int64_t)R * V * 4);
    rg[K + 1] = wr(stats, stats ? (int64_t)R * ((V + 15) / 16) * 8 : 0);
    op(s, "ensemble_combine", rg, (size_t)K + 2);
  }
  auto launch = [&](auto kc) {
    constexpr int KC = decltype(kc)::value;
    if (vec) ensemble_combine_kernel<KC, true><<<R, 256, 0, s>>>(A, mode, V, out, stats);
    else ensemble_combine_kernel<KC, false><<<R, 256, 0, s>>>(A, mode, V, out, stats);
  };
  switch (K) {
    case 1: launch(std::integral_constant<int, 1>{}); break;
    case 2: launch(std::integral_constant<int, 2>{}); break;
    case 3: launch(std::integral_constant<int, 3>{}); break;
    case 4: launch(std::integral_constant<int, 4>{}); break;
    case 5: launch(std::integral_constant<int, 5>{}); break;
    case 6: launch(std::integral_constant<int, 6>{}); break;
    case 7: launch(std::integral_constant<int, 7>{}); break;
    default: launch(std::integral_constant<int, 8>{}); break;
  }
  CAPGEN_HIP(hipGetLastError());
}

// ---- the generation loops' bookkeeping ------------------------------------------------------
__global__ void init_gen_ids_kernel(int64_t* out, int rows, int width, int32_t* ids, int tcap) {
  int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c < rows * width) out[c] = (c % width) == 0 ? 1 : 0;
  if (c < rows * tcap) ids[c] = (c % tcap) == 0 ? 1 : 0;
}
void init_gen_ids(int64_t* out, int rows, int width, int32_t* ids, int tcap, hipStream_t s) {
  init_gen_ids_kernel<<<(rows * std::max(width, tcap) + 255) / 256, 256, 0, s>>>(out, rows, width, ids, tcap);
  CAPGEN_HIP(hipGetLastError());
}

// dst row r = (j, i) <- src row (src[j][i], i); then optionally set column `col` to tok
template <typename E>
__global__ void beam_gather_kernel(const E* __restrict__ src, E* __restrict__ dst, int64_t row_elems,
                                   int64_t copy_elems, const int32_t* __restrict__ bsrc, int B, int R,
                                   const int32_t* __restrict__ tok, int col) {
  const int r = blockIdx.y;
  const int srow = bsrc[r] * B + (r % B);
  const E* s = src + (int64_t)srow * row_elems;
  E* d = dst + (int64_t)r * row_elems;
  for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; c < copy_elems; c += (int64_t)gridDim.x * blockDim.x)
    d[c] = (tok && c == col) ? (E)tok[r] : s[c];
}
template <typename E>
static void beam_gather_launch(const E* src, E* dst, int row_elems, const int32_t* bsrc, int B, int R,
                               const int32_t* tok, int col, hipStream_t s) {
  beam_gather_kernel<E><<<dim3(1, R), 64, 0, s>>>(src, dst, row_elems, row_elems, bsrc, B, R, tok, col);
  CAPGEN_HIP(hipGetLastError());
}
void beam_gather(const int64_t* src, int64_t* dst, int row_elems, const int32_t* bsrc, int B, int R,
                 const int32_t* tok, int col, hipStream_t s) {
  beam_gather_launch(src, dst, row_elems, bsrc, B, R, tok, col, s);
}
void beam_gather(const int32_t* src, int32_t* dst, int row_elems, const int32_t* bsrc, int B, int R,
                 const int32_t* tok, int col, hipStream_t s) {
  beam_gather_launch(src, dst, row_elems, bsrc, B, R, tok, col, s);
}

__global__ void beam_kvrow_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int Tc, int t,
                                  const int32_t* __restrict__ bsrc, int B, int R) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= R * Tc) return;
  const int r = e / Tc, c = e % Tc;
  const int srow = bsrc[r] * B + (r % B);
  dst[e] = c <= t ? src[(int64_t)srow * Tc + c] : (c == t + 1 ? r : 0);
}
void beam_kvrow(const int32_t* src, int32_t* dst, int Tc, int t, const int32_t* bsrc, int B, int R, hipStream_t s) {
  beam_kvrow_kernel<<<(R * Tc + 255) / 256, 256, 0, s>>>(src, dst, Tc, t, bsrc, B, R);
  CAPGEN_HIP(hipGetLastError());
}

}  // namespace capgen
