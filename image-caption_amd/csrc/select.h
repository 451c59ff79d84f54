// capgen — decode selection: greedy argmax, beam top-k, sampled / nucleus decoding and the beam
// bookkeeping of the generation loops (launcher interface; kernels and their contracts: select.hip).
#pragma once
#include "capgen_common.h"
#include "gemm.h"

namespace capgen {

// greedy: out token = argmax(softmax(logits[b])) (first index on ties)   (model.py:126-128)
void argmax_softmax(const float* logits, int B, int V, int64_t* ids_out, int64_t ids_ld, int col,
                    int32_t* next_ids, int64_t next_ld, hipStream_t s, int logsm = 0);
// sampled decoding: token of row r ~ softmax(logits[r] * inv_tau) restricted to the row's top_k logits
// (top_k = 0: every column), drawn by Gumbel-max from the counter hash of (seed, site, r * V + v);
// logp_out (optional): its log-probability under that distribution.
void sample_softmax(const float* logits, int R, int V, float inv_tau, int top_k, uint64_t seed, uint32_t site,
                    int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids, int64_t next_ld, float* logp_out,
                    int64_t logp_ld, int logp_col, hipStream_t s);
// nucleus (top-p) sampling: sample_softmax with the candidate set cut to the columns v whose strictly
// more likely columns hold less than top_p of the (top_k-renormalised) mass; top_p in (0, 1], 1 launches
// sample_softmax's kernels.  count_out (optional): the size of each row's candidate set.
void sample_nucleus(const float* logits, int R, int V, float inv_tau, int top_k, float top_p, uint64_t seed,
                    uint32_t site, int64_t* ids_out, int64_t ids_ld, int col, int32_t* next_ids, int64_t next_ld,
                    float* logp_out, int64_t logp_ld, int logp_col, int32_t* count_out, hipStream_t s);
// bf16 decode selection from the classifier epilogue's slab stats (GemmArgs::dec_stats: {max,
// sum exp(v - max)} per row and 16-column slab, stats row stride S = ceil(V / 16)):
// greedy -- argmax of the logits (first index on ties), read from the best slab only;
// beam -- each row's k best scores from its k best slabs (every top-k element lies in the k
// slabs with the largest maxima under (max desc, slab asc)), then the per-image merge.
// V <= 16384 (S <= 1024 slabs, 16 per lane in registers).
bool slab_select_ok(int V);
void slab_argmax(const float* logits, const float2* stats, int B, int V, int64_t* ids_out, int64_t ids_ld, int col,
                 int32_t* next_ids, int64_t next_ld, hipStream_t s);

// The END-aware beam step (beam_nbest; definition: select.hip): a finished source row offers one candidate
// (its logp, token 0) whatever its logits hold, a live one its log-softmax scores (always, as logsm = 1
// scores them).  fin / len of the k_in * B source rows are read, those of the k * B new rows written.
struct BeamEnd {
  const int32_t* fin_src;
  const int32_t* len_src;
  int32_t* fin_dst;
  int32_t* len_dst;
  int end_id;  // -1: nothing ever finishes
};
// the one-launch form's reorder behind its selection: sequences [.][Tw] (int64), ids and the K/V row table
// [.][Tc] (int32) of the k * B new rows gathered from their source beams, chosen token at column t + 1 < Tw, Tc
struct BeamReorder {
  const int64_t* seq_src = nullptr;
  int64_t* seq_dst = nullptr;
  const int32_t *ids_src = nullptr, *kv_src = nullptr;
  int32_t *ids_dst = nullptr, *kv_dst = nullptr;
  int Tw = 0, Tc = 0, t = 0;  // (filled by name, as BeamStep: adjacent pointers of one type are easy to swap)
};
// Diverse beam search (beam_diverse; definition: select.hip): the k beams are G groups of k / G, served in
// order; a group's live candidates lose lambda for every hypothesis an earlier group of the image chose at
// this step with the same token.  G divides k, lambda finite and >= 0.
struct BeamGroups {
  int G;
  float lambda;
};
// Forced-word beam search (beam_forced; definition: select.hip): image i has W slots (word[i * W + s],
// group[i * W + s]), word = -1 an empty slot, group in [0, 16); met [rows] is each hypothesis' bitmask of the
// groups it has met, read from met_src and written to met_dst like fin / len.  k + W <= 15, k + W + 1 <= V.
struct BeamForced {
  const int32_t* word;
  const int32_t* group;
  int W;
  const int32_t* met_src;
  int32_t* met_dst;
};
// One beam-search step (model.py:183-190): rows j * B + i (j < k_in) of logits [k_in * B][V]; per image i the
// k best (prev[j * B + i] (null: 0) + softmax, or log-softmax with logsm, of row j * B + i at v) under (score
// desc, j * V + v asc) -> out_prob / src / tok[sel * B + i].  k, k_in >= 1, k <= 16, k_in * k <= 256.
// The five nullable members choose the kernels, and beam_step is the only place that knows how:
//   end   stats  reorder  groups  forced   launches
//   null  null   null     null    null     beam_row_topk_kernel (the exact full-row softmax) + beam_merge_kernel
//   null  set    null     null    null     slab_row_topk_kernel + beam_merge_kernel
//   null  set    set      null    null     beam_slab_step_kernel: selection, merge and reorder in one launch per image
//   set   null   null     null    null     beam_row_topk_kernel<ENDED> + beam_merge_kernel<ENDED>
//   set   set    set      null    null     beam_slab_step_kernel<ENDED>
//   set   null   null     set     null     beam_row_topk_kernel<ENDED> + beam_group_merge_kernel (k_in = 1 or k)
//   set   null   null     null    set      beam_row_topk_kernel<ENDED, FORCED> with kf = min(16, k + W + 1) finalists and
//                                          the W forced-word scores per row + beam_forced_merge_kernel (k_in <= k)
// Every other combination has no kernel and is refused.  groups with G = 1 is no groups at all: the step is
// the null-groups row of the same end / stats / reorder, whatever lambda.  stats: the rows' slab stats (above; V <= 16384); the
// one-launch form also needs k_in <= 16.  cand_v / cand_i: k_in * B * k scratch (each row's k finalists) of
// the two-launch forms only.  With end set the step always scores with the log-softmax: logsm is ignored.
// forced: cand_v is k_in * B * (kf + W) (row r: its kf finalists' scores, then its W forced-word scores) and
// cand_i k_in * B * kf.
struct BeamStep {
  const float* logits = nullptr;
  const float2* stats = nullptr;
  const float* prev = nullptr;
  int k_in = 0, B = 0, V = 0, k = 0, logsm = 0;
  float *cand_v = nullptr, *out_prob = nullptr;
  int32_t *cand_i = nullptr, *out_src = nullptr, *out_tok = nullptr;
  const BeamEnd* end = nullptr;          // null: the reference step
  const BeamReorder* reorder = nullptr;  // null: selection only
  const BeamGroups* groups = nullptr;    // null: one group
  const BeamForced* forced = nullptr;    // null: no forced words
};
void beam_step(const BeamStep& b, hipStream_t s);
// the end of the search: score = logp (alpha == 0) or logp / max(len, 1)^alpha; per image the n_best of the
// k hypotheses (rows j * B + i of seq [k * B][Tw], logp, len) under (score desc, beam asc) -> row
// rank * B + i of ids_out [n_best * B][Tw], score_out, logp_out, len_out (the last three nullable).
// met (null: none; beam_forced's [k * B] bitmasks): the order is (popcount(met) desc, score desc, beam asc), and
// met_out (nullable) [n_best * B] gets the chosen hypotheses' masks.
void beam_finish(const int64_t* seq, const float* logp, const int32_t* len, int k, int B, int Tw, float alpha,
                 int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out, hipStream_t s,
                 const int32_t* met = nullptr, int32_t* met_out = nullptr);

// Decode constraints (beam_nbest and sample; definition: select.hip): what a row may not say next, from its
// own token history.  banned is a DEVICE array here (the C ABI's struct carries a host one).
struct DecodeConstraints {
  int no_repeat_ngram = 0;         // 0: off
  int min_length = 0;              // 0: off; needs end_id >= 0
  int end_id = -1;
  float repetition_penalty = 1.f;  // 1: off
  const int32_t* banned = nullptr;
  int n_banned = 0;
  bool on() const { return no_repeat_ngram > 0 || min_length > 0 || repetition_penalty != 1.f || n_banned > 0; }
};
// edits logits [R][V] in place before the selection of position t (row r's history: ids[r * ids_ld + 1 .. t]);
// stats (nullable): the rows' slab stats [R][ceil(V / 16)], rebuilt for every slab an edit touched
void constrain_logits(float* logits, float2* stats, int R, int V, const int32_t* ids, int64_t ids_ld, int t,
                      const DecodeConstraints& c, hipStream_t s);

// Ensemble decoding (definition: select.hip): the K members' logits [R][V] of one step (logits: a HOST array
// of K device pointers, log_w: K host floats, log of the normalised weights) fused into out [R][V], which
// everything downstream reads as the step's logits.  mode 0: log sum_k w_k softmax_k, mode 1:
// sum_k w_k log_softmax_k.  out may be logits[0]; stats (nullable): out's slab stats [R][ceil(V / 16)].
void ensemble_combine(const float* const* logits, const float* log_w, int K, int mode, int R, int V, float* out,
                      float2* stats, hipStream_t s);

// the generation loops' bookkeeping
// out [rows][width] (int64) and ids [rows][tcap] (int32): column 0 = <START> (1), the rest 0
void init_gen_ids(int64_t* out, int rows, int width, int32_t* ids, int tcap, hipStream_t s);
// beam reorder of a [R][row_elems] array: dst row r = (j, i) <- src row (bsrc[r], i), then column col = tok[r]
void beam_gather(const int64_t* src, int64_t* dst, int row_elems, const int32_t* bsrc, int B, int R,
                 const int32_t* tok, int col, hipStream_t s);
void beam_gather(const int32_t* src, int32_t* dst, int row_elems, const int32_t* bsrc, int B, int R,
                 const int32_t* tok, int col, hipStream_t s);
// beam reorder of the K/V row table (attention kv_row) [R][Tc]: row r's positions 0..t come from its
// source beam's row, position t + 1 (written by row r's own next decoder step) is row r
void beam_kvrow(const int32_t* src, int32_t* dst, int Tc, int t, const int32_t* bsrc, int B, int R, hipStream_t s);

}  // namespace capgen
