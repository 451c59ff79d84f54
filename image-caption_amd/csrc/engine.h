// capgen — the training/decoding engine behind the C ABI (include/capgen.h).
//
// One engine = one (process, device).  It owns the packed f32 parameter arena (+ bf16
// shadow for the MFMA path), the gradient arena, Adam moments and every activation
// buffer, and sequences the hot path as explicit forward/backward kernel launches on
// its own HIP stream — no autograd, no tracing compiler.  A train step is captured once
// per (shape, input pointers) into a hipGraph and replayed.
//
// Reference call stack restated: models.py:115-126 train_step ->
// model.py:79-98 forward -> Encoder (model.py:294-332) -> EncoderBlock (modules.py:146-157)
// -> Decoder (model.py:419-459) -> DecoderBlock (modules.py:185-206) -> classifier + CE
// (model.py:93-96) -> autograd backward -> Adam.step.
//
// This header is the engine's shape: the helper types, every data member grouped by concern, the
// switches frozen at creation in one block, and -- inline -- what is small and called per launch (the
// step is host-issue bound, and there is no LTO).  Everything larger is declared at the end and
// defined by concern in engine_forward / _backward / _update / _step / _decode.hip; the C ABI over it
// is api.hip (hooks.hip: the handle-free test hooks, which do not read this header).
#pragma once
#include <rccl/rccl.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/capgen.h"
#include "attention.h"
#include "gemm.h"
#include "hazard.h"
#include "layout.h"
#include "ops.h"
#include "qkv_attn.h"
#include "select.h"
#include "variants.h"
#include "rl.h"

namespace capgen {

#define NCCL_CHECK(expr)                                                                             \
  do {                                                                                               \
    ncclResult_t _r = (expr);                                                                        \
    if (_r != ncclSuccess) throw Error(std::string(#expr) + ": " + ncclGetErrorString(_r));          \
  } while (0)

// bump allocator: a dry run (base == nullptr) sizes the block, the second run assigns pointers
struct Planner {
  char* base = nullptr;
  size_t used = 0;
  void* raw(size_t bytes) {
    size_t off = (used + 255) & ~size_t(255);
    used = off + bytes;
    return base ? base + off : nullptr;
  }
  template <class P>
  void take(P*& p, size_t count) {
    p = (P*)raw(count * sizeof(P));
  }
};

// a value set for a scope: the old one is put back when the scope ends, also by an exception
template <class T>
struct Scoped {
  T& ref;
  T old;
  Scoped(T& r, T v) : ref(r), old(r) { r = v; }
  ~Scoped() { ref = old; }
};

// What the forward and the backward of one LayerNorm site share: the saved input and statistics,
// the arena offsets of gamma, beta and the producing Linear's bias (-1: none), the row mask and
// the dropout on the Linear's output.  ln_fwd / ln_bwd turn it into the launch descriptors.
struct LnSite {
  int M, d;
  void* v;
  float *mean, *rstd;
  int64_t g, b, bias;
  RowMask mask;
  Drop drop;
};

// the step inputs that reach forward() beside its arguments (set for the scope of one C-ABI call)
struct StepIn {
  const int32_t* idx = nullptr;  // resident feature store: forward() gathers image idx[b] from feats/pos
  int n_img = 0;                 // ... of n_img images
  // per-caption loss weights [B] (capgen_train_step_weighted): forward()'s CE scales caption b's loss
  // rows and logit gradients by w[b]; the count stays the number of non-pad targets
  const float* w = nullptr;
  // score mode (capgen_score_captions): forward()'s classifier section ends in score_finish / score_rows,
  // which write these, in place of the CE kernels, loss_finalize and every collective; dropout is off
  bool score = false;
  float* s_tok = nullptr;    // [B, T-1] token log-probabilities, or null
  float* s_logp = nullptr;   // [B]
  int32_t* s_len = nullptr;  // [B] or null
  int32_t* s_hits = nullptr;  // [B] or null
  bool operator==(const StepIn& o) const {
    return idx == o.idx && n_img == o.n_img && w == o.w && score == o.score && s_tok == o.s_tok &&
           s_logp == o.s_logp && s_len == o.s_len && s_hits == o.s_hits;
  }
};

struct EncAct {
  void *qkv, *att, *v1, *Y, *H, *v2;
  float *P, *m1, *r1, *m2, *r2;
};
struct DecAct {
  void *qkv, *atts, *vs, *D1, *qc, *attc, *vc, *D2, *H, *vf;
  float *Ps, *ms, *rs, *Pc, *mc, *rc, *mf, *rf;
};

struct Acts {
  int B = 0, N = 0, T = 0;  // capacity
  // encoder
  void* Aenc;
  uint8_t* valid;
  void* ev0;
  float *em0, *er0;
  std::vector<void*> X;
  std::vector<EncAct> enc;
  void* KV;
  // decoder
  int32_t *ids, *tgt;
  float* count;
  void* E;
  void* dv0;
  float *dm0, *dr0;
  std::vector<void*> D;
  std::vector<DecAct> dec;
  float* logits;
  void* dlogits;
  float2* ce_stats;  // fused classifier + CE (bf16): {max, sum exp} per row and 16-column slab
  float* ce_tl;      // its target logits
  float* sc_tok;     // score mode, logits path: per-row log-probability when the caller wants none ...
  int32_t* sc_hit;   // ... and per-row hits, read by the per-caption pass
  float *loss_row, *grad_scale, *loss, *loss_ce;
  void* gEnc;     // encoder-chain residual gradient while decoder block 0 finishes on es2 (overlap_dec0)
  // SCST (rl.hip): per-row sample / lse / logp[sample] / entropy, per-image entropy, scalars
  int32_t* rl_sample;
  float *rl_lse, *rl_logp, *rl_ent, *rl_ent_img, *rl_score, *rl_scal;
  // scratch / backward.  gOut/gRes carry the residual-stream gradient (critical path);
  // every other gradient buffer is per block, so the weight-gradient GEMMs that read them can
  // run later on the side stream without a write-after-read hazard.
  void *tmp, *gOut, *gRes, *gKV, *gE, *gAe, *gAd;
  void* tmpf;  // the decoder front's GEMM -> LayerNorm scratch (runs on es2 beside the encoder)
  struct GradBufs {
    void *gAf, *gH, *gA1, *gATT1, *gQKV, *gA2, *gATT2, *gQc;
  };
  std::vector<GradBufs> genc, gdec;
  // split_image_objects (model.py:258-292): the image block runs over 2*B*N pair rows
  void *siY, *siEp, *siX2, *siZ, *siV, *siG0, *siG1, *siGY, *siGEp;
  uint8_t* siValid;
  float *siM, *siR;
  EncAct si;
  GradBufs gsi;
  // move_first_image_feature (model.py:451-457): U = D + enc[:, 0], H, LN output
  void *mfU, *mfH, *mfV, *mfOut, *mfGA, *mfGH, *mfGU;
  float *mfM, *mfR;
};

struct GenWS {
  int R = 0, N = 0;  // capacity (rows, regions)
  void *x, *x1, *x2, *q, *att, *tmp, *h, *E;
  float *mean, *rstd, *Pc, *logits;
  float2* dstats;         // bf16 decode: classifier slab stats [R][ceil(V/16)] (GemmArgs::dec_stats)
  float* cand_v;          // beam: each row's k finalists (beam_step's two-launch forms)
  int32_t* cand_i;
  void* cache;            // [Ld][R][Tcap][2d]: row r's K/V of position t at [l][r][t]
  int32_t *ids, *ids2;    // [R][Tcap]
  int32_t *kvrow, *kvrow2;  // beam: [R][Tcap] row holding the K/V of (beam row, position)
  int64_t *seq, *seq2;   // beam [R][Tw]
  float *bprob, *bprob2;
  int32_t *bsrc, *btok;
  int32_t *bfin, *bfin2, *blen, *blen2;  // beam_nbest: [R] finished flag and length of each hypothesis
  // beam_forced: [R] met masks, and its own finalist scratch (each row's kf <= 16 finalists and W <= 14 word scores)
  int32_t *bmet, *bmet2;
  float* fcand_v;   // [R][32]
  int32_t* fcand_i;  // [R][16]
};

// Ensemble decoding: a capgen_ensemble after its checks.  m[0] leads: the call runs on its stream, over its
// hypotheses, selection state, decode constraints and outputs; the others only run their decoder steps.
struct EnsembleRun {
  std::vector<capgen_engine*> m;
  float log_w[8];  // log of the weights, normalised in double to sum 1
  int mode;        // CAPGEN_ENS_PROB / CAPGEN_ENS_LOGPROB
};

}  // namespace capgen

using namespace capgen;

struct capgen_engine {
  // ==== state ============================================================================
  capgen_config cfg;
  Layout L;
  int device = 0;
  DType act = DType::BF16;
  bool training = true;

  // ---- streams / events
  hipStream_t es = nullptr;   // engine stream (critical path)
  hipStream_t es2 = nullptr;  // side stream: weight-gradient GEMMs
  hipStream_t ec = nullptr;   // bucket stream: per-bucket gradient all-reduce (RCCL) + Adam
  hipEvent_t ev_in = nullptr, ev_out = nullptr, ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_b1 = nullptr, ev_b2 = nullptr, ev_cj = nullptr;
  hipEvent_t ev_ff = nullptr, ev_fj = nullptr;  // forward: decoder front forked to / joined from es2

  // ---- arenas
  float *params = nullptr, *grads = nullptr, *am = nullptr, *av = nullptr;
  bf16* shadow = nullptr;
  float* pe = nullptr;  // [max_length-1, dd] f32 sinusoid table
  uint64_t* seed = nullptr;
  float* scalars = nullptr;  // internal loss

  // ---- weight tiles
  // the fused attention fronts' weights (every self-attention Wqkv, every cross Wq) in the tiled
  // layout of qkv_tile_weights, re-tiled from the shadow wherever the shadow is written
  bf16* wtile = nullptr;
  // arena offset -> (element offset in wtile, rows); rows < 0: an output projection Wo [512][512]
  // kept as the tiled Wo^T (the fused attention backward's dO = dA . Wo[:, head], qkv_attn_bwd)
  std::map<int64_t, std::pair<int64_t, int>> tiled;
  // the weight version: bumped at every enqueued change of the bf16 shadow (each one is followed by
  // retile), so the decode tiles are rebuilt only when the weights moved
  uint64_t wver = 1, dtiles_ver = 0;
  // bf16 decode: the decoder Linears as MFMA fragment pieces for the register-B GEMM (gemm_breg.hip,
  // CAPGEN_BREG_DECODE, default on).  Wqkv / Wq_c are the fronts' tiles (the same layout at K = 512);
  // the others (Wo_s, Wo_c, W1, W2, the word-embedding projection) are rebuilt from the bf16 shadow at
  // the start of every greedy / beam call -- ~30 MB at C4, the weights may have moved since the last one
  bf16* dtiles = nullptr;
  std::map<int64_t, int64_t> dtile;  // arena offset -> element offset in dtiles
  bf16* emb_bf = nullptr;  // bf16 decode: the word-embedding table, read by the Wel GEMM through the ids
  bool dtiles_init = false;  // set once: a model whose Linears fit no tile shape allocates nothing, once

  // ---- optimizer control and gradient norm
  int64_t* step = nullptr;
  float* adam_scal = nullptr;
  // run-time optimizer control (capgen_set_lr / capgen_set_grad_clip).  opt: device words {lr, max_norm,
  // norm, coef} -- the Adam prep reads the learning rate, the norm finish reads max_norm and writes
  // {norm, coef}, the clipped Adam reads coef -- so a captured step sees new values without re-capture.
  // opt_host: the pinned staging words {lr, max_norm} of the setters' ordered async copies on es;
  // ev_opt: recorded after such a copy (the next setter waits for it before it overwrites the staging
  // word, and the bucket stream, which runs the Adam prep, waits for it on the device)
  float* opt = nullptr;
  float* opt_host = nullptr;
  hipEvent_t ev_opt = nullptr;
  float lr_cur = 0.f;
  float clip_cur = 0.f;  // 0: clipping off (the default schedule); > 0 clips, +inf measures only
  bool norm_valid = false;  // opt[2] holds the norm of an update issued with clip_on()
  // decoupled weight decay and the averaged weights (capgen_set_weight_decay / capgen_set_ema), both off
  // by default.  Two more device words beside the four above, set through set_opt_word like them:
  // opt[4] = wd (the Adam prep derives adam_scal[2] = 1 - lr * wd from it), opt[5] = 1 - decay (read by
  // the update kernel).  ema: the average's arena, L.total f32, allocated at the first enable.
  static constexpr int kOptWd = 4, kOptEmaRate = 5;
  float wd_cur = 0.f;
  float* ema = nullptr;
  float ema_decay = 0.f;     // 0: off
  int64_t ema_updates = 0;   // updates issued while on (a graph replay counts, its capture does not)
  bool ema_swapped = false;  // params holds the average and ema the raw weights (ema_swap)
  // the norm's partial sums: gn_part[gn_slots_cap] doubles, one slot per sum-of-squares workgroup, filled
  // in issue order within a step (gn_slots: used so far), and the step's total (all-reduced under DP)
  double* gn_part = nullptr;
  double* gn_sum = nullptr;
  int gn_slots_cap = 0, gn_slots = 0;
  struct DeferredAdam {
    int64_t off, n;
    int grid_cap;
  };
  std::vector<DeferredAdam> gn_deferred;  // buckets whose Adam waits for the step's clip coefficient
  // Adam grid of the step's last buckets (embedding, encoder LN/biases), which sit between the
  // backward's end and the next forward: the common cap (0).  The whole chip for them measured
  // slower (4-round A/B: 3.012 vs 2.982 ms/step with 2048 vs 256 workgroups)
  static constexpr int tail_grid = 0;

  // ---- stripes
  // striped partial sums for the small accumulated gradients (LayerNorm gamma/beta, biases):
  // [NSTRIPE][total - enc_lng]; folded into the gradient arena by stripe_reduce
  static constexpr int NSTRIPE = 16;
  float* gstripe = nullptr;
  bool stripes_dirty = true;  // gstripe may hold partials (the next backward zeroes it first)
  int64_t n_small = 0;

  // ---- workspaces
  Acts a;
  void* ws = nullptr;
  GenWS g;
  void* gws = nullptr;

  // ---- graphs and keys
  // graph: off by default.  Measured on MI355X / ROCm 7 (tools/launch_probe.py): a replay of
  // the three-stream step graph costs ~3 ms of host time and runs ~0.7 ms SLOWER on the GPU
  // than the same kernels issued eagerly on three streams (4.3 vs 5.0 ms at C2); a
  // single-stream graph launches in 0.1 ms but loses the stream overlap (5.5 ms).
  bool graph_on = false;
  hipGraphExec_t gexec = nullptr;
  hipGraphExec_t fexec = nullptr;  // eager step mode: the forward alone as a linear graph (fwd_graph_mode)
  struct Key {
    const void *f, *p, *c;
    float* loss;
    int ft, B, N, T;
    bool drop;
    StepIn in;
    bool operator==(const Key& o) const {
      return f == o.f && p == o.p && c == o.c && loss == o.loss && ft == o.ft && B == o.B && N == o.N && T == o.T &&
             drop == o.drop && in == o.in;
    }
  } gkey{}, fkey{};
  std::vector<std::array<int, 3>> tuned_shapes;  // (B, N, T) whose GEMM shapes tune_once has run

  // ---- data parallel / ZeRO
  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  float* count_host = nullptr;  // pinned: global count override
  hipEvent_t ev_count = nullptr;  // recorded after the copy of count_host (host writes wait for it)
  bool count_override = false;
  int zemu_rank = 0, zemu_world = 1;  // capgen_dp_debug_shard: shard as rank r of w, no collectives
  // set by the sharded update (zero_mode): the Adam moments (resp. the gradient arena) are current in this
  // rank's chunks only until capgen_dp_sync_adam_state (resp. the next backward) -- the whole-arena getters
  // refuse them in between instead of returning stale data
  bool moments_sharded = false, grads_sharded = false;
  bool ema_sharded = false;  // the same for the average (updated while on by a sharded step)
  // what the captured whole-step graph's host code set of the two flags above: a replay runs no host
  // code, so train_step sets them (and ema_sharded) again where it launches the graph
  bool gexec_moments_sharded = false, gexec_grads_sharded = false;
  std::vector<std::array<int64_t, 2>> zbuckets;  // this step's bucket ranges, in issue order
  bool zbuckets_checked = false;
  bool dp_checked = false;  // dp_check has run
  float* dp_chk = nullptr;  // [4] device scratch: count max, count min, loss max, loss min

  // ---- decode state and constraints
  // decode scoring: false = Softmax, probabilities accumulated over beams (Transformer,
  // model.py:124-128,183); true = LogSoftmax, log-probabilities (PolicyNetwork, model_RL.py:72,182)
  bool decode_logsm = false;
  // decode constraints of beam_nbest and sample (select.hip; capgen_set_decode_constraints): off by default
  DecodeConstraints dc;
  int32_t* dc_banned = nullptr;  // the device copy of the banned list dc.banned points to (1024 entries)
  static constexpr uint32_t kSampleSite0 = 0x5A00;  // sample(): position t draws at site kSampleSite0 + t

  // ---- stamps
  // diagnostic in-kernel timestamps (capgen_debug_stamps): every GEMM / LayerNorm / attention
  // launch of a step gets a slot of the ring (forward slots first: a captured forward graph keeps
  // its slots, the backward re-numbers from where the forward ended); names for the report
  bool stamp_on = false;
  uint64_t* stamp_ring = nullptr;
  static constexpr int kStampSlots = 4096;
  int stamp_next = 0, stamp_fwd_end = 0, stamp_max = 0;
  std::vector<std::string> stamp_names;

  // ---- logs
  // the RCCL collectives issued (capgen_debug_collectives: every rank must issue the same sequence, or
  // the job hangs)
  bool coll_log_on = false;
  std::vector<std::string> coll_log;
  // CAPGEN_HOST_TIMING=1 (debug build): the mean host time of a step's two halves, every 20 steps
  using host_clock = std::chrono::steady_clock;
  double ht_fwd = 0, ht_bwd = 0;
  int ht_steps = 0;

  // ---- per-call state
  int fB = 0, fN = 0, fT = 0;  // shape of the last forward
  bool fwd_drop = true;        // dropout state of the last forward (backward must match)
  float* pending_loss = nullptr;    // set by train_step: the backward finalises the loss into it on es2
  const float* last_loss = nullptr;  // the loss buffer the last forward wrote (dp_check reads it)
  bool bstep = false;         // backward(): the bucketed parameter update runs with it (train_step)
  bool dec0_on_side = false;  // backward(): decoder block 0 was issued on es2 (overlap_dec0)
  int rl_B = 0;               // batch of the rl_sample that rl_finish completes (0: none)
  hipStream_t crit = nullptr;  // critical stream of the running call (es, or the caller's: direct)
  bool need_logits = false;  // the next forward must materialise the f32 logits (SCST sampling)
  StepIn in;
  // Weight-gradient GEMMs are queued and issued on es2 in one batch per block (flush): an event
  // record/wait pair costs the recording stream ~7 us of bubble on ROCm 7 (tools/kprobe.hip:
  // 13 us per eager fork/join pair), so the critical stream records one event per block instead
  // of one per weight.  Every buffer a queued dW reads is per block (or never rewritten in the
  // backward pass), so issuing it later is hazard-free.
  struct DwJob {
    const void *dY, *X;
    int64_t ldy, ldx, goff, ldg;
    int M, N, K;
    const float* alpha_ptr;
  };
  std::vector<DwJob> dw_pending;
  // FFN bias gradients (column sums of the ReLU'-masked hidden gradient) queued like the weight
  // gradients: off the critical stream instead of as atomics in the dX GEMM's epilogue (colsum_side)
  struct ColJob {
    const void* X;
    int M, N;
    float* db;
  };
  std::vector<ColJob> col_pending;

  // ==== the switches frozen at creation (knobs.cpp) =======================================
  // CAPGEN_BREG_DECODE: the register-B GEMM in bf16 decode (dtiles above)
  bool breg_decode_on = knob(Knob::BregDecode) != 0;
  // CAPGEN_CLIP_ADAM_GRID: Adam grid of the deferred buckets (0: the bucket's own cap).  They sit on the
  // step's tail with nothing left to run beside, so they take the whole chip: 2.944 vs 2.975 ms per C2
  // step with 2048 vs 256 workgroups, 1024 and 4096 level with 2048 (2.692 with clipping off;
  // profiles/r09_gradclip.txt)
  int clip_adam_grid = knob(Knob::ClipAdamGrid);
  // CAPGEN_STRIPE_CLEAR: the folds zero the partials they read (0: memset per step)
  bool stripe_clear = knob(Knob::StripeClear) != 0;
  // CAPGEN_FWD_GRAPH: eager step mode runs the forward alone as a linear graph (0 disables)
  // (1: at world size 1 -- its RCCL count / CE all-reduces, if any, capture into the graph; at world > 1
  // the forward is issued eagerly, the collectives as plain stream calls: the multi-rank path keeps
  // RCCL's standard usage, and eager vs graph measured level on the GPU; 2: the graph at any world size)
  int fwd_graph_mode = knob(Knob::FwdGraph);
  bool fwd_graph_on = fwd_graph_mode != 0;
  // CAPGEN_ZERO: sharded update (ZeRO-1, SURVEY §8(e) "later"): with world > 1 each bucket's gradients are
  // reduce-scattered, each rank runs Adam on its 1/world chunk only (its chunk of the moments is
  // the only one it keeps current), the updated f32 chunk is all-gathered in place and the bf16
  // shadow of the bucket re-cast locally.  Same bytes over xGMI as the all-reduce (RS + AG), 1/world
  // of the 1.67 GB Adam stream.  CAPGEN_ZERO=0: all-reduce + full Adam on every rank;
  // CAPGEN_ZERO=2: the sharded code path even at world 1 (RCCL test hook).
  int zero_mode = knob(Knob::Zero);
  // CAPGEN_FUSED_CE: fused classifier + cross entropy in the bf16 path (0: logits in f32 + ce_kernel)
  bool fused_ce_on = knob(Knob::FusedCe) != 0;
  // CAPGEN_DEFER_LOSS: the loss finalisation leaves the critical stream (loss_deferrable below)
  bool defer_loss_on = knob(Knob::DeferLoss) != 0;
  // CAPGEN_FRONT_JOIN: encoder block before which the forward joins the decoder front
  int front_join = knob(Knob::FrontJoin);
  // CAPGEN_FUSED_QKV: the self-attention front of a block as ONE fused launch (self_attention;
  // 0: the projection GEMM and the attention launch)
  bool fused_qkv_on = knob(Knob::FusedQkv) != 0;
  // CAPGEN_DEBUG_DROP_JOIN=1 (debug build only), hazard-checker self-test: the side stream is never
  // joined back -- a deliberately missing edge the checker must report (results are then racy: test use only)
  bool dbg_drop_join = knob(Knob::DebugDropJoin) == 1;
  // CAPGEN_GROUP_DW: the weight gradients of a block as grouped launches (0: one launch per weight, tests)
  bool group_dw = knob(Knob::GroupDw) != 0;
  // CAPGEN_COLSUM_SIDE: the FFN bias column sums on es2 (0 restores the dX GEMM's epilogue form)
  bool colsum_side = knob(Knob::ColsumSide) != 0;
  // CAPGEN_OVERLAP_FRONT: the decoder front on es2 beside the encoder (0: it runs after the encoder)
  bool overlap_front = knob(Knob::OverlapFront) != 0;
  // CAPGEN_OVERLAP_DEC0: decoder block 0's self-attention half (and the decoder-embedding branch) on es2,
  // concurrent with the encoder chain: once block 0's cross-attention backward has produced its K/V
  // gradient, the encoder-output gradient (all blocks' gKV . Wkv_all) is complete, and nothing
  // the encoder backward reads depends on the rest of block 0 (0: serial)
  bool overlap_dec0 = knob(Knob::OverlapDec0) != 0;
  // CAPGEN_FUSED_ATTN_BWD: the output projection's input gradient inside the attention backward launch
  // (mha_bwd; 0: the dX GEMM into gATT and the attention backward launch)
  bool fused_attn_bwd_on = knob(Knob::FusedAttnBwd) != 0;
  // CAPGEN_BUCKET_BLOCKS: transformer blocks per gradient bucket (one flush = one event record on the
  // critical stream)
  int bucket_blocks = std::max(1, knob(Knob::BucketBlocks));
  // CAPGEN_DECODE_LN_FOLD: the decoder LayerNorms of a decode step inside the GEMM that reads them
  // (ln_fold, dec_step).  Every site below 1024 rows (greedy's 256; 2: at any row count); at beam-5's
  // 1280 rows only the cross-query site: folding the QKV / FFN-up sites too replaces their 64 x 64
  // register-B tiles and measured slower (13.56-13.57 vs 12.82-12.84 ms per batch).  0: separate launches
  int decode_ln_fold = knob(Knob::DecodeLnFold);
  // CAPGEN_DECODE_CROSS_MFMA: bf16 beam decode runs the cross attention of an image's beam rows on the
  // MFMA attention kernel (0: the grouped VALU decode kernel, attention.hip)
  bool cross_mfma_on = knob(Knob::DecodeCrossMfma) != 0;
  // CAPGEN_FUSED_BEAM_STEP: bf16 beam selection and reorder of a step as one launch per image
  // (beam_step with a reorder; 0 restores the top-k, merge and three reorder launches)
  bool fused_beam_step_on = knob(Knob::FusedBeamStep) != 0;
  // CAPGEN_SLAB_DECODE: bf16 decode: the classifier epilogue writes slab stats and the greedy / beam
  // selection reads k * 16 logits per row instead of the whole row (0: full-row kernels)
  bool slab_decode_on = knob(Knob::SlabDecode) != 0;
  // (CAPGEN_STREAMS and CAPGEN_EVENT_FENCE are read once, by the constructor; CAPGEN_HOST_TIMING by
  // host_timing)

  // ==== inline: small, and called per launch =============================================
  const bf16* WT(int64_t woff) const {
    auto it = tiled.find(woff);
    return it == tiled.end() || it->second.second < 0 ? nullptr : wtile + it->second.first;
  }
  const bf16* WTo(int64_t woff) const {
    auto it = tiled.find(woff);
    return it == tiled.end() || it->second.second > 0 ? nullptr : wtile + it->second.first;
  }
  bool breg_decode() const { return breg_decode_on && act == DType::BF16; }
  const void* DT(int64_t off) const {
    if (!breg_decode()) return nullptr;
    if (const bf16* t = WT(off)) return t;
    auto it = dtile.find(off);
    return it == dtile.end() || !dtiles ? nullptr : dtiles + it->second;
  }
  bool clip_on() const { return clip_cur != 0.f; }
  bool wd_on() const { return wd_cur != 0.f; }
  bool ema_on() const { return ema_decay != 0.f; }
  // the optional parts of an update of the arena range starting at off (none by default)
  AdamOpt adam_opt(int64_t off) const {
    return {wd_on() ? adam_scal + 2 : nullptr, ema_on() ? ema + off : nullptr, opt + kOptEmaRate};
  }
  const float* wd_word() const { return wd_on() ? opt + kOptWd : nullptr; }
  // the calls that update parameters refuse to run on the averaged weights
  void require_unswapped(const char* what) const {
    require(!ema_swapped, std::string(what) + ": the averaged weights are swapped into the parameters; call "
                                              "capgen_ema_swap to swap them back first");
  }
  bool tuned(int B, int N, int T) const {
    for (auto& t : tuned_shapes)
      if (t[0] == B && t[1] == N && t[2] == T) return true;
    return false;
  }
  int zworld() const {
    if (zemu_world > 1) return zemu_world;
    if (!comm || zero_mode == 0) return 1;
    return world > 1 || zero_mode == 2 ? world : 1;
  }
  int zrank() const { return zemu_world > 1 ? zemu_rank : rank; }
  bool zsharded() const { return zemu_world > 1 || (comm && (world > 1 ? zero_mode != 0 : zero_mode == 2)); }
  const void* W(int64_t off) const {
    return act == DType::BF16 ? (const void*)(shadow + off) : (const void*)(params + off);
  }
  const float* P(int64_t off) const { return params + off; }
  float* G(int64_t off) const { return grads + off; }
  float* GS(int64_t off) const { return gstripe + (off - L.enc_lng); }  // striped small-gradient slot
  size_t es_() const { return dsize(act); }
  void* at(void* base, int64_t elems) const { return (char*)base + elems * es_(); }
  Drop mk_drop(float p, uint32_t site, bool on) const {
    Drop d{};
    if (!on || p <= 0.f) return d;
    d.seed_ptr = seed;
    d.site = site;
    d.thresh = drop_threshold(p);
    d.scale = 1.f / (1.f - p);
    return d;
  }
  // the f32 VALU attention backward reads the saved probabilities; the bf16 MFMA one recomputes
  bool keep_probs(const AttnGeom& g) const { return !(act == DType::BF16 && attention_mfma_ok(g)); }
  // a dropout site = (encoder 0 / decoder 1, layer, kind): the hash input that makes its mask.  The
  // values are part of the results (golden fixtures, bit-identity tests): never renumber
  enum DropKind {
    kDropEncAttn = 0, kDropEncMha = 1, kDropEncFfn = 2,
    kDropDecSelfAttn = 3, kDropDecSelf = 4, kDropDecCrossAttn = 5, kDropDecCross = 6, kDropDecFfn = 7,
    kDropMoveFirst = 0,  // (decoder, kMfLayer)
  };
  static constexpr int kImgLayer = 63;  // dropout-site layer index of encoder.image_encoder
  static constexpr int kMfLayer = 62;   // dropout-site layer index of the decoder's move-first FFN
  static uint32_t site(int dec, int layer, DropKind kind) { return (uint32_t)((dec * 64 + layer) * 16 + kind); }
  // ---- the attention sites: the complete geometry (masks and dropout included) of each, built
  // here for the forward and the backward alike (the bf16 MFMA backward recomputes the probabilities)
  // encoder self-attention of B sequences of N rows (the image block: B = Me pairs of N = 2)
  AttnGeom enc_self_geom(const EncAct& A, int B, int N, const uint8_t* valid, int layer, bool on) const {
    const int d = L.d;
    AttnGeom g = attn_dense(B, L.He, N, N, d / L.He, A.qkv, 3 * d, at(A.qkv, d), 3 * d, at(A.qkv, 2 * d), 3 * d, d);
    if (valid) g.key_valid = valid, g.kv_bs = N, g.causal = 1;
    g.drop = mk_drop(cfg.attention_dropout, site(0, layer, kDropEncAttn), on);
    return g;
  }
  // decoder self-attention: key-pad(ids) OR causal (model.py:421-430)
  AttnGeom dec_self_geom(int l, int B, int Lq, bool on) const {
    const int dd = L.dd;
    void* qkv = a.dec[l].qkv;
    AttnGeom g = attn_dense(B, L.Hd, Lq, Lq, dd / L.Hd, qkv, 3 * dd, at(qkv, dd), 3 * dd, at(qkv, 2 * dd), 3 * dd, dd);
    g.key_ids = a.ids, g.kid_bs = Lq, g.pad_idx = cfg.pad_idx, g.causal = 1;
    g.drop = mk_drop(cfg.attention_dropout, site(1, l, kDropDecSelfAttn), on);
    return g;
  }
  // the K/V half of decoder block l's cross-attention: its columns of a.KV (every block's K | V side
  // by side per encoder row), N regions per image, context mask = region key-pad (model.py:82).
  // The caller sets B, Lq and the q / o layouts.
  AttnGeom cross_kv(int l, int N) const {
    const int dd = L.dd;
    const int64_t kvld = (int64_t)L.Ld * 2 * dd;
    AttnGeom c = attn_dense(0, L.Hd, 0, N, dd / L.Hd, nullptr, 0, at(a.KV, (int64_t)l * 2 * dd), kvld,
                            at(a.KV, (int64_t)l * 2 * dd + dd), kvld, 0);
    c.key_valid = a.valid, c.kv_bs = N;
    return c;
  }
  // decoder cross-attention at the training shape
  AttnGeom dec_cross_geom(int l, int B, int Lq, int N, bool on) const {
    const int dd = L.dd;
    AttnGeom c = cross_kv(l, N);
    c.B = B, c.Lq = Lq;
    c.q = a.dec[l].qc, c.q_ld = dd, c.q_bs = (int64_t)Lq * dd;
    c.o_ld = dd, c.o_bs = (int64_t)Lq * dd;
    c.drop = mk_drop(cfg.attention_dropout, site(1, l, kDropDecCrossAttn), on);
    return c;
  }
  // ---- the LayerNorm sites (model.py:86-90, 114-120), each described once for both directions
  LnSite enc_embed_site(int Me) const {  // the shared norm after the region embedding (model.py:294)
    return {Me, L.d, a.ev0, a.em0, a.er0, L.enc_lng, L.enc_lnb, -1, RowMask{}, Drop{}};
  }
  LnSite img_norm2_site(int Me) const {  // the shared norm again, after the image block
    return {Me, L.d, a.siV, a.siM, a.siR, L.enc_lng, L.enc_lnb, -1, RowMask{}, Drop{}};
  }
  LnSite enc_ln1_site(const EncLayerOff& w, const EncAct& A, int Me, int layer, bool on) const {
    return {Me, L.d, A.v1, A.m1, A.r1, w.ln1g, w.ln1b, -1, RowMask{}, mk_drop(cfg.dropout, site(0, layer, kDropEncMha), on)};
  }
  LnSite enc_ln2_site(const EncLayerOff& w, const EncAct& A, int Me, const uint8_t* valid, int layer, bool on) const {
    RowMask mask{};
    mask.valid = valid;
    return {Me, L.d, A.v2, A.m2, A.r2, w.ln2g, w.ln2b, w.b2, mask, mk_drop(cfg.dropout, site(0, layer, kDropEncFfn), on)};
  }
  LnSite dec_embed_site(int Md) const {  // LN(E.Wel^T + PE) (model.py:432-436): no residual, no dropout
    return {Md, L.dd, a.dv0, a.dm0, a.dr0, L.dec_lng, L.dec_lnb, -1, RowMask{}, Drop{}};
  }
  LnSite dec_self_site(int l, int Md, bool on) const {
    const auto& A = a.dec[l];
    const auto& w = L.dec[l];
    return {Md, L.dd, A.vs, A.ms, A.rs, w.lsg, w.lsb, -1, RowMask{}, mk_drop(cfg.dropout, site(1, l, kDropDecSelf), on)};
  }
  LnSite dec_cross_site(int l, int Md, bool on) const {
    const auto& A = a.dec[l];
    const auto& w = L.dec[l];
    return {Md, L.dd, A.vc, A.mc, A.rc, w.lcg, w.lcb, -1, RowMask{}, mk_drop(cfg.dropout, site(1, l, kDropDecCross), on)};
  }
  LnSite dec_ffn_site(int l, int Md, bool on) const {  // x non_pad (modules.py:201-204)
    const auto& A = a.dec[l];
    const auto& w = L.dec[l];
    RowMask mask{};
    mask.ids = a.ids, mask.pad_idx = cfg.pad_idx;
    return {Md, L.dd, A.vf, A.mf, A.rf, w.lfg, w.lfb, w.b2, mask, mk_drop(cfg.dropout, site(1, l, kDropDecFfn), on)};
  }
  LnSite move_first_site(int M, bool on) const {
    return {M, L.dd, a.mfV, a.mfM, a.mfR, L.mf_lng, L.mf_lnb, L.mf_b2, RowMask{},
            mk_drop(cfg.dropout, site(1, kMfLayer, kDropMoveFirst), on)};
  }
  // y = LayerNorm(drop(a + bias) + res); keep = false (decoding): nothing is saved for a backward
  LnFwd ln_fwd(const LnSite& s, const void* a_in, const void* res, void* y, bool keep = true) const {
    LnFwd f;
    f.M = s.M, f.d = s.d, f.a = a_in, f.a_bias = s.bias >= 0 ? P(s.bias) : nullptr, f.drop = s.drop, f.res = res;
    f.gamma = P(s.g), f.beta = P(s.b), f.mask = s.mask, f.y = y;
    if (keep) f.v_save = s.v, f.mean = s.mean, f.rstd = s.rstd;
    return f;
  }
  // its backward (striped accumulators): d_res = grad wrt the residual, d_a = grad wrt a
  LnBwd ln_bwd(const LnSite& s, const void* dy, void* d_res, void* d_a) const {
    LnBwd lb;
    lb.M = s.M, lb.d = s.d, lb.dy = dy, lb.v = s.v, lb.mean = s.mean, lb.rstd = s.rstd, lb.gamma = P(s.g);
    lb.mask = s.mask, lb.drop = s.drop, lb.d_res = d_res, lb.d_a = d_a;
    lb.dgamma = GS(s.g), lb.dbeta = GS(s.b), lb.dbias = s.bias >= 0 ? GS(s.bias) : nullptr;
    lb.stripes = NSTRIPE, lb.stripe_stride = n_small;
    return lb;
  }
  // issue priority of a launch: kernels on the critical stream run their waves at s_setprio 3 so
  // that the weight-gradient / Adam waves of the side streams sharing their CUs yield the issue
  // slots to them (measured 2.779 / 2.788 vs 2.782 / 2.795 ms/step without, round 4)
  int prio(hipStream_t s) const { return s == (crit ? crit : es) && es2 != s ? 1 : 0; }
  bool fused_ce() const { return fused_ce_on && !need_logits && act == DType::BF16 && L_().V % 4 == 0; }
  // train step without a collective or FocalLoss: the CE gradient scale 1/count comes from the caption
  // prep (the count is known there), so the loss finalisation (the mean of the loss rows) leaves the
  // critical stream: the step's forward skips it and its backward issues it on es2 after the first
  // fork (pending_loss).  With a count all-reduce or FocalLoss the scale needs the finalisation first.
  bool loss_deferrable() const { return !comm && !count_override && !cfg.focal_loss && defer_loss_on; }
  uint64_t* stamp(hipStream_t s, const std::string& what) {
    if (!stamp_on || !stamp_ring || stamp_next >= kStampSlots) return nullptr;
    const int i = stamp_next++;
    stamp_max = std::max(stamp_max, stamp_next);
    if ((int)stamp_names.size() <= i) stamp_names.resize(i + 1);
    stamp_names[i] = std::string(s == ec && ec != es2 ? "bucket " : s == es2 && es2 != (crit ? crit : es) ? "side " : "crit ") + what;
    return stamp_ring + (size_t)i * 16;
  }
  static std::string dims(int M, int N, int K) {
    return std::to_string(M) + "x" + std::to_string(N) + "x" + std::to_string(K);
  }
  // the row / attention kernels with the launch's issue priority (prio above)
  void lnf(LnFwd l, hipStream_t s) {
    l.prio = prio(s);
    if (stamp_on) l.stamp = stamp(s, "ln_fwd " + std::to_string(l.M));
    layernorm_fwd(l, act, s);
  }
  void lnb(LnBwd l, hipStream_t s) {
    l.prio = prio(s);
    if (stamp_on) l.stamp = stamp(s, "ln_bwd " + std::to_string(l.M));
    layernorm_bwd(l, act, s);
  }
  void attf(AttnGeom g, void* o, float* probs, DType t, hipStream_t s) {
    g.prio = prio(s);
    if (stamp_on) g.stamp = stamp(s, "attn_fwd " + std::to_string(g.Lq) + "x" + std::to_string(g.Lk));
    attention_fwd(g, o, probs, t, s);
  }
  void attb(AttnGeom g, const float* probs, const void* dout, void* dq, void* dk, void* dv, DType t,
            hipStream_t s) {
    g.prio = prio(s);
    if (stamp_on) g.stamp = stamp(s, "attn_bwd " + std::to_string(g.Lq) + "x" + std::to_string(g.Lk));
    attention_bwd(g, probs, dout, dq, dk, dv, t, s);
  }
  bool cross_fusable(int Lq) const {
    return fused_qkv_on && act == DType::BF16 && wtile && L.dd == 512 && L.Hd * 64 == L.dd && Lq >= 1 && Lq <= 64;
  }
  // C[M,N] = A[M,K] . W[N,K]^T  (nn.Linear)
  // bt: the weight's fragment pieces (DT), read by the register-B GEMM where it takes the shape
  void linear(const void* X, int64_t ldx, int64_t woff, int64_t ldw, void* C, int64_t ldc, DType tout, int M,
              int N, int K, const float* bias, int relu, hipStream_t s, const void* bt = nullptr) {
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = X, ga.lda = ldx, ga.B = W(woff), ga.ldb = ldw, ga.C = C, ga.ldc = ldc;
    ga.bt = bt;
    ga.bias = bias;
    ga.relu = relu;
    ga.prio = prio(s);
    if (stamp_on) ga.stamp = stamp(s, "gemm fwd " + dims(M, N, K));
    gemm(ga, act, tout, false, false, s);
  }
  // C = X . W^T into ln.a, then y = LayerNorm(drop(C + bias) + res (+ pe)) (modules.py:86-90).
  // (Fusing the LayerNorm into the GEMM -- a row-block finisher reloading the rows write-through
  // -- was measured slower than this separate launch: DESIGN.md section 6.)
  void linear_ln(const void* X, int64_t ldx, int64_t woff, int64_t ldw, int M, int N, int K, const LnFwd& ln,
                 hipStream_t s) {
    linear(X, ldx, woff, ldw, const_cast<void*>(ln.a), N, act, M, N, K, nullptr, 0, s);
    lnf(ln, s);
  }
  // dX[M,K] (+)= alpha * dY[M,N] . W[N,K]
  void linear_dx(const void* dY, int64_t ldy, int64_t woff, int64_t ldw, void* dX, int64_t ldx, int M, int N, int K,
                 int beta, const void* relu_aux, const float* alpha_ptr, hipStream_t s, float* colsum = nullptr) {
    GemmArgs ga;
    ga.colsum = colsum;
    ga.colsum_stripes = NSTRIPE, ga.colsum_stride = n_small;  // colsum always targets gstripe
    ga.M = M, ga.N = K, ga.K = N, ga.A = dY, ga.lda = ldy, ga.B = W(woff), ga.ldb = ldw, ga.C = dX, ga.ldc = ldx;
    ga.beta = beta;
    ga.aux = relu_aux;
    ga.ldaux = ldx;
    ga.alpha_ptr = alpha_ptr;
    ga.prio = prio(s);
    if (stamp_on) ga.stamp = stamp(s, "gemm dX " + dims(M, K, N));
    gemm(ga, act, act, false, true, s);
  }
  // dW[N,K] = alpha * dY[M,N]^T . X[M,K]   (f32, overwrites)
  void linear_dw(const void* dY, int64_t ldy, const void* X, int64_t ldx, int64_t goff, int64_t ldg, int M, int N,
                 int K, const float* alpha_ptr, hipStream_t s) {
    GemmArgs ga;
    ga.M = N, ga.N = K, ga.K = M, ga.A = dY, ga.lda = ldy, ga.B = X, ga.ldb = ldx, ga.C = G(goff), ga.ldc = ldg;
    ga.alpha_ptr = alpha_ptr;
    ga.prio = prio(s);
    if (stamp_on) ga.stamp = stamp(s, "gemm dW " + dims(N, K, M));
    gemm(ga, act, DType::F32, true, true, s);
  }
  const Layout& L_() const { return L; }
  // (re)allocate a workspace block: plan(p) lays its buffers out on p, once without a base for the size
  // and once over the new block for the pointers
  template <class F>
  void replan(void*& block, F&& plan) {
    if (block) {
      hz::host_sync(es);
      CAPGEN_HIP(hipFree(block));
      block = nullptr;
    }
    Planner p;
    plan(p);
    CAPGEN_HIP(hipMalloc(&block, p.used));
    Planner q;
    q.base = (char*)block;
    plan(q);
  }
  // body() captured on s into an instantiated graph (the capture is ended, and the graph object
  // destroyed, whether or not body throws)
  template <class F>
  hipGraphExec_t capture(hipStream_t s, F&& body) {
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    CAPGEN_HIP(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    try {
      body();
    } catch (...) {
      (void)hipStreamEndCapture(s, &graph);
      if (graph) (void)hipGraphDestroy(graph);
      throw;
    }
    CAPGEN_HIP(hipStreamEndCapture(s, &graph));
    const hipError_t inst = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    CAPGEN_HIP(inst);
    return exec;
  }
  // the decoder output the classifier reads
  void* dec_out() const { return L.has_mf ? a.mfOut : a.D[L.Ld]; }
  // weight-gradient GEMMs run on the side stream es2, forked from the main stream right after
  // their inputs are produced; backward() joins es2 back at the end (both in eager mode and
  // inside the captured graph, where this becomes a parallel branch)
  // `to` waits for everything issued so far on `from` (no-op when they are one stream)
  static void dep(hipStream_t from, hipStream_t to, hipEvent_t e) {
    if (from == to) return;
    hz::record(e, from);
    hz::wait(to, e);
  }
  static void memset_async(void* p, size_t bytes, hipStream_t s) {
    if (hz::active()) hz::op(s, "memset", {hz::wr(p, (int64_t)bytes)});
    CAPGEN_HIP(hipMemsetAsync(p, 0, bytes, s));
  }
  // an RCCL collective on s, in place over [p, p + bytes): hazard log + the collective log
  // (capgen_debug_collectives: every rank must issue the same sequence, or the job hangs)
  void nccl_op(hipStream_t s, const char* name, const void* p, int64_t bytes) {
    if (hz::g_log) hz::op(s, name, {hz::wr(p, bytes)});
    if (coll_log_on) {
      const char* role = s == ec ? "bucket" : s == es2 ? "side" : "critical";
      coll_log.push_back(std::string(name) + " " + std::to_string(bytes) + " B on " + role);
    }
  }
  void fork(hipStream_t s) { dep(s, es2, ev_fork); }
  void dw_side(const void* dY, int64_t ldy, const void* X, int64_t ldx, int64_t goff, int64_t ldg, int M, int N,
               int K, const float* alpha_ptr, hipStream_t s) {
    if (es2 == s) {
      linear_dw(dY, ldy, X, ldx, goff, ldg, M, N, K, alpha_ptr, s);
      return;
    }
    dw_pending.push_back(DwJob{dY, X, ldy, ldx, goff, ldg, M, N, K, alpha_ptr});
  }
  GemmArgs dw_args(const DwJob& j) const {
    GemmArgs ga;
    ga.M = j.N, ga.N = j.K, ga.K = j.M, ga.A = j.dY, ga.lda = j.ldy, ga.B = j.X, ga.ldb = j.ldx;
    ga.C = G(j.goff), ga.ldc = j.ldg, ga.alpha_ptr = j.alpha_ptr;
    return ga;
  }
  // GemmArgs of dX[M,K] (+)= dY[M,N] . W[N,K] (linear_dx) without launching it
  GemmArgs dx_args(const void* dY, int64_t ldy, int64_t woff, int64_t ldw, void* dX, int64_t ldx, int M, int N,
                   int K, int beta) const {
    GemmArgs ga;
    ga.M = M, ga.N = K, ga.K = N, ga.A = dY, ga.lda = ldy, ga.B = W(woff), ga.ldb = ldw, ga.C = dX, ga.ldc = ldx;
    ga.beta = beta;
    return ga;
  }
  // sharded update (ZeRO-1); buckets are 64-element aligned
  bool bucket_sharded(int64_t n) const { return zsharded() && n % (4 * zworld()) == 0; }
  int64_t enc_end(int l) const { return l + 1 < L.Le ? L.enc[l + 1].Wqkv : L.Wel; }
  int64_t dec_end(int l) const { return l + 1 < L.Ld ? L.dec[l + 1].Wqkv : L.Wkv_all; }
  // after a train step's forward (eager, captured or replayed): its deferred loss goes to `loss`
  void set_pending_loss(float* loss) {
    pending_loss = loss_deferrable() ? (loss ? loss : a.loss) : nullptr;
    if (pending_loss) last_loss = pending_loss;
  }
  // one decode Linear: C = X . W^T (+ bias) (ReLU), C's row stride ldc (0: N).  ln: X is the output of
  // that LayerNorm: its own launch in front of the GEMM, or (fold) the GEMM reads the LayerNorm's input
  // and residual, normalises the rows itself and stores them into X (= ln->y).  C2: the columns from
  // ldc on go to C2 (row stride ldc2)
  void dec_linear(const void* X, int64_t woff, int M, int N, int K, void* C, const float* bias, int relu,
                  hipStream_t s, const LnFwd* ln = nullptr, bool fold = false, int64_t ldc = 0, void* C2 = nullptr,
                  int64_t ldc2 = 0) {
    GemmArgs ga;
    ga.M = M, ga.N = N, ga.K = K, ga.A = X, ga.lda = K, ga.B = W(woff), ga.ldb = K, ga.C = C, ga.ldc = ldc ? ldc : N;
    ga.bt = DT(woff), ga.bias = bias, ga.relu = relu, ga.prio = prio(s);
    if (C2) ga.C2 = C2, ga.ldc2 = ldc2, ga.nsplit = (int)ldc;
    if (ln && fold) {
      ga.A = ln->a, ga.ln_res = ln->res, ga.ln_gamma = ln->gamma, ga.ln_beta = ln->beta, ga.ln_y = ln->y;
      if (ln->mask.ids) ga.ln_ids = ln->mask.ids, ga.ln_ids_ld = ln->mask.ids_ld, ga.ln_pad = ln->mask.pad_idx;
    } else if (ln) {
      lnf(*ln, s);
    }
    if (stamp_on) ga.stamp = stamp(s, std::string(ga.ln_gamma ? "gemm fwd+ln " : "gemm fwd ") + dims(M, N, K));
    gemm(ga, act, act, false, false, s);
  }
  bool slab_decode() const { return slab_decode_on && act == DType::BF16 && L.V % 4 == 0 && slab_select_ok(L.V); }

  // ==== out of line, by concern ==========================================================
  // (the comments stand with the definitions)
  capgen_engine(const capgen_config& c, int dev);  // engine_step.hip, beside the destructor
  capgen_engine(const capgen_config& c, int dev, DType t);  // (the fields alone: its delegation target)
  ~capgen_engine();
  // ---- engine_forward.hip
  void self_attention(const void* X, int64_t wqkv, int M, int d, const AttnGeom& g, void* qkv, void* att, float* probs,
                      hipStream_t s);
  void cross_attention(const AttnGeom& c, const void* D1, int64_t wq, int d, void* qc, void* attc, float* probs,
                       bool q_done, hipStream_t s);
  void plan_acts(Planner& p, int B, int N, int T);
  void ensure_acts(int B, int N, int T);
  void enc_layer_fwd(const EncLayerOff& w, EncAct& A, const void* X, void* Xout, int B, int N, const uint8_t* valid,
                     int layer, bool drop_on, hipStream_t s, bool keep = true);
  void enc_embed_fwd(int Me, bool keep, hipStream_t s);
  void image_objects_fwd(int B, int N, bool drop_on, hipStream_t s);
  void move_first_fwd(const void* x, const void* enc, int M, int rows_per_img, int bmod, int N, void* U, void* H,
                      void* tmp, void* y, bool keep, bool drop_on, hipStream_t s);
  void forward(const void* feats, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
               float* loss_out, bool drop_on, hipStream_t s, bool defer_loss = false);
  void copy_logits(float* dst, int64_t n, hipStream_t cs);
  void* debug_buffer(int which) const;
  // ---- engine_backward.hip
  void join(hipStream_t s);
  void dw_launch(const DwJob* jobs, size_t n, hipStream_t st);
  void flush(hipStream_t s);
  void ffn_bwd(int M, int d, int f, const LnBwd& lb, const void* X, const void* H, int64_t W1, int64_t b1, int64_t W2,
               void* gH, hipStream_t s);
  void mha_out_bwd(int M, int d, const LnBwd& lb, const void* att, int64_t Wo, void* gATT, hipStream_t s);
  void mha_bwd(int M, int d, const LnBwd& lb, const void* att, int64_t Wo, void* gATT, const AttnGeom& g,
               const float* probs, void* dq, void* dk, void* dv, hipStream_t s);
  void enc_layer_bwd(const EncLayerOff& w, EncAct& A, Acts::GradBufs& gb, const void* X, int B, int N,
                     const uint8_t* valid, int layer, bool on, void* gO, void* gR, hipStream_t s);
  void image_objects_bwd(const void* gX0, int B, int N, bool on, hipStream_t s);
  void move_first_bwd(int Md, bool on, hipStream_t s);
  void backward(hipStream_t s, bool step_params = false);
  // ---- engine_update.hip
  void build_tiles();
  void retile(int64_t off, int64_t n, hipStream_t s, bool trans_only = false);
  void set_opt_word(int idx, float v);
  void adam_range(int64_t off, int64_t n, hipStream_t s, int grid_cap = 0, const float* gscale = nullptr);
  void bucket(int64_t off, int64_t n, hipStream_t s, bool sync = true, bool from_s = false);
  void bucket_update(int64_t off, int64_t n, int grid_cap = 0);
  void bucket_reduce(int64_t off, int64_t n);
  void bucket_adam(int64_t off, int64_t n, int grid_cap, const float* gscale);
  void clip_tail();
  void check_buckets();
  void allreduce_grads(hipStream_t s);
  void adam(hipStream_t s);
  void refresh_shadow(hipStream_t s);
  void dp_check(hipStream_t cs, const float* loss, bool force = false);
  void set_lr(float lr);
  void set_grad_clip(float max_norm);
  void drop_step_graph();
  void count_update(hipStream_t s);
  void set_weight_decay(float wd);
  void set_ema(float decay);
  void set_ema_state(const float* host_src, int64_t n_updates);
  void ema_swap();
  void dp_init(const char id[128], int rank_, int world_);
  void dp_sync_adam_state();
  void dp_set_global_count(float count);
  // ---- engine_step.hip
  void drop_graph();
  void enter(hipStream_t cs);
  void leave(hipStream_t cs);
  void tune_once(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T, float* loss);
  void host_timing(const char* fwd_what, host_clock::time_point t0, host_clock::time_point t1);
  void train_step(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T, float* loss,
                  hipStream_t cs);
  void rl_sample(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
                 int64_t* sample_out, float* entropy_out, float* lm_out, hipStream_t cs);
  void rl_finish(const float* score, float w, float* out3, bool train, hipStream_t cs);
  void forward_call(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
                    float* loss_out, bool drop_on, hipStream_t cs, bool hand_back = true);
  std::string collectives(int op);
  std::string stamps(int op, double* out, int cap, int& count);
  // ---- engine_decode.hip
  std::vector<std::array<int64_t, 3>> dtile_list() const;
  void ensure_dtiles();
  void build_dtiles(hipStream_t s);
  void encode_only(const void* feats, DType ft, const float* pos, int B, int N, hipStream_t s);
  void plan_gen(Planner& p, int R, int N);
  void ensure_gen(int R, int N);
  void begin_decode(const void* feats, DType ft, const float* pos, int B, int N, int R, hipStream_t s);
  int ln_fold(int M) const;
  void dec_step(int R, int Bimg, int N, int t, void* cache, const int32_t* ids, bool want_attn, hipStream_t s,
                const int32_t* kv_row = nullptr);
  void greedy(const void* feats, DType ft, const float* pos, int B, int N, int64_t* ids_out, float* attn_out,
              hipStream_t s);
  void beam(const void* feats, DType ft, const float* pos, int B, int N, int k, int64_t* ids_out, hipStream_t s);
  void beam_nbest(const void* feats, DType ft, const float* pos, int B, int N, int k, int end_id, float alpha,
                  int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out, hipStream_t s,
                  const EnsembleRun* ens = nullptr);
  void beam_diverse(const void* feats, DType ft, const float* pos, int B, int N, int k, int G, float lambda, int end_id,
                    float alpha, int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out,
                    hipStream_t s, const EnsembleRun* ens = nullptr);
  void beam_forced(const void* feats, DType ft, const float* pos, int B, int N, int k, int end_id, float alpha,
                   int n_best, const int32_t* word, const int32_t* group, int W, int64_t* ids_out, float* score_out,
                   float* logp_out, int32_t* len_out, int32_t* met_out, hipStream_t s, const EnsembleRun* ens = nullptr);
  void beam_run(const void* feats, DType ft, const float* pos, int B, int N, int k, const int* end_id, hipStream_t s,
                const EnsembleRun* ens = nullptr, const BeamGroups* groups = nullptr,
                const BeamForced* forced = nullptr);
  void sample(const void* feats, DType ft, const float* pos, int B, int N, int n, float temperature, int top_k,
              float top_p, uint64_t sd, int64_t* ids_out, float* logp_out, hipStream_t s,
              const EnsembleRun* ens = nullptr);
  static EnsembleRun checked_ensemble(const capgen_ensemble* e, const std::string& who);
  void ensemble_begin(const EnsembleRun& ens, const void* feats, DType ft, const float* pos, int B, int N, int R,
                      hipStream_t s);
  void ensemble_step(const EnsembleRun& ens, int R, int Bimg, int N, int t, const int32_t* kv_row, hipStream_t s);
  void ensemble_enter(const EnsembleRun& ens, hipStream_t cs);
  void ensemble_leave(const EnsembleRun& ens, hipStream_t cs);
  void set_constraints(const capgen_decode_constraints* c);
};
