// capgen engine -- the parameter update: the tiled weight copies, Adam over arena ranges, the
// bucketed (all-reduced or ZeRO-1 sharded) update with its clipping tail, and the data-parallel set-up.
#include "engine.h"

void capgen_engine::build_tiles() {  // (bf16 engines, at creation: model widths of 512 only)
  std::vector<std::pair<int64_t, int>> ws;
  if (L.d == 512) {
    for (const auto& e : L.enc) ws.push_back({e.Wqkv, 3 * L.d}), ws.push_back({e.Wo, -512});
    if (L.has_img) ws.push_back({L.img.Wqkv, 3 * L.d}), ws.push_back({L.img.Wo, -512});
  }
  if (L.dd == 512)
    for (const auto& e : L.dec)
      ws.push_back({e.Wqkv, 3 * L.dd}), ws.push_back({e.Wq_c, L.dd}), ws.push_back({e.Wo_s, -512}),
          ws.push_back({e.Wo_c, -512});
  int64_t n = 0;
  for (auto& w : ws) tiled[w.first] = {n, w.second}, n += (int64_t)std::abs(w.second) * 512;
  if (n) CAPGEN_HIP(hipMalloc(&wtile, (size_t)n * 2));
}

// re-tile the fronts' weights that overlap the arena range [off, off + n) from the shadow (a matrix
// cut by a range boundary is re-tiled by both ranges' calls; the later one, on the same stream, sees
// the whole matrix updated)
void capgen_engine::retile(int64_t off, int64_t n, hipStream_t s, bool trans_only) {
  ++wver;
  for (auto& kv : tiled)
    if (kv.first < off + n && kv.first + (int64_t)std::abs(kv.second.second) * 512 > off) {
      if (kv.second.second < 0) qkv_tile_weights_t(shadow + kv.first, 512, wtile + kv.second.first, s);
      else if (!trans_only) qkv_tile_weights(shadow + kv.first, kv.second.second, 512, wtile + kv.second.first, s);
    }
}

void capgen_engine::set_opt_word(int idx, float v) {
  // the previous copy may still be queued: it must read the old value (as capgen_dp_set_global_count)
  CAPGEN_HIP(hipEventSynchronize(ev_opt));
  opt_host[idx] = v;
  if (hz::active()) hz::op(es, "opt_copy", {hz::wr(opt + idx, 4)});
  CAPGEN_HIP(hipMemcpyAsync(opt + idx, opt_host + idx, sizeof(float), hipMemcpyHostToDevice, es));
  // es follows every step issued so far (leave / the direct step's hand-back), so the copy lands after
  // their reads; the steps issued from now on read the words on es or on ec
  hz::record(ev_opt, es);
  if (ec != es) hz::wait(ec, ev_opt);
}

// Adam over arena ranges; ranges are 64-element aligned so the bf16 shadow slices line up
void capgen_engine::adam_range(int64_t off, int64_t n, hipStream_t s, int grid_cap, const float* gscale) {
  ++wver;  // (the embedding table has no shadow: its bf16 decode copy follows the version too)
  const int64_t ns = shadow ? std::max<int64_t>(0, std::min(n, L.n_dense - off)) : 0;
  // the fronts' tiled weights in this range: written by the Adam kernel itself (else re-tiled after)
  AdamTiles at;
  bool fused_tiles = true;
  for (auto& kv : tiled)
    if (ns > 0 && kv.second.second > 0 && kv.first < off + ns && kv.first + (int64_t)kv.second.second * 512 > off) {
      // a tiled matrix only partly inside this range (a bucket boundary through it): re-tile after
      if (at.n == AdamTiles::kMax || kv.first < off || kv.first + (int64_t)kv.second.second * 512 > off + ns ||
          (kv.first - off) % 4 != 0) {
        fused_tiles = false;
        break;
      }
      at.off[at.n] = kv.first - off, at.len[at.n] = (int64_t)kv.second.second * 512;
      at.dst[at.n++] = wtile + kv.second.first;
    }
  adam_update(params + off, grads + off, am + off, av + off, (size_t)n, cfg.beta1, cfg.beta2, cfg.eps, adam_scal,
              ns > 0 ? shadow + off : nullptr, (size_t)ns, s, grid_cap, fused_tiles ? at : AdamTiles{}, gscale,
              adam_opt(off));
  if (ns > 0) retile(off, ns, s, /*trans_only=*/fused_tiles);  // (the transposed ones: always a launch)
}

// Step mode (train_step): the parameter update is bucketed.  A bucket is an arena range
// whose gradients are final and whose weights nothing later in the backward pass reads
// (one transformer block, the classifier, ...).  When backward reaches that point, the
// bucket stream ec waits for both compute streams, all-reduces the bucket's gradients
// over RCCL (DP) and runs Adam on it, overlapped with the rest of the backward pass.
// Buckets are issued in reverse layer order: 12-20 MB each at C2, one per block.
// sync: first flush (es2 waits for s, queued dW issued); sync=false when es2 already holds
// every producer of the bucket's gradients (consecutive buckets after one flush)
// from_s: every producer of the bucket's gradients ran on s (no flush, ec waits for s)
void capgen_engine::bucket(int64_t off, int64_t n, hipStream_t s, bool sync, bool from_s) {
  if (sync && !from_s) flush(s);
  if (!bstep) return;
  if (from_s) dep(s, ec, ev_b1);
  else dep(es2, ec, ev_b2);
  bucket_update(off, n);
}

// the bucket's all-reduce (DP) + Adam on the bucket stream (its producers already waited for).
// With clipping on (capgen_set_grad_clip) the bucket's sum of squares follows its reduction and its
// Adam is deferred to clip_tail, after the step's last bucket: the norm is known only then.
void capgen_engine::bucket_update(int64_t off, int64_t n, int grid_cap) {
  ++wver;
  zbuckets.push_back({off, n});
  bucket_reduce(off, n);
  if (clip_on()) {
    gn_deferred.push_back({off, n, grid_cap});
    return;
  }
  bucket_adam(off, n, grid_cap, nullptr);
}

void capgen_engine::bucket_reduce(int64_t off, int64_t n) {
  const int zw = zworld();
  const bool sharded = bucket_sharded(n);
  int64_t noff = off, nn = n;  // what this rank adds to the step's gradient norm
  if (sharded) {
    const int64_t c = n / zw, o = off + (int64_t)zrank() * c;
    if (zw > 1) moments_sharded = true;  // this rank's moments are current in its chunks only
    if (zw > 1 && ema_on()) ema_sharded = true;  // ... and so is its average
    if (comm && zw > 1) grads_sharded = true;  // the gradient arena holds reduce-scattered chunks
    // in place: rank r's chunk of the summed gradients lands at grads + o
    if (comm) {
      nccl_op(ec, "reduce_scatter", grads + off, n * 4);
      NCCL_CHECK(ncclReduceScatter(grads + off, grads + o, (size_t)c, ncclFloat, ncclSum, comm, ec));
      noff = o, nn = c;  // the ranks' chunk sums are all-reduced in clip_tail
    }
    // (capgen_dp_debug_shard: no collectives, every emulated rank holds the full gradients -- the
    // norm over the whole bucket gives each of them the same coefficient)
  } else if (comm) {
    nccl_op(ec, "allreduce(bucket)", grads + off, n * 4);
    NCCL_CHECK(ncclAllReduce(grads + off, grads + off, (size_t)n, ncclFloat, ncclSum, comm, ec));
  }
  if (!clip_on()) return;
  // a bucket every rank holds whole (all-reduced): clip_tail's all-reduce of the sum would count it
  // `world` times, so rank 0 alone adds it
  if (!sharded && comm && world > 1 && rank != 0) return;
  gn_slots += grad_sumsq(grads + noff, (size_t)nn, gn_part + gn_slots, gn_slots_cap - gn_slots, ec);
}

void capgen_engine::bucket_adam(int64_t off, int64_t n, int grid_cap, const float* gscale) {
  if (bucket_sharded(n)) {
    const int zw = zworld();
    const int64_t c = n / zw, o = off + (int64_t)zrank() * c;
    const int64_t ns = shadow ? std::max<int64_t>(0, std::min(n, L.n_dense - off)) : 0;
    adam_update(params + o, grads + o, am + o, av + o, (size_t)c, cfg.beta1, cfg.beta2, cfg.eps, adam_scal, nullptr, 0,
                ec, grid_cap, AdamTiles{}, gscale, adam_opt(o));
    // in place: every rank's updated chunk -> params + off (sendbuff = recvbuff + rank * c)
    if (comm) {
      nccl_op(ec, "all_gather", params + off, n * 4);
      NCCL_CHECK(ncclAllGather(params + o, params + off, (size_t)c, ncclFloat, comm, ec));
    }
    if (ns > 0) to_bf16(params + off, shadow + off, (size_t)ns, ec);
    if (ns > 0) retile(off, ns, ec);
    return;
  }
  adam_range(off, n, ec, grid_cap, gscale);
}

// the clipped step's tail on the bucket stream, after its last bucket: the slots' sum (all-reduced as
// one double under DP: every rank then derives the same coefficient), {norm, coef}, then every
// deferred bucket's Adam with its gradients scaled by coef, in issue order.  Every slot read here was
// written in this step, so a graph replay needs nothing re-zeroed.
void capgen_engine::clip_tail() {
  grad_norm_finish(gn_part, gn_slots, gn_sum, opt + 1, 0.f, opt + 2, comm ? 1 : 3, ec);
  if (comm) {
    nccl_op(ec, "allreduce(gnorm)", gn_sum, 8);
    NCCL_CHECK(ncclAllReduce(gn_sum, gn_sum, 1, ncclDouble, ncclSum, comm, ec));
    grad_norm_finish(nullptr, 0, gn_sum, opt + 1, 0.f, opt + 2, 2, ec);
  }
  for (const DeferredAdam& d : gn_deferred)
    bucket_adam(d.off, d.n, clip_adam_grid > 0 ? clip_adam_grid : d.grid_cap, opt + 3);
  gn_deferred.clear();
  gn_slots = 0;
  norm_valid = true;
}

// once: the step's buckets cover the arena exactly (each element updated by exactly one bucket)
void capgen_engine::check_buckets() {
  if (zbuckets_checked) return;
  auto v = zbuckets;
  std::sort(v.begin(), v.end());
  int64_t end = 0;
  for (auto& b : v) {
    require(b[0] == end && b[1] > 0, "internal: gradient buckets do not tile the parameter arena");
    end = b[0] + b[1];
  }
  require(end == L.total, "internal: gradient buckets do not cover the parameter arena");
  zbuckets_checked = true;
}

void capgen_engine::allreduce_grads(hipStream_t s) {
  if (!comm) return;
  nccl_op(s, "allreduce(grads)", grads, L.total * 4);
  NCCL_CHECK(ncclAllReduce(grads, grads, (size_t)L.total, ncclFloat, ncclSum, comm, s));
}

void capgen_engine::adam(hipStream_t s) {
  ++wver;
  adam_prepare(step, opt, cfg.beta1, cfg.beta2, adam_scal, s, wd_word());
  count_update(s);
  // clipping on: the norm of the whole arena (the gradients are whole and, under DP, already
  // all-reduced on every rank: no collective), then Adam with the scale
  const float* gscale = nullptr;
  if (clip_on()) {
    const int slots = grad_sumsq(grads, (size_t)L.total, gn_part, gn_slots_cap, s);
    grad_norm_finish(gn_part, slots, nullptr, opt + 1, 0.f, opt + 2, 3, s);
    gscale = opt + 3;
    norm_valid = true;
  }
  adam_update(params, grads, am, av, (size_t)L.total, cfg.beta1, cfg.beta2, cfg.eps, adam_scal, shadow,
              shadow ? (size_t)L.n_dense : 0, s, 0, AdamTiles{}, gscale, adam_opt(0));
  if (shadow) retile(0, L.n_dense, s);
}

void capgen_engine::refresh_shadow(hipStream_t s) {
  if (shadow) to_bf16(params, shadow, (size_t)L.n_dense, s);
  if (shadow) retile(0, L.n_dense, s);
}

// Once, after the first train step at world > 1: every rank must hold the same GLOBAL non-pad count
// (the count all-reduce inside the forward -- captured in its graph -- gives the reference's mean over
// the global batch, model.py:76) and so the same loss.  Max and min over the ranks of both, one
// grouped 4-value exchange; a mismatch fails the step (non-zero status, capgen_last_error).
// `force` runs it regardless of world size and of an earlier check (capgen_dp_check: the world-1
// rehearsal of the exchange; the step's own call passes false).  `loss` null = the loss buffer the
// last forward wrote (its loss_out, or the internal one).
void capgen_engine::dp_check(hipStream_t cs, const float* loss, bool force) {
  if (!comm || (!force && (dp_checked || world <= 1))) return;
  dp_checked = true;
  if (!dp_chk) CAPGEN_HIP(hipMalloc(&dp_chk, 4 * sizeof(float)));
  const float* lo = loss ? loss : last_loss;
  require(a.count && lo, "dp_check: no train step yet");
  for (int i = 0; i < 2; ++i) {
    CAPGEN_HIP(hipMemcpyAsync(dp_chk + i, a.count, sizeof(float), hipMemcpyDeviceToDevice, cs));
    CAPGEN_HIP(hipMemcpyAsync(dp_chk + 2 + i, lo, sizeof(float), hipMemcpyDeviceToDevice, cs));
  }
  NCCL_CHECK(ncclGroupStart());
  NCCL_CHECK(ncclAllReduce(dp_chk, dp_chk, 1, ncclFloat, ncclMax, comm, cs));
  NCCL_CHECK(ncclAllReduce(dp_chk + 1, dp_chk + 1, 1, ncclFloat, ncclMin, comm, cs));
  NCCL_CHECK(ncclAllReduce(dp_chk + 2, dp_chk + 2, 1, ncclFloat, ncclMax, comm, cs));
  NCCL_CHECK(ncclAllReduce(dp_chk + 3, dp_chk + 3, 1, ncclFloat, ncclMin, comm, cs));
  NCCL_CHECK(ncclGroupEnd());
  float hv[4];
  CAPGEN_HIP(hipMemcpyAsync(hv, dp_chk, sizeof hv, hipMemcpyDeviceToHost, cs));
  CAPGEN_HIP(hipStreamSynchronize(cs));
  require(hv[0] == hv[1] && hv[0] > 0.f,
          "dp: the global target count differs across ranks after the first step (max " + std::to_string(hv[0]) +
              ", min " + std::to_string(hv[1]) + ")");
  require(hv[2] == hv[3], "dp: the global loss differs across ranks after the first step (max " +
                              std::to_string(hv[2]) + ", min " + std::to_string(hv[3]) + ")");
}

void capgen_engine::set_lr(float lr) {
  set_opt_word(0, lr);
  lr_cur = lr;
}

// the whole-step graph holds the update's schedule and kernel variants; the forward graph does not
void capgen_engine::drop_step_graph() {
  if (!gexec) return;
  (void)hipGraphExecDestroy(gexec);
  gexec = nullptr;
}

void capgen_engine::set_grad_clip(float max_norm) {
  const bool on = max_norm != 0.f;
  if (on != clip_on()) drop_step_graph();  // (norm pass, deferred Adam)
  if (on) set_opt_word(1, max_norm);
  clip_cur = max_norm;
}

// one parameter update is being issued on s (not: captured -- the replays are counted where they launch)
void capgen_engine::count_update(hipStream_t s) {
  if (!ema_on()) return;
  hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
  CAPGEN_HIP(hipStreamIsCapturing(s, &cst));
  if (cst == hipStreamCaptureStatusNone) ++ema_updates;
}

// on <-> off changes the prepare kernel and the update's variant: the step graph is re-captured; a new
// value while on is one device word, read by the replay
void capgen_engine::set_weight_decay(float wd) {
  if ((wd != 0.f) != wd_on()) drop_step_graph();
  if (wd != 0.f) set_opt_word(kOptWd, wd);
  wd_cur = wd;
}

void capgen_engine::set_ema(float decay) {
  const bool on = decay != 0.f;
  if (on != ema_on()) {
    // (swapped: the parameter arena holds the average -- neither a copy of it nor a stop would mean anything)
    require(!ema_swapped, "set_ema: the averaged weights are swapped in (capgen_ema_swap): only the decay of an "
                          "enabled average may change until they are swapped back");
    drop_step_graph();
  }
  if (on && !ema_on()) {  // off -> on: the average starts as a copy of the parameters
    hz::host_sync(es);
    hz::host_sync(ec);
    if (!ema) CAPGEN_HIP(hipMalloc(&ema, (size_t)L.total * 4));
    CAPGEN_HIP(hipMemcpyAsync(ema, params, (size_t)L.total * 4, hipMemcpyDeviceToDevice, es));
    hz::host_sync(es);
    ema_updates = 0;
    ema_sharded = false;
  }
  if (on) set_opt_word(kOptEmaRate, (float)(1.0 - (double)decay));
  ema_decay = decay;
}

void capgen_engine::set_ema_state(const float* host_src, int64_t n_updates) {
  hz::host_sync(es);
  hz::host_sync(ec);
  CAPGEN_HIP(hipMemcpy(ema, host_src, (size_t)L.total * 4, hipMemcpyHostToDevice));
  hz::host_sync(nullptr);
  ema_updates = n_updates;
  ema_sharded = false;
}

// params <-> ema in place: no pointer moves, so the cached graphs stay valid; the bf16 shadow and the
// tiles follow (the decode tiles and the bf16 embedding copy through the weight version)
void capgen_engine::ema_swap() {
  require(ema_on() && ema, "ema_swap: the average is off (capgen_set_ema)");
  require(!(ema_sharded && zworld() > 1), "ema_swap: after sharded (ZeRO-1) steps this rank's average is current in "
                                          "its own chunks only: call capgen_dp_sync_adam_state on every rank first");
  hz::host_sync(es);
  hz::host_sync(ec);
  arena_swap(params, ema, (size_t)L.total, es);
  refresh_shadow(es);
  ++wver;  // (an fp32 engine has no shadow to re-tile: its weights moved all the same)
  hz::host_sync(es);
  ema_swapped = !ema_swapped;
}

// join the communicator as rank of world, and replicate rank 0's parameters
void capgen_engine::dp_init(const char id[128], int rank_, int world_) {
  ncclUniqueId uid;
  std::memcpy(uid.internal, id, 128);
  if (comm) ncclCommDestroy(comm);
  NCCL_CHECK(ncclCommInitRank(&comm, world_, uid, rank_));
  rank = rank_, world = world_;
  drop_graph();
  NCCL_CHECK(ncclBroadcast(params, params, (size_t)L.total, ncclFloat, 0, comm, es));
  // an average enabled before this call followed this rank's former weights: it restarts as a copy of
  // the replicated ones, on every rank alike (as off -> on)
  if (ema_on()) {
    CAPGEN_HIP(hipMemcpyAsync(ema, params, (size_t)L.total * 4, hipMemcpyDeviceToDevice, es));
    ema_updates = 0;
    ema_sharded = false;
  }
  refresh_shadow(es);
  hz::host_sync(es);
}

// after sharded (ZeRO-1) steps: every rank gathers the others' chunks of the Adam moments
void capgen_engine::dp_sync_adam_state() {
  hz::host_sync(es);
  hz::host_sync(ec);
  const int zw = zworld();
  if (!comm || zw <= 1 || !zsharded()) return;
  for (auto& b : zbuckets) {
    if (b[1] % (4 * zw)) continue;  // updated by all-reduce + full Adam: already replicated
    const int64_t c = b[1] / zw, o = b[0] + (int64_t)zrank() * c;
    NCCL_CHECK(ncclAllGather(am + o, am + b[0], (size_t)c, ncclFloat, comm, es));
    NCCL_CHECK(ncclAllGather(av + o, av + b[0], (size_t)c, ncclFloat, comm, es));
    if (ema_on()) NCCL_CHECK(ncclAllGather(ema + o, ema + b[0], (size_t)c, ncclFloat, comm, es));
  }
  moments_sharded = false;
  if (ema_on()) ema_sharded = false;
  hz::host_sync(es);
}

// the global target count of the next steps, set by the host (<= 0: back to the count all-reduce)
void capgen_engine::dp_set_global_count(float count) {
  // the previous step's asynchronous copy may still be queued: it must read the old value
  CAPGEN_HIP(hipEventSynchronize(ev_count));
  if (count_override != (count > 0.f)) drop_graph();  // the forward graph's count source changes
  count_override = count > 0.f;
  *count_host = count;
}
