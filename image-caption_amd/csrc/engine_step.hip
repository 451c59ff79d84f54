// capgen engine -- creation and destruction, the stream hand-off of a C-ABI call, the train step
// (eager / forward graph / whole-step graph) and the SCST roll-out step.
#include "abi_util.h"
#include "engine.h"

void capgen_engine::drop_graph() {
  if (gexec) {
    (void)hipGraphExecDestroy(gexec);
    gexec = nullptr;
  }
  if (fexec) {
    (void)hipGraphExecDestroy(fexec);
    fexec = nullptr;
  }
}

// stream hand-off: caller stream -> engine stream -> caller stream
void capgen_engine::enter(hipStream_t cs) {
  hz::record(ev_in, cs);
  hz::wait(es, ev_in);
  hz::set_critical(es);
}

void capgen_engine::leave(hipStream_t cs) {
  hz::record(ev_out, es);
  hz::wait(cs, ev_out);
}

// The forward of one C-ABI call (capgen_forward, the weighted step without an update, score_captions,
// rl_sample): the workspace, the caller's stream -> the engine's, forward() there, and back.
// hand_back = false: the caller enqueues more on es and calls leave(cs) itself
void capgen_engine::forward_call(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
    float* loss_out, bool drop_on, hipStream_t cs, bool hand_back) {
  ensure_acts(B, N, T);
  enter(cs);
  forward(f, ft, pos, caps, B, N, T, loss_out, drop_on, es);
  if (hand_back) leave(cs);
}

// one eager forward + backward (dropout off: no RNG advance; no all-reduce, no Adam) so that every
// GEMM shape of the step is autotuned outside a capture; its gradients are overwritten by the step
void capgen_engine::tune_once(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T, float* loss) {
  if (tuned(B, N, T)) return;
  forward(f, ft, pos, caps, B, N, T, loss, /*drop_on=*/false, es);
  backward(es);
  hz::host_sync(es);
  tuned_shapes.push_back({B, N, T});
}

// CAPGEN_HOST_TIMING=1 (debug build): the mean host time of a step's two halves, every 20 steps
void capgen_engine::host_timing(const char* fwd_what, host_clock::time_point t0, host_clock::time_point t1) {
  if (!fwd_what || knob(Knob::HostTiming) == 0) return;
  const auto t2 = host_clock::now();
  ht_fwd += std::chrono::duration<double, std::micro>(t1 - t0).count();
  ht_bwd += std::chrono::duration<double, std::micro>(t2 - t1).count();
  if (++ht_steps % 20 == 0) {
    std::fprintf(stderr, "[capgen host] per step: %s %.1f us, backward enqueue %.1f us\n", fwd_what, ht_fwd / 20,
                 ht_bwd / 20);
    ht_fwd = ht_bwd = 0;
  }
}

void capgen_engine::train_step(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T, float* loss,
    hipStream_t cs) {
  ensure_acts(B, N, T);
  Key k{f, pos, caps, loss, (int)ft, B, N, T, training, in};
  // (the hazard checker's log runs the eager forward: the graph replays the same launches)
  // under DP the forward graph holds the count and partial-CE all-reduces (RCCL ops capture);
  // a host-set global count (capgen_dp_set_global_count) runs the forward eagerly instead --
  // its pinned-memory copy must stay ordered against the host write
  const bool fwd_graph =
      !graph_on && fwd_graph_on && !hz::g_log && (world <= 1 || fwd_graph_mode == 2) && !count_override;
  // the step's two halves on stream s: fwd (the eager forward, or the forward graph's launch), then the
  // backward with the bucketed RCCL all-reduce (DP) and Adam
  auto halves = [&](hipStream_t s, auto&& fwd, const char* timed_as) {
    const auto t0 = host_clock::now();
    fwd();
    const auto t1 = host_clock::now();
    fB = B, fN = N, fT = T, fwd_drop = training;  // host state forward() sets (a graph launch does not)
    set_pending_loss(loss);
    backward(s, /*step_params=*/true);
    host_timing(timed_as, t0, t1);
  };
  auto eager_fwd = [&] { forward(f, ft, pos, caps, B, N, T, loss, training, es, /*defer_loss=*/true); };
  // direct steps: once the forward graph exists, train_step runs its critical path on the CALLER's
  // stream -- no caller -> engine -> caller event round trip per step; es then waits for the step so
  // the engine's host-side syncs on es still cover it (measured: 3.165 vs 3.170 ms/step, within
  // noise -- the step-boundary gap is the Adam tail)
  if (fwd_graph && fexec && fkey == k && cs != es) {
    {
      Scoped<hipStream_t> on_caller(crit, cs);
      hz::set_critical(cs);
      halves(cs, [&] { CAPGEN_HIP(hipGraphLaunch(fexec, cs)); }, nullptr);
    }
    hz::record(ev_out, cs);
    hz::wait(es, ev_out);
    return;
  }
  enter(cs);
  if (fwd_graph) {
    // forward replayed as one hipGraph (cheap to launch: ~0.1 us/node of host time vs ~2.7 us per
    // eager launch, tools/kprobe.hip); backward issued eagerly on three streams (a multi-branch
    // graph costs the same host time per node as eager issue on ROCm 7)
    if (!(fexec && fkey == k)) {
      drop_graph();
      tune_once(f, ft, pos, caps, B, N, T, loss);
      fexec = capture(es, eager_fwd);
      fkey = k;
    }
    halves(es, [&] { CAPGEN_HIP(hipGraphLaunch(fexec, es)); }, "forward graph launch");
  } else if (!graph_on) {
    halves(es, eager_fwd, "forward enqueue");
  } else {
    if (!(gexec && gkey == k)) {
      drop_graph();
      tune_once(f, ft, pos, caps, B, N, T, loss);
      const bool moments_were = moments_sharded;
      moments_sharded = false;
      gexec = capture(es, [&] { halves(es, eager_fwd, "forward enqueue"); });
      gkey = k;
      gexec_moments_sharded = moments_sharded, gexec_grads_sharded = grads_sharded;
      moments_sharded = moments_sharded || moments_were;
    }
    // the replay runs the captured Adam and re-cast of the shadow with no host code: the weight
    // version must move with it, or the decode tiles (build_dtiles) would keep the old weights
    ++wver;
    if (ema_on()) ++ema_updates;  // (the capture's host code counted nothing)
    // a sharded step leaves the moments, the average and the gradient arena current in this rank's
    // chunks only, replayed or not (after capgen_dp_sync_adam_state, or an eager backward, as well)
    if (gexec_moments_sharded) moments_sharded = true, ema_sharded = ema_sharded || ema_on();
    grads_sharded = gexec_grads_sharded;
    CAPGEN_HIP(hipGraphLaunch(gexec, es));
  }
  leave(cs);
}

// SCST (SelfCriticNetwork.train_step, models.py:179-195): rl_sample = teacher-forced forward,
// PolicyNetwork.sample and the per-image entropy; the host scores the samples; rl_finish =
// ReinforcementLearningLoss + backward + Adam.
void capgen_engine::rl_sample(const void* f, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
    int64_t* sample_out, float* entropy_out, float* lm_out, hipStream_t cs) {
  const int Lq = T - 1, Md = B * Lq;
  {
    Scoped<bool> logits_on(need_logits, true);  // rl_rows samples from the logits
    forward_call(f, ft, pos, caps, B, N, T, nullptr, training, cs, /*hand_back=*/false);
  }
  rl_rows(a.logits, Md, L.V, a.rl_sample, a.rl_lse, a.rl_logp, a.rl_ent, es);
  rl_image(a.rl_sample, a.rl_ent, B, Lq, a.rl_ent_img, a.rl_scal, es);
  if (sample_out) rl_export(a.rl_sample, Md, sample_out, es);
  if (entropy_out) CAPGEN_HIP(hipMemcpyAsync(entropy_out, a.rl_ent_img, B * sizeof(float), hipMemcpyDeviceToDevice, es));
  if (lm_out) CAPGEN_HIP(hipMemcpyAsync(lm_out, a.loss, sizeof(float), hipMemcpyDeviceToDevice, es));
  rl_B = B;
  leave(cs);
}

void capgen_engine::rl_finish(const float* score, float w, float* out3, bool train, hipStream_t cs) {
  require(rl_B > 0 && rl_B == fB, "rl_finish: call rl_sample first");
  require(w >= 0.f && w <= 1.f, "rl_finish: structure_loss_weight must be in [0, 1]");
  enter(cs);
  const int B = fB, Lq = fT - 1;
  CAPGEN_HIP(hipMemcpyAsync(a.rl_score, score, B * sizeof(float), hipMemcpyDeviceToDevice, es));
  rl_numer(a.rl_sample, a.rl_logp, a.rl_score, B, Lq, a.rl_scal, es);
  if (comm) NCCL_CHECK(ncclAllReduce(a.rl_scal, a.rl_scal, 2, ncclFloat, ncclSum, comm, es));
  rl_loss(a.rl_scal, a.loss, w, out3 ? out3 : a.rl_scal + 2, a.grad_scale, es);
  if (train) {
    rl_grad(a.logits, a.tgt, a.rl_sample, a.rl_lse, a.rl_score, a.count, a.rl_scal, B, Lq, L.V, cfg.pad_idx, w,
            a.dlogits, act, es);
    backward(es, /*step_params=*/true);
  }
  rl_B = 0;
  leave(cs);
}

namespace {

void pe_table(const Layout& L, std::vector<float>& out) {
  // model.py:502-514: float64 angles, sin on even columns, cos on odd, cast to f32
  const int n = L.maxlen - 1, d = L.dd;
  out.resize((size_t)n * d);
  for (int p = 0; p < n; ++p)
    for (int j = 0; j < d; ++j) {
      double ang = (double)p / std::pow(10000.0, 2.0 * (j / 2) / (double)d);
      out[(size_t)p * d + j] = (float)((j % 2 == 0) ? std::sin(ang) : std::cos(ang));
    }
}

}  // namespace

// What the engine owns is allocated here and freed by the destructor below, to be read against each other.
// (Delegating: the object counts as constructed once the fields-only constructor has run, so a throw
// part-way through this body still frees through the destructor.)
capgen_engine::capgen_engine(const capgen_config& c, int dev, DType t) : cfg(c), L(make_layout(c)), device(dev), act(t) {}
capgen_engine::capgen_engine(const capgen_config& c, int dev) : capgen_engine(c, dev, dt(c.dtype)) {
  CAPGEN_HIP(hipSetDevice(device));
  gemm_init();
  const size_t n = (size_t)L.total;
  // (stream priorities measured: no gain for one engine, and with two engines in a process
  // the high-priority queues serialised each other -- plain streams)
  CAPGEN_HIP(hipStreamCreateWithFlags(&es, hipStreamNonBlocking));
  // CAPGEN_STREAMS (experiment knob): 3 = critical path + weight-grad + bucket streams
  // (default), 2 = buckets on the weight-grad stream, 1 = everything on one stream
  const int nstreams = knob(Knob::Streams);
  if (nstreams >= 2) CAPGEN_HIP(hipStreamCreateWithFlags(&es2, hipStreamNonBlocking));
  else es2 = es;
  // the fork / join / bucket events only order this device's own streams, so they skip the
  // system-scope acquire / release HIP puts on an event by default (that fence writes back and
  // invalidates L2 around every record / wait; the kernels' own device-scope fences order the
  // streams).  Measured, three alternating runs each: 2.760-2.776 ms/step vs 2.817-2.838 with the
  // system fence, 2.815-2.832 with a device-scope release only (CAPGEN_EVENT_FENCE = 1 / 0 / 2).
  const int ef = knob(Knob::EventFence);
  const unsigned evf = hipEventDisableTiming | (ef == 1 ? hipEventDisableSystemFence : ef == 2 ? hipEventReleaseToDevice : 0u);
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_fork, evf));
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_join, evf));
  if (nstreams >= 3) CAPGEN_HIP(hipStreamCreateWithFlags(&ec, hipStreamNonBlocking));
  else ec = es2;
  for (hipEvent_t* e : {&ev_b1, &ev_b2, &ev_cj, &ev_ff, &ev_fj})
    CAPGEN_HIP(hipEventCreateWithFlags(e, evf));
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_count, hipEventDisableTiming));
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
  CAPGEN_HIP(hipMalloc(&params, n * 4));
  CAPGEN_HIP(hipMalloc(&grads, n * 4));
  CAPGEN_HIP(hipMalloc(&am, n * 4));
  CAPGEN_HIP(hipMalloc(&av, n * 4));
  CAPGEN_HIP(hipMemset(params, 0, n * 4));
  CAPGEN_HIP(hipMemset(grads, 0, n * 4));
  CAPGEN_HIP(hipMemset(am, 0, n * 4));
  CAPGEN_HIP(hipMemset(av, 0, n * 4));
  if (act == DType::BF16) {
    CAPGEN_HIP(hipMalloc(&shadow, (size_t)L.n_dense * 2));
    CAPGEN_HIP(hipMemset(shadow, 0, (size_t)L.n_dense * 2));
    build_tiles();
  }
  std::vector<float> table;
  pe_table(L, table);
  CAPGEN_HIP(hipMalloc(&pe, table.size() * 4));
  CAPGEN_HIP(hipMemcpy(pe, table.data(), table.size() * 4, hipMemcpyHostToDevice));
  CAPGEN_HIP(hipMalloc(&step, 64));
  CAPGEN_HIP(hipMemset(step, 0, 64));
  CAPGEN_HIP(hipMalloc(&adam_scal, 64));
  CAPGEN_HIP(hipMalloc(&opt, 64));
  CAPGEN_HIP(hipMemset(opt, 0, 64));
  lr_cur = cfg.lr;
  CAPGEN_HIP(hipMemcpy(opt, &lr_cur, sizeof(float), hipMemcpyHostToDevice));
  CAPGEN_HIP(hipHostMalloc(&opt_host, 64, hipHostMallocDefault));
  CAPGEN_HIP(hipEventCreateWithFlags(&ev_opt, hipEventDisableTiming));
  // one slot per sum-of-squares workgroup: at most 256 per bucket, one bucket per block plus the fixed ones
  gn_slots_cap = 256 * (L.Le + L.Ld + 16);
  CAPGEN_HIP(hipMalloc(&gn_part, (size_t)gn_slots_cap * sizeof(double)));
  CAPGEN_HIP(hipMalloc(&gn_sum, 64));
  CAPGEN_HIP(hipMalloc(&seed, 64));
  uint64_t sd = cfg.seed;
  CAPGEN_HIP(hipMemcpy(seed, &sd, 8, hipMemcpyHostToDevice));
  CAPGEN_HIP(hipMalloc(&scalars, 256));
  n_small = L.total - L.enc_lng;
  CAPGEN_HIP(hipMalloc(&gstripe, (size_t)NSTRIPE * n_small * sizeof(float)));
  CAPGEN_HIP(hipHostMalloc(&count_host, 64, hipHostMallocDefault));
  // the null-stream memsets above are not ordered before the engine's non-blocking streams
  hz::host_sync(nullptr);
}

capgen_engine::~capgen_engine() {
  if (es) (void)hipStreamSynchronize(es);
  drop_graph();
  if (comm) ncclCommDestroy(comm);
  for (void* p : {(void*)params, (void*)grads, (void*)am, (void*)av, (void*)shadow, (void*)wtile, (void*)dtiles, (void*)emb_bf, (void*)pe, (void*)step,
                  (void*)adam_scal, (void*)seed, (void*)scalars, (void*)gstripe, ws, gws, (void*)stamp_ring,
                  (void*)dc_banned})
    if (p) (void)hipFree(p);
  if (count_host) (void)hipHostFree(count_host);
  if (opt_host) (void)hipHostFree(opt_host);
  for (void* p : {(void*)opt, (void*)gn_part, (void*)gn_sum, (void*)ema})
    if (p) (void)hipFree(p);
  if (ev_opt) (void)hipEventDestroy(ev_opt);
  if (dp_chk) (void)hipFree(dp_chk);
  if (ev_in) (void)hipEventDestroy(ev_in);
  if (ev_out) (void)hipEventDestroy(ev_out);
  if (ev_fork) (void)hipEventDestroy(ev_fork);
  if (ev_join) (void)hipEventDestroy(ev_join);
  for (hipEvent_t e : {ev_b1, ev_b2, ev_cj, ev_count, ev_ff, ev_fj})
    if (e) (void)hipEventDestroy(e);
  if (ec && ec != es && ec != es2) (void)hipStreamSynchronize(ec), (void)hipStreamDestroy(ec);
  if (es2 && es2 != es) (void)hipStreamSynchronize(es2), (void)hipStreamDestroy(es2);
  if (es) (void)hipStreamDestroy(es);
}

// capgen_debug_collectives: op 0 (off) / 1 (on) clear the log, 2 returns it, one collective per line
std::string capgen_engine::collectives(int op) {
  std::string all;
  if (op < 2) {
    coll_log_on = op == 1;
    coll_log.clear();
  } else {
    for (auto& l : coll_log) all += l + "\n";
  }
  return all;
}

// capgen_debug_stamps: op 0 (off), 1 (on), 2 (read), 3 (arm).  Read: {start, end} in us of each of the
// count launches that fit into out[cap]; returns their names, one per line
std::string capgen_engine::stamps(int op, double* out, int cap, int& count) {
  std::string all;
  if (op == 0 || op == 1) {
    hz::host_sync(nullptr);
    stamp_on = op == 1;
    if (stamp_on && !stamp_ring) CAPGEN_HIP(hipMalloc(&stamp_ring, (size_t)kStampSlots * 16 * sizeof(uint64_t)));
    drop_graph();  // a captured forward holds its launches' stamp pointers
  }
  if (op == 3 || op == 1) {
    hz::host_sync(nullptr);
    if (stamp_ring) CAPGEN_HIP(hipMemset(stamp_ring, 0, (size_t)kStampSlots * 16 * sizeof(uint64_t)));
    CAPGEN_HIP(hipDeviceSynchronize());
  }
  if (op == 2) {
    require(stamp_ring != nullptr, "debug_stamps: not enabled");
    hz::host_sync(nullptr);
    std::vector<uint64_t> ring((size_t)stamp_max * 16);
    CAPGEN_HIP(hipMemcpy(ring.data(), stamp_ring, ring.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (int i = 0; i < stamp_max && 2 * i + 1 < cap; ++i) {
      uint64_t e = 0;
      for (int k = 1; k <= 8; ++k) e = std::max(e, ring[(size_t)i * 16 + k]);
      out[2 * i] = (double)ring[(size_t)i * 16] * 0.01;  // 100 MHz ticks -> us
      out[2 * i + 1] = (double)e * 0.01;
      all += (i < (int)stamp_names.size() ? stamp_names[i] : std::string("?")) + "\n";
      ++count;
    }
  }
  return all;
}
