// capgen engine -- the forward pass (model.py:79-98): the attention fronts, the encoder and decoder
// blocks, the classifier + CE / score read-out, and the activation workspace they run over.
#include "engine.h"

// The self-attention front of a block (modules.py:67-76 + 16-27): qkv = X . Wqkv^T, then the
// attention of g over it into att.  bf16 with head size 64 and d = 512: ONE fused launch
// (qkv_attn.hip: projection straight into the attention's LDS images; qkv still written for the
// backward).  Otherwise (f32 parity mode, other geometries, CAPGEN_FUSED_QKV=0) the GEMM and the
// attention launch.
void capgen_engine::self_attention(const void* X, int64_t wqkv, int M, int d, const AttnGeom& g, void* qkv, void* att, float* probs,
    hipStream_t s) {
  if (fused_qkv_on && act == DType::BF16 && !keep_probs(g)) {
    QkvAttn qa;
    qa.g = g, qa.g.prio = prio(s);
    qa.X = reinterpret_cast<const bf16*>(X), qa.ldx = d, qa.W = WT(wqkv);
    qa.d = d, qa.qkv = reinterpret_cast<bf16*>(qkv), qa.ldqkv = 3 * d, qa.o = reinterpret_cast<bf16*>(att);
    if (qkv_attn_ok(qa)) {
      if (stamp_on) qa.g.stamp = stamp(s, "qkv_attn " + std::to_string(g.Lq) + "x" + std::to_string(g.Lk));
      qkv_attn_fwd(qa, s);
      return;
    }
  }
  linear(X, d, wqkv, d, qkv, 3 * d, act, M, 3 * d, d, nullptr, 0, s);
  attf(g, att, probs, act, s);
}

// The cross-attention of a decoder block (modules.py:195-197): q = D1 . Wq^T then attention over
// the precomputed cross K/V.  q_done: q already projected (else bf16: the fused launch projects it
// straight into the attention's LDS image, qkv_attn.hip cross mode).
void capgen_engine::cross_attention(const AttnGeom& c, const void* D1, int64_t wq, int d, void* qc, void* attc, float* probs,
    bool q_done, hipStream_t s) {
  if (!q_done) {
    QkvAttn qa;
    qa.g = c, qa.g.prio = prio(s), qa.cross = 1;
    qa.X = reinterpret_cast<const bf16*>(D1), qa.ldx = d, qa.W = WT(wq);
    qa.d = d, qa.qkv = reinterpret_cast<bf16*>(qc), qa.ldqkv = d, qa.o = reinterpret_cast<bf16*>(attc);
    require(!probs && qkv_attn_ok(qa), "internal: cross-attention geometry the fused launch does not take");
    if (stamp_on) qa.g.stamp = stamp(s, "qkv_attn cross " + std::to_string(c.Lq) + "x" + std::to_string(c.Lk));
    qkv_attn_fwd(qa, s);
    return;
  }
  attf(c, attc, probs, act, s);
}

void capgen_engine::plan_acts(Planner& p, int B, int N, int T) {
  const int64_t Me = (int64_t)B * N, L = T - 1, Md = (int64_t)B * L, d = L_().d, dd = L_().dd;
  const int64_t Mx = std::max(Me, Md);
  const size_t e = es_();
  auto T_ = [&](void*& ptr, int64_t n) { ptr = p.raw(n * e); };
  T_(a.Aenc, Me * L_().Kp);
  p.take(a.valid, Me);
  T_(a.ev0, Me * d);
  p.take(a.em0, Me);
  p.take(a.er0, Me);
  a.X.resize(L_().Le + 1);
  for (auto& x : a.X) T_(x, Me * d);
  a.enc.resize(L_().Le);
  for (auto& l : a.enc) {
    T_(l.qkv, Me * 3 * d);
    p.take(l.P, (size_t)B * L_().He * N * N);
    T_(l.att, Me * d);
    T_(l.v1, Me * d);
    p.take(l.m1, Me);
    p.take(l.r1, Me);
    T_(l.Y, Me * d);
    T_(l.H, Me * L_().fe);
    T_(l.v2, Me * d);
    p.take(l.m2, Me);
    p.take(l.r2, Me);
  }
  T_(a.KV, Me * L_().Ld * 2 * dd);
  p.take(a.ids, Md);
  p.take(a.tgt, Md);
  p.take(a.count, 4);
  T_(a.E, Md * L_().dwe);
  T_(a.dv0, Md * dd);
  T_(a.tmpf, Md * dd);
  p.take(a.dm0, Md);
  p.take(a.dr0, Md);
  a.D.resize(L_().Ld + 1);
  for (auto& x : a.D) T_(x, Md * dd);
  a.dec.resize(L_().Ld);
  for (auto& l : a.dec) {
    T_(l.qkv, Md * 3 * dd);
    p.take(l.Ps, (size_t)B * L_().Hd * L * L);
    T_(l.atts, Md * dd);
    T_(l.vs, Md * dd);
    p.take(l.ms, Md);
    p.take(l.rs, Md);
    T_(l.D1, Md * dd);
    T_(l.qc, Md * dd);
    p.take(l.Pc, (size_t)B * L_().Hd * L * N);
    T_(l.attc, Md * dd);
    T_(l.vc, Md * dd);
    p.take(l.mc, Md);
    p.take(l.rc, Md);
    T_(l.D2, Md * dd);
    T_(l.H, Md * L_().fd);
    T_(l.vf, Md * dd);
    p.take(l.mf, Md);
    p.take(l.rf, Md);
  }
  p.take(a.logits, Md * L_().V);
  T_(a.dlogits, Md * L_().V);
  a.ce_stats = reinterpret_cast<float2*>(p.raw((size_t)Md * ((L_().V + 15) / 16) * sizeof(float2)));
  p.take(a.ce_tl, Md);
  p.take(a.loss_row, Md);
  p.take(a.grad_scale, 4);
  p.take(a.loss, 4);
  p.take(a.loss_ce, 4);
  T_(a.gEnc, Me * d);
  p.take(a.rl_sample, Md);
  p.take(a.rl_lse, Md);
  p.take(a.rl_logp, Md);
  p.take(a.rl_ent, Md);
  p.take(a.rl_ent_img, B);
  p.take(a.rl_score, B);
  p.take(a.rl_scal, 8);
  const int64_t dmax = std::max<int64_t>(std::max(d, dd), L_().dwe);
  T_(a.tmp, Mx * dmax);
  T_(a.gOut, Mx * dmax);
  T_(a.gRes, Mx * dmax);
  T_(a.gKV, Me * L_().Ld * 2 * dd);
  T_(a.gE, Md * L_().dwe);
  T_(a.gAe, Me * d);
  T_(a.gAd, Md * dd);
  a.genc.resize(L_().Le);
  for (auto& gb : a.genc) {
    T_(gb.gAf, Me * d);
    T_(gb.gH, Me * L_().fe);
    T_(gb.gA1, Me * d);
    T_(gb.gATT1, Me * d);
    T_(gb.gQKV, Me * 3 * d);
    gb.gA2 = gb.gATT2 = gb.gQc = nullptr;
  }
  if (L_().has_img) {  // sized 0 otherwise (the planner still hands out aligned pointers)
    const int64_t M2 = 2 * Me;
    T_(a.siY, Me * d);
    T_(a.siEp, Me * d);
    T_(a.siX2, M2 * d);
    T_(a.siZ, M2 * d);
    T_(a.siV, Me * d);
    T_(a.siG0, M2 * d);
    T_(a.siG1, M2 * d);
    T_(a.siGY, Me * d);
    T_(a.siGEp, Me * d);
    p.take(a.siValid, M2);
    p.take(a.siM, Me);
    p.take(a.siR, Me);
    auto& l = a.si;
    T_(l.qkv, M2 * 3 * d);
    p.take(l.P, (size_t)Me * L_().He * 4);
    T_(l.att, M2 * d);
    T_(l.v1, M2 * d);
    p.take(l.m1, M2);
    p.take(l.r1, M2);
    T_(l.Y, M2 * d);
    T_(l.H, M2 * L_().fe);
    T_(l.v2, M2 * d);
    p.take(l.m2, M2);
    p.take(l.r2, M2);
    auto& gb = a.gsi;
    T_(gb.gAf, M2 * d);
    T_(gb.gH, M2 * L_().fe);
    T_(gb.gA1, M2 * d);
    T_(gb.gATT1, M2 * d);
    T_(gb.gQKV, M2 * 3 * d);
    gb.gA2 = gb.gATT2 = gb.gQc = nullptr;
  }
  if (L_().has_mf) {
    T_(a.mfU, Md * dd);
    T_(a.mfH, Md * L_().fd);
    T_(a.mfV, Md * dd);
    T_(a.mfOut, Md * dd);
    T_(a.mfGA, Md * dd);
    T_(a.mfGH, Md * L_().fd);
    T_(a.mfGU, Md * dd);
    p.take(a.mfM, Md);
    p.take(a.mfR, Md);
  }
  a.gdec.resize(L_().Ld);
  for (auto& gb : a.gdec) {
    T_(gb.gAf, Md * dd);
    T_(gb.gH, Md * L_().fd);
    T_(gb.gA1, Md * dd);
    T_(gb.gATT1, Md * dd);
    T_(gb.gQKV, Md * 3 * dd);
    T_(gb.gA2, Md * dd);
    T_(gb.gATT2, Md * dd);
    T_(gb.gQc, Md * dd);
  }
  // score mode's per-row scratch, last: every buffer of the train step keeps its offset
  p.take(a.sc_tok, Md);
  p.take(a.sc_hit, Md);
}

void capgen_engine::ensure_acts(int B, int N, int T) {
  if (ws && B <= a.B && N <= a.N && T <= a.T) return;
  int nB = std::max(B, a.B), nN = std::max(N, a.N), nT = std::max(T, a.T);
  if (ws) {  // the graphs hold the old block's addresses
    hz::host_sync(es);
    drop_graph();
  }
  replan(ws, [&](Planner& p) { plan_acts(p, nB, nN, nT); });
  a.B = nB, a.N = nN, a.T = nT;
}

// one EncoderBlock (modules.py:146-157) over B sequences of N rows: X -> Xout.  valid != null:
// key-pad OR causal self-attention mask and the non-pad multiply (model.py:312-328).
// keep = false (decoding): nothing is saved for a backward (LayerNorm inputs and statistics,
// attention probabilities); the launches are the same
void capgen_engine::enc_layer_fwd(const EncLayerOff& w, EncAct& A, const void* X, void* Xout, int B, int N, const uint8_t* valid,
    int layer, bool drop_on, hipStream_t s, bool keep) {
  const int Me = B * N, d = L.d;
  const AttnGeom g = enc_self_geom(A, B, N, valid, layer, drop_on);
  self_attention(X, w.Wqkv, Me, d, g, A.qkv, A.att, keep && keep_probs(g) ? A.P : nullptr, s);
  linear_ln(A.att, d, w.Wo, d, Me, d, d, ln_fwd(enc_ln1_site(w, A, Me, layer, drop_on), a.tmp, X, A.Y, keep), s);
  linear(A.Y, d, w.W1, d, A.H, L.fe, act, Me, L.fe, d, P(w.b1), 1, s);
  linear_ln(A.H, L.fe, w.W2, L.fe, Me, d, L.fe,
            ln_fwd(enc_ln2_site(w, A, Me, valid, layer, drop_on), a.tmp, A.Y, Xout, keep), s);
}

// the region embedding and the shared norm (model.py:294): a.Aenc -> a.X[0]; keep as above
void capgen_engine::enc_embed_fwd(int Me, bool keep, hipStream_t s) {
  linear_ln(a.Aenc, L.Kp, L.enc_emb_W, L.Kp, Me, L.d, L.Kp, ln_fwd(enc_embed_site(Me), a.tmp, nullptr, a.X[0], keep), s);
}

// split_image_objects (model.py:258-292, then the shared norm :294): a.Aenc -> a.X[0]
void capgen_engine::image_objects_fwd(int B, int N, bool drop_on, hipStream_t s) {
  const int Me = B * N, d = L.d;
  // LN([feats | pos] . W^T) per token; the pair rows only repeat rows, so embed each region once
  linear_ln(a.Aenc, L.Kp, L.enc_emb_W, L.Kp, Me, d, L.Kp, ln_fwd(enc_embed_site(Me), a.tmp, nullptr, a.siY), s);
  // the position embedding alone (added to the region token after the image block): the
  // position columns [F, Kp) of the packed input and weight (zero beyond F + P)
  linear(at(a.Aenc, L.F), L.Kp, L.enc_emb_W + L.F, L.Kp, a.siEp, d, act, Me, d, L.Kp - L.F, nullptr, 0, s);
  pair_gather(a.siY, a.valid, B, N, d, a.siX2, a.siValid, act, s);
  enc_layer_fwd(L.img, a.si, a.siX2, a.siZ, Me, 2, a.siValid, kImgLayer, drop_on, s);
  pair_take_add(a.siZ, a.siEp, Me, d, a.tmp, act, s);
  lnf(ln_fwd(img_norm2_site(Me), a.tmp, nullptr, a.X[0]), s);
}

// move_first_image_feature (model.py:451-457): y = LN(x + drop(W2 relu(W1 (x + enc[:, 0]) + b1) + b2))
// over the M decoder rows in x (row r -> image r / rows_per_img, or r % bmod); keep = false
// (decoding): dropout off, nothing saved
void capgen_engine::move_first_fwd(const void* x, const void* enc, int M, int rows_per_img, int bmod, int N, void* U, void* H,
    void* tmp, void* y, bool keep, bool drop_on, hipStream_t s) {
  const int dd = L.dd;
  add_first_region(x, enc, M, rows_per_img, bmod, N, dd, U, act, s);
  linear(U, dd, L.mf_W1, dd, H, L.fd, act, M, L.fd, dd, P(L.mf_b1), 1, s);
  linear_ln(H, L.fd, L.mf_W2, L.fd, M, dd, L.fd, ln_fwd(move_first_site(M, drop_on), tmp, x, y, keep), s);
}

// forward (model.py:79-98).  Always keeps the activations needed by backward.
void capgen_engine::forward(const void* feats, DType ft, const float* pos, const int32_t* caps, int B, int N, int T,
    float* loss_out, bool drop_on, hipStream_t s, bool defer_loss) {
  const bool defer = defer_loss && loss_deferrable();
  require(B >= 1 && N >= 1 && T >= 2, "forward: need B>=1, N>=1, T>=2");
  require(N <= 64 && T - 1 <= L.maxlen - 1, "forward: N must be <= 64 and T <= max_length");
  const int Lq = T - 1, Me = B * N, Md = B * Lq, d = L.d, dd = L.dd;
  fB = B, fN = N, fT = T, fwd_drop = drop_on;
  stamp_next = 0;

  // (+ the dropout seed advance when dropout is on: the pack kernel does not read the seed, every
  // dropout site of this forward runs after this launch)
  pack_encoder_input(feats, ft, pos, Me, L.F, L.P, L.Kp, a.Aenc, act, a.valid, s, in.idx, N, in.n_img,
                     drop_on ? seed : nullptr);
  // caption ids / targets / count: with the decoder front on es2 (and no count all-reduce, which
  // stays on the critical stream) the prep runs there too, first thing of the front
  const bool caps_front = overlap_front && es2 != s && !comm;
  if (!caps_front) prepare_captions(caps, B, T, cfg.pad_idx, a.ids, a.tgt, a.count, s, nullptr, defer ? a.grad_scale : nullptr);
  if (comm && !in.score) {  // (scoring is rank-local: no collective, and the count is not read)
    if (count_override) {
      if (hz::active()) hz::op(s, "count_copy", {hz::wr(a.count, 4)});
      CAPGEN_HIP(hipMemcpyAsync(a.count, count_host, sizeof(float), hipMemcpyHostToDevice, s));
      hz::record(ev_count, s);  // capgen_dp_set_global_count waits for this copy
    }
    else {
      nccl_op(s, "allreduce(count)", a.count, 4);
      NCCL_CHECK(ncclAllReduce(a.count, a.count, 1, ncclFloat, ncclSum, comm, s));
    }
  }

  // ---- decoder front (model.py:432-436 and block 0's self-attention half + cross query,
  // modules.py:185-197): depends on the captions only, so with overlap_front it runs on es2
  // beside the whole encoder and joins before block 0's cross attention
  const bool front = overlap_front && es2 != s;
  auto dec_embed = [&](void* tmp, hipStream_t fs) {
    embedding_gather(P(L.emb), a.ids, 1, Md, L.dwe, a.E, act, fs, L.V);
    LnFwd ln = ln_fwd(dec_embed_site(Md), tmp, nullptr, a.D[0]);
    ln.pe = pe, ln.pe_L = Lq;
    linear_ln(a.E, L.dwe, L.Wel, L.dwe, Md, dd, L.dwe, ln, fs);
  };
  // self attention, then the cross-attention query
  // q_proj: also the cross-attention query projection (else the fused cross-attention launch does it)
  auto dec_self_half = [&](int l, void* tmp, hipStream_t fs, bool q_proj) {
    const auto& w = L.dec[l];
    auto& A = a.dec[l];
    const AttnGeom g = dec_self_geom(l, B, Lq, drop_on);
    self_attention(a.D[l], w.Wqkv, Md, dd, g, A.qkv, A.atts, keep_probs(g) ? A.Ps : nullptr, fs);
    linear_ln(A.atts, dd, w.Wo_s, dd, Md, dd, dd, ln_fwd(dec_self_site(l, Md, drop_on), tmp, a.D[l], A.D1), fs);
    if (q_proj) linear(A.D1, dd, w.Wq_c, dd, A.qc, dd, act, Md, dd, dd, nullptr, 0, fs);
  };
  if (front) {
    dep(s, es2, ev_ff);
    if (caps_front) prepare_captions(caps, B, T, cfg.pad_idx, a.ids, a.tgt, a.count, es2, nullptr, defer ? a.grad_scale : nullptr);
    dec_embed(a.tmpf, es2);
    dec_self_half(0, a.tmpf, es2, true);
    hz::record(ev_fj, es2);
  }

  // ---- encoder (model.py:294-332) ----
  if (L.has_img) image_objects_fwd(B, N, drop_on, s);
  else enc_embed_fwd(Me, /*keep=*/true, s);
  // where the critical stream joins the decoder front (eager / single graph): before encoder block
  // front_join (Le + 1: before the decoder, its first reader)
  const int fj = std::max(0, std::min(front_join, L.Le + 1));
  for (int l = 0; l < L.Le; ++l) {
    if (front && l == fj) hz::wait(s, ev_fj);
    enc_layer_fwd(L.enc[l], a.enc[l], a.X[l], a.X[l + 1], B, N, cfg.encode_mask ? a.valid : nullptr, l, drop_on, s);
  }
  if (front && fj == L.Le) hz::wait(s, ev_fj);
  // cross-attention K/V of every decoder block in one GEMM over the encoder output
  linear(a.X[L.Le], d, L.Wkv_all, d, a.KV, (int64_t)L.Ld * 2 * dd, act, Me, L.Ld * 2 * dd, d, nullptr, 0, s);

  // ---- decoder (model.py:419-459) ----
  if (front && fj > L.Le) hz::wait(s, ev_fj);
  else if (!front) dec_embed(a.tmp, s);
  for (int l = 0; l < L.Ld; ++l) {
    const auto& w = L.dec[l];
    auto& A = a.dec[l];
    const bool q_done = front && l == 0;  // block 0's query was projected on es2 with the front
    if (!q_done) dec_self_half(l, a.tmp, s, !cross_fusable(Lq));
    // cross attention over the encoder output
    const AttnGeom c = dec_cross_geom(l, B, Lq, N, drop_on);
    cross_attention(c, A.D1, w.Wq_c, dd, A.qc, A.attc, keep_probs(c) ? A.Pc : nullptr, q_done || !cross_fusable(Lq), s);
    linear_ln(A.attc, dd, w.Wo_c, dd, Md, dd, dd, ln_fwd(dec_cross_site(l, Md, drop_on), a.tmp, A.D1, A.D2), s);
    // FFN
    linear(A.D2, dd, w.W1, dd, A.H, L.fd, act, Md, L.fd, dd, P(w.b1), 1, s);
    linear_ln(A.H, L.fd, w.W2, L.fd, Md, dd, L.fd, ln_fwd(dec_ffn_site(l, Md, drop_on), a.tmp, A.D2, a.D[l + 1]), s);
  }
  if (L.has_mf)
    move_first_fwd(a.D[L.Ld], a.X[L.Le], Md, Lq, 0, N, a.mfU, a.mfH, a.tmp, a.mfOut, /*keep=*/true, drop_on, s);
  // ---- classifier + CE (model.py:93-96) ----
  // score mode (capgen_score_captions): the same classifier, then a read-out that writes B + Md numbers
  // in place of the CE rows -- no softmax - onehot, no loss word, no gradient scale, no collective
  require(!in.score || (!drop_on && !defer), "forward: score mode runs without dropout and writes no loss");
  if (fused_ce()) {
    // the logits are never written: the GEMM epilogue leaves exp(v - slab max) + slab stats,
    // ce_finish turns them into the loss rows and softmax - onehot (model.py:93-96)
    GemmArgs ga;
    ga.M = Md, ga.N = L.V, ga.K = dd, ga.A = dec_out(), ga.lda = dd, ga.B = W(L.Wc), ga.ldb = dd;
    ga.C = a.dlogits, ga.ldc = L.V, ga.bias = P(L.bc), ga.prio = prio(s);
    ga.ce_stats = a.ce_stats, ga.ce_ld = (L.V + 15) / 16, ga.ce_tgt = a.tgt, ga.ce_tlogit = a.ce_tl;
    if (stamp_on) ga.stamp = stamp(s, "gemm classifier+CE " + dims(Md, L.V, dd));
    gemm(ga, act, act, false, false, s);
    if (in.score)
      score_finish(a.ce_stats, (L.V + 15) / 16, a.ce_tl, a.tgt, Md, L.V, cfg.pad_idx, Lq, in.s_tok, nullptr,
                   in.s_logp, in.s_len, in.s_hits, s);
    else
      ce_finish(a.ce_stats, (L.V + 15) / 16, a.ce_tl, a.tgt, Md, L.V, cfg.pad_idx, a.loss_row,
                reinterpret_cast<bf16*>(a.dlogits), s, in.w, Lq);
  } else {
    linear(dec_out(), dd, L.Wc, dd, a.logits, L.V, DType::F32, Md, L.V, dd, P(L.bc), 0, s);
    if (in.score)
      score_rows(a.logits, a.tgt, Md, L.V, cfg.pad_idx, Lq, in.s_tok ? in.s_tok : a.sc_tok, a.sc_hit, in.s_logp,
                 in.s_len, in.s_hits, s);
    else
      cross_entropy_rows(a.logits, a.tgt, Md, L.V, cfg.pad_idx, a.loss_row, a.dlogits, act, s, in.w, Lq);
  }
  if (in.score) {
    stamp_fwd_end = stamp_next;
    return;
  }
  float* lo = loss_out ? loss_out : a.loss;
  last_loss = lo;
  if (comm) {
    // data parallel: the mean CE over the GLOBAL batch (model.py:76) is the sum of the ranks'
    // partial sums / global count -- one 4-byte all-reduce, then the (Focal) loss and the
    // gradient scale from it on every rank (FocalLoss transforms the global mean, loss.py:20-28)
    loss_finalize(a.loss_row, Md, a.count, 0, a.loss_ce, nullptr, s, nullptr, /*partial=*/1);
    nccl_op(s, "allreduce(ce)", a.loss_ce, 4);
    NCCL_CHECK(ncclAllReduce(a.loss_ce, a.loss_ce, 1, ncclFloat, ncclSum, comm, s));
    loss_finalize(nullptr, 0, a.count, cfg.focal_loss, lo, a.grad_scale, s, a.loss_ce);
  } else if (!defer) {
    loss_finalize(a.loss_row, Md, a.count, cfg.focal_loss, lo, a.grad_scale, s);
  }
  stamp_fwd_end = stamp_next;
}

// capgen_copy_logits (test hook): the f32 logits [fB * (fT - 1), V] of the last forward
void capgen_engine::copy_logits(float* dst, int64_t n, hipStream_t cs) {
  require(fB > 0, "copy_logits: no forward yet");
  const int64_t want = (int64_t)fB * (fT - 1) * L.V;
  require(n == want, "copy_logits: size mismatch");
  enter(cs);
  if (fused_ce())  // the fused step never writes the logits: recompute them
    linear(dec_out(), L.dd, L.Wc, L.dd, a.logits, L.V, DType::F32, fB * (fT - 1), L.V, L.dd, P(L.bc), 0, es);
  CAPGEN_HIP(hipMemcpyAsync(dst, a.logits, n * 4, hipMemcpyDeviceToDevice, es));
  leave(cs);
}

// capgen_debug_copy_buffer's selector: the workspace buffer number `which` (null: no such number)
void* capgen_engine::debug_buffer(int which) const {
  const int Le = L.Le;
  void* src = which == 0 ? a.tmp : which == 1 ? a.gOut : which == 2 ? a.gRes : which == 3 ? a.gKV
            : which == 4 ? a.genc[Le - 1].gH : which == 5 ? a.genc[Le - 1].gAf
            : which == 6 ? a.genc[Le - 1].gA1 : which == 7 ? a.genc[Le - 1].gQKV
            // 32 + 8 l + j: encoder block l's per-block gradient buffers (never overwritten later in
            // the backward): j = 0 gAf, 1 gH, 2 gA1, 3 gATT1, 4 gQKV
            : which >= 32 && (which - 32) / 8 < Le && (which - 32) % 8 < 5
                ? (&a.genc[(which - 32) / 8].gAf)[(which - 32) % 8 == 0 ? 0 : (which - 32) % 8 == 1 ? 1
                                                      : (which - 32) % 8 == 2 ? 2 : (which - 32) % 8 == 3 ? 3 : 4]
            // 80 + l: the forward's encoder activations X[l] (l = 0 .. Le: embedding output .. encoder output)
            : which >= 80 && which - 80 <= Le ? a.X[which - 80]
            // 128 + 8 l + j: encoder block l's saved forward tensors: j = 0 att, 1 v1, 2 m1, 3 r1, 4 Y,
            // 5 v2, 6 m2, 7 r2
            : which >= 128 && (which - 128) / 8 < Le
                ? ((which - 128) % 8 == 0 ? a.enc[(which - 128) / 8].att
                   : (which - 128) % 8 == 1 ? a.enc[(which - 128) / 8].v1
                   : (which - 128) % 8 == 2 ? (void*)a.enc[(which - 128) / 8].m1
                   : (which - 128) % 8 == 3 ? (void*)a.enc[(which - 128) / 8].r1
                   : (which - 128) % 8 == 4 ? a.enc[(which - 128) / 8].Y
                   : (which - 128) % 8 == 5 ? a.enc[(which - 128) / 8].v2
                   : (which - 128) % 8 == 6 ? (void*)a.enc[(which - 128) / 8].m2
                                           : (void*)a.enc[(which - 128) / 8].r2)
            // 200 + l / 216 + l: encoder / decoder block l's FFN hidden activations relu(x W1^T + b1)
            // (the ReLU mask the backward applies)
            : which >= 200 && which - 200 < Le ? a.enc[which - 200].H
            : which >= 216 && which - 216 < L.Ld ? a.dec[which - 216].H
                : nullptr;
  return src;
}
