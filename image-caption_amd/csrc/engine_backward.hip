// capgen engine -- the backward pass: the hand-ordered gradient launches on the critical stream, the
// weight-gradient queue of the side stream, and the points where the parameter buckets are handed over.
#include "engine.h"

void capgen_engine::join(hipStream_t s) {
  flush(s);
  if (!dbg_drop_join) dep(es2, s, ev_join);
}

// run weight-gradient jobs on stream st now: in bf16 mode as grouped launches (every dW tile
// of a block in one grid: better chip fill than 4-6 small launches, tools/dw_variant_probe.sh)
void capgen_engine::dw_launch(const DwJob* jobs, size_t n, hipStream_t st) {
  if (act == DType::BF16 && group_dw) {
    std::vector<GemmArgs> probs;
    for (size_t i = 0; i < n; ++i) probs.push_back(dw_args(jobs[i]));
    for (size_t i = 0; i < n; i += kMaxGroup) {
      if (stamp_on) probs[i].stamp = stamp(st, "gemm dW group of " + std::to_string(std::min<size_t>(kMaxGroup, n - i)));
      gemm_grouped(probs.data() + i, (int)std::min<size_t>(kMaxGroup, n - i), DType::F32, true, true, st);
    }
  } else {
    for (size_t i = 0; i < n; ++i) {
      const DwJob& j = jobs[i];
      linear_dw(j.dY, j.ldy, j.X, j.ldx, j.goff, j.ldg, j.M, j.N, j.K, j.alpha_ptr, st);
    }
  }
}

// es2 waits for everything issued on s so far, then runs the queued weight-gradient GEMMs
void capgen_engine::flush(hipStream_t s) {
  fork(s);
  dw_launch(dw_pending.data(), dw_pending.size(), es2);
  dw_pending.clear();
  for (const ColJob& j : col_pending) column_sum(j.X, j.M, j.N, j.N, 1.f, nullptr, j.db, act, es2, NSTRIPE, n_small);
  col_pending.clear();
}

// lb = the block's LayerNorm backward (dy = grad wrt block output, d_res -> r_out, d_a -> gA);
// X = block input, H = hidden activations.
void capgen_engine::ffn_bwd(int M, int d, int f, const LnBwd& lb, const void* X, const void* H, int64_t W1, int64_t b1, int64_t W2,
    void* gH, hipStream_t s) {
  lnb(lb, s);
  void* gA = lb.d_a;
  dw_side(gA, d, H, f, W2, f, M, d, f, nullptr, s);
  const bool side = colsum_side && es2 != s;
  linear_dx(gA, d, W2, f, gH, f, M, d, f, 0, H, nullptr, s, side ? nullptr : GS(b1));  // x relu'(H)
  if (side) col_pending.push_back(ColJob{gH, M, f, GS(b1)});                           // db1 = colsum
  dw_side(gH, f, X, d, W1, d, M, f, d, nullptr, s);
  linear_dx(gH, f, W1, d, lb.d_res, d, M, f, d, 1, nullptr, nullptr, s);
}

// MHA output projection + LayerNorm backward: lb as above (d_res = grad wrt the residual /
// query input); writes grad wrt the attention output into gATT.
void capgen_engine::mha_out_bwd(int M, int d, const LnBwd& lb, const void* att, int64_t Wo, void* gATT, hipStream_t s) {
  lnb(lb, s);
  dw_side(lb.d_a, d, att, d, Wo, d, M, d, d, nullptr, s);
  linear_dx(lb.d_a, d, Wo, d, gATT, d, M, d, d, 0, nullptr, nullptr, s);
}

// ... followed by the attention backward of g: in bf16 with the tiled Wo^T, the projection's input
// gradient (dO = dA . Wo, dA = lb.d_a) runs INSIDE the attention backward launch (qkv_attn_bwd):
// one launch and one dependent boundary fewer per attention block (CAPGEN_FUSED_ATTN_BWD=0: the
// dX GEMM into gATT and the attention backward launch)
void capgen_engine::mha_bwd(int M, int d, const LnBwd& lb, const void* att, int64_t Wo, void* gATT, const AttnGeom& g,
    const float* probs, void* dq, void* dk, void* dv, hipStream_t s) {
  if (fused_attn_bwd_on && act == DType::BF16 && WTo(Wo) && attention_mfma_ok(g)) {
    QkvBwd qb;
    qb.g = g, qb.g.prio = prio(s);
    qb.dA = reinterpret_cast<const bf16*>(lb.d_a), qb.ldda = d, qb.Wt = WTo(Wo);
    qb.dq = reinterpret_cast<bf16*>(dq), qb.dk = reinterpret_cast<bf16*>(dk), qb.dv = reinterpret_cast<bf16*>(dv);
    if (qkv_bwd_ok(qb)) {
      lnb(lb, s);
      dw_side(lb.d_a, d, att, d, Wo, d, M, d, d, nullptr, s);
      if (stamp_on) qb.g.stamp = stamp(s, "attn_bwd_wo " + std::to_string(g.Lq) + "x" + std::to_string(g.Lk));
      qkv_attn_bwd(qb, s);
      return;
    }
  }
  mha_out_bwd(M, d, lb, att, Wo, gATT, s);
  attb(g, probs, gATT, dq, dk, dv, act, s);
}

// backward of enc_layer_fwd: gO = grad wrt Xout on entry, grad wrt X on exit; gR scratch
void capgen_engine::enc_layer_bwd(const EncLayerOff& w, EncAct& A, Acts::GradBufs& gb, const void* X, int B, int N,
    const uint8_t* valid, int layer, bool on, void* gO, void* gR, hipStream_t s) {
  const int Me = B * N, d = L.d;
  const LnBwd lffn = ln_bwd(enc_ln2_site(w, A, Me, valid, layer, on), gO, gR, gb.gAf);
  const LnBwd lmha = ln_bwd(enc_ln1_site(w, A, Me, layer, on), gR, gO, gb.gA1);
  ffn_bwd(Me, d, L.fe, lffn, A.Y, A.H, w.W1, w.b1, w.W2, gb.gH, s);  // gR = grad wrt Y
  mha_bwd(Me, d, lmha, A.att, w.Wo, gb.gATT1, enc_self_geom(A, B, N, valid, layer, on), A.P, gb.gQKV,
          at(gb.gQKV, d), at(gb.gQKV, 2 * d), s);
  dw_side(gb.gQKV, 3 * d, X, d, w.Wqkv, d, Me, 3 * d, d, nullptr, s);
  linear_dx(gb.gQKV, 3 * d, w.Wqkv, d, gO, d, Me, 3 * d, d, 1, nullptr, nullptr, s);  // gO = grad wrt X
}

// backward of image_objects_fwd: gX0 = grad wrt a.X[0] -> embedding weight gradient
void capgen_engine::image_objects_bwd(const void* gX0, int B, int N, bool on, hipStream_t s) {
  const int Me = B * N, d = L.d;
  // second norm: grad wrt Z[2r+1] + Ep[r] (no residual, no dropout)
  lnb(ln_bwd(img_norm2_site(Me), gX0, nullptr, a.siGEp), s);
  pair_scatter(a.siGEp, Me, d, a.siG0, act, s);  // only the region token's output is kept
  enc_layer_bwd(L.img, a.si, a.gsi, a.siX2, Me, 2, a.siValid, kImgLayer, on, a.siG0, a.siG1, s);
  pair_reduce(a.siG0, B, N, d, a.siGY, act, s);  // image-row tokens fold back onto region 0
  lnb(ln_bwd(enc_embed_site(Me), a.siGY, nullptr, a.gAe), s);
  // feature columns see the first embedding only; position columns both (+ Ep after the block)
  linear_dw(a.gAe, d, a.Aenc, L.Kp, L.enc_emb_W, L.Kp, Me, d, L.F, nullptr, s);
  add_inplace(a.siGEp, a.gAe, (int64_t)Me * d, act, s);
  linear_dw(a.siGEp, d, at(a.Aenc, L.F), L.Kp, L.enc_emb_W + L.F, L.Kp, Me, d, L.Kp - L.F, nullptr, s);
}

// backward of move_first_fwd at the training shape (dy = a.gOut): a.gRes = grad wrt D[Ld]
// (residual + U), a.mfGU = grad wrt U
void capgen_engine::move_first_bwd(int Md, bool on, hipStream_t s) {
  const int dd = L.dd, fd = L.fd;
  lnb(ln_bwd(move_first_site(Md, on), a.gOut, a.gRes, a.mfGA), s);
  dw_side(a.mfGA, dd, a.mfH, fd, L.mf_W2, fd, Md, dd, fd, nullptr, s);
  linear_dx(a.mfGA, dd, L.mf_W2, fd, a.mfGH, fd, Md, dd, fd, 0, a.mfH, nullptr, s, GS(L.mf_b1));
  dw_side(a.mfGH, fd, a.mfU, dd, L.mf_W1, dd, Md, fd, dd, nullptr, s);
  linear_dx(a.mfGH, fd, L.mf_W1, dd, a.mfGU, dd, Md, fd, dd, 0, nullptr, nullptr, s);
  add_inplace(a.gRes, a.mfGU, (int64_t)Md * dd, act, s);
}

// step_params: bucketed all-reduce + Adam (see bucket()); otherwise gradients only
void capgen_engine::backward(hipStream_t s, bool step_params) {
  bstep = step_params;
  require(fB > 0, "backward: call forward first");
  grads_sharded = false;
  stamp_next = stamp_fwd_end;
  const int B = fB, N = fN, Lq = fT - 1, Me = B * N, Md = B * Lq, d = L.d, dd = L.dd;
  const bool on = fwd_drop;
  // the striped LN/bias partials start at 0 (the critical stream's first LayerNorm backward adds
  // into them); the accumulated word-embedding gradient (20 MB at C2) is zeroed on es2 after the
  // fork below -- its only writer is the embedding scatter on es2
  const bool emb_zero_side = es2 != s && !L.has_img && !L.has_mf;
  if (!emb_zero_side) memset_async(grads + L.n_dense, (L.enc_lng - L.n_dense) * sizeof(float), s);
  // the striped partials are cleared by the previous backward's folds (stripe_reduce(clear)); a
  // backward that did not reach both folds (diagnostic stops, errors) leaves them marked dirty
  if (stripes_dirty || !stripe_clear) memset_async(gstripe, (size_t)NSTRIPE * n_small * sizeof(float), s);
  stripes_dirty = true;
  int folds = 0;
  if (bstep) {
    // the step counter / bias corrections only feed the bucket stream's Adam: issue them there
    // (off the critical stream) unless the step is being captured (ec joins a capture only
    // through the buckets' events)
    hipStreamCaptureStatus cst = hipStreamCaptureStatusNone;
    CAPGEN_HIP(hipStreamIsCapturing(s, &cst));
    adam_prepare(step, opt, cfg.beta1, cfg.beta2, adam_scal, cst == hipStreamCaptureStatusNone ? ec : s, wd_word());
    if (ema_on() && cst == hipStreamCaptureStatusNone) ++ema_updates;  // (a replay is counted where it launches)
    zbuckets.clear();
    gn_deferred.clear();
    gn_slots = 0;
  }

  // classifier: dlogits are unscaled (softmax - onehot); grad_scale folds 1/count (+focal).  The
  // critical stream goes straight from the forward into the dX GEMM: the side work (weight and bias
  // gradients, the embedding-gradient clear, a deferred loss finalisation) forks after it, with the
  // flush the classifier's bucket needs anyway (one event record on the critical stream, not two)
  dw_side(a.dlogits, L.V, dec_out(), dd, L.Wc, dd, Md, L.V, dd, a.grad_scale, s);
  linear_dx(a.dlogits, L.V, L.Wc, dd, a.gOut, dd, Md, L.V, dd, 0, nullptr, a.grad_scale, s);
  flush(s);  // es2: the classifier dW (the bucket below waits for it: it reads Wc's gradient)
  bucket(L.Wc, L.n_dense - L.Wc, s, /*sync=*/false);
  if (emb_zero_side) memset_async(grads + L.n_dense, (L.enc_lng - L.n_dense) * sizeof(float), es2);
  column_sum(a.dlogits, Md, L.V, L.V, 1.f, a.grad_scale, GS(L.bc), act, es2, NSTRIPE, n_small);
  if (pending_loss) {  // the mean CE (model.py:96); grad_scale was written by the caption prep
    loss_finalize(a.loss_row, Md, a.count, 0, pending_loss, nullptr, es2);
    pending_loss = nullptr;
  }

  const int64_t kvld = (int64_t)L.Ld * 2 * dd;
  void* gO = a.gOut;
  void* gR = a.gRes;
  if (L.has_mf) {  // gRes = grad wrt D[Ld]; a.mfGU = grad wrt U (its encoder part is added below)
    move_first_bwd(Md, on, s);
    std::swap(gO, gR);
  }
  for (int l = L.Ld - 1; l >= 0; --l) {
    const auto& w = L.dec[l];
    auto& A = a.dec[l];
    auto& gb = a.gdec[l];
    const LnBwd lffn = ln_bwd(dec_ffn_site(l, Md, on), gO, gR, gb.gAf);
    const LnBwd lcross = ln_bwd(dec_cross_site(l, Md, on), gR, gO, gb.gA2);
    const LnBwd lself = ln_bwd(dec_self_site(l, Md, on), gO, gR, gb.gA1);
    ffn_bwd(Md, dd, L.fd, lffn, A.D2, A.H, w.W1, w.b1, w.W2, gb.gH, s);  // gR = grad wrt D2
    // (lcross.d_res = grad wrt D1, the residual part)
    mha_bwd(Md, dd, lcross, A.attc, w.Wo_c, gb.gATT2, dec_cross_geom(l, B, Lq, N, on), A.Pc, gb.gQc,
            at(a.gKV, (int64_t)l * 2 * dd), at(a.gKV, (int64_t)l * 2 * dd + dd), s);
    // block 0: the rest of the block runs on es2 (ov), the encoder chain starts on s below
    const bool ov = l == 0 && overlap_dec0 && es2 != s;
    const hipStream_t hs = ov ? es2 : s;
    if (ov) flush(s);  // es2 waits for block 0's cross-attention backward; queued dW issued
    dw_side(gb.gQc, dd, A.D1, dd, w.Wq_c, dd, Md, dd, dd, nullptr, hs);
    linear_dx(gb.gQc, dd, w.Wq_c, dd, gO, dd, Md, dd, dd, 1, nullptr, nullptr, hs);  // gO = grad wrt D1
    // (lself.d_res = grad wrt D_l, the residual part)
    mha_bwd(Md, dd, lself, A.atts, w.Wo_s, gb.gATT1, dec_self_geom(l, B, Lq, on), A.Ps, gb.gQKV, at(gb.gQKV, dd),
            at(gb.gQKV, 2 * dd), hs);
    dw_side(gb.gQKV, 3 * dd, a.D[l], dd, w.Wqkv, dd, Md, 3 * dd, dd, nullptr, hs);
    linear_dx(gb.gQKV, 3 * dd, w.Wqkv, dd, gR, dd, Md, 3 * dd, dd, 1, nullptr, nullptr, hs);
    if (l % bucket_blocks == 0)  // blocks l .. l + bucket_blocks - 1 (contiguous in the arena)
      bucket(w.Wqkv, dec_end(std::min(l + bucket_blocks - 1, L.Ld - 1)) - w.Wqkv, hs);
    if (ov) dec0_on_side = true;
    std::swap(gO, gR);  // gO = grad wrt D_l
  }
  // cross K/V of all decoder blocks -> encoder output (the encoder chain starts here; the
  // Wkv_all weight gradient is queued after the dX GEMM below, which reads Wkv_all)
  // the buffer gO is not using -- or, with block 0 finishing on es2 (both in use there), gEnc
  void* eO = dec0_on_side ? a.gEnc : gO == a.gOut ? a.gRes : a.gOut;
  dec0_on_side = false;
  // decoder embedding: LN(E.Wel^T + PE) (model.py:432-436) -- off the critical path
  {
    const LnBwd lb = ln_bwd(dec_embed_site(Md), gO, nullptr, a.gAd);
    flush(s);
    lnb(lb, es2);
    linear_dx(a.gAd, dd, L.Wel, L.dwe, a.gE, L.dwe, Md, dd, L.dwe, 0, nullptr, nullptr, es2);
    const DwJob wel{a.gAd, a.E, dd, L.dwe, L.Wel, L.dwe, Md, dd, L.dwe, nullptr};
    dw_launch(&wel, 1, es2);
    embedding_scatter_add(a.gE, a.ids, Md, L.dwe, cfg.pad_idx, G(L.emb), act, es2, L.V);
    // every decoder-side gradient is final here (in es2 order, after the fork above)
    stripe_reduce(GS(L.dec_lng), NSTRIPE, n_small, L.total - L.dec_lng, G(L.dec_lng), 0, es2, stripe_clear);
    ++folds;
  }
  // the encoder chain must not overwrite gO (read by the decoder-embedding branch on es2):
  // it runs on the other residual buffer and on tmp (free during backward)
  gO = eO;
  gR = a.tmp;
  linear_dx(a.gKV, kvld, L.Wkv_all, d, gO, d, Me, L.Ld * 2 * dd, d, 0, nullptr, nullptr, s);
  if (L.has_mf) first_region_grad(a.mfGU, B, Lq, N, d, gO, act, s);  // enc[:, 0] of U = D + enc[:, 0]
  dw_side(a.gKV, kvld, a.X[L.Le], d, L.Wkv_all, d, Me, L.Ld * 2 * dd, d, nullptr, s);
  // the decoder-embedding branch (es2) has been issued: every decoder-side gradient is final
  // the flush of the first bucket follows the dX GEMM above (it reads Wkv_all); es2 then holds
  // every producer of the other three buckets
  bucket(L.Wkv_all, L.Wc - L.Wkv_all, s);               // cross K/V of all decoder blocks
  bucket(L.Wel, L.dec[0].Wqkv - L.Wel, s, false);       // word-embedding projection
  bucket(L.emb, L.enc_lng - L.emb, s, false);           // word embedding table
  bucket(L.dec_lng, L.total - L.dec_lng, s, false);     // decoder LN / biases, classifier bias
  for (int l = L.Le - 1; l >= 0; --l) {
    const auto& w = L.enc[l];
    enc_layer_bwd(w, a.enc[l], a.genc[l], a.X[l], B, N, cfg.encode_mask ? a.valid : nullptr, l, on, gO, gR, s);
    if (l % bucket_blocks == 0) bucket(w.Wqkv, enc_end(std::min(l + bucket_blocks - 1, L.Le - 1)) - w.Wqkv, s);
  }
  // the tail of the step's dependency chain: the encoder-embedding LayerNorm backward and
  // weight gradient, then its Adam, which the next forward's first GEMM needs -- on the
  // critical stream, so it does not queue behind the weight-gradient groups still on es2
  // (a single GEMM: the plain launch with its autotuned split-K, K = B*N = 2304 deep)
  if (L.has_img) {
    image_objects_bwd(gO, B, N, on, s);
    flush(s);  // the image block's weight gradients share the embedding bucket
  } else {
    lnb(ln_bwd(enc_embed_site(Me), gO, nullptr, a.gAe), s);
    linear_dw(a.gAe, d, a.Aenc, L.Kp, L.enc_emb_W, L.Kp, Me, d, L.Kp, nullptr, s);
  }
  // every encoder LayerNorm/bias partial was accumulated on s; in step mode the fold and the
  // last two buckets (feature/position embedding, encoder LN / biases) run on the bucket
  // stream behind ONE event (each event record costs the critical stream ~5 us)
  const hipStream_t tail = bstep ? ec : s;
  if (!bstep) join(s);  // queued bias column sums (es2) precede the fold below
  if (bstep) dep(s, ec, ev_b1);
  if (bstep && L.has_img) dep(es2, ec, ev_b2);
  stripe_reduce(GS(L.enc_lng), NSTRIPE, n_small, L.dec_lng - L.enc_lng, G(L.enc_lng), 0, tail, stripe_clear);
  if (++folds == 2) stripes_dirty = false;
  if (bstep) {
    bucket_update(0, L.enc[0].Wqkv, tail_grid);                   // feature/position embedding
    bucket_update(L.enc_lng, L.dec_lng - L.enc_lng, tail_grid);   // encoder LN / biases
    if (clip_on()) clip_tail();
  }
  join(s);
  if (bstep) {
    dep(ec, s, ev_cj);
    bstep = false;
    check_buckets();
  }
}

//@NEW
