// capgen engine -- decoding (model.py:101-200), KV-cached: the decode tiles and workspace, the
// per-position decoder step, greedy, beam, beam_nbest and sample, the decode constraints, and ensemble decoding.
#include "abi_util.h"
#include "engine.h"

std::vector<std::array<int64_t, 3>> capgen_engine::dtile_list() const {  // {arena offset, rows N, columns K}
  std::vector<std::array<int64_t, 3>> v;
  v.push_back({L.Wel, L.dd, L.dwe});
  for (const auto& e : L.dec)
    v.push_back({e.Wo_s, L.dd, L.dd}), v.push_back({e.Wo_c, L.dd, L.dd}), v.push_back({e.W1, L.fd, L.dd}),
        v.push_back({e.W2, L.dd, L.fd});
  return v;
}

void capgen_engine::ensure_dtiles() {  // (outside any capture)
  if (dtiles_init || !breg_decode()) return;
  dtiles_init = true;
  int64_t tot = 0;
  for (const auto& t : dtile_list())
    if (t[1] % 16 == 0 && t[2] % 32 == 0) dtile[t[0]] = tot, tot += t[1] * t[2];
  if (tot) CAPGEN_HIP(hipMalloc(&dtiles, (size_t)tot * 2));
#ifndef CAPGEN_NO_GATHER_FOLD
  // only the tiled word-embedding projection reads the bf16 table
  if (L.dwe % 8 == 0 && dtile.count(L.Wel)) CAPGEN_HIP(hipMalloc(&emb_bf, (size_t)L.V * L.dwe * 2));
#endif
}

void capgen_engine::build_dtiles(hipStream_t s) {
  if (!dtiles) return;
  // skipped while the tiles match the weights (~0.12 ms per greedy / beam call)
  if (dtiles_ver == wver) return;
  dtiles_ver = wver;
  if (emb_bf) to_bf16(P(L.emb), emb_bf, (size_t)L.V * L.dwe, s);
  for (const auto& t : dtile_list()) {
    auto it = dtile.find(t[0]);
    if (it != dtile.end()) gemm_tile_b(shadow + t[0], t[2], 0, (int)t[1], (int)t[2], dtiles + it->second, s);
  }
}

// decoding (model.py:101-200), KV-cached.  Bit-identical to recomputing the prefix: row
// results of every kernel are independent of how many rows/positions are in the launch.
void capgen_engine::encode_only(const void* feats, DType ft, const float* pos, int B, int N, hipStream_t s) {
  const int Me = B * N, d = L.d;
  pack_encoder_input(feats, ft, pos, Me, L.F, L.P, L.Kp, a.Aenc, act, a.valid, s);
  if (L.has_img) image_objects_fwd(B, N, false, s);
  else enc_embed_fwd(Me, /*keep=*/false, s);
  for (int l = 0; l < L.Le; ++l)
    enc_layer_fwd(L.enc[l], a.enc[l], a.X[l], a.X[l + 1], B, N, cfg.encode_mask ? a.valid : nullptr, l, false, s,
                  /*keep=*/false);
  linear(a.X[L.Le], d, L.Wkv_all, d, a.KV, (int64_t)L.Ld * 2 * L.dd, act, Me, L.Ld * 2 * L.dd, d, nullptr, 0, s);
}

void capgen_engine::plan_gen(Planner& p, int R, int N) {
  const int64_t dd = L.dd, Tc = L.maxlen, e = es_();
  auto T_ = [&](void*& ptr, int64_t n) { ptr = p.raw(n * e); };
  T_(g.x, R * dd);
  T_(g.x1, R * dd);
  T_(g.x2, R * dd);
  T_(g.q, R * dd);
  T_(g.att, R * dd);
  T_(g.tmp, R * std::max<int64_t>(dd, L.dwe));
  T_(g.h, (int64_t)R * L.fd);
  T_(g.E, (int64_t)R * L.dwe);
  p.take(g.mean, R);
  p.take(g.rstd, R);
  p.take(g.Pc, (size_t)R * L.Hd * N);
  p.take(g.logits, (size_t)R * L.V);
  p.take(g.dstats, (size_t)R * ((L.V + 15) / 16));
  p.take(g.cand_v, (size_t)R * 16);
  p.take(g.cand_i, (size_t)R * 16);
  T_(g.cache, (int64_t)L.Ld * R * Tc * 2 * dd);
  p.take(g.ids, (size_t)R * Tc);
  p.take(g.ids2, (size_t)R * Tc);
  p.take(g.kvrow, (size_t)R * Tc);
  p.take(g.kvrow2, (size_t)R * Tc);
  p.take(g.seq, (size_t)R * Tc);
  p.take(g.seq2, (size_t)R * Tc);
  p.take(g.bprob, R);
  p.take(g.bprob2, R);
  p.take(g.bsrc, R);
  p.take(g.btok, R);
  p.take(g.bfin, R);
  p.take(g.bfin2, R);
  p.take(g.blen, R);
  p.take(g.blen2, R);
  p.take(g.bmet, R);  // (beam_forced's, behind everything else: no other array moves)
  p.take(g.bmet2, R);
  p.take(g.fcand_v, (size_t)R * 32);
  p.take(g.fcand_i, (size_t)R * 16);
}

void capgen_engine::ensure_gen(int R, int N) {
  if (gws && R <= g.R && N <= g.N) return;
  int nR = std::max(R, g.R), nN = std::max(N, g.N);
  replan(gws, [&](Planner& p) { plan_gen(p, nR, nN); });
  g.R = nR, g.N = nN;
}

// What greedy, beam_run and sample do first, for B images and R decoder rows.  The order matters: every
// allocation before anything is enqueued, the decode tiles built after the encoder has run
void capgen_engine::begin_decode(const void* feats, DType ft, const float* pos, int B, int N, int R, hipStream_t s) {
  ensure_acts(B, N, 2);
  ensure_gen(R, N);
  ensure_dtiles();
  encode_only(feats, ft, pos, B, N, s);
  build_dtiles(s);
}

// 2: every site, 1: only the cross-query site (beam's rows: 12.50-12.53 vs 12.62-12.73 ms per C4
// batch with none, profiles/r05_decode_16row_tiles.txt), 0: none
int capgen_engine::ln_fold(int M) const {
  if (!decode_ln_fold || !breg_decode() || L.dd != 512 || L.fd % 64 != 0) return 0;
  for (const auto& w : L.dec)
    if (!DT(w.Wqkv) || !DT(w.Wq_c) || !DT(w.W1)) return 0;
  return decode_ln_fold == 2 || M < 1024 ? 2 : 1;
}

// decoder for position t of R rows (rows r -> image r % Bimg); tokens = ids[:, t].
// Leaves logits [R, V] in g.logits; cross-attn probs of the last block in g.Pc if want_attn.
// bf16 decode: each decoder LayerNorm whose output feeds a register-B GEMM (the cross-query
// projection, the FFN's first Linear, the next block's QKV projection) runs inside that GEMM
// (GemmArgs::ln_gamma, gemm_breg.hip breg_ln_kernel): the consumer reads the producing Linear's
// output (bias included) and the residual, normalises the rows and its column-tile-0 workgroups
// store them as the next residual.  17 of the 19 LayerNorm launches of a token go away
// (CAPGEN_DECODE_LN_FOLD=0: separate launches).
void capgen_engine::dec_step(int R, int Bimg, int N, int t, void* cache, const int32_t* ids, bool want_attn, hipStream_t s,
    const int32_t* kv_row) {
  const int dd = L.dd, Hd = L.Hd, dkd = dd / Hd, Tc = L.maxlen;
  GemmArgs ge;  // the embedding rows gathered by the projection GEMM itself (where it takes the shape)
  ge.M = R, ge.N = dd, ge.K = L.dwe, ge.A = emb_bf, ge.lda = L.dwe, ge.B = W(L.Wel), ge.ldb = L.dwe;
  ge.C = g.tmp, ge.ldc = dd, ge.bt = DT(L.Wel), ge.prio = prio(s);
  ge.a_ids = ids + t, ge.a_ids_ld = Tc, ge.a_table_rows = L.V;
  if (emb_bf && ge.bt && gemm_breg_ok(ge)) {
    if (stamp_on) ge.stamp = stamp(s, "gemm fwd (gathered A) " + dims(R, dd, L.dwe));
    gemm(ge, act, act, false, false, s);
  } else {
    embedding_gather(P(L.emb), ids + t, Tc, R, L.dwe, g.E, act, s, L.V);
    dec_linear(g.E, L.Wel, R, dd, L.dwe, g.tmp, nullptr, 0, s);
  }
  // ln: the LayerNorm whose output g.x the next QKV projection reads: the embedding's (position t of
  // the PE table; never folded), then each block's FFN LayerNorm
  LnFwd ln = ln_fwd(dec_embed_site(R), g.tmp, nullptr, g.x, false);
  ln.pe = pe + (int64_t)t * dd, ln.pe_L = 1;
  RowMask rm{};
  rm.ids = ids + t, rm.ids_ld = Tc, rm.pad_idx = cfg.pad_idx;
  const int64_t cld = (int64_t)Tc * 2 * dd;
  // which LayerNorms run inside the GEMM that reads them: every site of a block / the cross-query site
  const int fmode = ln_fold(R);
  const bool fold = fmode == 2, fold1 = fmode >= 1;
  for (int l = 0; l < L.Ld; ++l) {
    const auto& w = L.dec[l];
    void* cl = at(cache, (int64_t)l * R * cld);
    void* kv = at(cl, (int64_t)t * 2 * dd);  // the cache at position t
    if (act == DType::BF16) {  // one GEMM: Q columns -> g.q, K/V columns -> the cache
      dec_linear(g.x, w.Wqkv, R, 3 * dd, dd, g.q, nullptr, 0, s, &ln, fold && l > 0, dd, kv, cld);
    } else {
      dec_linear(g.x, w.Wqkv, R, dd, dd, g.q, nullptr, 0, s, &ln);
      dec_linear(g.x, w.Wqkv + (int64_t)dd * dd, R, 2 * dd, dd, kv, nullptr, 0, s, nullptr, false, cld);
    }
    AttnGeom sg;
    sg.B = R, sg.H = Hd, sg.Lq = 1, sg.Lk = t + 1, sg.dk = dkd;
    sg.q = g.q, sg.q_ld = dd, sg.q_bs = dd;
    sg.k = cl, sg.k_ld = 2 * dd, sg.k_bs = cld;
    sg.v = at(cl, dd), sg.v_ld = 2 * dd, sg.v_bs = cld;
    sg.o_ld = dd, sg.o_bs = dd;
    sg.key_ids = ids, sg.kid_bs = Tc, sg.pad_idx = cfg.pad_idx, sg.causal = 1, sg.q_pos0 = t;
    sg.kv_row = kv_row, sg.kv_row_ld = Tc;
    sg.temperature = std::sqrt((float)dkd);
    attf(sg, g.att, nullptr, act, s);
    dec_linear(g.att, w.Wo_s, R, dd, dd, g.tmp, nullptr, 0, s);
    const LnFwd ls = ln_fwd(dec_self_site(l, R, false), g.tmp, g.x, g.x1, false);
    dec_linear(g.x1, w.Wq_c, R, dd, dd, g.q, nullptr, 0, s, &ls, fold1);
    const bool want_p = want_attn && l == L.Ld - 1;
    AttnGeom c = cross_kv(l, N);  // rows r -> image r % Bimg
    const int kb = R / Bimg;  // beam rows per image: row j * Bimg + b
    if (act == DType::BF16 && cross_mfma_on && !want_p && kb > 1 && R % Bimg == 0 && kb <= 64) {
      // an image's kb beam rows as ONE query block of the MFMA attention (attention_mfma.hip), one
      // workgroup per (image, head): the rows are Bimg * d apart
      c.B = Bimg, c.Lq = kb;
      c.q = g.q, c.q_ld = (int64_t)Bimg * dd, c.q_bs = dd;
      c.o_ld = (int64_t)Bimg * dd, c.o_bs = dd;
    } else {
      c.B = R, c.Lq = 1;
      c.q = g.q, c.q_ld = dd, c.q_bs = dd;
      c.kv_bmod = Bimg;
      c.o_ld = dd, c.o_bs = dd;
    }
    attf(c, g.att, want_p ? g.Pc : nullptr, act, s);
    dec_linear(g.att, w.Wo_c, R, dd, dd, g.tmp, nullptr, 0, s);
    const LnFwd lc = ln_fwd(dec_cross_site(l, R, false), g.tmp, g.x1, g.x2, false);
    dec_linear(g.x2, w.W1, R, L.fd, dd, g.h, P(w.b1), 1, s, &lc, fold);
    // b2: a GEMM that normalises its A rows adds no bias to them, so where the FFN LayerNorm folds, the
    // W2 GEMM adds b2 (also in the last block, so that every block rounds alike); else the LayerNorm does
    dec_linear(g.h, w.W2, R, dd, L.fd, g.tmp, fold ? P(w.b2) : nullptr, 0, s);
    ln = ln_fwd(dec_ffn_site(l, R, false), g.tmp, g.x2, g.x, false);
    ln.mask = rm;  // the tokens of position t, not the training captions
    if (fold) ln.a_bias = nullptr;
  }
  lnf(ln, s);  // the last block's FFN LayerNorm feeds the classifier (or move-first): its own launch
  const void* xo = g.x;
  if (L.has_mf) {  // rows r -> image r % Bimg
    move_first_fwd(g.x, a.X[L.Le], R, 1, Bimg, N, g.x2, g.h, g.tmp, g.x1, /*keep=*/false, /*drop_on=*/false, s);
    xo = g.x1;
  }
  if (slab_decode()) {  // f32 logits + per-16-column-slab {max, exp-sum} for the selection
    GemmArgs ga;
    ga.M = R, ga.N = L.V, ga.K = dd, ga.A = xo, ga.lda = dd, ga.B = W(L.Wc), ga.ldb = dd;
    ga.C = g.logits, ga.ldc = L.V, ga.bias = P(L.bc);
    ga.dec_stats = g.dstats, ga.dec_ld = (L.V + 15) / 16;
    if (stamp_on) ga.stamp = stamp(s, "gemm NT " + dims(R, L.V, dd) + " classifier+slab stats");
    gemm(ga, act, DType::F32, false, false, s);
  } else {
    linear(xo, dd, L.Wc, dd, g.logits, L.V, DType::F32, R, L.V, dd, P(L.bc), 0, s);
  }
}

void capgen_engine::greedy(const void* feats, DType ft, const float* pos, int B, int N, int64_t* ids_out, float* attn_out,
    hipStream_t s) {
  require(N >= 1 && N <= 64, "greedy: N must be in [1, 64]");
  require(B >= 1, "greedy: need B >= 1");
  begin_decode(feats, ft, pos, B, N, B, s);
  const int Tc = L.maxlen, W = L.maxlen + 1;
  init_gen_ids(ids_out, B, W, g.ids, Tc, s);
  for (int t = 0; t < L.maxlen - 1; ++t) {
    dec_step(B, B, N, t, g.cache, g.ids, attn_out != nullptr, s);
    if (attn_out) attention_head_mean(g.Pc, B, L.Hd, 1, N, 0, attn_out + (int64_t)t * B * N, s);
    if (slab_decode())  // argmax of the logits = argmax of the (log-)softmax
      slab_argmax(g.logits, g.dstats, B, L.V, ids_out, W, t + 1, g.ids + t + 1, Tc, s);
    else
      argmax_softmax(g.logits, B, L.V, ids_out, W, t + 1, g.ids + t + 1, Tc, s, decode_logsm);
  }
}

void capgen_engine::beam(const void* feats, DType ft, const float* pos, int B, int N, int k, int64_t* ids_out, hipStream_t s) {
  require(k >= 1 && k <= 16, "beam_search: beam_size must be in [1, 16]");
  require(k <= L.V, "beam_search: beam_size must be <= num_vocab");
  require(B >= 1 && N >= 1 && N <= 64, "beam_search: need B >= 1 and N in [1, 64]");
  beam_run(feats, ft, pos, B, N, k, nullptr, s);
  CAPGEN_HIP(hipMemcpyAsync(ids_out, g.seq, sizeof(int64_t) * B * L.maxlen, hipMemcpyDeviceToDevice, s));
}

// The standard beam search (definition: select.hip): a hypothesis stops at <END> (end_id; -1: never),
// finished hypotheses compete with their log-probability frozen, and the n_best of the k per image come
// back ordered by logp / len^alpha with score, logp and length.  beam's loop and launch sequence with the
// END-aware selection kernels (always the log-softmax); finished rows still run through the decoder and
// there is no early exit: nothing here waits for the device.  One more launch, beam_finish, at the end.
void capgen_engine::beam_nbest(const void* feats, DType ft, const float* pos, int B, int N, int k, int end_id, float alpha,
    int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out, hipStream_t s,
    const EnsembleRun* ens) {
  require(k >= 1 && k <= 16 && k <= L.V, "beam_nbest: beam_size must be in [1, min(16, num_vocab)]");
  require(n_best >= 1 && n_best <= k, "beam_nbest: n_best must be in [1, beam_size]");
  require(end_id >= -1 && end_id < L.V, "beam_nbest: end_id must be in [-1, num_vocab)");
  require(alpha >= 0.f && alpha < INFINITY, "beam_nbest: length_penalty must be finite and >= 0");  // (false for a NaN)
  require(N >= 1 && N <= 64, "beam_nbest: N must be in [1, 64]");
  require(B >= 1, "beam_nbest: need B >= 1");
  require(ids_out != nullptr, "beam_nbest: null ids_out");
  require(dc.min_length == 0 || dc.end_id == end_id,
          "beam_nbest: end_id differs from the end_id of the decode constraints' min_length");
  beam_run(feats, ft, pos, B, N, k, &end_id, s, ens);
  beam_finish(g.seq, g.bprob, g.blen, k, B, L.maxlen, alpha, n_best, ids_out, score_out, logp_out, len_out, s);
}

// Diverse beam search (definition: select.hip): beam_nbest's search with the k beams split into num_groups
// groups that are penalised, lambda per earlier hypothesis, for choosing the words earlier groups chose at the
// same position.  beam_run's loop with the full-row END-aware top-k, the group merge and the three reorder
// launches per token in either dtype (no fused slab form), then one beam_finish per group: n_best <= k / G of
// each, output rows (g * n_best + rank) * B + b.  One group is beam_nbest itself, fused slab step included.
void capgen_engine::beam_diverse(const void* feats, DType ft, const float* pos, int B, int N, int k, int G, float lambda,
    int end_id, float alpha, int n_best, int64_t* ids_out, float* score_out, float* logp_out, int32_t* len_out,
    hipStream_t s, const EnsembleRun* ens) {
  require(k >= 1 && k <= 16 && k <= L.V, "beam_diverse: beam_size must be in [1, min(16, num_vocab)]");
  require(G >= 1 && G <= k && k % G == 0, "beam_diverse: num_groups must be in [1, beam_size] and divide it");
  require(lambda >= 0.f && lambda < INFINITY, "beam_diverse: diversity_penalty must be finite and >= 0");  // (false for a NaN)
  const int kg = k / G;
  require(n_best >= 1 && n_best <= kg, "beam_diverse: n_best must be in [1, beam_size / num_groups]");
  require(end_id >= -1 && end_id < L.V, "beam_diverse: end_id must be in [-1, num_vocab)");
  require(alpha >= 0.f && alpha < INFINITY, "beam_diverse: length_penalty must be finite and >= 0");
  require(N >= 1 && N <= 64, "beam_diverse: N must be in [1, 64]");
  require(B >= 1, "beam_diverse: need B >= 1");
  require(ids_out != nullptr, "beam_diverse: null ids_out");
  require(dc.min_length == 0 || dc.end_id == end_id,
          "beam_diverse: end_id differs from the end_id of the decode constraints' min_length");
  if (G == 1) return beam_nbest(feats, ft, pos, B, N, k, end_id, alpha, n_best, ids_out, score_out, logp_out, len_out, s, ens);
  const BeamGroups groups{G, lambda};
  beam_run(feats, ft, pos, B, N, k, &end_id, s, ens, &groups);
  const int64_t Tw = L.maxlen, in = (int64_t)kg * B, out = (int64_t)n_best * B;  // rows per group
  for (int64_t h = 0; h < G; ++h)  // group h's hypotheses: rows h * k' * B .. of the k * B
    beam_finish(g.seq + h * in * Tw, g.bprob + h * in, g.blen + h * in, kg, B, (int)Tw, alpha, n_best,
                ids_out + h * out * Tw, score_out ? score_out + h * out : nullptr,
                logp_out ? logp_out + h * out : nullptr, len_out ? len_out + h * out : nullptr, s);
}

// Forced-word beam search (definition: select.hip): beam_nbest's search in banks by the number of word groups a
// hypothesis has met, word / group the images' W slots (device int32 [B][W]).  beam_run's loop with the full-row
// END-aware top-k (kf = min(16, k + W + 1) finalists and the W slot words' scores per row), the bank merge and
// the three reorder launches per token in either dtype (no fused slab form), then beam_finish with the bank key.
// W = 0 (no slots: word / group unread) is beam_nbest itself, fused slab step included, with met_out zeroed.
void capgen_engine::beam_forced(const void* feats, DType ft, const float* pos, int B, int N, int k, int end_id, float alpha,
    int n_best, const int32_t* word, const int32_t* group, int W, int64_t* ids_out, float* score_out, float* logp_out,
    int32_t* len_out, int32_t* met_out, hipStream_t s, const EnsembleRun* ens) {
  require(k >= 1 && k <= 16 && k <= L.V, "beam_forced: beam_size must be in [1, min(16, num_vocab)]");
  require(W >= 0, "beam_forced: words must be >= 0");
  require(W == 0 || k + W <= 15, "beam_forced: beam_size + words must be <= 15");
  require(W == 0 || k + W + 1 <= L.V, "beam_forced: beam_size + words + 1 must be <= num_vocab");
  require(W == 0 || (word && group), "beam_forced: null word / group");
  require(n_best >= 1 && n_best <= k, "beam_forced: n_best must be in [1, beam_size]");
  require(end_id >= -1 && end_id < L.V, "beam_forced: end_id must be in [-1, num_vocab)");
  require(alpha >= 0.f && alpha < INFINITY, "beam_forced: length_penalty must be finite and >= 0");  // (false for a NaN)
  require(N >= 1 && N <= 64, "beam_forced: N must be in [1, 64]");
  require(B >= 1, "beam_forced: need B >= 1");
  require(ids_out != nullptr, "beam_forced: null ids_out");
  require(dc.min_length == 0 || dc.end_id == end_id,
          "beam_forced: end_id differs from the end_id of the decode constraints' min_length");
  if (W == 0) {
    beam_nbest(feats, ft, pos, B, N, k, end_id, alpha, n_best, ids_out, score_out, logp_out, len_out, s, ens);
    if (met_out) memset_async(met_out, sizeof(int32_t) * n_best * B, s);
    return;
  }
  const BeamForced forced{word, group, W, nullptr, nullptr};  // (met: beam_run's double buffer)
  beam_run(feats, ft, pos, B, N, k, &end_id, s, ens, nullptr, &forced);
  beam_finish(g.seq, g.bprob, g.blen, k, B, L.maxlen, alpha, n_best, ids_out, score_out, logp_out, len_out, s, g.bmet,
              met_out);
}

// The loop of beam (end_id == nullptr: the reference's search, model.py:135-200) and of beam_nbest: leaves
// the k * B hypotheses in g.seq, their scores in g.bprob and, for beam_nbest, g.bfin / g.blen.
// ens (null: none): every step's logits are the ensemble's (ensemble_step below), nothing else changes.
// groups (null: none; needs end_id): beam_diverse's selection, the hypotheses left group by group.
// forced (null: none; needs end_id; its met pointers are ignored): beam_forced's selection, met left in g.bmet.
void capgen_engine::beam_run(const void* feats, DType ft, const float* pos, int B, int N, int k, const int* end_id, hipStream_t s,
    const EnsembleRun* ens, const BeamGroups* groups, const BeamForced* forced) {
  const int R = k * B, Tc = L.maxlen, Tw = L.maxlen;
  if (ens) ensemble_begin(*ens, feats, ft, pos, B, N, R, s);
  else begin_decode(feats, ft, pos, B, N, R, s);
  init_gen_ids(g.seq, R, Tw, g.ids, Tc, s);  // (Tw == Tc)
  // position 0: every beam holds <START>; top-k of beam 0's distribution (model.py:148-166)
  beam_kvrow(g.kvrow2, g.kvrow, Tc, -1, g.ids, B, R, s);  // [r][0] = r
  dec_step(R, B, N, 0, g.cache, g.ids, false, s);
  if (ens) ensemble_step(*ens, R, B, N, 0, nullptr, s);
  // decode constraints edit the step's logits (and repair the slab stats) in front of beam_nbest's selection
  const bool constrained = end_id && dc.on();
  if (constrained) constrain_logits(g.logits, slab_decode() ? g.dstats : nullptr, R, L.V, g.ids, Tc, 0, dc, s);
  // The step's form (select.h: BeamStep).  bf16: the selection and the reorder as one launch per image
  // (CAPGEN_FUSED_BEAM_STEP=0 restores the top-k, merge and three reorder launches); off that form the
  // END-aware step takes the full-row kernel, which reads the f32 logits of either dtype
  // (groups: the full-row top-k and the group merge; no fused form)
  // (forced: the full-row top-k and the bank merge; no fused form)
  const bool fused_step = slab_decode() && fused_beam_step_on && k <= 16 && Tw == Tc && !groups && !forced;
  if (end_id) {  // every hypothesis starts live with no tokens
    memset_async(g.bfin, sizeof(int32_t) * R, s);
    memset_async(g.blen, sizeof(int32_t) * R, s);
  }
  if (forced) memset_async(g.bmet, sizeof(int32_t) * R, s);  // no group met
  BeamStep b;  // what no step changes; the double-buffered arrays are set per step
  b.logits = g.logits, b.B = B, b.V = L.V, b.k = k, b.logsm = decode_logsm;
  b.stats = fused_step || (slab_decode() && !end_id) ? g.dstats : nullptr;
  b.cand_v = g.cand_v, b.cand_i = g.cand_i, b.out_src = g.bsrc, b.out_tok = g.btok, b.groups = groups;
  BeamForced fo{};  // (met: set per step, double-buffered like fin / len)
  if (forced) fo = *forced, b.forced = &fo, b.cand_v = g.fcand_v, b.cand_i = g.fcand_i;
  // The selection of position t over the k_in live beams per image with scores prev, and the reorder
  // behind it.  The K/V cache is never copied: row r writes its position-t K/V at [l][r][t] and reads
  // position j of its history from row kvrow[r][j] (the beam it descended from there); a reorder
  // moves only the ids / sequences and this [R][Tc] table
  auto select = [&](int t, const float* prev, int k_in) {
    // the END-aware step's state: read from bfin / blen, written to bfin2 / blen2, then swapped
    const BeamEnd ended{g.bfin, g.blen, g.bfin2, g.blen2, end_id ? *end_id : -1};
    BeamReorder ro;
    ro.seq_src = g.seq, ro.seq_dst = g.seq2, ro.ids_src = g.ids, ro.ids_dst = g.ids2;
    ro.kv_src = g.kvrow, ro.kv_dst = g.kvrow2, ro.Tw = Tw, ro.Tc = Tc, ro.t = t;
    b.prev = prev, b.k_in = k_in, b.out_prob = g.bprob2;
    b.end = end_id ? &ended : nullptr, b.reorder = fused_step ? &ro : nullptr;
    if (forced) fo.met_src = g.bmet, fo.met_dst = g.bmet2;
    beam_step(b, s);
    if (forced) std::swap(g.bmet, g.bmet2);
    std::swap(g.bprob, g.bprob2);
    if (end_id) std::swap(g.bfin, g.bfin2), std::swap(g.blen, g.blen2);
    if (!fused_step) {
      if (t == 0) memset_async(g.bsrc, sizeof(int32_t) * R, s);  // all beams descend from beam 0
      // seq/ids rows follow their source beam, then column t+1 = chosen token
      beam_gather(g.seq, g.seq2, Tw, g.bsrc, B, R, g.btok, t + 1, s);
      beam_gather(g.ids, g.ids2, Tc, g.bsrc, B, R, g.btok, t + 1, s);
      beam_kvrow(g.kvrow, g.kvrow2, Tc, t, g.bsrc, B, R, s);
    }
    std::swap(g.seq, g.seq2);
    std::swap(g.ids, g.ids2);
    std::swap(g.kvrow, g.kvrow2);
  };
  select(0, nullptr, 1);  // (beam 0's finalists only: every source is beam 0 at t = 0)
  for (int t = 1; t < Tw - 1; ++t) {
    dec_step(R, B, N, t, g.cache, g.ids, false, s, g.kvrow);
    if (ens) ensemble_step(*ens, R, B, N, t, g.kvrow, s);
    if (constrained) constrain_logits(g.logits, slab_decode() ? g.dstats : nullptr, R, L.V, g.ids, Tc, t, dc, s);
    select(t, g.bprob, k);
  }
}

// Sampled decoding: n draws per image from softmax(logits / temperature) over the top_k logits
// (0: the whole vocabulary), rows j * B + b as beam's, one encoder pass, every row its own K/V
// cache.  Tokens are drawn to the end (<END> is not special, as in greedy); logp_out (nullable)
// [R, max_length - 1]: each token's log-probability under the distribution it was drawn from.
// The selection reads the f32 logits of either decode mode (sample_softmax, select.hip); position t
// draws at site kSampleSite0 + t, above every dropout site (< 2048).  top_p < 1 cuts each position's
// candidates to the nucleus (sample_nucleus, select.hip); top_p == 1 launches sample_softmax as before.
void capgen_engine::sample(const void* feats, DType ft, const float* pos, int B, int N, int n, float temperature, int top_k,
    float top_p, uint64_t sd, int64_t* ids_out, float* logp_out, hipStream_t s, const EnsembleRun* ens) {
  require(n >= 1 && n <= 16, "sample: n_samples must be in [1, 16]");
  require(temperature > 0.f && temperature < INFINITY, "sample: temperature must be > 0 and finite");
  require(top_k >= 0 && top_k <= 16 && top_k <= L.V, "sample: top_k must be in [0, min(16, num_vocab)]");
  require(top_p > 0.f && top_p <= 1.f, "sample: top_p must be in (0, 1]");
  require(B >= 1 && N >= 1 && N <= 64, "sample: need B >= 1 and N in [1, 64]");
  require((int64_t)n * B * L.V < ((int64_t)1 << 32), "sample: n_samples * B * num_vocab must be < 2^32");
  require(ids_out != nullptr, "sample: null ids_out");
  const float inv_tau = 1.f / temperature;
  require(inv_tau > 0.f && inv_tau < INFINITY, "sample: temperature out of range");
  const int R = n * B, Tc = L.maxlen, W = L.maxlen + 1;
  if (ens) ensemble_begin(*ens, feats, ft, pos, B, N, R, s);
  else begin_decode(feats, ft, pos, B, N, R, s);
  init_gen_ids(ids_out, R, W, g.ids, Tc, s);
  for (int t = 0; t < L.maxlen - 1; ++t) {
    dec_step(R, B, N, t, g.cache, g.ids, false, s);
    if (ens) ensemble_step(*ens, R, B, N, t, nullptr, s);
    if (dc.on()) constrain_logits(g.logits, slab_decode() ? g.dstats : nullptr, R, L.V, g.ids, Tc, t, dc, s);
    sample_nucleus(g.logits, R, L.V, inv_tau, top_k, top_p, sd, kSampleSite0 + (uint32_t)t, ids_out, W, t + 1,
                   g.ids + t + 1, Tc, logp_out, Tc - 1, t, nullptr, s);
  }
}

// ---- ensemble decoding (capgen_ensemble_beam_nbest / capgen_ensemble_sample; the fusing kernel and the
// definition of the two modes: ensemble_combine, select.hip) ----
// Members k < K decode the SAME hypotheses in lock-step: at every position each member runs its own decoder
// step -- its own weights, encoder output, K/V cache and scratch -- on the leader's token table and beam K/V
// row table, which dec_step takes as arguments, so nothing is copied; one launch then fuses the K logit rows
// over the leader's (and rebuilds the leader's slab stats on the bf16 path), and the leader's constraints and
// selection run on that as on its own logits.  Depth, width and dtype may differ between members; what the
// shared tables and inputs fix may not.  Everything is enqueued on the leader's stream.

// The checks of a capgen_ensemble, before anything is launched; each message names the member and the field
EnsembleRun capgen_engine::checked_ensemble(const capgen_ensemble* e, const std::string& who) {
  require(e != nullptr, who + ": null ensemble");
  require(e->n_members >= 1 && e->n_members <= 8, who + ": n_members must be in [1, 8]");
  require(e->members != nullptr, who + ": null members");
  require(e->mode == CAPGEN_ENS_PROB || e->mode == CAPGEN_ENS_LOGPROB,
          who + ": mode must be CAPGEN_ENS_PROB or CAPGEN_ENS_LOGPROB");
  EnsembleRun r;
  r.mode = e->mode;
  const int K = e->n_members;
  double sum = 0;
  for (int k = 0; k < K; ++k) {
    const std::string mk = who + ": member " + std::to_string(k);
    capgen_engine* m = e->members[k];
    require(m != nullptr, mk + ": null handle");
    for (int j = 0; j < k; ++j) require(e->members[j] != m, mk + ": duplicate handle (same as member " + std::to_string(j) + ")");
    const capgen_engine* m0 = e->members[0];
    require(m->device == m0->device, mk + ": device differs from member 0's");
    auto same = [&](int a, int b, const char* field) {
      require(a == b, mk + ": " + field + " = " + std::to_string(a) + " differs from member 0's " + std::to_string(b));
    };
    same(m->cfg.num_vocab, m0->cfg.num_vocab, "num_vocab");
    same(m->cfg.max_length, m0->cfg.max_length, "max_length");
    same(m->cfg.pad_idx, m0->cfg.pad_idx, "pad_idx");
    same(m->cfg.dim_features, m0->cfg.dim_features, "dim_features");
    same(m->cfg.dim_positions, m0->cfg.dim_positions, "dim_positions");
    const float w = e->weights ? e->weights[k] : 1.f;
    require(std::isfinite(w) && w > 0.f, mk + ": weights[" + std::to_string(k) + "] must be finite and > 0");
    sum += (double)w;
    r.m.push_back(m);
  }
  for (int k = 0; k < K; ++k) {  // normalised in double, rounded to f32 once
    const float w = (float)((double)(e->weights ? e->weights[k] : 1.f) / sum);
    r.log_w[k] = logf(w);
  }
  return r;
}

// The call between the streams: the leader's enter / leave, and every other member's own stream ordered
// against the call in both directions -- what the member had enqueued is done before the call touches its
// buffers, and the host_sync(es) a member does before it re-plans a workspace covers this call.
void capgen_engine::ensemble_enter(const EnsembleRun& ens, hipStream_t cs) {
  enter(cs);
  for (size_t k = 1; k < ens.m.size(); ++k) dep(ens.m[k]->es, es, ens.m[k]->ev_out);
}
void capgen_engine::ensemble_leave(const EnsembleRun& ens, hipStream_t cs) {
  for (size_t k = 1; k < ens.m.size(); ++k) dep(es, ens.m[k]->es, ens.m[k]->ev_in);
  leave(cs);
}

// begin_decode of every member on s: every allocation of every member before anything is enqueued
void capgen_engine::ensemble_begin(const EnsembleRun& ens, const void* feats, DType ft, const float* pos, int B, int N,
    int R, hipStream_t s) {
  for (capgen_engine* m : ens.m) m->ensure_acts(B, N, 2), m->ensure_gen(R, N), m->ensure_dtiles();
  for (capgen_engine* m : ens.m) m->begin_decode(feats, ft, pos, B, N, R, s);
}

// After the leader's dec_step of position t: the other members' steps on the leader's ids (and kv_row), then
// the fused distribution over the leader's logits
void capgen_engine::ensemble_step(const EnsembleRun& ens, int R, int Bimg, int N, int t, const int32_t* kv_row,
    hipStream_t s) {
  const float* z[8];
  z[0] = g.logits;
  for (size_t k = 1; k < ens.m.size(); ++k) {
    capgen_engine* m = ens.m[k];
    m->dec_step(R, Bimg, N, t, m->g.cache, g.ids, false, s, kv_row);
    z[k] = m->g.logits;
  }
  ensemble_combine(z, ens.log_w, (int)ens.m.size(), ens.mode, R, L.V, g.logits, slab_decode() ? g.dstats : nullptr, s);
}

// capgen_set_decode_constraints: c checked against the model and installed (null: none), its banned
// list copied to the device
void capgen_engine::set_constraints(const capgen_decode_constraints* c) {
  if (!c) {
    dc = DecodeConstraints{};
    return;
  }
  DecodeConstraints d = checked_constraints(*c, L.V, L.maxlen, "set_decode_constraints");
  require(L.V - d.n_banned - L.maxlen >= 16,
          "set_decode_constraints: num_vocab - n_banned - max_length must be >= 16 (every row keeps 16 words)");
  if (d.n_banned > 0) {
    hz::host_sync(es);  // (an earlier decode may still read the former list)
    if (!dc_banned) CAPGEN_HIP(hipMalloc(&dc_banned, sizeof(int32_t) * 1024));
    CAPGEN_HIP(hipMemcpy(dc_banned, c->banned, sizeof(int32_t) * d.n_banned, hipMemcpyHostToDevice));
  }
  d.banned = d.n_banned > 0 ? dc_banned : nullptr;
  dc = d;
}
