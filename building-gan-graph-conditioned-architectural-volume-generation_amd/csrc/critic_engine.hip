// One critic iteration issued from C++: vg_critic_loss_and_grad (include/vgan.h).
//
// A restatement of vgan/critic.py CriticEngine.loss_and_grad in its default
// configuration -- the WGAN-GP loss of trainer.py:291-332 and its double
// backward (trainer.py:476-479) as four passes over the discriminator's op
// chain (A: stacked real / fake / mix forward; B: input VJP of the mix copy
// and the penalty head; C: tangent sweep with the second-order terms; D:
// stacked VJP of all copies, weight gradients grouped, folds deferred).  The
// same entry points are called in the same order with the same arguments, so
// the results are bit-identical to the Python engine's; only the host-side
// cost per launch changes (Python: marshalling + one torch allocation per
// temporary; here: a bump allocator over the caller's arena).  Two runs of
// launches are one here where a kernel exists, with the bits of the separate
// ones: a GAT backward source pass with its dX product (gat_bwd), and the MLP
// encoder's row-local products with the block-0 projection, one
// vg_gemm_chain per pass (links_or_gemms).  The steps the
// generator iteration issues too -- the GAT block forward and backward, the
// decoder's chains, the precision dispatch -- are engine.h's; the four passes
// share too much state to be more than one function.  Host code only: every
// launch goes through the library's own extern "C" entry points.
#include "engine.h"

namespace {

using namespace vg_engine;
constexpr int64_t kFoldWsFloats = 1 << 17;  // the split folds' chunk sums

int run(Ctx& cx, const vg_critic_model* md, const vg_critic_batch* bt, float* out) {
  const int n = bt->n, F = bt->feat, K = bt->classes;
  const int R = 3 * n, W0 = F + K, X4 = 4 * n;
  const int E = bt->g1.num_edges;
  const int nb = md->n_blocks, nd = md->n_dec, nm = md->n_mlp;
  const int mrow = 2 * n, trow = 3 * n;  // first row of the mix copy / of the tangent (pass-B) rows
  const vg_csr_ref& g1 = bt->g1;
  const vg_csr_ref& g3 = bt->g3;
  auto rows = [](float* t, int r0, int width) { return at(t, (int64_t)r0 * width); };
  Folds folds(cx, kFoldWsFloats);

  // ------------------------------------------------------------ pass A
  float* X0 = cx.take((int64_t)X4 * W0);
  VG_RUN(vg_critic_input_drawn(bt->mvx, n, F, bt->real, bt->hard, bt->soft, bt->seed, bt->iter, bt->eps_salt, K, 4,
                               X0, cx.stream));
  // the MLP encoder and block 0's projection: row-local, one chain
  std::vector<float*> mlp_out(nm);
  std::vector<vg_gemm_link> enc;
  float* x = X0;
  int xw = W0;
  for (int i = 0; i < nm; ++i) {
    const vg_critic_linear& L = md->mlp[i];
    float* y = cx.take((int64_t)X4 * L.out);
    enc.push_back(gemm_link(L.weight, xw, 0, L.out, y, L.bias, kActRelu, nullptr));
    mlp_out[i] = y;
    x = y;
    xw = L.out;
  }
  // per-block state of the forward (critic.py's blk dicts): all three copies, and from the mix copy on
  std::vector<GatS> blk(nb), mixb(nb);
  blk[0] = gat_proj_take(cx, R, x, xw, md->block[0]);
  enc.push_back(att_link(md->block[0], xw, blk[0].H, blk[0].a_s, blk[0].a_d));
  VG_TRY(cx.links_or_gemms(X0, W0, W0, R, enc));
  for (int b = 0; b < nb; ++b) {
    VG_TRY(gat_fwd(cx, g3, n, X4, x, xw, md->block[b], md->p_drop, bt->seed, bt->iter, bt->keep_salt[b], &blk[b],
                   b == 0));
    const GatS& S = blk[b];
    const int c = S.c;
    GatS& M = mixb[b] = S;
    M.H = rows(S.H, mrow, c), M.O = rows(S.O, mrow, c), M.keep = rows(S.keep, mrow, c), M.stats = at(S.stats, 2 * 2 * c);
    M.a_s = at(S.a_s, mrow), M.a_d = at(S.a_d, mrow), M.alpha = at(S.alpha, 2LL * E);
    x = S.Y;
    xw = c;
  }
  std::vector<float*> dec_out(nd);
  for (int i = 0; i < nd; ++i) dec_out[i] = cx.take((int64_t)(i == nd - 1 ? R : X4) * md->dec[i].out);
  VG_TRY(cx.chain_or_gemms(x, xw, R, fwd_chain(md->dec, nd, dec_out.data(), xw)));
  float* scores = dec_out[nd - 1];
  if (md->dec[nd - 1].out != 1) return VG_EINVAL;

  // adjoint buffers of pass D (rows [0,3N)) whose rows [3N,4N) pass B fills
  std::vector<float*> adj_dec(nd), adj_H(nb), adj_mlp(nm);
  for (int i = 0; i < nd - 1; ++i) adj_dec[i] = cx.take((int64_t)X4 * md->dec[i].out);
  adj_dec[nd - 1] = const_cast<float*>(bt->seeds4);
  for (int b = 0; b < nb; ++b) adj_H[b] = cx.take((int64_t)X4 * blk[b].c);
  for (int i = 0; i < nm; ++i) adj_mlp[i] = cx.take((int64_t)X4 * md->mlp[i].out);

  // the decoder's adjoint chain adj_dec[nd-1] -> ... -> adj_dec[0] (rows r0..)
  auto dec_adj = [&](int r0, int r_aux) { return adj_chain(md->dec, nd, dec_out.data(), adj_dec.data(), r0, r_aux); };
  auto take_tp = [&](int nrows, int m) { return cx.take(vg_gemm_gn_tpart_floats(nrows, m)); };
  // block S's GraphNorm(+ReLU+Dropout) backward over segs segments, column sums
  // only: the descriptor with which vg_gat_bwd_gn forms g_x in its destination-row pass
  auto gn_bwd = [&](const GatS& S, int segs, const float* tp, const float* g_y, bool pgrads, const float* inj,
                    int64_t inj_off, vg_gn_bwd_in* gn) -> int {
    const vg_critic_block& N = *S.B;
    float* ws = cx.take(vg_graphnorm_seg_ws_floats(segs, n, S.c));
    *gn = vg_gn_bwd_in{S.O, S.keep, g_y, inj, N.gn_weight, N.gn_bias, N.gn_mean_scale, S.stats,
                       at(ws, vg_graphnorm_bwd_sums_offset(segs, S.c)), N.gn_eps, segs, n, inj ? inj_off : 0};
    if (cx.dry) return 0;
    return vg_graphnorm_bwd_seg_tiles(S.O, segs, n, S.c, N.gn_weight, N.gn_bias, N.gn_mean_scale, S.keep, N.gn_eps,
                                      S.stats, g_y, tp, nullptr, pgrads ? N.g_gn_weight : nullptr,
                                      pgrads ? N.g_gn_bias : nullptr, pgrads ? N.g_gn_mean_scale : nullptr,
                                      pgrads ? 1 : 0, inj, inj_off, ws, cx.stream);
  };
  auto gemm_tn = [&](const float* A, int lda, const float* B, int ldb, int N, int M, int Kk, float* C, int ldc,
                     float* db, int db_rows) -> int {
    float* ws = cx.take(std::max<int64_t>(1, vg_gemm_tn_ws_floats(N, M, Kk)));
    return folds.tn(cx, A, lda, B, ldb, N, M, Kk, C, ldc, db, db_rows, ws);
  };

  // ------------------------------------------------------------ pass B
  VG_TRY(cx.chain_or_gemms(rows(adj_dec[nd - 1], trow, 1), 1, n, dec_adj(trow, mrow)));
  float* tp = nullptr;
  const vg_critic_linear& D0 = md->dec[0];
  float* dY = cx.take((int64_t)n * D0.in);
  tp = take_tp(n, D0.in);
  VG_TRY(cx.gemm_gn_bwd(rows(adj_dec[0], trow, D0.out), D0.out, D0.weight, D0.in, n, D0.in, D0.out, dY, mixb[nb - 1], n,
                        tp));
  std::vector<float*> dY_b(nb), dO_b(nb);
  for (int b = nb - 1; b >= 0; --b) {
    const GatS& S = mixb[b];
    const float* Wl = S.B->lin_weight;
    const int c = S.c, cin = S.xw;
    dY_b[b] = dY;
    float* dO = cx.take((int64_t)n * c);
    float* dH = rows(adj_H[b], trow, c);
    float* ws = cx.take(vg_gat_bwd_ws_floats(n, E, c));
    vg_gn_bwd_in gn;
    VG_TRY(gn_bwd(S, 1, tp, dY, false, nullptr, 0, &gn));
    float* dX = b > 0 ? cx.take((int64_t)n * cin) : nullptr;
    float* tpx = b > 0 ? take_tp(n, cin) : nullptr;
    const vg_dx_in dx = b > 0 ? dx_in(Wl, cin, dX, cin, mixb[b - 1], n, tpx) : vg_dx_in{};
    bool fused;
    VG_TRY(gat_bwd(cx, folds, g1, S, gn, dO, dH, ws, false, nullptr, 0, b > 0 ? &dx : nullptr, &fused));
    dO_b[b] = dO;
    if (b > 0) {
      if (!fused) VG_TRY(cx.gemm_gn_bwd(dH, c, Wl, cin, n, cin, c, dX, mixb[b - 1], n, tpx));
      tp = tpx;
      dY = dX;
    }
  }
  // block 0's masked dX, the MLP's adjoints and g = adj W0[:, F:]: row-local, one chain
  const vg_critic_linear& M0 = md->mlp[0];
  const int hd = M0.out, c0 = mixb[0].c;
  float* g = cx.take((int64_t)n * K);
  {
    std::vector<vg_gemm_link> tail;
    tail.push_back(gemm_link(md->block[0].lin_weight, mixb[0].xw, 1, mixb[0].xw, rows(adj_mlp[nm - 1], trow, mixb[0].xw),
                             nullptr, kActMask, rows(mlp_out[nm - 1], mrow, mixb[0].xw)));
    for (int i = nm - 1; i >= 1; --i) {
      const int m = md->mlp[i].in;
      tail.push_back(gemm_link(md->mlp[i].weight, m, 1, m, rows(adj_mlp[i - 1], trow, m), nullptr, kActMask,
                               rows(mlp_out[i - 1], mrow, m)));
    }
    tail.push_back(gemm_link(M0.weight + F, W0, 1, K, g, nullptr, kActNone, nullptr));
    VG_TRY(cx.links_or_gemms(rows(adj_H[0], trow, c0), c0, c0, n, tail));
  }
  float* gws = cx.take(vg_gp_head_ws_floats(n));
  float* u0 = X0 ? X0 + (int64_t)trow * W0 + F : nullptr;  // dGP/dg into the label columns of X0's tangent rows
  VG_RUN(vg_gp_head(g, n, K, scores, md->lambda_gp, u0, W0, out, gws, bt->gp_counter, cx.stream));

  // ------------------------------------------------------------ pass C
  // u0 W0[:, F:]^T, the MLP's tangents and block 0's tangent projection: row-local, one chain
  std::vector<vg_gemm_link> head;
  head.push_back(gemm_link(M0.weight + F, W0, 0, hd, rows(mlp_out[0], trow, hd), nullptr, kActMask,
                           rows(mlp_out[0], mrow, hd)));
  int uw = hd;
  for (int i = 1; i < nm; ++i) {
    const int o = md->mlp[i].out;
    head.push_back(gemm_link(md->mlp[i].weight, uw, 0, o, rows(mlp_out[i], trow, o), nullptr, kActMask,
                             rows(mlp_out[i], mrow, o)));
    uw = o;
  }
  float* u_in = rows(mlp_out[nm - 1], trow, uw);
  const GatS U0 = gat_proj_take(cx, n, u_in, uw, md->block[0]);
  head.push_back(att_link(md->block[0], uw, U0.H, U0.a_s, U0.a_d));
  VG_TRY(cx.links_or_gemms(u0, W0, K, n, head));
  std::vector<float*> hinj_b(nb), oinj_b(nb);
  for (int b = 0; b < nb; ++b) {
    const vg_critic_block& B = md->block[b];
    const GatS& S = mixb[b];
    const int c = S.c, cin = S.xw;
    float* uH = b == 0 ? U0.H : cx.take((int64_t)n * c);
    float* up_s = b == 0 ? U0.a_s : cx.take(n);
    float* up_d = b == 0 ? U0.a_d : cx.take(n);
    if (b > 0) VG_TRY(cx.lin_att(u_in, cin, B, n, uH, up_s, up_d));
    float* uO = cx.take((int64_t)n * c);
    float* hinj = cx.take((int64_t)n * c);
    float* ws = cx.take(vg_gat_jvp2_ws_floats(n, E, c));
    const float *gx = S.O, *gkeep = S.keep, *gstats = S.stats;
    float* oinj = cx.take((int64_t)n * c);
    float* gws2 = cx.take(vg_graphnorm_seg_ws_floats(1, n, c));
    if (!cx.dry) {
      // the GAT tangent's destination-row pass, its folds deferred
      // (FoldCollector.jvp) and its source pass described: the source pass
      // writes only pass D's injection and att_src partials, so it runs in the
      // GraphNorm fold's launch (vg_graphnorm_jvp2_fold_src) instead of one of
      // its own -- the same kernels and values as vg_gat_jvp2_deferred +
      // vg_graphnorm_jvp2, one launch fewer per block
      vg_fold f[2];
      int32_t nf = 0;
      vg_jvp_src src;
      VG_TRY(vg_gat_jvp2_plan(g1.row_ptr, g1.col, g1.csc_ptr, g1.csc_slot, g1.csc_dst, n, E, c, S.H, uH, dO_b[b],
                              B.att_src, B.att_dst, S.a_s, S.a_d, S.alpha, B.slope, uO, hinj, B.g_att_src, B.g_att_dst, up_s, up_d, ws, f, &nf, &src, cx.stream));
      folds.add(f, nf);
      VG_TRY(vg_graphnorm_jvp2_sums(gx, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, gkeep, B.gn_eps, gstats, uO,
                                    dY_b[b], gws2, cx.stream));
      VG_TRY(vg_graphnorm_jvp2_fold_src(n, c, B.gn_weight, B.gn_mean_scale, gstats, gws2, B.g_gn_weight,
                                        B.g_gn_mean_scale, &src, cx.stream));
      VG_TRY(vg_graphnorm_jvp2_apply(gx, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, gkeep, B.gn_eps, gstats, uO,
                                     dY_b[b], rows(blk[b].Y, trow, c), oinj, gws2, cx.stream));
    }
    hinj_b[b] = hinj;
    oinj_b[b] = oinj;
    u_in = rows(blk[b].Y, trow, c);
    uw = c;
  }
  Chain tan{{uw}, {}};  // the tangent through the decoder's hidden layers
  for (int i = 0; i < nd - 1; ++i) {
    const int o = md->dec[i].out;
    tan.w.push_back(o);
    tan.layers.push_back(vg_chain_layer{md->dec[i].weight, nullptr, rows(dec_out[i], mrow, o), rows(dec_out[i], trow, o),
                                        o, o, 0, kActMask});
  }
  VG_TRY(cx.chain_or_gemms(u_in, uw, n, tan));

  // ------------------------------------------------------------ pass D
  // weight gradients over 4N rows: [pass-D adjoint ; pass-B adjoint]^T [activation ; tangent]
  std::vector<float*> dec_in(nd);
  dec_in[0] = nb ? blk[nb - 1].Y : mlp_out[nm - 1];
  for (int i = 1; i < nd; ++i) dec_in[i] = dec_out[i - 1];
  const int chained = cx.chain(adj_dec[nd - 1], 1, R, dec_adj(0, 0));
  if (chained < 0) return -chained;
  for (int i = nd - 1; i >= 0; --i) {
    const vg_critic_linear& L = md->dec[i];
    const int aw = L.out, m = L.in;
    VG_TRY(gemm_tn(adj_dec[i], aw, dec_in[i], m, X4, aw, m, L.g_weight, m, L.g_bias, R));
    if (i > 0) {
      if (!chained)
        VG_TRY(cx.gemm(adj_dec[i], aw, L.weight, m, 0, adj_dec[i - 1], m, R, m, aw, nullptr, kActMask, dec_out[i - 1],
                       m));
    } else {
      dY = cx.take((int64_t)R * m);
      tp = take_tp(R, m);
      VG_TRY(cx.gemm_gn_bwd(adj_dec[0], aw, L.weight, m, R, m, aw, dY, blk[nb - 1], n, tp));
    }
  }
  for (int b = nb - 1; b >= 0; --b) {
    const vg_critic_block& B = md->block[b];
    const GatS& S = blk[b];
    const int c = S.c, cin = S.xw;
    float* dO = cx.take((int64_t)R * c);
    float* ws = cx.take(vg_gat_bwd_ws_floats(R, 3 * E, c));
    vg_gn_bwd_in gn;
    VG_TRY(gn_bwd(S, 3, tp, dY, true, oinj_b[b], (int64_t)mrow * c, &gn));
    float* dX = b > 0 ? cx.take((int64_t)R * cin) : nullptr;
    float* tpx = b > 0 ? take_tp(R, cin) : nullptr;
    const vg_dx_in dx = b > 0 ? dx_in(B.lin_weight, cin, dX, cin, blk[b - 1], n, tpx) : vg_dx_in{};
    bool fused;  // folds deferred (FoldCollector.call)
    VG_TRY(gat_bwd(cx, folds, g3, S, gn, dO, adj_H[b], ws, true, hinj_b[b], mrow, b > 0 ? &dx : nullptr, &fused));
    VG_TRY(gemm_tn(adj_H[b], c, S.X, cin, X4, c, cin, B.g_lin_weight, cin, nullptr, X4));
    if (b > 0) {
      if (!fused) VG_TRY(cx.gemm_gn_bwd(adj_H[b], c, B.lin_weight, cin, R, cin, c, dX, blk[b - 1], n, tpx));
      tp = tpx;
      dY = dX;
    } else {
      // block 0's masked dX and the MLP's adjoints: row-local, one chain (its
      // weight-gradient products below are planned only, launched by the flush)
      std::vector<vg_gemm_link> tail;
      tail.push_back(gemm_link(B.lin_weight, cin, 1, cin, adj_mlp[nm - 1], nullptr, kActMask, mlp_out[nm - 1]));
      for (int i = nm - 1; i >= 1; --i) {
        const int m = md->mlp[i].in;
        tail.push_back(gemm_link(md->mlp[i].weight, m, 1, m, adj_mlp[i - 1], nullptr, kActMask, mlp_out[i - 1]));
      }
      VG_TRY(cx.links_or_gemms(adj_H[b], c, c, R, tail));
    }
  }
  for (int i = nm - 1; i >= 0; --i) {
    const vg_critic_linear& L = md->mlp[i];
    const int o = L.out, m = L.in;
    const float* xin = i == 0 ? X0 : mlp_out[i - 1];
    VG_TRY(gemm_tn(adj_mlp[i], o, xin, m, X4, o, m, L.g_weight, m, L.g_bias, R));
  }
  return folds.flush(cx);
}

bool model_ok(const vg_critic_model* md, const vg_critic_batch* bt) {
  if (!md || !bt) return false;
  if (md->n_mlp < 1 || md->n_blocks < 1 || md->n_dec < 1 || md->n_mlp > VG_CRITIC_MAX_LAYERS ||
      md->n_blocks > VG_CRITIC_MAX_LAYERS || md->n_dec > VG_CRITIC_MAX_LAYERS)
    return false;
  if (bt->n < 64 || bt->feat < 1 || bt->classes < 1 || bt->g1.num_nodes != bt->n || bt->g3.num_nodes != 3 * bt->n ||
      bt->g3.num_edges != 3 * bt->g1.num_edges)
    return false;
  if (md->mlp[0].in != bt->feat + bt->classes) return false;
  int w = md->mlp[0].in;
  for (int i = 0; i < md->n_mlp; ++i) {
    if (md->mlp[i].in != w) return false;
    w = md->mlp[i].out;
  }
  for (int b = 0; b < md->n_blocks; ++b) {
    if (md->block[b].in != w) return false;
    w = md->block[b].out;
  }
  for (int i = 0; i < md->n_dec; ++i) {
    if (md->dec[i].in != w) return false;
    w = md->dec[i].out;
  }
  return w == 1;
}

}  // namespace

extern "C" int64_t vg_critic_arena_floats(const vg_critic_model* model, const vg_critic_batch* batch) {
  if (!model_ok(model, batch)) return -1;
  Ctx cx{true, model->bf16, nullptr, nullptr, 0, 0};
  if (run(cx, model, batch, nullptr)) return -1;
  return cx.off;
}

extern "C" int vg_critic_loss_and_grad(const vg_critic_model* model, const vg_critic_batch* batch, float* arena,
                                       int64_t arena_floats, float* out, void* stream) {
  if (!model_ok(model, batch) || !arena || !out || !batch->mvx || !batch->real || !batch->hard || !batch->soft ||
      !batch->seeds4 || !batch->iter || !batch->gp_counter)
    return VG_EINVAL;
  if (reinterpret_cast<uintptr_t>(arena) & 255) return VG_EINVAL;
  const int64_t need = vg_critic_arena_floats(model, batch);
  if (need < 0 || need > arena_floats) return VG_EINVAL;
  Ctx cx{false, model->bf16, stream, arena, arena_floats, 0};
  return run(cx, model, batch, out);
}
