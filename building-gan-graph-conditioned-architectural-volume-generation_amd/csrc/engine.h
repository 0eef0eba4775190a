// Host-side plumbing shared by the iterations issued from C++
// (critic_engine.hip: vg_critic_loss_and_grad; gen_engine.hip:
// vg_gen_loss_and_grad and its hoisted pair): a bump allocator over the
// caller's arena with a dry (sizing) mode, the library's entry points that
// come in an f32 and a bf16 form dispatched on the model's precision (Ctx),
// the FoldCollector of vgan/_lib.py (Folds: grouped weight-gradient products,
// then the parameter-gradient folds merged and batched exactly as the Python
// collector merges them), and the steps both engines issue: a run of narrow
// linear layers as one vg_linear_chain launch or layer by layer (Chain), a run
// of 64-wide products as one vg_gemm_chain launch or product by product
// (links_or_gemms), the forward of one GAT block (gat_fwd) and the backward of one with the dX
// product fused into its source pass where a kernel exists (gat_bwd).  Host
// code only: every launch goes through the library's own extern "C" entry points.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/vgan.h"

#define VG_TRY(expr)          \
  do {                        \
    const int _rc = (expr);   \
    if (_rc) return _rc;      \
  } while (0)
#define VG_RUN(expr)                  \
  do {                                \
    if (!cx.dry) {                    \
      const int _rc = (expr);         \
      if (_rc) return _rc;            \
    }                                 \
  } while (0)

namespace vg_engine {

constexpr int kActNone = 0, kActRelu = 1, kActMask = 3, kActAdd = 4;

// p + off, NULL where p is (a dry pass)
template <class T>
T* at(T* p, int64_t off) {
  return p ? p + off : nullptr;
}

// a run of narrow linear layers as vg_linear_chain takes it; every layer's
// output rows are its width apart
struct Chain {
  std::vector<int32_t> w;  // [layers + 1]
  std::vector<vg_chain_layer> layers;
};

// one GAT block's forward state: GATConv (H, a_s, a_d, alpha, O) -> GraphNorm
// (stats) -> ReLU -> Dropout (keep) -> Y, of the input X [rows, xw]
struct GatS {
  const vg_critic_block* B;
  const float* X;
  int xw, c;
  float *H, *O, *alpha, *a_s, *a_d, *Y, *stats, *keep;
};

// the dX product o [rows, m] = dH Wt below block D's GraphNorm (segments of seg_rows rows), as vg_gat_bwd_gn_dx takes it
inline vg_dx_in dx_in(const float* Wt, int ldw, float* o, int m, const GatS& D, int seg_rows, float* tp) {
  const vg_critic_block& N = *D.B;
  return vg_dx_in{Wt, ldw, m, o, m, D.O, D.keep, seg_rows, N.gn_weight, N.gn_bias, N.gn_mean_scale, N.gn_eps, D.stats, tp};
}

struct Ctx {
  bool dry;  // size the arena only: no launches, no plans
  int bf16;
  void* stream;
  float* base;
  int64_t cap, off;

  // 256-byte aligned temporaries (the quad / float4 kernel forms need 16 B)
  float* take(int64_t floats) {
    const int64_t at = off;
    off += (std::max<int64_t>(floats, 1) + 63) / 64 * 64;
    return dry ? nullptr : base + at;
  }

  int gemm(const float* A, int lda, const float* B, int ldb, int bt, float* C, int ldc, int n, int m, int k,
           const float* bias = nullptr, int act = kActNone, const float* aux = nullptr, int ldaux = 0) const {
    if (dry) return 0;
    return bf16 ? vg_gemm_bf16(A, lda, B, ldb, bt, bias, act, aux, ldaux, C, ldc, n, m, k, stream)
                : vg_gemm(A, lda, B, ldb, bt, bias, act, aux, ldaux, C, ldc, n, m, k, stream);
  }

  // vg_linear_chain: 1 launched, 0 no kernel for this width chain (the caller
  // runs its per-layer GEMMs), < 0 error
  int chain(const float* x, int ldx, int rows, const Chain& ch) const {
    if (dry) return 1;
    const int rc = (bf16 ? vg_linear_chain_bf16 : vg_linear_chain)(x, ldx, rows, ch.w.data(), (int32_t)ch.layers.size(),
                                                                   ch.layers.data(), stream);
    if (rc == VG_EINVAL) return 0;
    return rc == 0 ? 1 : (rc > 0 ? -rc : rc);
  }

  // the chain in one launch, or its layers as one GEMM each where no kernel has this width chain
  int chain_or_gemms(const float* x, int ldx, int rows, const Chain& ch) const {
    const int rc = chain(x, ldx, rows, ch);
    if (rc < 0) return -rc;
    for (size_t i = 0; rc == 0 && i < ch.layers.size(); ++i) {
      const vg_chain_layer& L = ch.layers[i];
      const int k = ch.w[i], m = ch.w[i + 1];
      const int e = gemm(x, ldx, L.weight, L.w_trans ? m : k, L.w_trans ? 0 : 1, L.out, L.ld_out, rows, m, k, L.bias,
                         L.act, L.aux, L.ld_aux);
      if (e) return e;
      x = L.out;
      ldx = L.ld_out;
    }
    return 0;
  }

  // 2-3 consecutive products x [rows, k] -> links (each at most 64 wide) in one
  // vg_gemm_chain launch where vg_gemm_chain_use agrees and the entry point has
  // a kernel (f32 only), else one vg_gemm / vg_gat_lin_att launch per link.
  // Takes nothing from the arena.
  int links_or_gemms(const float* x, int ldx, int k, int rows, const std::vector<vg_gemm_link>& links) const {
    if (dry) return 0;
    const int nl = (int)links.size();
    for (int i = 0; i < nl; ++i) {
      // the links from i on as a chain; where that is refused (a first K that
      // is no multiple of 4: the label columns' tangent), link i alone and the rest again
      if (!bf16 && vg_gemm_chain_use(rows, nl - i)) {
        const int rc = vg_gemm_chain(x, ldx, k, rows, links.data() + i, nl - i, 0, stream);
        if (rc != VG_EINVAL) return rc;
      }
      const vg_gemm_link& L = links[i];
      int e;
      if (L.att_src) {
        if (L.ldw != k || ldx != k || L.ld_out != L.m) return VG_EINVAL;
        e = (bf16 ? vg_gat_lin_att_bf16 : vg_gat_lin_att)(x, ldx, L.w, rows, k, L.m, L.att_src, L.att_dst, L.out, L.a_src,
                                                           L.a_dst, stream);
      } else {
        e = gemm(x, ldx, L.w, L.ldw, L.w_trans ? 0 : 1, L.out, L.ld_out, rows, L.m, k, L.bias, L.act, L.aux, L.ld_aux);
      }
      if (e) return e;
      x = L.out;
      ldx = L.ld_out;
      k = L.m;
    }
    return 0;
  }

  int lin_att(const float* x, int ldx, const vg_critic_block& B, int rows, float* H, float* a_s, float* a_d) const {
    if (dry) return 0;
    return (bf16 ? vg_gat_lin_att_bf16 : vg_gat_lin_att)(x, ldx, B.lin_weight, rows, ldx, B.out, B.att_src, B.att_dst,
                                                         H, a_s, a_d, stream);
  }

  // o [rows, m] = A Wt, the output gradient of block D's GraphNorm (segments of
  // seg_rows rows), with that backward's column partials from the GEMM's epilogue in tp
  int gemm_gn_bwd(const float* A, int lda, const float* Wt, int ldw, int rows, int m, int k, float* o, const GatS& D,
                  int seg_rows, float* tp) const {
    if (dry) return 0;
    const vg_critic_block& N = *D.B;
    return (bf16 ? vg_gemm_gn_bwd_bf16 : vg_gemm_gn_bwd)(A, lda, Wt, ldw, rows, m, k, o, m, D.O, D.keep, seg_rows,
                                                         N.gn_weight, N.gn_bias, N.gn_mean_scale, N.gn_eps, D.stats, tp,
                                                         stream);
  }

  int gemm_ln_act(const float* x, int ldx, const vg_gen_ln_layer& L, int rows, float* h, float* y, float* mean,
                  float* rstd) const {
    if (dry) return 0;
    return (bf16 ? vg_gemm_ln_act_bf16 : vg_gemm_ln_act)(x, ldx, L.weight, rows, L.out, L.in, L.bias, L.ln_weight,
                                                         L.ln_bias, L.ln_eps, L.slope, h, y, mean, rstd, stream);
  }
};

// the forward chain x [., xw] -> lin[0] -> ReLU -> ... -> lin[nl - 1] (no activation) into out[i]
inline Chain fwd_chain(const vg_critic_linear* lin, int nl, float* const* out, int xw) {
  Chain ch{{xw}, {}};
  for (int i = 0; i < nl; ++i) {
    ch.w.push_back(lin[i].out);
    ch.layers.push_back(
        vg_chain_layer{lin[i].weight, lin[i].bias, nullptr, out[i], 0, lin[i].out, 0, i == nl - 1 ? kActNone : kActRelu});
  }
  return ch;
}
// its adjoint chain adj[nl - 1] -> ... -> adj[0] over the rows from r0 on, ReLU's mask from out's rows from r_aux on
inline Chain adj_chain(const vg_critic_linear* lin, int nl, float* const* out, float* const* adj, int r0, int r_aux) {
  Chain ch{{lin[nl - 1].out}, {}};
  for (int i = nl - 1; i >= 1; --i) {
    const int in = lin[i].in;
    ch.w.push_back(lin[i - 1].out);
    ch.layers.push_back(vg_chain_layer{lin[i].weight, nullptr, at(out[i - 1], (int64_t)r_aux * in),
                                       at(adj[i - 1], (int64_t)r0 * in), in, in, 1, kActMask});
  }
  return ch;
}

#ifndef VG_CRITIC_FOLD_SPLIT
#define VG_CRITIC_FOLD_SPLIT 1  // long folds in two levels (vg_fold_batch_split); 0: vg_fold_batch (A/B)
#endif

struct Folds {
  std::vector<vg_fold> folds;
  std::vector<vg_tn> prods;  // planned, not yet launched
  float* ws = nullptr;       // the split folds' chunk sums (arena)
  int64_t ws_floats = 0;

  Folds(Ctx& cx, int64_t floats) : ws(cx.take(floats)), ws_floats(floats) {}

  void add(const vg_fold* f, int n) { folds.insert(folds.end(), f, f + n); }

  int tn(const Ctx& cx, const float* A, int lda, const float* B, int ldb, int N, int M, int K, float* C, int ldc,
         float* db, int db_rows, float* w) {
    if (cx.dry) return 0;
    vg_tn p;
    vg_fold f[2];
    int32_t n = 0;
    const int rc = cx.bf16 ? vg_gemm_tn_plan_bf16(A, lda, B, ldb, N, M, K, C, ldc, db, db_rows, 1, w, &p, f, &n)
                           : vg_gemm_tn_plan(A, lda, B, ldb, N, M, K, C, ldc, db, db_rows, 1, w, &p, f, &n);
    if (rc) return rc;
    prods.push_back(p);
    add(f, n);
    return 0;
  }

  int launch_products(void* stream) {
    for (int bf = 0; bf < 2; ++bf) {
      std::vector<vg_tn> sel;
      for (const vg_tn& p : prods)
        if ((p.bf16 != 0) == (bf != 0)) sel.push_back(p);
      for (size_t i = 0; i < sel.size(); i += VG_TN_GROUP_MAX) {
        const int n = (int)std::min<size_t>(VG_TN_GROUP_MAX, sel.size() - i);
        const int rc = vg_gemm_tn_group(sel.data() + i, n, stream);
        if (rc) return rc;
      }
    }
    prods.clear();
    return 0;
  }

  int flush(Ctx& cx) {
    if (cx.dry) return 0;
    int rc = launch_products(cx.stream);  // the products first: their partials feed the folds
    if (rc) return rc;
    // folds into one destination merge into a two-source fold (applied in
    // call order); one that cannot merge starts a new batch, so the two never race
    std::vector<std::vector<vg_fold>> batches;
    std::vector<vg_fold> cur;
    std::vector<std::pair<float*, int>> where;
    auto find = [&](float* out) -> int {
      for (auto& w : where)
        if (w.first == out) return w.second;
      return -1;
    };
    for (const vg_fold& f : folds) {
      const int j = find(f.out);
      if (j >= 0) {
        vg_fold& g = cur[j];
        if (g.nsrc == 1 && f.nsrc == 1 && f.accumulate && g.width == f.width && g.k == f.k && g.ldo == f.ldo) {
          g.src[1] = f.src[0];
          g.nsrc = 2;
          continue;
        }
        batches.push_back(cur);
        cur.clear();
        where.clear();
      }
      if ((int)cur.size() == VG_FOLD_MAX) {
        batches.push_back(cur);
        cur.clear();
        where.clear();
      }
      where.emplace_back(f.out, (int)cur.size());
      cur.push_back(f);
    }
    if (!cur.empty()) batches.push_back(cur);
    for (auto& b : batches) {
      const int rc = VG_CRITIC_FOLD_SPLIT ? vg_fold_batch_split(b.data(), (int32_t)b.size(), ws, ws_floats, cx.stream)
                                          : vg_fold_batch(b.data(), (int32_t)b.size(), cx.stream);
      if (rc) return rc;
    }
    folds.clear();
    return 0;
  }
};

// the buffers of a block's projection H, a_s, a_d over `rows` rows of x, in gat_fwd's order
inline GatS gat_proj_take(Ctx& cx, int rows, const float* x, int xw, const vg_critic_block& B) {
  GatS s{&B, x, xw, B.out};
  s.H = cx.take((int64_t)rows * B.out);
  s.a_s = cx.take(rows);
  s.a_d = cx.take(rows);
  return s;
}
// the projection as the last link of a vg_gemm_chain
inline vg_gemm_link att_link(const vg_critic_block& B, int cin, float* H, float* a_s, float* a_d) {
  return vg_gemm_link{B.lin_weight, nullptr, nullptr, H, B.att_src, B.att_dst, a_s, a_d, cin, 0, B.out, B.out, 0, kActNone};
}
// y = act(x op(w) + bias) with aux [., m] and y [., m] contiguous
inline vg_gemm_link gemm_link(const float* w, int ldw, int w_trans, int m, float* y, const float* bias, int act,
                              const float* aux) {
  return vg_gemm_link{w, bias, aux, y, nullptr, nullptr, nullptr, nullptr, ldw, aux ? m : 0, m, m, w_trans, act};
}

// One GAT block's forward over g's rows as GraphNorm segments of seg_rows rows:
// projection (projected: done by the caller into gat_proj_take's buffers in
// *S), aggregation (with the GraphNorm column partials), GraphNorm -> ReLU ->
// Dropout with the mask drawn in-kernel and stored.  Y has y_rows rows.
inline int gat_fwd(Ctx& cx, const vg_csr_ref& g, int seg_rows, int64_t y_rows, const float* x, int xw,
                   const vg_critic_block& B, float p_drop, uint64_t seed, const int64_t* iter, uint32_t salt, GatS* S,
                   bool projected = false) {
  const int rows = g.num_nodes, c = B.out;
  if (B.in != xw) return VG_EINVAL;
  const int gr = vg_gat_gnp_rows(rows, c);
  if (gr <= 0 || seg_rows < gr || rows % seg_rows) return VG_EINVAL;  // (the Python engines' unfused path)
  GatS s = projected ? *S : gat_proj_take(cx, rows, x, xw, B);
  if (!projected) VG_TRY(cx.lin_att(x, xw, B, rows, s.H, s.a_s, s.a_d));
  s.O = cx.take((int64_t)rows * c);
  s.alpha = cx.take(g.num_edges);
  float* gnp = cx.take(vg_gat_gnp_floats(rows, c));
  VG_RUN(vg_gat_aggregate_fwd_gnp(g.row_ptr, g.col, g.ell, g.ell ? g.ell_width : 0, rows, c, s.H, s.a_s, s.a_d, B.bias,
                                  B.slope, s.O, s.alpha, seg_rows, gnp, cx.stream));
  s.Y = cx.take(y_rows * c);
  s.stats = cx.take((int64_t)(rows / seg_rows) * 2 * c);
  s.keep = cx.take((int64_t)rows * c);
  VG_RUN(vg_graphnorm_fwd_gnp(s.O, rows / seg_rows, seg_rows, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, nullptr,
                              p_drop, seed, iter, salt, B.gn_eps, s.Y, s.keep, s.stats, gnp, gr, cx.stream));
  *S = s;
  return 0;
}

// The GATConv backward of block S over g's rows, below the GraphNorm backward
// gn describes (vg_gat_bwd_gn forms dO from it): dH; with pgrads the block's
// attention / bias gradients, their folds deferred.  dx (NULL: none) is the dX
// product that consumes dH: run in the source pass's launch (*fused) where
// vg_bwd_src_gemm_use says so and vg_gat_bwd_gn_dx has a kernel for the shape
// (f32 only), else left to the caller.
inline int gat_bwd(const Ctx& cx, Folds& folds, const vg_csr_ref& g, const GatS& S, const vg_gn_bwd_in& gn, float* dO,
                   float* dH, float* ws, bool pgrads, const float* inj, int inj_row0, const vg_dx_in* dx, bool* fused) {
  *fused = false;
  if (cx.dry) return 0;
  const vg_critic_block& B = *S.B;
  const int rows = g.num_nodes, E = g.num_edges, c = S.c, acc = pgrads ? 1 : 0;
  vg_fold f[3];
  int32_t nf = 0;
  float *gas = pgrads ? B.g_att_src : nullptr, *gad = pgrads ? B.g_att_dst : nullptr, *gbi = pgrads ? B.g_bias : nullptr;
  vg_fold* fo = pgrads ? f : nullptr;
  int32_t* no = pgrads ? &nf : nullptr;
  int rc = VG_EINVAL;
  if (dx && !cx.bf16 && vg_bwd_src_gemm_use(rows, c))
    rc = vg_gat_bwd_gn_dx(g.row_ptr, g.col, g.csc_ptr, g.csc_slot, g.csc_dst, rows, E, c, S.H, B.att_src, B.att_dst, S.a_s,
                          S.a_d, S.alpha, &gn, dO, B.slope, dH, gas, gad, gbi, acc, inj, inj_row0, ws, fo, no, dx,
                          cx.stream);
  if (rc == 0)
    *fused = true;
  else if (rc != VG_EINVAL)
    return rc;
  else
    VG_TRY(vg_gat_bwd_gn(g.row_ptr, g.col, g.csc_ptr, g.csc_slot, g.csc_dst, rows, E, c, S.H, B.att_src, B.att_dst, S.a_s,
                         S.a_d, S.alpha, &gn, dO, B.slope, dH, gas, gad, gbi, acc, inj, inj_row0, ws, fo, no, cx.stream));
  folds.add(f, nf);
  return 0;
}

}  // namespace vg_engine
