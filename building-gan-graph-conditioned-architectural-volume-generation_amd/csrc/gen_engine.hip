// One generator iteration issued from C++: vg_gen_loss_and_grad (include/vgan.h).
//
// A restatement of vgan/genstep.py GeneratorEngine.loss_and_grad in its
// default configuration -- the generator half of trainer.py:483-491: G(z) ->
// Gumbel straight-through labels -> D(label_hard) in train mode -> the loss of
// trainer.py:334-385 -> the backward into G's parameters (D's input VJP only,
// the Gumbel backward, G's backward with every fold and weight-gradient
// product deferred to one grouped flush).  The same entry points run in the
// same order with the same arguments, the device-RNG draws under the same
// salts, so loss, labels and gradients are bit-identical to the Python
// engine's (tests/test_gen_engine_gpu.py); the host pays ~1-2 us per launch
// instead of ~10 (a fresh batch's generator iteration runs eagerly,
// Trainer.step_fresh).  The two kernels below are the copies torch.cat and
// Tensor.add_ make in the Python engine.
//
// vg_gen_forward_stacked + vg_gen_loss_and_grad_from split the iteration: the
// forward runs ahead, as the last copy of the stacked critic-label forward at
// the start of the step (G's weights do not change in between and its draws
// are counter-based), and the rest starts from the state that forward left
// in the arena.  Same bits as the whole iteration (tests/test_gen_hoist_gpu.py).
//
// Layout: GenFwd is what a forward leaves behind; Gen::forward (the whole
// iteration's) or Gen::forward_stacked fills it, Bwd::rest (D forward, loss
// head, D input VJP, Gumbel backward, G backward, flush) reads it.  The entry
// points compose them: whole() = fold workspace, forward, rest; the hoisted
// pair = forward_stacked, then rest_from() = fold workspace, rest.  Gen holds
// a call's context and the forward steps, Bwd adds the Folds and the backward
// steps; the steps the critic iteration issues too are engine.h's.
#include "common.h"
#include "engine.h"

namespace {

using namespace vg_engine;
constexpr int64_t kFoldWsFloats = 1 << 20;  // the split folds' chunk sums (the Python collector sizes them exactly)
constexpr int kCatMax = 6;

struct CatSrc {
  const float* p;
  int w, col0;
};
struct CatSrcs {
  CatSrc s[kCatMax];
  int n;
};

// out [rows][total] = the column blocks of srcs side by side (torch.cat(dim=-1))
__global__ void k_cat_cols(CatSrcs src, int rows, int total, float* __restrict__ out) {
  const long long all = (long long)rows * total;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < all; i += (long long)gridDim.x * blockDim.x) {
    const int r = static_cast<int>(i / total), c = static_cast<int>(i - (long long)r * total);
    int j = 0;
#pragma unroll
    for (int q = 1; q < kCatMax; ++q)
      if (q < src.n && c >= src.s[q].col0) j = q;
    out[i] = src.s[j].p[(long long)r * src.s[j].w + (c - src.s[j].col0)];
  }
}

__global__ void k_add_to(float* __restrict__ a, const float* __restrict__ b, long long n) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    a[i] = a[i] + b[i];
}

int cat_cols(const Ctx& cx, std::initializer_list<std::pair<const float*, int>> parts, int rows, float* out,
             int total) {
  if (cx.dry) return 0;
  CatSrcs s{};
  int col = 0;
  for (const auto& p : parts) {
    if (s.n == kCatMax || !p.first) return VG_EINVAL;
    s.s[s.n++] = CatSrc{p.first, p.second, col};
    col += p.second;
  }
  if (col != total) return VG_EINVAL;
  const long long all = (long long)rows * total;
  const int blocks = static_cast<int>(std::min<long long>((all + 255) / 256, 4096));
  k_cat_cols<<<blocks, 256, 0, static_cast<hipStream_t>(cx.stream)>>>(s, rows, total, out);
  VG_CHECK_LAUNCH();
  return 0;
}

// _ln_fwd's saved state
struct LnS {
  const vg_gen_ln_layer* L;
  const float* x;
  int ldx;
  float *h, *y, *mean, *rstd;
};

// What a generator forward leaves behind for the rest of the iteration: every
// layer's saved state, the widths of em / the MLP encoder's output / the GAT
// encoder's output (hl, hg, ec), the last linear layer's input and the head.
struct GenFwd {
  LnS mfe[VG_GEN_MAX_LAYERS], mlp[VG_GEN_MAX_LAYERS], dec[VG_GEN_MAX_LAYERS];
  GatS genc[VG_GEN_MAX_BLOCKS];
  int32_t hl, hg, ec, a_last_w;
  const float* a_last;
  float *logits, *soft, *hard;
};

// The forward as vg_gen_forward_stacked leaves it for vg_gen_loss_and_grad_from
// (host memory, caller-owned: vg_gen_state_bytes).
struct GenState {
  uint32_t magic;
  int32_t n, copies;
  const float* arena;  // the arena fwd's pointers point into
  int64_t arena_off;   // its floats below this offset hold the state
  GenFwd fwd;
};
constexpr uint32_t kStateMagic = 0x56474753u;

// the layer pointers (LnS::L, GatS::B) of a record copied out of a GenState, from the model
void resolve(GenFwd& f, const vg_gen_model* md) {
  for (int i = 0; i < md->n_mfe; ++i) f.mfe[i].L = &md->mfe[i];
  for (int i = 0; i < md->n_mlp; ++i) f.mlp[i].L = &md->mlp[i];
  for (int i = 0; i < md->n_dec; ++i) f.dec[i].L = &md->dec[i];
  for (int b = 0; b < md->n_gblocks; ++b) f.genc[b].B = &md->gblock[b];
}

// One call's context and the two forwards.
struct Gen {
  Ctx& cx;
  const vg_gen_model* md;
  const vg_gen_batch* bt;
  const int n = bt->n, K = bt->classes, E = bt->g.num_edges;

  int ln_fwd(const float* x, int ldx, const vg_gen_ln_layer& L, LnS* S) const {
    const int m = L.out;
    if (L.in != ldx) return VG_EINVAL;
    *S = LnS{&L, x, ldx, cx.take((int64_t)n * m), cx.take((int64_t)n * m), cx.take(n), cx.take(n)};
    return cx.gemm_ln_act(x, ldx, L, n, S->h, S->y, S->mean, S->rstd);
  }
  // nl such layers one after the other; x / xw: the input, then the last output
  int ln_fwd(const float*& x, int& xw, const vg_gen_ln_layer* L, int nl, LnS* S) const {
    for (int i = 0; i < nl; ++i) {
      VG_TRY(ln_fwd(x, xw, L[i], &S[i]));
      x = S[i].y;
      xw = L[i].out;
    }
    return 0;
  }
  // GATConv -> GraphNorm -> ReLU -> Dropout over the batch graph, one segment
  int gat_fwd(const float* x, int xw, const vg_critic_block& B, float p_drop, uint32_t salt, GatS* S,
              bool projected = false) const {
    return vg_engine::gat_fwd(cx, bt->g, bt->seg_rows, n, x, xw, B, p_drop, bt->seed, bt->iter, salt, S, projected);
  }
  int forward(float* hard, GenFwd* f) const;
  int first_layer(const vg_gen_ln_layer& L, int k, const vg_asrc* src, int nsrc, const float* emvx, int ew, int w0,
                  const float* cat_in, LnS* S, float** y_out) const;
  int later_layer(const float* xin, int kin, const vg_gen_ln_layer& L, int k, LnS* S, float** y_out) const;
  int forward_stacked(const vg_gen_stack* sk, float* hard_all, float* soft_all, GenFwd* f) const;
};

// The generator forward of one iteration (models.py:119-155) and the Gumbel
// head; the labels into the caller's hard.
int Gen::forward(float* hard, GenFwd* f) const {
  const int zd = bt->z_dim, vd = bt->vx_w;
  float* z = cx.take((int64_t)n * zd);
  VG_RUN(vg_rng_fill(z, (int64_t)n * zd, 0, bt->seed, bt->iter, bt->z_salt, cx.stream));
  const float* x = bt->mx;
  int xw = bt->mx_w;
  VG_TRY(ln_fwd(x, xw, md->mfe, md->n_mfe, f->mfe));  // models.py:122-131 matched-features encoder
  const float* em = x;
  const int hl = f->hl = xw;
  const int mlp_w = hl + vd + zd;
  float* mlp_in = cx.take((int64_t)n * mlp_w);
  VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, vd}, {z, zd}}, n, mlp_in, mlp_w));
  x = mlp_in;
  xw = mlp_w;
  VG_TRY(ln_fwd(x, xw, md->mlp, md->n_mlp, f->mlp));
  const float* xm = x;
  const int hg = f->hg = xw;
  for (int b = 0; b < md->n_gblocks; ++b) {
    VG_TRY(gat_fwd(x, xw, md->gblock[b], md->p_drop_g, bt->g_keep_salt[b], &f->genc[b]));
    x = f->genc[b].Y;
    xw = f->genc[b].c;
  }
  const float* enc = x;
  const int ec = f->ec = xw;
  const int dec_w = ec + hg + hl + vd + zd;  // models.py:145
  float* dec_in = cx.take((int64_t)n * dec_w);
  VG_TRY(cat_cols(cx, {{enc, ec}, {xm, hg}, {em, hl}, {bt->vx, vd}, {z, zd}}, n, dec_in, dec_w));
  x = dec_in;
  xw = dec_w;
  VG_TRY(ln_fwd(x, xw, md->dec, md->n_dec, f->dec));
  const vg_critic_linear& last = md->dec_last;
  if (last.in != xw || last.out != K) return VG_EINVAL;
  f->logits = cx.take((int64_t)n * K);
  VG_TRY(cx.gemm(x, xw, last.weight, xw, 1, f->logits, K, n, K, xw, last.bias));
  f->a_last = x;
  f->a_last_w = xw;
  float* noise = cx.take((int64_t)n * K);
  VG_RUN(vg_rng_fill(noise, (int64_t)n * K, 2, bt->seed, bt->iter, bt->noise_salt, cx.stream));
  f->soft = cx.take((int64_t)n * K);
  f->hard = hard;
  VG_RUN(vg_gumbel_fwd(f->logits, noise, n, K, md->tau, f->soft, hard, nullptr, cx.stream));
  return 0;
}

// A first [Linear, LayerNorm, LeakyReLU] layer of the stacked forward over k
// label copies + copy k: the label copies from the sources in place plus the
// copy-invariant addend (emvx [n, ew] times L's columns from w0 on), copy k
// from its own concatenated input (cat_in: [n, L.in], filled by the caller)
// with its backward state stored.  *y_out: all (k + 1) n rows.
int Gen::first_layer(const vg_gen_ln_layer& L, int k, const vg_asrc* src, int nsrc, const float* emvx, int ew, int w0,
                     const float* cat_in, LnS* S, float** y_out) const {
  const int m = L.out;
  const int64_t Rk = (int64_t)k * n;
  if (m <= 64 || m > 128) return VG_EINVAL;
  float* add = cx.take((int64_t)n * m);
  VG_TRY(cx.gemm(emvx, ew, at(L.weight, w0), L.in, 1, add, m, n, m, ew, L.bias));
  float* y = *y_out = cx.take((Rk + n) * m);
  VG_RUN(vg_gemm_ln_act_ms(src, nsrc, L.weight, L.in, static_cast<int32_t>(Rk), m, nullptr, add, m, n, L.ln_weight,
                           L.ln_bias, L.ln_eps, L.slope, y, m, cx.stream));
  *S = LnS{&L, cat_in, L.in, cx.take((int64_t)n * m), at(y, Rk * m), cx.take(n), cx.take(n)};
  return cx.gemm_ln_act(cat_in, L.in, L, n, S->h, S->y, S->mean, S->rstd);
}

// a later layer over all (k + 1) n rows, copy k's backward state stored
int Gen::later_layer(const float* xin, int kin, const vg_gen_ln_layer& L, int k, LnS* S, float** y_out) const {
  const int m = L.out;
  const int64_t Rk = (int64_t)k * n;
  if (L.in != kin) return VG_EINVAL;
  float* y = *y_out = cx.take((Rk + n) * m);
  *S = LnS{&L, at(xin, Rk * kin), kin, cx.take((int64_t)n * m), at(y, Rk * m), cx.take(n), cx.take(n)};
  VG_RUN(vg_gemm_ln_act_from(xin, kin, L.weight, static_cast<int32_t>(Rk + n), m, kin, L.bias, L.ln_weight, L.ln_bias,
                             L.ln_eps, L.slope, static_cast<int32_t>(Rk), S->h, y, S->mean, S->rstd, cx.stream));
  return 0;
}

// The forward over copies + 1 stacked copies of the batch: copies 0 .. k - 1 as
// VoxelGNNGenerator._forward_stacked_nograd issues them (the critic labels),
// copy k the generator iteration's forward -- the arithmetic of Gen::forward,
// row for row, in the label copies' launches; *f is copy k's record.  Its draws
// use the counter value the generator iteration will see (*iter + iter_delta)
// at the indices an n-row launch would use.  The first MLP-encoder and decoder
// layers of copy k stay their own n-row launches: the label copies form them
// with vg_gemm_ln_act_ms and a shared addend, another summation order than the
// concatenate + vg_gemm_ln_act of the generator iteration.  f32 only.
int Gen::forward_stacked(const vg_gen_stack* sk, float* hard_all, float* soft_all, GenFwd* f) const {
  const int k = sk->copies, zd = bt->z_dim, vd = bt->vx_w;
  const int64_t R = (int64_t)(k + 1) * n, Rk = (int64_t)k * n, dl = sk->iter_delta;
  const vg_csr_ref& gs = sk->gs;
  float* z = cx.take(R * zd);
  VG_RUN(vg_rng_fill(z, Rk * zd, 0, bt->seed, bt->iter, bt->z_salt, cx.stream));
  VG_RUN(vg_rng_fill_at(at(z, Rk * zd), (int64_t)n * zd, 0, bt->seed, bt->iter, dl, bt->z_salt, cx.stream));
  const float* zt = at(z, Rk * zd);
  const float* em = bt->mx;
  int xw = bt->mx_w;
  VG_TRY(ln_fwd(em, xw, md->mfe, md->n_mfe, f->mfe));  // once per step: the same em for every copy
  const int hl = f->hl = xw;
  float* emvx = cx.take((int64_t)n * (hl + vd));
  VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, vd}}, n, emvx, hl + vd));
  const int mlp_w = hl + vd + zd;
  if (md->mlp[0].in != mlp_w) return VG_EINVAL;
  float* mlp_in = cx.take((int64_t)n * mlp_w);
  VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, vd}, {zt, zd}}, n, mlp_in, mlp_w));
  float* y = nullptr;
  {
    const vg_asrc src[1] = {{z, zd, zd, hl + vd, 0}};
    VG_TRY(first_layer(md->mlp[0], k, src, 1, emvx, hl + vd, 0, mlp_in, &f->mlp[0], &y));
  }
  xw = md->mlp[0].out;
  for (int i = 1; i < md->n_mlp; ++i) {
    VG_TRY(later_layer(y, xw, md->mlp[i], k, &f->mlp[i], &y));
    xw = md->mlp[i].out;
  }
  const float* xm = y;
  const int hg = f->hg = xw;
  // GAT blocks over the stacked graph, one GraphNorm segment per copy
  if (gs.num_nodes != R || gs.num_edges != (int64_t)(k + 1) * E) return VG_EINVAL;
  const float* xb = xm;               // the block's input, all R rows (NULL: the pending GraphNorm's)
  const float* xt = at(xm, Rk * hg);  // copy k's rows of it
  bool pend = false;
  vg_gn_apply desc{};
  const float* pend_O = nullptr;
  for (int b = 0; b < md->n_gblocks; ++b) {
    const vg_critic_block& B = md->gblock[b];
    const int c = B.out, cin = B.in;
    if (cin != xw) return VG_EINVAL;
    const int g = vg_gat_gnp_rows(static_cast<int32_t>(R), c);
    // the same aggregation form (64-channel slices or not: C = 128 keeps its
    // partial-block rows across the two) and partial blocks at n, k n and
    // (k + 1) n rows
    const int sl = vg_gat_fwd_sliced(static_cast<int32_t>(R), c);
    if (g <= 0 || n < g || vg_gat_gnp_rows(n, c) != g || vg_gat_gnp_rows(static_cast<int32_t>(Rk), c) != g ||
        vg_gat_fwd_sliced(n, c) != sl || vg_gat_fwd_sliced(static_cast<int32_t>(Rk), c) != sl)
      return VG_EINVAL;
    float* H = cx.take(R * c);
    float* a_s = cx.take(R);
    float* a_d = cx.take(R);
    float* O = cx.take(R * c);
    float* alpha = cx.take((int64_t)(k + 1) * E);
    float* gnp = cx.take(vg_gat_gnp_floats(static_cast<int32_t>(R), c));
    float* stats = cx.take((int64_t)(k + 1) * 2 * c);
    float* keep_t = cx.take((int64_t)n * c);
    if (pend)
      VG_RUN(vg_gat_lin_att_gn(pend_O, B.lin_weight, static_cast<int32_t>(R), cin, c, B.att_src, B.att_dst, H, a_s, a_d,
                               &desc, cx.stream));
    else
      VG_RUN(vg_gat_lin_att(xb, cin, B.lin_weight, static_cast<int32_t>(R), cin, c, B.att_src, B.att_dst, H, a_s, a_d,
                            cx.stream));
    pend = false;
    VG_RUN(vg_gat_aggregate_fwd_gnp(gs.row_ptr, gs.col, gs.ell, gs.ell ? gs.ell_width : 0, static_cast<int32_t>(R), c, H,
                                    a_s, a_d, B.bias, B.slope, O, alpha, n, gnp, cx.stream));
    GatS& s = f->genc[b] = GatS{&B, xt, cin, c};  // copy k's rows
    s.H = at(H, Rk * c), s.O = at(O, Rk * c), s.alpha = at(alpha, (int64_t)k * E);
    s.a_s = at(a_s, Rk), s.a_d = at(a_d, Rk), s.stats = at(stats, (int64_t)k * 2 * c), s.keep = keep_t;
    const uint32_t salt = bt->g_keep_salt[b];
    const int nxt = b + 1 < md->n_gblocks ? md->gblock[b + 1].out : 0;
    if (0 < nxt && nxt <= 64 && c <= 128 && c % 4 == 0) {  // applied in the next block's projection
      VG_RUN(vg_graphnorm_stats_gnp(k + 1, n, c, gnp, g, B.gn_mean_scale, B.gn_eps, stats, cx.stream));
      s.Y = cx.take((int64_t)n * c);
      desc = vg_gn_apply{stats, B.gn_weight, B.gn_bias, B.gn_mean_scale, nullptr, B.gn_eps, md->p_drop_g, n, salt,
                         bt->seed, bt->iter, nullptr, nullptr,
                         vg_draw_tail{static_cast<int32_t>(Rk), salt, dl, keep_t, s.Y}};
      pend = true;
      pend_O = O;
      xb = nullptr;
    } else {
      float* yb = cx.take(R * c);
      const vg_draw_tail tail{static_cast<int32_t>(Rk), salt, dl, keep_t, nullptr};
      VG_RUN(vg_graphnorm_fwd_gnp_tail(O, k + 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, md->p_drop_g, bt->seed,
                                       bt->iter, salt, B.gn_eps, yb, nullptr, stats, gnp, g, &tail, cx.stream));
      s.Y = at(yb, Rk * c);
      xb = yb;
    }
    xt = s.Y;
    xw = c;
  }
  if (pend) return VG_EINVAL;  // (the last block's GraphNorm is always applied: nxt = 0)
  const float* enc = xb;
  const int ec = f->ec = xw;
  const int dec_w = ec + hg + hl + vd + zd;  // models.py:145
  if (md->dec[0].in != dec_w) return VG_EINVAL;
  float* dec_in = cx.take((int64_t)n * dec_w);
  VG_TRY(cat_cols(cx, {{at(enc, Rk * ec), ec}, {at(xm, Rk * hg), hg}, {em, hl}, {bt->vx, vd}, {zt, zd}}, n, dec_in,
                  dec_w));
  {
    const vg_asrc src[3] = {{enc, ec, ec, 0, 0}, {xm, hg, hg, ec, 0}, {z, zd, zd, ec + hg + hl + vd, 0}};
    VG_TRY(first_layer(md->dec[0], k, src, 3, emvx, hl + vd, ec + hg, dec_in, &f->dec[0], &y));
  }
  xw = md->dec[0].out;
  for (int i = 1; i < md->n_dec; ++i) {
    VG_TRY(later_layer(y, xw, md->dec[i], k, &f->dec[i], &y));
    xw = md->dec[i].out;
  }
  const vg_critic_linear& last = md->dec_last;
  if (last.in != xw || last.out != K) return VG_EINVAL;
  float* lg = cx.take(R * K);
  VG_TRY(cx.gemm(y, xw, last.weight, xw, 1, lg, K, static_cast<int>(R), K, xw, last.bias));
  float* noise = cx.take(R * K);
  VG_RUN(vg_rng_fill(noise, Rk * K, 2, bt->seed, bt->iter, bt->noise_salt, cx.stream));
  VG_RUN(vg_rng_fill_at(at(noise, Rk * K), (int64_t)n * K, 2, bt->seed, bt->iter, dl, bt->noise_salt, cx.stream));
  VG_RUN(vg_gumbel_fwd(lg, noise, static_cast<int32_t>(R), K, md->tau, soft_all, hard_all, nullptr, cx.stream));
  f->a_last = at(static_cast<const float*>(y), Rk * xw);
  f->a_last_w = xw;
  f->logits = at(lg, Rk * K), f->soft = at(soft_all, Rk * K), f->hard = at(hard_all, Rk * K);
  return 0;
}

// The steps of the backward, their folds and weight-gradient products
// collected in folds, and the iteration from a finished forward on.
struct Bwd : Gen {
  Folds& folds;

  int tn(const float* A, int lda, const float* B, int ldb, int N, int M, int Kk, float* C, int ldc, float* db) const {
    float* ws = cx.take(std::max<int64_t>(1, vg_gemm_tn_ws_floats(N, M, Kk)));
    return folds.tn(cx, A, lda, B, ldb, N, M, Kk, C, ldc, db, N, ws);
  }
  // g_h = d(pre-norm) from g_y; gamma / beta and weight / bias gradients deferred
  int ln_bwd(const LnS& S, const float* g_y, float** g_h_out) const {
    const vg_gen_ln_layer& L = *S.L;
    const int m = L.out, k = L.in;
    float* g_h = *g_h_out = cx.take((int64_t)n * m);
    float* ws = cx.take(vg_ln_act_bwd_ws_floats(m));
    if (!cx.dry) {
      vg_fold f[3];
      int32_t nf = 0;
      VG_TRY(vg_ln_act_bwd_deferred(S.h, n, m, L.ln_weight, L.ln_bias, L.slope, S.mean, S.rstd, g_y, g_h,
                                    L.g_ln_weight, L.g_ln_bias, 1, ws, f, &nf, cx.stream));
      folds.add(f, nf);
    }
    return tn(g_h, m, S.x, S.ldx, n, m, k, L.g_weight, k, L.g_bias);
  }
  // ln_bwd through S[nl - 1] .. S[0] from g (the top layer's output gradient):
  // *g_h the bottom layer's pre-norm gradient, its dX product left to the caller
  int ln_bwd(const LnS* S, int nl, const float* g, float** g_h) const {
    for (int i = nl - 1; i >= 0; --i) {
      VG_TRY(ln_bwd(S[i], g, g_h));
      if (i == 0) break;
      const int m = S[i].L->out, k = S[i].L->in;
      float* gx = cx.take((int64_t)n * k);
      VG_TRY(cx.gemm(*g_h, m, S[i].L->weight, k, 0, gx, k, n, k, m));
      g = gx;
    }
    return 0;
  }
  // o [n, m] = A Wt, the output gradient of S's GraphNorm; that backward's
  // column partials from the GEMM epilogue (*tp; NULL when m % 4 != 0)
  // (taken: the partials' buffer where the caller took it already)
  int gemm_dy(const float* A, int lda, const float* Wt, int ldw, float* o, int m, int k, const GatS& S, float* taken,
              float** tp) const {
    if (m % 4 != 0) {
      *tp = nullptr;
      return cx.gemm(A, lda, Wt, ldw, 0, o, m, n, m, k);
    }
    *tp = taken ? taken : cx.take(vg_gemm_gn_tpart_floats(n, m));
    return cx.gemm_gn_bwd(A, lda, Wt, ldw, n, m, k, o, S, n, *tp);
  }
  // GraphNorm(+ReLU+Dropout) and GATConv backward of one block: dH; with
  // pgrads the block's GraphNorm and attention / bias gradients (deferred).
  // dx / *fused: vg_engine::gat_bwd's
  int gat_bwd(const GatS& S, const float* g_y, const float* tp, bool pgrads, float** dH_out, const vg_dx_in* dx,
              bool* fused) const {
    const vg_critic_block& B = *S.B;
    const int c = S.c, acc = pgrads ? 1 : 0;
    float* dO = cx.take((int64_t)n * c);
    float* dH = *dH_out = cx.take((int64_t)n * c);
    float* ws = cx.take(vg_gat_bwd_ws_floats(n, E, c));
    float* gws = cx.take(vg_graphnorm_seg_ws_floats(1, n, c));
    float *gw = pgrads ? B.g_gn_weight : nullptr, *gb = pgrads ? B.g_gn_bias : nullptr;
    float* gm = pgrads ? B.g_gn_mean_scale : nullptr;
    if (tp)
      VG_RUN(vg_graphnorm_bwd_seg_tiles(S.O, 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, S.keep, B.gn_eps, S.stats,
                                        g_y, tp, nullptr, gw, gb, gm, acc, nullptr, 0, gws, cx.stream));
    else
      VG_RUN(vg_graphnorm_bwd_seg(S.O, 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, S.keep, B.gn_eps, S.stats, g_y,
                                  nullptr, gw, gb, gm, acc, nullptr, 0, gws, bt->sync, cx.stream));
    const vg_gn_bwd_in gn{S.O,     S.keep,  g_y, nullptr, B.gn_weight, B.gn_bias, B.gn_mean_scale,
                          S.stats, at(gws, vg_graphnorm_bwd_sums_offset(1, c)), B.gn_eps, 1, n, 0};
    return vg_engine::gat_bwd(cx, folds, bt->g, S, gn, dO, dH, ws, pgrads, nullptr, 0, dx, fused);
  }
  // The backward through the blocks S[nb - 1] .. S[0] from the top block's
  // output gradient g_y (tp: its GraphNorm partials, or NULL): a block's dX is
  // the g_y of the one below, formed in the GAT source pass's launch where
  // gat_bwd can; with pgrads the blocks' parameter gradients (D's input VJP
  // takes none).  Block 0's dX product is the caller's: *dH0 is its dH.
  int blocks_bwd(const GatS* S, int nb, const float* g_y, float* tp, bool pgrads, float** dH0) const {
    for (int b = nb - 1; b >= 0; --b) {
      const GatS& T = S[b];
      const int c = T.c, cin = T.xw;
      const float* Wl = T.B->lin_weight;
      float* dX = b > 0 ? cx.take((int64_t)n * cin) : nullptr;
      float* tpx = b > 0 && cin % 4 == 0 ? cx.take(vg_gemm_gn_tpart_floats(n, cin)) : nullptr;
      const vg_dx_in dx = tpx ? dx_in(Wl, cin, dX, cin, S[b - 1], n, tpx) : vg_dx_in{};
      bool fused;
      VG_TRY(gat_bwd(T, g_y, tp, pgrads, dH0, tpx ? &dx : nullptr, &fused));
      if (pgrads) VG_TRY(tn(*dH0, c, T.X, cin, n, c, cin, T.B->g_lin_weight, cin, nullptr));
      if (b == 0) break;
      if (!fused) VG_TRY(gemm_dy(*dH0, c, Wl, cin, dX, cin, c, S[b - 1], tpx, &tp));
      else tp = tpx;
      g_y = dX;
    }
    return 0;
  }
  int rest(const GenFwd& f, float* out) const;
};

// The iteration after G's forward f: D(label_hard) in train mode, the loss
// head, D's input VJP, the Gumbel backward, G's backward, the grouped flush.
int Bwd::rest(const GenFwd& f, float* out) const {
  // ------------------------------------------------- discriminator forward
  const int F = bt->mvx_w, nd = md->n_ddec, nm = md->n_dmlp, nb = md->n_dblocks;
  float* X0 = cx.take((int64_t)n * (F + K));
  VG_TRY(cat_cols(cx, {{bt->mvx, F}, {f.hard, K}}, n, X0, F + K));
  float *d_mlp_out[VG_GEN_MAX_LAYERS], *dec_out[VG_GEN_MAX_LAYERS], *adj[VG_GEN_MAX_LAYERS], *adj_m[VG_GEN_MAX_LAYERS];
  const float* x = X0;
  int xw = F + K;
  std::vector<vg_gemm_link> enc;  // D's MLP encoder and block 0's projection: row-local, one chain
  for (int i = 0; i < nm; ++i) {
    const vg_critic_linear& L = md->dmlp[i];
    if (L.in != xw) return VG_EINVAL;
    float* y = d_mlp_out[i] = cx.take((int64_t)n * L.out);
    enc.push_back(gemm_link(L.weight, xw, 0, L.out, y, L.bias, kActRelu, nullptr));
    x = y;
    xw = L.out;
  }
  GatS denc[VG_GEN_MAX_BLOCKS];
  if (md->dblock[0].in != xw) return VG_EINVAL;
  denc[0] = gat_proj_take(cx, n, x, xw, md->dblock[0]);
  enc.push_back(att_link(md->dblock[0], xw, denc[0].H, denc[0].a_s, denc[0].a_d));
  VG_TRY(cx.links_or_gemms(X0, F + K, F + K, n, enc));
  for (int b = 0; b < nb; ++b) {
    VG_TRY(gat_fwd(x, xw, md->dblock[b], md->p_drop_d, bt->d_keep_salt[b], &denc[b], b == 0));
    x = denc[b].Y;
    xw = denc[b].c;
  }
  for (int i = 0; i < nd; ++i) dec_out[i] = cx.take((int64_t)n * md->ddec[i].out);
  VG_TRY(cx.chain_or_gemms(x, xw, n, fwd_chain(md->ddec, nd, dec_out, xw)));
  if (md->ddec[nd - 1].out != 1) return VG_EINVAL;
  const float* d_fake = dec_out[nd - 1];

  // ------------------------------------------------------------- loss head
  const int ng = bt->num_graphs;
  float* far_gen = cx.take(ng);
  float* far_ref = cx.take(ng);
  VG_RUN(vg_far_per_graph(bt->vx, bt->vx_w, f.hard, K, bt->graph_ptr, ng, bt->site_area, bt->far_col, bt->dy_col,
                          bt->dx_col, md->dim_scale, md->void_class, far_gen, far_ref, cx.stream));
  float* lws = cx.take(vg_gen_loss_ws_floats(n, K));
  VG_RUN(vg_gen_loss_fwd(d_fake, f.hard, f.logits, bt->onehot, bt->type, n, K, far_gen, far_ref, ng, md->lambda_adv,
                         md->lambda_label, md->lambda_ratio, md->lambda_void, md->lambda_far, out, lws, cx.stream));
  float* g_d = cx.take(n);
  float* g_hard = cx.take((int64_t)n * K);
  float* g_l = md->lambda_label != 0.f ? cx.take((int64_t)n * K) : nullptr;
  VG_RUN(vg_gen_loss_bwd(bt->one, out, f.logits, bt->type, n, K, g_d, g_hard, g_l, cx.stream));

  // --------------------------- discriminator input VJP (no parameter grads)
  for (int i = 0; i < nd - 1; ++i) adj[i] = cx.take((int64_t)n * md->ddec[i].out);
  adj[nd - 1] = g_d;
  VG_TRY(cx.chain_or_gemms(g_d, 1, n, adj_chain(md->ddec, nd, dec_out, adj, 0, 0)));
  const vg_critic_linear& W = md->ddec[0];
  float* dY = cx.take((int64_t)n * W.in);
  float *tp = nullptr, *dH = nullptr;
  VG_TRY(gemm_dy(adj[0], W.out, W.weight, W.in, dY, W.in, W.out, denc[nb - 1], nullptr, &tp));
  for (int i = 0; i < nm; ++i) adj_m[i] = cx.take((int64_t)n * md->dmlp[i].out);
  VG_TRY(blocks_bwd(denc, nb, dY, tp, false, &dH));
  // block 0's masked dX, the MLP's adjoints and the label columns' adjoint: row-local, one chain
  const vg_critic_linear& W0 = md->dmlp[0];
  float* g_lab = cx.take((int64_t)n * K);
  std::vector<vg_gemm_link> tail;
  tail.push_back(gemm_link(denc[0].B->lin_weight, denc[0].xw, 1, denc[0].xw, adj_m[nm - 1], nullptr, kActMask,
                           d_mlp_out[nm - 1]));
  for (int i = nm - 1; i >= 1; --i) {
    const int m = md->dmlp[i].in;
    tail.push_back(gemm_link(md->dmlp[i].weight, m, 1, m, adj_m[i - 1], nullptr, kActMask, d_mlp_out[i - 1]));
  }
  // label_hard feeds the loss head and D (models.py:229-239): both adjoints summed in the product's epilogue
  tail.push_back(gemm_link(W0.weight + F, W0.in, 1, K, g_lab, nullptr, kActAdd, g_hard));
  VG_TRY(cx.links_or_gemms(dH, denc[0].c, denc[0].c, n, tail));

  // ----------------------------------------------------- Gumbel backward
  float* g_logits = cx.take((int64_t)n * K);
  VG_RUN(vg_gumbel_bwd(f.soft, g_lab, nullptr, n, K, md->tau, g_logits, cx.stream));
  if (g_l && !cx.dry) {
    const long long all = (long long)n * K;
    k_add_to<<<static_cast<int>(std::min<long long>((all + 255) / 256, 4096)), 256, 0,
               static_cast<hipStream_t>(cx.stream)>>>(g_logits, g_l, all);
    VG_CHECK_LAUNCH();
  }

  // -------------------------------------------------- generator backward
  const vg_critic_linear& last = md->dec_last;
  const int hl = f.hl, hg = f.hg, ec = f.ec, lw = f.a_last_w;
  VG_TRY(tn(g_logits, K, f.a_last, lw, n, K, lw, last.g_weight, lw, last.g_bias));
  float* g = cx.take((int64_t)n * lw);
  VG_TRY(cx.gemm(g_logits, K, last.weight, lw, 0, g, lw, n, lw, K));
  float* g_h = nullptr;
  VG_TRY(ln_bwd(f.dec, md->n_dec, g, &g_h));
  const vg_gen_ln_layer& Ld = md->dec[0];
  const int md_ = Ld.out, kd = Ld.in;
  float* g_enc = cx.take((int64_t)n * ec);
  VG_TRY(gemm_dy(g_h, md_, Ld.weight, kd, g_enc, ec, md_, f.genc[md->n_gblocks - 1], nullptr, &tp));
  float* g_xem = cx.take((int64_t)n * (hg + hl));  // [x | em] columns of the decoder input (enc taken above)
  VG_TRY(cx.gemm(g_h, md_, Ld.weight + ec, kd, 0, g_xem, hg + hl, n, hg + hl, md_));
  VG_TRY(blocks_bwd(f.genc, md->n_gblocks, g_enc, tp, true, &dH));
  const GatS& G0 = f.genc[0];  // x feeds the encoder and the decoder (models.py:132-145)
  g = cx.take((int64_t)n * G0.xw);
  VG_TRY(cx.gemm(dH, G0.c, G0.B->lin_weight, G0.xw, 0, g, G0.xw, n, G0.xw, G0.c, nullptr, kActAdd, g_xem, hg + hl));
  VG_TRY(ln_bwd(f.mlp, md->n_mlp, g, &g_h));
  {  // the em columns of [em | voxel.x | z]: em feeds the MLP encoder and the decoder
    const vg_gen_ln_layer& L = md->mlp[0];
    g = cx.take((int64_t)n * hl);
    VG_TRY(cx.gemm(g_h, L.out, L.weight, L.in, 0, g, hl, n, hl, L.out, nullptr, kActAdd, at(g_xem, hg), hg + hl));
  }
  VG_TRY(ln_bwd(f.mfe, md->n_mfe, g, &g_h));
  return folds.flush(cx);
}

// The whole iteration.  The fold workspace is the arena's first block.
int whole(Ctx& cx, const vg_gen_model* md, const vg_gen_batch* bt, float* out, float* hard) {
  Folds folds(cx, kFoldWsFloats);
  GenFwd f{};
  VG_TRY((Gen{cx, md, bt}).forward(hard, &f));
  return Bwd{{cx, md, bt}, folds}.rest(f, out);
}

// The iteration from a forward that ran ahead (f, below cx.off) on.  The fold
// workspace is the first block above it.
int rest_from(Ctx& cx, const vg_gen_model* md, const vg_gen_batch* bt, const GenFwd& f, float* out) {
  Folds folds(cx, kFoldWsFloats);
  return Bwd{{cx, md, bt}, folds}.rest(f, out);
}

bool model_ok(const vg_gen_model* md, const vg_gen_batch* bt) {
  if (!md || !bt) return false;
  auto in_range = [](int v, int hi) { return v >= 1 && v <= hi; };
  if (!in_range(md->n_mfe, VG_GEN_MAX_LAYERS) || !in_range(md->n_mlp, VG_GEN_MAX_LAYERS) ||
      !in_range(md->n_dec, VG_GEN_MAX_LAYERS) || !in_range(md->n_gblocks, VG_GEN_MAX_BLOCKS) ||
      !in_range(md->n_dmlp, VG_GEN_MAX_LAYERS) || !in_range(md->n_dblocks, VG_GEN_MAX_BLOCKS) ||
      !in_range(md->n_ddec, VG_GEN_MAX_LAYERS))
    return false;
  if (bt->n < 64 || bt->classes < 1 || bt->mx_w < 1 || bt->vx_w < 1 || bt->mvx_w < 1 || bt->z_dim < 1 ||
      bt->num_graphs < 1 || bt->g.num_nodes != bt->n || bt->seg_rows != bt->n)
    return false;
  if (md->mfe[0].in != bt->mx_w || md->dmlp[0].in != bt->mvx_w + bt->classes) return false;
  return true;
}

}  // namespace

extern "C" int64_t vg_gen_arena_floats(const vg_gen_model* model, const vg_gen_batch* batch) {
  if (!model_ok(model, batch)) return -1;
  Ctx cx{true, model->bf16, nullptr, nullptr, 0, 0};
  if (whole(cx, model, batch, nullptr, nullptr)) return -1;
  return cx.off;
}

extern "C" int vg_gen_loss_and_grad(const vg_gen_model* model, const vg_gen_batch* batch, float* arena,
                                    int64_t arena_floats, float* out, float* hard, void* stream) {
  if (!model_ok(model, batch) || !arena || !out || !hard || !batch->mx || !batch->vx || !batch->mvx ||
      !batch->onehot || !batch->type || !batch->graph_ptr || !batch->site_area || !batch->iter || !batch->one ||
      !batch->g.row_ptr || !batch->g.col || !batch->g.csc_ptr || !batch->g.csc_slot || !batch->g.csc_dst)
    return VG_EINVAL;
  if (reinterpret_cast<uintptr_t>(arena) & 255) return VG_EINVAL;
  const int64_t need = vg_gen_arena_floats(model, batch);
  if (need < 0 || need > arena_floats) return VG_EINVAL;
  Ctx cx{false, model->bf16, stream, arena, arena_floats, 0};
  return whole(cx, model, batch, out, hard);
}

namespace {

bool stack_ok(const vg_gen_model* md, const vg_gen_batch* bt, const vg_gen_stack* sk) {
  if (!model_ok(md, bt) || !sk || md->bf16 || sk->copies < 1 || sk->iter_delta < 0) return false;
  const int64_t rows = (int64_t)(sk->copies + 1) * bt->n;
  return rows < (1LL << 31) / 128 * 4 && sk->gs.num_nodes == rows;
}

}  // namespace

extern "C" int64_t vg_gen_state_bytes(void) { return (int64_t)sizeof(GenState); }

extern "C" int64_t vg_gen_hoist_arena_floats(const vg_gen_model* model, const vg_gen_batch* batch,
                                             const vg_gen_stack* stack) {
  if (!stack_ok(model, batch, stack)) return -1;
  Ctx cx{true, 0, nullptr, nullptr, 0, 0};
  GenFwd f{};
  if ((Gen{cx, model, batch}).forward_stacked(stack, nullptr, nullptr, &f)) return -1;
  if (rest_from(cx, model, batch, f, nullptr)) return -1;  // continues above the state
  return cx.off;
}

extern "C" int vg_gen_forward_stacked(const vg_gen_model* model, const vg_gen_batch* batch, const vg_gen_stack* stack,
                                      float* arena, int64_t arena_floats, float* hard_all, float* soft_all,
                                      void* state, void* stream) {
  if (!stack_ok(model, batch, stack) || !arena || !hard_all || !soft_all || !state || !batch->mx || !batch->vx ||
      !batch->iter || !stack->gs.row_ptr || !stack->gs.col)
    return VG_EINVAL;
  if (reinterpret_cast<uintptr_t>(arena) & 255) return VG_EINVAL;
  const int64_t need = vg_gen_hoist_arena_floats(model, batch, stack);
  if (need < 0 || need > arena_floats) return VG_EINVAL;
  GenState* st = static_cast<GenState*>(state);
  st->magic = 0;
  Ctx cx{false, 0, stream, arena, arena_floats, 0};
  GenFwd f{};
  VG_TRY((Gen{cx, model, batch}).forward_stacked(stack, hard_all, soft_all, &f));
  *st = GenState{kStateMagic, batch->n, stack->copies, cx.base, cx.off, f};
  return 0;
}

extern "C" int vg_gen_loss_and_grad_from(const vg_gen_model* model, const vg_gen_batch* batch, const void* state,
                                         float* arena, int64_t arena_floats, float* out, void* stream) {
  const GenState* in = static_cast<const GenState*>(state);
  if (!model_ok(model, batch) || model->bf16 || !in || in->magic != kStateMagic || in->n != batch->n || !arena ||
      in->arena != arena ||
      !out || !batch->mvx || !batch->vx || !batch->onehot || !batch->type || !batch->graph_ptr || !batch->site_area ||
      !batch->iter || !batch->one || !batch->g.row_ptr || !batch->g.col || !batch->g.csc_ptr || !batch->g.csc_slot ||
      !batch->g.csc_dst)
    return VG_EINVAL;
  if (reinterpret_cast<uintptr_t>(arena) & 255) return VG_EINVAL;
  GenFwd f = in->fwd;
  resolve(f, model);
  if (model->dec_last.in != f.a_last_w || model->dec_last.out != batch->classes) return VG_EINVAL;
  Ctx cx{false, 0, stream, arena, arena_floats, in->arena_off};
  Ctx dry{true, 0, nullptr, nullptr, 0, in->arena_off};
  if (rest_from(dry, model, batch, f, nullptr) || dry.off > arena_floats) return VG_EINVAL;
  return rest_from(cx, model, batch, f, out);
}
