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
#include "common.h"
#include "engine.h"

namespace {

using vg_engine::Ctx;
using vg_engine::Folds;
using vg_engine::kActAdd;
using vg_engine::kActMask;
using vg_engine::kActNone;
using vg_engine::kActRelu;
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

// _gat_fwd's saved state
struct GatS {
  const vg_critic_block* B;
  const float* X;
  int xw, c;
  float *H, *O, *alpha, *a_s, *a_d, *Y, *stats, *keep;
};

// The generator forward's state as vg_gen_forward_stacked leaves it for
// vg_gen_loss_and_grad_from (host memory, caller-owned: vg_gen_state_bytes).
// The layer pointers (LnS::L, GatS::B) are re-resolved from the model on load.
struct GenState {
  uint32_t magic;
  int32_t n, copies;
  const float* arena;  // the arena the pointers below point into
  int64_t arena_off;   // its floats below this offset hold the state
  LnS mfe[VG_GEN_MAX_LAYERS], mlp[VG_GEN_MAX_LAYERS], dec[VG_GEN_MAX_LAYERS];
  GatS genc[VG_GEN_MAX_BLOCKS];
  int32_t hl, hg, ec, a_last_w;
  const float* a_last;
  float *logits, *soft, *hard;
};
constexpr uint32_t kStateMagic = 0x56474753u;

enum Mode { kWhole = 0, kStackedFwd = 1, kFromState = 2 };

// p + off, NULL in a dry (sizing) pass
template <class T>
T* at(T* p, int64_t off) {
  return p ? p + off : nullptr;
}

struct StackIO {
  const vg_gen_stack* sk;
  float *hard_all, *soft_all;
};

int run(Ctx& cx, const vg_gen_model* md, const vg_gen_batch* bt, float* out, float* hard, Mode mode = kWhole,
        GenState* st = nullptr, const StackIO* io = nullptr) {
  const int n = bt->n, K = bt->classes, E = bt->g.num_edges;
  const vg_csr_ref& g1 = bt->g;
  Folds folds;
  if (mode != kStackedFwd) {
    folds.ws = cx.take(kFoldWsFloats);
    folds.ws_floats = kFoldWsFloats;
  }

  auto ln_fwd = [&](const float* x, int ldx, const vg_gen_ln_layer& L, LnS* S) -> int {
    const int m = L.out, k = L.in;
    if (k != ldx) return VG_EINVAL;
    *S = LnS{&L, x, ldx, cx.take((int64_t)n * m), cx.take((int64_t)n * m), cx.take(n), cx.take(n)};
    if (cx.dry) return 0;
    return cx.bf16 ? vg_gemm_ln_act_bf16(x, ldx, L.weight, n, m, k, L.bias, L.ln_weight, L.ln_bias, L.ln_eps, L.slope,
                                         S->h, S->y, S->mean, S->rstd, cx.stream)
                   : vg_gemm_ln_act(x, ldx, L.weight, n, m, k, L.bias, L.ln_weight, L.ln_bias, L.ln_eps, L.slope, S->h,
                                    S->y, S->mean, S->rstd, cx.stream);
  };
  auto tn = [&](const float* A, int lda, const float* B, int ldb, int N, int M, int Kk, float* C, int ldc,
                float* db) -> int {
    float* ws = cx.take(std::max<int64_t>(1, vg_gemm_tn_ws_floats(N, M, Kk)));
    return folds.tn(cx, A, lda, B, ldb, N, M, Kk, C, ldc, db, N, ws);
  };
  // g_h = d(pre-norm) from g_y; gamma / beta and weight / bias gradients deferred
  auto ln_bwd = [&](const LnS& S, const float* g_y, float** g_h_out) -> int {
    const vg_gen_ln_layer& L = *S.L;
    const int m = L.out, k = L.in;
    float* g_h = cx.take((int64_t)n * m);
    float* ws = cx.take(vg_ln_act_bwd_ws_floats(m));
    *g_h_out = g_h;
    if (!cx.dry) {
      vg_fold f[3];
      int32_t nf = 0;
      VG_TRY(vg_ln_act_bwd_deferred(S.h, n, m, L.ln_weight, L.ln_bias, L.slope, S.mean, S.rstd, g_y, g_h,
                                    L.g_ln_weight, L.g_ln_bias, 1, ws, f, &nf, cx.stream));
      folds.add(f, nf);
    }
    return tn(g_h, m, S.x, S.ldx, n, m, k, L.g_weight, k, L.g_bias);
  };
  // GATConv -> GraphNorm -> ReLU -> Dropout with the mask drawn in-kernel and stored
  auto gat_fwd = [&](const float* x, int xw, const vg_critic_block& B, float p_drop, uint32_t salt, GatS* S) -> int {
    const int c = B.out;
    if (B.in != xw) return VG_EINVAL;
    const int g = vg_gat_gnp_rows(n, c);
    if (g <= 0 || bt->seg_rows < g || n % bt->seg_rows) return VG_EINVAL;  // (the Python engine's unfused path)
    GatS s{&B, x, xw, c};
    s.H = cx.take((int64_t)n * c);
    s.a_s = cx.take(n);
    s.a_d = cx.take(n);
    s.O = cx.take((int64_t)n * c);
    s.alpha = cx.take(E);
    float* gnp = cx.take(vg_gat_gnp_floats(n, c));
    s.Y = cx.take((int64_t)n * c);
    s.stats = cx.take(2LL * c);
    s.keep = cx.take((int64_t)n * c);
    *S = s;
    VG_RUN(cx.bf16 ? vg_gat_lin_att_bf16(x, xw, B.lin_weight, n, xw, c, B.att_src, B.att_dst, s.H, s.a_s, s.a_d,
                                         cx.stream)
                   : vg_gat_lin_att(x, xw, B.lin_weight, n, xw, c, B.att_src, B.att_dst, s.H, s.a_s, s.a_d, cx.stream));
    VG_RUN(vg_gat_aggregate_fwd_gnp(g1.row_ptr, g1.col, g1.ell, g1.ell ? g1.ell_width : 0, n, c, s.H, s.a_s, s.a_d,
                                    B.bias, B.slope, s.O, s.alpha, bt->seg_rows, gnp, cx.stream));
    VG_RUN(vg_graphnorm_fwd_gnp(s.O, 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, nullptr, p_drop, bt->seed,
                                bt->iter, salt, B.gn_eps, s.Y, s.keep, s.stats, gnp, g, cx.stream));
    return 0;
  };
  // o [n, m] = A Wt, the output gradient of S's GraphNorm; that backward's
  // column partials from the GEMM epilogue (*tp; NULL when m % 4 != 0)
  // (taken: the partials' buffer where the caller took it already)
  auto gemm_dy = [&](const float* A, int lda, const float* Wt, int ldw, float* o, int m, int k, const GatS& S,
                     float* taken, float** tp) -> int {
    if (m % 4 != 0) {
      *tp = nullptr;
      return cx.gemm(A, lda, Wt, ldw, 0, o, m, n, m, k);
    }
    const vg_critic_block& N = *S.B;
    float* t = taken ? taken : cx.take(vg_gemm_gn_tpart_floats(n, m));
    *tp = t;
    if (cx.dry) return 0;
    return cx.bf16 ? vg_gemm_gn_bwd_bf16(A, lda, Wt, ldw, n, m, k, o, m, S.O, S.keep, n, N.gn_weight, N.gn_bias,
                                         N.gn_mean_scale, N.gn_eps, S.stats, t, cx.stream)
                   : vg_gemm_gn_bwd(A, lda, Wt, ldw, n, m, k, o, m, S.O, S.keep, n, N.gn_weight, N.gn_bias,
                                    N.gn_mean_scale, N.gn_eps, S.stats, t, cx.stream);
  };
  // GraphNorm(+ReLU+Dropout) and GATConv backward of one block: dH; with
  // pgrads the block's GraphNorm and attention / bias gradients (deferred).
  // dx: the dX product that consumes dH, run in the source pass's launch where
  // vg_gat_bwd_gn_dx has a kernel for the shape (*fused; else the caller's gemm_dy)
  auto gat_bwd = [&](const GatS& S, const float* g_y, const float* tp, bool pgrads, float** dH_out,
                     const vg_dx_in* dx = nullptr, bool* fused = nullptr) -> int {
    const vg_critic_block& B = *S.B;
    const int c = S.c;
    float* dO = cx.take((int64_t)n * c);
    float* dH = cx.take((int64_t)n * c);
    float* ws = cx.take(vg_gat_bwd_ws_floats(n, E, c));
    float* gws = cx.take(vg_graphnorm_seg_ws_floats(1, n, c));
    *dH_out = dH;
    if (cx.dry) return 0;
    float* gw = pgrads ? B.g_gn_weight : nullptr;
    float* gb = pgrads ? B.g_gn_bias : nullptr;
    float* gm = pgrads ? B.g_gn_mean_scale : nullptr;
    if (tp)
      VG_TRY(vg_graphnorm_bwd_seg_tiles(S.O, 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, S.keep, B.gn_eps, S.stats,
                                        g_y, tp, nullptr, gw, gb, gm, pgrads ? 1 : 0, nullptr, 0, gws, cx.stream));
    else
      VG_TRY(vg_graphnorm_bwd_seg(S.O, 1, n, c, B.gn_weight, B.gn_bias, B.gn_mean_scale, S.keep, B.gn_eps, S.stats, g_y,
                                  nullptr, gw, gb, gm, pgrads ? 1 : 0, nullptr, 0, gws, bt->sync, cx.stream));
    const vg_gn_bwd_in gn{S.O,        S.keep,   g_y, nullptr, B.gn_weight, B.gn_bias, B.gn_mean_scale, S.stats,
                          gws + vg_graphnorm_bwd_sums_offset(1, c), B.gn_eps, 1, n, 0};
    vg_fold f[3];
    int32_t nf = 0;
    float* gas = pgrads ? B.g_att_src : nullptr;
    float* gad = pgrads ? B.g_att_dst : nullptr;
    float* gbi = pgrads ? B.g_bias : nullptr;
    vg_fold* fo = pgrads ? f : nullptr;
    int32_t* no = pgrads ? &nf : nullptr;
    int rc = VG_EINVAL;
    if (dx && !cx.bf16 && vg_bwd_src_gemm_use(n, c))
      rc = vg_gat_bwd_gn_dx(g1.row_ptr, g1.col, g1.csc_ptr, g1.csc_slot, g1.csc_dst, n, E, c, S.H, B.att_src, B.att_dst,
                            S.a_s, S.a_d, S.alpha, &gn, dO, B.slope, dH, gas, gad, gbi, pgrads ? 1 : 0, nullptr, 0, ws, fo,
                            no, dx, cx.stream);
    if (rc == 0)
      *fused = true;
    else if (rc != VG_EINVAL)
      return rc;
    else
      VG_TRY(vg_gat_bwd_gn(g1.row_ptr, g1.col, g1.csc_ptr, g1.csc_slot, g1.csc_dst, n, E, c, S.H, B.att_src, B.att_dst,
                           S.a_s, S.a_d, S.alpha, &gn, dO, B.slope, dH, gas, gad, gbi, pgrads ? 1 : 0, nullptr, 0, ws, fo,
                           no, cx.stream));
    folds.add(f, nf);
    return 0;
  };
  // the dX product of block S (weight Wl, into o [n, m]) below block D's GraphNorm, as vg_gat_bwd_gn_dx takes it
  auto dx_in = [&](const float* Wl, float* o, int m, const GatS& D, float* tpart) {
    const vg_critic_block& N = *D.B;
    return vg_dx_in{Wl, m, m, o, m, D.O, D.keep, n, N.gn_weight, N.gn_bias, N.gn_mean_scale, N.gn_eps, D.stats, tpart};
  };

  // ----------------------------------------------------- generator forward
  std::vector<LnS> mfe_s(md->n_mfe), mlp_s(md->n_mlp), dec_s(md->n_dec);
  std::vector<GatS> genc(md->n_gblocks);
  const vg_critic_linear& last = md->dec_last;
  const float* x = nullptr;
  int xw = 0, hl = 0, hg = 0, ec = 0, a_last_w = 0;
  const float* a_last = nullptr;
  float *logits = nullptr, *soft = nullptr;
  if (mode == kFromState) {  // vg_gen_forward_stacked ran it as the label forward's last copy
    for (int i = 0; i < md->n_mfe; ++i) (mfe_s[i] = st->mfe[i]).L = &md->mfe[i];
    for (int i = 0; i < md->n_mlp; ++i) (mlp_s[i] = st->mlp[i]).L = &md->mlp[i];
    for (int i = 0; i < md->n_dec; ++i) (dec_s[i] = st->dec[i]).L = &md->dec[i];
    for (int b = 0; b < md->n_gblocks; ++b) (genc[b] = st->genc[b]).B = &md->gblock[b];
    hl = st->hl, hg = st->hg, ec = st->ec, a_last_w = st->a_last_w;
    a_last = st->a_last, logits = st->logits, soft = st->soft, hard = st->hard;
    if (last.in != a_last_w || last.out != K) return VG_EINVAL;
  } else if (mode == kStackedFwd) {
    // The forward over copies + 1 stacked copies of the batch: copies 0 ..
    // k - 1 as VoxelGNNGenerator._forward_stacked_nograd issues them (the
    // critic labels), copy k the generator iteration's forward -- the
    // arithmetic of the kWhole branch below, row for row, in the label
    // copies' launches.  Its draws use the counter value the generator
    // iteration will see (*iter + iter_delta) at the indices an n-row launch
    // would use.  The first MLP-encoder and decoder layers of copy k stay
    // their own n-row launches: the label copies form them with
    // vg_gemm_ln_act_ms and a shared addend, another summation order than the
    // concatenate + vg_gemm_ln_act of the generator iteration.
    const vg_gen_stack* sk = io->sk;
    const int k = sk->copies, zd = bt->z_dim, vd = bt->vx_w;
    const int64_t R = (int64_t)(k + 1) * n, Rk = (int64_t)k * n, dl = sk->iter_delta;
    const vg_csr_ref& gs = sk->gs;
    float* z = cx.take(R * zd);
    VG_RUN(vg_rng_fill(z, Rk * zd, 0, bt->seed, bt->iter, bt->z_salt, cx.stream));
    VG_RUN(vg_rng_fill_at(at(z, Rk * zd), (int64_t)n * zd, 0, bt->seed, bt->iter, dl, bt->z_salt, cx.stream));
    const float* zt = at(z, Rk * zd);
    x = bt->mx;
    xw = bt->mx_w;
    for (int i = 0; i < md->n_mfe; ++i) {  // once per step: the same em for every copy
      VG_TRY(ln_fwd(x, xw, md->mfe[i], &mfe_s[i]));
      x = mfe_s[i].y;
      xw = md->mfe[i].out;
    }
    const float* em = x;
    hl = xw;
    float* emvx = cx.take((int64_t)n * (hl + vd));
    VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, vd}}, n, emvx, hl + vd));
    // a first [Linear, LayerNorm, LeakyReLU] layer: the label copies from the
    // sources in place plus the copy-invariant addend, copy k from its own
    // concatenated input (cat_in: [n, L.in], filled by the caller)
    auto first_layer = [&](const vg_gen_ln_layer& L, const vg_asrc* src, int nsrc, int emvx_w0, const float* cat_in,
                           LnS* S, float** y_out) -> int {
      const int m = L.out;
      if (m <= 64 || m > 128) return VG_EINVAL;
      float* add = cx.take((int64_t)n * m);
      VG_TRY(cx.gemm(emvx, hl + vd, at(L.weight, emvx_w0), L.in, 1, add, m, n, m, hl + vd, L.bias));
      float* y = cx.take(R * m);
      VG_RUN(vg_gemm_ln_act_ms(src, nsrc, L.weight, L.in, static_cast<int32_t>(Rk), m, nullptr, add, m, n, L.ln_weight,
                               L.ln_bias, L.ln_eps, L.slope, y, m, cx.stream));
      *S = LnS{&L, cat_in, L.in, cx.take((int64_t)n * m), at(y, Rk * m), cx.take(n), cx.take(n)};
      VG_RUN(vg_gemm_ln_act(cat_in, L.in, L.weight, n, m, L.in, L.bias, L.ln_weight, L.ln_bias, L.ln_eps, L.slope, S->h,
                            S->y, S->mean, S->rstd, cx.stream));
      *y_out = y;
      return 0;
    };
    // a later layer over all R rows, copy k's backward state stored
    auto later_layer = [&](const float* xin, int kin, const vg_gen_ln_layer& L, LnS* S, float** y_out) -> int {
      const int m = L.out;
      if (L.in != kin) return VG_EINVAL;
      float* y = cx.take(R * m);
      *S = LnS{&L, at(xin, Rk * kin), kin, cx.take((int64_t)n * m), at(y, Rk * m), cx.take(n), cx.take(n)};
      VG_RUN(vg_gemm_ln_act_from(xin, kin, L.weight, static_cast<int32_t>(R), m, kin, L.bias, L.ln_weight, L.ln_bias,
                                 L.ln_eps, L.slope, static_cast<int32_t>(Rk), S->h, y, S->mean, S->rstd, cx.stream));
      *y_out = y;
      return 0;
    };
    const int mlp_w = hl + vd + zd;
    if (md->mlp[0].in != mlp_w) return VG_EINVAL;
    float* mlp_in = cx.take((int64_t)n * mlp_w);
    VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, vd}, {zt, zd}}, n, mlp_in, mlp_w));
    float* y = nullptr;
    {
      const vg_asrc src[1] = {{z, zd, zd, hl + vd, 0}};
      VG_TRY(first_layer(md->mlp[0], src, 1, 0, mlp_in, &mlp_s[0], &y));
    }
    xw = md->mlp[0].out;
    for (int i = 1; i < md->n_mlp; ++i) {
      const float* xin = y;
      VG_TRY(later_layer(xin, xw, md->mlp[i], &mlp_s[i], &y));
      xw = md->mlp[i].out;
    }
    const float* xm = y;
    hg = xw;
    // GAT blocks over the stacked graph, one GraphNorm segment per copy
    if (gs.num_nodes != R || gs.num_edges != (int64_t)(k + 1) * E) return VG_EINVAL;
    const float* xb = xm;       // the block's input, all R rows (NULL: the pending GraphNorm's)
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
        VG_RUN(vg_gat_lin_att_gn(pend_O, B.lin_weight, static_cast<int32_t>(R), cin, c, B.att_src, B.att_dst, H, a_s,
                                 a_d, &desc, cx.stream));
      else
        VG_RUN(vg_gat_lin_att(xb, cin, B.lin_weight, static_cast<int32_t>(R), cin, c, B.att_src, B.att_dst, H, a_s, a_d,
                              cx.stream));
      pend = false;
      VG_RUN(vg_gat_aggregate_fwd_gnp(gs.row_ptr, gs.col, gs.ell, gs.ell ? gs.ell_width : 0, static_cast<int32_t>(R), c,
                                      H, a_s, a_d, B.bias, B.slope, O, alpha, n, gnp, cx.stream));
      GatS s{&B, xt, cin, c};
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
      genc[b] = s;
      xt = s.Y;
      xw = c;
    }
    if (pend) return VG_EINVAL;  // (the last block's GraphNorm is always applied: nxt = 0)
    const float* enc = xb;
    ec = xw;
    const int dec_w = ec + hg + hl + vd + zd;  // models.py:145
    if (md->dec[0].in != dec_w) return VG_EINVAL;
    float* dec_in = cx.take((int64_t)n * dec_w);
    VG_TRY(cat_cols(cx, {{at(enc, Rk * ec), ec}, {at(xm, Rk * hg), hg}, {em, hl}, {bt->vx, vd}, {zt, zd}}, n, dec_in,
                    dec_w));
    {
      const vg_asrc src[3] = {{enc, ec, ec, 0, 0}, {xm, hg, hg, ec, 0}, {z, zd, zd, ec + hg + hl + vd, 0}};
      VG_TRY(first_layer(md->dec[0], src, 3, ec + hg, dec_in, &dec_s[0], &y));
    }
    xw = md->dec[0].out;
    for (int i = 1; i < md->n_dec; ++i) {
      const float* xin = y;
      VG_TRY(later_layer(xin, xw, md->dec[i], &dec_s[i], &y));
      xw = md->dec[i].out;
    }
    if (last.in != xw || last.out != K) return VG_EINVAL;
    float* lg = cx.take(R * K);
    VG_TRY(cx.gemm(y, xw, last.weight, xw, 1, lg, K, static_cast<int>(R), K, xw, last.bias));
    float* noise = cx.take(R * K);
    VG_RUN(vg_rng_fill(noise, Rk * K, 2, bt->seed, bt->iter, bt->noise_salt, cx.stream));
    VG_RUN(vg_rng_fill_at(at(noise, Rk * K), (int64_t)n * K, 2, bt->seed, bt->iter, dl, bt->noise_salt, cx.stream));
    VG_RUN(vg_gumbel_fwd(lg, noise, static_cast<int32_t>(R), K, md->tau, io->soft_all, io->hard_all, nullptr,
                         cx.stream));
    if (st) {
      st->magic = kStateMagic;
      st->n = n, st->copies = k, st->arena = cx.base, st->arena_off = cx.off;
      std::copy(mfe_s.begin(), mfe_s.end(), st->mfe);
      std::copy(mlp_s.begin(), mlp_s.end(), st->mlp);
      std::copy(dec_s.begin(), dec_s.end(), st->dec);
      std::copy(genc.begin(), genc.end(), st->genc);
      st->hl = hl, st->hg = hg, st->ec = ec, st->a_last_w = xw;
      st->a_last = at(static_cast<const float*>(y), Rk * xw);
      st->logits = at(lg, Rk * K), st->soft = at(io->soft_all, Rk * K), st->hard = at(io->hard_all, Rk * K);
    }
    return 0;
  } else {
    float* z = cx.take((int64_t)n * bt->z_dim);
    VG_RUN(vg_rng_fill(z, (int64_t)n * bt->z_dim, 0, bt->seed, bt->iter, bt->z_salt, cx.stream));
    x = bt->mx;
    xw = bt->mx_w;
    for (int i = 0; i < md->n_mfe; ++i) {  // models.py:122-131 matched-features encoder
      VG_TRY(ln_fwd(x, xw, md->mfe[i], &mfe_s[i]));
      x = mfe_s[i].y;
      xw = md->mfe[i].out;
    }
    const float* em = x;
    hl = xw;
    const int mlp_w = hl + bt->vx_w + bt->z_dim;
    float* mlp_in = cx.take((int64_t)n * mlp_w);
    VG_TRY(cat_cols(cx, {{em, hl}, {bt->vx, bt->vx_w}, {z, bt->z_dim}}, n, mlp_in, mlp_w));
    x = mlp_in;
    xw = mlp_w;
    for (int i = 0; i < md->n_mlp; ++i) {
      VG_TRY(ln_fwd(x, xw, md->mlp[i], &mlp_s[i]));
      x = mlp_s[i].y;
      xw = md->mlp[i].out;
    }
    const float* xm = x;
    hg = xw;
    for (int b = 0; b < md->n_gblocks; ++b) {
      VG_TRY(gat_fwd(x, xw, md->gblock[b], md->p_drop_g, bt->g_keep_salt[b], &genc[b]));
      x = genc[b].Y;
      xw = genc[b].c;
    }
    const float* enc = x;
    ec = xw;
    const int dec_w = ec + hg + hl + bt->vx_w + bt->z_dim;  // models.py:145
    float* dec_in = cx.take((int64_t)n * dec_w);
    VG_TRY(cat_cols(cx, {{enc, ec}, {xm, hg}, {em, hl}, {bt->vx, bt->vx_w}, {z, bt->z_dim}}, n, dec_in, dec_w));
    x = dec_in;
    xw = dec_w;
    for (int i = 0; i < md->n_dec; ++i) {
      VG_TRY(ln_fwd(x, xw, md->dec[i], &dec_s[i]));
      x = dec_s[i].y;
      xw = md->dec[i].out;
    }
    if (last.in != xw || last.out != K) return VG_EINVAL;
    logits = cx.take((int64_t)n * K);
    VG_TRY(cx.gemm(x, xw, last.weight, xw, 1, logits, K, n, K, xw, last.bias));
    a_last = x;
    a_last_w = xw;
    float* noise = cx.take((int64_t)n * K);
    VG_RUN(vg_rng_fill(noise, (int64_t)n * K, 2, bt->seed, bt->iter, bt->noise_salt, cx.stream));
    soft = cx.take((int64_t)n * K);
    VG_RUN(vg_gumbel_fwd(logits, noise, n, K, md->tau, soft, hard, nullptr, cx.stream));
  }

  // ------------------------------------------------- discriminator forward
  const int F = bt->mvx_w;
  float* X0 = cx.take((int64_t)n * (F + K));
  VG_TRY(cat_cols(cx, {{bt->mvx, F}, {hard, K}}, n, X0, F + K));
  std::vector<float*> d_mlp_out(md->n_dmlp);
  x = X0;
  xw = F + K;
  for (int i = 0; i < md->n_dmlp; ++i) {
    const vg_critic_linear& L = md->dmlp[i];
    if (L.in != xw) return VG_EINVAL;
    float* y = cx.take((int64_t)n * L.out);
    VG_TRY(cx.gemm(x, xw, L.weight, xw, 1, y, L.out, n, L.out, xw, L.bias, kActRelu));
    d_mlp_out[i] = y;
    x = y;
    xw = L.out;
  }
  std::vector<GatS> denc(md->n_dblocks);
  for (int b = 0; b < md->n_dblocks; ++b) {
    VG_TRY(gat_fwd(x, xw, md->dblock[b], md->p_drop_d, bt->d_keep_salt[b], &denc[b]));
    x = denc[b].Y;
    xw = denc[b].c;
  }
  const int nd = md->n_ddec;
  std::vector<float*> dec_out(nd);
  for (int i = 0; i < nd; ++i) dec_out[i] = cx.take((int64_t)n * md->ddec[i].out);
  {
    std::vector<int32_t> w{xw};
    std::vector<vg_chain_layer> layers;
    for (int i = 0; i < nd; ++i) {
      w.push_back(md->ddec[i].out);
      layers.push_back(vg_chain_layer{md->ddec[i].weight, md->ddec[i].bias, nullptr, dec_out[i], 0, md->ddec[i].out, 0,
                                      i == nd - 1 ? kActNone : kActRelu});
    }
    const int rc = cx.chain(x, xw, n, w, layers);
    if (rc < 0) return -rc;
    if (rc == 0)
      for (int i = 0; i < nd; ++i) {
        const vg_critic_linear& L = md->ddec[i];
        VG_TRY(cx.gemm(x, xw, L.weight, xw, 1, dec_out[i], L.out, n, L.out, xw, L.bias,
                       i == nd - 1 ? kActNone : kActRelu));
        x = dec_out[i];
        xw = L.out;
      }
  }
  if (md->ddec[nd - 1].out != 1) return VG_EINVAL;
  const float* d_fake = dec_out[nd - 1];

  // ------------------------------------------------------------- loss head
  const int ng = bt->num_graphs;
  float* far_gen = cx.take(ng);
  float* far_ref = cx.take(ng);
  VG_RUN(vg_far_per_graph(bt->vx, bt->vx_w, hard, K, bt->graph_ptr, ng, bt->site_area, bt->far_col, bt->dy_col,
                          bt->dx_col, md->dim_scale, md->void_class, far_gen, far_ref, cx.stream));
  float* lws = cx.take(vg_gen_loss_ws_floats(n, K));
  VG_RUN(vg_gen_loss_fwd(d_fake, hard, logits, bt->onehot, bt->type, n, K, far_gen, far_ref, ng, md->lambda_adv,
                         md->lambda_label, md->lambda_ratio, md->lambda_void, md->lambda_far, out, lws, cx.stream));
  float* g_d = cx.take(n);
  float* g_hard = cx.take((int64_t)n * K);
  float* g_l = md->lambda_label != 0.f ? cx.take((int64_t)n * K) : nullptr;
  VG_RUN(vg_gen_loss_bwd(bt->one, out, logits, bt->type, n, K, g_d, g_hard, g_l, cx.stream));

  // --------------------------- discriminator input VJP (no parameter grads)
  std::vector<float*> adj(nd);
  for (int i = 0; i < nd - 1; ++i) adj[i] = cx.take((int64_t)n * md->ddec[i].out);
  adj[nd - 1] = g_d;
  {
    std::vector<int32_t> w;
    for (int i = nd - 1; i >= 1; --i) w.push_back(md->ddec[i].out);
    w.push_back(md->ddec[0].out);
    std::vector<vg_chain_layer> layers;
    for (int i = nd - 1; i >= 1; --i) {
      const int in = md->ddec[i].in;
      layers.push_back(vg_chain_layer{md->ddec[i].weight, nullptr, dec_out[i - 1], adj[i - 1], in, in, 1, kActMask});
    }
    const int rc = cx.chain(g_d, 1, n, w, layers);
    if (rc < 0) return -rc;
    if (rc == 0)
      for (int i = nd - 1; i >= 1; --i) {
        const int aw = md->ddec[i].out, m = md->ddec[i].in;
        VG_TRY(cx.gemm(adj[i], aw, md->ddec[i].weight, m, 0, adj[i - 1], m, n, m, aw, nullptr, kActMask, dec_out[i - 1],
                       m));
      }
  }
  const vg_critic_linear& W = md->ddec[0];
  float* dY = cx.take((int64_t)n * W.in);
  float* tp = nullptr;
  VG_TRY(gemm_dy(adj[0], W.out, W.weight, W.in, dY, W.in, W.out, denc[md->n_dblocks - 1], nullptr, &tp));
  std::vector<float*> adj_m(md->n_dmlp);
  for (int i = 0; i < md->n_dmlp; ++i) adj_m[i] = cx.take((int64_t)n * md->dmlp[i].out);
  for (int b = md->n_dblocks - 1; b >= 0; --b) {
    const GatS& S = denc[b];
    const int c = S.c, cin = S.xw;
    float* dH = nullptr;
    const float* Wl = S.B->lin_weight;
    float* dX = b > 0 ? cx.take((int64_t)n * cin) : nullptr;
    float* tpx = b > 0 && cin % 4 == 0 ? cx.take(vg_gemm_gn_tpart_floats(n, cin)) : nullptr;
    bool fused = false;
    if (tpx) {
      const vg_dx_in dx = dx_in(Wl, dX, cin, denc[b - 1], tpx);
      VG_TRY(gat_bwd(S, dY, tp, false, &dH, &dx, &fused));
    } else {
      VG_TRY(gat_bwd(S, dY, tp, false, &dH));
    }
    if (b > 0) {
      if (!fused) VG_TRY(gemm_dy(dH, c, Wl, cin, dX, cin, c, denc[b - 1], tpx, &tp));
      else tp = tpx;
      dY = dX;
    } else {
      VG_TRY(cx.gemm(dH, c, Wl, cin, 0, adj_m[md->n_dmlp - 1], cin, n, cin, c, nullptr, kActMask,
                     d_mlp_out[md->n_dmlp - 1], cin));
    }
  }
  for (int i = md->n_dmlp - 1; i >= 1; --i) {
    const int o = md->dmlp[i].out, m = md->dmlp[i].in;
    VG_TRY(cx.gemm(adj_m[i], o, md->dmlp[i].weight, m, 0, adj_m[i - 1], m, n, m, o, nullptr, kActMask, d_mlp_out[i - 1],
                   m));
  }
  const vg_critic_linear& W0 = md->dmlp[0];
  // label_hard feeds the loss head and D (models.py:229-239): both adjoints summed in the product's epilogue
  float* g_lab = cx.take((int64_t)n * K);
  VG_TRY(cx.gemm(adj_m[0], W0.out, W0.weight + F, W0.in, 0, g_lab, K, n, K, W0.out, nullptr, kActAdd, g_hard, K));

  // ----------------------------------------------------- Gumbel backward
  float* g_logits = cx.take((int64_t)n * K);
  VG_RUN(vg_gumbel_bwd(soft, g_lab, nullptr, n, K, md->tau, g_logits, cx.stream));
  if (g_l && !cx.dry) {
    const long long all = (long long)n * K;
    k_add_to<<<static_cast<int>(std::min<long long>((all + 255) / 256, 4096)), 256, 0,
               static_cast<hipStream_t>(cx.stream)>>>(g_logits, g_l, all);
    VG_CHECK_LAUNCH();
  }

  // -------------------------------------------------- generator backward
  VG_TRY(tn(g_logits, K, a_last, a_last_w, n, K, a_last_w, last.g_weight, a_last_w, last.g_bias));
  float* g = cx.take((int64_t)n * a_last_w);
  VG_TRY(cx.gemm(g_logits, K, last.weight, a_last_w, 0, g, a_last_w, n, a_last_w, K));
  float* g_h = nullptr;
  for (int i = md->n_dec - 1; i > 0; --i) {
    const LnS& S = dec_s[i];
    const int m = S.L->out, k = S.L->in;
    VG_TRY(ln_bwd(S, g, &g_h));
    g = cx.take((int64_t)n * k);
    VG_TRY(cx.gemm(g_h, m, S.L->weight, k, 0, g, k, n, k, m));
  }
  {
    const LnS& S = dec_s[0];
    VG_TRY(ln_bwd(S, g, &g_h));
  }
  const vg_gen_ln_layer& Ld = md->dec[0];
  const int md_ = Ld.out, kd = Ld.in;
  float* g_enc = cx.take((int64_t)n * ec);
  VG_TRY(gemm_dy(g_h, md_, Ld.weight, kd, g_enc, ec, md_, genc[md->n_gblocks - 1], nullptr, &tp));
  float* g_xem = cx.take((int64_t)n * (hg + hl));  // [x | em] columns of the decoder input (enc taken above)
  VG_TRY(cx.gemm(g_h, md_, Ld.weight + ec, kd, 0, g_xem, hg + hl, n, hg + hl, md_));
  const float* g_y = g_enc;
  float* g_x = nullptr;
  for (int b = md->n_gblocks - 1; b >= 0; --b) {
    const GatS& S = genc[b];
    const int c = S.c, cin = S.xw;
    float* dH = nullptr;
    const vg_critic_block& B = *S.B;
    float* gy = b > 0 ? cx.take((int64_t)n * cin) : nullptr;
    float* tpx = b > 0 && cin % 4 == 0 ? cx.take(vg_gemm_gn_tpart_floats(n, cin)) : nullptr;
    bool fused = false;
    if (tpx) {
      const vg_dx_in dx = dx_in(B.lin_weight, gy, cin, genc[b - 1], tpx);
      VG_TRY(gat_bwd(S, g_y, tp, true, &dH, &dx, &fused));
    } else {
      VG_TRY(gat_bwd(S, g_y, tp, true, &dH));
    }
    VG_TRY(tn(dH, c, S.X, cin, n, c, cin, B.g_lin_weight, cin, nullptr));
    if (b > 0) {
      if (!fused) VG_TRY(gemm_dy(dH, c, B.lin_weight, cin, gy, cin, c, genc[b - 1], tpx, &tp));
      else tp = tpx;
      g_y = gy;
    } else {  // x feeds the encoder and the decoder (models.py:132-145)
      g_x = cx.take((int64_t)n * cin);
      VG_TRY(cx.gemm(dH, c, B.lin_weight, cin, 0, g_x, cin, n, cin, c, nullptr, kActAdd, g_xem, hg + hl));
    }
  }
  g = g_x;
  for (int i = md->n_mlp - 1; i >= 0; --i) {
    const LnS& S = mlp_s[i];
    const int m = S.L->out, k = S.L->in;
    VG_TRY(ln_bwd(S, g, &g_h));
    if (i > 0) {
      g = cx.take((int64_t)n * k);
      VG_TRY(cx.gemm(g_h, m, S.L->weight, k, 0, g, k, n, k, m));
    } else {  // the em columns of [em | voxel.x | z]: em feeds the MLP encoder and the decoder
      g = cx.take((int64_t)n * hl);
      VG_TRY(cx.gemm(g_h, m, S.L->weight, k, 0, g, hl, n, hl, m, nullptr, kActAdd, g_xem ? g_xem + hg : nullptr,
                     hg + hl));
    }
  }
  for (int i = md->n_mfe - 1; i >= 0; --i) {
    const LnS& S = mfe_s[i];
    const int m = S.L->out, k = S.L->in;
    VG_TRY(ln_bwd(S, g, &g_h));
    if (i > 0) {
      g = cx.take((int64_t)n * k);
      VG_TRY(cx.gemm(g_h, m, S.L->weight, k, 0, g, k, n, k, m));
    }
  }
  return folds.flush(cx);
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
  if (run(cx, model, batch, nullptr, nullptr)) return -1;
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
  return run(cx, model, batch, out, hard);
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
  GenState st{};
  const StackIO io{stack, nullptr, nullptr};
  if (run(cx, model, batch, nullptr, nullptr, kStackedFwd, &st, &io)) return -1;
  if (run(cx, model, batch, nullptr, nullptr, kFromState, &st)) return -1;  // continues above the state
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
  const StackIO io{stack, hard_all, soft_all};
  return run(cx, model, batch, nullptr, nullptr, kStackedFwd, st, &io);
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
  GenState st = *in;
  Ctx cx{false, 0, stream, arena, arena_floats, st.arena_off};
  Ctx dry{true, 0, nullptr, nullptr, 0, st.arena_off};
  if (run(dry, model, batch, nullptr, nullptr, kFromState, &st) || dry.off > arena_floats) return VG_EINVAL;
  return run(cx, model, batch, out, nullptr, kFromState, &st);
}
