// GATv2Conv (heads = 1, share_weights = False) message passing, fused.
//
// Forward, per destination row i (torch_geometric 2.6.1 GATv2Conv semantics;
// x_l = lin_l(x), x_r = lin_r(x) are the two halves of one projection GEMM):
//   u_k     = x_l[col_k] + x_r[i]                              (self loop last)
//   e_k     = sum_c att_c leaky_relu(u_k,c, 0.2)
//   alpha_k = exp(e_k - max_row e) / (sum_row exp(e - max) + 1e-16)
//   out_i   = sum_k alpha_k x_l[col_k] + bias
// The logit is a C-wide reduction per EDGE -- not the sum of two per-node
// scalars GATConv's aggregation reads -- so the kernel is channel-parallel
// throughout: a lane group (rowgroup.h, pick_fused_shape; 8 x 1 for C <= 8)
// owns the row, keeps x_r[i], att and the accumulator in registers, loads
// each neighbour row ONCE and uses it for the logit (add, LeakyReLU, dot with
// att, one group reduction) and, through an online softmax (running maximum,
// rescaled sum and accumulator), for the weighted sum.  Logits wait in
// registers (rows up to 4L edges) or in the row's alpha slots (longer rows)
// until the row's maximum and denominator are final.
//
// Backward (no atomics; deterministic):
//   B1 (destination rows)  ga_k = <g_i, x_l[col_k]>,  t_i = sum alpha ga,
//                          ge_k = alpha_k (ga_k - t_i)            -> workspace
//                          g_xr_i = sum_k ge_k att * lrelu'(u_k)
//                          block partials of sum_k ge_k lrelu(u_k) (att) and
//                          sum_i g_i (bias)
//   B2 (source nodes, CSC) g_xl_j = sum_{k: col_k = j} alpha_k g[dst_k]
//                                   + ge_k att * lrelu'(x_l[j] + x_r[dst_k])
//   B3 (columns)           fold the block partials into g_att, g_bias.
//
// x_l / x_r / g_xl / g_xr carry their own row strides; the vector-load shapes
// are taken only when every base address and stride allows them.
#include "rowgroup.h"

namespace {

using namespace vg;

#ifndef VG_V2_MAX_BLOCKS
#define VG_V2_MAX_BLOCKS 4096
#endif
constexpr int kMaxBlocks = VG_V2_MAX_BLOCKS;  // grid cap of the destination-row backward pass (partials count)
constexpr int kRows = 4;                      // neighbour rows in flight per step

__device__ __forceinline__ float lrelu_grad(float v, float slope) { return v > 0.f ? 1.f : slope; }

// ===================================================================== forward
template <int L, int CPL, bool VEC>
__global__ void __launch_bounds__(kBlock) k_gatv2_fwd(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int N, int C,
    const float* __restrict__ xl, int ld_l, const float* __restrict__ xr, int ld_r,
    const float* __restrict__ att, const float* __restrict__ bias, float slope, float* __restrict__ out,
    float* alpha) {
  constexpr int T = 4;  // logits per lane kept in registers (rows up to 4L edges)
  const GroupIdx g = group_index<L>();
  if (g.row >= N) return;
  const int i = g.row, c0 = g.lane * CPL;
  const int beg = row_ptr[i], end = row_ptr[i + 1];
  const int deg = end - beg;
  Vec<CPL> ri, va, acc;
  load_row<CPL, VEC>(ri, xr + (size_t)i * ld_r, c0, C);
  load_row<CPL, false>(va, att, c0, C);  // parameters live at arbitrary offsets of the flat buffer
#pragma unroll
  for (int q = 0; q < CPL; ++q) acc.v[q] = 0.f;
  const int s_own = g.lane < deg ? col[beg + g.lane] : 0;
  float e_t[T] = {0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, ssum = 0.f;
  for (int j0 = 0; j0 < deg; j0 += kRows) {
    const int nj = deg - j0 < kRows ? deg - j0 : kRows;
    Vec<CPL> hv[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u)
      if (u < nj) {
        const int j = j0 + u;
        const int s = (deg <= L) ? __shfl(s_own, g.base + j, 64) : col[beg + j];
        load_row<CPL, VEC>(hv[u], xl + (size_t)s * ld_l, c0, C);
      }
#pragma unroll
    for (int u = 0; u < kRows; ++u)
      if (u < nj) {
        const int j = j0 + u;
        float p = 0.f;
#pragma unroll
        for (int q = 0; q < CPL; ++q) p = fmaf(va.v[q], lrelu(hv[u].v[q] + ri.v[q], slope), p);
        const float e = group_sum<L>(p);
        if (g.lane == (j & (L - 1))) {  // edge j waits in lane j % L, slot j / L
          const int slot = j / L;
          if (slot == 0) e_t[0] = e;
          else if (slot == 1) e_t[1] = e;
          else if (slot == 2) e_t[2] = e;
          else if (slot == 3) e_t[3] = e;
          else alpha[beg + j] = e;  // very long rows: the logit waits in its alpha slot
        }
        // online softmax: the first edge rescales the empty sums by exp(-inf) = 0
        const float mn = fmaxf(m, e);
        const float sc = expf(m - mn), pe = expf(e - mn);
        ssum = fmaf(ssum, sc, pe);
#pragma unroll
        for (int q = 0; q < CPL; ++q) acc.v[q] = fmaf(acc.v[q], sc, pe * hv[u].v[q]);
        m = mn;
      }
  }
  const float denom = ssum + kSoftmaxEps;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int j = g.lane + t * L;
    if (j < deg) alpha[beg + j] = expf(e_t[t] - m) / denom;
  }
  for (int k = beg + T * L + g.lane; k < end; k += L) alpha[k] = expf(alpha[k] - m) / denom;  // this lane wrote it
  Vec<CPL> b;
  load_row<CPL, false>(b, bias, c0, C);
#pragma unroll
  for (int q = 0; q < CPL; ++q) acc.v[q] = acc.v[q] / denom + b.v[q];
  store_row<CPL, VEC>(acc, out + (size_t)i * C, c0, C);
}

// ================================================== backward B1 (destination)
template <int L, int CPL, bool VEC>
__global__ void __launch_bounds__(kBlock) k_gatv2_bwd_rows(
    const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int N, int C,
    const float* __restrict__ xl, int ld_l, const float* __restrict__ xr, int ld_r,
    const float* __restrict__ att, const float* __restrict__ alpha, const float* __restrict__ g_out, float slope,
    float* __restrict__ ge_out, float* __restrict__ g_xr, int ld_gr, float* __restrict__ part) {
  constexpr int G = kBlock / L;
  const int grp = threadIdx.x / L, lane = threadIdx.x & (L - 1);
  const int base = (threadIdx.x & 63) & ~(L - 1);
  const int c0 = lane * CPL;
  Vec<CPL> va, pa, pb;  // att; sum ge lrelu(u); sum g_out
  load_row<CPL, false>(va, att, c0, C);
#pragma unroll
  for (int q = 0; q < CPL; ++q) pa.v[q] = pb.v[q] = 0.f;
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  for (int i = lb * G + grp; i < N; i += gridDim.x * G) {
    const int beg = row_ptr[i], end = row_ptr[i + 1];
    const int deg = end - beg;
    Vec<CPL> go, ri, gr;
    load_row<CPL, VEC>(go, g_out + (size_t)i * C, c0, C);
    load_row<CPL, VEC>(ri, xr + (size_t)i * ld_r, c0, C);
    const int s_own = lane < deg ? col[beg + lane] : 0;
    const float al_own = lane < deg ? alpha[beg + lane] : 0.f;
    // pass 1: t_i = sum_k alpha_k ga_k
    float t = 0.f;
    for (int j0 = 0; j0 < deg; j0 += kRows) {
      const int nj = deg - j0 < kRows ? deg - j0 : kRows;
      Vec<CPL> hv[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (u < nj) {
          const int j = j0 + u;
          const int s = (deg <= L) ? __shfl(s_own, base + j, 64) : col[beg + j];
          load_row<CPL, VEC>(hv[u], xl + (size_t)s * ld_l, c0, C);
        }
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (u < nj) {
          const int j = j0 + u;
          const float ga = group_sum<L>(dot_row<CPL, VEC>(go, hv[u]));
          const float al = (deg <= L) ? __shfl(al_own, base + j, 64) : alpha[beg + j];
          t = fmaf(al, ga, t);
        }
    }
    // pass 2: the neighbour rows again (cache hits), ga recomputed bit for bit
#pragma unroll
    for (int q = 0; q < CPL; ++q) gr.v[q] = 0.f;
    for (int j0 = 0; j0 < deg; j0 += kRows) {
      const int nj = deg - j0 < kRows ? deg - j0 : kRows;
      Vec<CPL> hv[kRows];
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (u < nj) {
          const int j = j0 + u;
          const int s = (deg <= L) ? __shfl(s_own, base + j, 64) : col[beg + j];
          load_row<CPL, VEC>(hv[u], xl + (size_t)s * ld_l, c0, C);
        }
#pragma unroll
      for (int u = 0; u < kRows; ++u)
        if (u < nj) {
          const int j = j0 + u;
          const float ga = group_sum<L>(dot_row<CPL, VEC>(go, hv[u]));
          const float al = (deg <= L) ? __shfl(al_own, base + j, 64) : alpha[beg + j];
          const float ge = al * (ga - t);
          if (lane == 0) ge_out[beg + j] = ge;
#pragma unroll
          for (int q = 0; q < CPL; ++q) {
            const float uq = hv[u].v[q] + ri.v[q];
            gr.v[q] = fmaf(ge * lrelu_grad(uq, slope), va.v[q], gr.v[q]);
            pa.v[q] = fmaf(ge, lrelu(uq, slope), pa.v[q]);
          }
        }
    }
    store_row<CPL, VEC>(gr, g_xr + (size_t)i * ld_gr, c0, C);
#pragma unroll
    for (int q = 0; q < CPL; ++q) pb.v[q] += go.v[q];
  }
  Vec<CPL> vals[2] = {pa, pb};
  block_partials<L, CPL>(vals, 2, C, part);
}

// ===================================================== backward B2 (sources)
template <int L, int CPL, bool VEC>
__global__ void __launch_bounds__(kBlock) k_gatv2_bwd_src(
    const int32_t* __restrict__ csc_ptr, const int32_t* __restrict__ csc_slot,
    const int32_t* __restrict__ csc_dst, int N, int C, const float* __restrict__ xl, int ld_l,
    const float* __restrict__ xr, int ld_r, const float* __restrict__ att, const float* __restrict__ alpha,
    const float* __restrict__ ge, const float* __restrict__ g_out, float slope, float* __restrict__ g_xl,
    int ld_gl) {
  const GroupIdx g = group_index<L>();
  if (g.row >= N) return;
  const int j = g.row, c0 = g.lane * CPL;
  const int beg = csc_ptr[j], end = csc_ptr[j + 1];
  const int deg = end - beg;
  Vec<CPL> va, lj, acc;
  load_row<CPL, false>(va, att, c0, C);
  load_row<CPL, VEC>(lj, xl + (size_t)j * ld_l, c0, C);
#pragma unroll
  for (int q = 0; q < CPL; ++q) acc.v[q] = 0.f;
  int d_own = 0;
  float a_own = 0.f, e_own = 0.f;
  if (g.lane < deg) {
    const int k = csc_slot[beg + g.lane];
    d_own = csc_dst[beg + g.lane];
    a_own = alpha[k];
    e_own = ge[k];
  }
  for (int e0 = 0; e0 < deg; e0 += kRows) {
    const int ne = deg - e0 < kRows ? deg - e0 : kRows;
    Vec<CPL> gv[kRows], rv[kRows];
    float a[kRows], w[kRows];
#pragma unroll
    for (int u = 0; u < kRows; ++u)
      if (u < ne) {
        const int e = e0 + u;
        int d;
        if (deg <= L) {
          d = __shfl(d_own, g.base + e, 64);
          a[u] = __shfl(a_own, g.base + e, 64);
          w[u] = __shfl(e_own, g.base + e, 64);
        } else {
          const int k = csc_slot[beg + e];
          d = csc_dst[beg + e];
          a[u] = alpha[k];
          w[u] = ge[k];
        }
        load_row<CPL, VEC>(gv[u], g_out + (size_t)d * C, c0, C);
        load_row<CPL, VEC>(rv[u], xr + (size_t)d * ld_r, c0, C);
      }
#pragma unroll
    for (int u = 0; u < kRows; ++u)
      if (u < ne)
#pragma unroll
        for (int q = 0; q < CPL; ++q) {
          acc.v[q] = fmaf(a[u], gv[u].v[q], acc.v[q]);
          acc.v[q] = fmaf(w[u] * lrelu_grad(lj.v[q] + rv[u].v[q], slope), va.v[q], acc.v[q]);
        }
  }
  store_row<CPL, VEC>(acc, g_xl + (size_t)j * ld_gl, c0, C);
}

// ===================================================== B3: fold the partials
// part [rows][2C] -> g_att (columns < C), g_bias (the rest); one 1024-thread
// block per 64 columns, 16 waves stride over the partial rows, LDS fold in a
// fixed order (deterministic).
__global__ void __launch_bounds__(1024) k_gatv2_fold(const float* __restrict__ part, int rows, int C, int acc,
                                                     float* __restrict__ g_att, float* __restrict__ g_bias) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int W = 2 * C;
  const int w = blockIdx.x * 64 + lane;
  float s = 0.f;
  if (w < W) {
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;  // loads in flight, fixed combine order
    int r = wave;
    for (; r + 48 < rows; r += 64) {
      a0 += part[(size_t)r * W + w];
      a1 += part[(size_t)(r + 16) * W + w];
      a2 += part[(size_t)(r + 32) * W + w];
      a3 += part[(size_t)(r + 48) * W + w];
    }
    for (; r < rows; r += 16) a0 += part[(size_t)r * W + w];
    s = (a0 + a1) + (a2 + a3);
  }
  __shared__ float red[16][64];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && w < W) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) v += red[k][lane];
    float* o = w < C ? g_att + w : g_bias + (w - C);
    *o = acc ? *o + v : v;
  }
}

// the vector shapes move CPL floats with float2 / float4 accesses: every row
// start must sit on that boundary
inline bool vec_ok(const void* p, int ld, int cpl) {
  const int a = cpl >= 4 ? 4 : cpl;  // floats per access
  return (reinterpret_cast<uintptr_t>(p) % (sizeof(float) * a)) == 0 && ld % a == 0;
}

inline bool pick_v2_shape(int C, Shape& sh) {
  if (C <= 0 || C > 256) return false;
  if (C <= 8) {
    sh = {8, 1, false};
    return true;
  }
  return pick_fused_shape(C, sh);
}

}  // namespace

// C <= 8 runs the scalar 8 x 1 shape; wider rows the fused shapes, vectorised
// when `vec` (shape divisibility, base addresses and strides) holds
#define VG_V2_DISPATCH(C, vec, KERNEL, GRID, ...)                                                  \
  do {                                                                                             \
    if ((C) <= 8) {                                                                                \
      KERNEL<8, 1, false><<<GRID(8), kBlock, 0, s>>>(__VA_ARGS__);                                 \
    } else {                                                                                       \
      VG_DISPATCH_FUSED(C, ((V_ && (vec)) ? KERNEL<L_, CPL_, V_><<<GRID(L_), kBlock, 0, s>>>(__VA_ARGS__)    \
                                          : KERNEL<L_, CPL_, false><<<GRID(L_), kBlock, 0, s>>>(__VA_ARGS__))); \
    }                                                                                              \
  } while (0)

extern "C" int vg_gatv2_fwd(const int32_t* row_ptr, const int32_t* col, int32_t N, int32_t C, const float* xl,
                            int32_t ld_l, const float* xr, int32_t ld_r, const float* att, const float* bias,
                            float slope, float* out, float* alpha, void* stream) {
  Shape sh;
  if (N <= 0 || !pick_v2_shape(C, sh) || !row_ptr || !col || !xl || !xr || !att || !bias || !out || !alpha ||
      ld_l < C || ld_r < C)
    return VG_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = sh.vec && vec_ok(xl, ld_l, sh.CPL) && vec_ok(xr, ld_r, sh.CPL) && vec_ok(out, C, sh.CPL);
#define VG_V2_GRID(L) grid_for(N, L)
  VG_V2_DISPATCH(C, vec, k_gatv2_fwd, VG_V2_GRID, row_ptr, col, N, C, xl, ld_l, xr, ld_r, att, bias, slope, out,
                 alpha);
#undef VG_V2_GRID
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t vg_gatv2_bwd_ws_floats(int32_t num_nodes, int32_t num_edges, int32_t channels) {
  (void)num_nodes;
  // ge [E'] + the destination pass's partials (2C per block)
  return (int64_t)num_edges + (int64_t)kMaxBlocks * 2 * channels;
}

extern "C" int vg_gatv2_bwd(const int32_t* row_ptr, const int32_t* col, const int32_t* csc_ptr,
                            const int32_t* csc_slot, const int32_t* csc_dst, int32_t N, int32_t E, int32_t C,
                            const float* xl, int32_t ld_l, const float* xr, int32_t ld_r, const float* att,
                            const float* alpha, const float* g_out, float slope, float* g_xl, int32_t ld_gl,
                            float* g_xr, int32_t ld_gr, float* g_att, float* g_bias, int32_t accumulate,
                            float* workspace, void* stream) {
  Shape sh;
  if (N <= 0 || E <= 0 || !pick_v2_shape(C, sh) || !row_ptr || !col || !csc_ptr || !csc_slot || !csc_dst ||
      !xl || !xr || !att || !alpha || !g_out || !g_xl || !g_xr || !workspace || ld_l < C || ld_r < C ||
      ld_gl < C || ld_gr < C || (g_att != nullptr) != (g_bias != nullptr))
    return VG_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* ge = workspace;
  float* part = workspace + E;  // [grid1][2C]
  const bool vec = sh.vec && vec_ok(xl, ld_l, sh.CPL) && vec_ok(xr, ld_r, sh.CPL) && vec_ok(g_out, C, sh.CPL) &&
                   vec_ok(g_xl, ld_gl, sh.CPL) && vec_ok(g_xr, ld_gr, sh.CPL);
  const int g1 = grid_for(N, sh.L);
  const int grid1 = g1 < kMaxBlocks ? g1 : kMaxBlocks;
#define VG_V2_GRID1(L) grid1
#define VG_V2_GRID2(L) grid_for(N, L)
  VG_V2_DISPATCH(C, vec, k_gatv2_bwd_rows, VG_V2_GRID1, row_ptr, col, N, C, xl, ld_l, xr, ld_r, att, alpha,
                 g_out, slope, ge, g_xr, ld_gr, part);
  VG_V2_DISPATCH(C, vec, k_gatv2_bwd_src, VG_V2_GRID2, csc_ptr, csc_slot, csc_dst, N, C, xl, ld_l, xr, ld_r, att,
                 alpha, ge, g_out, slope, g_xl, ld_gl);
#undef VG_V2_GRID1
#undef VG_V2_GRID2
  if (g_att)
    k_gatv2_fold<<<vg_blocks(2 * C, 64), 1024, 0, s>>>(part, grid1, C, accumulate, g_att, g_bias);
  VG_CHECK_LAUNCH();
  return 0;
}
