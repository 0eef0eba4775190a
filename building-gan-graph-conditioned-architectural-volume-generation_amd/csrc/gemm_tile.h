// The 64 x 64 output tile of the f32 products on 16 x 16 x 4 MFMA sub-tiles:
// the device code shared by k_gemm16 / k_gemm8w (gemm.hip, gemm16_body) and
// the GAT backward source pass that runs its dX product in the same launch
// (gat_fused.hip, k_gat_bwd_src_dx).  One definition of the sub-tile layout,
// the MFMA order over a K-tile, the store and the GraphNorm-backward
// epilogue, so every kernel built from them gives the same bits.
//
// Layout: NW = 16 waves as 4 x 4, one 16 x 16 sub-tile each, or NW = 8 waves
// as 4 x 2 with NS = 2 side-by-side sub-tiles; wave row wr, first sub-tile
// column wc0.  Lane l of a sub-tile holds column l % 16, rows 4 (l / 16) + r.
#pragma once
#include "common.h"

namespace vg {
namespace tile {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int TM = 64, TN = 64, TK = 32, LDP = TK + 1;

template <int ACT>
__device__ __forceinline__ float act_fn(float v, float aux) {
  if constexpr (ACT == 1) return v > 0.f ? v : 0.f;
  else if constexpr (ACT == 2) return v > 0.f ? v : 0.2f * v;
  else if constexpr (ACT == 3) return aux > 0.f ? v : 0.f;
  else if constexpr (ACT == 4) return v + aux;  // a second adjoint summed in (torch's add_ after the GEMM)
  else return v;
}

// GraphNorm-backward partials in the epilogue of the GEMM that produces the
// layer's output gradient g_y (vg_gemm_gn_bwd): x, keep [rows, M] (the
// GraphNorm input and dropout multiplier), stats [S][2M] of segments of
// seg_rows rows, tpart [row tile][2 slots][M][2] (sum gz, sum gz * xhat).
struct GnpDesc {
  const float* x;
  const float* keep;
  const float* stats;
  const float* w;
  const float* b;
  const float* ms;
  float eps;
  int seg_rows;
  float* tpart;
};

// The epilogue's GraphNorm operands of one lane: its 4 rows of x / keep per
// sub-tile, the two segments' statistics, the column's parameters.
template <int NS>
struct GnpRegs {
  float x[NS][4], k[NS][4];
  float mu[NS][2], sd[NS][2], w[NS], b[NS], ms[NS];
  int bound;  // first row of the tile's second segment slot
};

// Loads them (issued before the K loop: nothing here depends on the product),
// in two parts: the column operands (parameters and statistics, L2 hits) and
// the lane's rows of x / keep (first reads of rows an earlier kernel wrote).
template <int NS>
__device__ __forceinline__ void gnp_load_cols(GnpRegs<NS>& g, const GnpDesc& gn, int n0, int N, int M,
                                              const int (&mcs)[NS]) {
  const int seg0 = n0 / gn.seg_rows;
  g.bound = (seg0 + 1) * gn.seg_rows;
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
    g.mu[s_][0] = g.mu[s_][1] = 0.f;
    g.sd[s_][0] = g.sd[s_][1] = 1.f;
    g.w[s_] = g.b[s_] = g.ms[s_] = 0.f;
    if (mc < M) {
      g.w[s_] = gn.w[mc];
      g.b[s_] = gn.b[mc];
      g.ms[s_] = gn.ms[mc];
#pragma unroll
      for (int q = 0; q < 2; ++q)
        if (q == 0 || g.bound < N) {
          const float* st = gn.stats + (size_t)(seg0 + q) * 2 * M;
          g.mu[s_][q] = st[mc];
          g.sd[s_][q] = st[M + mc];
        }
    }
  }
}

template <int NS>
__device__ __forceinline__ void gnp_load_rows(GnpRegs<NS>& g, const GnpDesc& gn, int n0, int N, int M,
                                              const int (&mcs)[NS], int wr, int lane) {
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wr * 16 + 4 * (lane >> 4) + r;
      const bool ok = n < N && mc < M;
      g.x[s_][r] = ok ? gn.x[(size_t)n * M + mc] : 0.f;
      g.k[s_][r] = ok && gn.keep ? gn.keep[(size_t)n * M + mc] : 1.f;
    }
  }
}

// One K-tile of TK: 8 MFMAs per sub-tile over As [TM][LD] (rows x k) and
// Bs [TN][LD] (Bs[j][k] = op(B)[k][j]), k ascending.
template <int NS, int LD>
__device__ __forceinline__ void mfma_ktile(f32x4 (&accs)[NS], const float (*As)[LD], const float (*Bs)[LD], int wr,
                                           int wc0, int lane) {
  const float* ar = &As[wr * 16 + (lane & 15)][lane >> 4];
#pragma unroll
  for (int kk = 0; kk < TK; kk += 4) {
    const float av = ar[kk];
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_)
      accs[s_] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, Bs[(wc0 + s_) * 16 + (lane & 15)][(lane >> 4) + kk],
                                                      accs[s_], 0, 0, 0);
  }
}

// C = act(acc + bias); returns each sub-tile's bias value in bvs.
template <int ACT, int NS>
__device__ __forceinline__ void tile_store(const f32x4 (&accs)[NS], const int (&mcs)[NS], float (&bvs)[NS],
                                           const float* __restrict__ bias, const float* __restrict__ aux, int ldaux,
                                           float* __restrict__ C, int ldc, int n0, int N, int M, int wr, int lane) {
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
    const f32x4 acc = accs[s_];
    const float bv = (bias && mc < M) ? bias[mc] : 0.f;
    bvs[s_] = bv;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wr * 16 + 4 * (lane >> 4) + r;
      if (n < N && mc < M) {
        const float av = ACT >= 3 ? aux[(size_t)n * ldaux + mc] : 0.f;
        C[(size_t)n * ldc + mc] = act_fn<ACT>(acc[r] + bv, av);
      }
    }
  }
}

// Column partials of gz = g_y [z > 0] keep and gz * xhat per segment slot:
// the lane's 4 rows in order, the 4 lanes of the column (xor 16, 32), then
// the 4 row waves of the column through LDS in order: deterministic.
// red: 4 x 64 x 4 floats of LDS that may alias the operand images (the first
// barrier here parks every wave behind the last K-tile's reads); `staged`
// runs between the two barriers (a caller's own LDS traffic on the same terms).
template <int NS, class F>
__device__ __forceinline__ void gnp_epilogue(const GnpDesc& gn, const GnpRegs<NS>& g, const f32x4 (&accs)[NS],
                                             const int (&mcs)[NS], int n0, int N, int M, int tx, int wr, int wc0,
                                             int lane, float* red, F&& staged) {
  float pa[NS][2], pb[NS][2];
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
    const f32x4 acc = accs[s_];
    pa[s_][0] = pa[s_][1] = pb[s_][0] = pb[s_][1] = 0.f;
    if (mc < M) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int n = n0 + wr * 16 + 4 * (lane >> 4) + r;
        if (n < N) {
          const int sl = n >= g.bound;
          const float xh = (g.x[s_][r] - (sl ? g.mu[s_][1] : g.mu[s_][0]) * g.ms[s_]) / (sl ? g.sd[s_][1] : g.sd[s_][0]);
          const float gz = xh * g.w[s_] + g.b[s_] > 0.f ? acc[r] * g.k[s_][r] : 0.f;
          if (sl) {
            pa[s_][1] += gz;
            pb[s_][1] = fmaf(gz, xh, pb[s_][1]);
          } else {
            pa[s_][0] += gz;
            pb[s_][0] = fmaf(gz, xh, pb[s_][0]);
          }
        }
      }
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      pa[s_][q] += __shfl_xor(pa[s_][q], 16, 64);
      pb[s_][q] += __shfl_xor(pb[s_][q], 16, 64);
      pa[s_][q] += __shfl_xor(pa[s_][q], 32, 64);
      pb[s_][q] += __shfl_xor(pb[s_][q], 32, 64);
    }
  }
  __syncthreads();  // every wave is done with the last K-tile's LDS images
  if (lane < 16)
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
      float* rp = red + ((wr * 64) + (wc0 + s_) * 16 + lane) * 4;
      rp[0] = pa[s_][0];
      rp[1] = pb[s_][0];
      rp[2] = pa[s_][1];
      rp[3] = pb[s_][1];
    }
  staged();
  __syncthreads();
  if (wr == 0 && lane < 16)
#pragma unroll
    for (int s_ = 0; s_ < NS; ++s_) {
      const int mc = mcs[s_];
      if (mc >= M) continue;
      float sm[4] = {0.f, 0.f, 0.f, 0.f};
      for (int w = 0; w < 4; ++w) {
        const float* rp = red + ((w * 64) + (wc0 + s_) * 16 + lane) * 4;
#pragma unroll
        for (int q = 0; q < 4; ++q) sm[q] += rp[q];
      }
      float* tp = gn.tpart + (size_t)tx * 2 * M * 2;
      tp[(size_t)mc * 2] = sm[0];
      tp[(size_t)mc * 2 + 1] = sm[1];
      tp[(size_t)(M + mc) * 2] = sm[2];
      tp[(size_t)(M + mc) * 2 + 1] = sm[3];
    }
}

}  // namespace tile
}  // namespace vg
