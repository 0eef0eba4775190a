// The 64 x 64 output tile of the f32 products on 16 x 16 x 4 MFMA sub-tiles:
// the device code shared by k_gemm16 / k_gemm8w (gemm.hip, gemm16_body), the
// chain of 2-3 such products in one launch (gemm.hip, k_gemm_chain) and the GAT
// backward source pass that runs its dX product in the same launch
// (gat_fused.hip, k_gat_bwd_src_dx).  One definition of the sub-tile layout,
// the MFMA order over a K-tile, the store, the attention-projection and the
// GraphNorm-backward epilogues, so every kernel built from them gives the
// same bits.
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

// tile_store with the bias and mask operands already in registers (loaded
// before the MFMAs they do not depend on): the same values stored, and kept in
// vals for a consumer in the same workgroup (vg_gemm_chain's next link).
template <int NS>
struct EpiRegs {
  float bv[NS], aux[NS][4];
};

template <int NS>
__device__ __forceinline__ void epi_load(EpiRegs<NS>& e, int act, const int (&mcs)[NS], const float* __restrict__ bias,
                                         const float* __restrict__ aux, int ldaux, int n0, int N, int M, int wr,
                                         int lane) {
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
    e.bv[s_] = (bias && mc < M) ? bias[mc] : 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wr * 16 + 4 * (lane >> 4) + r;
      e.aux[s_][r] = (act >= 3 && n < N && mc < M) ? aux[(size_t)n * ldaux + mc] : 0.f;
    }
  }
}

template <int ACT, int NS>
__device__ __forceinline__ void tile_store_regs(const f32x4 (&accs)[NS], const int (&mcs)[NS], const EpiRegs<NS>& e,
                                                float (&vals)[NS][4], float* __restrict__ C, int ldc, int n0, int N,
                                                int M, int wr, int lane) {
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_) {
    const int mc = mcs[s_];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = n0 + wr * 16 + 4 * (lane >> 4) + r;
      const float v = act_fn<ACT>(accs[s_][r] + e.bv[s_], e.aux[s_][r]);
      vals[s_][r] = mc < M ? v : 0.f;  // columns past M: the next product's zero K padding
      if (n < N && mc < M) C[(size_t)n * ldc + mc] = v;
    }
  }
}

// The attention projections of a 64 x 64 tile (acc + bias, before any
// activation): the tile staged in LDS (Ct: TM x (TN + 1) floats that may alias
// the operand images; the first barrier parks every wave behind the last
// K-tile's reads), then 16 threads per row dot 4 columns each with att_s /
// att_d and combine over the 16 lanes.  NT threads.
template <int NS, int NT>
__device__ __forceinline__ void att_epilogue(const f32x4 (&accs)[NS], const float (&bvs)[NS], float* smem,
                                             const float* __restrict__ att_s, const float* __restrict__ att_d,
                                             float* __restrict__ a_src, float* __restrict__ a_dst, int n0, int N, int M,
                                             int t, int wr, int wc0, int lane) {
  float(*Ct)[TN + 1] = reinterpret_cast<float(*)[TN + 1]>(smem);
  __syncthreads();  // every wave is done with the last K-tile's images
#pragma unroll
  for (int s_ = 0; s_ < NS; ++s_)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      Ct[wr * 16 + 4 * (lane >> 4) + r][(wc0 + s_) * 16 + (lane & 15)] = accs[s_][r] + bvs[s_];
  __syncthreads();
  const int q = t & 15;
#pragma unroll
  for (int row = t >> 4; row < TM; row += NT / 16) {
    float ss = 0.f, sd = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int c = q * 4 + j;
      if (c < M) {
        const float v = Ct[row][c];
        ss = fmaf(v, att_s[c], ss);
        sd = fmaf(v, att_d[c], sd);
      }
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      ss += __shfl_xor(ss, o, 64);
      sd += __shfl_xor(sd, o, 64);
    }
    if (q == 0 && n0 + row < N) {
      a_src[n0 + row] = ss;
      a_dst[n0 + row] = sd;
    }
  }
}

// A whole operand of at most 64 x 64 as float4 quads, NQ per thread of NT
// (NQ NT = 1024 quads): thread quad i covers row i / 16, columns 4 (i % 16)..+3
// of the two K-tile images img[k / TK][row][k % TK].  Rows past `rows` and
// columns past `cols` load as zero (the K padding, the ragged last tile).
// ld % 4 == 0, 16-B aligned p, cols % 4 == 0.
template <int NQ, int NT>
__device__ __forceinline__ void quads_load(float4 (&q)[NQ], const float* __restrict__ p, int ld, int row0, int rows,
                                           int cols, int t) {
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int e = t + NT * i, r = row0 + e / 16, c = 4 * (e % 16);
    q[i] = (r < rows && c < cols) ? *reinterpret_cast<const float4*>(p + (size_t)r * ld + c)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
  }
}

// The same registers filled by scalar loads, for an operand whose stride,
// width or address rules quads out (the `weight + F` column window of an odd
// F): element e = t + NT j is p[e / 64][e % 64], coalesced along the row.
template <int NQ>
__device__ __forceinline__ float& quad_elem(float4 (&q)[NQ], int j) {
  return (j & 3) == 0 ? q[j >> 2].x : (j & 3) == 1 ? q[j >> 2].y : (j & 3) == 2 ? q[j >> 2].z : q[j >> 2].w;
}
template <int NQ, int NT>
__device__ __forceinline__ void scalars_load(float4 (&q)[NQ], const float* __restrict__ p, int ld, int rows, int cols,
                                             int t) {
#pragma unroll
  for (int j = 0; j < 4 * NQ; ++j) {
    const int e = t + NT * j, r = e / 64, c = e % 64;
    quad_elem<NQ>(q, j) = (r < rows && c < cols) ? p[(size_t)r * ld + c] : 0.f;
  }
}
// trans: p's rows are k (img[k / TK][c][k % TK]), else image rows (img[c / TK][r][c % TK])
template <int NQ, int NT>
__device__ __forceinline__ void scalars_store(float4 (&q)[NQ], float (*img)[TN][LDP], bool trans, int t) {
#pragma unroll
  for (int j = 0; j < 4 * NQ; ++j) {
    const int e = t + NT * j, r = e / 64, c = e % 64;
    const float v = quad_elem<NQ>(q, j);
    if (trans) img[r / TK][c][r % TK] = v;
    else img[c / TK][r][c % TK] = v;
  }
}

// rows of p are image rows (A, or B used transposed: p [m][k])
template <int NQ, int NT>
__device__ __forceinline__ void quads_store_rows(const float4 (&q)[NQ], float (*img)[TM][LDP], int t) {
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int e = t + NT * i, r = e / 16, c = 4 * (e % 16);
    float* d = &img[c / TK][r][c % TK];
    d[0] = q[i].x;
    d[1] = q[i].y;
    d[2] = q[i].z;
    d[3] = q[i].w;
  }
}

// rows of p are k (B used as stored: p [k][m]): transposed into img[k / TK][m][k % TK]
template <int NQ, int NT>
__device__ __forceinline__ void quads_store_cols(const float4 (&q)[NQ], float (*img)[TN][LDP], int t) {
#pragma unroll
  for (int i = 0; i < NQ; ++i) {
    const int e = t + NT * i, k = e / 16, m = 4 * (e % 16);
    float(*d)[LDP] = img[k / TK];
    d[m][k % TK] = q[i].x;
    d[m + 1][k % TK] = q[i].y;
    d[m + 2][k % TK] = q[i].z;
    d[m + 3][k % TK] = q[i].w;
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
