// What the two f16 engines (hgen_engine.hip: the generator sweep;
// hcritic_engine.hip: the critic scorer) share: the arena their temporaries
// are carved from (dry: sizes only), the launch guard, the kernel that
// stacks a batch's CSR block-diagonally and the GAT encoder's schedule.
// Internal linkage: one copy per translation unit.
#pragma once
#include <stdint.h>

#include <algorithm>

#include "common.h"

namespace {

inline int r8(int c) { return (c + 7) / 8 * 8; }

// block-diagonal stack of `copies` copies of a destination CSR (vgan.ops
// CSR.stacked: node ids offset by c * n, edge slots by c * e)
__global__ void k_hg_stack_csr(const int32_t* __restrict__ row_ptr, const int32_t* __restrict__ col, int n, int e,
                               int copies, int32_t* __restrict__ rp_out, int32_t* __restrict__ col_out) {
  const long long nr = (long long)copies * n + 1, ne = (long long)copies * e;
  for (long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x; t < nr + ne;
       t += (long long)gridDim.x * blockDim.x) {
    if (t < nr) {
      const int c = static_cast<int>(t / n), i = static_cast<int>(t - (long long)c * n);
      rp_out[t] = t == nr - 1 ? static_cast<int32_t>(ne) : row_ptr[i] + c * e;
    } else {
      const long long k = t - nr;
      const int c = static_cast<int>(k / e), j = static_cast<int>(k - (long long)c * e);
      col_out[k] = col[j] + c * n;
    }
  }
}

// temporaries of one call: 256-byte-aligned pieces of a caller-owned buffer;
// dry: nothing is handed out, off ends as the size the schedule needs
struct Arena {
  bool dry;
  char* base;
  int64_t off = 0;
  template <class T>
  T* take(int64_t count) {
    const int64_t at = off;
    off += (std::max<int64_t>(count * (int64_t)sizeof(T), 1) + 255) / 256 * 256;
    return dry ? nullptr : reinterpret_cast<T*>(base + at);
  }
};

// a launch of the schedule: skipped in a dry run, its error returned
#define VG_RUN(expr)                  \
  do {                                \
    if (!ar.dry) {                    \
      const int _rc = (expr);         \
      if (_rc) return _rc;            \
    }                                 \
  } while (0)

int launched() { return static_cast<int>(hipGetLastError()); }

int blocks_for(long long work) {
  const long long b = (work + 255) / 256;
  return static_cast<int>(std::min<long long>(std::max<long long>(b, 1), 4096));
}

// The GAT encoder (models.py:68-90 of the reference, eval) over rows = copies
// * n stacked f16 rows of x: per block vg_hgat_lin_att, the aggregation and
// the GraphNorm + ReLU.  The GraphNorm's column partials come from the
// aggregation's epilogue (vg_hgat_fwd_gnp) when one copy spans a partial
// block; its statistics then take one small launch and the next block's
// projection applies it as it loads its operand (vg_hgat_lin_att_gn) when
// copies <= vg_hgat_gna_max_segments().  The last block's GraphNorm is stored:
// into last_out (stride last_ld > 0; NULL in a dry run) when given, else
// into the arena.  These are
// vgan/half.py _gat_encoder's choices, launch for launch.  The workspace of a
// GraphNorm that takes its own statistics pass is reserved once, the widest
// block's, whatever the sizes: the arena only grows with n and copies.
int run_gat_blocks(Arena& ar, hipStream_t s, const vg_hgen_block* blocks, int nb, const uint16_t* x, int ldx, int n,
                   int copies, const int32_t* rp, const int32_t* cl, uint16_t* last_out, int last_ld,
                   const uint16_t** out, int* out_ld) {
  const int kk = copies, rows = kk * n;
  struct Pend {
    const uint16_t* agg;
    int ld;
    const vg_hgen_block* blk;
    const float* stats;
  } pend{nullptr, 0, nullptr, nullptr};
  int64_t ws_floats = 0;
  for (int b = 0; b < nb; ++b)
    ws_floats = std::max<int64_t>(ws_floats, vg_graphnorm_seg_ws_floats(kk, n, blocks[b].out));
  float* ws = ar.take<float>(ws_floats);
  for (int b = 0; b < nb; ++b) {
    const vg_hgen_block& B = blocks[b];
    const int cout = B.out, ldh = r8(cout);
    uint16_t* h = ar.take<uint16_t>((int64_t)rows * ldh);
    float* a_s = ar.take<float>(rows);
    float* a_d = ar.take<float>(rows);
    if (pend.agg) {
      const vg_hgen_block& P = *pend.blk;
      VG_RUN(vg_hgat_lin_att_gn(pend.agg, pend.ld, B.lin_weight, B.ldw, rows, r8(B.in), cout, B.att_src, B.att_dst, h,
                                ldh, a_s, a_d, P.gn_weight, P.gn_bias, P.gn_mean_scale, pend.stats, kk, n, P.out, s));
      pend = Pend{nullptr, 0, nullptr, nullptr};
    } else {
      VG_RUN(vg_hgat_lin_att(x, ldx, B.lin_weight, B.ldw, rows, r8(B.in), cout, B.att_src, B.att_dst, h, ldh, a_s,
                             a_d, s));
    }
    uint16_t* agg = ar.take<uint16_t>((int64_t)rows * ldh);
    const int g = vg_hgat_gnp_rows(rows, ldh);
    const bool use_gnp = g > 0 && g <= n;
    float* gnp = use_gnp ? ar.take<float>(vg_hgat_gnp_floats(rows, ldh)) : nullptr;
    if (use_gnp)
      VG_RUN(vg_hgat_fwd_gnp(rp, cl, rows, cout, ldh, h, a_s, a_d, B.bias, B.slope, agg, ldh, n, gnp, s));
    else
      VG_RUN(vg_hgat_fwd(rp, cl, rows, cout, ldh, h, a_s, a_d, B.bias, B.slope, agg, ldh, s));
    float* stats = ar.take<float>((int64_t)kk * 2 * cout);
    if (use_gnp && b < nb - 1 && kk <= vg_hgat_gna_max_segments()) {
      VG_RUN(vg_graphnorm_stats_gnp(kk, n, cout, gnp, g, B.gn_mean_scale, B.gn_eps, stats, s));
      pend = Pend{agg, ldh, &B, stats};
      continue;
    }
    uint16_t* y;
    int ldy;
    if (b == nb - 1 && last_ld > 0) {
      y = last_out;
      ldy = last_ld;
    } else {
      y = ar.take<uint16_t>((int64_t)rows * ldh);
      ldy = ldh;
    }
    if (use_gnp) {
      VG_RUN(vg_graphnorm_fwd_h_gnp(agg, ldh, kk, n, cout, B.gn_weight, B.gn_bias, B.gn_mean_scale, B.gn_eps, y, ldy,
                                    stats, gnp, g, s));
    } else {
      VG_RUN(vg_graphnorm_fwd_h(agg, ldh, kk, n, cout, B.gn_weight, B.gn_bias, B.gn_mean_scale, B.gn_eps, y, ldy, stats,
                                ws, s));
    }
    x = y;
    ldx = ldy;
  }
  *out = x;
  *out_ld = ldx;
  return 0;
}

}  // namespace
