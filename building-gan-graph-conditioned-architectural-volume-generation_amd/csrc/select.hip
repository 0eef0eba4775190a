// Best-of-k selection for the inference sweep (vg_sweep_select):
// one launch scores the k candidate labellings of every building (macro-F1
// against the true types, FAR against the target), picks one candidate per
// building and gathers its labels.  The reference does this on the host,
// trainer.py:65-84 (_visualize_one: sklearn f1_score per sample, strict
// best_f1 < f1) and trainer.py:357-378 (the FAR of a labelling).
#include "common.h"

namespace {

constexpr int kMaxClasses = 32;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / VG_WAVE;
constexpr int kQuad = 4;  // consecutive voxels per thread: 4 bytes of pred per candidate
constexpr int kGroup = 8;  // candidates whose reads are in flight together
constexpr size_t kLdsBytes = 64 * 1024;

// The 4 predictions row[v0 .. v0+3] of one candidate row in two steps, so that
// the reads of several candidates are in flight together: quad_issue only
// loads (raw registers, nothing computed from them -- no wait), quad_decode
// turns them into one word, a prediction per byte, 0xff (-1: counted nowhere)
// for a voxel outside the building's rows [lo, hi).
// Where every byte read lies in the candidate row's [rlo, rhi) = [ptr[0],
// ptr[G]) -- bytes of a neighbouring building are read and masked, nothing
// outside the row is touched: one aligned 32-bit read, or the two aligned
// words the quad straddles when row + v0 is not 4-byte aligned (a candidate
// row of a [k, N] tensor starts at any byte).  At the two ends of the row:
// the building's own bytes, one by one.
struct Span {
  int64_t lo, hi, rlo, rhi;
};

__device__ __forceinline__ bool quad_wide(const int8_t* row, int64_t v0, const Span& sp,
                                          unsigned& sh) {
  sh = reinterpret_cast<uintptr_t>(row + v0) & 3;
  const int64_t a = v0 - sh;  // voxel of the first byte read
  return a >= sp.rlo && a + (sh ? 8 : 4) <= sp.rhi;
}

// the raw reads of one quad: two words (the aligned forms) or four bytes (a
// ragged end) -- registers of their own, so neither form waits for the other
struct QuadRaw {
  uint32_t w0, w1;
  uint32_t b[kQuad];
};

__device__ __forceinline__ void quad_issue(const int8_t* __restrict__ row, int64_t v0,
                                           const Span& sp, QuadRaw& r) {
  unsigned sh;
  if (quad_wide(row, v0, sp, sh)) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(row + v0 - sh);
    r.w0 = q[0];
    if (sh) r.w1 = q[1];
  } else {
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
      r.b[j] = 0xffu;
      if (v0 + j >= sp.lo && v0 + j < sp.hi) r.b[j] = static_cast<uint8_t>(row[v0 + j]);
    }
  }
}

__device__ __forceinline__ uint32_t quad_decode(const int8_t* row, int64_t v0, const Span& sp,
                                                const QuadRaw& r) {
  unsigned sh;
  uint32_t w;
  if (quad_wide(row, v0, sp, sh))
    w = sh ? static_cast<uint32_t>(((static_cast<uint64_t>(r.w1) << 32) | r.w0) >> (8 * sh)) : r.w0;
  else
    w = r.b[0] | (r.b[1] << 8) | (r.b[2] << 16) | (r.b[3] << 24);
#pragma unroll
  for (int j = 0; j < kQuad; ++j)
    if (v0 + j < sp.lo || v0 + j >= sp.hi) w |= 0xffu << (8 * j);
  return w;
}

// One 256-thread workgroup per building, all candidates.  A thread owns 4
// consecutive voxels of a 1024-voxel stride: their truth and floor area are
// read once and reused for every candidate, whose 4 predictions are one or
// two 32-bit reads.  The k confusion matrices are int32 counters in dynamic LDS
// (one matrix per candidate shared by the 4 waves: the adds of one wave
// instruction collide on the few frequent (truth, prediction) pairs whether
// or not the other waves have matrices of their own, and private ones would
// quarter the candidates that fit).  Floor areas: 4 terms per thread in voxel
// order, a butterfly over the wave, the wave's strides in order, the 4 waves
// in order -- a fixed tree, no float atomics.  The same workgroup then scores
// its candidates, picks the winner and copies its rows: no second launch, no
// counter, no memset.
template <bool kTruth>
__global__ void __launch_bounds__(kThreads) k_sweep_select(
    const int8_t* __restrict__ pred, int64_t copy_stride, int copies,
    const int64_t* __restrict__ truth, int K, const int64_t* __restrict__ ptr, int G,
    const float* __restrict__ x, int xs, const float* __restrict__ site, int far_col, int dy_col,
    int dx_col, float scale, int void_class, int criterion, int32_t* __restrict__ conf,
    double* __restrict__ f1, float* __restrict__ far_gen, float* __restrict__ far_ref,
    int32_t* __restrict__ best, int8_t* __restrict__ labels) {
  extern __shared__ int32_t cm[];  // [copies][K][K], kTruth only
  __shared__ float area[kWaves][VG_SELECT_MAX_COPIES];
  __shared__ double s_f1[VG_SELECT_MAX_COPIES];
  __shared__ float s_diff[VG_SELECT_MAX_COPIES];
  __shared__ int s_best;

  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (VG_WAVE - 1), wave = tid / VG_WAVE;
  const int64_t lo = ptr[g], hi = ptr[g + 1];
  const Span sp = {lo, hi, ptr[0], ptr[G]};
  const int KK = K * K;
  // the building's two scalars, read up front (not a further memory round trip after the counting)
  const float ref = hi > lo ? x[lo * xs + far_col] : 0.f;
  const float site_g = hi > lo ? site[lo] : 1.f;
  if (kTruth)
    for (int i = tid; i < copies * KK; i += kThreads) cm[i] = 0;
  for (int i = tid; i < kWaves * VG_SELECT_MAX_COPIES; i += kThreads) (&area[0][0])[i] = 0.f;
  __syncthreads();

  // quads count from the building's first row, whatever the addresses: the
  // order of the floor-area sum depends on nothing but the building
  for (int64_t c0 = lo + static_cast<int64_t>(wave) * VG_WAVE * kQuad; c0 < hi;
       c0 += kThreads * kQuad) {  // uniform per wave: every lane joins the butterfly
    const int64_t v0 = c0 + lane * kQuad;
    int t[kQuad];
    float a[kQuad];
#pragma unroll
    for (int j = 0; j < kQuad; ++j) {
      const int64_t v = v0 + j;
      const bool in = v >= lo && v < hi;
      t[j] = -1;
      a[j] = 0.f;
      if (in) {
        if (kTruth) {
          const int64_t tv = truth[v];
          t[j] = (tv >= 0 && tv < K) ? static_cast<int>(tv) : -1;
        }
        a[j] = (x[v * xs + dy_col] * scale) * (x[v * xs + dx_col] * scale);
      }
    }
    // candidates in groups of kGroup: one memory latency per group, not per candidate
    for (int cb = 0; cb < copies; cb += kGroup) {
      QuadRaw r[kGroup];
#pragma unroll
      for (int i = 0; i < kGroup; ++i)
        if (cb + i < copies) quad_issue(pred + (cb + i) * copy_stride, v0, sp, r[i]);
      float s[kGroup];
#pragma unroll
      for (int i = 0; i < kGroup; ++i) {
        const int c = cb + i;
        s[i] = 0.f;
        if (c >= copies) continue;  // uniform
        const uint32_t w = quad_decode(pred + c * copy_stride, v0, sp, r[i]);
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
          const int p = static_cast<int8_t>((w >> (8 * j)) & 0xff);
          if (p < 0 || p >= K) continue;
          if (kTruth && t[j] >= 0) atomicAdd(&cm[c * KK + t[j] * K + p], 1);
          if (p != void_class) s[i] += a[j];
        }
      }
      // the group's butterflies side by side: 6 dependent exchanges, not 6 per candidate
#pragma unroll
      for (int off = VG_WAVE / 2; off > 0; off >>= 1)
#pragma unroll
        for (int i = 0; i < kGroup; ++i) s[i] += __shfl_xor(s[i], off, VG_WAVE);
      if (lane == 0) {
#pragma unroll
        for (int i = 0; i < kGroup; ++i)
          if (cb + i < copies) area[wave][cb + i] += s[i];
      }
    }
  }
  __syncthreads();

  if (kTruth && conf)
    for (int i = tid; i < copies * KK; i += kThreads)
      conf[(static_cast<size_t>(i / KK) * G + g) * KK + i % KK] = cm[i];

  if (tid < copies) {
    const int c = tid;
    // sklearn f1_score(average="macro", zero_division=0) from the counts
    // (vgan/metrics.py:scores): labels present in truth or prediction, per
    // label 2tp / (2tp + fp + fn) = 2tp / (row + col), their plain mean
    double f = 0.0;
    if (kTruth) {
      const int32_t* m = cm + c * KK;
      int present = 0;
      for (int l = 0; l < K; ++l) {
        int64_t rc = 0;
        for (int j = 0; j < K; ++j) rc += static_cast<int64_t>(m[l * K + j]) + m[j * K + l];
        if (rc > 0) {
          ++present;
          f += 2.0 * static_cast<double>(m[l * K + l]) / static_cast<double>(rc);
        }
      }
      f = present ? f / present : 0.0;
      if (f1) f1[static_cast<size_t>(c) * G + g] = f;
    }
    float fg = 0.f;
    if (hi > lo) fg = (((area[0][c] + area[1][c]) + area[2][c]) + area[3][c]) / site_g;
    if (far_gen) far_gen[static_cast<size_t>(c) * G + g] = fg;
    s_f1[c] = f;
    s_diff[c] = fabsf(fg - ref);
  }
  __syncthreads();
  if (tid == 0) {
    int b = 0;  // strict comparisons: ties (and an all-zero building) keep the lowest index
    for (int c = 1; c < copies; ++c)
      if (criterion == VG_SELECT_F1 ? s_f1[b] < s_f1[c] : s_diff[c] < s_diff[b]) b = c;
    s_best = b;
    best[g] = b;
    if (far_ref) far_ref[g] = ref;
  }
  __syncthreads();
  if (!labels) return;
  const int8_t* __restrict__ row = pred + s_best * copy_stride;
  const int64_t lfirst = lo - static_cast<int64_t>((reinterpret_cast<uintptr_t>(labels) + lo) & 3);
  for (int64_t v0 = lfirst + static_cast<int64_t>(tid) * kQuad; v0 < hi; v0 += kThreads * kQuad) {
    unsigned sh;
    if (v0 >= lo && v0 + kQuad <= hi && quad_wide(row, v0, sp, sh)) {
      QuadRaw r;
      quad_issue(row, v0, sp, r);
      *reinterpret_cast<uint32_t*>(labels + v0) = quad_decode(row, v0, sp, r);  // aligned: lfirst
    } else {
#pragma unroll
      for (int j = 0; j < kQuad; ++j)
        if (v0 + j >= lo && v0 + j < hi) labels[v0 + j] = row[v0 + j];
    }
  }
}

}  // namespace

extern "C" int vg_sweep_select(const int8_t* pred, int64_t copy_stride, int32_t copies,
                               const int64_t* truth, int32_t classes, const int64_t* ptr,
                               int32_t num_graphs, const float* x, int32_t x_stride,
                               const float* site_area, int32_t far_col, int32_t dy_col,
                               int32_t dx_col, float dim_scale, int32_t void_class,
                               int32_t criterion, int32_t* conf, double* f1, float* far_gen,
                               float* far_ref, int32_t* best, int8_t* labels, void* stream) {
  if (!pred || !ptr || !x || !site_area || !best || num_graphs <= 0 || copy_stride < 0) return VG_EINVAL;
  if (copies < 1 || copies > VG_SELECT_MAX_COPIES || classes < 1 || classes > kMaxClasses) return VG_EINVAL;
  const size_t lds = static_cast<size_t>(copies) * classes * classes * sizeof(int32_t);
  if (lds > kLdsBytes) return VG_EINVAL;
  if (criterion != VG_SELECT_F1 && criterion != VG_SELECT_FAR) return VG_EINVAL;
  if (!truth && (criterion == VG_SELECT_F1 || conf || f1)) return VG_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (truth) {
    // the counters plus the kernel's static arrays pass the default 64 KB per
    // workgroup at the largest shapes (the CU has 160 KB)
    if (lds > 48 * 1024) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_sweep_select<true>),
                                               hipFuncAttributeMaxDynamicSharedMemorySize,
                                               static_cast<int>(lds));
      if (e != hipSuccess) return static_cast<int>(e);
    }
    k_sweep_select<true><<<num_graphs, kThreads, lds, s>>>(
        pred, copy_stride, copies, truth, classes, ptr, num_graphs, x, x_stride, site_area, far_col,
        dy_col, dx_col, dim_scale, void_class, criterion, conf, f1, far_gen, far_ref, best, labels);
  } else {
    k_sweep_select<false><<<num_graphs, kThreads, 0, s>>>(
        pred, copy_stride, copies, truth, classes, ptr, num_graphs, x, x_stride, site_area, far_col,
        dy_col, dx_col, dim_scale, void_class, criterion, conf, f1, far_gen, far_ref, best, labels);
  }
  VG_CHECK_LAUNCH();
  return 0;
}
