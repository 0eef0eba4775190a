// Best-of-k selection by the critic's score: the two kernels
// around the stacked critic forward of VoxelGNNDiscriminator.score_labels.
//   vg_critic_embed_labels   the critic's first Linear + ReLU (models.py:
//                            166-175 of the reference, over [matched | voxel.x
//                            | one-hot]) for k stacked candidate labellings,
//                            reading their int8 labels: the one-hot's product
//                            is one column of the weight
//   vg_sweep_select_score    per building the mean score of every candidate,
//                            the first arg-max and the gather of its labels
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / VG_WAVE;
constexpr int kMaxWidth = 256;    // H: the label slab is at most 32 x 256 floats of LDS
constexpr int kMaxClasses = 32;
constexpr int kQuad = 4;   // consecutive voxels per thread
constexpr int kGroup = 8;  // candidates whose reads are in flight together

// y[c N + v, :] = max(0, base[v, :] + W[:, col0 + pred[c, v]]).  The K x H
// label columns of W (stride ldw) are staged once per workgroup, transposed to
// [K][H], so that a voxel's addend is one contiguous LDS row.  A thread owns
// kVec consecutive columns of one voxel: its piece of base is read once and
// serves every candidate; per candidate one label byte (the 16 lanes of a row
// read the same one), one LDS read and one store.  kVec = 4: H % 4 == 0 and
// base, its stride and y 16-byte aligned -- float4 all the way.
template <int kVec>
__global__ void __launch_bounds__(kThreads) k_critic_embed_labels(
    const float* __restrict__ base, int ld_base, const float* __restrict__ W, int ldw, int col0, int K,
    const int8_t* __restrict__ pred, int64_t copy_stride, int copies, int N, int H,
    float* __restrict__ y) {
  extern __shared__ float4 slab4[];  // [K][H] floats
  float* slab = reinterpret_cast<float*>(slab4);
  for (int i = threadIdx.x; i < K * H; i += kThreads) {
    const int j = i / K, p = i - j * K;  // consecutive threads walk a weight row's K columns
    slab[p * H + j] = W[static_cast<size_t>(j) * ldw + col0 + p];
  }
  __syncthreads();

  const int per_row = H / kVec;
  const int64_t items = static_cast<int64_t>(N) * per_row;
  const int64_t rows = static_cast<int64_t>(N);
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t v = it / per_row;
    const int q = static_cast<int>(it - v * per_row);
    if (kVec == 4) {
      const float4 b = *reinterpret_cast<const float4*>(base + v * ld_base + q * 4);
#pragma unroll 4
      for (int c = 0; c < copies; ++c) {
        const int p = pred[c * copy_stride + v];
        float4 w = make_float4(0.f, 0.f, 0.f, 0.f);
        if (p >= 0 && p < K) w = slab4[p * per_row + q];
        const float4 o = make_float4(fmaxf(b.x + w.x, 0.f), fmaxf(b.y + w.y, 0.f), fmaxf(b.z + w.z, 0.f),
                                     fmaxf(b.w + w.w, 0.f));
        *reinterpret_cast<float4*>(y + (c * rows + v) * H + q * 4) = o;
      }
    } else {
      const float b = base[v * ld_base + q];
#pragma unroll 4
      for (int c = 0; c < copies; ++c) {
        const int p = pred[c * copy_stride + v];
        const float w = (p >= 0 && p < K) ? slab[p * H + q] : 0.f;
        y[(c * rows + v) * H + q] = fmaxf(b + w, 0.f);
      }
    }
  }
}

// The 4 values row[v0 .. v0+3] of one candidate's score row, 0 outside the
// building's rows [lo, hi): one float4 where the address is 16-byte aligned
// and the quad lies inside the building, the building's own floats otherwise.
__device__ __forceinline__ float4 quad_scores(const float* __restrict__ row, int64_t v0, int64_t lo,
                                              int64_t hi) {
  if (v0 + kQuad <= hi && (reinterpret_cast<uintptr_t>(row + v0) & 15) == 0)
    return *reinterpret_cast<const float4*>(row + v0);
  float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
  if (v0 < hi) r.x = row[v0];
  if (v0 + 1 < hi) r.y = row[v0 + 1];
  if (v0 + 2 < hi) r.z = row[v0 + 2];
  if (v0 + 3 < hi) r.w = row[v0 + 3];
  return r;
}

// One 256-thread workgroup per building, all candidates, in groups of kGroup.
// A thread owns 4 consecutive voxels of a 1024-voxel stride, counted from the
// building's first row whatever the addresses.  The sum of a candidate is f64
// in a fixed tree: a thread's terms in voxel order, a butterfly over the wave,
// the 4 waves in order -- no atomics, the same bits every run.  Thread 0 keeps
// the running first arg-max (strict >: a tie or a NaN never replaces an
// earlier candidate); the workgroup then copies the winner's labels.
__global__ void __launch_bounds__(kThreads) k_sweep_select_score(
    const float* __restrict__ scores, int64_t score_stride, const int8_t* __restrict__ pred,
    int64_t copy_stride, int copies, const int64_t* __restrict__ ptr, int G, int64_t N,
    double* __restrict__ score, int32_t* __restrict__ best, int8_t* __restrict__ labels) {
  __shared__ double part[kWaves][kGroup];
  __shared__ double s_val[kGroup];
  __shared__ int s_best;

  const int g = blockIdx.x;
  const int tid = threadIdx.x, lane = tid & (VG_WAVE - 1), wave = tid / VG_WAVE;
  // a building's rows, kept inside the candidate rows whatever ptr holds
  const int64_t p0 = ptr[g], p1 = ptr[g + 1];
  const int64_t lo = p0 < 0 ? 0 : p0 > N ? N : p0;
  const int64_t hi = p1 < lo ? lo : p1 > N ? N : p1;
  const double count = static_cast<double>(hi - lo);
  int b = 0;
  double bv = 0.0;  // thread 0 only

  for (int cb = 0; cb < copies; cb += kGroup) {
    double acc[kGroup];
#pragma unroll
    for (int i = 0; i < kGroup; ++i) acc[i] = 0.0;
    for (int64_t v0 = lo + static_cast<int64_t>(tid) * kQuad; v0 < hi; v0 += kThreads * kQuad) {
      float4 r[kGroup];
#pragma unroll
      for (int i = 0; i < kGroup; ++i)
        if (cb + i < copies) r[i] = quad_scores(scores + (cb + i) * score_stride, v0, lo, hi);
#pragma unroll
      for (int i = 0; i < kGroup; ++i)
        if (cb + i < copies) {
          acc[i] += static_cast<double>(r[i].x);
          acc[i] += static_cast<double>(r[i].y);
          acc[i] += static_cast<double>(r[i].z);
          acc[i] += static_cast<double>(r[i].w);
        }
    }
    // the group's butterflies side by side: 6 dependent exchanges, not 6 per candidate
#pragma unroll
    for (int off = VG_WAVE / 2; off > 0; off >>= 1)
#pragma unroll
      for (int i = 0; i < kGroup; ++i) acc[i] += __shfl_xor(acc[i], off, VG_WAVE);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < kGroup; ++i) part[wave][i] = acc[i];
    }
    __syncthreads();
    if (tid < kGroup && cb + tid < copies) {
      const double s = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
      const double m = hi > lo ? s / count : 0.0;  // an empty building scores 0
      score[static_cast<size_t>(cb + tid) * G + g] = m;
      s_val[tid] = m;
    }
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < kGroup && cb + i < copies; ++i) {
        if (cb + i == 0) {
          bv = s_val[0];
        } else if (s_val[i] > bv) {
          b = cb + i;
          bv = s_val[i];
        }
      }
    }
  }
  if (tid == 0) {
    s_best = b;
    best[g] = b;
  }
  __syncthreads();
  if (!labels) return;

  // the winner's bytes [lo, hi): aligned 32-bit stores, each from the one or
  // two aligned source words it straddles (a candidate row starts at any byte;
  // every byte read lies in the row's [0, N)), single bytes at the ragged ends
  const int8_t* __restrict__ row = pred + s_best * copy_stride;
  const int64_t first = lo - static_cast<int64_t>((reinterpret_cast<uintptr_t>(labels) + lo) & 3);
  for (int64_t v0 = first + static_cast<int64_t>(tid) * kQuad; v0 < hi; v0 += kThreads * kQuad) {
    const unsigned sh = reinterpret_cast<uintptr_t>(row + v0) & 3;
    const int64_t a = v0 - sh;  // voxel of the first byte read
    if (v0 >= lo && v0 + kQuad <= hi && a >= 0 && a + (sh ? 8 : 4) <= N) {
      const uint32_t* q = reinterpret_cast<const uint32_t*>(row + a);
      uint32_t w = q[0];
      if (sh) w = static_cast<uint32_t>(((static_cast<uint64_t>(q[1]) << 32) | w) >> (8 * sh));
      *reinterpret_cast<uint32_t*>(labels + v0) = w;
    } else {
#pragma unroll
      for (int j = 0; j < kQuad; ++j)
        if (v0 + j >= lo && v0 + j < hi) labels[v0 + j] = row[v0 + j];
    }
  }
}

}  // namespace

extern "C" int vg_critic_embed_labels(const float* base, int32_t ld_base, const float* W, int32_t ldw,
                                      int32_t col0, int32_t classes, const int8_t* pred,
                                      int64_t copy_stride, int32_t copies, int32_t N, int32_t H, float* y,
                                      void* stream) {
  if (!base || !W || !pred || !y) return VG_EINVAL;
  if (H < 1 || H > kMaxWidth || classes < 1 || classes > kMaxClasses || copies < 1 || N < 1) return VG_EINVAL;
  if (ld_base < H || col0 < 0 || static_cast<int64_t>(ldw) < static_cast<int64_t>(col0) + classes) return VG_EINVAL;
  if (copy_stride < N) return VG_EINVAL;
  if (static_cast<int64_t>(copies) * N > INT32_MAX) return VG_EINVAL;  // the stacked rows index int32 graphs
  const bool vec = H % 4 == 0 && ld_base % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(y) & 15) == 0;
  const int64_t items = static_cast<int64_t>(N) * (vec ? H / 4 : H);
  // a workgroup stages the slab once: at most 2048 of them, each striding over the voxels
  const int blocks = vg_blocks(items, kThreads) < 2048 ? vg_blocks(items, kThreads) : 2048;
  const size_t lds = static_cast<size_t>(classes) * H * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    k_critic_embed_labels<4><<<blocks, kThreads, lds, s>>>(base, ld_base, W, ldw, col0, classes, pred,
                                                           copy_stride, copies, N, H, y);
  else
    k_critic_embed_labels<1><<<blocks, kThreads, lds, s>>>(base, ld_base, W, ldw, col0, classes, pred,
                                                           copy_stride, copies, N, H, y);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_sweep_select_score(const float* scores, int64_t score_stride, const int8_t* pred,
                                     int64_t copy_stride, int32_t copies, const int64_t* ptr,
                                     int32_t num_graphs, int64_t N, double* score, int32_t* best,
                                     int8_t* labels, void* stream) {
  if (!scores || !pred || !ptr || !score || !best) return VG_EINVAL;
  if (copies < 1 || num_graphs < 1 || N < 1) return VG_EINVAL;
  if (score_stride < N || copy_stride < N) return VG_EINVAL;
  k_sweep_select_score<<<num_graphs, kThreads, 0, static_cast<hipStream_t>(stream)>>>(
      scores, score_stride, pred, copy_stride, copies, ptr, num_graphs, N, score, best, labels);
  VG_CHECK_LAUNCH();
  return 0;
}
