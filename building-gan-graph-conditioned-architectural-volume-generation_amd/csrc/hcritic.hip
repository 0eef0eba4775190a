// The two kernels the f16 critic scorer (hcritic_engine.hip)
// has of its own -- everything else it runs is the f16 sweep's (half.hip,
// graphnorm.hip):
//   vg_hcritic_embed_labels  vg_critic_embed_labels (score.hip) with f16 rows
//                            out: the critic's first Linear + ReLU for k
//                            stacked candidate labellings from their int8
//                            labels
//   vg_hcritic_decode        the decoder H -> H/2 -> H/4 -> H/8 -> 1 (ReLU
//                            between, optional Sigmoid) in one launch, f16
//                            rows in, f32 scores out
//   vg_hcritic_sigmoid       the Sigmoid behind the per-layer decoder of a
//                            shape vg_hcritic_decode has no kernel for
#include <hip/hip_fp16.h>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxWidth = 256;  // H: the label slab is at most 32 x 256 floats (32 KB) of LDS
constexpr int kMaxClasses = 32;
constexpr int kRowPad = 4;  // floats between slab rows below 256 columns (below)

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  return static_cast<uint32_t>(__half_as_ushort(__float2half_rn(a))) |
         (static_cast<uint32_t>(__half_as_ushort(__float2half_rn(b))) << 16);
}

// y[c N + v, j] = f16(max(0, base[v, j] + W[j, col0 + pred[c, v]])), 0 for the
// pad columns j in [H, Hp), Hp = H rounded up to 8.  The K x H label columns of
// W are staged once per workgroup, transposed to [K][lds_row] (lds_row = Hp +
// kRowPad; Hp itself at 256, where the slab fills 32 KB) with zero pad
// columns, so a voxel's addend is one contiguous 16-byte-aligned LDS row.
// A thread owns 8 consecutive columns of one voxel: 32 bytes of base read once
// for all candidates; per candidate one label byte (the Hp / 8 lanes of a voxel
// read the same one), two 16-byte LDS reads and one 16-byte store.  Lanes with
// the same label read the same LDS addresses (broadcast); rows sit 4 banks
// apart, so rows an odd number of labels apart never share a bank and the
// others cost the 16-lane group one extra cycle at most -- against a 16-byte
// global store per lane.  kVecBase: base 16-byte aligned with ld_base % 4 == 0
// -- float4 reads wherever 4 columns lie inside H; else single floats, the
// same values.
template <bool kVecBase>
__global__ void __launch_bounds__(kThreads) k_hcritic_embed_labels(
    const float* __restrict__ base, int ld_base, const float* __restrict__ W, int ldw, int col0, int K,
    const int8_t* __restrict__ pred, int64_t copy_stride, int copies, int N, int H, int Hp,
    int lds_row, uint16_t* __restrict__ y, int ldy) {
  extern __shared__ float4 slab4[];  // [K][lds_row] floats
  float* slab = reinterpret_cast<float*>(slab4);
  for (int i = threadIdx.x; i < K * Hp; i += kThreads) {
    const int j = i / K, p = i - j * K;  // consecutive threads walk a weight row's K columns
    slab[p * lds_row + j] = j < H ? W[static_cast<size_t>(j) * ldw + col0 + p] : 0.f;
  }
  __syncthreads();

  const int per_row = Hp / 8;
  const int64_t items = static_cast<int64_t>(N) * per_row;
  for (int64_t it = static_cast<int64_t>(blockIdx.x) * kThreads + threadIdx.x; it < items;
       it += static_cast<int64_t>(gridDim.x) * kThreads) {
    const int64_t v = it / per_row;
    const int j0 = static_cast<int>(it - v * per_row) * 8;
    const float* b = base + v * ld_base + j0;
    float bv[8];
#pragma unroll
    for (int hlf = 0; hlf < 2; ++hlf) {
      if (kVecBase && j0 + 4 * hlf + 4 <= H) {
        const float4 t = *reinterpret_cast<const float4*>(b + 4 * hlf);
        bv[4 * hlf] = t.x, bv[4 * hlf + 1] = t.y, bv[4 * hlf + 2] = t.z, bv[4 * hlf + 3] = t.w;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[4 * hlf + i] = j0 + 4 * hlf + i < H ? b[4 * hlf + i] : 0.f;
      }
    }
    // columns at or past H: base read as 0, the slab's pad 0 -> f16(max(0, 0)) = 0
#pragma unroll 4
    for (int c = 0; c < copies; ++c) {
      const int p = pred[c * copy_stride + v];
      float4 w0 = make_float4(0.f, 0.f, 0.f, 0.f), w1 = w0;
      if (p >= 0 && p < K) {
        const float4* row = reinterpret_cast<const float4*>(slab + p * lds_row + j0);
        w0 = row[0];
        w1 = row[1];
      }
      uint4 o;
      o.x = pack2(fmaxf(bv[0] + w0.x, 0.f), fmaxf(bv[1] + w0.y, 0.f));
      o.y = pack2(fmaxf(bv[2] + w0.z, 0.f), fmaxf(bv[3] + w0.w, 0.f));
      o.z = pack2(fmaxf(bv[4] + w1.x, 0.f), fmaxf(bv[5] + w1.y, 0.f));
      o.w = pack2(fmaxf(bv[6] + w1.z, 0.f), fmaxf(bv[7] + w1.w, 0.f));
      *reinterpret_cast<uint4*>(y + (static_cast<int64_t>(c) * N + v) * ldy + j0) = o;
    }
  }
}

// One row per thread.  The parameters, f32, are staged once per workgroup:
// W1 [H/2][H], W2 transposed to [H/2][H/4], W3 [H/8][H/4], W4 [H/8], then the
// biases -- 2757 floats (10.8 KB) at H = 64.  Every weight read is at an
// address common to the wave (a broadcast: no bank conflict).  The row's H
// halves are read as 16-byte pieces and widened to f32 registers; layer 1's
// output j is formed in a rolled loop (its dot product over the H registers
// unrolled), passed through the ReLU and at once folded into layer 2's H/4
// accumulators (column j of W2: why W2 is staged transposed), so the H/2
// values never exist together; layers 3 and 4 are unrolled.  Every sum runs
// in ascending input order from the bias, in f32 FMAs; nothing is rounded
// between the layers.
template <int H>
struct DecodeLayout {
  static constexpr int w1 = 0, w2t = w1 + (H / 2) * H, w3 = w2t + (H / 2) * (H / 4), w4 = w3 + (H / 8) * (H / 4),
                       b1 = w4 + H / 8, b2 = b1 + H / 2, b3 = b2 + H / 4, b4 = b3 + H / 8, total = b4 + 1,
                       padded = (total + 3) / 4 * 4;
};

struct DecodeParams {
  const float* w[4];
  const float* b[4];
};

template <int H>
__global__ void __launch_bounds__(kThreads) k_hcritic_decode(const uint16_t* __restrict__ x, int ld, int rows,
                                                             const DecodeParams P, int has_sigmoid,
                                                             float* __restrict__ out) {
  using L = DecodeLayout<H>;
  __shared__ float4 lds4[L::padded / 4];
  float* lds = reinterpret_cast<float*>(lds4);
  constexpr int H2 = H / 2, H4 = H / 4, H8 = H / 8;
  for (int i = threadIdx.x; i < H2 * H; i += kThreads) lds[L::w1 + i] = P.w[0][i];
  for (int i = threadIdx.x; i < H4 * H2; i += kThreads) {
    const int o = i / H2, j = i - o * H2;  // W2 [H/4][H/2] read in order, stored [j][o]
    lds[L::w2t + j * H4 + o] = P.w[1][i];
  }
  for (int i = threadIdx.x; i < H8 * H4; i += kThreads) lds[L::w3 + i] = P.w[2][i];
  if (threadIdx.x < H8) lds[L::w4 + threadIdx.x] = P.w[3][threadIdx.x];
  for (int i = threadIdx.x; i < H2; i += kThreads) lds[L::b1 + i] = P.b[0] ? P.b[0][i] : 0.f;
  if (threadIdx.x < H4) lds[L::b2 + threadIdx.x] = P.b[1] ? P.b[1][threadIdx.x] : 0.f;
  if (threadIdx.x < H8) lds[L::b3 + threadIdx.x] = P.b[2] ? P.b[2][threadIdx.x] : 0.f;
  if (threadIdx.x == 0) lds[L::b4] = P.b[3] ? P.b[3][0] : 0.f;
  __syncthreads();

  const int r = blockIdx.x * kThreads + threadIdx.x;
  if (r >= rows) return;
  float xv[H];
  const uint4* xr = reinterpret_cast<const uint4*>(x + static_cast<int64_t>(r) * ld);
#pragma unroll
  for (int q = 0; q < H / 8; ++q) {
    const uint4 t = xr[q];
    const uint32_t wds[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xv[8 * q + 2 * i] = __half2float(__ushort_as_half(static_cast<uint16_t>(wds[i] & 0xffffu)));
      xv[8 * q + 2 * i + 1] = __half2float(__ushort_as_half(static_cast<uint16_t>(wds[i] >> 16)));
    }
  }
  float y2[H4];
#pragma unroll
  for (int o = 0; o < H4; ++o) y2[o] = lds[L::b2 + o];
#pragma unroll 1
  for (int j = 0; j < H2; ++j) {
    const float4* wr = reinterpret_cast<const float4*>(lds + L::w1 + j * H);
    float a = lds[L::b1 + j];
#pragma unroll
    for (int q = 0; q < H / 4; ++q) {
      const float4 w = wr[q];
      a = fmaf(w.x, xv[4 * q], a);
      a = fmaf(w.y, xv[4 * q + 1], a);
      a = fmaf(w.z, xv[4 * q + 2], a);
      a = fmaf(w.w, xv[4 * q + 3], a);
    }
    a = fmaxf(a, 0.f);
    const float4* wc = reinterpret_cast<const float4*>(lds + L::w2t + j * H4);
#pragma unroll
    for (int q = 0; q < H4 / 4; ++q) {
      const float4 w = wc[q];
      y2[4 * q] = fmaf(w.x, a, y2[4 * q]);
      y2[4 * q + 1] = fmaf(w.y, a, y2[4 * q + 1]);
      y2[4 * q + 2] = fmaf(w.z, a, y2[4 * q + 2]);
      y2[4 * q + 3] = fmaf(w.w, a, y2[4 * q + 3]);
    }
  }
#pragma unroll
  for (int o = 0; o < H4; ++o) y2[o] = fmaxf(y2[o], 0.f);
  float s = lds[L::b4];
#pragma unroll
  for (int o = 0; o < H8; ++o) {
    float a = lds[L::b3 + o];
#pragma unroll
    for (int j = 0; j < H4; ++j) a = fmaf(lds[L::w3 + o * H4 + j], y2[j], a);
    s = fmaf(lds[L::w4 + o], fmaxf(a, 0.f), s);
  }
  if (has_sigmoid) s = 1.f / (1.f + expf(-s));
  out[r] = s;
}

__global__ void k_hcritic_sigmoid(float* __restrict__ x, int64_t n) {
  for (int64_t i = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n;
       i += static_cast<int64_t>(gridDim.x) * blockDim.x)
    x[i] = 1.f / (1.f + expf(-x[i]));
}

}  // namespace

extern "C" int vg_hcritic_embed_labels(const float* base, int32_t ld_base, const float* W, int32_t ldw,
                                       int32_t col0, int32_t classes, const int8_t* pred, int64_t copy_stride,
                                       int32_t copies, int32_t N, int32_t H, uint16_t* y, int32_t ldy,
                                       void* stream) {
  if (!base || !W || !pred || !y) return VG_EINVAL;
  if (H < 1 || H > kMaxWidth || classes < 1 || classes > kMaxClasses || copies < 1 || N < 1) return VG_EINVAL;
  if (ld_base < H || col0 < 0 || static_cast<int64_t>(ldw) < static_cast<int64_t>(col0) + classes) return VG_EINVAL;
  if (copy_stride < N) return VG_EINVAL;
  if (static_cast<int64_t>(copies) * N > INT32_MAX) return VG_EINVAL;  // the stacked rows index int32 graphs
  const int Hp = (H + 7) / 8 * 8;
  if (ldy % 8 || ldy < Hp || (reinterpret_cast<uintptr_t>(y) & 15)) return VG_EINVAL;
  const bool vec = ld_base % 4 == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0;
  const int64_t items = static_cast<int64_t>(N) * (Hp / 8);
  // a workgroup stages the slab once: at most 2048 of them, each striding over the voxels
  const int blocks = vg_blocks(items, kThreads) < 2048 ? vg_blocks(items, kThreads) : 2048;
  const int lds_row = Hp < kMaxWidth ? Hp + kRowPad : Hp;
  const size_t lds = static_cast<size_t>(classes) * lds_row * sizeof(float);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec)
    k_hcritic_embed_labels<true><<<blocks, kThreads, lds, s>>>(base, ld_base, W, ldw, col0, classes, pred,
                                                               copy_stride, copies, N, H, Hp, lds_row, y, ldy);
  else
    k_hcritic_embed_labels<false><<<blocks, kThreads, lds, s>>>(base, ld_base, W, ldw, col0, classes, pred,
                                                                copy_stride, copies, N, H, Hp, lds_row, y, ldy);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_hcritic_decode(const uint16_t* x, int32_t ld, int32_t rows, const int32_t* widths,
                                 int32_t n_layers, const float* const* weights, const float* const* biases,
                                 int32_t has_sigmoid, float* out, void* stream) {
  if (!x || !widths || !weights || !biases || !out || rows < 1 || n_layers != 4) return VG_EINVAL;
  const int H = widths[0];
  if ((H != 16 && H != 32 && H != 64 && H != 128) || widths[1] != H / 2 || widths[2] != H / 4 ||
      widths[3] != H / 8 || widths[4] != 1)
    return VG_EINVAL;
  if (ld % 8 || ld < H || (reinterpret_cast<uintptr_t>(x) & 15)) return VG_EINVAL;
  DecodeParams P;
  for (int i = 0; i < 4; ++i) {
    if (!weights[i]) return VG_EINVAL;
    P.w[i] = weights[i];
    P.b[i] = biases[i];
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int blocks = vg_blocks(rows, kThreads);
  if (H == 16) k_hcritic_decode<16><<<blocks, kThreads, 0, s>>>(x, ld, rows, P, has_sigmoid, out);
  else if (H == 32) k_hcritic_decode<32><<<blocks, kThreads, 0, s>>>(x, ld, rows, P, has_sigmoid, out);
  else if (H == 64) k_hcritic_decode<64><<<blocks, kThreads, 0, s>>>(x, ld, rows, P, has_sigmoid, out);
  else k_hcritic_decode<128><<<blocks, kThreads, 0, s>>>(x, ld, rows, P, has_sigmoid, out);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_hcritic_sigmoid(float* x, int64_t n, void* stream) {
  if (!x || n < 1) return VG_EINVAL;
  const int blocks = vg_blocks(n, kThreads) < 4096 ? vg_blocks(n, kThreads) : 4096;
  k_hcritic_sigmoid<<<blocks, kThreads, 0, static_cast<hipStream_t>(stream)>>>(x, n);
  VG_CHECK_LAUNCH();
  return 0;
}
