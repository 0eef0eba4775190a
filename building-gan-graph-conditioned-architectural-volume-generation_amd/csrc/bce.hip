// Loss head of the BCE critic engine (USE_WGANGP = False, vgan/bce.py).
//
// vg_bce_critic_head  from the stacked pre-sigmoid scores s [2N] (rows [0,N)
//                  D(real), target 1; rows [N,2N) D(fake), target 0):
//                  p = sigmoid(s)                         (models.py:185, the decoder's Sigmoid)
//                  loss = BCE(p_fake, 0) + BCE(p_real, 1) (trainer.py:329-330)
//                  seeds = dloss/ds, the adjoint seeds of the engine's backward.
//                  Row-parallel like vg_gp_head; per-block sums folded in block
//                  order by the last block to finish (no float atomics:
//                  bit-identical run to run).
#include "common.h"
#include "bce.h"

namespace {

__global__ void __launch_bounds__(256) k_bce_critic_head(const float* __restrict__ s, int N,
                                                         float* __restrict__ seeds,
                                                         float* __restrict__ part, int* counter,
                                                         float* __restrict__ out) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float fn = static_cast<float>(N);
  float lr = 0.f, lf = 0.f;
  const int n = blockIdx.x * 256 + t;
  if (n < N) {
    float g;
    vg_bce_row<true>(s[n], fn, lr, g);
    seeds[n] = g;
    vg_bce_row<false>(s[(size_t)N + n], fn, lf, g);
    seeds[(size_t)N + n] = g;
  }
  for (int off = 32; off > 0; off >>= 1) {
    lr += __shfl_xor(lr, off, 64);
    lf += __shfl_xor(lf, off, 64);
  }
  __shared__ float red[4][2];
  if (lane == 0) {
    red[wave][0] = lr;
    red[wave][1] = lf;
  }
  __syncthreads();
  if (t < 2) part[blockIdx.x * 2 + t] = ((red[0][t] + red[1][t]) + red[2][t]) + red[3][t];
  if (vg_last_block(counter) && t == 0) {
    float a = 0.f, b = 0.f;
    for (int k = 0; k < (int)gridDim.x; ++k) {
      a += part[k * 2];
      b += part[k * 2 + 1];
    }
    const float real = a / fn, fake = b / fn;
    out[0] = fake + real;  // the reference's order (trainer.py:329-330)
    out[1] = real;
    out[2] = fake;
  }
}

}  // namespace

extern "C" int64_t vg_bce_critic_head_ws_floats(int32_t N) { return 2 * (int64_t)vg_blocks(N, 256); }

extern "C" int vg_bce_critic_head(const float* s, int32_t N, float* out, float* seeds, float* workspace,
                                  int32_t* sync, void* stream) {
  if (N <= 0 || !s || !out || !seeds || !workspace || !sync) return VG_EINVAL;
  k_bce_critic_head<<<vg_blocks(N, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(s, N, seeds, workspace, sync,
                                                                                   out);
  VG_CHECK_LAUNCH();
  return 0;
}
