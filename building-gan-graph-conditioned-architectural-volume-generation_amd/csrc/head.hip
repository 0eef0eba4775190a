// Gumbel-softmax type head, per-building loss/metric reductions, flat Adam.
#include "common.h"
#include "bce.h"

namespace {

constexpr int kMaxClasses = 32;

// models.py:150-153 -- F.gumbel_softmax(logits, tau=1.0) (hard=False):
//   g = -log(E), E ~ Exp(1);  soft = softmax((logits + g) / tau)
// then label_hard = onehot(argmax soft) - soft.detach() + soft.
// tau_dev != NULL: row r uses tau_dev[r / seg_rows] (per-copy temperatures of a
// stacked inference sweep, read from device memory so a replayed hipGraph
// follows the schedule).
__global__ void k_gumbel_fwd(const float* __restrict__ logits, const float* __restrict__ noise,
                             int rows, int K, float tau, float* __restrict__ soft,
                             float* __restrict__ hard, int32_t* __restrict__ idx,
                             const float* __restrict__ tau_dev = nullptr, int seg_rows = 1) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  if (tau_dev) tau = tau_dev[r / seg_rows];
  float y[kMaxClasses];
  float mx = -INFINITY;
  for (int k = 0; k < K; ++k) {
    const float g = -logf(noise[(size_t)r * K + k]);
    y[k] = (logits[(size_t)r * K + k] + g) / tau;
    mx = fmaxf(mx, y[k]);
  }
  float sum = 0.f;
  for (int k = 0; k < K; ++k) {
    y[k] = expf(y[k] - mx);
    sum += y[k];
  }
  int best = 0;
  float bv = -INFINITY;
  for (int k = 0; k < K; ++k) {
    y[k] = y[k] / sum;
    if (y[k] > bv) {  // strict: first maximum wins (torch.argmax)
      bv = y[k];
      best = k;
    }
  }
  for (int k = 0; k < K; ++k) {
    soft[(size_t)r * K + k] = y[k];
    const float oh = (k == best) ? 1.f : 0.f;
    hard[(size_t)r * K + k] = (oh - y[k]) + y[k];
  }
  if (idx) idx[r] = best;
}

__global__ void k_gumbel_bwd(const float* __restrict__ soft, const float* __restrict__ gh,
                             const float* __restrict__ gs, int rows, int K, float tau,
                             float* __restrict__ gl) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float dot = 0.f;
  for (int k = 0; k < K; ++k) {
    const size_t t = (size_t)r * K + k;
    const float g = (gh ? gh[t] : 0.f) + (gs ? gs[t] : 0.f);
    dot = fmaf(soft[t], g, dot);
  }
  for (int k = 0; k < K; ++k) {
    const size_t t = (size_t)r * K + k;
    const float g = (gh ? gh[t] : 0.f) + (gs ? gs[t] : 0.f);
    gl[t] = soft[t] * (g - dot) / tau;
  }
}

__device__ __forceinline__ int row_argmax(const float* __restrict__ row, int K) {
  int best = 0;
  float bv = row[0];
  for (int k = 1; k < K; ++k)
    if (row[k] > bv) {
      bv = row[k];
      best = k;
    }
  return best;
}

// trainer.py:357-378, one 256-thread block per building
__global__ void __launch_bounds__(256) k_far(const float* __restrict__ x, int xs,
                                             const float* __restrict__ label, int K,
                                             const int64_t* __restrict__ ptr,
                                             const float* __restrict__ site, int far_col,
                                             int dy_col, int dx_col, float scale, int void_class,
                                             float* __restrict__ far_gen,
                                             float* __restrict__ far_ref) {
  const int gi = blockIdx.x;
  const int lo = static_cast<int>(ptr[gi]), hi = static_cast<int>(ptr[gi + 1]);
  float acc = 0.f;
  for (int v = lo + threadIdx.x; v < hi; v += blockDim.x) {
    if (row_argmax(label + (size_t)v * K, K) != void_class)
      acc += (x[(size_t)v * xs + dy_col] * scale) * (x[(size_t)v * xs + dx_col] * scale);
  }
  __shared__ float red[256];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    far_gen[gi] = hi > lo ? red[0] / site[lo] : 0.f;
    far_ref[gi] = hi > lo ? x[(size_t)lo * xs + far_col] : 0.f;
  }
}

// trainer.py:387-443 -- per-building confusion matrices (truth x prediction)
__global__ void __launch_bounds__(256) k_confusion(const int64_t* __restrict__ truth,
                                                   const float* __restrict__ label, int K,
                                                   const int64_t* __restrict__ ptr,
                                                   int32_t* __restrict__ conf,
                                                   int32_t* __restrict__ conf_all) {
  const int gi = blockIdx.x;
  __shared__ int32_t cm[kMaxClasses * kMaxClasses];
  for (int t = threadIdx.x; t < K * K; t += blockDim.x) cm[t] = 0;
  __syncthreads();
  const int lo = static_cast<int>(ptr[gi]), hi = static_cast<int>(ptr[gi + 1]);
  for (int v = lo + threadIdx.x; v < hi; v += blockDim.x) {
    const int64_t t = truth[v];
    const int p = row_argmax(label + (size_t)v * K, K);
    if (t >= 0 && t < K) atomicAdd(&cm[t * K + p], 1);
  }
  __syncthreads();
  for (int t = threadIdx.x; t < K * K; t += blockDim.x) conf[(size_t)gi * K * K + t] = cm[t];
}

// The whole batch's matrix: per entry the sum over the buildings in order
// (no memset node and no atomics in a captured evaluation graph; deterministic).
__global__ void __launch_bounds__(64) k_confusion_all(const int32_t* __restrict__ conf, int G, int KK,
                                                      int32_t* __restrict__ conf_all) {
  for (int t = threadIdx.x; t < KK; t += blockDim.x) {
    int32_t s = 0;
    for (int g = 0; g < G; ++g) s += conf[(size_t)g * KK + t];
    conf_all[t] = s;
  }
}

// torch.optim.Adam single-tensor update (torch/optim/adam.py, _single_tensor_adam):
//   g += wd * p;  m.lerp_(g, 1 - b1);  v = v*b2 + ((1-b2)*g)*g
//   p += (-step_size * m) / (sqrt(v) / bc2_sqrt + eps)       (addcdiv order)
// (1 - b1), (1 - b2), step_size and bc2_sqrt arrive pre-rounded from double
// exactly as the Python scalars reach the ATen kernels.
// The roundings are those of ATen's vectorised CPU kernels, written out so no
// contraction choice of the compiler enters: add(alpha) and at::lerp are one
// fused multiply-add each, addcmul_ adds the rounded v*b2 to ((1-b2)*g)*g in a
// fused multiply-add ((1-b2)*g rounded first); sqrt, both divisions and the
// final sum are rounded one by one.  Both moments are then bit-identical to
// torch's on the CPU (tests/test_head_gpu.py).
__device__ __forceinline__ void adam_element(float& p, float g, float& m, float& v, float b2, float omb1,
                                             float omb2, float eps, float wd, float neg_step,
                                             float bc2_sqrt) {
  const float gi = wd != 0.f ? fmaf(wd, p, g) : g;
  const float d = gi - m;
  // at::lerp: |w| < 0.5 ? self + w*(end-self) : end - (end-self)*(1-w)
  const float mn = (fabsf(omb1) < 0.5f) ? fmaf(omb1, d, m) : fmaf(omb1 - 1.f, d, gi);
  const float vn = fmaf(omb2 * gi, gi, v * b2);
  m = mn;
  v = vn;
  const float denom = sqrtf(vn) / bc2_sqrt + eps;
  p = p + (neg_step * mn) / denom;
}

__global__ void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                       float* __restrict__ v, long long n, float b2, float omb1, float omb2,
                       float eps, float wd, float neg_step, float bc2_sqrt) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    adam_element(p[i], g[i], m[i], v[i], b2, omb1, omb2, eps, wd, neg_step, bc2_sqrt);
  }
}

// Same update with the step count and learning rate read from device memory
// (hipGraph replays: host scalars would be frozen into the graph).  Bias
// corrections are formed in double exactly as torch forms them in Python.
// The bookkeeping that opens every training iteration, as one launch: the
// device RNG's iteration counter += 1 (RNG.reset), the optimizer's step count
// += 1 (the increment optimizer.step() makes before its update, made here so
// the update kernel reads a settled count) and the flat gradient zeroed
// (optimizer.zero_grad(), trainer.py:475, 486).  Each pointer may be NULL.
__global__ void k_iter_begin(long long* __restrict__ ctr, int32_t* __restrict__ step, float* __restrict__ grad,
                             long long n) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    if (ctr) *ctr += 1;
    if (step) *step += 1;
  }
  if (!grad) return;
  const long long q = n >> 2;
  float4* g4 = reinterpret_cast<float4*>(grad);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < q; i += (long long)gridDim.x * blockDim.x)
    g4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (long long i = 4 * q + blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x)
    grad[i] = 0.f;
}

__global__ void k_adam_dev(float* __restrict__ p, const float* __restrict__ g,
                           float* __restrict__ m, float* __restrict__ v, long long n, double b1,
                           double b2, float eps, float wd, const double* __restrict__ lr_p,
                           const int32_t* __restrict__ step_p) {
  const double t = static_cast<double>(*step_p);
  const double lr = *lr_p;
  const float neg_step = static_cast<float>(-(lr / (1.0 - pow(b1, t))));
  const float bc2_sqrt = static_cast<float>(sqrt(1.0 - pow(b2, t)));
  const float fb2 = static_cast<float>(b2), omb1 = static_cast<float>(1.0 - b1),
              omb2 = static_cast<float>(1.0 - b2);
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n;
       i += (long long)gridDim.x * blockDim.x) {
    adam_element(p[i], g[i], m[i], v[i], fb2, omb1, omb2, eps, wd, neg_step, bc2_sqrt);
  }
}

// ---------------------------------------------------------------- generator loss head
// trainer.py:334-385 with USE_WGANGP (the FAR term has no gradient, :380):
//   loss = (((adv + ratio) + ce) + ratio_void) + far
//   adv = -mean(d_fake) l_adv;  ce = CE(logits, type) l_label
//   rg = sum_n hard / N, rr = sum_n onehot / N
//   ratio = mean_{c<K-2} (rg - rr)^2 l_ratio;  ratio_void = mean_{c>=K-2} (rg - rr)^2 l_void
//   far = mean_g (far_gen - far_ref)^2 l_far
// Partial row of block b: [sum d_fake | sum hard[:, c] (K) | sum onehot[:, c] (K) | sum ce_n].
// BCE (USE_WGANGP = False, trainer.py:341): d_fake holds D's pre-sigmoid
// scores, adv = mean(-max(log sigmoid(d_fake), -100)) l_adv (vg_bce_row, bce.h);
// the first partial is the sum of those terms and every other term is shared.
constexpr int kGLThreads = 256;
constexpr int kGLMaxBlocks = 256;

template <int KM, bool BCE>  // KM >= K: class-count bound the loops unroll to (8 or kMaxClasses)
__global__ void __launch_bounds__(kGLThreads) k_gen_loss_partial(
    const float* __restrict__ d_fake, const float* __restrict__ hard,
    const float* __restrict__ logits, const float* __restrict__ onehot,
    const int64_t* __restrict__ type, int N, int K, float* __restrict__ part) {
  constexpr int WM = 2 * KM + 2;
  const int W = 2 * K + 2;
  // acc slots: [0] d_fake, [1 + c] hard, [1 + KM + c] onehot, [WM - 1] ce
  float acc[WM];
#pragma unroll
  for (int i = 0; i < WM; ++i) acc[i] = 0.f;
  for (int n = blockIdx.x * blockDim.x + threadIdx.x; n < N; n += gridDim.x * blockDim.x) {
    if (BCE) {
      float unused;
      vg_bce_row<true>(d_fake[n], 1.f, acc[0], unused);
    } else {
      acc[0] += d_fake[n];
    }
    float lg[KM];
    float m = -INFINITY;
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) {
        acc[1 + c] += hard[(size_t)n * K + c];
        acc[1 + KM + c] += onehot[(size_t)n * K + c];
        lg[c] = logits[(size_t)n * K + c];
        m = fmaxf(m, lg[c]);
      }
    float se = 0.f, lt = 0.f;
    const int64_t ty = type[n];
#pragma unroll
    for (int c = 0; c < KM; ++c)
      if (c < K) {
        se += expf(lg[c] - m);
        if (c == ty) lt = lg[c];
      }
    acc[WM - 1] += (m + logf(se)) - lt;
  }
  // fixed-order reduction: xor tree inside each wave, then the waves in order
#pragma unroll
  for (int i = 0; i < WM; ++i)
    for (int off = 32; off > 0; off >>= 1) acc[i] += __shfl_xor(acc[i], off, 64);
  __shared__ float red[kGLThreads / 64][WM];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int i = 0; i < WM; ++i) red[wave][i] = acc[i];
  __syncthreads();
  if ((int)threadIdx.x < W) {  // output slot -> acc slot
    const int i = threadIdx.x;
    const int slot = i == 0 ? 0 : i <= K ? i : i <= 2 * K ? 1 + KM + (i - 1 - K) : WM - 1;
    float v = 0.f;
    for (int w = 0; w < kGLThreads / 64; ++w) v += red[w][slot];
    part[(size_t)blockIdx.x * W + i] = v;
  }
}

// out: [0] loss, [1..K] d loss / d hard[n, c], [K+1] d loss / d d_fake[n],
// [K+2] l_label / N (the cross-entropy gradient scale).  BCE: [K+1] = l_adv,
// the scale of the per-row d adv / d d_fake[n] that k_gen_loss_bwd forms.
template <bool BCE>
__global__ void __launch_bounds__(1024) k_gen_loss_final(const float* __restrict__ part, int nb, int N,
                                                       int K, const float* __restrict__ far_gen,
                                                       const float* __restrict__ far_ref, int G,
                                                       float l_adv, float l_label, float l_ratio,
                                                       float l_void, float l_far,
                                                       float* __restrict__ out) {
  __shared__ float tot[2 * kMaxClasses + 2];
  const int W = 2 * K + 2;
  {  // one wave per value, lanes over the partial rows, fixed xor tree
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = wave; i < W; i += blockDim.x / 64) {
      float v = 0.f;
      for (int b = lane; b < nb; b += 64) v += part[(size_t)b * W + i];
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) tot[i] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  const float fn = static_cast<float>(N);
  const float adv = BCE ? (tot[0] / fn) * l_adv : -(tot[0] / fn) * l_adv;
  float r1 = 0.f, r2 = 0.f;
  const int k1 = K - 2;
  for (int c = 0; c < K; ++c) {
    const float d = tot[1 + c] / fn - tot[1 + K + c] / fn;
    if (c < k1) r1 += d * d;
    else r2 += d * d;
    out[1 + c] = (c < k1 ? l_ratio * 2.f * d / k1 : l_void * 2.f * d / 2.f) / fn;
  }
  const float ratio = (r1 / k1) * l_ratio, ratio_void = (r2 / 2.f) * l_void;
  const float ce = (tot[2 * K + 1] / fn) * l_label;
  float f = 0.f;
  for (int g = 0; g < G; ++g) {
    const float d = far_gen[g] - far_ref[g];
    f += d * d;
  }
  const float far = (f / G) * l_far;
  out[0] = (((adv + ratio) + ce) + ratio_void) + far;
  out[K + 1] = BCE ? l_adv : -l_adv / fn;
  out[K + 2] = l_label / fn;
}

// BCE: d_fake [N] are the scores the forward read (the adversarial gradient
// depends on each row's score; under WGAN-GP it is one constant and d_fake is
// not read).
template <bool BCE>
__global__ void k_gen_loss_bwd(const float* __restrict__ g_loss, const float* __restrict__ coef,
                               const float* __restrict__ d_fake, const float* __restrict__ logits,
                               const int64_t* __restrict__ type, int N, int K, float* __restrict__ g_dfake,
                               float* __restrict__ g_hard, float* __restrict__ g_logits) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const float g = *g_loss;
  if (g_dfake) {
    if (BCE) {
      float unused = 0.f, ds;
      vg_bce_row<true>(d_fake[n], static_cast<float>(N), unused, ds);
      g_dfake[n] = (g * coef[K + 1]) * ds;
    } else {
      g_dfake[n] = g * coef[K + 1];
    }
  }
  if (g_hard)
    for (int c = 0; c < K; ++c) g_hard[(size_t)n * K + c] = g * coef[1 + c];
  if (g_logits) {
    float m = -INFINITY;
    for (int c = 0; c < K; ++c) m = fmaxf(m, logits[(size_t)n * K + c]);
    float se = 0.f;
    for (int c = 0; c < K; ++c) se += expf(logits[(size_t)n * K + c] - m);
    const float sc = g * coef[K + 2];
    for (int c = 0; c < K; ++c) {
      const float p = expf(logits[(size_t)n * K + c] - m) / se;
      g_logits[(size_t)n * K + c] = sc * (p - (c == type[n] ? 1.f : 0.f));
    }
  }
}

}  // namespace

extern "C" int vg_gumbel_fwd(const float* logits, const float* noise, int32_t rows,
                             int32_t classes, float tau, float* soft, float* hard, int32_t* idx,
                             void* stream) {
  if (rows <= 0 || classes <= 0 || classes > kMaxClasses || !logits || !noise || !soft || !hard)
    return VG_EINVAL;
  k_gumbel_fwd<<<vg_blocks(rows, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      logits, noise, rows, classes, tau, soft, hard, idx);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_gumbel_fwd_dev(const float* logits, const float* noise, int32_t rows,
                                 int32_t classes, const float* tau, int32_t seg_rows, float* soft,
                                 float* hard, int32_t* idx, void* stream) {
  if (rows <= 0 || classes <= 0 || classes > kMaxClasses || seg_rows <= 0 || !logits || !noise ||
      !tau || !soft || !hard)
    return VG_EINVAL;
  k_gumbel_fwd<<<vg_blocks(rows, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      logits, noise, rows, classes, 1.f, soft, hard, idx, tau, seg_rows);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_gumbel_bwd(const float* soft, const float* g_hard, const float* g_soft,
                             int32_t rows, int32_t classes, float tau, float* g_logits,
                             void* stream) {
  if (rows <= 0 || classes <= 0 || classes > kMaxClasses || !soft || !g_logits) return VG_EINVAL;
  k_gumbel_bwd<<<vg_blocks(rows, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      soft, g_hard, g_soft, rows, classes, tau, g_logits);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_far_per_graph(const float* x, int32_t x_stride, const float* label,
                                int32_t classes, const int64_t* ptr, int32_t num_graphs,
                                const float* site_area, int32_t far_col, int32_t dy_col,
                                int32_t dx_col, float dim_scale, int32_t void_class,
                                float* far_gen, float* far_ref, void* stream) {
  if (num_graphs <= 0 || classes <= 0 || classes > kMaxClasses || !x || !label || !ptr ||
      !site_area || !far_gen || !far_ref)
    return VG_EINVAL;
  k_far<<<num_graphs, 256, 0, static_cast<hipStream_t>(stream)>>>(
      x, x_stride, label, classes, ptr, site_area, far_col, dy_col, dx_col, dim_scale, void_class,
      far_gen, far_ref);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_confusion(const int64_t* truth, const float* label, int32_t classes,
                            const int64_t* ptr, int32_t num_graphs, int32_t* conf,
                            int32_t* conf_all, void* stream) {
  if (num_graphs <= 0 || classes <= 0 || classes > kMaxClasses || !truth || !label || !ptr ||
      !conf)
    return VG_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  k_confusion<<<num_graphs, 256, 0, s>>>(truth, label, classes, ptr, conf, conf_all);
  if (conf_all) k_confusion_all<<<1, 64, 0, s>>>(conf, num_graphs, classes * classes, conf_all);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_adam(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                       int64_t n, float beta2, float one_minus_beta1, float one_minus_beta2,
                       float eps, float weight_decay, float step_size, float bc2_sqrt,
                       void* stream) {
  if (n < 0 || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq))) return VG_EINVAL;
  if (n == 0) return 0;
  int blocks = vg_blocks(n, 256);
  if (blocks > 2048) blocks = 2048;
  k_adam<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, n, beta2, one_minus_beta1, one_minus_beta2, eps,
      weight_decay, -step_size, bc2_sqrt);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_adam_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                           int64_t n, double beta1, double beta2, float eps, float weight_decay,
                           const double* lr, const int32_t* step, void* stream) {
  if (n < 0 || !lr || !step || (n > 0 && (!param || !grad || !exp_avg || !exp_avg_sq)))
    return VG_EINVAL;
  if (n == 0) return 0;
  int blocks = vg_blocks(n, 256);
  if (blocks > 2048) blocks = 2048;
  k_adam_dev<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(
      param, grad, exp_avg, exp_avg_sq, n, beta1, beta2, eps, weight_decay, lr, step);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_iter_begin(int64_t* rng_iter, int32_t* step, float* grad, int64_t n, void* stream) {
  if (n < 0 || (grad && (reinterpret_cast<uintptr_t>(grad) & 15))) return VG_EINVAL;
  long long blocks = vg_blocks((n >> 2) + 1, 256);
  if (blocks > 1024) blocks = 1024;
  k_iter_begin<<<static_cast<int>(blocks), 256, 0, static_cast<hipStream_t>(stream)>>>(
      reinterpret_cast<long long*>(rng_iter), step, n > 0 ? grad : nullptr, n);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int64_t vg_gen_loss_ws_floats(int32_t N, int32_t classes) {
  const int nb = vg_blocks(N, kGLThreads) < kGLMaxBlocks ? vg_blocks(N, kGLThreads) : kGLMaxBlocks;
  return (int64_t)nb * (2 * classes + 2);
}

namespace {
template <bool BCE>
int gen_loss_fwd(const float* d_fake, const float* hard, const float* logits, const float* onehot,
                 const int64_t* type, int32_t N, int32_t classes, const float* far_gen, const float* far_ref,
                 int32_t num_graphs, float l_adv, float l_label, float l_ratio, float l_void, float l_far,
                 float* out, float* workspace, void* stream) {
  if (N <= 0 || classes < 3 || classes > kMaxClasses || num_graphs <= 0 || !d_fake || !hard ||
      !logits || !onehot || !type || !far_gen || !far_ref || !out || !workspace)
    return VG_EINVAL;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int nb = vg_blocks(N, kGLThreads) < kGLMaxBlocks ? vg_blocks(N, kGLThreads) : kGLMaxBlocks;
  if (classes <= 8)
    k_gen_loss_partial<8, BCE><<<nb, kGLThreads, 0, s>>>(d_fake, hard, logits, onehot, type, N, classes, workspace);
  else
    k_gen_loss_partial<kMaxClasses, BCE><<<nb, kGLThreads, 0, s>>>(d_fake, hard, logits, onehot, type, N, classes,
                                                                   workspace);
  k_gen_loss_final<BCE><<<1, 1024, 0, s>>>(workspace, nb, N, classes, far_gen, far_ref, num_graphs, l_adv,
                                         l_label, l_ratio, l_void, l_far, out);
  VG_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int vg_gen_loss_fwd(const float* d_fake, const float* hard, const float* logits,
                               const float* onehot, const int64_t* type, int32_t N, int32_t classes,
                               const float* far_gen, const float* far_ref, int32_t num_graphs,
                               float l_adv, float l_label, float l_ratio, float l_void, float l_far,
                               float* out, float* workspace, void* stream) {
  return gen_loss_fwd<false>(d_fake, hard, logits, onehot, type, N, classes, far_gen, far_ref, num_graphs, l_adv,
                             l_label, l_ratio, l_void, l_far, out, workspace, stream);
}

extern "C" int vg_gen_loss_bce_fwd(const float* d_fake, const float* hard, const float* logits,
                                   const float* onehot, const int64_t* type, int32_t N, int32_t classes,
                                   const float* far_gen, const float* far_ref, int32_t num_graphs,
                                   float l_adv, float l_label, float l_ratio, float l_void, float l_far,
                                   float* out, float* workspace, void* stream) {
  return gen_loss_fwd<true>(d_fake, hard, logits, onehot, type, N, classes, far_gen, far_ref, num_graphs, l_adv,
                            l_label, l_ratio, l_void, l_far, out, workspace, stream);
}

extern "C" int vg_gen_loss_bwd(const float* g_loss, const float* out, const float* logits,
                               const int64_t* type, int32_t N, int32_t classes, float* g_dfake,
                               float* g_hard, float* g_logits, void* stream) {
  if (N <= 0 || classes <= 0 || classes > kMaxClasses || !g_loss || !out || (g_logits && (!logits || !type)))
    return VG_EINVAL;
  k_gen_loss_bwd<false><<<vg_blocks(N, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      g_loss, out, nullptr, logits, type, N, classes, g_dfake, g_hard, g_logits);
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_gen_loss_bce_bwd(const float* g_loss, const float* out, const float* d_fake,
                                   const float* logits, const int64_t* type, int32_t N, int32_t classes,
                                   float* g_dfake, float* g_hard, float* g_logits, void* stream) {
  if (N <= 0 || classes <= 0 || classes > kMaxClasses || !g_loss || !out || (g_dfake && !d_fake) ||
      (g_logits && (!logits || !type)))
    return VG_EINVAL;
  k_gen_loss_bwd<true><<<vg_blocks(N, 256), 256, 0, static_cast<hipStream_t>(stream)>>>(
      g_loss, out, d_fake, logits, type, N, classes, g_dfake, g_hard, g_logits);
  VG_CHECK_LAUNCH();
  return 0;
}

// ---- counter-based random draws (device RNG mode) -------------------------
// Four draws per Philox4x32-10 call on the counter (element group, salt,
// *iter): a captured hipGraph reads *iter at replay, so every replay draws
// fresh numbers without torch's generator bookkeeping (two int64 fills per
// graph replay for the registered philox seed / offset).
namespace {
__global__ void k_rng_fill(float* __restrict__ out, long long n, int kind, unsigned long long seed,
                           const long long* __restrict__ iter, unsigned int salt, long long delta) {
  const long long it = *iter + delta;
  const uint2 key = make_uint2(static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
  for (long long g = blockIdx.x * (long long)blockDim.x + threadIdx.x; 4 * g < n;
       g += (long long)gridDim.x * blockDim.x) {
    const uint4 r = vg_philox(make_uint4(static_cast<uint32_t>(g), static_cast<uint32_t>(g >> 32), salt,
                                         static_cast<uint32_t>(it)),
                              key);
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
    float v[4];
    if (kind == 0) {  // standard normal, Box-Muller on (x, y) and (z, w)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const float u1 = (static_cast<float>(w[2 * p] >> 8) + 1.f) * (1.0f / 16777216.0f);  // (0, 1]
        const float u2 = static_cast<float>(w[2 * p + 1] >> 8) * (1.0f / 16777216.0f);
        const float rad = sqrtf(-2.f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        v[2 * p] = rad * cs;
        v[2 * p + 1] = rad * sn;
      }
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float u = static_cast<float>(w[q] >> 8) * (1.0f / 16777216.0f);  // [0, 1)
        // Exp(1) strictly positive: the Gumbel noise g = -log(E) (models.py:150)
        // is +inf at E = 0 and the label softmax NaN.  -log(1 - u) with u = 0
        // hit that once per 2^24 draws -- ~130 training steps at 16 buildings.
        // u' = (x + 0.5) / 2^23 on 23 bits lies in [2^-24, 1 - 2^-24], both
        // exact, so E in [6e-8, 16.6] (torch's GPU exponential_ likewise keeps
        // its log away from 0).
        const float ue = (static_cast<float>(w[q] >> 9) + 0.5f) * (1.0f / 8388608.0f);
        v[q] = kind == 1 ? u : -logf(1.f - ue);  // uniform / Exp(1)
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (4 * g + q < n) out[4 * g + q] = v[q];
  }
}
}  // namespace

extern "C" int vg_rng_fill_at(float* out, int64_t n, int32_t kind, uint64_t seed, const int64_t* iter,
                              int64_t iter_delta, uint32_t salt, void* stream) {
  if (n < 0 || !out || !iter || kind < 0 || kind > 2) return VG_EINVAL;
  if (n == 0) return 0;
  const long long groups = (n + 3) / 4;
  const int blocks = static_cast<int>(groups / 256 + 1 < 2048 ? groups / 256 + 1 : 2048);
  k_rng_fill<<<blocks, 256, 0, static_cast<hipStream_t>(stream)>>>(out, n, kind, (unsigned long long)seed,
                                                                   reinterpret_cast<const long long*>(iter), salt,
                                                                   static_cast<long long>(iter_delta));
  VG_CHECK_LAUNCH();
  return 0;
}

extern "C" int vg_rng_fill(float* out, int64_t n, int32_t kind, uint64_t seed, const int64_t* iter, uint32_t salt,
                           void* stream) {
  return vg_rng_fill_at(out, n, kind, seed, iter, 0, salt, stream);
}
