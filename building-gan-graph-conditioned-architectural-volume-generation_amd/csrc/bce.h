// One row of torch's binary_cross_entropy on a sigmoid output, forward and
// backward, in f32 (shared by the critic head, bce.hip, and the generator's
// BCE loss head, head.hip).
#pragma once
#include <hip/hip_runtime.h>

// s: the pre-sigmoid score; ONE: target 1 (else 0); fn = float(N) of the mean.
//   p = 1 / (1 + exp(-s))                                  (ATen sigmoid)
//   term = -max(log p, -100) | -max(log1p(-p), -100)      (ATen binary_cross_entropy)
//   dL/dp = (p - y) / max((1 - p) p, 1e-12) / N            (its backward, mean reduction)
//   dL/ds = dL/dp (1 - p) p                                (sigmoid backward)
// This is the arithmetic on the probability, not a softplus form: a saturated
// row (p == 0 or 1 in f32) gives the clamped term 100 and gradient 0, and the
// 1e-12 clamp bites for |s| > ~27.6, exactly as in the reference.
// term is ADDED to `acc`; `grad` is dL/ds.
template <bool ONE>
__device__ __forceinline__ void vg_bce_row(float s, float fn, float& acc, float& grad) {
  const float p = 1.f / (1.f + expf(-s));
  const float term = ONE ? -fmaxf(logf(p), -100.f) : -fmaxf(log1pf(-p), -100.f);
  const float q = (1.f - p) * p;
  const float dp = (p - (ONE ? 1.f : 0.f)) / fmaxf(q, 1e-12f) / fn;
  acc += term;
  grad = dp * q;
}
