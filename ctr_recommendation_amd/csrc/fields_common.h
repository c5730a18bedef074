// Device functions shared by the training fields kernels (fields.hip) and the serving kernels
// (recommend.hip): both compile the same operations in the same order, so a field or a SENET
// weight computed by either is the same bits.
#pragma once
#include "common.h"

#define FBN_MAXR 8   // max SENET reduced width supported (reference: 3)
#define FBN_MAX_L 32 // max history length (the reference keeps the last 20)

// field 4 = ReLU(LayerNorm(h)) for this lane's 4 columns; shared by the forward and the
// backward's recompute so both run the same operations (bit-identical)
template <int G>
__device__ __forceinline__ f32x4 ln_relu(const f32x4& h, const float* ln_g, const float* ln_b, float eps, int q) {
  constexpr int D = 4 * G;
  const float s1 = group_sum<G>(h[0] + h[1] + h[2] + h[3]);
  const float mean = s1 / (float)D;
  const f32x4 dh = h - mean;
  const float s2 = group_sum<G>(dh[0] * dh[0] + dh[1] * dh[1] + dh[2] * dh[2] + dh[3] * dh[3]);
  const float rstd = 1.f / sqrtf(s2 / (float)D + eps);
  const f32x4 g4 = *reinterpret_cast<const f32x4*>(ln_g + 4 * q);
  const f32x4 bb4 = *reinterpret_cast<const f32x4*>(ln_b + 4 * q);
  f32x4 x4;
#pragma unroll
  for (int e = 0; e < 4; ++e) x4[e] = fmaxf(dh[e] * rstd * g4[e] + bb4[e], 0.f);
  return x4;
}

template <int D>
__device__ __forceinline__ void senet_excite(const float (&z)[6], const float* w1, const float* b1,
                                             const float* w2, const float* b2, int R, float (&q)[FBN_MAXR],
                                             float (&a)[6]) {
  for (int j = 0; j < R; ++j) {
    float s = b1[j];
#pragma unroll
    for (int f = 0; f < 6; ++f) s += w1[j * 6 + f] * z[f];
    q[j] = s;
  }
#pragma unroll
  for (int f = 0; f < 6; ++f) {
    float s = b2[f];
    for (int j = 0; j < R; ++j) s += w2[f * R + j] * fmaxf(q[j], 0.f);
    a[f] = 1.f / (1.f + __expf(-s));
  }
}
