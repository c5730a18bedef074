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

// ------------------------------------------------------------------------------ fields backward
// The per-sample body and the folds of the fields backward, shared by fields_bwd_kernel (fields.hip)
// and the fused bilinear + fields backward (bilinear.hip): one copy of the arithmetic, so both write
// the same bits.
struct FieldBwdArgs {
  const int64_t* item_id; const int64_t* item_seq; const int64_t* likes; const int64_t* views;
  const float* hmm; const float* ln_g;
  const float* w1; const float* b1; const float* w2;
  const float* X;      // [B][2][D] fields 3, 5 (fields 1, 2, 4 are recomputed)
  const float* cate;   // [n_cate][D] (field 1, 2 recompute)
  const float* ln_b;   // [D] (field 4 recompute)
  const float* a;      // [B][6]
  const float* cnt;    // [B]
  const float* dV;     // [B][5][D] total gradient wrt V_1..V_5
  float* dhmm;         // [B][D] gradient wrt the pre-LN projection, or null: not written (bf16 mode reads dhmm16)
  short* dhmm16;       // optional bf16 copy (operand of the mm_proj weight-gradient GEMM)
  long long dhmm16_lo; // > 0: dhmm16 is split images (hi, lo this many elements further; bf16_fwd)
  float* partials;     // [gridDim.x][P]; P = 6R + R + 6R + 6 + 2D + n_cate*D
  // table gradient, mode 0: dense gtab[V][D] (atomics) if gvec == null; otherwise the two
  // per-sample vectors gvec[b][0] = dX3 (item row), gvec[b][1] = dX5/count (each history row)
  float* gtab; float* gvec;
  double* gnorm;       // optional with gvec: [B][2] sums of squares of the two vectors (clip norm)
  // slot form (fbn_fields_bwd_slot): gvec is the base of the deferred-gradient ring [ring_n][ring_stride];
  // the vectors go to slot *slot_step % ring_n and that slot's address to *slot_cell (FBN_GRAD_CELL readers)
  const int* slot_step; float** slot_cell; long long ring_stride; int ring_n;
  // mode 1: rows written to sendbuf at pos[b][t] (f32); mode 2: the same in bf16 (bf16 mode's wire)
  const int* pos; void* sendbuf;
  long long V;
  int B, L, R, n_cate;
  float ln_eps;
};

// Column-transposed copy of a group's row vector for coalesced atomics: lane q of a G-lane
// group holds columns 4q..4q+3; after the transpose, t[e] is column e*G + q, so atomic
// instruction e of the group covers one contiguous G*4-byte run of the row (full-rate
// global_atomic_add_f32 shape) instead of four 16-B-strided runs.
template <int G>
__device__ __forceinline__ f32x4 transpose_cols(const f32x4& v, int lane) {
  const int base = lane - lane % G, q = lane % G;
  f32x4 t;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int src = base + e * (G / 4) + q / 4;
    const float x0 = __shfl(v[0], src, 64), x1 = __shfl(v[1], src, 64);
    const float x2 = __shfl(v[2], src, 64), x3 = __shfl(v[3], src, 64);
    const int c = q & 3;
    t[e] = c == 0 ? x0 : (c == 1 ? x1 : (c == 2 ? x2 : x3));
  }
  return t;
}
template <int G>
__device__ __forceinline__ void atomic_add_row_t(float* row, const f32x4& t, int q) {
  atomicAdd(row + q, t[0]); atomicAdd(row + G + q, t[1]); atomicAdd(row + 2 * G + q, t[2]);
  atomicAdd(row + 3 * G + q, t[3]);
}

// what a sample's lanes read before any arithmetic: ids, fields 1, 2, 3, 5, the pre-LN projection,
// the SENET weights a and the history count (lane q: columns 4q..4q+3)
struct FieldsBwdIn {
  f32x4 x0, x1, x2, x4, h;
  float a[6];
  float cnt;
  long long lk, vw;
};
template <int D>
__device__ __forceinline__ FieldsBwdIn fields_bwd_load(const FieldBwdArgs& p, int b, int q) {
  FieldsBwdIn in;
  const float* Xb = p.X + (size_t)b * 2 * D + 4 * q;
  in.lk = p.likes[b];
  in.vw = p.views[b];
  // fields 1, 2 as the forward read them (an out-of-range id read row 0 and raised the flag)
  const long long lkc = (in.lk >= 0 && in.lk < p.n_cate) ? in.lk : 0, vwc = (in.vw >= 0 && in.vw < p.n_cate) ? in.vw : 0;
  in.x0 = *reinterpret_cast<const f32x4*>(p.cate + lkc * D + 4 * q);
  in.x1 = *reinterpret_cast<const f32x4*>(p.cate + vwc * D + 4 * q);
  in.x2 = *reinterpret_cast<const f32x4*>(Xb);
  in.x4 = *reinterpret_cast<const f32x4*>(Xb + D);
  in.h = *reinterpret_cast<const f32x4*>(p.hmm + (size_t)b * D + 4 * q);
#pragma unroll
  for (int f = 0; f < 6; ++f) in.a[f] = p.a[(size_t)b * 6 + f];
  in.cnt = p.cnt[b];
  return in;
}

// the parameter gradients a lane accumulates over its samples: LN gain / bias, the mm_proj bias, and
// its SENET entries (entry k of the flattened [w1 | b1 | w2 | b2] in lane k mod G)
template <int D, int RMAX>
struct FieldsBwdAcc {
  static constexpr int SJ = (13 * RMAX + 6 + D / 4 - 1) / (D / 4);
  f32x4 lg, lb, hb;
  float se[SJ];
  __device__ __forceinline__ void zero() {
    lg = lb = hb = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < SJ; ++j) se[j] = 0.f;
  }
};

// One live sample b: SENET + mean + LayerNorm + ReLU backward from dv = dL/dV_1..5 (this lane's
// columns), the table-gradient vectors / rows and dhmm stored, the parameter gradients added to acc.
// dx0 / dx1: the gradients of fields 1, 2 for the cate rows (fields_bwd_cate).  sv: the group's
// SENET staging {ds[6], z[6], dq[RMAX], rj[RMAX]} in LDS.  gvec: p.gvec, or the ring slot of the step.
template <int D, int MODE, int RMAX>
__device__ __forceinline__ void fields_bwd_sample(const FieldBwdArgs& p, float* gvec, int b, int lane,
                                                  const FieldsBwdIn& in, const f32x4 (&dv)[5], float* sv,
                                                  FieldsBwdAcc<D, RMAX>& acc, f32x4& dx0, f32x4& dx1) {
  constexpr int G = D / 4;
  constexpr int SJ = FieldsBwdAcc<D, RMAX>::SJ;
  const int q = lane % G;
  const int R = p.R;
  const int NP = 13 * R + 6;
  const int L = p.L;
  const f32x4 h = in.h;
  f32x4 x[5];
  x[0] = in.x0;
  x[1] = in.x1;
  x[2] = in.x2;
  x[4] = in.x4;
  x[3] = ln_relu<G>(h, p.ln_g, p.ln_b, p.ln_eps, q);
  float a[6];
#pragma unroll
  for (int f = 0; f < 6; ++f) a[f] = in.a[f];
  // recompute squeeze + hidden exactly as the forward did
  float z[6];
  z[0] = 0.f;
#pragma unroll
  for (int f = 0; f < 5; ++f) z[f + 1] = group_sum<G>(x[f][0] + x[f][1] + x[f][2] + x[f][3]) / (float)D;
  float qv[RMAX], rj[RMAX], dq[RMAX];
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    float s = 0.f;
    if (j < R) {
      s = p.b1[j];
#pragma unroll
      for (int f = 0; f < 6; ++f) s += p.w1[j * 6 + f] * z[f];
    }
    qv[j] = s;
    rj[j] = fmaxf(s, 0.f);
  }
  // excitation backward
  float ds[6];
  ds[0] = 0.f;   // da_0 = sum(dV_0 * X_0) = 0 since X_0 == 0
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const float da = group_sum<G>(dv[f][0] * x[f][0] + dv[f][1] * x[f][1] + dv[f][2] * x[f][2] + dv[f][3] * x[f][3]);
    ds[f + 1] = da * (1.f - a[f + 1]) * a[f + 1];
  }
  float dz[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < RMAX; ++j) {
    float dr = 0.f;
    if (j < R) {
#pragma unroll
      for (int f = 0; f < 6; ++f) dr += p.w2[f * R + j] * ds[f];
    }
    dq[j] = (j < R && qv[j] > 0.f) ? dr : 0.f;
    if (j < R) {
#pragma unroll
      for (int f = 0; f < 6; ++f) dz[f] += p.w1[j * 6 + f] * dq[j];
    }
  }
  // SENET parameter-gradient entries (group-uniform): lane q owns entries q, q+G, ... of the
  // flattened [w1 R*6 | b1 R | w2 6*R | b2 6]; the values come through LDS (runtime indices
  // into registers would go to scratch)
  if (q == 0) {
#pragma unroll
    for (int f = 0; f < 6; ++f) { sv[f] = ds[f]; sv[6 + f] = z[f]; }
#pragma unroll
    for (int jj = 0; jj < RMAX; ++jj) { sv[12 + jj] = dq[jj]; sv[12 + RMAX + jj] = rj[jj]; }
  }
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < SJ; ++j) {
    const int k = q + j * G;
    float v = 0.f;
    if (k < 6 * R) v = sv[12 + k / 6] * sv[6 + k % 6];                                  // dq_j * z_f
    else if (k < 7 * R) v = sv[12 + (k - 6 * R)];                                        // dq_j
    else if (k < 13 * R) v = sv[(k - 7 * R) / R] * sv[12 + RMAX + (k - 7 * R) % R];      // ds_f * r_j
    else if (k < NP) v = sv[k - 13 * R];                                                 // ds_f
    acc.se[j] += v;
  }
  __builtin_amdgcn_wave_barrier();
  f32x4 dx[5];
#pragma unroll
  for (int f = 0; f < 5; ++f) dx[f] = dv[f] * a[f + 1] + dz[f + 1] / (float)D;
  dx0 = dx[0];
  dx1 = dx[1];

  // field 4: ReLU + LayerNorm backward -> d(h_mm)
  {
    const float mean = group_sum<G>(h[0] + h[1] + h[2] + h[3]) / (float)D;
    const f32x4 dh = h - mean;
    const float s2 = group_sum<G>(dh[0] * dh[0] + dh[1] * dh[1] + dh[2] * dh[2] + dh[3] * dh[3]);
    const float rstd = 1.f / sqrtf(s2 / (float)D + p.ln_eps);
    const f32x4 gam = *reinterpret_cast<const f32x4*>(p.ln_g + 4 * q);
    f32x4 gl, xh, gx;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      gl[e] = x[3][e] > 0.f ? dx[3][e] : 0.f;
      xh[e] = dh[e] * rstd;
      gx[e] = gl[e] * gam[e];
      acc.lg[e] += gl[e] * xh[e];
      acc.lb[e] += gl[e];
    }
    const float m1 = group_sum<G>(gx[0] + gx[1] + gx[2] + gx[3]) / (float)D;
    const float m2 = group_sum<G>(gx[0] * xh[0] + gx[1] * xh[1] + gx[2] * xh[2] + gx[3] * xh[3]) / (float)D;
    f32x4 out;
#pragma unroll
    for (int e = 0; e < 4; ++e) out[e] = rstd * (gx[e] - m1 - xh[e] * m2);
    if (p.dhmm) *reinterpret_cast<f32x4*>(p.dhmm + (size_t)b * D + 4 * q) = out;
    acc.hb += out;                              // mm_proj.0.bias gradient (sum over the batch)
    if (p.dhmm16) {
      const bf16x4 hi = (bf16x4){f2bf(out[0]), f2bf(out[1]), f2bf(out[2]), f2bf(out[3])};
      *reinterpret_cast<bf16x4*>(p.dhmm16 + (size_t)b * D + 4 * q) = hi;
      if (p.dhmm16_lo)
        *reinterpret_cast<bf16x4*>(p.dhmm16 + p.dhmm16_lo + (size_t)b * D + 4 * q) =
            (bf16x4){f2bf(out[0] - bf2f(hi[0])), f2bf(out[1] - bf2f(hi[1])), f2bf(out[2] - bf2f(hi[2])),
                     f2bf(out[3] - bf2f(hi[3]))};
    }
  }
  // item table: dX3 -> row item_id, dX5 / count -> each non-padding history row
  const f32x4 gh = dx[4] / in.cnt;
  if (MODE == 0 && p.gvec) {
    // sparse mode: plain stores; rows are resolved later through map / slot_row
    *reinterpret_cast<f32x4*>(gvec + (size_t)b * 2 * D + 4 * q) = dx[2];
    *reinterpret_cast<f32x4*>(gvec + ((size_t)b * 2 + 1) * D + 4 * q) = gh;
    if (p.gnorm) {
      double si = 0.0, sh = 0.0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        si += (double)(dx[2][e] * dx[2][e]);
        sh += (double)(gh[e] * gh[e]);
      }
#pragma unroll
      for (int o = G / 2; o > 0; o >>= 1) {
        si += __shfl_xor(si, o, 64);
        sh += __shfl_xor(sh, o, 64);
      }
      if (q == 0) {
        p.gnorm[(size_t)b * 2] = si;
        p.gnorm[(size_t)b * 2 + 1] = sh;
      }
    }
  } else if (MODE == 0) {
    const f32x4 ti = transpose_cols<G>(dx[2], lane);
    const f32x4 th = transpose_cols<G>(gh, lane);
    const long long item = p.item_id[b];
    if (item > 0 && item < p.V) atomic_add_row_t<G>(p.gtab + item * D, ti, q);
    for (int t = 0; t < L; ++t) {
      const long long s = p.item_seq[(size_t)b * L + t];
      if (s > 0 && s < p.V) atomic_add_row_t<G>(p.gtab + s * D, th, q);
    }
  } else {
    const int* pb = p.pos + (size_t)b * (L + 1);
    auto put = [&](int row, const f32x4& x) {
      if constexpr (MODE == 2) {
        *reinterpret_cast<bf16x4*>(reinterpret_cast<short*>(p.sendbuf) + (size_t)row * D + 4 * q) =
            (bf16x4){f2bf(x[0]), f2bf(x[1]), f2bf(x[2]), f2bf(x[3])};
      } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(p.sendbuf) + (size_t)row * D + 4 * q) = x;
      }
    };
    if (pb[0] >= 0) put(pb[0], dx[2]);
    for (int t = 0; t < L; ++t)
      if (pb[t + 1] >= 0) put(pb[t + 1], gh);
  }
}

// cate table (likes, views share one table): the wave's groups take turns on its slice w_ct
template <int D>
__device__ __forceinline__ void fields_bwd_cate(float* w_ct, int n_cate, int lane, bool live, long long lk,
                                                long long vw, const f32x4& dx0, const f32x4& dx1) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int q = lane % G, grp = lane / G;
#pragma unroll
  for (int gi = 0; gi < SPW; ++gi) {
    if (grp == gi && live) {
      if (lk >= 0 && lk < n_cate) {
        f32x4* c = reinterpret_cast<f32x4*>(w_ct + lk * D + 4 * q);
        *c = *c + dx0;
      }
      if (vw >= 0 && vw < n_cate) {
        f32x4* c = reinterpret_cast<f32x4*>(w_ct + vw * D + 4 * q);
        *c = *c + dx1;
      }
    }
  }
}

// After a wave's last sample: fold its groups (lanes q, q+G, ... hold the same entries / columns) into
// group 0 and that into the wave's slice ws of sp (4 slices of P floats, zeroed before the first
// sample); then the block sums its 4 slices into its partial row.  Every thread of the block calls it.
template <int D, int RMAX>
__device__ __forceinline__ void fields_bwd_fold(const FieldBwdArgs& p, float* sp, FieldsBwdAcc<D, RMAX>& acc) {
  constexpr int G = D / 4;
  constexpr int SJ = FieldsBwdAcc<D, RMAX>::SJ;
  const int NP = 13 * p.R + 6;
  const int P = NP + 3 * D + p.n_cate * D;      // ... | cate rows | mm_proj bias (column sums of dhmm)
  const int lane = threadIdx.x & 63, q = lane % G, grp = lane / G;
  float* ws = sp + (threadIdx.x >> 6) * P;
  float* w_lg = ws + NP;
  float* w_hb = w_lg + 2 * D + p.n_cate * D;
#pragma unroll
  for (int o = G; o < 64; o <<= 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc.lg[e] += __shfl_xor(acc.lg[e], o, 64);
      acc.lb[e] += __shfl_xor(acc.lb[e], o, 64);
      acc.hb[e] += __shfl_xor(acc.hb[e], o, 64);
    }
#pragma unroll
    for (int j = 0; j < SJ; ++j) acc.se[j] += __shfl_xor(acc.se[j], o, 64);
  }
  if (grp == 0) {
    *reinterpret_cast<f32x4*>(w_lg + 4 * q) = acc.lg;
    *reinterpret_cast<f32x4*>(w_lg + D + 4 * q) = acc.lb;
    *reinterpret_cast<f32x4*>(w_hb + 4 * q) = acc.hb;
#pragma unroll
    for (int j = 0; j < SJ; ++j) {
      const int k = q + j * G;
      if (k < NP) ws[k] = acc.se[j];
    }
  }
  __syncthreads();
  float* out = p.partials + (size_t)blockIdx.x * P;
  for (int i = threadIdx.x; i < P; i += blockDim.x) out[i] = (sp[i] + sp[P + i]) + (sp[2 * P + i] + sp[3 * P + i]);
}

// blocks of the fields backward (= rows of its partials): 4 waves of 64 / (D/4) samples, capped
#ifndef FBN_FB_MAXBLK
#define FBN_FB_MAXBLK 512    // backward: partial rows to reduce vs samples in flight (tools/time_fields.py)
#endif
static inline int fields_grid(int B, int D, int cap = 1024) {
  const int spw = 64 / (D / 4);
  const int waves = (B + spw - 1) / spw;
  int blocks = (waves + 3) / 4;
  return blocks < 1 ? 1 : (blocks > cap ? cap : blocks);
}
// bytes of LDS of the fields backward: 4 wave slices of P floats + the SENET staging of its 4 * SPW groups
static inline size_t fields_bwd_lds(int D, int R, int n_cate, int rmax) {
  return (4 * (size_t)(13 * R + 6 + 3 * D + n_cate * D) + 4 * (64 / (D / 4)) * (12 + 2 * rmax)) * sizeof(float);
}
// the optional last step of the fields backward entry points: the partial rows summed into the 8
// parameter gradients (fields.hip)
int fbn_fields_reduce_partials(const float* partials, float* const* param_grads, int B, int D, int R, int n_cate,
                               hipStream_t st);
