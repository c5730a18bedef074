// K8 / K9: global-norm gradient clipping + Adam (coupled L2) for the FiBiNET trainer.
//
// Semantics of train_fibinet.py:78,119,121-122 with torch's single-tensor Adam:
//   g  <- g * min(1, max_norm / (||g||_2 + 1e-6))          (clip_grad_norm_, all params)
//   g  <- g + wd * p                                        (coupled weight decay)
//   m  <- m + (1-b1) * (g - m)                              (lerp, weight < 0.5 branch)
//   v  <- v * b2 + ((1-b2) * g) * g                         (mul_ + addcmul_)
//   p  <- p + (-lr/bc1 * m) / (sqrt(v) / sqrt(bc2) + eps)   (addcdiv_)
// The per-step scalars (1-b1, -lr/bc1, sqrt(bc2)) come from a host-built schedule table
// (OneCycleLR with beta1 cycling, double precision like torch) indexed by a device-resident
// step counter, so a whole training step can be captured in a hipGraph and replayed.
//
// Table parameter: the gradient of E is non-zero only on the rows the batch touched.  The
// dense pass reads w, m, v (24 B/element, the HBM floor for exact dense-Adam semantics) and
// the gradient only through the row->slot map (4 B/row); untouched rows get g = 0 + wd*p.
// The map entries of touched rows are reset in the same pass.
#include "common.h"
#include "convert.h"
#include <cstdlib>
#include <algorithm>

#pragma clang fp contract(off)

// squared-norm accumulators: FBN_SUMSQ_SLOTS doubles, block b adds into slot b % SLOTS (one
// address per block would serialise the returning-free f64 atomics of thousands of blocks)

struct AdamConsts {
  float w1;     // 1 - beta1 (as float)
  float nss;    // -lr / bias_correction1 (as float)
  float bc2s;   // sqrt(bias_correction2) (as float)
  float rbc2s;  // 1 / sqrt(bias_correction2) (as float; the table-row step multiplies by it)
  float dmul;   // AdamW's decoupled decay factor 1 - lr * weight_decay (1 for Adam: p * 1 == p exactly)
  float pad0, pad1, pad2;
};

// ------------------------------------------------------------------ squared norm partials
// out slot += sum x^2 over n elements (double atomics on one slot per call; few blocks)
__global__ void sumsq_kernel(const float* __restrict__ x, long long n, const int* __restrict__ n_rows, int row_len,
                             double* __restrict__ out) {
  __shared__ double red[256];
  long long lim = n_rows ? (long long)(*n_rows) * row_len : n;
  double s = 0.0;
  const long long n4 = lim / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
    s += (double)(v[0] * v[0]) + (double)(v[1] * v[1]) + (double)(v[2] * v[2]) + (double)(v[3] * v[3]);
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < lim; i += (long long)gridDim.x * blockDim.x)
    s += (double)(x[i] * x[i]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out + (blockIdx.x & (FBN_SUMSQ_SLOTS - 1)), red[0]);
}

// coef = min(1, max_norm / (sqrt(total) + 1e-6)); also exposes the norm
__global__ void clip_coef_kernel(const double* sumsq, float max_norm, float* coef_out, float* norm_out) {
  double s = 0.0;
  for (int i = 0; i < FBN_SUMSQ_SLOTS; ++i) s += sumsq[i];
  const float total = sqrtf((float)s);
  float c = max_norm / (total + 1e-6f);
  coef_out[0] = c < 1.f ? c : 1.f;
  if (norm_out) norm_out[0] = total;
}

__device__ __forceinline__ float adam_elem(float& p, float& m, float& v, float g, float coef, float wd, float b2,
                                           float omb2, float eps, const AdamConsts& k) {
  g = g * coef;
  g = g + wd * p;
  p = p * k.dmul;   // AdamW: param.mul_(1 - lr * wd) (torch.optim.AdamW); Adam: dmul == 1, exact
  m = m + k.w1 * (g - m);
  v = v * b2;
  v = v + (omb2 * g) * g;
  const float denom = sqrtf(v) / k.bc2s + eps;
  p = p + (k.nss * m) / denom;
  return p;
}

// ------------------------------------------------------------------ table-row Adam step
// item_emb.weight is updated with the same operations as adam_elem except that the square root and
// the division use the hardware v_sqrt_f32 / v_rcp_f32 (about 1 ulp each) and the moment updates
// use fused multiply-adds:
//   g = g*coef + wd*p;  m = fma(w1, g - m, m);  v = fma((1-b2)*g, g, v*b2)
//   p = fma(nss*m, rcp(fma(sqrt(v), 1/sqrt(bc2), eps)), p)
// 13 VALU issue-slot equivalents per element instead of ~50 for IEEE division + correctly rounded
// sqrt.  Every table kernel (eager pass, lazy replay, touched / deferred commit, flush) uses this one
// function, so the lazy replay stays bit-identical to eager dense Adam; the deviation from the IEEE
// step is bounded by fbn_adam_selftest (a few ulp of the update, far inside the parity tolerance).
// The dense parameters use the same step (adam_dense_body).  What anchors it to torch is
// tests/test_gpu_adam.py: every kernel that calls it, one launch at a time, against a float64
// torch-semantics step under bounds derived from the roundings above (tests/_adam_ref.py).
// adam_elem, the same update unfused in torch's operation order, is only fbn_adam_selftest's
// comparison arm: no production kernel calls it.
// rbc2s = 1/sqrt(bc2) from the host schedule table (column 4, computed in double).
typedef float f32x2 __attribute__((ext_vector_type(2)));

// DW: apply AdamW's decoupled decay p *= dmul (opt-in); the zero-gradient replay of the Adam path
// instantiates DW = false and skips the multiply -- bit-identical, as p * 1 == p.
template <bool DW>
__device__ __forceinline__ float adam_tab1(float p, float& m, float& v, float g, float wd, float b2, float omb2,
                                           float eps, const AdamConsts& k) {
#ifdef FBN_ADAM_IEEE
  // A/B build only (build.build_variant("ieee")): unfused, correctly rounded sqrt and division --
  // the parity bisection's IEEE arm (profiles/r05_auc_bisect.json); adam_tabk has the same form
  g = g + wd * p;
  if (DW) p = p * k.dmul;
  m = m + k.w1 * (g - m);
  v = v * b2 + (omb2 * g) * g;
  return p + (k.nss * m) / (sqrtf(v) * k.rbc2s + eps);
#endif
  g = __builtin_fmaf(wd, p, g);
  if (DW) p = p * k.dmul;
  m = __builtin_fmaf(k.w1, g - m, m);
  v = __builtin_fmaf(omb2 * g, g, v * b2);
  const float den = __builtin_fmaf(__builtin_amdgcn_sqrtf(v), k.rbc2s, eps);
  return __builtin_fmaf(k.nss * m, __builtin_amdgcn_rcpf(den), p);
}
// four elements; gg already scaled by the clip coefficient (zero for a zero-gradient step)
template <bool DW>
__device__ __forceinline__ void adam_tab4(f32x4& pp, f32x4& mm, f32x4& vv, f32x4 gg, float wd, float b2, float omb2,
                                          float eps, const AdamConsts& k) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    float me = mm[e], ve = vv[e];
    pp[e] = adam_tab1<DW>(pp[e], me, ve, gg[e], wd, b2, omb2, eps, k);
    mm[e] = me;
    vv[e] = ve;
  }
}
template <bool DW>
__device__ __forceinline__ void adam_zero_tab4(f32x4& pp, f32x4& mm, f32x4& vv, float wd, float b2, float omb2,
                                               float eps, const AdamConsts& k) {
  adam_tab4<DW>(pp, mm, vv, (f32x4){0.f, 0.f, 0.f, 0.f}, wd, b2, omb2, eps, k);
}

// clip coefficient of clip_grad_norm_ from the sumsq slots (same sequential order as
// clip_coef_kernel, so the value is bit-identical)
__device__ __forceinline__ float clip_from_slots(const double* sumsq, float max_norm, float* total_out) {
  double s = 0.0;
  for (int i = 0; i < FBN_SUMSQ_SLOTS; ++i) s += sumsq[i];
  const float total = sqrtf((float)s);
  const float c = max_norm / (total + 1e-6f);
  *total_out = total;
  return c < 1.f ? c : 1.f;
}

// sumsq != null: the clip coefficient is computed here (every block, thread 0) and block 0
// publishes it (coef_out, norm_out) for the table passes that follow -- no clip_coef launch.
// dense Adam over elements [0, n) by `nblk` blocks (block index `bid`)
__device__ __forceinline__ void adam_dense_body(float* __restrict__ p, const float* __restrict__ g,
                                                float* __restrict__ m, float* __restrict__ v, long long n, float coef,
                                                const AdamConsts& k, float wd, float b2, float omb2, float eps,
                                                long long bid, long long nblk) {
  const long long n4 = n / 4;
  const long long st = nblk * blockDim.x;
  // four vectors per thread per round, every load of the round in flight before the first
  // update (the pass is latency-bound otherwise: a few blocks per CU, one round trip per vector)
  for (long long i0 = bid * blockDim.x + threadIdx.x; i0 < n4; i0 += 4 * st) {
    f32x4 pp[4], mm[4], vv[4], gg[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * st < n4 ? i0 + u * st : i0;
      pp[u] = *reinterpret_cast<f32x4*>(p + 4 * i);
      mm[u] = *reinterpret_cast<f32x4*>(m + 4 * i);
      vv[u] = *reinterpret_cast<f32x4*>(v + 4 * i);
      gg[u] = *reinterpret_cast<const f32x4*>(g + 4 * i);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const long long i = i0 + u * st;
      if (i >= n4) break;
      adam_tab4<true>(pp[u], mm[u], vv[u], gg[u] * coef, wd, b2, omb2, eps, k);
      *reinterpret_cast<f32x4*>(p + 4 * i) = pp[u];
      *reinterpret_cast<f32x4*>(m + 4 * i) = mm[u];
      *reinterpret_cast<f32x4*>(v + 4 * i) = vv[u];
    }
  }
  for (long long i = n4 * 4 + bid * blockDim.x + threadIdx.x; i < n; i += nblk * blockDim.x) {
    float mm = m[i], vv = v[i];
    p[i] = adam_tab1<true>(p[i], mm, vv, g[i] * coef, wd, b2, omb2, eps, k);
    m[i] = mm; v[i] = vv;
  }
}

__global__ void adam_dense_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                  float* __restrict__ v, long long n, const float* __restrict__ coef_ptr,
                                  const AdamConsts* __restrict__ table, const int* __restrict__ step_ptr, float wd,
                                  float b2, float omb2, float eps, const double* __restrict__ sumsq, float max_norm,
                                  float* coef_out, float* norm_out) {
  const AdamConsts k = table[*step_ptr];
  float coef;
  if (sumsq) {
    __shared__ float sc;
    if (threadIdx.x == 0) {
      float total;
      sc = clip_from_slots(sumsq, max_norm, &total);
      if (blockIdx.x == 0) {
        if (coef_out) *coef_out = sc;
        if (norm_out) *norm_out = total;
      }
    }
    __syncthreads();
    coef = sc;
  } else {
    coef = coef_ptr ? *coef_ptr : 1.f;
  }
  adam_dense_body(p, g, m, v, n, coef, k, wd, b2, omb2, eps, blockIdx.x, gridDim.x);
}

// ------------------------------------------------------------------ sparse table gradient
// Slots are entry indices.  Single GPU: entry e = b*(L+1)+t (t = 0 item, t >= 1 history), its
// gradient vector is gvec[b][t ? 1 : 0] (the backward stores 2 vectors per sample); a row hit
// by several entries keeps them in `extra` (slot of the claiming entry; FLAG in slot_row).
// Multi-GPU owner: entry = received row i, its gradient is rows[i] (Lp1 = 1), duplicates are
// added into the claimer's own row.
#define FBN_SLOT_FLAG 0x40000000
// Lp1 | FBN_GRAD_FULL (deterministic mode): extra[e] of a flagged claimer holds the row's FULL
// gradient (fbn_sparse_fold_fx), not the sum of its duplicates
// Lp1 | FBN_GRAD_CELL: `vec` is the address of a device cell holding the row pointer (fbn_ring_slot:
// the owner's received gradient rows in deferred-gradient ring slot step % ring_n, a slot chosen on
// the device, so a recorded step program needs no host-side ring index)
// Lp1 | FBN_GRAD_BF16 (Lp1 == 1 only): the per-entry rows are bf16 (the sharded owner's bf16 deferred-
// gradient ring: the bf16 mode's wire rows kept as they arrived; widened on every read)
// ring_n | FBN_RING_BF16 (PendSrc, fbn_owner_fold): the deferred-gradient ring holds bf16 rows
#define FBN_FOLD_CHUNKS 1     // sparse_fixup_dup_kernel: 64-entry chunks per wave
#define FBN_FOLD_THREADS 1024 // sparse_fixup_dup_kernel: 16 waves share one LDS table
struct GradSrc {
  const float* vec;     // Lp1 > 1: [B][2][D] per-sample vectors;  Lp1 == 1: [n][D] per-entry rows
  float* extra;         // [n][D] duplicate accumulation (single GPU) or null
  int* slot_row;        // [n] claimed row | FLAG, or -1
  int Lp1;
  int full;             // extra of a flagged claimer = the whole row gradient
  int cell;             // vec holds the address of a device cell with the row pointer (FBN_GRAD_CELL)
  int bf16;             // per-entry rows stored as bf16 (FBN_GRAD_BF16; Lp1 == 1)
};
static inline GradSrc make_src(const float* vec, float* extra, int* slot_row, int lp1_flags) {
  return GradSrc{vec, extra, slot_row, lp1_flags & 0xffff, (lp1_flags & FBN_GRAD_FULL) ? 1 : 0,
                 (lp1_flags & FBN_GRAD_CELL) ? 1 : 0, (lp1_flags & FBN_GRAD_BF16) ? 1 : 0};
}
__device__ __forceinline__ f32x4 widen_bf16x4(bf16x4 h) {
  f32x4 x;
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = __uint_as_float((unsigned)(unsigned short)h[k] << 16);
  return x;
}
// a kernel's first step with a GradSrc: FBN_GRAD_CELL's pointer read from its cell
__device__ __forceinline__ void resolve_src(GradSrc& s) {
  if (s.cell) s.vec = *reinterpret_cast<const float* const*>(s.vec);
}

template <int D>
__device__ __forceinline__ const float* grad_base(const GradSrc& s, int e) {
  if (s.Lp1 == 1) return s.vec + (size_t)e * D;
  const int b = e / s.Lp1, t = e - b * s.Lp1;
  return s.vec + ((size_t)b * 2 + (t ? 1 : 0)) * D;
}
// elements [c, c + 4) of entry e's gradient, f32 (a bf16 per-entry row widened; branch-free as
// ring_load: a bf16 row is read 16 B wide from its bf16 address, the ring padded for the last row)
template <int D>
__device__ __forceinline__ f32x4 grad4(const GradSrc& s, int e, int c) {
  const char* a = s.bf16 ? reinterpret_cast<const char*>(s.vec) + 2 * ((size_t)e * D + c)
                         : reinterpret_cast<const char*>(grad_base<D>(s, e) + c);
  const f32x4 raw = *reinterpret_cast<const f32x4*>(a);
  f32x4 x;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const unsigned w = __float_as_uint(raw[k >> 1]);
    x[k] = s.bf16 ? __uint_as_float((k & 1) ? (w & 0xffff0000u) : (w << 16)) : raw[k];
  }
  return x;
}

// duplicates of a claimed row: single GPU -> extra[claimer] += vec(e) (and flag the claimer);
// owner mode -> rows[claimer] += rows[e].  One G-lane group per entry, contiguous atomics.
template <int D>
__global__ void __launch_bounds__(256) sparse_fixup_kernel(const int64_t* __restrict__ item,
                                                           const int64_t* __restrict__ seq, const int* __restrict__ ids,
                                                           int n, int L, long long V, int rank,
                                                           const int* __restrict__ map, GradSrc s) {
  resolve_src(s);
  constexpr int G = D / 4, RPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long e0 = gw * RPW; e0 < n; e0 += nw * RPW) {
    const long long e = e0 + lane / G;
    if (e >= n) continue;
    long long r;
    if (ids) {
      r = ids[e];
      if (r < 0 || (rank == 0 && r == 0)) continue;   // r < 0: a fixed-capacity block's empty slot
    } else {
      const long long b = e / (L + 1), t = e - b * (L + 1);
      r = t == 0 ? item[b] : seq[b * L + (t - 1)];
      if (r <= 0 || r >= V) continue;
    }
    const int u = map[r];
    if (u == (int)e || u < 0) continue;
    const float* src = grad_base<D>(s, (int)e);
    float* dst;
    if (s.extra) {
      if (q == 0) atomicOr(&s.slot_row[u], FBN_SLOT_FLAG);
      dst = s.extra + (size_t)u * D;
    } else {
      dst = const_cast<float*>(s.vec) + (size_t)u * D;   // (the resolved pointer under FBN_GRAD_CELL)
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) atomicAdd(dst + k * G + q, src[k * G + q]);
  }
}

// Row claiming for the sparse gradient (single GPU): entry e = b*(L+1)+t claims row r if it is
// the first to touch it.  Run as the first kernel of a step so the untouched-row Adam can start
// on the side stream before the forward's GEMMs.
// dup (optional): dup[e] = the entry that claimed e's row when that is not e itself, else -1
// (a claim never changes within a step, so the value a failed claim observes is final); the
// fix-up then reads dup coalesced instead of re-resolving every id through the map.
__global__ void claim_rows_kernel(const int64_t* __restrict__ item, const int64_t* __restrict__ seq, int B, int L,
                                  long long V, int* __restrict__ map, int* __restrict__ slot_row, int* __restrict__ dup,
                                  int* __restrict__ hasdup) {
  const long long n = (long long)B * (L + 1);
  for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
    const long long b = e / (L + 1), t = e - b * (L + 1);
    const long long r = t == 0 ? item[b] : seq[b * L + (t - 1)];
    int owner = -1;
    if (r > 0 && r < V) {
      owner = __hip_atomic_load(map + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (owner == -1) {
        int expected = -1;
        if (__hip_atomic_compare_exchange_strong(map + r, &expected, (int)e, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
          slot_row[e] = (int)r;
        else
          owner = expected;
      }
    }
    if (dup) dup[e] = owner;
    if (hasdup && owner >= 0) hasdup[owner] = 1;   // benign race: every writer stores 1
  }
}

// duplicates resolved at claim time (single GPU): extra[dup[e]] += vec(e), claimer flagged.
// One entry per lane.  Popular rows (Zipf ids: the hottest row can take ~9 % of a batch's
// entries) must not take one row of atomics per duplicate -- same-address atomics serialise at
// the memory side -- so duplicates are summed on chip first, in two levels:
//  * wave: a wave's 64 entries span a few samples, each with just two gradient vectors (item
//    slot, history slots); the wave loads those vectors once, together, and a claimer's sum is
//    (number of its lanes on each vector) x vector;
//  * block: a claimer with several lanes in a chunk (a popular row) adds its chunk sum into a small
//    LDS table keyed by claimer (LDS float atomics, at most 4 probes); the table is flushed with
//    ONE row of global atomics and ONE flag per (block, claimer).  Single duplicates, and
//    claimers that find no slot, add straight to global memory.
template <int D>
__global__ void __launch_bounds__(FBN_FOLD_THREADS) sparse_fixup_dup_kernel(const int* __restrict__ dup, int n, GradSrc s) {
  resolve_src(s);
  constexpr int NPL = D / 64 > 0 ? D / 64 : 1;   // floats per lane of a row
  constexpr int MAXV = 16;                        // distinct vectors of a wave chunk (2 per sample)
  constexpr int CPW = FBN_FOLD_CHUNKS;            // 64-entry chunks per wave
  constexpr int NS = D >= 256 ? 32 : 64;          // LDS slots (NS x D floats)
  __shared__ int skey[NS];
  __shared__ float sacc[NS * D];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < NS; i += blockDim.x) skey[i] = -1;
  for (int i = tid; i < NS * D; i += blockDim.x) sacc[i] = 0.f;
  __syncthreads();
  const int Lp1 = s.Lp1;
  const long long base = (long long)blockIdx.x * blockDim.x * CPW;
  int uu[CPW];
#pragma unroll
  for (int c = 0; c < CPW; ++c) {
    const long long e = base + ((long long)(wave * CPW + c) << 6) + lane;
    uu[c] = e < n ? dup[e] : -1;
  }
  // wave-uniform ue; hot: the claimer has several lanes in this chunk (a popular row) -> LDS table
  // (at most 4 probes), else one row of global atomics
  auto add_row = [&](int ue, const float (&acc)[NPL], bool hot) {
    int slot = -1;
    if (hot && lane == 0) {
      for (int k = 0, h = (int)(((unsigned)ue * 2654435761u) >> 20) & (NS - 1); k < 4; ++k, h = (h + 1) & (NS - 1)) {
        int cur = __hip_atomic_load(skey + h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == -1) {
          int expected = -1;
          if (__hip_atomic_compare_exchange_strong(skey + h, &expected, ue, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_WORKGROUP)) {
            slot = h;
            break;
          }
          cur = expected;
        }
        if (cur == ue) {
          slot = h;
          break;
        }
      }
    }
    slot = __shfl(slot, 0, 64);
    if (slot >= 0) {
#pragma unroll
      for (int k = 0; k < NPL; ++k)
        if (D >= 64 || lane < D) atomicAdd(sacc + slot * D + (D >= 64 ? k * 64 : 0) + lane, acc[k]);
    } else {
      float* dst = s.extra + (size_t)ue * D;
      if (lane == 0) atomicOr(&s.slot_row[ue], FBN_SLOT_FLAG);
#pragma unroll
      for (int k = 0; k < NPL; ++k)
        if (D >= 64 || lane < D) atomicAdd(dst + (D >= 64 ? k * 64 : 0) + lane, acc[k]);
    }
  };
#pragma unroll 1
  for (int c = 0; c < CPW; ++c) {
    const long long e0 = base + ((long long)(wave * CPW + c) << 6);
    const long long e = e0 + lane;
    const int u = uu[c];
    unsigned long long act = __ballot(u >= 0);
    if (!act) continue;
    const long long bs = e0 / Lp1, blast = (min((long long)n, e0 + 64) - 1) / Lp1;
    const int nv = 2 * (int)(blast - bs + 1);
    if (Lp1 >= 2 && nv <= MAXV) {
      int vid = -1;
      if (u >= 0) {
        const long long b = e / Lp1, t = e - b * Lp1;
        vid = 2 * (int)(b - bs) + (t ? 1 : 0);
      }
      float vec[MAXV][NPL];
      unsigned long long vm[MAXV];
#pragma unroll
      for (int v = 0; v < MAXV; ++v) {
        vm[v] = __ballot(vid == v);
        const float* src = s.vec + ((size_t)bs * 2 + (v < nv ? v : 0)) * D;   // branch-free: all loads in flight
#pragma unroll
        for (int k = 0; k < NPL; ++k)
          vec[v][k] = (D >= 64 || lane < D) ? src[(D >= 64 ? k * 64 : 0) + (lane & (D - 1))] : 0.f;
      }
      while (act) {
        const int l = __ffsll((long long)act) - 1;
        const int ue = __shfl(u, l, 64);
        const unsigned long long m = __ballot(u == ue) & act;
        act &= ~m;
        float acc[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) acc[k] = 0.f;
#pragma unroll
        for (int v = 0; v < MAXV; ++v) {
          const float cnt = (float)__popcll(m & vm[v]);
#pragma unroll
          for (int k = 0; k < NPL; ++k) acc[k] = __builtin_fmaf(cnt, vec[v][k], acc[k]);
        }
        add_row(ue, acc, __popcll(m) > 1);
      }
    } else {   // per-entry rows or very short histories: one duplicate at a time
      while (act) {
        const int l = __ffsll((long long)act) - 1;
        act &= act - 1;
        const int ue = __shfl(u, l, 64);
        const float* src = grad_base<D>(s, (int)(e0 + l));
        float acc[NPL];
#pragma unroll
        for (int k = 0; k < NPL; ++k) acc[k] = (D >= 64 || lane < D) ? src[(D >= 64 ? k * 64 : 0) + (lane & (D - 1))] : 0.f;
        add_row(ue, acc, false);
      }
    }
  }
  __syncthreads();
  for (int slot = wave; slot < NS; slot += blockDim.x >> 6) {
    const int ue = skey[slot];
    if (ue < 0) continue;
    if (lane == 0) atomicOr(&s.slot_row[ue], FBN_SLOT_FLAG);
    float* dst = s.extra + (size_t)ue * D;
    for (int k = lane; k < D; k += 64) atomicAdd(dst + k, sacc[slot * D + k]);
  }
}

// Deterministic duplicate fold (single GPU, deterministic mode).  Every entry of a row that
// several entries hit -- its claimer included -- adds its vector into the claimer's int64
// fixed-point accumulator acc[claimer] (scale 2^FBN_FX_SHIFT): integer addition is associative, so
// the row's total depends neither on the order the atomics land in nor on which entry won the
// claim.  The claimer flags itself (only it writes its own slot_row) and clears hasdup.
// fbn_sumsq_sparse_norms(acc) then turns each total into extra[claimer] (float, the FULL row
// gradient) and resets acc.  |element| < 2^23, resolution 2^-40 (9e-13).
#define FBN_FX_SHIFT 40
__device__ __forceinline__ long long to_fx(float x) { return __double2ll_rn((double)x * 1099511627776.0); }
template <int D>
__global__ void __launch_bounds__(256) sparse_fold_fx_kernel(const int* __restrict__ dup, int* __restrict__ hasdup,
                                                             int n, GradSrc s, unsigned long long* __restrict__ acc) {
  resolve_src(s);
  const int lane = threadIdx.x & 63;
  for (long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane; e0 < n;
       e0 += (long long)gridDim.x * blockDim.x) {
    const long long e = e0 + lane;
    int u = -1;
    if (e < n) {
      u = dup[e];
      if (u < 0 && hasdup[e]) {          // a claimer whose row other entries hit
        u = (int)e;
        hasdup[e] = 0;
        s.slot_row[e] |= FBN_SLOT_FLAG;
      }
    }
    unsigned long long mask = __ballot(u >= 0);
    while (mask) {
      const int l = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const int ue = __shfl(u, l, 64);
      const float* src = grad_base<D>(s, (int)(e0 + l));
      unsigned long long* dst = acc + (size_t)ue * D;
      for (int k = lane; k < D; k += 64) atomicAdd(dst + k, (unsigned long long)to_fx(src[k]));
    }
  }
}

// sum of squares of the table gradient from per-sample vector norms (fbn_fields_bwd's gnorm
// [B][2]): a claiming entry without duplicates adds its vector's norm; one with duplicates
// (FLAG, rare) sums vector + extra explicitly, cooperatively across the wave.  One entry per lane.
template <int D>
__global__ void __launch_bounds__(256) sumsq_norms_kernel(GradSrc s, const double* __restrict__ gnorm, int n,
                                                          double* __restrict__ out, unsigned long long* __restrict__ fx,
                                                          const float* __restrict__ dense, long long n_dense) {
  resolve_src(s);
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  double acc = 0.0;
  // the dense gradients' squares too (fbn_sumsq's work, one launch fewer): n_dense % 4 == 0
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_dense / 4;
       i += (long long)gridDim.x * blockDim.x) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(dense + 4 * i);
    acc += (double)(v[0] * v[0]) + (double)(v[1] * v[1]) + (double)(v[2] * v[2]) + (double)(v[3] * v[3]);
  }
  for (long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) - lane; e0 < n;
       e0 += (long long)gridDim.x * blockDim.x) {
    const long long e = e0 + lane;
    const int sr = e < n ? s.slot_row[e] : -1;
    const bool flag = sr != -1 && (sr & FBN_SLOT_FLAG);
    if (sr != -1 && !flag) {
      const int b = (int)(e / s.Lp1), t = (int)(e - (long long)b * s.Lp1);
      acc += gnorm[(size_t)b * 2 + (t ? 1 : 0)];
    }
    unsigned long long mask = __ballot(flag);
    if (fx) {
      while (mask) {
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        float* x = s.extra + (size_t)(e0 + l) * D;
        // deterministic fold: the full row gradient from the fixed-point total
        unsigned long long* a = fx + (size_t)(e0 + l) * D;
        for (int k = lane; k < D; k += 64) {
          const float y = (float)((double)(long long)a[k] * (1.0 / 1099511627776.0));
          x[k] = y;
          a[k] = 0ull;
          acc += (double)(y * y);
        }
      }
    } else {
      // the wave's flagged claimers RPR at a time, D/8 lanes per row (8 elements each): a wave
      // with up to RPR of them pays one round trip, not one per claimer
      constexpr int LPR = D / 8, RPR = 64 / LPR;
      while (mask) {
        int mine = -1;
#pragma unroll
        for (int gi = 0; gi < RPR; ++gi) {
          if (!mask) break;
          const int l = __ffsll((long long)mask) - 1;
          mask &= mask - 1;
          if (lane / LPR == gi) mine = l;
        }
        if (mine < 0) continue;
        const int c = (lane % LPR) * 8;
        const float* v = grad_base<D>(s, (int)(e0 + mine)) + c;
        const float* x = s.extra + (size_t)(e0 + mine) * D + c;
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(v), v1 = *reinterpret_cast<const f32x4*>(v + 4);
        const f32x4 x0 = *reinterpret_cast<const f32x4*>(x), x1 = *reinterpret_cast<const f32x4*>(x + 4);
        const f32x4 y0 = v0 + x0, y1 = v1 + x1;
#pragma unroll
        for (int k = 0; k < 4; ++k) acc += (double)(y0[k] * y0[k]) + (double)(y1[k] * y1[k]);
      }
    }
  }
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) atomicAdd(out + (blockIdx.x & (FBN_SUMSQ_SLOTS - 1)), (red[0] + red[1]) + (red[2] + red[3]));
}

// sum of squares of the clipped-to-be table gradient, over claiming entries only
template <int D>
__global__ void __launch_bounds__(256) sumsq_sparse_kernel(GradSrc s, int n, double* __restrict__ out) {
  resolve_src(s);
  constexpr int G = D / 4, RPW = 64 / G;
  __shared__ double red[256];
  const int lane = threadIdx.x & 63, q = lane % G;
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  double acc = 0.0;
  // two entries per group and round, each row loaded beside its slot_row (the row address does
  // not depend on it: one round trip per round instead of two dependent ones per entry)
  for (long long e0 = gw * RPW * 2; e0 < n; e0 += nw * RPW * 2) {
    const long long ea = e0 + lane / G, eb = ea + RPW;
    const bool oka = ea < n, okb = eb < n;
    const int sra = oka ? s.slot_row[ea] : -1, srb = okb ? s.slot_row[eb] : -1;
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    f32x4 va = oka ? grad4<D>(s, (int)ea, 4 * q) : z;
    f32x4 vb = okb ? grad4<D>(s, (int)eb, 4 * q) : z;
    if (sra != -1 && (sra & FBN_SLOT_FLAG)) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(s.extra + (size_t)ea * D + 4 * q);
      va = s.full ? x : va + x;
    }
    if (srb != -1 && (srb & FBN_SLOT_FLAG)) {
      const f32x4 x = *reinterpret_cast<const f32x4*>(s.extra + (size_t)eb * D + 4 * q);
      vb = s.full ? x : vb + x;
    }
    if (sra != -1)
      acc += (double)(va[0] * va[0]) + (double)(va[1] * va[1]) + (double)(va[2] * va[2]) + (double)(va[3] * va[3]);
    if (srb != -1)
      acc += (double)(vb[0] * vb[0]) + (double)(vb[1] * vb[1]) + (double)(vb[2] * vb[2]) + (double)(vb[3] * vb[3]);
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(out + (blockIdx.x & (FBN_SUMSQ_SLOTS - 1)), red[0]);
}

// One group of D/4 lanes per row; rows_per_wave = 256/D.  map[r] = claiming entry or -1.
// UNTOUCHED_ONLY: update only rows the batch did not touch (map[r] == -1).  Their gradient is
// exactly 0, so the update (g = 0*coef + wd*p) does not depend on the backward or the clip
// coefficient and runs on a side stream concurrently with the whole backward; the touched
// rows are updated afterwards by adam_touched_kernel.  Otherwise: every row, reading the
// gradient of touched rows through the map.
template <int D, bool UNTOUCHED_ONLY>
__device__ __forceinline__ void adam_table_body(float* __restrict__ p, float* __restrict__ m,
                                                         float* __restrict__ v, long long nrows, int* __restrict__ map,
                                                         GradSrc gs, const float* __restrict__ coef_ptr,
                                                         const AdamConsts* __restrict__ table,
                                                         const int* __restrict__ step_ptr, float wd, float b2, float omb2,
                                                         float eps) {
  resolve_src(gs);
  constexpr int G = D / 4;
  constexpr int RPW = 64 / G;
  const AdamConsts k = table[*step_ptr];
  const float coef = coef_ptr ? *coef_ptr : 1.f;
  const int lane = threadIdx.x & 63, q = lane % G;
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long r0 = gw * RPW; r0 < nrows; r0 += nw * RPW) {
    const long long r = r0 + lane / G;
    if (r >= nrows) continue;
    const int u = map[r];
    if (UNTOUCHED_ONLY && u >= 0) continue;
    const size_t off = (size_t)r * D + 4 * q;
    f32x4 pp = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + off));
    f32x4 mm = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m + off));
    f32x4 vv = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v + off));
    f32x4 gg = {0.f, 0.f, 0.f, 0.f};
    if (!UNTOUCHED_ONLY && u >= 0) {
      gg = grad4<D>(gs, u, 4 * q);
      if (gs.extra && (gs.slot_row[u] & FBN_SLOT_FLAG)) {
        float* ex = gs.extra + (size_t)u * D + 4 * q;
        gg = gs.full ? *reinterpret_cast<const f32x4*>(ex) : gg + *reinterpret_cast<const f32x4*>(ex);
        *reinterpret_cast<f32x4*>(ex) = (f32x4){0.f, 0.f, 0.f, 0.f};   // keep `extra` all-zero
      }
    }
    adam_tab4<true>(pp, mm, vv, gg * coef, wd, b2, omb2, eps, k);
    __builtin_nontemporal_store(pp, reinterpret_cast<f32x4*>(p + off));
    __builtin_nontemporal_store(mm, reinterpret_cast<f32x4*>(m + off));
    __builtin_nontemporal_store(vv, reinterpret_cast<f32x4*>(v + off));
    if (!UNTOUCHED_ONLY && u >= 0 && q == 0) map[r] = -1;
  }
}

#define FBN_ADAM_TABLE_ARGS                                                                                  \
  float *p, float *m, float *v, long long nrows, int *map, GradSrc gs, const float *coef, const AdamConsts *t,   \
      const int *step, float wd, float b2, float omb2, float eps
template <int D>
__global__ void __launch_bounds__(256) adam_table_all(FBN_ADAM_TABLE_ARGS) {
  adam_table_body<D, false>(p, m, v, nrows, map, gs, coef, t, step, wd, b2, omb2, eps);
}

// Untouched rows, as a low-footprint streaming kernel: it runs beside the backward on a side
// stream, so it must not take the CUs' wave slots from the backward's kernels.  Launched with
// <= 2 workgroups per CU; each lane keeps UNR rows (3 x 16 B each) in flight so the few waves
// still stream HBM near its rate (Little: ~12 MB in flight chip-wide).
template <int D>
__global__ void __launch_bounds__(256) adam_table_untouched(FBN_ADAM_TABLE_ARGS) {
  constexpr int G = D / 4, RPW = 64 / G, UNR = 4;
  const AdamConsts k = t[*step];
  const int lane = threadIdx.x & 63, q = lane % G;
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long r0 = gw * RPW * UNR; r0 < nrows; r0 += nw * RPW * UNR) {
    f32x4 pp[UNR], mm[UNR], vv[UNR];
    bool act[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const long long r = r0 + u * RPW + lane / G;
      act[u] = r < nrows && map[r] < 0;
      if (act[u]) {
        const size_t off = (size_t)r * D + 4 * q;
        pp[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(p + off));
        mm[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(m + off));
        vv[u] = __builtin_nontemporal_load(reinterpret_cast<f32x4*>(v + off));
      }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if (!act[u]) continue;
      const long long r = r0 + u * RPW + lane / G;
      const size_t off = (size_t)r * D + 4 * q;
      adam_zero_tab4<true>(pp[u], mm[u], vv[u], wd, b2, omb2, eps, k);
      __builtin_nontemporal_store(pp[u], reinterpret_cast<f32x4*>(p + off));
      __builtin_nontemporal_store(mm[u], reinterpret_cast<f32x4*>(m + off));
      __builtin_nontemporal_store(vv[u], reinterpret_cast<f32x4*>(v + off));
    }
  }
}

// ------------------------------------------------------------------ self-test of adam_tab4
// n threads x 4 elements of random Adam states (p in [2^-10, 4), m in [2^-30, 2^-2), v = m^2 x
// [1, 1025) -- |m| <= sqrt(v) as Adam's moments keep it -- and g zero or in [2^-30, 2^-2)) under
// random step constants and clip coefficients: the table-row step (hardware sqrt / rcp, fused
// moments) against the IEEE element step adam_elem.  dev[0..2] = max deviation of m, v, p in 1/16
// ulp of each update's scale (m: |m| + |g*coef| + |wd*p|; v: max(v, (1-b2) * that^2);
// p: max(|p|, |IEEE update|)).
__device__ __forceinline__ unsigned st_hash(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
  return x;
}
__device__ float st_value(unsigned h, int lo_exp, int hi_exp, bool sign) {
  const int ex = lo_exp + (int)(st_hash(h + 3) % (unsigned)(hi_exp - lo_exp + 1));
  const unsigned bits = ((unsigned)(ex + 127) << 23) | (h & 0x007fffffu) | ((sign && (h & 0x80000000u)) ? 0x80000000u : 0u);
  return __uint_as_float(bits);
}
__device__ __forceinline__ float ulp_of(float x) {   // ulp of |x| (normal range)
  return __uint_as_float(((__float_as_uint(fabsf(x)) >> 23) - 23u) << 23);
}
__global__ void adam_selftest_kernel(int n, unsigned seed, unsigned long long* dev) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned h = st_hash(seed * 0x9E3779B9u + (unsigned)i);
  AdamConsts k;
  k.w1 = 0.05f + 0.1f * (float)(st_hash(h + 1) & 0xffff) / 65536.f;
  k.nss = -1e-4f * (1.f + 200.f * (float)(st_hash(h + 2) & 0xffff) / 65536.f);
  k.bc2s = 0.0316f + 0.968f * (float)(st_hash(h + 3) & 0xffff) / 65536.f;
  k.rbc2s = (float)(1.0 / (double)k.bc2s);
  const float coef = (st_hash(h + 5) & 1) ? 1.f : 0.01f + 0.99f * (float)(st_hash(h + 6) & 0xffff) / 65536.f;
  const float wd = 1e-5f, b2 = 0.999f, omb2 = (float)(1.0 - 0.999), eps = 1e-8f;
  f32x4 p, m, v, g;
  for (int e = 0; e < 4; ++e) {
    const unsigned a = st_hash(h + 10 + 4 * e), b = st_hash(a), c = st_hash(b), d = st_hash(c);
    p[e] = st_value(a, -10, 1, true);
    m[e] = st_value(b, -30, -3, true);
    v[e] = m[e] * m[e] * (1.f + (float)(c & 0xffff) / 64.f);
    g[e] = (d & 3) ? 0.f : st_value(d, -30, -3, true);
  }
  f32x4 pf = p, mf = m, vf = v;
  k.dmul = 1.f;
  adam_tab4<true>(pf, mf, vf, g * coef, wd, b2, omb2, eps, k);
  float dm = 0.f, dv = 0.f, dp = 0.f;
  for (int e = 0; e < 4; ++e) {
    float pe = p[e], me = m[e], ve = v[e];
    adam_elem(pe, me, ve, g[e], coef, wd, b2, omb2, eps, k);
    const float gs = fabsf(g[e] * coef) + fabsf(wd * p[e]);
    dm = fmaxf(dm, fabsf(mf[e] - me) / ulp_of(fmaxf(fabsf(m[e]), gs)));
    dv = fmaxf(dv, fabsf(vf[e] - ve) / ulp_of(fmaxf(v[e], omb2 * gs * gs)));
    dp = fmaxf(dp, fabsf(pf[e] - pe) / ulp_of(fmaxf(fabsf(p[e]), fabsf(pe - p[e]))));
  }
  atomicMax(dev + 0, (unsigned long long)(dm * 16.f));
  atomicMax(dev + 1, (unsigned long long)(dv * 16.f));
  atomicMax(dev + 2, (unsigned long long)(dp * 16.f));
}

extern "C" int fbn_adam_selftest(int n, unsigned seed, unsigned long long* dev, void* stream) {
  if (n <= 0) return FBN_OK;
  fbn_launch(adam_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, seed, dev);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------ lazy table Adam (bit-identical to eager)
// A row whose loss gradient is zero at step s still gets torch's coupled-L2 Adam update
// (g = 0 * coef + wd * p, then m, v, p).  That update depends only on the row and on step s's
// schedule constants, so it can be REPLAYED later with the same float operations in the same
// order: bit-identical to stepping it eagerly.  last[r] = number of Adam steps applied to row r.
// Each step, before the gather reads the table, fbn_adam_catchup brings every row the batch
// claimed, plus a rolling window of nrows/F rows (window (step mod F)), up to `step`; the rolling
// window bounds every row's lag by F steps.  fbn_adam_touched then applies the step with the real
// gradient (last = step + 1) -- or, single GPU, fbn_adam_commit DEFERS it: the row records which
// per-sample gradient vector it received (pend[r]), the step's vectors are kept in a ring of
// F+1 steps and its clip coefficient in coef_hist, and the next replay of the row applies step
// last[r] with that gradient before the zero-gradient steps (same operations, same order: still
// bit-identical to eager Adam), so a touched row is read and written once per visit instead of
// twice.  fbn_adam_flush brings the whole table up to date (checkpoint, evaluation).
// ONE replay engine does the per-row arithmetic of all of them (replay_sorted: adam_tabk on four
// wave-wide rows at a time at D >= 128, on one row per lane group below).  Every kernel is a front
// end that decides which rows its lanes take (take_row: last and pend updated there) and hands the
// wave's rows to the engine: the step's claims (adam_claim2), the claimed rows of the host-split
// exchange (adam_catchup), the rolling window and the flush (adam_window2), the prefetches
// (adam_pretag + adam_prefetch2, the one-pass adam_prefetch, adam_pfbin + adam_pfreplay).
#define FBN_LAZY_MAX_LAG 512   // the largest window F

// Row state: ONE 16-B record per table row, {u64 pre-claim tag, i32 last, i32 pend}, so a claim
// that needs all three (the critical-path adam_claim2, the prefetch) pulls one sector per row
// instead of three.  The C ABI keeps field pointers: preclaim = record base, last = base + 8 B,
// pend = base + 12 B; each field is indexed with the record stride below.
#define FBN_RS_I 4   // record stride in ints
#define FBN_RS_Q 2   // in u64
static_assert(FBN_RS_I * 4 == FBN_ROW_STATE_BYTES && FBN_RS_Q * 8 == FBN_ROW_STATE_BYTES, "the header's record size");
// the whole record of row r from its `last` field pointer: {tag lo, tag hi, last, pend}
__device__ __forceinline__ int4 row_state(const int* last, long long r) {
  return *reinterpret_cast<const int4*>(last + (size_t)r * FBN_RS_I - 2);
}

// deferred gradients: pend[r] = index (b*2 + slot) of the per-sample vector row r received at step
// last[r] (-1 = none); ring[(s % ring_n) * ring_stride + idx * D] holds step s's vectors
struct PendSrc {
  int* pend;
  const float* ring;
  const float* coef_hist;   // [steps] clip coefficient of each step
  long long ring_stride;    // elements per ring slot (B * 2 * D)
  int ring_n;
  int bf16;                 // ring rows stored as bf16 (ring_n | FBN_RING_BF16 at the C ABI; sharded owner)
};
static inline PendSrc make_pend(int* pend, const float* ring, const float* coef_hist, long long stride, int ring_n) {
  return PendSrc{pend, ring, coef_hist, stride, ring_n & ~FBN_RING_BF16, (ring_n & FBN_RING_BF16) ? 1 : 0};
}
// N ring elements at element offset go (f32, or bf16 widened).  Branch-free, as pend_load needs (a load
// under a branch makes hipcc drain every load in flight at the next use): ONE load of N floats' bytes
// from the f32 address or the bf16 one -- a bf16 ring reads N bf16 values plus N more it ignores (the
// trainer pads a bf16 ring by 16 elements so the last row's wider read stays inside the allocation) --
// and the widening selected per element.
template <typename V, int N>
__device__ __forceinline__ V ring_load(const float* ring, int bf16, size_t go) {
  const char* a = reinterpret_cast<const char*>(ring) + (bf16 ? 2 * go : 4 * go);
  const V raw = *reinterpret_cast<const V*>(a);
  V x;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const unsigned w = __float_as_uint(raw[k >> 1]);
    const float h = __uint_as_float((k & 1) ? (w & 0xffff0000u) : (w << 16));
    x[k] = bf16 ? h : raw[k];
  }
  return x;
}
// A row's deferred gradient -- the N elements from element `col` of vector pe in the ring slot of step
// k0 -- and that step's clip coefficient.  Branch-free (a load under a branch makes hipcc wait
// vmcnt(0) at the next use of any load, which would drain the next rows' loads in flight): a row with
// no deferred gradient (pe < 0) reads an L2-resident dummy line, the head of p.
template <typename V, int N, int D>
__device__ __forceinline__ void pend_load(V& g, float& c, const PendSrc& ps, const float* __restrict__ p, int k0,
                                          int pe, int col) {
  const float* ring = ps.ring ? ps.ring : p;
  const float* coef = ps.coef_hist ? ps.coef_hist : p;
  const size_t go = pe >= 0 ? (size_t)(k0 % ps.ring_n) * ps.ring_stride + (size_t)pe * D : 0;
  g = ring_load<V, N>(ring, ps.bf16, go + col);
  c = coef[pe >= 0 ? k0 : 0];
}

// This lane takes row rr (row state rs, behind step T) for the replay: r = the row, pe = its deferred
// vector, key = its first zero-gradient step (after the deferred one); the row is marked up to date.
__device__ __forceinline__ void take_row(int& r, int& key, int& pe, long long rr, const int4& rs, int T,
                                         int* __restrict__ last, const PendSrc& ps) {
  r = (int)rr;
  if (ps.pend) pe = rs.w;
  key = rs.z + (pe >= 0 ? 1 : 0);
  last[(size_t)(rr) * FBN_RS_I] = T;
  if (pe >= 0) ps.pend[(size_t)(rr) * FBN_RS_I] = -1;
}

// A wave's rows, one per lane (row r, key, deferred vector pe), sorted by key ascending: a bitonic
// network over lane shuffles.  (A macro: as an inline function taking the three by reference the
// engines compiled to other code than with the network written in place; this and the two helpers
// written out below are recorded in profiles/r09_one_engine_asm_compare.txt.)
#define FBN_SORT_ROWS(r, key, pe, lane)                                                                          \
  _Pragma("unroll") for (int kk = 2; kk <= 64; kk <<= 1)                                                         \
    _Pragma("unroll") for (int j = kk >> 1; j > 0; j >>= 1) {                                                    \
      const int ok = __shfl_xor(key, j, 64), orr = __shfl_xor(r, j, 64), ope = __shfl_xor(pe, j, 64);            \
      const bool up = (lane & kk) == 0, lower = (lane & j) == 0;                                                 \
      if (lower == up ? ok < key : ok > key) {                                                                   \
        key = ok;                                                                                                \
        r = orr;                                                                                                 \
        pe = ope;                                                                                                \
      }                                                                                                          \
    }

// A wave-wide row (D >= 128): 64 lanes x D/64 elements.
template <int N> struct FVec;
template <> struct FVec<2> { typedef float T __attribute__((ext_vector_type(2))); };
template <> struct FVec<4> { typedef f32x4 T; };
template <int D>
struct WideRow {
  static constexpr int N = D / 64;
  typedef typename FVec<N>::T V;
  V p, m, v, g;
  float c;
};
template <int D>
__device__ __forceinline__ void wide_load(WideRow<D>& x, const float* __restrict__ p, const float* __restrict__ m,
                                          const float* __restrict__ v, int r, int k0, int pe, const PendSrc& ps,
                                          int lane) {
  typedef typename WideRow<D>::V V;
  constexpr int N = WideRow<D>::N;
  const size_t off = (size_t)r * D + lane * N;
  x.p = *reinterpret_cast<const V*>(p + off);
  x.m = *reinterpret_cast<const V*>(m + off);
  x.v = *reinterpret_cast<const V*>(v + off);
  pend_load<V, N, D>(x.g, x.c, ps, p, k0, pe, lane * N);
}
template <int D>
__device__ __forceinline__ void wide_store(const WideRow<D>& x, float* __restrict__ p, float* __restrict__ m,
                                           float* __restrict__ v, int r, int lane) {
  typedef typename WideRow<D>::V V;
  const size_t off = (size_t)r * D + lane * WideRow<D>::N;
  *reinterpret_cast<V*>(p + off) = x.p;
  *reinterpret_cast<V*>(m + off) = x.m;
  *reinterpret_cast<V*>(v + off) = x.v;
}

// The entries of a batch and where their row claims go (adam_claim2, the prefetch kernels): entry
// e = b*(L+1)+t claims its row as claim_rows_kernel does (first CAS wins; map, slot_row, dup
// written), and a winning entry's row joins the replay at once -- one launch instead of claim +
// catch-up.
struct ClaimSrc {
  const int64_t* item;
  const int64_t* seq;
  int L;
  long long V;
  int* map;
  int* slot_row;
  int* dup;
  int* hasdup;   // optional: hasdup[claimer] = 1 when another entry hit its row (deterministic fold)
  // optional pre-claims (fbn_adam_prefetch of the previous step, for this very batch): pre[id] =
  // (step << 32) | (0xFFFFFFFF - the smallest entry index with this id); a claim whose tag is the
  // current step is final -- no CAS (popular rows would serialise thousands on one word)
  unsigned long long* pre;
  // owner mode (N > 1, fbn_adam_prefetch_rows): entry i's row is the local row lids[i] (-1: none;
  // rank 0's row 0 is the padding id and skipped when skip0); item / seq unused
  const int* lids;
  int skip0;
};

// ---- Ahead-of-time catch-up of the NEXT batch, on the side stream during step t, after step t's
// claims: a row of the next batch that batch t does not touch (map == -1) takes only zero-gradient
// steps through step t inclusive -- g = 0 * coef + wd * p, whatever step t's clip coefficient -- so
// it is brought to last = t + 1 now (same operations, same order: still bit-identical to eager Adam)
// and step t + 1's claimed-row catch-up finds it up to date.  With pre-claims (the bench and every
// trainer step given a next batch of its own shape) it runs in two passes:
//   pass 1 (adam_pretag_kernel): every entry posts its tagged claim with one non-returning
//     atomic max -- the smallest entry index of an id wins, as the claim at step t + 1 expects;
//   pass 2 (adam_prefetch2_kernel): one entry per lane and no atomics: the winning entry of a row
//     this batch does not touch takes the row (last[r] = T, pend[r] consumed), a wave sorts its
//     rows by replay start and replays them FOUR at a time (eight independent update chains per
//     lane at D = 128) while the next four rows' loads are in flight; the schedule constants of
//     the last FBN_PF_WIN steps sit in LDS and each step's are read one step ahead.
// Without them (a next batch of another shape, D >= 128) one pass, adam_prefetch_kernel: a row is
// taken by the entry whose returning CAS moves last[r] to T.
#define FBN_PF_WIN 256

// entry i's row, or -1: the batch's ids (item, then history slots; 0 = padding), or in owner mode
// (cs.lids, N > 1) the local rows the next step's requests name (-1 = none; rank 0's row 0 is the
// padding id)
__device__ __forceinline__ long long entry_row(const ClaimSrc& cs, long long i) {
  if (cs.lids) {
    const long long id = cs.lids[i];
    return (id >= 0 && id < cs.V && !(cs.skip0 && id == 0)) ? id : -1;
  }
  const long long b = i / (cs.L + 1), tt = i - b * (cs.L + 1);
  const long long id = tt == 0 ? cs.item[b] : cs.seq[b * cs.L + (tt - 1)];
  return (id > 0 && id < cs.V) ? id : -1;
}

// One block of FBN_PRETAG_BLOCK entries folds its claims in an LDS table first (id -> smallest
// entry index, LDS atomics) and posts ONE global atomic max per distinct id: with Zipf ids the
// hottest row takes ~9 % of a batch's entries, and one same-address atomic per entry serialised
// ~15 K of them at one L2 channel (~100 us, stalling every stream's traffic through it).  The
// posted value is the same maximum as per-entry posting: bit-identical pre-claims.
#define FBN_PRETAG_BLOCK 1024
#define FBN_PRETAG_SLOTS 2048   // open addressing, load factor <= 1/2
__global__ void __launch_bounds__(FBN_PRETAG_BLOCK) adam_pretag_kernel(ClaimSrc cs, int n,
                                                                        const int* __restrict__ step) {
  __shared__ int hkey[FBN_PRETAG_SLOTS];
  __shared__ int hval[FBN_PRETAG_SLOTS];
  for (int k = threadIdx.x; k < FBN_PRETAG_SLOTS; k += blockDim.x) {
    hkey[k] = -1;
    hval[k] = 0x7fffffff;
  }
  __syncthreads();
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  const long long id = i < n ? entry_row(cs, i) : -1;
  if (id >= 0) {   // (local rows and entry indices fit 31 bits: V, n < 2^31)
    unsigned h = ((unsigned)id * 2654435761u) >> (32 - 11);
    for (;;) {
      int cur = hkey[h];
      if (cur == -1) {
        const int prev = atomicCAS(&hkey[h], -1, (int)id);
        cur = prev == -1 ? (int)id : prev;
      }
      if (cur == (int)id) {
        atomicMin(&hval[h], (int)i);
        break;
      }
      h = (h + 1) & (FBN_PRETAG_SLOTS - 1);
    }
  }
  __syncthreads();
  const unsigned long long T = (unsigned long long)(*step + 1);
  for (int k = threadIdx.x; k < FBN_PRETAG_SLOTS; k += blockDim.x) {
    const int r = hkey[k];
    if (r >= 0)
      atomicMax(cs.pre + (size_t)r * FBN_RS_Q, (T << 32) | (0xFFFFFFFFull - (unsigned long long)(unsigned)hval[k]));
  }
}

// adam_tab1 with the step's constants as (w1, nss, rbc2s, dmul): the same operations, same order
// written on whole vectors so every non-transcendental step is a packed v_pk_* instruction (the
// element-wise fmas round exactly as adam_tab1's scalar ones)
template <bool DW, int N>
__device__ __forceinline__ void adam_tabk(typename FVec<N>::T& pp, typename FVec<N>::T& mm, typename FVec<N>::T& vv,
                                          typename FVec<N>::T gg, float wd, float b2, float omb2, float eps,
                                          f32x4 k) {
  typedef typename FVec<N>::T V;
  const V vwd = wd, vb2 = b2, vomb2 = omb2, veps = eps, w1 = k[0], nss = k[1], rb = k[2];
#ifdef FBN_ADAM_IEEE
  {
    const V g = gg + vwd * pp;
    V p = pp;
    if (DW) p = p * (V)k[3];
    mm = mm + w1 * (g - mm);
    vv = vv * vb2 + (vomb2 * g) * g;
#pragma unroll
    for (int e = 0; e < N; ++e) pp[e] = p[e] + (k[1] * mm[e]) / (sqrtf(vv[e]) * k[2] + eps);
    return;
  }
#endif
  const V g = __builtin_elementwise_fma(vwd, pp, gg);
  V p = pp;
  if (DW) p = p * (V)k[3];
  mm = __builtin_elementwise_fma(w1, g - mm, mm);
  vv = __builtin_elementwise_fma(vomb2 * g, g, vv * vb2);
  V sq, rc;
#pragma unroll
  for (int e = 0; e < N; ++e) sq[e] = __builtin_amdgcn_sqrtf(vv[e]);
  const V den = __builtin_elementwise_fma(sq, rb, veps);
#pragma unroll
  for (int e = 0; e < N; ++e) rc[e] = __builtin_amdgcn_rcpf(den[e]);
  pp = __builtin_elementwise_fma(nss * mm, rc, p);
}
__device__ __forceinline__ f32x4 consts4(const AdamConsts& k) { return (f32x4){k.w1, k.nss, k.rbc2s, k.dmul}; }

// One group of the replay engine: G wave-wide rows (cur, rows cr, replay starts ck, deferred
// vectors cp; slots past cnt carry row 0 and no steps) brought to T, then stored.
#define FBN_REPLAY_G 4   // rows per group: eight independent update chains per lane at D = 128
template <int D, bool DW>
__device__ __forceinline__ void replay_group(WideRow<D> (&cur)[FBN_REPLAY_G], const int (&cr)[FBN_REPLAY_G],
                                             const int (&ck)[FBN_REPLAY_G], const int (&cp)[FBN_REPLAY_G], int j0,
                                             int cnt, int T, float* __restrict__ p, float* __restrict__ m,
                                             float* __restrict__ v, const AdamConsts* __restrict__ table, float wd,
                                             float b2, float omb2, float eps, int lane) {
  constexpr int G = FBN_REPLAY_G;
  typedef typename WideRow<D>::V V;
  constexpr int N = WideRow<D>::N;
  const V zero = {};
  // A row spans the whole wave, so its step -- and the step's schedule constants -- are
  // wave-uniform: scalar loads from the table (no LDS staging, no vector registers for them).
  // deferred-gradient steps (step ck - 1 with its stored vector and clip coefficient)
#pragma unroll
  for (int x = 0; x < G; ++x)
    if (cp[x] >= 0) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, cur[x].g * cur[x].c, wd, b2, omb2, eps,
                                     consts4(table[ck[x] - 1]));
  // END-aligned staircase: every row replays up to T and the rows are sorted by start (ck
  // ascending; slots past cnt start at T), so at step s the rows x with ck[x] <= s are all at the
  // SAME step and share one set of constants -- read by a scalar load one step ahead.  Phase k runs
  // rows 0..k from ck[k] to ck[k+1] (ck[G] = T): the longest row never replays alone while a later
  // row could join it, and no step waits on its own constants' load.
  int s = ck[0] < T ? ck[0] : T;
  // steps in blocks of four: the next block's four constant sets are loaded while this block runs,
  // so a scalar-cache miss (every other step: 32-B records) is hidden behind four steps of the
  // update chains instead of one; the partial last block of a phase uses the block's own sets
#pragma unroll
  for (int k = 0; k < G; ++k) {
    const int send = k + 1 < G ? min(ck[k + 1], T) : T;
    if (s >= send) continue;
    f32x4 k0 = consts4(table[s]), k1 = consts4(table[min(s + 1, T)]), k2 = consts4(table[min(s + 2, T)]),
          k3 = consts4(table[min(s + 3, T)]);
    for (; s + 4 <= send; s += 4) {
      const f32x4 n0 = consts4(table[min(s + 4, T)]), n1 = consts4(table[min(s + 5, T)]),
                  n2 = consts4(table[min(s + 6, T)]), n3 = consts4(table[min(s + 7, T)]);
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k0);
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k1);
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k2);
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k3);
      k0 = n0;
      k1 = n1;
      k2 = n2;
      k3 = n3;
    }
    if (s < send) {
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k0);
      ++s;
    }
    if (s < send) {
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k1);
      ++s;
    }
    if (s < send) {
#pragma unroll
      for (int x = 0; x <= k; ++x) adam_tabk<DW, N>(cur[x].p, cur[x].m, cur[x].v, zero, wd, b2, omb2, eps, k2);
      ++s;
    }
  }
#pragma unroll
  for (int x = 0; x < G; ++x)
    if (j0 + x < cnt) wide_store<D>(cur[x], p, m, v, cr[x], lane);
}

// The replay engine of the two-pass prefetch and the window pass: a wave's rows (one per lane:
// row r, first zero-gradient step key -- INT_MAX = none --, deferred vector pe), sorted by key,
// brought to T steps FBN_REPLAY_G at a time, the next group's loads in flight while one replays.
template <int D, bool DW>
__device__ __forceinline__ void replay4_sorted(int r, int key, int pe, int cnt, int T, int w0,
                                               const f32x4* __restrict__ win, float* __restrict__ p,
                                               float* __restrict__ m, float* __restrict__ v,
                                               const AdamConsts* __restrict__ table, float wd, float b2,
                                               float omb2, float eps, const PendSrc& ps, int lane) {
  constexpr int G = FBN_REPLAY_G;
  FBN_SORT_ROWS(r, key, pe, lane);   // ascending replay start (descending replay length); rows past cnt last
  // group slot x of the rows at j0: (row, first zero step, deferred vector); past cnt: row 0, no steps
  auto get = [&](int idx, int& rr, int& kk, int& pp) {   // idx wave-uniform
    const int sl = idx < cnt ? idx : 0;
    rr = __builtin_amdgcn_readlane(r, sl);
    kk = __builtin_amdgcn_readlane(key, sl);
    pp = __builtin_amdgcn_readlane(pe, sl);
    if (idx >= cnt) { rr = 0; kk = T; pp = -1; }
  };
  struct Grp {
    WideRow<D> w[G];
    int r[G], k[G], p[G];
  };
  auto fill = [&](Grp& g, int j) {   // past the last group: row 0, discarded
#pragma unroll
    for (int x = 0; x < G; ++x) {
      get(j + x, g.r[x], g.k[x], g.p[x]);
      wide_load<D>(g.w[x], p, m, v, g.r[x], g.p[x] >= 0 ? g.k[x] - 1 : g.k[x], g.p[x], ps, lane);
    }
  };
  Grp a, b;
  fill(a, 0);
  for (int j0 = 0; j0 < cnt; j0 += G) {
    fill(b, j0 + G);
    replay_group<D, DW>(a.w, a.r, a.k, a.p, j0, cnt, T, p, m, v, table, wd, b2, omb2, eps, lane);
    a = b;
  }
}

// The same engine for d < 128 (C2's d = 16): a row is G = d/4 lanes of 4 elements, so a wave replays
// 64/G sorted rows per round, each lane group stepping its own row (the sort keeps a round's replay
// lengths alike); the next round's rows are loaded before this round's arithmetic, and each step's
// constants are read from the LDS window one step ahead.
template <int D, bool DW>
__device__ __forceinline__ void replay_narrow_sorted(int r, int key, int pe, int cnt, int T, int w0,
                                                     const f32x4* __restrict__ win, float* __restrict__ p,
                                                     float* __restrict__ m, float* __restrict__ v,
                                                     const AdamConsts* __restrict__ table, float wd, float b2,
                                                     float omb2, float eps, const PendSrc& ps, int lane) {
  constexpr int G = D / 4, RPW = 64 / G;
  FBN_SORT_ROWS(r, key, pe, lane);
  const int q = lane % G, grp = lane / G;
  auto fetch = [&](int j0, int& rr, int& kk, int& pp) {
    const int src = j0 + grp;
    const int sl = src < 64 ? src : 0;
    rr = __shfl(r, sl, 64);
    kk = __shfl(key, sl, 64);
    pp = __shfl(pe, sl, 64);
    if (src >= cnt) { rr = 0; kk = T; pp = -1; }
  };
  struct Row { f32x4 p, m, v, g; float c; };
  auto load = [&](Row& x, int rr, int kk, int pp) {
    const size_t off = (size_t)rr * D + 4 * q;
    x.p = *reinterpret_cast<const f32x4*>(p + off);
    x.m = *reinterpret_cast<const f32x4*>(m + off);
    x.v = *reinterpret_cast<const f32x4*>(v + off);
    // pend_load, written out (through the helper the narrow engine compiled to other code)
    const int k0 = pp >= 0 ? kk - 1 : kk;   // the deferred gradient's step
    const float* ring = ps.ring ? ps.ring : p;
    const float* coef = ps.coef_hist ? ps.coef_hist : p;
    const size_t go = pp >= 0 ? (size_t)(k0 % ps.ring_n) * ps.ring_stride + (size_t)pp * D : 0;
    x.g = ring_load<f32x4, 4>(ring, ps.bf16, go + 4 * q);
    x.c = coef[pp >= 0 ? k0 : 0];
  };
  int rc, kc, pc;
  fetch(0, rc, kc, pc);
  Row cur;
  load(cur, rc, kc, pc);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  for (int j0 = 0; j0 < cnt; j0 += RPW) {
    int rn, kn, pn;
    fetch(j0 + RPW, rn, kn, pn);
    Row nxt;
    load(nxt, rn, kn, pn);   // past the last round: row 0, discarded
    if (pc >= 0) {
      const int s = kc - 1;
      adam_tabk<DW, 4>(cur.p, cur.m, cur.v, cur.g * cur.c, wd, b2, omb2, eps, s >= w0 ? win[s - w0] : consts4(table[s]));
    }
    int s = kc;
    for (; s < T && s < w0; ++s) adam_tabk<DW, 4>(cur.p, cur.m, cur.v, zero, wd, b2, omb2, eps, consts4(table[s]));
    if (s < T) {
      f32x4 k = win[s - w0];
      for (; s < T; ++s) {
        const f32x4 kx = win[s + 1 - w0];   // <= T - w0: in the window
        adam_tabk<DW, 4>(cur.p, cur.m, cur.v, zero, wd, b2, omb2, eps, k);
        k = kx;
      }
    }
    if (j0 + grp < cnt) {
      const size_t off = (size_t)rc * D + 4 * q;
      *reinterpret_cast<f32x4*>(p + off) = cur.p;
      *reinterpret_cast<f32x4*>(m + off) = cur.m;
      *reinterpret_cast<f32x4*>(v + off) = cur.v;
    }
    cur = nxt;
    rc = rn;
    kc = kn;
    pc = pn;
  }
}

template <int D, bool DW>
__device__ __forceinline__ void replay_sorted(int r, int key, int pe, int cnt, int T, int w0,
                                              const f32x4* __restrict__ win, float* __restrict__ p,
                                              float* __restrict__ m, float* __restrict__ v,
                                              const AdamConsts* __restrict__ table, float wd, float b2, float omb2,
                                              float eps, const PendSrc& ps, int lane) {
  if constexpr (D >= 128) replay4_sorted<D, DW>(r, key, pe, cnt, T, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
  else replay_narrow_sorted<D, DW>(r, key, pe, cnt, T, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
}

template <int D, bool DW>
__device__ __forceinline__ void adam_prefetch2_body(float* __restrict__ p, float* __restrict__ m,
                                                    float* __restrict__ v, const ClaimSrc& cs, int n,
                                                    int* __restrict__ last, const AdamConsts* __restrict__ table,
                                                    const int* __restrict__ step, float wd, float b2, float omb2,
                                                    float eps, const PendSrc& ps, int epw, int blk, int nblk) {
  __shared__ f32x4 win[FBN_PF_WIN + 1];   // constants of steps [w0, T]
  const int T = *step + 1;
  const int w0 = T > FBN_PF_WIN ? T - FBN_PF_WIN : 0;
  if constexpr (D < 128)   // the narrow engine's LDS constants (wave-wide rows read the table directly)
    for (int s = threadIdx.x; s <= T - w0; s += blockDim.x) win[s] = consts4(table[w0 + s]);
  const int lane = threadIdx.x & 63;
  if constexpr (D < 128) __syncthreads();   // the LDS window (no barrier after this point)
  // epw entries per wave (lanes past epw hold none); a grid smaller than the entry chunks walks
  // them wave-strided
  const long long nchunk = ((long long)n + epw - 1) / epw;
  const long long wstride = ((long long)nblk * blockDim.x) >> 6;
  for (long long ch = ((long long)blk * blockDim.x + threadIdx.x) >> 6; ch < nchunk; ch += wstride) {
  const long long i = lane < epw ? ch * epw + lane : n;
  int r = 0, key = 0x7fffffff, pe = -1;
  if (i < n) {
    const long long id = entry_row(cs, i);
    if (id >= 0) {
      const int4 rs = row_state(last, id);   // tag, last, pend: one 16-B load
      const unsigned long long pv = ((unsigned long long)(unsigned)rs.y << 32) | (unsigned)rs.x;
      if ((int)(pv >> 32) == T && (0xFFFFFFFFu - (unsigned)pv) == (unsigned)i && cs.map[id] == -1) {
        if (rs.z < T) take_row(r, key, pe, id, rs, T, last, ps);   // this entry owns the row: its replay through step T - 1
      }
    }
  }
  const int cnt = __popcll(__ballot(key != 0x7fffffff));
  if (cnt == 0) continue;
  replay_sorted<D, DW>(r, key, pe, cnt, T, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
  }
}
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_prefetch2_kernel(float* __restrict__ p, float* __restrict__ m,
                                                             float* __restrict__ v, ClaimSrc cs, int n,
                                                             int* __restrict__ last,
                                                             const AdamConsts* __restrict__ table,
                                                             const int* __restrict__ step, float wd, float b2,
                                                             float omb2, float eps, PendSrc ps, int epw) {
  adam_prefetch2_body<D, DW>(p, m, v, cs, n, last, table, step, wd, b2, omb2, eps, ps, epw, blockIdx.x, gridDim.x);
}
// The one-pass form (no pre-claims; D >= 128): one entry per lane, 64 entries per wave, walked
// wave-strided; duplicates of a row lose the CAS and skip.
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_prefetch_kernel(float* __restrict__ p, float* __restrict__ m,
                                                            float* __restrict__ v, ClaimSrc cs, int n,
                                                            int* __restrict__ last,
                                                            const AdamConsts* __restrict__ table,
                                                            const int* __restrict__ step, float wd, float b2,
                                                            float omb2, float eps, PendSrc ps) {
  const int T = *step + 1;
  const int lane = threadIdx.x & 63;
  const long long nchunk = ((long long)n + 63) / 64;
  const long long wstride = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long ch = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6; ch < nchunk; ch += wstride) {
    const long long i = ch * 64 + lane;
    int r = 0, key = 0x7fffffff, pe = -1;
    if (i < n) {
      const long long id = entry_row(cs, i);
      if (id >= 0 && cs.map[id] == -1) {
        const int4 rs = row_state(last, id);
        // (pend[r] changes only with last[r]: the pair read above is the winner's; take_row stores
        // last[r] = T once more, the value the CAS wrote)
        if (rs.z < T && atomicCAS(last + (size_t)id * FBN_RS_I, rs.z, T) == rs.z) take_row(r, key, pe, id, rs, T, last, ps);
      }
    }
    const int cnt = __popcll(__ballot(key != 0x7fffffff));
    if (cnt == 0) continue;
    replay4_sorted<D, DW>(r, key, pe, cnt, T, 0, nullptr, p, m, v, table, wd, b2, omb2, eps, ps, lane);
  }
}

// ---- The prefetch with its replay balanced longest-first (fbn_adam_prefetch_binned, D >= 128).
// adam_prefetch2 takes 64 entries per wave; a wave's rows carry Exp(~14)-distributed replay lengths,
// so the slowest wave runs ~2x the mean and sets the launch time (VERDICT r4 "weak" 3).  Here the
// same claims are made in a binning pass that appends each owned row's record {row, first zero-
// gradient step, deferred vector} to a bin by replay length, and a replay pass hands every wave a
// chunk of 64 records of one bin, longest bins first (the lowest wave ids, dispatched first):
// longest-processing-time-first, with like lengths in a wave so the four-row staircase rarely
// replays a row alone.  Round 4's binned attempt (profiles/r04_binned_prefetch_rejected.txt) lost on
// two counts fixed here: its 32 bin counters shared one 128-B line (every wave's appends met on
// it; ~88 atomics per us per line) -- here every (bin, block % 8) counter has a line of its own and
// a wave issues its appends for all bins in ONE round trip (lane j adds the wave's count of bin j);
// and its replay took one record per lane -- here the records feed the four-row engine as before.
// Same rows, same operations in the same order: bit-identical to adam_prefetch2.
#define FBN_PFB_NB 32       // replay-length bins: bin = min((len - 1) / 4, 31)  (lags stay <= F = 128)
#define FBN_PFB_NC 8        // counter copies per bin (block id % 8)
#define FBN_PFB_LINE 32     // counter stride in ints (one 128-B line each)

__device__ __forceinline__ long long pfb_cap(int nblk) { return (long long)((nblk + FBN_PFB_NC - 1) / FBN_PFB_NC) * 256; }

// pass A: the claims of adam_prefetch2 (one entry per lane), the owned rows appended to the bins
__global__ void __launch_bounds__(256) adam_pfbin_kernel(ClaimSrc cs, int n, int* __restrict__ last,
                                                         const int* __restrict__ step, PendSrc ps,
                                                         unsigned* __restrict__ counts, int4* __restrict__ recs) {
  const int T = *step + 1;
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  int r = 0, key = 0x7fffffff, pe = -1;
  if (i < n) {
    const long long id = entry_row(cs, i);
    if (id >= 0) {
      const int4 rs = row_state(last, id);
      const unsigned long long pv = ((unsigned long long)(unsigned)rs.y << 32) | (unsigned)rs.x;
      if ((int)(pv >> 32) == T && (0xFFFFFFFFu - (unsigned)pv) == (unsigned)i && cs.map[id] == -1) {
        if (rs.z < T) take_row(r, key, pe, id, rs, T, last, ps);
      }
    }
  }
  const bool own = key != 0x7fffffff;
  // replay length T - (k0) counts the deferred step too: len >= 1 for every owned row
  const int len = own ? T - key + (pe >= 0 ? 1 : 0) : 1;
  const int bin = own ? min((len - 1) >> 2, FBN_PFB_NB - 1) : 0;
  // every bin's count in this wave and each lane's rank inside its bin (32 ballots)
  int rank = 0, mycnt = 0;
#pragma unroll
  for (int j = 0; j < FBN_PFB_NB; ++j) {
    const unsigned long long mk = __ballot(own && bin == j);
    if (own && bin == j)
      rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0u));
    if (lane == j) mycnt = __popcll(mk);
  }
  // lane j < 32: ONE returning atomic for bin j (every bin's append in the same round trip)
  const int c8 = blockIdx.x & (FBN_PFB_NC - 1);
  unsigned base = 0;
  if (lane < FBN_PFB_NB && mycnt > 0)
    base = atomicAdd(counts + ((size_t)lane * FBN_PFB_NC + c8) * FBN_PFB_LINE, (unsigned)mycnt);
  const unsigned mybase = __shfl(base, bin, 64);
  if (own) {
    const long long cap = pfb_cap(gridDim.x);
    recs[((long long)bin * FBN_PFB_NC + c8) * cap + mybase + rank] = (int4){r, key, pe, 0};
  }
}

// pass B: wave w takes the w-th chunk of `ch` records (ch <= 64) in the order (bin descending, block
// copy c8 ascending); waves past the last chunk exit.  The counts are zeroed by the next call's
// pfb_zero.  ch = 32 by default: about as many waves as adam_prefetch2's (64 entries -> ~31 rows
// each); chunks of 64 halve the waves and measured 0.474 vs 0.431 ms/step (fewer chains in flight).
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_pfreplay_kernel(float* __restrict__ p, float* __restrict__ m,
                                                            float* __restrict__ v, const int* __restrict__ step,
                                                            float wd, float b2, float omb2, float eps,
                                                            const AdamConsts* __restrict__ table, PendSrc ps,
                                                            const unsigned* __restrict__ counts,
                                                            const int4* __restrict__ recs, int nblk_bin, int ch) {
  const int T = *step + 1;
  const int lane = threadIdx.x & 63;
  const int w = (int)(((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  // lane l holds lists o = 4l .. 4l+3 of the longest-first order (o -> bin 31 - o / 8, c8 = o % 8)
  int nc[4], tot = 0;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int o = 4 * lane + u;
    const int bin = FBN_PFB_NB - 1 - o / FBN_PFB_NC, c8 = o % FBN_PFB_NC;
    const unsigned c = counts[((size_t)bin * FBN_PFB_NC + c8) * FBN_PFB_LINE];
    nc[u] = (int)((c + ch - 1) / ch);
    tot += nc[u];
  }
  // inclusive prefix of the chunk counts over the lanes
  int inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  const int start = inc - tot;
  const int total = __shfl(inc, 63, 64);
  if (w >= total) return;
  const unsigned long long hit = __ballot(w >= start && w < inc);
  const int src = __ffsll((long long)hit) - 1;
  int lo = __shfl(start, src, 64);
  int sel = 0;
  const int c0 = __shfl(nc[0], src, 64), c1 = __shfl(nc[1], src, 64), c2 = __shfl(nc[2], src, 64);
  if (w >= lo + c0) { lo += c0; sel = 1;
    if (w >= lo + c1) { lo += c1; sel = 2;
      if (w >= lo + c2) { lo += c2; sel = 3; } } }
  const int o = 4 * src + sel;
  const int bin = FBN_PFB_NB - 1 - o / FBN_PFB_NC, c8 = o % FBN_PFB_NC;
  const int cntl = (int)counts[((size_t)bin * FBN_PFB_NC + c8) * FBN_PFB_LINE];
  const int j0 = (w - lo) * ch;
  const int cnt = min(ch, cntl - j0);
  int r = 0, key = 0x7fffffff, pe = -1;
  if (lane < cnt) {
    const int4 rec = recs[((long long)bin * FBN_PFB_NC + c8) * pfb_cap(nblk_bin) + j0 + lane];
    r = rec.x;
    key = rec.y;
    pe = rec.z;
  }
  replay4_sorted<D, DW>(r, key, pe, cnt, T, 0, nullptr, p, m, v, table, wd, b2, omb2, eps, ps, lane);
}

__global__ void pfb_zero_kernel(unsigned* __restrict__ counts) {
  const int i = threadIdx.x;
  if (i < FBN_PFB_NB * FBN_PFB_NC) counts[(size_t)i * FBN_PFB_LINE] = 0u;
}

// Single GPU, D >= 128: the step's row claims + the claimed rows' catch-up (fbn_adam_claim_catchup)
// with one entry per lane.  A lane's row state -- its pre-claim tag, last[] and pend[] -- is loaded
// in ONE round trip right after the id (they depend on the id only; nothing else writes them while
// this kernel runs: the previous step's side work was joined before its step tail, this step's starts
// after the claims), instead of id -> tag -> claim -> last -> pend one after another; the rows that
// are behind are replayed by the four-row engine.  Claims are those of claim_rows_kernel (a tagged
// pre-claim, else plain load + CAS; dup / hasdup written the same way).
template <int D, bool DW>
__device__ __forceinline__ void adam_claim2_body(float* __restrict__ p, float* __restrict__ m,
                                                 float* __restrict__ v, const ClaimSrc& cs, int n,
                                                 int* __restrict__ last, const AdamConsts* __restrict__ table,
                                                 const int* __restrict__ step, float wd, float b2,
                                                 float omb2, float eps, const PendSrc& ps, int blk) {
  __shared__ f32x4 win[FBN_PF_WIN + 1];
  const int t = *step;
  const int w0 = t > FBN_PF_WIN ? t - FBN_PF_WIN : 0;
  const int lane = threadIdx.x & 63;
  const long long i = (long long)blk * blockDim.x + threadIdx.x;
  int r = 0, key = 0x7fffffff, pe = -1;
  if (i < n) {
    // (entry_row and take_row written out: through the helpers this kernel, the step's critical path,
    // compiled to other code)
    long long id;
    bool ok;
    if (cs.lids) {   // owner mode (N > 1): the received local rows (negative: an empty slot)
      id = cs.lids[i];
      ok = id >= 0 && id < cs.V && !(cs.skip0 && id == 0);
    } else {
      const long long b = i / (cs.L + 1), tt = i - b * (cs.L + 1);
      id = tt == 0 ? cs.item[b] : cs.seq[b * cs.L + (tt - 1)];
      ok = id > 0 && id < cs.V;
    }
    int owner = -1, mine = -1;
    if (ok) {
      const int4 rs = row_state(last, id);   // tag, last, pend: one 16-B load
      const unsigned long long pv = cs.pre ? (((unsigned long long)(unsigned)rs.y << 32) | (unsigned)rs.x) : 0ull;
      const int k0 = rs.z;
      const int pe0 = ps.pend ? rs.w : -1;
      if ((int)(pv >> 32) == t && t > 0) {   // pre-claimed: the smallest entry index claims
        owner = (int)(0xFFFFFFFFu - (unsigned)pv);
        if (owner == (int)i) {
          cs.map[id] = (int)i;
          cs.slot_row[i] = (int)id;
          mine = (int)id;
          owner = -1;
        }
      } else {
        owner = __hip_atomic_load(cs.map + id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (owner == -1) {
          int expected = -1;
          if (__hip_atomic_compare_exchange_strong(cs.map + id, &expected, (int)i, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT)) {
            cs.slot_row[i] = (int)id;
            mine = (int)id;
          } else {
            owner = expected;
          }
        }
      }
      if (mine >= 0 && k0 < t) {
        r = mine;
        pe = pe0;
        key = k0 + (pe0 >= 0 ? 1 : 0);
        last[(size_t)(mine) * FBN_RS_I] = t;
        if (pe0 >= 0) ps.pend[(size_t)(mine) * FBN_RS_I] = -1;
      }
    }
    if (cs.dup) cs.dup[i] = owner;
    if (cs.hasdup && owner >= 0) cs.hasdup[owner] = 1;
  }
  // stage the constants only where some wave of the block has rows to replay (block-uniform)
  if constexpr (D < 128) {
    const int any = __syncthreads_or(key != 0x7fffffff);
    if (!any) return;
    for (int s = threadIdx.x; s <= t - w0; s += blockDim.x) win[s] = consts4(table[w0 + s]);
    __syncthreads();
  }
  const int cnt = __popcll(__ballot(key != 0x7fffffff));
  if (cnt == 0) return;
  replay_sorted<D, DW>(r, key, pe, cnt, t, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
}
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_claim2_kernel(float* __restrict__ p, float* __restrict__ m,
                                                          float* __restrict__ v, ClaimSrc cs, int n,
                                                          int* __restrict__ last, const AdamConsts* __restrict__ table,
                                                          const int* __restrict__ step, float wd, float b2,
                                                          float omb2, float eps, PendSrc ps) {
  adam_claim2_body<D, DW>(p, m, v, cs, n, last, table, step, wd, b2, omb2, eps, ps, blockIdx.x);
}
// The step's head in one launch: blocks [0, nclaim) make the row claims + claimed-row catch-up
// (adam_claim2_kernel), the rest convert the bf16 images (fbn_convert_bf16: the weights the previous
// step's tail wrote, this batch's item_emb_d128) -- independent work, side by side instead of one
// launch after the other.
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_claim2_conv_kernel(float* __restrict__ p, float* __restrict__ m,
                                                               float* __restrict__ v, ClaimSrc cs, int n,
                                                               int* __restrict__ last,
                                                               const AdamConsts* __restrict__ table,
                                                               const int* __restrict__ step, float wd, float b2,
                                                               float omb2, float eps, PendSrc ps, ConvJobs cj,
                                                               int njobs, int nclaim) {
  if ((int)blockIdx.x < nclaim)
    adam_claim2_body<D, DW>(p, m, v, cs, n, last, table, step, wd, b2, omb2, eps, ps, blockIdx.x);
  else
    convert_tile(cj, njobs, blockIdx.x - nclaim);
}

// The claimed rows' catch-up where the claims were made by another launch (fbn_adam_catchup,
// parts = 1: the owner of the host-split exchange): adam_claim2 without the claim -- entry i of
// [0, n_ent) with slot_row[i] != -1 brings its row (named once) up to the step.
#define FBN_CATCHUP_EPW_WIDE 16
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_catchup_kernel(float* __restrict__ p, float* __restrict__ m,
                                                           float* __restrict__ v, const int* __restrict__ slot_row,
                                                           int n_ent, int F, int* __restrict__ last,
                                                           const AdamConsts* __restrict__ table,
                                                           const int* __restrict__ step, float wd, float b2,
                                                           float omb2, float eps, PendSrc ps) {
  __shared__ f32x4 win[FBN_PF_WIN + 1];
  const int t = *step;
  // every row is within F steps of t (the rolling window): only that many steps' constants are staged
  const int W = F < FBN_PF_WIN ? F : FBN_PF_WIN;
  const int w0 = t > W ? t - W : 0;
  const int lane = threadIdx.x & 63;
  // nearly every entry names a row, so wave-wide rows take FBN_CATCHUP_EPW_WIDE entries per wave (four
  // groups of the engine): four times the waves replaying side by side
  constexpr int EPW = D >= 128 ? FBN_CATCHUP_EPW_WIDE : 64;
  const long long wv = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long i = lane < EPW ? wv * EPW + lane : n_ent;
  int r = 0, key = 0x7fffffff, pe = -1;
  if (i < n_ent) {
    const int sr = slot_row[i];
    const int rr = sr == -1 ? -1 : sr & ~FBN_SLOT_FLAG;
    if (rr >= 0) {
      const int4 rs = row_state(last, rr);
      if (rs.z < t) take_row(r, key, pe, rr, rs, t, last, ps);
    }
  }
  if constexpr (D < 128) {   // as adam_claim2_body: staged only where the block has rows (block-uniform)
    if (!__syncthreads_or(key != 0x7fffffff)) return;
    for (int s = threadIdx.x; s <= t - w0; s += blockDim.x) win[s] = consts4(table[w0 + s]);
    __syncthreads();
  }
  const int cnt = __popcll(__ballot(key != 0x7fffffff));
  if (cnt == 0) return;
  replay_sorted<D, DW>(r, key, pe, cnt, t, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
}

__global__ void __launch_bounds__(256) convert_bf16_kernel_o(ConvJobs jobs, int njobs) {
  convert_tile(jobs, njobs, blockIdx.x);
}

// The rolling window (step mod F) with the replay engine: rpw rows per wave
// (one per lane), so a window of ~1e5 rows (C5's 12.5 M-row shard: 97.7 K rows replaying up to F
// steps each) spreads over thousands of waves instead of one wave per SIMD; claimed rows are left
// to their claiming entry.  With F = 1, chunk = nrows and no map it is the flush: every row up to
// the step (rows further back than FBN_PF_WIN steps read the schedule table itself).
#define FBN_WIN_ROWS 16
template <int D, bool DW>
__device__ __forceinline__ void adam_window2_body(float* __restrict__ p, float* __restrict__ m,
                                                  float* __restrict__ v, const int* __restrict__ map,
                                                  long long nrows, int F, long long chunk, int* __restrict__ last,
                                                  const AdamConsts* __restrict__ table,
                                                  const int* __restrict__ step, float wd, float b2, float omb2,
                                                  float eps, const PendSrc& ps, int rpw, int blk, int nblk) {
  __shared__ f32x4 win[FBN_PF_WIN + 1];   // constants of steps [w0, t]
  const int t = *step;
  const int w0 = t > FBN_PF_WIN ? t - FBN_PF_WIN : 0;
  if constexpr (D < 128)
    for (int s = threadIdx.x; s <= t - w0; s += blockDim.x) win[s] = consts4(table[w0 + s]);
  const long long roll0 = (long long)(t % F) * chunk;
  const long long nroll = roll0 < nrows ? min(chunk, nrows - roll0) : 0;
  const int lane = threadIdx.x & 63;
  if constexpr (D < 128) __syncthreads();   // the LDS window (no barrier after this point)
  // rpw rows per wave; a grid smaller than the row groups walks them wave-strided
  const long long ngrp = (nroll + rpw - 1) / rpw;
  const long long wstride = ((long long)nblk * blockDim.x) >> 6;
  for (long long gq = ((long long)blk * blockDim.x + threadIdx.x) >> 6; gq < ngrp; gq += wstride) {
  const long long j = gq * rpw + lane;
  int r = 0, key = 0x7fffffff, pe = -1;
  if (lane < rpw && j < nroll) {
    const long long rr = roll0 + j;
    const int4 rs = row_state(last, rr);
    if ((!map || map[rr] == -1) && rs.z < t) take_row(r, key, pe, rr, rs, t, last, ps);
  }
  const int cnt = __popcll(__ballot(key != 0x7fffffff));
  if (cnt == 0) continue;
  replay_sorted<D, DW>(r, key, pe, cnt, t, w0, win, p, m, v, table, wd, b2, omb2, eps, ps, lane);
  }
}
template <int D, bool DW>
__global__ void __launch_bounds__(256) adam_window2_kernel(float* __restrict__ p, float* __restrict__ m,
                                                           float* __restrict__ v, const int* __restrict__ map,
                                                           long long nrows, int F, long long chunk,
                                                           int* __restrict__ last, const AdamConsts* __restrict__ table,
                                                           const int* __restrict__ step, float wd, float b2,
                                                           float omb2, float eps, PendSrc ps, int rpw) {
  adam_window2_body<D, DW>(p, m, v, map, nrows, F, chunk, last, table, step, wd, b2, omb2, eps, ps, rpw,
                           blockIdx.x, gridDim.x);
}

// Touched rows: one group per claiming entry e (slot_row[e] = row | FLAG); gradient =
// gvec-slot(e) (+ extra[e]); Adam with the clip coefficient; the row's map entry is reset.
template <int D>
__global__ void __launch_bounds__(256) adam_touched_kernel(float* __restrict__ p, float* __restrict__ m,
                                                           float* __restrict__ v, int* __restrict__ map, GradSrc gs,
                                                           int n, const float* __restrict__ coef_ptr,
                                                           const AdamConsts* __restrict__ table,
                                                           const int* __restrict__ step_ptr, float wd, float b2,
                                                           float omb2, float eps, int* __restrict__ last) {
  resolve_src(gs);
  constexpr int G = D / 4, RPW = 64 / G;
  const AdamConsts k = table[*step_ptr];
  const float coef = coef_ptr ? *coef_ptr : 1.f;
  const int lane = threadIdx.x & 63, q = lane % G;
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long e0 = gw * RPW; e0 < n; e0 += nw * RPW) {
    const long long e = e0 + lane / G;
    if (e >= n) continue;
    const int sr = gs.slot_row[e];
    if (sr == -1) continue;
    const long long r = sr & ~FBN_SLOT_FLAG;
    f32x4 gg = grad4<D>(gs, (int)e, 4 * q);
    if (sr & FBN_SLOT_FLAG) {
      float* ex = gs.extra + (size_t)e * D + 4 * q;
      gg = gs.full ? *reinterpret_cast<const f32x4*>(ex) : gg + *reinterpret_cast<const f32x4*>(ex);
      *reinterpret_cast<f32x4*>(ex) = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const size_t off = (size_t)r * D + 4 * q;
    f32x4 pp = *reinterpret_cast<f32x4*>(p + off);
    f32x4 mm = *reinterpret_cast<f32x4*>(m + off);
    f32x4 vv = *reinterpret_cast<f32x4*>(v + off);
    adam_tab4<true>(pp, mm, vv, gg * coef, wd, b2, omb2, eps, k);
    *reinterpret_cast<f32x4*>(p + off) = pp;
    *reinterpret_cast<f32x4*>(m + off) = mm;
    *reinterpret_cast<f32x4*>(v + off) = vv;
    if (q == 0) {
      map[r] = -1;
      if (last) last[(size_t)(r) * FBN_RS_I] = *step_ptr + 1;
    }
  }
}

// Single-GPU end of step with deferred table gradients: each claiming entry e (row r) either
// records its gradient vector in pend[r] (no duplicates: the gradient is one per-sample vector),
// or -- claimer of a row several entries hit (FLAG) -- applies the step now as adam_touched does.
// map[r] and slot_row[e] are reset; the step's vectors are copied into ring slot step % ring_n and
// the clip coefficient into coef_hist[step].
template <int D>
__device__ __forceinline__ void adam_commit_body(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v,
                                                 int* __restrict__ map, const GradSrc& gs, int n, float coef,
                                                 const AdamConsts& k, int t, float wd, float b2, float omb2, float eps,
                                                 int* __restrict__ last, const PendSrc& ps, int B, long long bid,
                                                 long long nblk) {
  constexpr int G = D / 4, RPW = 64 / G;
  // ring copy of this step's per-sample vectors (N > 1, per-entry rows: the rows were received
  // straight into the ring slot -- nothing to copy; nor when the backward wrote them there itself,
  // fbn_fields_bwd_slot: the source IS the slot)
  float* dst = const_cast<float*>(ps.ring) + (size_t)(t % ps.ring_n) * ps.ring_stride;
  if (gs.Lp1 > 1 && gs.vec != dst) {
    const long long n4 = (long long)B * 2 * D / 4, st = nblk * blockDim.x;
    for (long long i0 = bid * blockDim.x + threadIdx.x; i0 < n4; i0 += 8 * st) {   // 8 loads in flight
      f32x4 x[8];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        x[u] = reinterpret_cast<const f32x4*>(gs.vec)[i0 + u * st < n4 ? i0 + u * st : i0];
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (i0 + u * st < n4) reinterpret_cast<f32x4*>(dst)[i0 + u * st] = x[u];
    }
  }
  // one entry per lane: an unflagged claimer records its vector in pend; flagged claimers (rare)
  // and rows the next batch reads are updated by the wave's G-lane groups afterwards
  const int lane = threadIdx.x & 63, q = lane % G;
  for (long long e0 = (bid * blockDim.x + threadIdx.x) - lane; e0 < n; e0 += nblk * blockDim.x) {
    const long long e = e0 + lane;
    const int sr = e < n ? gs.slot_row[e] : -1;
    const bool flag = sr != -1 && (sr & FBN_SLOT_FLAG);
    bool imm = flag;
    if (sr != -1 && !flag) {
      // a row the NEXT batch also reads (its pre-claim tag is step t + 1: fbn_adam_prefetch's
      // pass for that batch ran during this step) takes step t now, so the next step's claims
      // find it current and replay nothing; the others defer it to their next replay
      if (last && (unsigned)row_state(last, sr).y == (unsigned)(t + 1)) {
        imm = true;
      } else {
        if (gs.Lp1 == 1) {   // per-entry rows (N > 1 owner): the entry's own row of the ring slot
          ps.pend[(size_t)(sr) * FBN_RS_I] = (int)e;
        } else {
          const int b = (int)(e / gs.Lp1), tt = (int)(e - (long long)b * gs.Lp1);
          ps.pend[(size_t)(sr) * FBN_RS_I] = b * 2 + (tt ? 1 : 0);
        }
        map[sr] = -1;
        gs.slot_row[e] = -1;
      }
    }
    unsigned long long mask = __ballot(imm);
    // up to RPW8 of them per round, one per group of D/8 lanes (8 elements each: every load of a
    // round in flight at once)
    constexpr int G8 = D / 8 > 0 ? D / 8 : 1, RPW8 = 64 / G8;
    const int q8 = lane % G8;
    while (mask) {
      int mine = -1;
#pragma unroll
      for (int gi = 0; gi < RPW8; ++gi) {
        if (!mask) break;
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (lane / G8 == gi) mine = l;
      }
      const int sr_l = __shfl(sr, mine < 0 ? 0 : mine, 64);
      if (mine < 0) continue;
      const long long ee = e0 + mine;
      const long long r = sr_l & ~FBN_SLOT_FLAG;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int c = 8 * q8 + 4 * h;
        if (D < 8 && c >= D) break;
        f32x4 gg = grad4<D>(gs, (int)ee, c);
        if (sr_l & FBN_SLOT_FLAG) {   // duplicates folded into extra (the only claimers with one)
          float* ex = gs.extra + (size_t)ee * D + c;
          gg = gs.full ? *reinterpret_cast<const f32x4*>(ex) : gg + *reinterpret_cast<const f32x4*>(ex);
          *reinterpret_cast<f32x4*>(ex) = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
        const size_t off = (size_t)r * D + c;
        f32x4 pp = *reinterpret_cast<f32x4*>(p + off);
        f32x4 mm = *reinterpret_cast<f32x4*>(m + off);
        f32x4 vv = *reinterpret_cast<f32x4*>(v + off);
        adam_tab4<true>(pp, mm, vv, gg * coef, wd, b2, omb2, eps, k);
        *reinterpret_cast<f32x4*>(p + off) = pp;
        *reinterpret_cast<f32x4*>(m + off) = mm;
        *reinterpret_cast<f32x4*>(v + off) = vv;
      }
      if (q8 == 0) {
        map[r] = -1;
        last[(size_t)(r) * FBN_RS_I] = t + 1;
        gs.slot_row[ee] = -1;
      }
    }
  }
}

// Single-GPU end of step with deferred table gradients: each claiming entry e (row r) either
// records its gradient vector in pend[r] (no duplicates: the gradient is one per-sample vector),
// or -- claimer of a row several entries hit (FLAG) -- applies the step now as adam_touched does.
// map[r] and slot_row[e] are reset; the step's vectors are copied into ring slot step % ring_n and
// the clip coefficient into coef_hist[step].
template <int D>
__global__ void __launch_bounds__(256) adam_commit_kernel(float* __restrict__ p, float* __restrict__ m,
                                                          float* __restrict__ v, int* __restrict__ map, GradSrc gs,
                                                          int n, const float* __restrict__ coef_ptr,
                                                          const AdamConsts* __restrict__ table,
                                                          const int* __restrict__ step_ptr, float wd, float b2,
                                                          float omb2, float eps, int* __restrict__ last, PendSrc ps,
                                                          float* __restrict__ coef_hist, int B) {
  resolve_src(gs);
  const int t = *step_ptr;
  const AdamConsts k = table[t];
  const float coef = coef_ptr ? *coef_ptr : 1.f;
  if (blockIdx.x == 0 && threadIdx.x == 0) coef_hist[t] = coef;
  adam_commit_body<D>(p, m, v, map, gs, n, coef, k, t, wd, b2, omb2, eps, last, ps, B, blockIdx.x, gridDim.x);
}

// The whole single-GPU step tail in ONE launch (each kernel boundary costs a few microseconds):
// blocks [0, ndense) run the dense Adam (clip coefficient from the norm slots, as adam_dense),
// the rest the deferred-gradient commit; the last block to finish (ticket counter) advances the
// step, the dropout offset and num_batches_tracked and clears the norm slots (fbn_step_end).
#define FBN_TICKET_GROUPS 16   // fbn_adam_step_tail: ticket is [1 + FBN_TICKET_GROUPS] words
static_assert(1 + FBN_TICKET_GROUPS == FBN_TICKET_WORDS, "the ticket words the header tells the caller to allocate");
struct StepEnd {
  int* step;
  unsigned long long* rng;
  double* sumsq;
  long long* nbt0;
  long long* nbt1;
  unsigned* ticket;   // [1 + FBN_TICKET_GROUPS], zero at rest; the last block of each level resets its word
  int max_step;       // total_steps: the counter saturates there (schedule table / coef_hist bounds)
  int* err;           // bit 2 set on a step past max_step (graph replays cannot raise on the host)
};
template <int D>
__global__ void __launch_bounds__(256) adam_tail_kernel(float* __restrict__ dp, const float* __restrict__ dg,
                                                        float* __restrict__ dm, float* __restrict__ dv,
                                                        long long ndense_elems, int ndense, float max_norm,
                                                        float* coef_out, float* norm_out, float* __restrict__ p,
                                                        float* __restrict__ m, float* __restrict__ v,
                                                        int* __restrict__ map, GradSrc gs, int n,
                                                        const AdamConsts* __restrict__ table, float wd, float b2,
                                                        float omb2, float eps, int* __restrict__ last, PendSrc ps,
                                                        float* __restrict__ coef_hist, int B, StepEnd se) {
  resolve_src(gs);
  __shared__ float sc;
  __shared__ unsigned is_last;
  const int t = *se.step;
  const AdamConsts k = table[t];
  if (threadIdx.x == 0) {
    float total;
    sc = clip_from_slots(se.sumsq, max_norm, &total);
    if (blockIdx.x == 0) {
      if (coef_out) *coef_out = sc;
      if (norm_out) *norm_out = total;
      coef_hist[t] = sc;
    }
  }
  __syncthreads();
  const float coef = sc;
  if ((int)blockIdx.x < ndense)
    adam_dense_body(dp, dg, dm, dv, ndense_elems, coef, k, wd, b2, omb2, eps, blockIdx.x, ndense);
  else
    adam_commit_body<D>(p, m, v, map, gs, n, coef, k, t, wd, b2, omb2, eps, last, ps, B, blockIdx.x - ndense,
                        gridDim.x - ndense);
  // Every block consumed its reads of step and the norm slots (above) before it draws its ticket,
  // and the last block publishes nothing another block of this launch reads: a relaxed ticket
  // needs no release/acquire fences (an agent-scope release writes back the XCD's L2 -- in every
  // block that costs tens of microseconds).  The next launch sees the stores at the kernel boundary.
  // Two-level ticket (ticket[1 + g] for the blocks with blockIdx % FBN_TICKET_GROUPS == g, then
  // ticket[0] once per group): a returning atomic on one word serialises at ~88 per microsecond,
  // so hundreds of blocks on one word alone would add microseconds to the tail.
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ng = min((unsigned)FBN_TICKET_GROUPS, gridDim.x), g = blockIdx.x % ng;
    const unsigned in_g = (gridDim.x - g + ng - 1) / ng;   // blocks of group g
    bool last = false;
    if (__hip_atomic_fetch_add(se.ticket + 1 + g, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == in_g - 1) {
      se.ticket[1 + g] = 0u;
      last = __hip_atomic_fetch_add(se.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == ng - 1;
    }
    is_last = last;
  }
  __syncthreads();
  if (is_last && threadIdx.x == 0) {
    if (t + 1 <= se.max_step) se.step[0] = t + 1;
    else if (se.err) atomicOr(se.err, 2);
    if (se.rng) se.rng[1] += 1;
    if (se.nbt0) se.nbt0[0] += 1;
    if (se.nbt1) se.nbt1[0] += 1;
    for (int i = 0; i < FBN_SUMSQ_SLOTS; ++i) se.sumsq[i] = 0.0;
    *se.ticket = 0u;
  }
}

// end of step: advance Adam step + dropout RNG offset, clear the norm accumulator
__global__ void step_end_kernel(int* step, unsigned long long* rng, double* sumsq, long long* nbt0, long long* nbt1,
                                int max_step, int* err) {
  if (step[0] + 1 <= max_step) step[0] += 1;
  else if (err) atomicOr(err, 2);   // past total_steps: the counter saturates (table bounds), flag it
  if (rng) rng[1] += 1;
  if (nbt0) nbt0[0] += 1;   // BatchNorm num_batches_tracked
  if (nbt1) nbt1[0] += 1;
  if (sumsq)
    for (int i = 0; i < FBN_SUMSQ_SLOTS; ++i) sumsq[i] = 0.0;
}

// ------------------------------------------------------------------ C ABI
extern "C" int fbn_sumsq(const float* x, long long n, const int* n_rows, int row_len, double* out, void* stream) {
  if (n <= 0 && !n_rows) return FBN_OK;
  fbn_launch(sumsq_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, x, n, n_rows, row_len, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_clip_coef(const double* sumsq, float max_norm, float* coef, float* norm, void* stream) {
  fbn_launch(clip_coef_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, sumsq, max_norm, coef, norm);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_adam_dense(float* p, const float* g, float* m, float* v, long long n, const float* coef,
                              const void* consts_table, const int* step, float wd, float beta2, float eps,
                              const double* sumsq, float max_norm, float* coef_out, float* norm_out, void* stream) {
  if (n <= 0) return FBN_OK;
  if (((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) {
    fbn_set_error("adam_dense: 16-byte alignment required");
    return FBN_ERR_ARG;
  }
  long long blocks = (n / 4 + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  if (blocks < 1) blocks = 1;
  fbn_launch(adam_dense_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, coef,
                     (const AdamConsts*)consts_table, step, wd, beta2, (float)(1.0 - (double)beta2), eps, sumsq,
                     max_norm, coef_out, norm_out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

#define FBN_DISPATCH_D(KERNEL, D, GRID, ...)                                                         \
  switch (D) {                                                                                      \
    case 16: fbn_launch((KERNEL<16>), GRID, dim3(256), 0, st, __VA_ARGS__); break;          \
    case 32: fbn_launch((KERNEL<32>), GRID, dim3(256), 0, st, __VA_ARGS__); break;          \
    case 64: fbn_launch((KERNEL<64>), GRID, dim3(256), 0, st, __VA_ARGS__); break;          \
    case 128: fbn_launch((KERNEL<128>), GRID, dim3(256), 0, st, __VA_ARGS__); break;        \
    case 256: fbn_launch((KERNEL<256>), GRID, dim3(256), 0, st, __VA_ARGS__); break;        \
    default: fbn_set_error("D must be 16/32/64/128/256"); return FBN_ERR_UNSUPPORTED;              \
  }

// the same with a block size of T threads
#define FBN_DISPATCH_D_T(KERNEL, D, GRID, T, ...)                                                    \
  switch (D) {                                                                                      \
    case 16: fbn_launch((KERNEL<16>), GRID, dim3(T), 0, st, __VA_ARGS__); break;            \
    case 32: fbn_launch((KERNEL<32>), GRID, dim3(T), 0, st, __VA_ARGS__); break;            \
    case 64: fbn_launch((KERNEL<64>), GRID, dim3(T), 0, st, __VA_ARGS__); break;            \
    case 128: fbn_launch((KERNEL<128>), GRID, dim3(T), 0, st, __VA_ARGS__); break;          \
    case 256: fbn_launch((KERNEL<256>), GRID, dim3(T), 0, st, __VA_ARGS__); break;          \
    default: fbn_set_error("D must be 16/32/64/128/256"); return FBN_ERR_UNSUPPORTED;              \
  }

// the same for a kernel templated on <D, bool>
#define FBN_DISPATCH_D_B(KERNEL, B, D, GRID, ...)                                                    \
  switch (D) {                                                                                      \
    case 16: fbn_launch((KERNEL<16, B>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    case 32: fbn_launch((KERNEL<32, B>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    case 64: fbn_launch((KERNEL<64, B>), GRID, dim3(256), 0, st, __VA_ARGS__); break;       \
    case 128: fbn_launch((KERNEL<128, B>), GRID, dim3(256), 0, st, __VA_ARGS__); break;     \
    case 256: fbn_launch((KERNEL<256, B>), GRID, dim3(256), 0, st, __VA_ARGS__); break;     \
    default: fbn_set_error("D must be 16/32/64/128/256"); return FBN_ERR_UNSUPPORTED;              \
  }

static dim3 group_grid(long long n, int D, long long cap) {
  const int rpw = 256 / D;
  long long blocks = ((n + rpw - 1) / rpw + 3) / 4;
  if (blocks < 1) blocks = 1;
  if (blocks > cap) blocks = cap;
  return dim3((unsigned)blocks);
}

// N > 1 owner, deferred table gradients: the received gradient rows (wire: n floats, bf16 or f32)
// widened / copied into ring slot step % ring_n, whose address goes to *cell (read by the fold,
// the norm and the step tail through FBN_GRAD_CELL).  Floats [self_lo, self_lo + self_n) come from
// wire_self instead (the caller's own block of the fixed-capacity exchange: the requester's send
// buffer, never sent through RCCL).
__global__ void __launch_bounds__(256) ring_slot_kernel(float* __restrict__ ring, int ring_n, long long stride,
                                                        const int* __restrict__ step, float** __restrict__ cell,
                                                        const void* __restrict__ wire, int wire_bf16, long long n8,
                                                        const void* __restrict__ wire_self, long long self_lo8,
                                                        long long self_n8) {
  float* dst = ring + (size_t)(*step % ring_n) * stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) *cell = dst;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (long long)gridDim.x * blockDim.x) {
    const void* src = (wire_self && i >= self_lo8 && i < self_lo8 + self_n8) ? wire_self : wire;
    f32x4 a, b;
    if (wire_bf16) {
      const bf16x8 v = reinterpret_cast<const bf16x8*>(src)[i];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        a[k] = __uint_as_float((unsigned)(unsigned short)v[k] << 16);
        b[k] = __uint_as_float((unsigned)(unsigned short)v[k + 4] << 16);
      }
    } else {
      a = reinterpret_cast<const f32x4*>(src)[2 * i];
      b = reinterpret_cast<const f32x4*>(src)[2 * i + 1];
    }
    reinterpret_cast<f32x4*>(dst)[2 * i] = a;
    reinterpret_cast<f32x4*>(dst)[2 * i + 1] = b;
  }
}

extern "C" int fbn_ring_slot(float* ring, int ring_n, long long stride, const int* step, void* cell, const void* wire,
                             int wire_bf16, long long n, const void* wire_self, long long self_lo, long long self_n,
                             void* stream) {
  if (ring_n & FBN_RING_BF16) {
    fbn_set_error("fbn_ring_slot: f32 rings only (a bf16 ring is filled by fbn_owner_fold)");
    return FBN_ERR_ARG;
  }
  if (!ring || !step || !cell || ring_n < 1 || n < 0 || n > stride || (n & 7) || (n > 0 && !wire) ||
      ((uintptr_t)ring & 15) || (stride & 7) || ((uintptr_t)wire & 15) || ((uintptr_t)wire_self & 15) ||
      (self_lo & 7) || (self_n & 7) || self_lo < 0 || self_n < 0 || self_lo + self_n > n ||
      (self_n > 0 && !wire_self)) {
    fbn_set_error("fbn_ring_slot: ring, step, cell; n, self_lo, self_n % 8 == 0, n <= stride, 16-B aligned buffers");
    return FBN_ERR_ARG;
  }
  long long blocks = (n / 8 + 255) / 256;
  if (blocks < 1) blocks = 1;
  if (blocks > 8192) blocks = 8192;
  fbn_launch(ring_slot_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, ring, ring_n, stride, step,
             (float**)cell, wire, wire_bf16, n / 8, self_n > 0 ? wire_self : nullptr, self_lo / 8, self_n / 8);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// N > 1 owner, the fixed-capacity exchange: the widen into the ring slot and the duplicate fold in ONE
// pass.  Received slot e (local row ids[e]; negative = empty, rank 0's row 0 = padding: skipped):
// the claimer of its row (map[row] == e) stores its widened row into ring slot step % ring_n (its
// address to *cell, as fbn_ring_slot); a duplicate adds its row into extra[claimer] (zero at rest)
// and flags the claimer (FBN_SLOT_FLAG), as the single-GPU fold does -- the norm and the step tail
// read claimer + extra (Lp1 | FBN_GRAD_CELL with extra), and a flagged claimer's step is applied at
// the tail, which zeroes its extra row.  Rows [self_lo, self_lo + self_n) come from wire_self.
template <int D>
__global__ void __launch_bounds__(256) owner_fold_kernel(const int* __restrict__ ids, int n, int rank,
                                                         const int* __restrict__ map, int* __restrict__ slot_row,
                                                         const void* __restrict__ wire, int wire_bf16,
                                                         const void* __restrict__ wire_self, long long self_lo,
                                                         long long self_n, float* __restrict__ ring, int ring_n,
                                                         long long stride, const int* __restrict__ step,
                                                         float** __restrict__ cell, float* __restrict__ extra,
                                                         double* __restrict__ part,
                                                         unsigned long long* __restrict__ fx, int ring_bf16) {
  constexpr int G = D / 4, RPW = 64 / G;
  __shared__ double red[256];
  // (a bf16 ring: `stride` and the row offsets count bf16 elements; the slot address is still a float*)
  float* dst = ring_bf16 ? reinterpret_cast<float*>(reinterpret_cast<short*>(ring) + (size_t)(*step % ring_n) * stride)
                         : ring + (size_t)(*step % ring_n) * stride;
  if (blockIdx.x == 0 && threadIdx.x == 0) *cell = dst;
  const int lane = threadIdx.x & 63, q = lane % G;
  double acc = 0.0;   // sumsq: the claimers' own rows (a flagged claimer's duplicates: fbn_sumsq_flagged)
  const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const long long nw = ((long long)gridDim.x * blockDim.x) >> 6;
  for (long long e0 = gw * RPW; e0 < n; e0 += nw * RPW) {
    const long long e = e0 + lane / G;
    if (e >= n) continue;
    const int r = ids[e];
    if (r < 0 || (rank == 0 && r == 0)) continue;
    const int u = map[r];
    if (u < 0) continue;
    const void* src = (wire_self && e >= self_lo && e < self_lo + self_n) ? wire_self : wire;
    f32x4 x;
    bf16x4 h;
    if (wire_bf16) {
      h = reinterpret_cast<const bf16x4*>(src)[(size_t)e * (D / 4) + q];
#pragma unroll
      for (int k = 0; k < 4; ++k) x[k] = __uint_as_float((unsigned)(unsigned short)h[k] << 16);
    } else {
      x = reinterpret_cast<const f32x4*>(src)[(size_t)e * (D / 4) + q];
    }
    if (u == (int)e) {
      if (ring_bf16)   // the wire's bf16 bits as they are (half the bytes of the widened f32 row)
        reinterpret_cast<bf16x4*>(dst)[(size_t)e * (D / 4) + q] = h;
      else
        reinterpret_cast<f32x4*>(dst)[(size_t)e * (D / 4) + q] = x;
      acc += (double)(x[0] * x[0]) + (double)(x[1] * x[1]) + (double)(x[2] * x[2]) + (double)(x[3] * x[3]);
    } else {
      if (q == 0) atomicOr(&slot_row[u], FBN_SLOT_FLAG);
      if (fx) {
        // deterministic mode: int64 fixed-point sums (as fbn_sparse_fold_fx) -- the total depends
        // neither on the order the atomics land in nor on which entry won the claim
        unsigned long long* a = fx + (size_t)u * D + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(a + k, (unsigned long long)to_fx(x[k]));
      } else {
        float* ex = extra + (size_t)u * D + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k) atomicAdd(ex + k, x[k]);
      }
    }
  }
  if (!part) return;
  // one partial per block (no atomics: thousands of blocks on 64 slots serialise at L2);
  // fbn_sumsq_flagged folds them
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

// After fbn_owner_fold(sumsq): the flagged claimers' correction |x + extra|^2 - |x|^2 (x = the claimer's
// own row in the ring slot, extra = its duplicates' sum): one lane per entry scans slot_row, the
// (rare) flagged rows are read by D/4-lane groups.  fx (deterministic mode): the duplicates' sums are
// in the fixed-point accumulator instead; the claimer's own row joins them there and extra[claimer]
// becomes the row's FULL gradient, float(total) -- the same integer total, hence the same float, as the
// single-GPU deterministic fold (fbn_sparse_fold_fx + fbn_sumsq_sparse_norms) on the same entries --
// and the accumulator row is reset.
template <int D>
__global__ void __launch_bounds__(256) sumsq_flagged_kernel(const int* __restrict__ slot_row, int n,
                                                            float* const* __restrict__ cell,
                                                            float* __restrict__ extra,
                                                            const double* __restrict__ part, int nparts,
                                                            double* __restrict__ sumsq,
                                                            unsigned long long* __restrict__ fx, int ring_bf16) {
  constexpr int G = D / 4, RPW = 64 / G;
  __shared__ double red[256];
  const float* src = *cell;
  const int lane = threadIdx.x & 63, q = lane % G;
  double acc = 0.0;
  if (part)
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nparts; i += gridDim.x * blockDim.x) acc += part[i];
  for (long long e0 = (long long)blockIdx.x * blockDim.x + threadIdx.x - lane; e0 < n;
       e0 += (long long)gridDim.x * blockDim.x) {
    const long long e = e0 + lane;
    const int sr = e < n ? slot_row[e] : -1;
    unsigned long long mask = __ballot(sr != -1 && (sr & FBN_SLOT_FLAG));
    while (mask) {
      int mine = -1;
#pragma unroll
      for (int gi = 0; gi < RPW; ++gi) {
        if (!mask) break;
        const int l = __ffsll((long long)mask) - 1;
        mask &= mask - 1;
        if (lane / G == gi) mine = l;
      }
      if (mine < 0) continue;
      const long long ee = e0 + mine;
      const f32x4 x = ring_load<f32x4, 4>(src, ring_bf16, (size_t)ee * D + 4 * q);
      f32x4 t;
      if (fx) {
        unsigned long long* a = fx + (size_t)ee * D + 4 * q;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const long long tot = (long long)(a[k] + (unsigned long long)to_fx(x[k]));
          t[k] = (float)((double)tot * (1.0 / 1099511627776.0));
          a[k] = 0ull;
        }
        *reinterpret_cast<f32x4*>(extra + (size_t)ee * D + 4 * q) = t;
      } else {
        t = x + *reinterpret_cast<const f32x4*>(extra + (size_t)ee * D + 4 * q);
      }
#pragma unroll
      for (int k = 0; k < 4; ++k) acc += (double)(t[k] * t[k]) - (double)(x[k] * x[k]);
    }
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) atomicAdd(sumsq + (blockIdx.x & (FBN_SUMSQ_SLOTS - 1)), red[0]);
}

#define FBN_FOLD_PARTS 8192   // fbn_owner_fold's block cap = its partial sums of squares
extern "C" int fbn_owner_fold(const int* ids, int n, int rank, const int* map, int* slot_row, const void* wire,
                              int wire_bf16, const void* wire_self, long long self_lo, long long self_n, float* ring,
                              int ring_n, long long stride, const int* step, void* cell, float* extra, int D,
                              double* part, unsigned long long* fx, void* stream) {
  if (n <= 0) return FBN_OK;
  const int ring_bf16 = (ring_n & FBN_RING_BF16) ? 1 : 0;
  ring_n &= ~FBN_RING_BF16;
  if (!ids || !map || !slot_row || !wire || !ring || !step || !cell || !extra || ring_n < 1 ||
      (long long)n * D > stride || self_lo < 0 || self_n < 0 || (self_n > 0 && !wire_self) ||
      (ring_bf16 && !wire_bf16)) {
    fbn_set_error("fbn_owner_fold: ids, map, slot_row, wire, ring, step, cell, extra; n * D <= stride; a bf16 ring "
                  "takes bf16 wire rows");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  FBN_DISPATCH_D(owner_fold_kernel, D, group_grid(n, D, FBN_FOLD_PARTS), ids, n, rank, map, slot_row, wire,
                 wire_bf16, self_n > 0 ? wire_self : nullptr, self_lo, self_n, ring, ring_n, stride, step,
                 (float**)cell, extra, part, fx, ring_bf16);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_sumsq_flagged(const int* slot_row, int n, const void* cell, float* extra, int D,
                                 const double* part, double* sumsq, unsigned long long* fx, int ring_bf16,
                                 void* stream) {
  if (n <= 0) return FBN_OK;
  if (!slot_row || !cell || !extra || !sumsq) {
    fbn_set_error("fbn_sumsq_flagged: slot_row, cell, extra, sumsq");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  int blocks = (n + 255) / 256;
  // deterministic mode: at most one block per norm slot, so each slot takes one addition (onto the
  // zero the previous step's pack left) and the f64 total does not depend on the blocks' order
  if (blocks > (fx ? FBN_SUMSQ_SLOTS : 1024)) blocks = fx ? FBN_SUMSQ_SLOTS : 1024;
  const int nparts = part ? (int)group_grid(n, D, FBN_FOLD_PARTS).x : 0;   // fbn_owner_fold's grid on the same n
  FBN_DISPATCH_D(sumsq_flagged_kernel, D, dim3(blocks), slot_row, n, (float* const*)cell, extra, part, nparts, sumsq,
                 fx, ring_bf16);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// gvec: single GPU per-sample vectors [B][2][D] (Lp1 = L+1) or owner per-entry rows [n][D] (Lp1 = 1)
extern "C" int fbn_sparse_fixup(const int64_t* item, const int64_t* seq, const int* ids, int n, int L, long long V,
                                int rank, const int* map, const float* gvec, float* extra, int* slot_row, int Lp1,
                                int D, void* stream) {
  if (n <= 0) return FBN_OK;
  if (Lp1 & FBN_GRAD_BF16) {
    fbn_set_error("fbn_sparse_fixup: f32 rows only (bf16 rows are folded by fbn_owner_fold)");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  FBN_DISPATCH_D(sparse_fixup_kernel, D, group_grid(n, D, 8192), item, L > 0 ? seq : nullptr, ids, n, L, V, rank,
                 map, s);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// single GPU: the fix-up from claim-time duplicates (fbn_claim_rows' dup), then the table
// gradient's sum of squares from fbn_fields_bwd's per-sample norms
extern "C" int fbn_sparse_fixup_dup(const int* dup, int n, const float* gvec, float* extra, int* slot_row, int Lp1,
                                    int D, void* stream) {
  if (n <= 0) return FBN_OK;
  if (!dup || !extra) { fbn_set_error("fbn_sparse_fixup_dup: dup and extra are required"); return FBN_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  const int per = FBN_FOLD_THREADS * FBN_FOLD_CHUNKS;
  const int blocks = (n + per - 1) / per;
  FBN_DISPATCH_D_T(sparse_fixup_dup_kernel, D, dim3(blocks), FBN_FOLD_THREADS, dup, n, s);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_sparse_fold_fx(const int* dup, int* hasdup, int n, const float* gvec, int* slot_row, int Lp1, int D,
                                  unsigned long long* acc, void* stream) {
  if (n <= 0) return FBN_OK;
  if (!dup || !hasdup || !acc || (Lp1 & 0xffff) < 2) {
    fbn_set_error("fbn_sparse_fold_fx: dup, hasdup, acc and per-sample vectors (Lp1 >= 2) are required");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const GradSrc s = make_src(gvec, nullptr, slot_row, Lp1);
  int blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  FBN_DISPATCH_D(sparse_fold_fx_kernel, D, dim3(blocks), dup, hasdup, n, s, acc);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_sumsq_sparse_norms(const double* gnorm, const float* gvec, float* extra, int* slot_row, int Lp1,
                                      int n, int D, double* out, unsigned long long* fx, const float* dense,
                                      long long n_dense, void* stream) {
  if (n <= 0) return FBN_OK;
  if (dense ? (n_dense < 0 || (n_dense & 3) || ((uintptr_t)dense & 15)) : n_dense != 0) {
    fbn_set_error("fbn_sumsq_sparse_norms: dense needs n_dense % 4 == 0 and 16-byte alignment");
    return FBN_ERR_ARG;
  }
  if ((Lp1 & 0xffff) < 2) { fbn_set_error("fbn_sumsq_sparse_norms: per-sample vectors only (Lp1 >= 2)"); return FBN_ERR_ARG; }
  hipStream_t st = (hipStream_t)stream;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  int blocks = (n + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  FBN_DISPATCH_D(sumsq_norms_kernel, D, dim3(blocks), s, gnorm, n, out, fx, dense, dense ? n_dense : 0);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_sumsq_sparse(const float* gvec, float* extra, int* slot_row, int Lp1, int n, int D, double* out,
                                void* stream) {
  if (n <= 0) return FBN_OK;
  hipStream_t st = (hipStream_t)stream;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  FBN_DISPATCH_D(sumsq_sparse_kernel, D, group_grid(n, D, 4096), s, n, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// mode 0: every row (touched rows read their gradient through the map and are reset);
// mode 1: untouched rows only (g = 0, coefficient-independent; run it concurrently with the
// backward, then fbn_adam_touched once the clip coefficient is known), throttled to 512
// workgroups so it leaves CUs to the backward; mode 2: as mode 1 on the full grid (serial use)
extern "C" int fbn_adam_table(float* p, float* m, float* v, long long nrows, int D, int* map, const float* gvec,
                              float* extra, int* slot_row, int Lp1, const float* coef, const void* consts_table,
                              const int* step, float wd, float beta2, float eps, int mode, void* stream) {
  if (nrows <= 0) return FBN_OK;
  hipStream_t st = (hipStream_t)stream;
  const float omb2 = (float)(1.0 - (double)beta2);
  const AdamConsts* t = (const AdamConsts*)consts_table;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  const dim3 grid = mode == 1 ? dim3(512) : group_grid(nrows, D, 16384);
  if (mode == 1 || mode == 2) {
    FBN_DISPATCH_D(adam_table_untouched, D, grid, p, m, v, nrows, map, s, coef, t, step, wd, beta2, omb2, eps);
  } else {
    FBN_DISPATCH_D(adam_table_all, D, grid, p, m, v, nrows, map, s, coef, t, step, wd, beta2, omb2, eps);
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_adam_touched(float* p, float* m, float* v, int D, int* map, const float* gvec, float* extra,
                                int* slot_row, int Lp1, int n, const float* coef, const void* consts_table,
                                const int* step, float wd, float beta2, float eps, int* last, void* stream) {
  if (n <= 0) return FBN_OK;
  hipStream_t st = (hipStream_t)stream;
  const float omb2 = (float)(1.0 - (double)beta2);
  const AdamConsts* t = (const AdamConsts*)consts_table;
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  FBN_DISPATCH_D(adam_touched_kernel, D, group_grid(n, D, 8192), p, m, v, map, s, n, coef, t, step, wd, beta2,
                 omb2, eps, last);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// single GPU, lazy table Adam with deferred gradients: see adam_commit_kernel.  ring: [ring_n][B][2][D]
extern "C" int fbn_adam_commit(float* p, float* m, float* v, int D, int* map, const float* gvec, float* extra,
                               int* slot_row, int Lp1, int n, const float* coef, const void* consts_table,
                               const int* step, float wd, float beta2, float eps, int* last, int* pend, float* ring,
                               float* coef_hist, int ring_n, int B, void* stream) {
  if (n <= 0) return FBN_OK;
  if (!pend || !ring || !coef_hist || !extra || ring_n < 2 || (Lp1 & 0xffff) < 2 || (ring_n & FBN_RING_BF16)) {
    fbn_set_error("fbn_adam_commit: pend, ring, coef_hist and extra are required (single-GPU layout, f32 ring)");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const float omb2 = (float)(1.0 - (double)beta2);
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  const PendSrc ps = make_pend(pend, ring, coef_hist, (long long)B * 2 * D, ring_n);
  int blocks = (n + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  FBN_DISPATCH_D(adam_commit_kernel, D, dim3(blocks), p, m, v, map, s, n, coef,
                 (const AdamConsts*)consts_table, step, wd, beta2, omb2, eps, last, ps, coef_hist, B);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// single-GPU step tail: dense Adam (+ clip) + deferred-gradient commit + step end in one launch.
// ticket: one device unsigned, zero before the first call (the kernel leaves it zero).
extern "C" int fbn_adam_step_tail(float* dp, const float* dg, float* dm, float* dv, long long n_dense,
                                  const double* sumsq, float max_norm, float* coef_out, float* norm_out, float* p,
                                  float* m, float* v, int D, int* map, const float* gvec, float* extra, int* slot_row,
                                  int Lp1, int n, const void* consts_table, int* step, float wd, float beta2, float eps,
                                  int* last, int* pend, float* ring, float* coef_hist, int ring_n, long long ring_stride,
                                  int B, unsigned long long* rng, long long* nbt0, long long* nbt1, unsigned* ticket,
                                  int max_step, int* err, void* stream) {
  const int lp = Lp1 & 0xffff;
  if (!pend || !ring || !coef_hist || !sumsq || !ticket || ring_n < 2 || lp < 1 || (lp >= 2 && !extra) ||
      (lp >= 2 && ring_stride != (long long)B * 2 * D) || (lp >= 2 && (ring_n & FBN_RING_BF16))) {
    fbn_set_error("fbn_adam_step_tail: pend, ring, coef_hist, sumsq, ticket (and extra with per-sample vectors, "
                  "ring_stride = B*2*D) are required");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const float omb2 = (float)(1.0 - (double)beta2);
  const GradSrc s = make_src(gvec, extra, slot_row, Lp1);
  const PendSrc ps = make_pend(pend, ring, coef_hist, ring_stride, ring_n);
  const StepEnd se{step, rng, (double*)sumsq, nbt0, nbt1, ticket, max_step, err};
  long long nd = (n_dense / 4 + 255) / 256;
  // block caps (every block draws the step-end ticket; two-level, so ~16x less contention than
  // one word)
  const long long cap_d = 256, cap_c = 1024;   // A/B: nc 1024 -5 us
  if (nd > cap_d) nd = cap_d;
  if (nd < 1) nd = 1;
  long long nc = ((long long)(n > 0 ? n : 1) + 255) / 256;
  if (nc > cap_c) nc = cap_c;
  if (nc < 1) nc = 1;
  FBN_DISPATCH_D(adam_tail_kernel, D, dim3((unsigned)(nd + nc)), dp, dg, dm, dv, n_dense, (int)nd, max_norm, coef_out,
                 norm_out, p, m, v, map, s, n, (const AdamConsts*)consts_table, wd, beta2, omb2, eps, last, ps,
                 coef_hist, B, se);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_claim_rows(const int64_t* item, const int64_t* seq, int B, int L, long long V, int* map,
                              int* slot_row, int* dup, int* hasdup, void* stream) {
  const long long n = (long long)B * (L + 1);
  if (n <= 0) return FBN_OK;
  int blocks = (int)((n + 255) / 256);
  if (blocks > 4096) blocks = 4096;
  fbn_launch(claim_rows_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, item, L > 0 ? seq : nullptr,
                     B, L, V, map, slot_row, dup, hasdup);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_step_end(int* step, unsigned long long* rng, double* sumsq, long long* nbt0, long long* nbt1,
                            int max_step, int* err, void* stream) {
  fbn_launch(step_end_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, step, rng, sumsq, nbt0, nbt1,
                     max_step, err);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}


// ---- lazy table Adam, the entry points.  Each ends in the same replay arguments (last,
// consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride, ring_n, decoupled): packed
// once into a ReplayArgs, whose kernel arguments FBN_RA spells in the kernels' order.
struct ReplayArgs {
  int* last;
  const AdamConsts* table;
  const int* step;
  float wd, beta2, omb2, eps;
  PendSrc ps;
  int decoupled;
};
static inline ReplayArgs make_replay(int* last, const void* consts_table, const int* step, float wd, float beta2,
                                     float eps, int* pend, const float* ring, const float* coef_hist,
                                     long long ring_stride, int ring_n, int decoupled) {
  return ReplayArgs{last, (const AdamConsts*)consts_table, step, wd, beta2, (float)(1.0 - (double)beta2), eps,
                    make_pend(pend, ring, coef_hist, ring_stride, ring_n), decoupled};
}
#define FBN_RA(ra) (ra).last, (ra).table, (ra).step, (ra).wd, (ra).beta2, (ra).omb2, (ra).eps, (ra).ps

// The checks every entry point makes on them: deferred gradients (pend) need their ring and
// coef_hist, and an entry point with a window F (has_F) needs 1 <= F <= FBN_LAZY_MAX_LAG and a ring
// of more than F steps (ring_n as passed, flag bits included).  false: the error text is set.
static bool replay_args_ok(const char* who, bool has_F, int F, const int* pend, const float* ring,
                           const float* coef_hist, int ring_n) {
  char msg[160];
  if (has_F && (F < 1 || F > FBN_LAZY_MAX_LAG)) {
    snprintf(msg, sizeof(msg), "%s: 1 <= F <= %d", who, FBN_LAZY_MAX_LAG);
  } else if (pend && (!ring || !coef_hist || (has_F && ring_n <= F))) {
    snprintf(msg, sizeof(msg), "%s: deferred gradients (pend) need ring and coef_hist%s", who,
             has_F ? ", and ring_n > F" : "");
  } else {
    return true;
  }
  fbn_set_error(msg);
  return false;
}

// a kernel templated on <D, decoupled>: every D, or the wave-wide rows only (D checked by the caller)
#define FBN_DISPATCH_D_DW(KERNEL, DW, D, GRID, ...)                                                  \
  if (DW) { FBN_DISPATCH_D_B(KERNEL, true, D, GRID, __VA_ARGS__) }                                   \
  else { FBN_DISPATCH_D_B(KERNEL, false, D, GRID, __VA_ARGS__) }
#define FBN_DISPATCH_WIDE_DW(KERNEL, DW, D, GRID, ...)                                               \
  if (D == 128) {                                                                                   \
    if (DW) fbn_launch((KERNEL<128, true>), GRID, dim3(256), 0, st, __VA_ARGS__);                   \
    else fbn_launch((KERNEL<128, false>), GRID, dim3(256), 0, st, __VA_ARGS__);                     \
  } else {                                                                                          \
    if (DW) fbn_launch((KERNEL<256, true>), GRID, dim3(256), 0, st, __VA_ARGS__);                   \
    else fbn_launch((KERNEL<256, false>), GRID, dim3(256), 0, st, __VA_ARGS__);                     \
  }

// The rolling window's launch over rows [roll0, roll0 + chunk) of window (step mod F) -- and, with
// F = 1 and no map, the flush of the whole table.  Rows per wave: wave-wide rows take 8, so more
// waves replay side by side; below d = 128 a window takes 16 (one round of the narrow engine: a
// window is small) and the flush a row per lane, on a capped grid that walks the table wave-strided.
static int launch_window(float* p, float* m, float* v, const int* map, long long nrows, int D, int F, long long chunk,
                         bool flush, const ReplayArgs& ra, hipStream_t st) {
  const int rpw = D >= 128 ? 8 : flush ? 64 : FBN_WIN_ROWS;
  const long long waves = (chunk + rpw - 1) / rpw;
  const dim3 g2((unsigned)std::min<long long>((waves + 3) / 4, flush ? 16384 : 1ll << 31));
  FBN_DISPATCH_D_DW(adam_window2_kernel, ra.decoupled, D, g2, p, m, v, map, nrows, F, chunk, FBN_RA(ra), rpw);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// lazy table Adam: replay the zero-loss-gradient steps of the claimed rows and of rolling window
// (step mod F) (chunk = ceil(nrows / F) rows) up to `step`; last: [nrows] steps applied per row
// parts: 1 = the claimed rows (must precede the gather): entry i of slot_row [n_ent] names a row
// (each at most once) or is -1; 2 = the rolling window (unclaimed rows: nothing else reads them this
// step -> may run on a side stream); any other value is FBN_ERR_ARG
extern "C" int fbn_adam_catchup(float* p, float* m, float* v, long long nrows, int D, const int* slot_row, int n_ent,
                                const int* map, int F, int parts, int* last, const void* consts_table, const int* step,
                                float wd, float beta2, float eps, int* pend, const float* ring,
                                const float* coef_hist, long long ring_stride, int ring_n, int decoupled,
                                void* stream) {
  if (nrows <= 0) return FBN_OK;
  if (F < 1 || F > FBN_LAZY_MAX_LAG) { fbn_set_error("fbn_adam_catchup: 1 <= F <= 512"); return FBN_ERR_ARG; }
  if (parts != 1 && parts != 2) {   // before any device work
    fbn_set_error("fbn_adam_catchup: parts is 1 (claimed rows) or 2 (rolling window), one launch each");
    return FBN_ERR_ARG;
  }
  hipStream_t st = (hipStream_t)stream;
  const long long chunk = (nrows + F - 1) / F;
  if ((parts == 1 ? (long long)n_ent : chunk) <= 0) return FBN_OK;
  if (!replay_args_ok("fbn_adam_catchup", true, F, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  if (parts == 2) return launch_window(p, m, v, map, nrows, D, F, chunk, false, ra, st);
  const int epw = D >= 128 ? FBN_CATCHUP_EPW_WIDE : 64;   // entries per wave, four waves per block
  const dim3 grid((unsigned)((((long long)n_ent + epw - 1) / epw + 3) / 4));
  FBN_DISPATCH_D_DW(adam_catchup_kernel, decoupled, D, grid, p, m, v, slot_row, n_ent, F, FBN_RA(ra));
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// every row up to `step` (checkpoint / evaluation): the window pass over the whole table
extern "C" int fbn_adam_flush(float* p, float* m, float* v, long long nrows, int D, int* last, const void* consts_table,
                              const int* step, float wd, float beta2, float eps, int* pend, const float* ring,
                              const float* coef_hist, long long ring_stride, int ring_n, int decoupled,
                              void* stream) {
  if (nrows <= 0) return FBN_OK;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  return launch_window(p, m, v, nullptr, nrows, D, 1, nrows, true, ra, (hipStream_t)stream);
}

// ---- the prefetches' launches (fbn_adam_prefetch, fbn_adam_prefetch_rows, fbn_adam_prefetch_binned)
static void launch_pretag(const ClaimSrc& cs, long long n, const int* step, hipStream_t st) {
  fbn_launch(adam_pretag_kernel, dim3((unsigned)((n + FBN_PRETAG_BLOCK - 1) / FBN_PRETAG_BLOCK)),
             dim3(FBN_PRETAG_BLOCK), 0, st, cs, (int)n, step);
}
// with pre-claims, the two passes (adam_pretag + adam_prefetch2): tagged pre-claims decide each row's
// owning entry with one non-returning atomic, the replay engine takes 64 entries per wave
static int launch_prefetch2(const ClaimSrc& cs, long long n, float* p, float* m, float* v, int D, const ReplayArgs& ra,
                            hipStream_t st) {
  launch_pretag(cs, n, ra.step, st);
  FBN_CHECK_LAUNCH();
  const int epw = 64;   // entries per wave
  const dim3 g3((unsigned)(((n + epw - 1) / epw + 3) / 4));   // 4 waves per block
  FBN_DISPATCH_D_DW(adam_prefetch2_kernel, ra.decoupled, D, g3, p, m, v, cs, (int)n, FBN_RA(ra), epw);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
// without them, D = 128 / 256: one pass (adam_prefetch_kernel), 64 entries per wave as well
static int launch_prefetch1(const ClaimSrc& cs, long long n, float* p, float* m, float* v, int D, const ReplayArgs& ra,
                            hipStream_t st) {
  const dim3 grid((unsigned)(((n + 63) / 64 + 3) / 4));
  FBN_DISPATCH_WIDE_DW(adam_prefetch_kernel, ra.decoupled, D, grid, p, m, v, cs, (int)n, FBN_RA(ra));
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// the two-pass prefetch with the longest-first replay (adam_pfbin + adam_pfreplay).  Workspace: the
// (bin, copy) counters, one 128-B line each, then the record lists.
static long long pfb_records_per_list(long long n) {
  const long long nblk = (n + 255) / 256;
  return (nblk + FBN_PFB_NC - 1) / FBN_PFB_NC * 256;
}
extern "C" size_t fbn_adam_prefetch_binned_ws_size(long long n) {
  const size_t cnt = (size_t)FBN_PFB_NB * FBN_PFB_NC * FBN_PFB_LINE * sizeof(unsigned);
  return cnt + (size_t)FBN_PFB_NB * FBN_PFB_NC * pfb_records_per_list(n) * sizeof(int4);
}

extern "C" int fbn_adam_prefetch_binned(const int64_t* item, const int64_t* seq, int B, int L, long long V,
                                        const int* map, unsigned long long* preclaim, float* p, float* m, float* v,
                                        int D, int* last, const void* consts_table, const int* step, float wd,
                                        float beta2, float eps, int* pend, const float* ring, const float* coef_hist,
                                        long long ring_stride, int ring_n, int decoupled, void* ws, size_t ws_bytes,
                                        void* stream) {
  const long long n = (long long)B * (L + 1);
  if (n <= 0) return FBN_OK;
  if (D != 128 && D != 256) {
    fbn_set_error("fbn_adam_prefetch_binned: D = 128 / 256 (wave-wide rows)");
    return FBN_ERR_ARG;
  }
  if (!item || (L > 0 && !seq) || !map || !last || !preclaim) {
    fbn_set_error("fbn_adam_prefetch_binned: item, seq (L > 0), map, last and preclaim are required");
    return FBN_ERR_ARG;
  }
  if (!replay_args_ok("fbn_adam_prefetch_binned", false, 0, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  if (ws_bytes < fbn_adam_prefetch_binned_ws_size(n) || !ws) {
    fbn_set_error("fbn_adam_prefetch_binned: workspace smaller than fbn_adam_prefetch_binned_ws_size(n)");
    return FBN_ERR_ARG;
  }
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  const ClaimSrc cs{item, L > 0 ? seq : nullptr, L, V, const_cast<int*>(map), nullptr, nullptr, nullptr, preclaim};
  hipStream_t st = (hipStream_t)stream;
  unsigned* counts = (unsigned*)ws;
  int4* recs = (int4*)((char*)ws + (size_t)FBN_PFB_NB * FBN_PFB_NC * FBN_PFB_LINE * sizeof(unsigned));
  const int nblk = (int)((n + 255) / 256);
  fbn_launch(pfb_zero_kernel, dim3(1), dim3(256), 0, st, counts);
  launch_pretag(cs, n, step, st);
  fbn_launch(adam_pfbin_kernel, dim3(nblk), dim3(256), 0, st, cs, (int)n, last, step, ra.ps, counts, recs);
  const int ch = 32;   // records per replay wave (see adam_pfreplay_kernel)
  // at most one chunk per ch records plus one partial chunk per list
  const long long waves = (n + ch - 1) / ch + FBN_PFB_NB * FBN_PFB_NC;
  const dim3 g((unsigned)((waves + 3) / 4));
  FBN_DISPATCH_WIDE_DW(adam_pfreplay_kernel, decoupled, D, g, p, m, v, step, wd, beta2, ra.omb2, eps, ra.table,
                       ra.ps, (const unsigned*)counts, (const int4*)recs, nblk, ch);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// single GPU: ahead-of-time catch-up of the next batch's rows; call on the stream of the rolling
// window, after this step's claims and before its step tail
extern "C" int fbn_adam_prefetch(const int64_t* item, const int64_t* seq, int B, int L, long long V, const int* map,
                                 unsigned long long* preclaim, float* p, float* m, float* v, int D, int* last,
                                 const void* consts_table, const int* step, float wd, float beta2, float eps, int* pend,
                                 const float* ring, const float* coef_hist, long long ring_stride, int ring_n,
                                 int decoupled, void* stream) {
  const long long n = (long long)B * (L + 1);
  if (n <= 0) return FBN_OK;
  if (D != 16 && D != 32 && D != 64 && D != 128 && D != 256) {
    fbn_set_error("fbn_adam_prefetch: D = 16 / 32 / 64 / 128 / 256");
    return FBN_ERR_ARG;
  }
  if (D < 128 && !preclaim) {   // the one-pass kernel replays wave-wide rows only
    fbn_set_error("fbn_adam_prefetch: d < 128 needs the pre-claims (a next batch of this batch's shape)");
    return FBN_ERR_ARG;
  }
  if (!item || (L > 0 && !seq) || !map || !last) {
    fbn_set_error("fbn_adam_prefetch: item, seq (L > 0), map and last are required");
    return FBN_ERR_ARG;
  }
  if (!replay_args_ok("fbn_adam_prefetch", false, 0, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  const ClaimSrc cs{item, L > 0 ? seq : nullptr, L, V, const_cast<int*>(map), nullptr, nullptr, nullptr, preclaim};
  return (preclaim ? launch_prefetch2 : launch_prefetch1)(cs, n, p, m, v, D, ra, (hipStream_t)stream);
}

// N > 1 (the owner's side): the same ahead-of-time catch-up over the local rows the NEXT step's
// requests name (lids [n], -1 = none: the padded id exchange of RowExchange.prepare); rows this
// step's requests claimed (map != -1) are left to the next step's claimed-row catch-up.  The tags
// of the two-pass form only decide this pass: the next step's owner claims do not read them.
extern "C" int fbn_adam_prefetch_rows(const int* lids, int n, int skip0, long long nrows, const int* map,
                                      unsigned long long* preclaim, float* p, float* m, float* v, int D, int* last,
                                      const void* consts_table, const int* step, float wd, float beta2, float eps,
                                      int* pend, const float* ring, const float* coef_hist, long long ring_stride,
                                      int ring_n, int decoupled, void* stream) {
  if (n <= 0 || nrows <= 0) return FBN_OK;
  if (D != 128 && D != 256) { fbn_set_error("fbn_adam_prefetch_rows: D = 128 or 256"); return FBN_ERR_ARG; }
  if (!lids || !map || !last) { fbn_set_error("fbn_adam_prefetch_rows: lids, map and last are required"); return FBN_ERR_ARG; }
  if (!replay_args_ok("fbn_adam_prefetch_rows", false, 0, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  ClaimSrc cs{nullptr, nullptr, 0, nrows, const_cast<int*>(map), nullptr, nullptr, nullptr, preclaim};
  cs.lids = lids;
  cs.skip0 = skip0;
  return (preclaim ? launch_prefetch2 : launch_prefetch1)(cs, n, p, m, v, D, ra, (hipStream_t)stream);
}

// single GPU: fbn_claim_rows + fbn_adam_catchup(parts = 1) in one launch (see ClaimSrc), one entry
// per lane (adam_claim2_kernel); with conversion jobs, those ride in the same launch
static int claim_catchup_impl(const int64_t* item, const int64_t* seq, int B, int L, long long V, int* map,
                              int* slot_row, int* dup, int* hasdup, unsigned long long* preclaim, float* p, float* m,
                              float* v, long long nrows, int D, int F, int* last, const void* consts_table,
                              const int* step, float wd, float beta2, float eps, int* pend, const float* ring,
                              const float* coef_hist, long long ring_stride, int ring_n, int decoupled,
                              const void* conv_jobs, int n_conv, void* stream) {
  const long long n = (long long)B * (L + 1);
  ConvJobs cj;
  const int conv_tiles = n_conv > 0 ? conv_jobs_pack(conv_jobs, n_conv, cj) : 0;
  if (conv_tiles > 0 && (n <= 0 || nrows <= 0)) {   // no claim launch to ride on: convert alone
    fbn_launch(convert_bf16_kernel_o, dim3(conv_tiles), dim3(256), 0, (hipStream_t)stream, cj, n_conv);
    FBN_CHECK_LAUNCH();
  }
  if (n <= 0 || nrows <= 0) return FBN_OK;
  if (!item || (L > 0 && !seq) || !map || !slot_row) {
    fbn_set_error("fbn_adam_claim_catchup: item, seq (L > 0), map and slot_row are required");
    return FBN_ERR_ARG;
  }
  if (!replay_args_ok("fbn_adam_claim_catchup", true, F, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  const ClaimSrc cs{item, L > 0 ? seq : nullptr, L, V, map, slot_row, dup, hasdup, preclaim};
  const int nclaim = (int)((n + 255) / 256);
  if (conv_tiles > 0) {
    const dim3 g2((unsigned)(nclaim + conv_tiles));
    FBN_DISPATCH_D_DW(adam_claim2_conv_kernel, decoupled, D, g2, p, m, v, cs, (int)n, FBN_RA(ra), cj, n_conv, nclaim);
  } else {
    const dim3 g2((unsigned)nclaim);
    FBN_DISPATCH_D_DW(adam_claim2_kernel, decoupled, D, g2, p, m, v, cs, (int)n, FBN_RA(ra));
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_adam_claim_catchup(const int64_t* item, const int64_t* seq, int B, int L, long long V, int* map,
                                      int* slot_row, int* dup, int* hasdup, unsigned long long* preclaim, float* p,
                                      float* m, float* v, long long nrows, int D,
                                      int F, int* last, const void* consts_table, const int* step, float wd,
                                      float beta2, float eps, int* pend, const float* ring, const float* coef_hist,
                                      long long ring_stride, int ring_n, int decoupled, void* stream) {
  return claim_catchup_impl(item, seq, B, L, V, map, slot_row, dup, hasdup, preclaim, p, m, v, nrows, D, F, last,
                            consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride, ring_n, decoupled,
                            nullptr, 0, stream);
}

extern "C" int fbn_adam_claim_catchup_conv(const int64_t* item, const int64_t* seq, int B, int L, long long V,
                                           int* map, int* slot_row, int* dup, int* hasdup,
                                           unsigned long long* preclaim, float* p, float* m, float* v,
                                           long long nrows, int D, int F, int* last, const void* consts_table,
                                           const int* step, float wd, float beta2, float eps, int* pend,
                                           const float* ring, const float* coef_hist, long long ring_stride,
                                           int ring_n, int decoupled, const void* conv_jobs, int n_conv,
                                           void* stream) {
  if (n_conv < 0 || n_conv > FBN_CONV_MAX || (n_conv > 0 && !conv_jobs)) {
    fbn_set_error("fbn_adam_claim_catchup_conv: 0 <= n_conv <= 8 conversion jobs");
    return FBN_ERR_ARG;
  }
  return claim_catchup_impl(item, seq, B, L, V, map, slot_row, dup, hasdup, preclaim, p, m, v, nrows, D, F, last,
                            consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride, ring_n, decoupled,
                            conv_jobs, n_conv, stream);
}

// N > 1 owner, the fixed-capacity exchange: the claims of the received local rows (lids [n], negative =
// empty slot; rank 0's row 0 is padding when skip0) and the claimed-row catch-up in ONE launch, as
// fbn_adam_claim_catchup does for the single GPU.  preclaim (optional): the tags
// fbn_adam_prefetch_rows posted during the previous step for this very routing (its entry indices
// are these slots): a row tagged for this step is claimed by its smallest slot without a CAS.
extern "C" int fbn_adam_owner_claim_catchup(const int* lids, int n, int skip0, int* map, int* slot_row,
                                            unsigned long long* preclaim, float* p, float* m, float* v,
                                            long long nrows, int D, int F, int* last, const void* consts_table,
                                            const int* step, float wd, float beta2, float eps, int* pend,
                                            const float* ring, const float* coef_hist, long long ring_stride,
                                            int ring_n, int decoupled, void* stream) {
  if (n <= 0 || nrows <= 0) return FBN_OK;
  if (!lids || !map || !slot_row || !last) {
    fbn_set_error("fbn_adam_owner_claim_catchup: lids, map, slot_row and last are required");
    return FBN_ERR_ARG;
  }
  if (!replay_args_ok("fbn_adam_owner_claim_catchup", true, F, pend, ring, coef_hist, ring_n)) return FBN_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const ReplayArgs ra = make_replay(last, consts_table, step, wd, beta2, eps, pend, ring, coef_hist, ring_stride,
                                    ring_n, decoupled);
  ClaimSrc cs{nullptr, nullptr, 0, nrows, map, slot_row, nullptr, nullptr, preclaim};
  cs.lids = lids;
  cs.skip0 = skip0;
  const dim3 g2((unsigned)((n + 255) / 256));
  FBN_DISPATCH_D_DW(adam_claim2_kernel, decoupled, D, g2, p, m, v, cs, n, FBN_RA(ra));
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// Multi-GPU: the loss and this rank's table-gradient sum of squares ride in the dense-gradient
// all-reduce (two floats appended to it): pack before, unpack after (sumsq += all ranks' table
// norms; the loss becomes the global mean).  One thread each.
// one wave: every slot loaded at once, folded in a fixed order (deterministic), then cleared
__global__ void pack_extras_kernel(const float* loss, double* tab_slots, float* out) {
  static_assert(FBN_SUMSQ_SLOTS == 64, "one lane per slot");
  const int lane = threadIdx.x;
  double s = tab_slots[lane];
  tab_slots[lane] = 0.0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
  if (lane == 0) {
    out[0] = *loss;
    out[1] = (float)s;
  }
}
__global__ void unpack_extras_kernel(const float* in, float* loss, double* sumsq) {
  *loss = in[0];
  sumsq[0] += (double)in[1];
}
// N > 1, after the all-reduce: fbn_unpack_extras and the dense gradients' sum of squares (fbn_sumsq
// over x[0, n)) in one launch -- block 0 adds the unpacked table sumsq into its slot atomically,
// beside the other blocks' dense partials
__global__ void unpack_sumsq_kernel(const float* __restrict__ in, float* __restrict__ loss,
                                    const float* __restrict__ x, long long n, double* __restrict__ sumsq) {
  __shared__ double red[256];
  double s = 0.0;
  const long long n4 = n / 4;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long long)gridDim.x * blockDim.x) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(x + 4 * i);
    s += (double)(v[0] * v[0]) + (double)(v[1] * v[1]) + (double)(v[2] * v[2]) + (double)(v[3] * v[3]);
  }
  for (long long i = n4 * 4 + (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
    s += (double)(x[i] * x[i]);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double t = red[0];
    if (blockIdx.x == 0) {
      *loss = in[0];
      t += (double)in[1];
    }
    atomicAdd(sumsq + (blockIdx.x & (FBN_SUMSQ_SLOTS - 1)), t);
  }
}
// out[i] = ((in[0][i] + in[1][i]) + in[2][i]) + ... -- the `ns` slices of an all-gather summed in rank
// order (deterministic mode's all-reduce: fbn_comm_allgather + this).  dtype 0 = f32, 1 = f64.
template <typename T>
__global__ void sum_slices_kernel(const T* __restrict__ in, int ns, long long n, T* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    T s = in[i];
    for (int k = 1; k < ns; ++k) s += in[(size_t)k * n + i];
    out[i] = s;
  }
}
extern "C" int fbn_sum_slices(const void* in, int ns, long long n, int dtype, void* out, void* stream) {
  if (n <= 0) return FBN_OK;
  if (!in || !out || ns < 1 || dtype < 0 || dtype > 1) {
    fbn_set_error("fbn_sum_slices: in, out, ns >= 1, dtype 0 (f32) / 1 (f64)");
    return FBN_ERR_ARG;
  }
  long long blocks = (n + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  if (dtype == 0)
    fbn_launch(sum_slices_kernel<float>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
               (const float*)in, ns, n, (float*)out);
  else
    fbn_launch(sum_slices_kernel<double>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
               (const double*)in, ns, n, (double*)out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_pack_extras(const float* loss, double* tab_slots, float* out, void* stream) {
  fbn_launch(pack_extras_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, tab_slots, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
extern "C" int fbn_unpack_sumsq(const float* in, float* loss, const float* x, long long n, double* sumsq, void* stream) {
  if (!in || !loss || !sumsq || (n > 0 && !x)) { fbn_set_error("fbn_unpack_sumsq: in, loss, x, sumsq"); return FBN_ERR_ARG; }
  fbn_launch(unpack_sumsq_kernel, dim3(512), dim3(256), 0, (hipStream_t)stream, in, loss, x, n, sumsq);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
extern "C" int fbn_unpack_extras(const float* in, float* loss, double* sumsq, void* stream) {
  fbn_launch(unpack_extras_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, in, loss, sumsq);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
