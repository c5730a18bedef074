#include <cstdlib>
// K1 / K2 / K4: FiBiNET field construction, SENET and the embedding scatter-add gradient.
//
// Forward (one "sample group" of D/4 lanes per sample, each lane owning 4 contiguous
// columns, so a D=128 fp32 row is one 512-B coalesced read by 32 lanes):
//   X1 = C[likes], X2 = C[views], X3 = E[item_id], X4 = ReLU(LN(h_mm)),
//   X5 = sum_{t: s_t != 0} E[s_t] / max(1, #nonzero)         (model_fibinet.py:152-176)
//   z_f = mean_d X_f ; a = sigmoid(W2 relu(W1 z + b1) + b2) ; V_f = X_f * a_f   (:24-35)
// All 21 table rows of a sample are issued before any is consumed (21 x 16 B in flight per
// lane); the (B,20,d) history tensor of the reference is never materialised.
// V_0 == 0 (the user field is all zeros, :152), so only fields 1..5 are stored.
//
// Backward: SENET + mean + LayerNorm + ReLU backward per sample, then the embedding
// gradient: E rows get dX3 (item) and dX5/count (each non-padding history slot); row 0 is
// never written (padding_idx=0, :100).  The table gradient is accumulated either into a
// dense V x d buffer (torch drop-in semantics) or into a compact per-unique-row buffer
// addressed through a row->slot map (the native trainer: see DESIGN.md "sparse table grad").
// Small parameter gradients (SENET, LN, cate table) are reduced per block in LDS and
// written as per-block partial slabs summed by fbn_reduce_partials (deterministic).
#include "common.h"
#include "fields_common.h"   // FBN_MAXR, FBN_MAX_L, ln_relu, senet_excite (shared with recommend.hip)

#ifndef FBN_HCH
// default history rows in flight per sample before they are summed (FBN_FIELDS_HCH: 5 / 10 / 20;
// the sum runs in slot order whatever the chunk, so every choice gives the same bits): 10 -- round 3
// measured 5 best beside the side-stream passes (0.4184 vs 0.4203 (10) vs 0.4212 ms/step (20),
// profiles/r03s2_group_knobs_ab.txt); on round 6's step the two tie on time (0.4027 / 0.4136 vs
// 0.4035 / 0.4141 ms/step, two boxes) and 10 runs the gather itself faster inside the step (in-step
// fraction of the HBM roofline 0.52-0.61 vs 0.37-0.51; profiles/r06_knob_resweep_ab.txt)
#define FBN_HCH 10
#endif

struct FieldArgs {
  const int64_t* item_id;   // [B]
  const int64_t* item_seq;  // [B][L] or null (L = 0)
  const int64_t* likes;     // [B]
  const int64_t* views;     // [B]
  const float* hmm;         // [B][D] pre-LayerNorm mm projection (bias included)
  const float* ln_g;        // [D]
  const float* ln_b;        // [D]
  const float* cate;        // [n_cate][D]
  const float* table;       // mode 0: [V][D] rows; mode 1: exchanged row buffer
  const int* pos;           // mode 1: [B][L+1] row index into `table` (-1 = none)
  const float* w1; const float* b1; const float* w2; const float* b2;  // SENET [R][6],[R],[6][R],[6]
  float* X;                 // [B][2][D] fields 3 and 5 (item row, history mean); the backward
                            // recomputes fields 1, 2 (cate rows) and 4 (LN of hmm) bit-identically
  float* Vc;                // [B][5][D] fields 1..5 (post-SENET)
  short* Vc16;              // optional bf16 copy of Vc (GEMM operand of the bilinear U = V W and its wgrad)
  void* c;                  // [B][ldc] float or bf16 (c16); cols [0,5D) <- Vc (MLP input, compact layout);
                            // null: not written (the bf16 GEMMs read those columns from Vc16)
  float* a_out;             // [B][6]
  float* cnt_out;           // [B]
  int* err;                 // id range violations (sticky flag)
  int* map;                 // sparse-grad map [V]: row -> claiming entry (-1 = untouched) or null
  int* slot_row;            // [B*(L+1)]: entry -> row it claimed, -1 otherwise (pre-filled with -1)
  long long V;              // rows of the table (mode 0)
  int B, L, ldc, R, n_cate, c16;
  float ln_eps;
  const int* hot;           // optional hot-row list (fbn_hot_rows) staged in LDS: [H] row ids
  const int* hot_n;         // its length (entries past H ignored)
  int H;
};

// hot-row staging (fbn_fields_fwd_hot, an A/B variant of the gather): up to FBN_HOT_ROWS(D) rows
// (32 KB of f32) sit in LDS, found through an open-addressed id table of twice that size
#define FBN_HOT_ROWS(D) ((8192 / (D)) < 256 ? (8192 / (D)) : 256)
__device__ __forceinline__ unsigned hot_hash(int r) { return (unsigned)r * 0x9E3779B1u; }

// Sparse-gradient registration: the first entry e = b*(L+1)+t that touches row r claims it
// (map[r] = e, slot_row[e] = r).  Slots are entry indices, so no shared counter is needed:
// a global "next free slot" atomic serialises on one address (~12 ns per wave-level atomic).
__device__ __forceinline__ void map_claim(int* map, int* slot_row, int r, int e) {
  if (__hip_atomic_load(map + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != -1) return;
  int expected = -1;
  if (__hip_atomic_compare_exchange_strong(map + r, &expected, e, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_AGENT))
    slot_row[e] = r;
}

// row r of the exchanged row buffer (MODE 1: f32 rows; MODE 2: bf16 rows, the bf16 mode's wire format)
template <int D, int MODE>
__device__ __forceinline__ f32x4 load_row(const FieldArgs& p, size_t r, int q) {
  if constexpr (MODE == 2) {
    const bf16x4 h = *reinterpret_cast<const bf16x4*>(reinterpret_cast<const short*>(p.table) + r * D + 4 * q);
    return (f32x4){bf2f(h[0]), bf2f(h[1]), bf2f(h[2]), bf2f(h[3])};
  } else {
    return *reinterpret_cast<const f32x4*>(p.table + r * D + 4 * q);
  }
}

// BUF (MODE 0, tables under 4 GB): the history rows are read through a buffer resource over the
// table, and a padding / past-L slot's load gets an out-of-range offset -- the buffer unit returns
// zeros without a memory request, so dead slots stay off the fetch path (the global-load form
// reads row 0 for them: an L2 hit, but L2 bandwidth and TA cycles all the same)
#define FBN_BUF_FLAGS 0x00020000   // gfx9 buffer descriptor word 3 (raw, 32-bit dwords)
// CMP: the sample's live history slots are compacted first (ballot + mbcnt; their rows staged in a
// per-sample LDS list in slot order), so a chunk of HCH loads carries only live rows and a sample
// takes ceil(n_live / HCH) rounds instead of L / HCH; summed in slot order like the plain form --
// the skipped padding slots added +0.0 there, so the two are bit-identical.
template <int D, int MODE, int HCH, bool BUF = false, bool HOT = false, bool CMP = false>
__global__ void __launch_bounds__(256) fields_fwd_kernel(FieldArgs p) {
  FBN_MAIN_PRIO();
  // (unused, and dropped, unless BUF)
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<float*>(p.table), 0, (int)((unsigned long long)p.V * D * 4), FBN_BUF_FLAGS);
  constexpr int HR = HOT ? FBN_HOT_ROWS(D) : 1, HT = 2 * HR;   // staged rows, id-table slots
  __shared__ f32x4 hrow[HOT ? HR * (D / 4) : 1];
  __shared__ int hkey[HOT ? HT : 1];   // staged row id (-1 = empty)
  __shared__ int hval[HOT ? HT : 1];   // its index in hrow
  int nh = 0;
  if constexpr (HOT) {
    nh = min(*p.hot_n, min(p.H, HR));
    for (int i = threadIdx.x; i < HT; i += blockDim.x) hkey[i] = -1;
    __syncthreads();
    for (int i = threadIdx.x; i < nh; i += blockDim.x) {   // insert (linear probing, CAS in LDS)
      const int r = p.hot[i];
      unsigned h = hot_hash(r) >> (32 - __builtin_ctz(HT));
      for (int k = 0; k < HT; ++k, h = (h + 1) & (HT - 1))
        if (atomicCAS(&hkey[h], -1, r) == -1) {
          hval[h] = i;
          break;
        }
    }
    for (int i = threadIdx.x; i < nh * (D / 4); i += blockDim.x) {
      const int j = i / (D / 4), c = i - j * (D / 4);
      hrow[i] = *reinterpret_cast<const f32x4*>(p.table + (size_t)p.hot[j] * D + 4 * c);
    }
    __syncthreads();
  }
  constexpr int G = D / 4;                  // lanes per sample
  constexpr int SPW = 64 / G;               // samples per wave
  const int lane = threadIdx.x & 63;
  const int q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int L = p.L;

  for (int b0 = gw * SPW; b0 < p.B; b0 += nwaves * SPW) {
    const int b = b0 + lane / G;
    if (b >= p.B) continue;
    // ---------------- ids + validation
    long long item = p.item_id[b];
    long long lk = p.likes[b], vw = p.views[b];
    bool bad = false;
    if (lk < 0 || lk >= p.n_cate) { bad = true; lk = 0; }
    if (vw < 0 || vw >= p.n_cate) { bad = true; vw = 0; }
    // history rows are issued in chunks of HCH slots (all loads of a chunk in flight before
    // any is consumed) and summed in slot order like the reference's sum over dim 1
    // independent loads first (they overlap the row gather below)
    const f32x4 c1 = *reinterpret_cast<const f32x4*>(p.cate + lk * D + 4 * q);
    const f32x4 c2 = *reinterpret_cast<const f32x4*>(p.cate + vw * D + 4 * q);
    const f32x4 h = *reinterpret_cast<const f32x4*>(p.hmm + (size_t)b * D + 4 * q);
    f32x4 rit = {0.f, 0.f, 0.f, 0.f};
    f32x4 hs = {0.f, 0.f, 0.f, 0.f};
    int nnz = 0;
    const int* pb = MODE >= 1 ? p.pos + (size_t)b * (L + 1) : nullptr;
    if (MODE == 0) {
      if (item < 0 || item >= p.V) { bad = true; item = -1; }
      if (item >= 0) rit = *reinterpret_cast<const f32x4*>(p.table + item * D + 4 * q);
    } else {
      const int pi = pb[0];
      if (pi >= 0) rit = load_row<D, MODE>(p, pi, q);
    }
    // all history ids in ONE round (lane q of the group holds slots q, q+G, ...), broadcast by
    // shuffles, then every row load is issued before any is consumed (two dependent round trips
    // per sample instead of one per chunk); summed in slot order like the reference
    constexpr int IPL = (FBN_MAX_L + G - 1) / G;      // ids per lane
    int sid[IPL];
#pragma unroll
    for (int j = 0; j < IPL; ++j) {
      const int t = q + j * G;
      int r = -1;
      if (t < L) {
        if (MODE == 0) {
          long long s = p.item_seq[(size_t)b * L + t];
          if (s < 0 || s >= p.V) { bad = true; s = 0; }
          r = s != 0 ? (int)s : -1;
        } else {
          r = pb[t + 1];
        }
      }
      sid[j] = r;
    }
    const int gbase = lane - q;
    if constexpr (CMP) {
      constexpr int SPB = 4 * SPW;                     // samples per 256-thread block
      __shared__ int lid[SPB][FBN_MAX_L];
      int* mine = lid[(threadIdx.x >> 6) * SPW + lane / G];
      const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << gbase;
      int nl = 0;
#pragma unroll
      for (int j = 0; j < IPL; ++j) {
        const unsigned long long mk = __ballot(sid[j] >= 0) & gmask;
        const int below = __popcll(mk & ((1ull << lane) - 1));
        if (sid[j] >= 0) mine[nl + below] = sid[j];
        nl += __popcll(mk);
      }
      __builtin_amdgcn_wave_barrier();
      __atomic_signal_fence(__ATOMIC_SEQ_CST);         // the list is read back by the group's lanes
      int nch = (nl + HCH - 1) / HCH;                  // wave-uniform bound: the wave's largest
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) nch = max(nch, __shfl_xor(nch, o, 64));
      for (int c = 0; c < nch; ++c) {
        f32x4 hist[HCH];
        bool live[HCH];
#pragma unroll
        for (int u = 0; u < HCH; ++u) {
          const int k = c * HCH + u;
          live[u] = k < nl;
          const int r = mine[live[u] ? k : 0];
          if constexpr (BUF) {
            const unsigned off = live[u] ? ((unsigned)r * D + 4 * q) * 4u : 0xFFFFFFF0u;
            hist[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
          } else {
            hist[u] = load_row<D, MODE>(p, live[u] ? r : 0, q);
          }
        }
#pragma unroll
        for (int u = 0; u < HCH; ++u) hs += live[u] ? hist[u] : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      nnz = nl;
      __builtin_amdgcn_wave_barrier();                 // the next sample's list overwrites this one
      __atomic_signal_fence(__ATOMIC_SEQ_CST);
    }
    for (int t0 = 0; t0 < (CMP ? 0 : L); t0 += HCH) {
      // branch-free: every slot of the chunk issues its load (a padding or past-L slot reads row
      // 0, an L2-resident line, and contributes +0 by a select) -- a load under a branch makes
      // hipcc drain vmcnt(0) before the next, which serialised the chunk's round trips
      f32x4 hist[HCH];
      bool live[HCH];
#pragma unroll
      for (int u = 0; u < HCH; ++u) {
        const int t = t0 + u;
        int r = -1;
#pragma unroll
        for (int j = 0; j < IPL; ++j)
          if ((t / G) == j) r = __shfl(sid[j], gbase + (t % G), 64);
        live[u] = t < L && r >= 0;
        if constexpr (HOT) {
          // two probes of the id table (slot -> list index): a staged row is read from LDS and
          // its global load is sent out of range (no fetch)
          int hi = -1;
          if (live[u] && nh > 0) {
            const unsigned h = hot_hash(r) >> (32 - __builtin_ctz(HT));
#pragma unroll
            for (int k = 0; k < 2; ++k) {
              const unsigned hk = (h + k) & (HT - 1);
              if (hi < 0 && hkey[hk] == r) hi = hval[hk];
            }
          }
          const unsigned off = (live[u] && hi < 0) ? ((unsigned)r * D + 4 * q) * 4u : 0xFFFFFFF0u;
          hist[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
          if (hi >= 0) hist[u] = hrow[hi * (D / 4) + q];
        } else if constexpr (BUF) {
          const unsigned off = live[u] ? ((unsigned)r * D + 4 * q) * 4u : 0xFFFFFFF0u;
          hist[u] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        } else {
          hist[u] = load_row<D, MODE>(p, live[u] ? r : 0, q);
        }
      }
#pragma unroll
      for (int u = 0; u < HCH; ++u) {
        hs += live[u] ? hist[u] : (f32x4){0.f, 0.f, 0.f, 0.f};
        nnz += live[u] ? 1 : 0;
      }
    }
    if (bad) atomicOr(p.err, 1);        // any lane: history ids are validated by the lane holding them

    // ---------------- history masked mean
    const float cnt = fmaxf((float)nnz, 1.f);
    f32x4 x5 = hs / cnt;

    // ---------------- mm field: LayerNorm(eps) + ReLU
    const f32x4 x4 = ln_relu<G>(h, p.ln_g, p.ln_b, p.ln_eps, q);

    // ---------------- SENET
    const f32x4 xs[5] = {c1, c2, rit, x4, x5};
    float z[6];
    z[0] = 0.f;
#pragma unroll
    for (int f = 0; f < 5; ++f) z[f + 1] = group_sum<G>(xs[f][0] + xs[f][1] + xs[f][2] + xs[f][3]) / (float)D;
    float qv[FBN_MAXR], a[6];
    senet_excite<D>(z, p.w1, p.b1, p.w2, p.b2, p.R, qv, a);

    // ---------------- stores
    float* Xb = p.X + (size_t)b * 2 * D + 4 * q;
    *reinterpret_cast<f32x4*>(Xb) = rit;
    *reinterpret_cast<f32x4*>(Xb + D) = x5;
    float* Vb = p.Vc ? p.Vc + (size_t)b * 5 * D + 4 * q : nullptr;
    float* cb = (p.c && !p.c16) ? (float*)p.c + (size_t)b * p.ldc + 4 * q : nullptr;
    short* cb16 = (p.c && p.c16) ? (short*)p.c + (size_t)b * p.ldc + 4 * q : nullptr;
#pragma unroll
    for (int f = 0; f < 5; ++f) {
      const f32x4 v = xs[f] * a[f + 1];
      if (p.Vc) *reinterpret_cast<f32x4*>(Vb + f * D) = v;   // bf16 mode: only the bf16 copies
      const bf16x4 v16 = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
      if (cb16) *reinterpret_cast<bf16x4*>(cb16 + f * D) = v16;
      else if (cb) *reinterpret_cast<f32x4*>(cb + f * D) = v;
      if (p.Vc16) *reinterpret_cast<bf16x4*>(p.Vc16 + ((size_t)b * 5 + f) * D + 4 * q) = v16;
    }
#pragma unroll
    for (int f = 0; f < 6; ++f)
      if (f % G == q) p.a_out[(size_t)b * 6 + f] = a[f];   // G may be < 6 (D = 16)
    if (q == 0) p.cnt_out[b] = cnt;

    // ---------------- sparse-grad map insert (rows that will receive a gradient)
    if (MODE == 0 && p.map) {
      for (int t = q; t <= L; t += G) {
        long long r = (t == 0) ? item : p.item_seq[(size_t)b * L + (t - 1)];
        if (r > 0 && r < p.V) map_claim(p.map, p.slot_row, (int)r, b * (L + 1) + t);
      }
    }
  }
}

// ------------------------------------------------------------------------------ backward
// FieldBwdArgs, the per-sample body and the folds of the backward: fields_common.h (shared with the
// fused bilinear + fields backward of bilinear.hip)

// Backward of the fields.  No LDS atomics (they serialised on the few hot addresses every
// sample adds into -- the LN columns, 11 cate rows, the SENET weights -- and cost ~25 LDS cycles
// each): the LN and SENET parameter gradients accumulate in registers (SENET's group-uniform
// entries spread over the group's lanes: entry k in lane k mod G), the cate rows by plain
// read-modify-write into a per-wave LDS slice with the wave's sample groups taking turns; each
// wave folds its groups with shuffles into its slice, and the block sums its 4 slices into its
// partial row (same layout as before).
template <int D, int MODE, int RMAX, bool SLOT = false>
__global__ void __launch_bounds__(256) fields_bwd_kernel(FieldBwdArgs p) {
  FBN_MAIN_PRIO();
  constexpr int G = D / 4;
  constexpr int SPW = 64 / G;
  extern __shared__ __attribute__((aligned(16))) float sp[];   // 4 wave slices of P floats + SENET staging
  const int NP = 13 * p.R + 6;
  const int P = NP + 3 * D + p.n_cate * D;      // ... | cate rows | mm_proj bias (column sums of dhmm)
  const int wave = threadIdx.x >> 6;
  // per group: {ds[6], z[6], dq[R], rj[R]} staged for the lanes that own SENET entries
  float* sv = sp + 4 * P + (wave * SPW + (threadIdx.x & 63) / G) * (12 + 2 * RMAX);
  for (int i = threadIdx.x; i < 4 * P; i += blockDim.x) sp[i] = 0.f;
  __syncthreads();
  float* w_ct = sp + wave * P + NP + 2 * D;        // the cate rows of this wave's slice

  const int lane = threadIdx.x & 63;
  const int q = lane % G, grp = lane / G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  float* gvec = p.gvec;
  if constexpr (SLOT) {   // the ring slot of this step, chosen on the device (as fbn_owner_fold); wave-uniform
    gvec += (size_t)(__builtin_amdgcn_readfirstlane(*p.slot_step) % p.ring_n) * p.ring_stride;
    if (blockIdx.x == 0 && threadIdx.x == 0) *p.slot_cell = gvec;
  }
  FieldsBwdAcc<D, RMAX> acc;
  acc.zero();

  for (int b0 = gw * SPW; b0 < p.B; b0 += nwaves * SPW) {
    const int b = b0 + grp;
    const bool live = b < p.B;
    f32x4 dx0 = {0.f, 0.f, 0.f, 0.f}, dx1 = {0.f, 0.f, 0.f, 0.f};
    long long lk = -1, vw = -1;
    if (live) {
      const FieldsBwdIn in = fields_bwd_load<D>(p, b, q);
      const float* dVb = p.dV + (size_t)b * 5 * D + 4 * q;
      f32x4 dv[5];
#pragma unroll
      for (int f = 0; f < 5; ++f) dv[f] = *reinterpret_cast<const f32x4*>(dVb + f * D);
      lk = in.lk;
      vw = in.vw;
      fields_bwd_sample<D, MODE, RMAX>(p, gvec, b, lane, in, dv, sv, acc, dx0, dx1);
    }
    fields_bwd_cate<D>(w_ct, p.n_cate, lane, live, lk, vw, dx0, dx1);
  }
  fields_bwd_fold<D, RMAX>(p, sp, acc);
}

// destinations of the 8 parameter-gradient segments (w1, b1, w2, b2, ln_g, ln_b, cate, mm_proj bias)
struct GradOuts {
  float* p[8];
  int off[9];
};
// One launch, 16 columns per block (P / 16 workgroups): 64 partial-row streams per column,
// 16 lanes reading one 64-B segment, then a fixed-order fold over the 64 streams (deterministic).
__global__ void __launch_bounds__(1024) reduce_partials_one16(const float* __restrict__ part, int nblk, int P, GradOuts o) {
  __shared__ float red[64][16];
  const int col = threadIdx.x & 15, str = threadIdx.x >> 4;
  const int i = blockIdx.x * 16 + col;
  float s = 0.f;
  if (i < P)
    for (int r = str; r < nblk; r += 64) s += part[(size_t)r * P + i];
  red[str][col] = s;
  __syncthreads();
  if (threadIdx.x < 16 && i < P) {
    float t = 0.f;
    for (int k = 0; k < 64; ++k) t += red[k][col];
    int seg = 0;
#pragma unroll
    for (int j = 1; j < 8; ++j) seg += (i >= o.off[j]) ? 1 : 0;
    if (o.p[seg]) o.p[seg][i - o.off[seg]] = t;
  }
}


// ------------------------------------------------------------------------------ C ABI
// (FBN_FB_MAXBLK and fields_grid: fields_common.h)

// history rows per chunk: every row of a chunk is in flight at once (branch-free issue); more rows
// per chunk = fewer dependent round trips but more registers (fewer waves resident)
template <int MODE, int HCH, bool BUF, bool HOT = false, bool CMP = false>
static int launch_fields_fwd_hb(const FieldArgs& a, int D, hipStream_t st) {
  // hot staging: fewer, longer-lived workgroups (each stages the hot rows once)
  const int grid = fields_grid(a.B, D, HOT ? 256 : 1024);
  switch (D) {
    case 16: fbn_launch((fields_fwd_kernel<16, MODE, HCH, BUF, HOT, CMP>), dim3(grid), dim3(256), 0, st, a); break;
    case 32: fbn_launch((fields_fwd_kernel<32, MODE, HCH, BUF, HOT, CMP>), dim3(grid), dim3(256), 0, st, a); break;
    case 64: fbn_launch((fields_fwd_kernel<64, MODE, HCH, BUF, HOT, CMP>), dim3(grid), dim3(256), 0, st, a); break;
    case 128: fbn_launch((fields_fwd_kernel<128, MODE, HCH, BUF, HOT, CMP>), dim3(grid), dim3(256), 0, st, a); break;
    case 256: fbn_launch((fields_fwd_kernel<256, MODE, HCH, BUF, HOT, CMP>), dim3(grid), dim3(256), 0, st, a); break;
    default: fbn_set_error("fields: embedding_dim must be one of 16,32,64,128,256"); return FBN_ERR_UNSUPPORTED;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

template <int MODE, int HCH, bool CMP>
static int launch_fields_fwd_h(const FieldArgs& a, int D, hipStream_t st) {
  if constexpr (MODE == 0) {
    if (a.hot) return launch_fields_fwd_hb<0, HCH, true, true>(a, D, st);
    // buffer-resource history loads while the table's byte extent fits the descriptor's 32 bits
    if ((unsigned long long)a.V * D * 4 < 0xFFFFFF00ull)
      return launch_fields_fwd_hb<0, HCH, true, false, CMP>(a, D, st);
  }
  return launch_fields_fwd_hb<MODE, HCH, false, false, CMP>(a, D, st);
}

template <int MODE>
static int launch_fields_fwd(const FieldArgs& a, int D, hipStream_t st) {
  const char* he = getenv("FBN_FIELDS_HCH");   // A/B knob, read per call
  const int hch = he ? atoi(he) : FBN_HCH;
  // FBN_FIELDS_CMP=1: the live history slots compacted first (A/B knob, read per call)
  const char* ce = getenv("FBN_FIELDS_CMP");
  if (ce && atoi(ce) == 1) {
    if (hch == 10) return launch_fields_fwd_h<MODE, 10, true>(a, D, st);
    if (hch == 8) return launch_fields_fwd_h<MODE, 8, true>(a, D, st);
    return launch_fields_fwd_h<MODE, 5, true>(a, D, st);
  }
  if (hch == 20) return launch_fields_fwd_h<MODE, 20, false>(a, D, st);
  if (hch == 5) return launch_fields_fwd_h<MODE, 5, false>(a, D, st);
  return launch_fields_fwd_h<MODE, 10, false>(a, D, st);
}

static int fields_fwd_impl(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                           const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                           float ln_eps, const float* cate, int n_cate, const float* table, long long V,
                           const int* pos, const float* w1, const float* b1, const float* w2,
                           const float* b2, int R, float* X, float* Vc, short* Vc16, void* c, int ldc, int c_bf16,
                           float* a_out, float* cnt_out, int* err, int* map, int* slot_row, int B, int L,
                           int D, int rows_bf16, const int* hot, const int* hot_n, int H, void* stream);

extern "C" int fbn_fields_fwd(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                              const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                              float ln_eps, const float* cate, int n_cate, const float* table, long long V,
                              const int* pos, const float* w1, const float* b1, const float* w2,
                              const float* b2, int R, float* X, float* Vc, short* Vc16, void* c, int ldc, int c_bf16,
                              float* a_out,
                              float* cnt_out, int* err, int* map, int* slot_row, int B, int L,
                              int D, int rows_bf16, void* stream) {
  return fields_fwd_impl(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, cate, n_cate, table, V, pos, w1,
                         b1, w2, b2, R, X, Vc, Vc16, c, ldc, c_bf16, a_out, cnt_out, err, map, slot_row, B, L, D,
                         rows_bf16, nullptr, nullptr, 0, stream);
}

// the gather with the batch's hot rows (fbn_hot_rows) staged in LDS (single GPU, f32 table < 4 GB)
extern "C" int fbn_fields_fwd_hot(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                                  const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                                  float ln_eps, const float* cate, int n_cate, const float* table, long long V,
                                  const float* w1, const float* b1, const float* w2, const float* b2, int R, float* X,
                                  float* Vc, short* Vc16, void* c, int ldc, int c_bf16, float* a_out, float* cnt_out,
                                  int* err, int* map, int* slot_row, int B, int L, int D, const int* hot,
                                  const int* hot_n, int H, void* stream) {
  if (!hot || !hot_n || (unsigned long long)V * D * 4 >= 0xFFFFFF00ull) {
    fbn_set_error("fbn_fields_fwd_hot: needs the hot list and a table under 4 GB");
    return FBN_ERR_ARG;
  }
  return fields_fwd_impl(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, cate, n_cate, table, V, nullptr,
                         w1, b1, w2, b2, R, X, Vc, Vc16, c, ldc, c_bf16, a_out, cnt_out, err, map, slot_row, B, L, D, 0,
                         hot, hot_n, H, stream);
}

// Hot rows of a batch (clear = 0): every entry counts its row (cnt [V] int32, zero on entry); the
// entry that brings a row's count to tau appends it to hot[] (hot_n: length, may exceed H).
// clear = 1: the same entries zero their counts and hot_n (after the gather has read the list).
__global__ void hot_rows_kernel(const int64_t* __restrict__ item, const int64_t* __restrict__ seq, int B, int L,
                                long long V, int* __restrict__ cnt, int* __restrict__ hot, int* __restrict__ hot_n,
                                int H, int tau, int clear) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (clear && i == 0) *hot_n = 0;
  if (i >= (long long)B * (L + 1)) return;
  const long long b = i / (L + 1), t = i - b * (L + 1);
  const long long id = t == 0 ? item[b] : seq[b * L + (t - 1)];
  if (id <= 0 || id >= V) return;
  if (clear) {
    cnt[id] = 0;
    return;
  }
  if (atomicAdd(cnt + id, 1) == tau - 1) {
    const int s = atomicAdd(hot_n, 1);
    if (s < H) hot[s] = (int)id;
  }
}

extern "C" int fbn_hot_rows(const int64_t* item, const int64_t* seq, int B, int L, long long V, int* cnt, int* hot,
                            int* hot_n, int H, int tau, int clear, void* stream) {
  const long long n = (long long)B * (L + 1);
  if (n <= 0) return FBN_OK;
  fbn_launch(hot_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, item,
                     L > 0 ? seq : nullptr, B, L, V, cnt, hot, hot_n, H, tau < 1 ? 1 : tau, clear);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

static int fields_fwd_impl(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                           const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                           float ln_eps, const float* cate, int n_cate, const float* table, long long V,
                           const int* pos, const float* w1, const float* b1, const float* w2,
                           const float* b2, int R, float* X, float* Vc, short* Vc16, void* c, int ldc, int c_bf16,
                           float* a_out, float* cnt_out, int* err, int* map, int* slot_row, int B, int L,
                           int D, int rows_bf16, const int* hot, const int* hot_n, int H, void* stream) {
  if (B <= 0) return FBN_OK;
  if (L < 0 || L > 32 || R < 1 || R > FBN_MAXR || (ldc & 3)) {
    fbn_set_error("fbn_fields_fwd: need 0 <= L <= 32, 1 <= R <= 8, ldc % 4 == 0");
    return FBN_ERR_ARG;
  }
  FieldArgs a;
  a.item_id = item_id; a.item_seq = L > 0 ? item_seq : nullptr; a.likes = likes; a.views = views;
  a.hmm = hmm; a.ln_g = ln_g; a.ln_b = ln_b; a.cate = cate; a.table = table; a.pos = pos;
  a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2;
  a.X = X; a.Vc = Vc; a.Vc16 = Vc16; a.c = c; a.a_out = a_out; a.cnt_out = cnt_out; a.err = err;
  a.map = map; a.slot_row = slot_row;
  a.V = V; a.B = B; a.L = L; a.ldc = ldc; a.R = R; a.n_cate = n_cate; a.ln_eps = ln_eps; a.c16 = c_bf16;
  a.hot = hot; a.hot_n = hot_n; a.H = H;
  if (pos && rows_bf16) return launch_fields_fwd<2>(a, D, (hipStream_t)stream);
  if (pos) return launch_fields_fwd<1>(a, D, (hipStream_t)stream);
  return launch_fields_fwd<0>(a, D, (hipStream_t)stream);
}

extern "C" int fbn_fields_bwd_partials_size(int D, int R, int n_cate) { return 13 * R + 6 + 3 * D + n_cate * D; }
// rows of the `partials` scratch the caller allocates: one per block
extern "C" int fbn_fields_bwd_grid(int B, int D) { return fields_grid(B, D, FBN_FB_MAXBLK); }

template <int MODE, int RMAX, bool SLOT = false>
static int launch_fields_bwd_r(const FieldBwdArgs& a, int D, hipStream_t st) {
  const int grid = fields_grid(a.B, D, FBN_FB_MAXBLK);
  const size_t lds = fields_bwd_lds(D, a.R, a.n_cate, RMAX);   // 4 wave slices + SENET staging
  switch (D) {
    case 16: fbn_launch((fields_bwd_kernel<16, MODE, RMAX, SLOT>), dim3(grid), dim3(256), lds, st, a); break;
    case 32: fbn_launch((fields_bwd_kernel<32, MODE, RMAX, SLOT>), dim3(grid), dim3(256), lds, st, a); break;
    case 64: fbn_launch((fields_bwd_kernel<64, MODE, RMAX, SLOT>), dim3(grid), dim3(256), lds, st, a); break;
    case 128: fbn_launch((fields_bwd_kernel<128, MODE, RMAX, SLOT>), dim3(grid), dim3(256), lds, st, a); break;
    case 256: fbn_launch((fields_bwd_kernel<256, MODE, RMAX, SLOT>), dim3(grid), dim3(256), lds, st, a); break;
    default: fbn_set_error("fields: embedding_dim must be one of 16,32,64,128,256"); return FBN_ERR_UNSUPPORTED;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// the reference's SENET width is 3 (reduction ratio 3 over 6 fields): register arrays sized 3
template <int MODE>
static int launch_fields_bwd(const FieldBwdArgs& a, int D, hipStream_t st) {
  if constexpr (MODE == 0)   // the slot form: an instantiation of its own, the other entry points' code unchanged
    if (a.slot_step)
      return a.R <= 3 ? launch_fields_bwd_r<0, 3, true>(a, D, st) : launch_fields_bwd_r<0, FBN_MAXR, true>(a, D, st);
  return a.R <= 3 ? launch_fields_bwd_r<MODE, 3>(a, D, st) : launch_fields_bwd_r<MODE, FBN_MAXR>(a, D, st);
}

// partials: [fbn_fields_bwd_grid(B,D)][P] scratch (P = fbn_fields_bwd_partials_size(D,R,n_cate));
// param_grads: host array of 8 device pointers receiving the gradients of w1, b1, w2, b2, ln_g,
// ln_b, cate, mm_proj bias (segments of 6R, R, 6R, 6, D, D, n_cate*D, D columns of a partial row),
// or NULL: the partial rows are left for the caller to sum (the trainer's one fbn_sum_jobs2 launch).
static int fields_bwd_impl(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                           const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                           float ln_eps, const float* w1, const float* b1, const float* w2, int R, int n_cate,
                           const float* cate, const float* X, const float* a, const float* cnt, const float* dV,
                           float* dhmm, short* dhmm16, float* partials, float* const* param_grads, float* gtab,
                           float* gvec, double* gnorm, long long V, const int* pos, void* sendbuf, int send_bf16,
                           int B, int L, int D, void* stream, long long dhmm16_lo, const int* slot_step = nullptr,
                           void* slot_cell = nullptr, int ring_n = 0, long long ring_stride = 0);
extern "C" int fbn_fields_bwd(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                              const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                              float ln_eps, const float* w1, const float* b1, const float* w2, int R, int n_cate,
                              const float* cate, const float* X, const float* a, const float* cnt, const float* dV, float* dhmm,
                              short* dhmm16, float* partials, float* const* param_grads, float* gtab, float* gvec,
                              double* gnorm, long long V, const int* pos, void* sendbuf, int send_bf16, int B,
                              int L, int D, void* stream) {
  return fields_bwd_impl(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, w1, b1, w2, R, n_cate, cate, X, a,
                         cnt, dV, dhmm, dhmm16, partials, param_grads, gtab, gvec, gnorm, V, pos, sendbuf, send_bf16, B,
                         L, D, stream, 0);
}
// fbn_fields_bwd with dhmm_img = split images of dhmm (hi, lo B*D elements further; bf16_fwd training)
extern "C" int fbn_fields_bwd_img(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                                  const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                                  float ln_eps, const float* w1, const float* b1, const float* w2, int R, int n_cate,
                                  const float* cate, const float* X, const float* a, const float* cnt, const float* dV,
                                  float* dhmm, void* dhmm_img, float* partials, float* const* param_grads,
                                  float* gtab, float* gvec, double* gnorm, long long V, const int* pos, void* sendbuf,
                                  int send_bf16, int B, int L, int D, void* stream) {
  if (!dhmm_img) { fbn_set_error("fbn_fields_bwd_img: dhmm_img"); return FBN_ERR_ARG; }
  return fields_bwd_impl(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, w1, b1, w2, R, n_cate, cate, X, a,
                         cnt, dV, dhmm, (short*)dhmm_img, partials, param_grads, gtab, gvec, gnorm, V, pos, sendbuf,
                         send_bf16, B, L, D, stream, (long long)B * D);
}
// The single-GPU trainer's form: the per-sample vectors written straight into deferred-gradient ring
// slot *step % ring_n of ring [ring_n][ring_stride] (ring_stride >= B*2*D floats), the slot's address
// to *cell -- the fold, the norm and the step tail read them there through Lp1 | FBN_GRAD_CELL, and the
// tail has nothing to copy.  dhmm_is_img: dhmm16 holds split images (fbn_fields_bwd_img).
extern "C" int fbn_fields_bwd_slot(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                                   const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                                   float ln_eps, const float* w1, const float* b1, const float* w2, int R, int n_cate,
                                   const float* cate, const float* X, const float* a, const float* cnt, const float* dV,
                                   float* dhmm, void* dhmm16, int dhmm_is_img, float* partials,
                                   float* const* param_grads, float* ring, int ring_n, long long ring_stride,
                                   const int* step, void* cell, double* gnorm, long long V, int B, int L, int D,
                                   void* stream) {
  if (!ring || !step || !cell || ring_n < 1 || ring_stride < (long long)B * 2 * D || (ring_stride & 3) ||
      ((uintptr_t)ring & 15) || (dhmm_is_img && !dhmm16)) {
    fbn_set_error("fbn_fields_bwd_slot: ring (16-B aligned), step, cell; ring_n >= 1, ring_stride >= B*2*D, % 4 == 0");
    return FBN_ERR_ARG;
  }
  return fields_bwd_impl(item_id, item_seq, likes, views, hmm, ln_g, ln_b, ln_eps, w1, b1, w2, R, n_cate, cate, X, a,
                         cnt, dV, dhmm, (short*)dhmm16, partials, param_grads, nullptr, ring, gnorm, V, nullptr, nullptr,
                         0, B, L, D, stream, dhmm_is_img ? (long long)B * D : 0, step, cell, ring_n, ring_stride);
}
static int fields_bwd_impl(const int64_t* item_id, const int64_t* item_seq, const int64_t* likes,
                           const int64_t* views, const float* hmm, const float* ln_g, const float* ln_b,
                           float ln_eps, const float* w1, const float* b1, const float* w2, int R, int n_cate,
                           const float* cate, const float* X, const float* a, const float* cnt, const float* dV,
                           float* dhmm, short* dhmm16, float* partials, float* const* param_grads, float* gtab,
                           float* gvec, double* gnorm, long long V, const int* pos, void* sendbuf, int send_bf16,
                           int B, int L, int D, void* stream, long long dhmm16_lo, const int* slot_step,
                           void* slot_cell, int ring_n, long long ring_stride) {
  if (B <= 0) return FBN_OK;
  if (L < 0 || L > 32 || R < 1 || R > FBN_MAXR) { fbn_set_error("fbn_fields_bwd: bad L/R"); return FBN_ERR_ARG; }
  FieldBwdArgs p;
  p.item_id = item_id; p.item_seq = L > 0 ? item_seq : nullptr; p.likes = likes; p.views = views;
  p.hmm = hmm; p.ln_g = ln_g; p.ln_b = ln_b; p.w1 = w1; p.b1 = b1; p.w2 = w2; p.cate = cate;
  p.X = X; p.a = a; p.cnt = cnt; p.dV = dV; p.dhmm = dhmm; p.dhmm16 = dhmm16; p.partials = partials;
  p.dhmm16_lo = dhmm16_lo;
  p.slot_step = slot_step; p.slot_cell = (float**)slot_cell; p.ring_n = ring_n; p.ring_stride = ring_stride;
  p.gtab = gtab; p.gvec = gvec; p.gnorm = gvec ? gnorm : nullptr; p.pos = pos; p.sendbuf = sendbuf;
  p.V = V; p.B = B; p.L = L; p.R = R; p.n_cate = n_cate; p.ln_eps = ln_eps;
  hipStream_t st = (hipStream_t)stream;
  int rc = !pos ? launch_fields_bwd<0>(p, D, st) : send_bf16 ? launch_fields_bwd<2>(p, D, st)
                                                               : launch_fields_bwd<1>(p, D, st);
  if (rc) return rc;
  if (!param_grads) return FBN_OK;   // deferred: the caller sums the partial rows (fbn_sum_jobs2, ld = P)
  return fbn_fields_reduce_partials(partials, param_grads, B, D, R, n_cate, st);
}

int fbn_fields_reduce_partials(const float* partials, float* const* param_grads, int B, int D, int R, int n_cate,
                               hipStream_t st) {
  const int P = 13 * R + 6 + 3 * D + n_cate * D;
  const int nblk = fields_grid(B, D, FBN_FB_MAXBLK);

  GradOuts o;
  const int sizes[8] = {6 * R, R, 6 * R, 6, D, D, n_cate * D, D};
  o.off[0] = 0;
  for (int j = 0; j < 8; ++j) {
    if (j < 7 && !param_grads[j]) {
      fbn_set_error("fbn_fields_bwd: null parameter-gradient destination");
      return FBN_ERR_ARG;
    }
    o.p[j] = param_grads[j];   // [7] (mm_proj bias) may be null: not written
    o.off[j + 1] = o.off[j] + sizes[j];
  }
  fbn_launch(reduce_partials_one16, dim3(fbn_cdiv(P, 16)), dim3(1024), 0, st, partials, nblk, P, o);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
