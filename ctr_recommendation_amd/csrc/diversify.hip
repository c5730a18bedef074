// Diversity of the served lists: greedy maximal marginal relevance over each user's own candidate list,
// and the intra-list diversity of finished lists.
//
//   fbn_mmr_select   K greedy picks per user: pick_t = argmax of lam * rel_j - (1 - lam) * max_{s picked}
//                    sim(j, s) over the live unpicked slots, ties to the smaller slot
//   fbn_list_ild     ild[u] = mean over the pairs a < b of a list's live entries of 1 - sim(a, b), in f64
//
// sim is the cosine of retrieve.hip between rows of the same L2-normalised matrix Xn, and keeps that
// file's contract: ONE f32 fmaf chain in ascending k from a +0 accumulator, so its bits are those of
// fbn_knn_scores for the pair and depend on the two vectors only.  A chain may therefore not be split
// over lanes: every lane owns whole candidates and runs their chains itself, its own row in 16-byte
// global loads against the picked row, which the workgroup reads as an LDS broadcast.  One workgroup of
// 256 threads per user; nothing crosses workgroups, so a user's result depends on its own row only.
#include <cmath>
#include <cstdio>

#include "common.h"
#include "rec_key.h"

#define MMR_THREADS 256
#define MMR_OWN (FBN_MMR_MAX_C / MMR_THREADS)   // slots per thread: j = t + 256 i
#define MMR_KMAX 256
#define MMR_MAX_L 32     // history slots (fields_common.h: FBN_MAX_L)
static_assert(FBN_MMR_MAX_C % MMR_THREADS == 0, "every thread owns the same number of slots");

static bool div_dim_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256; }

static void div_err(const char* who, const char* what) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  fbn_set_error(msg);
}

// <x, s>: x a row of Xn in global memory, s the workgroup's row in LDS; 8 loads in flight at the most
template <int D>
__device__ __forceinline__ float div_chain(const float* __restrict__ x, const float* s) {
  float acc = 0.f;
#pragma unroll 8
  for (int k = 0; k < D; k += 4) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + k);
    const f32x4 b = *reinterpret_cast<const f32x4*>(s + k);
    acc = __fmaf_rn(a[0], b[0], acc);
    acc = __fmaf_rn(a[1], b[1], acc);
    acc = __fmaf_rn(a[2], b[2], acc);
    acc = __fmaf_rn(a[3], b[3], acc);
  }
  return acc;
}

// the workgroup's largest key: a 64-bit max over the wave, then over the four waves (red: 2 x 4 words,
// the parity alternates per call so that one barrier per call is enough)
__device__ __forceinline__ unsigned long long div_block_max(unsigned long long key, unsigned long long* red,
                                                            int parity) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  unsigned long long* r = red + 4 * parity;
  if ((threadIdx.x & 63) == 0) r[threadIdx.x >> 6] = key;
  __syncthreads();
  const unsigned long long a = r[0] > r[1] ? r[0] : r[1], b = r[2] > r[3] ? r[2] : r[3];
  return a > b ? a : b;
}

// ------------------------------------------------------------------------------ MMR selection
struct MmrArgs {
  const float* rel;            // [U][ldr]
  const int64_t* cand_pos;     // [U][ldp]
  const float* Xn;             // [M][D]
  const int64_t* item_id;      // [M]
  const int64_t* item_seq;     // [U][L] or null
  int64_t* out_slot; int64_t* out_index; int64_t* out_item;   // [U][K]
  float* out_rel; float* out_mmr; float* out_pen;             // [U][K]
  unsigned* status;
  int ldr, ldp, C, M, L, exclude, K;
  float lam;
};

template <int D>
__global__ void __launch_bounds__(MMR_THREADS) mmr_select_kernel(MmrArgs p) {
  __shared__ __attribute__((aligned(16))) float srow[D];     // the row picked last
  __shared__ int spos[FBN_MMR_MAX_C];                         // slot -> catalogue position, -1: not live
  __shared__ long long hist[MMR_MAX_L];
  __shared__ unsigned long long red[8];
  const int t = threadIdx.x, u = blockIdx.x;
  const int K = p.K, L = p.item_seq ? p.L : 0;
  const float lam = p.lam, oml = 1.0f - lam;
  if (t < L) hist[t] = p.item_seq[(size_t)u * L + t];
  __syncthreads();

  // this thread's slots: relevance, running penalty (the raw maximum; -inf before the first pick), and
  // whether the slot can still be picked
  float rel[MMR_OWN], pen[MMR_OWN];
  bool open[MMR_OWN];
  bool nan_seen = false;
#pragma unroll
  for (int i = 0; i < MMR_OWN; ++i) {
    const int j = t + MMR_THREADS * i;
    long long m = -1;
    rel[i] = 0.f;
    pen[i] = -__builtin_inff();
    if (j < p.C) {
      m = p.cand_pos[(size_t)u * p.ldp + j];
      if (m >= p.M) m = -1;
      if (m >= 0 && p.exclude && rec_id_excluded(hist, L, p.item_id[m])) m = -1;
    }
    if (m >= 0) {
      rel[i] = p.rel[(size_t)u * p.ldr + j];
      nan_seen |= rel[i] != rel[i];
    }
    open[i] = m >= 0;
    spos[j] = (int)m;
  }
  if (nan_seen) atomicOr(p.status, 1u);

  const size_t o0 = (size_t)u * K;
  int step = 0;
  for (; step < K; ++step) {
    // ---- scores and the arg-max
    float mmr[MMR_OWN];
    unsigned long long best = 0ull;
#pragma unroll
    for (int i = 0; i < MMR_OWN; ++i) {
      mmr[i] = (step == 0 ? __fmul_rn(lam, rel[i]) : __fmaf_rn(lam, rel[i], -__fmul_rn(oml, pen[i]))) + 0.0f;
      bool nan;
      const unsigned long long key = open[i] ? rec_key(mmr[i], (unsigned)(t + MMR_THREADS * i), nan) : 0ull;
      best = key > best ? key : best;
    }
    best = div_block_max(best, red, step & 1);
    if (best == 0ull) break;                           // no live unpicked slot is left (workgroup-uniform)
    const int js = (int)(0xFFFFFFFFu - (unsigned)best);
    const int ms = spos[js];

    // ---- the owner of the picked slot writes the step's outputs and closes the slot
    if ((js & (MMR_THREADS - 1)) == t) {
#pragma unroll
      for (int i = 0; i < MMR_OWN; ++i) {
        if (i != js / MMR_THREADS) continue;
        p.out_slot[o0 + step] = js;
        p.out_index[o0 + step] = ms;
        p.out_item[o0 + step] = p.item_id[ms];
        p.out_rel[o0 + step] = rel[i];
        p.out_mmr[o0 + step] = mmr[i];
        p.out_pen[o0 + step] = step == 0 ? 0.f : pen[i];
        open[i] = false;
      }
    }
    if (step + 1 == K) { ++step; break; }

    // ---- the picked row into LDS, then every open slot's similarity to it
    if (t < D / 4)
      *reinterpret_cast<f32x4*>(srow + 4 * t) = *reinterpret_cast<const f32x4*>(p.Xn + (size_t)ms * D + 4 * t);
    __syncthreads();
#pragma unroll
    for (int i = 0; i < MMR_OWN; ++i) {
      if (!open[i]) continue;
      const float sim = div_chain<D>(p.Xn + (size_t)spos[t + MMR_THREADS * i] * D, srow);
      pen[i] = fmaxf(pen[i], sim);
    }
    // (the next step's barrier in div_block_max orders these reads of srow before its next write)
  }

  // ---- the empty tail
  for (int k = step + t; k < K; k += MMR_THREADS) {
    p.out_slot[o0 + k] = -1;
    p.out_index[o0 + k] = -1;
    p.out_item[o0 + k] = -1;
    p.out_rel[o0 + k] = -__builtin_inff();
    p.out_mmr[o0 + k] = -__builtin_inff();
    p.out_pen[o0 + k] = 0.f;
  }
}

extern "C" int fbn_mmr_select(const float* rel, int ldr, const int64_t* cand_pos, int ldp, int U, int C,
                              const float* Xn, int M, int D, const int64_t* item_id, const int64_t* item_seq, int L,
                              int exclude, float lam, int K, int64_t* out_slot, int64_t* out_index, int64_t* out_item,
                              float* out_rel, float* out_mmr, float* out_pen, unsigned* status, void* stream) {
  const char* who = "fbn_mmr_select";
  if (K < 1 || K > MMR_KMAX) {
    div_err(who, "K must be in 1..256");
    return FBN_ERR_ARG;
  }
  if (C < 0 || C > FBN_MMR_MAX_C) {
    div_err(who, "C must be in 0..1024 (FBN_MMR_MAX_C)");
    return FBN_ERR_ARG;
  }
  if (!div_dim_ok(D)) {
    div_err(who, "vector length D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (L < 0 || L > MMR_MAX_L) {
    div_err(who, "history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (!std::isfinite(lam) || lam < 0.f || lam > 1.f) {
    div_err(who, "lam must be finite and in [0, 1]");
    return FBN_ERR_ARG;
  }
  if (ldr < C || ldp < C || U < 0 || U > 65535 || M < 0) {
    div_err(who, "need ldr >= C, ldp >= C, 0 <= U <= 65535 and M >= 0");
    return FBN_ERR_ARG;
  }
  if (U == 0 || C == 0) return FBN_OK;
  MmrArgs a;
  a.rel = rel; a.cand_pos = cand_pos; a.Xn = Xn; a.item_id = item_id; a.item_seq = L > 0 ? item_seq : nullptr;
  a.out_slot = out_slot; a.out_index = out_index; a.out_item = out_item; a.out_rel = out_rel; a.out_mmr = out_mmr;
  a.out_pen = out_pen; a.status = status; a.ldr = ldr; a.ldp = ldp; a.C = C; a.M = M; a.L = L; a.exclude = exclude;
  a.K = K; a.lam = lam;
  const dim3 grid(U), block(MMR_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(mmr_select_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(mmr_select_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(mmr_select_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(mmr_select_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(mmr_select_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------------------ intra-list diversity
// Thread a owns entry a of the list.  For b = 1 .. K-1 the workgroup reads row b from LDS and every
// thread a < b adds 1 - sim(a, b) to its own f64 sum -- ascending b -- and thread 0 adds the K sums in
// ascending a: the order of the additions is a function of (a, b) alone, and nothing is atomic.
struct IldArgs {
  const int64_t* list_pos;     // [U][ldp]
  const float* Xn;             // [M][D]
  double* ild;                 // [U]
  int* n_pairs;                // [U]
  int ldp, K, M;
};

template <int D>
__global__ void __launch_bounds__(MMR_THREADS) list_ild_kernel(IldArgs p) {
  __shared__ __attribute__((aligned(16))) float srow[2][D];
  __shared__ int spos[MMR_KMAX];
  __shared__ double ssum[MMR_KMAX];
  const int t = threadIdx.x, u = blockIdx.x, K = p.K;
  long long m = -1;
  if (t < K) {
    m = p.list_pos[(size_t)u * p.ldp + t];
    if (m >= p.M) m = -1;
  }
  spos[t] = (int)m;
  const int n = __syncthreads_count(m >= 0);
  const float* mine = p.Xn + (size_t)(m >= 0 ? m : 0) * D;
  double sum = 0.0;
  int buf = 0;
  for (int b = 1; b < K; ++b) {
    const int mb = spos[b];
    if (mb < 0) continue;                              // (workgroup-uniform)
    float* row = srow[buf];                            // two buffers in turn: one barrier per live b
    buf ^= 1;
    if (t < D / 4)
      *reinterpret_cast<f32x4*>(row + 4 * t) = *reinterpret_cast<const f32x4*>(p.Xn + (size_t)mb * D + 4 * t);
    __syncthreads();
    if (t < b && m >= 0) sum += 1.0 - (double)div_chain<D>(mine, row);
  }
  ssum[t] = sum;
  __syncthreads();
  if (t == 0) {
    double total = 0.0;
    for (int a = 0; a < K; ++a) total += ssum[a];
    const int pairs = n * (n - 1) / 2;
    p.n_pairs[u] = pairs;
    p.ild[u] = pairs > 0 ? total / (double)pairs : 0.0;
  }
}

extern "C" int fbn_list_ild(const int64_t* list_pos, int ldp, int U, int K, const float* Xn, int M, int D, double* ild,
                            int* n_pairs, void* stream) {
  const char* who = "fbn_list_ild";
  if (K < 1 || K > MMR_KMAX) {
    div_err(who, "K must be in 1..256");
    return FBN_ERR_ARG;
  }
  if (!div_dim_ok(D)) {
    div_err(who, "vector length D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (ldp < K || U < 0 || U > 65535 || M < 0) {
    div_err(who, "need ldp >= K, 0 <= U <= 65535 and M >= 0");
    return FBN_ERR_ARG;
  }
  if (U == 0) return FBN_OK;
  IldArgs a;
  a.list_pos = list_pos; a.Xn = Xn; a.ild = ild; a.n_pairs = n_pairs; a.ldp = ldp; a.K = K; a.M = M;
  const dim3 grid(U), block(MMR_THREADS);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(list_ild_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(list_ild_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(list_ild_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(list_ild_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(list_ild_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
