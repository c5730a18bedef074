// Retrieval: cosine similarity between L2-normalised vectors, the stage in front of the per-user lists.
//
//   fbn_knn_normalize   Xn[m] = x / |x| of a catalogue matrix (or of table rows gathered by id), once per space
//   fbn_knn_query_pool  Qn[u] = the normalised sum of the Xn rows of a user's history (slot order)
//   fbn_knn_scores      S[q][j] = <a_q, Xn[m0 + j]> for a chunk of the catalogue: the hot path, one pass
//                       over Xn on the exact f32-input MFMA
// Selection is fbn_rec_topk / fbn_rec_rank on S (recommend.hip): key order, tie rule, exclusion by id,
// carry across chunks and the NaN flag are theirs, so nothing here selects.
//
// Every score is ONE accumulator chain in ascending k: the K loop is cut into slabs of 32 only to bound
// the LDS image, and every slab's MFMAs add into the same registers, step t taking k = 2t (lanes 0..31)
// and k = 2t + 1 (lanes 32..63) -- the instruction is a k-ordered fmaf chain.  A score's bits therefore
// depend on its two vectors alone: not on Q, on the query's place in its tile, on the chunk (m0, Mc) or
// on the other queries of the call, and <a, b> == <b, a>.
#include <cstdio>

#include "common.h"

static bool knn_dim_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256; }

static void knn_err(const char* who, const char* what) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  fbn_set_error(msg);
}

// workgroups of 256 threads for `rows` rows of D/4 lanes each (grid-stride beyond the cap)
static int knn_grid(long long rows, int D) {
  const int spw = 64 / (D / 4);
  const long long waves = (rows + spw - 1) / spw;
  const long long blocks = (waves + 3) / 4;
  return blocks < 1 ? 1 : (blocks > 4096 ? 4096 : (int)blocks);
}

// v / |v| over the G lanes that hold one row (4 columns each); the zero row stays zero: no 0 * inf
template <int G>
__device__ __forceinline__ f32x4 knn_unit(f32x4 v) {
  const float ss = group_sum<G>(v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]);
  const float inv = ss > 0.f ? rsqrtf(ss) : 0.f;
  return v * inv;
}

// ------------------------------------------------------------------------------ normalise
struct KnnNormArgs {
  const float* X;            // [n_src][ldx]
  const int64_t* row_of;     // [M] or null (row m)
  float* Xn;                 // [M][D]
  int* err;
  long long n_src;
  int ldx, M;
};

template <int D>
__global__ void __launch_bounds__(256) knn_normalize_kernel(KnnNormArgs p) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (long long m0 = (long long)gw * SPW; m0 < p.M; m0 += (long long)nwaves * SPW) {
    const long long m = m0 + lane / G;
    if (m >= p.M) continue;
    const long long r = p.row_of ? p.row_of[m] : m;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (r >= 0 && r < p.n_src) x = *reinterpret_cast<const f32x4*>(p.X + r * p.ldx + 4 * q);
    else if (q == 0) atomicOr(p.err, 1);
    *reinterpret_cast<f32x4*>(p.Xn + m * D + 4 * q) = knn_unit<G>(x);
  }
}

extern "C" int fbn_knn_normalize(const float* X, int ldx, const int64_t* row_of, long long n_src, float* Xn, int M,
                                 int D, int* err, void* stream) {
  if (!knn_dim_ok(D)) {
    knn_err("fbn_knn_normalize", "vector length D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (ldx < D || (ldx & 3) || n_src < 0 || M < 0) {
    knn_err("fbn_knn_normalize", "need ldx >= D, ldx % 4 == 0, n_src >= 0 and M >= 0");
    return FBN_ERR_ARG;
  }
  if (M == 0) return FBN_OK;
  KnnNormArgs a;
  a.X = X; a.row_of = row_of; a.Xn = Xn; a.err = err; a.n_src = n_src; a.ldx = ldx; a.M = M;
  const dim3 grid(knn_grid(M, D)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(knn_normalize_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(knn_normalize_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(knn_normalize_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(knn_normalize_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(knn_normalize_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------------------ user query
struct KnnPoolArgs {
  const int64_t* item_seq;   // [U][L]
  const int* pos_of_id;      // [V] id -> catalogue position, negative: not in the catalogue
  const float* Xn;           // [M][D]
  float* Qn;                 // [U][D]
  int* n_used;               // [U]
  long long V;
  int U, L, M;
};

template <int D>
__global__ void __launch_bounds__(256) knn_query_pool_kernel(KnnPoolArgs p) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int u0 = gw * SPW; u0 < p.U; u0 += nwaves * SPW) {
    const int u = u0 + lane / G;
    if (u >= p.U) continue;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int n = 0;
    for (int t = 0; t < p.L; ++t) {                   // slot order; a repeated id counts each time
      const long long id = p.item_seq[(size_t)u * p.L + t];
      long long pos = -1;
      if (id > 0 && id < p.V) pos = p.pos_of_id[id];
      if (pos >= 0 && pos < p.M) {
        s += *reinterpret_cast<const f32x4*>(p.Xn + pos * D + 4 * q);
        ++n;
      }
    }
    *reinterpret_cast<f32x4*>(p.Qn + (size_t)u * D + 4 * q) = knn_unit<G>(s);
    if (q == 0) p.n_used[u] = n;
  }
}

extern "C" int fbn_knn_query_pool(const int64_t* item_seq, int U, int L, const int* pos_of_id, long long V,
                                  const float* Xn, int M, int D, float* Qn, int* n_used, void* stream) {
  if (!knn_dim_ok(D)) {
    knn_err("fbn_knn_query_pool", "vector length D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (L < 0 || L > 32) {
    knn_err("fbn_knn_query_pool", "history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (V < 0 || M < 0) {
    knn_err("fbn_knn_query_pool", "negative V or M");
    return FBN_ERR_ARG;
  }
  if (U <= 0) return FBN_OK;
  KnnPoolArgs a;
  a.item_seq = item_seq; a.pos_of_id = pos_of_id; a.Xn = Xn; a.Qn = Qn; a.n_used = n_used; a.V = V; a.U = U;
  a.L = item_seq ? L : 0; a.M = M;
  const dim3 grid(knn_grid(U, D)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(knn_query_pool_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(knn_query_pool_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(knn_query_pool_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(knn_query_pool_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(knn_query_pool_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------------------ scores
// One workgroup (4 waves as 2 x 2) owns 64 queries x 128 items; a wave owns 32 x 64 as two 32 x 32
// accumulators.  Per K slab of 32 both operand tiles go global -> registers -> LDS (the next slab's loads
// are in flight under this slab's MFMAs) as [row][36] f32 images.  v_mfma_f32_32x32x2_f32 reads
// A[lane & 31][lane >> 5], one dword per lane; here a lane reads 16 bytes and feeds four steps from them,
// so inside every group of 8 k the image is stored as {k0 k2 k4 k6 | k1 k3 k5 k7}: the lower lane half
// reads the even k, the upper the odd, and step s of the group is k = 2s, 2s + 1 -- ascending.  The row
// stride 36 (9 sixteen-byte slots, odd) puts the 16 rows of each ds_read_b128 lane group on 16 distinct
// slots of the 64 banks; a stride of 32 would put all 32 rows of a half on one.
#define KNN_BQ 64
#define KNN_BN 128
#define KNN_BK 32
#define KNN_LDK 36

struct KnnScoreArgs {
  const float* Qn;           // [Q][ldq] (q_pos null)
  const int64_t* q_pos;      // [Q] catalogue positions of item queries, or null
  const float* Xn;           // [M][D]
  float* S;                  // [Q][Mc]
  int ldq, M, Q, m0, Mc;
};

struct KnnFrag { f32x4 lo, hi; };   // 8 consecutive k of one row

__device__ __forceinline__ KnnFrag knn_load8(const float* row, int k) {
  KnnFrag f;
  const f32x4 z = {0.f, 0.f, 0.f, 0.f};
  f.lo = row ? *reinterpret_cast<const f32x4*>(row + k) : z;
  f.hi = row ? *reinterpret_cast<const f32x4*>(row + k + 4) : z;
  return f;
}
__device__ __forceinline__ void knn_store8(float* dst, const KnnFrag& f) {
  *reinterpret_cast<f32x4*>(dst) = (f32x4){f.lo[0], f.lo[2], f.hi[0], f.hi[2]};
  *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){f.lo[1], f.lo[3], f.hi[1], f.hi[3]};
}

template <int D>
__global__ void __launch_bounds__(256) knn_scores_kernel(KnnScoreArgs p) {
  __shared__ __attribute__((aligned(16))) float sA[KNN_BQ * KNN_LDK];
  __shared__ __attribute__((aligned(16))) float sB[KNN_BN * KNN_LDK];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6, wm = w >> 1, wn = w & 1, lr = lane & 31, lh = lane >> 5;
  constexpr int KB = D < KNN_BK ? D : KNN_BK;         // the slab: all of K at D = 16
  const int q0 = blockIdx.y * KNN_BQ;
  const long long j0 = (long long)blockIdx.x * KNN_BN;

  // this thread's staging units: row sr of the query tile and rows sr, sr + 64 of the item tile, the 8 k
  // at 8 * sg of each slab.  A null source is a zero row: past Q or Mc, or a query position outside [0, M).
  // (a unit past a short slab, 8 * sg >= KB, stores zeros that nothing reads.)
  const int sr = t >> 2, sg = t & 3;
  const bool live = 8 * sg < KB;
  const float* asrc = nullptr;
  if (live && q0 + sr < p.Q) {
    if (p.q_pos) {
      const long long m = p.q_pos[q0 + sr];
      if (m >= 0 && m < p.M) asrc = p.Xn + (size_t)m * D;
    } else {
      asrc = p.Qn + (size_t)(q0 + sr) * p.ldq;
    }
  }
  const float* bsrc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const long long j = j0 + sr + 64 * i;
    bsrc[i] = live && j < p.Mc ? p.Xn + ((size_t)p.m0 + j) * D : nullptr;
  }

  f32x16 acc[2];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;

  KnnFrag fa = knn_load8(asrc, 8 * sg), fb0 = knn_load8(bsrc[0], 8 * sg), fb1 = knn_load8(bsrc[1], 8 * sg);
#pragma unroll
  for (int k0 = 0; k0 < D; k0 += KB) {
    if (k0) __syncthreads();                          // the previous slab's reads are done
    knn_store8(sA + sr * KNN_LDK + 8 * sg, fa);
    knn_store8(sB + sr * KNN_LDK + 8 * sg, fb0);
    knn_store8(sB + (sr + 64) * KNN_LDK + 8 * sg, fb1);
    __syncthreads();
    if (k0 + KB < D) {
      fa = knn_load8(asrc, k0 + KB + 8 * sg);
      fb0 = knn_load8(bsrc[0], k0 + KB + 8 * sg);
      fb1 = knn_load8(bsrc[1], k0 + KB + 8 * sg);
    }
#pragma unroll
    for (int kk = 0; kk < KB / 8; ++kk) {
      const f32x4 af = *reinterpret_cast<const f32x4*>(sA + (wm * 32 + lr) * KNN_LDK + kk * 8 + lh * 4);
      f32x4 bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j)
        bf[j] = *reinterpret_cast<const f32x4*>(sB + (wn * 64 + j * 32 + lr) * KNN_LDK + kk * 8 + lh * 4);
#pragma unroll
      for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[j][s], acc[j], 0, 0, 0);
    }
  }

  // C/D map of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long long col = j0 + wn * 64 + j * 32 + lr;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const int row = q0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
      if (row < p.Q && col < p.Mc) p.S[(size_t)row * p.Mc + col] = acc[j][e];
    }
  }
}

extern "C" int fbn_knn_scores(const float* Qn, int ldq, const int64_t* q_pos, const float* Xn, int M, int Q, int m0,
                              int Mc, int D, float* S, void* stream) {
  if (!knn_dim_ok(D)) {
    knn_err("fbn_knn_scores", "vector length D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (M < 0 || Q < 0 || Mc < 0 || m0 < 0 || (long long)m0 + Mc > M) {
    knn_err("fbn_knn_scores", "need Q >= 0 and a chunk with m0 >= 0, Mc >= 0 and m0 + Mc <= M");
    return FBN_ERR_ARG;
  }
  if (Q > 65535 || (long long)Q * Mc > 0x7FFFFFFFll) {
    knn_err("fbn_knn_scores", "need Q <= 65535 and Q * Mc within 31 bits (score in chunks)");
    return FBN_ERR_ARG;
  }
  if (!q_pos && (ldq < D || (ldq & 3))) {
    knn_err("fbn_knn_scores", "need ldq >= D and ldq % 4 == 0");
    return FBN_ERR_ARG;
  }
  if (Q == 0 || Mc == 0) return FBN_OK;
  KnnScoreArgs a;
  a.Qn = Qn; a.q_pos = q_pos; a.Xn = Xn; a.S = S; a.ldq = ldq; a.M = M; a.Q = Q; a.m0 = m0; a.Mc = Mc;
  const dim3 grid(fbn_cdiv(Mc, KNN_BN), fbn_cdiv(Q, KNN_BQ)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(knn_scores_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(knn_scores_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(knn_scores_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(knn_scores_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(knn_scores_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
