// Serving: score a catalogue of M items for U users and keep each user's K best on the device.
//
// The training forward (fields.hip) builds the five fields of every batch row from scratch: 21 table
// rows per row, and the mm projection's LayerNorm.  Scoring U x M (user, candidate) pairs through it
// repeats work that depends on one side only, so the pair's fields are composed from two caches:
//   per candidate m (fbn_rec_item_cache, once per catalogue):  X4[m] = ReLU(LN(hmm[m]))
//   per user u      (fbn_rec_hist_pool, once per call):        X5[u] = masked mean of E[seq[u]]
//   per pair        (fbn_rec_fields):  X1 = C[likes[m]], X2 = C[views[m]], X3 = E[item[m]] (contiguous
//                   over a run of candidates), X4[m], X5[u] (one L2-resident row), then SENET -- the same
//                   device functions in the same order as fields_fwd_kernel (fields_common.h), so the
//                   operands handed to the bilinear / MLP kernels are the same bits.
// fbn_rec_topk turns a chunk's logits into 64-bit keys {ordered logit, ~catalogue position} and keeps
// each user's K largest across chunks: integer compares only, no float atomics, no sort of U x M.
// fbn_rec_rank counts, in the same key order, how many eligible candidates of a user's full row of
// logits lie above one held-out target; fbn_rank_hist adds such ranks to an integer record from which
// the host derives HR / NDCG / MRR@K.
// The *_list entry points run the same kernels over per-user candidate lists cand_pos [U][ldp] of
// catalogue positions (negative: an empty slot): the pair's position is read through the list, and the
// key's low word carries the slot -- the index into the user's list -- instead of the position.
#include <cstdio>

#include "common.h"
#include "fields_common.h"
#include "rec_key.h"

static bool rec_dim_ok(int D) { return D == 16 || D == 32 || D == 64 || D == 128 || D == 256; }

// workgroups of 256 threads for `rows` rows of D/4 lanes each (grid-stride beyond the cap)
static int rec_grid(long long rows, int D) {
  const int spw = 64 / (D / 4);
  const long long waves = (rows + spw - 1) / spw;
  const long long blocks = (waves + 3) / 4;
  return blocks < 1 ? 1 : (blocks > 4096 ? 4096 : (int)blocks);
}

// ------------------------------------------------------------------------------ item-side cache
struct RecItemArgs {
  const int64_t* item_id; const int64_t* likes; const int64_t* views;   // [M]
  const float* hmm;          // [M][D] pre-LayerNorm mm projection (bias included)
  const float* ln_g; const float* ln_b;
  float* cache;              // [M][D] field 4
  int* err;
  long long V;
  int M, n_cate;
  float ln_eps;
};

template <int D>
__global__ void __launch_bounds__(256) rec_item_cache_kernel(RecItemArgs p) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (long long m0 = (long long)gw * SPW; m0 < p.M; m0 += (long long)nwaves * SPW) {
    const long long m = m0 + lane / G;
    if (m >= p.M) continue;
    const long long item = p.item_id[m], lk = p.likes[m], vw = p.views[m];
    if (item < 0 || item >= p.V || lk < 0 || lk >= p.n_cate || vw < 0 || vw >= p.n_cate) atomicOr(p.err, 1);
    const f32x4 h = *reinterpret_cast<const f32x4*>(p.hmm + m * D + 4 * q);
    *reinterpret_cast<f32x4*>(p.cache + m * D + 4 * q) = ln_relu<G>(h, p.ln_g, p.ln_b, p.ln_eps, q);
  }
}

extern "C" int fbn_rec_item_cache(const int64_t* item_id, const int64_t* likes, const int64_t* views,
                                  const float* hmm, const float* ln_g, const float* ln_b, float ln_eps, int n_cate,
                                  long long V, float* cache, int* err, int M, int D, void* stream) {
  if (!rec_dim_ok(D)) {
    fbn_set_error("fbn_rec_item_cache: embedding_dim D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (M <= 0) return FBN_OK;
  RecItemArgs a;
  a.item_id = item_id; a.likes = likes; a.views = views; a.hmm = hmm; a.ln_g = ln_g; a.ln_b = ln_b;
  a.cache = cache; a.err = err; a.V = V; a.M = M; a.n_cate = n_cate; a.ln_eps = ln_eps;
  const dim3 grid(rec_grid(M, D)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(rec_item_cache_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(rec_item_cache_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(rec_item_cache_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(rec_item_cache_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(rec_item_cache_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------------------ user-side pooling
struct RecHistArgs {
  const int64_t* item_seq;   // [U][L] or null (zero rows)
  const float* table;        // [V][D]
  float* hist;               // [U][D]
  int* err;
  long long V;
  int U, L;
};

#define REC_HCH 8   // history rows in flight per user before they are summed (slot order whatever the chunk)

template <int D>
__global__ void __launch_bounds__(256) rec_hist_pool_kernel(RecHistArgs p) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int L = p.item_seq ? p.L : 0;
  for (int u0 = gw * SPW; u0 < p.U; u0 += nwaves * SPW) {
    const int u = u0 + lane / G;
    if (u >= p.U) continue;
    f32x4 hs = {0.f, 0.f, 0.f, 0.f};
    int nnz = 0;
    bool bad = false;
    for (int t0 = 0; t0 < L; t0 += REC_HCH) {
      // branch-free: a padding or past-L slot reads row 0 and contributes +0 by a select
      f32x4 rows[REC_HCH];
      bool live[REC_HCH];
#pragma unroll
      for (int k = 0; k < REC_HCH; ++k) {
        const int t = t0 + k;
        long long s = t < L ? p.item_seq[(size_t)u * L + t] : 0;
        if (s < 0 || s >= p.V) { bad = true; s = 0; }
        live[k] = s != 0;
        rows[k] = *reinterpret_cast<const f32x4*>(p.table + s * D + 4 * q);
      }
#pragma unroll
      for (int k = 0; k < REC_HCH; ++k) {
        hs += live[k] ? rows[k] : (f32x4){0.f, 0.f, 0.f, 0.f};
        nnz += live[k] ? 1 : 0;
      }
    }
    if (bad) atomicOr(p.err, 1);
    const float cnt = fmaxf((float)nnz, 1.f);
    *reinterpret_cast<f32x4*>(p.hist + (size_t)u * D + 4 * q) = hs / cnt;
  }
}

extern "C" int fbn_rec_hist_pool(const int64_t* item_seq, const float* table, long long V, float* hist, int* err,
                                 int U, int L, int D, void* stream) {
  if (!rec_dim_ok(D)) {
    fbn_set_error("fbn_rec_hist_pool: embedding_dim D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (L < 0 || L > FBN_MAX_L) {
    fbn_set_error("fbn_rec_hist_pool: history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (U <= 0) return FBN_OK;
  RecHistArgs a;
  a.item_seq = L > 0 ? item_seq : nullptr; a.table = table; a.hist = hist; a.err = err; a.V = V; a.U = U; a.L = L;
  const dim3 grid(rec_grid(U, D)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(rec_hist_pool_kernel<16>, grid, block, 0, st, a); break;
    case 32: fbn_launch(rec_hist_pool_kernel<32>, grid, block, 0, st, a); break;
    case 64: fbn_launch(rec_hist_pool_kernel<64>, grid, block, 0, st, a); break;
    case 128: fbn_launch(rec_hist_pool_kernel<128>, grid, block, 0, st, a); break;
    default: fbn_launch(rec_hist_pool_kernel<256>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ------------------------------------------------------------------------------ pair composition + SENET
struct RecFieldArgs {
  const int64_t* item_id; const int64_t* likes; const int64_t* views;   // [M] catalogue columns
  const float* cache;        // [M][D] field 4 (fbn_rec_item_cache)
  const float* hist;         // [U][D] field 5 (fbn_rec_hist_pool)
  const float* cate;         // [n_cate][D]
  const float* table;        // [V][D]
  const float* w1; const float* b1; const float* w2; const float* b2;   // SENET [R][6],[R],[6][R],[6]
  float* Vc;                 // [P][5][D] fields 1..5 after SENET (optional)
  short* Vc16;               // bf16 copy (optional)
  void* c;                   // [P][ldc] float or bf16 (c16): cols [0,5D) <- V (optional)
  float* a_out;              // [P][6] (optional)
  int* err;
  const int64_t* cand_pos;   // [U][ldp] per-user lists (the list kernel only)
  long long V;
  int U, m0, Mc, ldc, R, n_cate, c16;   // list kernel: m0 / Mc are the first slot c0 / the slot count Cc
  int ldp, M;
};

// Pair row b = (user u, catalogue position m), this lane's 4 columns q.  LIST: m < 0 is an empty slot --
// no table or cache read, X1..X4 = 0 -- and the rest runs unchanged, so the row is the SENET of
// (0, 0, 0, 0, hist[u]): defined operands for the GEMMs, and no flag.
template <int D, bool LIST>
__device__ __forceinline__ void rec_pair_row(const RecFieldArgs& p, int u, long long m, long long b, int q) {
  constexpr int G = D / 4;
  // ---------------- ids (validated as fbn_fields_fwd does: a bad id reads row 0 / a zero row)
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 c1 = zero, c2 = zero, rit = zero, x4 = zero;
  bool bad = false;
  if (!LIST || m >= 0) {
    long long item = p.item_id[m], lk = p.likes[m], vw = p.views[m];
    if (lk < 0 || lk >= p.n_cate) { bad = true; lk = 0; }
    if (vw < 0 || vw >= p.n_cate) { bad = true; vw = 0; }
    if (item < 0 || item >= p.V) { bad = true; item = -1; }
    c1 = *reinterpret_cast<const f32x4*>(p.cate + lk * D + 4 * q);
    c2 = *reinterpret_cast<const f32x4*>(p.cate + vw * D + 4 * q);
    if (item >= 0) rit = *reinterpret_cast<const f32x4*>(p.table + item * D + 4 * q);
    x4 = *reinterpret_cast<const f32x4*>(p.cache + m * D + 4 * q);
  }
  const f32x4 x5 = *reinterpret_cast<const f32x4*>(p.hist + (size_t)u * D + 4 * q);
  if (bad) atomicOr(p.err, 1);

  // ---------------- SENET
  const f32x4 xs[5] = {c1, c2, rit, x4, x5};
  float z[6];
  z[0] = 0.f;
#pragma unroll
  for (int f = 0; f < 5; ++f) z[f + 1] = group_sum<G>(xs[f][0] + xs[f][1] + xs[f][2] + xs[f][3]) / (float)D;
  float qv[FBN_MAXR], a[6];
  senet_excite<D>(z, p.w1, p.b1, p.w2, p.b2, p.R, qv, a);

  // ---------------- stores
  float* Vb = p.Vc ? p.Vc + (size_t)b * 5 * D + 4 * q : nullptr;
  float* cb = (p.c && !p.c16) ? (float*)p.c + (size_t)b * p.ldc + 4 * q : nullptr;
  short* cb16 = (p.c && p.c16) ? (short*)p.c + (size_t)b * p.ldc + 4 * q : nullptr;
#pragma unroll
  for (int f = 0; f < 5; ++f) {
    const f32x4 v = xs[f] * a[f + 1];
    if (p.Vc) *reinterpret_cast<f32x4*>(Vb + f * D) = v;
    const bf16x4 v16 = (bf16x4){f2bf(v[0]), f2bf(v[1]), f2bf(v[2]), f2bf(v[3])};
    if (cb16) *reinterpret_cast<bf16x4*>(cb16 + f * D) = v16;
    else if (cb) *reinterpret_cast<f32x4*>(cb + f * D) = v;
    if (p.Vc16) *reinterpret_cast<bf16x4*>(p.Vc16 + ((size_t)b * 5 + f) * D + 4 * q) = v16;
  }
  if (p.a_out) {
#pragma unroll
    for (int f = 0; f < 6; ++f)
      if (f % G == q) p.a_out[(size_t)b * 6 + f] = a[f];   // G may be < 6 (D = 16)
  }
}

// D/4 lanes per pair row, 64/(D/4) rows per wave.  LIST: a row's catalogue position comes from the
// user's list (one 8-byte read per lane group, the same address in all its lanes), so the row indices
// of a wave's 16-byte loads are per lane group instead of consecutive; everything after is the same.
template <int D, bool LIST>
__global__ void __launch_bounds__(256) rec_fields_kernel(RecFieldArgs p) {
  constexpr int G = D / 4, SPW = 64 / G;
  const int lane = threadIdx.x & 63, q = lane % G;
  const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const long long P = (long long)p.U * p.Mc;
  for (long long r0 = (long long)gw * SPW; r0 < P; r0 += (long long)nwaves * SPW) {
    const long long b = r0 + lane / G;            // pair row u * Mc + (m - m0)
    if (b >= P) continue;
    const int u = (int)(b / p.Mc);
    long long m = p.m0 + (b - (long long)u * p.Mc);
    if (LIST) {
      m = p.cand_pos[(size_t)u * p.ldp + m];      // slot -> catalogue position
      if (m >= p.M) { atomicOr(p.err, 1); m = -1; }
    }
    rec_pair_row<D, LIST>(p, u, m, b, q);
  }
}

// fbn_last_error() names the entry point the caller used, whichever of a shared check refused
static void rec_err(const char* who, const char* what) {
  char msg[192];
  snprintf(msg, sizeof(msg), "%s: %s", who, what);
  fbn_set_error(msg);
}

template <bool LIST>
static int rec_fields_launch(const char* who, RecFieldArgs& a, int D, void* stream) {
  if (!rec_dim_ok(D)) {
    rec_err(who, "embedding_dim D must be one of 16,32,64,128,256");
    return FBN_ERR_ARG;
  }
  if (a.R < 1 || a.R > FBN_MAXR || (a.ldc & 3) || a.m0 < 0) {
    rec_err(who, LIST ? "need 1 <= R <= 8, ldc % 4 == 0, c0 >= 0" : "need 1 <= R <= 8, ldc % 4 == 0, m0 >= 0");
    return FBN_ERR_ARG;
  }
  if (LIST && (a.M < 0 || (long long)a.ldp < (long long)a.m0 + a.Mc)) {
    rec_err(who, "need M >= 0 and ldp >= c0 + Cc");
    return FBN_ERR_ARG;
  }
  if (a.U <= 0 || a.Mc <= 0) return FBN_OK;
  if ((long long)a.U * a.Mc > 0x7FFFFFFFll) {
    rec_err(who, LIST ? "U * Cc pair rows must fit 31 bits (score in chunks)"
                      : "U * Mc pair rows must fit 31 bits (score in chunks)");
    return FBN_ERR_ARG;
  }
  const dim3 grid(rec_grid((long long)a.U * a.Mc, D)), block(256);
  hipStream_t st = (hipStream_t)stream;
  switch (D) {
    case 16: fbn_launch(rec_fields_kernel<16, LIST>, grid, block, 0, st, a); break;
    case 32: fbn_launch(rec_fields_kernel<32, LIST>, grid, block, 0, st, a); break;
    case 64: fbn_launch(rec_fields_kernel<64, LIST>, grid, block, 0, st, a); break;
    case 128: fbn_launch(rec_fields_kernel<128, LIST>, grid, block, 0, st, a); break;
    default: fbn_launch(rec_fields_kernel<256, LIST>, grid, block, 0, st, a); break;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_rec_fields(const int64_t* item_id, const int64_t* likes, const int64_t* views, const float* cache,
                              const float* hist, const float* cate, int n_cate, const float* table, long long V,
                              const float* w1, const float* b1, const float* w2, const float* b2, int R, float* Vc,
                              short* Vc16, void* c, int ldc, int c_bf16, float* a_out, int* err, int U, int m0, int Mc,
                              int D, void* stream) {
  RecFieldArgs a;
  a.item_id = item_id; a.likes = likes; a.views = views; a.cache = cache; a.hist = hist; a.cate = cate;
  a.table = table; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.Vc = Vc; a.Vc16 = Vc16; a.c = c; a.a_out = a_out;
  a.err = err; a.V = V; a.U = U; a.m0 = m0; a.Mc = Mc; a.ldc = ldc; a.R = R; a.n_cate = n_cate; a.c16 = c_bf16;
  a.cand_pos = nullptr; a.ldp = 0; a.M = 0;
  return rec_fields_launch<false>("fbn_rec_fields", a, D, stream);
}

extern "C" int fbn_rec_fields_list(const int64_t* item_id, const int64_t* likes, const int64_t* views,
                                   const float* cache, const float* hist, const float* cate, int n_cate,
                                   const float* table, long long V, const float* w1, const float* b1, const float* w2,
                                   const float* b2, int R, float* Vc, short* Vc16, void* c, int ldc, int c_bf16,
                                   float* a_out, int* err, int U, const int64_t* cand_pos, int ldp, int c0, int Cc,
                                   int M, int D, void* stream) {
  RecFieldArgs a;
  a.item_id = item_id; a.likes = likes; a.views = views; a.cache = cache; a.hist = hist; a.cate = cate;
  a.table = table; a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.Vc = Vc; a.Vc16 = Vc16; a.c = c; a.a_out = a_out;
  a.err = err; a.V = V; a.U = U; a.m0 = c0; a.Mc = Cc; a.ldc = ldc; a.R = R; a.n_cate = n_cate; a.c16 = c_bf16;
  a.cand_pos = cand_pos; a.ldp = ldp; a.M = M;
  return rec_fields_launch<true>("fbn_rec_fields_list", a, D, stream);
}

// ------------------------------------------------------------------------------ top-K selection
// key = {ordered image of the f32 logit (32) | 0xFFFFFFFF - catalogue position (32)}: unique per
// candidate, and a larger key is a larger logit or, on equal logits, a smaller position.  0 is the
// "no candidate" key (excluded, filtered out, or an empty slot); a NaN logit takes the high word 1,
// below -inf's 0x007FFFFF (rec_key.h).
#define REC_TILE 256     // keys a workgroup takes in per round
#define REC_SEG 1024     // candidates per workgroup of the selection launch
#define REC_KMAX 256

struct RecTopkArgs {
  const float* logits;        // mode 0: [U][Mc] chunk logits
  const int64_t* item_id;     // [M] catalogue ids
  const int64_t* item_seq;    // [U][L] or null
  unsigned long long* carry;  // [U][K] running K best (mode 1: read, then rewritten)
  unsigned long long* ws;     // [U][nseg][K] per-segment K best (mode 0: written; mode 1: read)
  int64_t* out_index; int64_t* out_item; float* out_logit; float* out_prob;   // [U][K] (mode 1, optional)
  unsigned* status;
  int U, m0, Mc, L, exclude, K, nseg, mode;
  // per-user lists (fbn_rec_topk_list; cand_pos null: the catalogue): column m0 + j of the chunk is slot
  // m0 + j of cand_pos [U][ldp], the key's low word carries the slot, and out_slot [U][K] receives it
  const int64_t* cand_pos;
  int64_t* out_slot;
  int ldp, M;
};

// One workgroup keeps the K largest of a key stream: buf[0, 256) is the running list (descending,
// zeros past the keys seen), buf[256, 512) takes a tile of 256 new keys -- those that cannot enter
// the K best (<= the current K-th) are dropped first, a tile left empty is skipped -- and a bitonic
// sort of the 512 puts the K best back in front.
// mode 0: the stream is segment blockIdx.x of user blockIdx.y's chunk logits -> ws[u][seg][K];
// mode 1: the stream is the user's carried list followed by its segment lists -> carry[u][K] + outputs.
__global__ void __launch_bounds__(256) rec_topk_kernel(RecTopkArgs p) {
  __shared__ unsigned long long buf[2 * REC_TILE];
  __shared__ long long hist[FBN_MAX_L];
  const int t = threadIdx.x, u = blockIdx.y, seg = blockIdx.x;
  const int K = p.K, L = p.item_seq ? p.L : 0;
  buf[t] = 0ull;
  int n, base = 0;
  if (p.mode == 0) {
    base = seg * REC_SEG;
    n = min(REC_SEG, p.Mc - base);
    if (t < L) hist[t] = p.item_seq[(size_t)u * L + t];
  } else {
    n = K * (1 + p.nseg);
  }
  __syncthreads();
  for (int i0 = 0; i0 < n; i0 += REC_TILE) {
    const int i = i0 + t;
    unsigned long long key = 0ull;
    if (i < n) {
      if (p.mode == 0) {
        const int j = base + i;
        const long long col = (long long)p.m0 + j;      // the key's low word: position, or slot of a list
        long long m = col;
        if (p.cand_pos) {
          m = p.cand_pos[(size_t)u * p.ldp + col];
          if (m >= p.M) m = -1;
        }
        if (m >= 0) {                                   // an empty slot keeps key 0, whatever its logit holds
          bool nan;
          key = rec_key(p.logits[(size_t)u * p.Mc + j], (unsigned)col, nan);
          if (nan) atomicOr(p.status, 1u);
          if (p.exclude) {
            if (rec_id_excluded(hist, L, p.item_id[m])) key = 0ull;
          }
        }
      } else {
        key = i < K ? p.carry[(size_t)u * K + i] : p.ws[(size_t)u * p.nseg * K + (i - K)];
      }
    }
    if (key <= buf[K - 1]) key = 0ull;               // cannot enter the K best
    if (!__syncthreads_or(key != 0ull)) continue;    // (workgroup-uniform)
    buf[REC_TILE + t] = key;
    __syncthreads();
    for (int k = 2; k <= 2 * REC_TILE; k <<= 1) {
      for (int j = k >> 1; j > 0; j >>= 1) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
        const unsigned long long x = buf[lo], y = buf[hi];
        const bool desc = (lo & k) == 0;
        if ((x < y) == desc) { buf[lo] = y; buf[hi] = x; }
        __syncthreads();
      }
    }
  }
  if (t >= K) return;
  const unsigned long long key = buf[t];
  if (p.mode == 0) {
    p.ws[((size_t)u * p.nseg + seg) * K + t] = key;
    return;
  }
  const size_t o = (size_t)u * K + t;
  p.carry[o] = key;
  if (!p.out_index) return;
  const unsigned col = 0xFFFFFFFFu - (unsigned)key;
  long long pos = col;
  if (p.cand_pos && key != 0ull) {                     // a key only ever came from a live slot of this list;
    pos = col < (unsigned)p.ldp ? p.cand_pos[(size_t)u * p.ldp + col] : -1;   // a foreign carry reads nothing
    if (pos >= p.M) pos = -1;
  }
  if (key == 0ull || pos < 0) {
    if (p.cand_pos) p.out_slot[o] = -1;
    p.out_index[o] = -1;
    p.out_item[o] = -1;
    p.out_logit[o] = -__builtin_inff();
    p.out_prob[o] = 0.f;
  } else {
    if (p.cand_pos) p.out_slot[o] = (int64_t)col;
    const float x = rec_key_logit(key);
    p.out_index[o] = (int64_t)pos;
    p.out_item[o] = p.item_id[pos];
    p.out_logit[o] = x;
    p.out_prob[o] = 1.f / (1.f + expf(-x));          // the head's sigmoid (mlp.hip head_lane)
  }
}

static int rec_topk_check(const char* who, int U, int Mc, int K) {
  if (K < 1 || K > REC_KMAX) {
    rec_err(who, "K must be in 1..256");
    return FBN_ERR_ARG;
  }
  if (U < 0 || Mc < 0) {
    rec_err(who, "negative U or Mc");
    return FBN_ERR_ARG;
  }
  return FBN_OK;
}

extern "C" size_t fbn_rec_topk_workspace_size(int U, int Mc, int K) {
  if (rec_topk_check("fbn_rec_topk", U, Mc, K)) return 0;
  return (size_t)U * (size_t)fbn_cdiv(Mc, REC_SEG) * (size_t)K * sizeof(unsigned long long);
}

// the checks and the two launches of fbn_rec_topk / fbn_rec_topk_list (a: the pointers and list fields)
static int rec_topk_run(const char* who, RecTopkArgs& a, int U, int m0, int Mc, int L, int exclude, int K,
                        size_t ws_bytes, void* stream) {
  if (int rc = rec_topk_check(who, U, Mc, K)) return rc;
  if (L < 0 || L > FBN_MAX_L) {
    rec_err(who, "history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (m0 < 0 || (long long)U * Mc > 0x7FFFFFFFll || U > 65535) {
    rec_err(who, "need m0 >= 0 (the first column of the chunk), U <= 65535 and U * Mc within 31 bits");
    return FBN_ERR_ARG;
  }
  if (a.out_index && !(a.out_item && a.out_logit && a.out_prob)) {
    rec_err(who, "the four outputs come together");
    return FBN_ERR_ARG;
  }
  if (ws_bytes < fbn_rec_topk_workspace_size(U, Mc, K)) {
    rec_err(who, "workspace smaller than fbn_rec_topk_workspace_size(U, Mc, K)");
    return FBN_ERR_ARG;
  }
  if (U == 0) return FBN_OK;
  if (L <= 0) a.item_seq = nullptr;
  a.U = U; a.m0 = m0; a.Mc = Mc; a.L = L; a.exclude = exclude; a.K = K;
  a.nseg = fbn_cdiv(Mc, REC_SEG);
  hipStream_t st = (hipStream_t)stream;
  if (a.nseg > 0) {
    a.mode = 0;
    fbn_launch(rec_topk_kernel, dim3(a.nseg, U), dim3(256), 0, st, a);
    FBN_CHECK_LAUNCH();
  }
  a.mode = 1;
  fbn_launch(rec_topk_kernel, dim3(1, U), dim3(256), 0, st, a);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_rec_topk(const float* logits, int U, int m0, int Mc, const int64_t* item_id,
                            const int64_t* item_seq, int L, int exclude, int K, unsigned long long* carry, void* ws,
                            size_t ws_bytes, int64_t* out_index, int64_t* out_item, float* out_logit, float* out_prob,
                            unsigned* status, void* stream) {
  RecTopkArgs a;
  a.logits = logits; a.item_id = item_id; a.item_seq = item_seq; a.carry = carry; a.ws = (unsigned long long*)ws;
  a.out_index = out_index; a.out_item = out_item; a.out_logit = out_logit; a.out_prob = out_prob; a.status = status;
  a.cand_pos = nullptr; a.out_slot = nullptr; a.ldp = 0; a.M = 0;
  return rec_topk_run("fbn_rec_topk", a, U, m0, Mc, L, exclude, K, ws_bytes, stream);
}

extern "C" int fbn_rec_topk_list(const float* logits, int U, int c0, int Cc, const int64_t* cand_pos, int ldp, int M,
                                 const int64_t* item_id, const int64_t* item_seq, int L, int exclude, int K,
                                 unsigned long long* carry, void* ws, size_t ws_bytes, int64_t* out_slot,
                                 int64_t* out_index, int64_t* out_item, float* out_logit, float* out_prob,
                                 unsigned* status, void* stream) {
  if (c0 < 0 || M < 0 || (long long)ldp < (long long)c0 + Cc) {
    rec_err("fbn_rec_topk_list", "need c0 >= 0, M >= 0 and ldp >= c0 + Cc");
    return FBN_ERR_ARG;
  }
  if ((out_index != nullptr) != (out_slot != nullptr)) {
    rec_err("fbn_rec_topk_list", "the five outputs come together");
    return FBN_ERR_ARG;
  }
  RecTopkArgs a;
  a.logits = logits; a.item_id = item_id; a.item_seq = item_seq; a.carry = carry; a.ws = (unsigned long long*)ws;
  a.out_index = out_index; a.out_item = out_item; a.out_logit = out_logit; a.out_prob = out_prob; a.status = status;
  a.cand_pos = cand_pos; a.out_slot = out_slot; a.ldp = ldp; a.M = M;
  return rec_topk_run("fbn_rec_topk_list", a, U, c0, Cc, L, exclude, K, ws_bytes, stream);
}

// ------------------------------------------------------------------------------ rank of a held-out item
// rank[u] = 1 + the number of eligible candidates whose rec_key is above the target's, over the user's
// whole row of logits [U][ld]: the place fbn_rec_topk would give the target, without selecting.  One
// workgroup per (user, REC_SEG candidates) counts two predicates with wave ballots and adds its two
// integers to rank[u] / n_eligible[u]: integer atomics, so the sums do not depend on launch order.
struct RecRankArgs {
  const float* logits;         // [U][ld]
  const int64_t* item_id;      // [M]
  const int64_t* item_seq;     // [U][L] or null
  const int64_t* target_pos;   // [U]
  int* rank; int* n_eligible;  // [U]
  unsigned* status;
  int U, M, ld, L, exclude;
  // per-user lists (fbn_rec_rank_list; cand_pos null: the catalogue, C == M): the C columns of logits are
  // the slots of cand_pos [U][ldp], target_pos holds slots, and the key's low word is the slot
  const int64_t* cand_pos;
  int ldp, C;
};

// the catalogue position behind column j of user u's logits (0 <= j < C), or -1 for an empty slot
__device__ __forceinline__ long long rec_rank_pos(const RecRankArgs& p, int u, long long j) {
  if (!p.cand_pos) return j;
  const long long m = p.cand_pos[(size_t)u * p.ldp + j];
  return m < p.M ? m : -1;
}

// a target is ranked when it names a column with a catalogue position whose item is not the padding item
__device__ __forceinline__ bool rec_rank_valid(const RecRankArgs& p, int u, long long t) {
  if (t < 0 || t >= p.C) return false;
  const long long m = rec_rank_pos(p, u, t);
  return m >= 0 && p.item_id[m] != 0;
}

__global__ void __launch_bounds__(256) rec_rank_init_kernel(RecRankArgs p) {
  const int u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= p.U) return;
  const long long t = p.target_pos[u];
  const bool valid = rec_rank_valid(p, u, t);
  if (valid) {
    bool nan;
    rec_key(p.logits[(size_t)u * p.ld + t], (unsigned)t, nan);
    if (nan) atomicOr(p.status, 1u);
  }
  p.rank[u] = valid ? 1 : 0;
  p.n_eligible[u] = 0;
}

__global__ void __launch_bounds__(256) rec_rank_kernel(RecRankArgs p) {
  __shared__ long long hist[FBN_MAX_L];
  __shared__ unsigned long long tkey_s;
  __shared__ int valid_s;
  __shared__ int cnt[4][2];
  const int t = threadIdx.x, u = blockIdx.y, seg = blockIdx.x;
  const int L = p.item_seq ? p.L : 0;
  const int base = seg * REC_SEG, n = min(REC_SEG, p.C - base);
  const long long tp = p.target_pos[u];
  if (t < L) hist[t] = p.item_seq[(size_t)u * L + t];
  if (t == 0) {
    const bool valid = rec_rank_valid(p, u, tp);
    bool nan;
    tkey_s = valid ? rec_key(p.logits[(size_t)u * p.ld + tp], (unsigned)tp, nan) : 0ull;
    valid_s = valid;
  }
  __syncthreads();
  const unsigned long long tkey = tkey_s;
  const bool valid = valid_s != 0;
  int above = 0, elig = 0;                                  // wave-uniform
  for (int i0 = 0; i0 < n; i0 += 256) {
    const int i = i0 + t;
    bool e = false, g = false;
    if (i < n) {
      const long long j = (long long)base + i;            // column: catalogue position, or slot of a list
      const long long m = rec_rank_pos(p, u, j);
      e = m >= 0;                                          // an empty slot is never eligible
      if (e && p.exclude) {
        const long long id = p.item_id[m];
        bool in_hist = false;
        for (int l = 0; l < L; ++l) in_hist |= hist[l] != 0 && hist[l] == id;
        e = id != 0 && (j == tp || !in_hist);             // the target stays eligible inside its own history
      }
      bool nan;
      g = e && valid && j != tp && rec_key(p.logits[(size_t)u * p.ld + j], (unsigned)j, nan) > tkey;
    }
    elig += __popcll(__ballot(e));
    above += __popcll(__ballot(g));
  }
  if ((t & 63) == 0) { cnt[t >> 6][0] = above; cnt[t >> 6][1] = elig; }
  __syncthreads();
  if (t == 0) {
    const int a = cnt[0][0] + cnt[1][0] + cnt[2][0] + cnt[3][0];
    const int e = cnt[0][1] + cnt[1][1] + cnt[2][1] + cnt[3][1];
    if (a) atomicAdd(p.rank + u, a);
    if (e) atomicAdd(p.n_eligible + u, e);
  }
}

// the two launches of fbn_rec_rank / fbn_rec_rank_list
static int rec_rank_launch(const RecRankArgs& a, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  fbn_launch(rec_rank_init_kernel, dim3(fbn_cdiv(a.U, 256)), dim3(256), 0, st, a);
  FBN_CHECK_LAUNCH();
  const int nseg = fbn_cdiv(a.C, REC_SEG);
  if (nseg > 0) {
    fbn_launch(rec_rank_kernel, dim3(nseg, a.U), dim3(256), 0, st, a);
    FBN_CHECK_LAUNCH();
  }
  return FBN_OK;
}

extern "C" int fbn_rec_rank(const float* logits, int ld, int U, int M, const int64_t* item_id,
                            const int64_t* item_seq, int L, int exclude, const int64_t* target_pos, int* rank,
                            int* n_eligible, unsigned* status, void* stream) {
  if (L < 0 || L > FBN_MAX_L) {
    fbn_set_error("fbn_rec_rank: history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (U < 0 || U > 65535 || M < 0 || ld < M) {
    fbn_set_error("fbn_rec_rank: need 0 <= U <= 65535, M >= 0 and ld >= M");
    return FBN_ERR_ARG;
  }
  if (U == 0) return FBN_OK;
  RecRankArgs a;
  a.logits = logits; a.item_id = item_id; a.item_seq = L > 0 ? item_seq : nullptr; a.target_pos = target_pos;
  a.rank = rank; a.n_eligible = n_eligible; a.status = status; a.U = U; a.M = M; a.ld = ld; a.L = L;
  a.exclude = exclude; a.cand_pos = nullptr; a.ldp = 0; a.C = M;
  return rec_rank_launch(a, stream);
}

extern "C" int fbn_rec_rank_list(const float* logits, int ld, int U, int C, const int64_t* cand_pos, int ldp, int M,
                                 const int64_t* item_id, const int64_t* item_seq, int L, int exclude,
                                 const int64_t* target_slot, int* rank, int* n_eligible, unsigned* status,
                                 void* stream) {
  if (L < 0 || L > FBN_MAX_L) {
    fbn_set_error("fbn_rec_rank_list: history length L must be in 0..32");
    return FBN_ERR_ARG;
  }
  if (U < 0 || U > 65535 || C < 0 || ld < C || ldp < C || M < 0) {
    fbn_set_error("fbn_rec_rank_list: need 0 <= U <= 65535, C >= 0, ld >= C, ldp >= C and M >= 0");
    return FBN_ERR_ARG;
  }
  if (U == 0) return FBN_OK;
  RecRankArgs a;
  a.logits = logits; a.item_id = item_id; a.item_seq = L > 0 ? item_seq : nullptr; a.target_pos = target_slot;
  a.rank = rank; a.n_eligible = n_eligible; a.status = status; a.U = U; a.M = M; a.ld = ld; a.L = L;
  a.exclude = exclude; a.cand_pos = cand_pos; a.ldp = ldp; a.C = C;
  return rec_rank_launch(a, stream);
}

// ------------------------------------------------------------------------------ rank record
// rec[0] ranks <= 0 (not ranked), rec[r] ranks == r for 1 <= r <= 256, rec[257] ranks > 256,
// rec[258] the sum of the ranks >= 1, rec[259] their number: a histogram per workgroup in LDS, then
// one integer atomic per non-empty word.  No floating point: HR / NDCG / MRR@K are host functions of
// these integers, additive over calls.
#define REC_RANK_WORDS FBN_RANK_REC_WORDS
static_assert(REC_RANK_WORDS == 1 + 256 + 3, "not ranked, ranks 1..256, above, sum, count");

__global__ void __launch_bounds__(256) rank_hist_kernel(const int* rank, long long n, unsigned long long* rec) {
  __shared__ unsigned long long h[REC_RANK_WORDS];
  const int t = threadIdx.x;
  for (int i = t; i < REC_RANK_WORDS; i += 256) h[i] = 0ull;
  __syncthreads();
  unsigned long long sum = 0ull, ranked = 0ull;
  for (long long i = (long long)blockIdx.x * 256 + t; i < n; i += (long long)gridDim.x * 256) {
    const int r = rank[i];
    atomicAdd(&h[r < 1 ? 0 : (r > 256 ? 257 : r)], 1ull);
    if (r >= 1) { sum += (unsigned long long)r; ++ranked; }
  }
  if (ranked) { atomicAdd(&h[258], sum); atomicAdd(&h[259], ranked); }
  __syncthreads();
  for (int i = t; i < REC_RANK_WORDS; i += 256)
    if (h[i]) atomicAdd(rec + i, h[i]);
}

extern "C" int fbn_rank_hist(const int* rank, long long n, unsigned long long* rec, void* stream) {
  if (n < 0) {
    fbn_set_error("fbn_rank_hist: negative n");
    return FBN_ERR_ARG;
  }
  if (n == 0) return FBN_OK;
  const long long blocks = (n + 255) / 256;
  const dim3 grid((unsigned)(blocks > 1024 ? 1024 : blocks));
  fbn_launch(rank_hist_kernel, grid, dim3(256), 0, (hipStream_t)stream, rank, n, rec);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
