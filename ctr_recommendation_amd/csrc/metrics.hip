// Device evaluation metrics: exact ROC-AUC and log-loss of a validation split, without pulling the
// probabilities to the host (replaces the per-batch .cpu() + the float64 host argsort of
// src/train_fibinet.py:133-146 with src/utils.py:18-32; DESIGN.md "device metrics").
//
// Key.  A probability p is fp32 in [0, 1]: its bit pattern is monotone in its value and at most
// 0x3F800000 (< 2^30).  One uint32 per sample, key = (bits(p) << 1) | y.  The AUC is a counting
// problem over the keys alone -- no payload, no float arithmetic:
//   U2 = sum over positives of (2 * #negatives with a smaller score + #negatives with an equal score)
//   auc = U2 / (2 n_pos n_neg)        (finished on the host as an exact integer division)
//
// Counting (not a sort).  The 30 score bits split into an 18-bit high part (the bucket) and a
// 12-bit low part:
//   A  eval_hist_kernel     (neg, pos) counts per bucket, summed per workgroup in an LDS table first
//                           (validation scores pile into a few hundred buckets: one atomic per bucket
//                           and workgroup), and the log-loss partial of each workgroup from the same read
//   S  eval_scan_*          exclusive scan of the counts: each bucket's segment start, the negatives
//                           below it, the list of non-empty buckets; the output record's counts and
//                           the log-loss sum (partials in index order, one thread)
//   B  eval_scatter_kernel  unstable counting scatter of (low, y) into the bucket segments (equal keys
//                           are interchangeable, so stability is not needed); positions per workgroup
//                           from the same LDS table, one returning global atomic per bucket
//   C  eval_count_kernel    one workgroup per non-empty bucket at a time: LDS histogram of the low
//                           part (2 x 4096 u32: a bucket may hold all n samples, so 32-bit counters),
//                           one sweep accumulating pos * (2 * (neg_below + neg_less) + neg_equal) in
//                           u64, one u64 atomic per workgroup
// Every total is an integer sum, so it is independent of execution order: reproducible by
// construction.  The log-loss is float64 with compute_logloss's semantics (clip to [1e-15, 1 - 1e-15],
// one log per sample), summed as a fixed-shape tree whose shape depends on n only -- no float atomics.
//
// Bad inputs never trap: they set bits of the evaluator's status word (EV_BAD_*), the host raises.
//
// The per-group AUC (GAUC) over an arbitrary 32-bit group id is the second half of this file: it
// sorts (csrc/sort.hip) where the ungrouped reduce counts.  The calibration table (reliability bins,
// the sums behind ECE / PCOC / Brier) is the third part: one sort of the keys and one prefix sum.
// The DeLong placements and their sums (the variance of an AUC, the covariance of two) are the fourth.
#include "common.h"
#include "scan.h"                                // ev_block_excl_scan, scan_top_kernel, fbn_sort_u64
#include <algorithm>

#define EV_LO_BITS 12
#define EV_NLO (1 << EV_LO_BITS)                 // low-part values per bucket
#define EV_NB (1 << 18)                          // buckets (0x3F800000 >> 12 = 0x3F800 < 2^18)
#define EV_MAX_BITS 0x3F800000u                  // bits(1.0f)
#define EV_SCAN_BLOCKS (EV_NB / 1024)            // scan: 1024 buckets per workgroup of 256
#define EV_LL_MAX 1024                           // log-loss partials (workgroups of pass A) at most
#define EV_ELEMS_PER_BLOCK 4096                  // pass A / B: keys per workgroup before grid-striding
#define EV_TAB 1024                              // pass A / B: per-workgroup LDS table of bucket counts (direct-mapped)
#define EV_EMPTY 0xFFFFFFFFu
#define EV_COUNT_THREADS 512
#define EV_COUNT_BLOCKS 1024

#define EV_BAD_NAN 1u
#define EV_BAD_RANGE 2u
#define EV_BAD_LABEL 4u
#define EV_BAD_KEY 8u

struct EvalRecord {
  unsigned long long U2, n_pos, n_neg;
  double logloss_sum;
};

// workspace layout (bytes from ws; every section 256-B aligned)
#define EV_OFF_HIST 0                                        // [EV_NB][2] u32 {neg, pos}; zeroed per reduce
#define EV_OFF_CURSOR (EV_OFF_HIST + (size_t)EV_NB * 8)      // [EV_NB] u32 segment start -> end after pass B
#define EV_OFF_NEGB (EV_OFF_CURSOR + (size_t)EV_NB * 4)      // [EV_NB] u32 negatives in lower buckets
#define EV_OFF_LIST (EV_OFF_NEGB + (size_t)EV_NB * 4)        // [EV_NB] u32 non-empty buckets, ascending
#define EV_OFF_BSUM (EV_OFF_LIST + (size_t)EV_NB * 4)        // [EV_SCAN_BLOCKS][4] u32 {total, neg, non-empty}
#define EV_OFF_NLIST (EV_OFF_BSUM + (size_t)EV_SCAN_BLOCKS * 16)   // u32 number of non-empty buckets
#define EV_OFF_LL (EV_OFF_NLIST + 256)                       // [EV_LL_MAX] f64 log-loss partials
#define EV_OFF_SEG (EV_OFF_LL + (size_t)EV_LL_MAX * 8)       // [n] u16 (low << 1) | y, grouped by bucket

static inline int ev_stream_blocks(long long n) {
  return (int)std::min<long long>(EV_LL_MAX, std::max<long long>(1, (n + EV_ELEMS_PER_BLOCK - 1) / EV_ELEMS_PER_BLOCK));
}

// ---------------------------------------------------------------- pack
__global__ void __launch_bounds__(256) eval_pack_kernel(const float* __restrict__ probs, const float* __restrict__ labels,
                                                        long long n, uint32_t* __restrict__ keys, unsigned* status) {
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float p = probs[i];
    const float y = labels[i];
    if (p != p) { bad |= EV_BAD_NAN; p = 0.f; }
    else if (p < 0.f || p > 1.f) { bad |= EV_BAD_RANGE; p = p < 0.f ? 0.f : 1.f; }
    if (y != 0.f && y != 1.f) bad |= EV_BAD_LABEL;
    const uint32_t bits = p == 0.f ? 0u : __float_as_uint(p);     // -0.0 compares equal to 0.0
    keys[i] = (bits << 1) | (y == 1.f ? 1u : 0u);
  }
  if (bad) atomicOr(status, bad);
}

// ---------------------------------------------------------------- pass A: bucket counts + log-loss partials
// Validation scores pile into a few hundred neighbouring buckets, whose counters share a handful of
// cache lines: the counts of a workgroup's keys are summed in a direct-mapped LDS table first (slot =
// bucket mod EV_TAB, claimed by the first bucket that reaches it; a bucket that finds its slot taken by
// another goes to the global word directly) and flushed as one atomic per bucket and workgroup.
__global__ void __launch_bounds__(256) eval_hist_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* hist,
                                                        double* __restrict__ llpart, unsigned* status) {
  __shared__ double red[256];
  __shared__ uint32_t tkey[EV_TAB], tneg[EV_TAB], tpos[EV_TAB];
  const int tid = threadIdx.x;
  const uint32_t stride = gridDim.x * 256u;
  double acc = 0.0;
  unsigned bad = 0;
  for (int k = tid; k < EV_TAB; k += 256) { tkey[k] = EV_EMPTY; tneg[k] = 0u; tpos[k] = 0u; }
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256u + tid; i < n; i += stride) {
    const uint32_t key = keys[i];
    uint32_t bits = key >> 1;
    const uint32_t y = key & 1u;
    if (bits > EV_MAX_BITS) { bits = EV_MAX_BITS; bad = EV_BAD_KEY; }   // a key fbn_eval_pack did not write
    const uint32_t b = bits >> EV_LO_BITS;                               // < EV_NB
    double p = (double)__uint_as_float(bits);
    p = fmin(fmax(p, 1e-15), 1.0 - 1e-15);
    acc += log(y ? p : 1.0 - p);
    const uint32_t slot = b & (EV_TAB - 1);
    const uint32_t prev = atomicCAS(&tkey[slot], EV_EMPTY, b);
    if (prev == EV_EMPTY || prev == b) atomicAdd(y ? &tpos[slot] : &tneg[slot], 1u);
    else atomicAdd(&hist[2 * b + y], 1u);
  }
  __syncthreads();
  for (int k = tid; k < EV_TAB; k += 256) {
    const uint32_t b = tkey[k];
    if (b != EV_EMPTY) {
      if (tneg[k]) atomicAdd(&hist[2 * b], tneg[k]);
      if (tpos[k]) atomicAdd(&hist[2 * b + 1], tpos[k]);
    }
  }
  if (bad) atomicOr(status, bad);
  red[tid] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  if (tid == 0) llpart[blockIdx.x] = red[0];
}

// ---------------------------------------------------------------- scan
// thread t of workgroup g owns buckets g*1024 + 4t .. +3
__device__ __forceinline__ void ev_load4(const uint32_t* hist, uint32_t b0, uint32_t* neg, uint32_t* pos) {
  const uint4 lo = *reinterpret_cast<const uint4*>(hist + 2 * (size_t)b0);
  const uint4 hi = *reinterpret_cast<const uint4*>(hist + 2 * (size_t)b0 + 4);
  neg[0] = lo.x; pos[0] = lo.y; neg[1] = lo.z; pos[1] = lo.w;
  neg[2] = hi.x; pos[2] = hi.y; neg[3] = hi.z; pos[3] = hi.w;
}

__global__ void __launch_bounds__(256) eval_scan_sums_kernel(const uint32_t* __restrict__ hist, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  uint32_t neg[4], pos[4];
  ev_load4(hist, blockIdx.x * 1024u + threadIdx.x * 4u, neg, pos);
  uint32_t tot = 0, ng = 0, ne = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { tot += neg[j] + pos[j]; ng += neg[j]; ne += (neg[j] + pos[j]) != 0; }
  uint32_t t_tot, t_ng, t_ne;
  ev_block_excl_scan<4>(tot, sh, t_tot);
  ev_block_excl_scan<4>(ng, sh, t_ng);
  ev_block_excl_scan<4>(ne, sh, t_ne);
  if (threadIdx.x == 0) {
    bsum[blockIdx.x * 4 + 0] = t_tot;
    bsum[blockIdx.x * 4 + 1] = t_ng;
    bsum[blockIdx.x * 4 + 2] = t_ne;
  }
}

__global__ void __launch_bounds__(256) eval_scan_kernel(const uint32_t* __restrict__ hist, const uint32_t* __restrict__ bsum,
                                                        uint32_t* __restrict__ cursor, uint32_t* __restrict__ negb,
                                                        uint32_t* __restrict__ list, uint32_t* __restrict__ nlist,
                                                        const double* __restrict__ llpart, int n_ll, EvalRecord* out) {
  __shared__ uint32_t sh[4];
  const int tid = threadIdx.x;
  // the workgroups before this one (EV_SCAN_BLOCKS == 256 == the workgroup size)
  const bool before = tid < (int)blockIdx.x;
  uint32_t all_tot, all_ng, all_ne, b_tot, b_ng, b_ne, dummy;
  const uint32_t s_tot = bsum[tid * 4 + 0], s_ng = bsum[tid * 4 + 1], s_ne = bsum[tid * 4 + 2];
  ev_block_excl_scan<4>(s_tot, sh, all_tot);
  ev_block_excl_scan<4>(s_ng, sh, all_ng);
  ev_block_excl_scan<4>(s_ne, sh, all_ne);
  ev_block_excl_scan<4>(before ? s_tot : 0u, sh, b_tot);
  ev_block_excl_scan<4>(before ? s_ng : 0u, sh, b_ng);
  ev_block_excl_scan<4>(before ? s_ne : 0u, sh, b_ne);
  const uint32_t b0 = blockIdx.x * 1024u + tid * 4u;
  uint32_t neg[4], pos[4];
  ev_load4(hist, b0, neg, pos);
  uint32_t tot = 0, ng = 0, ne = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) { tot += neg[j] + pos[j]; ng += neg[j]; ne += (neg[j] + pos[j]) != 0; }
  uint32_t r_tot = b_tot + ev_block_excl_scan<4>(tot, sh, dummy);
  uint32_t r_ng = b_ng + ev_block_excl_scan<4>(ng, sh, dummy);
  uint32_t r_ne = b_ne + ev_block_excl_scan<4>(ne, sh, dummy);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    cursor[b0 + j] = r_tot;
    negb[b0 + j] = r_ng;
    const uint32_t c = neg[j] + pos[j];
    if (c) list[r_ne++] = b0 + j;                // r_ne < number of non-empty buckets <= EV_NB
    r_tot += c;
    r_ng += neg[j];
  }
  if (blockIdx.x == 0 && tid == 0) {
    *nlist = all_ne;
    out->U2 = 0ull;                              // pass C adds into it
    out->n_pos = (unsigned long long)(all_tot - all_ng);
    out->n_neg = (unsigned long long)all_ng;
    double s = 0.0;                              // the partials in index order
    for (int k = 0; k < n_ll; ++k) s += llpart[k];
    out->logloss_sum = -s;
  }
}

// ---------------------------------------------------------------- pass B: counting scatter
// A workgroup takes EV_ELEMS_PER_BLOCK consecutive keys at a time: (1) counts them per bucket in the LDS
// table (as pass A), (2) takes each bucket's base from its global cursor with one returning atomic,
// (3) reads the keys again and hands out the positions from LDS.  A key whose slot another bucket holds
// takes its position from the global cursor directly.
__global__ void __launch_bounds__(256) eval_scatter_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t* cursor,
                                                           uint16_t* __restrict__ seg) {
  __shared__ uint32_t tkey[EV_TAB], tcnt[EV_TAB], tbase[EV_TAB];
  const int tid = threadIdx.x;
  for (int k = tid; k < EV_TAB; k += 256) { tkey[k] = EV_EMPTY; tcnt[k] = 0u; }
  __syncthreads();
  const uint32_t chunks = (n + EV_ELEMS_PER_BLOCK - 1) / EV_ELEMS_PER_BLOCK;
  for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {            // workgroup-uniform
    const uint32_t lo = c * (uint32_t)EV_ELEMS_PER_BLOCK;
    const uint32_t hi = n - lo < (uint32_t)EV_ELEMS_PER_BLOCK ? n : lo + EV_ELEMS_PER_BLOCK;
    for (uint32_t i = lo + tid; i < hi; i += 256) {
      uint32_t bits = keys[i] >> 1;
      if (bits > EV_MAX_BITS) bits = EV_MAX_BITS;                        // as pass A counted it
      const uint32_t b = bits >> EV_LO_BITS, slot = b & (EV_TAB - 1);
      const uint32_t prev = atomicCAS(&tkey[slot], EV_EMPTY, b);
      if (prev == EV_EMPTY || prev == b) atomicAdd(&tcnt[slot], 1u);
    }
    __syncthreads();
    for (int k = tid; k < EV_TAB; k += 256) {
      const uint32_t cnt = tcnt[k];
      if (cnt) { tbase[k] = atomicAdd(&cursor[tkey[k]], cnt); tcnt[k] = 0u; }
    }
    __syncthreads();
    for (uint32_t i = lo + tid; i < hi; i += 256) {
      const uint32_t key = keys[i];
      uint32_t bits = key >> 1;
      if (bits > EV_MAX_BITS) bits = EV_MAX_BITS;
      const uint32_t b = bits >> EV_LO_BITS, slot = b & (EV_TAB - 1);
      const uint16_t v = (uint16_t)(((bits & (EV_NLO - 1)) << 1) | (key & 1u));
      uint32_t dst;
      if (tkey[slot] == b) dst = tbase[slot] + atomicAdd(&tcnt[slot], 1u);
      else dst = atomicAdd(&cursor[b], 1u);
      if (dst < n) seg[dst] = v;                 // always true: the cursors partition [0, n)
    }
    __syncthreads();
    for (int k = tid; k < EV_TAB; k += 256) tcnt[k] = 0u;                // the slots stay claimed
    __syncthreads();
  }
}

// ---------------------------------------------------------------- pass C: per-bucket counting
__global__ void __launch_bounds__(EV_COUNT_THREADS) eval_count_kernel(
    const uint32_t* __restrict__ hist, const uint32_t* __restrict__ cursor, const uint32_t* __restrict__ negb,
    const uint32_t* __restrict__ list, const uint32_t* __restrict__ nlist, const uint16_t* __restrict__ seg, uint32_t n,
    EvalRecord* out) {
  constexpr int NW = EV_COUNT_THREADS / 64, PER = EV_NLO / EV_COUNT_THREADS;
  __shared__ uint32_t hneg[EV_NLO], hpos[EV_NLO];
  __shared__ uint32_t sh[NW];
  __shared__ unsigned long long red[NW];
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned long long acc = 0ull;
  const uint32_t nl = *nlist;
  for (uint32_t li = blockIdx.x; li < nl; li += gridDim.x) {           // every branch below is workgroup-uniform
    const uint32_t b = list[li];
    const uint32_t cn = hist[2 * b], cp = hist[2 * b + 1];
    const unsigned long long below = negb[b];
    if (cp == 0) continue;                                             // negatives only: nothing to add
    if (cn == 0) {                                                     // positives only: every lower negative counts twice
      if (tid == 0) acc += (unsigned long long)cp * (2ull * below);
      continue;
    }
    const uint32_t cnt = cn + cp, start = cursor[b] - cnt;             // pass B left each cursor at its segment's end
    for (int k = tid; k < EV_NLO; k += EV_COUNT_THREADS) { hneg[k] = 0u; hpos[k] = 0u; }
    __syncthreads();
    for (uint32_t j0 = 0; j0 < cnt; j0 += EV_COUNT_THREADS) {
      const uint32_t j = j0 + tid;
      const bool valid = j < cnt && start + j < n;
      const uint32_t v = valid ? (seg[start + j] & (2u * EV_NLO - 1u)) : 0u;   // (low << 1) | y: in range whatever seg holds
      // a wave whose 64 values are equal (heavy ties) adds once
      const uint32_t v0 = __shfl(v, 0, 64);
      const bool same = __ballot(valid && v == v0) == ~0ull;
      if (same) {
        if (lane == 0) atomicAdd((v0 & 1u) ? &hpos[v0 >> 1] : &hneg[v0 >> 1], 64u);
      } else if (valid) {
        atomicAdd((v & 1u) ? &hpos[v >> 1] : &hneg[v >> 1], 1u);
      }
    }
    __syncthreads();
    uint32_t ng[PER], ps[PER], s = 0;
#pragma unroll
    for (int k = 0; k < PER; ++k) { ng[k] = hneg[tid * PER + k]; ps[k] = hpos[tid * PER + k]; s += ng[k]; }
    uint32_t dummy;
    unsigned long long less = below + ev_block_excl_scan<NW>(s, sh, dummy);
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      acc += (unsigned long long)ps[k] * (2ull * less + ng[k]);
      less += ng[k];
    }
    __syncthreads();                                                   // the histograms are zeroed again next
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (lane == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    unsigned long long t = 0ull;
#pragma unroll
    for (int k = 0; k < NW; ++k) t += red[k];
    if (t) atomicAdd(&out->U2, t);
  }
}

__global__ void eval_empty_kernel(EvalRecord* out) {
  out->U2 = 0ull; out->n_pos = 0ull; out->n_neg = 0ull; out->logloss_sum = 0.0;
}

// ---------------------------------------------------------------- entry points
extern "C" int fbn_eval_pack(const float* probs, const float* labels, long long n, uint32_t* keys_out, unsigned* status,
                             void* stream) {
  if (n <= 0) return FBN_OK;
  if (!probs || !labels || !keys_out || !status) { fbn_set_error("fbn_eval_pack: null argument"); return FBN_ERR_ARG; }
  if (n >= (1ll << 31)) { fbn_set_error("fbn_eval_pack: n must be below 2^31"); return FBN_ERR_ARG; }
  const int blocks = (int)std::min<long long>(2048, (n + 255) / 256);
  fbn_launch(eval_pack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, probs, labels, n, keys_out, status);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" size_t fbn_eval_workspace_size(long long n) {
  if (n < 0) n = 0;
  return EV_OFF_SEG + (((size_t)n * 2 + 255) & ~(size_t)255);
}

extern "C" int fbn_eval_reduce(const uint32_t* keys, long long n, void* ws, size_t ws_bytes, void* out, unsigned* status,
                               void* stream) {
  static_assert(EV_SCAN_BLOCKS == 256, "eval_scan_kernel reads one block sum per thread");
  static_assert(sizeof(EvalRecord) == 32, "record layout");
  hipStream_t st = (hipStream_t)stream;
  if (!out || ((uintptr_t)out & 7)) { fbn_set_error("fbn_eval_reduce: out must be an 8-B aligned device record"); return FBN_ERR_ARG; }
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_eval_reduce: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  EvalRecord* rec = (EvalRecord*)out;
  if (n == 0) {
    fbn_launch(eval_empty_kernel, dim3(1), dim3(1), 0, st, rec);
    FBN_CHECK_LAUNCH();
    return FBN_OK;
  }
  if (!keys || !ws || !status || ((uintptr_t)ws & 15)) {
    fbn_set_error("fbn_eval_reduce: keys, status and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  if (ws_bytes < fbn_eval_workspace_size(n)) { fbn_set_error("fbn_eval_reduce: ws smaller than fbn_eval_workspace_size(n)"); return FBN_ERR_ARG; }
  char* w = (char*)ws;
  uint32_t* hist = (uint32_t*)(w + EV_OFF_HIST);
  uint32_t* cursor = (uint32_t*)(w + EV_OFF_CURSOR);
  uint32_t* negb = (uint32_t*)(w + EV_OFF_NEGB);
  uint32_t* list = (uint32_t*)(w + EV_OFF_LIST);
  uint32_t* bsum = (uint32_t*)(w + EV_OFF_BSUM);
  uint32_t* nlist = (uint32_t*)(w + EV_OFF_NLIST);
  double* llpart = (double*)(w + EV_OFF_LL);
  uint16_t* seg = (uint16_t*)(w + EV_OFF_SEG);
  const uint32_t un = (uint32_t)n;
  const int sb = ev_stream_blocks(n);            // depends on n only: the log-loss tree's shape
  if (hipMemsetAsync(hist, 0, (size_t)EV_NB * 8, st) != hipSuccess) { fbn_set_error("fbn_eval_reduce: memset failed"); return FBN_ERR_LAUNCH; }
  fbn_launch(eval_hist_kernel, dim3(sb), dim3(256), 0, st, keys, un, hist, llpart, status);
  fbn_launch(eval_scan_sums_kernel, dim3(EV_SCAN_BLOCKS), dim3(256), 0, st, (const uint32_t*)hist, bsum);
  fbn_launch(eval_scan_kernel, dim3(EV_SCAN_BLOCKS), dim3(256), 0, st, (const uint32_t*)hist, (const uint32_t*)bsum, cursor,
             negb, list, nlist, (const double*)llpart, sb, rec);
  fbn_launch(eval_scatter_kernel, dim3(sb), dim3(256), 0, st, keys, un, cursor, seg);
  fbn_launch(eval_count_kernel, dim3(EV_COUNT_BLOCKS), dim3(EV_COUNT_THREADS), 0, st, (const uint32_t*)hist,
             (const uint32_t*)cursor, (const uint32_t*)negb, (const uint32_t*)list, (const uint32_t*)nlist,
             (const uint16_t*)seg, un, rec);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ================================================================ grouped AUC (GAUC)
// The AUC of every group (user) of the samples held, and its three usual averages over the mixed groups
// (both classes present).  The grouping key is an arbitrary 32-bit id, so the counting of the ungrouped
// reduce (a table indexed by the key's high bits) has nothing to index: the samples are SORTED by the
// composite (gid << 31) | key (63 bits; keys are below 2^31) with fbn_sort_u64.  In the sorted array S
// a group is a segment, a tie a sub-segment, and within a tie the negatives (key bit 0 clear) come first:
//   c  gauc_compose_kernel   the composite keys
//      fbn_sort_u64(bits = 63)
//   s  gauc_scan_*           one two-level scan of (negative, group head) flags packed in a u64:
//                            N[0 .. n] = negatives before each position, ord[i] = the group's ordinal,
//                            start[0 .. G] = the groups' first positions, table[g] = {id, U2 = 0}, G
//   u  gauc_u2_kernel        per group head the class counts from N; per positive the ends of its tie by
//                            binary search inside its group, 2 * (N[lower] - N[group start]) +
//                            (N[upper] - N[lower]) added to table[g].U2 -- one u64 atomic per wave when
//                            the wave's lanes share a group (after the sort they usually do)
//   f  gauc_part / _final    AUC_g = U2_g / (2 n_pos_g n_neg_g), ONE IEEE double division of exactly
//                            represented integers (while 2 n_pos_g n_neg_g < 2^53; no fast-math), and the
//                            three float64 sums over the groups in ascending id order as a fixed-shape
//                            tree whose shape depends on G only (per-thread index order, an LDS binary
//                            tree, one thread adding the partials) -- no float atomics.  The group list is
//                            sorted, so the sums do not depend on the samples' order, on how update()
//                            split them or on which rank held them.
// Grids are sized by n and iterate to the device-resident G: no host read anywhere.
#define EV_BAD_GROUP 0x10000u                    // status bit 16: a group id outside [0, 2^32)
#define GA_PART_MAX 256                          // workgroups of the fixed tree at most (gauc_final_kernel: one per thread)

struct GaucLayout {
  size_t comp, sorted, negs, ord, start, bsum, ngroups, partd, partc, sortws, total;
};
static inline GaucLayout gauc_layout(long long n) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t un = (size_t)n, nb = (un + 255) / 256;
  GaucLayout L;
  L.comp = 0;
  L.sorted = L.comp + al(un * 8);
  L.negs = L.sorted + al(un * 8);
  L.ord = L.negs + al((un + 1) * 4);
  L.start = L.ord + al(un * 4);
  L.bsum = L.start + al((un + 1) * 4);
  L.ngroups = L.bsum + al(nb * 8);
  L.partd = L.ngroups + 256;
  L.partc = L.partd + al((size_t)GA_PART_MAX * 3 * 8);
  L.sortws = L.partc + al((size_t)GA_PART_MAX * 3 * 8);
  L.total = L.sortws + al(fbn_sort_u64_workspace_size(n));
  return L;
}

// workgroups of the fixed tree over g groups: a function of g alone (the host sizes the grid with g = n >= G)
__host__ __device__ static inline uint32_t gauc_blocks(uint32_t g) {
  const uint32_t b = (g + 255u) / 256u;
  return b < 1u ? 1u : (b > (uint32_t)GA_PART_MAX ? (uint32_t)GA_PART_MAX : b);
}

__global__ void __launch_bounds__(256) eval_pack_groups_kernel(const long long* __restrict__ ids, long long n,
                                                               uint32_t* __restrict__ gids, unsigned* status) {
  unsigned bad = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    long long g = ids[i];
    if (g < 0) { bad = EV_BAD_GROUP; g = 0; }
    else if (g > 0xFFFFFFFFll) { bad = EV_BAD_GROUP; g = 0xFFFFFFFFll; }
    gids[i] = (uint32_t)g;
  }
  if (bad) atomicOr(status, bad);
}

__global__ void __launch_bounds__(256) gauc_compose_kernel(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ gids,
                                                           uint32_t n, uint64_t* __restrict__ comp, unsigned* status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t key = keys[i];
  if ((key >> 1) > EV_MAX_BITS) {                // a key fbn_eval_pack did not write: counted as 1.0, as the ungrouped reduce does
    key = (EV_MAX_BITS << 1) | (key & 1u);
    atomicOr(status, EV_BAD_KEY);
  }
  comp[i] = ((uint64_t)gids[i] << 31) | (uint64_t)key;
}

// (group head << 32) | negative of sorted position i
__device__ __forceinline__ uint64_t gauc_flags(const uint64_t* __restrict__ S, uint32_t i) {
  const uint64_t s = S[i];
  const uint64_t head = (i == 0u || (S[i - 1] >> 31) != (s >> 31)) ? 1ull : 0ull;
  return (head << 32) | ((s & 1ull) ^ 1ull);
}

__global__ void __launch_bounds__(256) gauc_scan_sums_kernel(const uint64_t* __restrict__ S, uint32_t n,
                                                             unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  unsigned long long total;
  ev_block_excl_scan<4>((unsigned long long)(i < n ? gauc_flags(S, i) : 0ull), sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) gauc_scan_apply_kernel(const uint64_t* __restrict__ S, uint32_t n,
                                                              const unsigned long long* __restrict__ bsum,
                                                              uint32_t* __restrict__ negs, uint32_t* __restrict__ ord,
                                                              uint32_t* __restrict__ start, unsigned long long* __restrict__ table,
                                                              uint32_t* __restrict__ ngroups) {
  __shared__ unsigned long long sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const unsigned long long v = i < n ? gauc_flags(S, i) : 0ull;
  unsigned long long total;
  const unsigned long long ex = bsum[blockIdx.x] + ev_block_excl_scan<4>(v, sh, total);
  if (i >= n) return;
  const uint32_t neg_before = (uint32_t)ex, head = (uint32_t)(v >> 32);
  const uint32_t o = (uint32_t)(ex >> 32) + head - 1u;       // position 0 is a head: never below 0
  negs[i] = neg_before;
  ord[i] = o;
  if (head) {
    start[o] = i;
    table[4 * (size_t)o + 0] = (unsigned long long)(S[i] >> 31);
    table[4 * (size_t)o + 1] = 0ull;             // gauc_u2_kernel adds into it
  }
  if (i == n - 1u) {
    negs[n] = neg_before + (uint32_t)(v & 1ull);
    start[o + 1u] = n;                           // o + 1 = G <= n
    *ngroups = o + 1u;
  }
}

__global__ void __launch_bounds__(256) gauc_u2_kernel(const uint64_t* __restrict__ S, uint32_t n, const uint32_t* __restrict__ negs,
                                                      const uint32_t* __restrict__ ord, const uint32_t* __restrict__ start,
                                                      unsigned long long* table) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const bool valid = i < n;
  uint32_t o = 0u;
  unsigned long long c = 0ull;
  if (valid) {
    const uint64_t s = S[i];
    o = ord[i];
    const uint32_t gs = start[o], ge = start[o + 1u];          // gs <= i < ge <= n
    if (gs == i) {
      const uint32_t nn = negs[ge] - negs[gs];
      table[4 * (size_t)o + 2] = (unsigned long long)(ge - gs - nn);
      table[4 * (size_t)o + 3] = (unsigned long long)nn;
    }
    if (s & 1ull) {
      const uint64_t run = s >> 1;               // group and score: the tie this positive belongs to
      uint32_t lo = gs, hi = i;                  // first position of the tie: S[i] itself qualifies
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((S[mid] >> 1) < run) lo = mid + 1u; else hi = mid;
      }
      const uint32_t lower = lo;
      lo = i + 1u; hi = ge;                      // first position past the tie
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if ((S[mid] >> 1) <= run) lo = mid + 1u; else hi = mid;
      }
      const uint32_t nl = negs[lower];
      c = 2ull * (unsigned long long)(nl - negs[gs]) + (unsigned long long)(negs[lo] - nl);
    }
  }
  // lane 0 is valid whenever any lane is (positions ascend with the lane)
  const uint32_t o0 = __shfl(o, 0, 64);
  if (__ballot(valid && o != o0) == 0ull) {      // one group in the wave: one atomic
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&table[4 * (size_t)o0 + 1], c);
  } else if (c) {
    atomicAdd(&table[4 * (size_t)o + 1], c);
  }
}

// the fixed tree's leaves: workgroup b of gauc_blocks(G), thread t takes groups b * 256 + t, + gauc_blocks(G) * 256, ...
__global__ void __launch_bounds__(256) gauc_part_kernel(const unsigned long long* __restrict__ table,
                                                        const uint32_t* __restrict__ ngroups, double* __restrict__ partd,
                                                        unsigned long long* __restrict__ partc) {
  __shared__ double rd[3][256];
  __shared__ unsigned long long rc[3][256];
  const uint32_t G = *ngroups, vb = gauc_blocks(G), tid = threadIdx.x;
  if (blockIdx.x >= vb) return;                  // workgroup-uniform
  double s_n = 0.0, s_1 = 0.0, s_p = 0.0;
  unsigned long long c_g = 0ull, c_n = 0ull, c_p = 0ull;
  for (uint32_t g = blockIdx.x * 256u + tid; g < G; g += vb * 256u) {
    const unsigned long long u2 = table[4 * (size_t)g + 1], np = table[4 * (size_t)g + 2], nn = table[4 * (size_t)g + 3];
    if (np && nn) {
      const double auc = (double)u2 / (double)(2ull * np * nn);
      s_n += __dmul_rn((double)(np + nn), auc);  // the rounded product, then the sum: no contraction
      s_1 += auc;
      s_p += __dmul_rn((double)np, auc);
      c_g += 1ull; c_n += np + nn; c_p += np;
    }
  }
  rd[0][tid] = s_n; rd[1][tid] = s_1; rd[2][tid] = s_p;
  rc[0][tid] = c_g; rc[1][tid] = c_n; rc[2][tid] = c_p;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)tid < s) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { rd[k][tid] += rd[k][tid + s]; rc[k][tid] += rc[k][tid + s]; }
    }
    __syncthreads();
  }
  if (tid < 3) { partd[blockIdx.x * 3 + tid] = rd[tid][0]; partc[blockIdx.x * 3 + tid] = rc[tid][0]; }
}

// the partials staged through LDS by one thread each, then added by one thread in index order
__global__ void __launch_bounds__(GA_PART_MAX) gauc_final_kernel(const uint32_t* __restrict__ ngroups, const double* __restrict__ partd,
                                                                 const unsigned long long* __restrict__ partc, unsigned long long* out) {
  __shared__ double sd[3][GA_PART_MAX];
  __shared__ unsigned long long sc[3][GA_PART_MAX];
  const uint32_t G = *ngroups, vb = gauc_blocks(G), tid = threadIdx.x;
  if (tid < vb) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { sd[k][tid] = partd[tid * 3 + k]; sc[k][tid] = partc[tid * 3 + k]; }
  }
  __syncthreads();
  if (tid != 0) return;
  double d[3] = {0.0, 0.0, 0.0};
  unsigned long long c[3] = {0ull, 0ull, 0ull};
  for (uint32_t b = 0; b < vb; ++b)
    for (int k = 0; k < 3; ++k) { d[k] += sd[k][b]; c[k] += sc[k][b]; }
  out[0] = (unsigned long long)G;
  out[1] = c[0]; out[2] = c[1]; out[3] = c[2];
  out[4] = (unsigned long long)__double_as_longlong(d[0]);
  out[5] = (unsigned long long)__double_as_longlong(d[1]);
  out[6] = (unsigned long long)__double_as_longlong(d[2]);
  out[7] = 0ull;
}

__global__ void gauc_empty_kernel(unsigned long long* out) {
  for (int k = 0; k < 8; ++k) out[k] = 0ull;     // 0.0 is all zero bits
}

extern "C" int fbn_eval_pack_groups(const long long* ids, long long n, uint32_t* gids_out, unsigned* status, void* stream) {
  if (n <= 0) return FBN_OK;
  if (!ids || !gids_out || !status) { fbn_set_error("fbn_eval_pack_groups: null argument"); return FBN_ERR_ARG; }
  if (n >= (1ll << 31)) { fbn_set_error("fbn_eval_pack_groups: n must be below 2^31"); return FBN_ERR_ARG; }
  const int blocks = (int)std::min<long long>(2048, (n + 255) / 256);
  fbn_launch(eval_pack_groups_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ids, n, gids_out, status);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" size_t fbn_gauc_workspace_size(long long n) {
  if (n < 0) n = 0;
  return gauc_layout(n).total;
}

extern "C" int fbn_gauc_reduce(const uint32_t* keys, const uint32_t* gids, long long n, void* ws, size_t ws_bytes,
                               unsigned long long* table, void* out, unsigned* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!out || ((uintptr_t)out & 7)) { fbn_set_error("fbn_gauc_reduce: out must be an 8-B aligned device record"); return FBN_ERR_ARG; }
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_gauc_reduce: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  unsigned long long* rec = (unsigned long long*)out;
  if (n == 0) {
    fbn_launch(gauc_empty_kernel, dim3(1), dim3(1), 0, st, rec);
    FBN_CHECK_LAUNCH();
    return FBN_OK;
  }
  if (!keys || !gids || !ws || !table || !status || ((uintptr_t)ws & 15) || ((uintptr_t)table & 7)) {
    fbn_set_error("fbn_gauc_reduce: keys, gids, status, an 8-B aligned table and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  const GaucLayout L = gauc_layout(n);
  if (ws_bytes < L.total) { fbn_set_error("fbn_gauc_reduce: ws smaller than fbn_gauc_workspace_size(n)"); return FBN_ERR_ARG; }
  char* w = (char*)ws;
  uint64_t* comp = (uint64_t*)(w + L.comp);
  uint64_t* sorted = (uint64_t*)(w + L.sorted);
  uint32_t* negs = (uint32_t*)(w + L.negs);
  uint32_t* ord = (uint32_t*)(w + L.ord);
  uint32_t* start = (uint32_t*)(w + L.start);
  unsigned long long* bsum = (unsigned long long*)(w + L.bsum);
  uint32_t* ngroups = (uint32_t*)(w + L.ngroups);
  double* partd = (double*)(w + L.partd);
  unsigned long long* partc = (unsigned long long*)(w + L.partc);
  const uint32_t un = (uint32_t)n, nb = (un + 255u) / 256u;
  fbn_launch(gauc_compose_kernel, dim3(nb), dim3(256), 0, st, keys, gids, un, comp, status);
  const int rc = fbn_sort_u64(comp, n, 63, w + L.sortws, L.total - L.sortws, sorted, stream);
  if (rc != FBN_OK) return rc;
  fbn_launch(gauc_scan_sums_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, bsum);
  fbn_launch(scan_top_kernel<unsigned long long>, dim3(1), dim3(256), 0, st, bsum, nb);
  fbn_launch(gauc_scan_apply_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, (const unsigned long long*)bsum,
             negs, ord, start, table, ngroups);
  fbn_launch(gauc_u2_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, (const uint32_t*)negs,
             (const uint32_t*)ord, (const uint32_t*)start, table);
  fbn_launch(gauc_part_kernel, dim3(gauc_blocks(un)), dim3(256), 0, st, (const unsigned long long*)table,
             (const uint32_t*)ngroups, partd, partc);
  fbn_launch(gauc_final_kernel, dim3(1), dim3(GA_PART_MAX), 0, st, (const uint32_t*)ngroups, (const double*)partd,
             (const unsigned long long*)partc, rec);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ================================================================ calibration
// The reliability table of the samples held, in two binnings of B bins each: equal width (bin =
// min(B - 1, floor((double)p * B))) and equal mass (bin b = the sorted ranks [floor(b n / B),
// floor((b + 1) n / B))).  Both binnings are monotone in the key, so after ONE sort of the keys a bin of
// either is a rank range [lo, hi) and every bin sum is a difference of one prefix sum at two ranks:
//   w  calib_widen_kernel    the keys as u64 (a key above bits(1.0) clamped and flagged, as above)
//      fbn_sort_u64(bits = 31)
//   s  calib_sums_kernel     per 256 sorted samples the sums of {y, fx, y fx, fx2}, fx = rint(p 2^32) and
//                            fx2 = rint(p p 2^32) through exact float64 products; scan_top_kernel turns
//                            each of the four columns into its exclusive prefix over the blocks
//   b  calib_bound_kernel    one workgroup per boundary (2 (B + 1) of them): its rank -- floor(b n / B),
//                            or the first rank whose width bin is >= b by binary search -- and the prefix
//                            there = the block's prefix + the samples of the block before the rank
//   t  calib_table_kernel    one thread per bin and plane: the differences, the first and last score of
//                            the range, and the trailing status word
// Every sum is a u64 integer sum (fx, fx2 <= 2^32 and n < 2^31: below 2^63), so nothing depends on any
// order; the sort makes the tie split (negatives first) canonical.  No atomics except the status bit.
#define CA_REC 4                                 // prefix columns: y, fx, y * fx, fx2
#define CA_BND 5                                 // words per boundary: rank + the four prefixes

struct CalibLayout {
  size_t wide, sorted, bsum, bnd, sortws, total;
  uint32_t nb1;                                  // blocks of 256 samples + 1 (the prefix at rank n has a block too)
};
static inline CalibLayout calib_layout(long long n) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t un = (size_t)n;
  CalibLayout L;
  L.nb1 = (uint32_t)((un + 255) / 256 + 1);
  L.wide = 0;
  L.sorted = L.wide + al(un * 8);
  L.bsum = L.sorted + al(un * 8);
  L.bnd = L.bsum + al((size_t)CA_REC * L.nb1 * 8);
  L.sortws = L.bnd + al((size_t)2 * (FBN_CALIB_MAX_BINS + 1) * CA_BND * 8);
  L.total = L.sortws + al(fbn_sort_u64_workspace_size(n));
  return L;
}

__global__ void __launch_bounds__(256) calib_widen_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                          uint64_t* __restrict__ wide, unsigned* status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t key = keys[i];
  if ((key >> 1) > EV_MAX_BITS) {                // a key fbn_eval_pack did not write: counted as 1.0
    key = (EV_MAX_BITS << 1) | (key & 1u);
    atomicOr(status, EV_BAD_KEY);
  }
  wide[i] = (uint64_t)key;
}

// {y, fx, y * fx, fx2} of a sorted key: p * 2^32 and p * p * 2^32 are exact in float64 (24- and 48-bit
// significands), rint rounds half to even
__device__ __forceinline__ void calib_record(uint64_t s, unsigned long long* r) {
  const double p = (double)__uint_as_float((uint32_t)(s >> 1));
  const unsigned long long y = s & 1ull;
  const unsigned long long fx = (unsigned long long)rint(p * 4294967296.0);
  r[0] = y;
  r[1] = fx;
  r[2] = y ? fx : 0ull;
  r[3] = (unsigned long long)rint(p * p * 4294967296.0);
}

// the sums of the samples [lo, hi) (hi - lo <= 256) in every thread
__device__ __forceinline__ void calib_block_sums(const uint64_t* __restrict__ S, uint32_t lo, uint32_t hi,
                                                 unsigned long long* sh, unsigned long long* tot) {
  const uint32_t i = lo + threadIdx.x;
  unsigned long long r[CA_REC] = {0ull, 0ull, 0ull, 0ull};
  if (i < hi) calib_record(S[i], r);
#pragma unroll
  for (int k = 0; k < CA_REC; ++k) ev_block_excl_scan<4>(r[k], sh, tot[k]);
}

// grid: nb1 workgroups; the last one (and the tail of the one before) holds no sample
__global__ void __launch_bounds__(256) calib_sums_kernel(const uint64_t* __restrict__ S, uint32_t n, uint32_t nb1,
                                                         unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[4];
  const uint32_t lo = blockIdx.x * 256u;         // the last workgroup's lo is >= n: an empty range
  unsigned long long tot[CA_REC];
  calib_block_sums(S, lo, lo + 256u < n ? lo + 256u : n, sh, tot);   // n < 2^31: lo + 256 does not wrap
#pragma unroll
  for (int k = 0; k < CA_REC; ++k)
    if (threadIdx.x == (unsigned)k) bsum[(size_t)k * nb1 + blockIdx.x] = tot[k];
}

// the width bin of a sorted key is >= b  (1 <= b <= B - 1, so the min(B - 1, .) of the rule does not enter)
__device__ __forceinline__ bool calib_width_ge(uint64_t s, int b, int B) {
  return (int)floor((double)__uint_as_float((uint32_t)(s >> 1)) * (double)B) >= b;
}

// workgroup (plane, b), b = 0 .. B: plane 0 equal width, plane 1 equal mass
__global__ void __launch_bounds__(256) calib_bound_kernel(const uint64_t* __restrict__ S, uint32_t n, int B, uint32_t nb1,
                                                          const unsigned long long* __restrict__ bsum,
                                                          unsigned long long* __restrict__ bnd) {
  __shared__ unsigned long long sh[4];
  __shared__ uint32_t rank;
  const int plane = blockIdx.x / (B + 1), b = blockIdx.x % (B + 1);
  if (threadIdx.x == 0) {
    uint32_t r;
    if (plane == 1) r = (uint32_t)(((unsigned long long)b * n) / (unsigned long long)B);
    else if (b == 0) r = 0u;
    else if (b == B) r = n;
    else {
      uint32_t lo = 0u, hi = n;                  // the first rank whose width bin is >= b (n: none)
      while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (calib_width_ge(S[mid], b, B)) hi = mid; else lo = mid + 1u;
      }
      r = lo;
    }
    rank = r;
  }
  __syncthreads();
  const uint32_t r = rank, blk = r >> 8;         // r <= n: blk <= nb1 - 1, and the samples [blk * 256, r) exist
  unsigned long long tot[CA_REC];
  calib_block_sums(S, blk * 256u, r, sh, tot);
  unsigned long long* o = bnd + (size_t)blockIdx.x * CA_BND;
  if (threadIdx.x == 0) o[0] = (unsigned long long)r;
#pragma unroll
  for (int k = 0; k < CA_REC; ++k)
    if (threadIdx.x == (unsigned)k) o[1 + k] = bsum[(size_t)k * nb1 + blk] + tot[k];
}

__global__ void __launch_bounds__(256) calib_table_kernel(const uint64_t* __restrict__ S, int B,
                                                          const unsigned long long* __restrict__ bnd,
                                                          const unsigned* __restrict__ status, uint64_t* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t == 0) out[(size_t)2 * B * FBN_CALIB_BIN_WORDS] = (uint64_t)*status;
  if (t >= 2 * B) return;
  const int plane = t / B, b = t % B;
  const unsigned long long* lo = bnd + ((size_t)plane * (B + 1) + b) * CA_BND;
  const unsigned long long* hi = lo + CA_BND;
  uint64_t* o = out + (size_t)t * FBN_CALIB_BIN_WORDS;
  const uint32_t r0 = (uint32_t)lo[0], r1 = (uint32_t)hi[0];     // r0 <= r1: both boundary rules are monotone in b
  o[0] = (uint64_t)(r1 - r0);
#pragma unroll
  for (int k = 0; k < CA_REC; ++k) o[1 + k] = hi[1 + k] - lo[1 + k];
  o[5] = r1 > r0 ? ((S[r0] >> 1) & 0xFFFFFFFFull) | (((S[r1 - 1u] >> 1) & 0xFFFFFFFFull) << 32) : 0ull;
  o[6] = 0ull;
  o[7] = 0ull;
}

__global__ void __launch_bounds__(256) calib_empty_kernel(int words, const unsigned* __restrict__ status,
                                                          uint64_t* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t < words) out[t] = 0ull;
  else if (t == words) out[t] = (uint64_t)*status;
}

extern "C" size_t fbn_calib_workspace_size(long long n) {
  if (n < 0) n = 0;
  return calib_layout(n).total;
}

extern "C" int fbn_calib_reduce(const uint32_t* keys, long long n, int bins, void* ws, size_t ws_bytes, uint64_t* out,
                                unsigned* status, void* stream) {
  static_assert(CA_REC + 1 == CA_BND && CA_REC + 2 <= FBN_CALIB_BIN_WORDS, "bin layout");
  hipStream_t st = (hipStream_t)stream;
  if (!out || !status || ((uintptr_t)out & 7)) {
    fbn_set_error("fbn_calib_reduce: status and an 8-B aligned out are required");
    return FBN_ERR_ARG;
  }
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_calib_reduce: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  if (bins < 1 || bins > FBN_CALIB_MAX_BINS) { fbn_set_error("fbn_calib_reduce: bins must be in [1, 1024]"); return FBN_ERR_ARG; }
  const int words = 2 * bins * FBN_CALIB_BIN_WORDS;
  if (n == 0) {
    fbn_launch(calib_empty_kernel, dim3((words + 1 + 255) / 256), dim3(256), 0, st, words, (const unsigned*)status, out);
    FBN_CHECK_LAUNCH();
    return FBN_OK;
  }
  if (!keys || !ws || ((uintptr_t)ws & 15)) {
    fbn_set_error("fbn_calib_reduce: keys and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  const CalibLayout L = calib_layout(n);
  if (ws_bytes < L.total) { fbn_set_error("fbn_calib_reduce: ws smaller than fbn_calib_workspace_size(n)"); return FBN_ERR_ARG; }
  char* w = (char*)ws;
  uint64_t* wide = (uint64_t*)(w + L.wide);
  uint64_t* sorted = (uint64_t*)(w + L.sorted);
  unsigned long long* bsum = (unsigned long long*)(w + L.bsum);
  unsigned long long* bnd = (unsigned long long*)(w + L.bnd);
  const uint32_t un = (uint32_t)n, nb1 = L.nb1;
  fbn_launch(calib_widen_kernel, dim3(nb1 - 1u), dim3(256), 0, st, keys, un, wide, status);
  const int rc = fbn_sort_u64(wide, n, 31, w + L.sortws, L.total - L.sortws, sorted, stream);
  if (rc != FBN_OK) return rc;
  fbn_launch(calib_sums_kernel, dim3(nb1), dim3(256), 0, st, (const uint64_t*)sorted, un, nb1, bsum);
  for (int k = 0; k < CA_REC; ++k)
    fbn_launch(scan_top_kernel<unsigned long long>, dim3(1), dim3(256), 0, st, bsum + (size_t)k * nb1, nb1);
  fbn_launch(calib_bound_kernel, dim3(2 * (bins + 1)), dim3(256), 0, st, (const uint64_t*)sorted, un, bins, nb1,
             (const unsigned long long*)bsum, bnd);
  fbn_launch(calib_table_kernel, dim3((2 * bins + 255) / 256), dim3(256), 0, st, (const uint64_t*)sorted, bins,
             (const unsigned long long*)bnd, (const unsigned*)status, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

// ================================================================ DeLong placements and sums
// The variance of the AUC and the covariance of two AUCs over the same samples (DeLong et al. 1988), as
// exact integers.  The placement of a sample is what it adds to U2: for a positive 2 * #negatives with a
// smaller score + #negatives with an equal score, for a negative 2 * #positives with a larger score +
// #positives with an equal score.  fbn_auc_place sorts (key, index) pairs -- the index rides in the high
// word of the u64, above the 32 bits the sort compares -- so that every search runs along the sorted array
// (neighbouring lanes look for neighbouring scores) and the only uncoalesced access is one 4-byte store
// per sample:
//   c  place_compose_kernel   (index << 32) | key (a key above bits(1.0) clamped and flagged, as above)
//      fbn_sort_u64(bits = 32)
//   s  place_scan_*           one two-level scan of the negative flags: N[0 .. n]
//   p  place_kernel           per sorted position the ends [lower, upper) of its tie by binary search; the
//                             tie's negatives come first, so mid = lower + N[upper] - N[lower]; a positive
//                             gets 2 N[lower] + (mid - lower), a negative 2 ((n - upper) - (N[n] - N[upper]))
//                             + (upper - mid), stored at place_out[index]
// fbn_delong_reduce sums two placement arrays and their products per class: a product is below 2^64 and a
// sum of n < 2^31 of them below 2^95, so the low and the high 32 bits of each product go to two separate
// u64 sums (each below 2^63, no carries).  Integer atomics, one per workgroup and word: order-independent.
#define EV_BAD_PAIR 0x20000u                     // status bit 17: the two key sets' labels differ
#define DL_BLOCKS_MAX 1024

struct PlaceLayout {
  size_t comp, sorted, negs, bsum, sortws, total;
};
static inline PlaceLayout place_layout(long long n) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t un = (size_t)n, nb = (un + 255) / 256;
  PlaceLayout L;
  L.comp = 0;
  L.sorted = L.comp + al(un * 8);
  L.negs = L.sorted + al(un * 8);
  L.bsum = L.negs + al((un + 1) * 4);
  L.sortws = L.bsum + al(nb * 4);
  L.total = L.sortws + al(fbn_sort_u64_workspace_size(n));
  return L;
}

__global__ void __launch_bounds__(256) place_compose_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                            uint64_t* __restrict__ comp, unsigned* status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t key = keys[i];
  if ((key >> 1) > EV_MAX_BITS) {                // a key fbn_eval_pack did not write: counted as 1.0
    key = (EV_MAX_BITS << 1) | (key & 1u);
    atomicOr(status, EV_BAD_KEY);
  }
  comp[i] = ((uint64_t)i << 32) | (uint64_t)key;
}

__global__ void __launch_bounds__(256) place_scan_sums_kernel(const uint64_t* __restrict__ S, uint32_t n,
                                                              uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t total;
  ev_block_excl_scan<4>(i < n ? ((uint32_t)S[i] & 1u) ^ 1u : 0u, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) place_scan_apply_kernel(const uint64_t* __restrict__ S, uint32_t n,
                                                               const uint32_t* __restrict__ bsum, uint32_t* __restrict__ negs) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  const uint32_t v = i < n ? ((uint32_t)S[i] & 1u) ^ 1u : 0u;
  uint32_t total;
  const uint32_t ex = bsum[blockIdx.x] + ev_block_excl_scan<4>(v, sh, total);
  if (i >= n) return;
  negs[i] = ex;
  if (i == n - 1u) negs[n] = ex + v;
}

__global__ void __launch_bounds__(256) place_kernel(const uint64_t* __restrict__ S, uint32_t n, const uint32_t* __restrict__ negs,
                                                    uint32_t* __restrict__ place_out) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = S[i];
  const uint32_t key = (uint32_t)s, idx = (uint32_t)(s >> 32), score = key >> 1;
  uint32_t lo = 0u, hi = i;                      // first position of the tie: S[i] itself qualifies
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (((uint32_t)S[mid] >> 1) < score) lo = mid + 1u; else hi = mid;
  }
  const uint32_t lower = lo;
  lo = i + 1u; hi = n;                           // first position past the tie
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (((uint32_t)S[mid] >> 1) <= score) lo = mid + 1u; else hi = mid;
  }
  const uint32_t upper = lo;
  const uint32_t nl = negs[lower], nu = negs[upper], tie_neg = nu - nl;          // the tie's negatives come first
  uint32_t v;
  if (key & 1u) v = 2u * nl + tie_neg;                                           // <= 2 n_neg < 2^32
  else v = 2u * ((n - upper) - (negs[n] - nu)) + ((upper - lower) - tie_neg);    // <= 2 n_pos
  if (idx < n) place_out[idx] = v;               // always true: the indices are a permutation of [0, n)
}

// out[0 .. 8) += this workgroup's sums; the launch's record was zeroed before it
__global__ void __launch_bounds__(256) delong_reduce_kernel(const uint32_t* __restrict__ keys_a, const uint32_t* __restrict__ place_a,
                                                            const uint32_t* __restrict__ keys_b, const uint32_t* __restrict__ place_b,
                                                            uint32_t n, unsigned long long* out, unsigned* status) {
  __shared__ unsigned long long red[4][FBN_DELONG_REC_WORDS];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  unsigned long long acc[FBN_DELONG_REC_WORDS];
#pragma unroll
  for (int k = 0; k < FBN_DELONG_REC_WORDS; ++k) acc[k] = 0ull;
  unsigned bad = 0u;
  const uint32_t stride = gridDim.x * 256u;      // at most 2^18: i + stride wraps only past n < 2^31
  for (uint32_t i = blockIdx.x * 256u + tid; i < n; i += stride) {
    const uint32_t ya = keys_a[i] & 1u;
    if ((keys_b[i] & 1u) != ya) bad = EV_BAD_PAIR;
    const unsigned long long pa = place_a[i], pb = place_b[i], prod = pa * pb;
    if (ya) {
      acc[0] += 1ull; acc[2] += pa; acc[3] += pb;
      acc[4] += prod & 0xFFFFFFFFull; acc[5] += prod >> 32;
    } else {
      acc[1] += 1ull;
      acc[6] += prod & 0xFFFFFFFFull; acc[7] += prod >> 32;
    }
  }
  if (bad) atomicOr(status, bad);
#pragma unroll
  for (int k = 0; k < FBN_DELONG_REC_WORDS; ++k) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc[k] += __shfl_xor(acc[k], o, 64);
    if (lane == 0) red[w][k] = acc[k];
  }
  __syncthreads();
  if (tid < FBN_DELONG_REC_WORDS) {
    const unsigned long long t = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    if (t) atomicAdd(&out[tid], t);
  }
}

__global__ void delong_status_kernel(unsigned long long* out, const unsigned* __restrict__ status) {
  out[FBN_DELONG_REC_WORDS] = (unsigned long long)*status;
}

extern "C" size_t fbn_auc_place_workspace_size(long long n) {
  if (n < 0) n = 0;
  return place_layout(n).total;
}

extern "C" int fbn_auc_place(const uint32_t* keys, long long n, void* ws, size_t ws_bytes, uint32_t* place_out,
                             unsigned* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_auc_place: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  if (n == 0) return FBN_OK;
  if (!keys || !ws || !place_out || !status || ((uintptr_t)ws & 15) || ((uintptr_t)place_out & 3)) {
    fbn_set_error("fbn_auc_place: keys, status, a 4-B aligned place_out and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  const PlaceLayout L = place_layout(n);
  if (ws_bytes < L.total) { fbn_set_error("fbn_auc_place: ws smaller than fbn_auc_place_workspace_size(n)"); return FBN_ERR_ARG; }
  char* w = (char*)ws;
  uint64_t* comp = (uint64_t*)(w + L.comp);
  uint64_t* sorted = (uint64_t*)(w + L.sorted);
  uint32_t* negs = (uint32_t*)(w + L.negs);
  uint32_t* bsum = (uint32_t*)(w + L.bsum);
  const uint32_t un = (uint32_t)n, nb = (un + 255u) / 256u;
  fbn_launch(place_compose_kernel, dim3(nb), dim3(256), 0, st, keys, un, comp, status);
  // 32 bits = four whole digits: the sort never looks at the index above them, it only carries it
  const int rc = fbn_sort_u64(comp, n, 32, w + L.sortws, L.total - L.sortws, sorted, stream);
  if (rc != FBN_OK) return rc;
  fbn_launch(place_scan_sums_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, bsum);
  fbn_launch(scan_top_kernel<uint32_t>, dim3(1), dim3(256), 0, st, bsum, nb);
  fbn_launch(place_scan_apply_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, (const uint32_t*)bsum, negs);
  fbn_launch(place_kernel, dim3(nb), dim3(256), 0, st, (const uint64_t*)sorted, un, (const uint32_t*)negs, place_out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_delong_reduce(const uint32_t* keys_a, const uint32_t* place_a, const uint32_t* keys_b,
                                 const uint32_t* place_b, long long n, unsigned long long* out, unsigned* status,
                                 void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!out || !status || ((uintptr_t)out & 7)) {
    fbn_set_error("fbn_delong_reduce: status and an 8-B aligned out are required");
    return FBN_ERR_ARG;
  }
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_delong_reduce: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  if (n > 0 && (!keys_a || !place_a || !keys_b || !place_b)) {
    fbn_set_error("fbn_delong_reduce: keys_a, place_a, keys_b and place_b are required");
    return FBN_ERR_ARG;
  }
  if (hipMemsetAsync(out, 0, (size_t)FBN_DELONG_REC_WORDS * 8, st) != hipSuccess) {
    fbn_set_error("fbn_delong_reduce: memset failed");
    return FBN_ERR_LAUNCH;
  }
  if (n > 0) {
    const int blocks = (int)std::min<long long>(DL_BLOCKS_MAX, (n + 255) / 256);
    fbn_launch(delong_reduce_kernel, dim3(blocks), dim3(256), 0, st, keys_a, place_a, keys_b, place_b, (uint32_t)n, out, status);
  }
  fbn_launch(delong_status_kernel, dim3(1), dim3(1), 0, st, out, (const unsigned*)status);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
