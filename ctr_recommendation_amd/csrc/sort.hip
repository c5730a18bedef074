// Device radix sort of 64-bit keys (fbn_sort_u64, include/fibinet.h): the library's
// general sort, first used by the grouped AUC of metrics.hip, whose grouping key is an arbitrary
// 32-bit id that §15's counting trick cannot bucket.
//
// LSD, 8 bits per pass, ceil(bits / 8) passes chosen by the host (no device round trip).  A pass:
//   H  sort_hist_kernel     digit counts of each tile of FBN_SORT_TILE keys into table[digit][tile]
//   S  sort_scan_* + top    exclusive scan of the table in that (digit-major) order: where each
//                           tile's keys of each digit start in the output
//   X  sort_scatter_kernel  STABLE scatter.  A wave takes 64 consecutive keys per step, in order;
//                           a lane finds its same-digit peers with eight 64-bit ballots; its rank is
//                           the popcount of the peers below it plus the wave's running digit counter
//                           in LDS; the waves' counters are then prefixed in wave order.  So equal
//                           digits keep tile, wave, step and lane order: the input order.
// The passes ping-pong between out and one buffer of the workspace so that the last one lands in
// out; in is only read.  No allocation, no host synchronisation; every offset is below n < 2^31.
#include "scan.h"

#define SORT_THREADS 256
#define SORT_WAVES (SORT_THREADS / 64)
#define SORT_STEPS (FBN_SORT_TILE / SORT_THREADS)          // keys per lane; a wave owns 64 * SORT_STEPS consecutive keys
static_assert(FBN_SORT_TILE % SORT_THREADS == 0, "whole steps");

static inline size_t sort_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline uint32_t sort_tiles(long long n) { return (uint32_t)((n + FBN_SORT_TILE - 1) / FBN_SORT_TILE); }

// ---------------------------------------------------------------- H: per-tile digit counts
__global__ void __launch_bounds__(SORT_THREADS) sort_hist_kernel(const uint64_t* __restrict__ in, uint32_t n, int shift,
                                                                 uint32_t tiles, uint32_t* __restrict__ table) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x;
  h[tid] = 0u;
  __syncthreads();
  const uint32_t base = blockIdx.x * (uint32_t)FBN_SORT_TILE;
#pragma unroll
  for (int s = 0; s < SORT_STEPS; ++s) {
    const uint32_t i = base + s * SORT_THREADS + tid;
    if (i < n) atomicAdd(&h[(uint32_t)(in[i] >> shift) & 255u], 1u);
  }
  __syncthreads();
  table[(size_t)tid * tiles + blockIdx.x] = h[tid];
}

// ---------------------------------------------------------------- S: scan of table[0 .. m), 256 words per workgroup
__global__ void __launch_bounds__(256) sort_scan_sums_kernel(const uint32_t* __restrict__ table, uint32_t m,
                                                             uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t total;
  ev_block_excl_scan<4>(i < m ? table[i] : 0u, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(256) sort_scan_apply_kernel(uint32_t* table, uint32_t m, const uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  uint32_t total;
  const uint32_t ex = ev_block_excl_scan<4>(i < m ? table[i] : 0u, sh, total);
  if (i < m) table[i] = bsum[blockIdx.x] + ex;
}

// ---------------------------------------------------------------- X: stable scatter
__global__ void __launch_bounds__(SORT_THREADS) sort_scatter_kernel(const uint64_t* __restrict__ in, uint32_t n, int shift,
                                                                    uint32_t tiles, const uint32_t* __restrict__ table,
                                                                    uint64_t* __restrict__ out) {
  __shared__ uint32_t wcnt[SORT_WAVES][256];     // per wave: running digit counter, then the wave's digit base
  const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < SORT_WAVES; ++k) wcnt[k][tid] = 0u;
  __syncthreads();
  const uint32_t wbase = blockIdx.x * (uint32_t)FBN_SORT_TILE + w * (64u * SORT_STEPS);
  const uint64_t below_mask = (1ull << lane) - 1ull;
  uint64_t key[SORT_STEPS];
  uint32_t rank[SORT_STEPS];
#pragma unroll
  for (int s = 0; s < SORT_STEPS; ++s) {         // wave-uniform: every lane reaches every ballot
    const uint32_t i = wbase + s * 64u + lane;
    const bool valid = i < n;
    key[s] = valid ? in[i] : 0ull;
    const uint32_t d = (uint32_t)(key[s] >> shift) & 255u;
    uint64_t peers = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = __ballot(valid && bit);
      peers &= bit ? m : ~m;
    }
    // a valid lane is its own peer; the lowest peer takes the wave's counter for all of them
    const uint64_t below = peers & below_mask;
    uint32_t prev = 0u;
    if (valid && below == 0ull) prev = atomicAdd(&wcnt[w][d], (uint32_t)__popcll(peers));
    prev = __shfl(prev, valid ? __ffsll((unsigned long long)peers) - 1 : (int)lane, 64);
    rank[s] = prev + (uint32_t)__popcll(below);
  }
  __syncthreads();
  {                                              // thread = digit: this tile's start, then the waves in order
    uint32_t g = table[(size_t)tid * tiles + blockIdx.x];
#pragma unroll
    for (int k = 0; k < SORT_WAVES; ++k) {
      const uint32_t c = wcnt[k][tid];
      wcnt[k][tid] = g;
      g += c;
    }
  }
  __syncthreads();
#pragma unroll
  for (int s = 0; s < SORT_STEPS; ++s) {
    const uint32_t i = wbase + s * 64u + lane;
    if (i < n) {
      const uint32_t dst = wcnt[w][(uint32_t)(key[s] >> shift) & 255u] + rank[s];
      if (dst < n) out[dst] = key[s];            // always true: the scanned table partitions [0, n)
    }
  }
}

// ---------------------------------------------------------------- entry points
extern "C" size_t fbn_sort_u64_workspace_size(long long n) {
  if (n < 0) n = 0;
  const size_t tiles = sort_tiles(n);
  return 256 + sort_align((size_t)n * 8) + sort_align(tiles * 256 * 4) + sort_align(tiles * 4);
}

extern "C" int fbn_sort_u64(const uint64_t* in, long long n, int bits, void* ws, size_t ws_bytes, uint64_t* out,
                            void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_sort_u64: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  if (bits < 1 || bits > 64) { fbn_set_error("fbn_sort_u64: bits must be in [1, 64]"); return FBN_ERR_ARG; }
  if (n == 0) return FBN_OK;
  if (!in || !out || !ws || in == out || ((uintptr_t)ws & 15) || ((uintptr_t)in & 7) || ((uintptr_t)out & 7)) {
    fbn_set_error("fbn_sort_u64: in, out (distinct, 8-B aligned) and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  if (ws_bytes < fbn_sort_u64_workspace_size(n)) {
    fbn_set_error("fbn_sort_u64: ws smaller than fbn_sort_u64_workspace_size(n)");
    return FBN_ERR_ARG;
  }
  const uint32_t un = (uint32_t)n, tiles = sort_tiles(n), m = tiles * 256u;   // m <= 2^28
  char* w = (char*)ws;
  uint64_t* tmp = (uint64_t*)w;
  uint32_t* table = (uint32_t*)(w + sort_align((size_t)n * 8));
  uint32_t* bsum = (uint32_t*)((char*)table + sort_align((size_t)m * 4));
  const int passes = (bits + 7) / 8;
  const uint64_t* src = in;
  for (int p = 0; p < passes; ++p) {
    uint64_t* dst = ((passes - 1 - p) & 1) ? tmp : out;      // the last pass writes out
    const int shift = 8 * p;
    fbn_launch(sort_hist_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, src, un, shift, tiles, table);
    fbn_launch(sort_scan_sums_kernel, dim3(tiles), dim3(256), 0, st, (const uint32_t*)table, m, bsum);
    fbn_launch(scan_top_kernel<uint32_t>, dim3(1), dim3(256), 0, st, bsum, tiles);
    fbn_launch(sort_scan_apply_kernel, dim3(tiles), dim3(256), 0, st, table, m, (const uint32_t*)bsum);
    fbn_launch(sort_scatter_kernel, dim3(tiles), dim3(SORT_THREADS), 0, st, src, un, shift, tiles, (const uint32_t*)table,
               dst);
    src = dst;
  }
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
