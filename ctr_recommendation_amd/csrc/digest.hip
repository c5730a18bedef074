// Order-independent 64-bit digest of a device buffer (fbn_digest_u64, include/fibinet.h):
// the integrity check of a full-state checkpoint where the state lives, and the tests' exact state
// comparison.  Over the buffer's 32-bit words w_i,
//   *out += sum_i mix64((base + i + 1) * GOLDEN + w_i)      (mod 2^64; mix64 = splitmix64's finaliser)
// The position enters through the key, so two swapped words change the sum; the sum itself is integer,
// so any grid, any order and atomics give the same value, and chunks compose through `base`.
//
// Memory-bound shape: the 16-byte-aligned body is read as uint4 (the buffer is only 4-byte aligned -- a
// parameter's view inside the flat buffer starts anywhere -- so up to three head and three tail words
// are read as scalars by the first workgroup), DIGEST_UNROLL independent loads per lane and round of a
// grid-stride loop, a wave-64 shuffle reduction, one LDS step per workgroup, one 64-bit atomic per
// workgroup.  Every index is 64-bit.
#include "common.h"

#define DIGEST_THREADS 256
#define DIGEST_UNROLL 4
#define DIGEST_WG_PER_CU 8

#define DIGEST_GOLDEN 0x9E3779B97F4A7C15ull

__device__ __forceinline__ uint64_t digest_mix64(uint64_t x) {
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return x;
}

// the term of word w at (base-relative) index i: key = (base + i + 1) * GOLDEN, passed in
__device__ __forceinline__ uint64_t digest_term(uint64_t key, uint32_t w) { return digest_mix64(key + (uint64_t)w); }

// x[0 .. n): head words [0, head), nvec uint4 from x + head, tail words [head + 4 nvec, n)
__global__ void __launch_bounds__(DIGEST_THREADS) digest_kernel(const uint32_t* __restrict__ x, long long n, int head,
                                                                long long nvec, uint64_t base,
                                                                unsigned long long* __restrict__ out) {
  __shared__ uint64_t part[DIGEST_THREADS / FBN_WAVE];
  const uint4* __restrict__ body = (const uint4*)(x + head);
  const long long stride = (long long)gridDim.x * DIGEST_THREADS;
  const uint64_t key0 = (base + (uint64_t)head + 1ull) * DIGEST_GOLDEN;     // key of the body's first word
  uint64_t acc = 0;
  for (long long v0 = (long long)blockIdx.x * DIGEST_THREADS + threadIdx.x; v0 < nvec; v0 += stride * DIGEST_UNROLL) {
    uint4 q[DIGEST_UNROLL];
#pragma unroll
    for (int u = 0; u < DIGEST_UNROLL; ++u) {
      const long long v = v0 + u * stride;
      q[u] = v < nvec ? body[v] : make_uint4(0u, 0u, 0u, 0u);
    }
#pragma unroll
    for (int u = 0; u < DIGEST_UNROLL; ++u) {
      const long long v = v0 + u * stride;
      if (v < nvec) {
        const uint64_t k = key0 + (uint64_t)(4 * v) * DIGEST_GOLDEN;
        acc += digest_term(k, q[u].x) + digest_term(k + DIGEST_GOLDEN, q[u].y) +
               digest_term(k + 2 * DIGEST_GOLDEN, q[u].z) + digest_term(k + 3 * DIGEST_GOLDEN, q[u].w);
      }
    }
  }
  if (blockIdx.x == 0) {
    // head and tail: at most three words each, one lane per word
    const long long tail0 = (long long)head + 4 * nvec;
    const int ntail = (int)(n - tail0);
    const int t = threadIdx.x;
    long long i = -1;
    if (t < head) i = t;
    else if (t - head < ntail) i = tail0 + (t - head);
    if (i >= 0) acc += digest_term((base + (uint64_t)i + 1ull) * DIGEST_GOLDEN, x[i]);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (uint64_t)__shfl_xor((unsigned long long)acc, o, 64);
  const int wave = threadIdx.x / FBN_WAVE;
  if ((threadIdx.x & (FBN_WAVE - 1)) == 0) part[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0;
#pragma unroll
    for (int w = 0; w < DIGEST_THREADS / FBN_WAVE; ++w) s += part[w];
    if (s) atomicAdd(out, (unsigned long long)s);
  }
}

// compute units of the current device (queried once)
static int digest_cus() {
  static int cus = 0;
  if (cus <= 0) {
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
      n = 256;
    cus = n;
  }
  return cus;
}

extern "C" int fbn_digest_u64(const void* x, long long n_words, unsigned long long base, unsigned long long* out,
                              void* stream) {
  if (n_words < 0) { fbn_set_error("fbn_digest_u64: n_words >= 0"); return FBN_ERR_ARG; }
  if (n_words == 0) return FBN_OK;
  if (!x || !out || ((uintptr_t)x & 3) || ((uintptr_t)out & 7)) {
    fbn_set_error("fbn_digest_u64: x (4-B aligned) and out (8-B aligned) are required");
    return FBN_ERR_ARG;
  }
  // words before the first 16-byte boundary, then whole uint4, then the rest
  long long head = (long long)(((16 - ((uintptr_t)x & 15)) & 15) / 4);
  if (head > n_words) head = n_words;
  const long long nvec = (n_words - head) / 4;
  long long grid = (nvec + (long long)DIGEST_THREADS * DIGEST_UNROLL - 1) / ((long long)DIGEST_THREADS * DIGEST_UNROLL);
  const long long cap = (long long)digest_cus() * DIGEST_WG_PER_CU;
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  fbn_launch(digest_kernel, dim3((unsigned)grid), dim3(DIGEST_THREADS), 0, (hipStream_t)stream, (const uint32_t*)x,
             n_words, (int)head, nvec, (uint64_t)base, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
