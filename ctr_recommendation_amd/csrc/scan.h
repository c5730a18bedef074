// Workgroup prefix sums shared by the device metrics (metrics.hip) and the radix sort (sort.hip).
#pragma once
#include "common.h"

// exclusive prefix sum of v over a workgroup of NW waves (sh: NW words); total = the workgroup's sum
template <int NW, typename T>
__device__ __forceinline__ T ev_block_excl_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  T incl = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(incl, o, 64);
    if (lane >= o) incl += t;
  }
  __syncthreads();                               // sh may still be read from the previous scan
  if (lane == 63) sh[w] = incl;
  __syncthreads();
  T base = 0, tot = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    const T s = sh[k];
    if (k < w) base += s;
    tot += s;
  }
  total = tot;
  return base + incl - v;
}

// In-place exclusive scan of the nb block sums of a two-level scan: one workgroup of 256 walks them
// in chunks of 256 with a running carry (nb = n / 256 at most: 2^23 words, 2^15 chunks).
template <typename T>
__global__ void __launch_bounds__(256) scan_top_kernel(T* bsum, uint32_t nb) {
  __shared__ T sh[4];
  T carry = 0;
  for (uint32_t c = 0; c < nb; c += 256) {       // workgroup-uniform
    const uint32_t i = c + threadIdx.x;
    const T v = i < nb ? bsum[i] : (T)0;
    T total;
    const T ex = ev_block_excl_scan<4>(v, sh, total);
    if (i < nb) bsum[i] = carry + ex;
    carry += total;
  }
}

