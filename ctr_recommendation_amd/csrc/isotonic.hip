// Exact isotonic calibration on the device: fit the monotone map from the keys the
// evaluator holds, apply it to a batch of probabilities.
//
// Fit.  Over 0/1 labels isotonic regression is an integer problem: with the keys sorted and a group a run
// of equal score bits, the points P_0 = (0, 0), P_g = (samples, positives in groups 1 .. g) form the
// cumulative diagram, and the fitted blocks are the edges of its lower convex hull with collinear points
// dropped (pool-adjacent-violators pooling on >=).  Every decision is the sign of a difference of two
// products of coordinate differences, each below 2^62 for n < 2^31: 64-bit integers, no float anywhere.
//   w  iso_widen_kernel    the keys as u64 (a key above bits(1.0) clamped and flagged, as the calibration
//      fbn_sort_u64(31)    reduce does), sorted
//   s  iso_sums_kernel     positives per tile of ISO_T sorted samples; scan_top_kernel: their prefix
//   t  iso_tile_kernel     one workgroup per tile: the tile's group ends as points (rank + 1, positives up
//                          to it), compacted in LDS, and their hull by a merge tree in LDS (below)
//   m  iso_merge_kernel    ceil(log2(tiles)) levels: one workgroup per adjacent pair of chains finds the
//                          bridge and copies the kept prefix and suffix into the other buffer
//   o  iso_table_kernel    the tangent from P_0 to the final chain, then one thread per block
// The merge (LDS and global alike).  L and R are strict lower chains, L left of R.  For a left vertex l,
// t(l) = the R vertex of least slope from l, the rightmost of equals: slope(l, R[k]) falls then rises
// along a convex chain, so "slope(R[k], R[k+1]) <= slope(l, R[k])" is true up to t(l) and false from
// there -- a binary search.  l is the bridge's left end iff its left neighbour lies strictly above the
// line l -> t(l) and its right neighbour on or above it; exactly one l qualifies (the hull's edge over the
// gap is unique, and strictness picks the outermost of collinear candidates), so it writes the pair
// without an atomic.  Launch counts and grid sizes are functions of n alone; the actual counts live in
// device words.  No atomics except the status bit.
//
// Apply.  fbn_isotonic_apply reads K from word 0 of the table, stages lo / hi / v = pos / n (float64) in
// LDS when K <= ISO_APPLY_LDS and searches the global table otherwise; per sample one binary search for
// the first block with hi >= p and the float64 rule of DESIGN §25, every operation rounded separately.
#include "common.h"
#include "scan.h"                                // ev_block_excl_scan, scan_top_kernel, fbn_sort_u64
#include <algorithm>

#define ISO_MAX_BITS 0x3F800000u                 // bits(1.0f)
#define ISO_BAD_KEY 8u                           // status bit 3: a key fbn_eval_pack did not write
#define ISO_T 1024                               // sorted samples (and points at most) per hull tile
#define ISO_APPLY_LDS 1024                       // blocks the apply kernel stages in LDS at most

struct IsoLayout {
  size_t wide, sorted, bufa, bufb, cnta, cntb, bsum, sortws, total;
  uint32_t nt;                                   // tiles
};
static inline IsoLayout iso_layout(long long n) {
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t un = (size_t)n;
  IsoLayout L;
  L.nt = (uint32_t)((un + ISO_T - 1) / ISO_T);
  L.wide = 0;
  L.sorted = L.wide + al(un * 8);
  L.bufa = L.sorted + al(un * 8);
  L.bufb = L.bufa + al((size_t)L.nt * ISO_T * 8);
  L.cnta = L.bufb + al((size_t)L.nt * ISO_T * 8);
  L.cntb = L.cnta + al((size_t)L.nt * 4 + 4);
  L.bsum = L.cntb + al((size_t)L.nt * 4 + 4);
  L.sortws = L.bsum + al((size_t)L.nt * 4 + 4);
  L.total = L.sortws + al(fbn_sort_u64_workspace_size(n));
  return L;
}

__global__ void __launch_bounds__(256) iso_widen_kernel(const uint32_t* __restrict__ keys, uint32_t n,
                                                        uint64_t* __restrict__ wide, unsigned* status) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint32_t key = keys[i];
  if ((key >> 1) > ISO_MAX_BITS) {               // counted as 1.0, as every other reduce does
    key = (ISO_MAX_BITS << 1) | (key & 1u);
    atomicOr(status, ISO_BAD_KEY);
  }
  wide[i] = (uint64_t)key;
}

// positives of tile b of the sorted keys
__global__ void __launch_bounds__(256) iso_sums_kernel(const uint64_t* __restrict__ S, uint32_t n, uint32_t* __restrict__ bsum) {
  __shared__ uint32_t sh[4];
  const uint32_t i0 = blockIdx.x * (uint32_t)ISO_T + threadIdx.x * 4u;
  uint32_t v = 0u;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k)
    if (i0 + k < n) v += (uint32_t)(S[i0 + k] & 1ull);
  uint32_t total;
  ev_block_excl_scan<4>(v, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// a point of the cumulative diagram: x = samples, y = positives (x strictly increasing along a chain)
// slope(a, b) <= / < slope(c, d); a.x < b.x, c.x < d.x, y non-decreasing: both products are below 2^62
__device__ __forceinline__ bool iso_slope_le(uint2 a, uint2 b, uint2 c, uint2 d) {
  return (long long)(b.y - a.y) * (long long)(d.x - c.x) <= (long long)(d.y - c.y) * (long long)(b.x - a.x);
}
__device__ __forceinline__ bool iso_slope_lt(uint2 a, uint2 b, uint2 c, uint2 d) {
  return (long long)(b.y - a.y) * (long long)(d.x - c.x) < (long long)(d.y - c.y) * (long long)(b.x - a.x);
}

// the vertex of the strict lower chain R[0 .. m), m >= 1, all right of l, of least slope from l (the
// rightmost of equals)
__device__ __forceinline__ uint32_t iso_tangent(uint2 l, const uint2* R, uint32_t m) {
  uint32_t lo = 0u, hi = m - 1u;
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo) >> 1);  // mid + 1 <= hi <= m - 1
    if (iso_slope_le(R[mid], R[mid + 1u], l, R[mid])) lo = mid + 1u; else hi = mid;
  }
  return lo;
}

// L[li] is the left end of the bridge to R[t], t = iso_tangent(L[li], R, nR)
__device__ __forceinline__ bool iso_is_bridge(const uint2* L, uint32_t nL, uint32_t li, uint2 r) {
  const uint2 l = L[li];
  if (li > 0u && !iso_slope_lt(L[li - 1u], l, l, r)) return false;
  if (li + 1u < nL && !iso_slope_le(l, r, l, L[li + 1u])) return false;
  return true;
}

// element o of the merged chain: L[0 .. l] then R[r ..]
__device__ __forceinline__ uint2 iso_merged(const uint2* L, const uint2* R, uint32_t l1, uint32_t r, uint32_t o) {
  return o < l1 ? L[o] : R[r + (o - l1)];
}

__global__ void __launch_bounds__(256) iso_tile_kernel(const uint64_t* __restrict__ S, uint32_t n,
                                                       const uint32_t* __restrict__ bsum, uint2* __restrict__ buf,
                                                       uint32_t* __restrict__ cnt) {
  __shared__ uint2 pa[ISO_T], pb[ISO_T];
  __shared__ uint32_t ca[ISO_T], cb[ISO_T];
  __shared__ uint32_t bl[ISO_T / 2], br[ISO_T / 2];
  __shared__ unsigned long long sh[4];
  const uint32_t tid = threadIdx.x;
  const uint32_t i0 = blockIdx.x * (uint32_t)ISO_T + tid * 4u;
  // (group end << 32) | positive of this thread's four samples
  uint32_t e[4], y[4];
  unsigned long long v = 0ull;
  uint64_t s = i0 < n ? S[i0] : 0ull;
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    const uint32_t i = i0 + k;
    e[k] = 0u; y[k] = 0u;
    if (i < n) {
      const uint64_t nx = i + 1u < n ? S[i + 1u] : 0ull;
      y[k] = (uint32_t)(s & 1ull);
      e[k] = (i + 1u == n || (nx >> 1) != (s >> 1)) ? 1u : 0u;
      s = nx;
    }
    v += ((unsigned long long)e[k] << 32) | y[k];
  }
  unsigned long long total;
  const unsigned long long ex = ev_block_excl_scan<4>(v, sh, total);
  uint32_t pos = bsum[blockIdx.x] + (uint32_t)ex, idx = (uint32_t)(ex >> 32);
#pragma unroll
  for (uint32_t k = 0; k < 4u; ++k) {
    pos += y[k];
    if (e[k] && idx < (uint32_t)ISO_T) pa[idx++] = make_uint2(i0 + k + 1u, pos);
  }
  const uint32_t c = (uint32_t)(total >> 32);    // points of this tile, <= ISO_T
  for (uint32_t k = tid; k < (uint32_t)ISO_T; k += 256u) ca[k] = k < c ? 1u : 0u;
  __syncthreads();
  uint2 *src = pa, *dst = pb;
  uint32_t *csrc = ca, *cdst = cb;
  // the points sit at the front: once a segment spans them all, the rest of the tree only copies
  for (uint32_t lg = 0u; (1u << lg) < (uint32_t)ISO_T && (1u << lg) < c; ++lg) {     // workgroup-uniform
    const uint32_t span = 1u << lg;
    for (uint32_t q = tid; q < (uint32_t)ISO_T / 2u; q += 256u) {
      const uint32_t p = q >> lg, li = q & (span - 1u);
      const uint32_t nL = csrc[2u * p], nR = csrc[2u * p + 1u];
      if (li < nL && nR > 0u) {
        const uint2* L = src + (size_t)p * 2u * span;
        const uint2* R = L + span;
        const uint32_t t = iso_tangent(L[li], R, nR);
        if (iso_is_bridge(L, nL, li, R[t])) { bl[p] = li; br[p] = t; }
      }
    }
    __syncthreads();
    for (uint32_t k = tid; k < (uint32_t)ISO_T; k += 256u) {
      const uint32_t p = k >> (lg + 1u), o = k & (2u * span - 1u);
      const uint32_t nL = csrc[2u * p], nR = csrc[2u * p + 1u];
      const uint2* L = src + (size_t)p * 2u * span;
      const uint2* R = L + span;
      uint32_t l1 = nL, r = 0u, m = nL;          // nR == 0: the left chain as it is (the points sit at the front)
      if (nR > 0u) {                             // the clamps are never taken: they keep a read inside the chains
        l1 = bl[p] < nL ? bl[p] + 1u : nL;
        r = br[p] < nR ? br[p] : nR - 1u;
        m = l1 + (nR - r);
      }
      if (o < m) dst[k] = iso_merged(L, R, l1, r, o);
      if (o == 0u) cdst[p] = m;
    }
    __syncthreads();
    uint2* tp = src; src = dst; dst = tp;
    uint32_t* tc = csrc; csrc = cdst; cdst = tc;
  }
  const uint32_t m = csrc[0] < (uint32_t)ISO_T ? csrc[0] : (uint32_t)ISO_T;
  for (uint32_t k = tid; k < m; k += 256u) buf[(size_t)blockIdx.x * ISO_T + k] = src[k];
  if (tid == 0u) cnt[blockIdx.x] = m;
}

// workgroup p merges the chains of segments 2p and 2p + 1 (span points of room each; the last segment
// may have no partner) into segment p of the other buffer; cap = points of room in a buffer
__global__ void __launch_bounds__(256) iso_merge_kernel(const uint2* __restrict__ src, const uint32_t* __restrict__ csrc,
                                                        uint32_t nseg, unsigned long long span, unsigned long long cap,
                                                        uint2* __restrict__ dst, uint32_t* __restrict__ cdst) {
  __shared__ uint32_t b[2];
  const uint32_t tid = threadIdx.x, p = blockIdx.x;
  const unsigned long long offL = 2ull * p * span, offR = offL + span;
  // the counts never exceed the room (a chain holds at most its segment's points): the clamp keeps every
  // index inside the buffers whatever the words hold
  uint32_t nL = csrc[2u * p], nR = 2u * p + 1u < nseg ? csrc[2u * p + 1u] : 0u;
  const unsigned long long roomL = offL >= cap ? 0ull : (cap - offL < span ? cap - offL : span);
  const unsigned long long roomR = offR >= cap ? 0ull : (cap - offR < span ? cap - offR : span);
  if (nL > roomL) nL = (uint32_t)roomL;
  if (nR > roomR) nR = (uint32_t)roomR;
  const uint2* L = src + offL;
  const uint2* R = src + offR;
  if (tid < 2u) b[tid] = 0u;
  __syncthreads();
  if (nL > 0u && nR > 0u) {                      // workgroup-uniform
    for (uint32_t li = tid; li < nL; li += 256u) {
      const uint32_t t = iso_tangent(L[li], R, nR);
      if (iso_is_bridge(L, nL, li, R[t])) { b[0] = li; b[1] = t; }
    }
  }
  __syncthreads();
  uint32_t l1 = nL, r = 0u, m = nL + nR;         // an empty side: the other chain as it is
  if (nL > 0u && nR > 0u) {
    l1 = b[0] < nL ? b[0] + 1u : nL;
    r = b[1] < nR ? b[1] : nR - 1u;
    m = l1 + (nR - r);
  }
  uint2* D = dst + offL;
  for (uint32_t o = tid; o < m; o += 256u) D[o] = iso_merged(L, R, l1, r, o);
  if (tid == 0u) cdst[p] = m;
}

// table: word 0 = K; block j: word 1 + 2j = bits(lo) | bits(hi) << 32, word 2 + 2j = n | pos << 32;
// word 1 + 2K = the status word
__global__ void __launch_bounds__(256) iso_table_kernel(const uint64_t* __restrict__ S, uint32_t n, const uint2* __restrict__ H,
                                                        const uint32_t* __restrict__ cnt, uint32_t maxk,
                                                        const unsigned* __restrict__ status, uint64_t* __restrict__ table) {
  __shared__ uint32_t sht;
  const uint32_t m = cnt[0] < n ? cnt[0] : n;    // vertices of the hull of P_1 .. P_G; >= 1 (P_G)
  if (threadIdx.x == 0) sht = m ? iso_tangent(make_uint2(0u, 0u), H, m) : 0u;      // P_0's edge
  __syncthreads();
  const uint32_t t = sht;
  uint32_t K = m - t;
  if (K > maxk) K = maxk;                        // never (K <= fbn_isotonic_max_blocks(n)): keeps the writes inside the table
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j == 0u) { table[0] = (uint64_t)K; table[1 + 2 * (size_t)K] = (uint64_t)*status; }
  if (j >= K) return;
  const uint2 a = j == 0u ? make_uint2(0u, 0u) : H[t + j - 1u];
  const uint2 bb = H[t + j];
  const uint32_t first = a.x < n ? a.x : n - 1u, last = (bb.x >= 1u && bb.x <= n) ? bb.x - 1u : n - 1u;
  const uint64_t lo = (S[first] >> 1) & 0xFFFFFFFFull, hi = (S[last] >> 1) & 0xFFFFFFFFull;
  table[1 + 2 * (size_t)j] = lo | (hi << 32);
  table[2 + 2 * (size_t)j] = (uint64_t)(bb.x - a.x) | ((uint64_t)(bb.y - a.y) << 32);
}

__global__ void iso_empty_kernel(const unsigned* __restrict__ status, uint64_t* __restrict__ table) {
  table[0] = 0ull;
  table[1] = (uint64_t)*status;
}

// ---------------------------------------------------------------- apply
// the block value is pos / n: the table word is n | pos << 32
__device__ __forceinline__ double iso_value(uint64_t w) {
  return __ddiv_rn((double)(uint32_t)(w >> 32), (double)(uint32_t)w);
}

__global__ void __launch_bounds__(256) iso_apply_kernel(const float* p, long long n, const uint64_t* __restrict__ table, int mode,
                                                        float* out) {
  __shared__ float slo[ISO_APPLY_LDS], shi[ISO_APPLY_LDS];
  __shared__ double sv[ISO_APPLY_LDS];
  const uint64_t k64 = table[0];
  const uint32_t K = k64 > 0x7FFFFFFFull ? 0x7FFFFFFFu : (uint32_t)k64;
  const bool lds = K <= (uint32_t)ISO_APPLY_LDS;
  if (lds) {
    for (uint32_t j = threadIdx.x; j < K; j += 256u) {
      const uint64_t w = table[1 + 2 * (size_t)j];
      slo[j] = __uint_as_float((uint32_t)w);
      shi[j] = __uint_as_float((uint32_t)(w >> 32));
      sv[j] = iso_value(table[2 + 2 * (size_t)j]);
    }
    __syncthreads();
  }
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const float pf = p[i];
    float res;
    if (pf != pf || K == 0u) {
      res = pf != pf ? pf : __uint_as_float(0x7FC00000u);   // NaN passes through; an empty table maps to NaN (the host refuses it)
    } else {
      uint32_t a = 0u, b = K;                    // the first block with hi >= p (K: none)
      while (a < b) {
        const uint32_t mid = a + ((b - a) >> 1);
        const float h = lds ? shi[mid] : __uint_as_float((uint32_t)(table[1 + 2 * (size_t)mid] >> 32));
        if (h >= pf) b = mid; else a = mid + 1u;
      }
      const uint32_t j = a < K ? a : K - 1u;
      const double vj = lds ? sv[j] : iso_value(table[2 + 2 * (size_t)j]);
      const float lo = lds ? slo[j] : __uint_as_float((uint32_t)table[1 + 2 * (size_t)j]);
      double r = vj;
      if (mode == 0 && a < K && j > 0u && !(pf >= lo)) {     // in the gap below block j: interpolate
        const double vp = lds ? sv[j - 1u] : iso_value(table[2 + 2 * (size_t)(j - 1u)]);
        const double hp = (double)(lds ? shi[j - 1u] : __uint_as_float((uint32_t)(table[1 + 2 * (size_t)(j - 1u)] >> 32)));
        // every operation rounded on its own (no FMA contraction)
        const double t = __ddiv_rn(__dsub_rn((double)pf, hp), __dsub_rn((double)lo, hp));
        r = fmin(__dadd_rn(vp, __dmul_rn(t, __dsub_rn(vj, vp))), vj);
      }
      res = (float)r;                            // the one rounding to fp32
    }
    out[i] = res;
  }
}

// ---------------------------------------------------------------- entry points
// floor((3n)^(2/3) / 2) + 2: the integer cube root of 9 n^2 (below 2^66: 128-bit), halved
extern "C" long long fbn_isotonic_max_blocks(long long n) {
  if (n < 0) n = 0;
  const unsigned __int128 m = (unsigned __int128)9 * (unsigned __int128)n * (unsigned __int128)n;
  unsigned long long lo = 0ull, hi = 1ull << 23;  // cbrt(9 * 2^62) < 2^22
  while (lo < hi) {                              // the largest r with r^3 <= m
    const unsigned long long mid = lo + (hi - lo + 1ull) / 2ull;
    if ((unsigned __int128)mid * mid * mid <= m) lo = mid; else hi = mid - 1ull;
  }
  return (long long)(lo / 2ull) + 2;
}

extern "C" size_t fbn_isotonic_workspace_size(long long n) {
  if (n < 0) n = 0;
  return iso_layout(n).total;
}

extern "C" int fbn_isotonic_fit(const uint32_t* keys, long long n, void* ws, size_t ws_bytes, uint64_t* table,
                                long long table_words, unsigned* status, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (!table || !status || ((uintptr_t)table & 7)) {
    fbn_set_error("fbn_isotonic_fit: status and an 8-B aligned table are required");
    return FBN_ERR_ARG;
  }
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_isotonic_fit: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  const long long maxk = n == 0 ? 0 : fbn_isotonic_max_blocks(n);
  if (table_words < 2 * maxk + 2) {
    fbn_set_error("fbn_isotonic_fit: table shorter than 2 * fbn_isotonic_max_blocks(n) + 2 words");
    return FBN_ERR_ARG;
  }
  if (n == 0) {
    fbn_launch(iso_empty_kernel, dim3(1), dim3(1), 0, st, (const unsigned*)status, table);
    FBN_CHECK_LAUNCH();
    return FBN_OK;
  }
  if (!keys || !ws || ((uintptr_t)ws & 15)) {
    fbn_set_error("fbn_isotonic_fit: keys and a 16-B aligned ws are required");
    return FBN_ERR_ARG;
  }
  const IsoLayout L = iso_layout(n);
  if (ws_bytes < L.total) { fbn_set_error("fbn_isotonic_fit: ws smaller than fbn_isotonic_workspace_size(n)"); return FBN_ERR_ARG; }
  char* w = (char*)ws;
  uint64_t* wide = (uint64_t*)(w + L.wide);
  uint64_t* sorted = (uint64_t*)(w + L.sorted);
  uint2* buf[2] = {(uint2*)(w + L.bufa), (uint2*)(w + L.bufb)};
  uint32_t* cnt[2] = {(uint32_t*)(w + L.cnta), (uint32_t*)(w + L.cntb)};
  uint32_t* bsum = (uint32_t*)(w + L.bsum);
  const uint32_t un = (uint32_t)n, nt = L.nt;
  fbn_launch(iso_widen_kernel, dim3((un + 255u) / 256u), dim3(256), 0, st, keys, un, wide, status);
  const int rc = fbn_sort_u64(wide, n, 31, w + L.sortws, L.total - L.sortws, sorted, stream);
  if (rc != FBN_OK) return rc;
  fbn_launch(iso_sums_kernel, dim3(nt), dim3(256), 0, st, (const uint64_t*)sorted, un, bsum);
  fbn_launch(scan_top_kernel<uint32_t>, dim3(1), dim3(256), 0, st, bsum, nt);
  fbn_launch(iso_tile_kernel, dim3(nt), dim3(256), 0, st, (const uint64_t*)sorted, un, (const uint32_t*)bsum, buf[0], cnt[0]);
  int cur = 0;
  unsigned long long span = ISO_T;
  const unsigned long long cap = (unsigned long long)nt * ISO_T;
  for (uint32_t nseg = nt; nseg > 1u; nseg = (nseg + 1u) / 2u, span *= 2ull, cur ^= 1)
    fbn_launch(iso_merge_kernel, dim3((nseg + 1u) / 2u), dim3(256), 0, st, (const uint2*)buf[cur], (const uint32_t*)cnt[cur],
               nseg, span, cap, buf[cur ^ 1], cnt[cur ^ 1]);
  fbn_launch(iso_table_kernel, dim3((unsigned)((maxk + 255) / 256)), dim3(256), 0, st, (const uint64_t*)sorted, un,
             (const uint2*)buf[cur], (const uint32_t*)cnt[cur], (uint32_t)maxk, (const unsigned*)status, table);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}

extern "C" int fbn_isotonic_apply(const float* p, long long n, const uint64_t* table, int mode, float* out, void* stream) {
  if (n < 0 || n >= (1ll << 31)) { fbn_set_error("fbn_isotonic_apply: need 0 <= n < 2^31"); return FBN_ERR_ARG; }
  if (mode != 0 && mode != 1) { fbn_set_error("fbn_isotonic_apply: mode must be 0 (interp) or 1 (step)"); return FBN_ERR_ARG; }
  if (!table || ((uintptr_t)table & 7)) { fbn_set_error("fbn_isotonic_apply: an 8-B aligned table is required"); return FBN_ERR_ARG; }
  if (n == 0) return FBN_OK;
  if (!p || !out) { fbn_set_error("fbn_isotonic_apply: null argument"); return FBN_ERR_ARG; }
  const int blocks = (int)std::min<long long>(2048, (n + 255) / 256);
  fbn_launch(iso_apply_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, p, n, table, mode, out);
  FBN_CHECK_LAUNCH();
  return FBN_OK;
}
