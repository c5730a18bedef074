// The selection key of the serving kernels (recommend.hip, diversify.hip) and the id rule of their
// exclusion: one definition, so every selection orders and filters candidates the same way.
#pragma once
#include "common.h"

// key = {ordered image of the f32 score (32) | 0xFFFFFFFF - pos (32)}: unique per candidate, and a larger
// key is a larger score or, on equal scores, a smaller pos.  0 is the "no candidate" key; a NaN score
// takes the high word 1, below -inf's 0x007FFFFF.
__device__ __forceinline__ unsigned long long rec_key(float x, unsigned pos, bool& nan) {
  const unsigned b = __float_as_uint(x);
  nan = (b & 0x7FFFFFFFu) > 0x7F800000u;
  const unsigned o = nan ? 1u : ((b & 0x80000000u) ? ~b : (b | 0x80000000u));
  return ((unsigned long long)o << 32) | (unsigned long long)(0xFFFFFFFFu - pos);
}
__device__ __forceinline__ float rec_key_logit(unsigned long long key) {
  const unsigned o = (unsigned)(key >> 32);
  if (o == 1u) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}

// exclude: the padding item (id 0) and every non-padding id of the user's history hist[0, L)
__device__ __forceinline__ bool rec_id_excluded(const long long* hist, int L, long long id) {
  bool ex = id == 0;
  for (int l = 0; l < L; ++l) ex |= hist[l] != 0 && hist[l] == id;
  return ex;
}
