// The kind byte of every op, shared by the difference list (swg_diffs.hip) and the divergence track
// (swg_divergence.hip): one thread per 16-byte chunk of the text writes, from chunk_rank[chunk] on, a kind byte at the rank of every
// byte that is no digit (the prefix sums cannot tell M from X, or D from N).  Every byte has one writer.  A user keeps its own
// __global__ entry (the profile's launch labels are kernel names).
#pragma once
#include "swg_cigar_build.h"
#include "swg_diffs_walk.h"

namespace swg_diffs {

#ifdef __HIPCC__
__device__ __forceinline__ void letters_of_chunk(const swg_cigar::CigarSet& S, int aligned, uint64_t chunk, uint8_t* __restrict__ kind) {
  using swg_cigar::is_digit;
  const uint64_t p0 = chunk * 16;
  if (p0 >= S.B) return;
  unsigned char ch[16];
  if (aligned && p0 + 16 <= S.B) {
    const uint4 q = *reinterpret_cast<const uint4*>(S.text + p0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) ch[b] = (unsigned char)(w[b >> 2] >> (8 * (b & 3)));
  } else {
#pragma unroll
    for (int b = 0; b < 16; ++b) ch[b] = p0 + b < S.B ? (unsigned char)S.text[p0 + b] : (unsigned char)'0';  // (a digit: never an op)
  }
  uint64_t r = S.chunk_rank[chunk];
#pragma unroll
  for (int b = 0; b < 16; ++b) {
    if (is_digit(ch[b])) continue;
    if (r < S.ops) kind[r] = (uint8_t)kind_of(ch[b]);  // (always: the ranks are the parse's own count of these bytes)
    ++r;
  }
}
#endif

}  // namespace swg_diffs
