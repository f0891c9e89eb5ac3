// What the calls built on parsed CIGARs share (swg_cigar.hip has the kernels; DESIGN.md sections 30 and 31): the set in device
// memory, its check, and cigar_build -- parse, the four exclusive prefix sums, op_first[] and a state byte per entry.  The base-exact
// lift (swg_cigar.hip) and the chain files (swg_ucsc.hip) both start from here.
#pragma once
#include "swg_internal.h"
#include "swg_lift_index.h"
#include "swg_cigar_walk.h"

namespace swg_cigar {

// device scalars of cigar_set_check and cigar_build; a caller's own scalars follow from C_BUILD_TOTAL on
enum { C_BAD = 0, C_BYTES = 1, C_BAD_ENTRIES = 2, C_BUILD_TOTAL = 3 };

struct CigarSet {  // device pointers
  uint64_t k, B, ops;
  const uint32_t* record;
  const uint64_t* offset;
  const char* text;
  const uint32_t* chunk_rank;
  uint32_t* op_first;  // [k + 1]
  uint32_t* state;     // the state bytes, four to a word
  Prefix P;
};

// The refusals of a set, in the words of `who`: k >= 2^31, NULL arrays, and -- the arrays on the host -- a record >= n, records that
// do not ascend strictly, offsets that do not start at 0 or decrease, a NULL text; *B receives offset[k].  k == 0 passes.
int cigar_set_check_host(swg_ctx* ctx, const char* who, const swg_cigar_set* cigars, bool on_device, uint64_t n, uint64_t* B);
// The same checks of the arrays in device memory, inside the arena frame: one thread per entry, the error word and offset[k] read
// back into S->B.  scalars: C_BUILD_TOTAL device words or more, zero before.
int cigar_set_check_device(swg_ctx* ctx, const char* who, uint64_t n, CigarSet* S, unsigned long long* scalars);
// Parse, prefix sums and entry states of a set whose arrays are in device memory (inside an arena frame).  S->k, B, record, offset
// and text are the caller's; everything else is filled in.  scalars[C_BAD_ENTRIES] counts the entries with a state bit of 1 .. 8.
int cigar_build(swg_ctx* ctx, const char* who, const swg_lift_ix::LiftCols& c, CigarSet* S, unsigned long long* scalars);

#ifdef __HIPCC__
// the ops in front of text byte p
__device__ __forceinline__ uint32_t rank_at(const CigarSet& S, uint64_t p) {
  if (p >= S.B) return (uint32_t)S.ops;
  uint32_t r = S.chunk_rank[p >> 4];
  for (uint64_t q = p & ~uint64_t(15); q < p; ++q) r += is_digit((unsigned char)S.text[q]) ? 0u : 1u;
  return r;
}
#endif

}  // namespace swg_cigar
