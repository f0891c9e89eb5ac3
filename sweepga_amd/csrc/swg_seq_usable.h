// What the calls that read bases through the CIGARs share (DESIGN.md sections 36 and 37): the sequence set in device memory, the
// check of its offsets, the usable test of one entry, the entry of an op, and four bases as one 32-bit load.  swg_eqx.hip and
// swg_maf.hip call them from kernels of their own (the profile's launch labels are kernel names).
#pragma once
#include "swg_cigar_build.h"

namespace swg_seq_usable {

struct Seqs {  // device pointers
  const uint64_t* offset;
  const uint8_t* bases;
  uint64_t n_bases;
};

#ifdef __HIPCC__
__device__ __forceinline__ void count_votes(bool vote, unsigned long long* slot) {
  const uint64_t votes = __ballot(vote);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(slot, (unsigned long long)__popcll(votes));
}

// whether the offsets descend behind sequence s
__device__ __forceinline__ bool offsets_descend(const uint64_t* __restrict__ offset, uint32_t n_seq, uint64_t s) {
  return s < n_seq && offset[s + 1] < offset[s];
}

// The usable test of entry j (j < S.k): state 0, record in `set`, both sequences present, t_end <= len(t), q_end <= len(q).  The
// first failing test is the one that is set; bad_id (a sequence id >= n_seq) refuses the call.
struct Usable {
  bool ok, empty, bad_id, no_seq, out_seq;
};
__device__ __forceinline__ Usable usable_of(const swg_cigar::CigarSet& S, const swg_lift_ix::LiftCols& c, uint32_t n_seq, uint32_t set,
                                            const uint64_t* __restrict__ seq_off, uint64_t j) {
  Usable u{false, false, false, false, false};
  const uint32_t rec = S.record[j], st = reinterpret_cast<const uint8_t*>(S.state)[j];
  u.empty = st == swg_cigar::ST_EMPTY;
  if (set == SWG_IV_ALL || c.status[rec] != 0) {
    const uint32_t q = c.id[0][rec], t = c.id[1][rec];
    u.bad_id = q >= n_seq || t >= n_seq;
    if (!u.bad_id && st == 0) {
      const uint64_t q0 = seq_off[q], q1 = seq_off[q + 1], t0 = seq_off[t], t1 = seq_off[t + 1];
      u.no_seq = !(q1 > q0 && t1 > t0);
      u.out_seq = !u.no_seq && !(c.end[0][rec] <= q1 - q0 && c.end[1][rec] <= t1 - t0);
      u.ok = !u.no_seq && !u.out_seq;
    }
  }
  return u;
}

// the last entry j in [lo, hi] with op_first[j] <= r (op_first[lo] <= r): of several entries that begin at one op all but the last
// are empty
__device__ __forceinline__ uint32_t entry_at(const uint32_t* __restrict__ op_first, uint32_t lo, uint32_t hi, uint32_t r) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (op_first[mid] <= r) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

// the four bytes at bases[at .. at + 4), all inside the bases, byte 0 in bits 0 .. 7: one aligned 32-bit load, or two and a shift
// where both lie inside the bases, else four byte loads
__device__ __forceinline__ uint32_t load_quad(const Seqs& seqs, uint64_t at) {
  const uint8_t* p = seqs.bases + at;
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const uint32_t sh = (uint32_t)(a & 3u);
  const uint32_t* w = reinterpret_cast<const uint32_t*>(a - sh);
  if (sh == 0) return w[0];
  if (reinterpret_cast<const uint8_t*>(w) >= seqs.bases && reinterpret_cast<const uint8_t*>(w + 2) <= seqs.bases + seqs.n_bases)
    return (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> (8 * sh));
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
}
#endif

}  // namespace swg_seq_usable
