// Variant calls: every SNV, insertion and deletion inside the mappings with its bases, from the CIGARs and the
// sequences -- one 32-byte variant per differing column under X or M and per anchored I or D, its alleles in a pool, sums per genome
// pair.  The parse, the four prefix sums, op_first[] and the entry states are cigar_build's, the kind bytes letters_of_chunk's;
// include/sweepga_gpu.h states the definitions, swg_variants_walk.h holds the rules.
//
//   variants_letters   the kind byte of every op (swg_diffs_letters.h).
//   variants_entries   one thread per entry: usable or not (state 0, record in the set, genome filters, both sequences present,
//                      the record inside them), the ids checked, the genome pair into entry_key[] (EMPTY: not usable), `entries`
//                      into the genome-pair table, no_sequence / out_of_sequence into the scalars.
//   variants_ops       a tile of 1,024 ops per work-group, 4 consecutive ones per thread, entries found as diffs_ops finds them: the
//                      op's CANDIDATES into a u64 array -- l for X and M, 1 for an I or D that gives a variant, else 0 -- and the
//                      six indel sums (runs of one pair folded along the wavefront, LDS table, one flush).
//   (scan)             the candidates' exclusive sums C[]: candidate s belongs to the op r with C[r] <= s < C[r + 1], so the
//                      candidates lie in (entry, op, column) order and one flag array over them needs no merge.
//   variants_columns   a tile of 1,024 candidates per work-group, thread t takes t, t + 256, ...: consecutive lanes read consecutive
//                      target bytes and consecutive (on '-' descending) query bytes.  The tile's first and last op and entry are
//                      searched once per work-group; a thread searches between them and keeps what it knows of its op while the
//                      next candidate lies in the same one.  An indel's candidate sets its flag; a column compares the two bases,
//                      flags an SNV and adds 1 to ONE of 15 counters of its pair: an LDS atomic on the work-group's table slot,
//                      flushed once per (work-group, key, counter).
//   (compaction)       swg_flags_count / swg_flags_compact over the flags: the variants' candidates, ascending.
//   variants_rows      one thread per variant: its op by a search in C[], its entry in op_first[], the six words and the allele
//                      length; skipped words when nobody can take the variants (the lengths are still summed for pool_bytes).
//   (scan)             the allele lengths' exclusive sums: the pool offsets.
//   variants_alleles   one thread per variant: its offset into the variant, its allele bytes into the pool, byte by byte.  An indel
//                      of l bases is l + 2 stores of one thread: max_indel bounds it (DESIGN.md section 34 on what no bound costs).
//   variants_collect   the occupied genome pairs (list_slots); the host orders them by (q_genome, t_genome).
//
// No work-group waits for another inside a launch; integer atomics only; the result does not depend on the grid's shape.
#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "swg_cigar_build.h"
#include "swg_diffs_walk.h"
#include "swg_diffs_letters.h"
#include "swg_variants_walk.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // TB, LdsTable, PairTable, run_end, run_sum, reserve_first
using swg_lift_ix::LiftCols;
using namespace swg_cigar;
using namespace swg_diffs;
using namespace swg_variants;

static_assert(sizeof(swg_variant) == 32 && sizeof(swg_variant_pair) == 200 && sizeof(swg_variant_request) == 144 && sizeof(swg_seq_set) == 24,
              "include/sweepga_gpu.h states these sizes");
static_assert(K_SNP == SWG_VARIANT_SNP && K_INS == SWG_VARIANT_INS && K_DEL == SWG_VARIANT_DEL, "the kind byte holds the ABI's bits");
enum { F_USABLE = C_BUILD_TOTAL, F_BAD_ID, F_NO_SEQ, F_OUT_SEQ, F_BAD_OFFSET, F_VARIANTS, F_LISTED, F_TOTAL };
// the sums of a genome pair as the table holds them: `entries` by variants_entries, the 15 column counters by variants_columns,
// the six indel sums by variants_ops
enum { Q_ENTRY = 1, Q_COL = C_TOTAL, Q_OP = 6, Q_TOTAL = Q_ENTRY + Q_COL + Q_OP };
enum { O_N_INS = 0, O_INS_BASES, O_N_DEL, O_DEL_BASES, O_LONG, O_UNANCHORED };

using SumTable = PairTable<Q_TOTAL, false>;
using SumList = PairList<Q_TOTAL, false>;

struct Seqs {  // device pointers
  const uint64_t* offset;
  const uint8_t* bases;
};

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void variants_letters_kernel(CigarSet S, int aligned, uint8_t* __restrict__ kind) {
  letters_of_chunk(S, aligned, (uint64_t)blockIdx.x * TB + threadIdx.x, kind);
}

__global__ __launch_bounds__(TB) void variants_offsets_kernel(const uint64_t* __restrict__ offset, uint32_t n_seq, unsigned long long* __restrict__ scalars) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (s < n_seq && offset[s + 1] < offset[s]) atomicOr(&scalars[F_BAD_OFFSET], 1ull);
}

// the sums of one run head into the work-group's table, or past it when its probes found no slot
template <int N>
__device__ __forceinline__ void fold_runs(LdsTable<N, false>& l_pairs, const SumTable& T, int offset, unsigned long long key, unsigned long long (&v)[N]) {
  if (!__ballot(key != EMPTY)) return;  // wavefront-uniform
  const int lane = threadIdx.x & 63;
  const unsigned long long before = __shfl_up(key, 1);
  const bool first_lane = lane == 0 || key != before;
  run_sum(v, lane, run_end(__ballot(first_lane), lane));
  if (first_lane && key != EMPTY && !l_pairs.add(key, v)) table_add<N, false>(T, key, v, offset);
}

__global__ __launch_bounds__(TB) void variants_entries_kernel(CigarSet S, LiftCols c, const uint32_t* __restrict__ seq_genome, uint32_t n_seq, uint32_t G,
                                                              uint32_t set, uint32_t want_q, uint32_t want_t, const uint64_t* __restrict__ seq_off,
                                                              SumTable T, unsigned long long* __restrict__ entry_key,
                                                              unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<Q_ENTRY, false> l_pairs;
  l_pairs.clear();
  __syncthreads();
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned long long key = EMPTY, v[Q_ENTRY] = {0};
  bool bad_id = false, no_seq = false, out_seq = false;
  if (j < S.k) {
    const uint32_t rec = S.record[j];
    if (set == SWG_IV_ALL || c.status[rec] != 0) {
      const uint32_t q = c.id[0][rec], t = c.id[1][rec];
      const uint32_t gq = q < n_seq ? seq_genome[q] : G, gt = t < n_seq ? seq_genome[t] : G;
      bad_id = gq >= G || gt >= G;
      if (!bad_id && reinterpret_cast<const uint8_t*>(S.state)[j] == 0 && (want_q == SWG_VARIANTS_ANY || gq == want_q) &&
          (want_t == SWG_VARIANTS_ANY || gt == want_t)) {
        const uint64_t q0 = seq_off[q], q1 = seq_off[q + 1], t0 = seq_off[t], t1 = seq_off[t + 1];
        no_seq = !(q1 > q0 && t1 > t0);
        out_seq = !no_seq && !(c.end[0][rec] <= q1 - q0 && c.end[1][rec] <= t1 - t0);
        if (!no_seq && !out_seq) key = (unsigned long long)gq * G + gt, v[0] = 1;
      }
    }
    entry_key[j] = key;
  }
  const uint64_t usable = __ballot(key != EMPTY), bad = __ballot(bad_id), ns = __ballot(no_seq), os = __ballot(out_seq);
  if ((threadIdx.x & 63) == 0) {
    if (usable) atomicAdd(&scalars[F_USABLE], (unsigned long long)__popcll(usable));
    if (ns) atomicAdd(&scalars[F_NO_SEQ], (unsigned long long)__popcll(ns));
    if (os) atomicAdd(&scalars[F_OUT_SEQ], (unsigned long long)__popcll(os));
    if (bad) atomicOr(&scalars[F_BAD_ID], 1ull);
  }
  fold_runs(l_pairs, T, 0, key, v);
  __syncthreads();
  l_pairs.flush(T, 0);
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
// the last op r in [lo, hi] with C[r] <= s (C[lo] <= s, hi < ops, s < C[ops]): the op that candidate s belongs to -- C[r + 1] > s,
// and the ops in front of it with the same sum have no candidate
__device__ __forceinline__ uint32_t op_at(const uint64_t* __restrict__ C, uint32_t lo, uint32_t hi, uint64_t s) {
  while (lo < hi) {
    const uint32_t mid = lo + ((hi - lo + 1) >> 1);
    if (C[mid] <= s) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}

constexpr int OPS = 4, TILE = TB * OPS;

__global__ __launch_bounds__(TB) void variants_ops_kernel(CigarSet S, LiftCols c, const uint8_t* __restrict__ kind,
                                                          const unsigned long long* __restrict__ entry_key, const uint64_t* __restrict__ seq_off,
                                                          uint32_t max_indel, SumTable T, uint64_t* __restrict__ cand) {
  __shared__ LdsTable<Q_OP, false> l_pairs;
  __shared__ uint32_t l_range[2];
  l_pairs.clear();
  const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;  // (the grid covers the ops: tile0 < S.ops)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + TILE - 1 < S.ops ? tile0 + TILE - 1 : S.ops - 1);
    l_range[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)edge);
  }
  __syncthreads();
  const uint64_t r0 = tile0 + (uint64_t)threadIdx.x * OPS;
  uint32_t kd[OPS];
#pragma unroll
  for (int j = 0; j < OPS; ++j) kd[j] = r0 + j < S.ops ? kind[r0 + j] & (K_SNP | K_M | K_INS | K_DEL) : 0u;
  unsigned long long key = EMPTY, v[Q_OP];
#pragma unroll
  for (int i = 0; i < Q_OP; ++i) v[i] = 0;
  uint64_t n_cand[OPS] = {0, 0, 0, 0};
  if (kd[0] | kd[1] | kd[2] | kd[3]) {
    const uint32_t last = l_range[1];
    uint32_t e = entry_at(S.op_first, l_range[0], last, (uint32_t)r0);
    uint32_t next = e < last ? S.op_first[e + 1] : 0xffffffffu;  // (the tile's ops end inside entry `last`)
    unsigned long long ek = entry_key[e];
#pragma unroll
    for (int j = 0; j < OPS; ++j) {
      const uint64_t r = r0 + j;
      if (next <= r) {
        while (e < last && S.op_first[e + 1] <= r) ++e;
        next = e < last ? S.op_first[e + 1] : 0xffffffffu;
        ek = entry_key[e];
      }
      if (!kd[j] || ek == EMPTY) continue;
      const uint64_t l = op_length(S.P, r, kd[j]);
      if (!l) continue;
      if (kd[j] & (K_SNP | K_M)) {
        n_cand[j] = l;
        continue;
      }
      if (ek != key) {  // (an entry of another genome pair begins inside the thread: rare)
        if (key != EMPTY && !l_pairs.add(key, v)) table_add<Q_OP, false>(T, key, v, Q_ENTRY + Q_COL);
        key = ek;
#pragma unroll
        for (int i = 0; i < Q_OP; ++i) v[i] = 0;
      }
      const bool ins = kd[j] == K_INS;
      int fate = max_indel && l > max_indel ? 2 : 0;
      if (!ins && S.P.Y[r] == S.P.Y[S.op_first[e]]) {  // a deletion at the record's first target base: the only one that can be unanchored
        const uint32_t rec = S.record[e], t = c.id[1][rec];
        fate = indel_fate(K_DEL, l, c.start[1][rec], seq_off[t + 1] - seq_off[t], max_indel);
      }
      v[O_N_INS] += ins, v[O_INS_BASES] += ins ? l : 0;
      v[O_N_DEL] += !ins, v[O_DEL_BASES] += ins ? 0 : l;
      v[O_LONG] += fate == 2, v[O_UNANCHORED] += fate == 1;
      n_cand[j] = fate == 0;
    }
  }
#pragma unroll
  for (int j = 0; j < OPS; ++j)
    if (r0 + j < S.ops) cand[r0 + j + 1] = n_cand[j];  // (cand[0] is the host's 0: the inclusive scan leaves the exclusive sums)
  fold_runs(l_pairs, T, Q_ENTRY + Q_COL, key, v);
  __syncthreads();
  l_pairs.flush(T, Q_ENTRY + Q_COL);
}

// What a thread knows of the op its candidate lies in.
struct OpAt {
  Site site;          // x, p: the op's first column
  const uint8_t *T, *Q;
  uint32_t rec;
};
__device__ __forceinline__ OpAt op_site(const CigarSet& S, const LiftCols& c, const Seqs& seqs, uint32_t kd, uint32_t r, uint32_t e) {
  OpAt o;
  const uint32_t first = S.op_first[e], rec = S.record[e];
  o.rec = rec;
  o.site.kind = kd & K_M ? K_SNP : kd;
  o.site.minus = c.strand[rec] != 0;
  o.site.l = (uint32_t)op_length(S.P, r, kd);
  o.site.x = (uint32_t)(S.P.X[r] - S.P.X[first]);
  o.site.p = (uint64_t)c.start[1][rec] + (S.P.Y[r] - S.P.Y[first]);
  o.site.q_start = c.start[0][rec], o.site.q_end = c.end[0][rec];
  o.T = seqs.bases + seqs.offset[c.id[1][rec]];
  o.Q = seqs.bases + seqs.offset[c.id[0][rec]];
  return o;
}

constexpr int COLS = 4, CTILE = TB * COLS;

__global__ __launch_bounds__(TB) void variants_columns_kernel(CigarSet S, LiftCols c, Seqs seqs, const uint8_t* __restrict__ kind,
                                                              const unsigned long long* __restrict__ entry_key, const uint64_t* __restrict__ C,
                                                              uint64_t total, SumTable T, uint8_t* __restrict__ flags) {
  __shared__ LdsTable<Q_COL, false> l_pairs;
  __shared__ uint32_t l_op[2], l_entry[2];
  l_pairs.clear();
  const uint64_t tile0 = (uint64_t)blockIdx.x * CTILE;  // (the grid covers the candidates: tile0 < total)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + CTILE - 1 < total ? tile0 + CTILE - 1 : total - 1);
    const uint32_t r = op_at(C, 0, (uint32_t)(S.ops - 1), edge);
    l_op[threadIdx.x] = r;
    l_entry[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), r);
  }
  __syncthreads();
  uint32_t r = 0xffffffffu, kd = 0, slot = 0;
  uint64_t c0 = 0, c1 = 0;  // the candidates of op r
  unsigned long long key = EMPTY;
  bool placed = false;
  OpAt o{};
#pragma unroll 1
  for (int j = 0; j < COLS; ++j) {
    const uint64_t s = tile0 + (uint64_t)j * TB + threadIdx.x;
    if (s >= total) break;
    if (r == 0xffffffffu || s >= c1) {
      r = op_at(C, l_op[0], l_op[1], s);
      c0 = C[r], c1 = C[r + 1];
      kd = kind[r];
      if (kd & (K_SNP | K_M)) {
        const uint32_t e = entry_at(S.op_first, l_entry[0], l_entry[1], r);
        o = op_site(S, c, seqs, kd, r, e);
        const unsigned long long ek = entry_key[e];  // (not EMPTY: the op has candidates)
        if (ek != key || !placed) {
          key = ek;
          uint32_t h = hash32(key) & (LSLOTS - 1);
          placed = false;
          for (int p = 0; p < LPROBES && !placed; ++p, h = (h + 1) & (LSLOTS - 1)) {
            unsigned long long at = l_pairs.key[h];
            if (at == EMPTY) {
              at = atomicCAS(&l_pairs.key[h], EMPTY, key);
              if (at == EMPTY) at = key;
            }
            if (at == key) slot = h, placed = true;
          }
        }
      }
    }
    if (!(kd & (K_SNP | K_M))) {  // an indel that gives a variant
      flags[s] = 1;
      continue;
    }
    const uint64_t b = s - c0;
    const int idx = column_counter(code_of(o.T[o.site.p + b]), query_column(o.site, o.Q, (uint64_t)o.site.x + b), (kd & K_M) != 0);
    flags[s] = idx < C_SAME;
    if (placed) {
      atomicAdd(&l_pairs.sum[slot][idx], 1ull);
    } else {  // more pairs in this tile than the table takes
      const unsigned long long one = 1;
      table_add<1, false>(T, key, &one, Q_ENTRY + idx);
    }
  }
  __syncthreads();
  l_pairs.flush(T, Q_ENTRY);
}

// the site of variant i's candidate: an SNV's is its own column
__device__ __forceinline__ OpAt variant_site(const CigarSet& S, const LiftCols& c, const Seqs& seqs, const uint8_t* __restrict__ kind,
                                             const uint64_t* __restrict__ C, uint32_t s) {
  const uint32_t r = op_at(C, 0, (uint32_t)(S.ops - 1), s);
  const uint32_t e = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), r);
  const uint32_t kd = kind[r];
  OpAt o = op_site(S, c, seqs, kd, r, e);
  if (kd & (K_SNP | K_M)) {
    const uint32_t b = (uint32_t)(s - C[r]);
    o.site.x += b, o.site.p += b, o.site.l = 1;
  }
  return o;
}

__global__ __launch_bounds__(TB) void variants_rows_kernel(uint64_t n, const uint32_t* __restrict__ list, CigarSet S, LiftCols c, Seqs seqs,
                                                           const uint8_t* __restrict__ kind, const uint64_t* __restrict__ C,
                                                           swg_variant* __restrict__ variants, uint64_t* __restrict__ len) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const OpAt o = variant_site(S, c, seqs, kind, C, list[i]);
  len[i + 1] = allele_bytes(o.site);  // (len[0] is the host's 0)
  if (!variants) return;
  uint32_t w[4];
  variant_words(o.site, w);
  uint4* out = reinterpret_cast<uint4*>(variants + i);  // 32 bytes: two 16-byte stores (arena blocks are 16-byte aligned)
  out[0] = make_uint4(o.rec, o.site.kind | (o.site.minus ? SWG_VARIANT_MINUS : 0u), w[0], w[1]);
  out[1] = make_uint4(w[2], w[3], 0u, 0u);  // (the offset is variants_alleles')
}

__global__ __launch_bounds__(TB) void variants_alleles_kernel(uint64_t n, const uint32_t* __restrict__ list, CigarSet S, LiftCols c, Seqs seqs,
                                                              const uint8_t* __restrict__ kind, const uint64_t* __restrict__ C,
                                                              const uint64_t* __restrict__ len, swg_variant* __restrict__ variants,
                                                              uint8_t* __restrict__ pool) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n) return;
  const OpAt o = variant_site(S, c, seqs, kind, C, list[i]);
  const uint64_t at = len[i], bytes = len[i + 1] - at;  // (bytes = allele_bytes of the site; at + bytes <= len[n], the pool's size)
  variants[i].allele_offset = at;
  for (uint64_t k = 0; k < bytes; ++k) pool[at + k] = allele_byte(o.site, o.T, o.Q, k);
}

__global__ __launch_bounds__(TB) void variants_collect_kernel(SumTable T, SumList L) { list_slots(T, L); }

bool variants_hash_forced() {  // test knob: the hashed genome-pair table at any size
  const char* knob = std::getenv("SWG_VARIANTS_HASH");
  return knob && knob[0] == '1';
}

// where: 0 = everything on the host, 1 = everything on the device, 2 = the host's, but seqs->bases in device memory (the PAF seam
// uploads the bases once per call, not once per batch).  entry_usable: host [k] or NULL, 1 for a usable entry.
int variants_run(swg_ctx* ctx, const swg_records* rec, int where, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                 const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req, uint8_t* entry_usable) {
  const bool on_device = where == 1;
  static const char* const who = "variant_records";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: reserved must be 0", who);
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (!seq_genome) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL seq_genome", who);
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq, G = n_genome;
  for (const uint32_t g : {req->t_genome, req->q_genome})
    if (g != SWG_VARIANTS_ANY && g >= G) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a genome filter >= n_genome that is not SWG_VARIANTS_ANY", who);
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  if (B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
  if (k && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column", who);
  if (k && G == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: entries without genomes (n_genome is 0)", who);
  if (k && (!seqs || !seqs->offset || !seqs->bases)) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL sequences, offsets or bases", who);
  if (k && (seqs->n_seq != n_seq || seqs->reserved != 0))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence set must have rec->n_seq sequences and reserved 0", who);
  uint64_t n_bases = 0;
  if (k && !on_device) {
    for (uint32_t s = 0; s < n_seq; ++s)
      if (seqs->offset[s + 1] < seqs->offset[s]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence offsets descend at sequence %u", who, s);
    n_bases = seqs->offset[n_seq];
  }
  req->n_variants = req->pool_bytes = req->n_pairs = req->ops = req->cigar_bad = req->usable = req->no_sequence = req->out_of_sequence = req->columns = 0;
  if (!k) return SWG_OK;  // no device work
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 12 + (where == 0 ? n_bases : 0)) + (size_t)B * 24 + (size_t)k * 32 + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const uint32_t* d_genome = seq_genome;  // (the frame may run twice: what the stager replaces is the frame's own)
    Seqs Q{seqs->offset, seqs->bases};
    CigarSet S{};
    S.k = k, S.B = B;
    S.record = cigars->record, S.offset = cigars->offset, S.text = cigars->text;
    if (!on_device) {
      swg_stager s(ctx);
      for (int a = 0; a < 2; ++a) s.add(&c.id[a], n), s.add(&c.start[a], n), s.add(&c.end[a], n);
      s.add(&c.strand, n);
      s.add(&c.status, n);
      s.add(&d_genome, (size_t)n_seq);
      s.add(&S.record, k);
      s.add(&S.offset, k + 1);
      s.add(&S.text, B);
      s.add(&Q.offset, (size_t)n_seq + 1);
      if (where == 0) s.add(&Q.bases, n_bases);
      SWG_TRY(s.run());
    }
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, F_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, F_TOTAL * sizeof(unsigned long long), st));
    if (on_device) {
      SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
      if (S.B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
      if (n_seq) {  // before anything reads a base through the offsets
        SWG_LAUNCH(ctx, "variants_offsets", variants_offsets_kernel<<<grid_of(n_seq), TB, 0, st>>>(Q.offset, n_seq, scalars));
        SWG_KERNEL_CHECK(ctx);
        uint64_t bad_offset = 0;
        SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + F_BAD_OFFSET, &bad_offset, 1));
        if (bad_offset) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the sequence offsets descend", who);
      }
    }
    SWG_TRY(cigar_build(ctx, who, c, &S, scalars));
    const uint64_t ops = S.ops;
    uint8_t* kind = swg_alloc<uint8_t>(ctx, ops + 1);
    uint64_t* C = swg_alloc<uint64_t>(ctx, ops + 1);
    unsigned long long* entry_key = swg_alloc<unsigned long long>(ctx, k);
    SumTable T{};
    SumList L{};
    const uint64_t g2 = (uint64_t)G * G, pairs_max = g2 < k ? g2 : k;  // genome pairs that occur <= entries
    SWG_TRY(table_create(ctx, G, pairs_max, variants_hash_forced() || (g2 > 4096 && g2 > 2 * pairs_max), false, scalars + F_LISTED, &T, &L));
    if (S.B) {
      const int aligned = (reinterpret_cast<uintptr_t>(S.text) & 15) == 0;
      SWG_LAUNCH(ctx, "variants_letters", variants_letters_kernel<<<grid_of((S.B + 15) / 16), TB, 0, st>>>(S, aligned, kind));
      SWG_KERNEL_CHECK(ctx);
    }
    SWG_LAUNCH(ctx, "variants_entries",
               variants_entries_kernel<<<grid_of(k), TB, 0, st>>>(S, c, d_genome, n_seq, G, req->set, req->q_genome, req->t_genome, Q.offset, T, entry_key, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t total = 0;
    if (ops) {
      SWG_HIP(ctx, hipMemsetAsync(C, 0, sizeof(uint64_t), st));
      SWG_LAUNCH(ctx, "variants_ops",
                 variants_ops_kernel<<<(unsigned)((ops + TILE - 1) / TILE), TB, 0, st>>>(S, c, kind, entry_key, Q.offset, req->max_indel, T, C));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_inclusive_sum_scan_u64(ctx, C, C, ops + 1));
      SWG_TRY(swg_read_scalars(ctx, C + ops, &total, 1));
    }
    uint64_t h[F_TOTAL];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, F_TOTAL));
    if (h[F_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the set has a sequence id >= n_seq or a genome id >= n_genome", who);
    if (total >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 candidate columns or more in one call", who);
    uint64_t n_variants = 0, pool_bytes = 0;
    if (total) {
      uint8_t* flags = swg_alloc<uint8_t>(ctx, total + 1);
      SWG_CHECK_ARENA(ctx);
      SWG_LAUNCH(ctx, "variants_columns",
                 variants_columns_kernel<<<(unsigned)((total + CTILE - 1) / CTILE), TB, 0, st>>>(S, c, Q, kind, entry_key, C, total, T, flags));
      SWG_KERNEL_CHECK(ctx);
      swg_flag_scan fs{};
      SWG_TRY(swg_flags_count(ctx, flags, total, &fs, reinterpret_cast<uint64_t*>(scalars) + F_VARIANTS));
      SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + F_VARIANTS, &n_variants, 1));
      if (n_variants >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 variants or more in one call", who);
      if (n_variants) {
        const bool taken = req->variants && req->pool && n_variants <= req->variant_capacity;
        uint32_t* list = swg_alloc<uint32_t>(ctx, n_variants);
        uint64_t* len = swg_alloc<uint64_t>(ctx, n_variants + 1);
        swg_variant* variants = taken ? swg_alloc<swg_variant>(ctx, n_variants) : nullptr;
        SWG_CHECK_ARENA(ctx);
        SWG_TRY(swg_flags_compact(ctx, fs, list));
        SWG_HIP(ctx, hipMemsetAsync(len, 0, sizeof(uint64_t), st));
        SWG_LAUNCH(ctx, "variants_rows", variants_rows_kernel<<<grid_of(n_variants), TB, 0, st>>>(n_variants, list, S, c, Q, kind, C, variants, len));
        SWG_KERNEL_CHECK(ctx);
        SWG_TRY(swg_inclusive_sum_scan_u64(ctx, len, len, n_variants + 1));
        SWG_TRY(swg_read_scalars(ctx, len + n_variants, &pool_bytes, 1));
        if (pool_bytes >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 allele bytes or more in one call", who);
        if (taken && pool_bytes <= req->pool_capacity) {  // (else nobody takes them: counted and not built)
          uint8_t* pool = swg_alloc<uint8_t>(ctx, pool_bytes);
          SWG_CHECK_ARENA(ctx);
          SWG_LAUNCH(ctx, "variants_alleles",
                     variants_alleles_kernel<<<grid_of(n_variants), TB, 0, st>>>(n_variants, list, S, c, Q, kind, C, len, variants, pool));
          SWG_KERNEL_CHECK(ctx);
          SWG_HIP(ctx, hipMemcpyAsync(req->variants, variants, n_variants * sizeof(swg_variant), hipMemcpyDeviceToHost, st));
          SWG_HIP(ctx, hipMemcpyAsync(req->pool, pool, pool_bytes, hipMemcpyDeviceToHost, st));
        }
      }
    }
    SWG_LAUNCH(ctx, "variants_collect", variants_collect_kernel<<<grid_of(T.slots), TB, 0, st>>>(T, L));
    SWG_KERNEL_CHECK(ctx);
    uint64_t listed = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + F_LISTED), &listed, 1));
    std::vector<SumList::Entry> list[1];
    SWG_TRY(list_fetch(ctx, who, L, &listed, list));  // (synchronises: the copies above are done)
    std::sort(list[0].begin(), list[0].end(), [](const SumList::Entry& a, const SumList::Entry& b) { return a.key < b.key; });
    uint64_t columns = 0;
    const bool fits = req->pairs && list[0].size() <= req->pair_capacity;
    for (size_t x = 0; x < list[0].size(); ++x) {
      const SumList::Entry& e = list[0][x];
      swg_variant_pair o{};
      o.q_genome = (uint32_t)(e.key / G), o.t_genome = (uint32_t)(e.key % G);
      o.entries = e.v[0];
      for (int i = 0; i < 12; ++i) o.sub[i] = e.v[Q_ENTRY + i], o.snvs += e.v[Q_ENTRY + i];
      o.same = e.v[Q_ENTRY + C_SAME], o.m_equal = e.v[Q_ENTRY + C_M_EQUAL], o.n_columns = e.v[Q_ENTRY + C_N];
      o.compared = o.snvs + o.same + o.m_equal + o.n_columns;
      std::memcpy(&o.n_ins, e.v + Q_ENTRY + Q_COL, Q_OP * sizeof(uint64_t));  // (the six indel sums in the structure's order)
      columns += o.compared;
      if (fits) req->pairs[x] = o;
    }
    if (entry_usable) {
      std::vector<unsigned long long> keys(k);
      SWG_HIP(ctx, hipMemcpyAsync(keys.data(), entry_key, k * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
      for (uint64_t j = 0; j < k; ++j) entry_usable[j] = keys[j] != EMPTY;
    }
    uint64_t bad = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + C_BAD_ENTRIES, &bad, 1));
    req->n_variants = n_variants, req->pool_bytes = pool_bytes, req->n_pairs = list[0].size(), req->ops = ops, req->cigar_bad = bad;
    req->usable = h[F_USABLE], req->no_sequence = h[F_NO_SEQ], req->out_of_sequence = h[F_OUT_SEQ], req->columns = columns;
    return SWG_OK;
  });
}

}  // namespace

int swg_variant_run(swg_ctx* ctx, const swg_records* rec, int where, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                    const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req, uint8_t* entry_usable) {
  try {
    return variants_run(ctx, rec, where, seq_genome, n_genome, status, cigars, seqs, req, entry_usable);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

// The bases of the sequences a PAF call names, end to end in one device block of its own (not the arena's: it lives across the
// batches): piece s is src[s] of len[s] bytes (NULL: absent); offset[n_seq + 1] receives where each lies.
int swg_variant_bases_upload(swg_ctx* ctx, const uint8_t* const* src, const uint64_t* len, uint32_t n_seq, uint64_t* offset, uint8_t** d_bases) {
  *d_bases = nullptr;
  offset[0] = 0;
  for (uint32_t s = 0; s < n_seq; ++s) offset[s + 1] = offset[s] + (src[s] ? len[s] : 0);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  void* block = nullptr;
  const hipError_t e = hipMalloc(&block, offset[n_seq] ? offset[n_seq] : 16);
  if (e != hipSuccess)
    return swg_set_error(ctx, e == hipErrorOutOfMemory ? SWG_ERR_OOM : SWG_ERR_HIP, "the sequences: hipMalloc of %llu bytes failed: %s",
                         (unsigned long long)offset[n_seq], hipGetErrorString(e));
  *d_bases = static_cast<uint8_t*>(block);
  for (uint32_t s = 0; s < n_seq; ++s) {
    if (offset[s + 1] == offset[s]) continue;
    const hipError_t c = hipMemcpyAsync(*d_bases + offset[s], src[s], len[s], hipMemcpyHostToDevice, ctx->stream);
    if (c != hipSuccess) {
      (void)hipStreamSynchronize(ctx->stream);
      (void)hipFree(block);
      *d_bases = nullptr;
      return swg_set_error(ctx, SWG_ERR_HIP, "the sequences: copy failed: %s", hipGetErrorString(c));
    }
  }
  SWG_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return SWG_OK;
}
void swg_variant_bases_free(swg_ctx* ctx, uint8_t* d_bases) {
  if (!d_bases) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->stream);
  (void)hipFree(d_bases);
}

// order[i] = the index of the i-th variant by key, ties in index order: one stable device sort over the key's low `bits` bits
int swg_variant_order(swg_ctx* ctx, const uint64_t* keys, uint64_t n, int bits, uint32_t* order) {
  if (!n) return SWG_OK;
  if (n >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "2^32 variants or more to order");
  try {
    SWG_HIP(ctx, hipSetDevice(ctx->device));
    SWG_TRY(swg_pair_table::reserve_first(ctx, (size_t)n * 24 + (size_t(4) << 20)));
    for (uint64_t i = 0; i < n; ++i) order[i] = (uint32_t)i;  // (the identity goes up through the caller's own array)
    return swg_run_with_arena(ctx, [&]() -> int {
      hipStream_t st = ctx->stream;
      uint64_t *k0 = swg_alloc<uint64_t>(ctx, n), *k1 = swg_alloc<uint64_t>(ctx, n);
      uint32_t *v0 = swg_alloc<uint32_t>(ctx, n), *v1 = swg_alloc<uint32_t>(ctx, n);
      SWG_CHECK_ARENA(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(k0, keys, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
      SWG_HIP(ctx, hipMemcpyAsync(v0, order, n * sizeof(uint32_t), hipMemcpyHostToDevice, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));  // (order is read before it is written)
      SWG_TRY(swg_radix_sort_pairs(ctx, &k0, &v0, &k1, &v1, n, 0, bits));
      SWG_HIP(ctx, hipMemcpyAsync(order, v0, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
      SWG_HIP(ctx, hipStreamSynchronize(st));
      return SWG_OK;
    });
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_variant_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                   const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req) {
  return swg_variant_run(ctx, rec, 0, seq_genome, n_genome, status, cigars, seqs, req, nullptr);
}
extern "C" int swg_variant_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                          const swg_cigar_set* cigars, const swg_seq_set* seqs, swg_variant_request* req) {
  return swg_variant_run(ctx, rec, 1, seq_genome, n_genome, status, cigars, seqs, req, nullptr);
}
