// Differences: every mismatch run, insertion and deletion inside the mappings, from their CIGARs -- one
// 32-byte row per X, I, D or N op, sums per genome pair and a length spectrum.  The parse, the four prefix sums, op_first[] and the
// entry states are cigar_build's (swg_cigar.hip, swg_cigar_build.h); include/sweepga_gpu.h states the definitions, swg_diffs_walk.h
// holds the rules.
//
//   diffs_letters  one thread per 16-byte chunk of the text: from chunk_rank[chunk] on, a kind byte at the rank of every byte that is
//                  no digit (the prefix sums cannot tell M from X, or D from N).  Every byte has one writer.  The body is
//                  swg_diffs_letters.h's, which the divergence track (swg_divergence.hip) calls too.
//   diffs_entries  one thread per entry: usable or not (state 0, record in the set), the ids checked, the entry's genome pair into
//                  entry_key[] (EMPTY: not usable), and its entries / aligned / eq into the genome-pair table.
//   diffs_ops      a tile of 1,024 ops per work-group, 4 consecutive ones per thread: the tile's first and last op are searched in
//                  op_first[] once, a thread with a letter of interest then searches between the two (a handful of entries) for its
//                  first op and steps from there.  Kind, length from the prefix differences, the nine sums of its kind, the
//                  spectrum bin, the row flag.  Sums: runs of one genome pair along the wavefront are folded first, then the
//                  work-group's LDS table, then one atomic per (work-group, key, quantity) (swg_pair_table.h).  The spectrum goes
//                  through an LDS histogram per work-group, flushed once.
//   (compaction)   swg_flags_count / swg_flags_compact over the row flags: the rows' ops, ascending = (entry, op) order; the count is
//                  read back.
//   diffs_rows     one thread per row: its entry by a search in op_first[], the record's columns, X, Y and E gathered, the row
//                  written as two 16-byte stores.  Not launched when nobody can take the rows.
//   diffs_collect  the occupied genome pairs (list_slots); the host orders them by (q_genome, t_genome).
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
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;  // TB, LdsTable, PairTable, run_end, run_sum, reserve_first
using swg_lift_ix::LiftCols;
using namespace swg_cigar;
using namespace swg_diffs;

constexpr int BINS = SWG_DIFF_BINS;
static_assert(sizeof(swg_diff_row) == 32 && sizeof(swg_diff_pair) == 104 && sizeof(swg_diff_request) == 104 && sizeof(swg_diff_counts) == 120,
              "include/sweepga_gpu.h states these sizes");
static_assert(K_SNP == SWG_DIFF_SNP && K_INS == SWG_DIFF_INS && K_DEL == SWG_DIFF_DEL && K_SKIP == SWG_DIFF_SKIP, "the kind byte holds the ABI's bits");
enum { F_USABLE = C_BUILD_TOTAL, F_BAD_ID, F_ROWS, F_LISTED, F_SPECTRUM, F_TOTAL = F_SPECTRUM + 4 * BINS };
// the sums of a genome pair, in the order of swg_diff_pair: the first Q_ENTRY by diffs_entries, the other Q_OP by diffs_ops
enum { Q_ENTRY = 3, Q_OP = 9, Q_TOTAL = Q_ENTRY + Q_OP };
enum { O_M = 0, O_SNP_RUNS, O_SNP_BASES, O_N_INS, O_INS_BASES, O_N_DEL, O_DEL_BASES, O_N_SKIP, O_SKIP_BASES };

using SumTable = PairTable<Q_TOTAL, false>;
using SumList = PairList<Q_TOTAL, false>;

unsigned grid_of(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

__global__ __launch_bounds__(TB) void diffs_letters_kernel(CigarSet S, int aligned, uint8_t* __restrict__ kind) {
  letters_of_chunk(S, aligned, (uint64_t)blockIdx.x * TB + threadIdx.x, kind);
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

__global__ __launch_bounds__(TB) void diffs_entries_kernel(CigarSet S, LiftCols c, const uint32_t* __restrict__ seq_genome, uint32_t n_seq, uint32_t G,
                                                           uint32_t set, SumTable T, unsigned long long* __restrict__ entry_key,
                                                           unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<Q_ENTRY, false> l_pairs;
  l_pairs.clear();
  __syncthreads();
  const uint64_t j = (uint64_t)blockIdx.x * TB + threadIdx.x;
  unsigned long long key = EMPTY, v[Q_ENTRY] = {0, 0, 0};
  bool bad_id = false;
  if (j < S.k) {
    const uint32_t rec = S.record[j];
    if (set == SWG_IV_ALL || c.status[rec] != 0) {
      const uint32_t q = c.id[0][rec], t = c.id[1][rec];
      const uint32_t gq = q < n_seq ? seq_genome[q] : G, gt = t < n_seq ? seq_genome[t] : G;
      bad_id = gq >= G || gt >= G;
      if (!bad_id && reinterpret_cast<const uint8_t*>(S.state)[j] == 0) {
        const uint32_t first = S.op_first[j], e = S.op_first[j + 1];
        key = (unsigned long long)gq * G + gt;
        v[0] = 1, v[1] = S.P.A[e] - S.P.A[first], v[2] = S.P.E[e] - S.P.E[first];
      }
    }
    entry_key[j] = key;
  }
  const uint64_t usable = __ballot(key != EMPTY), bad = __ballot(bad_id);
  if ((threadIdx.x & 63) == 0) {
    if (usable) atomicAdd(&scalars[F_USABLE], (unsigned long long)__popcll(usable));
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

// OPS consecutive ops per thread, TILE per work-group: the LDS table's clear and flush and the fold along the lanes are paid once
// per TILE ops
constexpr int OPS = 4, TILE = TB * OPS;

__global__ __launch_bounds__(TB) void diffs_ops_kernel(CigarSet S, const uint8_t* __restrict__ kind, const unsigned long long* __restrict__ entry_key,
                                                       uint32_t kinds, uint32_t min_indel, SumTable T, uint8_t* __restrict__ flags,
                                                       unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<Q_OP, false> l_pairs;
  __shared__ uint32_t l_spec[4 * BINS];
  __shared__ uint32_t l_range[2];
  l_pairs.clear();
  if (threadIdx.x < 4 * BINS) l_spec[threadIdx.x] = 0;
  const uint64_t tile0 = (uint64_t)blockIdx.x * TILE;  // (the grid covers the ops: tile0 < S.ops)
  if (threadIdx.x < 2) {
    const uint64_t edge = threadIdx.x == 0 ? tile0 : (tile0 + TILE - 1 < S.ops ? tile0 + TILE - 1 : S.ops - 1);
    l_range[threadIdx.x] = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), (uint32_t)edge);
  }
  __syncthreads();
  const uint64_t r0 = tile0 + (uint64_t)threadIdx.x * OPS;
  uint32_t kd[OPS];
  if (r0 + OPS <= S.ops) {  // (arena blocks are 16-byte aligned and r0 is a multiple of 4)
    const uchar4 w = *reinterpret_cast<const uchar4*>(kind + r0);
    kd[0] = w.x, kd[1] = w.y, kd[2] = w.z, kd[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < OPS; ++j) kd[j] = r0 + j < S.ops ? kind[r0 + j] : 0u;
  }
  unsigned long long key = EMPTY, v[Q_OP];
#pragma unroll
  for (int i = 0; i < Q_OP; ++i) v[i] = 0;
  uint32_t row[OPS] = {0, 0, 0, 0};
  if (kd[0] | kd[1] | kd[2] | kd[3]) {
    // the entry of the thread's first op by a search between the tile's two ends, the later ones by stepping: entries that begin
    // at or in front of op r and are not the last such are empty or lie in front of it
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
      if (ek != key) {  // (an entry of another genome pair begins inside the thread: rare)
        if (key != EMPTY && !l_pairs.add(key, v)) table_add<Q_OP, false>(T, key, v, Q_ENTRY);
        key = ek;
#pragma unroll
        for (int i = 0; i < Q_OP; ++i) v[i] = 0;
      }
      const bool m = kd[j] == K_M, snp = kd[j] == K_SNP, ins = kd[j] == K_INS, del = kd[j] == K_DEL, skip = kd[j] == K_SKIP;  // (constant indices below)
      v[O_M] += m ? l : 0;
      v[O_SNP_RUNS] += snp, v[O_SNP_BASES] += snp ? l : 0;
      v[O_N_INS] += ins, v[O_INS_BASES] += ins ? l : 0;
      v[O_N_DEL] += del, v[O_DEL_BASES] += del ? l : 0;
      v[O_N_SKIP] += skip, v[O_SKIP_BASES] += skip ? l : 0;
      if (!m) atomicAdd(&l_spec[kind_index(kd[j]) * BINS + length_bin(l)], 1u);
      row[j] = is_row(kd[j], l, kinds, min_indel) ? 1u : 0u;
    }
  }
  if (r0 + OPS <= S.ops) {
    *reinterpret_cast<uchar4*>(flags + r0) = make_uchar4((uint8_t)row[0], (uint8_t)row[1], (uint8_t)row[2], (uint8_t)row[3]);
  } else {
#pragma unroll
    for (int j = 0; j < OPS; ++j)
      if (r0 + j < S.ops) flags[r0 + j] = (uint8_t)row[j];
  }
  fold_runs(l_pairs, T, Q_ENTRY, key, v);
  __syncthreads();
  l_pairs.flush(T, Q_ENTRY);
  if (threadIdx.x < 4 * BINS && l_spec[threadIdx.x]) atomicAdd(&scalars[F_SPECTRUM + threadIdx.x], (unsigned long long)l_spec[threadIdx.x]);
}

__global__ __launch_bounds__(TB) void diffs_rows_kernel(uint64_t n_rows, const uint32_t* __restrict__ list, CigarSet S, LiftCols c,
                                                        const uint8_t* __restrict__ kind, swg_diff_row* __restrict__ rows) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_rows) return;
  const uint32_t r = list[i];  // (positions of set row flags: < ops)
  const uint32_t j = entry_at(S.op_first, 0, (uint32_t)(S.k - 1), r);
  const uint32_t rec = S.record[j];
  uint32_t w[8];
  row_of(S.P, S.op_first[j], S.op_first[j + 1], r, kind[r], rec, c.strand[rec] != 0, c.start[0][rec], c.end[0][rec], c.start[1][rec], w);
  uint4* o = reinterpret_cast<uint4*>(rows + i);  // 32 bytes: two 16-byte stores (arena blocks are 16-byte aligned)
  o[0] = make_uint4(w[0], w[1], w[2], w[3]);
  o[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__global__ __launch_bounds__(TB) void diffs_collect_kernel(SumTable T, SumList L) { list_slots(T, L); }

bool diffs_hash_forced() {  // test knob: the hashed genome-pair table at any size
  const char* knob = std::getenv("SWG_DIFFS_HASH");
  return knob && knob[0] == '1';
}

int diffs_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
              const swg_cigar_set* cigars, swg_diff_request* req) {
  static const char* const who = "diff_records";
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL records or request", who);
  if (req->set > 1) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: set must be SWG_IV_ALL or SWG_IV_KEPT", who);
  if (req->kinds == 0 || req->kinds > 15) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: kinds names nothing, or a bit beyond the four", who);
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: reserved must be 0", who);
  if (req->set == SWG_IV_KEPT && !status) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: the kept set needs a status column", who);
  if (!seq_genome) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL seq_genome", who);
  const uint64_t n = rec->n, k = cigars ? cigars->k : 0;
  const uint32_t n_seq = rec->n_seq, G = n_genome;
  uint64_t B = 0;
  SWG_TRY(cigar_set_check_host(ctx, who, cigars, on_device, n, &B));
  if (B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
  if (k && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand))
    return swg_set_error(ctx, SWG_ERR_INVALID, "%s: NULL column", who);
  if (k && G == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: entries without genomes (n_genome is 0)", who);
  req->n_rows = req->n_pairs = req->ops = req->cigar_bad = req->usable = 0;
  if (req->spectrum) std::memset(req->spectrum, 0, 4 * BINS * sizeof(uint64_t));
  if (!k) return SWG_OK;  // no device work
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)(on_device ? 0 : n * 26 + (size_t)n_seq * 4) + (size_t)B * 24 + (size_t)k * 32 + (size_t(4) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    hipStream_t st = ctx->stream;
    LiftCols c{{rec->q_id, rec->t_id}, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, rec->strand, status};
    const uint32_t* d_genome = seq_genome;  // (the frame may run twice: what the stager replaces is the frame's own)
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
      SWG_TRY(s.run());
    }
    unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, F_TOTAL);
    SWG_CHECK_ARENA(ctx);
    SWG_HIP(ctx, hipMemsetAsync(scalars, 0, F_TOTAL * sizeof(unsigned long long), st));
    if (on_device) {
      SWG_TRY(cigar_set_check_device(ctx, who, n, &S, scalars));
      if (S.B >> 32) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^32 bytes of CIGAR text or more in one call", who);
    }
    SWG_TRY(cigar_build(ctx, who, c, &S, scalars));
    const uint64_t ops = S.ops;
    uint8_t* kind = swg_alloc<uint8_t>(ctx, ops + 1);
    uint8_t* flags = swg_alloc<uint8_t>(ctx, ops + 1);
    unsigned long long* entry_key = swg_alloc<unsigned long long>(ctx, k);
    SumTable T{};
    SumList L{};
    const uint64_t g2 = (uint64_t)G * G, pairs_max = g2 < k ? g2 : k;  // genome pairs that occur <= entries
    // (a dense table of G x G rows of 96 bytes is cleared per call: beyond a few thousand slots only while the entries can fill it)
    SWG_TRY(table_create(ctx, G, pairs_max, diffs_hash_forced() || (g2 > 4096 && g2 > 2 * pairs_max), false, scalars + F_LISTED, &T, &L));
    if (S.B) {
      const int aligned = (reinterpret_cast<uintptr_t>(S.text) & 15) == 0;
      SWG_LAUNCH(ctx, "diffs_letters", diffs_letters_kernel<<<grid_of((S.B + 15) / 16), TB, 0, st>>>(S, aligned, kind));
      SWG_KERNEL_CHECK(ctx);
    }
    SWG_LAUNCH(ctx, "diffs_entries", diffs_entries_kernel<<<grid_of(k), TB, 0, st>>>(S, c, d_genome, n_seq, G, req->set, T, entry_key, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t n_rows = 0;
    swg_flag_scan fs{};
    if (ops) {
      SWG_LAUNCH(ctx, "diffs_ops", diffs_ops_kernel<<<(unsigned)((ops + TILE - 1) / TILE), TB, 0, st>>>(S, kind, entry_key, req->kinds, req->min_indel, T, flags, scalars));
      SWG_KERNEL_CHECK(ctx);
      SWG_TRY(swg_flags_count(ctx, flags, ops, &fs, reinterpret_cast<uint64_t*>(scalars) + F_ROWS));
    }
    uint64_t h[F_SPECTRUM];
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, F_SPECTRUM));
    if (h[F_BAD_ID]) return swg_set_error(ctx, SWG_ERR_INVALID, "%s: a record of the set has a sequence id >= n_seq or a genome id >= n_genome", who);
    n_rows = h[F_ROWS];
    if (n_rows >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "%s: 2^31 rows or more in one call", who);
    if (n_rows && req->rows && n_rows <= req->row_capacity) {  // (else nobody takes the rows: they are counted and not built)
      uint32_t* list = swg_alloc<uint32_t>(ctx, n_rows);
      swg_diff_row* rows = swg_alloc<swg_diff_row>(ctx, n_rows);
      SWG_CHECK_ARENA(ctx);
      SWG_TRY(swg_flags_compact(ctx, fs, list));
      SWG_LAUNCH(ctx, "diffs_rows", diffs_rows_kernel<<<grid_of(n_rows), TB, 0, st>>>(n_rows, list, S, c, kind, rows));
      SWG_KERNEL_CHECK(ctx);
      SWG_HIP(ctx, hipMemcpyAsync(req->rows, rows, n_rows * sizeof(swg_diff_row), hipMemcpyDeviceToHost, st));
    }
    SWG_LAUNCH(ctx, "diffs_collect", diffs_collect_kernel<<<grid_of(T.slots), TB, 0, st>>>(T, L));
    SWG_KERNEL_CHECK(ctx);
    uint64_t listed = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars + F_LISTED), &listed, 1));
    std::vector<SumList::Entry> list[1];
    SWG_TRY(list_fetch(ctx, who, L, &listed, list));
    std::sort(list[0].begin(), list[0].end(), [](const SumList::Entry& a, const SumList::Entry& b) { return a.key < b.key; });
    if (req->pairs && list[0].size() <= req->pair_capacity) {
      for (size_t x = 0; x < list[0].size(); ++x) {
        const SumList::Entry& e = list[0][x];
        swg_diff_pair& o = req->pairs[x];
        o.q_genome = (uint32_t)(e.key / G), o.t_genome = (uint32_t)(e.key % G);
        std::memcpy(&o.entries, e.v, Q_TOTAL * sizeof(uint64_t));  // (the sums in the structure's order)
      }
    }
    if (req->spectrum) SWG_HIP(ctx, hipMemcpyAsync(req->spectrum, scalars + F_SPECTRUM, 4 * BINS * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    if (req->state) SWG_HIP(ctx, hipMemcpyAsync(req->state, S.state, k, hipMemcpyDeviceToHost, st));
    uint64_t bad = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + C_BAD_ENTRIES, &bad, 1));  // (and the copies above are done)
    req->n_rows = n_rows, req->n_pairs = list[0].size(), req->ops = ops, req->cigar_bad = bad, req->usable = h[F_USABLE];
    return SWG_OK;
  });
}

}  // namespace

int swg_diff_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                 const swg_cigar_set* cigars, swg_diff_request* req) {
  try {
    return diffs_run(ctx, rec, on_device, seq_genome, n_genome, status, cigars, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

extern "C" int swg_diff_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                const swg_cigar_set* cigars, swg_diff_request* req) {
  return swg_diff_run(ctx, rec, false, seq_genome, n_genome, status, cigars, req);
}
extern "C" int swg_diff_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_genome, uint32_t n_genome, const uint8_t* status,
                                       const swg_cigar_set* cigars, swg_diff_request* req) {
  return swg_diff_run(ctx, rec, true, seq_genome, n_genome, status, cigars, req);
}
