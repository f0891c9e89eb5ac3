// Components: which sequences belong together under the mappings a filter call kept.  A link is an
// unordered sequence pair {a, b}, a < b, that a kept record with q_id != t_id names; it carries the summed bases of either end,
// its records and its first record.  A link JOINS its ends when it is heavy enough (swg_component_params); the components are
// the connected sets over the joined links, numbered by their smallest member.  include/sweepga_gpu.h has the definition.
//
//   components_count    the runs of one pair in input order (a record that takes part and whose predecessor names another
//                       pair, or none): with n_seq (n_seq - 1) / 2 the bound on the pairs that occur, which sizes the table.
//                       Also the check of every id.  One read-back.
//   components_links    one pass over the records in input order, a contiguous share per work-group, four consecutive records per
//                       thread (16-byte loads).  A thread folds its consecutive records of one pair in registers; what it holds
//                       last goes along the lanes, where runs of one pair are summed towards the run's first lane (run_end,
//                       run_sum); the run heads are staged in the work-group's LDS table and flushed with one atomic per
//                       (work-group, pair, quantity) into the table of swg_pair_table.h, keyed a * n_seq + b: dense while
//                       n_seq^2 <= DENSE_LIMIT, open addressing beyond.  Pair-major input -- tens of thousands of records of one
//                       pair side by side, DESIGN section 13 (3) -- costs one LDS atomic per wavefront and pair.
//   components_list     the occupied slots as swg_link, one atomic per wavefront (wave_place); `joined` is evaluated here.  The
//                       list stays in device memory for what follows; the host's copy is ordered by (a, b) on the host.
//   components_hook     per joined link: both ends walk towards their roots, at most WALK steps, and the larger of the two labels
//   components_compress reached is hooked under the smaller by an atomic minimum; then every sequence walks at most WALK steps
//                       and points at what it reached.  label[s] <= s always, and a label is a member of s's component, so the
//                       fixed point labels every sequence with the smallest id of its component, whatever the order of the
//                       atomics.  No loop waits for another work-group: a walk that did not arrive, like a hook or a move, sets
//                       the `changed` word and the host launches another round.  One read-back of that word per round.
//   components_number   the roots are flagged, swg_exclusive_scan_u32 numbers them, every sequence takes its root's number and
//                       adds itself to the component's row (runs of one component along the lanes first).
//   components_sums     one pass over the LINK list: a link inside a component adds to its row (runs along the lanes first), one
//                       across two adds to the three cross totals (one atomic per wavefront and total).
//
// Device memory, from the context's arena: nothing per record (the host seam stages its six columns and the status there: 25
// bytes per record); per slot 24 bytes of sums and 8 of first records (of which the KEPT half is not used: the table keeps the
// layout its other users have), 8 more per slot when hashed; 40 bytes per link; per sequence label, root flag, scan and
// component number, 16 bytes (the host seam's seq_len: 4 more); 40 bytes per component.  Integer atomics only; no floating point.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"

static_assert(sizeof(swg_link) == 40 && sizeof(swg_component) == 40 && sizeof(swg_component_params) == 16 &&
                  sizeof(swg_component_table) == 80,
              "include/sweepga_gpu.h states these layouts");

namespace {

using namespace swg_pair_table;  // the pair table, the run and wavefront helpers, the host entry helpers
constexpr int ITEMS = 4;         // consecutive records per thread
constexpr int TILE = TB * ITEMS;
constexpr int WALK = 16;         // steps towards the root per launch
constexpr int MAX_ROUNDS = 4096;
enum { V_A = 0, V_B, V_RECORDS, V_COUNT };
enum { D_BAD = 0, D_HEADS, D_LINKS, D_CHANGED, D_ROOTS, D_CROSS_LINKS, D_CROSS_RECORDS, D_CROSS_BASES, D_TOTAL };
using LinkTable = PairTable<V_COUNT, true>;  // sums: a_bases, b_bases, records; first[.][0]: the first record

struct Cols {
  const uint32_t *q_id, *t_id, *start[2], *end[2], *seq_len;
  const uint8_t* status;
};

// the pair of a record that takes part, EMPTY otherwise (ids out of range take no part: components_count reports them)
__device__ __forceinline__ unsigned long long link_key(uint32_t q, uint32_t t, bool kept, uint32_t n_seq) {
  if (!kept || q == t || q >= n_seq || t >= n_seq) return EMPTY;
  return q < t ? (unsigned long long)q * n_seq + t : (unsigned long long)t * n_seq + q;
}

// ---- the runs in input order ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void components_count_kernel(uint64_t n, const uint32_t* __restrict__ q_id, const uint32_t* __restrict__ t_id,
                                                              const uint8_t* __restrict__ status, uint32_t n_seq,
                                                              unsigned long long* __restrict__ scalars) {
  unsigned long long heads = 0;
  bool bad = false;
  for (uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x; i < n; i += (uint64_t)gridDim.x * TB) {
    const uint32_t q = q_id[i], t = t_id[i];
    bad |= q >= n_seq || t >= n_seq;
    const unsigned long long key = link_key(q, t, !status || status[i] != 0, n_seq);
    if (key == EMPTY) continue;
    const unsigned long long before = i ? link_key(q_id[i - 1], t_id[i - 1], !status || status[i - 1] != 0, n_seq) : EMPTY;
    heads += key != before;
  }
  heads = wave_sum(heads);
  const uint64_t any_bad = __ballot(bad);
  if ((threadIdx.x & 63) == 0) {
    if (heads) atomicAdd(&scalars[D_HEADS], heads);
    if (any_bad) atomicOr(&scalars[D_BAD], 1ull);
  }
}

// ---- the link reduction --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void load4(const uint32_t* __restrict__ col, uint64_t end, uint64_t p0, bool vec, uint32_t (&v)[ITEMS]) {
  if (vec) {
    const uint4 w = *reinterpret_cast<const uint4*>(col + p0);
    v[0] = w.x, v[1] = w.y, v[2] = w.z, v[3] = w.w;
  } else {
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) v[j] = p0 + j < end ? col[p0 + j] : 0u;
  }
}

__device__ __forceinline__ void stage(LdsTable<V_COUNT, true>& l_pairs, const LinkTable& T, unsigned long long key,
                                      const unsigned long long (&v)[V_COUNT], uint32_t first) {
  if (!l_pairs.add(key, v, first)) table_add<V_COUNT, true>(T, key, v, 0, first);  // more pairs in this share than the LDS table takes
}

// `aligned`: the six columns start on a 16-byte boundary (the shares are whole tiles of TB records: a thread's four are one load)
__global__ __launch_bounds__(TB) void components_links_kernel(uint64_t n, uint64_t per_group, Cols c, uint32_t n_seq, bool aligned, LinkTable T) {
  __shared__ LdsTable<V_COUNT, true> l_pairs;
  l_pairs.clear();
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const uint64_t b0 = (uint64_t)blockIdx.x * per_group;
  const uint64_t b1 = b0 + per_group < n ? b0 + per_group : n;
  for (uint64_t base = b0; base < b1; base += TILE) {  // uniform trip count per work-group
    const uint64_t p0 = base + (uint64_t)threadIdx.x * ITEMS;
    const bool vec = aligned && p0 + ITEMS <= b1;
    uint32_t q_id[ITEMS], t_id[ITEMS], qs[ITEMS], qe[ITEMS], ts[ITEMS], te[ITEMS];
    load4(c.q_id, b1, p0, vec, q_id);
    load4(c.t_id, b1, p0, vec, t_id);
    load4(c.start[0], b1, p0, vec, qs);
    load4(c.end[0], b1, p0, vec, qe);
    load4(c.start[1], b1, p0, vec, ts);
    load4(c.end[1], b1, p0, vec, te);
    unsigned long long key = EMPTY;
    unsigned long long v[V_COUNT] = {0, 0, 0};
    uint32_t first = NONE32;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) {
      if (p0 + j >= b1) continue;
      const uint32_t q = q_id[j], t = t_id[j];
      const unsigned long long k = link_key(q, t, !c.status || c.status[p0 + j] != 0, n_seq);
      if (k == EMPTY) continue;  // (a record that takes no part does not end a thread's run)
      if (k != key) {
        if (key != EMPTY) stage(l_pairs, T, key, v, first);
        key = k, first = (uint32_t)(p0 + j);
        v[V_A] = v[V_B] = v[V_RECORDS] = 0;
      }
      const uint32_t lq = qe[j] > qs[j] ? qe[j] - qs[j] : 0u, lt = te[j] > ts[j] ? te[j] - ts[j] : 0u;
      v[V_A] += q < t ? lq : lt;
      v[V_B] += q < t ? lt : lq;
      v[V_RECORDS] += 1;
    }
    // what the threads hold last: runs of one pair along the lanes summed towards the run's first lane, whose record is the
    // run's first
    if (__ballot(key != EMPTY) == 0) continue;  // wavefront-uniform
    const unsigned long long before = __shfl_up(key, 1);
    const bool head = lane == 0 || key != before;
    run_sum(v, lane, run_end(__ballot(head), lane));
    if (head && key != EMPTY) stage(l_pairs, T, key, v, first);
  }
  __syncthreads();
  l_pairs.flush(T, 0);
}

// ---- the occupied slots as links -------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long need_bases(uint32_t ppm, uint32_t len) {  // ceil(ppm * len / 10^6): < 2^52
  return ((unsigned long long)ppm * len + 999999ull) / 1000000ull;
}

__global__ __launch_bounds__(TB) void components_list_kernel(LinkTable T, uint32_t n_seq, const uint32_t* __restrict__ seq_len,
                                                             swg_component_params P, swg_link* __restrict__ out, uint64_t cap,
                                                             unsigned long long* __restrict__ scalars) {
  const uint64_t s = (uint64_t)blockIdx.x * TB + threadIdx.x;
  const uint32_t f = s < T.slots ? T.first[s * 2] : NONE32;
  const bool have = f != NONE32;
  const unsigned long long at = wave_place(__ballot(have), &scalars[D_LINKS]);
  if (!have || at >= cap) return;
  const unsigned long long key = T.keys ? T.keys[s] : s;
  const unsigned long long* row = T.sums + s * V_COUNT;
  swg_link l;
  l.a = (uint32_t)(key / n_seq);
  l.b = (uint32_t)(key % n_seq);
  l.n_records = (uint32_t)row[V_RECORDS];
  l.a_bases = row[V_A];
  l.b_bases = row[V_B];
  l.first_record = f;
  const unsigned long long heavier = l.a_bases > l.b_bases ? l.a_bases : l.b_bases;
  l.joined = heavier >= P.min_bases && (l.a_bases >= need_bases(P.min_share_ppm, seq_len[l.a]) || l.b_bases >= need_bases(P.min_share_ppm, seq_len[l.b]));
  out[at] = l;
}

// ---- components over the link list -----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TB) void components_iota_kernel(uint32_t n_seq, uint32_t* __restrict__ label) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n_seq) label[i] = (uint32_t)i;
}

// at most WALK steps from x towards its root (other work-groups lower labels meanwhile: any value read is an ancestor)
__device__ __forceinline__ uint32_t walk(const uint32_t* label, uint32_t x) {
  for (int k = 0; k < WALK; ++k) {
    const uint32_t p = __hip_atomic_load(&label[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (p == x) break;
    x = p;
  }
  return x;
}

__global__ __launch_bounds__(TB) void components_hook_kernel(uint64_t m, const swg_link* __restrict__ links, uint32_t* label,
                                                             unsigned long long* __restrict__ scalars) {
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (e >= m || !links[e].joined) return;
  const uint32_t ra = walk(label, links[e].a), rb = walk(label, links[e].b);
  if (ra == rb) return;
  atomicMin(&label[ra > rb ? ra : rb], ra > rb ? rb : ra);
  scalars[D_CHANGED] = 1;
}

__global__ __launch_bounds__(TB) void components_compress_kernel(uint32_t n_seq, uint32_t* label, unsigned long long* __restrict__ scalars) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i >= n_seq) return;
  const uint32_t l = __hip_atomic_load(&label[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const uint32_t r = walk(label, l);
  if (r == l) return;  // l is a root
  __hip_atomic_store(&label[i], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  scalars[D_CHANGED] = 1;  // (a walk that stopped short of the root moved too)
}

__global__ __launch_bounds__(TB) void components_roots_kernel(uint32_t n_seq, const uint32_t* __restrict__ label, uint32_t* __restrict__ flag) {
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  if (i < n_seq) flag[i] = label[i] == i ? 1u : 0u;
}

// rows: zeroed.  A root writes its row's id and first_seq; every sequence adds itself, runs of one component along the lanes first.
__global__ __launch_bounds__(TB) void components_number_kernel(uint32_t n_seq, const uint32_t* __restrict__ label, const uint32_t* __restrict__ excl,
                                                               const uint32_t* __restrict__ seq_len, uint32_t* __restrict__ seq_component,
                                                               swg_component* rows) {
  const int lane = threadIdx.x & 63;
  const uint64_t i = (uint64_t)blockIdx.x * TB + threadIdx.x;
  uint32_t comp = 0;  // 0: past the end
  unsigned long long v[2] = {0, 0};
  if (i < n_seq) {
    const uint32_t root = label[i];
    comp = excl[root] + 1;
    seq_component[i] = comp;
    v[0] = 1, v[1] = seq_len[i];
    if (root == i) rows[comp - 1].id = comp, rows[comp - 1].first_seq = (uint32_t)i;
  }
  const uint32_t before = __shfl_up(comp, 1);
  const bool head = lane == 0 || comp != before;
  run_sum(v, lane, run_end(__ballot(head), lane));
  if (head && comp) {
    atomicAdd(&rows[comp - 1].n_seq, (uint32_t)v[0]);
    if (v[1]) atomicAdd(reinterpret_cast<unsigned long long*>(&rows[comp - 1].length), v[1]);
  }
}

__global__ __launch_bounds__(TB) void components_sums_kernel(uint64_t m, const swg_link* __restrict__ links, const uint32_t* __restrict__ seq_component,
                                                             swg_component* rows, unsigned long long* __restrict__ scalars) {
  const int lane = threadIdx.x & 63;
  const uint64_t e = (uint64_t)blockIdx.x * TB + threadIdx.x;
  uint32_t comp = 0;  // 0: no link here, or one across two components
  unsigned long long v[3] = {0, 0, 0}, x[3] = {0, 0, 0};
  if (e < m) {
    const swg_link l = links[e];
    const uint32_t ca = seq_component[l.a], cb = seq_component[l.b];
    const unsigned long long bases = l.a_bases + l.b_bases;
    if (ca == cb)
      comp = ca, v[0] = 1, v[1] = l.n_records, v[2] = bases;
    else
      x[0] = 1, x[1] = l.n_records, x[2] = bases;
  }
  const uint32_t before = __shfl_up(comp, 1);
  const bool head = lane == 0 || comp != before;
  run_sum(v, lane, run_end(__ballot(head), lane));
  if (head && comp) {
    atomicAdd(&rows[comp - 1].n_links, (uint32_t)v[0]);
    atomicAdd(reinterpret_cast<unsigned long long*>(&rows[comp - 1].n_records), v[1]);
    if (v[2]) atomicAdd(reinterpret_cast<unsigned long long*>(&rows[comp - 1].bases), v[2]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    x[k] = wave_sum(x[k]);
    if (lane == 0 && x[k]) atomicAdd(&scalars[D_CROSS_LINKS + k], x[k]);
  }
}

bool aligned_to(const void* p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
unsigned groups(uint64_t items) { return (unsigned)((items + TB - 1) / TB); }

// inside an arena frame
int components_device(swg_ctx* ctx, uint64_t n, uint32_t n_seq, const Cols& d, const swg_component_params& P, bool want_links, bool want_seq,
                      swg_components_result* res) {
  hipStream_t st = ctx->stream;
  const char* knob = std::getenv("SWG_COMPONENTS_HASH");  // test knob: the hashed pair table at any size
  const bool force_hash = knob && knob[0] == '1';
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  uint32_t* label = swg_alloc<uint32_t>(ctx, n_seq);
  uint32_t* flag = swg_alloc<uint32_t>(ctx, n_seq);
  uint32_t* excl = swg_alloc<uint32_t>(ctx, n_seq);
  uint32_t* comp = swg_alloc<uint32_t>(ctx, n_seq);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  uint64_t h[D_TOTAL] = {};
  // ---- links
  swg_link* links = nullptr;
  uint64_t m = 0;
  if (n) {
    SWG_LAUNCH(ctx, "components_count", components_count_kernel<<<grid_for(ctx, n), TB, 0, st>>>(n, d.q_id, d.t_id, d.status, n_seq, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, 2));
    if (h[D_BAD]) return swg_set_error(ctx, SWG_ERR_INVALID, "components: a sequence id >= n_seq");
  }
  if (h[D_HEADS]) {
    const uint64_t all_pairs = (uint64_t)n_seq * (n_seq - 1) / 2;
    const uint64_t pairs_max = all_pairs < h[D_HEADS] ? all_pairs : h[D_HEADS];
    LinkTable T;
    table_alloc(ctx, n_seq, pairs_max, force_hash, &T);
    links = swg_alloc<swg_link>(ctx, pairs_max);
    SWG_CHECK_ARENA(ctx);
    SWG_TRY(table_clear(ctx, T));
    bool aligned = true;
    for (const uint32_t* p : {d.q_id, d.t_id, d.start[0], d.start[1], d.end[0], d.end[1]}) aligned = aligned && aligned_to(p, 16);
    const Share share = share_for(ctx, n);
    SWG_LAUNCH(ctx, "components_links", components_links_kernel<<<share.grid, TB, 0, st>>>(n, share.per_group, d, n_seq, aligned, T));
    SWG_KERNEL_CHECK(ctx);
    SWG_LAUNCH(ctx, "components_list", components_list_kernel<<<groups(T.slots), TB, 0, st>>>(T, n_seq, d.seq_len, P, links, pairs_max, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + D_LINKS, &m, 1));
    if (m == 0 || m > pairs_max)
      return swg_set_error(ctx, SWG_ERR_HIP, "components: internal: %llu links listed, between 1 and %llu expected", (unsigned long long)m,
                           (unsigned long long)pairs_max);
  }
  // ---- components
  SWG_LAUNCH(ctx, "components_iota", components_iota_kernel<<<groups(n_seq), TB, 0, st>>>(n_seq, label));
  SWG_KERNEL_CHECK(ctx);
  for (int round = 0; m; ++round) {
    if (round == MAX_ROUNDS) return swg_set_error(ctx, SWG_ERR_HIP, "components: internal: no fixed point after %d rounds", MAX_ROUNDS);
    SWG_HIP(ctx, hipMemsetAsync(scalars + D_CHANGED, 0, sizeof(unsigned long long), st));
    SWG_LAUNCH(ctx, "components_hook", components_hook_kernel<<<groups(m), TB, 0, st>>>(m, links, label, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_LAUNCH(ctx, "components_compress", components_compress_kernel<<<groups(n_seq), TB, 0, st>>>(n_seq, label, scalars));
    SWG_KERNEL_CHECK(ctx);
    uint64_t changed = 0;
    SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + D_CHANGED, &changed, 1));
    if (!changed) break;
  }
  // ---- numbering and rows
  SWG_LAUNCH(ctx, "components_roots", components_roots_kernel<<<groups(n_seq), TB, 0, st>>>(n_seq, label, flag));
  SWG_KERNEL_CHECK(ctx);
  SWG_TRY(swg_exclusive_scan_u32(ctx, flag, excl, n_seq, reinterpret_cast<uint64_t*>(scalars) + D_ROOTS));
  uint64_t C = 0;
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars) + D_ROOTS, &C, 1));
  if (C == 0 || C > n_seq)
    return swg_set_error(ctx, SWG_ERR_HIP, "components: internal: %llu components of %u sequences", (unsigned long long)C, n_seq);
  swg_component* rows = swg_alloc<swg_component>(ctx, C);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(rows, 0, C * sizeof(swg_component), st));
  SWG_LAUNCH(ctx, "components_number", components_number_kernel<<<groups(n_seq), TB, 0, st>>>(n_seq, label, excl, d.seq_len, comp, rows));
  SWG_KERNEL_CHECK(ctx);
  if (m) {
    SWG_LAUNCH(ctx, "components_sums", components_sums_kernel<<<groups(m), TB, 0, st>>>(m, links, comp, rows, scalars));
    SWG_KERNEL_CHECK(ctx);
  }
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  res->cross_links = h[D_CROSS_LINKS];
  res->cross_records = h[D_CROSS_RECORDS];
  res->cross_bases = h[D_CROSS_BASES];
  res->components.resize(C);
  SWG_HIP(ctx, hipMemcpyAsync(res->components.data(), rows, C * sizeof(swg_component), hipMemcpyDeviceToHost, st));
  res->links.resize(m);  // (the number is wanted either way)
  if (want_links && m) SWG_HIP(ctx, hipMemcpyAsync(res->links.data(), links, m * sizeof(swg_link), hipMemcpyDeviceToHost, st));
  if (want_seq) {
    res->seq_component.resize(n_seq);
    SWG_HIP(ctx, hipMemcpyAsync(res->seq_component.data(), comp, (size_t)n_seq * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  }
  SWG_HIP(ctx, hipStreamSynchronize(st));
  if (want_links)  // (the listing order is whatever the atomics made it)
    std::sort(res->links.begin(), res->links.end(), [](const swg_link& x, const swg_link& y) { return x.a != y.a ? x.a < y.a : x.b < y.b; });
  return SWG_OK;
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status,
                const swg_component_params* params, swg_component_table* table) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!table) return swg_set_error(ctx, SWG_ERR_INVALID, "components: NULL table");
  try {
    swg_components_result r;
    SWG_TRY(swg_components_run(ctx, rec, on_device, seq_len, status, params, table->links != nullptr, table->seq_component != nullptr, &r));
    table->n_components = r.components.size();
    table->n_links = r.links.size();
    table->cross_links = r.cross_links;
    table->cross_records = r.cross_records;
    table->cross_bases = r.cross_bases;
    if (table->components && table->n_components <= table->component_capacity) std::copy(r.components.begin(), r.components.end(), table->components);
    if (table->links && table->n_links <= table->link_capacity) std::copy(r.links.begin(), r.links.end(), table->links);
    if (table->seq_component) std::copy(r.seq_component.begin(), r.seq_component.end(), table->seq_component);
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

}  // namespace

int swg_components_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const uint32_t* seq_len, const uint8_t* status,
                       const swg_component_params* params, bool want_links, bool want_seq, swg_components_result* res) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !res) return swg_set_error(ctx, SWG_ERR_INVALID, "components: NULL records");
  *res = swg_components_result{};
  const swg_component_params P = params ? *params : swg_component_params{0, 0, 0};
  if (P.min_share_ppm > 1000000u) return swg_set_error(ctx, SWG_ERR_INVALID, "components: min_share_ppm above 1000000");
  if (P.reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "components: reserved must be 0");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "components: 2^31 records or more in one call");
  if (n && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end))
    return swg_set_error(ctx, SWG_ERR_INVALID, "components: NULL column (q_id, t_id and the four coordinates are read)");
  if (n && n_seq == 0) return swg_set_error(ctx, SWG_ERR_INVALID, "components: records without sequences");
  if (n_seq == 0) return SWG_OK;
  if (!seq_len) return swg_set_error(ctx, SWG_ERR_INVALID, "components: NULL seq_len");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (on_device ? 8 : 32) + (size_t)n_seq * 64 + (size_t(8) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    Cols d{rec->q_id, rec->t_id, {rec->q_start, rec->t_start}, {rec->q_end, rec->t_end}, seq_len, status};
    if (!on_device) {  // (n == 0 with sequences: the record columns may be NULL and stay so)
      swg_stager s(ctx);
      for (const uint32_t** col : {&d.q_id, &d.t_id, &d.start[0], &d.start[1], &d.end[0], &d.end[1]}) s.add(col, n);
      s.add(&d.seq_len, n_seq);
      s.add(&d.status, n);
      SWG_TRY(s.run());
    }
    return components_device(ctx, n, n_seq, d, P, want_links, want_seq, res);
  });
}

extern "C" int swg_components_records(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status,
                                      const swg_component_params* params, swg_component_table* table) {
  return records_abi(ctx, rec, false, seq_len, status, params, table);
}

extern "C" int swg_components_records_device(swg_ctx* ctx, const swg_records* rec, const uint32_t* seq_len, const uint8_t* status,
                                             const swg_component_params* params, swg_component_table* table) {
  return records_abi(ctx, rec, true, seq_len, status, params, table);
}

// The components report of an open PAF: records from the handle, seq_len from the handle's text (host/paf_io.cpp), the tables
// from the device, the names from the handle.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_components(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_component_params* params, int detailed,
                                  char** out_text, uint64_t* out_len) {
  if (out_text) *out_text = nullptr;
  if (out_len) *out_len = 0;
  if (!p || !out_text || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_components: NULL argument");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_components: the file has a value >= 2^32, its columns are rebased: components of 64-bit columns are not supported");
  const swg_records* rec = swg_paf_records(p);
  const uint64_t n = rec->n;
  try {
    swg_components_result r;
    std::vector<uint32_t> seq_len;
    const uint32_t n_seq = n ? swg_paf_num_sequences(p) : 0;
    if (n) {
      if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_components: NULL context");
      SWG_TRY(swg_paf_seq_last_lengths(p, &seq_len));
      const int rc = swg_components_run(ctx, rec, false, seq_len.data(), status, params, true, true, &r);
      if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
    }
    std::vector<uint64_t> own((size_t)n_seq * 3, 0);  // links, records, bases of every sequence's own links
    for (const swg_link& l : r.links)
      for (uint32_t s : {l.a, l.b}) {
        own[(size_t)s * 3] += 1;
        own[(size_t)s * 3 + 1] += l.n_records;
        own[(size_t)s * 3 + 2] += l.a_bases + l.b_bases;
      }
    std::string o = "sequence\tlength\tcomponent\tcomponent_sequences\tcomponent_length\tlinks\trecords\tbases\n";
    for (uint32_t s = 0; s < n_seq; ++s) {
      const swg_component& c = r.components[r.seq_component[s] - 1];
      o += swg_paf_sequence_name(p, s);
      o += '\t';
      append_u64(o, seq_len[s], '\t');
      append_u64(o, c.id, '\t');
      append_u64(o, c.n_seq, '\t');
      append_u64(o, c.length, '\t');
      append_u64(o, own[(size_t)s * 3], '\t');
      append_u64(o, own[(size_t)s * 3 + 1], '\t');
      append_u64(o, own[(size_t)s * 3 + 2], '\n');
    }
    if (detailed) {
      o += "#links\n";
      for (const swg_link& l : r.links) {
        o += swg_paf_sequence_name(p, l.a);
        o += '\t';
        o += swg_paf_sequence_name(p, l.b);
        o += '\t';
        append_u64(o, l.n_records, '\t');
        append_u64(o, l.a_bases, '\t');
        append_u64(o, l.b_bases, '\t');
        append_u64(o, l.joined, '\n');
      }
    }
    o += "#cross\t";
    append_u64(o, r.cross_links, '\t');
    append_u64(o, r.cross_records, '\t');
    append_u64(o, r.cross_bases, '\n');
    char* t = text_copy(o);
    if (!t) return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
    *out_text = t;
    *out_len = o.size();
    return SWG_OK;
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
