// Dot plot: the records rasterised into four uint32 count planes -- ALL '+', ALL '-', KEPT '+', KEPT '-' --
// of height x width pixels over two concatenated axes (x = targets, y = queries), every record a line of max(dx, dy) + 1 pixels
// whose steps are closed forms of the step number.  The sort / scan / compact reports before this one never scatter; this one
// does nothing else, and at 10^8 records almost every mapping is smaller than a pixel and lands on a few thousand diagonal pixels:
// one global atomic per record would be DESIGN.md section 13 item (3) again.
//
//   dot_classify   one thread per record, contiguous shares per work-group: the endpoints, the error word, the drawn counts.
//                  Sub-pixel records (L = 0): equal pixels along neighbouring lanes are summed towards the run's first lane (the
//                  four plane counts packed into one word, 16 bits each: a run has at most 64 lanes), the run heads go through the
//                  work-group's LdsTable<4, false> keyed by pixel, and at the end one atomic per (work-group, pixel, non-zero
//                  plane) reaches the planes.  Records with L >= 1 are appended to a list of record indices, one atomic per
//                  wavefront (wave_place); its order is arbitrary, integer adds commute.
//   dot_lines      a wavefront per listed record, grid-stride over the list (its length is read from the device scalar: no
//                  read-back in between); lanes stride over the steps k = lane, lane + 64, ...: one atomic per pixel and plane.
//                  The major axis advances by one per step, so the lanes' pixels are distinct.
//   dot_sums       work-group reduction of every wanted plane into hits, one atomic per work-group and plane.
//
// Only the planes named by `want` are allocated, cleared, summed and read back.  No work-group waits for another inside a launch;
// all accumulation is integer, so the planes do not depend on record order or grid shape.
#include <algorithm>
#include <cstring>
#include <new>
#include <string>

#include "swg_internal.h"
#include "swg_pair_table.h"
#include "host/host_internal.h"

namespace {

using namespace swg_pair_table;
// device scalars: bad input (bit 0: an id out of range, bit 1: a drawn record ends beyond its axis), the drawn records of ALL and
// KEPT, the length of the line list, the four plane sums
enum { D_BAD = 0, D_DRAWN = 1, D_LIST = 3, D_HITS = 4, D_TOTAL = 8 };
constexpr uint32_t MAX_SIDE = 16384;
constexpr uint64_t MAX_TOTAL = uint64_t(1) << 48;

struct DotCols {
  const uint32_t *q_id, *t_id, *q_start, *q_end, *t_start, *t_end;
  const uint8_t *strand, *status;
};
struct DotAxes {
  uint32_t width, height, n_seq;
  uint64_t x_total, y_total;
  const uint64_t *x_off, *y_off;
};
struct DotPlanes {
  uint32_t* p[4];  // nullptr = not wanted
};
struct DotLine {
  uint32_t x0, y0, dx, dy;  // dy = |y1 - y0|; the line falls when `minus`
  uint32_t mask;            // the planes the record counts in: bit strand, bit 2 + strand when kept (before `want`)
};

// The endpoints of record i.  false: not drawn (zero length, an absent sequence, or bad input, which raises the error word when
// `scalars` is given).  Every pixel of a drawn record lies inside the image: off + end <= total, so px <= width - 1.
__device__ __forceinline__ bool dot_endpoints(uint64_t i, const DotCols& c, const DotAxes& a, unsigned long long* scalars, DotLine* out) {
  const uint32_t q = c.q_id[i], t = c.t_id[i];
  if (q >= a.n_seq || t >= a.n_seq) {
    if (scalars) atomicOr(&scalars[D_BAD], 1ull);
    return false;
  }
  const uint32_t qs = c.q_start[i], qe = c.q_end[i], ts = c.t_start[i], te = c.t_end[i];
  const uint64_t xo = a.x_off[t], yo = a.y_off[q];
  if (qe <= qs || te <= ts || xo == SWG_DOT_ABSENT || yo == SWG_DOT_ABSENT) return false;
  if (xo > a.x_total || yo > a.y_total || xo + te > a.x_total || yo + qe > a.y_total) {  // (offsets first: the sums cannot wrap)
    if (scalars) atomicOr(&scalars[D_BAD], 2ull);
    return false;
  }
  const uint32_t minus = c.strand[i] != 0 ? 1u : 0u;
  const uint32_t x0 = (uint32_t)((xo + ts) * a.width / a.x_total), x1 = (uint32_t)((xo + te - 1) * a.width / a.x_total);
  const uint32_t ya = (uint32_t)((yo + qs) * a.height / a.y_total), yb = (uint32_t)((yo + qe - 1) * a.height / a.y_total);
  out->x0 = x0;
  out->y0 = minus ? yb : ya;
  out->dx = x1 - x0;
  out->dy = yb - ya;
  out->mask = (1u << minus) | (c.status && c.status[i] != 0 ? 4u << minus : 0u);
  return true;
}

__global__ __launch_bounds__(TB) void dot_classify_kernel(uint64_t n, uint64_t per_group, DotCols c, DotAxes a, uint32_t want, DotPlanes P,
                                                          uint32_t* __restrict__ list, unsigned long long* __restrict__ scalars) {
  __shared__ LdsTable<4, false> l_table;
  __shared__ unsigned long long l_drawn[2][WAVES];
  l_table.clear();
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t begin = (uint64_t)blockIdx.x * per_group, end = begin + per_group < n ? begin + per_group : n;
  unsigned long long drawn[2] = {0, 0};
  for (uint64_t base = begin; base < end; base += TB) {  // (uniform: whole wavefronts vote)
    const uint64_t i = base + threadIdx.x;
    unsigned long long key = EMPTY, v[1] = {0};
    bool is_line = false;
    DotLine ln;
    if (i < end && dot_endpoints(i, c, a, scalars, &ln)) {
      ++drawn[0];
      if (ln.mask & 0xcu) ++drawn[1];
      const uint32_t m = ln.mask & want;
      if (m) {
        if ((ln.dx | ln.dy) == 0) {
          key = (unsigned long long)ln.y0 * a.width + ln.x0;
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (m >> j & 1u) v[0] |= 1ull << (16 * j);
        } else {
          is_line = true;
        }
      }
    }
    // sub-pixel records: runs of one pixel along the lanes, summed towards the run's first lane
    const unsigned long long left = __shfl_up(key, 1);
    const bool first_lane = lane == 0 || key != left;
    run_sum(v, lane, run_end(__ballot(first_lane), lane));
    if (first_lane && key != EMPTY) {
      unsigned long long cnt[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) cnt[j] = (v[0] >> (16 * j)) & 0xffffull;
      if (!l_table.add(key, cnt)) {  // more pixels in this work-group's share than the LDS table takes
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (cnt[j]) atomicAdd(&P.p[j][key], (uint32_t)cnt[j]);
      }
    }
    // records of two pixels or more: to the list
    const unsigned long long at = wave_place(__ballot(is_line), &scalars[D_LIST]);
    if (is_line && at < n) list[at] = (uint32_t)i;  // (always: a record is listed once)
  }
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    const unsigned long long d = wave_sum(drawn[s]);
    if (lane == 0) l_drawn[s][wave] = d;
  }
  __syncthreads();  // (also behind the last add of the table)
  if (threadIdx.x < 2) {
    unsigned long long d = 0;
    for (int w = 0; w < WAVES; ++w) d += l_drawn[threadIdx.x][w];
    if (d) atomicAdd(&scalars[D_DRAWN + threadIdx.x], d);
  }
  for (int s = threadIdx.x; s < LSLOTS; s += TB) {
    const unsigned long long key = l_table.key[s];
    if (key == EMPTY) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (l_table.sum[s][j]) atomicAdd(&P.p[j][key], (uint32_t)l_table.sum[s][j]);  // (non-zero only for wanted planes)
  }
}

__global__ __launch_bounds__(TB) void dot_lines_kernel(uint64_t n, DotCols c, DotAxes a, uint32_t want, DotPlanes P,
                                                       const uint32_t* __restrict__ list, const unsigned long long* __restrict__ scalars) {
  const int lane = threadIdx.x & 63;
  const unsigned long long listed = scalars[D_LIST];
  const uint64_t m = listed < n ? listed : n;
  for (uint64_t r = (uint64_t)blockIdx.x * WAVES + (threadIdx.x >> 6); r < m; r += (uint64_t)gridDim.x * WAVES) {
    const uint64_t i = list[r];
    DotLine ln;
    if (i >= n || !dot_endpoints(i, c, a, nullptr, &ln)) continue;  // (never: classify listed it)
    const uint32_t mask = ln.mask & want, L = ln.dx > ln.dy ? ln.dx : ln.dy;
    if (L == 0 || mask == 0) continue;  // (never)
    const bool minus = (ln.mask & 0x2u) != 0;
    for (uint32_t k = lane; k <= L; k += 64) {  // 2 k d + L < 2^30
      const uint32_t x = ln.x0 + (2u * k * ln.dx + L) / (2u * L), sy = (2u * k * ln.dy + L) / (2u * L);
      const uint32_t y = minus ? ln.y0 - sy : ln.y0 + sy;
      const uint32_t at = y * a.width + x;  // < 2^28
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (mask >> j & 1u) atomicAdd(&P.p[j][at], 1u);
    }
  }
}

__global__ __launch_bounds__(TB) void dot_sums_kernel(DotPlanes P, uint64_t size, unsigned long long* __restrict__ scalars) {
  __shared__ unsigned long long l_sum[WAVES];
  for (int j = 0; j < 4; ++j) {
    if (!P.p[j]) continue;  // (uniform)
    unsigned long long s = 0;
    for (uint64_t x = (uint64_t)blockIdx.x * TB + threadIdx.x; x < size; x += (uint64_t)gridDim.x * TB) s += P.p[j][x];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) l_sum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      unsigned long long t = 0;
      for (int w = 0; w < WAVES; ++w) t += l_sum[w];
      if (t) atomicAdd(&scalars[D_HITS + j], t);
    }
    __syncthreads();
  }
}

// inside an arena frame; c and a hold device pointers
int dotplot_device(swg_ctx* ctx, uint64_t n, const DotCols& c, const DotAxes& a, swg_dot_request* req) {
  hipStream_t st = ctx->stream;
  const uint32_t want = req->want;
  const uint64_t size = (uint64_t)a.width * a.height;
  unsigned long long* scalars = swg_alloc<unsigned long long>(ctx, D_TOTAL);
  DotPlanes P{};
  for (int j = 0; j < 4; ++j)
    if (want >> j & 1u) P.p[j] = swg_alloc<uint32_t>(ctx, size);
  uint32_t* list = swg_alloc<uint32_t>(ctx, n ? n : 1);
  SWG_CHECK_ARENA(ctx);
  SWG_HIP(ctx, hipMemsetAsync(scalars, 0, D_TOTAL * sizeof(unsigned long long), st));
  for (int j = 0; j < 4; ++j)
    if (P.p[j]) SWG_HIP(ctx, hipMemsetAsync(P.p[j], 0, size * sizeof(uint32_t), st));
  if (n) {
    const Share sh = share_for(ctx, n);
    SWG_LAUNCH(ctx, "dot_classify", dot_classify_kernel<<<sh.grid, TB, 0, st>>>(n, sh.per_group, c, a, want, P, list, scalars));
    SWG_KERNEL_CHECK(ctx);
    const unsigned grid_l = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + WAVES - 1) / WAVES, (uint64_t)ctx->num_cu * 8));
    SWG_LAUNCH(ctx, "dot_lines", dot_lines_kernel<<<grid_l, TB, 0, st>>>(n, c, a, want, P, list, scalars));
    SWG_KERNEL_CHECK(ctx);
    SWG_LAUNCH(ctx, "dot_sums", dot_sums_kernel<<<grid_for(ctx, size), TB, 0, st>>>(P, size, scalars));
    SWG_KERNEL_CHECK(ctx);
  }
  uint64_t h[D_TOTAL];
  SWG_TRY(swg_read_scalars(ctx, reinterpret_cast<uint64_t*>(scalars), h, D_TOTAL));
  if (h[D_BAD] & 1u) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: a sequence id >= n_seq");
  if (h[D_BAD] & 2u) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: a drawn record ends beyond the total of its axis");
  for (int j = 0; j < 4; ++j)
    if (P.p[j]) SWG_HIP(ctx, hipMemcpyAsync(req->plane[j], P.p[j], size * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  for (int j = 0; j < 4; ++j)
    if (P.p[j]) req->hits[j] = h[D_HITS + j];
  req->drawn[0] = h[D_DRAWN];
  req->drawn[1] = h[D_DRAWN + 1];
  return SWG_OK;
}

// the seams' argument checks, then the device work inside an arena frame
int dotplot_run(swg_ctx* ctx, const swg_records* rec, bool on_device, const swg_dot_axes* axes, const uint8_t* status, swg_dot_request* req) {
  if (!ctx) return SWG_ERR_INVALID;
  if (!rec || !axes || !req) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: NULL records, axes or request");
  if (req->reserved != 0) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: reserved must be 0");
  const uint32_t want = req->want;
  if (want == 0 || want >> 4) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: want names nothing, or a bit beyond the four");
  if (!status && (want & 0xcu)) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: the KEPT planes need a status column");
  for (int j = 0; j < 4; ++j)
    if ((want >> j & 1u) && !req->plane[j]) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: a wanted plane with a NULL array");
  if (axes->width < 1 || axes->width > MAX_SIDE || axes->height < 1 || axes->height > MAX_SIDE)
    return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: width and height must lie in 1 .. 16384");
  if (axes->x_total < 1 || axes->x_total >= MAX_TOTAL || axes->y_total < 1 || axes->y_total >= MAX_TOTAL)
    return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: the axis totals must lie in 1 .. 2^48 - 1");
  const uint64_t n = rec->n;
  const uint32_t n_seq = rec->n_seq;
  if (n >= (uint64_t(1) << 31)) return swg_set_error(ctx, SWG_ERR_RANGE, "dotplot: 2^31 records or more in one call");
  if (n && (!rec->q_id || !rec->t_id || !rec->q_start || !rec->q_end || !rec->t_start || !rec->t_end || !rec->strand))
    return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: NULL column (q_id, t_id, the four coordinates and strand are read)");
  if (n && (!axes->x_off || !axes->y_off || n_seq == 0)) return swg_set_error(ctx, SWG_ERR_INVALID, "dotplot: records without sequences or offsets");
  const uint64_t size = (uint64_t)axes->width * axes->height;
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  SWG_TRY(reserve_first(ctx, (size_t)n * (on_device ? 4 : 30) + (size_t)n_seq * 16 + (size_t)size * 4 * __builtin_popcount(want) + (size_t(1) << 20)));
  return swg_run_with_arena(ctx, [&]() -> int {
    DotCols c{rec->q_id, rec->t_id, rec->q_start, rec->q_end, rec->t_start, rec->t_end, rec->strand, status};
    DotAxes a{axes->width, axes->height, n_seq, axes->x_total, axes->y_total, axes->x_off, axes->y_off};
    if (!on_device && n) {
      swg_stager s(ctx);
      for (const uint32_t** col : {&c.q_id, &c.t_id, &c.q_start, &c.q_end, &c.t_start, &c.t_end}) s.add(col, n);
      s.add(&a.x_off, n_seq);
      s.add(&a.y_off, n_seq);
      s.add(&c.strand, n);
      s.add(&c.status, n);
      SWG_TRY(s.run());
    }
    return dotplot_device(ctx, n, c, a, req);
  });
}

int records_abi(swg_ctx* ctx, const swg_records* rec, bool on_device, const swg_dot_axes* axes, const uint8_t* status, swg_dot_request* req) {
  try {
    return dotplot_run(ctx, rec, on_device, axes, status, req);
  } catch (const std::bad_alloc&) {
    return swg_set_error(ctx, SWG_ERR_OOM, "out of host memory");
  }
}

// ---- the texts of swg_paf_dotplot --------------------------------------------------------------------------------------------
struct AxisSeq {
  uint32_t seq, genome;
  uint64_t off, len;
};
struct Axis {
  std::vector<AxisSeq> seqs;  // in axis order: (genome id, sequence id)
  uint64_t total = 0;
};

bool starts_with(const char* name, const char* prefix) { return !prefix || std::strncmp(name, prefix, std::strlen(prefix)) == 0; }

// the sequences flagged in `occurs` whose name starts with the prefix, ordered by (genome, id), with cumulative offsets
void build_axis(const swg_paf* p, const std::vector<uint8_t>& occurs, const uint32_t* seq_genome, const std::vector<uint32_t>& seq_len,
                const char* prefix, Axis* ax) {
  for (uint32_t s = 0; s < occurs.size(); ++s)
    if (occurs[s] && starts_with(swg_paf_sequence_name(p, s), prefix)) ax->seqs.push_back(AxisSeq{s, seq_genome[s], 0, seq_len[s]});
  std::sort(ax->seqs.begin(), ax->seqs.end(), [](const AxisSeq& x, const AxisSeq& y) { return x.genome != y.genome ? x.genome < y.genome : x.seq < y.seq; });
  for (AxisSeq& e : ax->seqs) {
    e.off = ax->total;
    ax->total += e.len;
  }
}

uint32_t pixel_of(uint64_t at, uint32_t side, uint64_t total) { return (uint32_t)(at * side / total); }

// per pixel column (row) of an axis: whether it is px(off) of the first sequence of a genome other than the axis' first
std::vector<uint8_t> genome_lines(const Axis& ax, uint32_t side) {
  std::vector<uint8_t> line(side, 0);
  for (size_t k = 1; k < ax.seqs.size(); ++k)
    if (ax.seqs[k].genome != ax.seqs[k - 1].genome && ax.seqs[k].off < ax.total) line[pixel_of(ax.seqs[k].off, side, ax.total)] = 1;
  return line;
}

void layout_rows(const swg_paf* p, const std::vector<std::string>& gname, const Axis& ax, char axis, uint32_t side, std::string* o) {
  for (const AxisSeq& e : ax.seqs) {
    const uint32_t first = pixel_of(std::min(e.off, ax.total - 1), side, ax.total);
    const uint32_t last = e.len ? pixel_of(e.off + e.len - 1, side, ax.total) : first;
    *o += axis;
    *o += '\t';
    *o += swg_paf_sequence_name(p, e.seq);
    *o += '\t';
    *o += gname[e.genome];
    *o += '\t' + std::to_string(e.off) + '\t' + std::to_string(e.len) + '\t' + std::to_string(first) + '\t' + std::to_string(last) + '\n';
  }
}

}  // namespace

extern "C" int swg_dotplot_records(swg_ctx* ctx, const swg_records* rec, const swg_dot_axes* axes, const uint8_t* status, swg_dot_request* req) {
  return records_abi(ctx, rec, false, axes, status, req);
}

extern "C" int swg_dotplot_records_device(swg_ctx* ctx, const swg_records* rec, const swg_dot_axes* axes, const uint8_t* status,
                                          swg_dot_request* req) {
  return records_abi(ctx, rec, true, axes, status, req);
}

// The image and the layout table of an open PAF: the axes are made on the host from the handle's id columns (which sequences
// occur), its names (prefixes), the last-'#' genome map (order) and the last-seen lengths (offsets); the four planes come from
// ONE device call and are coloured here.  Errors: swg_alnstats_last_error().
extern "C" int swg_paf_dotplot(swg_ctx* ctx, const swg_paf* p, const uint8_t* status, const swg_dot_view* view, char* out[2], uint64_t out_len[2]) {
  if (!p || !view || !out || !out_len) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_dotplot: NULL argument");
  const bool wanted[2] = {out[0] != nullptr, out[1] != nullptr};
  out[0] = out[1] = nullptr;
  out_len[0] = out_len[1] = 0;
  if (!wanted[0] && !wanted[1]) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_dotplot: neither text is asked for");
  if (!status) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_dotplot: the kept planes need a status column");
  const uint32_t W = view->width, H = view->height;
  if (W < 1 || W > MAX_SIDE || H < 1 || H > MAX_SIDE)
    return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_dotplot: width and height must lie in 1 .. 16384");
  if (swg_paf_seq_offsets(p) || swg_paf_record_offsets(p, 0))
    return swg_alnstats_error(SWG_ERR_UNSUPPORTED,
                              "swg_paf_dotplot: the file has a value >= 2^32, its columns are rebased: a dot plot of 64-bit columns is not supported");
  try {
    const swg_records* rec = swg_paf_records(p);
    const uint64_t n = rec->n;
    const uint32_t n_seq = n ? rec->n_seq : 0;
    const char* prefix[2] = {view->target_prefix && *view->target_prefix ? view->target_prefix : nullptr,
                             view->query_prefix && *view->query_prefix ? view->query_prefix : nullptr};
    Axis ax[2];  // 0 = x (targets), 1 = y (queries)
    std::vector<std::string> gname;
    if (n) {
      std::vector<uint32_t> seq_len;
      SWG_TRY(swg_paf_seq_last_lengths(p, &seq_len));
      std::vector<uint8_t> occurs[2] = {std::vector<uint8_t>(n_seq, 0), std::vector<uint8_t>(n_seq, 0)};
      for (uint64_t r = 0; r < n; ++r) {
        occurs[0][rec->t_id[r]] = 1;
        occurs[1][rec->q_id[r]] = 1;
      }
      for (int k = 0; k < 2; ++k) build_axis(p, occurs[k], rec->seq_genome_last, seq_len, prefix[k], &ax[k]);
      swg_paf_stats_genome_names(p, &gname);
    }
    if (ax[0].total >= MAX_TOTAL || ax[1].total >= MAX_TOTAL) return swg_alnstats_error(SWG_ERR_RANGE, "swg_paf_dotplot: an axis of 2^48 bases or more");
    const bool empty = ax[0].total == 0 || ax[1].total == 0;  // no record, no sequence under a prefix, or no base: all white
    const uint64_t size = (uint64_t)W * H;
    std::string text[2];
    if (wanted[1]) {
      text[1] = "axis\tsequence\tgenome\toffset\tlength\tfirst_pixel\tlast_pixel\n";
      if (!empty) {
        layout_rows(p, gname, ax[0], 'x', W, &text[1]);
        layout_rows(p, gname, ax[1], 'y', H, &text[1]);
      }
    }
    if (wanted[0]) {
      std::vector<uint32_t> plane[4];
      std::vector<uint8_t> line[2] = {std::vector<uint8_t>(W, 0), std::vector<uint8_t>(H, 0)};
      if (!empty) {
        if (!ctx) return swg_alnstats_error(SWG_ERR_INVALID, "swg_paf_dotplot: NULL context");
        std::vector<uint64_t> off[2] = {std::vector<uint64_t>(n_seq, SWG_DOT_ABSENT), std::vector<uint64_t>(n_seq, SWG_DOT_ABSENT)};
        for (int k = 0; k < 2; ++k)
          for (const AxisSeq& e : ax[k].seqs) off[k][e.seq] = e.off;
        swg_dot_axes axes{W, H, ax[0].total, ax[1].total, off[0].data(), off[1].data()};
        swg_dot_request req{};
        req.want = 0xfu;
        for (int j = 0; j < 4; ++j) {
          plane[j].resize(size);
          req.plane[j] = plane[j].data();
        }
        const int rc = dotplot_run(ctx, rec, false, &axes, status, &req);
        if (rc != SWG_OK) return swg_alnstats_error(rc, "%s", swg_last_error(ctx));
        line[0] = genome_lines(ax[0], W);
        line[1] = genome_lines(ax[1], H);
      }
      char head[64];
      const int hl = std::snprintf(head, sizeof head, "P6\n%u %u\n255\n", W, H);
      text[0].assign(head, (size_t)hl);
      text[0].resize((size_t)hl + 3 * size, (char)255);
      if (!empty) {
        unsigned char* px = reinterpret_cast<unsigned char*>(&text[0][(size_t)hl]);
        for (uint32_t r = 0; r < H; ++r) {
          const uint32_t y = H - 1 - r;  // the origin is bottom-left
          for (uint32_t x = 0; x < W; ++x, px += 3) {
            const uint64_t at = (uint64_t)y * W + x;
            const uint64_t ap = plane[0][at], am = plane[1][at], kp = plane[2][at], km = plane[3][at];
            unsigned char rgb[3] = {255, 255, 255};
            if (kp + km > 0) {
              if (km > kp) rgb[0] = 200, rgb[1] = rgb[2] = 30;
              else rgb[0] = rgb[1] = rgb[2] = 0;
            } else if (ap + am > 0) {
              if (am > ap) rgb[0] = 245, rgb[1] = rgb[2] = 190;
              else rgb[0] = rgb[1] = rgb[2] = 190;
            } else if (line[0][x] || line[1][y]) {
              rgb[0] = 225, rgb[1] = 232, rgb[2] = 245;
            }
            px[0] = rgb[0], px[1] = rgb[1], px[2] = rgb[2];
          }
        }
      }
    }
    return texts_hand_over(text, wanted, 2, out, out_len);
  } catch (const std::bad_alloc&) {
    return swg_alnstats_error(SWG_ERR_OOM, "out of host memory");
  }
}
