// MinHash sketches, Mash distances and random haplotype pairs for `--joblist` (src/mash.rs, src/knn_graph.rs).
//
//   swg_mash_sketch ........ per contig, the bottom-s multiset of min(h_fwd, h_rev) over every window of k bytes in ACGTacgt
//                            (mash.rs:78-107).  h = DefaultHasher (SipHash-1-3, zero keys) over `<[u8] as Hash>`: le64(k)
//                            then the bytes; h_fwd over the window as it is (case kept), h_rev over its reverse complement
//                            upper-cased (mash.rs:122-131).
//   swg_mash_distances ..... all-vs-all -1/k * ln(2J / (1 + J)) over the SETS of two sketches (mash.rs:39-73), glibc ln for any
//                            double (swg_log_glibc_any: the ratio is a fraction, in glibc's near-1 branch from J = 15/17).
//   swg_mash_random_pairs .. bit j of row i (i < j) = SipHash-1-3(le64(i) || le64(j)) <= fraction * 2^64, saturated
//                            (knn_graph.rs:365-386).
//
// The sketch streams every contig through the device in chunks of MASH_CHUNK windows (k - 1 bytes of overlap between
// consecutive chunks of a contig): device memory is fixed by the chunk and by s, never by the genome.  Bytes travel
// through a two-slot pinned ring on a copy stream of their own while the previous chunk hashes.  Per chunk:
//   hash .......... one window per lane; the 1 KiB tile of the chunk sits in LDS; windows with a byte outside ACGTacgt are
//                   skipped; the value is kept when the contig's running set is not full yet or the value is below its
//                   current s-th smallest (exact: the bottom s of a multiset = the bottom s of (bottom s of a prefix) +
//                   the rest); kept values are appended after the running set (one atomic per work-group);
//   select ........ an exact MSD radix select (8 passes of 8 bits) finds the s-th smallest V of running set + candidates;
//                   every value < V and as many copies of V as are still missing form the new running set (duplicates
//                   included, as sort + truncate keeps them).  No host round trip: the counts live on the device.
// At the end of a contig the set (<= s values) is read back and sorted on the host.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include "swg_internal.h"
#include "swg_log.h"

namespace {

constexpr int MASH_THREADS = 256;
constexpr int MASH_TILE = 1024;                 // windows per work-group of the hash kernel (4 per lane)
constexpr uint64_t MASH_CHUNK = uint64_t(1) << 22;  // windows per chunk (the chunk's bytes: + k - 1)
constexpr int MASH_SEL_BLOCKS = 1024;

struct MashState {  // the first 64 bytes (everything before hist) are read back per contig
  uint64_t prefix, mask;  // radix select: the digits fixed so far
  uint64_t thr;           // s-th smallest value of the running set (valid when full)
  uint32_t k_rem;         // values still to take at the current digit
  uint32_t full;          // running set holds s values
  uint32_t take_all;      // this chunk: running set + candidates < s values, all of them stay
  uint32_t m;             // running set + candidates of this chunk
  uint32_t lt;            // append counter of the compaction
  uint32_t pad;
  uint32_t cnt[2];        // values in buffer 0 / 1
  uint32_t hist[256];
};

static_assert(offsetof(MashState, hist) <= 64, "MashState header is read back into 8 words");

__device__ __forceinline__ uint64_t rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }

struct Sip {
  uint64_t v0, v1, v2, v3;
  __device__ __forceinline__ void round() {
    v0 += v1; v2 += v3;
    v1 = rotl64(v1, 13) ^ v0; v3 = rotl64(v3, 16) ^ v2;
    v0 = rotl64(v0, 32);
    v2 += v1; v0 += v3;
    v1 = rotl64(v1, 17) ^ v2; v3 = rotl64(v3, 21) ^ v0;
    v2 = rotl64(v2, 32);
  }
  __device__ __forceinline__ void block(uint64_t m) {  // SipHash-1-3: one compression round per 8-byte block
    v3 ^= m;
    round();
    v0 ^= m;
  }
  __device__ __forceinline__ uint64_t finish() {
    v2 ^= 0xff;
    round();
    round();
    round();
    return v0 ^ v1 ^ v2 ^ v3;
  }
};

constexpr uint64_t SIP_V0 = 0x736f6d6570736575ull, SIP_V1 = 0x646f72616e646f6dull, SIP_V2 = 0x6c7967656e657261ull,
                   SIP_V3 = 0x7465646279746573ull;

// the state after the first block, le64(k): the same for every window of a call (host-side fold)
void sip_after_len(uint64_t k, uint64_t c[4]) {
  uint64_t v[4] = {SIP_V0, SIP_V1, SIP_V2, SIP_V3 ^ k};
  auto rot = [](uint64_t x, int r) { return (x << r) | (x >> (64 - r)); };
  v[0] += v[1]; v[2] += v[3];
  v[1] = rot(v[1], 13) ^ v[0]; v[3] = rot(v[3], 16) ^ v[2];
  v[0] = rot(v[0], 32);
  v[2] += v[1]; v[0] += v[3];
  v[1] = rot(v[1], 17) ^ v[2]; v[3] = rot(v[3], 21) ^ v[0];
  v[2] = rot(v[2], 32);
  v[0] ^= k;
  for (int i = 0; i < 4; ++i) c[i] = v[i];
}

__device__ __forceinline__ bool is_base(uint8_t b) {  // mash.rs:116-118 (to_ascii_uppercase in {A, C, G, T})
  const uint8_t u = b & 0xDF;
  return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
__device__ __forceinline__ uint64_t comp_upper(uint8_t b) {  // mash.rs:120-131 on a base: complement of the upper case
  const uint8_t u = b & 0xDF;
  return u == 'A' ? 'T' : u == 'C' ? 'G' : u == 'G' ? 'C' : 'A';
}

__global__ void __launch_bounds__(MASH_THREADS) mash_hash_kernel(const uint8_t* __restrict__ seq, uint64_t nwin, int k, uint64_t c0,
                                                                 uint64_t c1, uint64_t c2, uint64_t c3, uint64_t* __restrict__ out,
                                                                 MashState* st, int a) {
  __shared__ uint8_t tile[MASH_TILE + 64];
  const uint64_t base = (uint64_t)blockIdx.x * MASH_TILE;
  const uint64_t left = nwin - base;
  const uint32_t tile_bytes = (uint32_t)(left < MASH_TILE ? left : MASH_TILE) + (uint32_t)k - 1;
  for (uint32_t i = threadIdx.x; i < tile_bytes; i += MASH_THREADS) tile[i] = seq[base + i];
  __syncthreads();
  const bool full = st->full != 0;
  const uint64_t thr = st->thr;
  const int nfull = k >> 3, rem = k & 7;
  constexpr int PER = MASH_TILE / MASH_THREADS;
  uint64_t hv[PER];
  bool kp[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    const uint32_t t = (uint32_t)r * MASH_THREADS + threadIdx.x;
    kp[r] = false;
    hv[r] = 0;
    if (t < left) {
      const uint8_t* p = tile + t;
      bool ok = true;
      for (int i = 0; i < k; ++i) ok &= is_base(p[i]);
      if (ok) {
        Sip f{c0, c1, c2, c3}, rv{c0, c1, c2, c3};
        for (int w = 0; w < nfull; ++w) {
          uint64_t mf = 0, mr = 0;
#pragma unroll
          for (int b = 0; b < 8; ++b) {
            const int i = 8 * w + b;
            mf |= (uint64_t)p[i] << (8 * b);
            mr |= comp_upper(p[k - 1 - i]) << (8 * b);
          }
          f.block(mf);
          rv.block(mr);
        }
        uint64_t mf = (uint64_t)(8 + k) << 56, mr = mf;  // total length 8 + k < 256
        for (int b = 0; b < rem; ++b) {
          const int i = 8 * nfull + b;
          mf |= (uint64_t)p[i] << (8 * b);
          mr |= comp_upper(p[k - 1 - i]) << (8 * b);
        }
        f.block(mf);
        rv.block(mr);
        const uint64_t hf = f.finish(), hr = rv.finish();
        hv[r] = hf < hr ? hf : hr;
        kp[r] = !full || hv[r] < thr;
      }
    }
  }
  // one append per work-group: every window of a contig's first chunk is kept, and one counter shared by all
  // wavefronts serialises in L2 (per-wavefront atomics made this kernel 7x slower)
  constexpr int WAVES = MASH_THREADS / 64;
  __shared__ uint32_t woff[WAVES * PER];
  __shared__ uint32_t gbase;
  const int lane = (int)__lane_id(), wave = (int)(threadIdx.x / 64);
  const uint64_t below = (1ull << lane) - 1;
  uint64_t bal[PER];
#pragma unroll
  for (int r = 0; r < PER; ++r) {
    bal[r] = __ballot(kp[r]);
    if (lane == 0) woff[r * WAVES + wave] = (uint32_t)__popcll(bal[r]);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t run = 0;
    for (int q = 0; q < WAVES * PER; ++q) {
      const uint32_t c = woff[q];
      woff[q] = run;
      run += c;
    }
    gbase = run ? atomicAdd(&st->cnt[a], run) : 0;
  }
  __syncthreads();
  const uint32_t g = gbase;
#pragma unroll
  for (int r = 0; r < PER; ++r)
    if (kp[r]) out[g + woff[r * WAVES + wave] + (uint32_t)__popcll(bal[r] & below)] = hv[r];
}

__global__ void mash_reset_kernel(MashState* st) {
  st->cnt[0] = 0;
  st->cnt[1] = 0;
  st->full = 0;
  st->thr = 0;
}

__global__ void mash_sel_init_kernel(MashState* st, uint32_t s, int a) {
  const uint32_t m = st->cnt[a];
  if (threadIdx.x == 0) {
    st->m = m;
    st->take_all = m < s;
    st->k_rem = m < s ? m : s;
    st->prefix = 0;
    st->mask = 0;
    st->lt = 0;
  }
  st->hist[threadIdx.x] = 0;
}

__global__ void __launch_bounds__(256) mash_sel_hist_kernel(const uint64_t* __restrict__ buf, MashState* st, int shift) {
  if (st->take_all) return;
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t m = st->m;
  const uint64_t prefix = st->prefix, mask = st->mask;
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < m; i += gridDim.x * 256) {
    const uint64_t x = buf[i];
    if ((x & mask) == prefix) atomicAdd(&h[(x >> shift) & 255], 1u);
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

__global__ void mash_sel_pick_kernel(MashState* st, int shift) {
  if (st->take_all) return;
  __shared__ uint32_t h[256];
  h[threadIdx.x] = st->hist[threadIdx.x];
  __syncthreads();
  st->hist[threadIdx.x] = 0;
  if (threadIdx.x == 0) {
    uint32_t cum = 0;
    const uint32_t want = st->k_rem;
    for (int d = 0; d < 256; ++d) {
      if (cum + h[d] >= want) {
        st->prefix |= (uint64_t)d << shift;
        st->mask |= (uint64_t)0xff << shift;
        st->k_rem = want - cum;
        break;
      }
      cum += h[d];
    }
  }
}

__global__ void __launch_bounds__(256) mash_sel_compact_kernel(const uint64_t* __restrict__ in, uint64_t* __restrict__ out, MashState* st,
                                                               uint32_t s, int b) {
  const uint32_t m = st->m;
  const uint32_t stride = gridDim.x * 256;
  const uint32_t first = blockIdx.x * 256 + threadIdx.x;
  if (st->take_all) {
    for (uint32_t i = first; i < m; i += stride) out[i] = in[i];
    if (first == 0) st->cnt[b] = m;
    return;
  }
  const uint64_t v = st->prefix;
  const uint32_t copies = st->k_rem, below = s - copies;
  const int lane = (int)__lane_id();
  for (uint32_t base = blockIdx.x * 256; base < m; base += stride) {  // uniform bound: whole wavefronts take part
    const uint32_t i = base + threadIdx.x;
    const uint64_t x = i < m ? in[i] : 0;
    const bool take = i < m && x < v;
    const uint64_t bal = __ballot(take);
    if (!bal) continue;
    const int leader = __ffsll((unsigned long long)bal) - 1;
    uint32_t pos = 0;
    if (lane == leader) pos = atomicAdd(&st->lt, (uint32_t)__popcll(bal));  // one atomic per wavefront
    pos = (uint32_t)__shfl((int)pos, leader);
    if (take) out[pos + (uint32_t)__popcll(bal & ((1ull << lane) - 1))] = x;
  }
  for (uint32_t j = first; j < copies; j += stride) out[below + j] = v;
  if (first == 0) {
    st->cnt[b] = s;
    st->full = 1;
    st->thr = v;
  }
}

__global__ void __launch_bounds__(256) mash_dist_kernel(const uint64_t* __restrict__ sk, const uint64_t* __restrict__ cnt, uint64_t stride,
                                                        uint32_t n, int k, double* __restrict__ dist, uint32_t* __restrict__ inter_out,
                                                        uint32_t* __restrict__ union_out) {
  constexpr uint32_t LDS_B = 4096;
  __shared__ uint64_t bl[LDS_B];
  __shared__ uint32_t acc[3];
  const uint32_t i = blockIdx.y, j = blockIdx.x;
  if (j < i) return;
  const uint64_t* A = sk + (uint64_t)i * stride;
  const uint64_t* Bg = sk + (uint64_t)j * stride;
  const uint32_t na = (uint32_t)cnt[i], nb = (uint32_t)cnt[j];
  if (threadIdx.x < 3) acc[threadIdx.x] = 0;
  const bool staged = nb <= LDS_B;
  if (staged)
    for (uint32_t t = threadIdx.x; t < nb; t += 256) bl[t] = Bg[t];
  __syncthreads();
  const uint64_t* B = staged ? bl : Bg;
  // the SETS of both sketches (mash.rs:43-47): a value counts once however often it repeats
  uint32_t inter = 0, da = 0, db = 0;
  for (uint32_t t = threadIdx.x; t < na; t += 256) {
    const uint64_t x = A[t];
    if (t && A[t - 1] == x) continue;
    ++da;
    uint32_t lo = 0, hi = nb;
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (B[mid] < x) lo = mid + 1; else hi = mid;
    }
    inter += lo < nb && B[lo] == x;
  }
  for (uint32_t t = threadIdx.x; t < nb; t += 256) db += (t == 0 || B[t - 1] != B[t]);
  if (inter) atomicAdd(&acc[0], inter);
  if (da) atomicAdd(&acc[1], da);
  if (db) atomicAdd(&acc[2], db);
  __syncthreads();
  if (threadIdx.x) return;
  const uint32_t in = acc[0], un = acc[1] + acc[2] - acc[0];
  double d = 0.0;
  if (i != j) {
    const double jac = un == 0 ? 0.0 : (double)in / (double)un;
    if (jac <= 0.0) {
      d = 1.0;
    } else {
      const double ratio = __dmul_rn(2.0, jac) / __dadd_rn(1.0, jac);  // no contraction: the reference's operation order
      d = ratio <= 0.0 ? 1.0 : __dmul_rn(-1.0 / (double)k, swg_log_glibc_any(ratio));  // a fraction: glibc's near-1 branch from J = 15/17
    }
  }
  dist[(uint64_t)i * n + j] = d;
  dist[(uint64_t)j * n + i] = d;
  if (inter_out) inter_out[(uint64_t)i * n + j] = inter_out[(uint64_t)j * n + i] = in;
  if (union_out) union_out[(uint64_t)i * n + j] = union_out[(uint64_t)j * n + i] = un;
}

__global__ void __launch_bounds__(256) mash_random_kernel(uint64_t n, uint64_t thr, uint64_t row0, uint64_t words, uint64_t wpr,
                                                          uint64_t* __restrict__ mask) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= words) return;
  const uint64_t i = row0 + t / wpr, j0 = (t % wpr) * 64;
  uint64_t word = 0;
  for (int b = 0; b < 64; ++b) {
    const uint64_t j = j0 + b;
    if (j <= i || j >= n) continue;
    Sip s{SIP_V0, SIP_V1, SIP_V2, SIP_V3};  // DefaultHasher: write_usize(i), write_usize(j)
    s.block(i);
    s.block(j);
    s.block(uint64_t(16) << 56);
    if (s.finish() <= thr) word |= uint64_t(1) << b;
  }
  mask[t] = word;
}

// device and host resources of one sketch call, released on every path
struct MashCall {
  swg_ctx* ctx;
  hipStream_t copy = nullptr;
  hipEvent_t copied[2] = {nullptr, nullptr}, used[2] = {nullptr, nullptr};
  uint8_t* pinned = nullptr;
  uint64_t* h_out = nullptr;
  uint8_t* d_seq = nullptr;
  uint64_t* d_buf = nullptr;
  MashState* d_st = nullptr;
  std::vector<hipEvent_t> tev;  // timing events, 6 per chunk of the longest contig so far
  ~MashCall() {
    if (copy) (void)hipStreamSynchronize(copy);
    if (ctx && ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (auto e : tev) (void)hipEventDestroy(e);
    for (int i = 0; i < 2; ++i) {
      if (copied[i]) (void)hipEventDestroy(copied[i]);
      if (used[i]) (void)hipEventDestroy(used[i]);
    }
    if (copy) (void)hipStreamDestroy(copy);
    if (pinned) (void)hipHostFree(pinned);
    if (h_out) (void)hipHostFree(h_out);
    if (d_seq) (void)hipFree(d_seq);
    if (d_buf) (void)hipFree(d_buf);
    if (d_st) (void)hipFree(d_st);
  }
};

}  // namespace

// Internal entry (also behind swg_joblist): calls emit(i, values, count) once per contig in order, values ascending.
int swg_mash_sketch_each(swg_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seq, int k, uint64_t s,
                         void (*emit)(void*, uint64_t, const uint64_t*, uint64_t), void* user, double* timing_ms) {
  if (!ctx) return swg_set_error(nullptr, SWG_ERR_NO_DEVICE, "swg_mash_sketch: no context (no usable HIP device)");
  if (k < 1 || k > 64 || s < 1 || s > 65536)
    return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "mash sketch: k must be in 1..64 and the sketch size in 1..65536 (got k=%d, s=%llu)",
                         k, (unsigned long long)s);
  if (n_seq && (!offsets || !emit)) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_sketch: NULL argument");
  for (uint64_t i = 0; i < n_seq; ++i)
    if (offsets[i + 1] < offsets[i]) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_sketch: offsets not ascending");
  if (n_seq && offsets[n_seq] > offsets[0] && !seq) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_sketch: NULL sequence");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  const auto w0 = std::chrono::steady_clock::now();
  double t_h2d = 0.0, t_hash = 0.0, t_sel = 0.0;
  uint64_t kmers = 0;
  MashCall c{ctx};
  const uint64_t chunk_bytes = MASH_CHUNK + 64;
  const uint64_t cap = s + MASH_CHUNK;
  // events and streams first, then memory: a failure leaves nothing half set up (the destructor frees what exists)
  for (int i = 0; i < 2; ++i) {
    SWG_HIP(ctx, hipEventCreateWithFlags(&c.copied[i], hipEventDisableTiming));
    SWG_HIP(ctx, hipEventCreateWithFlags(&c.used[i], hipEventDisableTiming));
  }
  SWG_HIP(ctx, hipStreamCreateWithFlags(&c.copy, hipStreamNonBlocking));
  SWG_HIP(ctx, hipHostMalloc((void**)&c.pinned, 2 * chunk_bytes, hipHostMallocDefault));
  SWG_HIP(ctx, hipHostMalloc((void**)&c.h_out, (s + 8) * sizeof(uint64_t), hipHostMallocDefault));
  SWG_HIP(ctx, hipMalloc((void**)&c.d_seq, 2 * chunk_bytes));
  SWG_HIP(ctx, hipMalloc((void**)&c.d_buf, 2 * cap * sizeof(uint64_t)));
  SWG_HIP(ctx, hipMalloc((void**)&c.d_st, sizeof(MashState)));
  uint64_t sc[4];
  sip_after_len((uint64_t)k, sc);
  const hipStream_t st = ctx->stream;
  bool slot_copied[2] = {false, false}, slot_used[2] = {false, false};
  uint64_t chunk_no = 0;
  std::vector<uint64_t> vals;
  for (uint64_t ci = 0; ci < n_seq; ++ci) {
    const uint64_t len = offsets[ci + 1] - offsets[ci];
    if (len < (uint64_t)k) {  // mash.rs:79-81
      emit(user, ci, nullptr, 0);
      continue;
    }
    const uint64_t nwin = len - (uint64_t)k + 1;
    const uint64_t nchunks = (nwin + MASH_CHUNK - 1) / MASH_CHUNK;
    if (timing_ms && c.tev.size() < 6 * nchunks) {
      const size_t old = c.tev.size();
      c.tev.resize(6 * nchunks, nullptr);
      for (size_t e = old; e < c.tev.size(); ++e) SWG_HIP(ctx, hipEventCreate(&c.tev[e]));
    }
    SWG_LAUNCH(ctx, "mash_reset", mash_reset_kernel<<<1, 1, 0, st>>>(c.d_st));
    SWG_KERNEL_CHECK(ctx);
    int a = 0;
    for (uint64_t q = 0; q < nchunks; ++q, ++chunk_no) {
      const int slot = (int)(chunk_no & 1);
      const uint64_t w_begin = q * MASH_CHUNK;
      const uint64_t w_n = std::min(MASH_CHUNK, nwin - w_begin);
      const uint64_t bytes = w_n + (uint64_t)k - 1;
      uint8_t* hslot = c.pinned + slot * chunk_bytes;
      uint8_t* dslot = c.d_seq + slot * chunk_bytes;
      // the pinned slot is free once its previous copy has landed; the device slot once the hash that read it has run
      if (slot_copied[slot]) SWG_HIP(ctx, hipEventSynchronize(c.copied[slot]));
      std::memcpy(hslot, seq + offsets[ci] + w_begin, bytes);
      if (slot_used[slot]) SWG_HIP(ctx, hipStreamWaitEvent(c.copy, c.used[slot], 0));
      hipEvent_t* te = timing_ms ? &c.tev[6 * q] : nullptr;
      if (te) SWG_HIP(ctx, hipEventRecord(te[0], c.copy));
      SWG_HIP(ctx, hipMemcpyAsync(dslot, hslot, bytes, hipMemcpyHostToDevice, c.copy));
      if (te) SWG_HIP(ctx, hipEventRecord(te[1], c.copy));
      SWG_HIP(ctx, hipEventRecord(c.copied[slot], c.copy));
      slot_copied[slot] = true;
      SWG_HIP(ctx, hipStreamWaitEvent(st, c.copied[slot], 0));
      uint64_t* buf_a = c.d_buf + (uint64_t)a * cap;
      uint64_t* buf_b = c.d_buf + (uint64_t)(1 - a) * cap;
      if (te) SWG_HIP(ctx, hipEventRecord(te[2], st));
      const unsigned grid = (unsigned)((w_n + MASH_TILE - 1) / MASH_TILE);
      SWG_LAUNCH_N(ctx, "mash_hash", w_n,
                   mash_hash_kernel<<<grid, MASH_THREADS, 0, st>>>(dslot, w_n, k, sc[0], sc[1], sc[2], sc[3], buf_a, c.d_st, a));
      SWG_KERNEL_CHECK(ctx);
      if (te) SWG_HIP(ctx, hipEventRecord(te[3], st));
      SWG_HIP(ctx, hipEventRecord(c.used[slot], st));
      slot_used[slot] = true;
      // bottom s of running set + candidates -> the other buffer
      SWG_LAUNCH(ctx, "mash_sel_init", mash_sel_init_kernel<<<1, 256, 0, st>>>(c.d_st, (uint32_t)s, a));
      SWG_KERNEL_CHECK(ctx);
      const unsigned sel_grid = (unsigned)std::min<uint64_t>(MASH_SEL_BLOCKS, (s + w_n + 255) / 256);
      for (int shift = 56; shift >= 0; shift -= 8) {
        SWG_LAUNCH(ctx, "mash_sel_hist", mash_sel_hist_kernel<<<sel_grid, 256, 0, st>>>(buf_a, c.d_st, shift));
        SWG_KERNEL_CHECK(ctx);
        SWG_LAUNCH(ctx, "mash_sel_pick", mash_sel_pick_kernel<<<1, 256, 0, st>>>(c.d_st, shift));
        SWG_KERNEL_CHECK(ctx);
      }
      SWG_LAUNCH(ctx, "mash_sel_compact", mash_sel_compact_kernel<<<sel_grid, 256, 0, st>>>(buf_a, buf_b, c.d_st, (uint32_t)s, 1 - a));
      SWG_KERNEL_CHECK(ctx);
      if (te) SWG_HIP(ctx, hipEventRecord(te[4], st));
      a = 1 - a;
      kmers += w_n;
    }
    SWG_HIP(ctx, hipMemcpyAsync(c.h_out, c.d_st, offsetof(MashState, hist), hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipMemcpyAsync(c.h_out + 8, c.d_buf + (uint64_t)a * cap, s * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipStreamSynchronize(st));
    MashState hs;
    std::memcpy(&hs, c.h_out, offsetof(MashState, hist));
    const uint64_t n_out = hs.cnt[a];
    if (n_out > s) return swg_set_error(ctx, SWG_ERR_HIP, "mash sketch: device set of %llu values > s", (unsigned long long)n_out);
    vals.assign(c.h_out + 8, c.h_out + 8 + n_out);
    std::sort(vals.begin(), vals.end());
    if (timing_ms) {
      for (uint64_t q = 0; q < nchunks; ++q) {
        float ms = 0.f;
        hipEvent_t* te = &c.tev[6 * q];
        if (hipEventElapsedTime(&ms, te[0], te[1]) == hipSuccess) t_h2d += ms;
        if (hipEventElapsedTime(&ms, te[2], te[3]) == hipSuccess) t_hash += ms;
        if (hipEventElapsedTime(&ms, te[3], te[4]) == hipSuccess) t_sel += ms;
      }
    }
    emit(user, ci, vals.data(), vals.size());
  }
  if (timing_ms) {
    timing_ms[0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
    timing_ms[1] = t_h2d;
    timing_ms[2] = t_hash;
    timing_ms[3] = t_sel;
    timing_ms[4] = (double)kmers;
  }
  return SWG_OK;
}

namespace {
struct RowsOut {
  uint64_t* counts;
  uint64_t* mins;
  uint64_t s;
};
void emit_rows(void* u, uint64_t i, const uint64_t* v, uint64_t n) {
  RowsOut* r = static_cast<RowsOut*>(u);
  r->counts[i] = n;
  if (n) std::memcpy(r->mins + i * r->s, v, n * sizeof(uint64_t));
}
}  // namespace

extern "C" int swg_mash_sketch(swg_ctx* ctx, const uint8_t* seq, const uint64_t* offsets, uint64_t n_seq, int k, uint64_t s,
                               uint64_t* counts_out, uint64_t* minimizers_out, double* timing_ms) {
  if (n_seq && (!counts_out || !minimizers_out)) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_sketch: NULL output");
  RowsOut r{counts_out, minimizers_out, s};
  return swg_mash_sketch_each(ctx, seq, offsets, n_seq, k, s, emit_rows, &r, timing_ms);
}

extern "C" int swg_mash_distances(swg_ctx* ctx, const uint64_t* sketches, const uint64_t* counts, uint64_t stride, uint64_t n, int k,
                                  double* dist_out, uint32_t* inter_out, uint32_t* union_out) {
  if (!ctx) return swg_set_error(nullptr, SWG_ERR_NO_DEVICE, "swg_mash_distances: no context (no usable HIP device)");
  if (k < 1 || k > 64) return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "mash distances: k must be in 1..64 (got %d)", k);
  if (n > 65535) return swg_set_error(ctx, SWG_ERR_UNSUPPORTED, "mash distances: more than 65535 sketches");
  if (n == 0) return SWG_OK;
  if (!sketches || !counts || !dist_out) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_distances: NULL argument");
  for (uint64_t i = 0; i < n; ++i)
    if (counts[i] > stride || counts[i] > UINT32_MAX / 2)
      return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_distances: sketch %llu holds more values than its row", (unsigned long long)i);
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  uint64_t *d_sk = nullptr, *d_cnt = nullptr;
  double* d_dist = nullptr;
  uint32_t *d_in = nullptr, *d_un = nullptr;
  struct Free {
    std::vector<void*> p;
    ~Free() {
      for (void* q : p) (void)hipFree(q);
    }
  } fr;
  auto dmalloc = [&](void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes ? bytes : 8);
    if (e == hipSuccess) fr.p.push_back(*p);
    return e;
  };
  SWG_HIP(ctx, dmalloc((void**)&d_sk, n * stride * sizeof(uint64_t)));
  SWG_HIP(ctx, dmalloc((void**)&d_cnt, n * sizeof(uint64_t)));
  SWG_HIP(ctx, dmalloc((void**)&d_dist, n * n * sizeof(double)));
  if (inter_out) SWG_HIP(ctx, dmalloc((void**)&d_in, n * n * sizeof(uint32_t)));
  if (union_out) SWG_HIP(ctx, dmalloc((void**)&d_un, n * n * sizeof(uint32_t)));
  SWG_HIP(ctx, hipMemcpyAsync(d_sk, sketches, n * stride * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  SWG_HIP(ctx, hipMemcpyAsync(d_cnt, counts, n * sizeof(uint64_t), hipMemcpyHostToDevice, st));
  SWG_LAUNCH_N(ctx, "mash_dist", n * n, mash_dist_kernel<<<dim3((unsigned)n, (unsigned)n), 256, 0, st>>>(d_sk, d_cnt, stride, (uint32_t)n, k, d_dist, d_in, d_un));
  SWG_KERNEL_CHECK(ctx);
  SWG_HIP(ctx, hipMemcpyAsync(dist_out, d_dist, n * n * sizeof(double), hipMemcpyDeviceToHost, st));
  if (inter_out) SWG_HIP(ctx, hipMemcpyAsync(inter_out, d_in, n * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (union_out) SWG_HIP(ctx, hipMemcpyAsync(union_out, d_un, n * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  SWG_HIP(ctx, hipStreamSynchronize(st));
  return SWG_OK;
}

// (f * u64::MAX as f64) as u64: u64::MAX rounds to 2^64; the cast saturates, NaN -> 0 (knn_graph.rs:368)
uint64_t swg_mash_random_threshold(double fraction) {
  const double t = fraction * 18446744073709551616.0;
  if (!(t > 0.0)) return 0;
  if (t >= 18446744073709551616.0) return UINT64_MAX;
  return (uint64_t)t;
}

extern "C" int swg_mash_random_pairs(swg_ctx* ctx, uint64_t n, double fraction, uint64_t row_begin, uint64_t row_end, uint64_t* mask_out) {
  if (!ctx) return swg_set_error(nullptr, SWG_ERR_NO_DEVICE, "swg_mash_random_pairs: no context (no usable HIP device)");
  if (row_begin > row_end || row_end > n) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_random_pairs: bad row range");
  if (row_end == row_begin) return SWG_OK;
  if (!mask_out) return swg_set_error(ctx, SWG_ERR_INVALID, "swg_mash_random_pairs: NULL output");
  SWG_HIP(ctx, hipSetDevice(ctx->device));
  const hipStream_t st = ctx->stream;
  const uint64_t wpr = (n + 63) / 64;
  const uint64_t thr = swg_mash_random_threshold(fraction);
  const uint64_t max_words = std::max<uint64_t>(wpr, uint64_t(8) << 20);  // <= 64 MiB of device words per launch (one row at least)
  const uint64_t rows_per = max_words / wpr;
  uint64_t* d_mask = nullptr;
  SWG_HIP(ctx, hipMalloc((void**)&d_mask, rows_per * wpr * sizeof(uint64_t)));
  struct Free {
    void* p;
    ~Free() { (void)hipFree(p); }
  } fr{d_mask};
  for (uint64_t r0 = row_begin; r0 < row_end; r0 += rows_per) {
    const uint64_t rows = std::min(rows_per, row_end - r0);
    const uint64_t words = rows * wpr;
    SWG_LAUNCH_N(ctx, "mash_random", words,
                 mash_random_kernel<<<(unsigned)((words + 255) / 256), 256, 0, st>>>(n, thr, r0, words, wpr, d_mask));
    SWG_KERNEL_CHECK(ctx);
    SWG_HIP(ctx, hipMemcpyAsync(mask_out + (r0 - row_begin) * wpr, d_mask, words * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
    SWG_HIP(ctx, hipStreamSynchronize(st));
  }
  return SWG_OK;
}
