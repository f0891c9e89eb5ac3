// Runs the scan, compaction and radix-sort primitives of csrc/swg_sort.hip on their own, one case after another in one process
// and one context (a GPU box tool; tests/test_gpu_primitives_native.py writes the cases and checks every output against
// tests/prim_model.py -- this file holds no reference logic):
//   prim_check <case list> <directory>
// The case list is text, one case per line: `<name> <operation> key=value ...`.  Inputs are raw little-endian arrays in
// <directory> (in=<file>: elements / flags / keys / words, in1=<file>: the sort's values); the outputs of a case go to
// <directory>/<name>.<what> and one line per case goes to stdout:
//   case <name> rc=<return code> guards=<ok | the broken ones> files=<comma-separated output files>
// Every buffer a primitive writes is allocated with 64 bytes of 0xa5 in front of and behind its elements (and in front of an
// element offset, in_off / out_off, which moves the pointer off its 16-byte alignment); `guards` says whether those bytes
// survived.  For `compact` the guard behind the list starts behind the `total` entries the count reported.
// The first HIP error ends the run: the case's name on stderr, exit status 2, nothing more is launched.
//   operations: scan_excl_sum_u32 scan_incl_max_u32 scan_incl_max_u64 scan_incl_sum_u64   n in_off out_off in_place want_total
//               compact                                                                  n in_off (bytes)
//               sort_pairs    n begin_bit end_bit use_prehist
//               sort_packed   n key_bits val_bits identity_vals use_prehist
//               sort_words    n sorted_bits val_bits use_prehist
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_internal.h"

namespace {

constexpr size_t GUARD = 64;
constexpr uint8_t POISON = 0xa5;

// An error ends the process on the spot (no unwinding: after a HIP error nothing more may touch the device).
std::string g_case = "(start)";
[[noreturn]] void die(int status, const std::string& what) {
  fflush(stdout);
  fprintf(stderr, "case %s: %s\n", g_case.c_str(), what.c_str());
  fflush(stderr);
  _Exit(status);
}
#define CK(x)                                                                                  \
  do {                                                                                         \
    hipError_t e_ = (x);                                                                       \
    if (e_ != hipSuccess) die(2, std::string("HIP error: " #x ": ") + hipGetErrorString(e_));  \
  } while (0)

// The digit histograms of a sort the way the library's callers accumulate them while they write the keys.
__global__ __launch_bounds__(256) void prehist_kernel(const uint64_t* __restrict__ keys, uint64_t n, swg_radix_plan plan,
                                                       uint32_t* __restrict__ ghist) {
  __shared__ uint32_t h[SWG_RADIX_MAX_PASSES][SWG_RADIX_BINS];
  swg_radix_hist_zero(h, plan.npasses);
  __syncthreads();
  for (uint64_t base = (uint64_t)blockIdx.x * blockDim.x; base < n; base += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t i = base + threadIdx.x;
    const bool valid = i < n;
    swg_radix_hist_add(h, valid ? keys[i] : 0ull, valid, plan);
  }
  __syncthreads();
  swg_radix_hist_flush(h, plan.npasses, ghist);
}

// A device buffer of `bytes` payload bytes `off` bytes into a 16-byte-aligned block, poison all round.
struct guarded {
  swg_ctx* ctx;
  char* base = nullptr;
  size_t off, bytes;
  std::vector<uint8_t> host;  // image of the whole allocation (before: what is uploaded; after fetch(): what came back)
  guarded(swg_ctx* c, size_t off_bytes, size_t payload) : ctx(c), off(off_bytes), bytes(payload), host(2 * GUARD + off_bytes + payload, POISON) {
    CK(hipMalloc(&base, host.size()));
  }
  ~guarded() {
    if (base) (void)hipFree(base);
  }
  guarded(const guarded&) = delete;
  guarded& operator=(const guarded&) = delete;
  char* ptr() const { return base + GUARD + off; }
  uint8_t* data() { return host.data() + GUARD + off; }
  void upload() {
    CK(hipMemcpyAsync(base, host.data(), host.size(), hipMemcpyHostToDevice, ctx->stream));
    CK(hipStreamSynchronize(ctx->stream));
  }
  void fetch() { CK(hipMemcpy(host.data(), base, host.size(), hipMemcpyDeviceToHost)); }
  // every byte outside [ptr, ptr + used) still poison?  (front: everything before the payload; back: everything behind `used`)
  bool front_ok() const {
    for (size_t i = 0; i < GUARD + off; ++i)
      if (host[i] != POISON) return false;
    return true;
  }
  bool back_ok(size_t used) const {
    for (size_t i = GUARD + off + used; i < host.size(); ++i)
      if (host[i] != POISON) return false;
    return true;
  }
};

struct run_case {
  std::string name, op;
  std::map<std::string, std::string> kv;
  long long num(const char* k, long long dflt = 0) const {
    auto it = kv.find(k);
    return it == kv.end() ? dflt : atoll(it->second.c_str());
  }
  std::string str(const char* k) const {
    auto it = kv.find(k);
    return it == kv.end() ? std::string() : it->second;
  }
};

void read_file(const std::string& path, void* dst, size_t bytes) {
  if (bytes == 0) return;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) die(3, "cannot open " + path);
  const size_t got = fread(dst, 1, bytes, f);
  fclose(f);
  if (got != bytes) die(3, path + " is shorter than the case needs");
}
void write_file(const std::string& path, const void* src, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f) die(3, "cannot create " + path);
  const size_t put = bytes ? fwrite(src, 1, bytes, f) : 0;
  if (fclose(f) != 0 || put != bytes) die(3, "short write to " + path);
}

struct report {
  int rc = 0;
  std::vector<std::string> bad_guards, files;
  void guard(const char* which, bool ok) {
    if (!ok) bad_guards.push_back(which);
  }
};

void sync_and_check(swg_ctx* ctx) {
  CK(hipStreamSynchronize(ctx->stream));
  CK(hipDeviceSynchronize());
  CK(hipGetLastError());
}

template <typename T, typename F>
void run_scan(swg_ctx* ctx, const run_case& c, const std::string& dir, report& rep, F&& call) {
  const uint64_t n = (uint64_t)c.num("n");
  const size_t in_off = (size_t)c.num("in_off") * sizeof(T), out_off = (size_t)c.num("out_off") * sizeof(T);
  const bool in_place = c.num("in_place") != 0, want_total = c.num("want_total") != 0;
  guarded in(ctx, in_off, n * sizeof(T));
  read_file(dir + "/" + c.str("in"), in.data(), n * sizeof(T));
  in.upload();
  guarded separate(ctx, out_off, in_place ? 0 : n * sizeof(T));
  separate.upload();
  guarded* out = in_place ? &in : &separate;
  guarded total(ctx, 0, sizeof(uint64_t));
  total.upload();
  {
    rep.rc = call(reinterpret_cast<const T*>(in.ptr()), reinterpret_cast<T*>(out->ptr()), n,
                  want_total ? reinterpret_cast<uint64_t*>(total.ptr()) : nullptr);
    if (rep.rc == SWG_ERR_HIP) die(2, std::string("HIP error: ") + swg_last_error(ctx));
    sync_and_check(ctx);
    if (rep.rc == SWG_OK) {
      out->fetch();
      total.fetch();
      rep.guard("out_front", out->front_ok());
      rep.guard("out_back", out->back_ok(n * sizeof(T)));
      rep.guard("total_front", total.front_ok());
      rep.guard("total_back", total.back_ok(want_total ? sizeof(uint64_t) : 0));
      if (!in_place) {  // the input is the primitive's to read only
        in.fetch();
        std::vector<uint8_t> again(n * sizeof(T));
        read_file(dir + "/" + c.str("in"), again.data(), again.size());
        rep.guard("input_intact", in.front_ok() && in.back_ok(n * sizeof(T)) && memcmp(in.data(), again.data(), again.size()) == 0);
      }
      write_file(dir + "/" + c.name + ".out", out->data(), n * sizeof(T));
      rep.files.push_back(c.name + ".out");
      if (want_total) {
        write_file(dir + "/" + c.name + ".total", total.data(), sizeof(uint64_t));
        rep.files.push_back(c.name + ".total");
      }
    }
  }
}

void run_compact(swg_ctx* ctx, const run_case& c, const std::string& dir, report& rep) {
  const uint64_t n = (uint64_t)c.num("n");
  guarded flags(ctx, (size_t)c.num("in_off"), n);
  read_file(dir + "/" + c.str("in"), flags.data(), n);
  flags.upload();
  guarded list(ctx, 0, n * sizeof(uint32_t));
  list.upload();
  guarded total(ctx, 0, sizeof(uint64_t));
  total.upload();
  swg_flag_scan fs{};
  rep.rc = swg_flags_count(ctx, reinterpret_cast<const uint8_t*>(flags.ptr()), n, &fs, reinterpret_cast<uint64_t*>(total.ptr()));
  if (rep.rc == SWG_OK) rep.rc = swg_flags_compact(ctx, fs, reinterpret_cast<uint32_t*>(list.ptr()));
  if (rep.rc == SWG_ERR_HIP) die(2, std::string("HIP error: ") + swg_last_error(ctx));
  sync_and_check(ctx);
  if (rep.rc != SWG_OK) return;
  const uint64_t nb = (n + 4095) / 4096;
  std::vector<uint32_t> tile_off(nb);
  if (nb) CK(hipMemcpy(tile_off.data(), fs.tile_off, nb * sizeof(uint32_t), hipMemcpyDeviceToHost));
  list.fetch();
  total.fetch();
  uint64_t t = 0;
  memcpy(&t, total.data(), sizeof t);
  rep.guard("list_front", list.front_ok());
  rep.guard("list_back", list.back_ok((size_t)(t < n ? t : n) * sizeof(uint32_t)));
  rep.guard("total_front", total.front_ok());
  rep.guard("total_back", total.back_ok(sizeof(uint64_t)));
  write_file(dir + "/" + c.name + ".list", list.data(), n * sizeof(uint32_t));  // all n slots: the unused ones keep the poison
  write_file(dir + "/" + c.name + ".total", total.data(), sizeof(uint64_t));
  write_file(dir + "/" + c.name + ".tile_off", tile_off.data(), nb * sizeof(uint32_t));
  rep.files = {c.name + ".list", c.name + ".total", c.name + ".tile_off"};
}

// [SWG_RADIX_MAX_PASSES][SWG_RADIX_BINS] histograms of `plan` over the n device words at `keys`
uint32_t* make_prehist(swg_ctx* ctx, const uint64_t* keys, uint64_t n, const swg_radix_plan& plan) {
  uint32_t* h = nullptr;
  const size_t bytes = sizeof(uint32_t) * SWG_RADIX_MAX_PASSES * SWG_RADIX_BINS;
  CK(hipMalloc(&h, bytes));
  CK(hipMemsetAsync(h, 0, bytes, ctx->stream));
  const uint64_t blocks = (n + 255) / 256;
  prehist_kernel<<<(unsigned)(blocks < 64 ? (blocks ? blocks : 1) : 64), 256, 0, ctx->stream>>>(keys, n, plan, h);
  CK(hipGetLastError());
  return h;
}

void run_sort(swg_ctx* ctx, const run_case& c, const std::string& dir, report& rep) {
  const uint64_t n = (uint64_t)c.num("n");
  const int val_bits = (int)c.num("val_bits");
  const bool use_prehist = c.num("use_prehist") != 0;
  guarded keys(ctx, 0, n * 8), keys_alt(ctx, 0, n * 8);
  read_file(dir + "/" + c.str("in"), keys.data(), n * 8);
  keys.upload();
  keys_alt.upload();
  uint32_t* prehist = nullptr;
  struct free_later {
    uint32_t*& p;
    ~free_later() {
      if (p) (void)hipFree(p);
    }
  } fl{prehist};
  uint64_t* k0 = reinterpret_cast<uint64_t*>(keys.ptr());
  uint64_t* k1 = reinterpret_cast<uint64_t*>(keys_alt.ptr());
  if (c.op == "sort_pairs") {
    const int begin_bit = (int)c.num("begin_bit"), end_bit = (int)c.num("end_bit");
    guarded vals(ctx, 0, n * 4), vals_alt(ctx, 0, n * 4);
    read_file(dir + "/" + c.str("in1"), vals.data(), n * 4);
    vals.upload();
    vals_alt.upload();
    uint32_t* v0 = reinterpret_cast<uint32_t*>(vals.ptr());
    uint32_t* v1 = reinterpret_cast<uint32_t*>(vals_alt.ptr());
    if (use_prehist) prehist = make_prehist(ctx, k0, n, swg_radix_plan_pairs(begin_bit, end_bit));
    rep.rc = swg_radix_sort_pairs(ctx, &k0, &v0, &k1, &v1, n, begin_bit, end_bit, prehist);
    if (rep.rc == SWG_ERR_HIP) die(2, std::string("HIP error: ") + swg_last_error(ctx));
    sync_and_check(ctx);
    if (rep.rc != SWG_OK) return;
    keys.fetch(), keys_alt.fetch(), vals.fetch(), vals_alt.fetch();
    rep.guard("keys_front", keys.front_ok());
    rep.guard("keys_back", keys.back_ok(n * 8));
    rep.guard("keys_alt_front", keys_alt.front_ok());
    rep.guard("keys_alt_back", keys_alt.back_ok(n * 8));
    rep.guard("vals_front", vals.front_ok());
    rep.guard("vals_back", vals.back_ok(n * 4));
    rep.guard("vals_alt_front", vals_alt.front_ok());
    rep.guard("vals_alt_back", vals_alt.back_ok(n * 4));
    guarded& ko = k0 == reinterpret_cast<uint64_t*>(keys.ptr()) ? keys : keys_alt;  // the pointers come back swapped or not
    guarded& vo = v0 == reinterpret_cast<uint32_t*>(vals.ptr()) ? vals : vals_alt;
    write_file(dir + "/" + c.name + ".keys", ko.data(), n * 8);
    write_file(dir + "/" + c.name + ".vals", vo.data(), n * 4);
    rep.files = {c.name + ".keys", c.name + ".vals"};
    return;
  }
  uint64_t* out = nullptr;
  const bool identity = c.op != "sort_packed" || c.num("identity_vals") != 0;
  guarded vals(ctx, 0, identity ? 0 : n * 4);  // (lives until the sort has run)
  if (c.op == "sort_packed") {
    const int key_bits = (int)c.num("key_bits");
    if (!identity) read_file(dir + "/" + c.str("in1"), vals.data(), n * 4);
    vals.upload();
    if (use_prehist) prehist = make_prehist(ctx, k0, n, swg_radix_plan_packed(key_bits));
    rep.rc = swg_radix_sort_packed(ctx, k0, identity ? nullptr : reinterpret_cast<const uint32_t*>(vals.ptr()), k1, n, key_bits, val_bits,
                                   prehist, &out);
  } else {  // sort_words
    const int sorted_bits = (int)c.num("sorted_bits");
    if (use_prehist) {  // the digits sit val_bits up in the words
      swg_radix_plan wp = swg_radix_plan_words(sorted_bits);
      for (int p = 0; p < wp.npasses; ++p) wp.shift[p] = (uint8_t)(wp.shift[p] + val_bits);
      prehist = make_prehist(ctx, k0, n, wp);
    }
    rep.rc = swg_radix_sort_words(ctx, k0, k1, n, sorted_bits, val_bits, prehist, &out);
  }
  if (rep.rc == SWG_ERR_HIP) die(2, std::string("HIP error: ") + swg_last_error(ctx));
  sync_and_check(ctx);
  if (rep.rc != SWG_OK) return;
  keys.fetch(), keys_alt.fetch();
  rep.guard("keys_front", keys.front_ok());
  rep.guard("keys_back", keys.back_ok(n * 8));
  rep.guard("scratch_front", keys_alt.front_ok());
  rep.guard("scratch_back", keys_alt.back_ok(n * 8));
  if (out != k0 && out != k1) {
    rep.guard("out_is_neither_buffer", false);
    return;
  }
  write_file(dir + "/" + c.name + ".words", (out == k0 ? keys : keys_alt).data(), n * 8);
  rep.files = {c.name + ".words"};
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) {
    fprintf(stderr, "usage: prim_check <case list> <directory>\n");
    return 3;
  }
  const std::string dir = argv[2];
  std::vector<run_case> cases;
  {
    std::ifstream f(argv[1]);
    if (!f) {
      fprintf(stderr, "cannot open %s\n", argv[1]);
      return 3;
    }
    std::string line;
    while (std::getline(f, line)) {
      std::istringstream ss(line);
      run_case c;
      if (!(ss >> c.name >> c.op)) continue;
      std::string tok;
      while (ss >> tok) {
        const size_t eq = tok.find('=');
        if (eq == std::string::npos) {
          fprintf(stderr, "%s: '%s' is not key=value\n", c.name.c_str(), tok.c_str());
          return 3;
        }
        c.kv[tok.substr(0, eq)] = tok.substr(eq + 1);
      }
      cases.push_back(c);
    }
  }
  uint64_t max_n = 0;
  for (const run_case& c : cases) max_n = std::max<uint64_t>(max_n, (uint64_t)c.num("n"));
  swg_ctx* ctx = nullptr;
  if (swg_create(0, &ctx) != SWG_OK) {
    fprintf(stderr, "swg_create: %s\n", swg_last_error(nullptr));
    return 2;
  }
  if (swg_arena_reserve(ctx, (size_t(256) << 20) + max_n / 8) != SWG_OK) {
    fprintf(stderr, "swg_arena_reserve: %s\n", swg_last_error(ctx));
    return 2;
  }
  for (const run_case& c : cases) {
    report rep;
    swg_arena_reset(ctx);
    g_case = c.name;
    {
      if (c.op == "scan_excl_sum_u32")
        run_scan<uint32_t>(ctx, c, dir, rep, [&](const uint32_t* in, uint32_t* out, uint64_t n, uint64_t* tot) {
          return swg_exclusive_scan_u32(ctx, in, out, n, tot);
        });
      else if (c.op == "scan_incl_max_u32")
        run_scan<uint32_t>(ctx, c, dir, rep, [&](const uint32_t* in, uint32_t* out, uint64_t n, uint64_t*) {
          return swg_inclusive_max_scan_u32(ctx, in, out, n);
        });
      else if (c.op == "scan_incl_max_u64")
        run_scan<uint64_t>(ctx, c, dir, rep, [&](const uint64_t* in, uint64_t* out, uint64_t n, uint64_t*) {
          return swg_inclusive_max_scan_u64(ctx, in, out, n);
        });
      else if (c.op == "scan_incl_sum_u64")
        run_scan<uint64_t>(ctx, c, dir, rep, [&](const uint64_t* in, uint64_t* out, uint64_t n, uint64_t*) {
          return swg_inclusive_sum_scan_u64(ctx, in, out, n);
        });
      else if (c.op == "compact")
        run_compact(ctx, c, dir, rep);
      else if (c.op == "sort_pairs" || c.op == "sort_packed" || c.op == "sort_words")
        run_sort(ctx, c, dir, rep);
      else
        die(3, "unknown operation '" + c.op + "'");
    }
    std::string guards = "ok", files = "-";
    if (!rep.bad_guards.empty()) {
      guards.clear();
      for (const std::string& g : rep.bad_guards) guards += (guards.empty() ? "" : ",") + g;
    }
    if (!rep.files.empty()) {
      files.clear();
      for (const std::string& g : rep.files) files += (files.empty() ? "" : ",") + g;
    }
    printf("case %s rc=%d guards=%s files=%s\n", c.name.c_str(), rep.rc, guards.c_str(), files.c_str());
  }
  fflush(stdout);
  swg_destroy(ctx);
  return 0;
}
