// Host-side check of sweepga_amd/csrc/swg_log.h against the platform libm log().
// usage: log_check <first> <count> [stride]   integers first + n*stride through swg_log_glibc
//        log_check file <path>                raw little-endian doubles through swg_log_glibc_any
//        log_check mash <max_union>           every Mash ratio 2J/(1+J), J = inter/union, 1 <= inter <= union <= max_union,
//                                             computed as mash_dist_kernel does, through swg_log_glibc_any
// Each prints the number of results whose bit pattern differs from libm's (two NaNs are equal whatever their payload)
// and exits 1 if there is any; the first few mismatches go to stderr.
// -DLOG_CHECK_HEADER='"..."' / -DLOG_CHECK_ANY=name measure another header or function the same way.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdint>
#include <vector>
#ifndef LOG_CHECK_HEADER
#define LOG_CHECK_HEADER "../../sweepga_amd/csrc/swg_log.h"
#endif
#include LOG_CHECK_HEADER
#ifndef LOG_CHECK_ANY
#define LOG_CHECK_ANY swg_log_glibc_any
#endif

static bool differs(double x, const char* what, uint64_t a0, uint64_t a1) {
  double a = LOG_CHECK_ANY(x), b = std::log(x);
  if (a != a && b != b) return false;
  if (std::memcmp(&a, &b, 8) == 0) return false;
#pragma omp critical
  {
    static int shown = 0;
    if (shown++ < 8) fprintf(stderr, "%s %llu %llu: x=%a got %a libm %a\n", what, (unsigned long long)a0, (unsigned long long)a1, x, a, b);
  }
  return true;
}

static int finish(uint64_t bad) {
  printf("%llu\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}

int main(int argc, char** argv) {
  uint64_t bad = 0;
  if (argc > 2 && !strcmp(argv[1], "file")) {
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    fseek(f, 0, SEEK_END);
    const uint64_t n = (uint64_t)ftell(f) / 8;
    fseek(f, 0, SEEK_SET);
    std::vector<double> x(n);
    if (fread(x.data(), 8, n, f) != n) { fprintf(stderr, "short read\n"); return 2; }
    fclose(f);
#pragma omp parallel for reduction(+ : bad) schedule(static)
    for (uint64_t t = 0; t < n; ++t) bad += differs(x[t], "index", t, 0);
    return finish(bad);
  }
  if (argc > 2 && !strcmp(argv[1], "mash")) {
    const uint64_t maxu = strtoull(argv[2], 0, 10);
    uint64_t in_window = 0;
#pragma omp parallel for reduction(+ : bad, in_window) schedule(dynamic, 16)
    for (uint64_t un = 1; un <= maxu; ++un)
      for (uint64_t in = 1; in <= un; ++in) {
        volatile double jac = (double)in / (double)un;
        volatile double num = 2.0 * jac, den = 1.0 + jac;  // three separately rounded operations
        volatile double ratio = num / den;
        in_window += ratio >= 0.9375;
        bad += differs(ratio, "inter union", in, un);
      }
    fprintf(stderr, "%llu ratios, %llu of them >= 0.9375\n", (unsigned long long)(maxu * (maxu + 1) / 2), (unsigned long long)in_window);
    return finish(bad);
  }
  uint64_t first = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
  uint64_t count = argc > 2 ? strtoull(argv[2], 0, 10) : 1000000;
  uint64_t stride = argc > 3 ? strtoull(argv[3], 0, 10) : 1;
#pragma omp parallel for reduction(+ : bad) schedule(static)
  for (uint64_t n = 0; n < count; ++n) {
    double x = (double)(first + n * stride);
    double a = swg_log_glibc(x), b = std::log(x);
    if (std::memcmp(&a, &b, 8) != 0) ++bad;
  }
  printf("%llu\n", (unsigned long long)bad);
  return bad ? 1 : 0;
}
