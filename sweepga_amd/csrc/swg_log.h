// Bit-exact restatement of glibc's log(), in two functions.
//
// The reference computes scores with Rust's f64::ln (plane_sweep_exact.rs:74), chain identities with
// ln(gap) (paf_filter.rs:903) and Mash distances with ln(2J / (1 + J)) (mash.rs:58-73); on Linux that
// is glibc's `log`.  Scores order the plane sweep and distances order the kNN selection, so a last-bit
// difference can flip a tie: the device therefore reproduces glibc's algorithm
// (sysdeps/ieee754/dbl-64/e_log.c, the FMA build `__log_fma` that the ifunc selects on every
// FMA-capable x86-64) operation for operation.  glibc's log has three branches:
//
//   table     (everything else)
//     tmp = ix - OFF; i = (tmp >> 45) & 127; k = (int64)tmp >> 52; z = ix - (tmp & 0xfff<<52)
//     r  = fma(z, invc[i], -1)            w  = fma(k, Ln2hi, logc[i])
//     hi = w + r                          lo = fma(k, Ln2lo, (w - hi) + r)
//     r2 = r*r
//     y  = fma(r*r2, fma(fma(r,A4,A3), r2, fma(r,A2,A1)), fma(r2, A0, lo)) + hi
//
//   near 1    (1 - 0x1p-4 <= x < 1 + 0x1.09p-4, tested on the bits: ix - LO < HI - LO)
//     x == 1 returns +0; otherwise, with the eleven `poly1` coefficients B0..B10 (B0 = -0.5):
//     r  = x - 1                          r2 = r*r                 r3 = r*r2
//     q  = fma(fma(pC, r3, pB), r3, pA)   pA = fma(r2,B3, fma(r,B2,B1))   pB = fma(r2,B6, fma(r,B5,B4))
//                                         pC = fma(r3,B10, fma(r2,B9, fma(r,B8,B7)))
//     rhi = fma(-0x1p27, r, fma(r, 0x1p27, r))                     rlo = r - rhi
//     hi = fma(rhi*rhi, B0, r)            lo = fma(rhi*rhi, B0, r - hi)
//     lo = fma(B0*rlo, rhi + r, lo)       y  = fma(q, r3, lo) + hi
//
//   special   (x < 0x1p-1022, inf or NaN, tested on the top 16 bits)
//     +-0 -> -inf; +inf -> +inf; negative or NaN -> NaN; a subnormal is scaled by 2^52, 52 is taken off
//     the exponent field of its bits and it goes through the table branch.
//
// The fused/unfused split of every branch is the one in the shipped `__log_fma` object code (read from
// its disassembly), so every operation here is written with explicit fma/mul/add primitives and the
// functions are compiled with contraction off.
//
//   swg_log_glibc(x)      the table branch alone (plus x == 1 -> +0).  Domain: integers >= 1 as f64,
//                         which are either 1 or >= 2 and so never in the near-1 window, and never
//                         special.  The callers on the hot paths use it: the sweep's score keys, the
//                         scaffold's gap term, the ANI keys, and swg_log_range.
//   swg_log_glibc_any(x)  all three branches: every double.  The Mash distance, whose argument
//                         2J / (1 + J) is a fraction in (0, 1] and lies in the near-1 window once
//                         J >= 15/17, and swg_log (arbitrary host doubles) use it.
//
// tests/native/log_check.cpp (run by tests/test_abi_cpu.py) checks both functions of this header
// against the host libm on the CPU: integers for the first; Mash ratios, the near-1 window and its
// edges, all binades, integers and the specials for the second.  tests/test_gpu_sweep.py
// (test_device_log_equals_host_libm) and tests/test_gpu_mash.py do the same for the device build.
#pragma once
#include <stdint.h>

#include "glibc_log_table.h"

#if defined(__HIPCC__)
#define SWG_HD __host__ __device__
#else
#define SWG_HD
#endif

#if defined(__HIP_DEVICE_COMPILE__)
__device__ __constant__ static const double swg_log_tab[256] = SWG_LOG_TABLE_INIT;
#define SWG_FMA(a, b, c) __fma_rn((a), (b), (c))
#define SWG_MUL(a, b) __dmul_rn((a), (b))
#define SWG_ADD(a, b) __dadd_rn((a), (b))
#define SWG_SUB(a, b) __dsub_rn((a), (b))
#else
static const double swg_log_tab[256] = SWG_LOG_TABLE_INIT;
#define SWG_FMA(a, b, c) __builtin_fma((a), (b), (c))
static inline double swg_mul_(double a, double b) { volatile double r = a * b; return r; }
static inline double swg_add_(double a, double b) { volatile double r = a + b; return r; }
static inline double swg_sub_(double a, double b) { volatile double r = a - b; return r; }
#define SWG_MUL(a, b) swg_mul_((a), (b))
#define SWG_ADD(a, b) swg_add_((a), (b))
#define SWG_SUB(a, b) swg_sub_((a), (b))
#endif

// the table branch, on the bits of a normal positive double
SWG_HD static inline double swg_log_table_(uint64_t ix) {
  union { double d; uint64_t u; } cv;
  const uint64_t OFF = 0x3fe6000000000000ULL;
  const uint64_t tmp = ix - OFF;
  const int i = (int)((tmp >> 45) & 127);
  const int64_t k = (int64_t)tmp >> 52;
  cv.u = ix - (tmp & (0xfffULL << 52));
  const double z = cv.d;
  const double invc = swg_log_tab[2 * i], logc = swg_log_tab[2 * i + 1];
  const double kd = (double)k;
  const double r = SWG_FMA(z, invc, -1.0);
  const double w = SWG_FMA(kd, SWG_LOG_LN2HI, logc);
  const double hi = SWG_ADD(w, r);
  const double lo = SWG_FMA(kd, SWG_LOG_LN2LO, SWG_ADD(SWG_SUB(w, hi), r));
  const double r2 = SWG_MUL(r, r);
  const double r3 = SWG_MUL(r, r2);
  const double p1 = SWG_FMA(r, SWG_LOG_A2, SWG_LOG_A1);
  const double p2 = SWG_FMA(r, SWG_LOG_A4, SWG_LOG_A3);
  const double q = SWG_FMA(p2, r2, p1);
  const double t1 = SWG_FMA(r2, SWG_LOG_A0, lo);
  const double t2 = SWG_FMA(r3, q, t1);
  return SWG_ADD(t2, hi);
}

// integers >= 1 (as f64) only: see the domain above
SWG_HD static inline double swg_log_glibc(double x) {
  union { double d; uint64_t u; } cv;
  cv.d = x;
  if (cv.u == 0x3ff0000000000000ULL) return 0.0;  // x == 1
  return swg_log_table_(cv.u);
}

// every double
SWG_HD static inline double swg_log_glibc_any(double x) {
  union { double d; uint64_t u; } cv;
  cv.d = x;
  uint64_t ix = cv.u;
  const uint64_t LO = 0x3fee000000000000ULL;  // 1 - 0x1p-4
  const uint64_t HI = 0x3ff1090000000000ULL;  // 1 + 0x1.09p-4
  if (ix - LO < HI - LO) {
    if (ix == 0x3ff0000000000000ULL) return 0.0;  // x == 1
    const double r = SWG_SUB(x, 1.0);
    const double r2 = SWG_MUL(r, r);
    const double r3 = SWG_MUL(r, r2);
    const double pa = SWG_FMA(r2, SWG_LOG_B3, SWG_FMA(r, SWG_LOG_B2, SWG_LOG_B1));
    const double pb = SWG_FMA(r2, SWG_LOG_B6, SWG_FMA(r, SWG_LOG_B5, SWG_LOG_B4));
    const double pc = SWG_FMA(r3, SWG_LOG_B10, SWG_FMA(r2, SWG_LOG_B9, SWG_FMA(r, SWG_LOG_B8, SWG_LOG_B7)));
    const double q = SWG_FMA(SWG_FMA(pc, r3, pb), r3, pa);
    const double rhi = SWG_FMA(-0x1p27, r, SWG_FMA(r, 0x1p27, r));
    const double rlo = SWG_SUB(r, rhi);
    const double rhi2 = SWG_MUL(rhi, rhi);
    const double hi = SWG_FMA(rhi2, SWG_LOG_B0, r);
    double lo = SWG_FMA(rhi2, SWG_LOG_B0, SWG_SUB(r, hi));
    lo = SWG_FMA(SWG_MUL(SWG_LOG_B0, rlo), SWG_ADD(rhi, r), lo);
    return SWG_ADD(hi, SWG_FMA(q, r3, lo));
  }
  const uint32_t top = (uint32_t)(ix >> 48);
  if (top - 0x0010u >= 0x7ff0u - 0x0010u) {  // x < 0x1p-1022, inf or NaN
    if (ix * 2 == 0) { cv.u = 0xfff0000000000000ULL; return cv.d; }  // log(+-0) = -inf
    if (ix == 0x7ff0000000000000ULL) return x;                       // log(inf) = inf
    if ((top & 0x8000u) || (top & 0x7ff0u) == 0x7ff0u) { cv.u = 0x7ff8000000000000ULL; return cv.d; }  // NaN
    cv.d = SWG_MUL(x, 0x1p52);  // subnormal: normalise
    ix = cv.u - (52ULL << 52);
  }
  return swg_log_table_(ix);
}
