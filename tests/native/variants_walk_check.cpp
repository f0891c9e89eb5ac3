// The rules of the variant calls (sweepga_amd/csrc/swg_variants_walk.h) on a CPU, without the library: a stand-alone program that a
// host compiler builds from the header as it is.  Standard input, one entry per line:
//   minus q_start q_end t_start max_indel first T Q n  then n pairs `length letter`
// T and Q are the whole target and query sequence.  The ops are laid behind `first` earlier ops of another entry (a 7= each), so that
// the entry's prefix sums do not start at 0.  Every op is taken as the kernels take it -- a column of X or M through column_counter,
// an I or D through indel_fate -- and every variant is printed as
//   kind_flags pos ref_len alt_len q_pos REF ALT
// from variant_words and allele_byte, then a line `= ` with the 15 column counters, long and unanchored, then `--`.
// tests/test_variants_cpu.py feeds it and compares with tests/variants_model.py.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_variants_walk.h"

using namespace swg_variants;

static void print_variant(const Site& s, const uint8_t* T, const uint8_t* Q) {
  uint32_t w[4];
  variant_words(s, w);
  std::printf("%u %u %u %u %u ", s.kind | (s.minus ? 256u : 0u), w[0], w[1], w[2], w[3]);
  const uint64_t bytes = allele_bytes(s);
  if (bytes != (uint64_t)w[1] + w[2]) std::printf("LENGTHS-DIFFER ");
  for (uint64_t k = 0; k < bytes; ++k) {
    if (k == w[1]) std::fputc(' ', stdout);
    std::fputc(allele_byte(s, T, Q, k), stdout);
  }
  std::fputc('\n', stdout);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    unsigned long long minus, q_start, q_end, t_start, max_indel, first, n;
    std::string Ts, Qs;
    if (!(in >> minus >> q_start >> q_end >> t_start >> max_indel >> first >> Ts >> Qs >> n)) return 2;
    // exactly the sequence's bytes on the heap: a read past either end is the sanitizer's
    std::vector<uint8_t> Tv(Ts.begin(), Ts.end()), Qv(Qs.begin(), Qs.end());
    const uint8_t *T = Tv.data(), *Q = Qv.data();
    std::vector<uint64_t> X(1, 0), Y(1, 0), A(1, 0), E(1, 0);
    std::vector<uint32_t> kind;
    auto push = [&](uint64_t l, char ch) {
      uint64_t dx, dy, da, de;
      swg_cigar::op_advance((unsigned char)ch, l, &dx, &dy, &da, &de);
      X.push_back(X.back() + dx), Y.push_back(Y.back() + dy), A.push_back(A.back() + da), E.push_back(E.back() + de);
      kind.push_back(swg_diffs::kind_of((unsigned char)ch));
    };
    for (unsigned long long j = 0; j < first; ++j) push(7, '=');
    for (unsigned long long j = 0; j < n; ++j) {
      unsigned long long l;
      char ch;
      if (!(in >> l >> ch)) return 2;
      push(l, ch);
    }
    const swg_cigar::Prefix P{X.data(), Y.data(), A.data(), E.data()};
    uint64_t counter[C_TOTAL] = {0}, n_long = 0, unanchored = 0;
    for (uint64_t r = first; r < first + n; ++r) {
      const uint32_t kd = kind[r] & (K_SNP | K_M | K_INS | K_DEL);
      if (!kd) continue;
      const uint64_t l = swg_diffs::op_length(P, r, kd);
      if (!l) continue;
      Site s{};
      s.kind = kd & K_M ? K_SNP : kd, s.minus = (uint32_t)minus, s.l = (uint32_t)l;
      s.x = (uint32_t)(X[r] - X[first]), s.p = t_start + (Y[r] - Y[first]);
      s.q_start = (uint32_t)q_start, s.q_end = (uint32_t)q_end;
      if (kd & (K_SNP | K_M)) {
        for (uint64_t b = 0; b < l; ++b) {
          const int idx = column_counter(code_of(T[s.p + b]), query_column(s, Q, (uint64_t)s.x + b), (kd & K_M) != 0);
          ++counter[idx];
          if (idx >= C_SAME) continue;
          Site c = s;
          c.x += (uint32_t)b, c.p += b, c.l = 1;
          print_variant(c, T, Q);
        }
        continue;
      }
      const int fate = indel_fate(kd, l, s.p, Tv.size(), (uint32_t)max_indel);
      n_long += fate == 2, unanchored += fate == 1;
      if (fate == 0) print_variant(s, T, Q);
    }
    std::printf("=");
    for (uint64_t v : counter) std::printf(" %llu", (unsigned long long)v);
    std::printf(" %llu %llu\n--\n", (unsigned long long)n_long, (unsigned long long)unanchored);
  }
  return 0;
}
