// The rules of the divergence track (sweepga_amd/csrc/swg_divergence_walk.h) on a CPU, without the library: a stand-alone program
// that a host compiler builds from the header as it is.  Standard input, one entry per line:
//   axis minus q_start q_end t_start W first n  then n pairs `length letter`
// The ops are laid behind `first` earlier ops of another entry (a 7= each), so that the entry's prefix sums do not start at 0 and the
// origin's arithmetic modulo 2^32 is exercised.  For every window the entry's ops touch it prints
//   k mismatches m_columns unaligned inserted mismatch_runs indels
// accumulated as the op pass does (the first window's share, the last window's share, W for every window between), then `--`.
// tests/test_divergence_cpu.py feeds it and compares with tests/divergence_model.py.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_divergence_walk.h"

using namespace swg_divergence;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    unsigned long long axis, minus, q_start, q_end, t_start, W, first, n;
    if (!(in >> axis >> minus >> q_start >> q_end >> t_start >> W >> first >> n)) return 2;
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
    const Prefix P{X.data(), Y.data(), A.data(), E.data()};
    const uint32_t origin = entry_origin(P, (uint32_t)first, (uint32_t)axis, minus != 0, (uint32_t)q_start, (uint32_t)q_end, (uint32_t)t_start);
    const uint32_t flags = E_USABLE | (!axis && minus ? E_DESCENDS : 0u);
    const uint32_t b = axis ? (uint32_t)(t_start + (Y.back() - Y[first])) : (uint32_t)q_end;
    std::map<uint32_t, std::vector<uint64_t>> table;
    auto cell = [&](uint32_t k) -> std::vector<uint64_t>& {
      std::vector<uint64_t>& c = table[k];
      c.resize(Q_OPS, 0);
      return c;
    };
    for (uint64_t r = first; r < first + n; ++r) {
      if (!kind[r]) continue;
      const uint64_t l = swg_diffs::op_length(P, r, kind[r]);
      if (!l) continue;
      const bool extent = has_extent(kind[r], (uint32_t)axis);
      uint32_t lo, hi, k0, k1;
      uint64_t in0, in1;
      op_where(P, r, (uint32_t)axis, flags, origin, b, extent, (uint32_t)l, &lo, &hi);
      window_span(lo, hi, (uint32_t)W, &k0, &k1, &in0, &in1);
      if (extent) {
        const int q = extent_quantity(kind[r]);
        cell(k0)[q] += in0;
        if (k1 != k0) cell(k1)[q] += in1;
        for (uint32_t k = k0 + 1; k < k1; ++k) cell(k)[q] += W;
      } else {
        cell(k0)[Q_INSERTED] += l;
      }
      cell(k0)[kind[r] == K_SNP ? Q_RUNS : Q_INDELS] += kind[r] != K_M;
    }
    for (const auto& kv : table) {
      std::printf("%u", kv.first);
      for (uint64_t v : kv.second) std::printf(" %llu", (unsigned long long)v);
      std::fputc('\n', stdout);
    }
    std::puts("--");
  }
  return 0;
}
