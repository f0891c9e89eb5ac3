// The rules of the alignment blocks (sweepga_amd/csrc/swg_maf_walk.h) on a CPU, without the library: a stand-alone program that a
// host compiler builds from the header as it is.  Standard input, one entry of state 0 per line:
//   minus q_start q_end t_start g T Q text
// T and Q are the whole target and query sequence.  The four prefix sums are built with op_advance, and everything else goes the way
// the kernels go with the header's functions alone: is_breaker per op, the candidate starts, the scans G and BK, candidate_end (no
// loop over the breakers), block_words, and for every output byte its op by a search in G and row_byte.  Per block one line
//   B op_first op_end t_start t_bases q_start q_bases aligned columns flags walk_x <target row> <query row>
// and per entry one line `E gap_only breakers skipped_t skipped_q`.  A line `comp` prints comp_raw of all 256 bytes.
// tests/test_maf_cpu.py feeds it and compares with tests/maf_model.py.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_maf_walk.h"

using namespace swg_maf;

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string first;
    in >> first;
    if (first == "comp") {
      for (int b = 0; b < 256; ++b) std::printf("%d%c", comp_raw((uint8_t)b), b == 255 ? '\n' : ' ');
      continue;
    }
    unsigned long long minus = std::stoull(first), q_start, q_end, t_start, g;
    std::string Ts, Qs, text;
    if (!(in >> q_start >> q_end >> t_start >> g >> Ts >> Qs >> text)) return 2;
    // exactly the sequences' bytes on the heap, one behind the other as the device has them: a read past either end is the sanitizer's
    std::vector<uint8_t> bases(Ts.begin(), Ts.end());
    const uint64_t q0 = bases.size();
    bases.insert(bases.end(), Qs.begin(), Qs.end());
    std::vector<uint64_t> X(1, 0), Y(1, 0), A(1, 0), E(1, 0);
    for (size_t at = 0; at < text.size();) {
      size_t d = at;
      uint64_t l = 0;
      while (d < text.size() && swg_cigar::is_digit((unsigned char)text[d])) l = l * 10 + (uint64_t)(text[d++] - '0');
      uint64_t dx, dy, da, de;
      if (swg_cigar::op_advance((unsigned char)text[d], l, &dx, &dy, &da, &de)) return 3;
      X.push_back(X.back() + dx), Y.push_back(Y.back() + dy), A.push_back(A.back() + da), E.push_back(E.back() + de);
      at = d + 1;
    }
    const Prefix P{X.data(), Y.data(), A.data(), E.data()};
    const uint64_t ops = X.size() - 1;
    std::vector<uint64_t> G(ops + 1, 0), BK(ops + 1, 0), starts;
    uint64_t skipped_t = 0, skipped_q = 0, gap_only = 0;
    for (uint64_t r = 0; r < ops; ++r) {
      const uint64_t dx = X[r + 1] - X[r], dy = Y[r + 1] - Y[r];
      const bool brk = is_breaker(dx, dy, (uint32_t)g);
      if (brk) skipped_t += dy, skipped_q += dx;
      else if (r == 0 || op_is_breaker(P, r - 1, (uint32_t)g)) starts.push_back(r);
      G[r + 1] = G[r] + (brk ? 0 : op_columns(dx, dy));
      BK[r + 1] = BK[r] + (brk ? 1 : 0);
    }
    for (size_t i = 0; i < starts.size(); ++i) {
      const uint64_t start = starts[i], next = i + 1 < starts.size() ? starts[i + 1] : ops;
      const uint64_t end = candidate_end(next, BK[next], BK[start]);
      uint32_t w[10];
      block_words(P, 0, start, end, minus != 0, (uint32_t)q_start, (uint32_t)q_end, (uint32_t)t_start, w);
      if (w[6] == 0) {
        ++gap_only;
        continue;
      }
      if ((uint64_t)w[7] != G[end] - G[start]) return 4;
      std::string rows[2];
      for (uint32_t row = 0; row < 2; ++row)
        for (uint64_t col = G[start]; col < G[end]; ++col) {
          uint64_t lo = start, hi = end - 1;  // the last op r with G[r] <= col
          while (lo < hi) {
            const uint64_t mid = lo + ((hi - lo + 1) >> 1);
            if (G[mid] <= col) lo = mid;
            else hi = mid - 1;
          }
          const uint64_t r = lo;
          OpBytes o;
          o.rows = op_rows(X[r + 1] - X[r], Y[r + 1] - Y[r]);
          o.minus = minus != 0;
          o.t_at = t_start + Y[r];
          o.q_at = minus ? q0 + q_end - 1 - X[r] : q0 + q_start + X[r];
          rows[row] += (char)row_byte(o, bases.data(), COMP_RAW, row, col - G[r]);
        }
      std::printf("B");
      for (int k = 0; k < 10; ++k) std::printf(" %u", w[k]);
      std::printf(" %s %s\n", rows[0].c_str(), rows[1].c_str());
    }
    std::printf("E %llu %llu %llu %llu\n", (unsigned long long)gap_only, (unsigned long long)BK[ops], (unsigned long long)skipped_t, (unsigned long long)skipped_q);
  }
  return 0;
}
