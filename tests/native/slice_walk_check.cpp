// The rules of the lift slices (sweepga_amd/csrc/swg_slice_walk.h) on a CPU, without the library: a stand-alone program meant to be
// built with the host sanitizers.  Standard input, one case per line:
//   cigar axis minus ca cb q_start q_end t_start
// The entry is parsed here by a plain loop (op_number / op_advance of swg_cigar_walk.h) into the four exclusive prefix sums and the
// letter positions, in heap blocks of exactly their size, in front of which stand the sums of a foreign record, so that `first` is
// not 0.  Output per case, one line: `-` without a column in the clip, else
//   q_start q_end t_start t_end aligned matches block has_eq cigar
// with the cigar read byte by byte through text_byte.  tests/test_lift_paf_cpu.py feeds it vectors and compares with
// tests/lift_paf_model.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_slice_walk.h"

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string cigar;
    uint32_t axis, minus, ca, cb, q_start, q_end, t_start;
    if (!(in >> cigar >> axis >> minus >> ca >> cb >> q_start >> q_end >> t_start)) return 2;
    const uint64_t lead = 3;  // bytes of another entry in front of this one
    const std::string all = "7M=" + cigar;  // (the three bytes in front are never read)
    char* text = static_cast<char*>(std::malloc(all.size()));
    if (!text) return 3;
    all.copy(text, all.size());
    std::vector<uint32_t> where;
    std::vector<uint64_t> adv[4];
    for (uint64_t p = lead; p < all.size(); ++p) {
      if (swg_cigar::is_digit((unsigned char)text[p])) continue;
      uint32_t len;
      uint64_t d[4];
      if (swg_cigar::op_number(text, lead, p, &len) || swg_cigar::op_advance((unsigned char)text[p], len, &d[0], &d[1], &d[2], &d[3])) return 2;
      where.push_back((uint32_t)(p - lead));
      for (int s = 0; s < 4; ++s) adv[s].push_back(d[s]);
    }
    const uint32_t nops = (uint32_t)where.size();
    const uint64_t first = 2;
    uint64_t* sums[4];
    for (int s = 0; s < 4; ++s) {
      sums[s] = static_cast<uint64_t*>(std::malloc((first + nops + 1) * sizeof(uint64_t)));
      if (!sums[s]) return 3;
      sums[s][0] = 0, sums[s][1] = 11, sums[s][2] = 11 + 13 * (uint64_t)(s + 1);
      for (uint32_t r = 0; r < nops; ++r) sums[s][first + r + 1] = sums[s][first + r] + adv[s][r];
    }
    uint32_t* pos = static_cast<uint32_t*>(std::malloc(nops ? nops * sizeof(uint32_t) : 1));
    if (!pos) return 3;
    for (uint32_t r = 0; r < nops; ++r) pos[r] = where[r];
    const swg_cigar::Prefix P{sums[0], sums[1], sums[2], sums[3]};
    swg_slice::Slice s;
    swg_slice::Plan p;
    if (!swg_slice::slice_of(P, first, nops, pos, text, lead, axis, minus, ca, cb, q_start, q_end, t_start, &s, &p)) {
      std::puts("-");
    } else {
      std::string out;
      for (uint32_t rel = 0; rel < s.text_len; ++rel) out += (char)swg_slice::text_byte(p, text, rel);
      std::printf("%u %u %u %u %u %u %llu %d %s\n", s.q_start, s.q_end, s.t_start, s.t_end, s.aligned, s.matches, (unsigned long long)s.block,
                  s.has_eq ? 1 : 0, out.c_str());
    }
    std::free(pos);
    for (auto& a : sums) std::free(a);
    std::free(text);
  }
  return 0;
}
