// The rules of the resolved CIGARs (sweepga_amd/csrc/swg_eqx_walk.h) on a CPU, without the library: a stand-alone program that a
// host compiler builds from the header as it is.  Standard input, one entry of state 0 per line:
//   minus q_start q_end t_start T Q text
// T and Q are the whole target and query sequence.  The text is walked op by op with the header's functions alone -- column_class and
// is_run_start for the runs, code_of / comp_code / column_eq / column_n for every column, sums_add / sums_field for the six sums,
// decimal_digits and op_text_byte for every generated op -- and one line is printed:
//   <output text or -> out_ops matches mismatches n_columns eq_wrong x_wrong m_columns
// A line `digits <v>` prints decimal_digits(v) and the bytes of `<v>=`.  tests/test_eqx_cpu.py feeds it and compares with
// tests/eqx_model.py.
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "../../sweepga_amd/csrc/swg_eqx_walk.h"

using namespace swg_eqx;

static void put_op(std::string& out, uint32_t length, uint8_t letter) {
  const uint32_t bytes = decimal_digits(length) + 1;
  for (uint32_t k = 0; k < bytes; ++k) out += (char)op_text_byte(length, letter, k);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string first;
    in >> first;
    if (first == "digits") {
      unsigned long long v;
      if (!(in >> v)) return 2;
      std::string o;
      put_op(o, (uint32_t)v, '=');
      std::printf("%u %s\n", decimal_digits((uint32_t)v), o.c_str());
      continue;
    }
    unsigned long long minus = std::stoull(first), q_start, q_end, t_start;
    std::string Ts, Qs, text;
    if (!(in >> q_start >> q_end >> t_start >> Ts >> Qs >> text)) return 2;
    // exactly the sequence's bytes on the heap: a read past either end is the sanitizer's
    std::vector<uint8_t> T(Ts.begin(), Ts.end()), Q(Qs.begin(), Qs.end());
    std::string out;
    ColumnSums sums{{0, 0}};
    uint64_t x = 0, y = 0, out_ops = 0, run_len = 0;
    bool run_eq = false;
    unsigned char prev = 0;
    auto close = [&]() {
      if (run_len) put_op(out, (uint32_t)run_len, run_eq ? '=' : 'X'), ++out_ops;
      run_len = 0;
    };
    for (size_t at = 0; at < text.size();) {
      size_t d = at;
      uint64_t l = 0;
      while (d < text.size() && swg_cigar::is_digit((unsigned char)text[d])) l = l * 10 + (uint64_t)(text[d++] - '0');
      const unsigned char ch = (unsigned char)text[d];
      const uint32_t cls = column_class(ch);
      if (is_run_start(ch, prev)) close();  // (nothing is open: the op in front closed it)
      if (cls) {
        for (uint64_t b = 0; b < l; ++b) {
          const uint32_t r = code_of(T[t_start + y + b]);
          const uint32_t a0 = code_of(Q[minus ? q_end - 1 - (x + b) : q_start + x + b]), a = minus ? comp_code(a0) : a0;
          const bool eq = column_eq(r, a);
          sums_add(sums, cls, eq, column_n(r, a));
          if (run_len && eq != run_eq) close();
          run_eq = eq, ++run_len;
        }
      } else {
        close();
        out.append(text, at, d + 1 - at);
        ++out_ops;
      }
      uint64_t dx, dy, da, de;
      swg_cigar::op_advance(ch, l, &dx, &dy, &da, &de);
      x += dx, y += dy;
      prev = ch;
      at = d + 1;
    }
    close();
    std::printf("%s %llu", out.empty() ? "-" : out.c_str(), (unsigned long long)out_ops);
    for (int i = 0; i < 6; ++i) std::printf(" %u", sums_field(sums, i));
    std::printf("\n");
  }
  return 0;
}
