// The ranged filter's host planning (sweepga_amd/csrc/host/range_plan.h) on the CPU: packing of genome pairs into ranges, the
// chain-number shifts and the budget search.  Prints one JSON line; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../sweepga_amd/csrc/host/range_plan.h"

static int failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

int main() {
  using namespace swg_range;
  {  // pair-major: five pairs of 10 records each, contiguous; R = 25 -> ranges {0,1}, {2,3}, {4}
    std::vector<uint64_t> cnt = {10, 10, 10, 10, 10}, first = {0, 10, 20, 30, 40}, last = {9, 19, 29, 39, 49};
    std::vector<Range> rs;
    std::vector<uint32_t> of(5);
    uint32_t bad = 0;
    CHECK(pack(5, cnt.data(), first.data(), last.data(), 25, &rs, of.data(), &bad) == PACK_OK);
    CHECK(rs.size() == 3);
    CHECK(rs[0].count == 20 && rs[0].lo == 0 && rs[0].hi == 20 && rs[0].contiguous && !rs[0].oversize);
    CHECK(rs[1].count == 20 && rs[1].lo == 20 && rs[1].hi == 40 && rs[1].contiguous);
    CHECK(rs[2].count == 10 && rs[2].contiguous);
    CHECK(of[0] == 0 && of[1] == 0 && of[2] == 1 && of[3] == 1 && of[4] == 2);
  }
  {  // interleaved pairs (shuffled input): never contiguous; packing follows first-record order, absent pairs get no range
    std::vector<uint64_t> cnt = {4, 0, 4, 4}, first = {1, UINT64_MAX, 0, 2}, last = {13, 0, 14, 15};
    std::vector<Range> rs;
    std::vector<uint32_t> of(4);
    uint32_t bad = 0;
    CHECK(pack(4, cnt.data(), first.data(), last.data(), 8, &rs, of.data(), &bad) == PACK_OK);
    CHECK(rs.size() == 2);
    CHECK(rs[0].pairs.size() == 2 && rs[0].pairs[0] == 2 && rs[0].pairs[1] == 0);
    CHECK(!rs[0].contiguous && !rs[1].contiguous);
    CHECK(of[1] == UINT32_MAX && of[2] == 0 && of[0] == 0 && of[3] == 1);
  }
  {  // a pair larger than R forms a range of its own, between its neighbours; nothing is packed behind it
    std::vector<uint64_t> cnt = {5, 50, 5, 5}, first = {0, 5, 55, 60}, last = {4, 54, 59, 64};
    std::vector<Range> rs;
    std::vector<uint32_t> of(4);
    uint32_t bad = 0;
    CHECK(pack(4, cnt.data(), first.data(), last.data(), 20, &rs, of.data(), &bad) == PACK_OK);
    CHECK(rs.size() == 3);
    CHECK(rs[0].count == 5 && !rs[0].oversize);
    CHECK(rs[1].count == 50 && rs[1].oversize && rs[1].contiguous && rs[1].lo == 5 && rs[1].hi == 55);
    CHECK(rs[2].count == 10 && !rs[2].oversize && rs[2].contiguous);
  }
  {  // a pair of 2^31 records is refused; R is capped below 2^31
    std::vector<uint64_t> cnt = {3, uint64_t(1) << 31}, first = {0, 3}, last = {2, (uint64_t(1) << 31) + 2};
    std::vector<Range> rs;
    std::vector<uint32_t> of(2);
    uint32_t bad = 0;
    CHECK(pack(2, cnt.data(), first.data(), last.data(), UINT64_MAX, &rs, of.data(), &bad) == PACK_PAIR_TOO_LARGE && bad == 1);
    cnt[1] = MAX_RANGE;
    last[1] = MAX_RANGE + 2;
    CHECK(pack(2, cnt.data(), first.data(), last.data(), UINT64_MAX, &rs, of.data(), &bad) == PACK_OK);
    CHECK(rs.size() == 2 && rs[1].count == MAX_RANGE && !rs[1].oversize);
  }
  {  // shifts: pairs with kept chains in order of their first retained record, numbers contiguous from 1
    // pair 0: local 3..5 (fret 40), pair 1: none, pair 2: local 1..2 (fret 10), pair 3: local 7..7 (fret 20)
    std::vector<uint32_t> lo = {3, 0xffffffffu, 1, 7}, hi = {5, 0, 2, 7};
    std::vector<uint64_t> fret = {40, 5, 10, 20};
    std::vector<int64_t> sh(4);
    uint64_t total = 0;
    CHECK(shifts(4, lo.data(), hi.data(), fret.data(), sh.data(), &total));
    CHECK(total == 6);
    CHECK(1 + sh[2] == 1 && 2 + sh[2] == 2);  // pair 2 first: 1, 2
    CHECK(7 + sh[3] == 3);                    // then pair 3: 3
    CHECK(3 + sh[0] == 4 && 5 + sh[0] == 6);  // then pair 0: 4 .. 6
    CHECK(sh[1] == 0);
    // numbers reaching 2^32 are refused
    std::vector<uint32_t> lo2 = {1, 1}, hi2 = {0xffffffffu, 2};
    std::vector<uint64_t> f2 = {0, 1};
    CHECK(!shifts(2, lo2.data(), hi2.data(), f2.data(), sh.data(), &total) && total == 0x100000001ull);
  }
  {  // budget search: the largest m with cost(m) <= budget
    auto cost = [](uint64_t m) { return 1000 + 300 * m; };
    CHECK(largest(MAX_RANGE, 1000 + 300 * 77, cost) == 77);
    CHECK(largest(MAX_RANGE, 1000 + 300 * 77 + 299, cost) == 77);
    CHECK(largest(MAX_RANGE, 999, cost) == 0);
    CHECK(largest(MAX_RANGE, UINT64_MAX / 2, cost) == MAX_RANGE);
    CHECK(largest(10, UINT64_MAX / 2, cost) == 10);
  }
  std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
  return failures ? 1 : 0;
}
