// texts_hand_over (sweepga_amd/csrc/host/host_internal.h) on the CPU: the one place where the report texts leave the library over
// the C ABI.  Host code only, linked without any object of the library.  Prints one JSON line; exit status 0 = every check held.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../../include/sweepga_gpu.h"
#include "../../sweepga_amd/csrc/host/host_internal.h"

// the library's error sink (host/alnstats.cpp); the hand-over reaches it only when malloc fails
int swg_alnstats_error(int code, const char*, ...) { return code; }

static int failures = 0;
#define CHECK(c)                                                          \
  do {                                                                    \
    if (!(c)) {                                                           \
      std::fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static char untouched;  // what a caller's slot holds when the library must leave it alone

// hands over `count` texts under `wanted` and checks every slot: a wanted one holds the text, NUL-terminated at its length, in a
// buffer of its own; an unwanted one is as the caller left it
static void check_case(const std::string* text, const bool* wanted, int count) {
  char* out[3] = {&untouched, &untouched, &untouched};
  uint64_t len[3] = {77, 77, 77};
  CHECK(texts_hand_over(text, wanted, count, out, len) == SWG_OK);
  for (int k = 0; k < 3; ++k) {
    if (k < count && wanted[k]) {
      CHECK(out[k] != nullptr && out[k] != &untouched && out[k] != text[k].data());
      CHECK(len[k] == text[k].size());
      CHECK(out[k] && std::memcmp(out[k], text[k].data(), text[k].size()) == 0);
      CHECK(out[k] && out[k][len[k]] == 0);
      for (int j = 0; j < k; ++j) CHECK(!(j < count && wanted[j]) || out[j] != out[k]);
      std::free(out[k]);
    } else {
      CHECK(out[k] == &untouched && len[k] == 77);
    }
  }
}

int main() {
  const std::string two[2] = {"rows\tof\ta\treport\n", std::string("a\0b\n", 4)};  // (a text may hold a NUL: the length says where it ends)
  const std::string three[3] = {"all\n", "kept\nkept\n", "lost\n"};
  const std::string empty[2] = {"", ""};
  const bool first[2] = {true, false}, second[2] = {false, true}, both[2] = {true, true}, last_two[3] = {false, true, true};
  check_case(two, first, 2);
  check_case(two, second, 2);
  check_case(two, both, 2);
  check_case(three, last_two, 3);
  check_case(empty, both, 2);  // an empty wanted text: a 1-byte buffer holding the NUL, length 0
  {
    char* out[2] = {nullptr, nullptr};
    uint64_t len[2] = {5, 5};
    CHECK(texts_hand_over(empty, first, 2, out, len) == SWG_OK);
    CHECK(out[0] != nullptr && out[0][0] == 0 && len[0] == 0);
    CHECK(out[1] == nullptr && len[1] == 5);
    std::free(out[0]);
  }
  std::printf("{\"ok\": %s, \"failures\": %d}\n", failures ? "false" : "true", failures);
  return failures ? 1 : 0;
}
