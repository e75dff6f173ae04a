// Host check of the argument checks the host-pointer entry points share (csrc/orb_argcheck.h): every case is accepted or rejected
// as stated, and a rejection names the entry point and the array.  No GPU, no HIP; built with -fsanitize=address,undefined by
// tests/test_arg_checks.py, so a check that reads past the array it was given stops the program too (every array below is a
// heap allocation of exactly its size).
#include "orb_argcheck.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <string>
#include <vector>

using namespace orbhip;

static int g_checked = 0;
#define CHECK(cond)                                                                               \
  do {                                                                                            \
    g_checked++;                                                                                  \
    if (!(cond)) { std::fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
  } while (0)

typedef std::vector<int32_t> V;
static const char E[] = "orbx_entry";

static bool accepted(const std::string& m) { return m.empty(); }
// rejected, and the message starts with the entry point's name and names the array
static bool rejected(const std::string& m, const char* array) {
  return m.rfind(std::string(E) + ": ", 0) == 0 && m.find(array) != std::string::npos;
}

static void csr_cases() {
  int total = -1;
  CHECK(accepted(check_csr(E, "slot_off", nullptr, 0, &total)) && total == 0);            // no rows: the array is not read
  { V o{0, 5}; CHECK(accepted(check_csr(E, "slot_off", o.data(), 1, &total)) && total == 5); }
  { V o{0, 0}; CHECK(accepted(check_csr(E, "slot_off", o.data(), 1, &total)) && total == 0); }
  { V o{0, 0, 3, 3, 3, 7, 7}; CHECK(accepted(check_csr(E, "obs_off", o.data(), 6, &total)) && total == 7); }      // empty rows at the start, inside, at the end
  { V o{0, 2, INT32_MAX}; CHECK(accepted(check_csr(E, "obs_off", o.data(), 2, &total)) && total == INT32_MAX); }
  { V o{0, INT32_MAX, INT32_MAX}; CHECK(accepted(check_csr(E, "obs_off", o.data(), 2, &total)) && total == INT32_MAX); }
  // does not start at 0
  { V o{1, 2, 3}; CHECK(rejected(check_csr(E, "conn_off", o.data(), 2, &total), "conn_off") && total == 0); }
  { V o{-1, 2, 3}; CHECK(rejected(check_csr(E, "conn_off", o.data(), 2, &total), "conn_off")); }
  // a decrease in the first, a middle and the last position
  { V o{0, -1, 3, 4}; CHECK(rejected(check_csr(E, "prev_off", o.data(), 3, &total), "prev_off")); }
  { V o{0, 2, 1, 4}; CHECK(rejected(check_csr(E, "prev_off", o.data(), 3, &total), "prev_off")); }
  { V o{0, 2, 3, 2}; CHECK(rejected(check_csr(E, "prev_off", o.data(), 3, &total), "prev_off") && total == 0); }
  { V o{0, INT32_MAX, INT32_MIN}; CHECK(rejected(check_csr(E, "prev_off", o.data(), 2, &total), "prev_off")); }
  // the four offset arrays of one entry stay distinguishable
  for (const char* name : {"slot_off", "obs_off", "conn_off", "prev_off"}) {
    V o{0, 2, 1};
    const std::string m = check_csr(E, name, o.data(), 2, &total);
    CHECK(rejected(m, name));
    for (const char* other : {"slot_off", "obs_off", "conn_off", "prev_off"})
      if (std::string(other) != name) CHECK(m.find(other) == std::string::npos);
  }
}

static void index_cases() {
  CHECK(accepted(check_index(E, "obs_kf", nullptr, 0, 5)));
  CHECK(accepted(check_index(E, "obs_kf", nullptr, 0, 0)));
  { V v{0, 4, 2}; CHECK(accepted(check_index(E, "obs_kf", v.data(), 3, 5))); }                                    // both bounds
  { V v{0, 4, 2}; CHECK(accepted(check_index(E, "obs_kf", v.data(), 3, 5, true))); }
  { V v{2, 5}; CHECK(rejected(check_index(E, "obs_kf", v.data(), 2, 5), "obs_kf")); }                              // one past the upper bound
  { V v{2, 5}; CHECK(rejected(check_index(E, "obs_kf", v.data(), 2, 5, true), "obs_kf")); }
  { V v{-1, 2}; CHECK(rejected(check_index(E, "obs_kf", v.data(), 2, 5), "obs_kf")); }                             // one past the lower bound
  { V v{-1, 2}; CHECK(accepted(check_index(E, "slot_pt", v.data(), 2, 5, true))); }                                // -1: none
  { V v{2, -2}; CHECK(rejected(check_index(E, "slot_pt", v.data(), 2, 5, true), "slot_pt")); }                     // one past it with the exemption
  { V v{0}; CHECK(rejected(check_index(E, "slot_pt", v.data(), 1, 0), "slot_pt")); }                               // nothing to index
  { V v{-1}; CHECK(accepted(check_index(E, "slot_pt", v.data(), 1, 0, true))); }
  { V v{INT32_MAX - 1}; CHECK(accepted(check_index(E, "slot_pt", v.data(), 1, INT32_MAX))); }
  { V v{INT32_MAX}; CHECK(rejected(check_index(E, "slot_pt", v.data(), 1, INT32_MAX), "slot_pt")); }
  { V v{INT32_MIN}; CHECK(rejected(check_index(E, "slot_pt", v.data(), 1, 5, true), "slot_pt")); }
  // rows the entry does not read are not checked
  { V v{9, 1, -7}; const auto odd = [](int i) { return i == 1; }; CHECK(accepted(check_index_if(E, "ref_kf", v.data(), 3, 5, odd))); }
  { V v{9, 5, -7}; const auto odd = [](int i) { return i == 1; }; CHECK(rejected(check_index_if(E, "ref_kf", v.data(), 3, 5, odd), "ref_kf")); }
  { V v{0, 7, INT32_MAX}; CHECK(accepted(check_not_negative(E, "obs_level", v.data(), 3))); }
  { V v{0, -1}; CHECK(rejected(check_not_negative(E, "obs_level", v.data(), 2), "obs_level")); }
  CHECK(accepted(check_not_negative(E, "obs_level", nullptr, 0)));
}

static void listed_once_cases() {
  CHECK(accepted(check_listed_once(E, "tgt_kf", nullptr, 0, 0)));
  CHECK(accepted(check_listed_once(E, "tgt_kf", nullptr, 0, 4)));
  { V v{3, 0}; CHECK(accepted(check_listed_once(E, "tgt_kf", v.data(), 2, 4))); }                                 // (a list need not name every index)
  { V v{3, 0, 1, 2}; CHECK(accepted(check_listed_once(E, "tgt_kf", v.data(), 4, 4))); }
  { V v{3, 0, 3}; CHECK(rejected(check_listed_once(E, "tgt_kf", v.data(), 3, 4), "tgt_kf")); }                     // a duplicate
  { V v{0, 0}; CHECK(rejected(check_listed_once(E, "tgt_kf", v.data(), 2, 1), "tgt_kf")); }
  { V v{0, 4}; CHECK(rejected(check_listed_once(E, "tgt_kf", v.data(), 2, 4), "tgt_kf")); }
  { V v{-1, 2}; CHECK(rejected(check_listed_once(E, "tgt_kf", v.data(), 2, 4), "tgt_kf")); }
  { V v{0}; CHECK(rejected(check_listed_once(E, "tgt_kf", v.data(), 1, 0), "tgt_kf")); }
}

static void permutation_cases() {
  CHECK(accepted(check_permutation(E, "kf_rank", nullptr, 0)));
  { V v{0}; CHECK(accepted(check_permutation(E, "kf_rank", v.data(), 1))); }
  { V v{2, 0, 3, 1}; CHECK(accepted(check_permutation(E, "kf_rank", v.data(), 4))); }
  { V v{2, 0, 2, 1}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 4), "kf_rank")); }                   // repeats 2, which also skips 3
  { V v{0, 1, 1}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 3), "kf_rank")); }
  { V v{1, 2, 3}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 3), "kf_rank")); }                      // skips 0: goes one past the end
  { V v{0, -1, 2}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 3), "kf_rank")); }
  { V v{1}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 1), "kf_rank")); }
  { V v{INT32_MAX, INT32_MIN}; CHECK(rejected(check_permutation(E, "kf_rank", v.data(), 2), "kf_rank")); }
}

int main() {
  csr_cases();
  index_cases();
  listed_once_cases();
  permutation_cases();
  std::printf("%d argument checks checked\n", g_checked);
  return 0;
}
