// ============================================================================
// orb_argcheck.h -- the checks a host-pointer entry point makes on its index arrays before any device work: CSR offsets, index
// ranges, "listed once" lists and permutations.  Standard library only, no HIP in it: a host compiler and its sanitizers reach
// all of it (tests/cpp/test_arg_checks.cpp).
//
// Every check returns the message of its failure, "<entry>: <array>... what is wrong", or an empty string when the array is
// acceptable (ORBHIP_ARG, common.h, turns a message into ORBHIP_EINVAL).  A check reads nothing when it has no rows / entries, so
// the array may then be NULL.
// ============================================================================
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace orbhip {

inline std::string arg_fail(const char* entry, const char* fmt, ...) {
  char what[192];
  va_list ap;
  va_start(ap, fmt);
  std::vsnprintf(what, sizeof(what), fmt, ap);
  va_end(ap);
  return std::string(entry) + ": " + what;
}

// CSR offsets of `rows` rows (rows + 1 entries): they start at 0 and do not decrease; *total = off[rows], the number of entries
inline std::string check_csr(const char* entry, const char* name, const int32_t* off, int rows, int* total) {
  *total = 0;
  if (rows <= 0) return {};
  if (off[0] != 0) return arg_fail(entry, "%s must start at 0 (it starts at %d)", name, off[0]);
  for (int r = 0; r < rows; r++)
    if (off[r] > off[r + 1]) return arg_fail(entry, "%s decreases at row %d (%d, then %d)", name, r, off[r], off[r + 1]);
  *total = off[rows];
  return {};
}

// v in [lo, n) as ONE unsigned comparison (lo is 0 or -1, n >= 0): these loops run over every observation of a map on the caller's thread
inline bool arg_in_range(int32_t v, int32_t lo, int32_t n) { return (uint32_t)v - (uint32_t)lo < (uint32_t)n - (uint32_t)lo; }

// v[i] in [0, n) - or -1, "none", where empty_ok - for every i
inline std::string check_index(const char* entry, const char* name, const int32_t* v, int count, int n, bool empty_ok = false) {
  const int32_t lo = empty_ok ? -1 : 0, hi = n > 0 ? n : 0;
  for (int i = 0; i < count; i++)
    if (!arg_in_range(v[i], lo, hi)) return arg_fail(entry, "%s[%d] = %d is out of range (%d to %d)", name, i, v[i], lo, n - 1);
  return {};
}
// the same for the i the entry reads: checked(i) says which those are
template <class Checked>
inline std::string check_index_if(const char* entry, const char* name, const int32_t* v, int count, int n, Checked checked) {
  const int32_t hi = n > 0 ? n : 0;
  for (int i = 0; i < count; i++)
    if (!arg_in_range(v[i], 0, hi) && checked(i)) return arg_fail(entry, "%s[%d] = %d is out of range (0 to %d)", name, i, v[i], n - 1);
  return {};
}

// no entry is negative (levels: their upper bound is not the entry's to know)
inline std::string check_not_negative(const char* entry, const char* name, const int32_t* v, int count) {
  for (int i = 0; i < count; i++)
    if (v[i] < 0) return arg_fail(entry, "%s[%d] = %d is negative", name, i, v[i]);
  return {};
}

// a list of indices into [0, n) that names each at most once
inline std::string check_listed_once(const char* entry, const char* name, const int32_t* v, int count, int n) {
  std::vector<int32_t> at((size_t)(n > 0 ? n : 0), -1);
  for (int i = 0; i < count; i++) {
    if (v[i] < 0 || v[i] >= n) return arg_fail(entry, "%s[%d] = %d is out of range (0 to %d)", name, i, v[i], n - 1);
    if (at[v[i]] >= 0) return arg_fail(entry, "%s lists %d twice (at %d and %d)", name, v[i], at[v[i]], i);
    at[v[i]] = i;
  }
  return {};
}

// v[0..n) holds every value of [0, n) once
inline std::string check_permutation(const char* entry, const char* name, const int32_t* v, int n) {
  std::vector<uint8_t> hit((size_t)(n > 0 ? n : 0), 0);
  for (int i = 0; i < n; i++) {
    if (v[i] < 0 || v[i] >= n || hit[v[i]]) return arg_fail(entry, "%s is not a permutation (entry %d = %d)", name, i, v[i]);
    hit[v[i]] = 1;
  }
  return {};
}

}  // namespace orbhip
