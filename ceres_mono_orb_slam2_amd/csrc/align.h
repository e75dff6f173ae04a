// Rounding helpers shared by the HIP sources (common.h) and the host-only extractor plan (orb_geometry.h).
#pragma once
#include <cstddef>

namespace orbhip {

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace orbhip
