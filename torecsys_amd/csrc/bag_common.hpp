// What the padded (bag.hip) and the ragged (bag_ragged.hip) bag kernels share: modes, queue thresholds, the max rule.
#pragma once
#include <algorithm>
#include <cmath>

#include "trs_common.hpp"

namespace trs {

constexpr int BAG_SUM = 0, BAG_MEAN = 1, BAG_MAX = 2;
constexpr int BAG_LONG_ROW = 64;        // lookups a single lane group walks by itself (scatter.hip: LONG_ROW)
constexpr int BAG_LONG_CHUNK = 256;     // lookups per queue entry of a hot row (scatter.hip: LONG_CHUNK)
constexpr int BAG_LONG_ROW_ELEM = 32;   // the same for the one-thread-per-element path
constexpr size_t BAG_STREAM_BYTES = (size_t)512 << 20;      // twice the Infinity Cache: the STREAM rule of fm.hip

// ATen's rule (adaptive_max_pool): a later value replaces the running maximum when it is greater or NaN
__device__ __forceinline__ bool bag_takes(float v, float m) { return v > m || v != v; }

}  // namespace trs
