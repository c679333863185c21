// What the padded (bag.hip) and the ragged (bag_ragged.hip) bag kernels share: modes, queue thresholds, the max rule; and
// the bounds of a ragged bag, which the ragged attention kernels (attn_pool.hip) read the same way.
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

// [begin, end) of ragged bag b (bag_ragged.hip, the ragged kernels of attn_pool.hip), clamped to [0, n]; end < begin:
// empty.  Either defect raises the flag.
__device__ __forceinline__ void bag_ragged_bounds(const void* __restrict__ offsets, bool off64, int64_t n_off, int64_t b,
                                                  int64_t n, int32_t* __restrict__ err_flag, int64_t* beg, int64_t* end) {
  int64_t o0, o1 = n;
  if (off64) {
    o0 = ((const int64_t*)offsets)[b];
    if (b + 1 < n_off) o1 = ((const int64_t*)offsets)[b + 1];
  } else {
    o0 = (int64_t)((const int32_t*)offsets)[b];
    if (b + 1 < n_off) o1 = (int64_t)((const int32_t*)offsets)[b + 1];
  }
  if (o0 < 0 || o0 > n || o1 < 0 || o1 > n || o1 < o0) {
    if (err_flag != nullptr) *err_flag = 1;
    o0 = o0 < 0 ? 0 : (o0 > n ? n : o0);
    o1 = o1 < 0 ? 0 : (o1 > n ? n : o1);
    if (o1 < o0) o1 = o0;
  }
  *beg = o0;
  *end = o1;
}

}  // namespace trs
