// Max over the 2^gsh adjacent lanes of a 16-lane row (multi-interest top-k and target ranks: a user's interests are 2^gsh
// adjacent anchors n of one MFMA accumulator group, topk.hip / target_rank.hip).  A butterfly on the vector ALU by DPP, no
// LDS traffic: lane ^ 1 and lane ^ 2 are quad permutations; once a quad is uniform the mirror of a half row is as good as
// lane ^ 4 and the mirror of the row as good as lane ^ 8.  Every lane of a group ends with the group's max.  fmaxf: a NaN
// loses to a number, the max of NaNs only is a NaN.  The max of floats is exact, so the result does not depend on the order.
#pragma once
#include <hip/hip_runtime.h>

namespace trs {

constexpr int GM_QUAD_1032 = 0xB1, GM_QUAD_2301 = 0x4E, GM_ROW_HALF_MIRROR = 0x141, GM_ROW_MIRROR = 0x140;

template <int CTRL>
__device__ __forceinline__ float gm_step(float v) {
  const int w = __float_as_int(v);
  return fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(w, w, CTRL, 0xf, 0xf, false)));
}

// gsh = log2 of the group width, 0 .. 4, the same in every lane
__device__ __forceinline__ float group_max(float v, int gsh) {
  if (gsh >= 1) v = gm_step<GM_QUAD_1032>(v);
  if (gsh >= 2) v = gm_step<GM_QUAD_2301>(v);
  if (gsh >= 3) v = gm_step<GM_ROW_HALF_MIRROR>(v);
  if (gsh >= 4) v = gm_step<GM_ROW_MIRROR>(v);
  return v;
}

// the smallest s with 2^s >= G, G in 1 .. 16
inline int gm_shift(int G) {
  int s = 0;
  while ((1 << s) < G) ++s;
  return s;
}

}  // namespace trs
