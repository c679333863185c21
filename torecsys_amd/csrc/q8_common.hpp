// Row-wise int8 (Q8) table rows: the byte layout and the register-level pieces the Q8 kernels (q8.hip) share.
//
// A row of E columns is S = round_up(E + 8, 16) bytes: E codes, fp32 scale, fp32 bias (little endian), zero padding.  On the
// lane-group path E = 16 * L, so S = 16 * (L + 1): lane i of the group owns code vector i (16 codes -> 16 fp32 values) and
// the tail is the first 8 bytes of vector L of the same row -- every lane of the group asks for the same 8 bytes, which
// the memory pipe serves as one access, and a row is one contiguous 16 * L + 8 byte read.
// x[e] = float(c[e]) * scale + bias, the product and the sum each rounded (the library is built with -ffp-contract=off).
#pragma once
#include "trs_common.hpp"

namespace trs {

__host__ __device__ inline int64_t q8_stride(int E) { return ((int64_t)E + 8 + 15) / 16 * 16; }

struct Q8Vec {      // what one lane holds of one row: its 16 codes and the row's (scale, bias)
  uint4 c;
  uint2 t;
};

// lane `lane_v` of the L-lane group of row r (< 0: a zero row -- codes 0, scale 0, bias 0 dequantize to +0)
template <int L, bool STREAM>
__device__ __forceinline__ Q8Vec q8_load(const uint4* __restrict__ q, int64_t r, int lane_v) {
  Q8Vec v;
  v.c = make_uint4(0, 0, 0, 0);
  v.t = make_uint2(0, 0);
  if (r >= 0) {
    const uint4* row = q + r * (L + 1);
    if (STREAM) {
      typedef __attribute__((ext_vector_type(2))) unsigned int u32x2;
      v.c = load_stream(row + lane_v);
      const u32x2 w = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(row + L));
      v.t = make_uint2(w.x, w.y);
    } else {
      v.c = row[lane_v];
      v.t = *reinterpret_cast<const uint2*>(row + L);
    }
  }
  return v;
}

// 16 codes -> 16 fp32 values: byte k of a word is (w >> 8k) & 0xff, which the compiler turns into v_cvt_f32_ubyte<k>
__device__ __forceinline__ void q8_unpack16(const Q8Vec& v, float* x) {
  const float scale = __uint_as_float(v.t.x), bias = __uint_as_float(v.t.y);
  const uint32_t w[4] = {v.c.x, v.c.y, v.c.z, v.c.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[4 * i + 0] = (float)(w[i] & 0xffu) * scale + bias;
    x[4 * i + 1] = (float)((w[i] >> 8) & 0xffu) * scale + bias;
    x[4 * i + 2] = (float)((w[i] >> 16) & 0xffu) * scale + bias;
    x[4 * i + 3] = (float)(w[i] >> 24) * scale + bias;
  }
}

// a lane's 16 values rounded once to OutT and stored as whole 16-byte vectors (4 for fp32, 2 for bf16) at dst
template <typename OutT, bool NT>
__device__ __forceinline__ void q8_store16(OutT* __restrict__ dst, const float* x) {
  constexpr int VE = Vec16<OutT>::VE;
  uint4* d = reinterpret_cast<uint4*>(dst);
#pragma unroll
  for (int j = 0; j < 16 / VE; ++j) {
    const uint4 u = Vec16<OutT>::pack(x + j * VE);
    if (NT) store_stream(d + j, u);
    else d[j] = u;
  }
}

// the element path: one value of row r (r*S is 16-byte aligned, E is not: the tail is assembled from bytes)
__device__ __forceinline__ float q8_f32_at(const uint8_t* __restrict__ p) {
  return __uint_as_float((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
}
__device__ __forceinline__ float q8_elem(const uint8_t* __restrict__ q, int64_t r, int64_t S, int E, int e) {
  const uint8_t* row = q + r * S;
  return (float)row[e] * q8_f32_at(row + E) + q8_f32_at(row + E + 4);
}

// ---- Q8 rows as matrix-core operands (topk.hip, target_rank.hip)
// the 4 codes of a word as fp32 (v_cvt_f32_ubyte<k>) and as bf16: a code has 8 significant bits, its fp32 form ends in 16
// zero bits and the high half IS the bf16
__device__ __forceinline__ uint4 tk_codes_f32(uint32_t w) {
  return make_uint4(__float_as_uint((float)(w & 0xffu)), __float_as_uint((float)((w >> 8) & 0xffu)),
                    __float_as_uint((float)((w >> 16) & 0xffu)), __float_as_uint((float)(w >> 24)));
}
__device__ __forceinline__ uint2 tk_codes_bf16(uint32_t w) {
  const uint4 f = tk_codes_f32(w);
  return make_uint2((f.x >> 16) | f.y, (f.z >> 16) | f.w);
}
__device__ __forceinline__ uint32_t tk_word(const uint4& v, int i) { return i == 0 ? v.x : i == 1 ? v.y : i == 2 ? v.z : v.w; }

}  // namespace trs
