// Stochastic rounding fp32 -> bf16 for the fused sparse optimizers (include/trs_abi.h, "stochastic rounding").
//
// The rule is integer arithmetic on the bits of the value plus 16 bits of a counter-based hash, so the host computes
// exactly what the kernels compute:  bits(x) + r, then drop the low 16 bits; r is a pure function of (seed, t, i) --
// i the element's position in the table, t the update number of the table -- and of nothing a launch is free to choose.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define TRS_SR_HD __host__ __device__ __forceinline__
#else
#define TRS_SR_HD inline
#endif

namespace trs {

struct Philox4 {
  uint32_t w[4];
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): counter c0..c3, key k0, k1
TRS_SR_HD Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// the four words that serve table elements 8q .. 8q+7 (one 16-byte vector of bf16) in update t
TRS_SR_HD Philox4 sr_words(int64_t q, uint64_t seed, uint64_t t) {
  return philox4x32_10((uint32_t)(uint64_t)q, (uint32_t)((uint64_t)q >> 32), (uint32_t)t, (uint32_t)(t >> 32),
                       (uint32_t)seed, (uint32_t)(seed >> 32));
}

// r of element j = i & 7 of the vector: word j >> 1, low half for even j, high half for odd j
TRS_SR_HD uint32_t sr_pick(const Philox4& p, int j) {
  const uint32_t w = p.w[j >> 1];
  return (j & 1) ? (w >> 16) : (w & 0xffffu);
}

// (bits + r) >> 16; inf / NaN (exponent all ones) are truncated, so they stay what they are
TRS_SR_HD uint32_t sr_bits(uint32_t u, uint32_t r) {
  return ((u & 0x7f800000u) == 0x7f800000u) ? (u >> 16) : ((u + r) >> 16);
}

TRS_SR_HD uint32_t sr_f32_bits(float x) {
  union { float f; uint32_t u; } c;
  c.f = x;
  return c.u;
}

// bf16 bits of the fp32 value x destined for table element i = table_row * E + column in update t of that table
TRS_SR_HD uint16_t sr_bf16(float x, int64_t i, uint64_t seed, uint64_t t) {
  const Philox4 p = sr_words(i >> 3, seed, t);
  return (uint16_t)sr_bits(sr_f32_bits(x), sr_pick(p, (int)(i & 7)));
}

// the eight values of one 16-byte vector (elements 8q .. 8q+7), packed as Vec16<bf16_t> packs them: ONE hash call
TRS_SR_HD void sr_bf16x8(const float* x, int64_t q, uint64_t seed, uint64_t t, uint32_t* out4) {
  const Philox4 p = sr_words(q, seed, t);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = sr_bits(sr_f32_bits(x[2 * k]), p.w[k] & 0xffffu);
    const uint32_t hi = sr_bits(sr_f32_bits(x[2 * k + 1]), p.w[k] >> 16);
    out4[k] = lo | (hi << 16);
  }
}

}  // namespace trs
