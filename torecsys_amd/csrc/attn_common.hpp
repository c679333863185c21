// What the per-sample attention kernels share (attn_pool.hip, self_attn.hip): one 256-thread workgroup owns one sample at
// a time on a persistent grid, operands live in LDS as fp32 with odd row strides, and every product is ap_gemm.
#pragma once
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <utility>

#include "trs_common.hpp"

namespace trs {

constexpr int AP_MAX_L = 64, AP_MAX_E = 128;
constexpr int AP_THREADS = 256;
constexpr size_t AP_MAX_LDS = 160 * 1024;

typedef __attribute__((ext_vector_type(8))) __bf16 ap_bf16x8;
typedef __attribute__((ext_vector_type(4))) float ap_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned ap_u32x4;

// C(m, n) (+)= alpha * sum_k A(m, k) B(k, n) (+ bias[n]) for m < M, n < N; element (i, j) of an operand is p[i * s_i + j * s_j].
// Called by all 256 threads; the caller synchronises.  BV (MFMA path only): B is bf16 in global memory with k contiguous
// (s_bk = 1), K % 8 == 0 and 16-byte aligned rows -- a lane's 8 values of a k-step are ONE 16-byte load instead of eight
// 2-byte ones (the projection's weight rows; the eight dependent-latency loads were most of the forward's time).
// ML (vector path only): adjacent lanes take adjacent m instead of adjacent n -- for the projection, whose B is the weight
// in global memory with n the strided index: a wave then reads two or three weight rows (broadcast) instead of 64 cache lines
// per load, and X with its odd row stride without LDS conflicts (fp32 forward at B = 65 536, L = 50, E = 64, H = 4:
// 47.0 -> 13.0 ms; with four outputs per thread 9.7 ms, profiles/attn_pool_kernels.md).
template <bool MF, bool BV = false, bool ML = false, typename TA, typename TB, typename TBias>
__device__ __forceinline__ void ap_gemm(float* C, int scm, int scn, bool acc, const TA* A, int sam, int sak, const TB* Bm,
                                        int sbk, int sbn, int M, int N, int K, float alpha, const TBias* bias) {
  if constexpr (MF) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r = lane & 15;
    const int nt = (N + 15) >> 4, tiles = ((M + 15) >> 4) * nt;
    for (int t = wave; t < tiles; t += AP_THREADS / 64) {
      const int m0 = (t / nt) << 4, n0 = (t - (t / nt) * nt) << 4;
      const int am = m0 + r, bn = n0 + r;
      ap_f32x4 c = {0.f, 0.f, 0.f, 0.f};
      for (int k0 = 0; k0 < K; k0 += 32) {
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int k = k0 + 8 * q + j;
          a[j] = (am < M && k < K) ? to_f32(A[am * sam + k * sak]) : 0.f;
        }
        const ap_u32x4 au = {f32x2_to_bf16x2_bits(a[0], a[1]), f32x2_to_bf16x2_bits(a[2], a[3]),
                             f32x2_to_bf16x2_bits(a[4], a[5]), f32x2_to_bf16x2_bits(a[6], a[7])};
        ap_u32x4 bu = {0u, 0u, 0u, 0u};
        if constexpr (BV) {
          if (bn < N && k0 + 8 * q < K) bu = *reinterpret_cast<const ap_u32x4*>(Bm + bn * sbn + k0 + 8 * q);
        } else {
          float b[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int k = k0 + 8 * q + j;
            b[j] = (bn < N && k < K) ? to_f32(Bm[k * sbk + bn * sbn]) : 0.f;
          }
          bu = ap_u32x4{f32x2_to_bf16x2_bits(b[0], b[1]), f32x2_to_bf16x2_bits(b[2], b[3]),
                        f32x2_to_bf16x2_bits(b[4], b[5]), f32x2_to_bf16x2_bits(b[6], b[7])};
        }
        c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(ap_bf16x8, au), __builtin_bit_cast(ap_bf16x8, bu), c,
                                                    0, 0, 0);
      }
      if (bn < N) {
        const float bv = bias != nullptr ? to_f32(bias[bn]) : 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = m0 + 4 * q + i;
          if (m < M) {
            float* dst = C + m * scm + bn * scn;
            const float v = alpha * c[i] + bv;
            *dst = acc ? *dst + v : v;
          }
        }
      }
    }
  } else {
    // four outputs per thread, columns n, n + N4, n + 2 N4, n + 3 N4 (adjacent lanes keep adjacent columns): one read of A
    // serves four FMAs; every output is still one sequential sum over k
    const int n4 = (N + 3) >> 2;
    for (int o = threadIdx.x; o < M * n4; o += AP_THREADS) {
      const int m = ML ? o % M : o / n4, g = ML ? o / M : o - m * n4;
      const TA* ap = A + m * sam;
      const TB* bp[4];
      float s[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = g + j * n4;
        bp[j] = Bm + (n < N ? n : N - 1) * sbn;      // past the edge: re-reads the last column, dropped at the store
        s[j] = 0.f;
      }
      for (int k = 0; k < K; ++k) {
        const float a = to_f32(ap[k * sak]);
#pragma unroll
        for (int j = 0; j < 4; ++j) s[j] = fmaf(a, to_f32(bp[j][k * sbk]), s[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int n = g + j * n4;
        if (n < N) {
          float* dst = C + m * scm + n * scn;
          const float v = alpha * s[j] + (bias != nullptr ? to_f32(bias[n]) : 0.f);
          *dst = acc ? *dst + v : v;
        }
      }
    }
  }
}

// S <- P = softmax_rows(S): 4 adjacent lanes per row (rows >= L idle but keep the shuffles whole)
__device__ __forceinline__ void ap_softmax_rows(float* S, int ss, int L) {
  const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
  const bool live = row < L;
  float* p = S + row * ss;
  float mx = -INFINITY;
  if (live)
    for (int c = sub; c < L; c += 4) mx = fmaxf(mx, p[c]);
  mx = fmaxf(mx, __shfl_xor(mx, 1, 64));
  mx = fmaxf(mx, __shfl_xor(mx, 2, 64));
  float sum = 0.f;
  if (live)
    for (int c = sub; c < L; c += 4) {
      const float e = expf(p[c] - mx);
      p[c] = e;
      sum += e;
    }
  sum = group_sum_up<4>(sum);
  if (live) {
    const float inv = 1.f / sum;
    for (int c = sub; c < L; c += 4) p[c] *= inv;
  }
}

// persistent grid: the workgroups that are resident at once, at most one per sample
// (asked of the runtime once per kernel and LDS size: the warm-up of a graph capture has then made every query)
inline int ap_resident(const void* kern, size_t lds) {
  static std::mutex mu;
  static std::map<std::pair<const void*, size_t>, int> seen;
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_pair(kern, lds);
  const auto it = seen.find(key);
  if (it != seen.end()) return it->second;
  if (lds > 64 * 1024) (void)hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)AP_MAX_LDS);
  const int res = resident_blocks(kern, AP_THREADS, lds);
  (void)hipGetLastError();
  seen[key] = res;
  return res;
}
inline int ap_blocks(const void* kern, size_t lds, int64_t B) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(B, ap_resident(kern, lds)));
}

}  // namespace trs
