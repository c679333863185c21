// Mixture-of-experts gating (MoE / MMoE): with z[b,g,:] = logits[b,g,:] + bias[g,:] (logits: the fp32 result of ONE GEMM over
// the stacked gate weights) and e[b,:] the concatenated expert outputs,
//   forward   out[b,g,k] = softmax_k(z[b,g,:])[k] * e[b,k]
//   backward  p recomputed from the logits;  t = gout * e;  glogits = p * (t - sum_k p t);  gexperts[b,k] = sum_g gout p
// The reference (layers/ctr/mixture_of_experts.py:137-160) runs G Linear + Softmax, G unflattens, a cat and an einsum, each
// with its own backward.  Everything between the loads and the final stores is fp32; the row maximum is subtracted.
//
// Vector path, as bag_pool_group_kernel (bag.hip): a row of K values of T is NV = K*sizeof(T)/16 sixteen-byte vectors; a GROUP
// of L = min(64, pow2 >= NV) adjacent lanes owns a sample for all G gates, lane l the vectors l, l + L, ... (R <= 4 of them,
// at most MOE_LANE_COLS columns: K <= MOE_GATE_MAX_K).  The e row is loaded once and stays in registers, per gate the fp32
// logits row comes in 16-byte loads, maximum and sums are folded with __shfl_xor inside the group, the backward keeps its
// gexperts sums in registers across the gates.  No LDS, no atomics, fixed summation order.
// HBM-bound: forward reads B*G*K*4 + B*K*s and writes B*G*K*s; backward reads B*G*K*(4 + s) + B*K*s and writes
// B*G*K*s + B*K*s (s = sizeof(T)); the G*K bias stays in cache.
//
// General path (any K >= 1: rows that are not whole vectors, K above the cap, unaligned pointers): one wave per row, lanes
// stride the columns with element loads, the statistics of a row take passes of their own over it (L2 hits).  The backward
// owns a sample per wave and covers the columns in tiles of 64 * MOE_TILE_COLS so that the gexperts sums stay in registers;
// beyond one tile (K > 512) the statistics of a gate are recomputed per tile.
#include <cmath>

#include "trs_common.hpp"

namespace trs {

constexpr int MOE_LANE_COLS = 16;                       // columns a lane of the vector path keeps in registers
constexpr int MOE_GATE_MAX_K = 64 * MOE_LANE_COLS;      // = functional.MOE_GATE_MAX_K
constexpr int MOE_TILE_COLS = 8;                        // general backward: columns per lane and tile

// z[0..VE) = logits + bias for vector v of row `row` (NV vectors of T per row); fp32 logits are VE/4 16-byte vectors
template <typename T>
__device__ __forceinline__ void moe_load_z(const uint4* __restrict__ logits, const uint4* __restrict__ bias, int64_t row,
                                           int g, int NV, int v, float* z) {
  constexpr int VE = Vec16<T>::VE;
  constexpr int Q = VE / 4;
  const uint4* src = logits + (row * NV + v) * Q;
#pragma unroll
  for (int q = 0; q < Q; ++q) Vec16<float>::unpack(load_stream(src + q), z + 4 * q);
  if (bias != nullptr) {
    float bv[VE];
    Vec16<T>::unpack(bias[(int64_t)g * NV + v], bv);
#pragma unroll
    for (int k = 0; k < VE; ++k) z[k] += bv[k];
  }
}

template <typename T, int LOG2L, int R, bool BWD>
__global__ __launch_bounds__(256) void moe_gate_group_kernel(const uint4* __restrict__ logits,
                                                             const uint4* __restrict__ bias,
                                                             const uint4* __restrict__ experts,
                                                             const uint4* __restrict__ gout, int64_t B, int G, int NV,
                                                             uint4* __restrict__ out /* BWD: glogits */,
                                                             uint4* __restrict__ gexperts) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < B; b += groups) {
    float e[R][VE], acc[R][VE];
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int v = r * L + lane_v;
      uint4 ev = make_uint4(0, 0, 0, 0);
      if (v < NV) ev = experts[b * NV + v];
      Vec16<T>::unpack(ev, e[r]);
#pragma unroll
      for (int k = 0; k < VE; ++k) acc[r][k] = 0.f;
    }
    for (int g = 0; g < G; ++g) {
      const int64_t row = b * G + g;
      float p[R][VE];
      float m = -INFINITY;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int v = r * L + lane_v;
        if (v < NV) {
          moe_load_z<T>(logits, bias, row, g, NV, v, p[r]);
        } else {
#pragma unroll
          for (int k = 0; k < VE; ++k) p[r][k] = -INFINITY;
        }
#pragma unroll
        for (int k = 0; k < VE; ++k) m = fmaxf(m, p[r][k]);
      }
      m = group_max_up<L>(m);
      float s = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int k = 0; k < VE; ++k) {
          p[r][k] = expf(p[r][k] - m);        // columns past the row: exp(-inf) = 0
          s += p[r][k];
        }
      }
      const float inv = 1.f / group_sum_up<L>(s);
      if (!BWD) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int v = r * L + lane_v;
          float o[VE];
#pragma unroll
          for (int k = 0; k < VE; ++k) o[k] = p[r][k] * inv * e[r][k];
          if (v < NV) store_stream(&out[row * NV + v], Vec16<T>::pack(o));
        }
      } else {
        float t[R][VE];
        float d = 0.f;
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int v = r * L + lane_v;
          uint4 gv = make_uint4(0, 0, 0, 0);
          if (v < NV) gv = load_stream(&gout[row * NV + v]);
          float go[VE];
          Vec16<T>::unpack(gv, go);
#pragma unroll
          for (int k = 0; k < VE; ++k) {
            p[r][k] *= inv;
            t[r][k] = go[k] * e[r][k];
            d += p[r][k] * t[r][k];
            acc[r][k] += go[k] * p[r][k];
          }
        }
        d = group_sum_up<L>(d);
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const int v = r * L + lane_v;
          float o[VE];
#pragma unroll
          for (int k = 0; k < VE; ++k) o[k] = p[r][k] * (t[r][k] - d);
          if (v < NV) store_stream(&out[row * NV + v], Vec16<T>::pack(o));
        }
      }
    }
    if (BWD) {
#pragma unroll
      for (int r = 0; r < R; ++r) {
        const int v = r * L + lane_v;
        if (v < NV) gexperts[b * NV + v] = Vec16<T>::pack(acc[r]);
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// general path: element loads, one wave per row (forward) or per sample (backward)

template <typename T>
__device__ __forceinline__ float moe_z(const float* __restrict__ zrow, const T* __restrict__ brow, int k) {
  return brow != nullptr ? zrow[k] + to_f32(brow[k]) : zrow[k];
}

template <typename T>
__global__ __launch_bounds__(256) void moe_gate_fwd_elem_kernel(const float* __restrict__ logits,
                                                                const T* __restrict__ bias,
                                                                const T* __restrict__ experts, int64_t B, int G, int K,
                                                                T* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const int64_t rows = B * G;
  for (int64_t row = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; row < rows; row += waves) {
    const int64_t b = row / G;
    const int g = (int)(row - b * G);
    const float* zrow = logits + row * K;
    const T* brow = bias != nullptr ? bias + (int64_t)g * K : nullptr;
    const T* erow = experts + b * K;
    T* orow = out + row * K;
    float m = -INFINITY;
    for (int k = lane; k < K; k += 64) m = fmaxf(m, moe_z<T>(zrow, brow, k));
    m = group_max_up<64>(m);
    float s = 0.f;
    for (int k = lane; k < K; k += 64) s += expf(moe_z<T>(zrow, brow, k) - m);
    const float inv = 1.f / group_sum_up<64>(s);
    for (int k = lane; k < K; k += 64)
      orow[k] = from_f32<T>(expf(moe_z<T>(zrow, brow, k) - m) * inv * to_f32(erow[k]));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void moe_gate_bwd_elem_kernel(const float* __restrict__ logits,
                                                                const T* __restrict__ bias,
                                                                const T* __restrict__ experts,
                                                                const T* __restrict__ gout, int64_t B, int G, int K,
                                                                T* __restrict__ glogits, T* __restrict__ gexperts) {
  constexpr int C = MOE_TILE_COLS;
  const int lane = threadIdx.x & 63;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < B; b += waves) {
    const T* erow = experts + b * K;
    for (int k0 = 0; k0 < K; k0 += 64 * C) {
      float acc[C];
#pragma unroll
      for (int j = 0; j < C; ++j) acc[j] = 0.f;
      for (int g = 0; g < G; ++g) {
        const int64_t row = b * G + g;
        const float* zrow = logits + row * K;
        const T* brow = bias != nullptr ? bias + (int64_t)g * K : nullptr;
        const T* grow = gout + row * K;
        float m = -INFINITY;
        for (int k = lane; k < K; k += 64) m = fmaxf(m, moe_z<T>(zrow, brow, k));
        m = group_max_up<64>(m);
        float s = 0.f, u = 0.f;
        for (int k = lane; k < K; k += 64) {
          const float x = expf(moe_z<T>(zrow, brow, k) - m);
          s += x;
          u += x * (to_f32(grow[k]) * to_f32(erow[k]));
        }
        const float inv = 1.f / group_sum_up<64>(s);
        const float d = group_sum_up<64>(u) * inv;
#pragma unroll
        for (int j = 0; j < C; ++j) {
          const int k = k0 + lane + 64 * j;
          if (k < K) {
            const float p = expf(moe_z<T>(zrow, brow, k) - m) * inv;
            const float go = to_f32(grow[k]);
            glogits[row * K + k] = from_f32<T>(p * (go * to_f32(erow[k]) - d));
            acc[j] += go * p;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < C; ++j) {
        const int k = k0 + lane + 64 * j;
        if (k < K) gexperts[b * K + k] = from_f32<T>(acc[j]);
      }
    }
  }
}

// rows of whole 16-byte vectors of T, at most MOE_LANE_COLS columns per lane of a 64-lane group
static bool moe_vector_shape(int K, int dtype) {
  return K >= 1 && K % 4 == 0 && ((int64_t)K * dtype_size(dtype)) % 16 == 0 && K <= MOE_GATE_MAX_K;
}

// which branch the last launch of this thread took (trs_moe_gate_last_path): 0 none yet, 1 vector, 2 element
static thread_local int moe_last_path = 0;

template <typename T, bool BWD>
static int moe_gate_launch(const float* logits, const void* bias, const void* experts, const void* gout, int64_t B, int G,
                           int K, void* out, void* gexperts, hipStream_t s, const char* what) {
  const int dtype = sizeof(T) == 4 ? TRS_F32 : TRS_BF16;
  const bool aligned = aligned16(logits) && aligned16(bias) && aligned16(experts) && aligned16(gout) && aligned16(out) &&
                       aligned16(gexperts);
  if (moe_vector_shape(K, dtype) && aligned) {
    moe_last_path = 1;
    const int NV = K / Vec16<T>::VE;
    int lg = 0;
    while ((1 << lg) < NV && lg < 6) ++lg;
    const int per_lane = (NV + (1 << lg) - 1) >> lg;      // 1 below 64 lanes; <= 4 (fp32) or 2 (bf16) by the cap
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    auto launch = [&](auto lg_c, auto r_c) {
      hipLaunchKernelGGL((moe_gate_group_kernel<T, decltype(lg_c)::value, decltype(r_c)::value, BWD>), dim3(grid),
                         dim3(256), 0, s, (const uint4*)logits, (const uint4*)bias, (const uint4*)experts,
                         (const uint4*)gout, B, G, NV, (uint4*)out, (uint4*)gexperts);
    };
    if (lg < 6) dispatch_int<0, 1, 2, 3, 4, 5>(lg, [&](auto lg_c) { launch(lg_c, int_c<1>{}); });
    else if (per_lane == 1) launch(int_c<6>{}, int_c<1>{});
    else if (per_lane == 2) launch(int_c<6>{}, int_c<2>{});
    else if constexpr (sizeof(T) == 4) launch(int_c<6>{}, int_c<4>{});      // 3 or 4 vectors of 4 floats
  } else if (!BWD) {
    moe_last_path = 2;
    hipLaunchKernelGGL((moe_gate_fwd_elem_kernel<T>), dim3(stream_grid(B * G * 64, 256, 256 * 16)), dim3(256), 0, s,
                       logits, (const T*)bias, (const T*)experts, B, G, K, (T*)out);
  } else {
    moe_last_path = 2;
    hipLaunchKernelGGL((moe_gate_bwd_elem_kernel<T>), dim3(stream_grid(B * 64, 256, 256 * 16)), dim3(256), 0, s, logits,
                       (const T*)bias, (const T*)experts, (const T*)gout, B, G, K, (T*)out, (T*)gexperts);
  }
  return check_launch(what);
}

}  // namespace trs

using namespace trs;

extern "C" int trs_moe_gate_vector_shape(int32_t K, int32_t dtype) {
  if (dtype != TRS_F32 && dtype != TRS_BF16) return 0;
  return moe_vector_shape(K, dtype) ? 1 : 0;
}

extern "C" int trs_moe_gate_last_path(void) { return moe_last_path; }

extern "C" int trs_moe_gate_fwd(const float* logits, const void* bias, const void* experts, int64_t B, int32_t G, int32_t K,
                                int32_t dtype, void* out, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(logits && experts && out, TRS_EINVAL, "moe_gate_fwd: NULL pointer");
  TRS_REQUIRE(B > 0, TRS_EINVAL, "moe_gate_fwd: bad size B=%lld", (long long)B);
  TRS_REQUIRE(G >= 1, TRS_EINVAL, "moe_gate_fwd: bad size G=%d", G);
  TRS_REQUIRE(K >= 1, TRS_EINVAL, "moe_gate_fwd: bad size K=%d", K);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "moe_gate_fwd: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32)
    return moe_gate_launch<float, false>(logits, bias, experts, nullptr, B, G, K, out, nullptr, s, "moe_gate_fwd");
  return moe_gate_launch<bf16_t, false>(logits, bias, experts, nullptr, B, G, K, out, nullptr, s, "moe_gate_fwd");
}

extern "C" int trs_moe_gate_bwd(const float* logits, const void* bias, const void* experts, const void* gout, int64_t B,
                                int32_t G, int32_t K, int32_t dtype, void* glogits, void* gexperts, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(logits && experts && gout && glogits && gexperts, TRS_EINVAL, "moe_gate_bwd: NULL pointer");
  TRS_REQUIRE(B > 0, TRS_EINVAL, "moe_gate_bwd: bad size B=%lld", (long long)B);
  TRS_REQUIRE(G >= 1, TRS_EINVAL, "moe_gate_bwd: bad size G=%d", G);
  TRS_REQUIRE(K >= 1, TRS_EINVAL, "moe_gate_bwd: bad size K=%d", K);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "moe_gate_bwd: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32)
    return moe_gate_launch<float, true>(logits, bias, experts, gout, B, G, K, glogits, gexperts, s, "moe_gate_bwd");
  return moe_gate_launch<bf16_t, true>(logits, bias, experts, gout, B, G, K, glogits, gexperts, s, "moe_gate_bwd");
}
