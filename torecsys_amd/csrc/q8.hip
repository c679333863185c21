// Row-wise int8 (Q8) embedding tables, forward only: the quantizer and the three read paths of a served table -- plain
// lookup, lookup + FM second order (+ first-order sum), pooled ragged bags -- dequantizing in registers.
// Format and dequantization rule: q8_common.hpp / include/trs_abi.h.
//
// Lane-group path (E = 16 * L, L a power of two <= 64; qrows and outputs 16-byte aligned).  One 16-byte load is 16 codes
// = 16 fp32 values per lane (a bf16 load is 8), so a row of E = 64 is 4 lanes wide and a wave instruction covers 16 rows
// (bf16: 8 lanes, 8 rows).  The row's (scale, bias) is an 8-byte load of the same address by every lane of the group.  A
// group owns one output row / sample / bag and keeps its 16 columns per lane in registers: no cross-lane traffic, no LDS.
// Rows in flight per lane (every row is a 16-byte and an 8-byte load, 6 VGPRs), from the compiler's register counts
// (-Rpass-analysis=kernel-resource-usage, E = 64, int64 ids, bf16 out):
//   embed_fm   s[16] + q[16] accumulators: CH = 2 -> 80 VGPRs, 6 waves per SIMD (12 rows in flight per SIMD lane);
//              CH = 4 -> 92, 5 waves (20 rows); CH = 8 -> 114, 4 waves (32 rows).  fm.hip's bf16 walk has 8 columns per lane,
//              fits 60 VGPRs at CH = 4 and keeps 8 waves; a Q8 lane carries twice the columns, so no depth reaches that
//              occupancy.  CH = 4 is kept as the middle: five waves still overlap one chunk's two dependent round trips
//              (ids, then rows) with the others' arithmetic.  The three depths were not raced on the device.
//   bag walk   s[16] only: CH = 4 -> 62 VGPRs, 8 waves; CH = 8 -> 86, 5 waves; CH = 16 -> 134, 3 waves.  CH = 8, the depth
//              of the bf16 kernel: most bags of a long-tailed batch are under 10 ids, one chunk instead of three.  The
//              second tier (one wave per queued bag) takes 2 * CH (140 VGPRs): that wave's registers buy latency hiding,
//              not occupancy.
//   gather     nothing carried between rows: 4 rows per lane, 63 VGPRs, 8 waves.
// Tables above 512 MiB (the threshold of fm.hip / bag_common.hpp) are read with streaming loads.
// Any other E, or a misaligned pointer: one thread per output element.
// Algorithmic bytes per looked-up row: id + S = E + 16 read (bf16: id + 2 E).
#include "bag_ragged.hpp"
#include "q8_common.hpp"

namespace trs {

constexpr int Q8_FM_CH = 4;
constexpr int Q8_BAG_CH = 8;
constexpr int Q8_BAG_LONG_CH = 2 * Q8_BAG_CH;
constexpr int Q8_GATHER_ROWS = 4;

// ------------------------------------------------------------------------------------------------ quantizer
__device__ __forceinline__ uint32_t q8_code(float x, float bias, float scale) {
  float c = 0.f;
  if (scale != 0.f) c = rintf((x - bias) / scale);      // round-half-even (v_rndne_f32); `/` is correctly rounded
  return (uint32_t)fminf(fmaxf(c, 0.f), 255.f);          // NaN -> 0
}

// one group of L lanes per row; a lane owns 16 columns.  min / max are folded by xor shuffles, widest step first.  A min
// or max of -0 counts as +0 (`+ 0.f`): IEEE leaves min(+0, -0) open, the stored bytes must not depend on the fold order.
template <typename T, int LOG2L>
__global__ __launch_bounds__(256) void q8_quantize_group_kernel(const uint4* __restrict__ table, int64_t V,
                                                                uint4* __restrict__ q) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; r < V; r += groups) {
    float x[16];
    const uint4* src = table + (r * L + lane_v) * (16 / VE);
#pragma unroll
    for (int j = 0; j < 16 / VE; ++j) Vec16<T>::unpack(src[j], x + j * VE);
    float mn = x[0], mx = x[0];
#pragma unroll
    for (int k = 1; k < 16; ++k) { mn = fminf(mn, x[k]); mx = fmaxf(mx, x[k]); }
#pragma unroll
    for (int m = L >> 1; m > 0; m >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, m, 64));
      mx = fmaxf(mx, __shfl_xor(mx, m, 64));
    }
    const float bias = mn + 0.f;
    const float scale = ((mx + 0.f) - bias) / 255.0f;
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      w[i] = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) w[i] |= q8_code(x[4 * i + k], bias, scale) << (8 * k);
    }
    uint4* row = q + r * (L + 1);
    row[lane_v] = make_uint4(w[0], w[1], w[2], w[3]);
    if (lane_v == 0) row[L] = make_uint4(__float_as_uint(scale), __float_as_uint(bias), 0, 0);
  }
}

// any E: one thread per row, bytes one by one
template <typename T>
__global__ __launch_bounds__(256) void q8_quantize_elem_kernel(const T* __restrict__ table, int64_t V, int E, int64_t S,
                                                               uint8_t* __restrict__ q) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < V; r += stride) {
    const T* src = table + r * E;
    float mn = to_f32(src[0]), mx = mn;
    for (int e = 1; e < E; ++e) { mn = fminf(mn, to_f32(src[e])); mx = fmaxf(mx, to_f32(src[e])); }
    const float bias = mn + 0.f;
    const float scale = ((mx + 0.f) - bias) / 255.0f;
    uint8_t* row = q + r * S;
    for (int e = 0; e < E; ++e) row[e] = (uint8_t)q8_code(to_f32(src[e]), bias, scale);
    const uint32_t sb = __float_as_uint(scale), bb = __float_as_uint(bias);
    for (int k = 0; k < 4; ++k) {
      row[E + k] = (uint8_t)(sb >> (8 * k));
      row[E + 4 + k] = (uint8_t)(bb >> (8 * k));
    }
    for (int64_t e = E + 8; e < S; ++e) row[e] = 0;
  }
}

// ------------------------------------------------------------------------------------------------ gather
// flat positions p = b*N + n; a group takes Q8_GATHER_ROWS positions a grid stride apart, all their loads issued first
template <typename OutT, typename IdxT, int LOG2L, bool STREAM>
__global__ __launch_bounds__(256) void q8_gather_group_kernel(const uint4* __restrict__ q, const IdxT* __restrict__ idx,
                                                              const int64_t* __restrict__ offsets,
                                                              OutT* __restrict__ out, int64_t rows, int N, int64_t V,
                                                              int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int UN = Q8_GATHER_ROWS;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t p0 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; p0 < rows; p0 += groups * UN) {
    Q8Vec v[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t p = p0 + u * groups;
      int64_t r = -1;
      if (p < rows) {
        // flat positions fit 32 bits (checked by the entry)
        r = load_row_id(idx, offsets, p, (int)((unsigned)p % (unsigned)N));
        if (r < 0 || r >= V) {
          if (err_flag != nullptr) *err_flag = 1;
          r = -1;
        }
      }
      v[u] = q8_load<L, STREAM>(q, r, lane_v);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int64_t p = p0 + u * groups;
      if (p < rows) {
        float x[16];
        q8_unpack16(v[u], x);
        // streaming store: the block is consumed by a later kernel, keep L2 for the table rows
        q8_store16<OutT, true>(out + (p * L + lane_v) * 16, x);
      }
    }
  }
}

template <typename OutT, typename IdxT>
__global__ __launch_bounds__(256) void q8_gather_elem_kernel(const uint8_t* __restrict__ q, const IdxT* __restrict__ idx,
                                                             const int64_t* __restrict__ offsets, OutT* __restrict__ out,
                                                             int64_t total, int E, int64_t S, int N, int64_t V,
                                                             int32_t* __restrict__ err_flag) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t p = udiv_fast(t, E, f32);
    const int e = (int)(t - p * E);
    const int n = (int)(p - udiv_fast(p, N, f32) * N);
    const int64_t r = load_row_id(idx, offsets, p, n);
    float x = 0.f;
    if (r < 0 || r >= V) {
      if (err_flag != nullptr) *err_flag = 1;
    } else {
      x = q8_elem(q, r, S, E, e);
    }
    out[t] = from_f32<OutT>(x);
  }
}

// ------------------------------------------------------------------------------------------------ lookup + FM
// One group per sample walks its N fields, Q8_FM_CH rows in flight; sum and sum of squares of the lane's 16 columns stay
// in registers, fields added in order.  The first-order values are fetched one field per lane (field n by lane n mod L)
// and folded over the group at the end, as fm.hip does.
template <typename OutT, typename IdxT, int LOG2L, bool STREAM>
__global__ __launch_bounds__(256) void q8_embed_fm_group_kernel(const uint4* __restrict__ q, const IdxT* __restrict__ idx,
                                                                const int64_t* __restrict__ offsets, int64_t B, int N,
                                                                int64_t V, OutT* __restrict__ emb, OutT* __restrict__ fm,
                                                                float* __restrict__ fm_sum,
                                                                const OutT* __restrict__ first_table,
                                                                OutT* __restrict__ first, int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int CH = Q8_FM_CH;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < B; b += groups) {
    float s[16], qq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { s[k] = 0.f; qq[k] = 0.f; }
    float f1 = 0.f;
    for (int n0 = 0; n0 < N; n0 += CH) {
      int64_t r[CH];
      Q8Vec v[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int n = n0 + c;
        r[c] = -1;
        if (n < N) {
          r[c] = load_row_id(idx, offsets, b * N + n, n);
          if (r[c] < 0 || r[c] >= V) {
            if (err_flag != nullptr) *err_flag = 1;
            r[c] = -1;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) v[c] = q8_load<L, STREAM>(q, r[c], lane_v);
      if (first_table != nullptr) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          if ((((n0 + c) & (L - 1)) == lane_v) && n0 + c < N && r[c] >= 0) f1 += to_f32(first_table[r[c]]);
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        const int n = n0 + c;
        if (n < N) {
          float x[16];
          q8_unpack16(v[c], x);
#pragma unroll
          for (int k = 0; k < 16; ++k) { s[k] += x[k]; qq[k] = fmaf(x[k], x[k], qq[k]); }
          if (emb != nullptr) q8_store16<OutT, true>(emb + ((b * N + n) * L + lane_v) * 16, x);
        }
      }
    }
    if (fm != nullptr) {
      float o[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) o[k] = 0.5f * (s[k] * s[k] - qq[k]);
      q8_store16<OutT, false>(fm + (b * L + lane_v) * 16, o);
    }
    if (fm_sum != nullptr) q8_store16<float, false>(fm_sum + (b * L + lane_v) * 16, s);
    if (first_table != nullptr) {
      f1 = group_sum_down<L>(f1);
      if (lane_v == 0) first[b] = from_f32<OutT>(f1);
    }
  }
}

template <typename OutT, typename IdxT>
__global__ __launch_bounds__(256) void q8_embed_fm_elem_kernel(const uint8_t* __restrict__ q, const IdxT* __restrict__ idx,
                                                               const int64_t* __restrict__ offsets, int64_t B, int N,
                                                               int E, int64_t S, int64_t V, OutT* __restrict__ emb,
                                                               OutT* __restrict__ fm, float* __restrict__ fm_sum,
                                                               const OutT* __restrict__ first_table,
                                                               OutT* __restrict__ first, int32_t* __restrict__ err_flag) {
  const int64_t total = B * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t b = udiv_fast(t, E, f32);
    const int e = (int)(t - b * E);
    float s = 0.f, qq = 0.f, f1 = 0.f;
    for (int n = 0; n < N; ++n) {
      const int64_t r = load_row_id(idx, offsets, b * N + n, n);
      const bool ok = r >= 0 && r < V;
      if (!ok && err_flag != nullptr) *err_flag = 1;
      const float x = ok ? q8_elem(q, r, S, E, e) : 0.f;
      s += x;
      qq = fmaf(x, x, qq);
      if (emb != nullptr) emb[(b * N + n) * E + e] = from_f32<OutT>(x);
      if (first_table != nullptr && e == 0 && ok) f1 += to_f32(first_table[r]);
    }
    if (fm != nullptr) fm[t] = from_f32<OutT>(0.5f * (s * s - qq));
    if (fm_sum != nullptr) fm_sum[t] = s;
    if (first_table != nullptr && e == 0) first[b] = from_f32<OutT>(f1);
  }
}

// ------------------------------------------------------------------------------------------------ ragged bags
// positions q0 = beg, beg + step, .. < end, CH rows in flight, added in that order; pad >= 0: a position that holds that id
// issues no load and does not count.  An id outside [0, V) reads as a zero row, raises the flag and counts.
// Positions are unsigned 32-bit: end <= n < 2^31 - 1 and a chunk spans at most 16 * 64 of them, so they never wrap.
template <typename IdxT, int LOG2L, int CH, bool STREAM>
__device__ __forceinline__ void q8_bag_walk(const uint4* __restrict__ q, const IdxT* __restrict__ ids, uint32_t beg,
                                            uint32_t end, uint32_t step, int64_t V, int64_t pad, int lane_v,
                                            int32_t* __restrict__ err_flag, float* s, int& cnt) {
  constexpr int L = 1 << LOG2L;
  for (uint32_t q0 = beg; q0 < end; q0 += CH * step) {
    int64_t r[CH];
    Q8Vec v[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const uint32_t p = q0 + c * step;
      r[c] = -1;
      if (p < end) {
        r[c] = (int64_t)ids[p];
        if (pad >= 0 && r[c] == pad) {
          r[c] = -1;
        } else {
          ++cnt;
          if (r[c] < 0 || r[c] >= V) {
            if (err_flag != nullptr) *err_flag = 1;
            r[c] = -1;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) v[c] = q8_load<L, STREAM>(q, r[c], lane_v);
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (r[c] >= 0) {      // a row that was not loaded would add +0: skipped
        float x[16];
        q8_unpack16(v[c], x);
#pragma unroll
        for (int k = 0; k < 16; ++k) s[k] += x[k];
      }
    }
  }
}

// mean: the sum over the live count, one correctly rounded division; an empty bag is a zero row
template <typename OutT, int LOG2L>
__device__ __forceinline__ void q8_bag_store(float* s, int cnt, bool mean, int64_t b, int lane_v, OutT* __restrict__ out,
                                             float* __restrict__ inv_cnt) {
  constexpr int L = 1 << LOG2L;
  if (mean) {
    const float c = (float)cnt;
    if (cnt > 0) {
#pragma unroll
      for (int k = 0; k < 16; ++k) s[k] = s[k] / c;
    }
    if (inv_cnt != nullptr && lane_v == 0) inv_cnt[b] = cnt > 0 ? 1.f / c : 0.f;
  }
  q8_store16<OutT, false>(out + (b * L + lane_v) * 16, s);
}

template <typename OutT, typename IdxT, int LOG2L, bool STREAM>
__global__ __launch_bounds__(256) void q8_bag_group_kernel(const uint4* __restrict__ q, const IdxT* __restrict__ ids,
                                                           int64_t n, const void* __restrict__ offsets, bool off64,
                                                           int64_t n_off, int64_t B, int64_t V, int64_t pad, bool mean,
                                                           OutT* __restrict__ out, float* __restrict__ inv_cnt,
                                                           int32_t* __restrict__ queue /* [0] = count */,
                                                           int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < B; b += groups) {
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, err_flag, &beg, &end);
    if (end - beg > BAG_RAGGED_LONG) {      // a whole wave takes it (q8_bag_long_kernel)
      if (lane_v == 0) queue[1 + atomicAdd(&queue[0], 1)] = (int32_t)b;
      continue;
    }
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.f;
    int cnt = 0;
    q8_bag_walk<IdxT, LOG2L, Q8_BAG_CH, STREAM>(q, ids, (uint32_t)beg, (uint32_t)end, 1, V, pad, lane_v, err_flag, s, cnt);
    q8_bag_store<OutT, LOG2L>(s, cnt, mean, b, lane_v, out, inv_cnt);
  }
}

// fixed grid, one wave per queued bag: its 64 / L groups stride the bag, the partials are folded across the groups by
// shuffles (steps L, 2L, .., 32) -- the order depends on the bag's length alone, not on the queue order
template <typename OutT, typename IdxT, int LOG2L, bool STREAM>
__global__ __launch_bounds__(256) void q8_bag_long_kernel(const uint4* __restrict__ q, const IdxT* __restrict__ ids,
                                                          int64_t n, const void* __restrict__ offsets, bool off64,
                                                          int64_t n_off, int64_t V, int64_t pad, bool mean,
                                                          OutT* __restrict__ out, float* __restrict__ inv_cnt,
                                                          const int32_t* __restrict__ queue,
                                                          int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63;
  const int lane_v = lane & (L - 1);
  const int grp = lane >> LOG2L;
  const int nlong = queue[0];
  const int waves = gridDim.x * (blockDim.x >> 6);
  for (int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < nlong; i += waves) {
    const int64_t b = queue[1 + i];
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, nullptr, &beg, &end);      // the flag was raised when b was queued
    float s[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = 0.f;
    int cnt = 0;
    q8_bag_walk<IdxT, LOG2L, Q8_BAG_LONG_CH, STREAM>(q, ids, (uint32_t)beg + grp, (uint32_t)end, G, V, pad, lane_v,
                                                     err_flag, s, cnt);
    cnt = across_groups_sum<L>(cnt);
#pragma unroll
    for (int k = 0; k < 16; ++k) s[k] = across_groups_sum<L>(s[k]);
    if (grp == 0) q8_bag_store<OutT, LOG2L>(s, cnt, mean, b, lane_v, out, inv_cnt);
  }
}

template <typename OutT, typename IdxT>
__global__ __launch_bounds__(256) void q8_bag_elem_kernel(const uint8_t* __restrict__ q, const IdxT* __restrict__ ids,
                                                          int64_t n, const void* __restrict__ offsets, bool off64,
                                                          int64_t n_off, int64_t B, int E, int64_t S, int64_t V,
                                                          int64_t pad, bool mean, OutT* __restrict__ out,
                                                          float* __restrict__ inv_cnt, int32_t* __restrict__ err_flag) {
  const int64_t total = B * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t b = udiv_fast(t, E, f32);
    const int e = (int)(t - b * E);
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, err_flag, &beg, &end);
    float s = 0.f;
    int cnt = 0;
    for (int64_t p = beg; p < end; ++p) {
      const int64_t r = (int64_t)ids[p];
      if (pad >= 0 && r == pad) continue;
      ++cnt;
      if (r < 0 || r >= V) {
        if (err_flag != nullptr) *err_flag = 1;
      } else {
        s += q8_elem(q, r, S, E, e);
      }
    }
    if (mean) {
      if (cnt > 0) s = s / (float)cnt;
      if (inv_cnt != nullptr && e == 0) inv_cnt[b] = cnt > 0 ? 1.f / (float)cnt : 0.f;
    }
    out[t] = from_f32<OutT>(s);
  }
}

// ------------------------------------------------------------------------------------------------ host
inline bool q8_streams(int64_t V, int E) { return (size_t)V * (size_t)q8_stride(E) > BAG_STREAM_BYTES; }

// f(std::bool_constant<STREAM>{}) for the table's size
template <typename F>
inline void q8_dispatch_stream(bool stream, F&& f) {
  if (stream) f(std::true_type{});
  else f(std::false_type{});
}

template <typename T>
static int q8_quantize_launch(const void* table, int64_t V, int E, void* qrows, hipStream_t s) {
  const int lg = log2_lanes(E);
  if (lg >= 0 && aligned16(table) && aligned16(qrows)) {
    dispatch_lanes(lg, [&](auto lg_c) {
      constexpr int LG = decltype(lg_c)::value;
      hipLaunchKernelGGL((q8_quantize_group_kernel<T, LG>), dim3(stream_grid(V << LG, 256, 256 * 16)), dim3(256), 0, s,
                         (const uint4*)table, V, (uint4*)qrows);
    });
  } else {
    hipLaunchKernelGGL((q8_quantize_elem_kernel<T>), dim3(stream_grid(V, 256, 256 * 16)), dim3(256), 0, s, (const T*)table,
                       V, E, q8_stride(E), (uint8_t*)qrows);
  }
  return check_launch("q8_quantize_rows");
}

template <typename OutT, typename IdxT>
static int q8_gather_launch(const void* qrows, int64_t V, int E, const IdxT* idx, const int64_t* offsets, int64_t rows,
                            int N, void* out, int32_t* err_flag, hipStream_t s) {
  const int lg = log2_lanes(E);
  if (lg >= 0 && aligned16(qrows) && aligned16(out)) {
    const int64_t items = ((rows + Q8_GATHER_ROWS - 1) / Q8_GATHER_ROWS) << lg;
    const int grid = stream_grid(items, 256, 256 * 32);
    dispatch_lanes(lg, [&](auto lg_c) {
      q8_dispatch_stream(q8_streams(V, E), [&](auto st_c) {
        hipLaunchKernelGGL((q8_gather_group_kernel<OutT, IdxT, decltype(lg_c)::value, decltype(st_c)::value>), dim3(grid),
                           dim3(256), 0, s, (const uint4*)qrows, idx, offsets, (OutT*)out, rows, N, V, err_flag);
      });
    });
  } else {
    const int64_t total = rows * E;
    hipLaunchKernelGGL((q8_gather_elem_kernel<OutT, IdxT>), dim3(stream_grid(total, 256, 256 * 32)), dim3(256), 0, s,
                       (const uint8_t*)qrows, idx, offsets, (OutT*)out, total, E, q8_stride(E), N, V, err_flag);
  }
  return check_launch("gather_rows_q8");
}

template <typename OutT, typename IdxT>
static int q8_embed_fm_launch(const void* qrows, int64_t V, int E, const IdxT* idx, const int64_t* offsets, int64_t B,
                              int N, void* emb, void* fm, float* fm_sum, const void* first_table, void* first,
                              int32_t* err_flag, hipStream_t s) {
  const int lg = log2_lanes(E);
  if (lg >= 0 && aligned16(qrows) && aligned16(emb) && aligned16(fm) && aligned16(fm_sum)) {
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    dispatch_lanes(lg, [&](auto lg_c) {
      q8_dispatch_stream(q8_streams(V, E), [&](auto st_c) {
        hipLaunchKernelGGL((q8_embed_fm_group_kernel<OutT, IdxT, decltype(lg_c)::value, decltype(st_c)::value>),
                           dim3(grid), dim3(256), 0, s, (const uint4*)qrows, idx, offsets, B, N, V, (OutT*)emb, (OutT*)fm,
                           fm_sum, (const OutT*)first_table, (OutT*)first, err_flag);
      });
    });
  } else {
    hipLaunchKernelGGL((q8_embed_fm_elem_kernel<OutT, IdxT>), dim3(stream_grid(B * E, 256, 256 * 16)), dim3(256), 0, s,
                       (const uint8_t*)qrows, idx, offsets, B, N, E, q8_stride(E), V, (OutT*)emb, (OutT*)fm, fm_sum,
                       (const OutT*)first_table, (OutT*)first, err_flag);
  }
  return check_launch("embed_fm_q8");
}

template <typename OutT, typename IdxT>
static int q8_bag_launch(const void* qrows, int64_t V, int E, const IdxT* ids, int64_t n, const void* offsets, bool off64,
                         int64_t n_off, int64_t B, bool mean, int64_t pad, void* out, float* inv_cnt, int32_t* queue,
                         int32_t* err_flag, hipStream_t s) {
  const int lg = log2_lanes(E);
  if (lg >= 0 && aligned16(qrows) && aligned16(out)) {
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    hipLaunchKernelGGL(bag_ragged_zero_counter_kernel<0>, dim3(1), dim3(64), 0, s, queue);
    dispatch_lanes(lg, [&](auto lg_c) {
      q8_dispatch_stream(q8_streams(V, E), [&](auto st_c) {
        constexpr int LG = decltype(lg_c)::value;
        constexpr bool ST = decltype(st_c)::value;
        hipLaunchKernelGGL((q8_bag_group_kernel<OutT, IdxT, LG, ST>), dim3(grid), dim3(256), 0, s, (const uint4*)qrows,
                           ids, n, offsets, off64, n_off, B, V, pad, mean, (OutT*)out, inv_cnt, queue, err_flag);
        // 4096 waves stride the queue (none queued: they read the counter and leave)
        hipLaunchKernelGGL((q8_bag_long_kernel<OutT, IdxT, LG, ST>), dim3(1024), dim3(256), 0, s, (const uint4*)qrows, ids,
                           n, offsets, off64, n_off, V, pad, mean, (OutT*)out, inv_cnt, queue, err_flag);
      });
    });
  } else {
    hipLaunchKernelGGL((q8_bag_elem_kernel<OutT, IdxT>), dim3(stream_grid(B * E, 256, 256 * 16)), dim3(256), 0, s,
                       (const uint8_t*)qrows, ids, n, offsets, off64, n_off, B, E, q8_stride(E), V, pad, mean, (OutT*)out,
                       inv_cnt, err_flag);
  }
  return check_launch("bag_pool_ragged_q8_fwd");
}

}  // namespace trs

using namespace trs;

// OutT x IdxT from the two dtype codes: TRS_CALL(T, I) is a return statement
#define TRS_Q8_DISPATCH(out_dtype, idx_dtype)        \
  if ((out_dtype) == TRS_F32) {                      \
    if ((idx_dtype) == TRS_I64) TRS_CALL(float, int64_t); \
    TRS_CALL(float, int32_t);                        \
  }                                                  \
  if ((idx_dtype) == TRS_I64) TRS_CALL(bf16_t, int64_t);  \
  TRS_CALL(bf16_t, int32_t)

extern "C" size_t trs_q8_row_bytes(int32_t E) { return E > 0 ? (size_t)q8_stride(E) : 0; }

extern "C" int trs_q8_quantize_rows(const void* table, int64_t V, int32_t E, int32_t dtype, void* qrows,
                                    trs_stream_t stream) {
  if (V == 0) return TRS_OK;
  TRS_REQUIRE(table && qrows, TRS_EINVAL, "q8_quantize_rows: NULL pointer");
  TRS_REQUIRE(V > 0 && E > 0, TRS_EINVAL, "q8_quantize_rows: bad size V=%lld E=%d", (long long)V, E);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "q8_quantize_rows: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32) return q8_quantize_launch<float>(table, V, E, qrows, s);
  return q8_quantize_launch<bf16_t>(table, V, E, qrows, s);
}

extern "C" int trs_gather_rows_q8(const void* qrows, int64_t V, int32_t E, const void* idx, int32_t idx_dtype,
                                  const int64_t* offsets, int64_t B, int32_t N, void* out, int32_t out_dtype,
                                  int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(qrows && idx && out, TRS_EINVAL, "gather_rows_q8: NULL pointer");
  TRS_REQUIRE(V > 0 && E > 0 && B >= 0 && N > 0, TRS_EINVAL, "gather_rows_q8: bad size V=%lld E=%d B=%lld N=%d",
              (long long)V, E, (long long)B, N);
  TRS_REQUIRE(out_dtype == TRS_F32 || out_dtype == TRS_BF16, TRS_EDTYPE, "gather_rows_q8: out dtype %d", out_dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "gather_rows_q8: idx dtype %d", idx_dtype);
  TRS_REQUIRE(B * (int64_t)N < ((int64_t)1 << 32), TRS_ESHAPE, "gather_rows_q8: B*N = %lld lookups must fit 32 bits",
              (long long)(B * (int64_t)N));
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I) return q8_gather_launch<T, I>(qrows, V, E, (const I*)idx, offsets, B * N, N, out, err_flag, s)
  TRS_Q8_DISPATCH(out_dtype, idx_dtype);
#undef TRS_CALL
}

extern "C" int trs_embed_fm_q8(const void* qrows, int64_t V, int32_t E, const void* idx, int32_t idx_dtype,
                               const int64_t* offsets, int64_t B, int32_t N, void* emb, void* fm, float* fm_sum,
                               const void* first_table, void* first, int32_t out_dtype, int32_t* err_flag,
                               trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(qrows && idx, TRS_EINVAL, "embed_fm_q8: NULL pointer");
  TRS_REQUIRE(V > 0 && E > 0 && B >= 0 && N > 0, TRS_EINVAL, "embed_fm_q8: bad size");
  TRS_REQUIRE(out_dtype == TRS_F32 || out_dtype == TRS_BF16, TRS_EDTYPE, "embed_fm_q8: out dtype %d", out_dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "embed_fm_q8: idx dtype %d", idx_dtype);
  TRS_REQUIRE((first_table == nullptr) == (first == nullptr), TRS_EINVAL,
              "embed_fm_q8: first_table and first must be given together");
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I) \
  return q8_embed_fm_launch<T, I>(qrows, V, E, (const I*)idx, offsets, B, N, emb, fm, fm_sum, first_table, first, err_flag, s)
  TRS_Q8_DISPATCH(out_dtype, idx_dtype);
#undef TRS_CALL
}

extern "C" size_t trs_bag_pool_ragged_q8_workspace_bytes(int64_t B) {
  if (B < 0) return 0;
  return bag_ragged_queue_bytes(B);      // [counter][at most B queued bags]
}

extern "C" int trs_bag_pool_ragged_q8_fwd(const void* qrows, int64_t V, int32_t E, const void* ids, int32_t ids_dtype,
                                          int64_t n, const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B,
                                          int32_t mode, int64_t exclude_row, void* out, int32_t out_dtype, float* inv_cnt,
                                          void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(qrows && offsets && out && workspace && (ids || n == 0), TRS_EINVAL,
              "bag_pool_ragged_q8_fwd: NULL pointer");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN, TRS_EINVAL,
              "bag_pool_ragged_q8_fwd: mode %d (0 = sum, 1 = mean; max pooling is not served on Q8 tables)", mode);
  TRS_REQUIRE(V > 0 && E > 0 && B > 0 && n >= 0, TRS_EINVAL,
              "bag_pool_ragged_q8_fwd: bad size V=%lld E=%d B=%lld n=%lld", (long long)V, E, (long long)B, (long long)n);
  TRS_REQUIRE(n_off == B || n_off == B + 1, TRS_EINVAL,
              "bag_pool_ragged_q8_fwd: %lld offsets for B=%lld bags (B or B + 1)", (long long)n_off, (long long)B);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE,
              "bag_pool_ragged_q8_fwd: n=%lld and B=%lld must fit int32", (long long)n, (long long)B);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL,
              "bag_pool_ragged_q8_fwd: exclude_row %lld outside [-1, V)", (long long)exclude_row);
  TRS_REQUIRE(out_dtype == TRS_F32 || out_dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_ragged_q8_fwd: out dtype %d",
              out_dtype);
  TRS_REQUIRE(ids_dtype == TRS_I64 || ids_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_q8_fwd: ids dtype %d", ids_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_q8_fwd: offsets dtype %d",
              off_dtype);
  TRS_REQUIRE(ws_bytes >= trs_bag_pool_ragged_q8_workspace_bytes(B), TRS_EWORKSPACE,
              "bag_pool_ragged_q8_fwd: workspace %zu < %zu", ws_bytes, trs_bag_pool_ragged_q8_workspace_bytes(B));
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I)                                                                                                \
  return q8_bag_launch<T, I>(qrows, V, E, (const I*)ids, n, offsets, off_dtype == TRS_I64, n_off, B, mode == BAG_MEAN, \
                             exclude_row, out, inv_cnt, (int32_t*)workspace, err_flag, s)
  TRS_Q8_DISPATCH(out_dtype, ids_dtype);
#undef TRS_CALL
}
