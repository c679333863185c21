// Bag pooling over a ROW-SHARDED table (torecsys_amd/dist.py, RowShardedListIndicesEmbedding): sum and mean are linear, so
// the looked-up rows never travel.  The sender routes the (B, Lb) ids of its batch by owner; every owner pools the rows it
// holds for each (source rank, sample) into ONE fp32 partial row; the partial rows cross the links and are added up.
//
//   route    counts (W, B) and the LOCAL ids grouped by owner, then sample, then list order.  A wave owns a sample and walks
//            its list 64 positions at a time; the place of a lookup inside its (owner, sample) segment is the number of
//            lower lanes with the same owner (ballot + popcount) behind the lookups of earlier chunks, which lane w keeps for
//            owner w (W <= 64 = one wave).  No atomics: the layout is a pure function of the ids.
//   pool     out (S, E) fp32: segment s = ids[seg_start[s] .. seg_start[s + 1]) summed in list order in fp32.  Layout of
//            bag_pool_group_kernel (bag.hip): a group of E*sizeof(T)/16 lanes owns a segment, CH rows in flight.
//   combine  out[b] = round((sum_p parts[p, b]) * scale), p ascending: the one rounding of the whole path.
//   expand   backward: the (S, E) output gradients the owner holds, written once per lookup of each segment -- the rows and
//            ids the owner-side reduction (row buckets + bucket walk / fused optimizer) takes.
// All four are HBM / latency bound; none uses LDS.
#include "trs_common.hpp"

namespace trs {

constexpr size_t BAGS_STREAM_BYTES = (size_t)512 << 20;      // twice the Infinity Cache: the STREAM rule of fm.hip / bag.hip

// ---------------------------------------------------------------------------------------------
// route: PLACE = false counts, PLACE = true writes the local ids to their slots
template <typename IdxT, bool PLACE>
__global__ __launch_bounds__(256) void bag_route_kernel(const IdxT* __restrict__ idx, int64_t B, int Lb, int64_t V,
                                                        int64_t rows_per_rank, int world, int32_t* __restrict__ counts,
                                                        const int32_t* __restrict__ seg_start,
                                                        int32_t* __restrict__ send_ids, int64_t n_send,
                                                        int32_t* __restrict__ err_flag) {
  const int lane = threadIdx.x & 63;
  const int64_t waves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  const bool f32 = V < ((int64_t)1 << 32) && rows_per_rank < ((int64_t)1 << 32);
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < B; b += waves) {
    // lane w < world: the lookups of owner w seen so far (count) / the next free slot of segment (w, b) and its end (place)
    int32_t mine = 0, lim = 0;
    if (PLACE && lane < world) {
      mine = seg_start[(int64_t)lane * B + b];
      lim = seg_start[(int64_t)lane * B + b + 1];
    }
    for (int l0 = 0; l0 < Lb; l0 += 64) {
      int owner = -1;
      int32_t local = 0;
      if (l0 + lane < Lb) {
        const int64_t r = (int64_t)idx[b * Lb + l0 + lane];
        if (r < 0 || r >= V) {      // not sent: contributes a zero row
          if (!PLACE && err_flag != nullptr) *err_flag = 1;
        } else {
          const int64_t o = f32 ? (int64_t)((unsigned)r / (unsigned)rows_per_rank) : r / rows_per_rank;
          owner = (int)o;
          local = (int32_t)(r - o * rows_per_rank);
        }
      }
      for (int w = 0; w < world; ++w) {
        const unsigned long long m = __ballot(owner == w);
        if (m == 0) continue;      // wave-uniform
        if (PLACE) {
          const int base = __shfl(mine, w, 64), end = __shfl(lim, w, 64);
          if (owner == w) {
            const int64_t pos = (int64_t)base + __popcll(m & (((unsigned long long)1 << lane) - 1));
            if (pos < end && pos < n_send) send_ids[pos] = local;      // (a seg_start that is not the scan of the counts)
          }
        }
        if (lane == w) mine += __popcll(m);
      }
    }
    if (!PLACE && lane < world) counts[(int64_t)lane * B + b] = mine;
  }
}

// ---------------------------------------------------------------------------------------------
// owner: one fp32 row per segment
template <typename T, int LOG2L, int CH, bool STREAM>
__global__ __launch_bounds__(256) void bag_seg_pool_group_kernel(const uint4* __restrict__ shard, int64_t n_valid,
                                                                 const int32_t* __restrict__ ids, int64_t n,
                                                                 const int32_t* __restrict__ seg_start, int64_t S,
                                                                 uint4* __restrict__ out, int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; s < S; s += groups) {
    int64_t beg = seg_start[s], end = seg_start[s + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;
    float acc[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) acc[k] = 0.f;
    for (int64_t q0 = beg; q0 < end; q0 += CH) {
      int64_t r[CH];
      uint4 v[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        r[c] = -1;
        if (q0 + c < end) {
          r[c] = (int64_t)ids[q0 + c];
          if (r[c] < 0 || r[c] >= n_valid) {      // reads as a zero row
            if (err_flag != nullptr) *err_flag = 1;
            r[c] = -1;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        v[c] = make_uint4(0, 0, 0, 0);
        if (r[c] >= 0) v[c] = STREAM ? load_stream(&shard[r[c] * L + lane_v]) : shard[r[c] * L + lane_v];
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (q0 + c < end) {
          float x[VE];
          Vec16<T>::unpack(v[c], x);
#pragma unroll
          for (int k = 0; k < VE; ++k) acc[k] += x[k];
        }
      }
    }
    uint4* o = out + (s * L + lane_v) * (VE / 4);
#pragma unroll
    for (int j = 0; j < VE / 4; ++j) o[j] = Vec16<float>::pack(acc + 4 * j);
  }
}

// generic path: any E; one thread per (segment, e)
template <typename T>
__global__ __launch_bounds__(256) void bag_seg_pool_elem_kernel(const T* __restrict__ shard, int64_t n_valid,
                                                                const int32_t* __restrict__ ids, int64_t n,
                                                                const int32_t* __restrict__ seg_start, int64_t S, int E,
                                                                float* __restrict__ out, int32_t* __restrict__ err_flag) {
  const int64_t total = S * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t s = udiv_fast(t, E, f32);
    const int e = (int)(t - s * E);
    int64_t beg = seg_start[s], end = seg_start[s + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;
    float acc = 0.f;
    for (int64_t q = beg; q < end; ++q) {
      const int64_t r = (int64_t)ids[q];
      if (r < 0 || r >= n_valid) {
        if (err_flag != nullptr) *err_flag = 1;
      } else {
        acc += to_f32(shard[r * E + e]);
      }
    }
    out[t] = acc;
  }
}

template <typename T>
static int bag_seg_pool_launch(const void* shard, int64_t n_valid, int E, const int32_t* ids, int64_t n,
                               const int32_t* seg_start, int64_t S, float* out, int32_t* err_flag, hipStream_t s) {
  const int lg = log2_lanes(E * (int)sizeof(T));
  if (lg >= 0 && aligned16(shard) && aligned16(out)) {
    const int grid = stream_grid(S << lg, 256, 256 * 16);
    const bool stream = (size_t)n_valid * E * sizeof(T) > BAGS_STREAM_BYTES;
    dispatch_lanes(lg, [&](auto lg_c) {
      constexpr int LG = decltype(lg_c)::value;
      if (stream)
        hipLaunchKernelGGL((bag_seg_pool_group_kernel<T, LG, 8, true>), dim3(grid), dim3(256), 0, s,
                           (const uint4*)shard, n_valid, ids, n, seg_start, S, (uint4*)out, err_flag);
      else
        hipLaunchKernelGGL((bag_seg_pool_group_kernel<T, LG, 8, false>), dim3(grid), dim3(256), 0, s,
                           (const uint4*)shard, n_valid, ids, n, seg_start, S, (uint4*)out, err_flag);
    });
  } else {
    hipLaunchKernelGGL((bag_seg_pool_elem_kernel<T>), dim3(stream_grid(S * E, 256, 256 * 16)), dim3(256), 0, s,
                       (const T*)shard, n_valid, ids, n, seg_start, S, E, out, err_flag);
  }
  return check_launch("bag_pool_segments");
}

// ---------------------------------------------------------------------------------------------
// combine: four adjacent elements per thread (fp32 partials read as 16-byte vectors), or one
template <typename T>
__device__ __forceinline__ void bag_store4(T* dst, const float* f);
template <>
__device__ __forceinline__ void bag_store4<float>(float* dst, const float* f) {
  *reinterpret_cast<uint4*>(dst) = Vec16<float>::pack(f);
}
template <>
__device__ __forceinline__ void bag_store4<bf16_t>(bf16_t* dst, const float* f) {
  *reinterpret_cast<uint2*>(dst) = make_uint2(f32x2_to_bf16x2_bits(f[0], f[1]), f32x2_to_bf16x2_bits(f[2], f[3]));
}

template <typename T>
__global__ __launch_bounds__(256) void bag_combine_vec_kernel(const uint4* __restrict__ parts, int P, int64_t quads,
                                                              float scale, T* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < quads; t += stride) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < P; ++p) {
      float x[4];
      Vec16<float>::unpack(load_stream(&parts[(int64_t)p * quads + t]), x);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] += x[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) acc[k] *= scale;
    bag_store4<T>(out + 4 * t, acc);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bag_combine_elem_kernel(const float* __restrict__ parts, int P, int64_t total,
                                                               float scale, T* __restrict__ out) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    float acc = 0.f;
    for (int p = 0; p < P; ++p) acc += parts[(int64_t)p * total + t];
    out[t] = from_f32<T>(acc * scale);
  }
}

template <typename T>
static int bag_combine_launch(const float* parts, int P, int64_t total, float scale, void* out, hipStream_t s) {
  if (total % 4 == 0 && aligned16(parts) && aligned16(out)) {
    hipLaunchKernelGGL((bag_combine_vec_kernel<T>), dim3(stream_grid(total / 4, 256, 256 * 16)), dim3(256), 0, s,
                       (const uint4*)parts, P, total / 4, scale, (T*)out);
  } else {
    hipLaunchKernelGGL((bag_combine_elem_kernel<T>), dim3(stream_grid(total, 256, 256 * 16)), dim3(256), 0, s, parts, P,
                       total, scale, (T*)out);
  }
  return check_launch("bag_combine");
}

// ---------------------------------------------------------------------------------------------
// expand (backward): grad_rows[q] = g_all[s] for the lookups q of segment s; zero row and id -1 for the padding row and
// for ids outside the shard (they read as zero rows in the forward)
__device__ __forceinline__ bool bag_no_grad(int32_t id, int64_t n_valid, int64_t pad_row) {
  return id < 0 || id >= n_valid || id == pad_row;
}

template <int LOG2L>
__global__ __launch_bounds__(256) void bag_expand_group_kernel(const uint4* __restrict__ g_all,
                                                               const int32_t* __restrict__ ids, int64_t n,
                                                               const int32_t* __restrict__ seg_start, int64_t S,
                                                               int64_t n_valid, int64_t pad_row,
                                                               uint4* __restrict__ grad_rows,
                                                               int32_t* __restrict__ ids_bwd) {
  constexpr int L = 1 << LOG2L;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t s = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; s < S; s += groups) {
    int64_t beg = seg_start[s], end = seg_start[s + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;
    if (beg < end) {
      const uint4 gv = g_all[s * L + lane_v];
      for (int64_t q = beg; q < end; ++q) {
        const int32_t id = ids[q];
        const bool none = bag_no_grad(id, n_valid, pad_row);
        store_stream(&grad_rows[q * L + lane_v], none ? make_uint4(0, 0, 0, 0) : gv);
        if (lane_v == 0) ids_bwd[q] = none ? -1 : id;
      }
    }
    if (s == S - 1) {      // slots behind the last segment (ids that were not sent): no gradient
      for (int64_t q = end > 0 ? end : 0; q < n; ++q) {
        store_stream(&grad_rows[q * L + lane_v], make_uint4(0, 0, 0, 0));
        if (lane_v == 0) ids_bwd[q] = -1;
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bag_expand_elem_kernel(const T* __restrict__ g_all, const int32_t* __restrict__ ids,
                                                              int64_t n, const int32_t* __restrict__ seg_start, int64_t S,
                                                              int E, int64_t n_valid, int64_t pad_row,
                                                              T* __restrict__ grad_rows, int32_t* __restrict__ ids_bwd) {
  const int64_t total = S * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t s = udiv_fast(t, E, f32);
    const int e = (int)(t - s * E);
    int64_t beg = seg_start[s], end = seg_start[s + 1];
    if (beg < 0) beg = 0;
    if (end > n) end = n;
    const T gv = g_all[t];
    for (int64_t q = beg; q < end; ++q) {
      const int32_t id = ids[q];
      const bool none = bag_no_grad(id, n_valid, pad_row);
      grad_rows[q * E + e] = none ? T{} : gv;
      if (e == 0) ids_bwd[q] = none ? -1 : id;
    }
    if (s == S - 1) {      // slots behind the last segment (ids that were not sent): no gradient
      for (int64_t q = end > 0 ? end : 0; q < n; ++q) {
        grad_rows[q * E + e] = T{};
        if (e == 0) ids_bwd[q] = -1;
      }
    }
  }
}

template <typename T>
static int bag_expand_launch(const void* g_all, int E, const int32_t* ids, int64_t n, const int32_t* seg_start, int64_t S,
                             int64_t n_valid, int64_t pad_row, void* grad_rows, int32_t* ids_bwd, hipStream_t s) {
  const int lg = log2_lanes(E * (int)sizeof(T));
  if (lg >= 0 && aligned16(g_all) && aligned16(grad_rows)) {
    const int grid = stream_grid(S << lg, 256, 256 * 16);
    dispatch_lanes(lg, [&](auto lg_c) {
      hipLaunchKernelGGL((bag_expand_group_kernel<decltype(lg_c)::value>), dim3(grid), dim3(256), 0, s,
                         (const uint4*)g_all, ids, n, seg_start, S, n_valid, pad_row, (uint4*)grad_rows, ids_bwd);
    });
  } else {
    hipLaunchKernelGGL((bag_expand_elem_kernel<T>), dim3(stream_grid(S * E, 256, 256 * 16)), dim3(256), 0, s,
                       (const T*)g_all, ids, n, seg_start, S, E, n_valid, pad_row, (T*)grad_rows, ids_bwd);
  }
  return check_launch("bag_expand_grad");
}

static int bag_route_check(const char* what, const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t V,
                           int64_t rows_per_rank, int32_t world) {
  TRS_REQUIRE(idx != nullptr, TRS_EINVAL, "%s: NULL pointer", what);
  TRS_REQUIRE(B >= 0 && V >= 1 && rows_per_rank >= 1, TRS_EINVAL, "%s: bad size B=%lld V=%lld rows_per_rank=%lld", what,
              (long long)B, (long long)V, (long long)rows_per_rank);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "%s: idx dtype %d", what, idx_dtype);
  TRS_REQUIRE(world >= 1 && world <= 64, TRS_ESHAPE, "%s: world=%d outside [1, 64]", what, world);
  TRS_REQUIRE(L >= 1 && L <= 65535, TRS_ESHAPE, "%s: list length L=%d outside [1, 65535]", what, L);
  TRS_REQUIRE(B * (int64_t)L < (int64_t)0x7fffffff, TRS_ESHAPE, "%s: B*L=%lld must fit int32", what,
              (long long)(B * (int64_t)L));
  TRS_REQUIRE(rows_per_rank >= (V + world - 1) / world, TRS_EINVAL,
              "%s: rows_per_rank=%lld times world=%d does not cover V=%lld", what, (long long)rows_per_rank, world,
              (long long)V);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" int trs_bag_route_count(const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t V,
                                   int64_t rows_per_rank, int32_t world, int32_t* counts, int32_t* err_flag,
                                   trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(counts != nullptr, TRS_EINVAL, "bag_route_count: NULL pointer");
  if (const int rc = bag_route_check("bag_route_count", idx, idx_dtype, B, L, V, rows_per_rank, world)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int grid = stream_grid(B * 64, 256, 256 * 16);
  if (idx_dtype == TRS_I64)
    hipLaunchKernelGGL((bag_route_kernel<int64_t, false>), dim3(grid), dim3(256), 0, s, (const int64_t*)idx, B, L, V,
                       rows_per_rank, world, counts, (const int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0, err_flag);
  else
    hipLaunchKernelGGL((bag_route_kernel<int32_t, false>), dim3(grid), dim3(256), 0, s, (const int32_t*)idx, B, L, V,
                       rows_per_rank, world, counts, (const int32_t*)nullptr, (int32_t*)nullptr, (int64_t)0, err_flag);
  return check_launch("bag_route_count");
}

extern "C" int trs_bag_route_place(const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t V,
                                   int64_t rows_per_rank, int32_t world, const int32_t* seg_start, int32_t* send_ids,
                                   int64_t n_send, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(seg_start != nullptr && (send_ids != nullptr || n_send == 0) && n_send >= 0, TRS_EINVAL,
              "bag_route_place: NULL pointer");
  if (const int rc = bag_route_check("bag_route_place", idx, idx_dtype, B, L, V, rows_per_rank, world)) return rc;
  TRS_REQUIRE(n_send <= B * (int64_t)L, TRS_EINVAL, "bag_route_place: n_send=%lld exceeds B*L=%lld", (long long)n_send,
              (long long)(B * (int64_t)L));
  if (n_send == 0) return TRS_OK;      // every id was out of range: nothing to place
  hipStream_t s = (hipStream_t)stream;
  const int grid = stream_grid(B * 64, 256, 256 * 16);
  if (idx_dtype == TRS_I64)
    hipLaunchKernelGGL((bag_route_kernel<int64_t, true>), dim3(grid), dim3(256), 0, s, (const int64_t*)idx, B, L, V,
                       rows_per_rank, world, (int32_t*)nullptr, seg_start, send_ids, n_send, (int32_t*)nullptr);
  else
    hipLaunchKernelGGL((bag_route_kernel<int32_t, true>), dim3(grid), dim3(256), 0, s, (const int32_t*)idx, B, L, V,
                       rows_per_rank, world, (int32_t*)nullptr, seg_start, send_ids, n_send, (int32_t*)nullptr);
  return check_launch("bag_route_place");
}

extern "C" int trs_bag_pool_segments(const void* shard, int64_t n_valid, int32_t E, int32_t dtype, const int32_t* ids,
                                     int64_t n, const int32_t* seg_start, int64_t S, float* out, int32_t* err_flag,
                                     trs_stream_t stream) {
  if (S == 0) return TRS_OK;
  TRS_REQUIRE(shard && seg_start && out && (ids || n == 0), TRS_EINVAL, "bag_pool_segments: NULL pointer");
  TRS_REQUIRE(S > 0 && n >= 0 && n_valid >= 0 && E > 0, TRS_EINVAL, "bag_pool_segments: bad size S=%lld n=%lld E=%d",
              (long long)S, (long long)n, E);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_segments: dtype %d", dtype);
  TRS_REQUIRE(n < (int64_t)0x7fffffff, TRS_ESHAPE, "bag_pool_segments: n=%lld must fit int32", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32) return bag_seg_pool_launch<float>(shard, n_valid, E, ids, n, seg_start, S, out, err_flag, s);
  return bag_seg_pool_launch<bf16_t>(shard, n_valid, E, ids, n, seg_start, S, out, err_flag, s);
}

extern "C" int trs_bag_combine(const float* parts, int32_t P, int64_t B, int32_t E, float scale, int32_t dtype, void* out,
                               trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(parts && out, TRS_EINVAL, "bag_combine: NULL pointer");
  TRS_REQUIRE(B > 0 && E > 0 && P >= 1, TRS_EINVAL, "bag_combine: bad size P=%d B=%lld E=%d", P, (long long)B, E);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_combine: dtype %d", dtype);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32) return bag_combine_launch<float>(parts, P, B * E, scale, out, s);
  return bag_combine_launch<bf16_t>(parts, P, B * E, scale, out, s);
}

extern "C" int trs_bag_expand_grad(const void* g_all, int32_t dtype, int32_t E, const int32_t* ids, int64_t n,
                                   const int32_t* seg_start, int64_t S, int64_t n_valid, int64_t pad_local_row,
                                   void* grad_rows, int32_t* ids_bwd, trs_stream_t stream) {
  if (S == 0 || n == 0) return TRS_OK;
  TRS_REQUIRE(g_all && ids && seg_start && grad_rows && ids_bwd, TRS_EINVAL, "bag_expand_grad: NULL pointer");
  TRS_REQUIRE(S > 0 && n > 0 && n_valid >= 0 && E > 0, TRS_EINVAL, "bag_expand_grad: bad size S=%lld n=%lld E=%d",
              (long long)S, (long long)n, E);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_expand_grad: dtype %d", dtype);
  TRS_REQUIRE(n < (int64_t)0x7fffffff, TRS_ESHAPE, "bag_expand_grad: n=%lld must fit int32", (long long)n);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32)
    return bag_expand_launch<float>(g_all, E, ids, n, seg_start, S, n_valid, pad_local_row, grad_rows, ids_bwd, s);
  return bag_expand_launch<bf16_t>(g_all, E, ids, n, seg_start, S, n_valid, pad_local_row, grad_rows, ids_bwd, s);
}
