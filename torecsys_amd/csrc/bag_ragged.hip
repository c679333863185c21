// Ragged bag pooling: one flat vector of ids (n,) plus offsets that say where each sample's bag begins -- the calling form of
// nn.EmbeddingBag and of feature pipelines -- pooled to one row per sample (sum / mean / max) without padding the bags to
// the longest one.  Bag b is ids[offsets[b], end_b), end_b = offsets[b + 1] where that entry exists, else n.
//
// The host never learns the longest bag, so the launch shape cannot depend on it.  Two tiers on the lane-group path (rows of
// a power-of-two number <= 64 of 16-byte vectors):
//   1. bag_ragged_group_kernel: one group of L lanes per bag, CH rows in flight, terms added in list order, sums in
//      registers, no LDS -- bag_pool_group_kernel (bag.hip) with the bag's bounds read from the offsets.  A bag of more
//      than BAG_RAGGED_LONG ids is not walked: lane 0 of its group appends b to a queue in the caller's workspace (one
//      counter + at most B entries: it cannot overflow).
//   2. bag_ragged_long_kernel, fixed grid: one WAVE per queued bag; its 64 / L lane groups stride the bag (group j takes
//      positions beg + j, beg + j + 64/L, ..), the partial sums -- or (maximum, position) pairs -- are folded across the
//      groups by shuffles, steps L, 2L, .., 32.  The queue ORDER depends on the atomics, the result does not: every bag is
//      reduced by one wave in an order that depends on its length alone.
// Any other E: one thread per (b, e), no long-bag tier.
//
// Offsets are range-checked on the device (no host read): begin and end are clamped to [0, n]; an offset outside [0, n]
// or a bag whose end lies before its begin (then empty) raises *err_flag.  Nothing is read outside ids[0, n).
// Algorithmic bytes: n * (idx bytes + E*s) + (B + 1) * offset bytes read, B * E*s written (+ 4 B for inv_cnt, + 4 B E for
// the max positions).
#include "bag_common.hpp"

#ifndef BAG_RAGGED_LONG
#define BAG_RAGGED_LONG 256     // measured: 64 / 128 / 256 / 512 on long-tailed bags, profiles/bag_ragged_kernels.md
#endif

namespace trs {

// Rows in flight per lane of the second tier, as a multiple of the first tier's CH.  A queued bag has one wave to itself and
// the queue is short (a few hundred waves on 256 CUs), so that wave's registers buy latency hiding, not occupancy; the
// terms of a lane are still added in list order, so the result does not depend on this.
constexpr int BAG_RAGGED_LONG_CH = 4;

// The positions q = beg, beg + step, .. < end, CH rows in flight: s[k] (+)= the term of q, am[k] = the winning FLAT
// position (max; < 0: none yet -- the first live position is always taken), cnt += the live positions.  pad >= 0: a position
// that holds that id issues no load and takes no part.  WGT (sum only): every term times wts[q].
// Positions are unsigned 32-bit: end <= n < 2^31 - 1 and a chunk spans at most 32 * 64 of them, so q never wraps.
template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT>
__device__ __forceinline__ void bag_ragged_walk(const uint4* __restrict__ table, const IdxT* __restrict__ ids,
                                                const T* __restrict__ wts, uint32_t beg, uint32_t end, uint32_t step,
                                                int64_t V, int64_t pad, int lane_v, int32_t* __restrict__ err_flag,
                                                float* s, int* am, int& cnt) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  for (uint32_t q0 = beg; q0 < end; q0 += CH * step) {
    int64_t r[CH];
    uint4 v[CH];
    bool live[CH];
    float wv[CH];                             // WGT only
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      const uint32_t q = q0 + c * step;
      r[c] = -1;
      live[c] = false;
      wv[c] = 1.f;
      if (q < end) {
        r[c] = (int64_t)ids[q];
        if (pad >= 0 && r[c] == pad) {        // excluded: no load, no term, no count
          r[c] = -1;
        } else {
          live[c] = true;
          if (WGT) wv[c] = to_f32(wts[q]);
          if (r[c] < 0 || r[c] >= V) {        // reads as a zero row
            if (err_flag != nullptr) *err_flag = 1;
            r[c] = -1;
          }
        }
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      v[c] = make_uint4(0, 0, 0, 0);
      if (r[c] >= 0) v[c] = STREAM ? load_stream(&table[r[c] * L + lane_v]) : table[r[c] * L + lane_v];
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (live[c]) {
        ++cnt;
        float x[VE];
        Vec16<T>::unpack(v[c], x);
#pragma unroll
        for (int k = 0; k < VE; ++k) {
          if (MAXP) {
            if (am[k] < 0 || bag_takes(x[k], s[k])) { s[k] = x[k]; am[k] = (int)(q0 + c * step); }
          } else if (WGT) {
            s[k] += wv[c] * x[k];
          } else {
            s[k] += x[k];
          }
        }
      }
    }
  }
}

// scale (mean: 1 / live count, written to inv_cnt; an empty bag: zero row, argmax -1) and store one lane's columns
template <typename T, int LOG2L, bool MAXP>
__device__ __forceinline__ void bag_ragged_store(float* s, const int* am, int cnt, int64_t b, int lane_v,
                                                 uint4* __restrict__ out, int32_t* __restrict__ amax,
                                                 float* __restrict__ inv_cnt) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  if (!MAXP) {
    if (inv_cnt != nullptr) {
      const float sc = cnt > 0 ? 1.f / (float)cnt : 0.f;
      if (lane_v == 0) inv_cnt[b] = sc;
#pragma unroll
      for (int k = 0; k < VE; ++k) s[k] *= sc;
    }
  } else if (cnt == 0) {
#pragma unroll
    for (int k = 0; k < VE; ++k) s[k] = 0.f;      // am[k] is still -1
  }
  out[b * L + lane_v] = Vec16<T>::pack(s);
  if (MAXP) {
    uint4* dst = reinterpret_cast<uint4*>(amax + (b * L + lane_v) * VE);
#pragma unroll
    for (int h = 0; h < VE / 4; ++h)
      dst[h] = make_uint4((uint32_t)am[4 * h], (uint32_t)am[4 * h + 1], (uint32_t)am[4 * h + 2], (uint32_t)am[4 * h + 3]);
  }
}

template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT>
__global__ __launch_bounds__(256) void bag_ragged_group_kernel(const uint4* __restrict__ table,
                                                               const IdxT* __restrict__ ids, int64_t n,
                                                               const void* __restrict__ offsets, bool off64,
                                                               int64_t n_off, int64_t B, int64_t V, int64_t pad,
                                                               const T* __restrict__ wts, uint4* __restrict__ out,
                                                               int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                               int32_t* __restrict__ queue /* [0] = count */,
                                                               int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < B; b += groups) {
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, err_flag, &beg, &end);
    if (end - beg > BAG_RAGGED_LONG) {      // a whole wave takes it (bag_ragged_long_kernel)
      if (lane_v == 0) queue[1 + atomicAdd(&queue[0], 1)] = (int32_t)b;
      continue;
    }
    float s[VE];
    int am[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) { s[k] = 0.f; am[k] = -1; }
    int cnt = 0;
    bag_ragged_walk<T, IdxT, LOG2L, MAXP, CH, STREAM, WGT>(table, ids, wts, (uint32_t)beg, (uint32_t)end, 1, V, pad,
                                                          lane_v, err_flag, s, am, cnt);
    bag_ragged_store<T, LOG2L, MAXP>(s, am, cnt, b, lane_v, out, amax, inv_cnt);
  }
}

// which of two (value, position) partials of one column the sequential scan would have ended on: a partial without a
// position loses; among NaNs the later one (bag_takes lets a NaN replace a NaN); else the greater value, the SMALLER
// position on equal values
__device__ __forceinline__ bool bag_ragged_other_wins(float ov, int op, float v, int p) {
  if (op < 0) return false;
  if (p < 0) return true;
  const bool on = ov != ov, vn = v != v;
  if (on || vn) return on && (!vn || op > p);
  return ov > v || (ov == v && op < p);
}

template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT>
__global__ __launch_bounds__(256) void bag_ragged_long_kernel(const uint4* __restrict__ table,
                                                              const IdxT* __restrict__ ids, int64_t n,
                                                              const void* __restrict__ offsets, bool off64,
                                                              int64_t n_off, int64_t B, int64_t V, int64_t pad,
                                                              const T* __restrict__ wts, uint4* __restrict__ out,
                                                              int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                              const int32_t* __restrict__ queue,
                                                              int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
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
    float s[VE];
    int am[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) { s[k] = 0.f; am[k] = -1; }
    int cnt = 0;
    bag_ragged_walk<T, IdxT, LOG2L, MAXP, CH, STREAM, WGT>(table, ids, wts, (uint32_t)beg + grp, (uint32_t)end, G, V, pad,
                                                          lane_v, err_flag, s, am, cnt);
    cnt = across_groups_sum<L>(cnt);
    if (MAXP) {
#pragma unroll
      for (int m = L; m < 64; m <<= 1) {
#pragma unroll
        for (int k = 0; k < VE; ++k) {
          const float ov = __shfl_xor(s[k], m, 64);
          const int op = __shfl_xor(am[k], m, 64);
          if (bag_ragged_other_wins(ov, op, s[k], am[k])) { s[k] = ov; am[k] = op; }
        }
      }
    } else {
#pragma unroll
      for (int k = 0; k < VE; ++k) s[k] = across_groups_sum<L>(s[k]);
    }
    if (grp == 0) bag_ragged_store<T, LOG2L, MAXP>(s, am, cnt, b, lane_v, out, amax, inv_cnt);
  }
}

// generic path: any E; one thread per (b, e), whatever the bag's length
template <typename T, typename IdxT, bool MAXP>
__global__ __launch_bounds__(256) void bag_ragged_elem_kernel(const T* __restrict__ table, const IdxT* __restrict__ ids,
                                                              int64_t n, const void* __restrict__ offsets, bool off64,
                                                              int64_t n_off, int64_t B, int E, int64_t V, int64_t pad,
                                                              const T* __restrict__ wts, T* __restrict__ out,
                                                              int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                              int32_t* __restrict__ err_flag) {
  const int64_t total = B * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t b = udiv_fast(t, E, f32);
    const int e = (int)(t - b * E);
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, err_flag, &beg, &end);
    float s = 0.f;
    int am = -1;
    int cnt = 0;
    for (int64_t q = beg; q < end; ++q) {
      const int64_t r = (int64_t)ids[q];
      if (pad >= 0 && r == pad) continue;
      ++cnt;
      T raw = T{};
      if (r < 0 || r >= V) {
        if (err_flag != nullptr) *err_flag = 1;
      } else {
        raw = table[r * E + e];
      }
      const float x = to_f32(raw);
      if (MAXP) {
        if (am < 0 || bag_takes(x, s)) { s = x; am = (int)q; }
      } else if (wts != nullptr) {
        s += to_f32(wts[q]) * x;
      } else {
        s += x;
      }
    }
    if (!MAXP && inv_cnt != nullptr) {
      const float sc = cnt > 0 ? 1.f / (float)cnt : 0.f;
      if (e == 0) inv_cnt[b] = sc;
      s *= sc;
    }
    out[t] = from_f32<T>(s);      // an empty bag: s is still 0, am still -1
    if (MAXP) amax[t] = am;
  }
}

__global__ void bag_ragged_zero_counter_kernel(int32_t* __restrict__ p) {
  if (threadIdx.x == 0) *p = 0;
}

static size_t bag_ragged_queue_bytes(int64_t B) { return align_up((size_t)(B + 1) * 4, 256); }

template <typename T, typename IdxT>
static int bag_ragged_launch(const void* table, const IdxT* ids, int64_t n, const void* offsets, bool off64,
                             int64_t n_off, int64_t B, int E, int64_t V, int mode, int64_t pad, const void* wts_,
                             void* out, int32_t* amax, float* inv_cnt, int32_t* queue, int32_t* err_flag,
                             hipStream_t s) {
  const T* wts = (const T*)wts_;
  const int lg = log2_lanes(E * (int)sizeof(T));
  if (lg >= 0 && aligned16(table) && aligned16(out) && aligned16(amax)) {
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    const bool stream = (size_t)V * E * sizeof(T) > BAG_STREAM_BYTES;
    hipLaunchKernelGGL(bag_ragged_zero_counter_kernel, dim3(1), dim3(64), 0, s, queue);
    dispatch_lanes(lg, [&](auto lg_c) {
      auto launch = [&](auto mx_c, auto ch_c, auto st_c, auto wg_c) {
        constexpr int LG = decltype(lg_c)::value, CH = decltype(ch_c)::value;
        constexpr bool MX = decltype(mx_c)::value, ST = decltype(st_c)::value, WG = decltype(wg_c)::value;
        hipLaunchKernelGGL((bag_ragged_group_kernel<T, IdxT, LG, MX, CH, ST, WG>), dim3(grid), dim3(256), 0, s,
                           (const uint4*)table, ids, n, offsets, off64, n_off, B, V, pad, wts, (uint4*)out, amax,
                           inv_cnt, queue, err_flag);
        // fixed grid, one wave per queued bag: 4096 waves stride the queue (none queued: the waves read the counter
        // and leave)
        hipLaunchKernelGGL((bag_ragged_long_kernel<T, IdxT, LG, MX, BAG_RAGGED_LONG_CH * CH, ST, WG>), dim3(1024),
                           dim3(256), 0, s,
                           (const uint4*)table, ids, n, offsets, off64, n_off, B, V, pad, wts, (uint4*)out, amax,
                           inv_cnt, queue, err_flag);
      };
      constexpr std::integral_constant<int, 4> ch4{};
      constexpr std::integral_constant<int, 8> ch8{};
      constexpr std::true_type yes{};
      constexpr std::false_type no{};
      if (mode == BAG_MAX) {
        if (stream) launch(yes, ch4, yes, no);
        else launch(yes, ch4, no, no);
      } else if (wts != nullptr) {      /* weights: sum only */
        if (stream) launch(no, ch8, yes, yes);
        else launch(no, ch8, no, yes);
      } else {
        if (stream) launch(no, ch8, yes, no);
        else launch(no, ch8, no, no);
      }
    });
  } else {
    const int grid = stream_grid(B * E, 256, 256 * 16);
    if (mode == BAG_MAX)
      hipLaunchKernelGGL((bag_ragged_elem_kernel<T, IdxT, true>), dim3(grid), dim3(256), 0, s, (const T*)table, ids, n,
                         offsets, off64, n_off, B, E, V, pad, wts, (T*)out, amax, inv_cnt, err_flag);
    else
      hipLaunchKernelGGL((bag_ragged_elem_kernel<T, IdxT, false>), dim3(grid), dim3(256), 0, s, (const T*)table, ids, n,
                         offsets, off64, n_off, B, E, V, pad, wts, (T*)out, amax, inv_cnt, err_flag);
  }
  return check_launch("bag_pool_ragged_fwd");
}

// bag_of[p] = the last b in [0, B) with offsets[b] <= p, provided p < end_b; else -1.  One thread per position, a binary
// search over the offsets (they sit in L2); a pure function of the offsets.
__global__ __launch_bounds__(256) void bag_owner_kernel(const void* __restrict__ offsets, bool off64, int64_t n_off,
                                                        int64_t B, int64_t n, int32_t* __restrict__ bag_of) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    auto at = [&](int64_t b) -> int64_t {
      return off64 ? ((const int64_t*)offsets)[b] : (int64_t)((const int32_t*)offsets)[b];
    };
    int64_t lo = 0, hi = B;                   // the first b in [0, B] with offsets[b] > p
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if (at(mid) <= p) lo = mid + 1;
      else hi = mid;
    }
    int32_t owner = -1;
    if (lo > 0) {
      const int64_t b = lo - 1;
      const int64_t end = b + 1 < n_off ? at(b + 1) : n;
      if (p < end) owner = (int32_t)b;
    }
    bag_of[p] = owner;
  }
}

}  // namespace trs

using namespace trs;

extern "C" int32_t trs_bag_ragged_long_len(void) { return BAG_RAGGED_LONG; }

extern "C" size_t trs_bag_ragged_workspace_bytes(int64_t B) {
  if (B < 0) return 0;
  return bag_ragged_queue_bytes(B);      // [counter][at most B queued bags]
}

extern "C" int trs_bag_pool_ragged_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids,
                                       int32_t ids_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                                       int64_t n_off, int64_t B, int32_t mode, int64_t exclude_row, const void* weights,
                                       void* out, int32_t* argmax, float* inv_cnt, void* workspace, size_t ws_bytes,
                                       int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && offsets && out && workspace && (ids || n == 0), TRS_EINVAL, "bag_pool_ragged_fwd: NULL pointer");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN || mode == BAG_MAX, TRS_EINVAL,
              "bag_pool_ragged_fwd: mode %d (0 = sum, 1 = mean, 2 = max)", mode);
  TRS_REQUIRE(V > 0 && E > 0 && B > 0 && n >= 0, TRS_EINVAL, "bag_pool_ragged_fwd: bad size V=%lld E=%d B=%lld n=%lld",
              (long long)V, E, (long long)B, (long long)n);
  TRS_REQUIRE(n_off == B || n_off == B + 1, TRS_EINVAL, "bag_pool_ragged_fwd: %lld offsets for B=%lld bags (B or B + 1)",
              (long long)n_off, (long long)B);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE,
              "bag_pool_ragged_fwd: n=%lld and B=%lld must fit int32", (long long)n, (long long)B);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL, "bag_pool_ragged_fwd: exclude_row %lld outside [-1, V)",
              (long long)exclude_row);
  TRS_REQUIRE(weights == nullptr || mode == BAG_SUM, TRS_EINVAL, "bag_pool_ragged_fwd: weights need mode 0 (sum), got %d",
              mode);
  TRS_REQUIRE(mode != BAG_MAX || argmax != nullptr, TRS_EINVAL,
              "bag_pool_ragged_fwd: max pooling needs the argmax output");
  TRS_REQUIRE(mode != BAG_MEAN || inv_cnt != nullptr, TRS_EINVAL, "bag_pool_ragged_fwd: the mean needs the inv_cnt output");
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_ragged_fwd: dtype %d", dtype);
  TRS_REQUIRE(ids_dtype == TRS_I64 || ids_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_fwd: ids dtype %d", ids_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_fwd: offsets dtype %d",
              off_dtype);
  TRS_REQUIRE(ws_bytes >= trs_bag_ragged_workspace_bytes(B), TRS_EWORKSPACE, "bag_pool_ragged_fwd: workspace %zu < %zu",
              ws_bytes, trs_bag_ragged_workspace_bytes(B));
  hipStream_t s = (hipStream_t)stream;
  float* ic = mode == BAG_MEAN ? inv_cnt : nullptr;
  int32_t* am = mode == BAG_MAX ? argmax : nullptr;
#define TRS_CALL(T, I)                                                                                                \
  return bag_ragged_launch<T, I>(table, (const I*)ids, n, offsets, off_dtype == TRS_I64, n_off, B, E, V, mode, exclude_row, \
                                 weights, out, am, ic, (int32_t*)workspace, err_flag, s)
  if (dtype == TRS_F32) {
    if (ids_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (ids_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}

extern "C" int trs_bag_owner(const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int64_t n,
                             int32_t* bag_of, trs_stream_t stream) {
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(offsets && bag_of, TRS_EINVAL, "bag_owner: NULL pointer");
  TRS_REQUIRE(B > 0 && n >= 0 && (n_off == B || n_off == B + 1), TRS_EINVAL,
              "bag_owner: bad size B=%lld n=%lld, %lld offsets (B or B + 1)", (long long)B, (long long)n,
              (long long)n_off);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE, "bag_owner: n=%lld and B=%lld must fit int32",
              (long long)n, (long long)B);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_owner: offsets dtype %d", off_dtype);
  hipLaunchKernelGGL(bag_owner_kernel, dim3(stream_grid(n, 256, 256 * 16)), dim3(256), 0, (hipStream_t)stream, offsets,
                     off_dtype == TRS_I64, n_off, B, n, bag_of);
  return check_launch("bag_owner");
}
