// The ragged bag forward, shared by its two entries: one field (bag_ragged.hip: bag b is out row b, ids are table rows) and
// F fields over one table (bag_fields.hip: FIELDS = true -- bag j = f * B + b of the field-major offsets is out row
// b * F + f, its ids are RAW ids of field f, checked against that field and moved by field_offsets[f]).  The kernels, the
// two tiers and the order of every sum are the same; see bag_ragged.hip for the description.
#pragma once
#include "bag_common.hpp"

#ifndef BAG_RAGGED_LONG
#define BAG_RAGGED_LONG 256     // measured: 64 / 128 / 256 / 512 on long-tailed bags, profiles/bag_ragged_kernels.md
#endif

namespace trs {

// Rows in flight per lane of the second tier, as a multiple of the first tier's CH.  A queued bag has one wave to itself and
// the queue is short (a few hundred waves on 256 CUs), so that wave's registers buy latency hiding, not occupancy; the
// terms of a lane are still added in list order, so the result does not depend on this.
constexpr int BAG_RAGGED_LONG_CH = 4;

// FIELDS: where the bags' fields lie.  field_offsets (F + 1,) int64 on the device, B bags per field.
struct BagFieldMap {
  const int64_t* field_offsets;
  int64_t B;
  int F;
};

// bag j -> the first table row of its field (base), the field's size (Vf: ids are checked against it) and its out row.
// A field that does not lie inside [0, V) has size 0: every id of it reads as a zero row and raises the flag.
template <bool FIELDS>
__device__ __forceinline__ void bag_field_of(const BagFieldMap& fm, int64_t j, int64_t V, int64_t* base, int64_t* Vf,
                                             int64_t* orow) {
  if constexpr (!FIELDS) {
    *base = 0;
    *Vf = V;
    *orow = j;
  } else {
    const int64_t f = udiv_fast(j, (int)fm.B, true);      // F * B < 2^31 - 1
    const int64_t lo = fm.field_offsets[f], hi = fm.field_offsets[f + 1];
    const bool ok = lo >= 0 && hi >= lo && hi <= V;
    *base = ok ? lo : 0;
    *Vf = ok ? hi - lo : 0;
    *orow = (j - f * fm.B) * fm.F + f;
  }
}

// The positions q = beg, beg + step, .. < end, CH rows in flight: s[k] (+)= the term of q, am[k] = the winning FLAT
// position (max; < 0: none yet -- the first live position is always taken), cnt += the live positions.  pad >= 0: a position
// that holds that id issues no load and takes no part.  WGT (sum only): every term times wts[q].  An id is checked against
// [0, V) and then moved by ``base`` rows (0 for a table of one field).
// Positions are unsigned 32-bit: end <= n < 2^31 - 1 and a chunk spans at most 32 * 64 of them, so q never wraps.
template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT>
__device__ __forceinline__ void bag_ragged_walk(const uint4* __restrict__ table, const IdxT* __restrict__ ids,
                                                const T* __restrict__ wts, uint32_t beg, uint32_t end, uint32_t step,
                                                int64_t V, int64_t base, int64_t pad, int lane_v,
                                                int32_t* __restrict__ err_flag, float* s, int* am, int& cnt) {
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
          } else {
            r[c] += base;
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

template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT, bool FIELDS>
__global__ __launch_bounds__(256) void bag_ragged_group_kernel(const uint4* __restrict__ table,
                                                               const IdxT* __restrict__ ids, int64_t n,
                                                               const void* __restrict__ offsets, bool off64,
                                                               int64_t n_off, int64_t B, int64_t V, int64_t pad,
                                                               const T* __restrict__ wts, uint4* __restrict__ out,
                                                               int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                               int32_t* __restrict__ queue /* [0] = count */,
                                                               int32_t* __restrict__ err_flag, BagFieldMap fm) {
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
    int64_t base, Vf, orow;
    bag_field_of<FIELDS>(fm, b, V, &base, &Vf, &orow);
    float s[VE];
    int am[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) { s[k] = 0.f; am[k] = -1; }
    int cnt = 0;
    bag_ragged_walk<T, IdxT, LOG2L, MAXP, CH, STREAM, WGT>(table, ids, wts, (uint32_t)beg, (uint32_t)end, 1, Vf, base, pad,
                                                          lane_v, err_flag, s, am, cnt);
    bag_ragged_store<T, LOG2L, MAXP>(s, am, cnt, orow, lane_v, out, amax, inv_cnt);
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

template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool WGT, bool FIELDS>
__global__ __launch_bounds__(256) void bag_ragged_long_kernel(const uint4* __restrict__ table,
                                                              const IdxT* __restrict__ ids, int64_t n,
                                                              const void* __restrict__ offsets, bool off64,
                                                              int64_t n_off, int64_t B, int64_t V, int64_t pad,
                                                              const T* __restrict__ wts, uint4* __restrict__ out,
                                                              int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                              const int32_t* __restrict__ queue,
                                                              int32_t* __restrict__ err_flag, BagFieldMap fm) {
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
    int64_t base, Vf, orow;
    bag_field_of<FIELDS>(fm, b, V, &base, &Vf, &orow);
    float s[VE];
    int am[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) { s[k] = 0.f; am[k] = -1; }
    int cnt = 0;
    bag_ragged_walk<T, IdxT, LOG2L, MAXP, CH, STREAM, WGT>(table, ids, wts, (uint32_t)beg + grp, (uint32_t)end, G, Vf, base,
                                                          pad, lane_v, err_flag, s, am, cnt);
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
    if (grp == 0) bag_ragged_store<T, LOG2L, MAXP>(s, am, cnt, orow, lane_v, out, amax, inv_cnt);
  }
}

// generic path: any E; one thread per (b, e), whatever the bag's length
template <typename T, typename IdxT, bool MAXP, bool FIELDS>
__global__ __launch_bounds__(256) void bag_ragged_elem_kernel(const T* __restrict__ table, const IdxT* __restrict__ ids,
                                                              int64_t n, const void* __restrict__ offsets, bool off64,
                                                              int64_t n_off, int64_t B, int E, int64_t V, int64_t pad,
                                                              const T* __restrict__ wts, T* __restrict__ out,
                                                              int32_t* __restrict__ amax, float* __restrict__ inv_cnt,
                                                              int32_t* __restrict__ err_flag, BagFieldMap fm) {
  const int64_t total = B * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t b = udiv_fast(t, E, f32);
    const int e = (int)(t - b * E);
    int64_t beg, end;
    bag_ragged_bounds(offsets, off64, n_off, b, n, err_flag, &beg, &end);
    int64_t base, Vf, orow;
    bag_field_of<FIELDS>(fm, b, V, &base, &Vf, &orow);
    float s = 0.f;
    int am = -1;
    int cnt = 0;
    for (int64_t q = beg; q < end; ++q) {
      const int64_t r = (int64_t)ids[q];
      if (pad >= 0 && r == pad) continue;
      ++cnt;
      T raw = T{};
      if (r < 0 || r >= Vf) {
        if (err_flag != nullptr) *err_flag = 1;
      } else {
        raw = table[(r + base) * E + e];
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
      if (e == 0) inv_cnt[orow] = sc;
      s *= sc;
    }
    out[orow * E + e] = from_f32<T>(s);      // an empty bag: s is still 0, am still -1
    if (MAXP) amax[orow * E + e] = am;
  }
}

template <int = 0>
__global__ void bag_ragged_zero_counter_kernel(int32_t* __restrict__ p) {
  if (threadIdx.x == 0) *p = 0;
}

inline size_t bag_ragged_queue_bytes(int64_t B) { return align_up((size_t)(B + 1) * 4, 256); }

// B: the bags (FIELDS: all F * fm.B of them); ``what`` names the entry in a launch error
template <typename T, typename IdxT, bool FIELDS>
static int bag_ragged_launch(const void* table, const IdxT* ids, int64_t n, const void* offsets, bool off64,
                             int64_t n_off, int64_t B, int E, int64_t V, int mode, int64_t pad, const void* wts_,
                             void* out, int32_t* amax, float* inv_cnt, int32_t* queue, int32_t* err_flag,
                             BagFieldMap fm, const char* what, hipStream_t s) {
  const T* wts = (const T*)wts_;
  const int lg = log2_lanes(E * (int)sizeof(T));
  if (lg >= 0 && aligned16(table) && aligned16(out) && aligned16(amax)) {
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    const bool stream = (size_t)V * E * sizeof(T) > BAG_STREAM_BYTES;
    hipLaunchKernelGGL(bag_ragged_zero_counter_kernel<0>, dim3(1), dim3(64), 0, s, queue);
    dispatch_lanes(lg, [&](auto lg_c) {
      auto launch = [&](auto mx_c, auto ch_c, auto st_c, auto wg_c) {
        constexpr int LG = decltype(lg_c)::value, CH = decltype(ch_c)::value;
        constexpr bool MX = decltype(mx_c)::value, ST = decltype(st_c)::value, WG = decltype(wg_c)::value;
        hipLaunchKernelGGL((bag_ragged_group_kernel<T, IdxT, LG, MX, CH, ST, WG, FIELDS>), dim3(grid), dim3(256), 0, s,
                           (const uint4*)table, ids, n, offsets, off64, n_off, B, V, pad, wts, (uint4*)out, amax,
                           inv_cnt, queue, err_flag, fm);
        // fixed grid, one wave per queued bag: 4096 waves stride the queue (none queued: the waves read the counter
        // and leave)
        hipLaunchKernelGGL((bag_ragged_long_kernel<T, IdxT, LG, MX, BAG_RAGGED_LONG_CH * CH, ST, WG, FIELDS>), dim3(1024),
                           dim3(256), 0, s,
                           (const uint4*)table, ids, n, offsets, off64, n_off, B, V, pad, wts, (uint4*)out, amax,
                           inv_cnt, queue, err_flag, fm);
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
      hipLaunchKernelGGL((bag_ragged_elem_kernel<T, IdxT, true, FIELDS>), dim3(grid), dim3(256), 0, s, (const T*)table,
                         ids, n, offsets, off64, n_off, B, E, V, pad, wts, (T*)out, amax, inv_cnt, err_flag, fm);
    else
      hipLaunchKernelGGL((bag_ragged_elem_kernel<T, IdxT, false, FIELDS>), dim3(grid), dim3(256), 0, s, (const T*)table,
                         ids, n, offsets, off64, n_off, B, E, V, pad, wts, (T*)out, amax, inv_cnt, err_flag, fm);
  }
  return check_launch(what);
}

// The owner of position p among bags [0, B): the last b with offsets[b] <= p, provided p < end_b; else -1.  A binary search
// over the offsets (they sit in L2); a pure function of the offsets.  Whatever the offsets hold, the result is in [-1, B).
__device__ __forceinline__ int32_t bag_ragged_owner_of(const void* __restrict__ offsets, bool off64, int64_t n_off,
                                                       int64_t B, int64_t n, int64_t p) {
  auto at = [&](int64_t b) -> int64_t {
    return off64 ? ((const int64_t*)offsets)[b] : (int64_t)((const int32_t*)offsets)[b];
  };
  int64_t lo = 0, hi = B;                   // the first b in [0, B] with offsets[b] > p
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (at(mid) <= p) lo = mid + 1;
    else hi = mid;
  }
  if (lo > 0) {
    const int64_t b = lo - 1;
    const int64_t end = b + 1 < n_off ? at(b + 1) : n;
    if (p < end) return (int32_t)b;
  }
  return -1;
}

}  // namespace trs
