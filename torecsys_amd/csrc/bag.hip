// Bag pooling: a padded (B, Lb) list of ids looked up in one table and reduced to ONE row per sample (sum / mean / max),
// and the backward of the max.  The reference's ListIndicesEmbedding (inputs/base/list_indices_emb.py:124-152) forms the
// (B, Lb, E) block with aten::embedding, transposes it and pools it; here the block never exists.
//
// Forward layout, as embed_fm_group_kernel (fm.hip): a row of E values is L = E*sizeof(T)/16 sixteen-byte vectors, a GROUP of
// L adjacent lanes owns a sample and walks its bag CH rows at a time, every lane keeping the running sum (or the running
// maximum and the list position that holds it) of its own VE columns in registers -- no cross-lane traffic, no LDS.
// HBM-bound: algorithmic bytes per sample = Lb * (idx bytes + E*s) read, E*s (+ 2*E for the max positions) written.
// Rows in flight: the walk keeps VE sums (max: VE maxima + VE positions) where the FM kernel keeps two sets of VE sums and a
// first-order term, so CH = 8 stays within 64 registers for the sums (compiler resource report) -- the
// occupancy that made 4 beat 8 in fm.hip is not lost here.  The max walk keeps CH = 4.
//
// Gradient walks (bag_walk_*_kernel): the bucket walk of scatter.hip, the term of a lookup and the way its sample is found
// chosen at compile time by a BagWalk policy passed by value.  Max backward: the term of lookup p = (b, l) is g[b, e]
// where amax[b, e] == l and 0 elsewhere.  It reads g (B, E) and amax (B, E), never a (B, Lb, E) block; every table row is
// written (padding row: zeros); no atomics on values, fixed summation order.  Rows with more than BAG_LONG_ROW lookups are
// queued and reduced by whole waves in chunks of BAG_LONG_CHUNK, as scatter.hip's hot rows are.
//
// Masked / weighted variants (trs_bag_pool_masked_fwd): the same two forward kernels with the compile-time flags MASK (a
// position that holds the excluded row id issues no table load and takes no part: sum over the live positions, mean over
// their count -- written as inv_cnt[b] = 1/cnt for the backward, 0 for an empty bag --, max over them with the sentinel
// 0xFFFF in argmax for an empty bag) and WGT (sum only: every term times w[b, l], the weight read once per position).  With
// both flags off the instantiations are the ones above: no branch is added to them.  Algorithmic bytes per sample =
// Lb * idx bytes + cnt * E*s (+ Lb * s of weights) read, E*s (+ 4 for inv_cnt, + 2*E for the max positions) written.
// Weighted backward: the same walk with the term of lookup p = (b, l) being w[p] * g[b, e] (BagTerm::Weighted, same queue
// thresholds BAG_LONG_ROW / BAG_LONG_CHUNK / BAG_LONG_ROW_ELEM), and bag_weight_grad_*_kernel:
// dw[b, l] = sum_e g[b, e] * table[idx[b, l], e], one lane group (or one thread) per position, 0 at excluded positions.
//
// Ragged bags (forward: bag_ragged.hip): the same walks with the mapped layout of the policy -- the sample of lookup p is
// read from a map (bag_of[p], trs_bag_owner) where the padded layout divides p by the list length, and the winners of the
// max are flat int32 positions -- and the same weight-gradient kernels with the compile-time flag RAG.
#include "bag_common.hpp"

namespace trs {

template <typename T, typename IdxT, int LOG2L, bool MAXP, int CH, bool STREAM, bool MASK, bool WGT>
__global__ __launch_bounds__(256) void bag_pool_group_kernel(const uint4* __restrict__ table,
                                                             const IdxT* __restrict__ idx, int64_t B, int Lb, int64_t V,
                                                             float scale, uint4* __restrict__ out,
                                                             uint16_t* __restrict__ amax, int32_t* __restrict__ err_flag,
                                                             int64_t pad, const T* __restrict__ wts,
                                                             float* __restrict__ inv_cnt) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < B; b += groups) {
    float s[VE];
    int am[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) { s[k] = MAXP ? -INFINITY : 0.f; am[k] = 0; }
    int cnt = 0;                            // MASK: live positions of the bag
    for (int l0 = 0; l0 < Lb; l0 += CH) {
      int64_t r[CH];
      uint4 v[CH];
      bool live[CH];                        // MASK only
      float wv[CH];                         // WGT only
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        r[c] = -1;
        live[c] = false;
        wv[c] = 1.f;
        if (l0 + c < Lb) {
          r[c] = (int64_t)idx[b * Lb + l0 + c];
          if (MASK && r[c] == pad) {        // excluded: no load, no term, no count
            r[c] = -1;
          } else {
            live[c] = true;
            if (WGT) wv[c] = to_f32(wts[b * Lb + l0 + c]);
            if (r[c] < 0 || r[c] >= V) {    // reads as a zero row
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
        // MASK: a branch per lane (the bags of a wave end at different positions).  Taking an excluded position as a term of
        // zero / a select instead measured slower: 67.0 against 60.2 us (35 % padding), 76.6 against 74.5 us (none),
        // profiles/bag_kernels.md
        if (MASK ? live[c] : (l0 + c < Lb)) {
          if (MASK) ++cnt;
          float x[VE];
          Vec16<T>::unpack(v[c], x);
#pragma unroll
          for (int k = 0; k < VE; ++k) {
            if (MAXP) {
              if (bag_takes(x[k], s[k])) { s[k] = x[k]; am[k] = l0 + c; }
            } else if (WGT) {
              s[k] += wv[c] * x[k];
            } else {
              s[k] += x[k];
            }
          }
        }
      }
    }
    if (!MAXP) {
      float sc = scale;
      if (MASK && inv_cnt != nullptr) {     // mean over the live positions; an empty bag is a zero row
        sc = cnt > 0 ? 1.f / (float)cnt : 0.f;
        if (lane_v == 0) inv_cnt[b] = sc;
      }
#pragma unroll
      for (int k = 0; k < VE; ++k) s[k] *= sc;
    } else if (MASK && cnt == 0) {          // empty bag: zero row, no position holds the maximum
#pragma unroll
      for (int k = 0; k < VE; ++k) { s[k] = 0.f; am[k] = 0xFFFF; }
    }
    out[b * L + lane_v] = Vec16<T>::pack(s);
    if (MAXP) {
      uint32_t w[VE / 2];
#pragma unroll
      for (int k = 0; k < VE; k += 2) w[k / 2] = (uint32_t)am[k] | ((uint32_t)am[k + 1] << 16);
      uint32_t* dst = reinterpret_cast<uint32_t*>(amax + (b * L + lane_v) * VE);
      if (VE == 8) *reinterpret_cast<uint4*>(dst) = make_uint4(w[0], w[1], w[VE / 2 - 2], w[VE / 2 - 1]);
      else *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    }
  }
}

// generic path: any E; one thread per (b, e)
template <typename T, typename IdxT, bool MAXP, bool MASK, bool WGT>
__global__ __launch_bounds__(256) void bag_pool_elem_kernel(const T* __restrict__ table, const IdxT* __restrict__ idx,
                                                            int64_t B, int Lb, int E, int64_t V, float scale,
                                                            T* __restrict__ out, uint16_t* __restrict__ amax,
                                                            int32_t* __restrict__ err_flag, int64_t pad,
                                                            const T* __restrict__ wts, float* __restrict__ inv_cnt) {
  const int64_t total = B * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t b = udiv_fast(t, E, f32);
    const int e = (int)(t - b * E);
    float s = MAXP ? -INFINITY : 0.f;
    int am = 0;
    int cnt = 0;
    for (int l = 0; l < Lb; ++l) {
      const int64_t r = (int64_t)idx[b * Lb + l];
      if (MASK) {
        if (r == pad) continue;
        ++cnt;
      }
      T raw = T{};
      if (r < 0 || r >= V) {
        if (err_flag != nullptr) *err_flag = 1;
      } else {
        raw = table[r * E + e];
      }
      const float x = to_f32(raw);
      if (MAXP) {
        if (bag_takes(x, s)) { s = x; am = l; }
      } else if (WGT) {
        s += to_f32(wts[b * Lb + l]) * x;
      } else {
        s += x;
      }
    }
    float sc = scale;
    if (MASK && !MAXP && inv_cnt != nullptr) {
      sc = cnt > 0 ? 1.f / (float)cnt : 0.f;
      if (e == 0) inv_cnt[b] = sc;
    }
    if (MASK && MAXP && cnt == 0) { s = 0.f; am = 0xFFFF; }
    out[t] = from_f32<T>(MAXP ? s : s * sc);
    if (MAXP) amax[t] = (uint16_t)am;
  }
}

template <typename T, typename IdxT, bool MASK, bool WGT>
static int bag_pool_launch(const void* table, const IdxT* idx, int64_t B, int Lb, int E, int64_t V, int mode, void* out,
                           uint16_t* amax, int32_t* err_flag, int64_t pad, const void* wts_, float* inv_cnt,
                           hipStream_t s) {
  const T* wts = (const T*)wts_;
  const int lg = log2_lanes(E * (int)sizeof(T));
  const float scale = mode == BAG_MEAN ? 1.f / (float)Lb : 1.f;
  if (lg >= 0 && aligned16(table) && aligned16(out) && aligned16(amax)) {
    const int grid = stream_grid(B << lg, 256, 256 * 16);
    const bool stream = (size_t)V * E * sizeof(T) > BAG_STREAM_BYTES;
    dispatch_lanes(lg, [&](auto lg_c) {
      auto launch = [&](auto mx_c, auto ch_c, auto st_c) {
        hipLaunchKernelGGL((bag_pool_group_kernel<T, IdxT, decltype(lg_c)::value, decltype(mx_c)::value,
                                                  decltype(ch_c)::value, decltype(st_c)::value, MASK, WGT>),
                           dim3(grid), dim3(256), 0, s, (const uint4*)table, idx, B, Lb, V, scale, (uint4*)out, amax,
                           err_flag, pad, wts, inv_cnt);
      };
      constexpr std::integral_constant<int, 4> ch4{};
      constexpr std::integral_constant<int, 8> ch8{};
      if (mode == BAG_MAX) {
        if constexpr (!WGT) {      /* weights: sum only */
          if (stream) launch(std::true_type{}, ch4, std::true_type{});
          else launch(std::true_type{}, ch4, std::false_type{});
        }
      } else {
        if (stream) launch(std::false_type{}, ch8, std::true_type{});
        else launch(std::false_type{}, ch8, std::false_type{});
      }
    });
  } else {
    const int grid = stream_grid(B * E, 256, 256 * 16);
    if (mode == BAG_MAX) {
      if constexpr (!WGT)
        hipLaunchKernelGGL((bag_pool_elem_kernel<T, IdxT, true, MASK, false>), dim3(grid), dim3(256), 0, s,
                           (const T*)table, idx, B, Lb, E, V, scale, (T*)out, amax, err_flag, pad, wts, inv_cnt);
    } else {
      hipLaunchKernelGGL((bag_pool_elem_kernel<T, IdxT, false, MASK, WGT>), dim3(grid), dim3(256), 0, s, (const T*)table,
                         idx, B, Lb, E, V, scale, (T*)out, amax, err_flag, pad, wts, inv_cnt);
    }
  }
  return check_launch(MASK || WGT ? "bag_pool_masked_fwd" : "bag_pool_fwd");
}

// ---------------------------------------------------------------------------------------------
// gradient walks: the bucket walk of scatter.hip, the term of a lookup chosen by a policy

// What lookup p adds to the gradient of its table row, g (samples, E) being the gradient of the pooled rows:
//   Plain     g[b, k]
//   Weighted  wts[p] * g[b, k]
//   Winner    g[b, k] where the stored winner of (b, k) is this lookup, else 0
// and how its sample b is found.  Padded: b = p / N, the winners are the list positions p - b * N, uint16 (B, E).
// Mapped (ragged bags): b = owner[p] (trs_bag_owner; below zero: no bag holds p, no term), the winners are the flat
// positions p, int32 (B, E).  Padded x Plain is the walk of scatter.hip and is not offered here.
enum class BagTerm { Plain, Weighted, Winner };
struct BagNoOperand {};

template <typename T, BagTerm TERM, bool MAPPED>
struct BagWalk {
  static_assert(MAPPED || TERM != BagTerm::Plain, "padded bags with the plain term are served by scatter.hip");
  using value_type = T;
  using WinnerT = std::conditional_t<MAPPED, int32_t, uint16_t>;
  using Operand = std::conditional_t<TERM == BagTerm::Plain, BagNoOperand,
                                     const std::conditional_t<TERM == BagTerm::Weighted, T, WinnerT>*>;
  static constexpr int VE = Vec16<T>::VE;
  // the operand of one lookup in registers (vector path): its weight, or the winners of this lane's VE columns
  struct Held {
    float wv;
    uint4 av[MAPPED ? VE / 4 : 1];
  };

  const T* g;
  std::conditional_t<MAPPED, const int32_t*, unsigned> where;      // mapped: owner (n); padded: the list length N
  [[no_unique_address]] Operand op;                                 // wts (n), or the winners (B, E)

  // of what the vector path loads as 16-byte (padded winners in fp32: 8-byte) vectors
  bool aligned() const {
    if constexpr (TERM == BagTerm::Winner) return aligned16(g) && aligned16(op);
    else return aligned16(g);
  }

  // p >= 0.  Padded: p < B * N < 2^31, one 32-bit unsigned division, never below zero.  Typed per layout -- the int the map
  // holds, the zero-extended quotient -- which keeps every kernel's occupancy (profiles/bag_walk_policy.md)
  using Sample = std::conditional_t<MAPPED, int, int64_t>;
  __device__ __forceinline__ Sample sample(int p) const {
    if constexpr (MAPPED) return where[p];
    else return (int64_t)((unsigned)p / where);
  }

  // vector path: o = b * L + lane_v is the 16-byte vector of g[b] that this lane owns
  __device__ __forceinline__ uint4 g_vec(int64_t o) const { return reinterpret_cast<const uint4*>(g)[o]; }

  __device__ __forceinline__ void hold(Held& h, int p, int64_t o) const {
    if constexpr (TERM == BagTerm::Weighted) {
      h.wv = to_f32(op[p]);
    } else if constexpr (TERM == BagTerm::Winner) {
      if constexpr (MAPPED) {
        const uint4* ap = reinterpret_cast<const uint4*>(op + o * VE);
#pragma unroll
        for (int i = 0; i < VE / 4; ++i) h.av[i] = ap[i];
      } else if constexpr (VE == 8) {
        h.av[0] = *reinterpret_cast<const uint4*>(op + o * VE);
      } else {
        const uint2 a2 = *reinterpret_cast<const uint2*>(op + o * VE);
        h.av[0] = make_uint4(a2.x, a2.y, 0, 0);
      }
    }
  }

  // acc[k] += the term of lookup p of sample b, for this lane's VE columns
  __device__ __forceinline__ void add(float* acc, int p, Sample b, const uint4& gv, const Held& h) const {
    float x[VE];
    Vec16<T>::unpack(gv, x);
    if constexpr (TERM == BagTerm::Plain) {
#pragma unroll
      for (int k = 0; k < VE; ++k) acc[k] += x[k];
    } else if constexpr (TERM == BagTerm::Weighted) {
#pragma unroll
      for (int k = 0; k < VE; ++k) acc[k] += h.wv * x[k];
    } else if constexpr (MAPPED) {
#pragma unroll
      for (int i = 0; i < VE / 4; ++i) {
        const int a[4] = {(int)h.av[i].x, (int)h.av[i].y, (int)h.av[i].z, (int)h.av[i].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[4 * i + j] += a[j] == p ? x[4 * i + j] : 0.f;
      }
    } else {
      const unsigned l = (unsigned)p - (unsigned)b * where;
      const uint32_t w[4] = {h.av[0].x, h.av[0].y, h.av[0].z, h.av[0].w};
#pragma unroll
      for (int k = 0; k < VE; ++k) {
        const unsigned a = (k & 1) ? (w[k >> 1] >> 16) : (w[k >> 1] & 0xffffu);
        acc[k] += a == l ? x[k] : 0.f;
      }
    }
  }

  // element path (any E): the term of lookup p for column e
  __device__ __forceinline__ float term(int p, int E, int e) const {
    const Sample b = sample(p);
    if (MAPPED && b < 0) return 0.f;
    const int64_t o = (int64_t)b * E + e;
    if constexpr (TERM == BagTerm::Plain) return to_f32(g[o]);
    else if constexpr (TERM == BagTerm::Weighted) return to_f32(op[p]) * to_f32(g[o]);
    else if constexpr (MAPPED) return op[o] == p ? to_f32(g[o]) : 0.f;
    else return (unsigned)op[o] == (unsigned)p - (unsigned)b * where ? to_f32(g[o]) : 0.f;
  }
};

// the lookups q = beg, beg + step, ... < end of one bucket, CH in flight per lane: perm, then the sample (mapped: a load),
// then g and the term's operand, then the sum in bucket order
template <typename W, int LOG2L, int CH>
__device__ __forceinline__ void bag_walk_bucket(float* acc, const W& w, const int32_t* __restrict__ perm, int beg,
                                                int end, int step, int lane_v) {
  constexpr int L = 1 << LOG2L;
  for (int q = beg; q < end; q += CH * step) {
    int p[CH];
    typename W::Sample b[CH];
    uint4 gv[CH];
    typename W::Held h[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) p[c] = (q + c * step) < end ? perm[q + c * step] : -1;
#pragma unroll
    for (int c = 0; c < CH; ++c) b[c] = p[c] >= 0 ? w.sample(p[c]) : -1;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      gv[c] = make_uint4(0, 0, 0, 0);
      if (b[c] >= 0) {
        gv[c] = w.g_vec((int64_t)b[c] * L + lane_v);
        w.hold(h[c], p[c], (int64_t)b[c] * L + lane_v);
      }
    }
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (b[c] >= 0) w.add(acc, p[c], b[c], gv[c], h[c]);
    }
  }
}

template <typename W, int LOG2L>
__global__ __launch_bounds__(256) void bag_walk_rows_kernel(W w, const int32_t* __restrict__ row_start,
                                                            const int32_t* __restrict__ perm, int64_t V,
                                                            int64_t padding_row, uint4* __restrict__ grad,
                                                            int32_t* __restrict__ long_rows /* [0] = count */) {
  using T = typename W::value_type;
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t r = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; r < V; r += groups) {
    const int beg = row_start[r], end = row_start[r + 1];
    float acc[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) acc[k] = 0.f;
    if (r != padding_row) {
      if (end - beg > BAG_LONG_ROW) {
        if (lane_v == 0) {
          const int nch = (end - beg + BAG_LONG_CHUNK - 1) / BAG_LONG_CHUNK;
          const int slot = atomicAdd(&long_rows[0], nch);      // the chunks of a row are adjacent in the queue
          for (int c = 0; c < nch; ++c) {
            long_rows[1 + 2 * (slot + c)] = (int32_t)r;
            long_rows[2 + 2 * (slot + c)] = c;
          }
        }
        continue;
      }
      bag_walk_bucket<W, LOG2L, 4>(acc, w, perm, beg, end, 1, lane_v);
    }
    store_stream(&grad[r * L + lane_v], Vec16<T>::pack(acc));
  }
}

// hot rows: one wave per (row, chunk) entry, its 64 / L lane groups stride the chunk, partial sums folded by shuffles.
// Rows of a single chunk are finished here; otherwise the partial goes to scratch[entry][E] (fp32) for the finish kernel.
template <typename W, int LOG2L>
__global__ __launch_bounds__(256) void bag_walk_long_kernel(W w, const int32_t* __restrict__ row_start,
                                                            const int32_t* __restrict__ perm, uint4* __restrict__ grad,
                                                            const int32_t* __restrict__ long_rows,
                                                            float* __restrict__ scratch) {
  using T = typename W::value_type;
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  constexpr int G = 64 / L;
  const int lane = threadIdx.x & 63;
  const int lane_v = lane & (L - 1);
  const int grp = lane >> LOG2L;
  const int nlong = long_rows[0];
  const int waves = gridDim.x * (blockDim.x >> 6);
  for (int i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); i < nlong; i += waves) {
    const int64_t r = long_rows[1 + 2 * i];
    const int c = long_rows[2 + 2 * i];
    const int rbeg = row_start[r], rend = row_start[r + 1];
    const int beg = rbeg + c * BAG_LONG_CHUNK, end = rend < beg + BAG_LONG_CHUNK ? rend : beg + BAG_LONG_CHUNK;
    float acc[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) acc[k] = 0.f;
    bag_walk_bucket<W, LOG2L, 4>(acc, w, perm, beg + grp, end, G, lane_v);
#pragma unroll
    for (int m = L; m < 64; m <<= 1) {
#pragma unroll
      for (int k = 0; k < VE; ++k) acc[k] += __shfl_xor(acc[k], m, 64);
    }
    if (grp == 0) {
      if (rend - rbeg <= BAG_LONG_CHUNK) {
        store_stream(&grad[r * L + lane_v], Vec16<T>::pack(acc));
      } else {
        float* sa = scratch + (size_t)i * (L * VE) + lane_v * VE;
#pragma unroll
        for (int k = 0; k < VE; ++k) sa[k] = acc[k];
      }
    }
  }
}

// rows of several chunks: the first chunk's entry adds the row's partials in chunk order
template <typename T, int LOG2L>
__global__ __launch_bounds__(256) void bag_walk_finish_kernel(const int32_t* __restrict__ row_start,
                                                              uint4* __restrict__ grad,
                                                              const int32_t* __restrict__ long_rows,
                                                              const float* __restrict__ scratch) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int nlong = long_rows[0];
  const int groups = (gridDim.x * blockDim.x) >> LOG2L;
  for (int i = (blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; i < nlong; i += groups) {
    if (long_rows[2 + 2 * i] != 0) continue;
    const int64_t r = long_rows[1 + 2 * i];
    const int len = row_start[r + 1] - row_start[r];
    if (len <= BAG_LONG_CHUNK) continue;
    const int nch = (len + BAG_LONG_CHUNK - 1) / BAG_LONG_CHUNK;
    float acc[VE];
#pragma unroll
    for (int k = 0; k < VE; ++k) acc[k] = 0.f;
    for (int c = 0; c < nch; ++c) {
      const float* sa = scratch + (size_t)(i + c) * (L * VE) + lane_v * VE;
#pragma unroll
      for (int k = 0; k < VE; ++k) acc[k] += sa[k];
    }
    store_stream(&grad[r * L + lane_v], Vec16<T>::pack(acc));
  }
}

// generic path (any E): one thread per (row, e); rows with more than BAG_LONG_ROW_ELEM lookups are queued (one id each)
// and reduced by one wave per row
template <typename W>
__global__ __launch_bounds__(256) void bag_walk_rows_elem_kernel(W w, const int32_t* __restrict__ row_start,
                                                                 const int32_t* __restrict__ perm, int64_t V, int E,
                                                                 int64_t padding_row,
                                                                 typename W::value_type* __restrict__ grad,
                                                                 int32_t* __restrict__ long_rows) {
  using T = typename W::value_type;
  const int64_t total = V * E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = udiv_fast(t, E, f32);
    const int e = (int)(t - r * E);
    float acc = 0.f;
    if (r != padding_row) {
      const int beg = row_start[r], end = row_start[r + 1];
      if (end - beg > BAG_LONG_ROW_ELEM) {
        if (e == 0) long_rows[1 + atomicAdd(&long_rows[0], 1)] = (int32_t)r;
        continue;
      }
      for (int q = beg; q < end; ++q) acc += w.term(perm[q], E, e);
    }
    grad[t] = from_f32<T>(acc);
  }
}

template <typename W>
__global__ __launch_bounds__(256) void bag_walk_long_elem_kernel(W w, const int32_t* __restrict__ row_start,
                                                                 const int32_t* __restrict__ perm, int E,
                                                                 typename W::value_type* __restrict__ grad,
                                                                 const int32_t* __restrict__ long_rows) {
  using T = typename W::value_type;
  const int nlong = long_rows[0];
  const int lane = threadIdx.x & 63;
  const int wid = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int i = wid; i < nlong; i += nwaves) {
    const int64_t r = long_rows[1 + i];
    const int beg = row_start[r], end = row_start[r + 1];
    for (int e = 0; e < E; ++e) {
      float acc = 0.f;
      constexpr int U = 4;
      for (int q = beg + lane; q < end; q += 64 * U) {
        int pp[U];
#pragma unroll
        for (int u = 0; u < U; ++u) pp[u] = (q + 64 * u) < end ? perm[q + 64 * u] : -1;
#pragma unroll
        for (int u = 0; u < U; ++u)
          if (pp[u] >= 0) acc += w.term(pp[u], E, e);
      }
      acc = group_sum_down<64>(acc);
      if (lane == 0) grad[r * E + e] = from_f32<T>(acc);
    }
  }
}

__global__ void bag_zero_counter_kernel(int32_t* __restrict__ p) {
  if (threadIdx.x == 0) *p = 0;
}

// queue entries: a row is queued with more than 32 (element path; one id) or 64 lookups (one (row, chunk) pair per chunk)
static size_t bag_queue_entries(int64_t BN) { return (size_t)(BN / BAG_LONG_ROW + BN / BAG_LONG_CHUNK + 2); }
static size_t bag_queue_bytes(int64_t BN) {
  return align_up(std::max(bag_queue_entries(BN) * 8 + 8, (size_t)(BN / BAG_LONG_ROW_ELEM + 3) * 4), 256);
}

// entry: the C entry that check_launch reports
template <typename W>
static int bag_walk_launch(const W& w, const char* entry, const int32_t* row_start, const int32_t* perm, int64_t V, int E,
                           int64_t padding_row, void* grad, int32_t* long_rows, float* scratch, hipStream_t s) {
  using T = typename W::value_type;
  const int lg = log2_lanes(E * (int)sizeof(T));
  hipLaunchKernelGGL(bag_zero_counter_kernel, dim3(1), dim3(64), 0, s, long_rows);
  if (lg >= 0 && w.aligned() && aligned16(grad)) {
    const int grid = stream_grid(V << lg, 256, 256 * 32);
    dispatch_lanes(lg, [&](auto lg_c) {
      constexpr int LG = decltype(lg_c)::value;
      hipLaunchKernelGGL((bag_walk_rows_kernel<W, LG>), dim3(grid), dim3(256), 0, s, w, row_start, perm, V, padding_row,
                         (uint4*)grad, long_rows);
      hipLaunchKernelGGL((bag_walk_long_kernel<W, LG>), dim3(2048), dim3(256), 0, s, w, row_start, perm, (uint4*)grad,
                         long_rows, scratch);
      hipLaunchKernelGGL((bag_walk_finish_kernel<T, LG>), dim3(64), dim3(256), 0, s, row_start, (uint4*)grad,
                         long_rows, scratch);
    });
  } else {
    hipLaunchKernelGGL((bag_walk_rows_elem_kernel<W>), dim3(stream_grid(V * E, 256, 256 * 32)), dim3(256), 0, s, w,
                       row_start, perm, V, E, padding_row, (T*)grad, long_rows);
    hipLaunchKernelGGL((bag_walk_long_elem_kernel<W>), dim3(2048), dim3(256), 0, s, w, row_start, perm, E, (T*)grad,
                       long_rows);
  }
  return check_launch(entry);
}

// ---------------------------------------------------------------------------------------------
// weight gradient: dw[b, l] = sum_e g[b, e] * table[idx[b, l], e]; 0 where the position is excluded or out of range

// a group of L lanes per position p = b * Lb + l: one 16-byte vector of the row and of g[b] per lane, fp32 products summed
// in column order inside the lane, then folded over the group by shuffles (fixed order)
// RAG (ragged bags): the sample of position p is bag_of[p]; < 0 (no bag holds p): dw[p] = 0
template <typename T, typename IdxT, int LOG2L, bool RAG>
__global__ __launch_bounds__(256) void bag_weight_grad_group_kernel(const uint4* __restrict__ table,
                                                                    const uint4* __restrict__ g,
                                                                    const IdxT* __restrict__ idx, int64_t BN, int Lb,
                                                                    int64_t V, int64_t pad, T* __restrict__ dw,
                                                                    const int32_t* __restrict__ bag_of) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  const int lane_v = threadIdx.x & (L - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L;
  const int64_t trips = (BN + groups - 1) / groups;      // the same for every lane: the shuffles need the whole wave
  const bool f32 = BN < ((int64_t)1 << 32);
  for (int64_t it = 0; it < trips; ++it) {
    const int64_t p = first + it * groups;
    float d = 0.f;
    if (p < BN) {
      const int64_t r = (int64_t)idx[p];
      if (r != pad && r >= 0 && r < V && (!RAG || bag_of[p] >= 0)) {
        const int64_t b = RAG ? (int64_t)bag_of[p] : udiv_fast(p, Lb, f32);
        float x[VE], y[VE];
        Vec16<T>::unpack(table[r * L + lane_v], x);
        Vec16<T>::unpack(g[b * L + lane_v], y);
#pragma unroll
        for (int k = 0; k < VE; ++k) d += x[k] * y[k];
      }
    }
    d = group_sum_up<L>(d);
    if (p < BN && lane_v == 0) dw[p] = from_f32<T>(d);
  }
}

// generic path (any E): one thread per position
template <typename T, typename IdxT, bool RAG>
__global__ __launch_bounds__(256) void bag_weight_grad_elem_kernel(const T* __restrict__ table, const T* __restrict__ g,
                                                                   const IdxT* __restrict__ idx, int64_t BN, int Lb,
                                                                   int E, int64_t V, int64_t pad, T* __restrict__ dw,
                                                                   const int32_t* __restrict__ bag_of) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = BN < ((int64_t)1 << 32);
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < BN; p += stride) {
    const int64_t r = (int64_t)idx[p];
    float d = 0.f;
    if (r != pad && r >= 0 && r < V && (!RAG || bag_of[p] >= 0)) {
      const int64_t b = RAG ? (int64_t)bag_of[p] : udiv_fast(p, Lb, f32);
      for (int e = 0; e < E; ++e) d += to_f32(table[r * E + e]) * to_f32(g[b * E + e]);
    }
    dw[p] = from_f32<T>(d);
  }
}

// RAG: B = the n positions of the flat id vector, Lb = 1
template <typename T, typename IdxT, bool RAG = false>
static int bag_weight_grad_launch(const void* table, const void* g, const IdxT* idx, int64_t B, int Lb, int E, int64_t V,
                                  int64_t pad, void* dw, hipStream_t s, const int32_t* bag_of = nullptr) {
  const int lg = log2_lanes(E * (int)sizeof(T));
  const int64_t BN = B * Lb;
  if (lg >= 0 && aligned16(table) && aligned16(g)) {
    const int grid = stream_grid(BN << lg, 256, 256 * 32);
    dispatch_lanes(lg, [&](auto lg_c) {
      hipLaunchKernelGGL((bag_weight_grad_group_kernel<T, IdxT, decltype(lg_c)::value, RAG>), dim3(grid), dim3(256), 0,
                         s, (const uint4*)table, (const uint4*)g, idx, BN, Lb, V, pad, (T*)dw, bag_of);
    });
  } else {
    hipLaunchKernelGGL((bag_weight_grad_elem_kernel<T, IdxT, RAG>), dim3(stream_grid(BN, 256, 256 * 32)), dim3(256), 0,
                       s, (const T*)table, (const T*)g, idx, BN, Lb, E, V, pad, (T*)dw, bag_of);
  }
  return check_launch(RAG ? "bag_weight_grad_ragged" : "bag_weight_grad");
}

}  // namespace trs

using namespace trs;

extern "C" int trs_bag_pool_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx,
                                int32_t idx_dtype, int64_t B, int32_t L, int32_t mode, void* out, uint16_t* argmax,
                                int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && idx && out, TRS_EINVAL, "bag_pool_fwd: NULL pointer");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN || mode == BAG_MAX, TRS_EINVAL,
              "bag_pool_fwd: mode %d (0 = sum, 1 = mean, 2 = max)", mode);
  TRS_REQUIRE(mode != BAG_MAX || argmax != nullptr, TRS_EINVAL, "bag_pool_fwd: max pooling needs the argmax output");
  TRS_REQUIRE(V > 0 && E > 0 && B >= 0, TRS_EINVAL, "bag_pool_fwd: bad size V=%lld E=%d B=%lld", (long long)V, E,
              (long long)B);
  TRS_REQUIRE(L >= 1 && L <= 65535, TRS_EINVAL, "bag_pool_fwd: list length L=%d outside [1, 65535]", L);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_fwd: dtype %d", dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_fwd: idx dtype %d", idx_dtype);
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I)                                                                                            \
  return bag_pool_launch<T, I, false, false>(table, (const I*)idx, B, L, E, V, mode, out, argmax, err_flag, -1, nullptr, \
                                             nullptr, s)
  if (dtype == TRS_F32) {
    if (idx_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (idx_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}

extern "C" size_t trs_scatter_argmax_workspace_bytes(int64_t BN, int32_t E) {
  // [queue of hot rows + its counter][chunk partials of the rows of several chunks: entries x E fp32]
  if (BN < 0 || E < 0) return 0;
  return bag_queue_bytes(BN) + align_up(bag_queue_entries(BN) * (size_t)E * 4, 256);
}

// What the walk entries share once their sizes are known to be sound: the dtype and workspace checks, under the entry's
// name, and the workspace carved into the queue and the chunk partials.
struct BagWalkSpace {
  int32_t* long_rows;
  float* scratch;
};

static int bag_walk_space(const char* name, int64_t BN, int32_t E, int32_t dtype, void* workspace, size_t ws_bytes,
                          BagWalkSpace* sp) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", name, dtype);
  const size_t need = trs_scatter_argmax_workspace_bytes(BN, E);
  TRS_REQUIRE(ws_bytes >= need, TRS_EWORKSPACE, "%s: workspace %zu < %zu", name, ws_bytes, need);
  sp->long_rows = (int32_t*)workspace;
  sp->scratch = (float*)((char*)workspace + bag_queue_bytes(BN));
  return TRS_OK;
}

// the two padded walks: operand = the winners (B, E) uint16, or the weights (B, N) of the table's dtype
template <BagTerm TERM>
static int bag_walk_padded(const char* name, const void* g, const void* operand, const int32_t* row_start,
                           const int32_t* perm, int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype,
                           int64_t padding_row, void* grad_table, void* workspace, size_t ws_bytes, trs_stream_t stream) {
  TRS_REQUIRE(g && operand && row_start && perm && grad_table && workspace, TRS_EINVAL, "%s: NULL pointer", name);
  TRS_REQUIRE(V > 0 && E > 0 && BN >= 0, TRS_EINVAL, "%s: bad size", name);
  TRS_REQUIRE(N >= 1 && N <= 65535, TRS_EINVAL, "%s: list length L=%d outside [1, 65535]", name, N);
  TRS_REQUIRE(BN % N == 0, TRS_EINVAL, "%s: B*L=%lld not a multiple of L=%d", name, (long long)BN, N);
  TRS_REQUIRE(BN < (int64_t)0x7fffffff, TRS_ESHAPE, "%s: B*L=%lld must fit int32", name, (long long)BN);
  BagWalkSpace sp;
  if (const int rc = bag_walk_space(name, BN, E, dtype, workspace, ws_bytes, &sp); rc != TRS_OK) return rc;
  auto launch = [&](auto t) {
    using W = BagWalk<decltype(t), TERM, false>;
    return bag_walk_launch(W{(const decltype(t)*)g, (unsigned)N, (typename W::Operand)operand}, name, row_start, perm, V,
                           E, padding_row, grad_table, sp.long_rows, sp.scratch, (hipStream_t)stream);
  };
  return dtype == TRS_F32 ? launch(float{}) : launch(bf16_t{});
}

extern "C" int trs_scatter_rows_argmax(const void* g, const uint16_t* argmax, const int32_t* row_start,
                                       const int32_t* perm, int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype,
                                       int64_t padding_row, void* grad_table, void* workspace, size_t ws_bytes,
                                       trs_stream_t stream) {
  return bag_walk_padded<BagTerm::Winner>("scatter_rows_argmax", g, argmax, row_start, perm, BN, V, E, N, dtype,
                                          padding_row, grad_table, workspace, ws_bytes, stream);
}

extern "C" int trs_bag_pool_masked_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx,
                                       int32_t idx_dtype, int64_t B, int32_t L, int32_t mode, int64_t exclude_row,
                                       const void* weights, void* out, uint16_t* argmax, float* inv_cnt,
                                       int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && idx && out, TRS_EINVAL, "bag_pool_masked_fwd: NULL pointer");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN || mode == BAG_MAX, TRS_EINVAL,
              "bag_pool_masked_fwd: mode %d (0 = sum, 1 = mean, 2 = max)", mode);
  TRS_REQUIRE(V > 0 && E > 0 && B >= 0, TRS_EINVAL, "bag_pool_masked_fwd: bad size V=%lld E=%d B=%lld", (long long)V, E,
              (long long)B);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL, "bag_pool_masked_fwd: exclude_row %lld outside [-1, V)",
              (long long)exclude_row);
  TRS_REQUIRE(exclude_row >= 0 || weights != nullptr, TRS_EINVAL,
              "bag_pool_masked_fwd: neither an excluded row nor weights (that case is trs_bag_pool_fwd)");
  TRS_REQUIRE(weights == nullptr || mode == BAG_SUM, TRS_EINVAL, "bag_pool_masked_fwd: weights need mode 0 (sum), got %d",
              mode);
  TRS_REQUIRE(mode != BAG_MAX || argmax != nullptr, TRS_EINVAL,
              "bag_pool_masked_fwd: max pooling needs the argmax output");
  TRS_REQUIRE(mode != BAG_MEAN || exclude_row < 0 || inv_cnt != nullptr, TRS_EINVAL,
              "bag_pool_masked_fwd: the mean over the live positions needs the inv_cnt output");
  TRS_REQUIRE(L >= 1 && L <= (mode == BAG_MAX && exclude_row >= 0 ? 65534 : 65535), TRS_EINVAL,
              "bag_pool_masked_fwd: list length L=%d outside [1, %d]", L,
              mode == BAG_MAX && exclude_row >= 0 ? 65534 : 65535);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_masked_fwd: dtype %d", dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_masked_fwd: idx dtype %d", idx_dtype);
  hipStream_t s = (hipStream_t)stream;
  float* ic = mode == BAG_MEAN ? inv_cnt : nullptr;
#define TRS_CALL3(T, I, M, W)                                                                                       \
  return bag_pool_launch<T, I, M, W>(table, (const I*)idx, B, L, E, V, mode, out, argmax, err_flag, exclude_row, weights, \
                                     ic, s)
#define TRS_CALL(T, I)                            \
  do {                                            \
    if (exclude_row >= 0) {                       \
      if (weights != nullptr) TRS_CALL3(T, I, true, true); \
      TRS_CALL3(T, I, true, false);               \
    }                                             \
    TRS_CALL3(T, I, false, true);                 \
  } while (0)
  if (dtype == TRS_F32) {
    if (idx_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (idx_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
#undef TRS_CALL3
}

extern "C" size_t trs_scatter_weighted_workspace_bytes(int64_t BN, int32_t E) {
  return trs_scatter_argmax_workspace_bytes(BN, E);      // the same queue and chunk partials
}

extern "C" int trs_scatter_rows_weighted(const void* g, const void* weights, const int32_t* row_start,
                                         const int32_t* perm, int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype,
                                         int64_t padding_row, void* grad_table, void* workspace, size_t ws_bytes,
                                         trs_stream_t stream) {
  return bag_walk_padded<BagTerm::Weighted>("scatter_rows_weighted", g, weights, row_start, perm, BN, V, E, N, dtype,
                                            padding_row, grad_table, workspace, ws_bytes, stream);
}

extern "C" int trs_bag_weight_grad(const void* g, const void* table, int64_t V, int32_t E, int32_t dtype,
                                   const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t exclude_row,
                                   void* dw, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(g && table && idx && dw, TRS_EINVAL, "bag_weight_grad: NULL pointer");
  TRS_REQUIRE(V > 0 && E > 0 && B >= 0, TRS_EINVAL, "bag_weight_grad: bad size V=%lld E=%d B=%lld", (long long)V, E,
              (long long)B);
  TRS_REQUIRE(L >= 1 && L <= 65535, TRS_EINVAL, "bag_weight_grad: list length L=%d outside [1, 65535]", L);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL, "bag_weight_grad: exclude_row %lld outside [-1, V)",
              (long long)exclude_row);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_weight_grad: dtype %d", dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "bag_weight_grad: idx dtype %d", idx_dtype);
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I) return bag_weight_grad_launch<T, I>(table, g, (const I*)idx, B, L, E, V, exclude_row, dw, s)
  if (dtype == TRS_F32) {
    if (idx_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (idx_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}

// ---------------------------------------------------------------------------------------------
// ragged bags (forward: bag_ragged.hip): the walks above with the sample of a lookup read from bag_of

extern "C" size_t trs_scatter_ragged_workspace_bytes(int64_t n, int32_t E) {
  return trs_scatter_argmax_workspace_bytes(n, E);      // the same queue and chunk partials
}

extern "C" int trs_scatter_rows_ragged(const void* g, const int32_t* bag_of, const void* weights, const int32_t* argmax,
                                       const int32_t* row_start, const int32_t* perm, int64_t n, int64_t B, int64_t V,
                                       int32_t E, int32_t dtype, int64_t padding_row, void* grad_table, void* workspace,
                                       size_t ws_bytes, trs_stream_t stream) {
  TRS_REQUIRE(g && bag_of && row_start && perm && grad_table && workspace, TRS_EINVAL,
              "scatter_rows_ragged: NULL pointer");
  TRS_REQUIRE(weights == nullptr || argmax == nullptr, TRS_EINVAL,
              "scatter_rows_ragged: weights and argmax are two different terms, pass one of them at most");
  TRS_REQUIRE(V > 0 && E > 0 && n >= 0 && B > 0, TRS_EINVAL, "scatter_rows_ragged: bad size n=%lld B=%lld V=%lld E=%d",
              (long long)n, (long long)B, (long long)V, E);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE,
              "scatter_rows_ragged: n=%lld and B=%lld must fit int32", (long long)n, (long long)B);
  BagWalkSpace sp;
  if (const int rc = bag_walk_space("scatter_rows_ragged", n, E, dtype, workspace, ws_bytes, &sp); rc != TRS_OK) return rc;
#define TRS_CALL(T, TERM, ...)                                                                                        \
  return bag_walk_launch(BagWalk<T, BagTerm::TERM, true>{(const T*)g, bag_of, __VA_ARGS__}, "scatter_rows_ragged",   \
                         row_start, perm, V, E, padding_row, grad_table, sp.long_rows, sp.scratch, (hipStream_t)stream)
#define TRS_TERM(T)                                                    \
  do {                                                                 \
    if (weights != nullptr) TRS_CALL(T, Weighted, (const T*)weights);  \
    if (argmax != nullptr) TRS_CALL(T, Winner, argmax);                \
    TRS_CALL(T, Plain, {});                                            \
  } while (0)
  if (dtype == TRS_F32) TRS_TERM(float);
  TRS_TERM(bf16_t);
#undef TRS_TERM
#undef TRS_CALL
}

extern "C" int trs_bag_weight_grad_ragged(const void* g, const void* table, int64_t V, int32_t E, int32_t dtype,
                                          const void* ids, int32_t ids_dtype, int64_t n, const int32_t* bag_of,
                                          int64_t exclude_row, void* dw, trs_stream_t stream) {
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(g && table && ids && bag_of && dw, TRS_EINVAL, "bag_weight_grad_ragged: NULL pointer");
  TRS_REQUIRE(V > 0 && E > 0 && n >= 0, TRS_EINVAL, "bag_weight_grad_ragged: bad size V=%lld E=%d n=%lld", (long long)V,
              E, (long long)n);
  TRS_REQUIRE(n < (int64_t)0x7fffffff, TRS_ESHAPE, "bag_weight_grad_ragged: n=%lld must fit int32", (long long)n);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL,
              "bag_weight_grad_ragged: exclude_row %lld outside [-1, V)", (long long)exclude_row);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_weight_grad_ragged: dtype %d", dtype);
  TRS_REQUIRE(ids_dtype == TRS_I64 || ids_dtype == TRS_I32, TRS_EDTYPE, "bag_weight_grad_ragged: ids dtype %d",
              ids_dtype);
  hipStream_t s = (hipStream_t)stream;
#define TRS_CALL(T, I) \
  return bag_weight_grad_launch<T, I, true>(table, g, (const I*)ids, n, 1, E, V, exclude_row, dw, s, bag_of)
  if (dtype == TRS_F32) {
    if (ids_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (ids_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}
