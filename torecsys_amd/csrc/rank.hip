// Pair scoring for the embedding models (MatrixFactorizationModel, StarSpaceModel) and the ranking losses over the scores.
//
//   scores[b, j] = sim(A[a_b], T[t_bj]),  j = 0 .. K  (column 0: the positive, 1 .. K: sampled negatives)
//       sim 0: inner product   layers/emb/generalized_matrix_factorization.py:44-57, utils/operations.py inner_product_similarity
//       sim 1: cosine          layers/emb/starspace.py:62-90 with F.cosine_similarity: dot / (max(|a|, eps) max(|t|, eps))
//
// The reference repeats the anchor id K times (miners/uniform_batch_miner.py:37-42), gathers a (B (1+K), 2, E) block and
// multiplies its two halves; here a lane group owns a sample, reads the anchor row ONCE into registers and walks the 1 + K
// target rows CH at a time: no block is formed.  HBM-bound: B (2+K) (idx bytes + E s) read, B (1+K) s written.
// Backward: rows re-gathered, norms and cosines recomputed; the gradient ROWS go to one (B, 2+K, E) block ordered
// [anchor, positive, negatives] that the bucket walk of scatter.hip reduces into the table(s).  No atomics, the anchor
// row's sum runs over j in order: reproducible bits.
//
// Paths, as bag.hip: rows that are 1, 2, 4 .. 64 whole 16-byte vectors behind 16-byte aligned pointers take the lane-group
// kernels; any other E runs one thread per (b, j) (the backward: one thread per (b, j) for the target rows and the
// coefficients of the anchor row, then one thread per (b, e) for the anchor row).
//
// Ranking losses (losses/ltr/functional.py, pairwise_ranking_loss.py, pointwise_ranking_loss.py): one thread per sample walks
// its K negatives, per-workgroup partial sums in a fixed order, a one-wave finish -- the pattern of head.hip's BCE.
#include <algorithm>
#include <cmath>

#include "trs_common.hpp"

namespace trs {

constexpr int SIM_DOT = 0, SIM_COS = 1;
constexpr float COS_EPS = 1e-8f;      // F.cosine_similarity's default eps; each norm is clamped separately

__device__ __forceinline__ int64_t rank_load_id(const void* __restrict__ idx, bool i64, int64_t p) {
  return i64 ? static_cast<const int64_t*>(idx)[p] : (int64_t) static_cast<const int32_t*>(idx)[p];
}
__device__ __forceinline__ float rank_load_val(const void* __restrict__ x, bool f32, int64_t p) {
  return f32 ? static_cast<const float*>(x)[p] : bf16_bits_to_f32(static_cast<const uint16_t*>(x)[p]);
}
__device__ __forceinline__ void rank_store_val(void* __restrict__ x, bool f32, int64_t p, float v) {
  if (f32) static_cast<float*>(x)[p] = v;
  else static_cast<uint16_t*>(x)[p] = (uint16_t)f32_to_bf16_bits(v);
}

struct PairArgs {
  const void* a_table;
  const void* a_idx;
  const void* t_table;
  const void* t_idx;
  int64_t a_off, t_off, Va, Vt, B;
  int K1;            // 1 + K target columns
  int E;
  int sim;
  bool idx64;
};

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int LOG2L>
__global__ __launch_bounds__(256) void pair_score_group_kernel(PairArgs p, void* __restrict__ scores, bool out_f32,
                                                               int32_t* __restrict__ err_flag) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  constexpr int CH = 4;
  const uint4* __restrict__ A = static_cast<const uint4*>(p.a_table);
  const uint4* __restrict__ Tt = static_cast<const uint4*>(p.t_table);
  const int lane_v = threadIdx.x & (L - 1);
  const bool cosine = p.sim == SIM_COS;
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < p.B; b += groups) {
    int64_t ra = rank_load_id(p.a_idx, p.idx64, b) + p.a_off;
    if (ra < 0 || ra >= p.Va) {      // reads as a zero row
      if (err_flag != nullptr) *err_flag = 1;
      ra = -1;
    }
    float a[VE];
    Vec16<T>::unpack(ra >= 0 ? A[ra * L + lane_v] : make_uint4(0, 0, 0, 0), a);
    float na = 1.f;
    if (cosine) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < VE; ++k) s += a[k] * a[k];
      na = fmaxf(sqrtf(group_sum_up<(1 << LOG2L)>(s)), COS_EPS);
    }
    for (int j0 = 0; j0 < p.K1; j0 += CH) {
      int64_t r[CH];
      uint4 v[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        r[c] = -1;
        if (j0 + c < p.K1) {
          r[c] = rank_load_id(p.t_idx, p.idx64, b * p.K1 + j0 + c) + p.t_off;
          if (r[c] < 0 || r[c] >= p.Vt) {
            if (err_flag != nullptr) *err_flag = 1;
            r[c] = -1;
          }
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) v[c] = r[c] >= 0 ? Tt[r[c] * L + lane_v] : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (j0 + c < p.K1) {      // uniform over the lane group (and the wave)
          float t[VE];
          Vec16<T>::unpack(v[c], t);
          float d = 0.f, s = 0.f;
#pragma unroll
          for (int k = 0; k < VE; ++k) {
            d += a[k] * t[k];
            s += t[k] * t[k];
          }
          d = group_sum_up<(1 << LOG2L)>(d);
          if (cosine) d = d / (na * fmaxf(sqrtf(group_sum_up<(1 << LOG2L)>(s)), COS_EPS));
          if (lane_v == 0) rank_store_val(scores, out_f32, b * p.K1 + j0 + c, d);
        }
      }
    }
  }
}

// generic path: any E; one thread per (b, j)
template <typename T>
__global__ __launch_bounds__(256) void pair_score_elem_kernel(PairArgs p, void* __restrict__ scores, bool out_f32,
                                                              int32_t* __restrict__ err_flag) {
  const T* __restrict__ A = static_cast<const T*>(p.a_table);
  const T* __restrict__ Tt = static_cast<const T*>(p.t_table);
  const int64_t total = p.B * p.K1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t b = udiv_fast(q, p.K1, f32);
    int64_t ra = rank_load_id(p.a_idx, p.idx64, b) + p.a_off;
    int64_t rt = rank_load_id(p.t_idx, p.idx64, q) + p.t_off;
    const bool oka = ra >= 0 && ra < p.Va, okt = rt >= 0 && rt < p.Vt;
    if ((!oka || !okt) && err_flag != nullptr) *err_flag = 1;
    float d = 0.f, sa = 0.f, st = 0.f;
    if (oka || okt) {
      for (int e = 0; e < p.E; ++e) {
        const float x = oka ? to_f32(A[ra * p.E + e]) : 0.f;
        const float y = okt ? to_f32(Tt[rt * p.E + e]) : 0.f;
        d += x * y;
        sa += x * x;
        st += y * y;
      }
    }
    if (p.sim == SIM_COS) d = d / (fmaxf(sqrtf(sa), COS_EPS) * fmaxf(sqrtf(st), COS_EPS));
    rank_store_val(scores, out_f32, q, d);
  }
}

// ------------------------------------------------------------------------------------------------ backward
// gblock (B, 2+K, E): row 0 of a sample its anchor's gradient, rows 1 .. 1+K its targets'
template <typename T, int LOG2L>
__global__ __launch_bounds__(256) void pair_score_bwd_group_kernel(PairArgs p, const void* __restrict__ g,
                                                                   bool g_f32, uint4* __restrict__ gblock) {
  constexpr int L = 1 << LOG2L;
  constexpr int VE = Vec16<T>::VE;
  constexpr int CH = 2;
  const uint4* __restrict__ A = static_cast<const uint4*>(p.a_table);
  const uint4* __restrict__ Tt = static_cast<const uint4*>(p.t_table);
  const int lane_v = threadIdx.x & (L - 1);
  const bool cosine = p.sim == SIM_COS;
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> LOG2L;
  for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> LOG2L; b < p.B; b += groups) {
    int64_t ra = rank_load_id(p.a_idx, p.idx64, b) + p.a_off;
    if (ra < 0 || ra >= p.Va) ra = -1;
    float a[VE], ga[VE];
    Vec16<T>::unpack(ra >= 0 ? A[ra * L + lane_v] : make_uint4(0, 0, 0, 0), a);
#pragma unroll
    for (int k = 0; k < VE; ++k) ga[k] = 0.f;
    float na2 = 0.f, na = 0.f, na_c = 1.f, gcos = 0.f;      // gcos = sum_j g_j cos_j
    if (cosine) {
#pragma unroll
      for (int k = 0; k < VE; ++k) na2 += a[k] * a[k];
      na2 = group_sum_up<(1 << LOG2L)>(na2);
      na = sqrtf(na2);
      na_c = fmaxf(na, COS_EPS);
    }
    uint4* __restrict__ rows = gblock + b * (p.K1 + 1) * L;
    for (int j0 = 0; j0 < p.K1; j0 += CH) {
      int64_t r[CH];
      uint4 v[CH];
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        r[c] = -1;
        if (j0 + c < p.K1) {
          r[c] = rank_load_id(p.t_idx, p.idx64, b * p.K1 + j0 + c) + p.t_off;
          if (r[c] < 0 || r[c] >= p.Vt) r[c] = -1;
        }
      }
#pragma unroll
      for (int c = 0; c < CH; ++c) v[c] = r[c] >= 0 ? Tt[r[c] * L + lane_v] : make_uint4(0, 0, 0, 0);
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (j0 + c < p.K1) {
          float t[VE], gt[VE];
          Vec16<T>::unpack(v[c], t);
          const float gj = rank_load_val(g, g_f32, b * p.K1 + j0 + c);
          if (!cosine) {
#pragma unroll
            for (int k = 0; k < VE; ++k) {
              gt[k] = gj * a[k];
              ga[k] += gj * t[k];
            }
          } else {
            float d = 0.f, s = 0.f;
#pragma unroll
            for (int k = 0; k < VE; ++k) {
              d += a[k] * t[k];
              s += t[k] * t[k];
            }
            d = group_sum_up<(1 << LOG2L)>(d);
            s = group_sum_up<(1 << LOG2L)>(s);
            const float nt = sqrtf(s);
            const float inv = 1.f / (na_c * fmaxf(nt, COS_EPS));
            const float cs = d * inv;
            const float back = nt > COS_EPS ? cs / s : 0.f;      // the clamp passes no gradient to a norm below eps
            gcos += gj * cs;
#pragma unroll
            for (int k = 0; k < VE; ++k) {
              gt[k] = gj * (a[k] * inv - back * t[k]);
              ga[k] += (gj * inv) * t[k];
            }
          }
          if (r[c] < 0) {
#pragma unroll
            for (int k = 0; k < VE; ++k) gt[k] = 0.f;
          }
          rows[(1 + j0 + c) * L + lane_v] = Vec16<T>::pack(gt);
        }
      }
    }
    if (cosine && na > COS_EPS) {
      const float back = gcos / na2;
#pragma unroll
      for (int k = 0; k < VE; ++k) ga[k] -= back * a[k];
    }
    if (ra < 0) {
#pragma unroll
      for (int k = 0; k < VE; ++k) ga[k] = 0.f;
    }
    rows[lane_v] = Vec16<T>::pack(ga);
  }
}

// generic path, first launch: one thread per (b, j) writes the target's gradient row and the two coefficients of the
// anchor row's sum: coef[b, j] = (multiplier of t_j, g_j cos_j)
template <typename T>
__global__ __launch_bounds__(256) void pair_score_bwd_elem_kernel(PairArgs p, const void* __restrict__ g, bool g_f32,
                                                                  T* __restrict__ gblock, float2* __restrict__ coef) {
  const T* __restrict__ A = static_cast<const T*>(p.a_table);
  const T* __restrict__ Tt = static_cast<const T*>(p.t_table);
  const int64_t total = p.B * p.K1;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t b = udiv_fast(q, p.K1, f32);
    const int j = (int)(q - b * p.K1);
    const int64_t ra = rank_load_id(p.a_idx, p.idx64, b) + p.a_off;
    const int64_t rt = rank_load_id(p.t_idx, p.idx64, q) + p.t_off;
    const bool oka = ra >= 0 && ra < p.Va, okt = rt >= 0 && rt < p.Vt;
    const float gj = rank_load_val(g, g_f32, q);
    T* __restrict__ row = gblock + (b * (p.K1 + 1) + 1 + j) * p.E;
    float inv = 1.f, back = 0.f, cs = 0.f;
    if (p.sim == SIM_COS) {
      float d = 0.f, sa = 0.f, st = 0.f;
      for (int e = 0; e < p.E; ++e) {
        const float x = oka ? to_f32(A[ra * p.E + e]) : 0.f;
        const float y = okt ? to_f32(Tt[rt * p.E + e]) : 0.f;
        d += x * y;
        sa += x * x;
        st += y * y;
      }
      const float nt = sqrtf(st);
      inv = 1.f / (fmaxf(sqrtf(sa), COS_EPS) * fmaxf(nt, COS_EPS));
      cs = d * inv;
      back = nt > COS_EPS ? cs / st : 0.f;
    }
    for (int e = 0; e < p.E; ++e) {
      const float x = oka ? to_f32(A[ra * p.E + e]) : 0.f;
      const float y = okt ? to_f32(Tt[rt * p.E + e]) : 0.f;
      row[e] = from_f32<T>(okt ? gj * (x * inv - back * y) : 0.f);
    }
    coef[q] = make_float2(gj * inv, gj * cs);
  }
}

// generic path, second launch: one thread per (b, e): the anchor's row, its sum over j in order
template <typename T>
__global__ __launch_bounds__(256) void pair_score_bwd_anchor_elem_kernel(PairArgs p, T* __restrict__ gblock,
                                                                         const float2* __restrict__ coef) {
  const T* __restrict__ A = static_cast<const T*>(p.a_table);
  const T* __restrict__ Tt = static_cast<const T*>(p.t_table);
  const int64_t total = p.B * p.E;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const bool f32 = total < ((int64_t)1 << 32);
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += stride) {
    const int64_t b = udiv_fast(q, p.E, f32);
    const int e = (int)(q - b * p.E);
    const int64_t ra = rank_load_id(p.a_idx, p.idx64, b) + p.a_off;
    float acc = 0.f;
    if (ra >= 0 && ra < p.Va) {
      float gcos = 0.f;
      for (int j = 0; j < p.K1; ++j) {
        const int64_t rt = rank_load_id(p.t_idx, p.idx64, b * p.K1 + j) + p.t_off;
        const float2 c = coef[b * p.K1 + j];
        if (rt >= 0 && rt < p.Vt) acc += c.x * to_f32(Tt[rt * p.E + e]);
        gcos += c.y;
      }
      if (p.sim == SIM_COS) {
        float sa = 0.f;
        for (int k = 0; k < p.E; ++k) {
          const float x = to_f32(A[ra * p.E + k]);
          sa += x * x;
        }
        if (sqrtf(sa) > COS_EPS) acc -= gcos / sa * to_f32(A[ra * p.E + e]);
      }
    }
    gblock[b * (p.K1 + 1) * p.E + e] = from_f32<T>(acc);
  }
}

template <typename T>
static int pair_score_fwd_launch(const PairArgs& p, void* scores, bool out_f32, int32_t* err_flag, hipStream_t s) {
  const int lg = log2_lanes(p.E * (int)sizeof(T));
  if (lg >= 0 && aligned16(p.a_table) && aligned16(p.t_table)) {
    const int grid = stream_grid(p.B << lg, 256, 256 * 16);
    dispatch_lanes(lg, [&](auto lg_c) {
      hipLaunchKernelGGL((pair_score_group_kernel<T, decltype(lg_c)::value>), dim3(grid), dim3(256), 0, s, p, scores,
                         out_f32, err_flag);
    });
  } else {
    hipLaunchKernelGGL((pair_score_elem_kernel<T>), dim3(stream_grid(p.B * p.K1, 256, 256 * 16)), dim3(256), 0, s, p,
                       scores, out_f32, err_flag);
  }
  return check_launch("embed_pair_score_fwd");
}

static size_t pair_bwd_ws_bytes(int64_t B, int K, int E, int dtype) {
  if (log2_lanes(E * dtype_size(dtype)) >= 0) return 0;
  return (size_t)B * (size_t)(K + 1) * sizeof(float2);
}

template <typename T>
static int pair_score_bwd_launch(const PairArgs& p, const void* g, bool g_f32, void* gblock, void* ws, hipStream_t s) {
  const int lg = log2_lanes(p.E * (int)sizeof(T));
  if (lg >= 0) {
    const int grid = stream_grid(p.B << lg, 256, 256 * 16);
    dispatch_lanes(lg, [&](auto lg_c) {
      hipLaunchKernelGGL((pair_score_bwd_group_kernel<T, decltype(lg_c)::value>), dim3(grid), dim3(256), 0, s, p, g, g_f32,
                         (uint4*)gblock);
    });
  } else {
    hipLaunchKernelGGL((pair_score_bwd_elem_kernel<T>), dim3(stream_grid(p.B * p.K1, 256, 256 * 16)), dim3(256), 0, s, p,
                       g, g_f32, (T*)gblock, (float2*)ws);
    hipLaunchKernelGGL((pair_score_bwd_anchor_elem_kernel<T>), dim3(stream_grid(p.B * p.E, 256, 256 * 16)), dim3(256), 0,
                       s, p, (T*)gblock, (const float2*)ws);
  }
  return check_launch("embed_pair_score_bwd");
}

// ------------------------------------------------------------------------------------------------ ranking losses
constexpr int RANK_POINTWISE = 0, RANK_BPR = 1, RANK_HINGE = 2, RANK_ADAPTIVE = 3;
constexpr int RANK_SUM = 0, RANK_MEAN = 1, RANK_PER_SAMPLE = 2;
constexpr int RANK_BLOCK = 256;
constexpr int RANK_MAX_BLOCKS = 256;

struct RankArgs {
  const void* pos;
  const void* neg;
  const uint8_t* mask;      // torch.bool: one byte per sample, or NULL
  int64_t pos_stride, neg_stride, B;
  int K, kind, reduction;
  float margin;
  bool f32;
};

// softplus(-d) = -log(sigmoid(d)), finite for every d
__device__ __forceinline__ float rank_softplus_neg(float d) { return fmaxf(-d, 0.f) + log1pf(expf(-fabsf(d))); }

// what the sum is divided by: 1, the kept terms, or the kept samples
__device__ __forceinline__ float rank_denominator(int reduction, int kind, int K, float kept) {
  if (reduction == RANK_SUM) return 1.f;
  if (reduction == RANK_MEAN) return kind == RANK_ADAPTIVE ? kept : kept * (float)K;
  return kept;
}

__device__ __forceinline__ float rank_sample_terms(const RankArgs& a, int64_t b) {
  const float p = rank_load_val(a.pos, a.f32, b * a.pos_stride);
  float acc = 0.f;
  if (a.kind == RANK_ADAPTIVE) {
    float mx = -INFINITY;
    for (int k = 0; k < a.K; ++k) mx = fmaxf(mx, rank_load_val(a.neg, a.f32, b * a.neg_stride + k));
    return fmaxf(a.margin - p + mx, 0.f);
  }
  const float sp = 1.f - sigmoid_f(p);
  for (int k = 0; k < a.K; ++k) {
    const float n = rank_load_val(a.neg, a.f32, b * a.neg_stride + k);
    if (a.kind == RANK_POINTWISE) acc += sp + sigmoid_f(n);
    else if (a.kind == RANK_BPR) acc += rank_softplus_neg(p - n);
    else acc += fmaxf(a.margin - p + n, 0.f);
  }
  return acc;
}

// partial[blockIdx] = the block's sum of terms, partial[RANK_MAX_BLOCKS + blockIdx] = its kept samples
__global__ __launch_bounds__(RANK_BLOCK) void rank_loss_partial_kernel(RankArgs a, float* __restrict__ partial) {
  __shared__ float red[2][RANK_BLOCK / 64];
  float acc = 0.f, kept = 0.f;
  const int64_t stride = (int64_t)gridDim.x * RANK_BLOCK;
  for (int64_t b = (int64_t)blockIdx.x * RANK_BLOCK + threadIdx.x; b < a.B; b += stride) {
    if (a.mask != nullptr && a.mask[b] == 0) continue;
    acc += rank_sample_terms(a, b);
    kept += 1.f;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    kept += __shfl_xor(kept, o, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = acc;
    red[1][threadIdx.x >> 6] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = 0.f, c = 0.f;
#pragma unroll
    for (int w = 0; w < RANK_BLOCK / 64; ++w) {
      s += red[0][w];
      c += red[1][w];
    }
    partial[blockIdx.x] = s;
    partial[RANK_MAX_BLOCKS + blockIdx.x] = c;
  }
}

// one wave: the partials in a fixed order; *denom (may be NULL) receives what the sum was divided by
__global__ __launch_bounds__(64) void rank_loss_finish_kernel(const float* __restrict__ partial, int n, int reduction,
                                                              int kind, int K, float* __restrict__ loss,
                                                              float* __restrict__ denom) {
  float acc = 0.f, kept = 0.f;
  for (int i = threadIdx.x; i < n; i += 64) {
    acc += partial[i];
    kept += partial[RANK_MAX_BLOCKS + i];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    acc += __shfl_xor(acc, o, 64);
    kept += __shfl_xor(kept, o, 64);
  }
  if (threadIdx.x == 0) {
    const float den = rank_denominator(reduction, kind, K, kept);
    *loss = acc / den;      // no kept sample under a mean: 0 / 0 = NaN, as the reference's
    if (denom != nullptr) *denom = den;
  }
}

__global__ __launch_bounds__(256) void rank_loss_bwd_kernel(RankArgs a, const float* __restrict__ gout,
                                                            const float* __restrict__ denom, void* __restrict__ g_pos,
                                                            int64_t g_pos_stride, void* __restrict__ g_neg,
                                                            int64_t g_neg_stride) {
  const float den = denom != nullptr ? *denom : rank_denominator(a.reduction, a.kind, a.K, (float)a.B);
  const float g = (gout != nullptr ? *gout : 1.f) / den;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; b < a.B; b += stride) {
    const bool keep = a.mask == nullptr || a.mask[b] != 0;
    const float p = rank_load_val(a.pos, a.f32, b * a.pos_stride);
    float gp = 0.f;
    if (a.kind == RANK_ADAPTIVE) {
      float mx = -INFINITY;
      int at = 0;
      for (int k = 0; k < a.K; ++k) {      // the first of equal maxima takes the gradient
        const float n = rank_load_val(a.neg, a.f32, b * a.neg_stride + k);
        if (n > mx) { mx = n; at = k; }
      }
      const float on = keep && (a.margin - p + mx >= 0.f) ? g : 0.f;      // clamp's derivative at 0 is 1
      for (int k = 0; k < a.K; ++k) rank_store_val(g_neg, a.f32, b * g_neg_stride + k, k == at ? on : 0.f);
      gp = -on;
    } else {
      const float sp = sigmoid_f(p);
      for (int k = 0; k < a.K; ++k) {
        const float n = rank_load_val(a.neg, a.f32, b * a.neg_stride + k);
        float dp, dn;
        if (a.kind == RANK_POINTWISE) {
          const float sn = sigmoid_f(n);
          dp = -sp * (1.f - sp);
          dn = sn * (1.f - sn);
        } else if (a.kind == RANK_BPR) {
          dn = sigmoid_f(n - p);
          dp = -dn;
        } else {
          dn = a.margin - p + n >= 0.f ? 1.f : 0.f;      // as ATen's clamp(min=0) and margin_ranking_loss: 1 at the kink
          dp = -dn;
        }
        gp += dp;
        rank_store_val(g_neg, a.f32, b * g_neg_stride + k, keep ? dn * g : 0.f);
      }
      gp = keep ? gp * g : 0.f;
    }
    rank_store_val(g_pos, a.f32, b * g_pos_stride, gp);
  }
}

static int rank_check(const char* what, int32_t dtype, int64_t B, int32_t K, int32_t kind, int32_t reduction,
                      int64_t pos_stride, int64_t neg_stride) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(kind >= RANK_POINTWISE && kind <= RANK_ADAPTIVE, TRS_EINVAL,
              "%s: kind %d (0 = pointwise logistic, 1 = BPR, 2 = hinge, 3 = adaptive hinge)", what, kind);
  TRS_REQUIRE(reduction >= RANK_SUM && reduction <= RANK_PER_SAMPLE, TRS_EINVAL,
              "%s: reduction %d (0 = sum, 1 = mean, 2 = per kept sample)", what, reduction);
  TRS_REQUIRE(B >= 0 && K >= 1, TRS_EINVAL, "%s: bad size B=%lld K=%d (K >= 1)", what, (long long)B, K);
  TRS_REQUIRE(pos_stride >= 1 && neg_stride >= K, TRS_EINVAL, "%s: row stride %lld / %lld", what, (long long)pos_stride,
              (long long)neg_stride);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" int trs_pair_score_path(int32_t E, int32_t dtype) {
  if (E <= 0 || (dtype != TRS_F32 && dtype != TRS_BF16)) return -1;
  return log2_lanes(E * dtype_size(dtype)) >= 0 ? 1 : 0;
}

static int pair_args(const char* what, PairArgs* p, const void* a_table, int64_t Va, const void* a_idx, int64_t a_offset,
                     const void* t_table, int64_t Vt, const void* t_idx, int64_t t_offset, int32_t E, int32_t dtype,
                     int32_t idx_dtype, int64_t B, int32_t K, int32_t sim) {
  TRS_REQUIRE(a_table && a_idx && t_table && t_idx, TRS_EINVAL, "%s: NULL pointer", what);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EINVAL, "%s: idx dtype %d", what, idx_dtype);
  TRS_REQUIRE(sim == SIM_DOT || sim == SIM_COS, TRS_EINVAL, "%s: sim %d (0 = inner product, 1 = cosine)", what, sim);
  TRS_REQUIRE(Va > 0 && Vt > 0 && E > 0 && B >= 0 && K >= 0, TRS_EINVAL, "%s: bad size Va=%lld Vt=%lld E=%d B=%lld K=%d",
              what, (long long)Va, (long long)Vt, E, (long long)B, K);
  *p = PairArgs{a_table, a_idx, t_table, t_idx, a_offset, t_offset, Va, Vt, B, K + 1, E, sim, idx_dtype == TRS_I64};
  return TRS_OK;
}

extern "C" int trs_embed_pair_score_fwd(const void* a_table, int64_t Va, const void* a_idx, int64_t a_offset,
                                        const void* t_table, int64_t Vt, const void* t_idx, int64_t t_offset, int32_t E,
                                        int32_t dtype, int32_t idx_dtype, int64_t B, int32_t K, int32_t sim, void* scores,
                                        int32_t out_dtype, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  PairArgs p;
  const int rc = pair_args("embed_pair_score_fwd", &p, a_table, Va, a_idx, a_offset, t_table, Vt, t_idx, t_offset, E, dtype,
                           idx_dtype, B, K, sim);
  if (rc != TRS_OK) return rc;
  TRS_REQUIRE(scores, TRS_EINVAL, "embed_pair_score_fwd: NULL pointer");
  TRS_REQUIRE(out_dtype == TRS_F32 || out_dtype == dtype, TRS_EDTYPE,
              "embed_pair_score_fwd: out dtype %d (the table's, or fp32)", out_dtype);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32) return pair_score_fwd_launch<float>(p, scores, true, err_flag, s);
  return pair_score_fwd_launch<bf16_t>(p, scores, out_dtype == TRS_F32, err_flag, s);
}

extern "C" size_t trs_pair_score_bwd_workspace_bytes(int64_t B, int32_t K, int32_t E, int32_t dtype) {
  if (B <= 0 || K < 0 || E <= 0 || (dtype != TRS_F32 && dtype != TRS_BF16)) return 0;
  return pair_bwd_ws_bytes(B, K, E, dtype);
}

extern "C" int trs_embed_pair_score_bwd(const void* a_table, int64_t Va, const void* a_idx, int64_t a_offset,
                                        const void* t_table, int64_t Vt, const void* t_idx, int64_t t_offset, int32_t E,
                                        int32_t dtype, int32_t idx_dtype, int64_t B, int32_t K, int32_t sim,
                                        const void* g_scores, int32_t g_dtype, void* g_block, void* workspace,
                                        size_t ws_bytes, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  PairArgs p;
  const int rc = pair_args("embed_pair_score_bwd", &p, a_table, Va, a_idx, a_offset, t_table, Vt, t_idx, t_offset, E, dtype,
                           idx_dtype, B, K, sim);
  if (rc != TRS_OK) return rc;
  TRS_REQUIRE(g_scores && g_block, TRS_EINVAL, "embed_pair_score_bwd: NULL pointer");
  TRS_REQUIRE(g_dtype == TRS_F32 || g_dtype == dtype, TRS_EDTYPE,
              "embed_pair_score_bwd: gradient dtype %d (the table's, or fp32)", g_dtype);
  const size_t need = pair_bwd_ws_bytes(B, K, E, dtype);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need), TRS_EWORKSPACE,
              "embed_pair_score_bwd: workspace %zu < %zu", ws_bytes, need);
  // the lane-group kernels move whole 16-byte vectors
  TRS_REQUIRE(need != 0 || (aligned16(a_table) && aligned16(t_table) && aligned16(g_block)), TRS_EALIGN,
              "embed_pair_score_bwd: tables and gradient block must be 16-byte aligned for E=%d", E);
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32) return pair_score_bwd_launch<float>(p, g_scores, true, g_block, workspace, s);
  return pair_score_bwd_launch<bf16_t>(p, g_scores, g_dtype == TRS_F32, g_block, workspace, s);
}

extern "C" size_t trs_rank_loss_workspace_bytes(int64_t B) { return (size_t)2 * RANK_MAX_BLOCKS * sizeof(float); }

extern "C" int trs_rank_loss_fwd(const void* pos, int64_t pos_stride, const void* neg, int64_t neg_stride, int32_t dtype,
                                 const void* mask, int64_t B, int32_t K, int32_t kind, float margin, int32_t reduction,
                                 float* loss, float* denom, void* workspace, size_t ws_bytes, trs_stream_t stream) {
  const int rc = rank_check("rank_loss_fwd", dtype, B, K, kind, reduction, pos_stride, neg_stride);
  if (rc != TRS_OK) return rc;
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(pos && neg && loss && workspace, TRS_EINVAL, "rank_loss_fwd: NULL pointer");
  TRS_REQUIRE(ws_bytes >= trs_rank_loss_workspace_bytes(B), TRS_EWORKSPACE, "rank_loss_fwd: workspace too small");
  const RankArgs a{pos, neg, (const uint8_t*)mask, pos_stride, neg_stride, B, K, kind, reduction, margin, dtype == TRS_F32};
  hipStream_t s = (hipStream_t)stream;
  const int blocks = (int)std::min<int64_t>(RANK_MAX_BLOCKS, (B + RANK_BLOCK - 1) / RANK_BLOCK);
  hipLaunchKernelGGL(rank_loss_partial_kernel, dim3(blocks), dim3(RANK_BLOCK), 0, s, a, (float*)workspace);
  hipLaunchKernelGGL(rank_loss_finish_kernel, dim3(1), dim3(64), 0, s, (const float*)workspace, blocks, reduction, kind, K,
                     loss, denom);
  return check_launch("rank_loss_fwd");
}

extern "C" int trs_rank_loss_bwd(const void* pos, int64_t pos_stride, const void* neg, int64_t neg_stride, int32_t dtype,
                                 const void* mask, int64_t B, int32_t K, int32_t kind, float margin, int32_t reduction,
                                 const float* gout, const float* denom, void* g_pos, int64_t g_pos_stride, void* g_neg,
                                 int64_t g_neg_stride, trs_stream_t stream) {
  const int rc = rank_check("rank_loss_bwd", dtype, B, K, kind, reduction, pos_stride, neg_stride);
  if (rc != TRS_OK) return rc;
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(pos && neg && g_pos && g_neg, TRS_EINVAL, "rank_loss_bwd: NULL pointer");
  TRS_REQUIRE(g_pos_stride >= 1 && g_neg_stride >= K, TRS_EINVAL, "rank_loss_bwd: gradient row stride %lld / %lld",
              (long long)g_pos_stride, (long long)g_neg_stride);
  TRS_REQUIRE(mask == nullptr || reduction == RANK_SUM || denom != nullptr, TRS_EINVAL,
              "rank_loss_bwd: a masked mean needs the forward's denominator");
  const RankArgs a{pos, neg, (const uint8_t*)mask, pos_stride, neg_stride, B, K, kind, reduction, margin, dtype == TRS_F32};
  hipLaunchKernelGGL(rank_loss_bwd_kernel, dim3(stream_grid(B, 256, 1024)), dim3(256), 0, (hipStream_t)stream, a, gout,
                     denom, g_pos, g_pos_stride, g_neg, g_neg_stride);
  return check_launch("rank_loss_bwd");
}
