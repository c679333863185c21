// Attention pooling of a bag of ids: self-attention over the looked-up rows followed by a sum / mean over the list, the
// use_attn branch of the reference's ListIndicesEmbedding (inputs/base/list_indices_emb.py:124-152: aten::embedding ->
// nn.MultiheadAttention -> pooling).  The pooling collapses most of the attention algebra.  Per sample and head
// (d = E / H, X the (L, E) looked-up rows, c = 1 / L for the mean and 1 for the sum):
//   Q = X Wq^T + bq,  K = X Wk^T + bk,  P = softmax_rows(Q_h K_h^T / sqrt(d))
//   pbar_h[m] = c sum_l P[l, m]                    xt_h = sum_m pbar_h[m] X[m, :]        <- what the forward emits, (B, H, E)
// and the layer output is concat_h(xt_h Wv_h^T + c' bv_h) Wout^T + c' bout (c' = 1 or L), two small GEMMs on B*H and B
// rows that the caller runs.  Neither the (B, L, E) block nor Q, K or the scores ever reach HBM in the forward.
//
// One workgroup of 256 threads owns one sample at a time (persistent: b = blockIdx.x, += gridDim.x); X, Q|K and one head's
// (L, L) scores live in LDS as fp32 with odd row strides.  Every product is one routine, ap_gemm, over strided operands:
//   vector path (1): four outputs per thread, fp32 FMA -- exact fp32, any L <= 64, E <= 128, E % H == 0;
//   MFMA path   (2): bf16 tables with E % 16 == 0 and d % 16 == 0: v_mfma_f32_16x16x32_bf16, a wave per 16x16 output tile,
//                    operands rounded to bf16 as they are read (X and W are bf16 already; Q, K, dS, dQ, dK take one
//                    rounding, as they would in ATen's bf16 module), fp32 accumulation, edges zero-filled.
// Wqk is read from global memory (16 KB at E = 64 in bf16: L1 / L2 resident) instead of being staged in LDS, which keeps
// two to four workgroups on a CU.
//
// Backward: Q, K and P are recomputed from the table rows; with g = d(xt) (B, H, E):
//   r[m] = X[m] . g_h      dS[l, m] = c P[l, m] (r[m] - sum_m' P[l, m'] r[m'])
//   dQ_h = dS K_h / sqrt(d)     dK_h = dS^T Q_h / sqrt(d)
//   dX = dQ Wq + dK Wk + sum_h pbar_h[m] g_h        dWq = dQ^T X   dWk = dK^T X   dbq = sum_l dQ   dbk = sum_m dK
// dK_h overwrites K_h and dX the Q half of the Q|K buffer once they are dead, so the sample needs 4 L E + L^2 floats of
// LDS.  The weight gradient is accumulated in fp32 in the workgroup's OWN (2E, E) slab of `dw_part` by plain
// read-modify-writes (the slabs of the resident workgroups stay in L2); samples are dealt to workgroups statically, the
// caller reduces the slabs in a fixed order, and there are no atomics: two calls give the same bits.  dX (B, L, E) is the
// one block the backward forms -- the per-position gradients differ, so there is nothing to broadcast -- and goes to the
// row-bucket walk (trs_scatter_rows*).
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <utility>

#include "trs_common.hpp"

namespace trs {

constexpr int AP_SUM = 0, AP_MEAN = 1;
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

// the sample's rows into X (fp32); an id outside [0, V) reads as a zero row and raises the flag
template <typename T, typename IdxT>
__device__ __forceinline__ void ap_gather(float* X, int sx, const T* __restrict__ table, const IdxT* __restrict__ ids,
                                          int L, int E, int64_t V, int32_t* __restrict__ err_flag, bool vec) {
  if constexpr (sizeof(T) == 2) {
    if (vec) {      // E % 8 == 0, 16-byte aligned table: a thread moves 8 columns of a row
      const int cpr = E >> 3;
      for (int c = threadIdx.x; c < L * cpr; c += AP_THREADS) {
        const int l = c / cpr, part = c - l * cpr;
        const int64_t r = (int64_t)ids[l];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (r < 0 || r >= V) {
          if (err_flag != nullptr && part == 0) *err_flag = 1;
        } else {
          v = *reinterpret_cast<const uint4*>(table + r * E + part * 8);
        }
        float f[8];
        Vec16<bf16_t>::unpack(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) X[l * sx + part * 8 + j] = f[j];
      }
      return;
    }
  }
  for (int i = threadIdx.x; i < L * E; i += AP_THREADS) {
    const int l = i / E, e = i - l * E;
    const int64_t r = (int64_t)ids[l];
    float v = 0.f;
    if (r < 0 || r >= V) {
      if (err_flag != nullptr && e == 0) *err_flag = 1;
    } else {
      v = to_f32(table[r * E + e]);
    }
    X[l * sx + e] = v;
  }
}

// S <- P = softmax_rows(S): 4 adjacent lanes per row (rows >= L idle but keep the shuffles whole)
__device__ __forceinline__ float ap_quad_sum(float v) {
  v += __shfl_xor(v, 1, 64);
  v += __shfl_xor(v, 2, 64);
  return v;
}
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
  sum = ap_quad_sum(sum);
  if (live) {
    const float inv = 1.f / sum;
    for (int c = sub; c < L; c += 4) p[c] *= inv;
  }
}

// scores and probabilities of head h into S, pbar_h[m] = cscale * sum_l P[l, m]; leaves the block synchronised
template <bool MF>
__device__ __forceinline__ void ap_head_probs(float* S, int ss, const float* QK, int sqk, int L, int E, int d, int h,
                                              float alpha, float cscale, float* pbar_h) {
  ap_gemm<MF>(S, ss, 1, false, QK + h * d, sqk, 1, QK + E + h * d, 1, sqk, L, L, d, alpha, (const float*)nullptr);
  __syncthreads();
  ap_softmax_rows(S, ss, L);
  __syncthreads();
  for (int m = threadIdx.x; m < L; m += AP_THREADS) {
    float s = 0.f;
    for (int l = 0; l < L; ++l) s += S[l * ss + m];
    pbar_h[m] = cscale * s;
  }
  __syncthreads();
}

// [Q | K] = X W^T + b
template <bool MF, typename T>
__device__ __forceinline__ void ap_project(float* QK, int sqk, const float* X, int sx, const T* __restrict__ W,
                                           const T* __restrict__ bqk, int L, int E, bool vec) {
  if constexpr (MF) {
    if (vec) {
      ap_gemm<true, true>(QK, sqk, 1, false, X, sx, 1, W, 1, E, L, 2 * E, E, 1.f, bqk);
      return;
    }
  }
  ap_gemm<MF, false, true>(QK, sqk, 1, false, X, sx, 1, W, 1, E, L, 2 * E, E, 1.f, bqk);
}

template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_fwd_kernel(const T* __restrict__ table,
                                                                   const IdxT* __restrict__ idx, int64_t B, int L, int E,
                                                                   int64_t V, const T* __restrict__ W,
                                                                   const T* __restrict__ bqk, int H, float cscale,
                                                                   T* __restrict__ out, int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int d = E / H, sx = E + 1, sqk = 2 * E + 1, ss = L + 1;
  float* X = ap_smem;
  float* QK = X + L * sx;
  float* S = QK + L * sqk;
  float* pbar = S + L * ss;          // (H, L)
  const float alpha = 1.f / sqrtf((float)d);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    ap_gather<T, IdxT>(X, sx, table, idx + b * L, L, E, V, err_flag, vec);
    __syncthreads();
    ap_project<MF, T>(QK, sqk, X, sx, W, bqk, L, E, vec);
    __syncthreads();
    for (int h = 0; h < H; ++h) ap_head_probs<MF>(S, ss, QK, sqk, L, E, d, h, alpha, cscale, pbar + h * L);
    for (int o = threadIdx.x; o < H * E; o += AP_THREADS) {
      const int h = o / E, e = o - h * E;
      float s = 0.f;
      for (int m = 0; m < L; ++m) s = fmaf(pbar[h * L + m], X[m * sx + e], s);
      out[b * H * E + o] = from_f32<T>(s);
    }
    __syncthreads();
  }
}

template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_bwd_kernel(
    const T* __restrict__ table, const IdxT* __restrict__ idx, int64_t B, int L, int E, int64_t V, const T* __restrict__ W,
    const T* __restrict__ bqk, int H, float cscale, const T* __restrict__ gout, T* __restrict__ dx,
    float* __restrict__ dw_part, float* __restrict__ db_part, float* pbar_ws, int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int d = E / H, sx = E + 1, sqk = 2 * E + 1, ss = L + 1, sdq = E + 1;
  float* X = ap_smem;
  float* QK = X + L * sx;
  float* S = QK + L * sqk;
  float* dQ = S + L * ss;
  float* rv = dQ + L * sdq;          // (L)
  // (H, L): in LDS unless H is so large that it does not fit beside the rest (the workgroup's slice of pbar_ws then)
  float* pbar = pbar_ws != nullptr ? pbar_ws + (size_t)blockIdx.x * H * L : rv + L;
  const float alpha = 1.f / sqrtf((float)d);
  float* dW = dw_part + (size_t)blockIdx.x * 2 * E * E;
  float* db = db_part + (size_t)blockIdx.x * 2 * E;
  for (int i = threadIdx.x; i < 2 * E * E; i += AP_THREADS) dW[i] = 0.f;
  for (int i = threadIdx.x; i < 2 * E; i += AP_THREADS) db[i] = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const T* g = gout + b * H * E;
    ap_gather<T, IdxT>(X, sx, table, idx + b * L, L, E, V, err_flag, vec);
    __syncthreads();
    ap_project<MF, T>(QK, sqk, X, sx, W, bqk, L, E, vec);
    __syncthreads();
    for (int h = 0; h < H; ++h) {
      {   // r[m] = X[m] . g_h, 4 lanes per row (S is not touched: no barrier needed before the scores)
        const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
        float s = 0.f;
        if (row < L)
          for (int e = sub; e < E; e += 4) s = fmaf(X[row * sx + e], to_f32(g[h * E + e]), s);
        s = ap_quad_sum(s);
        if (row < L && sub == 0) rv[row] = s;
      }
      ap_head_probs<MF>(S, ss, QK, sqk, L, E, d, h, alpha, cscale, pbar + h * L);
      {   // S <- dS
        const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
        float* p = S + row * ss;
        float t = 0.f;
        if (row < L)
          for (int c = sub; c < L; c += 4) t = fmaf(p[c], rv[c], t);
        t = ap_quad_sum(t);
        if (row < L)
          for (int c = sub; c < L; c += 4) p[c] = cscale * p[c] * (rv[c] - t);
      }
      __syncthreads();
      // dQ_h = alpha dS K_h
      ap_gemm<MF>(dQ + h * d, sdq, 1, false, S, ss, 1, QK + E + h * d, sqk, 1, L, d, L, alpha, (const float*)nullptr);
      __syncthreads();
      // K_h <- dK_h = alpha dS^T Q_h
      ap_gemm<MF>(QK + E + h * d, sqk, 1, false, S, 1, ss, QK + h * d, sqk, 1, L, d, L, alpha, (const float*)nullptr);
      __syncthreads();
    }
    for (int j = threadIdx.x; j < 2 * E; j += AP_THREADS) {
      float s = 0.f;
      for (int l = 0; l < L; ++l) s += j < E ? dQ[l * sdq + j] : QK[l * sqk + j];
      db[j] += s;
    }
    // dWq += dQ^T X, dWk += dK^T X
    ap_gemm<MF>(dW, E, 1, true, dQ, 1, sdq, X, sx, 1, E, E, L, 1.f, (const float*)nullptr);
    ap_gemm<MF>(dW + E * E, E, 1, true, QK + E, 1, sqk, X, sx, 1, E, E, L, 1.f, (const float*)nullptr);
    // Q half <- dQ Wq + dK Wk
    ap_gemm<MF>(QK, sqk, 1, false, dQ, sdq, 1, W, E, 1, L, E, E, 1.f, (const float*)nullptr);
    __syncthreads();
    ap_gemm<MF>(QK, sqk, 1, true, QK + E, sqk, 1, W + E * E, E, 1, L, E, E, 1.f, (const float*)nullptr);
    __syncthreads();
    for (int i = threadIdx.x; i < L * E; i += AP_THREADS) {
      const int m = i / E, e = i - m * E;
      float v = QK[m * sqk + e];
      for (int h = 0; h < H; ++h) v = fmaf(pbar[h * L + m], to_f32(g[h * E + e]), v);
      dx[(b * L + m) * E + e] = from_f32<T>(v);
    }
    __syncthreads();
  }
}

static int ap_path(int L, int E, int H, int dtype) {
  if (dtype != TRS_F32 && dtype != TRS_BF16) return 0;
  if (L < 1 || L > AP_MAX_L || E < 1 || E > AP_MAX_E || H < 1 || E % H != 0) return 0;
  if (dtype == TRS_BF16 && E % 16 == 0 && (E / H) % 16 == 0) return 2;
  return 1;
}

static size_t ap_fwd_lds(int L, int E, int H) {
  return sizeof(float) * ((size_t)L * (E + 1) + (size_t)L * (2 * E + 1) + (size_t)L * (L + 1) + (size_t)H * L);
}
static size_t ap_bwd_lds_base(int L, int E) {
  return sizeof(float) * ((size_t)2 * L * (E + 1) + (size_t)L * (2 * E + 1) + (size_t)L * (L + 1) + (size_t)L);
}
static bool ap_bwd_pbar_in_lds(int L, int E, int H) {
  return ap_bwd_lds_base(L, E) + sizeof(float) * (size_t)H * L <= AP_MAX_LDS;
}
static size_t ap_bwd_lds(int L, int E, int H) {
  return ap_bwd_lds_base(L, E) + (ap_bwd_pbar_in_lds(L, E, H) ? sizeof(float) * (size_t)H * L : 0);
}

template <typename T, bool MF>
static const void* ap_kernel_of(bool backward, bool i64) {
  if (backward)
    return i64 ? (const void*)attn_pool_bwd_kernel<T, int64_t, MF> : (const void*)attn_pool_bwd_kernel<T, int32_t, MF>;
  return i64 ? (const void*)attn_pool_fwd_kernel<T, int64_t, MF> : (const void*)attn_pool_fwd_kernel<T, int32_t, MF>;
}
static const void* ap_kernel(int path, int dtype, bool backward, bool i64) {
  if (dtype == TRS_F32) return ap_kernel_of<float, false>(backward, i64);
  return path == 2 ? ap_kernel_of<bf16_t, true>(backward, i64) : ap_kernel_of<bf16_t, false>(backward, i64);
}

// persistent grid: the workgroups that are resident at once, at most one per sample
// (asked of the runtime once per kernel and LDS size: the warm-up of a graph capture has then made every query)
static int ap_resident(const void* kern, size_t lds) {
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
static int ap_blocks(const void* kern, size_t lds, int64_t B) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(B, ap_resident(kern, lds)));
}

static int ap_check(const char* what, int64_t V, int E, int dtype, int idx_dtype, int64_t B, int L, int H, int mode) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EDTYPE, "%s: idx dtype %d", what, idx_dtype);
  TRS_REQUIRE(mode == AP_SUM || mode == AP_MEAN, TRS_EDTYPE, "%s: mode %d (0 = sum, 1 = mean)", what, mode);
  TRS_REQUIRE(V > 0 && B >= 0, TRS_EINVAL, "%s: bad size V=%lld B=%lld", what, (long long)V, (long long)B);
  TRS_REQUIRE(ap_path(L, E, H, dtype) != 0, TRS_EDTYPE,
              "%s: unsupported shape L=%d E=%d H=%d (1 <= L <= %d, E <= %d, E %% H == 0)", what, L, E, H, AP_MAX_L,
              AP_MAX_E);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" int trs_attn_pool_path(int32_t L, int32_t E, int32_t H, int32_t dtype) { return ap_path(L, E, H, dtype); }

extern "C" int trs_attn_pool_blocks(int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, int32_t backward) {
  const int path = ap_path(L, E, H, dtype);
  if (path == 0 || B < 1) return 0;
  return ap_blocks(ap_kernel(path, dtype, backward != 0, true), backward ? ap_bwd_lds(L, E, H) : ap_fwd_lds(L, E, H), B);
}

extern "C" size_t trs_attn_pool_bwd_workspace_bytes(int32_t blocks, int32_t L, int32_t E, int32_t H) {
  if (blocks < 1 || L < 1 || E < 1 || H < 1 || ap_bwd_pbar_in_lds(L, E, H)) return 0;
  return sizeof(float) * (size_t)blocks * H * L;
}

extern "C" int trs_attn_pool_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx,
                                 int32_t idx_dtype, int64_t B, int32_t L, const void* w_qk, const void* b_qk, int32_t H,
                                 int32_t mode, void* out, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(table && idx && w_qk && out, TRS_EINVAL, "attn_pool_fwd: NULL pointer");
  if (int rc = ap_check("attn_pool_fwd", V, E, dtype, idx_dtype, B, L, H, mode)) return rc;
  const int path = ap_path(L, E, H, dtype);
  const bool i64 = idx_dtype == TRS_I64;
  const size_t lds = ap_fwd_lds(L, E, H);
  const int grid = ap_blocks(ap_kernel(path, dtype, false, i64), lds, B);
  const float cscale = mode == AP_MEAN ? 1.f / (float)L : 1.f;
  const bool vec = path == 2 && aligned16(table) && aligned16(w_qk);      // 16-byte loads of table and weight rows
  hipStream_t s = (hipStream_t)stream;
#define TRS_AP(T, I, MF)                                                                                              \
  hipLaunchKernelGGL((attn_pool_fwd_kernel<T, I, MF>), dim3(grid), dim3(AP_THREADS), lds, s, (const T*)table,          \
                     (const I*)idx, B, L, E, V, (const T*)w_qk, (const T*)b_qk, H, cscale, (T*)out, err_flag, vec)
  if (dtype == TRS_F32) {
    if (i64) TRS_AP(float, int64_t, false);
    else TRS_AP(float, int32_t, false);
  } else if (path == 2) {
    if (i64) TRS_AP(bf16_t, int64_t, true);
    else TRS_AP(bf16_t, int32_t, true);
  } else {
    if (i64) TRS_AP(bf16_t, int64_t, false);
    else TRS_AP(bf16_t, int32_t, false);
  }
#undef TRS_AP
  return check_launch("attn_pool_fwd");
}

extern "C" int trs_attn_pool_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx,
                                 int32_t idx_dtype, int64_t B, int32_t L, const void* w_qk, const void* b_qk, int32_t H,
                                 int32_t mode, const void* gout, void* dx, float* dw_part, float* db_part, int32_t blocks,
                                 void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(table && idx && w_qk && gout && dx && dw_part && db_part, TRS_EINVAL, "attn_pool_bwd: NULL pointer");
  if (int rc = ap_check("attn_pool_bwd", V, E, dtype, idx_dtype, B, L, H, mode)) return rc;
  TRS_REQUIRE(blocks >= 1 && blocks <= B, TRS_EINVAL, "attn_pool_bwd: blocks=%d outside [1, B]", blocks);
  const size_t need = trs_attn_pool_bwd_workspace_bytes(blocks, L, E, H);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need), TRS_EWORKSPACE,
              "attn_pool_bwd: workspace %zu < %zu", ws_bytes, need);
  const int path = ap_path(L, E, H, dtype);
  const bool i64 = idx_dtype == TRS_I64;
  const size_t lds = ap_bwd_lds(L, E, H);
  (void)ap_resident(ap_kernel(path, dtype, true, i64), lds);      // raises the kernel's LDS limit where needed
  float* pbar_ws = need ? (float*)workspace : nullptr;
  const float cscale = mode == AP_MEAN ? 1.f / (float)L : 1.f;
  const bool vec = path == 2 && aligned16(table) && aligned16(w_qk);      // 16-byte loads of table and weight rows
  hipStream_t s = (hipStream_t)stream;
#define TRS_AP(T, I, MF)                                                                                               \
  hipLaunchKernelGGL((attn_pool_bwd_kernel<T, I, MF>), dim3(blocks), dim3(AP_THREADS), lds, s, (const T*)table,         \
                     (const I*)idx, B, L, E, V, (const T*)w_qk, (const T*)b_qk, H, cscale, (const T*)gout, (T*)dx,      \
                     dw_part, db_part, pbar_ws, err_flag, vec)
  if (dtype == TRS_F32) {
    if (i64) TRS_AP(float, int64_t, false);
    else TRS_AP(float, int32_t, false);
  } else if (path == 2) {
    if (i64) TRS_AP(bf16_t, int64_t, true);
    else TRS_AP(bf16_t, int32_t, true);
  } else {
    if (i64) TRS_AP(bf16_t, int64_t, false);
    else TRS_AP(bf16_t, int32_t, false);
  }
#undef TRS_AP
  return check_launch("attn_pool_bwd");
}
