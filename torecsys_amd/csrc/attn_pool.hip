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
//
// Ragged bags (trs_attn_pool_ragged_*): one flat id vector plus offsets, a bag attends to its own live ids only.  Sibling
// kernels that call the same per-sample bodies (ap_fwd_sample / ap_bwd_sample) with L_b, the number of ids the bag takes,
// for L; how the rows are found, the LDS layout and the flat dX are described at the kernels below.
#include "attn_common.hpp"
#include "bag_common.hpp"

namespace trs {

constexpr int AP_SUM = 0, AP_MEAN = 1;

// the sample's rows into X (fp32), id_of(l) the id of list position l; an id outside [0, V) reads as a zero row and raises
// the flag
template <typename T, typename IdF>
__device__ __forceinline__ void ap_gather(float* X, int sx, const T* __restrict__ table, IdF id_of, int L, int E,
                                          int64_t V, int32_t* __restrict__ err_flag, bool vec) {
  if constexpr (sizeof(T) == 2) {
    if (vec) {      // E % 8 == 0, 16-byte aligned table: a thread moves 8 columns of a row
      const int cpr = E >> 3;
      for (int c = threadIdx.x; c < L * cpr; c += AP_THREADS) {
        const int l = c / cpr, part = c - l * cpr;
        const int64_t r = (int64_t)id_of(l);
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
    const int64_t r = (int64_t)id_of(l);
    float v = 0.f;
    if (r < 0 || r >= V) {
      if (err_flag != nullptr && e == 0) *err_flag = 1;
    } else {
      v = to_f32(table[r * E + e]);
    }
    X[l * sx + e] = v;
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

// one sample of the forward: L rows (ids id_of(0 .. L-1)) to the (H, E) block at out_b; leaves the block synchronised
template <bool MF, typename T, typename IdF>
__device__ __forceinline__ void ap_fwd_sample(float* X, int sx, float* QK, int sqk, float* S, int ss, float* pbar,
                                              const T* __restrict__ table, IdF id_of, int L, int E, int64_t V,
                                              const T* __restrict__ W, const T* __restrict__ bqk, int H, float cscale,
                                              T* __restrict__ out_b, int32_t* __restrict__ err_flag, bool vec) {
  const int d = E / H;
  const float alpha = 1.f / sqrtf((float)d);
  ap_gather<T>(X, sx, table, id_of, L, E, V, err_flag, vec);
  __syncthreads();
  ap_project<MF, T>(QK, sqk, X, sx, W, bqk, L, E, vec);
  __syncthreads();
  for (int h = 0; h < H; ++h) ap_head_probs<MF>(S, ss, QK, sqk, L, E, d, h, alpha, cscale, pbar + h * L);
  for (int o = threadIdx.x; o < H * E; o += AP_THREADS) {
    const int h = o / E, e = o - h * E;
    float s = 0.f;
    for (int m = 0; m < L; ++m) s = fmaf(pbar[h * L + m], X[m * sx + e], s);
    out_b[o] = from_f32<T>(s);
  }
  __syncthreads();
}

// one sample of the backward: g the (H, E) gradient of its block, dx_row(m) the row of dx that list position m owns; adds
// to the workgroup's dW / db slabs; leaves the block synchronised
template <bool MF, typename T, typename IdF, typename RowF>
__device__ __forceinline__ void ap_bwd_sample(float* X, int sx, float* QK, int sqk, float* S, int ss, float* dQ, int sdq,
                                              float* rv, float* pbar, const T* __restrict__ table, IdF id_of, int L,
                                              int E, int64_t V, const T* __restrict__ W, const T* __restrict__ bqk,
                                              int H, float cscale, const T* __restrict__ g, T* __restrict__ dx,
                                              RowF dx_row, float* dW, float* db, int32_t* __restrict__ err_flag,
                                              bool vec) {
  const int d = E / H;
  const float alpha = 1.f / sqrtf((float)d);
  ap_gather<T>(X, sx, table, id_of, L, E, V, err_flag, vec);
  __syncthreads();
  ap_project<MF, T>(QK, sqk, X, sx, W, bqk, L, E, vec);
  __syncthreads();
  for (int h = 0; h < H; ++h) {
    {   // r[m] = X[m] . g_h, 4 lanes per row (S is not touched: no barrier needed before the scores)
      const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
      float s = 0.f;
      if (row < L)
        for (int e = sub; e < E; e += 4) s = fmaf(X[row * sx + e], to_f32(g[h * E + e]), s);
      s = group_sum_up<4>(s);
      if (row < L && sub == 0) rv[row] = s;
    }
    ap_head_probs<MF>(S, ss, QK, sqk, L, E, d, h, alpha, cscale, pbar + h * L);
    {   // S <- dS
      const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
      float* p = S + row * ss;
      float t = 0.f;
      if (row < L)
        for (int c = sub; c < L; c += 4) t = fmaf(p[c], rv[c], t);
      t = group_sum_up<4>(t);
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
    dx[dx_row(m) * E + e] = from_f32<T>(v);
  }
  __syncthreads();
}

template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_fwd_kernel(const T* __restrict__ table,
                                                                   const IdxT* __restrict__ idx, int64_t B, int L, int E,
                                                                   int64_t V, const T* __restrict__ W,
                                                                   const T* __restrict__ bqk, int H, float cscale,
                                                                   T* __restrict__ out, int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int sx = E + 1, sqk = 2 * E + 1, ss = L + 1;
  float* X = ap_smem;
  float* QK = X + L * sx;
  float* S = QK + L * sqk;
  float* pbar = S + L * ss;          // (H, L)
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const IdxT* ids = idx + b * L;
    ap_fwd_sample<MF, T>(X, sx, QK, sqk, S, ss, pbar, table, [ids](int l) { return ids[l]; }, L, E, V, W, bqk, H, cscale,
                         out + b * H * E, err_flag, vec);
  }
}

template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_bwd_kernel(
    const T* __restrict__ table, const IdxT* __restrict__ idx, int64_t B, int L, int E, int64_t V, const T* __restrict__ W,
    const T* __restrict__ bqk, int H, float cscale, const T* __restrict__ gout, T* __restrict__ dx,
    float* __restrict__ dw_part, float* __restrict__ db_part, float* pbar_ws, int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int sx = E + 1, sqk = 2 * E + 1, ss = L + 1, sdq = E + 1;
  float* X = ap_smem;
  float* QK = X + L * sx;
  float* S = QK + L * sqk;
  float* dQ = S + L * ss;
  float* rv = dQ + L * sdq;          // (L)
  // (H, L): in LDS unless H is so large that it does not fit beside the rest (the workgroup's slice of pbar_ws then)
  float* pbar = pbar_ws != nullptr ? pbar_ws + (size_t)blockIdx.x * H * L : rv + L;
  float* dW = dw_part + (size_t)blockIdx.x * 2 * E * E;
  float* db = db_part + (size_t)blockIdx.x * 2 * E;
  for (int i = threadIdx.x; i < 2 * E * E; i += AP_THREADS) dW[i] = 0.f;
  for (int i = threadIdx.x; i < 2 * E; i += AP_THREADS) db[i] = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const IdxT* ids = idx + b * L;
    ap_bwd_sample<MF, T>(X, sx, QK, sqk, S, ss, dQ, sdq, rv, pbar, table, [ids](int l) { return ids[l]; }, L, E, V, W, bqk,
                         H, cscale, gout + b * H * E, dx, [b, L](int m) { return b * L + m; }, dW, db, err_flag, vec);
  }
}

// ---- ragged bags: bag b is ids[beg_b, end_b) read from the offsets, the ids equal to `pad` (>= 0) left out ----------------
// The LDS layout is the padded one at L = max_len plus max_len + 4 ints; the rows a sample takes (L_b <= max_len) are only a
// workgroup-uniform loop bound, and every ap_gemm edge is zero-filled by predicate, so a short bag never reads the rows a
// longer one left behind.

// lpos[0 .. L_b) = the flat positions of the first max_len live ids of bag b in list order (wtot: 4 ints of scratch); returns
// L_b.  The bag is scanned 256 positions at a time until it ends or max_len + 1 live ids were seen; more live ids than
// max_len raise the flag.  Called by all 256 threads, the result is uniform; leaves the block synchronised.
template <typename IdxT>
__device__ __forceinline__ int ap_live_ids(const IdxT* __restrict__ ids, int64_t n, const void* __restrict__ offsets,
                                           bool off64, int64_t n_off, int64_t b, int64_t pad, int max_len, int* lpos,
                                           int* wtot, int32_t* __restrict__ err_flag) {
  int64_t beg, end;
  bag_ragged_bounds(offsets, off64, n_off, b, n, threadIdx.x == 0 ? err_flag : nullptr, &beg, &end);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int taken = 0;
  for (int64_t q0 = beg; q0 < end && taken <= max_len; q0 += AP_THREADS) {
    const int64_t q = q0 + threadIdx.x;
    const bool live = q < end && !(pad >= 0 && (int64_t)ids[q] == pad);
    const unsigned long long mask = __ballot(live);
    if (lane == 0) wtot[wave] = __popcll(mask);
    __syncthreads();
    int rank = taken + __popcll(mask & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; ++w) rank += wtot[w];
    if (live && rank < max_len) lpos[rank] = (int)q;      // q < n < 2^31 - 1
    taken += wtot[0] + wtot[1] + wtot[2] + wtot[3];
    __syncthreads();
  }
  if (taken > max_len) {
    if (err_flag != nullptr && threadIdx.x == 0) *err_flag = 1;
    taken = max_len;
  }
  return taken;
}

template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_ragged_fwd_kernel(
    const T* __restrict__ table, const IdxT* __restrict__ ids, int64_t n, const void* __restrict__ offsets, bool off64,
    int64_t n_off, int64_t B, int max_len, int64_t pad, int E, int64_t V, const T* __restrict__ W,
    const T* __restrict__ bqk, int H, int mode, T* __restrict__ out, float* __restrict__ cnt,
    int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int sx = E + 1, sqk = 2 * E + 1, ss = max_len | 1;
  float* X = ap_smem;
  float* QK = X + max_len * sx;
  float* S = QK + max_len * sqk;
  float* pbar = S + max_len * (max_len + 1);      // (H, L_b)
  int* lpos = reinterpret_cast<int*>(pbar + H * max_len);
  int* wtot = lpos + max_len;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int L = ap_live_ids<IdxT>(ids, n, offsets, off64, n_off, b, pad, max_len, lpos, wtot, err_flag);
    if (threadIdx.x == 0) cnt[b] = (float)L;
    if (L == 0) {      // uniform: a zero block
      for (int o = threadIdx.x; o < H * E; o += AP_THREADS) out[b * H * E + o] = from_f32<T>(0.f);
      continue;
    }
    const float cscale = mode == AP_MEAN ? 1.f / (float)L : 1.f;
    ap_fwd_sample<MF, T>(X, sx, QK, sqk, S, ss, pbar, table, [ids, lpos](int l) { return ids[lpos[l]]; }, L, E, V, W, bqk,
                         H, cscale, out + b * H * E, err_flag, vec);
  }
}

// dx (n, E): only the rows of the positions a bag takes are written -- the caller zero-fills it
template <typename T, typename IdxT, bool MF>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_ragged_bwd_kernel(
    const T* __restrict__ table, const IdxT* __restrict__ ids, int64_t n, const void* __restrict__ offsets, bool off64,
    int64_t n_off, int64_t B, int max_len, int64_t pad, int E, int64_t V, const T* __restrict__ W,
    const T* __restrict__ bqk, int H, int mode, const T* __restrict__ gout, T* __restrict__ dx,
    float* __restrict__ dw_part, float* __restrict__ db_part, float* pbar_ws, int32_t* __restrict__ err_flag, bool vec) {
  extern __shared__ __attribute__((aligned(16))) float ap_smem[];
  const int sx = E + 1, sqk = 2 * E + 1, ss = max_len | 1, sdq = E + 1;
  float* X = ap_smem;
  float* QK = X + max_len * sx;
  float* S = QK + max_len * sqk;
  float* dQ = S + max_len * (max_len + 1);
  float* rv = dQ + max_len * sdq;      // (L_b)
  int* lpos = reinterpret_cast<int*>(rv + max_len);
  int* wtot = lpos + max_len;
  float* pbar = pbar_ws != nullptr ? pbar_ws + (size_t)blockIdx.x * H * max_len : reinterpret_cast<float*>(wtot + 4);
  float* dW = dw_part + (size_t)blockIdx.x * 2 * E * E;
  float* db = db_part + (size_t)blockIdx.x * 2 * E;
  for (int i = threadIdx.x; i < 2 * E * E; i += AP_THREADS) dW[i] = 0.f;
  for (int i = threadIdx.x; i < 2 * E; i += AP_THREADS) db[i] = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const int L = ap_live_ids<IdxT>(ids, n, offsets, off64, n_off, b, pad, max_len, lpos, wtot, err_flag);
    if (L == 0) continue;      // uniform: no gradient from this sample
    const float cscale = mode == AP_MEAN ? 1.f / (float)L : 1.f;
    ap_bwd_sample<MF, T>(X, sx, QK, sqk, S, ss, dQ, sdq, rv, pbar, table, [ids, lpos](int l) { return ids[lpos[l]]; }, L,
                         E, V, W, bqk, H, cscale, gout + b * H * E, dx, [lpos](int m) { return (int64_t)lpos[m]; }, dW, db,
                         err_flag, vec);
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

// ragged: the padded layout at L = max_len plus lpos (max_len ints) and the four wave totals of ap_live_ids
static size_t apr_ints(int max_len) { return sizeof(int) * ((size_t)max_len + 4); }
static size_t apr_fwd_lds(int max_len, int E, int H) { return ap_fwd_lds(max_len, E, H) + apr_ints(max_len); }
static bool apr_bwd_pbar_in_lds(int max_len, int E, int H) {
  return ap_bwd_lds_base(max_len, E) + apr_ints(max_len) + sizeof(float) * (size_t)H * max_len <= AP_MAX_LDS;
}
static size_t apr_bwd_lds(int max_len, int E, int H) {
  return ap_bwd_lds_base(max_len, E) + apr_ints(max_len) +
         (apr_bwd_pbar_in_lds(max_len, E, H) ? sizeof(float) * (size_t)H * max_len : 0);
}

template <typename T, bool MF>
static const void* apr_kernel_of(bool backward, bool i64) {
  if (backward)
    return i64 ? (const void*)attn_pool_ragged_bwd_kernel<T, int64_t, MF>
               : (const void*)attn_pool_ragged_bwd_kernel<T, int32_t, MF>;
  return i64 ? (const void*)attn_pool_ragged_fwd_kernel<T, int64_t, MF>
             : (const void*)attn_pool_ragged_fwd_kernel<T, int32_t, MF>;
}
static const void* apr_kernel(int path, int dtype, bool backward, bool i64) {
  if (dtype == TRS_F32) return apr_kernel_of<float, false>(backward, i64);
  return path == 2 ? apr_kernel_of<bf16_t, true>(backward, i64) : apr_kernel_of<bf16_t, false>(backward, i64);
}

static int apr_check(const char* what, int64_t V, int E, int dtype, int ids_dtype, int64_t n, int off_dtype, int64_t n_off,
                     int64_t B, int max_len, int64_t exclude_row, int H, int mode) {
  TRS_REQUIRE(V > 0 && B > 0 && n >= 0, TRS_EINVAL, "%s: bad size V=%lld B=%lld n=%lld", what, (long long)V, (long long)B,
              (long long)n);
  TRS_REQUIRE(n_off == B || n_off == B + 1, TRS_EINVAL, "%s: %lld offsets for B=%lld bags (B or B + 1)", what,
              (long long)n_off, (long long)B);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL, "%s: exclude_row %lld outside [-1, V)", what,
              (long long)exclude_row);
  TRS_REQUIRE(max_len >= 1 && max_len <= AP_MAX_L, TRS_EINVAL, "%s: max_len %d outside [1, %d]", what, max_len, AP_MAX_L);
  TRS_REQUIRE(mode == AP_SUM || mode == AP_MEAN, TRS_EINVAL, "%s: mode %d (0 = sum, 1 = mean)", what, mode);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE, "%s: n=%lld and B=%lld must fit int32", what,
              (long long)n, (long long)B);
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(ids_dtype == TRS_I64 || ids_dtype == TRS_I32, TRS_EDTYPE, "%s: ids dtype %d", what, ids_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "%s: offsets dtype %d", what, off_dtype);
  TRS_REQUIRE(ap_path(max_len, E, H, dtype) != 0, TRS_EDTYPE,
              "%s: unsupported shape max_len=%d E=%d H=%d (E <= %d, E %% H == 0)", what, max_len, E, H, AP_MAX_E);
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

extern "C" int trs_attn_pool_ragged_blocks(int64_t B, int32_t max_len, int32_t E, int32_t H, int32_t dtype,
                                           int32_t backward) {
  const int path = ap_path(max_len, E, H, dtype);
  if (path == 0 || B < 1) return 0;
  return ap_blocks(apr_kernel(path, dtype, backward != 0, true),
                   backward ? apr_bwd_lds(max_len, E, H) : apr_fwd_lds(max_len, E, H), B);
}

extern "C" size_t trs_attn_pool_ragged_bwd_workspace_bytes(int32_t blocks, int32_t max_len, int32_t E, int32_t H) {
  if (blocks < 1 || max_len < 1 || E < 1 || H < 1 || apr_bwd_pbar_in_lds(max_len, E, H)) return 0;
  return sizeof(float) * (size_t)blocks * H * max_len;
}

extern "C" int trs_attn_pool_ragged_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids,
                                        int32_t ids_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                                        int64_t n_off, int64_t B, int32_t max_len, int64_t exclude_row, const void* w_qk,
                                        const void* b_qk, int32_t H, int32_t mode, void* out, float* cnt,
                                        int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(table && offsets && w_qk && out && cnt && (ids || n == 0), TRS_EINVAL,
              "attn_pool_ragged_fwd: NULL pointer");
  if (int rc = apr_check("attn_pool_ragged_fwd", V, E, dtype, ids_dtype, n, off_dtype, n_off, B, max_len, exclude_row, H,
                         mode))
    return rc;
  const int path = ap_path(max_len, E, H, dtype);
  const bool i64 = ids_dtype == TRS_I64, off64 = off_dtype == TRS_I64;
  const size_t lds = apr_fwd_lds(max_len, E, H);
  const int grid = ap_blocks(apr_kernel(path, dtype, false, i64), lds, B);
  const bool vec = path == 2 && aligned16(table) && aligned16(w_qk);      // 16-byte loads of table and weight rows
  hipStream_t s = (hipStream_t)stream;
#define TRS_AP(T, I, MF)                                                                                                \
  hipLaunchKernelGGL((attn_pool_ragged_fwd_kernel<T, I, MF>), dim3(grid), dim3(AP_THREADS), lds, s, (const T*)table,    \
                     (const I*)ids, n, offsets, off64, n_off, B, max_len, exclude_row, E, V, (const T*)w_qk,            \
                     (const T*)b_qk, H, mode, (T*)out, cnt, err_flag, vec)
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
  return check_launch("attn_pool_ragged_fwd");
}

extern "C" int trs_attn_pool_ragged_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids,
                                        int32_t ids_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                                        int64_t n_off, int64_t B, int32_t max_len, int64_t exclude_row, const void* w_qk,
                                        const void* b_qk, int32_t H, int32_t mode, const void* gout, void* dx,
                                        float* dw_part, float* db_part, int32_t blocks, void* workspace, size_t ws_bytes,
                                        int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(table && offsets && w_qk && gout && dw_part && db_part && ((ids && dx) || n == 0), TRS_EINVAL,
              "attn_pool_ragged_bwd: NULL pointer");
  if (int rc = apr_check("attn_pool_ragged_bwd", V, E, dtype, ids_dtype, n, off_dtype, n_off, B, max_len, exclude_row, H,
                         mode))
    return rc;
  TRS_REQUIRE(blocks >= 1 && blocks <= B, TRS_EINVAL, "attn_pool_ragged_bwd: blocks=%d outside [1, B]", blocks);
  const size_t need = trs_attn_pool_ragged_bwd_workspace_bytes(blocks, max_len, E, H);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need), TRS_EWORKSPACE,
              "attn_pool_ragged_bwd: workspace %zu < %zu", ws_bytes, need);
  const int path = ap_path(max_len, E, H, dtype);
  const bool i64 = ids_dtype == TRS_I64, off64 = off_dtype == TRS_I64;
  const size_t lds = apr_bwd_lds(max_len, E, H);
  (void)ap_resident(apr_kernel(path, dtype, true, i64), lds);      // raises the kernel's LDS limit where needed
  float* pbar_ws = need ? (float*)workspace : nullptr;
  const bool vec = path == 2 && aligned16(table) && aligned16(w_qk);      // 16-byte loads of table and weight rows
  hipStream_t s = (hipStream_t)stream;
#define TRS_AP(T, I, MF)                                                                                                \
  hipLaunchKernelGGL((attn_pool_ragged_bwd_kernel<T, I, MF>), dim3(blocks), dim3(AP_THREADS), lds, s, (const T*)table,  \
                     (const I*)ids, n, offsets, off64, n_off, B, max_len, exclude_row, E, V, (const T*)w_qk,            \
                     (const T*)b_qk, H, mode, (const T*)gout, (T*)dx, dw_part, db_part, pbar_ws, err_flag, vec)
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
  return check_launch("attn_pool_ragged_bwd");
}
