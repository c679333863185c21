// Residual multi-head self-attention over a short list, un-pooled: Y = X + nn.MultiheadAttention(X, X, X) for a (B, L, E)
// block (no masks, no dropout) -- the attention half of an encoder layer of the reference's PersonalizedReRankingModel
// (models/ltr/personalized_reranking.py).  Per sample, X (L, E), d = E / H, Win (3E, E), Wout (E, E):
//   [Q|K|V] = X Win^T + bin          P_h = softmax_rows(Q_h K_h^T / sqrt(d))
//   O = concat_h(P_h V_h)            Y = X + O Wout^T + bout                   <- (B, L, E), the only HBM write
// Q|K|V, the scores and O never reach HBM.
//
// The arrangement is attn_pool.hip's (attn_common.hpp): one workgroup of 256 threads owns one sample at a time
// (persistent: b = blockIdx.x, += gridDim.x), operands live in LDS as fp32 with odd row strides, every product is ap_gemm:
//   vector path (1): fp32 FMA, fp32 or bf16 operands, any E % H == 0;
//   MFMA path   (2): bf16 with E % 16 == 0 and d % 16 == 0: v_mfma_f32_16x16x32_bf16, operands rounded to bf16 as they are
//                    read (X, G and the weights are bf16 already; Q, K, V, P, O, dO, dS and dQ|dK|dV take one rounding, as
//                    they would in ATen's bf16 module), fp32 accumulation, edges zero-filled.  The list index is the k index
//                    of P V, P^T dO and the weight gradients.
// The weights are read from global memory (32 KB at E = 64 in bf16: L1 / L2 resident).
//
// Backward, G = dY; Q, K, V, P and O are recomputed from X, so the forward saves nothing but its input:
//   dO = G Wout          dWout += G^T O        dbout += sum_l G
//   dV_h = P_h^T dO_h    dP = dO_h V_h^T       dS = P o (dP - rowsum(dP o P))
//   dQ_h = dS K_h / sqrt(d)                    dK_h = dS^T Q_h / sqrt(d)
//   dX = G + [dQ|dK|dV] Win                    dWin += [dQ|dK|dV]^T X      dbin += sum_l [dQ|dK|dV]
// dV_h overwrites V_h, dK_h overwrites K_h and dQ_h overwrites dO_h once they are dead; the sum [dQ|dK|dV] Win lands in the
// Q third of the Q|K|V buffer; G is read from global memory where it is needed (three times, L2 resident).
//
// LDS per sample, floats (row strides padded by one):
//   forward : X  L (E + 1) | QKV  L (3E + 1) | S  L (L + 1) | O  L (E + 1)          = 5 L E + L^2 + 4 L
//             L = 30, E = 64: 42 KB (three workgroups per CU); L = 64, E = 64: 99 KB
//   backward: X | QKV | dO  L (E + 1) | O | S | dP  L (L + 1)                       = 6 L E + 2 L^2 + 6 L
//             L = 30, E = 64: 54 KB (two workgroups per CU); L = 64, E = 64: 133 KB; E = 128 fits 160 KB up to L = 47
// A shape whose backward does not fit reports path 0.
//
// The weight and bias gradients are accumulated in fp32 in the workgroup's OWN slab of the workspace,
// [dWin (3E, E) | dWout (E, E) | dbin (3E) | dbout (E)], by plain read-modify-writes; samples are dealt to workgroups
// statically, the caller reduces the slabs in a fixed order, and there are no atomics: two calls give the same bits.
#include "attn_common.hpp"

namespace trs {

// the sample's (L, E) rows into LDS as fp32
template <typename T>
__device__ __forceinline__ void sa_load(float* X, int sx, const T* __restrict__ x, int L, int E) {
  for (int i = threadIdx.x; i < L * E; i += AP_THREADS) {
    const int l = i / E;
    X[l * sx + (i - l * E)] = to_f32(x[i]);
  }
}

// C = A W^T + b with W (N, E) in global memory: 16-byte weight loads on the MFMA path where the rows are aligned
template <bool MF, typename T>
__device__ __forceinline__ void sa_project(float* C, int sc, const float* A, int sa, const T* __restrict__ W,
                                           const T* __restrict__ b, int L, int N, int E, bool vec) {
  if constexpr (MF) {
    if (vec) {
      ap_gemm<true, true>(C, sc, 1, false, A, sa, 1, W, 1, E, L, N, E, 1.f, b);
      return;
    }
  }
  ap_gemm<MF, false, true>(C, sc, 1, false, A, sa, 1, W, 1, E, L, N, E, 1.f, b);
}

// S <- P_h, then O_h = P_h V_h (and, in the backward, dP = dO_h V_h^T beside it); leaves the block synchronised
template <bool MF, bool BWD>
__device__ __forceinline__ void sa_head(float* S, int ss, const float* QKV, int sq, float* O, int so, const float* dO,
                                        int sdo, float* dP, int L, int E, int d, int h, float alpha) {
  const float* Qh = QKV + h * d;
  const float* Kh = QKV + E + h * d;
  const float* Vh = QKV + 2 * E + h * d;
  ap_gemm<MF>(S, ss, 1, false, Qh, sq, 1, Kh, 1, sq, L, L, d, alpha, (const float*)nullptr);
  __syncthreads();
  ap_softmax_rows(S, ss, L);
  __syncthreads();
  ap_gemm<MF>(O + h * d, so, 1, false, S, ss, 1, Vh, sq, 1, L, d, L, 1.f, (const float*)nullptr);
  if constexpr (BWD) ap_gemm<MF>(dP, ss, 1, false, dO + h * d, sdo, 1, Vh, 1, sq, L, L, d, 1.f, (const float*)nullptr);
  __syncthreads();
}

template <typename T, bool MF>
__global__ __launch_bounds__(AP_THREADS) void self_attn_fwd_kernel(const T* __restrict__ x, int64_t B, int L, int E, int H,
                                                                   const T* __restrict__ w_in, const T* __restrict__ b_in,
                                                                   const T* __restrict__ w_out,
                                                                   const T* __restrict__ b_out, T* __restrict__ y,
                                                                   bool vec) {
  extern __shared__ __attribute__((aligned(16))) float sa_smem[];
  const int d = E / H, sx = E + 1, sq = 3 * E + 1, ss = L + 1;
  float* X = sa_smem;
  float* QKV = X + L * sx;
  float* S = QKV + L * sq;
  float* O = S + L * ss;
  const float alpha = 1.f / sqrtf((float)d);
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    sa_load<T>(X, sx, x + b * L * E, L, E);
    __syncthreads();
    sa_project<MF, T>(QKV, sq, X, sx, w_in, b_in, L, 3 * E, E, vec);
    __syncthreads();
    for (int h = 0; h < H; ++h) sa_head<MF, false>(S, ss, QKV, sq, O, sx, nullptr, 0, nullptr, L, E, d, h, alpha);
    // Q third <- O Wout^T + bout (Q is dead)
    sa_project<MF, T>(QKV, sq, O, sx, w_out, b_out, L, E, E, vec);
    __syncthreads();
    T* yb = y + b * L * E;
    for (int i = threadIdx.x; i < L * E; i += AP_THREADS) {
      const int l = i / E, e = i - l * E;
      yb[i] = from_f32<T>(X[l * sx + e] + QKV[l * sq + e]);
    }
    __syncthreads();
  }
}

template <typename T, bool MF>
__global__ __launch_bounds__(AP_THREADS) void self_attn_bwd_kernel(const T* __restrict__ x, int64_t B, int L, int E, int H,
                                                                   const T* __restrict__ w_in, const T* __restrict__ b_in,
                                                                   const T* __restrict__ w_out, const T* __restrict__ gout,
                                                                   T* __restrict__ dx, float* __restrict__ slabs,
                                                                   bool vec) {
  extern __shared__ __attribute__((aligned(16))) float sa_smem[];
  const int d = E / H, sx = E + 1, sq = 3 * E + 1, ss = L + 1;
  float* X = sa_smem;
  float* QKV = X + L * sx;
  float* dO = QKV + L * sq;          // dO, then dQ head by head
  float* O = dO + L * sx;
  float* S = O + L * sx;
  float* dP = S + L * ss;            // dP, then dS
  const float alpha = 1.f / sqrtf((float)d);
  const size_t slab = (size_t)4 * E * E + 4 * E;
  float* dWin = slabs + (size_t)blockIdx.x * slab;
  float* dWout = dWin + 3 * E * E;
  float* dbin = dWout + E * E;
  float* dbout = dbin + 3 * E;
  for (int i = threadIdx.x; i < (int)slab; i += AP_THREADS) dWin[i] = 0.f;
  __syncthreads();
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const T* g = gout + b * L * E;
    sa_load<T>(X, sx, x + b * L * E, L, E);
    __syncthreads();
    sa_project<MF, T>(QKV, sq, X, sx, w_in, b_in, L, 3 * E, E, vec);
    // dO = G Wout
    ap_gemm<MF>(dO, sx, 1, false, g, E, 1, w_out, E, 1, L, E, E, 1.f, (const float*)nullptr);
    __syncthreads();
    for (int h = 0; h < H; ++h) {
      sa_head<MF, true>(S, ss, QKV, sq, O, sx, dO, sx, dP, L, E, d, h, alpha);
      // V_h <- dV_h = P^T dO_h
      ap_gemm<MF>(QKV + 2 * E + h * d, sq, 1, false, S, 1, ss, dO + h * d, sx, 1, L, d, L, 1.f, (const float*)nullptr);
      {   // dP <- dS = P o (dP - rowsum(dP o P)), 4 lanes per row
        const int row = threadIdx.x >> 2, sub = threadIdx.x & 3;
        const float* p = S + row * ss;
        float* dp = dP + row * ss;
        float t = 0.f;
        if (row < L)
          for (int c = sub; c < L; c += 4) t = fmaf(p[c], dp[c], t);
        t = group_sum_up<4>(t);
        if (row < L)
          for (int c = sub; c < L; c += 4) dp[c] = p[c] * (dp[c] - t);
      }
      __syncthreads();
      // dO_h <- dQ_h = alpha dS K_h
      ap_gemm<MF>(dO + h * d, sx, 1, false, dP, ss, 1, QKV + E + h * d, sq, 1, L, d, L, alpha, (const float*)nullptr);
      __syncthreads();
      // K_h <- dK_h = alpha dS^T Q_h
      ap_gemm<MF>(QKV + E + h * d, sq, 1, false, dP, 1, ss, QKV + h * d, sq, 1, L, d, L, alpha, (const float*)nullptr);
      __syncthreads();
    }
    // from here: dO holds dQ, QKV holds Q | dK | dV
    for (int j = threadIdx.x; j < 4 * E; j += AP_THREADS) {
      float s = 0.f;
      if (j < E) {
        for (int l = 0; l < L; ++l) s += dO[l * sx + j];
      } else if (j < 3 * E) {
        for (int l = 0; l < L; ++l) s += QKV[l * sq + j];
      } else {
        for (int l = 0; l < L; ++l) s += to_f32(g[l * E + j - 3 * E]);
      }
      dbin[j] += s;          // dbout follows dbin in the slab
    }
    // dWq += dQ^T X, dW[k|v] += [dK|dV]^T X, dWout += G^T O
    ap_gemm<MF>(dWin, E, 1, true, dO, 1, sx, X, sx, 1, E, E, L, 1.f, (const float*)nullptr);
    ap_gemm<MF>(dWin + E * E, E, 1, true, QKV + E, 1, sq, X, sx, 1, 2 * E, E, L, 1.f, (const float*)nullptr);
    ap_gemm<MF>(dWout, E, 1, true, g, 1, E, O, sx, 1, E, E, L, 1.f, (const float*)nullptr);
    if (dx != nullptr) {
      // Q third <- dQ Wq + [dK|dV] W[k|v]
      ap_gemm<MF>(QKV, sq, 1, false, dO, sx, 1, w_in, E, 1, L, E, E, 1.f, (const float*)nullptr);
      __syncthreads();
      ap_gemm<MF>(QKV, sq, 1, true, QKV + E, sq, 1, w_in + E * E, E, 1, L, E, 2 * E, 1.f, (const float*)nullptr);
      __syncthreads();
      T* dxb = dx + b * L * E;
      for (int i = threadIdx.x; i < L * E; i += AP_THREADS) {
        const int l = i / E, e = i - l * E;
        dxb[i] = from_f32<T>(to_f32(g[i]) + QKV[l * sq + e]);
      }
    }
    __syncthreads();
  }
}

static size_t sa_fwd_lds(int L, int E) {
  return sizeof(float) * ((size_t)2 * L * (E + 1) + (size_t)L * (3 * E + 1) + (size_t)L * (L + 1));
}
static size_t sa_bwd_lds(int L, int E) {
  return sizeof(float) * ((size_t)3 * L * (E + 1) + (size_t)L * (3 * E + 1) + (size_t)2 * L * (L + 1));
}

static int sa_path(int L, int E, int H, int dtype) {
  if (dtype != TRS_F32 && dtype != TRS_BF16) return 0;
  if (L < 1 || L > AP_MAX_L || E < 1 || E > AP_MAX_E || H < 1 || E % H != 0) return 0;
  if (sa_bwd_lds(L, E) > AP_MAX_LDS) return 0;
  if (dtype == TRS_BF16 && E % 16 == 0 && (E / H) % 16 == 0) return 2;
  return 1;
}

static const void* sa_kernel(int path, int dtype, bool backward) {
  if (dtype == TRS_F32)
    return backward ? (const void*)self_attn_bwd_kernel<float, false> : (const void*)self_attn_fwd_kernel<float, false>;
  if (path == 2)
    return backward ? (const void*)self_attn_bwd_kernel<bf16_t, true> : (const void*)self_attn_fwd_kernel<bf16_t, true>;
  return backward ? (const void*)self_attn_bwd_kernel<bf16_t, false> : (const void*)self_attn_fwd_kernel<bf16_t, false>;
}

static int sa_check(const char* what, int64_t B, int L, int E, int H, int dtype) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(B >= 0, TRS_EINVAL, "%s: bad size B=%lld", what, (long long)B);
  TRS_REQUIRE(sa_path(L, E, H, dtype) != 0, TRS_EDTYPE,
              "%s: unsupported shape L=%d E=%d H=%d (1 <= L <= %d, E <= %d, E %% H == 0, backward within %zu bytes of LDS)",
              what, L, E, H, AP_MAX_L, AP_MAX_E, AP_MAX_LDS);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" int trs_self_attn_path(int32_t L, int32_t E, int32_t H, int32_t dtype) { return sa_path(L, E, H, dtype); }

extern "C" int trs_self_attn_blocks(int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, int32_t backward) {
  const int path = sa_path(L, E, H, dtype);
  if (path == 0 || B < 1) return 0;
  return ap_blocks(sa_kernel(path, dtype, backward != 0), backward ? sa_bwd_lds(L, E) : sa_fwd_lds(L, E), B);
}

extern "C" size_t trs_self_attn_bwd_workspace_bytes(int32_t blocks, int32_t E) {
  if (blocks < 1 || E < 1) return 0;
  return sizeof(float) * (size_t)blocks * ((size_t)4 * E * E + 4 * E);
}

extern "C" int trs_self_attn_fwd(const void* x, int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, const void* w_in,
                                 const void* b_in, const void* w_out, const void* b_out, void* y, trs_stream_t stream) {
  TRS_REQUIRE(B == 0 || (x && w_in && w_out && y), TRS_EINVAL, "self_attn_fwd: NULL pointer");
  TRS_REQUIRE((b_in == nullptr) == (b_out == nullptr), TRS_EINVAL, "self_attn_fwd: b_in and b_out come together or not at all");
  if (int rc = sa_check("self_attn_fwd", B, L, E, H, dtype)) return rc;
  if (B == 0) return TRS_OK;
  const int path = sa_path(L, E, H, dtype);
  const size_t lds = sa_fwd_lds(L, E);
  const int grid = ap_blocks(sa_kernel(path, dtype, false), lds, B);
  const bool vec = path == 2 && aligned16(w_in) && aligned16(w_out);      // 16-byte loads of weight rows
  hipStream_t s = (hipStream_t)stream;
#define TRS_SA(T, MF)                                                                                                  \
  hipLaunchKernelGGL((self_attn_fwd_kernel<T, MF>), dim3(grid), dim3(AP_THREADS), lds, s, (const T*)x, B, L, E, H,      \
                     (const T*)w_in, (const T*)b_in, (const T*)w_out, (const T*)b_out, (T*)y, vec)
  if (dtype == TRS_F32) TRS_SA(float, false);
  else if (path == 2) TRS_SA(bf16_t, true);
  else TRS_SA(bf16_t, false);
#undef TRS_SA
  return check_launch("self_attn_fwd");
}

extern "C" int trs_self_attn_bwd(const void* x, int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, const void* w_in,
                                 const void* b_in, const void* w_out, const void* b_out, const void* gout, void* dx,
                                 void* workspace, size_t ws_bytes, int32_t blocks, trs_stream_t stream) {
  TRS_REQUIRE(B == 0 || (x && w_in && w_out && gout && workspace), TRS_EINVAL, "self_attn_bwd: NULL pointer");
  TRS_REQUIRE((b_in == nullptr) == (b_out == nullptr), TRS_EINVAL, "self_attn_bwd: b_in and b_out come together or not at all");
  if (int rc = sa_check("self_attn_bwd", B, L, E, H, dtype)) return rc;
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(blocks >= 1 && blocks <= B, TRS_EINVAL, "self_attn_bwd: blocks=%d outside [1, B]", blocks);
  const size_t need = trs_self_attn_bwd_workspace_bytes(blocks, E);
  TRS_REQUIRE(ws_bytes >= need, TRS_EWORKSPACE, "self_attn_bwd: workspace %zu < %zu", ws_bytes, need);
  const int path = sa_path(L, E, H, dtype);
  const size_t lds = sa_bwd_lds(L, E);
  (void)ap_resident(sa_kernel(path, dtype, true), lds);      // raises the kernel's LDS limit where needed
  const bool vec = path == 2 && aligned16(w_in) && aligned16(w_out);
  hipStream_t s = (hipStream_t)stream;
#define TRS_SA(T, MF)                                                                                                  \
  hipLaunchKernelGGL((self_attn_bwd_kernel<T, MF>), dim3(blocks), dim3(AP_THREADS), lds, s, (const T*)x, B, L, E, H,    \
                     (const T*)w_in, (const T*)b_in, (const T*)w_out, (const T*)gout, (T*)dx, (float*)workspace, vec)
  if (dtype == TRS_F32) TRS_SA(float, false);
  else if (path == 2) TRS_SA(bf16_t, true);
  else TRS_SA(bf16_t, false);
#undef TRS_SA
  return check_launch("self_attn_bwd");
}
