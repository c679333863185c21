// Behaviour-to-interest dynamic routing (MIND capsule routing; layers/ctr/dynamic_routing.py).  With the fp32 priors
// pri[b,n,:] = x[b,n,:] @ S (a library GEMM in front of the kernel), the coupling noise b0 (B, K, N, R) and c[b,k,n] = 0:
//   num_iter - 1 times:  w = softmax_k(b0[b,k,n,r] + c[b,k,n]);  z[b,k,r] = sum_n w pri[b,n,r];  v = squash(z)
//                        c[b,k,n] += sum_r pri[b,n,r] v[b,k,r]
//   out = squash(sum_n softmax_k(b0 + c) pri),      squash(z) = n2 / (1 + n2) * z / (sqrt(n2) + 1e-8),  n2 = sum_r z^2
// The reference repeats the priors K times into (B, K, N, R) and makes six to eight passes over tensors of that size per
// iteration.  Its similarity update is a (B, K, N, 1) tensor broadcast over R, so all the routing state beyond the noise
// is the (B, K, N) sum c; its loop runs on detached priors, so the backward is
//   dpri[b,n,r] = sum_k softmax_k(b0 + c)[b,k,n,r] dz[b,k,r],   dz = the squash backward of gout at z
// and needs b0, the final c and z, and gout only: no iterations, no priors.
// Everything between the loads and the final stores is fp32; the softmax subtracts the maximum over k; no atomics, the
// summation order is fixed: results are bit-reproducible.
// An all-zero sample (n2 == 0) gives a zero output and a zero dz here.  The reference's forward gives zero as well, but its
// autograd yields NaN there (the derivative of sqrt at 0 is inf, times 0).
//
// Forward: a workgroup of 512 threads owns a sample for all iterations.  Priors (row stride R | 1: the c update reads them
// by row, the routing pass by column), c, z and the partial sums live in LDS.  The noise is staged into LDS in its own
// dtype, all K * N * R of it once where the sample fits beside the rest in 160 KiB, else in chunks of NC rows that every
// iteration fetches again (L2 / Infinity Cache hits after the first).  Thread t owns column t % R of the rows
// t / R, t / R + NG, ... (NG = 512 / R): one softmax over k per (n, r) from LDS reads, K running sums in registers; the
// NG partial sums per (k, r) are added in the order of their row groups.  The vector path stages priors and noise with
// 16-byte loads (rows of whole 16-byte vectors, aligned pointers), the element path with element loads; they share
// everything else.  K is a template parameter (1 <= K <= 8).
// Backward: streaming, 256 threads; dz (K, R) and c (K, N) of a sample go to LDS, then every thread owns 16 bytes (vector
// path) or one element of a dpri row: K noise loads, one softmax per column, K multiply-adds, one store.
// Algorithmic bytes per sample (s = sizeof(T)): forward K N R s + 4 N R in, K R s (+ 4 K (N + R)) out;
// backward K N R s + 4 K (N + R) + K R s in, N R s out.
#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <utility>

#include "trs_common.hpp"

namespace trs {

constexpr int DR_MAX_N = 128, DR_MAX_R = 128, DR_MAX_K = 8;
constexpr int DR_THREADS = 512;
constexpr int DR_BWD_THREADS = 256;
constexpr size_t DR_MAX_LDS = 160 * 1024;
constexpr size_t DR_CHUNK_LDS = 80 * 1024;      // chunked noise: two workgroups per CU where a chunk of >= 8 rows allows it

// bytes of LDS in front of the noise: priors, c, partial sums, z / v, n2
__host__ __device__ inline size_t dr_fixed_bytes(int N, int R, int K) {
  const size_t floats = (size_t)N * (R | 1) + (size_t)K * N + (size_t)(DR_THREADS / R) * K * R + (size_t)K * R + 8;
  return (floats * sizeof(float) + 15) & ~(size_t)15;
}

template <typename T, int K, bool VEC>
__global__ __launch_bounds__(DR_THREADS) void dr_fwd_kernel(const float* __restrict__ pri, const T* __restrict__ noise,
                                                            int64_t B, int N, int R, int iters, int NC,
                                                            T* __restrict__ out, float* __restrict__ c_out,
                                                            float* __restrict__ z_out) {
  extern __shared__ __attribute__((aligned(16))) char dr_smem[];
  constexpr int VE = Vec16<T>::VE;
  const int RP = R | 1;
  const int NG = DR_THREADS / R;
  float* pri_s = reinterpret_cast<float*>(dr_smem);      // [N][RP]
  float* c_s = pri_s + N * RP;                           // [K][N]
  float* zpart = c_s + K * N;                            // [NG][K][R]
  float* z_s = zpart + NG * K * R;                       // [K][R]: z, then v
  float* n2_s = z_s + K * R;                             // [K]
  T* noise_s = reinterpret_cast<T*>(dr_smem + dr_fixed_bytes(N, R, K));      // [K][NC][R]
  const int t = threadIdx.x;
  const int g = t / R, r = t - g * R;
  const bool active = g < NG;
  const int lane = t & 63, wave = t >> 6;
  const bool resident = NC >= N;

  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    const float* prow = pri + b * N * R;
    if (VEC) {
      const uint4* src = reinterpret_cast<const uint4*>(prow);
      for (int i = t; i < N * R / 4; i += DR_THREADS) {
        float f[4];
        Vec16<float>::unpack(load_stream(src + i), f);
        const int n = (4 * i) / R, rr = 4 * i - n * R;
#pragma unroll
        for (int j = 0; j < 4; ++j) pri_s[n * RP + rr + j] = f[j];
      }
    } else {
      for (int i = t; i < N * R; i += DR_THREADS) {
        const int n = i / R;
        pri_s[n * RP + (i - n * R)] = prow[i];
      }
    }
    for (int i = t; i < K * N; i += DR_THREADS) c_s[i] = 0.f;

    for (int it = 0; it < iters; ++it) {
      float zacc[K];
#pragma unroll
      for (int k = 0; k < K; ++k) zacc[k] = 0.f;
      for (int n0 = 0; n0 < N; n0 += NC) {
        const int nc = min(NC, N - n0);
        if (it == 0 || !resident) {
          __syncthreads();      // the readers of the previous chunk (and of the previous sample) are done
          if (VEC) {
            const int nvec = nc * R / VE;
            for (int i = t; i < K * nvec; i += DR_THREADS) {
              const int k = i / nvec, j = i - k * nvec;
              const uint4* src = reinterpret_cast<const uint4*>(noise + ((b * K + k) * N + n0) * R) + j;
              reinterpret_cast<uint4*>(noise_s + (size_t)k * NC * R)[j] = resident ? load_stream(src) : *src;
            }
          } else {
            const int ne = nc * R;
            for (int i = t; i < K * ne; i += DR_THREADS) {
              const int k = i / ne, j = i - k * ne;
              noise_s[(size_t)k * NC * R + j] = noise[((b * K + k) * N + n0) * R + j];
            }
          }
          __syncthreads();
        }
        if (active) {
          for (int n = n0 + g; n < n0 + nc; n += NG) {
            const float p = pri_s[n * RP + r];
            float x[K];
            float m = -INFINITY;
#pragma unroll
            for (int k = 0; k < K; ++k) {
              x[k] = to_f32(noise_s[((size_t)k * NC + (n - n0)) * R + r]) + c_s[k * N + n];
              m = fmaxf(m, x[k]);
            }
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
              x[k] = __expf(x[k] - m);
              s += x[k];
            }
            const float ps = p * __builtin_amdgcn_rcpf(s);
#pragma unroll
            for (int k = 0; k < K; ++k) zacc[k] = fmaf(x[k], ps, zacc[k]);
          }
        }
      }
      if (active) {
#pragma unroll
        for (int k = 0; k < K; ++k) zpart[(g * K + k) * R + r] = zacc[k];
      }
      __syncthreads();
      for (int i = t; i < K * R; i += DR_THREADS) {
        float s = 0.f;
        for (int gg = 0; gg < NG; ++gg) s += zpart[gg * K * R + i];
        z_s[i] = s;
      }
      __syncthreads();
      if (wave < K) {
        float s = 0.f;
        for (int rr = lane; rr < R; rr += 64) s = fmaf(z_s[wave * R + rr], z_s[wave * R + rr], s);
        s = group_sum_up<64>(s);
        if (lane == 0) n2_s[wave] = s;
      }
      __syncthreads();
      const bool last = it == iters - 1;
      if (last && z_out != nullptr) {
        for (int i = t; i < K * R; i += DR_THREADS) z_out[b * K * R + i] = z_s[i];
        for (int i = t; i < K * N; i += DR_THREADS) c_out[b * K * N + i] = c_s[i];
      }
      for (int i = t; i < K * R; i += DR_THREADS) {
        const float n2 = n2_s[i / R];
        const float v = (n2 / (1.f + n2)) * (z_s[i] / (sqrtf(n2) + 1e-8f));      // n2 == 0: z == 0, v = 0
        if (last) out[b * K * R + i] = from_f32<T>(v);
        else z_s[i] = v;
      }
      if (!last) {
        __syncthreads();
        for (int i = t; i < K * N; i += DR_THREADS) {
          const int k = i / N, n = i - k * N;
          float s = 0.f;
          for (int rr = 0; rr < R; ++rr) s = fmaf(pri_s[n * RP + rr], z_s[k * R + rr], s);
          c_s[i] += s;
        }
      }
      __syncthreads();
    }
  }
}

template <typename T, int VE>
__device__ __forceinline__ void dr_load(const T* p, float* f) {
  if constexpr (VE == 1) f[0] = to_f32(*p);
  else Vec16<T>::unpack(load_stream(reinterpret_cast<const uint4*>(p)), f);
}
template <typename T, int VE>
__device__ __forceinline__ void dr_store(T* p, const float* f) {
  if constexpr (VE == 1) *p = from_f32<T>(f[0]);
  else store_stream(reinterpret_cast<uint4*>(p), Vec16<T>::pack(f));
}

template <typename T, int K, int VE>
__global__ __launch_bounds__(DR_BWD_THREADS) void dr_bwd_kernel(const T* __restrict__ noise, const float* __restrict__ c,
                                                                const float* __restrict__ z, const T* __restrict__ gout,
                                                                int64_t B, int N, int R, T* __restrict__ dpri) {
  __shared__ __attribute__((aligned(16))) float dz_s[K * DR_MAX_R];
  __shared__ float c_s[K * DR_MAX_N];
  const int t = threadIdx.x;
  const int lane = t & 63, wave = t >> 6;
  const int NV = R / VE;
  for (int64_t b = blockIdx.x; b < B; b += gridDim.x) {
    // squash backward: out = f(n2) z, f = n2 / ((1 + n2)(s + eps)), s = sqrt(n2):
    //   dz = f g + 2 f'(n2) (g . z) z,   f' = ((s + eps) - s (1 + n2) / 2) / ((1 + n2)(s + eps))^2   (divided twice: den^2 overflows early)
    for (int k = wave; k < K; k += DR_BWD_THREADS / 64) {
      const float* zr = z + (b * K + k) * R;
      const T* gr = gout + (b * K + k) * R;
      float n2 = 0.f, gz = 0.f;
      for (int rr = lane; rr < R; rr += 64) {
        n2 = fmaf(zr[rr], zr[rr], n2);
        gz = fmaf(to_f32(gr[rr]), zr[rr], gz);
      }
      n2 = group_sum_up<64>(n2);
      gz = group_sum_up<64>(gz);
      const float s = sqrtf(n2), den = (1.f + n2) * (s + 1e-8f);
      const float f = n2 > 0.f ? n2 / den : 0.f;
      const float f2 = n2 > 0.f ? 2.f * gz * ((s + 1e-8f) - 0.5f * s * (1.f + n2)) / den / den : 0.f;
      for (int rr = lane; rr < R; rr += 64) dz_s[k * R + rr] = f * to_f32(gr[rr]) + f2 * zr[rr];
    }
    for (int i = t; i < K * N; i += DR_BWD_THREADS) c_s[i] = c[b * K * N + i];
    __syncthreads();
    for (int i = t; i < N * NV; i += DR_BWD_THREADS) {
      const int n = i / NV, col = (i - n * NV) * VE;
      float x[K][VE], m[VE], s[VE], acc[VE];
#pragma unroll
      for (int j = 0; j < VE; ++j) m[j] = -INFINITY;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        dr_load<T, VE>(noise + ((b * K + k) * N + n) * R + col, x[k]);
        const float ck = c_s[k * N + n];
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          x[k][j] += ck;
          m[j] = fmaxf(m[j], x[k][j]);
        }
      }
#pragma unroll
      for (int j = 0; j < VE; ++j) s[j] = acc[j] = 0.f;
#pragma unroll
      for (int k = 0; k < K; ++k) {
#pragma unroll
        for (int j = 0; j < VE; ++j) {
          const float e = __expf(x[k][j] - m[j]);
          s[j] += e;
          acc[j] = fmaf(e, dz_s[k * R + col + j], acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < VE; ++j) acc[j] *= __builtin_amdgcn_rcpf(s[j]);
      dr_store<T, VE>(dpri + (b * N + n) * R + col, acc);
    }
    __syncthreads();      // dz_s / c_s are rewritten for the next sample
  }
}

// ---------------------------------------------------------------------------------------------
static int dr_path(int N, int R, int K, int dtype) {
  if (dtype != TRS_F32 && dtype != TRS_BF16) return 0;
  if (N < 1 || N > DR_MAX_N || R < 1 || R > DR_MAX_R || K < 1 || K > DR_MAX_K) return 0;
  return ((int64_t)R * dtype_size(dtype)) % 16 == 0 ? 1 : 2;
}

// rows of noise per staged chunk: all N where the sample fits beside the fixed part, else what DR_CHUNK_LDS (at least 8
// rows) or the whole LDS leaves
static int dr_chunk_rows(int N, int R, int K, int dtype) {
  const size_t fixed = dr_fixed_bytes(N, R, K), row = (size_t)K * R * dtype_size(dtype);
  if (fixed + row * N <= DR_MAX_LDS) return N;
  size_t rows = DR_CHUNK_LDS > fixed ? (DR_CHUNK_LDS - fixed) / row : 0;
  if (rows < 8) rows = (DR_MAX_LDS - fixed) / row;
  return (int)std::max<size_t>(1, std::min<size_t>(rows, (size_t)N));
}
static size_t dr_fwd_lds(int N, int R, int K, int dtype, int NC) {
  return dr_fixed_bytes(N, R, K) + (size_t)K * NC * R * dtype_size(dtype);
}

template <typename T, bool VEC>
static const void* dr_fwd_kernel_of(int K) {
  const void* kern = nullptr;      // dr_check admitted 1 <= K <= DR_MAX_K
  dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(K, [&](auto k_c) { kern = (const void*)dr_fwd_kernel<T, decltype(k_c)::value, VEC>; });
  return kern;
}

// persistent grid of the forward: the workgroups resident at once on the current device (asked of the runtime once per
// device, kernel and LDS size: the warm-up of a graph capture has then made every query); raises the kernel's LDS limit
// on that device where needed.  0: the runtime refused the LDS size.
static int dr_resident(const void* kern, size_t lds) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, size_t>, int> seen;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  const auto key = std::make_tuple(dev, kern, lds);
  const auto it = seen.find(key);
  if (it != seen.end()) return it->second;
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)DR_MAX_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return 0;
  }
  const int res = resident_blocks(kern, DR_THREADS, lds);
  (void)hipGetLastError();
  seen[key] = res;
  return res;
}

template <typename T, bool VEC>
static int dr_fwd_launch(const float* pri, const void* noise, int64_t B, int N, int R, int K, int iters, int dtype,
                         void* out, float* c_out, float* z_out, hipStream_t s) {
  const int NC = dr_chunk_rows(N, R, K, dtype);
  const size_t lds = dr_fwd_lds(N, R, K, dtype, NC);
  const void* kern = dr_fwd_kernel_of<T, VEC>(K);
  const int resident = dr_resident(kern, lds);
  TRS_REQUIRE(resident > 0, TRS_ELAUNCH, "dynamic_routing_fwd: %zu bytes of LDS per workgroup refused", lds);
  const int grid = (int)std::min<int64_t>(B, resident);
  const T* nz = (const T*)noise;
  T* o = (T*)out;
  int nc = NC;
  void* args[] = {&pri, &nz, &B, &N, &R, &iters, &nc, &o, &c_out, &z_out};
  (void)hipLaunchKernel(kern, dim3(grid), dim3(DR_THREADS), args, lds, s);
  return check_launch("dynamic_routing_fwd");
}

template <typename T, int VE>
static int dr_bwd_launch(const void* noise, const float* c, const float* z, const void* gout, int64_t B, int N, int R,
                         int K, void* dpri, hipStream_t s) {
  const int grid = stream_grid(B * DR_BWD_THREADS, DR_BWD_THREADS, 256 * 16);
  dispatch_int<1, 2, 3, 4, 5, 6, 7, 8>(K, [&](auto k_c) {
    hipLaunchKernelGGL((dr_bwd_kernel<T, decltype(k_c)::value, VE>), dim3(grid), dim3(DR_BWD_THREADS), 0, s,
                       (const T*)noise, c, z, (const T*)gout, B, N, R, (T*)dpri);
  });
  return check_launch("dynamic_routing_bwd");
}

static int dr_check(const char* what, int64_t B, int N, int R, int K, int dtype) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(B > 0, TRS_EINVAL, "%s: bad size B=%lld", what, (long long)B);
  TRS_REQUIRE(dr_path(N, R, K, dtype) != 0, TRS_ESHAPE,
              "%s: unsupported shape N=%d R=%d K=%d (1 <= N <= %d, 1 <= R <= %d, 1 <= K <= %d)", what, N, R, K, DR_MAX_N,
              DR_MAX_R, DR_MAX_K);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" int trs_dynamic_routing_path(int32_t N, int32_t R, int32_t K, int32_t dtype) { return dr_path(N, R, K, dtype); }

extern "C" int trs_dynamic_routing_fwd(const float* priors, const void* noise, int64_t B, int32_t N, int32_t R, int32_t K,
                                       int32_t num_iter, int32_t dtype, void* out, float* c_out, float* z_out,
                                       trs_stream_t stream) {
  if (B == 0) return TRS_OK;      // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(priors && noise && out, TRS_EINVAL, "dynamic_routing_fwd: NULL pointer");
  TRS_REQUIRE((c_out == nullptr) == (z_out == nullptr), TRS_EINVAL, "dynamic_routing_fwd: c_out and z_out go together");
  if (int rc = dr_check("dynamic_routing_fwd", B, N, R, K, dtype)) return rc;
  TRS_REQUIRE(num_iter >= 1, TRS_EINVAL, "dynamic_routing_fwd: bad num_iter=%d", num_iter);
  hipStream_t s = (hipStream_t)stream;
  const bool vec = dr_path(N, R, K, dtype) == 1 && aligned16(priors) && aligned16(noise);
  if (dtype == TRS_F32)
    return vec ? dr_fwd_launch<float, true>(priors, noise, B, N, R, K, num_iter, dtype, out, c_out, z_out, s)
               : dr_fwd_launch<float, false>(priors, noise, B, N, R, K, num_iter, dtype, out, c_out, z_out, s);
  return vec ? dr_fwd_launch<bf16_t, true>(priors, noise, B, N, R, K, num_iter, dtype, out, c_out, z_out, s)
             : dr_fwd_launch<bf16_t, false>(priors, noise, B, N, R, K, num_iter, dtype, out, c_out, z_out, s);
}

extern "C" int trs_dynamic_routing_bwd(const void* noise, const float* c, const float* z, const void* gout, int64_t B,
                                       int32_t N, int32_t R, int32_t K, int32_t dtype, void* dpri, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(noise && c && z && gout && dpri, TRS_EINVAL, "dynamic_routing_bwd: NULL pointer");
  if (int rc = dr_check("dynamic_routing_bwd", B, N, R, K, dtype)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = dr_path(N, R, K, dtype) == 1 && aligned16(noise) && aligned16(dpri);
  if (dtype == TRS_F32)
    return vec ? dr_bwd_launch<float, 4>(noise, c, z, gout, B, N, R, K, dpri, s)
               : dr_bwd_launch<float, 1>(noise, c, z, gout, B, N, R, K, dpri, s);
  return vec ? dr_bwd_launch<bf16_t, 8>(noise, c, z, gout, B, N, R, K, dpri, s)
             : dr_bwd_launch<bf16_t, 1>(noise, c, z, gout, B, N, R, K, dpri, s);
}
