// SENET / compose-excitation gate (layers/ctr/compose_excitation_network.py:72-109):
//   z[b,m] = mean_e x[b,m,e];  h = relu(W1 z + b1);  a = relu(W2 h + b2);  out[b,m,:] = x[b,m,:] * a[b,m]
// The reference runs AdaptiveAvgPool1d (reads the block), two tiny Linear + ReLU, and an einsum (reads the block, writes
// it); its backward forms the pooled gradient expanded to (B,M,E) and adds two input gradients.
//
// Fused family (M <= 64, 1 <= H <= M, rows of whole 16-byte vectors, a sample of at most 16 KiB, ReLU): a WAVE owns a
// sample.  The sample is M*L contiguous 16-byte vectors (L per row); lane l holds vectors l, l + 64, ... in registers (K per
// lane, a template parameter), so every load and store instruction of the wave covers 1 KiB of contiguous memory whatever
// L is.  Per-vector partial sums go through a per-wave LDS strip, lane m adds the L partials of row m, and the two layers
// run with lane = output unit: the input of a layer is broadcast lane by lane (v_readlane), the weights are fp32 in LDS,
// staged once per workgroup in quads of the input unit (a 16-byte read per four multiply-adds).  The rows are still in
// registers when the gates are known.  Forward: x read once, out written once (+ a (B,M), h (B,H) fp32 for a backward).
// Backward: x and g read once, dx written once; z is recomputed, the parameter gradients are accumulated per wave in LDS
// (plain read-modify-writes of the wave's own strip: no atomics, fixed order), folded per workgroup into one slab of the
// caller's workspace, and a finish kernel adds the slabs in a fixed order.  Every intermediate is fp32.
//
// General family (any M, E, activation; H = 0): three single-pass streaming kernels around an excitation the caller runs
// itself -- squeeze (z), scale forward (out = x * a), scale backward (ga = sum_e g x; dx = g a + gz / E).
#include <algorithm>

#include "trs_common.hpp"

namespace trs {

constexpr int SENET_MAX_M = 64;          // a lane per field
constexpr int SENET_MAX_VEC = 16;        // 16-byte vectors of a sample per lane: samples of up to 16 KiB
constexpr int SENET_MAX_BLOCKS = 1024;   // workgroups of the backward = slabs in the workspace (trs_senet_bwd_workspace_bytes)
constexpr int SENET_FIN_SEG = 8;         // finish kernel: slab segments summed side by side, then folded in order

// LDS written by some lanes of a wave and read by others of the SAME wave: the LDS serves a wave's instructions in order,
// the compiler must not move the accesses across this point
__device__ __forceinline__ void senet_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}
__device__ __forceinline__ float senet_lane(float v, int l) {      // l is uniform over the wave
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// ATen's relu: negative -> 0, NaN stays
__device__ __forceinline__ float senet_relu(float v) { return v <= 0.f ? 0.f : v; }

// the K vectors lane + 64 k of a sample (row[k] < 0: beyond the sample)
template <int K>
__device__ __forceinline__ void senet_load(uint4* v, const uint4* __restrict__ src, const int* row, int lane) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
    v[k] = make_uint4(0, 0, 0, 0);
    if (row[k] >= 0) v[k] = src[lane + 64 * k];
  }
}

// acc + sum_i w[i] * in[lane i]: w = this lane's column of a quad-packed matrix (quad q at w[q * stride]), nq quads
__device__ __forceinline__ float senet_dot4(const float4* w, int stride, int nq, float in, float acc) {
  for (int q = 0; q < nq; ++q) {
    const float4 c = w[q * stride];
    acc = __builtin_fmaf(c.x, senet_lane(in, 4 * q), acc);
    acc = __builtin_fmaf(c.y, senet_lane(in, 4 * q + 1), acc);
    acc = __builtin_fmaf(c.z, senet_lane(in, 4 * q + 2), acc);
    acc = __builtin_fmaf(c.w, senet_lane(in, 4 * q + 3), acc);
  }
  return acc;
}

template <typename T, int K>
__global__ __launch_bounds__(256) void senet_fwd_kernel(const uint4* __restrict__ x, const T* __restrict__ W1,
                                                        const T* __restrict__ b1, const T* __restrict__ W2,
                                                        const T* __restrict__ b2, int64_t B, int M, int H, int L,
                                                        float inv_E, uint4* __restrict__ out, float* __restrict__ a_out,
                                                        float* __restrict__ h_out) {
  extern __shared__ __align__(16) float senet_smem[];
  constexpr int VE = Vec16<T>::VE;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nvec = M * L;
  // weights in quads of the INPUT unit: one 16-byte LDS read per lane serves four multiply-adds, consecutive lanes read
  // consecutive quads.  (One 4-byte read, one v_readlane and the loop's scalar bookkeeping per multiply-add made the
  // excitation two thirds of the kernel's instructions, and the kernel is bound by instruction issue, not by HBM.)
  const int M4 = (M + 3) >> 2, H4 = (H + 3) >> 2;
  float4* W1q = reinterpret_cast<float4*>(senet_smem);      // [(m / 4) * H + h][m % 4] = W1[h, m], zero beyond M
  float4* W2q = W1q + M4 * H;                               // [(h / 4) * M + m][h % 4] = W2[m, h], zero beyond H
  float* sb1 = reinterpret_cast<float*>(W2q + H4 * M);
  float* sb2 = sb1 + H;
  float* svec = sb2 + M + wave * (nvec + 64);      // per wave: nvec partial sums, 64 gates
  float* sgate = svec + nvec;
  for (int i = threadIdx.x; i < 4 * M4 * H; i += blockDim.x) {
    const int h = (i >> 2) % H, m = ((i >> 2) / H) * 4 + (i & 3);
    reinterpret_cast<float*>(W1q)[i] = m < M ? to_f32(W1[h * M + m]) : 0.f;
  }
  for (int i = threadIdx.x; i < 4 * H4 * M; i += blockDim.x) {
    const int m = (i >> 2) % M, h = ((i >> 2) / M) * 4 + (i & 3);
    reinterpret_cast<float*>(W2q)[i] = h < H ? to_f32(W2[m * H + h]) : 0.f;
  }
  for (int i = threadIdx.x; i < H; i += blockDim.x) sb1[i] = to_f32(b1[i]);
  for (int i = threadIdx.x; i < M; i += blockDim.x) sb2[i] = to_f32(b2[i]);
  __syncthreads();
  int row[K];
#pragma unroll
  for (int k = 0; k < K; ++k) row[k] = (lane + 64 * k) < nvec ? (lane + 64 * k) / L : -1;
  const int hl = lane < H ? lane : H - 1, ml = lane < M ? lane : M - 1;
  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < B; b += (int64_t)gridDim.x * nw) {
    uint4 xv[K];
    senet_load<K>(xv, x + b * nvec, row, lane);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (row[k] >= 0) {
        float f[VE];
        Vec16<T>::unpack(xv[k], f);
        float s = 0.f;
#pragma unroll
        for (int e = 0; e < VE; ++e) s += f[e];
        svec[lane + 64 * k] = s;
      }
    }
    senet_wave_sync();
    float z = 0.f;
    if (lane < M) {
      for (int j = 0; j < L; ++j) z += svec[lane * L + j];
      z *= inv_E;
    }
    const float u = senet_dot4(W1q + hl, H, M4, z, sb1[hl]);        // lanes >= M hold z = 0
    const float hv = lane < H ? senet_relu(u) : 0.f;
    const float v = senet_dot4(W2q + ml, M, H4, hv, sb2[ml]);       // lanes >= H hold h = 0
    const float a = senet_relu(v);
    if (lane < M) {
      sgate[lane] = a;
      if (a_out != nullptr) a_out[b * M + lane] = a;
    }
    if (h_out != nullptr && lane < H) h_out[b * H + lane] = hv;
    senet_wave_sync();
    uint4* ob = out + b * nvec;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (row[k] >= 0) {
        const float ar = sgate[row[k]];
        float f[VE];
        Vec16<T>::unpack(xv[k], f);
#pragma unroll
        for (int e = 0; e < VE; ++e) f[e] *= ar;
        ob[lane + 64 * k] = Vec16<T>::pack(f);
      }
    }
    senet_wave_sync();                             // the next sample overwrites svec / sgate
  }
}

// slab layout (P = 2*M*H + M + H floats): [dW1 (H, M)][dW2 TRANSPOSED (H, M)][db1 (H)][db2 (M)]
template <typename T, int K>
__global__ __launch_bounds__(256) void senet_bwd_kernel(const uint4* __restrict__ x, const uint4* __restrict__ g,
                                                        const float* __restrict__ a_in, const float* __restrict__ h_in,
                                                        const T* __restrict__ W1, const T* __restrict__ W2, int64_t B,
                                                        int M, int H, int L, float inv_E, uint4* __restrict__ dx,
                                                        float* __restrict__ slabs) {
  extern __shared__ __align__(16) float senet_smem[];
  constexpr int VE = Vec16<T>::VE;
  const int nw = blockDim.x >> 6, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int nvec = M * L, MH = M * H, P = 2 * MH + M + H;
  const int M4 = (M + 3) >> 2, H4 = (H + 3) >> 2;
  float4* W2q = reinterpret_cast<float4*>(senet_smem);      // [(m / 4) * H + h][m % 4] = W2[m, h]   (gu = W2^T gv: lane = h)
  float4* W1q = W2q + M4 * H;                               // [(h / 4) * M + m][h % 4] = W1[h, m]   (gz = W1^T gu: lane = m)
  float* accs = reinterpret_cast<float*>(W1q + H4 * M);     // nw strips of P accumulators, slab layout
  float* acc = accs + wave * P;
  float* svx = accs + nw * P + wave * (2 * nvec + 128);      // per wave: sums of x, sums of g*x, (gate, gz/E) per row
  float* svg = svx + nvec;
  float* srow_a = svg + nvec;
  float* srow_z = srow_a + 64;
  for (int i = threadIdx.x; i < 4 * M4 * H; i += blockDim.x) {
    const int h = (i >> 2) % H, m = ((i >> 2) / H) * 4 + (i & 3);
    reinterpret_cast<float*>(W2q)[i] = m < M ? to_f32(W2[m * H + h]) : 0.f;
  }
  for (int i = threadIdx.x; i < 4 * H4 * M; i += blockDim.x) {
    const int m = (i >> 2) % M, h = ((i >> 2) / M) * 4 + (i & 3);
    reinterpret_cast<float*>(W1q)[i] = h < H ? to_f32(W1[h * M + m]) : 0.f;
  }
  const bool params = slabs != nullptr;
  if (params)
    for (int i = threadIdx.x; i < nw * P; i += blockDim.x) accs[i] = 0.f;
  __syncthreads();
  int row[K];
#pragma unroll
  for (int k = 0; k < K; ++k) row[k] = (lane + 64 * k) < nvec ? (lane + 64 * k) / L : -1;
  const int hl = lane < H ? lane : H - 1, ml = lane < M ? lane : M - 1;
  float db1 = 0.f, db2 = 0.f;
  for (int64_t b = (int64_t)blockIdx.x * nw + wave; b < B; b += (int64_t)gridDim.x * nw) {
    uint4 xv[K], gv[K];
    senet_load<K>(xv, x + b * nvec, row, lane);
    senet_load<K>(gv, g + b * nvec, row, lane);
    const float a = lane < M ? a_in[b * M + lane] : 0.f;
    const float hv = lane < H ? h_in[b * H + lane] : 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      if (row[k] >= 0) {
        float fx[VE], fg[VE];
        Vec16<T>::unpack(xv[k], fx);
        Vec16<T>::unpack(gv[k], fg);
        float sx = 0.f, sg = 0.f;
#pragma unroll
        for (int e = 0; e < VE; ++e) {
          sx += fx[e];
          sg += fg[e] * fx[e];
        }
        svx[lane + 64 * k] = sx;
        svg[lane + 64 * k] = sg;
      }
    }
    senet_wave_sync();
    float z = 0.f, ga = 0.f;
    if (lane < M) {
      for (int j = 0; j < L; ++j) {
        z += svx[lane * L + j];
        ga += svg[lane * L + j];
      }
      z *= inv_E;
    }
    const float gvv = a > 0.f ? ga : 0.f;                    // gradient at the second pre-activation (lane = m)
    float gu = senet_dot4(W2q + hl, H, M4, gvv, 0.f);        // lanes >= M hold gv = 0
    gu = (lane < H && hv > 0.f) ? gu : 0.f;                  // gradient at the first pre-activation (lane = h)
    const float gz = senet_dot4(W1q + ml, M, H4, gu, 0.f);   // lanes >= H hold gu = 0
    if (params) {
      for (int h = 0; h < H; ++h) {
        const float hh = senet_lane(hv, h);
        if (hh == 0.f) continue;                             // dead hidden unit: h = 0 and gu = 0, both terms vanish
        const float gh = senet_lane(gu, h);
        if (lane < M) {
          acc[h * M + lane] = __builtin_fmaf(gh, z, acc[h * M + lane]);                 // dW1[h, m] += gu[h] * z[m]
          acc[MH + h * M + lane] = __builtin_fmaf(gvv, hh, acc[MH + h * M + lane]);     // dW2[m, h] += gv[m] * h[h]
        }
      }
      db1 += gu;
      db2 += gvv;
    }
    if (dx != nullptr) {
      if (lane < M) {
        srow_a[lane] = a;
        srow_z[lane] = gz * inv_E;
      }
      senet_wave_sync();
      uint4* db = dx + b * nvec;
#pragma unroll
      for (int k = 0; k < K; ++k) {
        if (row[k] >= 0) {
          const float ra = srow_a[row[k]], rz = srow_z[row[k]];
          float fg[VE];
          Vec16<T>::unpack(gv[k], fg);
#pragma unroll
          for (int e = 0; e < VE; ++e) fg[e] = fg[e] * ra + rz;
          db[lane + 64 * k] = Vec16<T>::pack(fg);
        }
      }
    }
    senet_wave_sync();                                       // the next sample overwrites svx / svg / srow
  }
  if (params) {
    if (lane < H) acc[2 * MH + lane] = db1;
    if (lane < M) acc[2 * MH + H + lane] = db2;
    __syncthreads();
    float* slab = slabs + (size_t)blockIdx.x * P;
    for (int i = threadIdx.x; i < P; i += blockDim.x) {
      float s = 0.f;
      for (int w = 0; w < nw; ++w) s += accs[w * P + i];     // wave order: fixed
      slab[i] = s;
    }
  }
}

// p-th parameter gradient = sum of slab[j][p] over the nslab slabs: SENET_FIN_SEG threads take a contiguous share of the
// slabs each, then thread 0 of the parameter adds the shares in order
template <typename T>
__global__ __launch_bounds__(256) void senet_finish_kernel(const float* __restrict__ slabs, int nslab, int M, int H,
                                                           T* __restrict__ dW1, T* __restrict__ db1,
                                                           T* __restrict__ dW2, T* __restrict__ db2) {
  __shared__ float part[SENET_FIN_SEG][32];
  const int MH = M * H, P = 2 * MH + M + H;
  const int pl = threadIdx.x & 31, seg = threadIdx.x >> 5;
  const int p = blockIdx.x * 32 + pl;
  const int per = (nslab + SENET_FIN_SEG - 1) / SENET_FIN_SEG;
  const int j0 = seg * per, j1 = (j0 + per) < nslab ? (j0 + per) : nslab;
  float s = 0.f;
  if (p < P)
    for (int j = j0; j < j1; ++j) s += slabs[(size_t)j * P + p];
  part[seg][pl] = s;
  __syncthreads();
  if (seg != 0 || p >= P) return;
  float t = 0.f;
#pragma unroll
  for (int q = 0; q < SENET_FIN_SEG; ++q) t += part[q][pl];
  if (p < MH) {
    if (dW1 != nullptr) dW1[p] = from_f32<T>(t);
  } else if (p < 2 * MH) {
    const int i = p - MH, h = i / M, m = i - h * M;          // slab holds dW2 as (H, M)
    if (dW2 != nullptr) dW2[m * H + h] = from_f32<T>(t);
  } else if (p < 2 * MH + H) {
    if (db1 != nullptr) db1[p - 2 * MH] = from_f32<T>(t);
  } else {
    if (db2 != nullptr) db2[p - 2 * MH - H] = from_f32<T>(t);
  }
}

// the two weight matrices in quads of the input unit, zero-padded to whole quads
static size_t senet_quad_floats(int M, int H) { return (size_t)4 * (((M + 3) / 4) * H + ((H + 3) / 4) * M); }
static size_t senet_fwd_lds(int M, int H, int nvec, int nw) {
  return sizeof(float) * (senet_quad_floats(M, H) + M + H + (size_t)nw * (nvec + 64));
}
static size_t senet_bwd_lds(int M, int H, int nvec, int nw) {
  const size_t P = (size_t)2 * M * H + M + H;
  return sizeof(float) * (senet_quad_floats(M, H) + nw * P + (size_t)nw * (2 * nvec + 128));
}
// waves per workgroup: four, fewer when the accumulator strips of four do not fit 64 KiB of LDS
static int senet_bwd_waves(int M, int H, int nvec) {
  int nw = 4;
  while (nw > 1 && senet_bwd_lds(M, H, nvec, nw) > 64 * 1024) nw >>= 1;
  return nw;
}
static int senet_vec_per_lane(int nvec) {
  const int k = (nvec + 63) / 64;
  static const int steps[] = {1, 2, 4, 5, 8, 10, 16};
  for (int s : steps)
    if (k <= s) return s;
  return -1;
}

template <typename T, int K>
static int senet_fwd_launch(const void* x, const void* W1, const void* b1, const void* W2, const void* b2, int64_t B,
                            int M, int H, int E, void* out, float* a_out, float* h_out, hipStream_t s) {
  const int L = E * (int)sizeof(T) / 16, nw = 4;
  const size_t lds = senet_fwd_lds(M, H, M * L, nw);
  auto kern = senet_fwd_kernel<T, K>;
  static size_t cap_lds = ~(size_t)0;
  static int cap = 0;
  if (cap_lds != lds * 8 + nw) { cap = resident_blocks((const void*)kern, 64 * nw, lds); cap_lds = lds * 8 + nw; }
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + nw - 1) / nw, cap));
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, s, (const uint4*)x, (const T*)W1, (const T*)b1, (const T*)W2,
                     (const T*)b2, B, M, H, L, 1.f / (float)E, (uint4*)out, a_out, h_out);
  return check_launch("senet_fwd");
}

template <typename T, int K>
static int senet_bwd_launch(const void* x, const void* g, const float* a, const float* h, const void* W1, const void* W2,
                            int64_t B, int M, int H, int E, void* dx, void* dW1, void* db1, void* dW2, void* db2,
                            float* slabs, hipStream_t s) {
  const int L = E * (int)sizeof(T) / 16, nvec = M * L;
  const int nw = senet_bwd_waves(M, H, nvec);
  const size_t lds = senet_bwd_lds(M, H, nvec, nw);
  auto kern = senet_bwd_kernel<T, K>;
  static bool attr_set = false;       // more than 64 KiB of dynamic LDS needs the attribute
  if (!attr_set && lds > 64 * 1024) {
    if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
      return check_launch("senet_bwd: LDS attribute");
    attr_set = true;
  }
  static size_t cap_lds = ~(size_t)0;
  static int cap = 0;
  if (cap_lds != lds * 8 + nw) { cap = resident_blocks((const void*)kern, 64 * nw, lds); cap_lds = lds * 8 + nw; }
  // one round of workgroups: each keeps its accumulators for the whole launch and leaves one slab
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((B + nw - 1) / nw, std::min(cap, SENET_MAX_BLOCKS)));
  const bool params = dW1 || db1 || dW2 || db2;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * nw), lds, s, (const uint4*)x, (const uint4*)g, a, h, (const T*)W1,
                     (const T*)W2, B, M, H, L, 1.f / (float)E, (uint4*)dx, params ? slabs : nullptr);
  if (params) {
    const int P = 2 * M * H + M + H;
    hipLaunchKernelGGL(senet_finish_kernel<T>, dim3((P + 31) / 32), dim3(32 * SENET_FIN_SEG), 0, s, slabs, grid, M, H,
                       (T*)dW1, (T*)db1, (T*)dW2, (T*)db2);
  }
  return check_launch("senet_bwd");
}

// ---------------------------------------------------------------------------------------------
// general family: rows = B*M rows of E values.  A group of G lanes (a power of two, <= 64) owns a row and strides it in
// units of U values: U = a 16-byte vector when the rows are whole vectors (VEC), else one element.

template <typename T, bool VEC>
struct SenetUnit {
  static constexpr int VE = VEC ? Vec16<T>::VE : 1;
  static __device__ __forceinline__ void load(const T* p, float* f) {
    if constexpr (VEC) Vec16<T>::unpack(*reinterpret_cast<const uint4*>(p), f);
    else f[0] = to_f32(*p);
  }
  static __device__ __forceinline__ void store(T* p, const float* f) {
    if constexpr (VEC) *reinterpret_cast<uint4*>(p) = Vec16<T>::pack(f);
    else *p = from_f32<T>(f[0]);
  }
};

// z[r] = mean_e x[r, e]   (g == nullptr)      |      ga[r] = sum_e g[r, e] * x[r, e]
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void senet_rowsum_kernel(const T* __restrict__ x, const T* __restrict__ g,
                                                           int64_t rows, int E, int log2g, float scale,
                                                           float* __restrict__ dst) {
  using U = SenetUnit<T, VEC>;
  constexpr int VE = U::VE;
  const int G = 1 << log2g, units = E / VE;
  const int gl = threadIdx.x & (G - 1);
  const int64_t groups = ((int64_t)gridDim.x * blockDim.x) >> log2g;
  const int64_t first = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> log2g;
  const int64_t trips = (rows + groups - 1) / groups;        // the same for every lane of a wave: shuffles stay convergent
  for (int64_t t = 0; t < trips; ++t) {
    const int64_t r = first + t * groups;
    float s = 0.f;
    if (r < rows) {
      for (int u = gl; u < units; u += G) {
        float fx[VE];
        U::load(x + r * E + (int64_t)u * VE, fx);
        if (g != nullptr) {
          float fg[VE];
          U::load(g + r * E + (int64_t)u * VE, fg);
#pragma unroll
          for (int e = 0; e < VE; ++e) s += fg[e] * fx[e];
        } else {
#pragma unroll
          for (int e = 0; e < VE; ++e) s += fx[e];
        }
      }
    }
    s = group_sum_up(s, G);
    if (r < rows && gl == 0) dst[r] = s * scale;
  }
}

// dst[r, e] = src[r, e] * a[r] + add[r] * add_scale      (src == nullptr: the second term alone; add == nullptr: the first)
template <typename T, bool VEC>
__global__ __launch_bounds__(256) void senet_rowscale_kernel(const T* __restrict__ src, const float* __restrict__ a,
                                                             const float* __restrict__ add, float add_scale,
                                                             int64_t rows, int E, T* __restrict__ dst) {
  using U = SenetUnit<T, VEC>;
  constexpr int VE = U::VE;
  const int units = E / VE;
  const int64_t total = rows * units;
  const bool f32 = total < ((int64_t)1 << 32);
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const int64_t r = udiv_fast(t, units, f32);
    float f[VE];
#pragma unroll
    for (int e = 0; e < VE; ++e) f[e] = 0.f;
    float ar = 0.f;
    if (src != nullptr) {
      U::load(src + t * VE, f);
      ar = a[r];
    }
    const float c = add != nullptr ? add[r] * add_scale : 0.f;
#pragma unroll
    for (int e = 0; e < VE; ++e) f[e] = f[e] * ar + c;
    U::store(dst + t * VE, f);
  }
}

static int senet_log2_group(int units) {
  int l = 0;
  while ((1 << l) < units && l < 6) ++l;
  return l;
}

template <typename T>
static int senet_rowsum_launch(const void* x, const void* g, int64_t rows, int E, float scale, float* dst,
                               hipStream_t s, const char* what) {
  const bool vec = (E * (int)sizeof(T)) % 16 == 0 && aligned16(x) && aligned16(g);
  const int units = vec ? E * (int)sizeof(T) / 16 : E;
  const int lg = senet_log2_group(units);
  const int grid = stream_grid(rows << lg, 256, 256 * 16);
  if (vec)
    hipLaunchKernelGGL((senet_rowsum_kernel<T, true>), dim3(grid), dim3(256), 0, s, (const T*)x, (const T*)g, rows, E, lg,
                       scale, dst);
  else
    hipLaunchKernelGGL((senet_rowsum_kernel<T, false>), dim3(grid), dim3(256), 0, s, (const T*)x, (const T*)g, rows, E,
                       lg, scale, dst);
  return check_launch(what);
}

template <typename T>
static int senet_rowscale_launch(const void* src, const float* a, const float* add, float add_scale, int64_t rows, int E,
                                 void* dst, hipStream_t s, const char* what) {
  const bool vec = (E * (int)sizeof(T)) % 16 == 0 && aligned16(src) && aligned16(dst);
  const int units = vec ? E * (int)sizeof(T) / 16 : E;
  const int grid = stream_grid(rows * units, 256, 256 * 16);
  if (vec)
    hipLaunchKernelGGL((senet_rowscale_kernel<T, true>), dim3(grid), dim3(256), 0, s, (const T*)src, a, add, add_scale,
                       rows, E, (T*)dst);
  else
    hipLaunchKernelGGL((senet_rowscale_kernel<T, false>), dim3(grid), dim3(256), 0, s, (const T*)src, a, add, add_scale,
                       rows, E, (T*)dst);
  return check_launch(what);
}

static int senet_check_fused(const char* what, int64_t B, int M, int H, int E, int dtype) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(B >= 0 && M > 0 && H >= 0 && E > 0, TRS_EINVAL, "%s: bad size B=%lld M=%d H=%d E=%d", what, (long long)B,
              M, H, E);
  TRS_REQUIRE(M <= SENET_MAX_M && H >= 1 && H <= M, TRS_ESHAPE,
              "%s: the fused family needs M <= %d and 1 <= H <= M (M=%d H=%d); use the squeeze / scale entries", what,
              SENET_MAX_M, M, H);
  const int row_bytes = E * dtype_size(dtype);
  TRS_REQUIRE(row_bytes % 16 == 0, TRS_ESHAPE, "%s: rows of %d bytes are not whole 16-byte vectors (E=%d)", what,
              row_bytes, E);
  TRS_REQUIRE((int64_t)M * row_bytes <= (int64_t)SENET_MAX_VEC * 64 * 16, TRS_ESHAPE,
              "%s: a sample of %lld bytes exceeds the %d a wave holds in registers", what, (long long)M * row_bytes,
              SENET_MAX_VEC * 64 * 16);
  return TRS_OK;
}

static int senet_check_rows(const char* what, int64_t B, int M, int E, int dtype) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(B >= 0 && M > 0 && E > 0, TRS_EINVAL, "%s: bad size B=%lld M=%d E=%d", what, (long long)B, M, E);
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

// K = 16-byte vectors of a sample per lane (senet_vec_per_lane): senet_check_fused has bounded the sample by
// SENET_MAX_VEC per lane, so it is one of the seven steps
template <typename T, typename F>
static int senet_dispatch_k(int M, int E, F&& f) {
  int rc = TRS_OK;
  dispatch_int<1, 2, 4, 5, 8, 10, 16>(senet_vec_per_lane(M * (E * (int)sizeof(T) / 16)), [&](auto k_c) { rc = f(k_c); });
  return rc;
}

extern "C" int trs_senet_fused_supported(int32_t M, int32_t H, int32_t E, int32_t dtype) {
  if (dtype != TRS_F32 && dtype != TRS_BF16) return 0;
  if (M <= 0 || M > SENET_MAX_M || H < 1 || H > M || E <= 0) return 0;
  const int row_bytes = E * dtype_size(dtype);
  return row_bytes % 16 == 0 && (int64_t)M * row_bytes <= (int64_t)SENET_MAX_VEC * 64 * 16;
}

extern "C" int trs_senet_fwd(const void* x, const void* W1, const void* b1, const void* W2, const void* b2, int64_t B,
                             int32_t M, int32_t H, int32_t E, int32_t dtype, void* out, float* gates, float* hidden,
                             trs_stream_t stream) {
  TRS_REQUIRE(x && W1 && b1 && W2 && b2 && out, TRS_EINVAL, "senet_fwd: NULL pointer");
  TRS_REQUIRE((gates == nullptr) == (hidden == nullptr), TRS_EINVAL,
              "senet_fwd: gates and hidden are written together (both or neither)");
  if (int rc = senet_check_fused("senet_fwd", B, M, H, E, dtype)) return rc;
  TRS_REQUIRE(aligned16(x) && aligned16(out), TRS_EALIGN, "senet_fwd: x / out not 16-byte aligned");
  if (B == 0) return TRS_OK;
  hipStream_t s = (hipStream_t)stream;
  auto run = [&](auto t) {
    using T = decltype(t);
    return senet_dispatch_k<T>(M, E, [&](auto k_c) {
      return senet_fwd_launch<T, decltype(k_c)::value>(x, W1, b1, W2, b2, B, M, H, E, out, gates, hidden, s);
    });
  };
  return dtype == TRS_F32 ? run(float{}) : run(bf16_t{});
}

extern "C" size_t trs_senet_bwd_workspace_bytes(int64_t B, int32_t M, int32_t H) {
  if (B < 0 || M <= 0 || H < 0) return 0;
  return (size_t)SENET_MAX_BLOCKS * ((size_t)2 * M * H + M + H) * sizeof(float);
}

extern "C" int trs_senet_bwd(const void* x, const void* g, const float* gates, const float* hidden, const void* W1,
                             const void* W2, int64_t B, int32_t M, int32_t H, int32_t E, int32_t dtype, void* dx,
                             void* dW1, void* db1, void* dW2, void* db2, void* workspace, size_t ws_bytes,
                             trs_stream_t stream) {
  TRS_REQUIRE(x && g && gates && hidden && W1 && W2, TRS_EINVAL, "senet_bwd: NULL pointer");
  if (int rc = senet_check_fused("senet_bwd", B, M, H, E, dtype)) return rc;
  TRS_REQUIRE(aligned16(x) && aligned16(g) && aligned16(dx), TRS_EALIGN, "senet_bwd: x / g / dx not 16-byte aligned");
  const bool params = dW1 || db1 || dW2 || db2;
  TRS_REQUIRE(!params || (workspace != nullptr && ws_bytes >= trs_senet_bwd_workspace_bytes(B, M, H)), TRS_EWORKSPACE,
              "senet_bwd: workspace %zu < %zu", workspace ? ws_bytes : (size_t)0,
              trs_senet_bwd_workspace_bytes(B, M, H));
  if (B == 0 && !params) return TRS_OK;
  hipStream_t s = (hipStream_t)stream;
  float* slabs = (float*)workspace;
  auto run = [&](auto t) {
    using T = decltype(t);
    return senet_dispatch_k<T>(M, E, [&](auto k_c) {
      return senet_bwd_launch<T, decltype(k_c)::value>(x, g, gates, hidden, W1, W2, B, M, H, E, dx, dW1, db1, dW2, db2,
                                                       slabs, s);
    });
  };
  return dtype == TRS_F32 ? run(float{}) : run(bf16_t{});
}

extern "C" int trs_senet_squeeze(const void* x, int64_t B, int32_t M, int32_t E, int32_t dtype, float* z,
                                 trs_stream_t stream) {
  TRS_REQUIRE(x && z, TRS_EINVAL, "senet_squeeze: NULL pointer");
  if (int rc = senet_check_rows("senet_squeeze", B, M, E, dtype)) return rc;
  if (B == 0) return TRS_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32)
    return senet_rowsum_launch<float>(x, nullptr, B * M, E, 1.f / (float)E, z, s, "senet_squeeze");
  return senet_rowsum_launch<bf16_t>(x, nullptr, B * M, E, 1.f / (float)E, z, s, "senet_squeeze");
}

extern "C" int trs_senet_scale_fwd(const void* x, const float* a, int64_t B, int32_t M, int32_t E, int32_t dtype,
                                   void* out, trs_stream_t stream) {
  TRS_REQUIRE(x && a && out, TRS_EINVAL, "senet_scale_fwd: NULL pointer");
  if (int rc = senet_check_rows("senet_scale_fwd", B, M, E, dtype)) return rc;
  if (B == 0) return TRS_OK;
  hipStream_t s = (hipStream_t)stream;
  if (dtype == TRS_F32)
    return senet_rowscale_launch<float>(x, a, nullptr, 0.f, B * M, E, out, s, "senet_scale_fwd");
  return senet_rowscale_launch<bf16_t>(x, a, nullptr, 0.f, B * M, E, out, s, "senet_scale_fwd");
}

extern "C" int trs_senet_scale_bwd(const void* x, const void* g, const float* a, const float* gz, int64_t B, int32_t M,
                                   int32_t E, int32_t dtype, float* ga, void* dx, trs_stream_t stream) {
  TRS_REQUIRE(ga || dx, TRS_EINVAL, "senet_scale_bwd: NULL pointer (neither ga nor dx asked for)");
  TRS_REQUIRE(!ga || (x && g), TRS_EINVAL, "senet_scale_bwd: NULL pointer (ga needs x and g)");
  TRS_REQUIRE(!dx || gz || (g && a), TRS_EINVAL, "senet_scale_bwd: NULL pointer (dx needs g and a, or gz)");
  TRS_REQUIRE(!dx || !g || a, TRS_EINVAL, "senet_scale_bwd: NULL pointer (g without the gates a)");
  if (int rc = senet_check_rows("senet_scale_bwd", B, M, E, dtype)) return rc;
  if (B == 0) return TRS_OK;
  hipStream_t s = (hipStream_t)stream;
  const int64_t rows = B * M;
  const float inv_E = 1.f / (float)E;
  int rc = TRS_OK;
  if (ga) {
    rc = dtype == TRS_F32 ? senet_rowsum_launch<float>(x, g, rows, E, 1.f, ga, s, "senet_scale_bwd")
                          : senet_rowsum_launch<bf16_t>(x, g, rows, E, 1.f, ga, s, "senet_scale_bwd");
    if (rc != TRS_OK) return rc;
  }
  if (dx)
    rc = dtype == TRS_F32 ? senet_rowscale_launch<float>(g, a, gz, inv_E, rows, E, dx, s, "senet_scale_bwd")
                          : senet_rowscale_launch<bf16_t>(g, a, gz, inv_E, rows, E, dx, s, "senet_scale_bwd");
  return rc;
}
