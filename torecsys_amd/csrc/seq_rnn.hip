// An ordered (B, L) list of ids through a one-layer RNN / LSTM / GRU, then pooled over the live steps: the reference's
// SequenceIndicesEmbedding (inputs/base/sequence_indices_emb.py:128-171: sort -> aten::embedding -> pack_padded_sequence
// -> nn.LSTM / nn.GRU / nn.RNN -> pad_packed_sequence -> un-sort -> pooling).  hidden_size == E, one layer, one direction,
// biases -- every instance the reference can construct.  Per sample b with len = lengths[b] and t < len
// (x_t = table[idx[b, t]], h_{-1} = c_{-1} = 0, PyTorch's gate order):
//   rnn  (0): h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh)
//   lstm (1): [i f g o] = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh;  c_t = s(f) c_{t-1} + s(i) tanh(g);  h_t = s(o) tanh(c_t)
//   gru  (2): r = s(W_ir x + b_ir + W_hr h + b_hr), z likewise, n = tanh(W_in x + b_in + r (W_hn h + b_hn)),
//             h_t = (1 - z) n + z h_{t-1}
//   mode 0: out[b] = scale * sum_{t < len} h_t;   mode 1: out[b, t] = h_t, zero from t = len on.
// Steps t >= len take no part and get no gradient: no sort, no packing, no host read of the lengths.
//
// One workgroup of 256 threads takes a tile of M samples through all steps (M = 4 * 256 / EJ, EJ = E rounded up to a
// power of two: 16 samples at E = 64).  A thread owns ONE hidden unit j of FOUR samples: all G gates of that unit are its
// own accumulators, so the cell update needs no exchange, and a weight it loads serves four FMAs.  x_t and h_{t-1} of the
// tile live in LDS as fp32 (a wave reads them as broadcasts); the weights are read through L2 from a transposed fp32 image
// [k][g E + j] that a small kernel writes into the caller's workspace first (lanes of a wave then read adjacent words; in
// the parameters' own (G E, E) layout a wave's load touches 64 cache lines).  fp32 FMA throughout; h is rounded to the
// value dtype once per step, as the next step's operand and as the saved state, so that the backward recomputes the
// forward's gates from what was saved.  Two barriers per step.  That is path 1 (trs_seq_rnn_path).  Path 2, bf16 at E = 16,
// 32 or 64, is the same pair of kernels with the two products on the matrix cores and the weights in registers: see "the
// matrix-core path" below.
//
// Backward: the same tile, t from the tile's longest length - 1 down to 0, the chain dh (and dc) in the owning thread's
// registers.  Per step the gates are recomputed from x_t, the saved h_{t-1} (and c_{t-1}); the pre-activation gradients
// go to `dgates` (B, L, G E) in the value dtype and, unrounded, to LDS, from which dh_{t-1} = dgates_h W_hh is formed
// (W_hh in its own layout: k is the lane index).  The sums over the batch (dX, dW_ih, dW_hh, the biases) are the caller's
// GEMMs.  No atomics, samples are dealt to workgroups statically, every sum runs in a fixed order: reproducible bits.
#include <algorithm>

#include "trs_common.hpp"

namespace trs {

constexpr int SR_RNN = 0, SR_LSTM = 1, SR_GRU = 2;
constexpr int SR_THREADS = 256;
constexpr int SR_S = 4;                 // samples per thread
constexpr int SR_MAX_E = 128;
constexpr int SR_TILE_WORDS = 1024;     // M * E <= (256 / EJ) * 4 * E <= 1024

__host__ __device__ constexpr int sr_gates(int cell) { return cell == SR_LSTM ? 4 : (cell == SR_GRU ? 3 : 1); }
// accumulators per hidden unit: the GRU keeps the two halves of its n gate apart (r multiplies the hidden half)
__host__ __device__ constexpr int sr_accs(int cell) { return cell == SR_RNN ? 1 : 4; }

static int sr_path(int cell, int L, int E, int dtype) {
  if (cell < SR_RNN || cell > SR_GRU || (dtype != TRS_F32 && dtype != TRS_BF16)) return 0;
  if (L < 1 || E < 1 || E > SR_MAX_E) return 0;
  if (dtype == TRS_BF16 && (E == 16 || E == 32 || E == 64)) return 2;
  return 1;
}
static int sr_pow2_above(int E) {
  int p = 1;
  while (p < E) p <<= 1;
  return p;
}

__device__ __forceinline__ int64_t sr_load_int(const void* p, int64_t i, bool is32) {
  return is32 ? (int64_t)((const int32_t*)p)[i] : ((const int64_t*)p)[i];
}

// wt[which][k][r] = w_which[r][k] as fp32 (which = 0: w_ih, 1: w_hh; r < G E, k < E)
template <typename T>
__global__ void sr_prep_kernel(const T* __restrict__ w_ih, const T* __restrict__ w_hh, int E, int GE,
                               float* __restrict__ wt) {
  const int n = GE * E;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * n; i += gridDim.x * blockDim.x) {
    const int which = i / n, rem = i - which * n;
    const int k = rem / GE, r = rem - k * GE;
    wt[i] = to_f32((which ? w_hh : w_ih)[r * E + k]);
  }
}

// *scale = 1 / max_b clamp(lengths[b], 0, L) (0 when every length is 0) or 1: one workgroup, no host read
__global__ void sr_scale_kernel(const void* __restrict__ lens, int len32, int64_t B, int L, int average,
                                float* __restrict__ scale) {
  __shared__ int red[SR_THREADS];
  int mx = 0;
  if (average)
    for (int64_t b = threadIdx.x; b < B; b += SR_THREADS) {
      int64_t l = sr_load_int(lens, b, len32 != 0);
      l = l < 0 ? 0 : (l > L ? L : l);
      mx = max(mx, (int)l);
    }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = SR_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] = max(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *scale = average ? (red[0] > 0 ? 1.f / (float)red[0] : 0.f) : 1.f;
}

// the tile's clamped lengths into s_len (0 for b >= B); returns the longest.  A length outside [1, L] raises the flag.
__device__ __forceinline__ int sr_tile_lengths(int* s_len, int* s_red, const void* lens, bool len32, int64_t b0, int M,
                                               int64_t B, int L, int32_t* err_flag) {
  int mx = 0;
  for (int m = threadIdx.x; m < M; m += SR_THREADS) {
    int l = 0;
    if (b0 + m < B) {
      const int64_t v = sr_load_int(lens, b0 + m, len32);
      if (v < 1 || v > L) {
        if (err_flag != nullptr) *err_flag = 1;
      }
      l = (int)(v < 0 ? 0 : (v > L ? L : v));
    }
    s_len[m] = l;
    mx = max(mx, l);
  }
  s_red[threadIdx.x] = mx;
  __syncthreads();
  for (int s = SR_THREADS / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) s_red[threadIdx.x] = max(s_red[threadIdx.x], s_red[threadIdx.x + s]);
    __syncthreads();
  }
  return s_red[0];
}

// xs[m][:] = table[idx[b0 + m, t]] for the samples live at step t, zero rows for the others; an id outside [0, V) reads
// as a zero row and raises the flag
template <typename T>
__device__ __forceinline__ void sr_gather_step(float* xs, const int* s_len, const T* __restrict__ table, int64_t V, int E,
                                               const void* idx, bool idx32, int64_t b0, int M, int L, int t,
                                               int32_t* err_flag) {
  for (int i = threadIdx.x; i < M * E; i += SR_THREADS) {
    const int m = i / E, e = i - m * E;
    float v = 0.f;
    if (t < s_len[m]) {
      const int64_t r = sr_load_int(idx, (b0 + m) * L + t, idx32);
      if (r < 0 || r >= V) {
        if (err_flag != nullptr && e == 0) *err_flag = 1;
      } else {
        v = to_f32(table[r * E + e]);
      }
    }
    xs[i] = v;
  }
}

// acc[a][s] += sum_k W_ih[g E + j, k] x_s[k] + W_hh[g E + j, k] h_s[k]; one sequential sum over k per accumulator
template <int CELL>
__device__ __forceinline__ void sr_preact(float (&acc)[sr_accs(CELL)][SR_S], const float* __restrict__ wt,
                                          const float* xs, const float* hs, int E, int j, int m0) {
  constexpr int G = sr_gates(CELL);
  const int GE = G * E;
  const float* wi = wt + j;
  const float* wh = wt + (size_t)GE * E + j;
  for (int k = 0; k < E; ++k) {
    float a[G], c[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
      a[g] = wi[k * GE + g * E];
      c[g] = wh[k * GE + g * E];
    }
#pragma unroll
    for (int s = 0; s < SR_S; ++s) {
      const float x = xs[(m0 + s) * E + k], h = hs[(m0 + s) * E + k];
#pragma unroll
      for (int g = 0; g < G; ++g) {
        if (CELL == SR_GRU && g == 2) {
          acc[2][s] = fmaf(a[2], x, acc[2][s]);
          acc[3][s] = fmaf(c[2], h, acc[3][s]);
        } else {
          acc[g][s] = fmaf(c[g], h, fmaf(a[g], x, acc[g][s]));
        }
      }
    }
  }
}

// ---- the matrix-core path (bf16, ME = E in {16, 32, 64}) ------------------------------------------------------------
// mfma_f32_16x16x32_bf16: lane l = 16 q + r holds A[row r][k = 8 q ..+7], B[k = 8 q ..+7][col r] and D[row 4 q ..+3][col r].
// With the samples as rows and the hidden units as columns a lane's four results are ONE unit of FOUR samples -- the
// ownership of the vector path -- so everything around the two products is shared.  Wave w takes the 16 units of tile
// w % (E / 16) for the 16 samples of tile w / (E / 16).  The weights are bf16 already: each lane keeps its B fragments of
// [W_ih | W_hh] (and, in the backward, of W_hh by rows) in registers for the whole tile of samples, loaded once.
typedef __attribute__((ext_vector_type(8))) __bf16 sr_bf16x8;
typedef __attribute__((ext_vector_type(4))) float sr_f32x4;
typedef __attribute__((ext_vector_type(4))) unsigned sr_u32x4;

// eight fp32 words of LDS that hold bf16 values (looked-up rows, the rounded h, the rounded gate gradients) -> an A fragment
__device__ __forceinline__ sr_u32x4 sr_afrag(const float* p) {
  const float4 lo = *reinterpret_cast<const float4*>(p), hi = *reinterpret_cast<const float4*>(p + 4);
  return sr_u32x4{f32x2_to_bf16x2_bits(lo.x, lo.y), f32x2_to_bf16x2_bits(lo.z, lo.w), f32x2_to_bf16x2_bits(hi.x, hi.y),
                  f32x2_to_bf16x2_bits(hi.z, hi.w)};
}

// wf[a][kk]: accumulator a's weights for k = 32 kk + 8 q ..+7 of [x | h] (k < E: W_ih, else W_hh).  The GRU's n gate
// keeps its two halves apart: accumulator 2 has zeros on the h side, accumulator 3 zeros on the x side.
template <int CELL, int ME>
__device__ __forceinline__ void sr_load_wfrags(sr_u32x4 (&wf)[sr_accs(CELL)][ME / 16], const bf16_t* __restrict__ w_ih,
                                               const bf16_t* __restrict__ w_hh, int j, int q) {
#pragma unroll
  for (int a = 0; a < sr_accs(CELL); ++a)
#pragma unroll
    for (int kk = 0; kk < ME / 16; ++kk) {
      const int k = 32 * kk + 8 * q;
      const bool inx = k < ME;
      const int g = (CELL == SR_GRU && a == 3) ? 2 : a;
      const bool use = CELL != SR_GRU || a < 2 || (a == 2 ? inx : !inx);
      const bf16_t* src = (inx ? w_ih : w_hh) + (size_t)(g * ME + j) * ME + (inx ? k : k - ME);
      wf[a][kk] = use ? *reinterpret_cast<const sr_u32x4*>(src) : sr_u32x4{0u, 0u, 0u, 0u};
    }
}

// acc[a][s] += the pre-activations of unit j for the lane's four samples; row = the sample 16 st + r of the A fragment
template <int CELL, int ME>
__device__ __forceinline__ void sr_preact_mfma(float (&acc)[sr_accs(CELL)][SR_S], const sr_u32x4 (&wf)[sr_accs(CELL)][ME / 16],
                                               const float* xs, const float* hs, int row, int q) {
#pragma unroll
  for (int kk = 0; kk < ME / 16; ++kk) {
    const int k = 32 * kk + 8 * q;
    const sr_u32x4 au = sr_afrag(k < ME ? xs + row * ME + k : hs + row * ME + (k - ME));
#pragma unroll
    for (int a = 0; a < sr_accs(CELL); ++a) {
      if (CELL == SR_GRU && a == 2 && 32 * kk >= ME) continue;            // all zeros: the h side of the x half
      if (CELL == SR_GRU && a == 3 && 32 * kk + 32 <= ME) continue;       // all zeros: the x side of the h half
      sr_f32x4 c = {acc[a][0], acc[a][1], acc[a][2], acc[a][3]};
      c = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sr_bf16x8, au), __builtin_bit_cast(sr_bf16x8, wf[a][kk]),
                                                  c, 0, 0, 0);
#pragma unroll
      for (int s = 0; s < SR_S; ++s) acc[a][s] = c[s];
    }
  }
}

// the backward's second product, dh_{t-1} = dgates_h W_hh: wb[kk] holds W_hh[k = 32 kk + 8 q ..+7][j] (zeros from G E on)
template <int CELL, int ME>
__device__ __forceinline__ void sr_load_wfrags_t(sr_u32x4 (&wb)[(sr_gates(CELL) * ME + 31) / 32],
                                                 const bf16_t* __restrict__ w_hh, int j, int q) {
  constexpr int GE = sr_gates(CELL) * ME;
#pragma unroll
  for (int kk = 0; kk < (GE + 31) / 32; ++kk) {
    const int k = 32 * kk + 8 * q;
    uint32_t u[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t lo = k < GE ? w_hh[(k + 2 * i) * ME + j].v : 0u, hi = k < GE ? w_hh[(k + 2 * i + 1) * ME + j].v : 0u;
      u[i] = lo | (hi << 16);
    }
    wb[kk] = sr_u32x4{u[0], u[1], u[2], u[3]};
  }
}

template <typename T, int CELL>
__device__ __forceinline__ void sr_load_bias(float (&bias)[sr_accs(CELL)], const T* __restrict__ b_ih,
                                             const T* __restrict__ b_hh, int E, int j) {
  constexpr int G = sr_gates(CELL);
#pragma unroll
  for (int g = 0; g < G; ++g) {
    if (CELL == SR_GRU && g == 2) {
      bias[2] = to_f32(b_ih[2 * E + j]);
      bias[3] = to_f32(b_hh[2 * E + j]);
    } else {
      bias[g] = to_f32(b_ih[g * E + j]) + to_f32(b_hh[g * E + j]);
    }
  }
}

template <typename T, int CELL, int ME>
__global__ __launch_bounds__(SR_THREADS) void sr_fwd_kernel(
    const T* __restrict__ table, int64_t V, int E, const void* __restrict__ idx, int idx32, const void* __restrict__ lens,
    int len32, int64_t B, int L, const float* __restrict__ wt, const T* __restrict__ b_ih, const T* __restrict__ b_hh,
    int mode, const float* __restrict__ scale, T* __restrict__ out, T* __restrict__ h_save, float* __restrict__ c_save,
    int32_t* __restrict__ err_flag, int EJ, const T* __restrict__ w_ih, const T* __restrict__ w_hh) {
  constexpr int NA = sr_accs(CELL);
  __shared__ __attribute__((aligned(16))) float xs[SR_TILE_WORDS], hs[SR_TILE_WORDS];
  __shared__ int s_len[SR_TILE_WORDS], s_red[SR_THREADS];
  const int M = (SR_THREADS / EJ) * SR_S;
  const int64_t b0 = (int64_t)blockIdx.x * M;
  // ME > 0 (then E == EJ == ME): the lane map of the MFMA's result; else unit j of the EJ-wide group, four samples a group
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mq = lane >> 4;
  const int mrow = ME > 0 ? 16 * (wave / (ME > 0 ? ME / 16 : 1)) + (lane & 15) : 0;
  const int j = ME > 0 ? 16 * (wave % (ME > 0 ? ME / 16 : 1)) + (lane & 15) : (int)(threadIdx.x & (EJ - 1));
  const int m0 = ME > 0 ? 16 * (wave / (ME > 0 ? ME / 16 : 1)) + 4 * mq : (int)(threadIdx.x / EJ) * SR_S;
  const bool active = j < E;
  sr_u32x4 wf[NA][ME > 0 ? ME / 16 : 1];
  if constexpr (ME > 0) sr_load_wfrags<CELL, ME>(wf, w_ih, w_hh, j, mq);
  const int tmax = sr_tile_lengths(s_len, s_red, lens, len32 != 0, b0, M, B, L, err_flag);
  for (int i = threadIdx.x; i < M * E; i += SR_THREADS) hs[i] = 0.f;

  float bias[NA], hcur[SR_S], c[SR_S], sum[SR_S];
  int len[SR_S];
  if (active) sr_load_bias<T, CELL>(bias, b_ih, b_hh, E, j);
#pragma unroll
  for (int s = 0; s < SR_S; ++s) {
    hcur[s] = c[s] = sum[s] = 0.f;
    len[s] = s_len[m0 + s];
  }

  for (int t = 0; t < tmax; ++t) {
    sr_gather_step(xs, s_len, table, V, E, idx, idx32 != 0, b0, M, L, t, err_flag);
    __syncthreads();
    if (active) {
      float acc[NA][SR_S];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int s = 0; s < SR_S; ++s) acc[a][s] = bias[a];
      if constexpr (ME > 0) sr_preact_mfma<CELL, ME>(acc, wf, xs, hs, mrow, mq);
      else sr_preact<CELL>(acc, wt, xs, hs, E, j, m0);
#pragma unroll
      for (int s = 0; s < SR_S; ++s) {
        const int64_t b = b0 + m0 + s;
        if (b >= B) continue;
        const bool live = t < len[s];
        float h = 0.f;
        if (live) {
          if constexpr (CELL == SR_RNN) {
            h = tanhf(acc[0][s]);
          } else if constexpr (CELL == SR_LSTM) {
            const float ig = sigmoid_f(acc[0][s]), fg = sigmoid_f(acc[1][s]), gg = tanhf(acc[2][s]),
                        og = sigmoid_f(acc[3][s]);
            c[s] = fmaf(fg, c[s], ig * gg);
            h = og * tanhf(c[s]);
          } else {
            const float r = sigmoid_f(acc[0][s]), z = sigmoid_f(acc[1][s]);
            const float n = tanhf(fmaf(r, acc[3][s], acc[2][s]));
            h = fmaf(z, hcur[s] - n, n);
          }
          sum[s] += h;
          h = to_f32(from_f32<T>(h));      // the next step's operand is what the backward will read back
          hcur[s] = h;
        }
        const int64_t o = (b * L + t) * E + j;
        if (h_save != nullptr) h_save[o] = from_f32<T>(h);
        if (CELL == SR_LSTM && c_save != nullptr && live) c_save[o] = c[s];
        if (mode == 1) out[o] = from_f32<T>(h);
      }
    }
    __syncthreads();
    if (active) {
#pragma unroll
      for (int s = 0; s < SR_S; ++s) hs[(m0 + s) * E + j] = hcur[s];
    }
  }

  if (active) {
    const float sc = *scale;
#pragma unroll
    for (int s = 0; s < SR_S; ++s) {
      const int64_t b = b0 + m0 + s;
      if (b >= B) continue;
      for (int t = tmax; t < L; ++t) {      // steps no sample of the tile reaches
        const int64_t o = (b * L + t) * E + j;
        if (h_save != nullptr) h_save[o] = from_f32<T>(0.f);
        if (mode == 1) out[o] = from_f32<T>(0.f);
      }
      if (mode == 0) out[b * E + j] = from_f32<T>(sum[s] * sc);
    }
  }
}

template <typename T, int CELL, int ME>
__global__ __launch_bounds__(SR_THREADS) void sr_bwd_kernel(
    const T* __restrict__ table, int64_t V, int E, const void* __restrict__ idx, int idx32, const void* __restrict__ lens,
    int len32, int64_t B, int L, const float* __restrict__ wt, const T* __restrict__ w_hh, const T* __restrict__ b_ih,
    const T* __restrict__ b_hh, int mode, const float* __restrict__ scale, const T* __restrict__ h_save,
    const float* __restrict__ c_save, const T* __restrict__ gout, T* __restrict__ dgates, T* __restrict__ dgates_h,
    int EJ, const T* __restrict__ w_ih) {
  constexpr int G = sr_gates(CELL), NA = sr_accs(CELL);
  __shared__ __attribute__((aligned(16))) float xs[SR_TILE_WORDS], hs[SR_TILE_WORDS], dgl[4 * SR_TILE_WORDS];
  __shared__ int s_len[SR_TILE_WORDS], s_red[SR_THREADS];
  const int M = (SR_THREADS / EJ) * SR_S, GE = G * E;
  const int64_t b0 = (int64_t)blockIdx.x * M;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, mq = lane >> 4;      // the forward's lane map
  const int mrow = ME > 0 ? 16 * (wave / (ME > 0 ? ME / 16 : 1)) + (lane & 15) : 0;
  const int j = ME > 0 ? 16 * (wave % (ME > 0 ? ME / 16 : 1)) + (lane & 15) : (int)(threadIdx.x & (EJ - 1));
  const int m0 = ME > 0 ? 16 * (wave / (ME > 0 ? ME / 16 : 1)) + 4 * mq : (int)(threadIdx.x / EJ) * SR_S;
  const bool active = j < E;
  constexpr int KB = ME > 0 ? (G * ME + 31) / 32 : 1;
  sr_u32x4 wf[NA][ME > 0 ? ME / 16 : 1], wb[KB];
  if constexpr (ME > 0) {
    sr_load_wfrags<CELL, ME>(wf, w_ih, w_hh, j, mq);
    sr_load_wfrags_t<CELL, ME>(wb, w_hh, j, mq);
  }
  // the forward raised the flag for what it clamped or skipped: no flag here
  const int tmax = sr_tile_lengths(s_len, s_red, lens, len32 != 0, b0, M, B, L, nullptr);

  float bias[NA], dh[SR_S], dc[SR_S], gpool[SR_S];
  int len[SR_S];
  if (active) sr_load_bias<T, CELL>(bias, b_ih, b_hh, E, j);
  const float sc = *scale;
#pragma unroll
  for (int s = 0; s < SR_S; ++s) {
    dh[s] = dc[s] = gpool[s] = 0.f;
    len[s] = s_len[m0 + s];
    const int64_t b = b0 + m0 + s;
    if (active && b < B) {
      if (mode == 0) gpool[s] = to_f32(gout[b * E + j]) * sc;
      for (int t = tmax; t < L; ++t) {      // steps no sample of the tile reaches
        const int64_t o = (b * L + t) * GE + j;
#pragma unroll
        for (int g = 0; g < G; ++g) {
          dgates[o + g * E] = from_f32<T>(0.f);
          if (CELL == SR_GRU) dgates_h[o + g * E] = from_f32<T>(0.f);
        }
      }
    }
  }

  for (int t = tmax - 1; t >= 0; --t) {
    sr_gather_step(xs, s_len, table, V, E, idx, idx32 != 0, b0, M, L, t, nullptr);
    for (int i = threadIdx.x; i < M * E; i += SR_THREADS) {
      const int m = i / E, e = i - m * E;
      hs[i] = (t > 0 && t < s_len[m]) ? to_f32(h_save[((b0 + m) * L + t - 1) * E + e]) : 0.f;
    }
    __syncthreads();
    float direct[SR_S];
    if (active) {
      float acc[NA][SR_S];
#pragma unroll
      for (int a = 0; a < NA; ++a)
#pragma unroll
        for (int s = 0; s < SR_S; ++s) acc[a][s] = bias[a];
      if constexpr (ME > 0) sr_preact_mfma<CELL, ME>(acc, wf, xs, hs, mrow, mq);
      else sr_preact<CELL>(acc, wt, xs, hs, E, j, m0);
#pragma unroll
      for (int s = 0; s < SR_S; ++s) {
        const int64_t b = b0 + m0 + s;
        float di[G], dhid[G];      // gradients of the input-side and hidden-side pre-activations
#pragma unroll
        for (int g = 0; g < G; ++g) di[g] = dhid[g] = 0.f;
        direct[s] = 0.f;
        if (b < B && t < len[s]) {
          const float dht = dh[s] + (mode == 0 ? gpool[s] : to_f32(gout[(b * L + t) * E + j]));
          if constexpr (CELL == SR_RNN) {
            const float h = tanhf(acc[0][s]);
            di[0] = dhid[0] = dht * (1.f - h * h);
          } else if constexpr (CELL == SR_LSTM) {
            const float ig = sigmoid_f(acc[0][s]), fg = sigmoid_f(acc[1][s]), gg = tanhf(acc[2][s]),
                        og = sigmoid_f(acc[3][s]);
            const float cprev = t > 0 ? c_save[(b * L + t - 1) * E + j] : 0.f;
            const float tc = tanhf(fmaf(fg, cprev, ig * gg));
            const float dct = fmaf(dht * og, 1.f - tc * tc, dc[s]);
            di[0] = dct * gg * ig * (1.f - ig);
            di[1] = dct * cprev * fg * (1.f - fg);
            di[2] = dct * ig * (1.f - gg * gg);
            di[3] = dht * tc * og * (1.f - og);
            dc[s] = dct * fg;
#pragma unroll
            for (int g = 0; g < G; ++g) dhid[g] = di[g];
          } else {
            const float r = sigmoid_f(acc[0][s]), z = sigmoid_f(acc[1][s]);
            const float n = tanhf(fmaf(r, acc[3][s], acc[2][s]));
            const float hprev = hs[(m0 + s) * E + j];
            const float dan = dht * (1.f - z) * (1.f - n * n);
            di[0] = dhid[0] = dan * acc[3][s] * r * (1.f - r);
            di[1] = dhid[1] = dht * (hprev - n) * z * (1.f - z);
            di[2] = dan;
            dhid[2] = dan * r;
            direct[s] = dht * z;
          }
        }
#pragma unroll
        for (int g = 0; g < G; ++g)      // (the matrix-core product takes what dgates_h stores: the rounded value)
          dgl[(m0 + s) * GE + g * E + j] = ME > 0 ? to_f32(from_f32<T>(dhid[g])) : dhid[g];
        if (b < B) {
          const int64_t o = (b * L + t) * GE + j;
#pragma unroll
          for (int g = 0; g < G; ++g) {
            dgates[o + g * E] = from_f32<T>(di[g]);
            if (CELL == SR_GRU) dgates_h[o + g * E] = from_f32<T>(dhid[g]);
          }
        }
      }
    }
    __syncthreads();
    if (active) {
      // dh_{t-1}[s][j] = direct + sum_r dgates_h[s][r] W_hh[r][j]: one sequential sum over r; a sample that is not live
      // at t has zero rows in dgl and keeps dh = 0
      if constexpr (ME > 0) {
        sr_f32x4 cv = {direct[0], direct[1], direct[2], direct[3]};
#pragma unroll
        for (int kk = 0; kk < KB; ++kk) {
          const int k = 32 * kk + 8 * mq;
          const sr_u32x4 au = k < G * ME ? sr_afrag(dgl + mrow * (G * ME) + k) : sr_u32x4{0u, 0u, 0u, 0u};
          cv = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sr_bf16x8, au), __builtin_bit_cast(sr_bf16x8, wb[kk]),
                                                       cv, 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < SR_S; ++s) dh[s] = cv[s];
      } else {
        float a[SR_S];
#pragma unroll
        for (int s = 0; s < SR_S; ++s) a[s] = direct[s];
        for (int r = 0; r < GE; ++r) {
          const float w = to_f32(w_hh[r * E + j]);
#pragma unroll
          for (int s = 0; s < SR_S; ++s) a[s] = fmaf(dgl[(m0 + s) * GE + r], w, a[s]);
        }
#pragma unroll
        for (int s = 0; s < SR_S; ++s) dh[s] = a[s];
      }
    }
  }
}

static int sr_check(const char* what, int64_t B, int L, int E, int dtype, int idx_dtype, int len_dtype, int cell, int mode) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", what, dtype);
  TRS_REQUIRE(cell >= SR_RNN && cell <= SR_GRU, TRS_EINVAL, "%s: bad cell %d (0 rnn, 1 lstm, 2 gru)", what, cell);
  TRS_REQUIRE(mode == 0 || mode == 1, TRS_EINVAL, "%s: bad mode %d", what, mode);
  TRS_REQUIRE((idx_dtype == TRS_I64 || idx_dtype == TRS_I32) && (len_dtype == TRS_I64 || len_dtype == TRS_I32), TRS_EINVAL,
              "%s: bad index dtype %d / %d", what, idx_dtype, len_dtype);
  TRS_REQUIRE(B > 0, TRS_EINVAL, "%s: bad size B=%lld", what, (long long)B);
  TRS_REQUIRE(sr_path(cell, L, E, dtype) != 0, TRS_ESHAPE, "%s: unsupported shape L=%d E=%d (L >= 1, 1 <= E <= %d)", what,
              L, E, SR_MAX_E);
  return TRS_OK;
}

// the matrix-core kernels read their weight fragments as 16-byte vectors: operands that are not so aligned (a view at an
// odd offset) take the vector kernels, which serve every covered shape
static bool sr_use_mfma(int cell, int L, int E, int dtype, const void* w_ih, const void* w_hh) {
  return sr_path(cell, L, E, dtype) == 2 && (((uintptr_t)w_ih | (uintptr_t)w_hh) & 15) == 0;
}

static size_t sr_ws_bytes(int cell, int E) { return (size_t)2 * sr_gates(cell) * E * E * sizeof(float); }

template <typename T>
static int sr_prep(const void* w_ih, const void* w_hh, int cell, int E, float* wt, hipStream_t s) {
  const int GE = sr_gates(cell) * E;
  hipLaunchKernelGGL((sr_prep_kernel<T>), dim3(stream_grid((int64_t)2 * GE * E, 256, 64)), dim3(256), 0, s, (const T*)w_ih,
                     (const T*)w_hh, E, GE, wt);
  return check_launch("seq_rnn weight image");
}

}  // namespace trs

using namespace trs;

extern "C" int trs_seq_rnn_path(int32_t cell, int32_t L, int32_t E, int32_t dtype) { return sr_path(cell, L, E, dtype); }

extern "C" size_t trs_seq_rnn_workspace_bytes(int32_t cell, int32_t E) {
  if (cell < SR_RNN || cell > SR_GRU || E < 1 || E > SR_MAX_E) return 0;
  return sr_ws_bytes(cell, E);
}

extern "C" int trs_seq_rnn_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                               const void* lengths, int32_t len_dtype, int64_t B, int32_t L, const void* w_ih,
                               const void* w_hh, const void* b_ih, const void* b_hh, int32_t cell, int32_t mode,
                               int32_t average, float* scale, void* out, void* h_save, float* c_save, void* workspace,
                               size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;      // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && idx && lengths && w_ih && w_hh && b_ih && b_hh && scale && out && workspace, TRS_EINVAL,
              "seq_rnn_fwd: NULL pointer");
  if (int rc = sr_check("seq_rnn_fwd", B, L, E, dtype, idx_dtype, len_dtype, cell, mode)) return rc;
  TRS_REQUIRE(V >= 0, TRS_EINVAL, "seq_rnn_fwd: bad size V=%lld", (long long)V);
  TRS_REQUIRE(ws_bytes >= sr_ws_bytes(cell, E), TRS_EWORKSPACE, "seq_rnn_fwd: workspace %zu < %zu bytes", ws_bytes,
              sr_ws_bytes(cell, E));
  hipStream_t s = (hipStream_t)stream;
  float* wt = (float*)workspace;
  const int EJ = sr_pow2_above(E), M = (SR_THREADS / EJ) * SR_S;
  const int grid = ceil_div_i(B, M);
  const int i32 = idx_dtype == TRS_I32, l32 = len_dtype == TRS_I32;
  hipLaunchKernelGGL(sr_scale_kernel, dim3(1), dim3(SR_THREADS), 0, s, lengths, l32, B, L, (int)(average != 0), scale);
  if (int rc = check_launch("seq_rnn scale")) return rc;
#define TRS_SR_ME(T_, CELL_, ME_)                                                                                     \
  hipLaunchKernelGGL((sr_fwd_kernel<T_, CELL_, ME_>), dim3(grid), dim3(SR_THREADS), 0, s, (const T_*)table, V, E, idx,  \
                     i32, lengths, l32, B, L, (const float*)wt, (const T_*)b_ih, (const T_*)b_hh, mode,               \
                     (const float*)scale, (T_*)out, (T_*)h_save, c_save, err_flag, EJ, (const T_*)w_ih,               \
                     (const T_*)w_hh)
#define TRS_SR(T_, CELL_)                                                                                             \
  do {                                                                                                                \
    if (int rc = sr_prep<T_>(w_ih, w_hh, cell, E, wt, s)) return rc;                                                  \
    TRS_SR_ME(T_, CELL_, 0);                                                                                          \
  } while (0)
#define TRS_SR_M(CELL_)                                                                                               \
  do {                                                                                                                \
    if (E == 16) TRS_SR_ME(bf16_t, CELL_, 16);                                                                        \
    else if (E == 32) TRS_SR_ME(bf16_t, CELL_, 32);                                                                   \
    else TRS_SR_ME(bf16_t, CELL_, 64);                                                                                \
  } while (0)
  if (sr_use_mfma(cell, L, E, dtype, w_ih, w_hh)) {
    if (cell == SR_RNN) TRS_SR_M(SR_RNN);
    else if (cell == SR_LSTM) TRS_SR_M(SR_LSTM);
    else TRS_SR_M(SR_GRU);
  } else if (dtype == TRS_F32) {
    if (cell == SR_RNN) TRS_SR(float, SR_RNN);
    else if (cell == SR_LSTM) TRS_SR(float, SR_LSTM);
    else TRS_SR(float, SR_GRU);
  } else {
    if (cell == SR_RNN) TRS_SR(bf16_t, SR_RNN);
    else if (cell == SR_LSTM) TRS_SR(bf16_t, SR_LSTM);
    else TRS_SR(bf16_t, SR_GRU);
  }
#undef TRS_SR
#undef TRS_SR_M
#undef TRS_SR_ME
  return check_launch("seq_rnn_fwd");
}

extern "C" int trs_seq_rnn_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                               const void* lengths, int32_t len_dtype, int64_t B, int32_t L, const void* w_ih,
                               const void* w_hh, const void* b_ih, const void* b_hh, int32_t cell, int32_t mode,
                               const float* scale, const void* h_save, const float* c_save, const void* gout,
                               void* dgates, void* dgates_h, void* workspace, size_t ws_bytes, trs_stream_t stream) {
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(table && idx && lengths && w_ih && w_hh && b_ih && b_hh && scale && h_save && gout && dgates && workspace,
              TRS_EINVAL, "seq_rnn_bwd: NULL pointer");
  if (int rc = sr_check("seq_rnn_bwd", B, L, E, dtype, idx_dtype, len_dtype, cell, mode)) return rc;
  TRS_REQUIRE(V >= 0, TRS_EINVAL, "seq_rnn_bwd: bad size V=%lld", (long long)V);
  TRS_REQUIRE(cell != SR_LSTM || c_save != nullptr, TRS_EINVAL, "seq_rnn_bwd: the lstm needs c_save");
  TRS_REQUIRE(cell != SR_GRU || dgates_h != nullptr, TRS_EINVAL, "seq_rnn_bwd: the gru needs dgates_h");
  TRS_REQUIRE(ws_bytes >= sr_ws_bytes(cell, E), TRS_EWORKSPACE, "seq_rnn_bwd: workspace %zu < %zu bytes", ws_bytes,
              sr_ws_bytes(cell, E));
  hipStream_t s = (hipStream_t)stream;
  float* wt = (float*)workspace;
  const int EJ = sr_pow2_above(E), M = (SR_THREADS / EJ) * SR_S;
  const int grid = ceil_div_i(B, M);
  const int i32 = idx_dtype == TRS_I32, l32 = len_dtype == TRS_I32;
#define TRS_SR_ME(T_, CELL_, ME_)                                                                                     \
  hipLaunchKernelGGL((sr_bwd_kernel<T_, CELL_, ME_>), dim3(grid), dim3(SR_THREADS), 0, s, (const T_*)table, V, E, idx,  \
                     i32, lengths, l32, B, L, (const float*)wt, (const T_*)w_hh, (const T_*)b_ih, (const T_*)b_hh,    \
                     mode, scale, (const T_*)h_save, c_save, (const T_*)gout, (T_*)dgates, (T_*)dgates_h, EJ,         \
                     (const T_*)w_ih)
#define TRS_SR(T_, CELL_)                                                                                             \
  do {                                                                                                                \
    if (int rc = sr_prep<T_>(w_ih, w_hh, cell, E, wt, s)) return rc;                                                  \
    TRS_SR_ME(T_, CELL_, 0);                                                                                          \
  } while (0)
#define TRS_SR_M(CELL_)                                                                                               \
  do {                                                                                                                \
    if (E == 16) TRS_SR_ME(bf16_t, CELL_, 16);                                                                        \
    else if (E == 32) TRS_SR_ME(bf16_t, CELL_, 32);                                                                   \
    else TRS_SR_ME(bf16_t, CELL_, 64);                                                                                \
  } while (0)
  if (sr_use_mfma(cell, L, E, dtype, w_ih, w_hh)) {
    if (cell == SR_RNN) TRS_SR_M(SR_RNN);
    else if (cell == SR_LSTM) TRS_SR_M(SR_LSTM);
    else TRS_SR_M(SR_GRU);
  } else if (dtype == TRS_F32) {
    if (cell == SR_RNN) TRS_SR(float, SR_RNN);
    else if (cell == SR_LSTM) TRS_SR(float, SR_LSTM);
    else TRS_SR(float, SR_GRU);
  } else {
    if (cell == SR_RNN) TRS_SR(bf16_t, SR_RNN);
    else if (cell == SR_LSTM) TRS_SR(bf16_t, SR_LSTM);
    else TRS_SR(bf16_t, SR_GRU);
  }
#undef TRS_SR
#undef TRS_SR_M
#undef TRS_SR_ME
  return check_launch("seq_rnn_bwd");
}
