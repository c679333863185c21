// Full-catalogue softmax cross-entropy for the embedding models: the anchor against EVERY row of a target table (or, in
// batch, against the other positives), forward and both gradients, with nothing of the (B, Vt) logits written anywhere.
//
//   z[b, j] = scale * <A[b], T[j]>                     loss[b] = logsumexp_j z[b, j] - z[b, y_b]      (0 where y_b is ignored)
//   dA[b]   = scale * sum_j w[b, j] T[j]               w[b, j] = g_b (exp(z[b, j] - lse_b) - [j == y_b])
//   dT[j]   = scale * sum_b w[b, j] A[b]               g_b = 0 for an ignored sample
//
// Forward (sl_fwd_kernel): the anchor-stationary split of topk.hip.  grid = (anchor tiles) x (S target ranges); a
// workgroup of NW waves holds NW * AR anchors in LDS for its whole life and streams its range in tiles of TR rows through
// a double buffer -- by LDS-DMA where a row is whole 64-byte k-steps, by zero-padded stores otherwise -- rows XOR-swizzled
// in 16-byte chunks as there.  Targets are the MFMA's A operand and anchors its B operand, so lane (n, q) holds, for
// anchor n, targets 4 q .. 4 q + 3 of every 16-target group: it keeps a running (max, sum of exponentials) over ITS
// targets, rescaled when the max rises, and picks up z[b, y_b] when the tile that holds y_b passes.  The four lanes of an
// anchor are folded once, behind the last tile.  S = 1: loss and lse are written at once; S > 1: (max, sum) per (anchor,
// range) go to the workspace and sl_fwd_finish_kernel folds them in range order.
//
// Backward (sl_bwd_kernel, one template for both gradients).  "Stationary" rows sit in LDS and own the fp32 gradient
// accumulators, "streamed" rows pass in tiles: dA has the anchors stationary and streams the targets, dT has a tile of
// targets stationary and streams the anchors (with their lse, g and labels in three small per-tile LDS arrays).  Per tile
// the scores are recomputed as in the forward (streamed rows = A operand) and w is formed in fp32 in the accumulator
// registers.  fp32 tables take it as it is; for bf16 it becomes the pair hi = bf16(w), lo = bf16(w - hi) and the second
// MFMA runs twice on one Y operand: a single bf16 rounding is 2^-8 relative in the worst case, and a target row with one
// positive has a one-term sum that shows all of it, against the 2^-9 the gradient's bound allows the operand.  The accumulator layout -- lane (n, q): streamed rows 4 q + r of each
// 16-row group for stationary row n -- is a fixed permutation of the k slots of a second MFMA that contracts over the
// streamed rows, out^T[e, n] += Y^T[e, k] w^T[k, n]: bf16 takes two groups (k slot 8 q + r <- row 16 nt + 4 q + r, slot
// 8 q + 4 + r <- row 16 (nt + 1) + 4 q + r), fp32 one row per 16x16x4 MFMA (slot q <- row 16 nt + 4 q + r for MFMA r).  w
// therefore goes from accumulator to operand in registers; only the Y operand is read from LDS with the same permutation,
// i.e. down a column of the tile (2- or 4-byte reads: see profiles/softmax_loss_kernels.md for why not the transposing
// read).  The gradient accumulators stay in registers for the whole range; S = 1 rounds and writes them, S > 1 writes fp32
// partials that sl_bwd_finish_kernel sums in range order.  No floating-point atomics: every sum has one fixed order.
//
// Cosine and a per-target bias (template parameter X of the three kernels; SL_PLAIN is the code described above):
//   s[b, j] = <A[b], T[j]> ra[b] rt[j],  r = 1 / max(|row|, 1e-8) from an fp32 sum of squares (rank.hip, topk.hip)
//   z[b, j] = scale s[b, j] + bias[j]                       d_bias[j] = sum_b w[b, j]
//   dA[b]   = scale ra[b] (sum_j (w[b, j] rt[j]) T[j] - ra[b] c[b] A[b]),  c[b] = sum_j w[b, j] s[b, j];  dT alike
// The inverse norms of the stationary rows are held per lane, those of a streamed tile are computed by the workgroup from
// the tile in LDS into a [2][TR] array one step ahead of the tile that is scored (tile_norms of topk.hip); a target
// tile's bias is loaded with it into a second [2][TR] array.  The backward adds w s to one scalar per stationary row
// before w replaces the score (and, for the target gradient, w to a second one: d_bias), multiplies w by the streamed
// row's inverse norm and runs the second MFMA as before; behind the last tile the scalars are folded over the row's four
// lanes and every lane applies scale r (G - r c x) to its columns, x from the stationary rows in LDS.  A row whose norm
// is not above eps gets no projection term (the clamp passes no gradient).  The projection is linear in a range's sums,
// so S > 1 writes projected partials and the finish is unchanged; d_bias partials (S, Vt) follow the gradient partials
// in the workspace and sl_dbias_finish_kernel sums them in range order.
#include <algorithm>

#include "lds_dma.hpp"

namespace trs {

typedef __attribute__((ext_vector_type(8))) __bf16 sl_bf16x8;
typedef __attribute__((ext_vector_type(4))) float sl_f32x4;

constexpr int SL_MAX_E = 256, SL_MAX_SPLITS = 64;
constexpr size_t SL_MAX_LDS = 160 * 1024;
constexpr int SL_BWD_AR = 32;      // stationary rows per wave of the backward
constexpr int SL_PLAIN = 0, SL_BIAS = 1, SL_COS = 2;      // X: inner product; + bias; cosine (+ bias where there is one)
constexpr float SL_COS_EPS = 1e-8f;                       // rank.hip's COS_EPS

struct SlArgs {
  const char* st;          // stationary rows (Ns, E): the anchors; dT: the targets
  const char* sr;          // streamed rows (Nr, E)
  const void* labels;      // (B)
  const float* lse;        // (B)   backward
  const float* g;          // (B)   backward
  const float* bias;       // (Vt)  or NULL
  float* dbias;            // (Vt)  dT, or NULL
  float* ws_db;            // (S, Vt) partials of dbias, S > 1
  float* loss;             // (B)   forward
  float* lse_out;          // (B)   forward
  float* ws;
  void* out;               // (Ns, E) gradient of the stationary rows
  int32_t* err_flag;
  int64_t Ns, Nr, ignore;
  int rows_per, S;
  int64_t Vt;
  float scale;
  int E, row_bytes;
  int nc, nce;             // 16-byte chunks of an LDS row (whole 64-byte k-steps) and of a table row
  int sw_shift, sw_mask;   // g(r) = (r >> sw_shift) & sw_mask
  bool lab64, dma;
};

__device__ __forceinline__ int64_t sl_label(const SlArgs& p, int64_t b) {
  return p.lab64 ? static_cast<const int64_t*>(p.labels)[b] : (int64_t) static_cast<const int32_t*>(p.labels)[b];
}

template <typename T>
__device__ __forceinline__ sl_f32x4 sl_mma(const uint4& a, const uint4& b, sl_f32x4 acc) {
  if constexpr (std::is_same<T, float>::value) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sl_bf16x8, a), __builtin_bit_cast(sl_bf16x8, b), acc, 0,
                                                   0, 0);
  }
}

// rows [r0, r0 + n) of `src` (those below `end`; the others and the padding chunks as zeros) into n swizzled LDS rows
__device__ __forceinline__ void sl_stage_padded(char* dst, const char* src, int64_t r0, int64_t end, int n, const SlArgs& p) {
  for (int u = threadIdx.x; u < n * p.nc; u += blockDim.x) {
    const int r = u / p.nc, c = u - r * p.nc;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (r0 + r < end && c < p.nce) v = *reinterpret_cast<const uint4*>(src + (r0 + r) * p.row_bytes + 16 * c);
    *reinterpret_cast<uint4*>(dst + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = v;
  }
}

// the same by LDS-DMA (rows of whole k-steps; n * nc a multiple of 64): rows past `end` re-read the last one, the caller
// masks what is computed from them.  At least one row lies below `end`.
__device__ __forceinline__ void sl_stage_dma(char* dst, const char* src, int64_t r0, int64_t end, int n, const SlArgs& p) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, NW = blockDim.x >> 6;
  const char* base_src = src + r0 * p.row_bytes;
  const unsigned base = lds_addr(dst);
  const int last = (int)std::min<int64_t>(n, end - r0) - 1;
  for (int pc = wave; pc < n * p.nc / 64; pc += NW) {
    const int u = pc * 64 + lane, r = u / p.nc, cp = u - r * p.nc;
    const int c = cp ^ ((r >> p.sw_shift) & p.sw_mask);
    lds_dma1(base_src, (unsigned)(std::min(r, last) * p.row_bytes + 16 * c), base + pc * 1024);
  }
}

// acc[at][nt] = (streamed rows 16 nt .. of Rb) x (this wave's stationary rows row0 + 16 at) over the whole row
template <typename T, int AT, int NT>
__device__ __forceinline__ void sl_scores(sl_f32x4 (&acc)[AT][NT], const char* Sb, const char* Rb, int row0, int n, int q,
                                          int RB, const SlArgs& p) {
  const int gsw = (n >> p.sw_shift) & p.sw_mask;      // g(r) depends on r & 15 only
#pragma unroll
  for (int at = 0; at < AT; ++at)
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) acc[at][nt] = sl_f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ks = 0; ks < (p.nc >> 2); ++ks) {
    const int coff = ((4 * ks + q) ^ gsw) << 4;
    uint4 bf[AT];
#pragma unroll
    for (int at = 0; at < AT; ++at) bf[at] = *reinterpret_cast<const uint4*>(Sb + (row0 + 16 * at) * RB + coff);
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const uint4 af = *reinterpret_cast<const uint4*>(Rb + (16 * nt + n) * RB + coff);
#pragma unroll
      for (int at = 0; at < AT; ++at) acc[at][nt] = sl_mma<T>(af, bf[at], acc[at][nt]);
    }
  }
}

// 1 / max(|LDS row r|, eps): the squares of its real chunks summed in order, fp32 (tk_row_sq of topk.hip)
template <typename T>
__device__ __forceinline__ float sl_row_norm(const char* rows, int r, const SlArgs& p) {
  const int g = (r >> p.sw_shift) & p.sw_mask;
  float s = 0.f;
  for (int c = 0; c < p.nce; ++c) {
    float f[Vec16<T>::VE];
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>(rows + ((size_t)r * p.nc + (c ^ g)) * 16), f);
#pragma unroll
    for (int e = 0; e < Vec16<T>::VE; ++e) s += f[e] * f[e];
  }
  return sqrtf(s);
}
__device__ __forceinline__ float sl_inv(float norm) { return 1.f / fmaxf(norm, SL_COS_EPS); }

// ------------------------------------------------------------------------------------------------ forward
template <typename T, int AR, int TR, int X>
__global__ __launch_bounds__(256) void sl_fwd_kernel(SlArgs p) {
  extern __shared__ __attribute__((aligned(16))) char sl_smem[];
  constexpr int AT = AR / 16, NT = TR / 16;
  const int NW = blockDim.x >> 6, NA = NW * AR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int RB = p.nc * 16;
  char* As = sl_smem;
  char* Ts = As + (size_t)NA * RB;
  float* t_inv = reinterpret_cast<float*>(Ts + (size_t)2 * TR * RB);      // X != SL_PLAIN: [2][TR] inverse norms (cosine)
  float* t_bias = t_inv + 2 * TR;                                         //                [2][TR] bias, 0 behind the end
  float* a_inv = t_bias + 2 * TR;                                         //                [NA] (cosine)

  const int64_t b0 = (int64_t)blockIdx.x * NA;
  sl_stage_padded(As, p.st, b0, p.Ns, NA, p);
  const int64_t lo = (int64_t)blockIdx.y * p.rows_per;
  const int64_t hi = std::min<int64_t>(lo + p.rows_per, p.Nr);
  const int ntile = hi > lo ? (int)((hi - lo + TR - 1) / TR) : 0;
  auto load_tile = [&](int t, int buf) {
    const int64_t t0 = lo + (int64_t)t * TR;
    char* dst = Ts + (size_t)buf * TR * RB;
    if (p.dma) sl_stage_dma(dst, p.sr, t0, hi, TR, p);
    else sl_stage_padded(dst, p.sr, t0, hi, TR, p);
    if constexpr (X != SL_PLAIN) {
      for (int r = threadIdx.x; r < TR; r += blockDim.x)
        t_bias[buf * TR + r] = p.bias != nullptr && t0 + r < hi ? p.bias[t0 + r] : 0.f;
    }
  };
  // a row behind the range's end is the last row again (LDS-DMA) or zeros (r = 1e8, score 0): finite, and masked below
  auto tile_norms = [&](int buf) {
    for (int r = threadIdx.x; r < TR; r += blockDim.x)
      t_inv[buf * TR + r] = sl_inv(sl_row_norm<T>(Ts + (size_t)buf * TR * RB, r, p));
  };
  if (ntile > 0) load_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if constexpr (X == SL_COS) {
    for (int r = threadIdx.x; r < NA; r += blockDim.x) a_inv[r] = sl_inv(sl_row_norm<T>(As, r, p));
    if (ntile > 0) tile_norms(0);
    __syncthreads();
  }

  // per lane: anchor n of each of the wave's AT groups of 16, over the targets 4 q .. 4 q + 3 of every group
  const int row0 = wave * AR + n;
  int64_t y[AT];
  float m[AT], s[AT], zp[AT];
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    const int64_t b = b0 + row0 + 16 * at;
    y[at] = -1;
    if (b < p.Ns) {
      const int64_t lab = sl_label(p, b);
      if (lab >= 0 && lab < p.Vt) y[at] = lab;
      else if (lab != p.ignore && q == 0 && blockIdx.y == 0 && p.err_flag != nullptr) *p.err_flag = 1;
    }
    m[at] = -INFINITY;
    s[at] = 0.f;
    zp[at] = 0.f;
  }
  float ra[AT];
#pragma unroll
  for (int at = 0; at < AT; ++at) ra[at] = X == SL_COS ? a_inv[row0 + 16 * at] : 1.f;

  for (int t = 0; t < ntile; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntile) load_tile(t + 1, buf ^ 1);
    sl_f32x4 acc[AT][NT];
    sl_scores<T, AT, NT>(acc, As, Ts + (size_t)buf * TR * RB, row0, n, q, RB, p);
    const int64_t t0 = lo + (int64_t)t * TR;
    const int valid = (int)std::min<int64_t>(TR, hi - t0);      // targets of this tile that exist
#pragma unroll
    for (int at = 0; at < AT; ++at) {
      const int yl = y[at] >= t0 && y[at] < t0 + TR ? (int)(y[at] - t0) : -1;      // the positive, where this tile holds it
      float tm = -INFINITY;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        float4 r4 = make_float4(1.f, 1.f, 1.f, 1.f), c4 = make_float4(0.f, 0.f, 0.f, 0.f);
        if constexpr (X == SL_COS) r4 = *reinterpret_cast<const float4*>(t_inv + buf * TR + 16 * nt + 4 * q);
        if constexpr (X != SL_PLAIN) c4 = *reinterpret_cast<const float4*>(t_bias + buf * TR + 16 * nt + 4 * q);
        const float rj[4] = {r4.x, r4.y, r4.z, r4.w}, cj[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int local = 16 * nt + 4 * q + j;
          float z = acc[at][nt][j];
          if constexpr (X == SL_COS) z = z * ra[at] * rj[j];
          z *= p.scale;
          if constexpr (X != SL_PLAIN) z += cj[j];
          if (local >= valid) z = -INFINITY;
          acc[at][nt][j] = z;
          tm = fmaxf(tm, z);
          if (local == yl) zp[at] = z;
        }
      }
      if (tm > m[at]) {      // the max rises: what was summed so far is rescaled (nothing was, where m is -inf)
        s[at] = m[at] == -INFINITY ? 0.f : s[at] * expf(m[at] - tm);
        m[at] = tm;
      }
      if (m[at] > -INFINITY) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) s[at] += expf(acc[at][nt][j] - m[at]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (X == SL_COS) {      // the next tile has landed: its norms, one step ahead
      if (t + 1 < ntile) {
        tile_norms(buf ^ 1);
        __syncthreads();
      }
    }
  }

  // ---- the four lanes of an anchor
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    float M = fmaxf(m[at], __shfl_xor(m[at], 16, 64));
    M = fmaxf(M, __shfl_xor(M, 32, 64));
    float v = m[at] == -INFINITY ? 0.f : s[at] * expf(m[at] - M);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    float z = zp[at];
    z += __shfl_xor(z, 16, 64);
    z += __shfl_xor(z, 32, 64);
    const int64_t b = b0 + row0 + 16 * at;
    if (q != 0 || b >= p.Ns) continue;
    if (p.S == 1) {
      const float lg = logf(v);
      p.lse_out[b] = M + lg;
      p.loss[b] = y[at] >= 0 ? (M - z) + lg : 0.f;      // not lse - z: M - z is small where lse is not
    } else {
      reinterpret_cast<float2*>(p.ws)[b * p.S + blockIdx.y] = make_float2(M, v);
      if (y[at] >= lo && y[at] < hi) p.ws[(size_t)2 * p.Ns * p.S + b] = z;
    }
  }
}

// S > 1: one thread per anchor folds the S (max, sum) pairs in range order
__global__ __launch_bounds__(256) void sl_fwd_finish_kernel(SlArgs p) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= p.Ns) return;
  const float2* ms = reinterpret_cast<const float2*>(p.ws) + b * p.S;
  float M = -INFINITY;
  for (int i = 0; i < p.S; ++i) M = fmaxf(M, ms[i].x);
  float v = 0.f;
  for (int i = 0; i < p.S; ++i) {
    const float2 e = ms[i];
    if (e.x > -INFINITY) v += e.y * expf(e.x - M);
  }
  const float lg = logf(v);
  const int64_t lab = sl_label(p, b);
  p.lse_out[b] = M + lg;
  p.loss[b] = lab >= 0 && lab < p.Vt ? (M - p.ws[(size_t)2 * p.Ns * p.S + b]) + lg : 0.f;
}

// ------------------------------------------------------------------------------------------------ backward
// element e of swizzled LDS row r
template <typename T>
__device__ __forceinline__ uint32_t sl_lds_elem(const char* rows, int r, int e, int RB, const SlArgs& p) {
  constexpr int PER = 16 / (int)sizeof(T);
  const int c = (e / PER) ^ ((r >> p.sw_shift) & p.sw_mask);
  const char* a = rows + (size_t)r * RB + (c << 4) + (e % PER) * (int)sizeof(T);
  if constexpr (std::is_same<T, float>::value) return *reinterpret_cast<const uint32_t*>(a);
  else return *reinterpret_cast<const uint16_t*>(a);
}

// DT false: stationary = anchors, streamed = targets (dA).  DT true: stationary = targets, streamed = anchors (dT).
// EB: 16-column blocks of the gradient a lane holds accumulators for (E <= 16 EB).
template <typename T, int EB, int TR, bool DT, int X, int AR = SL_BWD_AR>
__global__ __launch_bounds__(256) void sl_bwd_kernel(SlArgs p) {
  extern __shared__ __attribute__((aligned(16))) char sl_smem[];
  constexpr int AT = AR / 16, NT = TR / 16;
  constexpr bool F32 = std::is_same<T, float>::value;
  constexpr bool COS = X == SL_COS, BIAS = X != SL_PLAIN;
  const int NW = blockDim.x >> 6, NA = NW * AR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int RB = p.nc * 16;
  char* Ss = sl_smem;
  char* Rs = Ss + (size_t)NA * RB;
  float* r_lse = reinterpret_cast<float*>(Rs + (size_t)2 * TR * RB);      // DT: [2][TR] each
  float* r_g = r_lse + 2 * TR;
  int* r_y = reinterpret_cast<int*>(r_g + 2 * TR);
  float* r_inv = DT ? r_lse + 6 * TR : r_lse;      // X != SL_PLAIN: [2][TR] inverse norms of the streamed rows (cosine)
  float* r_bias = r_inv + 2 * TR;                  //                dA: [2][TR] bias of the streamed targets

  const int64_t s0 = (int64_t)blockIdx.x * NA;
  sl_stage_padded(Ss, p.st, s0, p.Ns, NA, p);
  const int64_t lo = (int64_t)blockIdx.y * p.rows_per;
  const int64_t hi = std::min<int64_t>(lo + p.rows_per, p.Nr);
  const int ntile = hi > lo ? (int)((hi - lo + TR - 1) / TR) : 0;
  auto load_tile = [&](int t, int buf) {
    const int64_t t0 = lo + (int64_t)t * TR;
    char* dst = Rs + (size_t)buf * TR * RB;
    if (p.dma) sl_stage_dma(dst, p.sr, t0, hi, TR, p);
    else sl_stage_padded(dst, p.sr, t0, hi, TR, p);
    if constexpr (DT) {      // the streamed anchors' lse, g and label; a row past the end or an ignored sample weighs 0
      for (int r = threadIdx.x; r < TR; r += blockDim.x) {
        float l = INFINITY, g = 0.f;
        int yy = -1;
        if (t0 + r < hi) {
          const int64_t lab = sl_label(p, t0 + r);
          l = p.lse[t0 + r];
          if (lab >= 0 && lab < p.Vt) {
            g = p.g[t0 + r];
            yy = (int)lab;
          }
        }
        r_lse[buf * TR + r] = l;
        r_g[buf * TR + r] = g;
        r_y[buf * TR + r] = yy;
      }
    } else if constexpr (BIAS) {
      for (int r = threadIdx.x; r < TR; r += blockDim.x)
        r_bias[buf * TR + r] = p.bias != nullptr && t0 + r < hi ? p.bias[t0 + r] : 0.f;
    }
  };
  // a streamed row behind the range's end: the last row again (LDS-DMA) or zeros (r = 1e8, score 0); its w is set to 0
  auto tile_norms = [&](int buf) {
    for (int r = threadIdx.x; r < TR; r += blockDim.x)
      r_inv[buf * TR + r] = sl_inv(sl_row_norm<T>(Rs + (size_t)buf * TR * RB, r, p));
  };
  if (ntile > 0) load_tile(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if constexpr (COS) {
    if (ntile > 0) tile_norms(0);
    __syncthreads();
  }

  const int row0 = wave * AR + n;
  float s_lse[AT], s_g[AT];
  int64_t s_y[AT];      // dA: the anchor's label; dT: the stationary target's own row number
  float s_inv[AT], s_bias[AT];      // the stationary row's inverse norm (cosine); dT: its bias
  float c[AT], db[AT];              // sum of w s (cosine) and, dT, of w over the streamed rows this lane sees
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    const int64_t sr = s0 + row0 + 16 * at;
    s_inv[at] = COS ? sl_inv(sl_row_norm<T>(Ss, row0 + 16 * at, p)) : 1.f;
    s_bias[at] = DT && BIAS && p.bias != nullptr && sr < p.Ns ? p.bias[sr] : 0.f;
    c[at] = db[at] = 0.f;
    s_lse[at] = INFINITY;
    s_g[at] = 0.f;
    s_y[at] = DT ? sr : -1;
    if (!DT && sr < p.Ns) {
      const int64_t lab = sl_label(p, sr);
      s_lse[at] = p.lse[sr];
      if (lab >= 0 && lab < p.Vt) {
        s_g[at] = p.g[sr];
        s_y[at] = lab;
      }
    }
  }
  const int neb = (p.E + 15) >> 4;
  sl_f32x4 dacc[AT][EB];
#pragma unroll
  for (int at = 0; at < AT; ++at)
#pragma unroll
    for (int eb = 0; eb < EB; ++eb) dacc[at][eb] = sl_f32x4{0.f, 0.f, 0.f, 0.f};

  for (int t = 0; t < ntile; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntile) load_tile(t + 1, buf ^ 1);
    const char* Rb = Rs + (size_t)buf * TR * RB;
    sl_f32x4 acc[AT][NT];
    sl_scores<T, AT, NT>(acc, Ss, Rb, row0, n, q, RB, p);
    const int64_t t0 = lo + (int64_t)t * TR;
    const int valid = (int)std::min<int64_t>(TR, hi - t0);
    // ---- w = g (exp(z - lse) - [label == target]) in place of the scores
    int yl[AT];      // dA: the anchor's positive as a row of this tile, or -1
#pragma unroll
    for (int at = 0; at < AT; ++at) yl[at] = !DT && s_y[at] >= t0 && s_y[at] < t0 + TR ? (int)(s_y[at] - t0) : -1;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      float4 l4 = make_float4(0.f, 0.f, 0.f, 0.f), g4 = l4;
      int4 y4 = make_int4(-1, -1, -1, -1);
      if constexpr (DT) {
        l4 = *reinterpret_cast<const float4*>(r_lse + buf * TR + 16 * nt + 4 * q);
        g4 = *reinterpret_cast<const float4*>(r_g + buf * TR + 16 * nt + 4 * q);
        y4 = *reinterpret_cast<const int4*>(r_y + buf * TR + 16 * nt + 4 * q);
      }
      const float lj[4] = {l4.x, l4.y, l4.z, l4.w}, gj[4] = {g4.x, g4.y, g4.z, g4.w};
      const int yj[4] = {y4.x, y4.y, y4.z, y4.w};
      float4 r4 = make_float4(1.f, 1.f, 1.f, 1.f), c4 = make_float4(0.f, 0.f, 0.f, 0.f);
      if constexpr (COS) r4 = *reinterpret_cast<const float4*>(r_inv + buf * TR + 16 * nt + 4 * q);
      if constexpr (BIAS && !DT) c4 = *reinterpret_cast<const float4*>(r_bias + buf * TR + 16 * nt + 4 * q);
      const float rj[4] = {r4.x, r4.y, r4.z, r4.w}, cj[4] = {c4.x, c4.y, c4.z, c4.w};
#pragma unroll
      for (int at = 0; at < AT; ++at)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int local = 16 * nt + 4 * q + j;
          float sc = acc[at][nt][j];      // the forward's order: the anchor's inverse norm first
          if constexpr (COS) sc = DT ? sc * rj[j] * s_inv[at] : sc * s_inv[at] * rj[j];
          float z = sc * p.scale;
          if constexpr (BIAS) z += DT ? s_bias[at] : cj[j];
          float w;
          if constexpr (DT) {
            w = gj[j] * (expf(z - lj[j]) - ((int64_t)yj[j] == s_y[at] ? 1.f : 0.f));
            if (BIAS && local >= valid) w = 0.f;
          } else {
            w = s_g[at] * (expf(z - s_lse[at]) - (local == yl[at] ? 1.f : 0.f));
            if (local >= valid) w = 0.f;
          }
          if constexpr (COS) c[at] += w * sc;
          if constexpr (DT && BIAS) db[at] += w;
          if constexpr (COS) w *= rj[j];
          acc[at][nt][j] = w;
        }
    }
    // ---- out^T += Y^T w^T over the tile's streamed rows, w straight from the accumulators
    if constexpr (F32) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int eb = 0; eb < EB; ++eb) {
            if (eb >= neb) continue;
            const float yv = __uint_as_float(sl_lds_elem<T>(Rb, 16 * nt + 4 * q + j, 16 * eb + n, RB, p));
#pragma unroll
            for (int at = 0; at < AT; ++at)
              dacc[at][eb] = __builtin_amdgcn_mfma_f32_16x16x4f32(yv, acc[at][nt][j], dacc[at][eb], 0, 0, 0);
          }
    } else {
#pragma unroll
      for (int np = 0; np < NT / 2; ++np) {
        uint4 wf[AT], wl[AT];      // w = hi + lo, both bf16
#pragma unroll
        for (int at = 0; at < AT; ++at) {
          const sl_f32x4 a = acc[at][2 * np], b = acc[at][2 * np + 1];
          const float w8[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
          uint32_t hi[4], lo[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            hi[j] = f32x2_to_bf16x2_bits(w8[2 * j], w8[2 * j + 1]);
            lo[j] = f32x2_to_bf16x2_bits(w8[2 * j] - __uint_as_float(hi[j] << 16),
                                         w8[2 * j + 1] - __uint_as_float(hi[j] & 0xffff0000u));
          }
          wf[at] = make_uint4(hi[0], hi[1], hi[2], hi[3]);
          wl[at] = make_uint4(lo[0], lo[1], lo[2], lo[3]);
        }
#pragma unroll
        for (int eb = 0; eb < EB; ++eb) {
          if (eb >= neb) continue;
          uint32_t h[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            h[j] = sl_lds_elem<T>(Rb, 32 * np + 16 * (j >> 2) + 4 * q + (j & 3), 16 * eb + n, RB, p);
          const uint4 yf = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
#pragma unroll
          for (int at = 0; at < AT; ++at) {
            dacc[at][eb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sl_bf16x8, yf),
                                                                   __builtin_bit_cast(sl_bf16x8, wl[at]), dacc[at][eb], 0, 0, 0);
            dacc[at][eb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(sl_bf16x8, yf),
                                                                   __builtin_bit_cast(sl_bf16x8, wf[at]), dacc[at][eb], 0, 0, 0);
          }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (COS) {      // the next tile has landed: its norms, one step ahead
      if (t + 1 < ntile) {
        tile_norms(buf ^ 1);
        __syncthreads();
      }
    }
  }

  // ---- the four lanes of a stationary row hold a quarter of the streamed rows each
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    if constexpr (COS) {
      c[at] += __shfl_xor(c[at], 16, 64);
      c[at] += __shfl_xor(c[at], 32, 64);
    }
    if constexpr (DT && BIAS) {
      db[at] += __shfl_xor(db[at], 16, 64);
      db[at] += __shfl_xor(db[at], 32, 64);
    }
  }

  // ---- lane (n, q) holds columns 16 eb + 4 q .. + 3 of stationary row n
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    const int64_t sr = s0 + row0 + 16 * at;
    if (sr >= p.Ns) continue;
    if constexpr (DT && BIAS) {
      if (q == 0 && p.dbias != nullptr) (p.S > 1 ? p.ws_db + (size_t)blockIdx.y * p.Ns : p.dbias)[sr] = db[at];
    }
    // cosine: scale r (G - r c x); a norm that is not above eps was clamped and passes no gradient: no projection
    const float rs = p.scale * s_inv[at];
    const float pc = COS && sl_row_norm<T>(Ss, row0 + 16 * at, p) > SL_COS_EPS ? s_inv[at] * c[at] : 0.f;
#pragma unroll
    for (int eb = 0; eb < EB; ++eb) {
      const int e = 16 * eb + 4 * q;
      if (e >= p.E) continue;      // E is a multiple of 4: four columns or none
      sl_f32x4 d;
      if constexpr (COS) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint32_t xb = sl_lds_elem<T>(Ss, row0 + 16 * at, e + k, RB, p);
          d[k] = (dacc[at][eb][k] - pc * (F32 ? __uint_as_float(xb) : bf16_bits_to_f32(xb))) * rs;
        }
      } else {
        d = dacc[at][eb] * p.scale;
      }
      if (p.S > 1) {
        *reinterpret_cast<float4*>(p.ws + ((size_t)blockIdx.y * p.Ns + sr) * p.E + e) = make_float4(d[0], d[1], d[2], d[3]);
      } else if constexpr (F32) {
        *reinterpret_cast<float4*>(static_cast<float*>(p.out) + sr * p.E + e) = make_float4(d[0], d[1], d[2], d[3]);
      } else {
        *reinterpret_cast<uint2*>(static_cast<uint16_t*>(p.out) + sr * p.E + e) =
            make_uint2(f32x2_to_bf16x2_bits(d[0], d[1]), f32x2_to_bf16x2_bits(d[2], d[3]));
      }
    }
  }
}

// S > 1: four columns per thread, the S partial rows summed in range order, rounded once
template <typename T>
__global__ __launch_bounds__(256) void sl_bwd_finish_kernel(const float* __restrict__ ws, int S, int64_t total, void* out) {
  const int64_t i = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= total) return;
  float4 a = *reinterpret_cast<const float4*>(ws + i);
  for (int s = 1; s < S; ++s) {
    const float4 b = *reinterpret_cast<const float4*>(ws + (size_t)s * total + i);
    a.x += b.x;
    a.y += b.y;
    a.z += b.z;
    a.w += b.w;
  }
  if constexpr (std::is_same<T, float>::value) *reinterpret_cast<float4*>(static_cast<float*>(out) + i) = a;
  else *reinterpret_cast<uint2*>(static_cast<uint16_t*>(out) + i) = make_uint2(f32x2_to_bf16x2_bits(a.x, a.y), f32x2_to_bf16x2_bits(a.z, a.w));
}

// ------------------------------------------------------------------------------------------------ host
// Ranges of the streamed rows, a pure function of (stationary rows, streamed rows), as tk_splits of topk.hip: few
// stationary tiles (of 128 rows) are spread over the 256 CUs twice, every range keeps at least 256 rows, and S = 1 once
// the stationary tiles alone fill the chip.
static int sl_splits(int64_t Ns, int64_t Nr) {
  const int64_t tiles = (Ns + 127) / 128;
  if (tiles >= 256) return 1;
  const int64_t want = (512 + tiles - 1) / tiles;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)SL_MAX_SPLITS, Nr / 256}));
}

static void sl_row_layout(SlArgs& p, int E, int dtype) {
  p.E = E;
  p.row_bytes = E * dtype_size(dtype);
  p.nce = p.row_bytes / 16;
  p.nc = (p.nce + 3) / 4 * 4;
  const int w = std::min(16, p.nc & -p.nc);      // the chunk swizzle of topk.hip
  p.sw_mask = w - 1;
  p.sw_shift = w == 16 ? 0 : w == 8 ? 1 : 2;
  p.dma = p.nce == p.nc;
}

template <typename K>
static int sl_go(const char* op, K kern, dim3 grid, int threads, size_t lds, hipStream_t s, const SlArgs& p) {
  if (lds > 64 * 1024 &&
      hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SL_MAX_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TRS_ELAUNCH, "%s: hipFuncSetAttribute(%zu bytes of LDS) failed", op, lds);
  }
  hipLaunchKernelGGL(kern, grid, dim3(threads), lds, s, p);
  return TRS_OK;
}


// S > 1: d_bias[j] = the S partial sums of target j in range order
__global__ __launch_bounds__(256) void sl_dbias_finish_kernel(const float* __restrict__ ws, int S, int64_t Vt, float* out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= Vt) return;
  float a = ws[j];
  for (int s = 1; s < S; ++s) a += ws[(size_t)s * Vt + j];
  out[j] = a;
}

struct SlShape {
  int AR, TR, NW;
};

template <typename T, int X>
static int sl_fwd_launch(const char* op, SlArgs& p, hipStream_t s) {
  // the first arrangement whose anchors and two target tiles (X != SL_PLAIN: and their norms and bias) fit the 160 KB of LDS
  static const SlShape shapes[] = {{32, 128, 4}, {16, 128, 4}, {16, 64, 4}, {16, 64, 2}, {16, 32, 2}, {16, 32, 1}};
  const size_t RB = (size_t)p.nc * 16;
  auto bytes = [&](const SlShape& c) {
    return ((size_t)c.NW * c.AR + 2 * c.TR) * RB + (X != SL_PLAIN ? (size_t)(4 * c.TR + c.NW * c.AR) * 4 : 0);
  };
  const SlShape* sh = nullptr;
  for (const SlShape& c : shapes)
    if (bytes(c) <= SL_MAX_LDS) {
      sh = &c;
      break;
    }
  TRS_REQUIRE(sh != nullptr, TRS_ESHAPE, "%s: no arrangement fits LDS (row %zu bytes)", op, RB);
  const size_t lds = bytes(*sh);
  const int NA = sh->NW * sh->AR;
  const dim3 grid((unsigned)((p.Ns + NA - 1) / NA), (unsigned)p.S);
  int rc;
  if (sh->AR == 32) rc = sl_go(op, sl_fwd_kernel<T, 32, 128, X>, grid, 64 * sh->NW, lds, s, p);
  else if (sh->TR == 128) rc = sl_go(op, sl_fwd_kernel<T, 16, 128, X>, grid, 64 * sh->NW, lds, s, p);
  else if (sh->TR == 64) rc = sl_go(op, sl_fwd_kernel<T, 16, 64, X>, grid, 64 * sh->NW, lds, s, p);
  else rc = sl_go(op, sl_fwd_kernel<T, 16, 32, X>, grid, 64 * sh->NW, lds, s, p);
  if (rc != TRS_OK) return rc;
  if (p.S > 1) hipLaunchKernelGGL(sl_fwd_finish_kernel, dim3((unsigned)((p.Ns + 255) / 256)), dim3(256), 0, s, p);
  return check_launch(op);
}

// one gradient: `p` already holds stationary / streamed rows and their counts
template <typename T, bool DT, int X>
static int sl_bwd_launch(const char* op, SlArgs& p, hipStream_t s) {
  // E > 64 holds 16 column blocks of accumulators per lane: with tiles of 64 rows that kernel spills, so 32 there
  static const SlShape shapes[] = {{SL_BWD_AR, 64, 4}, {SL_BWD_AR, 64, 2}, {SL_BWD_AR, 32, 4}, {SL_BWD_AR, 32, 2},
                                   {SL_BWD_AR, 32, 1}};
  // cosine on wide bf16 rows: the inverse norms and the scalar beside 16 column blocks of two row groups spill (5 VGPRs),
  // so a wave holds one group of 16 stationary rows there
  constexpr int WAR = X == SL_COS && !std::is_same<T, float>::value ? 16 : SL_BWD_AR;
  static const SlShape wide_shapes[] = {{WAR, 32, 4}, {WAR, 32, 2}, {WAR, 32, 1}};
  const size_t RB = (size_t)p.nc * 16;
  const bool wide = p.E > 64;
  auto bytes = [&](const SlShape& c) {      // X != SL_PLAIN: the streamed rows' inverse norms and (dA) bias, [2][TR] each
    return ((size_t)c.NW * c.AR + 2 * c.TR) * RB + (DT ? (size_t)2 * c.TR * 12 : 0) + (X != SL_PLAIN ? (size_t)2 * c.TR * 8 : 0);
  };
  const SlShape* sh = nullptr;
  for (const SlShape& c : shapes)
    if (!wide && bytes(c) <= SL_MAX_LDS && sh == nullptr) sh = &c;
  for (const SlShape& c : wide_shapes)
    if (wide && bytes(c) <= SL_MAX_LDS && sh == nullptr) sh = &c;
  TRS_REQUIRE(sh != nullptr, TRS_ESHAPE, "%s: no arrangement fits LDS (row %zu bytes)", op, RB);
  const int NA = sh->NW * sh->AR;
  const dim3 grid((unsigned)((p.Ns + NA - 1) / NA), (unsigned)p.S);
  int rc;
  if (wide) rc = sl_go(op, sl_bwd_kernel<T, 16, 32, DT, X, WAR>, grid, 64 * sh->NW, bytes(*sh), s, p);
  else if (sh->TR == 64) rc = sl_go(op, sl_bwd_kernel<T, 4, 64, DT, X>, grid, 64 * sh->NW, bytes(*sh), s, p);
  else rc = sl_go(op, sl_bwd_kernel<T, 4, 32, DT, X>, grid, 64 * sh->NW, bytes(*sh), s, p);
  if (rc != TRS_OK) return rc;
  if (p.S > 1) {
    const int64_t total = p.Ns * p.E;
    hipLaunchKernelGGL(sl_bwd_finish_kernel<T>, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, s, p.ws, p.S, total,
                       p.out);
    if (DT && p.dbias != nullptr)
      hipLaunchKernelGGL(sl_dbias_finish_kernel, dim3((unsigned)((p.Ns + 255) / 256)), dim3(256), 0, s, p.ws_db, p.S, p.Ns,
                         p.dbias);
  }
  return check_launch(op);
}

template <typename T>
static int sl_fwd_pick(const char* op, int X, SlArgs& p, hipStream_t s) {
  return X == SL_PLAIN ? sl_fwd_launch<T, SL_PLAIN>(op, p, s)
         : X == SL_BIAS ? sl_fwd_launch<T, SL_BIAS>(op, p, s)
                        : sl_fwd_launch<T, SL_COS>(op, p, s);
}
template <typename T, bool DT>
static int sl_bwd_pick(const char* op, int X, SlArgs& p, hipStream_t s) {
  return X == SL_PLAIN ? sl_bwd_launch<T, DT, SL_PLAIN>(op, p, s)
         : X == SL_BIAS ? sl_bwd_launch<T, DT, SL_BIAS>(op, p, s)
                        : sl_bwd_launch<T, DT, SL_COS>(op, p, s);
}

static size_t sl_fwd_ws(int64_t B, int64_t Vt) {
  const int S = sl_splits(B, Vt);
  return S > 1 ? (size_t)B * S * 8 + (size_t)B * 4 : 0;
}
static size_t sl_bwd_ws(int64_t Ns, int64_t Nr, int E) {
  const int S = sl_splits(Ns, Nr);
  return S > 1 ? (size_t)S * Ns * E * 4 : 0;
}
// the (S, Vt) partials of d_bias behind the target gradient's
static size_t sl_dbias_ws(int64_t Vt, int64_t B) {
  const int S = sl_splits(Vt, B);
  return S > 1 ? (size_t)S * Vt * 4 : 0;
}

static int sl_check(const char* op, int64_t B, int64_t Vt, int32_t E, int32_t dtype, int32_t label_dtype) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", op, dtype);
  TRS_REQUIRE(label_dtype == TRS_I64 || label_dtype == TRS_I32, TRS_EINVAL, "%s: label dtype %d", op, label_dtype);
  TRS_REQUIRE(B >= 0 && B <= INT32_MAX && Vt > 0 && Vt <= INT32_MAX, TRS_EINVAL, "%s: bad size B=%lld Vt=%lld", op,
              (long long)B, (long long)Vt);
  TRS_REQUIRE(E > 0 && E <= SL_MAX_E && (E * dtype_size(dtype)) % 16 == 0, TRS_ESHAPE,
              "%s: E = %d (rows of whole 16-byte vectors, E <= %d)", op, E, SL_MAX_E);
  return TRS_OK;
}

// X of the kernels: the plain instantiations for the inner product without a bias, and nothing else
static int sl_variant(int32_t sim, const float* bias) { return sim == 1 ? SL_COS : bias != nullptr ? SL_BIAS : SL_PLAIN; }

static int sl_fwd_host(const char* op, const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                       int32_t dtype, int32_t sim, const float* bias, const void* labels, int32_t label_dtype,
                       int64_t ignore_index, float scale, float* loss, float* lse, void* workspace, size_t ws_bytes,
                       int32_t* err_flag, trs_stream_t stream) {
  if (int rc = sl_check(op, B, Vt, E, dtype, label_dtype)) return rc;
  TRS_REQUIRE(sim == 0 || sim == 1, TRS_EINVAL, "%s: sim %d (0 inner product, 1 cosine)", op, sim);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(anchors && targets && labels && loss && lse, TRS_EINVAL, "%s: NULL pointer", op);
  TRS_REQUIRE(aligned16(anchors) && aligned16(targets), TRS_EALIGN, "%s: anchors and targets must be 16-byte aligned", op);
  const size_t need = sl_fwd_ws(B, Vt);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need), TRS_EWORKSPACE, "%s: workspace %zu < %zu", op,
              ws_bytes, need);
  SlArgs p = {};
  sl_row_layout(p, E, dtype);
  p.st = static_cast<const char*>(anchors);
  p.sr = static_cast<const char*>(targets);
  p.labels = labels;
  p.lab64 = label_dtype == TRS_I64;
  p.ignore = ignore_index;
  p.bias = bias;
  p.loss = loss;
  p.lse_out = lse;
  p.ws = static_cast<float*>(workspace);
  p.err_flag = err_flag;
  p.Ns = B;
  p.Nr = Vt;
  p.Vt = Vt;
  p.S = sl_splits(B, Vt);
  p.rows_per = (int)((Vt + p.S - 1) / p.S);
  p.scale = scale;
  hipStream_t s = (hipStream_t)stream;
  const int X = sl_variant(sim, bias);
  return dtype == TRS_F32 ? sl_fwd_pick<float>(op, X, p, s) : sl_fwd_pick<bf16_t>(op, X, p, s);
}

static int sl_bwd_host(const char* op, const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                       int32_t dtype, int32_t sim, const float* bias, const void* labels, int32_t label_dtype, float scale,
                       const float* lse, const float* g_loss, void* d_anchors, void* d_targets, float* d_bias,
                       void* workspace, size_t ws_bytes, trs_stream_t stream) {
  if (int rc = sl_check(op, B, Vt, E, dtype, label_dtype)) return rc;
  TRS_REQUIRE(sim == 0 || sim == 1, TRS_EINVAL, "%s: sim %d (0 inner product, 1 cosine)", op, sim);
  TRS_REQUIRE(d_bias == nullptr || (bias != nullptr && d_targets != nullptr), TRS_EINVAL,
              "%s: d_bias needs bias and d_targets (the sum lives in the target-gradient kernel)", op);
  hipStream_t s = (hipStream_t)stream;
  if (B == 0) {      // no sample: the target and bias gradients are zero
    if (d_bias != nullptr)
      if (int rc = zero_bytes(d_bias, (size_t)Vt * 4, s)) return rc;
    if (d_targets != nullptr) return zero_bytes(d_targets, (size_t)Vt * E * dtype_size(dtype), s);
    return TRS_OK;
  }
  TRS_REQUIRE(anchors && targets && labels && lse && g_loss, TRS_EINVAL, "%s: NULL pointer", op);
  TRS_REQUIRE(aligned16(anchors) && aligned16(targets) && aligned16(d_anchors) && aligned16(d_targets), TRS_EALIGN,
              "%s: operands and gradients must be 16-byte aligned", op);
  const size_t need = std::max(d_anchors ? sl_bwd_ws(B, Vt, E) : 0,
                               d_targets ? sl_bwd_ws(Vt, B, E) + (d_bias ? sl_dbias_ws(Vt, B) : 0) : 0);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need && aligned16(workspace)), TRS_EWORKSPACE,
              "%s: workspace %zu < %zu (16-byte aligned)", op, ws_bytes, need);
  SlArgs p = {};
  sl_row_layout(p, E, dtype);
  p.labels = labels;
  p.lab64 = label_dtype == TRS_I64;
  p.lse = lse;
  p.g = g_loss;
  p.bias = bias;
  p.ws = static_cast<float*>(workspace);
  p.Vt = Vt;
  p.scale = scale;
  const int X = sl_variant(sim, bias);
  if (d_anchors != nullptr) {
    p.st = static_cast<const char*>(anchors);
    p.sr = static_cast<const char*>(targets);
    p.Ns = B;
    p.Nr = Vt;
    p.out = d_anchors;
    p.S = sl_splits(B, Vt);
    p.rows_per = (int)((Vt + p.S - 1) / p.S);
    const int rc = dtype == TRS_F32 ? sl_bwd_pick<float, false>(op, X, p, s) : sl_bwd_pick<bf16_t, false>(op, X, p, s);
    if (rc != TRS_OK) return rc;
  }
  if (d_targets != nullptr) {
    p.st = static_cast<const char*>(targets);
    p.sr = static_cast<const char*>(anchors);
    p.Ns = Vt;
    p.Nr = B;
    p.out = d_targets;
    p.dbias = d_bias;
    p.S = sl_splits(Vt, B);
    p.ws_db = p.ws + (size_t)p.S * Vt * E;
    p.rows_per = (int)((B + p.S - 1) / p.S);
    return dtype == TRS_F32 ? sl_bwd_pick<float, true>(op, X, p, s) : sl_bwd_pick<bf16_t, true>(op, X, p, s);
  }
  return TRS_OK;
}

}  // namespace trs

using namespace trs;

extern "C" size_t trs_softmax_loss_workspace_bytes(int64_t B, int64_t Vt, int32_t E, int32_t backward) {
  if (B <= 0 || Vt <= 0 || E <= 0) return 0;
  return backward ? std::max(sl_bwd_ws(B, Vt, E), sl_bwd_ws(Vt, B, E)) : sl_fwd_ws(B, Vt);
}

extern "C" size_t trs_softmax_loss_sim_workspace_bytes(int64_t B, int64_t Vt, int32_t E, int32_t backward) {
  if (B <= 0 || Vt <= 0 || E <= 0) return 0;
  return backward ? std::max(sl_bwd_ws(B, Vt, E), sl_bwd_ws(Vt, B, E) + sl_dbias_ws(Vt, B)) : sl_fwd_ws(B, Vt);
}

extern "C" int trs_softmax_loss_fwd(const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                                    int32_t dtype, const void* labels, int32_t label_dtype, int64_t ignore_index,
                                    float scale, float* loss, float* lse, void* workspace, size_t ws_bytes,
                                    int32_t* err_flag, trs_stream_t stream) {
  return sl_fwd_host("softmax_loss_fwd", anchors, B, targets, Vt, E, dtype, 0, nullptr, labels, label_dtype, ignore_index,
                     scale, loss, lse, workspace, ws_bytes, err_flag, stream);
}

extern "C" int trs_softmax_loss_bwd(const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                                    int32_t dtype, const void* labels, int32_t label_dtype, float scale, const float* lse,
                                    const float* g_loss, void* d_anchors, void* d_targets, void* workspace,
                                    size_t ws_bytes, trs_stream_t stream) {
  return sl_bwd_host("softmax_loss_bwd", anchors, B, targets, Vt, E, dtype, 0, nullptr, labels, label_dtype, scale, lse,
                     g_loss, d_anchors, d_targets, nullptr, workspace, ws_bytes, stream);
}

extern "C" int trs_softmax_loss_sim_fwd(const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                                        int32_t dtype, int32_t sim, const float* bias, const void* labels,
                                        int32_t label_dtype, int64_t ignore_index, float scale, float* loss, float* lse,
                                        void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  return sl_fwd_host("softmax_loss_sim_fwd", anchors, B, targets, Vt, E, dtype, sim, bias, labels, label_dtype,
                     ignore_index, scale, loss, lse, workspace, ws_bytes, err_flag, stream);
}

extern "C" int trs_softmax_loss_sim_bwd(const void* anchors, int64_t B, const void* targets, int64_t Vt, int32_t E,
                                        int32_t dtype, int32_t sim, const float* bias, const void* labels,
                                        int32_t label_dtype, float scale, const float* lse, const float* g_loss,
                                        void* d_anchors, void* d_targets, float* d_bias, void* workspace, size_t ws_bytes,
                                        trs_stream_t stream) {
  return sl_bwd_host("softmax_loss_sim_bwd", anchors, B, targets, Vt, E, dtype, sim, bias, labels, label_dtype, scale, lse,
                     g_loss, d_anchors, d_targets, d_bias, workspace, ws_bytes, stream);
}
