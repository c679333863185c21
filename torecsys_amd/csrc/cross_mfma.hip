// K4 on the matrix cores (bf16): x_{l+1} = x0 * (x_l W_l^T + b_l) + x0 for all L layers of a 16-row tile
// without leaving registers.
//
// Formulation: Y^T = W * X^T with v_mfma_f32_16x16x32_bf16:  A = W tile (M = e_out, K = e_in),
// B = X^T (K = e_in, N = 16 rows), D = Y^T (M = e_out, N = rows).  D's lane layout is
// (col = lane&15 -> row r of x, rows 4*(lane>>4)+i -> e_out slot), B's is (col = lane&15 -> r,
// k = 8*(lane>>4)+j).  The rows of W are fed in a permuted order
//     e_out(mt, q, i) = 32*(mt>>1) + 8*q + 4*(mt&1) + i          (mt = M-tile, q = lane>>4, i = reg)
// so that the 16 outputs a lane holds for its row r are exactly the 8-element chunks [32c+8q, 32c+8q+8)
// of that row: the NEXT layer's B operand is the lane's own registers (converted to bf16, no shuffle,
// no LDS), x0/out move as 16-byte vectors, and the elementwise epilogue x0*(u+b)+x0 is lane-local (the
// bias enters as the accumulator's initial value).  W_l fragments are pre-packed once per call into
// fragment order (1 KiB per (layer, mt, ks), lane-linear -> conflict-free ds_read_b128) and kept in LDS.
// HBM traffic: x read once, out written once (2*E*2 bytes per row); FLOPs 2*E*E*L per row on MFMA.
#include <stdlib.h>

#include <algorithm>

#include "trs_common.hpp"

namespace trs {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

// e_out of D-row slot (mt, m) where m = 4*q + i is the row inside the 16-row M tile
__host__ __device__ __forceinline__ int cross_row_of_slot(int mt, int m) {
  return 32 * (mt >> 1) + 8 * (m >> 2) + 4 * (mt & 1) + (m & 3);
}

// Pre-pack: Wp[(l*NT + mt)*KS + ks][lane][8] = W_l[row(mt, lane&15)][32*ks + 8*(lane>>4) + 0..7]
// Wtp (optional, backward): the same fragment order for W_l^T, layers 1 .. L-1 (the gradient chain g_l = W_l^T du_l;
// layer 0's is only needed without the detach quirk and is then read out of the forward fragments):
//   Wtp[((l-1)*NT + mt)*KS + ks][lane][8] = W_l[32*ks + 8*(lane>>4) + 0..7][row(mt, lane&15)]
__global__ __launch_bounds__(256) void cross_prepack_kernel(const bf16_t* __restrict__ W, const bf16_t* __restrict__ b,
                                                            bf16_t* __restrict__ Wp, float* __restrict__ bp, int E,
                                                            int L, bf16_t* __restrict__ Wtp = nullptr) {
  const int NT = E / 16, KS = E / 32;
  const int total = L * NT * KS * 64;
  for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
    const int lane = t & 63;
    int f = t >> 6;
    const int ks = f % KS;
    f /= KS;
    const int mt = f % NT;
    const int l = f / NT;
    const int row = cross_row_of_slot(mt, lane & 15);
    const int k0 = 32 * ks + 8 * (lane >> 4);
    const bf16_t* Wl = W + (size_t)l * E * E;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      Wp[(size_t)t * 8 + j] = Wl[(size_t)row * E + k0 + j];
    if (Wtp != nullptr && l > 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j)
        Wtp[((size_t)t - (size_t)NT * KS * 64) * 8 + j] = Wl[(size_t)(k0 + j) * E + row];
    }
  }
  if (bp != nullptr)
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < L * E; t += gridDim.x * blockDim.x) bp[t] = to_f32(b[t]);
}

template <int NT>
struct XTile {
  float v[NT][4];  // D layout: v[mt][i] <-> e = 32*(mt>>1) + 8*q + 4*(mt&1) + i of row r = lane&15
};

template <int NT>
__device__ __forceinline__ void load_tile(const uint4* __restrict__ x, int64_t row, int64_t rows, int E, int q,
                                          XTile<NT>& t, uint4* raw) {
  constexpr int KS = NT / 2;
#pragma unroll
  for (int c = 0; c < KS; ++c) {
    uint4 u = make_uint4(0, 0, 0, 0);
    if (row < rows) u = x[(row * E + 32 * c + 8 * q) >> 3];
    raw[c] = u;
    float f[8];
    Vec16<bf16_t>::unpack(u, f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t.v[2 * c][i] = f[i];
      t.v[2 * c + 1][i] = f[4 + i];
    }
  }
}

template <int NT>
__device__ __forceinline__ void pack_tile(const XTile<NT>& t, uint4* raw) {
  constexpr int KS = NT / 2;
#pragma unroll
  for (int c = 0; c < KS; ++c) {
    float f[8];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      f[i] = t.v[2 * c][i];
      f[4 + i] = t.v[2 * c + 1][i];
    }
    raw[c] = Vec16<bf16_t>::pack(f);
  }
}

// one layer for TP tiles at once: acc[t][mt] = bias + sum_ks A[mt][ks] * B[t][ks]; every A fragment read
// from LDS feeds TP MFMAs, and the TP independent chains let the MFMA of one tile overlap the VALU
// epilogue of the other inside a single wave.
template <int NT, int TP>
__device__ __forceinline__ void layer_matmul(const uint4* __restrict__ Wfrag /* [NT][KS][64] */,
                                             const float* __restrict__ bias /* [E] or null */,
                                             const uint4 (*B)[NT / 2], int lane, int q, f32x4 (*acc)[NT]) {
  constexpr int KS = NT / 2;
#pragma unroll
  for (int mt = 0; mt < NT; ++mt) {
    f32x4 init = f32x4{0.f, 0.f, 0.f, 0.f};
    if (bias != nullptr) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1));
      init = f32x4{bv.x, bv.y, bv.z, bv.w};
    }
#pragma unroll
    for (int t = 0; t < TP; ++t) acc[t][mt] = init;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
      const uint4 a = Wfrag[(mt * KS + ks) * 64 + lane];
#pragma unroll
      for (int t = 0; t < TP; ++t)
        acc[t][mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a),
                                                             __builtin_bit_cast(bf16x8, B[t][ks]), acc[t][mt], 0, 0, 0);
    }
  }
}

// RESIDENT: all layers' fragments + biases are copied into LDS once per workgroup; otherwise they are
// read from the pre-packed global buffer (L1/L2-resident) -- large E*E*L only.
template <int NT, bool RESIDENT>
__global__ __launch_bounds__(256) void cross_mfma_fwd_kernel(const uint4* __restrict__ x,
                                                             const uint4* __restrict__ Wp,
                                                             const float* __restrict__ bp, int64_t rows, int L,
                                                             uint4* __restrict__ out) {
  constexpr int KS = NT / 2;
  constexpr int E = NT * 16;
  constexpr int TP = NT <= 4 ? 2 : 1;           // tiles per wave iteration
  constexpr int FRAG_PER_LAYER = NT * KS * 64;  // uint4 units
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const uint4* Wl = Wp;
  const float* bl = bp;
  if (RESIDENT) {
    uint4* Ws = reinterpret_cast<uint4*>(smem);
    float* bs = reinterpret_cast<float*>(smem + (size_t)L * FRAG_PER_LAYER * 16);
    for (int i = threadIdx.x; i < L * FRAG_PER_LAYER; i += blockDim.x) Ws[i] = Wp[i];
    for (int i = threadIdx.x; i < L * E; i += blockDim.x) bs[i] = bp[i];
    __syncthreads();
    Wl = Ws;
    bl = bs;
  }
  const int lane = threadIdx.x & 63, q = lane >> 4, r = lane & 15;
  const int64_t ngroups = (rows + 16 * TP - 1) / (16 * TP);
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  // The rows of the NEXT group are requested while this one runs through its L layers: a group is one dependent chain
  // (load -> L x (MFMAs -> epilogue) -> store) and only three waves share a SIMD (the resident W fragments take 48 KB of
  // LDS per workgroup).  Hand-issued loads, addresses clamped into the tensor (every lane issues every load), waited
  // for after the last layer and before this group's stores.
  typedef __attribute__((ext_vector_type(4))) unsigned cx_u32x4;
  cx_u32x4 nxt[TP][KS];
#define TRS_CX_FETCH(g_)                                                                              \
  _Pragma("unroll") for (int t = 0; t < TP; ++t) {                                                    \
    int64_t rr_ = ((g_) * TP + t) * 16 + r;                                                           \
    rr_ = rr_ < rows ? rr_ : rows - 1;                                                                \
    _Pragma("unroll") for (int c = 0; c < KS; ++c) {                                                  \
      const uint4* a_ = x + ((rr_ * E + 32 * c + 8 * q) >> 3);                                        \
      asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(nxt[t][c]) : "v"(a_));                    \
    }                                                                                                 \
  }
#define TRS_CX_COMMIT()                                                                               \
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                    \
  _Pragma("unroll") for (int t = 0; t < TP; ++t)                                                      \
    _Pragma("unroll") for (int c = 0; c < KS; ++c) asm volatile("" : "+v"(nxt[t][c]));
  if (wave < ngroups) {
    TRS_CX_FETCH(wave)
    TRS_CX_COMMIT()
  }
  for (int64_t grp = wave; grp < ngroups; grp += nwaves) {
    XTile<NT> x0[TP], cur[TP];
    uint4 B[TP][KS];
    int64_t row[TP];
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      row[t] = (grp * TP + t) * 16 + r;
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        uint4 u = make_uint4(nxt[t][c][0], nxt[t][c][1], nxt[t][c][2], nxt[t][c][3]);
        if (row[t] >= rows) u = make_uint4(0, 0, 0, 0);
        B[t][c] = u;
        float f[8];
        Vec16<bf16_t>::unpack(u, f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          x0[t].v[2 * c][i] = f[i];
          x0[t].v[2 * c + 1][i] = f[4 + i];
        }
      }
    }
    {
      const int64_t gn = grp + nwaves < ngroups ? grp + nwaves : grp;
      TRS_CX_FETCH(gn)
    }
    __builtin_amdgcn_sched_barrier(0);
    for (int l = 0; l < L; ++l) {
      f32x4 acc[TP][NT];
      layer_matmul<NT, TP>(Wl + (size_t)l * FRAG_PER_LAYER, bl + l * E, B, lane, q, acc);
#pragma unroll
      for (int t = 0; t < TP; ++t) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) cur[t].v[mt][i] = fmaf(x0[t].v[mt][i], acc[t][mt][i], x0[t].v[mt][i]);
        pack_tile<NT>(cur[t], B[t]);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
    TRS_CX_COMMIT()
#pragma unroll
    for (int t = 0; t < TP; ++t) {
      if (row[t] < rows) {
#pragma unroll
        for (int c = 0; c < KS; ++c) out[(row[t] * E + 32 * c + 8 * q) >> 3] = B[t][c];
      }
    }
  }
#undef TRS_CX_FETCH
#undef TRS_CX_COMMIT
}

// ---------------------------------------------------------------------------------------------
// backward: helpers shared by the role-specialised kernel below (chain waves own row tiles, dW waves own the E*E*L
// weight-gradient accumulators; du / x rows are handed over through LDS slabs laid out [16-column panel][row][16 columns]
// so that ds_read_b64_tr_b16 delivers [row][e] data with rows along K -- directly the A (du^T) and B (x) operands).
// Round 2's forward-first kernel (cross_mfma_bwd2_kernel: x store of all L layers in LDS, 1.0-1.08 ms at 2.5 M rows) was
// superseded by cross_mfma_bwd3_kernel in round 3 and removed in round 4.
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((ext_vector_type(8))) short s16x8;

// fp32 value (mt, i) of a row held as bf16 B fragments (the D-layout slot order of XTile)
template <int KS>
__device__ __forceinline__ float frag_value(const uint4 (&B)[KS], int mt, int i) {
  const uint4& u = B[mt >> 1];
  const unsigned w = (mt & 1) ? (i < 2 ? u.z : u.w) : (i < 2 ? u.x : u.y);
  return (i & 1) ? __uint_as_float(w & 0xffff0000u) : __uint_as_float(w << 16);
}

// A operand of g^T = W^T du^T for output slot tile mt' and k-step ks', read out of the FORWARD fragments of the layer
// (Wl: [mt][ks][64 lanes][8 bf16], lane 16*b + m of fragment (mt, ks) holds W[row(mt, m)][32*ks + 8*b .. +7]).
// Wanted per lane (q' = lane>>4, m' = lane&15): W[32*ks' + 8*q' + j][row(mt', m')], j = 0..7.  With
// row(mt, m) = 32*(mt>>1) + 8*(m>>2) + 4*(mt&1) + (m&3): rows 32*ks' + 8*q' + (0..3 | 4..7) are lanes 4*q' + (0..3) of
// fragment rows mt = 2*ks' (| 2*ks'+1), and column row(mt', 4*b' + d') is element 4*(mt'&1) + d' of the chunk of lane
// group b' in fragment column mt'>>1 -- so source lane s = 4*j + b' of a transpose read points at 4 contiguous bf16.
template <int KS>
__device__ __forceinline__ bf16x8 wt_frag(const uint4* Wl, int mtp, int ksp, int lane) {
  typedef __attribute__((address_space(3))) s16x4* lds_p;
  const int qp = lane >> 4, sl = lane & 15;
  const char* p = reinterpret_cast<const char*>(Wl) + ((2 * ksp) * KS + (mtp >> 1)) * 1024 +
                  (16 * (sl & 3) + 4 * qp + (sl >> 2)) * 16 + 8 * (mtp & 1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p + KS * 1024));
  const s16x8 v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// acc[mt] = bias + sum_ks A[mt][ks] * B[ks] with every A fragment of the layer requested before the first MFMA
// (TRANSPOSED: the fragments of W^T, no bias)
template <int NT, bool TRANSPOSED>
__device__ __forceinline__ void layer_matmul_pre(const uint4* Wl, const float* bias, const uint4 (&B)[NT / 2], int lane,
                                                 int q, f32x4 (&acc)[NT]) {
  constexpr int KS = NT / 2;
  bf16x8 A[NT][KS];
#pragma unroll
  for (int mt = 0; mt < NT; ++mt)
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
      A[mt][ks] = TRANSPOSED ? wt_frag<KS>(Wl, mt, ks, lane) : __builtin_bit_cast(bf16x8, Wl[(mt * KS + ks) * 64 + lane]);
#pragma unroll
  for (int mt = 0; mt < NT; ++mt) {
    if (!TRANSPOSED && bias != nullptr) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1));
      acc[mt] = f32x4{bv.x, bv.y, bv.z, bv.w};
    } else {
      acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks)
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[mt][ks], __builtin_bit_cast(bf16x8, B[ks]), acc[mt], 0, 0, 0);
}

// ---------------------------------------------------------------------------------------------
// backward, round 3: gradient chain FIRST, forward recompute SECOND.
//
// The gradient chain needs no activation at all: du_l = g_{l+1} * x0, g_l = W_l^T du_l depends only on the incoming
// gradient, x0 and the weights.  Only dx0 += g_{l+1} * (u_l + 1) and dW_l += du_l^T x_l need the forward values, and both
// consume them in FORWARD order.  So a tile (16 rows, one chain wave) runs
//   phase A  g_L -> g_{L-1} -> ... -> g_1 (-> g_0 without the detach quirk): L-1 matmuls with W_l^T, the g_l kept as
//            packed bf16 registers (the role the u_l + 1 registers played in cross_mfma_bwd2); no slab traffic, no barrier;
//   phase B  x_0 -> x_1 -> ... : per layer one forward matmul (u_l + 1), dx0 += g_{l+1} (u_l + 1), du_l = g_{l+1} x0 and
//            x_l handed to the dW waves through double-buffered slabs, x_{l+1} = x0 (u_l + 1); one barrier per layer.
// Against cross_mfma_bwd2 (forward first): no x store of all L layers in LDS (48 KiB -> two 12 KiB slab pairs), which
// pays for (a) 96 rows per group with SIX chain waves beside two dW waves (two waves per SIMD, 256 registers: two SIMDs
// host a pair of chain waves that overlap each other's MFMA and VALU phases, two host a chain wave beside a dW wave
// that holds half of the E*E*L accumulators; six barriers per 96 rows instead of seven per 64.  Twelve waves -- eight
// chain, four dW, three per SIMD on 168 registers -- was built first: hipcc spills ~100 registers of the chain waves
// there and the kernel ran 2.4 ms) and (b) a second, TRANSPOSED set of W fragments for phase A: reading W^T out of the forward fragments with
// ds_read_b64_tr_b16 is a 4-way bank conflict by construction (the four 256-byte quarters of a fragment a 16-lane group
// gathers from map to the same banks; no swizzle that keeps the forward ds_read_b128 conflict-free gets below 2-way) --
// counters of the first version of this kernel: half of all LDS cycles were conflict cycles, LDS 65 % busy.
// Slab layout: [16-column panel][row][32 B], the two 16-byte halves of a row piece swapped for rows with bit 2 set (the
// 8 lanes of a ds_write_b128 group then hit 8 different bank quads) and the dW waves' transpose reads take rows
// k0..k0+3 first on even lane groups, k0+4..k0+7 first on odd ones (the two groups of a 32-lane half then cover all 64
// banks; the permutation of k is the same for both MFMA operands).
// LDS at E = 64, L = 6: W 48 KiB + W^T (layers 1..5) 40 KiB + biases 1.5 KiB + slabs 48 KiB = 137.5 KiB.
// wave roles per workgroup, the same for both E (NT = E / 16): E = 32 has only NT * NT = 4 dW tiles per layer, i.e. at
// most two dW waves that own whole row tiles
template <int NT>
struct B3 {
  static constexpr int CHAIN = 6;                                 // chain waves per workgroup (one 16-row tile each)
  static constexpr int DW = 2;                                    // weight-gradient waves
  static constexpr int ROWS = CHAIN * 16;                         // rows per workgroup step
  static constexpr int PANEL = ROWS * 32;                         // bytes of one 16-column panel of a slab
};

// 8 k-values (rows) x this lane's column of panel ``panel``: two transpose reads of a [4 rows][16 cols] block each
template <int PANEL_BYTES>
__device__ __forceinline__ s16x8 rows_frag3(const char* tensor, int k0, int panel, int i, int q) {
  typedef __attribute__((address_space(3))) s16x4* lds_p;
  const int cq = i & 3, odd = q & 1;
  const char* base = tensor + panel * PANEL_BYTES + (k0 + (i >> 2)) * 32 + (cq & 1) * 8;
  const int h0 = (cq >> 1) * 16, h1 = 16 - h0;                 // rows with bit 2 clear / set: halves swapped
  const char* p_lo = base + (odd ? 4 * 32 + h1 : h0);
  const char* p_hi = base + (odd ? h0 : 4 * 32 + h1);
  const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p_lo));
  const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(p_hi));
  return s16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int NT>
__device__ __forceinline__ void unpack_tile(const uint4* raw, XTile<NT>& t) {
#pragma unroll
  for (int c = 0; c < NT / 2; ++c) {
    float f[8];
    Vec16<bf16_t>::unpack(raw[c], f);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      t.v[2 * c][i] = f[i];
      t.v[2 * c + 1][i] = f[4 + i];
    }
  }
}

// acc[mt] = bias + sum_ks A[mt][ks] * B[ks], the fragments of ONE k-step in registers at a time (16 instead of 32 at
// E = 64: the chain waves of cross_mfma_bwd3 live on 168 registers; the other chain wave of the SIMD covers the latency)
template <int NT>
__device__ __forceinline__ void layer_matmul_ks(const uint4* Wl, const float* bias, const uint4 (&B)[NT / 2], int lane,
                                                int q, f32x4 (&acc)[NT]) {
  constexpr int KS = NT / 2;
#pragma unroll
  for (int mt = 0; mt < NT; ++mt) {
    if (bias != nullptr) {
      const float4 bv = *reinterpret_cast<const float4*>(bias + 32 * (mt >> 1) + 8 * q + 4 * (mt & 1));
      acc[mt] = f32x4{bv.x, bv.y, bv.z, bv.w};
    } else {
      acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) {
    bf16x8 A[NT];
#pragma unroll
    for (int mt = 0; mt < NT; ++mt) A[mt] = __builtin_bit_cast(bf16x8, Wl[(mt * KS + ks) * 64 + lane]);
#pragma unroll
    for (int mt = 0; mt < NT; ++mt)
      acc[mt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(A[mt], __builtin_bit_cast(bf16x8, B[ks]), acc[mt], 0, 0, 0);
  }
}

// (slab hand-over by LDS counters instead of barriers: 760-780 vs 633-679 us, profiles/r06_logs/ab_cross_flags.txt)
template <int NT, int L, bool DETACH>
__global__ __launch_bounds__(64 * (B3<NT>::CHAIN + B3<NT>::DW), 2) void cross_mfma_bwd3_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ gout, const uint4* __restrict__ Wp,
    const uint4* __restrict__ Wtp, const float* __restrict__ bp, int64_t rows, uint4* __restrict__ dx,
    float* __restrict__ dWpart, float* __restrict__ dbpart) {
  constexpr int detach_first = DETACH ? 1 : 0;
  constexpr int B3_CHAIN = B3<NT>::CHAIN, B3_DW = B3<NT>::DW, B3_ROWS = B3<NT>::ROWS, B3_PANEL = B3<NT>::PANEL;
  constexpr int KS = NT / 2;
  constexpr int E = NT * 16;
  constexpr int FRAG = NT * KS * 64;            // uint4 per layer
  constexpr int TENSOR = NT * B3_PANEL;         // one (128-row x E) bf16 slab in the panel layout
  constexpr int TPW = NT * NT / B3_DW;          // dW output tiles per dW wave
  static_assert((NT * NT) % B3_DW == 0, "E must be a multiple of 32");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4* Ws = reinterpret_cast<uint4*>(smem);                 // forward fragments, layers 0 .. L-1
  uint4* Wts = Ws + L * FRAG;                                 // transposed fragments, layers 1 .. L-1
  float* bs = reinterpret_cast<float*>(Wts + (L - 1) * FRAG);
  char* duslab = reinterpret_cast<char*>(bs + L * E);         // [slot 2][panel NT][B3_ROWS][32 B]
  char* xslab = duslab + 2 * TENSOR;                          // same
  for (int i = threadIdx.x; i < L * FRAG; i += blockDim.x) Ws[i] = Wp[i];
  for (int i = threadIdx.x; i < (L - 1) * FRAG; i += blockDim.x) Wts[i] = Wtp[i];
  for (int i = threadIdx.x; i < L * E; i += blockDim.x) bs[i] = bp[i] + 1.f;      // the backward only ever needs u_l + 1
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, r = lane & 15;
  const int64_t ngroups = (rows + B3_ROWS - 1) / B3_ROWS;
  int step = 0;                                  // global step counter (slab slot = step & 1)

  if (wave < B3_CHAIN) {
    // ------------------------------------------------------------------ chain waves
    uint4 nx_raw[KS], ng_raw[KS];
    // Prefetch of the next group's rows: UNCONDITIONAL loads (row index clamped into the tensor, out-of-range rows zeroed
    // when consumed) -- loads under a branch make hipcc's wait-count insertion wait for them wherever an older load is
    // consumed.  Issued in the middle of phase B, when the first two g_l registers of the group are dead (the wave lives
    // on a tight register budget), consumed after the group's last step.
    auto fetch = [&](int64_t grp_) {
      int64_t row_ = grp_ * B3_ROWS + wave * 16 + r;
      row_ = row_ < rows ? row_ : rows - 1;
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        nx_raw[c] = x[(row_ * E + 32 * c + 8 * q) >> 3];
        ng_raw[c] = gout[(row_ * E + 32 * c + 8 * q) >> 3];
      }
    };
    constexpr int FETCH_AT = L >= 3 ? 2 : L - 1;
    uint4 x0raw[KS], Gp[L + 1][KS];    // packed bf16: x0 (the layer-0 B operand); g_l of every layer (g_L = the input)
    auto take = [&](int64_t grp_) {
      const bool live = grp_ * B3_ROWS + wave * 16 + r < rows;
#pragma unroll
      for (int c = 0; c < KS; ++c) {
        x0raw[c] = live ? nx_raw[c] : make_uint4(0, 0, 0, 0);
        Gp[L][c] = live ? ng_raw[c] : make_uint4(0, 0, 0, 0);
      }
    };
    fetch(blockIdx.x);
    take(blockIdx.x);
    // this lane's 16-byte pieces of a slab: piece c covers columns 32c+8q .. +7 -> panel 2c + (q>>1), half q&1 (swapped
    // for rows with bit 2 set)
    const int piece0 = (q >> 1) * B3_PANEL + (wave * 16 + r) * 32 + (((q & 1) ^ ((r >> 2) & 1)) * 16);
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
      // LDS addresses are re-derived from two laundered lane offsets in every group: left alone, LICM keeps ~40
      // loop-invariant per-fragment / per-slot addresses in registers for the whole kernel (LDS offsets beyond 64 KiB
      // do not fit the DS immediate) and the wave, which lives on 168 registers, spills its g_l to scratch
      int lane16 = lane * 16, pc0 = piece0;
      asm volatile("" : "+v"(lane16), "+v"(pc0));
      const uint4* Wsl = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Ws) + lane16);
      const uint4* Wtsl = reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(Wts) + lane16);
      XTile<NT> x0f;                   // fp32 copy of this tile's x0 rows
      unpack_tile<NT>(x0raw, x0f);
      // ---- phase A: the gradient chain, layers L-1 .. 1 (.. 0 without the detach quirk)
      {
        XTile<NT> g;
        unpack_tile<NT>(Gp[L], g);
#pragma unroll
        for (int l = L - 1; l >= 0; --l) {
          if (l > 0 || detach_first == 0) {
            XTile<NT> du;
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
              for (int i = 0; i < 4; ++i) du.v[mt][i] = g.v[mt][i] * x0f.v[mt][i];
            uint4 Bdu[KS];
            pack_tile<NT>(du, Bdu);
            f32x4 ga[NT];
            if (l > 0) layer_matmul_ks<NT>(Wtsl + (l > 0 ? l - 1 : 0) * FRAG, nullptr, Bdu, 0, q, ga);
            else layer_matmul_pre<NT, true>(Ws, nullptr, Bdu, lane, q, ga);      // W_0^T out of the forward fragments
#pragma unroll
            for (int mt = 0; mt < NT; ++mt)
#pragma unroll
              for (int i = 0; i < 4; ++i) g.v[mt][i] = ga[mt][i];
            pack_tile<NT>(g, Gp[l]);
          }
        }
      }
      // ---- phase B: forward recompute; dx0, and du_l / x_l for the dW waves
      XTile<NT> dx0;
#pragma unroll
      for (int mt = 0; mt < NT; ++mt)
#pragma unroll
        for (int i = 0; i < 4; ++i) dx0.v[mt][i] = 0.f;
      // (Issuing x_{l+1} and the MFMAs of layer l+1 before the rest of layer l -- a software pipeline inside the wave --
      // was built and measured: +16 accumulator registers push the wave into scratch and the kernel ran 727 vs ~650 us.)
      uint4 Bx[KS];
#pragma unroll
      for (int c = 0; c < KS; ++c) Bx[c] = x0raw[c];
#pragma unroll
      for (int l = 0; l < L; ++l, ++step) {
        if (l == FETCH_AT) fetch(grp + gridDim.x);
        f32x4 up[NT];                                   // u_l + 1 (the +1 rides in the bias)
        layer_matmul_ks<NT>(Wsl + l * FRAG, bs + l * E, Bx, 0, q, up);
        XTile<NT> du;
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const float gv = frag_value<KS>(Gp[l + 1], mt, i);
            dx0.v[mt][i] = fmaf(gv, up[mt][i], dx0.v[mt][i]);
            du.v[mt][i] = gv * x0f.v[mt][i];
          }
        uint4 Bdu[KS];
        pack_tile<NT>(du, Bdu);
        char* dslot = duslab + ((step & 1) ? TENSOR : 0) + pc0;
        char* xslot = xslab + ((step & 1) ? TENSOR : 0) + pc0;
#pragma unroll
        for (int c = 0; c < KS; ++c) {
          *reinterpret_cast<uint4*>(dslot + 2 * c * B3_PANEL) = Bdu[c];
          *reinterpret_cast<uint4*>(xslot + 2 * c * B3_PANEL) = Bx[c];
        }
        if (l + 1 < L) {
          XTile<NT> nx;
#pragma unroll
          for (int mt = 0; mt < NT; ++mt)
#pragma unroll
            for (int i = 0; i < 4; ++i) nx.v[mt][i] = x0f.v[mt][i] * up[mt][i];
          pack_tile<NT>(nx, Bx);
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if (detach_first == 0) {
#pragma unroll
        for (int mt = 0; mt < NT; ++mt)
#pragma unroll
          for (int i = 0; i < 4; ++i) dx0.v[mt][i] += frag_value<KS>(Gp[0], mt, i);
      }
      const int64_t row = grp * B3_ROWS + wave * 16 + r;
      if (row < rows) {
        uint4 raw[KS];
        pack_tile<NT>(dx0, raw);
#pragma unroll
        for (int c = 0; c < KS; ++c) dx[(row * E + 32 * c + 8 * q) >> 3] = raw[c];
      }
      take(grp + gridDim.x);
    }
  } else {
    // ------------------------------------------------------------------ dW waves
    // wave wq owns output tiles t = wq*TPW .. +TPW-1, t -> (row tile mo = t / NT, column tile no = t % NT): whole row
    // tiles (TPW is a multiple of NT), so it also owns db of its MO row tiles.  db_l = du_l^T 1 rides on the matrix pipe:
    // one more MFMA per A fragment whose B operand is the one-hot column l (ones in column l, zeros elsewhere), so ONE
    // accumulator tile per row tile collects the sums of all L <= 16 layers, layer l in column l.  (Summing the A
    // fragments on the VALU, as cross_mfma_bwd2 does, made these waves the critical path: 5.9 -> 9.9 us per 96 rows.)
    const int wq = wave - B3_CHAIN;
    constexpr int MO = TPW / NT;
    static_assert(TPW % NT == 0 && MO >= 1 && L <= 16, "a dW wave owns whole row tiles; db columns = layers");
    f32x4 dWacc[L][TPW], dbacc[MO];
#pragma unroll
    for (int m = 0; m < MO; ++m) dbacc[m] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
      for (int k = 0; k < TPW; ++k) dWacc[l][k] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    for (int64_t grp = blockIdx.x; grp < ngroups; grp += gridDim.x) {
#pragma unroll
      for (int l = 0; l < L; ++l, ++step) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                   // the chain waves have written slot step & 1 (layer l)
        const char* du_t = duslab + ((step & 1) ? TENSOR : 0);
        const char* x_t = xslab + ((step & 1) ? TENSOR : 0);
        const unsigned hot = (r == l) ? 0x3f803f80u : 0u;               // bf16 1.0 pairs in column l
        const uint4 onehot = make_uint4(hot, hot, hot, hot);
#pragma unroll
        for (int ks = 0; ks < B3_ROWS / 32; ++ks) {
          s16x8 Bf[NT];
#pragma unroll
          for (int no = 0; no < NT; ++no) Bf[no] = rows_frag3<B3_PANEL>(x_t, 32 * ks + 8 * q, no, r, q);
#pragma unroll
          for (int m = 0; m < MO; ++m) {
            const s16x8 A = rows_frag3<B3_PANEL>(du_t, 32 * ks + 8 * q, wq * MO + m, r, q);
#pragma unroll
            for (int no = 0; no < NT; ++no)
              dWacc[l][m * NT + no] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
                  __builtin_bit_cast(bf16x8, A), __builtin_bit_cast(bf16x8, Bf[no]), dWacc[l][m * NT + no], 0, 0, 0);
            dbacc[m] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, A),
                                                               __builtin_bit_cast(bf16x8, onehot), dbacc[m], 0, 0, 0);
          }
        }
      }
    }
    // partial results of this workgroup: D layout -> (row m = 4q+i -> e_out, col n = r -> e_in)
    float* myW = dWpart + (size_t)blockIdx.x * L * E * E;
    float* myb = dbpart + (size_t)blockIdx.x * L * E;
#pragma unroll
    for (int l = 0; l < L; ++l) {
#pragma unroll
      for (int k = 0; k < TPW; ++k) {
        const int mo = wq * MO + k / NT, no = k % NT;
#pragma unroll
        for (int i = 0; i < 4; ++i) myW[(size_t)l * E * E + (16 * mo + 4 * q + i) * E + 16 * no + r] = dWacc[l][k][i];
      }
    }
    if (r < L) {                           // column r of the db tiles = layer r
#pragma unroll
      for (int m = 0; m < MO; ++m)
#pragma unroll
        for (int i = 0; i < 4; ++i) myb[r * E + 16 * (wq * MO + m) + 4 * q + i] = dbacc[m][i];
    }
  }
}

// out[i] += sum_p part[p][i]: 64 elements per workgroup, the partials split sixteen ways over the waves (fixed order:
// the sum does not depend on timing), four loads in flight per thread
__global__ __launch_bounds__(1024) void cross_reduce_partials_kernel(const float* __restrict__ part, int nparts,
                                                                     int n, float* __restrict__ out) {
  __shared__ float red[16][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + tx;
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  if (i < n) {
    int p = ty;
    for (; p + 48 < nparts; p += 64) {
      s0 += part[(size_t)p * n + i];
      s1 += part[(size_t)(p + 16) * n + i];
      s2 += part[(size_t)(p + 32) * n + i];
      s3 += part[(size_t)(p + 48) * n + i];
    }
    for (; p < nparts; p += 16) s0 += part[(size_t)p * n + i];
  }
  red[ty][tx] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (ty == 0 && i < n) {
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) s += red[k][tx];
    out[i] += s;
  }
}

constexpr int BW_MAX_BLOCKS = 256;      // one persistent workgroup per CU

static size_t cross_pack_bytes(int E, int L) { return (size_t)L * E * E * 2; }

size_t cross_mfma_workspace_bytes(int E, int L) {
  // [W fragments][bias fp32][per-workgroup dW partials][db partials][W^T fragments (backward)], each 256-byte aligned
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  return al(cross_pack_bytes(E, L)) + al((size_t)L * E * 4) + al((size_t)BW_MAX_BLOCKS * L * E * E * 4) +
         al((size_t)BW_MAX_BLOCKS * L * E * 4) + al(cross_pack_bytes(E, L));
}

static bool cross_mfma_covers(int E, int L) { return E % 32 == 0 && E >= 32 && E <= 128 && L >= 1; }

int cross_mfma_fwd(const void* x, const void* W, const void* b, int64_t rows, int E, int L, void* out,
                   void* workspace, size_t ws_bytes, hipStream_t s) {
  if (!cross_mfma_covers(E, L) || !aligned16(x) || !aligned16(out) || workspace == nullptr) return 1;
  if (ws_bytes < cross_mfma_workspace_bytes(E, L)) return fail(TRS_EWORKSPACE, "cross_fwd: workspace too small");
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  bf16_t* Wp = (bf16_t*)workspace;
  float* bp = (float*)((char*)workspace + al(cross_pack_bytes(E, L)));
  hipLaunchKernelGGL((cross_prepack_kernel), dim3(std::min(64, (L * E * E / 8 + 255) / 256)), dim3(256), 0, s,
                     (const bf16_t*)W, (const bf16_t*)b, Wp, bp, E, L);
  const size_t lds = cross_pack_bytes(E, L) + (size_t)L * E * 4;
  const bool resident = lds <= 64 * 1024;
  const int64_t ntiles = (rows + 15) / 16;
  const int grid = (int)std::min<int64_t>((ntiles + 7) / 8, resident ? 256 * 3 : 256 * 8);
  dispatch_int<2, 4, 6, 8>(E / 16, [&](auto nt_c) {      // cross_mfma_covers: E = 32, 64, 96 or 128
    constexpr int NT = decltype(nt_c)::value;
    if (resident)
      hipLaunchKernelGGL((cross_mfma_fwd_kernel<NT, true>), dim3(grid), dim3(256), lds, s, (const uint4*)x,
                         (const uint4*)Wp, bp, rows, L, (uint4*)out);
    else
      hipLaunchKernelGGL((cross_mfma_fwd_kernel<NT, false>), dim3(grid), dim3(256), 0, s, (const uint4*)x,
                         (const uint4*)Wp, bp, rows, L, (uint4*)out);
  });
  return check_launch("cross_fwd(mfma)");
}

template <int NT, int L>
static int cross_bwd_launch(const void* x, const void* g, const uint4* Wp, const uint4* Wtp, const float* bp,
                            int64_t rows, void* dx, float* dWpart, float* dbpart, float* dW, float* db,
                            int detach_first, hipStream_t s) {
  constexpr int E = NT * 16;
  int grid;
  {
    constexpr int B3_CHAIN = B3<NT>::CHAIN, B3_DW = B3<NT>::DW, B3_ROWS = B3<NT>::ROWS, B3_PANEL = B3<NT>::PANEL;
    const size_t lds = (size_t)(2 * L - 1) * E * E * 2 + (size_t)L * E * 4 + (size_t)4 * NT * B3_PANEL;
    auto kern = detach_first ? cross_mfma_bwd3_kernel<NT, L, true> : cross_mfma_bwd3_kernel<NT, L, false>;
    static bool attr_set[2] = {false, false};
    if (!attr_set[detach_first ? 1 : 0]) {
      if (hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
        return check_launch("cross_bwd(mfma): LDS attribute");
      attr_set[detach_first ? 1 : 0] = true;
    }
    const int64_t ngroups = (rows + B3_ROWS - 1) / B3_ROWS;
    grid = (int)std::min<int64_t>(ngroups, BW_MAX_BLOCKS);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(64 * (B3_CHAIN + B3_DW)), lds, s, (const uint4*)x, (const uint4*)g, Wp, Wtp,
                       bp, rows, (uint4*)dx, dWpart, dbpart);
  }
  hipLaunchKernelGGL(cross_reduce_partials_kernel, dim3((L * E * E + 63) / 64), dim3(1024), 0, s, dWpart, grid,
                     L * E * E, dW);
  hipLaunchKernelGGL(cross_reduce_partials_kernel, dim3((L * E + 63) / 64), dim3(1024), 0, s, dbpart, grid, L * E, db);
  return check_launch("cross_bwd(mfma)");
}

int cross_mfma_bwd(const void* x, const void* W, const void* b, const void* g, int64_t rows, int E, int L, void* dx,
                   float* dW, float* db, int detach_first, void* workspace, size_t ws_bytes, hipStream_t s) {
  if (!(E == 32 || E == 64) || L < 1 || L > 6 || !aligned16(x) || !aligned16(g) || !aligned16(dx) ||
      workspace == nullptr)
    return 1;
  if (ws_bytes < cross_mfma_workspace_bytes(E, L)) return fail(TRS_EWORKSPACE, "cross_bwd: workspace too small");
  auto al = [](size_t v) { return (v + 255) / 256 * 256; };
  char* ws = (char*)workspace;
  bf16_t* Wp = (bf16_t*)ws;
  float* bp = (float*)(ws + al(cross_pack_bytes(E, L)));
  float* dWpart = (float*)((char*)bp + al((size_t)L * E * 4));
  float* dbpart = (float*)((char*)dWpart + al((size_t)BW_MAX_BLOCKS * L * E * E * 4));
  bf16_t* Wtp = (bf16_t*)((char*)dbpart + al((size_t)BW_MAX_BLOCKS * L * E * 4));
  const int pgrid = std::min(64, (L * E * E / 8 + 255) / 256);
  hipLaunchKernelGGL((cross_prepack_kernel), dim3(pgrid), dim3(256), 0, s, (const bf16_t*)W, (const bf16_t*)b, Wp, bp, E,
                     L, Wtp);
  int rc = TRS_OK;      // E = 32 or 64 and 1 <= L <= 6 by the test above
  dispatch_int<2, 4>(E / 16, [&](auto nt_c) {
    dispatch_int<1, 2, 3, 4, 5, 6>(L, [&](auto l_c) {
      rc = cross_bwd_launch<decltype(nt_c)::value, decltype(l_c)::value>(x, g, (const uint4*)Wp, (const uint4*)Wtp, bp, rows,
                                                                         dx, dWpart, dbpart, dW, db, detach_first, s);
    });
  });
  return rc;
}

}  // namespace trs
