// Top-k retrieval for the embedding models (MatrixFactorization / StarSpace serving, and what hit rate@k / NDCG@k are
// computed from): for every anchor the best k rows of a whole target table, scores on the matrix cores and the selection
// next to the accumulators.  Nothing of the (B, Vt) score matrix is written anywhere.
//
//   score[b, j] = sim(A[a_b], T[lo + j]),  j = 0 .. Vt-1     sim 0: inner product, 1: cosine as rank.hip (eps 1e-8, each
//   out[b, :]   = the k best j by (score descending, j ascending), -inf / -1 behind the last one          norm clamped)
//
// Split.  grid = (anchor tiles) x (S target ranges).  A workgroup of NW waves (4; fewer only where k and the row width
// leave no room in LDS) owns NW * AR anchors: gathered ONCE through the ids into LDS (cosine: with their inverse norms).
// It streams its target range through LDS in tiles of TR rows, double-buffered: rows that are whole 64-byte k-steps go by
// LDS-DMA and land while the current tile is multiplied; other widths are loaded to registers and stored zero-padded.
// LDS rows are XOR-swizzled in 16-byte chunks (chunk c of row r sits at c ^ g(r)), so that the 16 rows an MFMA operand
// load touches fall into 16 different bank groups whatever the row width; the DMA applies the swizzle on the global side.
//
// Scores.  A wave owns AR whole anchor rows against all TR targets of the tile: targets are the MFMA's A operand, anchors
// its B operand, so lane (n, q) holds, for anchor n, the targets 4 q .. 4 q + 3 of every 16-target group.  One anchor's
// scores sit in 4 lanes of one wave and never leave it: no merge across waves exists.  bf16: mfma_f32_16x16x32_bf16, one
// per 64-byte k-step; fp32: four mfma_f32_16x16x4f32 per k-step, the lane's 16 bytes feeding element i of MFMA i (the
// same permutation of k on both operands).
//
// Selection.  Every anchor row keeps tau, the key of its current k-th best, and a candidate buffer of P = pow2 >= max(2 k,
// k + 16) keys in LDS.  A key is 64 bits, larger = better: the score's bits mapped order-preserving into the high word,
// ~id in the low word -- so "score descending, id ascending" is one unsigned compare and the tie rule costs nothing.  Key 0
// is the empty slot.  Per 16-target group a lane compares its 4 scores with tau's score (the common case: nothing passes,
// one ballot); groups with a hit are revisited: full key compare, then the exclusion list (only here: its cost scales
// with insertions, not with Vt), then an LDS counter hands out the slot.  A group adds at most 16 keys to a row and a
// row enters a group with at least 16 free slots; behind the group, rows with fewer are sorted by their wave (bitonic
// network over the P keys, descending), cut to k, and tau rises.
//
// Merge.  S > 1: every (anchor, split) writes its k sorted keys to the workspace and a second kernel, one wave per anchor,
// folds the S lists through the same sort.  S = 1: the first kernel writes values / ids itself.
//
// Q8 targets (template parameter Q8; trs_topk_scores_q8).  The target table is row-wise int8 (q8_common.hpp: a row of E
// codes, fp32 scale, fp32 bias, S = round_up(E + 8, 16) bytes) and the score is taken in the format's factored form:
//   d[b, j] = sum_e a_b[e] c_j[e]  (MFMA; the codes 0..255 are exact in bf16 and fp32)      sa[b] = sum_e a_b[e]  (fp32)
//   score   = d * scale_j + sa * bias_j                                  cosine: * ainv[b] * tinv[j], tinv from the sum of
// squares of c * scale + bias.  LDS-DMA cannot convert, so a Q8 tile goes through registers: a thread owns up to
// TK_Q8_UNITS 16-byte vectors of the tile's rows (tails included, consecutive lanes consecutive vectors), loads those of
// tile t + 1 before the k-loop of tile t, and behind the k-loop converts the codes to the anchor dtype -- each code once per
// workgroup -- and stores them as ordinary swizzled operand chunks into the other buffer; the (scale, bias) words of the
// vectors that hold them go to two per-tile LDS arrays next to tinv, sa sits next to ainv.  Operand loads, k-loop,
// selection and merge are the float kernel's.  Rows past the end of a range stage as code 0, scale 0, bias 0.
//
// Multi-interest (template parameter MI; trs_topk_scores_multi).  A user is G anchors (1 .. 16) and score[u, j] = max_g
// sim(a[u, g], t[j]), each sim the bits above.  Gp = the power of two >= G is a kernel argument (gsh = log2 Gp); MI = false
// compiles to the kernels of one anchor per row unchanged (same registers and occupancy in the compiler's report).  A
// workgroup's NA LDS anchor rows hold NA / Gp users: row r is slot r % Gp of user r / Gp, gathered from the user's interest
// min(slot, G - 1), so a G that is no power of two is padded on chip by repeating the last interest, which leaves the max
// as it is.  A user's Gp rows are Gp adjacent n of one accumulator group, and the max over them is log2 Gp DPP steps on the
// vector ALU (group_max.hpp).  The first pass is the one above, untouched: every lane compares its own interest's scores
// with its user's tau (all Gp lanes carry the same tk / tf), because max_g s_g >= tau iff some s_g >= tau -- no max is
// taken where nothing passes.  Only the revisit pass takes the group max; the leader lane (n % Gp == 0) builds the keys,
// scans excl[u] and inserts, and a new tau goes to all Gp lanes of the user.  Candidate buffers, tauk and cnt exist per
// user, so k = 128 fits a larger arrangement than with one anchor per row; sort, write-out, workspace (U, S, k) and merge
// run per user.  The grid's anchor dimension and the split count U Gp rows.  Registers (compiler's report, no spill):
// 32 x 128 198 + 76 (fp32) / 198 + 64 (bf16) vector + accumulator registers, one wave per SIMD; 16 x 128 150 + 36 / 32, two;
// 16 x 64 96 + 24 / 16, four; 16 x 32 62 + 8, seven: the occupancies of the MI = false kernels.
#include <algorithm>

#include "group_max.hpp"
#include "lds_dma.hpp"
#include "q8_common.hpp"

namespace trs {

typedef __attribute__((ext_vector_type(8))) __bf16 tk_bf16x8;
typedef __attribute__((ext_vector_type(4))) float tk_f32x4;

constexpr int TK_DOT = 0, TK_COS = 1;
constexpr float TK_COS_EPS = 1e-8f;      // rank.hip's COS_EPS
constexpr int TK_MAX_K = 128, TK_MAX_E = 256, TK_MAX_SPLITS = 64;
constexpr int TK_SLACK = 16;             // keys one 16-target group can add to a row: 4 lanes x 4 targets
constexpr size_t TK_MAX_LDS = 160 * 1024;
constexpr int TK_Q8_UNITS = 9;           // 16-byte vectors of a Q8 tile per thread: TR * 17 / threads <= 8.5 in every arrangement

struct TopkArgs {
  const char* a_table;
  const void* a_idx;       // NULL: anchor b is row b
  const char* t_table;
  const void* excl;        // (B, X) or NULL
  float* out_val;
  int64_t* out_idx;
  uint64_t* ws;            // (B, S, k) keys, S > 1
  int32_t* err_flag;
  int64_t Va, a_off, B, t_lo;
  int Vt, rows_per, S, k, P, X;
  int row_bytes;           // E * sizeof(T)
  int nc, nce;             // 16-byte chunks of an LDS row (whole 64-byte k-steps) and of a table row
  int sw_shift, sw_mask;   // g(r) = (r >> sw_shift) & sw_mask
  int sim;
  bool idx64, excl64, dma;
  int E, q_stride, q_nv;   // Q8 targets: columns, bytes of a row (S) and its 16-byte vectors
};
// multi-interest (template parameter MI): B users of G anchors each, in groups of Gp = 1 << gsh LDS rows.  Arguments of
// their own, so that the kernels of one anchor per row keep theirs
struct TopkArgsMI : TopkArgs {
  int G, gsh;
};
template <bool MI>
using TopkArgsOf = std::conditional_t<MI, TopkArgsMI, TopkArgs>;

__device__ __forceinline__ void tk_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ uint64_t tk_key(float s, int id) {
  const uint32_t u = __float_as_uint(s + 0.f);      // -0 -> +0: equal scores, equal bits
  const uint32_t hi = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((uint64_t)hi << 32) | (uint32_t)~(uint32_t)id;
}
__device__ __forceinline__ float tk_key_score(uint64_t key) {
  if (key == 0) return -INFINITY;
  const uint32_t hi = (uint32_t)(key >> 32);
  return __uint_as_float((hi & 0x80000000u) ? (hi & 0x7fffffffu) : ~hi);
}
__device__ __forceinline__ int64_t tk_key_id(uint64_t key) { return key == 0 ? -1 : (int64_t)(~(uint32_t)key); }

// One wave (all 64 lanes) sorts the P keys of a row descending; slots [cnt, P) are emptied first.
__device__ void tk_sort_row(uint64_t* c, int P, int cnt, int lane) {
  for (int i = lane; i < P; i += 64)
    if (i >= cnt) c[i] = 0;
  tk_wave_sync();
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int pr = lane; pr < (P >> 1); pr += 64) {
        const int i = ((pr & ~(stride - 1)) << 1) | (pr & (stride - 1)), j = i | stride;
        const uint64_t a = c[i], b = c[j];
        if ((a < b) == ((i & size) == 0)) {
          c[i] = b;
          c[j] = a;
        }
      }
      tk_wave_sync();
    }
  }
}

template <typename T>
__device__ __forceinline__ tk_f32x4 tk_mma(const uint4& tgt, const uint4& anc, tk_f32x4 acc) {
  if constexpr (std::is_same<T, float>::value) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.x), __uint_as_float(anc.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.y), __uint_as_float(anc.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.z), __uint_as_float(anc.z), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.w), __uint_as_float(anc.w), acc, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tk_bf16x8, tgt), __builtin_bit_cast(tk_bf16x8, anc),
                                                   acc, 0, 0, 0);
  }
}

// squared norm of LDS row r (its real chunks, in order), fp32
template <typename T>
__device__ __forceinline__ float tk_row_sq(const char* rows, int r, const TopkArgs& p) {
  const int g = (r >> p.sw_shift) & p.sw_mask;
  float s = 0.f;
  for (int c = 0; c < p.nce; ++c) {
    float f[Vec16<T>::VE];
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>(rows + ((size_t)r * p.nc + (c ^ g)) * 16), f);
#pragma unroll
    for (int e = 0; e < Vec16<T>::VE; ++e) s += f[e] * f[e];
  }
  return s;
}

// sum of LDS row r (its real chunks, in order), fp32: sa of the factored Q8 score
template <typename T>
__device__ __forceinline__ float tk_row_sum(const char* rows, int r, const TopkArgs& p) {
  const int g = (r >> p.sw_shift) & p.sw_mask;
  float s = 0.f;
  for (int c = 0; c < p.nce; ++c) {
    float f[Vec16<T>::VE];
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>(rows + ((size_t)r * p.nc + (c ^ g)) * 16), f);
#pragma unroll
    for (int e = 0; e < Vec16<T>::VE; ++e) s += f[e];
  }
  return s;
}

// squared norm of the dequantized row whose codes are LDS row r: the sum of squares of c * scale + bias itself (expanded
// into sums of c and c^2 it cancels where bias = the row minimum < 0)
template <typename T>
__device__ __forceinline__ float tk_q8_row_sq(const char* rows, int r, float scale, float bias, const TopkArgs& p) {
  const int g = (r >> p.sw_shift) & p.sw_mask;
  float s = 0.f;
  for (int c = 0; c < p.nce; ++c) {
    float f[Vec16<T>::VE];
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>(rows + ((size_t)r * p.nc + (c ^ g)) * 16), f);
#pragma unroll
    for (int e = 0; e < Vec16<T>::VE; ++e) {
      const float x = f[e] * scale + bias;
      s += x * x;
    }
  }
  return s;
}

template <typename T, int AR, int TR, bool Q8, bool MI>
__global__ __launch_bounds__(256) void topk_scores_kernel(TopkArgsOf<MI> p) {
  static_assert(!(Q8 && MI), "multi-interest scores are taken over float tables only");
  extern __shared__ __attribute__((aligned(16))) char tk_smem[];
  constexpr int AT = AR / 16, NT = TR / 16;
  const int NW = blockDim.x >> 6, NA = NW * AR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int RB = p.nc * 16, P = p.P, k = p.k;
  char* As = tk_smem;
  char* Ts = As + (size_t)NA * RB;
  uint64_t* cand = reinterpret_cast<uint64_t*>(Ts + (size_t)2 * TR * RB);
  // MI: a user is Gp adjacent LDS rows; candidate buffers, tauk and cnt exist per user (16 bytes of them kept whole)
  int gsh = 0, G = 1;
  if constexpr (MI) gsh = p.gsh, G = p.G;
  const int gm = (1 << gsh) - 1, NU = NA >> gsh;
  uint64_t* tauk = cand + (size_t)NU * P;
  int* cnt = reinterpret_cast<int*>(tauk + NU);
  float* ainv = MI ? reinterpret_cast<float*>(reinterpret_cast<char*>(tauk) + ((NU * 12 + 15) & ~15))
                   : reinterpret_cast<float*>(cnt + NA);
  float* tinv = ainv + NA;      // [2][TR]
  float* tsc = tinv + 2 * TR;   // Q8: [2][TR] scales, [2][TR] biases, [NA] anchor sums
  float* tbi = tsc + 2 * TR;
  float* sa = tbi + 2 * TR;
  const bool cosine = p.sim == TK_COS;
  constexpr int CPV = 16 * (int)sizeof(T) / 16;      // operand chunks the 16 codes of one vector become

  // ---- the anchors, once
  // MI: b counts users; LDS row r is slot r & gm of user r >> gsh, loaded from its interest min(slot, G - 1)
  const int64_t b0 = (int64_t)blockIdx.x * NU;
  for (int u = threadIdx.x; u < NA * p.nc; u += blockDim.x) {
    const int r = u / p.nc, c = u - r * p.nc;
    uint4 v = make_uint4(0, 0, 0, 0);
    const int64_t b = b0 + (r >> gsh);
    if (b < p.B) {
      const int64_t ia = MI ? b * G + std::min(r & gm, G - 1) : b;
      int64_t ra = ia;
      if (p.a_idx != nullptr)
        ra = p.idx64 ? static_cast<const int64_t*>(p.a_idx)[ia] : (int64_t) static_cast<const int32_t*>(p.a_idx)[ia];
      ra += p.a_off;
      if (ra < 0 || ra >= p.Va) {      // reads as a zero row
        if (c == 0 && p.err_flag != nullptr) *p.err_flag = 1;
      } else if (c < p.nce) {
        v = *reinterpret_cast<const uint4*>(p.a_table + ra * p.row_bytes + 16 * c);
      }
    }
    *reinterpret_cast<uint4*>(As + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = v;
  }
  for (int r = threadIdx.x; r < NU; r += blockDim.x) {
    cnt[r] = 0;
    tauk[r] = 0;
  }

  // ---- this workgroup's target rows [lo, hi), absolute row numbers of the target table
  const int64_t lo = p.t_lo + (int64_t)blockIdx.y * p.rows_per;
  const int64_t hi = std::min<int64_t>(lo + p.rows_per, p.t_lo + p.Vt);
  const int ntile = hi > lo ? (int)((hi - lo + TR - 1) / TR) : 0;
  auto load_tile = [&](int t, int buf) {
    const int64_t t0 = lo + (int64_t)t * TR;
    char* dst = Ts + (size_t)buf * TR * RB;
    if (p.dma) {      // RB == row_bytes; rows past the end re-read the last one (their scores are masked)
      const char* src = p.t_table + t0 * p.row_bytes;
      const unsigned base = lds_addr(dst);
      const int last = (int)std::min<int64_t>(TR, hi - t0) - 1;
      for (int pc = wave; pc < TR * p.nc / 64; pc += NW) {
        const int u = pc * 64 + lane, r = u / p.nc, cp = u - r * p.nc;
        const int c = cp ^ ((r >> p.sw_shift) & p.sw_mask);
        lds_dma1(src, (unsigned)(std::min(r, last) * p.row_bytes + 16 * c), base + pc * 1024);
      }
    } else {
      for (int u = threadIdx.x; u < TR * p.nc; u += blockDim.x) {
        const int r = u / p.nc, c = u - r * p.nc;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (t0 + r < hi && c < p.nce) v = *reinterpret_cast<const uint4*>(p.t_table + (t0 + r) * p.row_bytes + 16 * c);
        *reinterpret_cast<uint4*>(dst + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = v;
      }
    }
  };
  auto tile_norms = [&](int buf) {
    for (int r = threadIdx.x; r < TR; r += blockDim.x) {
      const char* rows = Ts + (size_t)buf * TR * RB;
      float sq;
      if constexpr (Q8) sq = tk_q8_row_sq<T>(rows, r, tsc[buf * TR + r], tbi[buf * TR + r], p);
      else sq = tk_row_sq<T>(rows, r, p);
      tinv[buf * TR + r] = 1.f / fmaxf(sqrtf(sq), TK_COS_EPS);
    }
  };
  // Q8: unit i of this thread is vector v of tile row r, packed r | v << 8 (-1: none); consecutive threads take
  // consecutive vectors of a row, so a wave's load is one contiguous stretch of the table
  uint4 pre[Q8 ? TK_Q8_UNITS : 1];
  int prv[Q8 ? TK_Q8_UNITS : 1];
  if constexpr (Q8) {
#pragma unroll
    for (int i = 0; i < TK_Q8_UNITS; ++i) {
      const int u = threadIdx.x + i * blockDim.x;
      prv[i] = u < TR * p.q_nv ? ((u / p.q_nv) | ((u % p.q_nv) << 8)) : -1;
    }
    // operand chunks behind the last one a vector is converted into are never staged: zero them once, both buffers
    for (int u = threadIdx.x; u < 2 * TR * p.nc; u += blockDim.x) {
      const int r = u / p.nc, c = u - r * p.nc;
      if (c >= CPV * p.q_nv)
        *reinterpret_cast<uint4*>(Ts + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = make_uint4(0, 0, 0, 0);
    }
  }
  auto q8_fetch = [&](int t) {
    const int64_t t0 = lo + (int64_t)t * TR;
#pragma unroll
    for (int i = 0; i < (Q8 ? TK_Q8_UNITS : 0); ++i) {
      pre[i] = make_uint4(0, 0, 0, 0);
      const int r = prv[i] & 0xff, v = prv[i] >> 8;
      if (prv[i] >= 0 && t0 + r < hi) pre[i] = *reinterpret_cast<const uint4*>(p.t_table + (t0 + r) * p.q_stride + 16 * v);
    }
  };
  auto q8_store = [&](int buf) {
    char* dst = Ts + (size_t)buf * TR * RB;
    const int vs = p.E >> 4, ws = (p.E >> 2) & 3, vb = (p.E + 4) >> 4, wb = ((p.E + 4) >> 2) & 3;      // scale, bias: vector, word
#pragma unroll
    for (int i = 0; i < (Q8 ? TK_Q8_UNITS : 0); ++i) {
      if (prv[i] < 0) continue;
      const int r = prv[i] & 0xff, v = prv[i] >> 8, e0 = 16 * v;
      const uint4 q4 = pre[i];
      if (v == vs) tsc[buf * TR + r] = __uint_as_float(tk_word(q4, ws));
      if (v == vb) tbi[buf * TR + r] = __uint_as_float(tk_word(q4, wb));
      // E is a multiple of 4: a word is all codes or none
      const uint32_t w[4] = {e0 < p.E ? q4.x : 0u, e0 + 4 < p.E ? q4.y : 0u, e0 + 8 < p.E ? q4.z : 0u, e0 + 12 < p.E ? q4.w : 0u};
      char* drow = dst + (size_t)r * RB;
      const int g = (r >> p.sw_shift) & p.sw_mask;
#pragma unroll
      for (int j = 0; j < CPV; ++j) {
        const int cb = CPV * v + j;
        if (cb >= p.nc) continue;
        uint4 o;
        if constexpr (std::is_same<T, float>::value) {
          o = tk_codes_f32(w[j]);
        } else {
          const uint2 a = tk_codes_bf16(w[2 * j]), b = tk_codes_bf16(w[2 * j + 1]);
          o = make_uint4(a.x, a.y, b.x, b.y);
        }
        *reinterpret_cast<uint4*>(drow + ((cb ^ g) << 4)) = o;
      }
    }
  };
  if (ntile > 0) {
    if constexpr (Q8) {
      q8_fetch(0);
      q8_store(0);
    } else {
      load_tile(0, 0);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (cosine || Q8) {
    for (int r = threadIdx.x; r < NA; r += blockDim.x) {
      if (cosine) ainv[r] = 1.f / fmaxf(sqrtf(tk_row_sq<T>(As, r, p)), TK_COS_EPS);
      if constexpr (Q8) sa[r] = tk_row_sum<T>(As, r, p);
    }
    if (cosine && ntile > 0) tile_norms(0);
    __syncthreads();
  }

  // ---- per lane: anchor n of each of the wave's AT groups of 16
  const int row0 = wave * AR + n;                         // + 16 at
  const int gsw = (n >> p.sw_shift) & p.sw_mask;          // g(r) depends on r & 15 only
  uint64_t tk[AT];
  float tf[AT], ai[AT], sav[AT];
  bool rowok[AT];
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    tk[at] = 0;
    tf[at] = -INFINITY;
    rowok[at] = (MI ? b0 + ((row0 + 16 * at) >> gsh) : b0 + row0 + 16 * at) < p.B;
    ai[at] = cosine ? ainv[row0 + 16 * at] : 1.f;
    sav[at] = Q8 ? sa[row0 + 16 * at] : 0.f;
  }
  const int nks = p.nc >> 2;

  for (int t = 0; t < ntile; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntile) {
      if constexpr (Q8) q8_fetch(t + 1);
      else load_tile(t + 1, buf ^ 1);
    }
    const char* Tb = Ts + (size_t)buf * TR * RB;
    tk_f32x4 acc[AT][NT];
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[at][nt] = tk_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      const int coff = ((4 * ks + q) ^ gsw) << 4;
      uint4 bf[AT];
#pragma unroll
      for (int at = 0; at < AT; ++at) bf[at] = *reinterpret_cast<const uint4*>(As + (row0 + 16 * at) * RB + coff);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const uint4 af = *reinterpret_cast<const uint4*>(Tb + (16 * nt + n) * RB + coff);
#pragma unroll
        for (int at = 0; at < AT; ++at) acc[at][nt] = tk_mma<T>(af, bf[at], acc[at][nt]);
      }
    }
    if constexpr (Q8) {
      // the next tile: converted behind the issued MFMAs into the buffer the last tile left (the barrier at its end)
      if (t + 1 < ntile) q8_store(buf ^ 1);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float4 sc = *reinterpret_cast<const float4*>(tsc + buf * TR + 16 * nt + 4 * q);
        const float4 bi = *reinterpret_cast<const float4*>(tbi + buf * TR + 16 * nt + 4 * q);
#pragma unroll
        for (int at = 0; at < AT; ++at) {
          acc[at][nt][0] = acc[at][nt][0] * sc.x + sav[at] * bi.x;
          acc[at][nt][1] = acc[at][nt][1] * sc.y + sav[at] * bi.y;
          acc[at][nt][2] = acc[at][nt][2] * sc.z + sav[at] * bi.z;
          acc[at][nt][3] = acc[at][nt][3] * sc.w + sav[at] * bi.w;
        }
      }
    }
    if (cosine) {
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const float4 ti = *reinterpret_cast<const float4*>(tinv + buf * TR + 16 * nt + 4 * q);
#pragma unroll
        for (int at = 0; at < AT; ++at) {
          acc[at][nt][0] = acc[at][nt][0] * ai[at] * ti.x;
          acc[at][nt][1] = acc[at][nt][1] * ai[at] * ti.y;
          acc[at][nt][2] = acc[at][nt][2] * ai[at] * ti.z;
          acc[at][nt][3] = acc[at][nt][3] * ai[at] * ti.w;
        }
      }
    }

    // ---- selection.  First pass, unrolled: which 16-target groups hold a score that reaches its row's tau
    const int64_t t0 = lo + (int64_t)t * TR;
    const int valid = (int)std::min<int64_t>(TR, hi - t0);      // targets of this tile that exist
    const int idbase = (int)(t0 - p.t_lo);
    uint32_t hit = 0;
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        bool any = false;
#pragma unroll
        for (int j = 0; j < 4; ++j) any |= acc[at][nt][j] >= tf[at] && 16 * nt + 4 * q + j < valid;
        if (__ballot(any && rowok[at]) != 0) hit |= 1u << (at * NT + nt);
      }
    // second pass, one copy of the code: the groups with a hit, in order
    while (hit != 0) {
      const int g = __builtin_ctz(hit);
      hit &= hit - 1;
      const int at = g / NT, nt = g - at * NT;
      tk_f32x4 s4 = acc[0][0];
      uint64_t tkey = tk[0];
      bool ok = rowok[0];
#pragma unroll
      for (int a = 0; a < AT; ++a)
#pragma unroll
        for (int m = 0; m < NT; ++m)
          if (g == a * NT + m) {
            s4 = acc[a][m];
            tkey = tk[a];
            ok = rowok[a];
          }
      const int row = (row0 + 16 * at) >> gsh;      // the row of the buffers: MI the user, whose leader lane inserts
      const int64_t b = b0 + row;
      if constexpr (MI) {
#pragma unroll
        for (int j = 0; j < 4; ++j) s4[j] = group_max(s4[j], gsh);
        ok = ok && (n & gm) == 0;
      }
      bool full = false;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int local = 16 * nt + 4 * q + j;
        const uint64_t key = tk_key(s4[j], idbase + local);
        bool pass = ok && local < valid && s4[j] == s4[j] && key > tkey;
        if (pass && p.excl != nullptr) {
          const int64_t id = idbase + local;
          for (int x = 0; x < p.X && pass; ++x) {
            const int64_t e = p.excl64 ? static_cast<const int64_t*>(p.excl)[b * p.X + x]
                                       : (int64_t) static_cast<const int32_t*>(p.excl)[b * p.X + x];
            pass = e != id;
          }
        }
        if (pass) {
          const int slot = atomicAdd(&cnt[row], 1);
          cand[(size_t)row * P + slot] = key;
          full |= slot + 1 > P - TK_SLACK;
        }
      }
      tk_wave_sync();
      uint64_t need = __ballot(full);
      while (need != 0) {
        const int rn = (__builtin_ffsll((long long)need) - 1) & 15;
        need &= ~(0x0001000100010001ull << rn);
        const int r = (wave * AR + 16 * at + rn) >> gsh;
        uint64_t* c = cand + (size_t)r * P;
        tk_sort_row(c, P, cnt[r], lane);
        const uint64_t nk = c[k - 1];
        tk_wave_sync();
        if (lane == 0) {
          cnt[r] = std::min(cnt[r], k);
          tauk[r] = nk;
        }
        tk_wave_sync();
        if ((n & ~gm) == rn) {      // the row's lanes: MI every interest of the user
#pragma unroll
          for (int a = 0; a < AT; ++a)
            if (a == at) {
              tk[a] = nk;
              tf[a] = tk_key_score(nk);
            }
        }
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (cosine && t + 1 < ntile) {
      tile_norms(buf ^ 1);
      __syncthreads();
    }
  }

  // ---- every row's best k, sorted: to the output (S == 1) or to the workspace as keys
  for (int rr = 0; rr < (AR >> gsh); ++rr) {
    const int r = wave * (AR >> gsh) + rr;
    const int64_t b = b0 + r;
    if (b >= p.B) break;
    uint64_t* c = cand + (size_t)r * P;
    tk_sort_row(c, P, cnt[r], lane);
    for (int i = lane; i < k; i += 64) {
      const uint64_t key = c[i];
      if (p.S == 1) {
        p.out_val[b * k + i] = tk_key_score(key);
        p.out_idx[b * k + i] = tk_key_id(key);
      } else {
        p.ws[(b * p.S + blockIdx.y) * k + i] = key;
      }
    }
  }
}

// one wave per anchor: the S sorted lists of k keys -> the best k
__global__ __launch_bounds__(64) void topk_merge_kernel(const uint64_t* __restrict__ ws, int S, int k, int P,
                                                        float* __restrict__ out_val, int64_t* __restrict__ out_idx) {
  extern __shared__ __attribute__((aligned(16))) char tk_smem[];
  uint64_t* c = reinterpret_cast<uint64_t*>(tk_smem);
  const int lane = threadIdx.x;
  const int64_t b = blockIdx.x;
  const int per = (P - k) / k;      // lists that fit behind the kept k: at least 1
  int cnt = 0;
  for (int s0 = 0; s0 < S; s0 += per) {
    const int m = std::min(per, S - s0) * k;
    for (int i = lane; i < m; i += 64) c[cnt + i] = ws[(b * S + s0) * k + i];
    tk_sort_row(c, P, cnt + m, lane);
    cnt = std::min(cnt + m, k);
  }
  for (int i = lane; i < k; i += 64) {
    const uint64_t key = c[i];
    out_val[b * k + i] = tk_key_score(key);
    out_idx[b * k + i] = tk_key_id(key);
  }
}

// ------------------------------------------------------------------------------------------------ host
static int tk_buffer_keys(int k) {
  int P = 32;
  while (P < std::max(2 * k, k + TK_SLACK)) P <<= 1;
  return P;
}

// Target ranges, a pure function of (B, Vt): a small B is spread over the 256 CUs (two workgroups each, counted in
// nominal tiles of 128 anchors), every range keeps at least two tiles of 128 rows, and S = 1 once the anchor tiles alone
// fill the chip.
static int tk_splits(int64_t B, int64_t Vt) {
  const int64_t tiles_a = (B + 127) / 128;
  if (tiles_a >= 256) return 1;
  const int64_t want = (512 + tiles_a - 1) / tiles_a;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)TK_MAX_SPLITS, Vt / 256}));
}

struct TopkShape {
  int AR, TR, NW;
};
static size_t tk_lds_bytes(const TopkShape& s, int RB, int P, bool q8, int gsh) {
  const size_t NA = (size_t)s.NW * s.AR, NU = NA >> gsh;      // candidate buffers, tauk and cnt: one per user
  // Q8: the tiles' scales and biases, the anchors' sums
  return NA * RB + (size_t)2 * s.TR * RB + NU * P * 8 + ((NU * 12 + 15) & ~(size_t)15) + NA * 4 + (size_t)2 * s.TR * 4 +
         (q8 ? (size_t)2 * s.TR * 8 + NA * 4 : 0);
}

template <typename T, bool Q8, bool MI>
static int topk_launch(const char* op, const TopkArgsMI& p, int RB, hipStream_t s) {
  // the first arrangement whose anchors, two target tiles and candidate buffers fit the 160 KB of LDS
  static const TopkShape shapes[] = {{32, 128, 4}, {16, 128, 4}, {16, 64, 4}, {16, 64, 2}, {16, 32, 2}, {16, 32, 1}};
  const TopkShape* sh = nullptr;
  for (const TopkShape& c : shapes)
    if (tk_lds_bytes(c, RB, p.P, Q8, p.gsh) <= TK_MAX_LDS) {
      sh = &c;
      break;
    }
  TRS_REQUIRE(sh != nullptr, TRS_ESHAPE, "%s: no arrangement fits LDS (row %d bytes, k %d)", op, RB, p.k);
  TRS_REQUIRE(!Q8 || (sh->TR * p.q_nv + 64 * sh->NW - 1) / (64 * sh->NW) <= TK_Q8_UNITS, TRS_ESHAPE,
              "%s: a tile of %d rows x %d vectors exceeds %d per thread", op, sh->TR, p.q_nv, TK_Q8_UNITS);
  const size_t lds = tk_lds_bytes(*sh, RB, p.P, Q8, p.gsh);
  const int NA = (sh->NW * sh->AR) >> p.gsh;      // users of a workgroup
  const dim3 grid((unsigned)((p.B + NA - 1) / NA), (unsigned)p.S);
  auto go = [&](auto kern) -> int {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TK_MAX_LDS) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TRS_ELAUNCH, "%s: hipFuncSetAttribute(%zu bytes of LDS) failed", op, lds);
    }
    hipLaunchKernelGGL(kern, grid, dim3(64 * sh->NW), lds, s, static_cast<const TopkArgsOf<MI>&>(p));
    return TRS_OK;
  };
  int rc;
  if (sh->AR == 32) rc = go(topk_scores_kernel<T, 32, 128, Q8, MI>);
  else if (sh->TR == 128) rc = go(topk_scores_kernel<T, 16, 128, Q8, MI>);
  else if (sh->TR == 64) rc = go(topk_scores_kernel<T, 16, 64, Q8, MI>);
  else rc = go(topk_scores_kernel<T, 16, 32, Q8, MI>);
  if (rc != TRS_OK) return rc;
  if (p.S > 1)
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)p.B), dim3(64), (size_t)p.P * 8, s, p.ws, p.S, p.k, p.P, p.out_val,
                       p.out_idx);
  return check_launch(op);
}

// the workspace of `users` result rows whose anchor tiles are filled as by `rows` anchor rows: (users, S, k) keys, S > 1
static size_t tk_workspace_bytes(int64_t users, int64_t rows, int64_t Vt, int32_t k) {
  if (users <= 0 || Vt <= 0 || k < 1 || k > TK_MAX_K) return 0;
  const int S = tk_splits(rows, Vt);
  return S > 1 ? (size_t)users * S * k * sizeof(uint64_t) : 0;
}

// all entries: `dtype` is the anchors' (and, for float targets, the table's); q8: target_table holds Q8 rows of E columns;
// G = 0: one anchor per result row (U unused); G >= 1: the multi-interest entry, B = U * G anchors, user-major
static int topk_entry(const char* op, bool q8, int64_t U, int32_t G, const void* anchor_table, int64_t Va, const void* anchor_idx,
                      int32_t idx_dtype, int64_t anchor_offset, int64_t B, const void* target_table, int64_t target_lo,
                      int64_t target_hi, int32_t E, int32_t dtype, int32_t sim, int32_t k, const void* exclude,
                      int32_t excl_dtype, int32_t X, float* out_val, int64_t* out_idx, void* workspace, size_t ws_bytes,
                      int32_t* err_flag, trs_stream_t stream) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", op, dtype);
  TRS_REQUIRE(sim == TK_DOT || sim == TK_COS, TRS_EINVAL, "%s: sim %d (0 = inner product, 1 = cosine)", op, sim);
  TRS_REQUIRE(anchor_idx == nullptr || idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EINVAL, "%s: idx dtype %d", op,
              idx_dtype);
  TRS_REQUIRE(exclude == nullptr || ((excl_dtype == TRS_I64 || excl_dtype == TRS_I32) && X >= 1), TRS_EINVAL,
              "%s: exclude dtype %d, X = %d (X >= 1)", op, excl_dtype, X);
  const int64_t Vt = target_hi - target_lo;
  TRS_REQUIRE(Va > 0 && B >= 0 && target_lo >= 0 && Vt > 0 && Vt <= INT32_MAX, TRS_EINVAL,
              "%s: bad size Va=%lld B=%lld targets [%lld, %lld)", op, (long long)Va, (long long)B, (long long)target_lo,
              (long long)target_hi);
  TRS_REQUIRE(k >= 1 && k <= TK_MAX_K && k <= Vt, TRS_EINVAL, "%s: k = %d (1 .. %d, at most the %lld targets)", op, k,
              TK_MAX_K, (long long)Vt);
  const bool multi = G != 0;
  TRS_REQUIRE(!multi || (G >= 1 && G <= 16 && U >= 0 && B == U * G), TRS_EINVAL,
              "%s: G = %d (1 .. 16), U = %lld (>= 0), B = %lld (U * G)", op, G, (long long)U, (long long)B);
  const int gsh = multi ? gm_shift(G) : 0;
  const int64_t users = multi ? U : B, rows = multi ? U << gsh : B;      // rows: what the anchor tiles are filled with
  const int row_bytes = E * dtype_size(dtype);
  TRS_REQUIRE(E > 0 && E <= TK_MAX_E && row_bytes % 16 == 0, TRS_ESHAPE,
              "%s: E = %d (rows of whole 16-byte vectors, E <= %d)", op, E, TK_MAX_E);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(anchor_table && target_table && out_val && out_idx, TRS_EINVAL, "%s: NULL pointer", op);
  TRS_REQUIRE(aligned16(anchor_table) && aligned16(target_table), TRS_EALIGN, "%s: tables must be 16-byte aligned", op);
  const size_t need = tk_workspace_bytes(users, rows, Vt, k);
  TRS_REQUIRE(need == 0 || (workspace != nullptr && ws_bytes >= need), TRS_EWORKSPACE, "%s: workspace %zu < %zu", op,
              ws_bytes, need);
  TopkArgsMI p;
  p.a_table = static_cast<const char*>(anchor_table);
  p.a_idx = anchor_idx;
  p.t_table = static_cast<const char*>(target_table);
  p.excl = exclude;
  p.out_val = out_val;
  p.out_idx = out_idx;
  p.ws = static_cast<uint64_t*>(workspace);
  p.err_flag = err_flag;
  p.Va = Va;
  p.a_off = anchor_offset;
  p.B = users;
  p.G = multi ? G : 1;
  p.gsh = gsh;
  p.t_lo = target_lo;
  p.Vt = (int)Vt;
  p.S = tk_splits(rows, Vt);
  p.rows_per = (int)((Vt + p.S - 1) / p.S);
  p.k = k;
  p.P = tk_buffer_keys(k);
  p.X = exclude != nullptr ? X : 0;
  p.row_bytes = row_bytes;
  p.nce = row_bytes / 16;
  p.nc = (p.nce + 3) / 4 * 4;
  // chunk swizzle: r * nc mod 16 takes 16 / w values (w = the power of two in nc, at most 16); the other bits of r & 15
  // go into the low bits of the chunk number
  const int w = std::min(16, p.nc & -p.nc);
  p.sw_mask = w - 1;
  p.sw_shift = w == 16 ? 0 : w == 8 ? 1 : 2;
  p.sim = sim;
  p.idx64 = idx_dtype == TRS_I64;
  p.excl64 = excl_dtype == TRS_I64;
  p.dma = !q8 && p.nce == p.nc;
  p.E = E;
  p.q_stride = (int)q8_stride(E);
  p.q_nv = p.q_stride / 16;
  hipStream_t s = (hipStream_t)stream;
  if (multi)
    return dtype == TRS_F32 ? topk_launch<float, false, true>(op, p, p.nc * 16, s)
                            : topk_launch<bf16_t, false, true>(op, p, p.nc * 16, s);
  if (q8)
    return dtype == TRS_F32 ? topk_launch<float, true, false>(op, p, p.nc * 16, s)
                            : topk_launch<bf16_t, true, false>(op, p, p.nc * 16, s);
  return dtype == TRS_F32 ? topk_launch<float, false, false>(op, p, p.nc * 16, s)
                          : topk_launch<bf16_t, false, false>(op, p, p.nc * 16, s);
}

}  // namespace trs

using namespace trs;

extern "C" size_t trs_topk_scores_workspace_bytes(int64_t B, int64_t Vt, int32_t k) {
  return tk_workspace_bytes(B, B, Vt, k);
}

extern "C" size_t trs_topk_scores_multi_workspace_bytes(int64_t U, int32_t G, int64_t Vt, int32_t k) {
  if (G < 1 || G > 16) return 0;
  return tk_workspace_bytes(U, U << gm_shift(G), Vt, k);
}

extern "C" int trs_topk_scores(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                               int64_t anchor_offset, int64_t B, const void* target_table, int64_t target_lo,
                               int64_t target_hi, int32_t E, int32_t dtype, int32_t sim, int32_t k, const void* exclude,
                               int32_t excl_dtype, int32_t X, float* out_val, int64_t* out_idx, void* workspace,
                               size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  return topk_entry("topk_scores", false, 0, 0, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_table, target_lo,
                    target_hi, E, dtype, sim, k, exclude, excl_dtype, X, out_val, out_idx, workspace, ws_bytes, err_flag,
                    stream);
}

extern "C" int trs_topk_scores_q8(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                                  int64_t anchor_offset, int64_t B, const void* target_q, int64_t target_lo,
                                  int64_t target_hi, int32_t E, int32_t anchor_dtype, int32_t sim, int32_t k,
                                  const void* exclude, int32_t excl_dtype, int32_t X, float* out_val, int64_t* out_idx,
                                  void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  return topk_entry("topk_scores_q8", true, 0, 0, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_q, target_lo,
                    target_hi, E, anchor_dtype, sim, k, exclude, excl_dtype, X, out_val, out_idx, workspace, ws_bytes,
                    err_flag, stream);
}

extern "C" int trs_topk_scores_multi(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                                     int64_t anchor_offset, int64_t B, int64_t U, int32_t G, const void* target_table,
                                     int64_t target_lo, int64_t target_hi, int32_t E, int32_t dtype, int32_t sim, int32_t k,
                                     const void* exclude, int32_t excl_dtype, int32_t X, float* out_val, int64_t* out_idx,
                                     void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  TRS_REQUIRE(G >= 1 && G <= 16, TRS_EINVAL, "topk_scores_multi: G = %d (1 .. 16)", G);
  return topk_entry("topk_scores_multi", false, U, G, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_table,
                    target_lo, target_hi, E, dtype, sim, k, exclude, excl_dtype, X, out_val, out_idx, workspace, ws_bytes,
                    err_flag, stream);
}
