// Rank of held-out targets over a whole target table (what hit rate@k, NDCG@k, MRR and MAP derive from): for every anchor
// b and each of its P labels the number of targets that sort in front of the label,
//
//   rank[b, p] = #{ j in [0, Vt) : j != l, j not in exclude[b, :], (score[b, j], -j) > (score[b, l], -l) },  l = labels[b, p]
//
// i.e. the 0-based position l takes in topk_scores(..., exclude) with an unbounded k: score descending, id ascending among
// equal scores.  score[b, j] = sim(A[a_b], T[lo + j]) as topk.hip (sim 0: inner product, 1: cosine, eps 1e-8, each norm
// clamped).  A rank is a count against a threshold that is known in advance, so there is no selection: two kernels.
//
// 1. List kernel: the scores of an anchor against its OWN listed rows, the P labels first, then the X excluded ids.  One
// wave per anchor.  The ids are staged in LDS (a label outside [0, Vt) or negative, an excluded id outside it: -1), the
// rows are gathered through them into LDS 16 at a time and multiplied as the A operand of the streaming kernel's MFMA
// against the anchor's row as every column of the B operand: the same instruction, k-step order, permutation of k, zero
// padding and cosine multiply order as below, so the score of a pair (a, t) is the same bits in both kernels -- else
// ties and copies of a row would be miscounted.  15/16 of each MFMA is waste; the work is 16 B (P + X) E against B Vt E.
// It writes label_scores and starts rank[b, p] at -(number of live excluded ids that sort in front of label p): an
// excluded id is live when it is in range, is not label p and is the first occurrence of its id in the list (each entry
// scans the entries before it in LDS: quadratic in X, hence TR_MAX_X).  A label that is not ranked starts, and stays, at -1.
//
// 2. Streaming kernel: the count.  The split is topk.hip's: grid = (anchor tiles) x (S target ranges); a workgroup of 4
// waves owns 4 AR anchors, gathered once into LDS; its target range streams through LDS in double-buffered tiles of TR
// rows, by LDS-DMA where rows are whole 64-byte k-steps, through registers and zero-padded otherwise; LDS rows carry the
// 16-byte-chunk XOR swizzle; targets are the A operand and anchors the B operand, so lane (n, q) holds, for anchor n, the
// targets 4 q .. 4 q + 3 of every 16-target group.  Behind a tile the lane compares its scores with anchor n's P
// thresholds and adds to P integer counters in registers.  Ids rise along a tile, so "score first, id among equals" is
// one float compare per score: a tile that lies wholly in front of the label counts s >= th, written s > below(th) with
// below(th) the next float under th; a tile wholly behind it counts s > th.  The one tile that holds the label (and
// every tile where th is -inf, which has no float under it) also adds its equal scores with a smaller id, element by
// element, behind one ballot.  A NaN never counts and nothing sorts in front of a NaN.  Rows past the end of a range
// are set to -inf first.  At the end the 4 q lanes of an anchor are summed in the wave and the (anchor, split, p) count
// goes into rank[b, p] by a 64-bit integer atomic add: integer sums do not depend on their order, the result is the
// same from run to run, and no workspace and no third launch exist.
//
// Arrangements (AR anchors per wave, TR targets per tile).  Without candidate buffers the LDS holds operands only, and
// what topk.hip spends on them goes into the anchors: AR = 64, 256 anchors per workgroup.  Every target tile that comes
// from L2 then serves 256 anchors (topk.hip at k = 100: 64), and a k-step is 4 + 4 operand loads for 16 MFMAs (16 x 64:
// 1 + 4 for 4).  TR stays 64: the accumulators of 64 x 64 are 64 registers and the kernel keeps two waves per SIMD, which
// it needs, because the comparisons run on the vector ALU while another wave's MFMAs run; 64 x 128 compiled to 365
// registers, one wave per SIMD, and was dropped before any run.  For the same reason the first two arrangements, (64, 64)
// and (32, 64), are taken only where anchors and two target tiles fit 80 KiB, two workgroups per CU: rows up to 128 bytes
// (bf16 E <= 64) take 64 x 64 in 49.5 KiB, rows up to 256 bytes 32 x 64; wider rows take the first of (32, 64) and (16, 32)
// that fits 160 KiB.  Thresholds and counters are registers for P = 1 and P <= 4; above that the thresholds sit in LDS
// (p-major) and the counters stay registers, with AR <= 32.  The arrangements have not been timed against each other.
//
// Q8 targets (template parameter Q8 of both kernels; trs_target_ranks_q8).  The target table is row-wise int8
// (q8_common.hpp: E codes, fp32 scale, fp32 bias, S = round_up(E + 8, 16) bytes a row) and the score is topk.hip's factored
//   d[b, j] = sum_e a_b[e] c_j[e]  (MFMA; the codes 0..255 are exact in bf16 and fp32)      sa[b] = sum_e a_b[e]  (fp32)
//   score   = d * scale_j + sa * bias_j                                  cosine: * ainv[b] * tinv[j], tinv from the sum of
// squares of c * scale + bias -- in the list kernel, in the streaming kernel and in topk_scores_q8 the same bits (code
// conversion, MFMA and k order, summation order of sa and the row norm, product, product, sum, each rounded: none of the
// three is compiled with contraction), through one function each for the staging of a Q8 vector, sa, the row norm and the
// epilogue.  So the rank is the position at which topk_scores_q8 serves the id.  Streaming kernel: split, arrangements,
// anchor gather, swizzle, k-loop, count and atomics are the float kernel's; LDS-DMA cannot convert, so a tile goes through
// registers as in topk.hip: a thread owns up to tr_q8_units 16-byte vectors of the tile's Q8 rows (tails included,
// consecutive lanes consecutive vectors), loads those of tile t + 1 before the k-loop of tile t and behind the issued
// MFMAs converts the codes to the anchor dtype -- each code once per workgroup -- into swizzled operand chunks of the other
// buffer; the vectors that hold scale and bias drop them into two per-tile LDS arrays next to tinv, sa sits next to ainv
// (2 x 2 x TR + NA more floats); chunks behind the last converted one are zeroed once; rows past the end of a range stage
// as code 0, scale 0, bias 0 and are set to -inf like any.  List kernel: the 16 listed rows of a group are gathered from
// the Q8 table vector by vector into the same operand chunks, scale, bias and tinv per row.
// Registers (compiler's report, no spill anywhere): the unit count is sized by arrangement, because with 5 units 64 x 64
// took 272 (bf16) / 291 (fp32) registers at P = 1, one wave per SIMD; with the 2 units its rows of at most 192 bytes need
// it takes 235 / 247 and keeps two, inside 80 KiB as before (bf16 E = 64: 51.5 KiB).  At P <= 4 the Q8 64 x 64 takes 287 /
// 303 registers, so Q8 with 2 .. 4 labels starts at 32 x 64 (217 / 231, two waves); 32 x 64 at P = 1 takes 190 / 204, 16 x 32
// at most 111.  Like the float ones, the Q8 arrangements have not been timed against each other.
//
// Multi-interest (template parameter MI of both kernels; trs_target_ranks_multi).  A user is G anchors (1 .. 16) and
// score[u, j] = max_g sim(a[u, g], t[j]), each sim the bits above; Gp = the power of two >= G is a kernel argument (gsh =
// log2 Gp), and MI = false compiles to the kernels above unchanged (same registers and occupancy in the compiler's report).
// Streaming kernel: a workgroup's NA LDS anchor rows hold NA / Gp users, row r slot r % Gp of user r / Gp, gathered from
// the user's interest min(slot, G - 1) -- padding by repetition, on chip.  Behind the tile's epilogue (and the -inf of rows
// past the range) the scores of a user's Gp adjacent lanes are replaced by their max, log2 Gp DPP steps per score on the
// vector ALU (group_max.hpp), each step over the whole tile behind one uniform branch; every score is compared, so there
// is no ballot shortcut as in topk.hip.  The leader lane (n % Gp == 0) carries the user's thresholds and counts; the
// other lanes carry (+inf, -1) like rows past B and add nothing.  Boundary tile, tie pass, the 4-lane sum and the atomic
// are the ones above.  The variant that ORs compare masks on the scalar ALU was not built.  List kernel: one wave per user,
// its Gp interest rows in LDS (swizzled) where the anchor's row stood; column n of the B operand is interest n % Gp (the
// waste is (16 - Gp) / 16), then the group max: every lane holds the user's score of its listed row, the same bits as the
// streaming kernel's (the max of identical bits is exact).  1 .. 4 waves a workgroup, as many as fit 160 KiB.
// Registers (compiler's report, no spill; vector + accumulator, fp32 / bf16): 64 x 64 at P = 1 144 + 68 / 141 + 64, two
// waves per SIMD; 64 x 64 at P <= 4 187 + 72 = 259 (fp32), ONE wave, so fp32 with 2 .. 4 labels starts at 32 x 64 (114 + 36,
// three waves); bf16 187 + 64 keeps two and stays.  32 x 64: P = 1 92 + 36 / 32, four; P = 16 111 + 36 / 32, three.  16 x 32: at
// most 61 + 8, seven.  List kernel 62 / 41 + 4, seven / eight.
#include <algorithm>

#include <type_traits>

#include "group_max.hpp"
#include "lds_dma.hpp"
#include "q8_common.hpp"

namespace trs {

typedef __attribute__((ext_vector_type(8))) __bf16 tr_bf16x8;
typedef __attribute__((ext_vector_type(4))) float tr_f32x4;

constexpr int TR_DOT = 0, TR_COS = 1;
constexpr float TR_COS_EPS = 1e-8f;      // rank.hip's COS_EPS
constexpr int TR_MAX_P = 16, TR_MAX_X = 1024, TR_MAX_E = 256, TR_MAX_SPLITS = 64;
constexpr size_t TR_MAX_LDS = 160 * 1024, TR_HALF_LDS = 80 * 1024;
// 16-byte vectors of a Q8 tile a thread owns, by arrangement (the rows the arrangement is taken for bound the vectors of a
// row): 64 x 64 rows up to 192 bytes, 7 vectors, 64 x 7 / 256 threads; 32 x 64 up to 17 vectors; 16 x 32 up to 17
constexpr int tr_q8_units(int AR, int TR) { return AR == 64 ? 2 : TR == 64 ? 5 : 3; }

struct RankArgs {
  const char* a_table;
  const void* a_idx;       // NULL: anchor b is row b
  const char* t_table;
  const void* labels;      // (B, P)
  const void* excl;        // (B, X) or NULL
  int64_t* ranks;          // (B, P)
  float* lscore;           // (B, P)
  int32_t* err_flag;
  int64_t Va, a_off, B, t_lo;
  int Vt, rows_per, S, P, X;
  int row_bytes;           // E * sizeof(T)
  int nc, nce;             // 16-byte chunks of an LDS row (whole 64-byte k-steps) and of a table row
  int sw_shift, sw_mask;   // g(r) = (r >> sw_shift) & sw_mask
  int sim;
  bool idx64, lab64, excl64, dma;
  int E, q_stride, q_nv;   // Q8 targets: columns, bytes of a row (S) and its 16-byte vectors
};
// multi-interest (template parameter MI): B users of G anchors each, in groups of Gp = 1 << gsh LDS rows.  Arguments of
// their own, so that the kernels of one anchor per sample keep theirs
struct RankArgsMI : RankArgs {
  int G, gsh;
};
template <bool MI>
using RankArgsOf = std::conditional_t<MI, RankArgsMI, RankArgs>;

__device__ __forceinline__ void tr_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ int64_t tr_id(const void* ids, bool wide, int64_t i) {
  return wide ? static_cast<const int64_t*>(ids)[i] : (int64_t) static_cast<const int32_t*>(ids)[i];
}

// (s, id) sorts in front of (th, lid): score descending, id ascending among equals; false where either score is a NaN
__device__ __forceinline__ bool tr_beats(float s, int id, float th, int lid) { return s > th || (s == th && id < lid); }

// c += s > thr: the compare and the add with carry, kept together (left to the scheduler, the compares of a tile are
// hoisted in front of their adds and their results no longer fit the scalar registers)
__device__ __forceinline__ void tr_count_gt(int& c, float s, float thr) {
  asm("v_cmp_gt_f32 vcc, %1, %2\n\tv_addc_co_u32 %0, vcc, 0, %0, vcc" : "+v"(c) : "v"(s), "v"(thr) : "vcc");
}

// the next float under th (s > below(th) is s >= th); -inf and NaN have none and stay
__device__ __forceinline__ float tr_below(float th) {
  const uint32_t u = __float_as_uint(th + 0.f);      // -0 -> +0
  if (th != th || u == 0xff800000u) return th;
  if (u == 0) return __uint_as_float(0x80000001u);
  return __uint_as_float((u & 0x80000000u) ? u + 1 : u - 1);
}

// the MFMA of topk.hip: targets A, anchors B; fp32: the lane's 16 bytes feed element i of MFMA i
template <typename T>
__device__ __forceinline__ tr_f32x4 tr_mma(const uint4& tgt, const uint4& anc, tr_f32x4 acc) {
  if constexpr (std::is_same<T, float>::value) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.x), __uint_as_float(anc.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.y), __uint_as_float(anc.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.z), __uint_as_float(anc.z), acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(tgt.w), __uint_as_float(anc.w), acc, 0, 0, 0);
  } else {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(tr_bf16x8, tgt), __builtin_bit_cast(tr_bf16x8, anc),
                                                   acc, 0, 0, 0);
  }
}

// 1 / max(|row r|, eps) of LDS row r: its real chunks in order, fp32 -- one function for both kernels
template <typename T>
__device__ __forceinline__ float tr_row_inv(const char* rows, int r, const RankArgs& p) {
  const int g = (r >> p.sw_shift) & p.sw_mask;
  float s = 0.f;
  for (int c = 0; c < p.nce; ++c) {
    float f[Vec16<T>::VE];
    Vec16<T>::unpack(*reinterpret_cast<const uint4*>(rows + ((size_t)r * p.nc + (c ^ g)) * 16), f);
#pragma unroll
    for (int e = 0; e < Vec16<T>::VE; ++e) s += f[e] * f[e];
  }
  return 1.f / fmaxf(sqrtf(s), TR_COS_EPS);
}

// ---- Q8 targets.  Every function below is called by both kernels and repeats topk.hip's arithmetic operation for
// operation (tk_row_sum, tk_q8_row_sq, q8_store, its epilogue), so a pair scores to the same bits in all three places.
// sa of the factored score: the sum of LDS row r (its real chunks, in order), fp32
template <typename T>
__device__ __forceinline__ float tr_row_sum(const char* rows, int r, const RankArgs& p) {
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

// 1 / max(|x|, eps) of the dequantized row whose codes are LDS row r: the squares of c * scale + bias themselves, in order
template <typename T>
__device__ __forceinline__ float tr_q8_row_inv(const char* rows, int r, float scale, float bias, const RankArgs& p) {
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
  return 1.f / fmaxf(sqrtf(s), TR_COS_EPS);
}

// 16-byte vector v of a Q8 row -> LDS row r: its codes, converted exactly to T, as the swizzled operand chunks they fill;
// the vectors that hold the row's scale and bias drop them into tsc[r], tbi[r]
template <typename T>
__device__ __forceinline__ void tr_q8_stage(char* rows, float* tsc, float* tbi, int r, int v, const uint4& q4, const RankArgs& p) {
  constexpr int CPV = (int)sizeof(T);      // operand chunks the 16 codes of one vector become
  const int e0 = 16 * v;
  if (v == p.E >> 4) tsc[r] = __uint_as_float(tk_word(q4, (p.E >> 2) & 3));
  if (v == (p.E + 4) >> 4) tbi[r] = __uint_as_float(tk_word(q4, ((p.E + 4) >> 2) & 3));
  // E is a multiple of 4: a word is all codes or none
  const uint32_t w[4] = {e0 < p.E ? q4.x : 0u, e0 + 4 < p.E ? q4.y : 0u, e0 + 8 < p.E ? q4.z : 0u, e0 + 12 < p.E ? q4.w : 0u};
  char* drow = rows + (size_t)r * p.nc * 16;
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

// operand chunks behind the last one a Q8 vector is converted into are never staged: zero them once
template <typename T>
__device__ __forceinline__ void tr_q8_zero_tail(char* rows, int nrows, int first, int step, const RankArgs& p) {
  for (int u = first; u < nrows * p.nc; u += step) {
    const int r = u / p.nc, c = u - r * p.nc;
    if (c >= (int)sizeof(T) * p.q_nv)
      *reinterpret_cast<uint4*>(rows + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = make_uint4(0, 0, 0, 0);
  }
}

// The epilogue, one function for both kernels: the MFMA sums of a lane's 4 targets against one anchor -> their scores.
// Q8: d * scale + sa * bias, two products and a sum, each rounded (the library is built without contraction, as topk.hip
// is: no fused multiply-add in either); cosine: then * ainv, then * tinv.
template <bool Q8>
__device__ __forceinline__ void tr_scores(tr_f32x4& acc, const float4& sc, const float4& bi, float sa, bool cosine, float ai,
                                          const float4& ti) {
  if constexpr (Q8) {
    acc[0] = acc[0] * sc.x + sa * bi.x;
    acc[1] = acc[1] * sc.y + sa * bi.y;
    acc[2] = acc[2] * sc.z + sa * bi.z;
    acc[3] = acc[3] * sc.w + sa * bi.w;
  }
  if (cosine) {
    acc[0] = acc[0] * ai * ti.x;
    acc[1] = acc[1] * ai * ti.y;
    acc[2] = acc[2] * ai * ti.z;
    acc[3] = acc[3] * ai * ti.w;
  }
}

// chunk c of anchor b's row (zero: past the row, past B, or an id outside the table, which raises the flag)
__device__ __forceinline__ uint4 tr_anchor_chunk(const RankArgs& p, int64_t b, int c) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (b < p.B) {
    int64_t ra = (p.a_idx != nullptr ? tr_id(p.a_idx, p.idx64, b) : b) + p.a_off;
    if (ra < 0 || ra >= p.Va) {
      if (c == 0 && p.err_flag != nullptr) *p.err_flag = 1;
    } else if (c < p.nce) {
      v = *reinterpret_cast<const uint4*>(p.a_table + ra * p.row_bytes + 16 * c);
    }
  }
  return v;
}

// multi-interest: chunk c of slot `slot` of user u's group of LDS rows, its interest min(slot, G - 1) (anchor u G + that);
// zero past the U users
__device__ __forceinline__ uint4 tr_interest_chunk(const RankArgsMI& p, int64_t u, int slot, int c) {
  uint4 v = make_uint4(0, 0, 0, 0);
  if (u < p.B) {
    const int64_t ia = u * p.G + min(slot, p.G - 1);
    int64_t ra = (p.a_idx != nullptr ? tr_id(p.a_idx, p.idx64, ia) : ia) + p.a_off;
    if (ra < 0 || ra >= p.Va) {
      if (c == 0 && p.err_flag != nullptr) *p.err_flag = 1;
    } else if (c < p.nce) {
      v = *reinterpret_cast<const uint4*>(p.a_table + ra * p.row_bytes + 16 * c);
    }
  }
  return v;
}

// ------------------------------------------------------------------------------------------------ 1. the listed rows
// LDS of a wave: the anchor's row, 16 listed rows, ids[LP], scores[LP], tinv[16], dec[16], Q8: scale[16], bias[16]; LP = P +
// X rounded up to 16
// multi-interest (MI): one wave per user, 1 .. 4 waves a workgroup; the anchor's row becomes the user's Gp interest rows,
// swizzled like any group of LDS rows, and column n of the B operand is interest n % Gp
static size_t tr_list_wave_bytes(int RB, int L, bool q8, int gsh = 0) {
  return (size_t)(16 + (1 << gsh)) * RB + (size_t)((L + 15) & ~15) * 8 + (q8 ? 256 : 128);
}

template <typename T, bool Q8, bool MI>
__global__ __launch_bounds__(256) void target_rank_list_kernel(RankArgsOf<MI> p) {
  static_assert(!(Q8 && MI), "multi-interest ranks are taken over float tables only");
  extern __shared__ __attribute__((aligned(16))) char tr_smem[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  const int RB = p.nc * 16, P = p.P, L = P + p.X, LP = (L + 15) & ~15;
  int gsh = 0;
  if constexpr (MI) gsh = p.gsh;
  const int GP = 1 << gsh, nw = MI ? (int)(blockDim.x >> 6) : 4;
  char* Arow = tr_smem + (size_t)wave * ((size_t)(16 + GP) * RB + (size_t)LP * 8 + (Q8 ? 256 : 128));
  char* Rows = Arow + (size_t)GP * RB;
  int* ids = reinterpret_cast<int*>(Rows + (size_t)16 * RB);
  float* sc = reinterpret_cast<float*>(ids + LP);
  float* tinv = sc + LP;
  int* dec = reinterpret_cast<int*>(tinv + 16);
  float* tsc = reinterpret_cast<float*>(dec + 16);
  float* tbi = tsc + 16;
  const int64_t b = (int64_t)blockIdx.x * nw + wave;
  if (b >= p.B) return;      // the whole wave; the kernel has no workgroup barrier
  const bool cosine = p.sim == TR_COS;

  for (int i = lane; i < LP; i += 64) {
    int64_t id = -1;
    if (i < P) {
      id = tr_id(p.labels, p.lab64, b * P + i);
      if (id >= p.Vt && p.err_flag != nullptr) *p.err_flag = 1;
    } else if (i < L) {
      id = tr_id(p.excl, p.excl64, b * p.X + (i - P));
    }
    ids[i] = id < 0 || id >= p.Vt ? -1 : (int)id;
  }
  if (lane < 16) dec[lane] = 0;
  if constexpr (MI) {
    for (int u = lane; u < GP * p.nc; u += 64) {
      const int r = u / p.nc, c = u - r * p.nc;
      *reinterpret_cast<uint4*>(Arow + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = tr_interest_chunk(p, b, r, c);
    }
  } else {
    for (int c = lane; c < p.nc; c += 64) *reinterpret_cast<uint4*>(Arow + 16 * c) = tr_anchor_chunk(p, b, c);
  }
  if constexpr (Q8) tr_q8_zero_tail<T>(Rows, 16, lane, 64, p);
  tr_wave_sync();
  const int arow = n & (GP - 1);      // the anchor row of this lane's column: 0, MI: its interest
  const float ai = cosine ? tr_row_inv<T>(Arow, arow, p) : 1.f;      // row 0 is not swizzled
  float sa = 0.f;
  if constexpr (Q8) sa = tr_row_sum<T>(Arow, 0, p);
  const int gsw = (n >> p.sw_shift) & p.sw_mask, nks = p.nc >> 2;
  const int asw = (arow >> p.sw_shift) & p.sw_mask;

  for (int g0 = 0; g0 < LP; g0 += 16) {
    if constexpr (Q8) {      // the 16 listed Q8 rows, vector by vector (a row that is not listed: code 0, scale 0, bias 0)
      for (int u = lane; u < 16 * p.q_nv; u += 64) {
        const int r = u / p.q_nv, v = u - r * p.q_nv, id = ids[g0 + r];
        uint4 q4 = make_uint4(0, 0, 0, 0);
        if (id >= 0) q4 = *reinterpret_cast<const uint4*>(p.t_table + (p.t_lo + id) * p.q_stride + 16 * v);
        tr_q8_stage<T>(Rows, tsc, tbi, r, v, q4, p);
      }
    } else {
      for (int u = lane; u < 16 * p.nc; u += 64) {
        const int r = u / p.nc, c = u - r * p.nc, id = ids[g0 + r];
        uint4 v = make_uint4(0, 0, 0, 0);
        if (id >= 0 && c < p.nce) v = *reinterpret_cast<const uint4*>(p.t_table + (p.t_lo + id) * p.row_bytes + 16 * c);
        *reinterpret_cast<uint4*>(Rows + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = v;
      }
    }
    tr_wave_sync();
    if (cosine && lane < 16) {
      if constexpr (Q8) tinv[lane] = tr_q8_row_inv<T>(Rows, lane, tsc[lane], tbi[lane], p);
      else tinv[lane] = tr_row_inv<T>(Rows, lane, p);
    }
    tr_f32x4 acc = tr_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      const uint4 af = *reinterpret_cast<const uint4*>(Rows + n * RB + (((4 * ks + q) ^ gsw) << 4));
      const uint4 bf = *reinterpret_cast<const uint4*>(Arow + arow * RB + (((4 * ks + q) ^ asw) << 4));
      acc = tr_mma<T>(af, bf, acc);
    }
    tr_wave_sync();
    if (cosine || Q8) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 sc = Q8 ? *reinterpret_cast<const float4*>(tsc + 4 * q) : zero;
      const float4 bi = Q8 ? *reinterpret_cast<const float4*>(tbi + 4 * q) : zero;
      tr_scores<Q8>(acc, sc, bi, sa, cosine, ai, cosine ? *reinterpret_cast<const float4*>(tinv + 4 * q) : zero);
    }
    if constexpr (MI) {      // the user's score of the listed row: the max over its interests, in every lane of the group
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = group_max(acc[j], gsh);
    }
    if (n == 0) *reinterpret_cast<float4*>(sc + g0 + 4 * q) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    tr_wave_sync();      // the scores are written, the rows may be replaced
  }

  if (lane < P) p.lscore[b * P + lane] = ids[lane] >= 0 ? sc[lane] : -INFINITY;
  for (int x = P + lane; x < L; x += 64) {
    const int id = ids[x];
    bool live = id >= 0;
    for (int y = P; y < x && live; ++y) live = ids[y] != id;
    if (!live) continue;
    const float sx = sc[x];
    for (int pp = 0; pp < P; ++pp) {
      const int lid = ids[pp];
      if (lid >= 0 && lid != id && tr_beats(sx, id, sc[pp], lid)) atomicAdd(&dec[pp], 1);
    }
  }
  tr_wave_sync();
  if (lane < P) p.ranks[b * P + lane] = ids[lane] >= 0 ? -(int64_t)dec[lane] : -1;
}

// ------------------------------------------------------------------------------------------------ 2. the count
template <typename T, int AR, int TR, int PT, bool Q8, bool MI>
__global__ __launch_bounds__(256) void target_rank_count_kernel(RankArgsOf<MI> p) {
  static_assert(!(Q8 && MI), "multi-interest ranks are taken over float tables only");
  extern __shared__ __attribute__((aligned(16))) char tr_smem[];
  constexpr int AT = AR / 16, NT = TR / 16, NA = 4 * AR;
  constexpr bool TLDS = PT > 4;      // thresholds in LDS
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane >> 4, n = lane & 15;
  // MI: b counts users; LDS row r is slot r & gm of user r >> gsh.  Behind the epilogue every lane of a user holds the
  // user's score (the max over its Gp rows); the leader lane (slot 0) counts, the others behave like rows past B
  int gsh = 0;
  if constexpr (MI) gsh = p.gsh;
  const int gm = (1 << gsh) - 1;
  const int RB = p.nc * 16, P = p.P;
  char* As = tr_smem;
  char* Ts = As + (size_t)NA * RB;
  float* ainv = reinterpret_cast<float*>(Ts + (size_t)2 * TR * RB);
  float* tinv = ainv + NA;      // [2][TR]
  float* tsc = tinv + 2 * TR;   // Q8: [2][TR] scales, [2][TR] biases, [NA] anchor sums
  float* tbi = tsc + 2 * TR;
  float* sa = tbi + 2 * TR;
  float* thS = Q8 ? sa + NA : tsc;      // TLDS: [PT][NA] thresholds, the floats under them, label ids
  float* tloS = thS + PT * NA;
  int* lidS = reinterpret_cast<int*>(tloS + PT * NA);
  const bool cosine = p.sim == TR_COS;

  // ---- the anchors, once
  const int64_t b0 = (int64_t)blockIdx.x * (NA >> gsh);
  for (int u = threadIdx.x; u < NA * p.nc; u += blockDim.x) {
    const int r = u / p.nc, c = u - r * p.nc;
    uint4 v;
    if constexpr (MI) v = tr_interest_chunk(p, b0 + (r >> gsh), r & gm, c);
    else v = tr_anchor_chunk(p, b0 + r, c);
    *reinterpret_cast<uint4*>(As + ((size_t)r * p.nc + (c ^ ((r >> p.sw_shift) & p.sw_mask))) * 16) = v;
  }
  // the sample whose labels LDS row r counts against: MI the user on its leader row, none (B) on the others
  auto row_sample = [&](int r) -> int64_t { return (r & gm) != 0 ? p.B : b0 + (r >> gsh); };

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
      for (int pc = wave; pc < TR * p.nc / 64; pc += 4) {
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
      if constexpr (Q8) tinv[buf * TR + r] = tr_q8_row_inv<T>(rows, r, tsc[buf * TR + r], tbi[buf * TR + r], p);
      else tinv[buf * TR + r] = tr_row_inv<T>(rows, r, p);
    }
  };
  // Q8: unit i of this thread is vector v of tile row r, packed r | v << 8 (-1: none); consecutive threads take
  // consecutive vectors of a row, so a wave's load is one contiguous stretch of the table
  constexpr int QU = Q8 ? tr_q8_units(AR, TR) : 0;
  uint4 pre[Q8 ? QU : 1];
  int prv[Q8 ? QU : 1];
  if constexpr (Q8) {
#pragma unroll
    for (int i = 0; i < QU; ++i) {
      const int u = threadIdx.x + i * 256;
      prv[i] = u < TR * p.q_nv ? ((u / p.q_nv) | ((u % p.q_nv) << 8)) : -1;
    }
    tr_q8_zero_tail<T>(Ts, 2 * TR, threadIdx.x, 256, p);      // both buffers
  }
  auto q8_fetch = [&](int t) {
    const int64_t t0 = lo + (int64_t)t * TR;
#pragma unroll
    for (int i = 0; i < QU; ++i) {
      pre[i] = make_uint4(0, 0, 0, 0);      // a row past the end of the range: code 0, scale 0, bias 0
      const int r = prv[i] & 0xff, v = prv[i] >> 8;
      if (prv[i] >= 0 && t0 + r < hi) pre[i] = *reinterpret_cast<const uint4*>(p.t_table + (t0 + r) * p.q_stride + 16 * v);
    }
  };
  auto q8_store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < QU; ++i)
      if (prv[i] >= 0)
        tr_q8_stage<T>(Ts + (size_t)buf * TR * RB, tsc + buf * TR, tbi + buf * TR, prv[i] & 0xff, prv[i] >> 8, pre[i], p);
  };
  if (ntile > 0) {
    if constexpr (Q8) {
      q8_fetch(0);
      q8_store(0);
    } else {
      load_tile(0, 0);
    }
  }

  // ---- the thresholds: label p of anchor r -> (score, the float under it, id); (+inf, +inf, -1) where nothing is ranked
  auto threshold = [&](int64_t b, int pp, float& th, float& tlo, int& lid) {
    th = tlo = INFINITY;
    lid = -1;
    if (b < p.B && pp < P) {
      const int64_t id = tr_id(p.labels, p.lab64, b * P + pp);
      if (id >= 0 && id < p.Vt) {
        th = p.lscore[b * P + pp] + 0.f;
        tlo = tr_below(th);
        lid = (int)id;
      }
    }
  };
  if constexpr (TLDS) {
    for (int u = threadIdx.x; u < PT * NA; u += blockDim.x) threshold(MI ? row_sample(u % NA) : b0 + u % NA, u / NA, thS[u], tloS[u], lidS[u]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (cosine || Q8) {
    for (int r = threadIdx.x; r < NA; r += blockDim.x) {
      if (cosine) ainv[r] = tr_row_inv<T>(As, r, p);
      if constexpr (Q8) sa[r] = tr_row_sum<T>(As, r, p);
    }
    if (cosine && ntile > 0) tile_norms(0);
    __syncthreads();
  }

  // ---- per lane: anchor n of each of the wave's AT groups of 16
  const int row0 = wave * AR + n;                         // + 16 at
  const int gsw = (n >> p.sw_shift) & p.sw_mask;          // g(r) depends on r & 15 only
  constexpr int PR = TLDS ? 1 : PT;
  float thr_[AT][PR], tlor_[AT][PR], ai[AT], sav[AT];
  int lidr_[AT][PR], cnt[AT][PT];
#pragma unroll
  for (int at = 0; at < AT; ++at) {
    ai[at] = cosine ? ainv[row0 + 16 * at] : 1.f;
    sav[at] = Q8 ? sa[row0 + 16 * at] : 0.f;
#pragma unroll
    for (int pp = 0; pp < PT; ++pp) cnt[at][pp] = 0;
    if constexpr (!TLDS) {
#pragma unroll
      for (int pp = 0; pp < PT; ++pp) threshold(MI ? row_sample(row0 + 16 * at) : b0 + row0 + 16 * at, pp, thr_[at][pp], tlor_[at][pp], lidr_[at][pp]);
    }
  }
  auto TH = [&](int at, int pp) { if constexpr (TLDS) return thS[pp * NA + row0 + 16 * at]; else return thr_[at][pp]; };
  auto TLO = [&](int at, int pp) { if constexpr (TLDS) return tloS[pp * NA + row0 + 16 * at]; else return tlor_[at][pp]; };
  auto LID = [&](int at, int pp) { if constexpr (TLDS) return lidS[pp * NA + row0 + 16 * at]; else return lidr_[at][pp]; };
  const int nks = p.nc >> 2;

  for (int t = 0; t < ntile; ++t) {
    const int buf = t & 1;
    if (t + 1 < ntile) {
      if constexpr (Q8) q8_fetch(t + 1);
      else load_tile(t + 1, buf ^ 1);
    }
    const char* Tb = Ts + (size_t)buf * TR * RB;
    tr_f32x4 acc[AT][NT];
#pragma unroll
    for (int at = 0; at < AT; ++at)
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[at][nt] = tr_f32x4{0.f, 0.f, 0.f, 0.f};
    for (int ks = 0; ks < nks; ++ks) {
      const int coff = ((4 * ks + q) ^ gsw) << 4;
      uint4 bf[AT];
#pragma unroll
      for (int at = 0; at < AT; ++at) bf[at] = *reinterpret_cast<const uint4*>(As + (row0 + 16 * at) * RB + coff);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const uint4 af = *reinterpret_cast<const uint4*>(Tb + (16 * nt + n) * RB + coff);
#pragma unroll
        for (int at = 0; at < AT; ++at) acc[at][nt] = tr_mma<T>(af, bf[at], acc[at][nt]);
      }
    }
    // Q8: the next tile, converted behind the issued MFMAs into the buffer the last tile left (the barrier at its end)
    if (Q8 && t + 1 < ntile) q8_store(buf ^ 1);
    if (cosine || Q8) {
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const int j0 = buf * TR + 16 * nt + 4 * q;
        const float4 sc = Q8 ? *reinterpret_cast<const float4*>(tsc + j0) : zero;
        const float4 bi = Q8 ? *reinterpret_cast<const float4*>(tbi + j0) : zero;
        const float4 ti = cosine ? *reinterpret_cast<const float4*>(tinv + j0) : zero;
#pragma unroll
        for (int at = 0; at < AT; ++at) tr_scores<Q8>(acc[at][nt], sc, bi, sav[at], cosine, ai[at], ti);
      }
    }

    // ---- the count
    const int64_t t0 = lo + (int64_t)t * TR;
    const int valid = (int)std::min<int64_t>(TR, hi - t0);      // targets of this tile that exist
    const int idbase = (int)(t0 - p.t_lo);
    if (valid < TR) {
#pragma unroll
      for (int at = 0; at < AT; ++at)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (16 * nt + 4 * q + j >= valid) acc[at][nt][j] = -INFINITY;
    }
    if constexpr (MI) {      // the user's scores: log2(Gp) butterfly steps over the tile, each behind one uniform branch
      auto step = [&](auto ctrl) {
#pragma unroll
        for (int at = 0; at < AT; ++at)
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[at][nt][j] = gm_step<decltype(ctrl)::value>(acc[at][nt][j]);
      };
      if (gsh >= 1) step(std::integral_constant<int, GM_QUAD_1032>{});
      if (gsh >= 2) step(std::integral_constant<int, GM_QUAD_2301>{});
      if (gsh >= 3) step(std::integral_constant<int, GM_ROW_HALF_MIRROR>{});
      if (gsh >= 4) step(std::integral_constant<int, GM_ROW_MIRROR>{});
    }
    bool slow = false;
#pragma unroll
    for (int pp = 0; pp < PT; ++pp) {
      if (pp < P) {
#pragma unroll
      for (int at = 0; at < AT; ++at) {
        const float th = TH(at, pp);
        const int lid = LID(at, pp);
        const int rel = lid - idbase;                // the label's place in the tile (no overflow: both are ids)
        const bool before = rel >= TR;               // every id of the tile is smaller: equal scores count
        const float thr = before ? TLO(at, pp) : th;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
          for (int j = 0; j < 4; ++j) tr_count_gt(cnt[at][pp], acc[at][nt][j], thr);
        slow |= lid >= 0 && ((rel >= 0 && !before) || th == -INFINITY);
      }
      }
    }
    if (__ballot(slow) != 0) {      // the tile that holds a label, or a threshold of -inf: equal scores with a smaller id
#pragma unroll
      for (int pp = 0; pp < PT; ++pp) {
        if (pp < P) {
#pragma unroll
        for (int at = 0; at < AT; ++at) {
          const float th = TH(at, pp);
          const int lid = LID(at, pp);
          const int rel = lid - idbase;
          if (lid < 0 || (rel >= TR && th != -INFINITY)) continue;
          int c = 0;
#pragma unroll
          for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int local = 16 * nt + 4 * q + j;
              c += acc[at][nt][j] == th && local < rel && local < valid ? 1 : 0;
            }
          cnt[at][pp] += c;
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

  // ---- the 4 q lanes of an anchor, then this range's count into the rank
#pragma unroll
  for (int pp = 0; pp < PT; ++pp) {
    if (pp < P) {
#pragma unroll
    for (int at = 0; at < AT; ++at) {
      int c = cnt[at][pp];
      c += __shfl_xor(c, 16);
      c += __shfl_xor(c, 32);
      // MI: the user, and LID is -1 on every lane but its leader
      const int64_t b = MI ? b0 + ((row0 + 16 * at) >> gsh) : b0 + row0 + 16 * at;
      if (q == 0 && b < p.B && LID(at, pp) >= 0 && c != 0)
        atomicAdd(reinterpret_cast<unsigned long long*>(p.ranks + b * P + pp), (unsigned long long)c);
    }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// Target ranges, a pure function of (B, Vt), the rule of topk.hip: a small B is spread over the 256 CUs (two workgroups
// each, counted in nominal tiles of 128 anchors), every range keeps at least two tiles of 128 rows, and S = 1 once the
// anchor tiles alone fill the chip.
static int tr_splits(int64_t B, int64_t Vt) {
  const int64_t tiles_a = (B + 127) / 128;
  if (tiles_a >= 256) return 1;
  const int64_t want = (512 + tiles_a - 1) / tiles_a;
  return (int)std::max<int64_t>(1, std::min<int64_t>({want, (int64_t)TR_MAX_SPLITS, Vt / 256}));
}

struct RankShape {
  int AR, TR;
  size_t lds;      // taken where it fits this much
};
static size_t tr_lds_bytes(const RankShape& s, int RB, int PT, bool q8) {
  const size_t NA = (size_t)4 * s.AR;
  // Q8: the tiles' scales and biases, the anchors' sums
  return NA * RB + (size_t)2 * s.TR * RB + NA * 4 + (size_t)2 * s.TR * 4 + (PT > 4 ? NA * PT * 12 : 0) +
         (q8 ? (size_t)2 * s.TR * 8 + NA * 4 : 0);
}

template <typename T, int PT, bool Q8, bool MI>
static int tr_count_launch(const char* op, const RankArgsMI& p, int RB, hipStream_t s) {
  static const RankShape shapes[] = {{64, 64, TR_HALF_LDS}, {32, 64, TR_HALF_LDS}, {32, 64, TR_MAX_LDS}, {16, 32, TR_MAX_LDS}};
  // the labels up to which 64 x 64 is taken (MI, fp32, 2 .. 4 labels: 259 registers, one wave per SIMD)
  constexpr int PT64 = Q8 || (MI && std::is_same<T, float>::value) ? 1 : 4;
  const RankShape* sh = nullptr;
  for (const RankShape& c : shapes)
    if ((PT <= PT64 || c.AR <= 32) && tr_lds_bytes(c, RB, PT, Q8) <= c.lds &&
        (!Q8 || (c.TR * p.q_nv + 255) / 256 <= tr_q8_units(c.AR, c.TR))) {
      sh = &c;
      break;
    }
  TRS_REQUIRE(sh != nullptr, TRS_ESHAPE, "%s: no arrangement fits LDS%s (row %d bytes, P %d)", op,
              Q8 ? " and the Q8 vectors of a tile its threads" : "", RB, p.P);
  const size_t lds = tr_lds_bytes(*sh, RB, PT, Q8);
  const int NA = (4 * sh->AR) >> p.gsh;      // users of a workgroup
  const dim3 grid((unsigned)((p.B + NA - 1) / NA), (unsigned)p.S);
  auto go = [&](auto kern) -> int {
    if (lds > 64 * 1024 &&
        hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)TR_MAX_LDS) != hipSuccess) {
      (void)hipGetLastError();
      return fail(TRS_ELAUNCH, "%s: hipFuncSetAttribute(%zu bytes of LDS) failed", op, lds);
    }
    hipLaunchKernelGGL(kern, grid, dim3(256), lds, s, static_cast<const RankArgsOf<MI>&>(p));
    return TRS_OK;
  };
  if constexpr (PT <= PT64) {
    if (sh->AR == 64) return go(target_rank_count_kernel<T, 64, 64, PT, Q8, MI>);
  }
  if (sh->AR == 32) return go(target_rank_count_kernel<T, 32, 64, PT, Q8, MI>);
  return go(target_rank_count_kernel<T, 16, 32, PT, Q8, MI>);
}

template <typename T, bool Q8, bool MI>
static int tr_launch(const char* op, const RankArgsMI& p, hipStream_t s) {
  const int RB = p.nc * 16;
  // MI: the user's Gp interest rows stand where the one anchor row stood; as many waves (users) a workgroup as fit
  int nw = 4;
  while (MI && nw > 1 && nw * tr_list_wave_bytes(RB, p.P + p.X, Q8, p.gsh) > TR_MAX_LDS) nw >>= 1;
  const size_t lds = nw * tr_list_wave_bytes(RB, p.P + p.X, Q8, p.gsh);
  if (lds > 64 * 1024 && hipFuncSetAttribute((const void*)target_rank_list_kernel<T, Q8, MI>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)TR_MAX_LDS) != hipSuccess) {
    (void)hipGetLastError();
    return fail(TRS_ELAUNCH, "%s: hipFuncSetAttribute(%zu bytes of LDS) failed", op, lds);
  }
  hipLaunchKernelGGL((target_rank_list_kernel<T, Q8, MI>), dim3((unsigned)((p.B + nw - 1) / nw)), dim3(64 * nw), lds, s,
                     static_cast<const RankArgsOf<MI>&>(p));
  const int rc = p.P == 1 ? tr_count_launch<T, 1, Q8, MI>(op, p, RB, s)
                 : p.P <= 4 ? tr_count_launch<T, 4, Q8, MI>(op, p, RB, s)
                            : tr_count_launch<T, TR_MAX_P, Q8, MI>(op, p, RB, s);
  return rc != TRS_OK ? rc : check_launch(op);
}

// all entries: `dtype` is the anchors' (and, for float targets, the table's); q8: target_table holds Q8 rows of E columns;
// G = 0: one anchor per sample (U unused); G >= 1: the multi-interest entry, B = U * G anchors, user-major
static int tr_entry(const char* op, bool q8, int64_t U, int32_t G, const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                    int64_t anchor_offset, int64_t B, const void* target_table, int64_t target_lo, int64_t target_hi,
                    int32_t E, int32_t dtype, int32_t sim, const void* labels, int32_t label_dtype, int32_t P,
                    const void* exclude, int32_t excl_dtype, int32_t X, int64_t* ranks, float* label_scores,
                    int32_t* err_flag, trs_stream_t stream) {
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "%s: dtype %d", op, dtype);
  TRS_REQUIRE(sim == TR_DOT || sim == TR_COS, TRS_EINVAL, "%s: sim %d (0 = inner product, 1 = cosine)", op, sim);
  TRS_REQUIRE(anchor_idx == nullptr || idx_dtype == TRS_I64 || idx_dtype == TRS_I32, TRS_EINVAL, "%s: idx dtype %d", op,
              idx_dtype);
  TRS_REQUIRE((label_dtype == TRS_I64 || label_dtype == TRS_I32) && P >= 1 && P <= TR_MAX_P, TRS_EINVAL,
              "%s: label dtype %d, P = %d (1 .. %d)", op, label_dtype, P, TR_MAX_P);
  TRS_REQUIRE(exclude == nullptr || ((excl_dtype == TRS_I64 || excl_dtype == TRS_I32) && X >= 1 && X <= TR_MAX_X),
              TRS_EINVAL, "%s: exclude dtype %d, X = %d (1 .. %d)", op, excl_dtype, X, TR_MAX_X);
  const int64_t Vt = target_hi - target_lo;
  TRS_REQUIRE(Va > 0 && B >= 0 && target_lo >= 0 && Vt > 0 && Vt <= INT32_MAX, TRS_EINVAL,
              "%s: bad size Va=%lld B=%lld targets [%lld, %lld)", op, (long long)Va, (long long)B, (long long)target_lo,
              (long long)target_hi);
  const bool multi = G != 0;
  TRS_REQUIRE(!multi || (G >= 1 && G <= 16 && U >= 0 && B == U * G), TRS_EINVAL,
              "%s: G = %d (1 .. 16), U = %lld (>= 0), B = %lld (U * G)", op, G, (long long)U, (long long)B);
  const int gsh = multi ? gm_shift(G) : 0;
  const int row_bytes = E * dtype_size(dtype);
  TRS_REQUIRE(E > 0 && E <= TR_MAX_E && row_bytes % 16 == 0, TRS_ESHAPE,
              "%s: E = %d (rows of whole 16-byte vectors, E <= %d)", op, E, TR_MAX_E);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(anchor_table && target_table && labels && ranks && label_scores, TRS_EINVAL, "%s: NULL pointer", op);
  TRS_REQUIRE(aligned16(anchor_table) && aligned16(target_table), TRS_EALIGN, "%s: tables must be 16-byte aligned", op);
  RankArgsMI p;
  p.a_table = static_cast<const char*>(anchor_table);
  p.a_idx = anchor_idx;
  p.t_table = static_cast<const char*>(target_table);
  p.labels = labels;
  p.excl = exclude;
  p.ranks = ranks;
  p.lscore = label_scores;
  p.err_flag = err_flag;
  p.Va = Va;
  p.a_off = anchor_offset;
  p.B = multi ? U : B;
  p.G = multi ? G : 1;
  p.gsh = gsh;
  p.t_lo = target_lo;
  p.Vt = (int)Vt;
  p.S = tr_splits(multi ? U << gsh : B, Vt);      // what the anchor tiles are filled with
  p.rows_per = (int)((Vt + p.S - 1) / p.S);
  p.P = P;
  p.X = exclude != nullptr ? X : 0;
  p.row_bytes = row_bytes;
  p.nce = row_bytes / 16;
  p.nc = (p.nce + 3) / 4 * 4;
  // chunk swizzle, as topk.hip: r * nc mod 16 takes 16 / w values (w = the power of two in nc, at most 16); the other bits
  // of r & 15 go into the low bits of the chunk number
  const int w = std::min(16, p.nc & -p.nc);
  p.sw_mask = w - 1;
  p.sw_shift = w == 16 ? 0 : w == 8 ? 1 : 2;
  p.sim = sim;
  p.idx64 = idx_dtype == TRS_I64;
  p.lab64 = label_dtype == TRS_I64;
  p.excl64 = excl_dtype == TRS_I64;
  p.dma = !q8 && p.nce == p.nc;
  p.E = E;
  p.q_stride = (int)q8_stride(E);
  p.q_nv = p.q_stride / 16;
  hipStream_t s = (hipStream_t)stream;
  if (multi) return dtype == TRS_F32 ? tr_launch<float, false, true>(op, p, s) : tr_launch<bf16_t, false, true>(op, p, s);
  if (q8) return dtype == TRS_F32 ? tr_launch<float, true, false>(op, p, s) : tr_launch<bf16_t, true, false>(op, p, s);
  return dtype == TRS_F32 ? tr_launch<float, false, false>(op, p, s) : tr_launch<bf16_t, false, false>(op, p, s);
}

}  // namespace trs

using namespace trs;

// the counts of the target ranges meet in the output itself (integer atomics): no workspace at any shape
extern "C" size_t trs_target_ranks_workspace_bytes(int64_t B, int64_t Vt, int32_t P) { return 0; }

extern "C" int trs_target_ranks(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                                int64_t anchor_offset, int64_t B, const void* target_table, int64_t target_lo,
                                int64_t target_hi, int32_t E, int32_t dtype, int32_t sim, const void* labels,
                                int32_t label_dtype, int32_t P, const void* exclude, int32_t excl_dtype, int32_t X,
                                int64_t* ranks, float* label_scores, void* workspace, size_t ws_bytes, int32_t* err_flag,
                                trs_stream_t stream) {
  return tr_entry("target_ranks", false, 0, 0, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_table, target_lo,
                  target_hi, E, dtype, sim, labels, label_dtype, P, exclude, excl_dtype, X, ranks, label_scores, err_flag,
                  stream);
}

extern "C" int trs_target_ranks_q8(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                                   int64_t anchor_offset, int64_t B, const void* target_q, int64_t target_lo,
                                   int64_t target_hi, int32_t E, int32_t anchor_dtype, int32_t sim, const void* labels,
                                   int32_t label_dtype, int32_t P, const void* exclude, int32_t excl_dtype, int32_t X,
                                   int64_t* ranks, float* label_scores, void* workspace, size_t ws_bytes,
                                   int32_t* err_flag, trs_stream_t stream) {
  return tr_entry("target_ranks_q8", true, 0, 0, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_q, target_lo,
                  target_hi, E, anchor_dtype, sim, labels, label_dtype, P, exclude, excl_dtype, X, ranks, label_scores,
                  err_flag, stream);
}

extern "C" int trs_target_ranks_multi(const void* anchor_table, int64_t Va, const void* anchor_idx, int32_t idx_dtype,
                                      int64_t anchor_offset, int64_t B, int64_t U, int32_t G, const void* target_table,
                                      int64_t target_lo, int64_t target_hi, int32_t E, int32_t dtype, int32_t sim,
                                      const void* labels, int32_t label_dtype, int32_t P, const void* exclude,
                                      int32_t excl_dtype, int32_t X, int64_t* ranks, float* label_scores, void* workspace,
                                      size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  TRS_REQUIRE(G >= 1 && G <= 16, TRS_EINVAL, "target_ranks_multi: G = %d (1 .. 16)", G);
  return tr_entry("target_ranks_multi", false, U, G, anchor_table, Va, anchor_idx, idx_dtype, anchor_offset, B, target_table,
                  target_lo, target_hi, E, dtype, sim, labels, label_dtype, P, exclude, excl_dtype, X, ranks, label_scores,
                  err_flag, stream);
}
