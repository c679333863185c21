// Ragged bag pooling: one flat vector of ids (n,) plus offsets that say where each sample's bag begins -- the calling form of
// nn.EmbeddingBag and of feature pipelines -- pooled to one row per sample (sum / mean / max) without padding the bags to
// the longest one.  Bag b is ids[offsets[b], end_b), end_b = offsets[b + 1] where that entry exists, else n.
//
// The host never learns the longest bag, so the launch shape cannot depend on it.  Two tiers on the lane-group path (rows of
// a power-of-two number <= 64 of 16-byte vectors):
//   1. bag_ragged_group_kernel: one group of L lanes per bag, CH rows in flight, terms added in list order, sums in
//      registers, no LDS -- bag_pool_group_kernel (bag.hip) with the bag's bounds read from the offsets.  A bag of more
//      than BAG_RAGGED_LONG ids is not walked: lane 0 of its group appends b to a queue in the caller's workspace (one
//      counter + at most B entries: it cannot overflow).
//   2. bag_ragged_long_kernel, fixed grid: one WAVE per queued bag; its 64 / L lane groups stride the bag (group j takes
//      positions beg + j, beg + j + 64/L, ..), the partial sums -- or (maximum, position) pairs -- are folded across the
//      groups by shuffles, steps L, 2L, .., 32.  The queue ORDER depends on the atomics, the result does not: every bag is
//      reduced by one wave in an order that depends on its length alone.
// Any other E: one thread per (b, e), no long-bag tier.
// The kernels live in bag_ragged.hpp: bag_fields.hip runs them over the bags of F fields of one table.
//
// Offsets are range-checked on the device (no host read): begin and end are clamped to [0, n]; an offset outside [0, n]
// or a bag whose end lies before its begin (then empty) raises *err_flag.  Nothing is read outside ids[0, n).
// Algorithmic bytes: n * (idx bytes + E*s) + (B + 1) * offset bytes read, B * E*s written (+ 4 B for inv_cnt, + 4 B E for
// the max positions).
#include "bag_ragged.hpp"

namespace trs {

// bag_of[p] = the last b in [0, B) with offsets[b] <= p, provided p < end_b; else -1 (bag_ragged_owner_of).  One thread per
// position.
__global__ __launch_bounds__(256) void bag_owner_kernel(const void* __restrict__ offsets, bool off64, int64_t n_off,
                                                        int64_t B, int64_t n, int32_t* __restrict__ bag_of) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    bag_of[p] = bag_ragged_owner_of(offsets, off64, n_off, B, n, p);
  }
}

}  // namespace trs

using namespace trs;

extern "C" int32_t trs_bag_ragged_long_len(void) { return BAG_RAGGED_LONG; }

extern "C" size_t trs_bag_ragged_workspace_bytes(int64_t B) {
  if (B < 0) return 0;
  return bag_ragged_queue_bytes(B);      // [counter][at most B queued bags]
}

extern "C" int trs_bag_pool_ragged_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids,
                                       int32_t ids_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                                       int64_t n_off, int64_t B, int32_t mode, int64_t exclude_row, const void* weights,
                                       void* out, int32_t* argmax, float* inv_cnt, void* workspace, size_t ws_bytes,
                                       int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && offsets && out && workspace && (ids || n == 0), TRS_EINVAL, "bag_pool_ragged_fwd: NULL pointer");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN || mode == BAG_MAX, TRS_EINVAL,
              "bag_pool_ragged_fwd: mode %d (0 = sum, 1 = mean, 2 = max)", mode);
  TRS_REQUIRE(V > 0 && E > 0 && B > 0 && n >= 0, TRS_EINVAL, "bag_pool_ragged_fwd: bad size V=%lld E=%d B=%lld n=%lld",
              (long long)V, E, (long long)B, (long long)n);
  TRS_REQUIRE(n_off == B || n_off == B + 1, TRS_EINVAL, "bag_pool_ragged_fwd: %lld offsets for B=%lld bags (B or B + 1)",
              (long long)n_off, (long long)B);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE,
              "bag_pool_ragged_fwd: n=%lld and B=%lld must fit int32", (long long)n, (long long)B);
  TRS_REQUIRE(exclude_row >= -1 && exclude_row < V, TRS_EINVAL, "bag_pool_ragged_fwd: exclude_row %lld outside [-1, V)",
              (long long)exclude_row);
  TRS_REQUIRE(weights == nullptr || mode == BAG_SUM, TRS_EINVAL, "bag_pool_ragged_fwd: weights need mode 0 (sum), got %d",
              mode);
  TRS_REQUIRE(mode != BAG_MAX || argmax != nullptr, TRS_EINVAL,
              "bag_pool_ragged_fwd: max pooling needs the argmax output");
  TRS_REQUIRE(mode != BAG_MEAN || inv_cnt != nullptr, TRS_EINVAL, "bag_pool_ragged_fwd: the mean needs the inv_cnt output");
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_ragged_fwd: dtype %d", dtype);
  TRS_REQUIRE(ids_dtype == TRS_I64 || ids_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_fwd: ids dtype %d", ids_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_ragged_fwd: offsets dtype %d",
              off_dtype);
  TRS_REQUIRE(ws_bytes >= trs_bag_ragged_workspace_bytes(B), TRS_EWORKSPACE, "bag_pool_ragged_fwd: workspace %zu < %zu",
              ws_bytes, trs_bag_ragged_workspace_bytes(B));
  hipStream_t s = (hipStream_t)stream;
  float* ic = mode == BAG_MEAN ? inv_cnt : nullptr;
  int32_t* am = mode == BAG_MAX ? argmax : nullptr;
#define TRS_CALL(T, I)                                                                                                \
  return bag_ragged_launch<T, I, false>(table, (const I*)ids, n, offsets, off_dtype == TRS_I64, n_off, B, E, V, mode,      \
                                        exclude_row, weights, out, am, ic, (int32_t*)workspace, err_flag,                 \
                                        BagFieldMap{nullptr, 0, 1}, "bag_pool_ragged_fwd", s)
  if (dtype == TRS_F32) {
    if (ids_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (ids_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}

extern "C" int trs_bag_owner(const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int64_t n,
                             int32_t* bag_of, trs_stream_t stream) {
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(offsets && bag_of, TRS_EINVAL, "bag_owner: NULL pointer");
  TRS_REQUIRE(B > 0 && n >= 0 && (n_off == B || n_off == B + 1), TRS_EINVAL,
              "bag_owner: bad size B=%lld n=%lld, %lld offsets (B or B + 1)", (long long)B, (long long)n,
              (long long)n_off);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B < (int64_t)0x7fffffff, TRS_ESHAPE, "bag_owner: n=%lld and B=%lld must fit int32",
              (long long)n, (long long)B);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_owner: offsets dtype %d", off_dtype);
  hipLaunchKernelGGL(bag_owner_kernel, dim3(stream_grid(n, 256, 256 * 16)), dim3(256), 0, (hipStream_t)stream, offsets,
                     off_dtype == TRS_I64, n_off, B, n, bag_of);
  return check_launch("bag_owner");
}
