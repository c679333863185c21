// Ragged bag pooling over F multi-valued fields of ONE table in one pass: the "keyed jagged" layout of feature pipelines --
// one values vector (n,) of RAW per-field ids and one offsets vector (F * B + 1,), field-major: bag j = f * B + b is the
// positions [offsets[j], offsets[j + 1]).  Field f owns the table rows [field_offsets[f], field_offsets[f + 1]).  The result
// is the (B, F, E) block the interaction layers consume: bag j is pooled into out row b * F + f, so F single-field passes
// and the copy that lines their (B, 1, E) results up are one gather.
//
// The forward is the two-tier forward of bag_ragged.hip over the F * B bags (bag_ragged.hpp, FIELDS = true): the same walk,
// the same order of every sum, the same queue of long bags; only where a bag's ids point (an id is checked against ITS
// field, then moved by the field's first row -- it can never reach a neighbouring field's row) and where its row is stored
// differ.  argmax and inv_cnt are indexed by OUT row, so the gradients are the existing ragged walks (bag.hip) on the map
// that bag_owner_fields_kernel writes: the out row and the table row of every position.
// Algorithmic bytes, forward: n * (idx bytes + E*s) + (F*B + 1) * offset bytes + 8 (F + 1) read, F*B * E*s written (+ 4 F*B
// for inv_cnt, + 4 F*B E for the max positions); map: n * idx bytes + the offsets a binary search touches (log2(F*B) per
// position, from L2) read, 12 n written.
#include "bag_ragged.hpp"

namespace trs {

// out_row_of[p] = b * F + f of the bag j = f * B + b that holds position p, rows[p] = values[p] + field_offsets[f]; -1 both
// where no bag holds p, rows[p] = -1 alone where the id lies outside its field.  One thread per position.
template <typename IdxT>
__global__ __launch_bounds__(256) void bag_owner_fields_kernel(const IdxT* __restrict__ values, int64_t n,
                                                               const void* __restrict__ offsets, bool off64,
                                                               int64_t n_off, int64_t FB, int64_t V, BagFieldMap fm,
                                                               int32_t* __restrict__ out_row_of,
                                                               int64_t* __restrict__ rows) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += stride) {
    const int64_t j = bag_ragged_owner_of(offsets, off64, n_off, FB, n, p);
    int32_t orow_p = -1;
    int64_t row = -1;
    if (j >= 0) {
      int64_t base, Vf, orow;
      bag_field_of<true>(fm, j, V, &base, &Vf, &orow);
      orow_p = (int32_t)orow;
      const int64_t id = (int64_t)values[p];
      if (id >= 0 && id < Vf) row = id + base;
    }
    out_row_of[p] = orow_p;
    rows[p] = row;
  }
}

}  // namespace trs

using namespace trs;

extern "C" size_t trs_bag_fields_workspace_bytes(int64_t FB) {
  if (FB < 0) return 0;
  return bag_ragged_queue_bytes(FB);      // [counter][at most F * B queued bags]
}

extern "C" int trs_bag_pool_fields_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* values,
                                       int32_t val_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                                       int64_t n_off, int64_t B, int32_t F, const int64_t* field_offsets, int32_t mode,
                                       const void* weights, void* out, int32_t* argmax, float* inv_cnt, void* workspace,
                                       size_t ws_bytes, int32_t* err_flag, trs_stream_t stream) {
  if (B == 0) return TRS_OK;  // empty batch: nothing to do (pointers may be NULL)
  TRS_REQUIRE(table && offsets && out && workspace && (values || n == 0), TRS_EINVAL,
              "bag_pool_fields_fwd: NULL pointer");
  TRS_REQUIRE(field_offsets != nullptr, TRS_EINVAL, "bag_pool_fields_fwd: field_offsets is NULL");
  TRS_REQUIRE(mode == BAG_SUM || mode == BAG_MEAN || mode == BAG_MAX, TRS_EINVAL,
              "bag_pool_fields_fwd: mode %d (0 = sum, 1 = mean, 2 = max)", mode);
  TRS_REQUIRE(F >= 1, TRS_EINVAL, "bag_pool_fields_fwd: F=%d fields, need at least one", F);
  TRS_REQUIRE(V > 0 && E > 0 && B > 0 && n >= 0, TRS_EINVAL, "bag_pool_fields_fwd: bad size V=%lld E=%d B=%lld n=%lld",
              (long long)V, E, (long long)B, (long long)n);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B <= (int64_t)0x7ffffffe / F, TRS_ESHAPE,
              "bag_pool_fields_fwd: n=%lld and F*B=%d*%lld must fit int32", (long long)n, F, (long long)B);
  const int64_t FB = (int64_t)F * B;
  TRS_REQUIRE(n_off == FB + 1, TRS_EINVAL, "bag_pool_fields_fwd: %lld offsets for F*B=%lld bags (F*B + 1)",
              (long long)n_off, (long long)FB);
  TRS_REQUIRE(weights == nullptr || mode == BAG_SUM, TRS_EINVAL, "bag_pool_fields_fwd: weights need mode 0 (sum), got %d",
              mode);
  TRS_REQUIRE(mode != BAG_MAX || argmax != nullptr, TRS_EINVAL,
              "bag_pool_fields_fwd: max pooling needs the argmax output");
  TRS_REQUIRE(mode != BAG_MEAN || inv_cnt != nullptr, TRS_EINVAL, "bag_pool_fields_fwd: the mean needs the inv_cnt output");
  TRS_REQUIRE(dtype == TRS_F32 || dtype == TRS_BF16, TRS_EDTYPE, "bag_pool_fields_fwd: dtype %d", dtype);
  TRS_REQUIRE(val_dtype == TRS_I64 || val_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_fields_fwd: values dtype %d", val_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_pool_fields_fwd: offsets dtype %d",
              off_dtype);
  TRS_REQUIRE(ws_bytes >= trs_bag_fields_workspace_bytes(FB), TRS_EWORKSPACE, "bag_pool_fields_fwd: workspace %zu < %zu",
              ws_bytes, trs_bag_fields_workspace_bytes(FB));
  hipStream_t s = (hipStream_t)stream;
  float* ic = mode == BAG_MEAN ? inv_cnt : nullptr;
  int32_t* am = mode == BAG_MAX ? argmax : nullptr;
  const BagFieldMap fm{field_offsets, B, F};
#define TRS_CALL(T, I)                                                                                                  \
  return bag_ragged_launch<T, I, true>(table, (const I*)values, n, offsets, off_dtype == TRS_I64, n_off, FB, E, V, mode,  \
                                       -1, weights, out, am, ic, (int32_t*)workspace, err_flag, fm,                     \
                                       "bag_pool_fields_fwd", s)
  if (dtype == TRS_F32) {
    if (val_dtype == TRS_I64) TRS_CALL(float, int64_t);
    TRS_CALL(float, int32_t);
  }
  if (val_dtype == TRS_I64) TRS_CALL(bf16_t, int64_t);
  TRS_CALL(bf16_t, int32_t);
#undef TRS_CALL
}

extern "C" int trs_bag_owner_fields(const void* values, int32_t val_dtype, int64_t n, const void* offsets,
                                    int32_t off_dtype, int64_t n_off, int64_t B, int32_t F, int64_t V,
                                    const int64_t* field_offsets, int32_t* out_row_of, int64_t* rows,
                                    trs_stream_t stream) {
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(values && offsets && field_offsets && out_row_of && rows, TRS_EINVAL, "bag_owner_fields: NULL pointer");
  TRS_REQUIRE(F >= 1 && B > 0 && n >= 0 && V > 0, TRS_EINVAL, "bag_owner_fields: bad size F=%d B=%lld n=%lld V=%lld", F,
              (long long)B, (long long)n, (long long)V);
  TRS_REQUIRE(n < (int64_t)0x7fffffff && B <= (int64_t)0x7ffffffe / F, TRS_ESHAPE,
              "bag_owner_fields: n=%lld and F*B=%d*%lld must fit int32", (long long)n, F, (long long)B);
  const int64_t FB = (int64_t)F * B;
  TRS_REQUIRE(n_off == FB + 1, TRS_EINVAL, "bag_owner_fields: %lld offsets for F*B=%lld bags (F*B + 1)", (long long)n_off,
              (long long)FB);
  TRS_REQUIRE(val_dtype == TRS_I64 || val_dtype == TRS_I32, TRS_EDTYPE, "bag_owner_fields: values dtype %d", val_dtype);
  TRS_REQUIRE(off_dtype == TRS_I64 || off_dtype == TRS_I32, TRS_EDTYPE, "bag_owner_fields: offsets dtype %d", off_dtype);
  const BagFieldMap fm{field_offsets, B, F};
  const dim3 grid(stream_grid(n, 256, 256 * 16));
  if (val_dtype == TRS_I64)
    hipLaunchKernelGGL(bag_owner_fields_kernel<int64_t>, grid, dim3(256), 0, (hipStream_t)stream, (const int64_t*)values,
                       n, offsets, off_dtype == TRS_I64, n_off, FB, V, fm, out_row_of, rows);
  else
    hipLaunchKernelGGL(bag_owner_fields_kernel<int32_t>, grid, dim3(256), 0, (hipStream_t)stream, (const int32_t*)values,
                       n, offsets, off_dtype == TRS_I64, n_off, FB, V, fm, out_row_of, rows);
  return check_launch("bag_owner_fields");
}
