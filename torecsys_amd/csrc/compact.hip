// Device-side compaction of the row ids a shard owner received: K ids with repeats -> a fixed-shape open-addressing
// table of the distinct ones (row_map, T + 1 int32) and the slot of every position (inv, K int32).  Replaces
// torch.unique(ids, return_inverse=True) -- a device sort plus a host read of the distinct count -- on the owner-side
// fused-optimizer path of a large shard: shapes depend on K alone, nothing is read back, so the step can be captured.
//
// T = smallest power of two >= 2K (load <= 0.5), slot of id = top log2(T) bits of id * 2654435769 (Fibonacci hashing: ids
// that share their low bits -- multiples of 4096, of T -- still spread), linear probing.  A position first LOADS its
// slot: the repeats of a hot row (Zipf heads collect thousands of lookups) then find the key and leave without an atomic;
// a compare-and-swap (relaxed, agent scope: decided in L2, visible across XCDs) is issued only on a slot that read empty.
// The load is a plain, cacheable one on purpose.  After the clear a slot changes exactly once, from empty to its key, and
// the only writers are those swaps: a key that was read -- however old the cache line -- is final, and an "empty" that
// was stale is corrected by the swap, which returns the key that got there first.  (Lines from before the clear cannot
// be met: the clear is an earlier kernel.)  The price of the cacheable load: a CU that cached a slot while it was empty
// goes on to swap for every repeat of its key; on Zipf(1.05) ids the plain load measured 7 % faster than an agent-scope
// atomic load, no more (profiles/capturable_optimizer.md).  Atomics touch the integer keys only, never gradient values;
// which slot an id ends up in depends on the order the workgroups arrive in.
#include "trs_common.hpp"

namespace trs {

constexpr int32_t COMPACT_EMPTY = -1;

// every slot, the reserved one (row_map[T]) included, starts empty.  A kernel, not hipMemsetAsync: memset nodes did not
// hold in hipGraph replays here (see bucket_zero_kernel in shard.hip)
__global__ __launch_bounds__(256) void compact_clear_kernel(int32_t* __restrict__ row_map, int64_t n,
                                                            int32_t* __restrict__ counter) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) row_map[i] = COMPACT_EMPTY;
  if (counter != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *counter = 0;
}

__global__ __launch_bounds__(256) void compact_insert_kernel(const int32_t* __restrict__ ids, int64_t K,
                                                             int32_t* __restrict__ row_map, uint32_t T, int shift,
                                                             int32_t* __restrict__ inv) {
  const uint32_t mask = T - 1u;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += stride) {
    const int32_t id = ids[k];
    if (id < 0) {          // padding of a fixed-capacity exchange: the reserved slot, whose key stays -1
      inv[k] = (int32_t)T;
      continue;
    }
    uint32_t h = ((uint32_t)id * 2654435769u) >> shift;
    // at most T probes: the table holds at most K <= T/2 keys, so an empty slot (or the id itself) is always met earlier
    for (uint32_t probe = 0; probe < T; ++probe, h = (h + 1u) & mask) {
      int32_t cur = row_map[h];      // plain: the repeats of a hot row are served by the CU's own L1
      if (cur == COMPACT_EMPTY) {
        int32_t expected = COMPACT_EMPTY;
        if (__hip_atomic_compare_exchange_strong(&row_map[h], &expected, id, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT))
          cur = id;
        else
          cur = expected;      // somebody else's key arrived first (possibly this very id)
      }
      if (cur == id) {
        inv[k] = (int32_t)h;
        break;
      }
    }
  }
}

// ---- dense ranks (trs_compact_rows_dense): the occupied slots are numbered 0 .. U-1 ------------------------------
// The bucket build and the walk behind the compaction cost per ROW of the space they are handed, occupied or not (at 2.56 M
// ids: 8.4 M slots, 2.5 M of them occupied -- the owner update took 1.17 ms over the slots against 0.88 ms over
// torch.unique's distinct rows, profiles/capturable_optimizer.md).  So every occupied slot draws a rank: a workgroup
// counts the keys among its COMPACT_RANK_TILE slots, reserves that many ranks with ONE atomic, and numbers its keys in
// slot order behind them; dense_map[rank] = key, and the slot is overwritten with its rank for the remap pass.  Which
// ranks a workgroup gets depends on arrival order, like the slots themselves.
constexpr int COMPACT_RANK_PER_THREAD = 4;
constexpr int COMPACT_RANK_TILE = 256 * COMPACT_RANK_PER_THREAD;

__global__ __launch_bounds__(256) void compact_rank_kernel(int32_t* __restrict__ slot, int64_t T,
                                                           int32_t* __restrict__ counter,
                                                           int32_t* __restrict__ dense_map) {
  __shared__ int wave_sum[4];
  __shared__ int s_base;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t i0 = (int64_t)blockIdx.x * COMPACT_RANK_TILE + (int64_t)threadIdx.x * COMPACT_RANK_PER_THREAD;
  int32_t key[COMPACT_RANK_PER_THREAD];
  int cnt = 0;
#pragma unroll
  for (int i = 0; i < COMPACT_RANK_PER_THREAD; ++i) {
    key[i] = i0 + i < T ? slot[i0 + i] : COMPACT_EMPTY;
    cnt += key[i] >= 0 ? 1 : 0;
  }
  int inc = cnt;      // inclusive scan inside the wave, then over the four waves
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) wave_sum[wave] = inc;
  __syncthreads();
  int before = 0, total = 0;
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    if (w < wave) before += wave_sum[w];
    total += wave_sum[w];
  }
  if (threadIdx.x == 0) s_base = total > 0 ? atomicAdd(counter, total) : 0;
  __syncthreads();
  int r = s_base + before + inc - cnt;
#pragma unroll
  for (int i = 0; i < COMPACT_RANK_PER_THREAD; ++i) {
    if (key[i] >= 0) {      // (r < number of distinct ids <= K: inside dense_map)
      dense_map[r] = key[i];
      slot[i0 + i] = r;
      ++r;
    }
  }
}

// inv: slot -> rank (padding: the reserved row K); the rows of dense_map behind the U ranks, row K included, read -1
__global__ __launch_bounds__(256) void compact_remap_kernel(const int32_t* __restrict__ slot, uint32_t T, int64_t K,
                                                            const int32_t* __restrict__ counter,
                                                            int32_t* __restrict__ inv, int32_t* __restrict__ dense_map) {
  const int64_t U = *counter;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= K; k += stride) {
    if (k < K) {
      const uint32_t s = (uint32_t)inv[k];
      inv[k] = s >= T ? (int32_t)K : slot[s];
    }
    if (k >= U) dense_map[k] = COMPACT_EMPTY;
  }
}

static int64_t compact_slots(int64_t K) {
  int64_t T = 2;
  while (T < 2 * K) T <<= 1;
  return T;
}

// clear + insert on stream s: row_map (slots + 1) and inv (K) as trs_compact_rows leaves them
static void compact_insert_launch(const int32_t* ids, int64_t K, int32_t* row_map, int64_t slots, int32_t* inv,
                                  int32_t* counter, hipStream_t s) {
  hipLaunchKernelGGL(compact_clear_kernel, dim3(stream_grid(slots + 1, 256, 256 * 8)), dim3(256), 0, s, row_map, slots + 1,
                     counter);
  if (K > 0) {
    int shift = 32;
    for (int64_t t = slots; t > 1; t >>= 1) --shift;      // 32 - log2(slots); slots >= 2, so shift <= 31
    hipLaunchKernelGGL(compact_insert_kernel, dim3(stream_grid(K, 256, 256 * 16)), dim3(256), 0, s, ids, K, row_map,
                       (uint32_t)slots, shift, inv);
  }
}

}  // namespace trs

using namespace trs;

extern "C" int64_t trs_compact_rows_slots(int64_t K) { return K < 0 ? 0 : compact_slots(K); }

extern "C" int trs_compact_rows(const int32_t* ids, int64_t K, int32_t* row_map, int64_t slots, int32_t* inv,
                                trs_stream_t stream) {
  TRS_REQUIRE(K >= 0 && K < ((int64_t)1 << 29), TRS_ESHAPE, "compact_rows: K = %lld (must be in [0, 2^29))", (long long)K);
  TRS_REQUIRE(row_map && (K == 0 || (ids && inv)), TRS_EINVAL, "compact_rows: NULL pointer");
  TRS_REQUIRE(slots == compact_slots(K), TRS_EINVAL, "compact_rows: slots %lld, trs_compact_rows_slots(%lld) = %lld",
              (long long)slots, (long long)K, (long long)compact_slots(K));
  compact_insert_launch(ids, K, row_map, slots, inv, nullptr, (hipStream_t)stream);
  return check_launch("compact_rows");
}

/* see include/trs_abi.h: the same compaction with the distinct ids numbered densely */
extern "C" size_t trs_compact_rows_dense_workspace_bytes(int64_t K) {
  return K < 0 ? 0 : ((size_t)(compact_slots(K) + 1) * 4 + 255) / 256 * 256 + 256;      // the slots, then the rank counter
}

extern "C" int trs_compact_rows_dense(const int32_t* ids, int64_t K, int32_t* dense_map, int32_t* inv, void* workspace,
                                      size_t ws_bytes, trs_stream_t stream) {
  TRS_REQUIRE(K >= 0 && K < ((int64_t)1 << 29), TRS_ESHAPE, "compact_rows_dense: K = %lld (must be in [0, 2^29))",
              (long long)K);
  TRS_REQUIRE(dense_map && workspace && (K == 0 || (ids && inv)), TRS_EINVAL, "compact_rows_dense: NULL pointer");
  TRS_REQUIRE(ws_bytes >= trs_compact_rows_dense_workspace_bytes(K), TRS_EWORKSPACE, "compact_rows_dense: workspace %zu < %zu",
              ws_bytes, trs_compact_rows_dense_workspace_bytes(K));
  hipStream_t s = (hipStream_t)stream;
  const int64_t slots = compact_slots(K);
  int32_t* slot = (int32_t*)workspace;
  int32_t* counter = (int32_t*)((char*)workspace + ((size_t)(slots + 1) * 4 + 255) / 256 * 256);
  compact_insert_launch(ids, K, slot, slots, inv, counter, s);
  hipLaunchKernelGGL(compact_rank_kernel, dim3((unsigned)((slots + COMPACT_RANK_TILE - 1) / COMPACT_RANK_TILE)), dim3(256), 0,
                     s, slot, slots, counter, dense_map);
  hipLaunchKernelGGL(compact_remap_kernel, dim3(stream_grid(K + 1, 256, 256 * 16)), dim3(256), 0, s, slot, (uint32_t)slots, K,
                     counter, inv, dense_map);
  return check_launch("compact_rows_dense");
}
