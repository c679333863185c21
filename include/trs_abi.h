/*
 * trs_abi.h -- C ABI of libtrs_hip.so, the MI355X (gfx950) kernels behind the torecsys
 * embedding-lookup + feature-interaction hot path.
 *
 * The reference (p768lwy3/torecsys) is pure Python on PyTorch: it has no FFI of its own, the
 * "plugin interface" for this path is nn.Module.forward().  Each entry point below therefore
 * cites the reference forward() (file:line, relative to the reference root) whose ATen ops it
 * replaces.  The Python host side (torecsys_amd/) mirrors those nn.Modules and calls these
 * symbols through ctypes; INTEGRATION.md shows the binding a maintainer adds on the reference side.
 *
 * Conventions
 *  - plain C: POD arguments only -- device pointers, sizes, dtype codes, a hipStream_t as void*;
 *  - the CALLER owns every buffer (inputs, outputs, workspaces); the library never allocates,
 *    frees or keeps a pointer after the call; all tensors are dense, row-major, contiguous;
 *  - every call only ENQUEUES work on the caller's stream (no hidden synchronisation);
 *  - return 0 (TRS_OK) or a negative TRS_E* code; trs_last_error_string() (thread-local) explains;
 *  - no C++ exception crosses this boundary; the library is stateless and re-entrant;
 *  - dtype codes: TRS_F32 / TRS_BF16 for values, TRS_I64 / TRS_I32 for indices;
 *  - "offsets" is the per-field row offset vector (N int64, device) added to the raw indices,
 *    or NULL for none; "err_flag" (device int32, may be NULL) is set to 1 when an index falls
 *    outside [0,V) -- the row is then skipped (zeros on a gather) instead of read out of bounds.
 */
#ifndef TRS_ABI_H_
#define TRS_ABI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRS_ABI_VERSION 3

enum { TRS_F32 = 0, TRS_BF16 = 1 };
enum { TRS_I64 = 0, TRS_I32 = 1 };
enum {
  TRS_OK = 0,
  TRS_EINVAL = -1,     /* NULL pointer / negative size / bad flag */
  TRS_EDTYPE = -2,     /* unsupported dtype code */
  TRS_ESHAPE = -3,     /* unsupported shape (e.g. N or E beyond a kernel's limits) */
  TRS_EALIGN = -4,     /* pointer not aligned for the vector path */
  TRS_ELAUNCH = -5,    /* hip launch error (hipGetLastError) */
  TRS_EWORKSPACE = -6  /* workspace too small */
};

typedef void* trs_stream_t; /* hipStream_t */

int trs_version(void);
const char* trs_last_error_string(void);

/* ---- diagnostics: device-side timestamps that survive hipGraph replay -----------------------
 * Enqueues a one-lane kernel that appends the device wall clock (constant rate, trs_wall_clock_khz())
 * to a ring in device memory:  i = ring[0]++;  ring[1 + i % capacity] = wall_clock64().
 * Two marks bracketing a launch on the same stream measure it like a HIP event pair does, but each
 * replay of a captured graph appends a new sample (a captured event pair only keeps the last one).
 * ring: capacity+1 uint64, zero-initialised by the caller.  No reference counterpart (measurement only). */
int trs_mark_timestamp(uint64_t* ring, int32_t capacity, trs_stream_t stream);
int64_t trs_wall_clock_khz(void);

/* ---- K1: row gather ---------------------------------------------------------------------
 * out[b,n,:] = table[idx[b,n] + offsets[n], :]            (bit-exact copy)
 * replaces aten::add + aten::embedding in
 *   torecsys/inputs/base/multi_indices_emb.py:104-105, single_index_emb.py:56-57.            */
int trs_gather_rows(const void* table, int64_t V, int32_t E, int32_t dtype,
                    const void* idx, int32_t idx_dtype, const int64_t* offsets,
                    int64_t B, int32_t N, void* out, int32_t* err_flag, trs_stream_t stream);

/* ---- N separate tables, one index column each: a StackedInput of SingleIndexEmbeddings in one launch -------------
 * inputs/base/stacked_inp.py:94-134 calls N SingleIndexEmbeddings (single_index_emb.py:48-59: nn.Embedding on a (B,1)
 * column) and concatenates along N.  out[b,n,:] = tables[n][idx[b,n],:], bit-exact.  tables: DEVICE array of N base
 * pointers (rows of E elements, 16-byte aligned when E*sizeof(T) is a multiple of 16); table_rows: DEVICE array of N row
 * counts; idx (B,N) int64/int32 RAW per-table indices (no offsets).  An index outside its table reads as a zero row and
 * raises *err_flag.  Backward: the caller buckets idx over the concatenated row space (trs_csr_build with offsets =
 * cumulative row counts) and scatters into one (sum rows, E) gradient whose slices are the tables' gradients.          */
int trs_gather_rows_tables(const void* const* tables, const int64_t* table_rows, int32_t E, int32_t dtype, const void* idx,
                           int32_t idx_dtype, int64_t B, int32_t N, void* out, int32_t* err_flag, trs_stream_t stream);

/* ---- I3: field-aware gather ---------------------------------------------------------------
 * out[b, i*N+j, :] = tables[i][idx[b,j] + offsets[j], :]   for i,j in [0,N)
 * `tables` = device array of N table base pointers (each V x E).
 * replaces the N lookups + cat of multi_indices_field_aware_emb.py:102-105.                   */
int trs_fa_gather_rows(const void* const* tables, int64_t V, int32_t E, int32_t dtype,
                       const void* idx, int32_t idx_dtype, const int64_t* offsets,
                       int64_t B, int32_t N, void* out, int32_t* err_flag, trs_stream_t stream);

/* ---- row-bucketed index (CSR) ---------------------------------------------------------------
 * Groups the B*N lookups by destination row: perm[row_start[r] .. row_start[r+1]) lists the
 * flat positions p = b*N+n with idx[p]+offsets[p%N] == r.  Built once per batch, shared by every
 * table looked up with the same indices.  row_start: V+1 int32; perm: B*N int32.
 * Replaces the index_add loop of aten::embedding_dense_backward (reached from
 * multi_indices_emb.py:105 through autograd) with an atomics-free segmented reduction.       */
size_t trs_csr_workspace_bytes(int64_t V, int64_t BN);
int trs_csr_build(const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N,
                  int64_t V, int32_t* row_start, int32_t* perm, void* workspace, size_t ws_bytes,
                  int32_t* err_flag, trs_stream_t stream);

/* The same index with the lookups of ONE row left out: row skip_row gets an empty bucket (row_start[skip_row + 1] ==
 * row_start[skip_row]) and its positions do not appear in perm (the tail of perm past row_start[V] is unspecified); the
 * flag is not raised for them.  skip_row = -1: identical to trs_csr_build.  For a padded list field (the (B, L) ids of
 * list_indices_emb.py:124, padding_idx = 0): the walks skip the padding row anyway, while filing a third or more of all
 * B*L positions under it is one returning atomic per position on a single counter -- measured at B*L = 3.3 M, 1 M rows:
 * 0.22 ms without padding, 22 ms with 60 % (profiles/bag_kernels.md).                                                  */
int trs_csr_build_skip(const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N, int64_t V,
                       int64_t skip_row, int32_t* row_start, int32_t* perm, void* workspace, size_t ws_bytes,
                       int32_t* err_flag, trs_stream_t stream);

/* ---- K1 backward: dense-gradient scatter ----------------------------------------------------
 * grad_table[r,:] = sum_{p in row r} ( g_rows[p,:]  +  g_fm[b_p,:] * (fm_sum[b_p,:] - table[r,:]) )
 * for EVERY r in [0,V) (rows without lookups are written as zeros: nn.Embedding's default
 * sparse=False gradient, multi_indices_emb.py:48).  g_rows (B*N x E, may be NULL) is the
 * gradient of the gathered block; the second term (g_fm B x E, fm_sum B x E fp32, table; all
 * NULL to disable) is the FM second-order backward dx = g*(S - x) of
 * layers/ctr/factorization_machine.py:62-73 fused into the same pass.  padding_row (-1: none)
 * gets a zero gradient (nn.Embedding padding_idx).  fp32 accumulation, one rounding on store.
 * g_fm_cols = E: g_fm holds full (B x E) rows; g_fm_cols = 1 (with fm_sum): g_fm holds ONE value per sample, the
 * gradient is constant along E (the backward of a sum over E -- what the reference's FM / DeepFM models feed back,
 * models/ctr/deep_fm.py:55-110): the walk then reads 144 instead of 256 bytes of FM operands per lookup.
 * With fm_sum == NULL, g_fm is a plain per-sample gradient broadcast over the N fields (the
 * first-order sum's backward; g_fm_cols = E).  g_rows_batch_stride (rows; 0 = N) lets g_rows be a (B, N, E) slice
 * of a larger (B, M, E) tensor: the row of position (b,n) is b*stride + n.
 * Rows with more than 256 lookups (Zipf-hot rows) are queued in `workspace`
 * (trs_scatter_workspace_bytes) and reduced by whole workgroups; the workspace also holds the
 * per-sample [g*S | g] rows the FM term is read from.                         */
size_t trs_scatter_workspace_bytes(int64_t BN, int32_t N, int32_t E, int32_t dtype);
int trs_scatter_rows(const void* g_rows, int64_t g_rows_batch_stride, const void* g_fm, int32_t g_fm_cols,
                     const float* fm_sum, const void* table, const int32_t* row_start,
                     const int32_t* perm, int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype,
                     int64_t padding_row, void* grad_table, void* workspace, size_t ws_bytes,
                     trs_stream_t stream);

/* trs_scatter_rows plus the dense gradient of the companion first-order table (V x 1) of the same lookups in the same
 * bucket walk: grad_first[r] = sum over the lookups (b,n) of row r of g_first[b,n]  (g_first: (B,N), one value per
 * lookup; every row of grad_first is written).  Rows must be whole 16-byte vectors (E*sizeof(dtype) % 16 == 0).
 * Replaces the second embedding backward of the (B,N,1) first-order lookup (torch embedding_dense_backward of
 * multi_indices_emb.py:104-105 at embed_size = 1).                                                               */
int trs_scatter_rows_first(const void* g_rows, int64_t g_rows_batch_stride, const void* g_fm, int32_t g_fm_cols,
                           const float* fm_sum,
                           const void* table, const int32_t* row_start, const int32_t* perm, int64_t BN, int64_t V,
                           int32_t E, int32_t N, int32_t dtype, int64_t padding_row, void* grad_table,
                           const void* g_first, void* grad_first, void* workspace, size_t ws_bytes,
                           trs_stream_t stream);

/* Same walk, but the finished row sum g is APPLIED to the table row in place by a fused sparse optimizer (SURVEY.md
 * section 8f N1) instead of being written out.  Rows nobody looked up have zero gradient and are not touched -- neither
 * the dense V x E gradient nor a dense optimizer pass over the table exists.  Both update entries end in the same
 * optimizer tail:
 *   optimizer  1 = SGD      w -= lr*g
 *              2 = Adagrad  state += g*g;  w -= lr*g/(sqrt(state)+eps)
 *              3 = lazy Adam (torch.optim.SparseAdam semantics: moments and weights of looked-up rows only; the reference
 *                  trains with dense Adam, trainer/torecsys_pipeline.py:562-578, which cannot exist at 1 B rows)
 *                  m = m + (g - m)(1 - beta1);  v = v + (g*g - v)(1 - beta2);  w -= lr * m / (sqrt(v) + eps)
 *                  where the step size passed as lr is already bias-corrected by the caller:
 *                  lr * sqrt(1 - beta2^t) / (1 - beta1^t); state = exp_avg (m), state2 = exp_avg_sq (v)
 *              1 and 2 are exactly the dense torch.optim.SGD / Adagrad step (no momentum / weight decay).
 *              2 | TRS_OPT_ROWWISE = row-wise Adagrad, ONE accumulator per table row (the flag is valid on 2 only; every
 *                  other value -- 0, 4, the bare flag, 1 | flag, 3 | flag, any other bit -- is TRS_EINVAL):
 *                  s[r] += mean_e(g[r,e]^2);  w[r,e] -= lr * g[r,e] / (sqrt(s[r]) + eps)
 *                  The mean is summed in this order, which is part of the result (fp32, every square and add rounded,
 *                  no fma): a row is L = E*sizeof/16 lanes of VE = 16/sizeof values (4 fp32, 8 bf16), lane l holding
 *                  elements l*VE .. l*VE+VE-1; each lane sums its squares left to right; the L partial sums are folded
 *                  by a butterfly that pairs lanes 1 apart, then 2, .., then L/2 apart; the total is multiplied by 1/E
 *                  (exact: E is a power of two) and added to s[r].  state is V fp32, indexed by the TABLE row (through
 *                  row_map in the mapped entry: an entry outside [0, V) moves neither weight nor state); state2 is
 *                  ignored.  Rows must be 1, 2, 4 .. 64 whole 16-byte vectors behind 16-byte aligned pointers (the walk
 *                  that puts a row into one lane group); any other width or alignment is TRS_ESHAPE before any launch.
 *                  For E = 1 the rule is optimizer 2 on a V x 1 state.
 *   lr, lr_dev lr_dev == NULL: the step size is lr, by value.  lr_dev != NULL: it is ONE fp32 in device memory, read by
 *              the kernels when they apply a row, and lr is ignored: a launch captured into a hipGraph then follows a
 *              learning rate written between replays (FusedSparse*.set_lr) and Adam's per-step bias correction
 *              (trs_adam_step_size below) instead of repeating the capture-time value.
 *   beta1, beta2   Adam only, each in [0, 1).
 *   state, state2  V x E fp32 (row-wise Adagrad: state is V fp32); state is needed by optimizers 2 and 3, state2 by 3;
 *              NULL otherwise.
 * The tail is validated before anything is launched (TRS_EINVAL).                                                    */
#define TRS_OPT_ROWWISE 16
int trs_scatter_rows_update(const void* g_rows, int64_t g_rows_batch_stride, const void* g_fm, int32_t g_fm_cols,
                            const float* fm_sum, void* table, const int32_t* row_start, const int32_t* perm,
                            int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype, int64_t padding_row,
                            int32_t optimizer, float lr, const float* lr_dev, float eps, float beta1, float beta2,
                            float* state, float* state2, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* The same fused optimizer step when the bucketed rows are a COMPACT list of U distinct table rows (the owner side of
 * a row-sharded table: a 125 M-row shard cannot afford a V-sized bucket index per step):  row_start (U+1) / perm (K)
 * bucket the K gradient rows g_rows (K,E) by compact row u, row_map[u] is the table row that compact row u updates
 * (distinct values; an entry outside [0, V) updates nothing).  The optimizer tail is the one described above; state
 * buffers are V x E fp32.  U == 0 or K == 0: nothing to do, TRS_OK.  Workspace: trs_scatter_workspace_bytes(K, 1, E,
 * dtype). */
int trs_scatter_rows_update_mapped(const void* g_rows, void* table, const int32_t* row_map, const int32_t* row_start,
                                   const int32_t* perm, int64_t K, int64_t U, int64_t V, int32_t E, int32_t dtype,
                                   int32_t optimizer, float lr, const float* lr_dev, float eps, float beta1, float beta2,
                                   float* state, float* state2, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* Adam's per-step scalars, on the device (one thread):  *step += 1;  *step_size_dev = *lr_dev * sqrt(1 - beta2^t) /
 * (1 - beta1^t) with t the new *step -- computed in double, rounded once to fp32 (what the host computes when it
 * passes the step size by value).  Enqueued once per table per backward in front of the update that reads it through
 * lr_dev. */
int trs_adam_step_size(int64_t* step, const float* lr_dev, double beta1, double beta2, float* step_size_dev,
                       trs_stream_t stream);

/* ---- stochastic rounding of bf16 tables under the fused optimizers ---------------------------------------------------
 * The update entries above compute the new weight of a touched row in fp32 and store it round-to-nearest-even; on a bf16
 * table (no fp32 master copy) an update below half an ulp of the weight -- 2^-9 at w = 1.0 -- is dropped at every step.
 * The _sr entries store it with stochastic rounding instead, by a rule in integer arithmetic that the host reproduces
 * bit for bit (csrc/stochastic_round.hpp, one __host__ __device__ function):
 *
 *   sr_bf16(x, i, seed, t): the fp32 value x, destined for table element i = table_row * E + column (int64), in update
 *   number t (uint64) of that table.  u = bits(x).
 *     exponent field of u all ones (inf, NaN):  result = u >> 16
 *     otherwise:                                result = (u + r) >> 16,  r a uniform 16-bit integer
 *   An fp32 value that already is a bf16 value is never changed; any other is rounded away from zero with probability
 *   (u & 0xffff) / 65536 and towards zero otherwise, so the expectation of the stored value is x.  (The largest finite
 *   values can round to infinity, as they do under round-to-nearest.)
 *
 *   r is a pure function of (seed, t, i): no launch geometry, lane-group width, vector or element walk, hot-row queue,
 *   chunk, or mapped / unmapped entry enters it.  Philox4x32-10 (Salmon et al., SC'11; multipliers D2511F53 and CD9E8D57,
 *   key increments 9E3779B9 and BB67AE85, ten rounds) with
 *     counter = (lo32(q), hi32(q), lo32(t), hi32(t)),  q = i >> 3
 *     key     = (lo32(seed), hi32(seed))
 *   gives four 32-bit words; element i takes 16 bits of word (i & 7) >> 1: the low half for even i, the high half for
 *   odd i.  One call therefore serves the 8 bf16 elements of one 16-byte vector of the table (q = row * L + lane in the
 *   lane-group walk).  In the mapped entry table_row is the table row row_map points at.
 *
 * trs_scatter_rows_update_sr / trs_scatter_rows_update_mapped_sr take the argument lists of their plain counterparts, the
 * same validated optimizer tail (every optimizer value, row-wise included) and the same walk, plus
 *   seed    of the optimizer
 *   t       the update number of this table, by value (the first update of a table is 1; every update call on a table
 *           takes the next value, so two walks over one table in one backward draw different bits)
 *   t_dev   NULL, or ONE int64 in device memory that overrides t (as lr_dev overrides lr): a launch captured into a
 *           hipGraph then draws fresh bits at every replay, with trs_sr_advance enqueued in front of it.
 * dtype TRS_BF16 takes the stochastic-rounding instantiations of the kernels; dtype TRS_F32 has nothing to round and runs
 * exactly what the plain entry runs.  The optimizer state (fp32) is what the plain entry leaves.                        */
int trs_scatter_rows_update_sr(const void* g_rows, int64_t g_rows_batch_stride, const void* g_fm, int32_t g_fm_cols,
                               const float* fm_sum, void* table, const int32_t* row_start, const int32_t* perm,
                               int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype, int64_t padding_row,
                               int32_t optimizer, float lr, const float* lr_dev, float eps, float beta1, float beta2,
                               float* state, float* state2, void* workspace, size_t ws_bytes, trs_stream_t stream,
                               uint64_t seed, uint64_t t, const int64_t* t_dev);
int trs_scatter_rows_update_mapped_sr(const void* g_rows, void* table, const int32_t* row_map, const int32_t* row_start,
                                      const int32_t* perm, int64_t K, int64_t U, int64_t V, int32_t E, int32_t dtype,
                                      int32_t optimizer, float lr, const float* lr_dev, float eps, float beta1,
                                      float beta2, float* state, float* state2, void* workspace, size_t ws_bytes,
                                      trs_stream_t stream, uint64_t seed, uint64_t t, const int64_t* t_dev);

/* *t_dev += 1 on the device (one thread): enqueued once per update call in front of the _sr entry that reads t_dev. */
int trs_sr_advance(int64_t* t_dev, trs_stream_t stream);

/* Host only, no device needed: out[k] = sr_bf16(x[k], first + k, seed, t) for k in [0, n) -- the rule itself, and
 * out[0..3] = Philox4x32-10(counter[0..3]; key[0..1]) -- the generator under it. */
int trs_sr_bf16_host(const float* x, int64_t n, int64_t first, uint64_t seed, uint64_t t, uint16_t* out);
int trs_philox4x32_10_host(const uint32_t* counter, const uint32_t* key, uint32_t* out);

/* ---- device-side row compaction (owner side of a large row-sharded table) ---------------------------------------
 * ids (K int32, local row ids with repeats) -> row_map (T + 1 int32) and inv (K int32), T = trs_compact_rows_slots(K) =
 * the smallest power of two >= max(2K, 2): fixed shapes, no read-back, no allocation -- replaces torch.unique(ids,
 * return_inverse=True) in front of trs_scatter_rows_update_mapped, so the step can be captured into a hipGraph.
 *   - every id >= 0 owns exactly one slot s < T: row_map[s] == id and inv[k] == s wherever ids[k] == id; distinct ids
 *     own distinct slots (ids >= the table's rows are stored like any other: the mapped update skips them);
 *   - every id < 0 (the -1 padding of a fixed-capacity exchange) gets inv[k] == T, and row_map[T] == -1;
 *   - every slot that holds no id reads -1.
 * Which slot an id gets is unspecified and differs from run to run (an open-addressing hash table filled by racing
 * workgroups: atomics on the integer keys only).  `slots` must equal trs_compact_rows_slots(K); K < 2^29.             */
int64_t trs_compact_rows_slots(int64_t K);
int trs_compact_rows(const int32_t* ids, int64_t K, int32_t* row_map, int64_t slots, int32_t* inv, trs_stream_t stream);

/* The same compaction with the U distinct ids numbered DENSELY, for consumers whose cost grows with the row space they
 * are handed (the bucket build and the bucket walk: what the owner-side optimizer step uses): two more passes give every
 * occupied slot a rank in [0, U).  dense_map (K + 1 int32) and inv (K int32):
 *   - every id >= 0 owns exactly one row u < U <= K: dense_map[u] == id and inv[k] == u wherever ids[k] == id;
 *   - every id < 0 gets inv[k] == K; dense_map[u] == -1 for every u in [U, K];
 *   - which row an id gets is unspecified.  U itself stays on the device.
 * workspace (trs_compact_rows_dense_workspace_bytes) holds the hash table; same limits and guarantees otherwise.        */
size_t trs_compact_rows_dense_workspace_bytes(int64_t K);
int trs_compact_rows_dense(const int32_t* ids, int64_t K, int32_t* dense_map, int32_t* inv, void* workspace,
                           size_t ws_bytes, trs_stream_t stream);

/* ---- K1+K2(+K8): fused embedding lookup + FM second order ----------------------------------
 * emb[b,n,:]  = table[idx[b,n]+offsets[n], :]                       (optional, may be NULL)
 * fm[b,:]     = 0.5 * ((sum_n x)^2 - sum_n x^2)                     (optional, may be NULL)
 * fm_sum[b,:] = sum_n x   (fp32, optional; saved for the backward)
 * first[b]    = sum_n first_table[idx[b,n]+offsets[n]]              (optional E=1 first-order term)
 * replaces multi_indices_emb.py:104-105 + factorization_machine.py:62-73
 * (+ models/ctr/deep_fm.py:73-89 first-order sum) in one pass over the table rows.           */
int trs_embed_fm(const void* table, int64_t V, int32_t E, int32_t dtype,
                 const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N,
                 void* emb, void* fm, float* fm_sum, const void* first_table, void* first,
                 int32_t* err_flag, trs_stream_t stream);

/* The same pass when the first-order term stays a per-field tensor, as the reference's models consume it
 * (``feat_inputs`` (B,N,1) of models/ctr/deep_fm.py:73-89, factorization_machine.py model, xdeep_fm.py):
 * first_vals[b,n] = first_table[idx[b,n]+offsets[n]]  (0 for an out-of-range lookup) -- replaces the separate
 * MultiIndicesEmbedding(embed_size=1) lookup (multi_indices_emb.py:104-105) of the same index block.            */
int trs_embed_fm_fields(const void* table, int64_t V, int32_t E, int32_t dtype,
                        const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N,
                        void* emb, void* fm, float* fm_sum, const void* first_table, void* first_vals,
                        int32_t* err_flag, trs_stream_t stream);

/* ---- bag pooling: a padded list of ids per sample, looked up in one table and pooled to one row -----------------------
 * idx (B, L) int64/int32 RAW row ids (no offsets), table (V, E):
 *   mode 0 (sum):  out[b,:] = sum_l table[idx[b,l], :]
 *   mode 1 (mean): out[b,:] = (sum_l table[idx[b,l], :]) * (1/L)        every position counts, padding ids included
 *   mode 2 (max):  out[b,e] = max_l table[idx[b,l], e];  argmax[b,e] (uint16) = the FIRST list position l that holds it
 *                  (a later value wins only when it is greater or NaN: ATen's adaptive_max_pool rule)
 * out (B, E) of the table's dtype; argmax (B, E) uint16, required for mode 2, ignored otherwise; 1 <= L <= 65535.
 * fp32 accumulation, one rounding on store; the max is a selection (bit-exact).  An id outside [0, V) reads as a zero
 * row and raises *err_flag.  The (B, L, E) block is never formed.  Rows that are a power-of-two number (<= 64) of whole
 * 16-byte vectors take the lane-group path; any other E one thread per (b, e).
 * replaces aten::embedding + align_to + AdaptiveAvgPool1d(1) / AdaptiveMaxPool1d(1) of
 *   torecsys/inputs/base/list_indices_emb.py:124-152 (use_attn=False).
 * Backward of sum / mean: trs_csr_build on the (B, L) ids (N = L) + trs_scatter_rows with g_rows = NULL, g_fm = the
 * (B, E) output gradient (times 1/L for the mean), fm_sum = NULL, g_fm_cols = E.                                      */
int trs_bag_pool_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                     int64_t B, int32_t L, int32_t mode, void* out, uint16_t* argmax, int32_t* err_flag,
                     trs_stream_t stream);

/* Backward of mode 2 on the row buckets of the same ids (trs_csr_build, N = L):
 *   grad_table[r,e] = sum over the lookups p = (b,l) of row r of ( argmax[b,e] == l ? g[b,e] : 0 )
 * for EVERY r in [0,V) (rows without lookups and padding_row are written as zeros; -1: no padding row).  g (B, E) of the
 * table's dtype, argmax (B, E) as written by trs_bag_pool_fwd.  No atomics on values, fixed summation order; rows with
 * more than 64 lookups are queued in `workspace` and reduced by whole waves, 256 lookups at a time.
 * replaces the adaptive_max_pool backward + transpose + embedding_dense_backward reached from
 *   list_indices_emb.py:124-152 through autograd.                                                                     */
size_t trs_scatter_argmax_workspace_bytes(int64_t BN, int32_t E);
int trs_scatter_rows_argmax(const void* g, const uint16_t* argmax, const int32_t* row_start, const int32_t* perm,
                            int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype, int64_t padding_row,
                            void* grad_table, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* Bag pooling that leaves one row id out and / or weights every id (nn.EmbeddingBag's padding_idx and
 * per_sample_weights).  live(b,l) := idx[b,l] != exclude_row (every position when exclude_row = -1), cnt[b] = the number
 * of live positions, w = weights (B, L) of the table's dtype or NULL (= 1):
 *   mode 0 (sum):  out[b,:] = sum_live w[b,l] * table[idx[b,l], :]
 *   mode 1 (mean): out[b,:] = (sum_live table[idx[b,l], :]) * inv_cnt[b],  inv_cnt[b] = 1/cnt[b], 0 when cnt[b] == 0
 *                  (an empty bag is a zero row); inv_cnt (B,) fp32 is written for the backward and required when
 *                  exclude_row >= 0; with exclude_row = -1 it is not touched and the scale is 1/L
 *   mode 2 (max):  the maximum over the live positions, the first live position winning a tie; an empty bag gives a zero
 *                  row and argmax[b,:] = 0xFFFF, which no position equals: L <= 65534 when exclude_row >= 0
 * An excluded position issues no table load and its weight is not read.  A live id outside [0, V) reads as a zero row,
 * raises *err_flag and counts in cnt.  Arithmetic, paths and outputs as trs_bag_pool_fwd.
 * TRS_EINVAL: NULL table / idx / out, exclude_row outside [-1, V), neither exclude_row >= 0 nor weights (that call is
 * trs_bag_pool_fwd), weights with mode != 0, mode 2 without argmax, mode 1 with exclude_row >= 0 without inv_cnt, L out
 * of range; TRS_EDTYPE: dtype / idx_dtype.  All before any launch.
 * Backward: trs_csr_build_skip(skip_row = exclude_row) + trs_scatter_rows with g_fm = g (mean: g * inv_cnt[b]) or
 * trs_scatter_rows_argmax; with weights trs_scatter_rows_weighted and, for the weights' own gradient, trs_bag_weight_grad.
 * replaces F.embedding_bag(idx, table, mode=..., padding_idx=..., per_sample_weights=...) on 2-D idx.                 */
int trs_bag_pool_masked_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                            int64_t B, int32_t L, int32_t mode, int64_t exclude_row, const void* weights, void* out,
                            uint16_t* argmax, float* inv_cnt, int32_t* err_flag, trs_stream_t stream);

/* Table gradient of the weighted sum on the row buckets of the same ids (trs_csr_build / trs_csr_build_skip, N = L):
 *   grad_table[r,:] = sum over the lookups p = (b,l) of row r of  weights[p] * g[b,:]
 * for EVERY r in [0,V) (rows without lookups and padding_row are written as zeros; -1: no padding row).  g (B, E) and
 * weights (B, L) of the table's dtype; positions that the bucket build left out contribute nothing.  The walk of
 * trs_scatter_rows_argmax with another term: fp32 products and sums, no atomics on values, fixed summation order, rows
 * with more than 64 lookups (32 on the any-E path) queued in `workspace` and reduced by whole waves, 256 lookups at a
 * time; the (B, L, E) block is never formed.
 * TRS_EINVAL: NULL pointer, bad size, L outside [1, 65535], B*L not a multiple of L; TRS_ESHAPE: B*L >= 2^31 - 1;
 * TRS_EDTYPE: dtype; TRS_EWORKSPACE: ws_bytes below the query.                                                         */
size_t trs_scatter_weighted_workspace_bytes(int64_t BN, int32_t E);
int trs_scatter_rows_weighted(const void* g, const void* weights, const int32_t* row_start, const int32_t* perm,
                              int64_t BN, int64_t V, int32_t E, int32_t N, int32_t dtype, int64_t padding_row,
                              void* grad_table, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* Gradient of the weights of the weighted sum:
 *   dw[b,l] = sum_e g[b,e] * table[idx[b,l], e]      (fp32, columns in order, one rounding to the table's dtype)
 * and exactly 0 where idx[b,l] == exclude_row (-1: no row is excluded) or lies outside [0, V).  g (B, E), dw (B, L) of
 * the table's dtype; one lane group (any E: one thread) per position re-reads the row, no (B, L, E) block.
 * TRS_EINVAL: NULL pointer, bad size, L outside [1, 65535], exclude_row outside [-1, V); TRS_EDTYPE: dtype / idx_dtype. */
int trs_bag_weight_grad(const void* g, const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx,
                        int32_t idx_dtype, int64_t B, int32_t L, int64_t exclude_row, void* dw, trs_stream_t stream);

/* ---- ragged bag pooling: one flat id vector plus offsets (nn.EmbeddingBag's calling form) ------------------------------
 * ids (n,) int64/int32 RAW row ids; offsets (n_off,) int64/int32 with n_off = B or B + 1.  Bag b is the positions
 * [offsets[b], end_b), end_b = offsets[b + 1] where that entry exists, else n; ids behind the last bag's end belong to no
 * bag.  live(p) := ids[p] != exclude_row (every position when exclude_row = -1), cnt[b] = the live positions of bag b,
 * w = weights (n,) of the table's dtype or NULL (= 1):
 *   mode 0 (sum):  out[b,:] = sum_live w[p] * table[ids[p], :]
 *   mode 1 (mean): out[b,:] = (sum_live table[ids[p], :]) * inv_cnt[b],  inv_cnt[b] = 1/cnt[b], 0 when cnt[b] == 0 (an
 *                  empty bag is a zero row); inv_cnt (B,) fp32 is always written in this mode and required
 *   mode 2 (max):  the maximum over the live positions, the first live position winning a tie (a later value wins only
 *                  when it is greater or NaN, the rule of trs_bag_pool_fwd); argmax (B, E) int32 = the FLAT position p of
 *                  the winner, -1 for an empty bag (a zero row): no limit on a bag's length
 * out (B, E) of the table's dtype; fp32 accumulation in list order, one rounding on store.  An excluded position issues
 * no table load and its weight is not read.  A live id outside [0, V) reads as a zero row, raises *err_flag and counts in
 * cnt.  Offsets are range-checked on the device, nothing on the host reads them: begin and end are clamped to [0, n]; an
 * offset outside [0, n], or a bag whose end lies before its begin (it is then empty), raises *err_flag; nothing is read
 * outside ids[0, n).  B == 0: TRS_OK, nothing touched.  n == 0 with B > 0: B zero rows (ids may be NULL).
 * Paths: rows that are a power-of-two number (<= 64) of whole 16-byte vectors: one lane group per bag; a bag of more than
 * trs_bag_ragged_long_len() ids is queued in `workspace` (trs_bag_ragged_workspace_bytes(B): a counter + at most B
 * entries) and reduced by ONE WAVE in a second, fixed-grid kernel whose 64/L lane groups stride the bag and fold their
 * partials in a fixed order -- the result of a bag depends on its ids and its length alone, not on the queue order.
 * Tables above 512 MiB are read with streaming loads.  Any other E: one thread per (b, e), no second tier.
 * TRS_EINVAL: NULL table / offsets / out / workspace (ids: unless n == 0), bad size, n_off not B or B + 1, exclude_row
 * outside [-1, V), weights with mode != 0, mode 2 without argmax, mode 1 without inv_cnt; TRS_ESHAPE: n or B >= 2^31 - 1;
 * TRS_EDTYPE: dtype / ids_dtype / off_dtype; TRS_EWORKSPACE: ws_bytes below the query.  All before any launch.
 * replaces F.embedding_bag(ids, table, offsets, mode=..., padding_idx=..., per_sample_weights=...,
 * include_last_offset=...) on 1-D ids.                                                                               */
int32_t trs_bag_ragged_long_len(void);
size_t trs_bag_ragged_workspace_bytes(int64_t B);
int trs_bag_pool_ragged_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids, int32_t ids_dtype,
                            int64_t n, const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int32_t mode,
                            int64_t exclude_row, const void* weights, void* out, int32_t* argmax, float* inv_cnt,
                            void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream);

/* Lookup -> sample map of ragged bags, for the gradients: bag_of[p] (n,) int32 = the last b in [0, B) with
 * offsets[b] <= p, provided p < end_b (end_b as above); -1 otherwise, which covers a position that no bag holds.  Of
 * several equal offsets (empty bags) the last, non-empty, bag owns the position.  One thread per position, a binary search
 * over the offsets; a pure function of the offsets, no atomics.  n == 0: TRS_OK.
 * Specified for offsets that do not decrease.  Where they do (trs_bag_pool_ragged_fwd raises *err_flag for such a batch)
 * every entry is still a bag in [0, B) or -1, but it need not be the bag whose clamped range the forward walked.
 * TRS_EINVAL: NULL pointer, bad size, n_off not B or B + 1; TRS_ESHAPE: n or B >= 2^31 - 1; TRS_EDTYPE: off_dtype.      */
int trs_bag_owner(const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int64_t n, int32_t* bag_of,
                  trs_stream_t stream);

/* Table gradient of ragged bags on the row buckets of ids viewed as (n, 1) (trs_csr_build_skip, B = n, N = 1, skip_row =
 * the excluded or the padding row):
 *   grad_table[r,:] = sum over the lookups p of row r with b = bag_of[p] >= 0 of term(p)
 * for EVERY r in [0,V) (rows without lookups and padding_row are written as zeros; -1: no padding row).  term(p):
 *   weights == NULL, argmax == NULL:  g[b,:]          (the mean passes g * inv_cnt[b], rounded once, on (B, E))
 *   weights (n,) of the table's dtype: weights[p] * g[b,:]
 *   argmax (B, E) int32 of trs_bag_pool_ragged_fwd:  argmax[b,e] == p ? g[b,e] : 0
 * g (B, E) of the table's dtype.  The walk of trs_scatter_rows_argmax / _weighted with the sample read from bag_of: fp32
 * sums, no atomics on values, fixed summation order, rows with more than 64 lookups (32 on the any-E path) queued in
 * `workspace` and reduced by whole waves, 256 lookups at a time; the (n, E) block is never formed.
 * TRS_EINVAL: NULL pointer, both weights and argmax, bad size; TRS_ESHAPE: n or B >= 2^31 - 1; TRS_EDTYPE: dtype;
 * TRS_EWORKSPACE: ws_bytes below the query.                                                                            */
size_t trs_scatter_ragged_workspace_bytes(int64_t n, int32_t E);
int trs_scatter_rows_ragged(const void* g, const int32_t* bag_of, const void* weights, const int32_t* argmax,
                            const int32_t* row_start, const int32_t* perm, int64_t n, int64_t B, int64_t V, int32_t E,
                            int32_t dtype, int64_t padding_row, void* grad_table, void* workspace, size_t ws_bytes,
                            trs_stream_t stream);

/* Gradient of the weights of the ragged weighted sum:
 *   dw[p] = sum_e g[bag_of[p], e] * table[ids[p], e]      (fp32, columns in order, one rounding to the table's dtype)
 * and exactly 0 where ids[p] == exclude_row (-1: none), lies outside [0, V), or bag_of[p] < 0.  g (B, E), dw (n,) of the
 * table's dtype.  n == 0: TRS_OK.
 * TRS_EINVAL: NULL pointer, bad size, exclude_row outside [-1, V); TRS_ESHAPE: n >= 2^31 - 1; TRS_EDTYPE: dtype /
 * ids_dtype.                                                                                                          */
int trs_bag_weight_grad_ragged(const void* g, const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids,
                               int32_t ids_dtype, int64_t n, const int32_t* bag_of, int64_t exclude_row, void* dw,
                               trs_stream_t stream);

/* ---- ragged bag pooling over F fields of one table (the "keyed jagged" layout) -----------------------------------------
 * One table of V = sum(field sizes) rows; field_offsets (F + 1,) int64 ON THE DEVICE is the exclusive prefix sum of the
 * field sizes: field f owns the rows [field_offsets[f], field_offsets[f + 1]).  values (n,) int64/int32 RAW per-field ids;
 * offsets (n_off,) int64/int32 with n_off = F*B + 1, FIELD-MAJOR: bag j = f*B + b is the positions
 * [offsets[j], offsets[j + 1]); positions behind offsets[F*B] belong to no bag.  w = weights (n,) of the table's dtype or
 * NULL (= 1), cnt = the bag's length:
 *   out[b, f, :] = pool over bag f*B + b of w[p] * table[values[p] + field_offsets[f], :]
 * out (B, F, E) of the table's dtype, sample-major and contiguous: bag j is OUT ROW b*F + f.  mode 0 (sum), 1 (mean over
 * the bag's own length, an empty bag a zero row; inv_cnt (B*F,) fp32 = 1/cnt, 0 when empty, always written and required),
 * 2 (max, the first position winning a tie, the rule of trs_bag_pool_fwd; argmax (B*F, E) int32 = the FLAT position of the
 * winner, -1 for an empty bag).  argmax and inv_cnt are indexed by OUT ROW, as out is.  fp32 accumulation in list order,
 * one rounding on store: the walk, the two tiers (a bag of more than trs_bag_ragged_long_len() ids is queued in
 * `workspace`, trs_bag_fields_workspace_bytes(F*B) bytes, and reduced by one wave), the streaming loads above 512 MiB and
 * the any-E path of trs_bag_pool_ragged_fwd, so a bag's result is bit-equal to that entry's on the field's table slice.
 * An id is checked against ITS OWN field: values[p] < 0 or >= the field's size reads as a zero row, raises *err_flag and
 * counts in cnt; it never reads another field's row.  A field that does not lie inside [0, V) (bad field_offsets) has size
 * 0.  Offsets are range-checked on the device as trs_bag_pool_ragged_fwd does: clamped to [0, n]; an offset outside it or
 * a decreasing pair (that bag is empty) raises *err_flag.  There is no padding id and no excluded row.
 * B == 0: TRS_OK, nothing touched.  n == 0 with B > 0: B*F zero rows (values may be NULL).
 * TRS_EINVAL: NULL table / offsets / out / workspace / field_offsets (values: unless n == 0), F < 1, bad size, n_off not
 * F*B + 1, weights with mode != 0, mode 2 without argmax, mode 1 without inv_cnt; TRS_ESHAPE: n or F*B >= 2^31 - 1;
 * TRS_EDTYPE: dtype / val_dtype / off_dtype; TRS_EWORKSPACE: ws_bytes below the query.  All before any launch.
 * replaces F calls of F.embedding_bag(values_f, table_f, offsets_f, ..., include_last_offset=True) and the cat.       */
size_t trs_bag_fields_workspace_bytes(int64_t FB);
int trs_bag_pool_fields_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* values, int32_t val_dtype,
                            int64_t n, const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int32_t F,
                            const int64_t* field_offsets, int32_t mode, const void* weights, void* out, int32_t* argmax,
                            float* inv_cnt, void* workspace, size_t ws_bytes, int32_t* err_flag, trs_stream_t stream);

/* Lookup -> out row and table row map of the F-field bags, for the gradients.  With j = the owner of position p among the
 * F*B bags by the rule of trs_bag_owner (the last j with offsets[j] <= p, provided p < offsets[j + 1]), f = j / B,
 * b = j - f*B:
 *   out_row_of[p] (n,) int32 = b*F + f,                        -1 where no bag holds p
 *   rows[p]       (n,) int64 = values[p] + field_offsets[f],   -1 where no bag holds p or the id lies outside its field
 * (V = the table's rows: a field that does not lie inside [0, V) has size 0, as in the forward)
 * so that trs_csr_build on rows viewed as (n, 1), trs_scatter_rows_ragged (bag_of = out_row_of, B := B*F, g (B*F, E)) and
 * trs_bag_weight_grad_ragged (ids = rows, exclude_row = -1) are the gradients of trs_bag_pool_fields_fwd.  One thread per
 * position, a binary search over the offsets; a pure function of its inputs, no atomics.  n == 0: TRS_OK.
 * Specified for offsets that do not decrease.  Where they do, every out_row_of entry is still an out row in [0, B*F) or
 * -1 and every rows entry a row of the owner's field or -1, but the owner need not be the bag whose clamped range the
 * forward walked.
 * TRS_EINVAL: NULL pointer, F < 1, bad size, n_off not F*B + 1; TRS_ESHAPE: n or F*B >= 2^31 - 1; TRS_EDTYPE: val_dtype /
 * off_dtype.                                                                                                            */
int trs_bag_owner_fields(const void* values, int32_t val_dtype, int64_t n, const void* offsets, int32_t off_dtype,
                         int64_t n_off, int64_t B, int32_t F, int64_t V, const int64_t* field_offsets,
                         int32_t* out_row_of, int64_t* rows, trs_stream_t stream);

/* ---- K2: FM layer on a materialised block -------------------------------------------------
 * fwd: fm[b,:] = 0.5*((sum_n x)^2 - sum_n x^2), fm_sum[b,:] = sum_n x (fp32, optional)
 * bwd: dx[b,n,:] = g[b,:] * (fm_sum[b,:] - x[b,n,:])
 * layers/ctr/factorization_machine.py:62-73.                                                  */
int trs_fm_fwd(const void* x, int64_t B, int32_t N, int32_t E, int32_t dtype, void* fm, float* fm_sum,
               trs_stream_t stream);
int trs_fm_bwd(const void* x, const void* g, const float* fm_sum, int64_t B, int32_t N, int32_t E,
               int32_t dtype, void* dx, trs_stream_t stream);

/* ---- K7: inner-product network ------------------------------------------------------------
 * fwd: out[b,p(i,j)] = sum_e x[b,i,e]*x[b,j,e], i<j lexicographic, P = N(N-1)/2
 * bwd: dx[b,i,:] = sum_{j!=i} g[b,p(min,max)] * x[b,j,:]
 * layers/ctr/inner_product_network.py:68-74.                                                  */
int trs_pair_dot_fwd(const void* x, int64_t B, int32_t N, int32_t E, int32_t dtype, void* out,
                     trs_stream_t stream);
int trs_pair_dot_bwd(const void* x, const void* g, int64_t B, int32_t N, int32_t E, int32_t dtype,
                     void* dx, trs_stream_t stream);

/* K7 fused with K1: out[b,p(i,j)] = <row(b,i), row(b,j)> with row(b,n) = table[idx[b,n]+offsets[n], :] read straight from
 * the embedding table (one wave per sample; an out-of-range id reads as a zero row and sets *err_flag); emb (optional,
 * may be NULL): the looked-up (B,N,E) block, written on the way for the backward / other consumers.  bf16 tables whose
 * rows the matrix-core path covers (E % 32 == 0, E <= 128, N <= 64); TRS_ESHAPE otherwise (callers then use
 * trs_gather_rows + trs_pair_dot_fwd).  Replaces multi_indices_emb.py:104-105 + inner_product_network.py:68-74.   */
int trs_embed_pair_dot(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                       const int64_t* offsets, int64_t B, int32_t N, void* emb, void* out, int32_t* err_flag,
                       trs_stream_t stream);

/* ---- K3: field-aware FM pair products -----------------------------------------------------
 * fwd: out[b,p(i,j),:] = x[b,i*N+j,:] * x[b,j*N+i,:], i<j      x: (B, N*N, E)
 * bwd: dx[b,i*N+j,:] = g[b,p,:]*x[b,j*N+i,:]; dx[b,j*N+i,:] = g[b,p,:]*x[b,i*N+j,:]; diagonal 0
 * layers/ctr/field_aware_factorization_machine.py:69-87.
 * trs_ffm_fused_fwd gathers straight from the N tables (never materialises (B,N*N,E)):
 *   out[b,p(i,j),:] = tables[i][g_j,:] * tables[j][g_i,:],  g_n = idx[b,n]+offsets[n].       */
int trs_ffm_fwd(const void* x, int64_t B, int32_t N, int32_t E, int32_t dtype, void* out,
                trs_stream_t stream);
int trs_ffm_bwd(const void* x, const void* g, int64_t B, int32_t N, int32_t E, int32_t dtype,
                void* dx, trs_stream_t stream);
int trs_ffm_fused_fwd(const void* const* tables, int64_t V, int32_t E, int32_t dtype,
                      const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N,
                      void* out, int32_t* err_flag, trs_stream_t stream);
/* dense gradients of the N tables of trs_ffm_fused_fwd (row_start/perm from trs_csr_build on the same
 * indices): grad_tables[i][r,:] = sum_{(b,j) in row r, j != i} gout[b,p(i,j),:] * tables[j][g_i,:].
 * row_ids_t (optional, may be NULL): the global row ids g_n = idx[b,n]+offsets[n] TRANSPOSED, (N, B) int32 -- the walk
 * of table i then finds the g_i of its lookups in one 4 B-per-sample column (256 KB at B = 65 536: cache-resident)
 * instead of one random 8-byte load per lookup from the (B, N) matrix.                                          */
int trs_ffm_fused_bwd(const void* const* tables, int64_t V, int32_t E, int32_t dtype, const void* idx,
                      int32_t idx_dtype, const int64_t* offsets, const void* gout,
                      const int32_t* row_start, const int32_t* perm, int64_t B, int32_t N,
                      void* const* grad_tables, const int32_t* row_ids_t, trs_stream_t stream);

/* ---- K4: cross network ----------------------------------------------------------------------
 * x_{l+1} = x0 * (x_l W_l^T + b_l) + x0, l = 0..L-1, rows = B*N vectors of length E.
 * W: (L,E,E) row-major [l][out][in] as nn.Linear.weight; b: (L,E).
 * bwd with detach_first=1 reproduces cross_network.py:65 (x_0 enters layer 0's linear map
 * detached); detach_first=0 gives the textbook gradient.
 *   dx (rows,E), dW (L,E,E) fp32, db (L,E) fp32 (dW/db are ACCUMULATED into: zero them first).
 * workspace (trs_cross_workspace_bytes; may be 0 / NULL for fp32) holds the W fragments re-packed for
 * the MFMA path (bf16, E % 32 == 0, E <= 128); without it the generic VALU kernels run.
 * layers/ctr/cross_network.py:65-79.                                                          */
size_t trs_cross_workspace_bytes(int64_t rows, int32_t E, int32_t L, int32_t dtype);
int trs_cross_fwd(const void* x, const void* W, const void* b, int64_t rows, int32_t E, int32_t L,
                  int32_t dtype, void* out, void* workspace, size_t ws_bytes, trs_stream_t stream);
int trs_cross_bwd(const void* x, const void* W, const void* b, const void* g, int64_t rows, int32_t E,
                  int32_t L, int32_t dtype, int32_t detach_first, void* dx, float* dW, float* db,
                  void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- K5/K6: compress interaction network, one layer ------------------------------------------
 * y[b,c,e] = bias[c] + sum_{n,h} Wc[c, n*H+h] * x0[b,n,e] * xk[b,h,e]
 *   x0: (B,N,E) the embedding block; xk: (B,H,E) previous hidden ((B,N,E) for layer 0);
 *   Wc: (C, N*H) = nn.Conv1d(N*H, C, 1).weight squeezed; bias (C) or NULL; y: (B,C,E).
 * The outer product Z[b,(n,h),e] is formed on the fly (never written to memory).
 * stats (2*C fp32, optional): per-channel sum and sum of squares of y over (B,E), accumulated
 * (zero first) -- the BatchNorm1d batch statistics.
 * bwd: given gy (B,C,E): dWc (C,N*H) fp32 accumulated, dx0 (B,N,E) and dxk (B,H,E) written.
 * layers/ctr/compress_interaction_network.py:125-137.                                          */
int trs_cin_fwd(const void* x0, const void* xk, const void* Wc, const void* bias, int64_t B, int32_t N,
                int32_t H, int32_t C, int32_t E, int32_t dtype, void* y, float* stats,
                trs_stream_t stream);
int trs_cin_bwd(const void* x0, const void* xk, const void* Wc, const void* gy, int64_t B, int32_t N,
                int32_t H, int32_t C, int32_t E, int32_t dtype, float* dWc, void* dx0, void* dxk,
                int32_t accumulate_dx0, trs_stream_t stream);

/* ---- K5 on the matrix cores: channels-last CIN contraction (bf16) ------------------------------
 * Same contraction as trs_cin_fwd with activations stored channels-last:
 *   x0T (B,E,ld0): x0T[b,e,n] = x0[b,n,e], row stride ld0 (multiple of 8, zero-filled past N)
 *   xkT rows = B*E pixels of stride ldk (multiple of 8, >= 32*ceil(H/32), zero-filled past H):
 *       xkT[b*E+e, h] = xk[b,h,e]   (a strided view of the previous layer's yT is fine)
 *   yT  (B,E,C): yT[b,e,c] = y[b,c,e]
 * Requirements: C % 32 == 0, E % 16 == 0, H <= 256.  workspace: trs_cin_cl_workspace_bytes.
 * The x0[n] factor multiplies the MFMA result, so the outer product never exists even in registers.
 * tri != 0 (needs xkT == x0T, ldk == ld0, N == H): the caller states that Wc[c, n*H + h] == 0 for every h > n -- the form the first
 * layer's weights take once W[n,h] + W[h,n] is folded onto h <= n, which is exact there because xk IS x0 and
 * the products x0[n]*x0[h] are symmetric -- and the k-steps that only hold such zeros are skipped.
 * layers/ctr/compress_interaction_network.py:125-137.                                          */
size_t trs_cin_cl_workspace_bytes(int32_t N, int32_t H, int32_t C);
int trs_cin_cl_fwd(const void* x0T, int32_t ld0, const void* xkT, int32_t ldk, const void* Wc,
                   const void* bias, int64_t B, int32_t N, int32_t H, int32_t C, int32_t E, int32_t dtype,
                   int32_t tri, void* yT, void* workspace, size_t ws_bytes, trs_stream_t stream);
/* data gradients of the same contraction, channels-last: given gyT (B,E,>=C) with ldg channels between two pixels
 * (ldg >= C, ldg % 8 == 0) and Wc = the first C rows of the layer's weight, C = the channels contracted over:
 *   dx0T (B,E,ld0)  : dx0T[b,e,n] = sum_{c,h} gy*Wc*xk   (zeros past N)
 *   dxkT rows of stride ldo (>= 32*ceil(H/32)): dxkT[b*E+e,h] = sum_{c,n} gy*Wc*x0
 * Requirements: C in {32,64,128,256}, E % 16 == 0.  bias gradient = sum of gy over (b,e) (caller).
 * ldg > C serves a layer whose output channels beyond the first C receive NO gradient: the reference splits EVERY CIN
 * layer's 2H output channels into a "direct" and a "hidden" half (compress_interaction_network.py:151-156: the
 * `i != len-1` guard is always true) and never uses the LAST layer's hidden half (:176-181 reads the direct halves only),
 * so dL/dy of those channels is exactly zero -- through BatchNorm and the activation too, which act per channel.  Their
 * terms of the contraction over c are zeros that need not be computed: the results are identical to ldg == C on the full
 * tensors.
 * tri: as in trs_cin_cl_fwd; xkT is x0T there, so the two gradients belong to the same values: dx0T receives
 * their SUM (added in fp32, rounded once) and dxkT is not written (may be NULL).                        */
size_t trs_cin_cl_bwd_data_workspace_bytes(int32_t N, int32_t H, int32_t C);
int trs_cin_cl_bwd_data(const void* x0T, int32_t ld0, const void* xkT, int32_t ldk, const void* gyT, int32_t ldg,
                        const void* Wc, int64_t B, int32_t N, int32_t H, int32_t C, int32_t E, int32_t dtype,
                        int32_t tri, void* dx0T, void* dxkT, int32_t ldo, void* workspace, size_t ws_bytes,
                        trs_stream_t stream);

/* weight gradient of the same contraction on the matrix cores; CHANNELS-FIRST operands (the sum runs over
 * pixels, which must be the contiguous axis): gy (B,>=C,E) with gy_batch_stride elements between two samples
 * (>= C*E, a multiple of 8, < 2^31), x0 (B,N,E), xk (B,H,E) bf16;
 * dW (C, N*H) fp32 is ACCUMULATED into (zero it first).  C in {64,128,256}, E in {32,64,128}.
 * gy_batch_stride > C*E: the layer's channels beyond the first C receive no gradient (see trs_cin_cl_bwd_data); dW is
 * then the first C rows of the gradient and the caller zero-fills the rest.
 * tri != 0 (needs xk == x0, N == H, gy_batch_stride == C*E): the first layer, where dW[c,n,h] is symmetric in (n,h) --
 * only the 16-h blocks at or below the diagonal are computed and the rest is mirrored; the result is the same full
 * (C, N*H) gradient of the UNFOLDED weights.                                                          */
size_t trs_cin_dw_workspace_bytes(int64_t B, int32_t N, int32_t H, int32_t C);
int trs_cin_dw(const void* gy, int64_t gy_batch_stride, const void* x0, const void* xk, int64_t B, int32_t N, int32_t H,
               int32_t C, int32_t E, int32_t dtype, int32_t tri, float* dW, void* workspace, size_t ws_bytes,
               trs_stream_t stream);

/* ---- MLP backward epilogue (the GEMMs stay on hipBLASLt) -----------------------------------------------
 * y = relu(linear(x)):  gz = gy * (y > 0) and gb[c] = sum_r gz[r,c] (fp32) in ONE pass over (rows, C) instead of
 * ATen's threshold_backward + column sum.  C*sizeof(T) must be a multiple of 16 and <= 4096.
 * layers/ctr/multilayer_perceptron.py:53-61 (Linear_i / Activation_i pairs).                                 */
size_t trs_relu_bwd_bias_workspace_bytes(int64_t rows, int32_t C);
int trs_relu_bwd_bias(const void* gy, const void* y, int64_t rows, int32_t C, int32_t dtype, void* gz,
                      float* gb, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- per-field MLP of DeepAndCrossNetwork as one kernel per direction -------------------------
 * models/ctr/deep_and_cross_network.py:71-87 applies MultilayerPerceptionLayer (layers/ctr/multilayer_perceptron.py:
 * 53-84: Linear -> ReLU ... -> Linear) to every (sample, field) row of the (B,N,E) block.  bf16 only.
 *   widths[0..num_layers]: in_features of layer 0, then out_features of every layer (multiples of 8, <= 512);
 *   weights[l]: (widths[l+1], widths[l]) row-major = nn.Linear.weight; biases[l]: (widths[l+1]); host arrays of
 *   device pointers.  ReLU after every layer but the last.
 * fwd: hidden[l] (rows, pad32(widths[l+1])) for l < num_layers-1 = the ReLU outputs, zero in the padding columns
 *      (kept for the weight-gradient GEMMs); masks[l]: trs_mlp_fused_mask_bytes(rows) bytes, the sign bits
 *      [hidden > 0] in the kernel's own (pass, lane) order -- opaque, read only by trs_mlp_fused_bwd_data on the same
 *      rows and widths; y (rows, widths[num_layers]).
 * bwd_data: gy (rows, widths[num_layers]) -> gz[l] (rows, pad32(widths[l+1])), l < num_layers-1 = gradient w.r.t. the
 *      pre-activation of layer l (that of the last layer is gy itself); gbias[l] (pad32(widths[l+1]) fp32, written) for
 *      every layer; gx (rows, widths[0]).  Weight gradients are left to the caller: dW_l = gz_l^T @ input_l.
 * A stack fed by the ReLU output of a layer in front of it (the hipBLASLt first layer of a deep branch): mask_in
 *      (trs_mlp_fused_mask_bytes(rows) bytes, may be NULL) receives the sign bits [x > 0] in the forward; given to the
 *      backward together with gbias_in (pad32(widths[0]) fp32, written), gx becomes the gradient w.r.t. that layer's
 *      pre-activation, gx * [x > 0], and gbias_in its column sums = that layer's bias gradient (needs num_layers <= 7).
 * trs_mlp_fused_supported: 1 when the widths fit the kernel (and its LDS budget).                              */
int trs_mlp_fused_supported(int32_t num_layers, const int32_t* widths);
/* Kernel families.  The two stack shapes of the models (64-400-400-400-64 on B*N rows; 416-400-400-8 behind a wide first
 * layer) have a second pair of kernels (csrc/mlp_ro.hpp: a wave owns 64 / 32 rows for the whole stack) behind the same
 * two entry points, and the two families lay the sign bits out differently.  Which family runs is a PER-CALL argument --
 * the library keeps no mode:
 *   trs_mlp_fused_fwd(family = AUTO | TILE | ROW_OWNER | MIXED); AUTO = ROW_OWNER for the covered shapes from 131 072
 *   rows on, MIXED for them from 32 768 rows on, TILE otherwise;
 *   trs_mlp_fused_family(num_layers, widths, rows, request) -> the family (TILE, ROW_OWNER or MIXED) that request runs, 0
 *   when it cannot be met (ROW_OWNER on an uncovered shape; the forward then returns TRS_EINVAL).  A pure function.
 *   trs_mlp_fused_bwd_data(family) must be given THAT value (TILE, ROW_OWNER or MIXED; AUTO is TRS_EINVAL): the caller records
 *   what its forward ran, so a policy or size threshold cannot come between a forward and its backward.              */
#define TRS_MLP_FAMILY_AUTO 0
#define TRS_MLP_FAMILY_TILE 1
#define TRS_MLP_FAMILY_ROW_OWNER 2
#define TRS_MLP_FAMILY_MIXED 3      /* row-owner forward, tile backward reading the row-owner sign-bit layout (covered
                                       shapes below 131 072 rows: each direction on the family that is faster there) */
/* Workspace: both entry points (and trs_rows_gemm) first copy the weights into MFMA fragment order in the workspace,
 * then run.                                                                                                          */
/* x_stride (trs_mlp_fused_fwd): elements between consecutive rows of x; 0 = widths[0].  A larger stride (a multiple of 8)
 * makes the stack read the first widths[0] columns of wider rows -- the 416-wide tail of a deep branch on the 512-wide
 * output of the library GEMM in front of it; row-owner and mixed family only (TRS_ESHAPE otherwise).  The matching
 * backward may then be called with widths[0] = that stride under TRS_MLP_FAMILY_MIXED: it computes the gradient of all
 * x_stride columns (those past the forward's width meet zero weights and come out as zeros).                       */
int32_t trs_mlp_fused_family(int32_t num_layers, const int32_t* widths, int64_t rows, int32_t request);
size_t trs_mlp_fused_workspace_bytes(int32_t num_layers, const int32_t* widths);
size_t trs_mlp_fused_mask_bytes(int64_t rows);
int trs_mlp_fused_fwd(const void* x, int64_t rows, int32_t num_layers, const int32_t* widths,
                      const void* const* weights, const void* const* biases, void* const* hidden, void* const* masks,
                      void* mask_in, void* y, int32_t dtype, int32_t family, int32_t x_stride, void* workspace,
                      size_t ws_bytes, trs_stream_t stream);
int trs_mlp_fused_bwd_data(const void* gy, int64_t rows, int32_t num_layers, const int32_t* widths,
                           const void* const* weights, const void* const* masks, void* const* gz, float* const* gbias,
                           void* gx, const void* mask_in, float* gbias_in, int32_t dtype, int32_t family,
                           void* workspace, size_t ws_bytes, trs_stream_t stream);
/* The same backward carrying the OUTPUT layer's weight gradient (a deep branch's 400 -> 1 logit layer: a product of its
 * own is two dependent launches for one read of the last hidden activation, which this kernel can stream beside its
 * GEMMs while the gy tile it needs lies in LDS).  Tile kernel only (family TILE or MIXED), bf16, num_layers >= 2.
 *   live: the real output columns, 1 <= live <= 3 and <= widths[num_layers] (the layer may run padded to 8 columns);
 *   gy_stride: widths[num_layers] -- gy as trs_mlp_fused_bwd_data takes it -- or, for live < 8, live: gy is then the
 *     contiguous (rows, live) gradient of the live columns alone, read by elements where it lies (no padded copy);
 *   h_last: (rows, h_stride) the last hidden activation (hidden[num_layers-2] of the forward), h_stride % 8 == 0 and
 *     >= pad32(widths[num_layers-1]), 16-byte aligned;
 *   wl_part: caller-owned fp32 scratch of trs_mlp_fused_bwd_wlast_part_bytes bytes, [workgroup][live][pad32(widths[
 *     num_layers-1])] partial rows, written; gw_last: (live, pad32(widths[num_layers-1])) fp32, written: row j =
 *     sum over rows of gy[row][j] * h_last[row], summed in a fixed order (no atomics) by the entry's own reduce launch.
 * Everything else as trs_mlp_fused_bwd_data, bit for bit.  trs_mlp_fused_bwd_wlast_part_bytes returns 0 where the
 * kernel does not carry it (fp32, the row-owner family, num_layers < 2, live outside 1..3, num_layers + 1 + live > 8
 * reduce entries, or 128 * act_stride + 16 KB + (num_layers + 1 + live) * 2 KB of LDS above 160 KB): the caller keeps
 * trs_mlp_fused_bwd_data and trs_wgrad_rows.  The entry returns TRS_ESHAPE for such a call, TRS_EWORKSPACE for a
 * wl_part_bytes below the query's answer, before anything is launched.                                                */
size_t trs_mlp_fused_bwd_wlast_part_bytes(int32_t num_layers, const int32_t* widths, int64_t rows, int32_t dtype,
                                          int32_t family, int32_t live);
int trs_mlp_fused_bwd_data_wlast(const void* gy, int32_t gy_stride, int64_t rows, int32_t num_layers,
                                 const int32_t* widths, const void* const* weights, const void* const* masks,
                                 void* const* gz, float* const* gbias, void* gx, const void* mask_in, float* gbias_in,
                                 const void* h_last, int32_t h_stride, int32_t live, float* wl_part,
                                 size_t wl_part_bytes, float* gw_last, int32_t dtype, int32_t family, void* workspace,
                                 size_t ws_bytes, trs_stream_t stream);
/* The tile backward WITHOUT its reduce launch (TILE and MIXED families, rows > 0).  Operands as the entry above; h_last =
 * NULL: the output layer's dW is not carried (live / wl_part unused, gy_stride = widths[L]).  Instead of gbias, gbias_in
 * and gw_last the call reports where the per-workgroup partial rows lie, in ``workspace`` and ``wl_part``:
 * part_out / stride_out [num_layers + 4] and *nparts_out -- set l < L: layer l's bias gradient (pad32(widths[l+1])
 * columns); set L: the input's column sums (with mask_in, else NULL); set L + 1 + j: row j of the output layer's dW
 * (pad32(widths[L-1]) columns, NULL from ``live`` on).  Column c of a set is the sum over p < nparts of
 * part[p * stride + c]; trs_wgrad_finish / trs_wgrad_finish_t with gb_nparts (or trs_colsum_parts_reduce) take that
 * sum in the reduce launch's order.  Both buffers must stay allocated until that consumer is enqueued on the stream. */
int trs_mlp_fused_bwd_data_parts(const void* gy, int32_t gy_stride, int64_t rows, int32_t num_layers,
                                 const int32_t* widths, const void* const* weights, const void* const* masks,
                                 void* const* gz, void* gx, const void* mask_in, const void* h_last, int32_t h_stride,
                                 int32_t live, float* wl_part, size_t wl_part_bytes, const float** part_out, int32_t* stride_out, int32_t* nparts_out, int32_t dtype,
                                 int32_t family, void* workspace, size_t ws_bytes, trs_stream_t stream);
/* out[k][c] = sum of set k's partials for c < n[k] (1 .. 8 sets of ``nparts`` rows): the reduce launch on its own, for a
 * caller of the entry above that has no batched finish to fold the sets in                                            */
int trs_colsum_parts_reduce(int32_t n_sets, const float* const* part, const int32_t* stride, const int32_t* n,
                            int32_t nparts, float* const* out, trs_stream_t stream);

/* dst (rows, c_out) = [src (rows, c_in) | zeros], bf16: the gradient of the first c_in columns of a padded output (the
 * logit column of a deep branch whose last layer runs at 8 columns) in one launch.                                   */
int trs_pad_cols(const void* src, int32_t c_in, void* dst, int32_t c_out, int64_t rows, int32_t dtype,
                 trs_stream_t stream);

/* ---- one wide layer with a short contraction: the input gradient of a deep branch's first Linear ----------------
 * y (rows, in_f) = x[:, :out_f] @ W, x (rows, x_stride) and W (out_f, in_f) = nn.Linear(in_f, out_f).weight, bf16:
 * dL/d(input) of that layer from dL/d(pre-activation) (multilayer_perceptron.py:53-61 under autograd).  out_f <= 512
 * (a 128-row tile of x stays in LDS), in_f % 8 == 0, x_stride % 8 == 0 and >= out_f rounded up to 32 (the columns
 * past out_f meet zero weight rows).  workspace: trs_rows_gemm_workspace_bytes (fragment-order copy of W).          */
size_t trs_rows_gemm_workspace_bytes(int32_t out_f, int32_t in_f);
int trs_rows_gemm_supported(int32_t out_f, int32_t in_f, int32_t x_stride);
int trs_rows_gemm(const void* x, int64_t rows, int32_t x_stride, const void* W, int32_t out_f, int32_t in_f,
                  int32_t dtype, void* y, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- row-sharded tables (multi-GPU lookup) -----------------------------
 * Bucket the B*N global row ids of the local batch by owner rank (owner = id / rows_per_rank):
 *   counts[w]  = number of ids owned by rank w                                  (W int64)
 *   send_ids   = LOCAL row ids (id - owner*rows_per_rank) grouped by owner      (B*N int32)
 *   send_pos   = for each grouped slot k the original flat position p = b*N+n   (B*N int32)
 *   inv_pos    = inverse permutation, inv_pos[p] = k (may be NULL)              (B*N int32)
 * Order inside one owner's group is unspecified.  workspace from trs_bucket_workspace_bytes. */
size_t trs_bucket_workspace_bytes(int64_t BN, int32_t world);
int trs_bucket_by_owner(const void* idx, int32_t idx_dtype, const int64_t* offsets, int64_t B, int32_t N,
                        int64_t rows_per_rank, int32_t world, int64_t* counts, int32_t* send_ids,
                        int32_t* send_pos, int32_t* inv_pos, void* workspace, size_t ws_bytes,
                        trs_stream_t stream);
/* Un-permute of the sharded lookup (step 5 of torecsys_amd/dist.py's forward) with the lookups this rank owns ITSELF read
 * straight from its shard: slot s = inv_pos[p]; s in [self_lo, self_lo + self_n) -> row local[send_ids[s]] (ids outside
 * [0, n_valid) read as zero rows and raise err_flag); every other slot -> back[s - (s >= self_lo + self_n ? self_n : 0)]
 * (the received rows are stored WITHOUT the self segment: back_rows of them).  Writes emb (B,N,E), and -- optional, as
 * trs_embed_fm -- the FM second-order term fm (B,E) and the fp32 field sums fm_sum (B,E).  New: the reference has no
 * distributed code. */
int trs_embed_fm_sharded(const void* back, int64_t back_rows, const void* local, int64_t local_rows, int64_t n_valid,
                         int32_t E, int32_t dtype, const int32_t* inv_pos, const int32_t* send_ids, int32_t self_lo,
                         int32_t self_n, int64_t B, int32_t N, void* emb, void* fm, float* fm_sum, int32_t* err_flag,
                         trs_stream_t stream);
/* out[k,:] = g_block[pos[k],:] + g_fm[b,:]*(fm_sum[b,:] - x[pos[k],:]), b = pos[k]/N: the block gradient (and
 * the FM second-order backward when the FM term was fused into the sharded lookup) in exchange order, one pass.
 * g_block or the (g_fm, fm_sum, x) triple may be NULL.  pos[k] < 0 marks a padding slot of a fixed-capacity
 * exchange: its row is written as zeros.                                                                      */
int trs_permute_grad(const void* g_block, const void* g_fm, const float* fm_sum, const void* x,
                     const int32_t* pos, int64_t K, int32_t N, int32_t E, int32_t dtype, void* out,
                     trs_stream_t stream);

/* ---- bag pooling over a row-sharded table (dist.RowShardedListIndicesEmbedding; csrc/bag_shard.hip) ---------------
 * Sum / mean pooling is linear: every owner pools the rows it holds for each (source rank, sample) into one fp32 partial
 * row and only those rows travel.  New: the reference has no distributed code.
 *
 * Route, on the sender.  idx (B, L) global row ids, owner = id / rows_per_rank (rows_per_rank * world >= V):
 *   counts (world, B) int32    counts[w, b] = lookups of sample b that rank w owns
 *   send_ids (n_send int32)    LOCAL ids (id - owner * rows_per_rank) grouped by owner, then by sample, then in list order:
 *                              segment (w, b) = send_ids[seg_start[w*B + b] .. seg_start[w*B + b + 1]), seg_start
 *                              (world*B + 1 int32) the exclusive scan of counts in that (owner-major) order, n_send its
 *                              last entry.  The layout is a pure function of idx: no atomics place a value.
 * An id outside [0, V) is not sent (no count, no slot) and raises *err_flag (trs_bag_route_count only; may be NULL).
 * A slot at or past the end of its segment or past n_send is never written (a seg_start that is not the scan of the counts).
 * One wave per sample, 64 list positions at a time; the place of a lookup in its segment is ballot + popcount per owner.
 * Limits: 1 <= world <= 64, 1 <= L <= 65535, B*L < 2^31, else TRS_ESHAPE.  B == 0 (and, for place, n_send == 0) returns
 * TRS_OK and touches nothing.  NULL pointer TRS_EINVAL, bad idx dtype TRS_EDTYPE, all before any launch.               */
int trs_bag_route_count(const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t V, int64_t rows_per_rank,
                        int32_t world, int32_t* counts, int32_t* err_flag, trs_stream_t stream);
int trs_bag_route_place(const void* idx, int32_t idx_dtype, int64_t B, int32_t L, int64_t V, int64_t rows_per_rank,
                        int32_t world, const int32_t* seg_start, int32_t* send_ids, int64_t n_send, trs_stream_t stream);
/* Owner: out[s, :] (S, E) fp32 = the sum, in list order and in fp32, of the shard rows ids[seg_start[s] .. seg_start[s+1])
 * (ids: n int32 local row ids; seg_start: S + 1 int32, clipped to [0, n]).  An empty segment gives a zero row; an id
 * outside [0, n_valid) reads as a zero row and raises *err_flag (may be NULL).  shard (rows, E) fp32 or bf16.  Rows that
 * are a power-of-two number (<= 64) of whole 16-byte vectors take the lane-group path of trs_bag_pool_fwd; any other E
 * one thread per (s, e).  S == 0 returns TRS_OK and touches nothing (n == 0 with S > 0 writes S zero rows).
 * NULL pointer TRS_EINVAL, bad dtype TRS_EDTYPE, n >= 2^31 TRS_ESHAPE, all before any launch.                            */
int trs_bag_pool_segments(const void* shard, int64_t n_valid, int32_t E, int32_t dtype, const int32_t* ids, int64_t n,
                          const int32_t* seg_start, int64_t S, float* out, int32_t* err_flag, trs_stream_t stream);
/* out[b, e] = round_to_dtype( (parts[0, b, e] + parts[1, b, e] + ... + parts[P-1, b, e]) * scale ), parts (P, B, E) fp32,
 * p ascending, fp32 sum, exactly one rounding; scale = 1.f / (float)L for the mean (the expression of trs_bag_pool_fwd).
 * B == 0 returns TRS_OK and touches nothing.  NULL pointer / P < 1 TRS_EINVAL, bad dtype TRS_EDTYPE.                     */
int trs_bag_combine(const float* parts, int32_t P, int64_t B, int32_t E, float scale, int32_t dtype, void* out,
                    trs_stream_t stream);
/* Backward on the owner: g_all (S, E) of `dtype`, one output-gradient row per segment (same ids / seg_start as
 * trs_bag_pool_segments).  For every lookup q of segment s: grad_rows[q, :] (n, E) = g_all[s, :] and ids_bwd[q] = ids[q];
 * a lookup of pad_local_row (-1: none) or of an id outside [0, n_valid) -- which read as a zero row in the forward -- gets
 * a zero row and ids_bwd[q] = -1 (trs_csr_build_skip / the unchecked bucket build leave -1 out of the index), and so do
 * the slots q in [seg_start[S], n) behind the last segment (the room a one-rank sender keeps for ids it did not send).
 * S == 0 or n == 0 returns TRS_OK and touches nothing.  NULL pointer TRS_EINVAL, bad dtype TRS_EDTYPE.                  */
int trs_bag_expand_grad(const void* g_all, int32_t dtype, int32_t E, const int32_t* ids, int64_t n,
                        const int32_t* seg_start, int64_t S, int64_t n_valid, int64_t pad_local_row, void* grad_rows,
                        int32_t* ids_bwd, trs_stream_t stream);

/* ---- Linear with one output unit (the logit layer of the DeepFM / xDeepFM MLP, multilayer_perceptron.py:51) -------
 * out[r] = h[r,:] . w + bias[0]: a row-wise dot product, not a GEMM.  h (rows, C), w (C); C * sizeof(T) / 16 must be
 * a power of two <= 64.  bwd: gh (rows, C) = g[r] * w (may be NULL); gw (C), gb (1) fp32, written (both or neither). */
int trs_rowdot_fwd(const void* h, const void* w, const void* bias, int64_t rows, int32_t C, int32_t dtype, void* out,
                   trs_stream_t stream);
size_t trs_rowdot_bwd_workspace_bytes(int64_t rows, int32_t C);
int trs_rowdot_bwd(const void* g, const void* h, const void* w, int64_t rows, int32_t C, int32_t dtype, void* gh,
                   float* gw, float* gb, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- batched 2-D transposition with zero padding (the channels-last entry of the CIN layer) --------------------------
 * out[b][c][r] = in[b][r][c] (r < R, c < Cc), 0 for R <= r < ld_out.  in (B, R, ld_in), out (B, Cc, ld_out), bf16;
 * R, Cc, ld_in <= 64; ld_in, ld_out multiples of 8.  compress_interaction_network.py:105 (align_to('B','E','N')):
 * x0 (B,N,E) -> x0T (B,E,ld0) with the field axis padded to the matrix-core k-step, and its gradient back.          */
int trs_transpose_pad(const void* in, int64_t B, int32_t R, int32_t Cc, int32_t ld_in, void* out, int32_t ld_out,
                      int32_t dtype, trs_stream_t stream);

/* ---- one-output Linear over the concatenation of two blocks, without the concatenation -----------------------------
 * The head of deep_and_cross_network.py:82-92: torch.cat([cross_out, deep_out], dim='O') -> flatten(('N','O'),'O') ->
 * nn.Linear(cat_size, 1).  a (rows, N, Ea), d (rows, N, Eb) contiguous, w (N * (Ea + Eb)) in the Linear's own order
 * (field-major [a_f | d_f]), bias (1) or NULL:
 *   out[r] = sum_f  a[r,f,:] . w[f*(Ea+Eb) : +Ea]  +  d[r,f,:] . w[f*(Ea+Eb)+Ea : +Eb]  + bias[0]
 * bwd: ga = g[r] * (a's part of w), gd = g[r] * (d's part) (either may be NULL); gw (N*(Ea+Eb)) and gb (1) fp32,
 * written (both or neither).  Ea, Eb whole 16-byte vectors; N * (Ea + Eb) * sizeof(T) / 16 <= 1024.               */
int trs_cat_head_fwd(const void* a, const void* d, const void* w, const void* bias, int64_t rows, int32_t N, int32_t Ea,
                     int32_t Eb, int32_t dtype, void* out, trs_stream_t stream);
size_t trs_cat_head_bwd_workspace_bytes(int64_t rows, int32_t N, int32_t Ea, int32_t Eb);
int trs_cat_head_bwd(const void* g, const void* a, const void* d, const void* w, int64_t rows, int32_t N, int32_t Ea,
                     int32_t Eb, int32_t dtype, void* ga, void* gd, float* gw, float* gb, void* workspace,
                     size_t ws_bytes, trs_stream_t stream);

/* ---- finish of a split-K weight gradient (the K = batch GEMM of multilayer_perceptron.py's nn.Linear backward) -----
 * 1 .. 8 jobs in one launch (HOST arrays, one S, one dtype; every job is checked before anything is launched), the
 * partials of trs_wgrad_rows[_many] / trs_wgrad_wide[_many] or of a batched library GEMM.  Job k: part[k] (S, R, Cc) fp32
 * partial products  ->  gw[k] (out_rows, out_cols) = sum_s part[k][s, :out_rows, :out_cols] cast to dtype (the un-padded
 * corner when the GEMMs ran on zero-padded weights); gb[k] (out_rows) = cast(gb_f32[k]) (both or neither).
 * trs_wgrad_finish needs out_rows <= 256 * ceil(out_cols / 256) for a job with a gb: its bias cast has one row of
 * workgroups.  trs_wgrad_finish_t is the same for partials stored transposed, part[k] (S, Cc, R) (slices of x^T g):
 * gw[r, c] = sum_s part[s, c, r] for r < out_rows <= R, c < out_cols <= Cc, the slices summed in order.
 * A job WITHOUT a product, part[k] = gw[k] = NULL, only casts: gb[k][c] = gb_f32[k][c] for c < out_cols[k] (R, Cc,
 * out_rows of the job are not read) -- a gradient that arrives summed in fp32, such as a row of
 * trs_mlp_fused_bwd_data_wlast's gw_last, rides in the finish of the other layers.
 * PARTIAL-ROW sources, gb_nparts / gb_stride (both NULL: every source is a summed vector): where gb_nparts[k] > 0,
 * gb_f32[k] is not a summed vector but gb_nparts[k] rows of per-workgroup partial sums, gb_stride[k] floats apart (>= the
 * job's columns) -- what trs_mlp_fused_bwd_data_parts reports.  Value c is the sum over p of gb_f32[k][p * gb_stride[k]
 * + c], taken in the order of the tile backward's own reduce launch, mlp_colsum_reduce_many_kernel (sixteen running sums
 * over p = w, w + 16, ..., then w = 0 .. 15), so the cast value has the bits that trs_mlp_fused_bwd_data + a finish on
 * the summed vector give.  gb_nparts[k] = 0: job k's source is a vector.  Applies to the bias row of a product job and
 * to a job without a product alike.
 * One trs_wgrad_finish job with a product, a vector source (or none), S >= 64 and ceil(out_cols / 256) * out_rows < 64
 * (the 400 -> 1 head) runs on a kernel with sixteen threads per column, which adds the slices in another order.     */
int trs_wgrad_finish(int32_t n_jobs, const float* const* part, int32_t S, const int32_t* R, const int32_t* Cc,
                     const int32_t* out_rows, const int32_t* out_cols, int32_t dtype, void* const* gw,
                     const float* const* gb_f32, void* const* gb, const int32_t* gb_nparts, const int32_t* gb_stride,
                     trs_stream_t stream);
int trs_wgrad_finish_t(int32_t n_jobs, const float* const* part, int32_t S, const int32_t* Cc, const int32_t* R,
                       const int32_t* out_rows, const int32_t* out_cols, int32_t dtype, void* const* gw,
                       const float* const* gb_f32, void* const* gb, const int32_t* gb_nparts, const int32_t* gb_stride,
                       trs_stream_t stream);
/* dW partials by a hand-written kernel instead of a batched library GEMM: part (S, M, N) fp32, slice s = g[rows_s, :M]^T
 * x[rows_s, :N] over the s-th of S contiguous row ranges (bf16 operands, row strides ldg / ldx, M and N multiples of
 * 8); trs_wgrad_finish then folds the slices.  S comes from trs_wgrad_rows_splits (0: shape not handled -- more than
 * 32 blocks of 224 x 224, or fewer than 256 rows); trs_wgrad_rows takes exactly that S.                                */
int32_t trs_wgrad_rows_splits(int32_t M, int32_t N, int64_t rows);
int trs_wgrad_rows(const void* g, int32_t ldg, const void* x, int32_t ldx, int64_t rows, int32_t M, int32_t N,
                   int32_t dtype, int32_t S, float* part, trs_stream_t stream);
/* 1 .. 8 such products over the SAME rows in one launch of the eight-wave LDS-DMA kernel (the tail layers of a deep
 * branch): job k is g[k] (rows, ldg[k]) against x[k] (rows, ldx[k]) into part[k] (S, M[k], N[k]).  The arrays are HOST
 * arrays; the job table travels in the kernel arguments, so nothing is uploaded or allocated and the launch can be
 * captured.  trs_wgrad_rows_many_splits answers S > 0 when every job on its own takes that kernel (blocks of 12 | 13
 * tiles, rows a multiple of 128 below 2^20) with the same block counts, every 208-column image lies inside its
 * operand's row stride, strides are multiples of 8 that cover M / N and keep 32 rows under 2^31 bytes, the batch is
 * resident in one round (blocks * jobs <= 32 per row range) and rows >= 256 * S (two 400 x 400 jobs: S = 32 from 8192
 * rows on); 0 otherwise -- the caller keeps the per-layer calls.  trs_wgrad_rows_many takes exactly that S and 16-byte
 * aligned operands and partials; every job is checked before anything is launched.  trs_wgrad_rows_many_map (host
 * only) tells where workgroup ``block`` works: out = {job, row range, output block, first row, end row}, returns the
 * grid size (0: not taken / no such block).  trs_wgrad_finish folds all the jobs' partials in one launch.          */
int32_t trs_wgrad_rows_many_splits(int32_t n_jobs, const int32_t* M, const int32_t* N, const int32_t* ldg,
                                   const int32_t* ldx, int64_t rows);
int32_t trs_wgrad_rows_many_map(int32_t n_jobs, const int32_t* M, const int32_t* N, const int32_t* ldg,
                                const int32_t* ldx, int64_t rows, int32_t block, int64_t* out);
int trs_wgrad_rows_many(int32_t n_jobs, const void* const* g, const int32_t* ldg, const void* const* x,
                        const int32_t* ldx, int64_t rows, const int32_t* M, const int32_t* N, int32_t S,
                        float* const* part, trs_stream_t stream);
/* the same product for a WIDE input, transposed: part (S, M_x, N_g) fp32, slice s = x[rows_s, :M_x]^T g[rows_s, :N_g] -- what
 * trs_wgrad_finish_t folds -- with no work spent on the padding columns of g.  Taken (trs_wgrad_wide_splits > 0) when M_x
 * is a multiple of 208 (at least two blocks of 13 tiles of 16), N_g a multiple of 16 that cuts into two blocks of 12 | 13
 * tiles whose 208-column images lie inside ld_g (384, 400 or 416 columns; ld_g >= 16 * (N_g / 32) + 208), ld_g a
 * multiple of 8, rows a multiple of 128 and at least 128 * S, and 32 rows of either operand span less than 2^31 bytes.
 * trs_wgrad_wide takes exactly that S, bf16 operands that are 16-byte aligned, ldx >= M_x a multiple of 8; it
 * allocates nothing and does not synchronise.                                                                         */
int32_t trs_wgrad_wide_splits(int32_t M_x, int32_t N_g, int32_t ld_g, int64_t rows);
int trs_wgrad_wide(const void* x, int32_t ldx, const void* g, int32_t ldg, int64_t rows, int32_t M_x, int32_t N_g,
                   int32_t S, float* part, trs_stream_t stream);
/* 1 .. 4 such products over the SAME rows in one launch of the four-wave kernel (a deep branch: the wide first layer and
 * the 400 x 400 layers behind it): job k is x[k] (rows, ldx[k]) against g[k] (rows, ldg[k]) into part[k] (S, M_x[k],
 * N_g[k]).  HOST arrays; the job table travels in the kernel arguments, nothing is uploaded or allocated, the launch can
 * be captured.  trs_wgrad_wide_many_splits answers S > 0 when every job is a shape trs_wgrad_wide takes (with ldx[k] >=
 * M_x[k] a multiple of 8), the blocks of all jobs, TB = sum of M_x[k] / 208, divide 32 -- then S = 8 * min(32 / TB, 4)
 * and all TB workgroups of a row range sit on one XCD, the jobs in table order --, rows is a multiple of 128 and at
 * least 128 * S; 0 otherwise, and the caller keeps the per-product calls.  trs_wgrad_wide_many takes exactly that S and
 * 16-byte aligned operands and partials; every job is checked before the launch.  trs_wgrad_wide_many_map (host only):
 * out = {job, row range, block of the job, first row, end row} of workgroup ``block``, returns the grid size (0: not
 * taken / no such block).  trs_wgrad_finish_t folds all the jobs' partials in one launch.                            */
int32_t trs_wgrad_wide_many_splits(int32_t n_jobs, const int32_t* M_x, const int32_t* ldx, const int32_t* N_g,
                                   const int32_t* ldg, int64_t rows);
int32_t trs_wgrad_wide_many_map(int32_t n_jobs, const int32_t* M_x, const int32_t* ldx, const int32_t* N_g,
                                const int32_t* ldg, int64_t rows, int32_t block, int64_t* out);
int trs_wgrad_wide_many(int32_t n_jobs, const void* const* x, const int32_t* ldx, const void* const* g,
                        const int32_t* ldg, int64_t rows, const int32_t* M_x, const int32_t* N_g, int32_t S,
                        float* const* part, trs_stream_t stream);
/* n strided 2-D copies in one launch: desc (device, n x 6 int64) = {src address, dst address, rows, cols, src_ld,
 * dst_ld} (sizes in elements of elem_size bytes); max_elems = the largest rows*cols (sizes the grid).  Refreshes the
 * zero-padded copies of an MLP stack's nn.Linear parameters (multilayer_perceptron.py:55-61) before a forward.     */
int trs_copy_padded_many(const int64_t* desc, int32_t n, int32_t elem_size, int64_t max_elems, trs_stream_t stream);

/* ---- CIN layer glue on channels-last activations y (B,E,C) bf16 ---------------------------------
 * BatchNorm1d + ReLU + chunk(2) + sum over E of the direct half, compress_interaction_network.py:137-181:
 *   z = relu(y * scale[c] + shift[c])      scale = gamma * invstd, shift = beta - mean * scale (fp32, caller)
 *   hidden[b,e,c-Hs] = z  for c >= Hs ;   pooled[b,c] = sum_e z[b,e,c]  for c < D
 *   (split layers: D = Hs = C/2;  is_direct layers: D = C, Hs = 0)
 * stats: partial (trs_cin_glue_blocks(B), 2, C) fp32 = per-workgroup column sums / sums of squares of y.
 * bwd_reduce: partial (blocks, 2, C) = [sum gz*mask, sum gz*mask*xhat] with gz = g_pooled (c < D) + g_hidden
 * (c >= Hs), mask = [z > 0], xhat = (y - mean) * invstd;  g_hidden / g_pooled may be NULL.
 * bwd_apply: gy = scale * (gz*mask - c1 - xhat * c2), c1 = dbeta/R, c2 = dgamma/R (zeros with running stats). */
int32_t trs_cin_glue_blocks(int64_t B);
int trs_cin_glue_stats(const void* y, int64_t B, int32_t E, int32_t C, int32_t dtype, float* partial,
                       trs_stream_t stream);
int trs_cin_glue_fwd(const void* y, const float* scale, const float* shift, int64_t B, int32_t E, int32_t C, int32_t D,
                     int32_t Hs, int32_t dtype, void* hidden, void* pooled, trs_stream_t stream);
int trs_cin_glue_bwd_reduce(const void* y, const void* g_hidden, const void* g_pooled, const float* scale,
                            const float* shift, const float* mean, const float* invstd, int64_t B, int32_t E, int32_t C,
                            int32_t D, int32_t Hs, int32_t dtype, float* partial, trs_stream_t stream);
int trs_cin_glue_bwd_apply(const void* y, const void* g_hidden, const void* g_pooled, const float* scale,
                           const float* shift, const float* mean, const float* invstd, const float* c1, const float* c2,
                           int64_t B, int32_t E, int32_t C, int32_t D, int32_t Hs, int32_t dtype, void* gy,
                           trs_stream_t stream);
/* The same two passes, also writing their output channels-first: hidden_cf (B, C-Hs, E), gy_cf (B, C, E) -- the
 * operand layout of trs_cin_dw, which otherwise costs one transposing copy of a 1-2 GB tensor per layer and step.
 * Shape limit: E == 8 * (256 / (C / 8)) (e.g. E = 64, C = 256); trs_cin_glue_cf_supported() tells.
 * colsum_partial (optional, may be NULL): [trs_cin_glue_blocks(B)][C] fp32 per-workgroup column sums of gy as stored
 * -- the Conv1d bias gradient of the layer (compress_interaction_network.py:62), which otherwise costs one more pass
 * over the 2 GB tensor.                                                                                             */
int trs_cin_glue_cf_supported(int32_t E, int32_t C);
int trs_cin_glue_fwd_cf(const void* y, const float* scale, const float* shift, int64_t B, int32_t E, int32_t C,
                        int32_t D, int32_t Hs, int32_t dtype, void* hidden, void* hidden_cf, void* pooled,
                        trs_stream_t stream);
int trs_cin_glue_bwd_apply_cf(const void* y, const void* g_hidden, const void* g_pooled, const float* scale,
                              const float* shift, const float* mean, const float* invstd, const float* c1,
                              const float* c2, int64_t B, int32_t E, int32_t C, int32_t D, int32_t Hs, int32_t dtype,
                              void* gy, void* gy_cf, float* colsum_partial, trs_stream_t stream);

/* ---- OuterProductNetwork / BilinearInteraction on the (i<j) pair pattern -------
 * Pair p = (i_p, j_p), i<j, lexicographic (the order of inner_product_network.py:51-52); NC2 = N(N-1)/2.
 *
 * OPN 'vec' / 'num'  (outer_product_network.py:123-129):
 *   out[b,p] = sum_e x[b,i_p,e] * x[b,j_p,e] * kern[p,e]      kern (NC2,E); kern_is_num: kern (NC2), no e index
 * bwd: gx (B,N,E) and gkern_vec (NC2,E) fp32, ACCUMULATED into (for 'num' the caller sums it over e);
 * either may be NULL.                                                                              */
int trs_opn_vec_fwd(const void* x, const void* kern, int32_t kern_is_num, int64_t B, int32_t N, int32_t E,
                    int32_t dtype, void* out, trs_stream_t stream);
size_t trs_opn_vec_bwd_workspace_bytes(int64_t B, int32_t N, int32_t E);
int trs_opn_vec_bwd(const void* g, const void* x, const void* kern, int32_t kern_is_num, int64_t B, int32_t N,
                    int32_t E, int32_t dtype, void* gx, float* gkern_vec, void* workspace, size_t ws_bytes,
                    trs_stream_t stream);

/* pair product:  out[b,p,:] = a[b,i_p,:] * c[b,j_p,:] + bias[(bias_per_pair ? p : 0), :]   (bias may be NULL)
 * Bilinear 'all' (bilinear_interaction.py:72-76) is  a = x W (one GEMM), c = x, shared bias.
 * bwd: ga[b,i,:] = sum_{p: i_p=i} g[b,p,:] c[b,j_p,:],  gc[b,j,:] = sum_{p: j_p=j} g[b,p,:] a[b,i_p,:].   */
int trs_pair_mul_fwd(const void* a, const void* c, const void* bias, int32_t bias_per_pair, int64_t B, int32_t N,
                     int32_t E, int32_t dtype, void* out, trs_stream_t stream);
int trs_pair_mul_bwd(const void* g, const void* a, const void* c, int64_t B, int32_t N, int32_t E, int32_t dtype,
                     void* ga, void* gc, trs_stream_t stream);

/* rows product with bias: the stand-alone forward of FieldAllTypeBilinear / FieldEachTypeBilinear
 * (bilinear_interaction.py:72-76, 144-149), whose operands arrive already gathered per pair as (B,P,E):
 *   out[r,:] = a[r,:] * c[r,:] + bias[(bias_per_pair ? r % P : 0), :]      r over rows = B*P   (bias may be NULL)
 * bwd: ga = g * c, gc = g * a (either may be NULL).  Element-wise passes, any E.                     */
int trs_rows_mul_bias_fwd(const void* a, const void* c, const void* bias, int32_t bias_per_pair, int64_t rows,
                          int32_t P, int32_t E, int32_t dtype, void* out, trs_stream_t stream);
int trs_rows_mul_bwd(const void* g, const void* a, const void* c, int64_t rows, int32_t E, int32_t dtype, void* ga,
                     void* gc, trs_stream_t stream);

/* per-pair bilinear form:  T[b,p,:] = x[b,i_p,:] @ W[(w_per_pair ? p : 0)]     W (NC2 | 1, E, E) row-major [e][h]
 *   mode 0 (OPN 'mat', outer_product_network.py:107-121 with W[p][e][h] = kernel[h,p,e]):
 *           out[b,p]   = sum_h T[b,p,h] * x[b,j_p,h]
 *   mode 1 (Bilinear 'each', bilinear_interaction.py:144-149):
 *           out[b,p,h] = T[b,p,h] * x[b,j_p,h] + bias[(bias_per_pair ? p : 0), h]
 * bwd_data: gx (B,N,E); gT (B,NC2,E) = dL/dT, written when not NULL (the weight gradient
 * dW[p] = sum_b x[b,i_p,:]^T gT[b,p,:] is a plain GEMM per field over it).                          */
int trs_pair_bilinear_fwd(const void* x, const void* W, int32_t w_per_pair, const void* bias, int32_t bias_per_pair,
                          int32_t mode, int64_t B, int32_t N, int32_t E, int32_t dtype, void* out,
                          trs_stream_t stream);
int trs_pair_bilinear_bwd_data(const void* g, const void* x, const void* W, int32_t w_per_pair, int32_t mode,
                               int64_t B, int32_t N, int32_t E, int32_t dtype, void* gx, void* gT,
                               trs_stream_t stream);

/* The same forward on the matrix cores (bf16, E = 32 | 64), one kernel, no (B,NC2,E) intermediate:
 * Wt (NC2, E, E) = the per-pair matrices TRANSPOSED, Wt[p][h][e] = W[p][e][h] (for OPN 'mat' that is kernel[h,p,e]
 * itself); tasks (ntasks, 3) int32 on the device = (i, j0, count <= 3): every pair exactly once, the pairs of a task
 * share i and are adjacent in p.  mode / bias / out as trs_pair_bilinear_fwd (bias per pair, (NC2,E), or NULL).   */
int trs_pair_bilinear_fwd_mfma(const void* x, const void* Wt, const void* bias, const int32_t* tasks, int32_t ntasks,
                               int32_t mode, int64_t B, int32_t N, int32_t E, int32_t dtype, void* out,
                               trs_stream_t stream);

/* Backward of the same on the matrix cores (bf16, E = 32 | 64).  gv = g[b,p] (mode 0) | g[b,p,h] (mode 1); dL/dT = gv * x_j.
 * data:   gx_i = sum_j W_p (gv x_j)   -- tasks_i (nti,3) = (i, j0, count) as in the forward, W resident;
 *         gx_j = sum_i gv * (x_i W_p) -- tasks_j (ntj,3) = (j, i0, count): pairs (i0..i0+count-1, j), Wt resident;
 *         every (sample, task) writes one row into contrib_i (B,nti,E) / contrib_j (B,ntj,E) (bf16 scratch), then
 *         gx[b,f,:] = sum of the rows of field f's tasks;  seg_i / seg_j (N+1) = first task of each field.
 * weight: gW (NC2,E,E) [e][h] = sum_b x_i^T (gv x_j), K = samples through per-wave LDS transposes.               */
int trs_pair_bilinear_bwd_data_mfma(const void* g, const void* x, const void* W, const void* Wt,
                                    const int32_t* tasks_i, int32_t nti, const int32_t* seg_i,
                                    const int32_t* tasks_j, int32_t ntj, const int32_t* seg_j, int32_t mode, int64_t B,
                                    int32_t N, int32_t E, int32_t dtype, void* contrib_i, void* contrib_j, void* gx,
                                    trs_stream_t stream);
size_t trs_pair_bilinear_bwd_w_mfma_workspace_bytes(int64_t B, int32_t N, int32_t E);
int trs_pair_bilinear_bwd_w_mfma(const void* g, const void* x, int32_t mode, int64_t B, int32_t N, int32_t E,
                                 int32_t dtype, void* gW, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* GEMM route of the same form for training batch sizes: T[b,p,:] = x[b,i_p,:] @ W_p comes from one plain GEMM per
 * field i (pairs (i, j>i) are adjacent: (B x E) @ (E x n_i*E)) into a (B,NC2,E) buffer; these passes finish it.
 *   fwd  mode 0: out[b,p] = sum_h T[b,p,h] x[b,j_p,h]       mode 1: T <- T * x_j + bias   (in place; out unused)
 *   bwd  gv = g[b,p] (mode 0) | g[b,p,h] (mode 1):  gxj[b,j_p,:] = sum_i gv * T[b,p,:];  T <- gv * x_j  (= dL/dT)   */
int trs_pair_epilogue_fwd(void* T, const void* x, const void* bias, int32_t bias_per_pair, int32_t mode, int64_t B,
                          int32_t N, int32_t E, int32_t dtype, void* out, trs_stream_t stream);
int trs_pair_epilogue_bwd(const void* g, const void* x, void* T, int32_t mode, int64_t B, int32_t N, int32_t E,
                          int32_t dtype, void* gxj, trs_stream_t stream);

/* AttentionalFactorizationMachineLayer (attentional_factorization_machine.py:82-125) with the reference's dropout on the
 * attention scores applied INSIDE the pass (nn.Dropout is the last module of ``self.attention``, so in training the
 * weighted sum and the returned scores both see the dropped scores):
 *   prod[b,p,:] = x[b,i_p,:] * x[b,j_p,:];  attn[b,p] = softmax_p(w2 . relu(W1 prod + b1) + b2)
 *   keep (B,NC2) uint8, nonzero = kept; multiplier m[b,p] = keep ? keep_scale : 0   (keep_scale = 1/(1-p))
 *   attn      (B,NC2) = the softmax BEFORE dropout (what the backward needs)
 *   attn_drop (B,NC2) = attn * m   (what the layer returns);   out[b,:] = sum_p attn_drop[b,p] prod[b,p,:]
 *   W1 (A,E), b1 (A), w2 (A), b2 (1); out (B,E).  E, A <= 128.
 * keep == NULL: no dropout -- out[b,:] = sum_p attn[b,p] prod[b,p,:]; attn_drop is not written (may be NULL).
 * bwd: g_out (B,E) / g_attn (B,NC2) may be NULL; g_attn is the gradient of attn_drop (of attn when keep == NULL),
 * ``attn`` the un-dropped softmax written by the forward; gx (B,N,E); gW1 (A,E), gb1 (A), gw2 (A), gb2 (1) fp32,
 * ACCUMULATED into.                                                                                                  */
int trs_afm_fwd_dropout(const void* x, const void* W1, const void* b1, const void* w2, const void* b2,
                        const uint8_t* keep, float keep_scale, int64_t B, int32_t N, int32_t E, int32_t A,
                        int32_t dtype, void* out, void* attn, void* attn_drop, trs_stream_t stream);
/* Host-side helper (no device work): the backward kernel's schedule of 16-pair tiles for N fields -- every pair (i < j)
 * exactly once, the pairs of a tile sharing no field (what lets a wave add into per-field gradient rows without
 * atomics), packed greedily from the round-robin rounds.  tiles[16 t + k] = (i << 8) | j, 0xffff = empty slot;
 * *ntiles = 0 when the table does not fit the kernel-argument block (the kernel then walks the rounds themselves).
 * attentional_factorization_machine.py:86-120 (the pair enumeration the attention runs over).                   */
int trs_afm_pair_tiles(int32_t N, uint16_t* tiles, int32_t capacity, int32_t* ntiles);
size_t trs_afm_bwd_workspace_bytes(int64_t B, int32_t N, int32_t E, int32_t A);
int trs_afm_bwd_dropout(const void* g_out, const void* g_attn, const void* x, const void* attn, const uint8_t* keep,
                        float keep_scale, const void* W1, const void* b1, const void* w2, int64_t B, int32_t N, int32_t E,
                        int32_t A, int32_t dtype, void* gx, float* gW1, float* gb1, float* gw2, float* gb2,
                        void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- SENET / compose-excitation gate (FiBiNET, FAT-DeepFFM) ----------------------------------------------------------
 *   z[b,m] = mean_e x[b,m,e];  h = relu(W1 z + b1);  a = relu(W2 h + b2);  out[b,m,:] = x[b,m,:] * a[b,m]
 * x, out (B, M, E); W1 (H, M), b1 (H), W2 (M, H), b2 (M): nn.Linear layouts, all of x's dtype.
 * replaces AdaptiveAvgPool1d + Sequential(Linear, ReLU, Linear, ReLU) + einsum('ijk,ijh->ijk') of
 *   torecsys/layers/ctr/compose_excitation_network.py:85-107.
 *
 * Fused family (trs_senet_fused_supported: M <= 64, 1 <= H <= M, rows of whole 16-byte vectors, M*E*sizeof <= 16 KiB):
 * one kernel, a wave owns a sample and keeps its rows in registers; x is read once and out written once.  gates (B, M) and
 * hidden (B, H), fp32, are written for a backward; both NULL: nothing but out is written.  Every intermediate is fp32,
 * one rounding on store.  Other shapes are refused (TRS_ESHAPE): the caller composes the three streaming entries below. */
int trs_senet_fused_supported(int32_t M, int32_t H, int32_t E, int32_t dtype);
int trs_senet_fwd(const void* x, const void* W1, const void* b1, const void* W2, const void* b2, int64_t B, int32_t M,
                  int32_t H, int32_t E, int32_t dtype, void* out, float* gates, float* hidden, trs_stream_t stream);

/* Backward of trs_senet_fwd; g (B, M, E) of x's dtype, gates / hidden as written by the forward.  With
 *   ga[m] = sum_e g[m,e] x[m,e],  gv = ga [a > 0],  gu = (W2^T gv) [h > 0],  gz = W1^T gu:
 *   dx[m,e] = g[m,e] a[m] + gz[m] / E;   dW2 = sum_b gv (x) h,  db2 = sum_b gv,  dW1 = sum_b gu (x) z,  db1 = sum_b gu
 * x and g are read once, dx is written once, z is recomputed.  dx and each of the four parameter gradients (x's dtype,
 * the parameters' layouts) may be NULL.  The sums over the batch are accumulated in fp32 on chip, one partial slab per
 * workgroup goes to `workspace` and a finish kernel adds the slabs in a fixed order: no float atomics, bit-reproducible
 * from run to run.  The workspace (only needed with a parameter gradient) does not depend on B.
 * replaces the autograd backward of compose_excitation_network.py:85-107 (einsum backward twice, the pooling backward
 * expanded to (B, M, E), the accumulation of the two input gradients, two Linear + ReLU backwards).                    */
size_t trs_senet_bwd_workspace_bytes(int64_t B, int32_t M, int32_t H);
int trs_senet_bwd(const void* x, const void* g, const float* gates, const float* hidden, const void* W1, const void* W2,
                  int64_t B, int32_t M, int32_t H, int32_t E, int32_t dtype, void* dx, void* dW1, void* db1, void* dW2,
                  void* db2, void* workspace, size_t ws_bytes, trs_stream_t stream);

/* General family: any M, any E (rows that are not whole 16-byte vectors take an element loop), any excitation -- the
 * caller runs it between these single-pass kernels, on fp32 (B, M) tensors.
 *   trs_senet_squeeze:    z[b,m] = mean_e x[b,m,e]                    fp32        (compose_excitation_network.py:85-91)
 *   trs_senet_scale_fwd:  out[b,m,:] = x[b,m,:] * a[b,m]              a fp32      (compose_excitation_network.py:103-106)
 *   trs_senet_scale_bwd:  ga[b,m] = sum_e g[b,m,e] x[b,m,e]           fp32, when ga != NULL (needs x and g)
 *                         dx[b,m,e] = g[b,m,e] a[b,m] + gz[b,m] / E   when dx != NULL; gz NULL: the first term alone;
 *                                                                     g NULL: the second alone (squeeze backward)
 * The excitation's backward turns ga into gz, so a layer calls trs_senet_scale_bwd twice: for ga (x and g read), then
 * for dx (g read, dx written).  No (B, M, E) temporary exists besides out and dx.                                      */
int trs_senet_squeeze(const void* x, int64_t B, int32_t M, int32_t E, int32_t dtype, float* z, trs_stream_t stream);
int trs_senet_scale_fwd(const void* x, const float* a, int64_t B, int32_t M, int32_t E, int32_t dtype, void* out,
                        trs_stream_t stream);
int trs_senet_scale_bwd(const void* x, const void* g, const float* a, const float* gz, int64_t B, int32_t M, int32_t E,
                        int32_t dtype, float* ga, void* dx, trs_stream_t stream);

/* ---- mixture-of-experts gating (MoE / MMoE) ----------------------------------------------------------------------------
 *   z[b,g,:] = logits[b,g,:] + bias[g,:];  p = softmax_K(z) (row maximum subtracted);  out[b,g,k] = p[b,g,k] * experts[b,k]
 * logits (B, G*K) is the fp32 result of ONE GEMM of the (B, D) input with the G stacked gate weights (G*K, D), WITHOUT the
 * bias; bias (G*K) or NULL, experts (B, K) -- the concatenated expert outputs -- and out (B, G, K) are of `dtype`.
 * replaces G x (Linear + Softmax + unflatten), the cat to (B, G, K) and einsum('ik,ijk->ijk') of
 *   torecsys/layers/ctr/mixture_of_experts.py:137-160.
 * Backward: p is recomputed from the logits (nothing else is saved); with t = gout * experts:
 *   glogits[b,g,k] = p (t - sum_k p t)   (B, G*K) of dtype -- the operand of the two gradient GEMMs and of the bias sum;
 *   gexperts[b,k]  = sum_g gout[b,g,k] p[b,g,k]   (B, K) of dtype.
 * Everything between the loads and the final stores is fp32; one pass per direction, no workspace, no atomics, a fixed
 * summation order.  Rows of whole 16-byte vectors with K <= 1024 and 16-byte aligned pointers take the vector path (a
 * lane group owns a sample for all gates; trs_moe_gate_vector_shape tells the shape half of that rule, a pure function);
 * any other K >= 1 or alignment takes an element path.  B == 0 returns TRS_OK and touches nothing.
 * trs_moe_gate_last_path: the branch the calling thread's last trs_moe_gate_fwd / _bwd launch took -- 0 none yet, 1 vector,
 * 2 element (a host-side record set where the kernel is launched; for tests and diagnostics).                           */
int trs_moe_gate_vector_shape(int32_t K, int32_t dtype);
int trs_moe_gate_last_path(void);
int trs_moe_gate_fwd(const float* logits, const void* bias, const void* experts, int64_t B, int32_t G, int32_t K,
                     int32_t dtype, void* out, trs_stream_t stream);
int trs_moe_gate_bwd(const float* logits, const void* bias, const void* experts, const void* gout, int64_t B, int32_t G,
                     int32_t K, int32_t dtype, void* glogits, void* gexperts, trs_stream_t stream);

/* ---- attention pooling of a bag of ids (csrc/attn_pool.hip) -------------------------------------------------------
 * Self-attention over the looked-up rows of a padded (B, L) list followed by a sum / mean over the list, collapsed.  Per
 * sample and head h (d = E / H, X the (L, E) rows, c = 1 for mode 0 (sum) and 1 / L for mode 1 (mean)):
 *   [Q | K] = X w_qk^T + b_qk;   P = softmax_rows(Q_h K_h^T / sqrt(d));   pbar_h[m] = c sum_l P[l, m]
 *   out[b, h, :] = sum_m pbar_h[m] X[m, :]                                                    (B, H, E) of the table's dtype
 * The pooled layer output is concat_h(out_h Wv_h^T + c' bv_h) Wout^T + c' bout with c' = 1 (mean) or L (sum): two small
 * GEMMs the caller runs.  replaces aten::embedding + nn.MultiheadAttention + the pooling of list_indices_emb.py:124-152;
 * no (B, L, E) or (B, L, 2E) write.  w_qk (2E, E): the first 2E rows of in_proj_weight, b_qk (2E) or NULL, both of the
 * table's dtype.  Every list position takes part (no key-padding mask, as in the reference); an id outside [0, V) reads
 * as a zero row and raises *err_flag.
 * trs_attn_pool_path (a pure function): 0 unsupported, 1 vector path (fp32 FMA; any 1 <= L <= 64, E <= 128, E % H == 0),
 *   2 MFMA path (bf16 with E % 16 == 0 and d % 16 == 0; operands bf16, fp32 accumulation).
 * trs_attn_pool_blocks: the workgroups a launch uses (persistent: min(B, resident workgroups)); the backward is launched
 *   with the count the caller passes (1 <= blocks <= B), which sizes its per-workgroup outputs.
 * Backward, g = gout (B, H, E); Q, K and P are recomputed from the table rows:
 *   dx (B, L, E) of the table's dtype: the gradient of every looked-up row (input of trs_scatter_rows*);
 *   dw_part (blocks, 2E, E), db_part (blocks, 2E) fp32: per-workgroup partial gradients of w_qk / b_qk, fully written;
 *   the caller adds them over `blocks`.  No atomics, samples are dealt to workgroups statically: reproducible bits.
 *   workspace: trs_attn_pool_bwd_workspace_bytes (0 unless H * L floats do not fit in LDS beside the sample).
 * Errors: NULL pointer TRS_EINVAL; bad dtype / mode, and a shape trs_attn_pool_path refuses, TRS_EDTYPE (-2).       */
int trs_attn_pool_path(int32_t L, int32_t E, int32_t H, int32_t dtype);
int trs_attn_pool_blocks(int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, int32_t backward);
size_t trs_attn_pool_bwd_workspace_bytes(int32_t blocks, int32_t L, int32_t E, int32_t H);
int trs_attn_pool_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                      int64_t B, int32_t L, const void* w_qk, const void* b_qk, int32_t H, int32_t mode, void* out,
                      int32_t* err_flag, trs_stream_t stream);
int trs_attn_pool_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                      int64_t B, int32_t L, const void* w_qk, const void* b_qk, int32_t H, int32_t mode,
                      const void* gout, void* dx, float* dw_part, float* db_part, int32_t blocks, void* workspace,
                      size_t ws_bytes, int32_t* err_flag, trs_stream_t stream);

/* Attention pooling of RAGGED bags: the four entries above with (idx, B, L) replaced by one flat vector of ids (n,) plus
 * offsets, as trs_bag_pool_ragged_fwd takes them: bag b is ids[offsets[b], end_b), end_b = offsets[b + 1] where that entry
 * exists (n_off = B or B + 1), else n; begin and end are clamped to [0, n] on the device and an offset outside it or a
 * decreasing pair (that bag is empty) raises *err_flag.  exclude_row >= 0: the ids equal to it are left out of the bag (no
 * table load); -1: every id is live.  A bag attends to its own live ids only: the sample's L_b is the number of live ids,
 * capped at max_len (1 <= max_len <= 64) -- the FIRST max_len live ids in list order are taken, the others contribute
 * nothing in either direction, and a bag with more raises *err_flag.  The algebra is the padded one with L_b for L
 * (c = 1 / L_b for the mean); no key-padding mask exists, the work is sum_b (L_b E^2 + L_b^2 E).  max_len sizes the LDS
 * layout (it takes the place of L in the path, blocks and workspace queries); no length is read on the host.
 *   out (B, H, E) of the table's dtype;  cnt (B,) fp32 = L_b.  L_b = 0: a zero block, cnt 0, no gradient.
 *   The pooled layer output is concat_h(out_h Wv_h^T + c' bv_h) Wout^T + c' bout with c' = L_b (sum) or [L_b > 0] (mean).
 * Backward: dx (n, E) of the table's dtype, row p = the gradient of position p.  The kernel writes the rows of the positions
 * that were taken and no other: THE CALLER ZERO-FILLS dx, which makes the rows of excluded, not taken and unowned
 * positions exact zeros.  (Bags overlap only behind a decreasing pair of offsets, which is flagged; a shared position's row
 * then holds the gradient of one of its bags.)  dw_part / db_part / blocks / workspace as in trs_attn_pool_bwd (queries:
 * trs_attn_pool_ragged_blocks, trs_attn_pool_ragged_bwd_workspace_bytes); static dealing, no atomics: reproducible bits.
 * Every argument error is reported before any launch: NULL pointer (ids and dx may be NULL when n == 0, b_qk always),
 * n_off not B or B + 1, exclude_row outside [-1, V), max_len outside [1, 64], a mode other than 0 / 1 TRS_EINVAL; n or
 * B >= 2^31 - 1 TRS_ESHAPE; a dtype, or a shape trs_attn_pool_path(max_len, E, H, dtype) refuses, TRS_EDTYPE; a workspace
 * below the query TRS_EWORKSPACE.  B == 0 returns TRS_OK and touches nothing; n == 0 with B > 0 gives B zero blocks.   */
int trs_attn_pool_ragged_blocks(int64_t B, int32_t max_len, int32_t E, int32_t H, int32_t dtype, int32_t backward);
size_t trs_attn_pool_ragged_bwd_workspace_bytes(int32_t blocks, int32_t max_len, int32_t E, int32_t H);
int trs_attn_pool_ragged_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids, int32_t ids_dtype,
                             int64_t n, const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int32_t max_len,
                             int64_t exclude_row, const void* w_qk, const void* b_qk, int32_t H, int32_t mode, void* out,
                             float* cnt, int32_t* err_flag, trs_stream_t stream);
int trs_attn_pool_ragged_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* ids, int32_t ids_dtype,
                             int64_t n, const void* offsets, int32_t off_dtype, int64_t n_off, int64_t B, int32_t max_len,
                             int64_t exclude_row, const void* w_qk, const void* b_qk, int32_t H, int32_t mode,
                             const void* gout, void* dx, float* dw_part, float* db_part, int32_t blocks, void* workspace,
                             size_t ws_bytes, int32_t* err_flag, trs_stream_t stream);

/* ---- residual multi-head self-attention over a short list (csrc/self_attn.hip) -------------------------------------
 * y = x + nn.MultiheadAttention(x, x, x) for x (B, L, E) contiguous, no masks, no dropout.  Per sample (d = E / H):
 *   [Q | K | V] = X w_in^T + b_in;   P_h = softmax_rows(Q_h K_h^T / sqrt(d));   O = concat_h(P_h V_h)
 *   y = X + O w_out^T + b_out                                                                  (B, L, E) of x's dtype
 * replaces the in_proj GEMM, two batched GEMMs, the softmax over (B H, L, L), the out_proj GEMM and the residual add of
 * models/ltr/personalized_reranking.py; nothing but y is written.  w_in (3E, E), w_out (E, E), b_in (3E) and b_out (E)
 * of x's dtype; the biases are both given or both NULL.
 * trs_self_attn_path (a pure function): 0 unsupported, 1 vector path (fp32 FMA; 1 <= L <= 64, E <= 128, E % H == 0 and a
 *   backward working set of 6 L E + 2 L^2 + 6 L floats within 160 KB of LDS: every L at E <= 64, L <= 47 at E = 128),
 *   2 MFMA path (bf16 with E % 16 == 0 and d % 16 == 0 in the same envelope; operands bf16, fp32 accumulation).
 * trs_self_attn_blocks: the workgroups a launch uses (persistent: min(B, resident workgroups)); the backward is launched
 *   with the count the caller passes (1 <= blocks <= B), which sizes its workspace.
 * Backward, gout (B, L, E); Q, K, V, P and O are recomputed from x:
 *   dx (B, L, E) of x's dtype, or NULL when the input needs no gradient;
 *   workspace (trs_self_attn_bwd_workspace_bytes): `blocks` fp32 slabs [dw_in (3E, E) | dw_out (E, E) | db_in (3E) |
 *   db_out (E)], fully written; the caller adds them over `blocks`.  No atomics, samples are dealt to workgroups
 *   statically: reproducible bits.
 * Errors: NULL pointer, one bias without the other, blocks outside [1, B] TRS_EINVAL; bad dtype and a shape
 * trs_self_attn_path refuses TRS_EDTYPE (-2); short workspace TRS_EWORKSPACE.                                          */
int trs_self_attn_path(int32_t L, int32_t E, int32_t H, int32_t dtype);
int trs_self_attn_blocks(int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, int32_t backward);
size_t trs_self_attn_bwd_workspace_bytes(int32_t blocks, int32_t E);
int trs_self_attn_fwd(const void* x, int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, const void* w_in,
                      const void* b_in, const void* w_out, const void* b_out, void* y, trs_stream_t stream);
int trs_self_attn_bwd(const void* x, int64_t B, int32_t L, int32_t E, int32_t H, int32_t dtype, const void* w_in,
                      const void* b_in, const void* w_out, const void* b_out, const void* gout, void* dx,
                      void* workspace, size_t ws_bytes, int32_t blocks, trs_stream_t stream);

/* ---- behaviour-to-interest dynamic routing, MIND (csrc/dynamic_routing.hip) ----------------------------------------
 * priors (B, N, R) fp32 = x @ S (the caller's GEMM, fp32 result), noise (B, K, N, R) of the value dtype, c[b,k,n] = 0:
 *   num_iter - 1 times:  w = softmax_k(noise[b,k,n,r] + c[b,k,n]);  z[b,k,r] = sum_n w priors[b,n,r];  v = squash(z)
 *                        c[b,k,n] += sum_r priors[b,n,r] v[b,k,r]
 *   out (B, K, R) of the value dtype = squash(sum_n softmax_k(noise + c) priors),
 *   squash(z) = n2 / (1 + n2) * z / (sqrt(n2) + 1e-8), n2 = sum_r z^2
 * replaces the repeat / randn_like / softmax / mul / sum / squash / matmul / add chain of layers/ctr/dynamic_routing.py:
 * 113-172; one workgroup keeps a sample's state on chip for all iterations.  c_out (B, K, N) and z_out (B, K, R), fp32,
 * both or neither: the final routing sum and the final z, all the backward needs beside the noise.
 * Backward (the loop runs on detached priors, so w is a constant):
 *   dpri[b,n,r] = sum_k softmax_k(noise + c)[b,k,n,r] dz[b,k,r], dz = the squash backward of gout (B, K, R) at z
 *   -> dpri (B, N, R) of the value dtype; the caller's two GEMMs turn it into the gradients of x and S.
 * A sample with n2 == 0 gives zero output and zero dz (the reference's autograd gives NaN there).  fp32 between loads and
 * stores, the maximum over k is subtracted, fixed summation order, no atomics: reproducible bits.
 * trs_dynamic_routing_path (a pure function): 0 outside 1 <= N <= 128, 1 <= R <= 128, 1 <= K <= 8, fp32 / bf16; 1 rows of
 *   whole 16-byte vectors (16-byte loads where the pointers are aligned as well); 2 element loads.
 * B == 0 returns TRS_OK and touches nothing.  Errors: NULL pointer, B < 0, num_iter < 1 TRS_EINVAL; dtype TRS_EDTYPE; a
 * shape the path function refuses TRS_ESHAPE.                                                                        */
int trs_dynamic_routing_path(int32_t N, int32_t R, int32_t K, int32_t dtype);
int trs_dynamic_routing_fwd(const float* priors, const void* noise, int64_t B, int32_t N, int32_t R, int32_t K,
                            int32_t num_iter, int32_t dtype, void* out, float* c_out, float* z_out, trs_stream_t stream);
int trs_dynamic_routing_bwd(const void* noise, const float* c, const float* z, const void* gout, int64_t B, int32_t N,
                            int32_t R, int32_t K, int32_t dtype, void* dpri, trs_stream_t stream);

/* ---- an ordered list of ids through a one-layer RNN, then pooled (csrc/seq_rnn.hip) --------------------------------
 * table (V, E), idx (B, L) and lengths (B,) int32 or int64, w_ih / w_hh (G E, E), b_ih / b_hh (G E) of the table's dtype,
 * hidden size == E, PyTorch's gate order.  cell: 0 rnn (tanh, G = 1), 1 lstm (G = 4), 2 gru (G = 3).  Per sample, with
 * len = clamp(lengths[b], 0, L), x_t = table[idx[b, t]], h_{-1} = c_{-1} = 0 and t < len:
 *   rnn:  h_t = tanh(W_ih x_t + b_ih + W_hh h_{t-1} + b_hh)
 *   lstm: [i f g o] = W_ih x_t + b_ih + W_hh h_{t-1} + b_hh;  c_t = s(f) c_{t-1} + s(i) tanh(g);  h_t = s(o) tanh(c_t)
 *   gru:  r, z = s(W_i* x_t + b_i* + W_h* h_{t-1} + b_h*);  n = tanh(W_in x_t + b_in + r (W_hn h_{t-1} + b_hn));
 *         h_t = (1 - z) n + z h_{t-1}
 *   mode 0: out (B, E) = *scale * sum_{t < len} h_t;      mode 1: out (B, L, E) = h_t, zeros from t = len on.
 * replaces the sort / aten::embedding / pack_padded_sequence (a host read of the lengths) / nn.LSTM | nn.GRU | nn.RNN /
 * pad_packed_sequence / un-sort / pooling chain of inputs/base/sequence_indices_emb.py:128-171; the (B, L, E) block of
 * looked-up rows is never formed.  scale: ONE float in device memory that the forward writes before its main kernel --
 * 1 / max_b len (the reference's divisor: pad_packed_sequence pads to the batch maximum; 0 when every length is 0) with
 * average != 0, else 1 -- and the backward reads.  No host synchronisation.
 * h_save (B, L, E) of the value dtype (h_t, zeros from t = len on) and c_save (B, L, E) fp32 (the lstm's c_t, written for
 * t < len only) are what the backward needs; either may be NULL in a forward that no backward follows.  fp32 FMA between
 * loads and stores; h_t is rounded to the value dtype once per step (the next step's operand and the saved state are the
 * same number).
 * Index rules: an id outside [0, V) at a live step reads as a zero row and raises *err_flag; ids at t >= len are never
 * read.  A length outside [1, L] is clamped to [0, L] and raises the same flag; length 0 gives a zero output row.
 * trs_seq_rnn_path (a pure function): 0 not covered; 1 the vector path (fp32 FMA; fp32 or bf16 operands, 1 <= E <= 128,
 *   any L >= 1, all three cells); 2 the matrix-core path (mfma_f32_16x16x32_bf16): bf16, E in {16, 32, 64} for all three
 *   cells, any L >= 1.  There a wave keeps its B fragments of [W_ih | W_hh] (and, in the backward, of W_hh by rows) in
 *   REGISTERS for its whole tile of samples, not in LDS: 16 (forward) + 8 (backward) fragments of four registers at the
 *   lstm's E = 64, which is what bounds E -- E = 128 would need four times that, and E = 48 is three 16-unit tiles that
 *   four waves do not divide; both take path 1.  The A operands are x_t (bf16 rows of the table: exact) and h_{t-1}
 *   (rounded once per step on both paths); in the backward's dh_{t-1} = dgates_h W_hh the A operand is dgates_h as it is
 *   stored, i.e. rounded to bf16.  fp32 accumulators.  Weight pointers that are not 16-byte aligned take the path-1
 *   kernels (same results to rounding; the path function, being pure, still says 2).
 * workspace: trs_seq_rnn_workspace_bytes(cell, E) = 2 G E E floats, a transposed fp32 image of the two weight matrices
 *   that each entry writes for itself (contents need not survive between calls).
 * Backward, t from len - 1 down to 0 with dh (and dc) on chip, the gates recomputed from x_t and the saved state; gout is
 * (B, E) for mode 0 and (B, L, E) for mode 1, of the value dtype:
 *   dgates (B, L, G E) of the value dtype: the gradient of the pre-activations on the INPUT side, zeros from t = len on;
 *   dgates_h (B, L, G E), gru only (NULL for the other cells, whose two sides are equal): the whole block on the HIDDEN
 *   side -- blocks r and z repeat dgates, block n is r * dn.  dh_{t-1} = dgates_h W_hh (+ z dh_t for the gru) on chip.
 *   The caller's GEMMs finish: dX = dgates W_ih -> trs_scatter_rows*, dW_ih = dgates^T X, dW_hh = dgates_h^T H_prev (the
 *   saved h shifted by one step), the biases as column sums.  No atomics, a static deal of samples to workgroups (which
 *   needs no count from the caller), fixed summation order: out, h_save, c_save, dgates and dgates_h have reproducible
 *   bits, and so has dX.  The TABLE gradient is not these entries' result: dX reaches the table through the row buckets
 *   (trs_csr_build*), where the order of a bucket's entries comes from int32 atomics, so for a row that more than two
 *   live positions look up its last bit may differ between two bucket builds, as for every lookup of this library.
 * B == 0 returns TRS_OK and touches nothing.  Errors: NULL pointer, B < 0, bad cell / mode / index dtype, an lstm without
 * c_save or a gru without dgates_h in the backward TRS_EINVAL; dtype TRS_EDTYPE; a shape the path function refuses
 * TRS_ESHAPE; a workspace that is too small TRS_EWORKSPACE -- all before any launch.                                 */
int trs_seq_rnn_path(int32_t cell, int32_t L, int32_t E, int32_t dtype);
size_t trs_seq_rnn_workspace_bytes(int32_t cell, int32_t E);
int trs_seq_rnn_fwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                    const void* lengths, int32_t len_dtype, int64_t B, int32_t L, const void* w_ih, const void* w_hh,
                    const void* b_ih, const void* b_hh, int32_t cell, int32_t mode, int32_t average, float* scale,
                    void* out, void* h_save, float* c_save, void* workspace, size_t ws_bytes, int32_t* err_flag,
                    trs_stream_t stream);
int trs_seq_rnn_bwd(const void* table, int64_t V, int32_t E, int32_t dtype, const void* idx, int32_t idx_dtype,
                    const void* lengths, int32_t len_dtype, int64_t B, int32_t L, const void* w_ih, const void* w_hh,
                    const void* b_ih, const void* b_hh, int32_t cell, int32_t mode, const float* scale,
                    const void* h_save, const float* c_save, const void* gout, void* dgates, void* dgates_h,
                    void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- index staging: pack per-field columns into the (B,N) index matrix --------
 * out[b, c] = src_j[b * width_j + t]  for the c-th output column = column t of source j.
 * replaces the per-field unsqueeze + torch.cat of inputs/inputs.py:75-80 by one pass.
 * srcs / widths are HOST arrays (nsrc device pointers, their column counts); sum(widths) <= 256.
 * src_dtype / out_dtype: TRS_I64 | TRS_I32 (narrowing to int32 is the caller's responsibility).   */
int trs_pack_columns(const void* const* srcs, const int32_t* widths, int32_t nsrc, int32_t src_dtype,
                     int64_t B, void* out, int32_t out_dtype, trs_stream_t stream);

/* ---- the scalar head of the CTR models and its loss (callers M1 / M2 / M4 of section 8a) ----------
 * logit[b] = sum_e fm[b,e] + sum_n feat[b,n] + sum_k extras[k][b * extra_strides[k]] + bias[0]          -> out (B,1)
 *   models/ctr/factorization_machine.py:55-66 (fm_second.sum('O') + feat_inputs.sum('N') + bias),
 *   models/ctr/deep_fm.py:75-104 (cat([fm_second, fm_first]).sum('O') + deep_out),
 *   models/ctr/xdeep_fm.py:117-121 (feat.sum('N') + cin_out + deep_out + bias).
 * fm (B,E) / feat (B,N) contiguous, either may be NULL (E / N = 0); extras: HOST array of n_extras <= 4 device pointers to
 * one value per sample with element stride extra_strides[k] (a (B,1) column, or column 0 of a wider padded output);
 * bias: one device value or NULL.  fp32 accumulation, one rounding on store.  The gradient of every operand is the
 * incoming (B,1) column itself (broadcast): there is no backward entry point.                                        */
int trs_ctr_logit_fwd(const void* fm, int32_t E, const void* feat, int32_t N, const void* const* extras,
                      const int64_t* extra_strides, int32_t n_extras, const void* bias, int64_t B, int32_t dtype,
                      void* out, trs_stream_t stream);
/* BCEWithLogitsLoss, reduction = mean (the loss the fwd+bwd metric is defined on):
 *   loss = mean_b( max(x,0) - x*y + log1p(exp(-|x|)) )   -> *loss (fp32, device);  logits (B) f32|bf16, labels (B) f32|bf16
 *   bwd: glogits[b] = (sigmoid(x) - y) * gout[0] / B     (gout: fp32 device scalar, NULL = 1)
 * Two launches forward (per-workgroup partial sums in a fixed order: reproducible), one backward.                    */
size_t trs_bce_logits_workspace_bytes(int64_t B);
int trs_bce_logits_fwd(const void* logits, int32_t dtype, const void* labels, int32_t label_dtype, int64_t B, float* loss,
                       void* workspace, size_t ws_bytes, trs_stream_t stream);
int trs_bce_logits_bwd(const void* logits, int32_t dtype, const void* labels, int32_t label_dtype, const float* gout,
                       int64_t B, void* glogits, trs_stream_t stream);

/* ---- pair scores of the embedding models (csrc/rank.hip) ----------------------------------------------------------
 * models/emb/matrix_factorization.py:21-36 + layers/emb/generalized_matrix_factorization.py:44-57 (inner product) and
 * models/emb/starspace.py:38-124 + layers/emb/starspace.py:62-90 (any similarity; here inner product and cosine) behind the
 * negative sampler miners/uniform_batch_miner.py:17-44, which repeats the anchor id K times and lets the input layer
 * gather a (B (1+K), 2, E) block.  Here:
 *   scores[b, j] = sim(A[a_idx[b] + a_offset], T[t_idx[b, j] + t_offset]),  j = 0 .. K  (column 0: the positive)
 * a_table (Va, E) and t_table (Vt, E) of one value dtype (the two pointers may be equal), a_idx (B) and t_idx (B, 1+K) of
 * one index dtype, the offsets plain row numbers added to every id of their side.  sim: 0 = inner product, 1 = cosine as
 * ATen's cosine_similarity, dot / (max(|a|, eps) max(|t|, eps)) with eps = 1e-8.  scores (B, 1+K) of out_dtype: the
 * table's or TRS_F32; fp32 accumulation, one rounding on store.  The anchor row is read once per sample; no (B (1+K), 2, E)
 * and no (B, 1+K, E) block exists.  An id outside its table reads as a zero row and raises *err_flag.
 * Backward from g_scores (B, 1+K) of g_dtype (the table's or TRS_F32): the rows are gathered again, norms and cosines
 * recomputed, and the gradient ROWS written to g_block (B, 2+K, E) of the table's dtype, ordered [anchor, positive,
 * negatives]:  g_block[b, 0] = sum_j g_bj dsim/da (j in order),  g_block[b, 1+j] = g_bj dsim/dt;  the row of an id outside
 * its table is zeros.  No atomics: reproducible bits.  The TABLE gradient is trs_csr_build* + trs_scatter_rows* over the
 * (B, 2+K) id matrix (one walk for a shared table, two walks over the column ranges 0 and 1 .. 1+K for two tables).
 * trs_pair_score_path (pure): 1 = lane-group kernels (rows of 1, 2, 4 .. 64 whole 16-byte vectors; one group per sample,
 * 16-byte loads, shuffles), 0 = one thread per (b, j) (any other E; the forward also when a table pointer is not 16-byte
 * aligned), -1 = bad E / dtype.  The backward of path 0 needs trs_pair_score_bwd_workspace_bytes (0 for path 1), and
 * path 1 needs 16-byte aligned tables and g_block (TRS_EALIGN).
 * K >= 0; B == 0 returns TRS_OK and touches nothing.  Errors, all before any launch: NULL pointer, bad sim, bad index dtype,
 * bad size TRS_EINVAL; value / out / gradient dtype TRS_EDTYPE; workspace TRS_EWORKSPACE.                             */
int trs_pair_score_path(int32_t E, int32_t dtype);
int trs_embed_pair_score_fwd(const void* a_table, int64_t Va, const void* a_idx, int64_t a_offset, const void* t_table,
                             int64_t Vt, const void* t_idx, int64_t t_offset, int32_t E, int32_t dtype, int32_t idx_dtype,
                             int64_t B, int32_t K, int32_t sim, void* scores, int32_t out_dtype, int32_t* err_flag,
                             trs_stream_t stream);
size_t trs_pair_score_bwd_workspace_bytes(int64_t B, int32_t K, int32_t E, int32_t dtype);
int trs_embed_pair_score_bwd(const void* a_table, int64_t Va, const void* a_idx, int64_t a_offset, const void* t_table,
                             int64_t Vt, const void* t_idx, int64_t t_offset, int32_t E, int32_t dtype, int32_t idx_dtype,
                             int64_t B, int32_t K, int32_t sim, const void* g_scores, int32_t g_dtype, void* g_block,
                             void* workspace, size_t ws_bytes, trs_stream_t stream);

/* ---- ranking losses over (positive, negatives) scores (csrc/rank.hip; losses/ltr/functional.py) ---------------------
 * pos: one value per sample at pos[b * pos_stride]; neg: K values per sample at neg[b * neg_stride + k] (columns 0 and
 * 1 .. K of one (B, 1+K) score matrix: pos = S, neg = S + 1, both strides 1 + K); dtype TRS_F32 | TRS_BF16; mask (B) one
 * byte per sample (torch.bool), 0 = the sample is dropped, or NULL.  Terms, per kept sample b and negative k:
 *   kind 0  (1 - sigmoid(p)) + sigmoid(n)      pointwise_logistic_ranking_loss
 *   kind 1  softplus(-(p - n))                 bayesian_personalized_ranking_loss (= -log sigmoid(p - n), finite for every
 *                                              argument); TripletLoss(margin = 0) -> nn.SoftMarginLoss
 *   kind 2  max(0, margin - p + n)             hinge_loss; TripletLoss(margin) -> nn.MarginRankingLoss
 *   kind 3  max(0, margin - p + max_k n)       ONE term per sample: adaptive_hinge_loss as documented
 * *loss (fp32, device) = the sum of the terms divided by: reduction 0 nothing (sum), 1 the number of kept terms (mean),
 * 2 the number of kept SAMPLES (the reference's apply_mask rule: loss[mask].sum() / mask.sum()).  No kept sample under
 * reduction 1 / 2 gives NaN (0 / 0), as the reference's.  *denom (fp32, device, may be NULL) receives the divisor.
 * Two launches: per-workgroup partial sums in a fixed order, then one wave (reproducible bits).
 * bwd: g_pos[b * g_pos_stride] = sum_k dterm/dp, g_neg[b * g_neg_stride + k] = dterm/dn, times gout[0] (fp32 device
 * scalar, NULL = 1) over the divisor (denom: the forward's, required for a masked mean; NULL = computed from B and K);
 * zeros for a dropped sample.  kind 3: the first of equal maximal negatives takes the gradient.  kinds 2 and 3: a hinge
 * argument of exactly 0 passes the gradient (margin - p + n >= 0), as ATen's clamp(min=0) and margin_ranking_loss do; the
 * forward's term is 0 either way.  K >= 1.  B == 0 returns TRS_OK.  Errors before any launch: dtype TRS_EDTYPE; kind,
 * reduction, sizes, strides, NULL TRS_EINVAL.                                                                         */
size_t trs_rank_loss_workspace_bytes(int64_t B);
int trs_rank_loss_fwd(const void* pos, int64_t pos_stride, const void* neg, int64_t neg_stride, int32_t dtype,
                      const void* mask, int64_t B, int32_t K, int32_t kind, float margin, int32_t reduction, float* loss,
                      float* denom, void* workspace, size_t ws_bytes, trs_stream_t stream);
int trs_rank_loss_bwd(const void* pos, int64_t pos_stride, const void* neg, int64_t neg_stride, int32_t dtype,
                      const void* mask, int64_t B, int32_t K, int32_t kind, float margin, int32_t reduction,
                      const float* gout, const float* denom, void* g_pos, int64_t g_pos_stride, void* g_neg,
                      int64_t g_neg_stride, trs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* TRS_ABI_H_ */
