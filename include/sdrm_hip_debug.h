/*
 * sdrm_hip_debug.h — test and tuning hooks of libsdrm_hip.so.  NOT part of the drop-in boundary (that is
 * sdrm_hip.h): nothing here has a counterpart in the reference, a production caller never needs it, and the
 * signatures may change between rounds.  Used by tests/ (to force every kernel variant through the same parity
 * checks, whatever the size thresholds currently are) and by tools/ (tile sweeps).
 *
 * Every setter acts on ONE handle: tile / path selection lives in the engine (sdrm_hip.h "Conventions"), so
 * forcing a variant on one engine never changes what another engine in the same process launches.  The kernel path of a
 * train step is decided once, by its sdrm_train_forward: a setter called between a forward and its backward takes effect at the
 * next sdrm_train_forward; some of them drop the pending forward, as said below.  The path of a sampling call - the narrow nets' one
 * launch, the persistent kernel, or a launch per layer - is decided once as well, by its sdrm_sample_begin.
 */
#ifndef SDRM_HIP_DEBUG_H
#define SDRM_HIP_DEBUG_H

#include "sdrm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* What sdrm_create checks of the device: SDRM_OK for a gfx950 (architecture string as hipDeviceProp_t::gcnArchName gives it,
 * e.g. "gfx950:sramecc+:xnack-") with 256 compute units, SDRM_ERR_DEVICE otherwise.  Pure function: callable without a GPU. */
int sdrm_debug_device_check(const char* gcn_arch, int compute_units);

/* What sdrm_vae_input_layer_fwd / _wgrad check and derive on the host before any launch: SDRM_ERR_SHAPE outside their envelope
 * (`first` is row0 / lo; `contiguous` != 0: rows first .. first + b - 1 must lie inside the feed), else SDRM_OK with the dropout
 * threshold floor((double)p_drop * 2^32) in *thr and the scale (float)(1 / (1 - (double)p_drop)) in *scale (either may be NULL).
 * Pure function: callable without a GPU. */
int sdrm_debug_input_layer_args(int n_items, int hidden, int64_t n_rows, int64_t first, int b, int contiguous, float p_drop,
                                uint32_t* thr, float* scale);

/* What sdrm_vae_latent_fwd / _bwd check on the host before any launch: SDRM_ERR_SHAPE outside their envelope (1 <= hidden <= 4096,
 * 1 <= latent <= 4096, 1 <= b <= 2^22; `contiguous` != 0, the forward without a `rows` array: the feed rows row0 .. row0 + b - 1 must
 * lie in [0, 2^31)), else SDRM_OK.  Pure function: callable without a GPU. */
int sdrm_debug_latent_args(int hidden, int latent, int b, int64_t row0, int contiguous);

/* What sdrm_vae_decoder_nll_fwd / _bwd check on the host before any launch: SDRM_ERR_SHAPE outside their envelope (1 <= latent <= 4096,
 * 1 <= hidden <= 4096, 1 <= n_items <= 2^20, 1 <= b <= 2^22, b x n_items < 2^40, n_rows >= 1, row0 >= 0; `contiguous` != 0, a call
 * without a `rows` array: row0 + b <= n_rows) and for anything a later GEMM launch would refuse on any tile - with the weight
 * gradient's K chunk chosen from n_items and the launches banded as the entry points do, nothing inside the envelope is - else
 * SDRM_OK.  Pure function: callable without a GPU. */
int sdrm_debug_decoder_nll_args(int latent, int hidden, int n_items, int b, int64_t row0, int64_t n_rows, int contiguous);

/* What sdrm_vae_adam_step checks on the host before any launch, on integers: addr [4 n_tensors] holds the addresses p, g, m, v of every
 * tensor, n [n_tensors] their element counts, l2_coef [n_tensors] their L2 coefficients; `has_partials` != 0: an l2_partials buffer of
 * l2_capacity elements is given.  The refusals are that entry point's (SDRM_ERR_ARG: a null array or address, step < 1, a negative
 * l2_coef, two of the ranges [addr, addr + 4 n) sharing a byte; SDRM_ERR_SHAPE: n_tensors <= 0, n outside 1 .. 2^40, more than 2^30
 * chunks, l2_capacity below the chunk count while some l2_coef > 0), else SDRM_OK with the chunk count of the table, sum over the
 * tensors of ceil(n / 4096), in *chunks_out (may be NULL).  Pure function: callable without a GPU. */
int sdrm_debug_vae_adam_args(const uint64_t* addr, const int64_t* n, const float* l2_coef, int n_tensors, int64_t step, int has_partials,
                             int64_t l2_capacity, int64_t* chunks_out);

/* What sdrm_holdout_split checks and derives on the host before any launch: SDRM_ERR_SHAPE outside its envelope (1 <= n_items <=
 * 2^20, 1 <= n_rows < 2^31, 0 <= nnz < 2^40, 0 < test_prop < 1), else SDRM_OK with the held-out count of a row of n_u entries,
 * n_u < 2 ? 0 : min(n_u, (int64)ceil(test_prop * (double)n_u)), in *m_out (may be NULL).  Pure function: callable without a GPU. */
int sdrm_debug_holdout_args(int n_items, int64_t n_rows, int64_t nnz, double test_prop, int64_t n_u, int64_t* m_out);

/* What sdrm_vae_eval_holdout checks on the host before any launch: SDRM_ERR_SHAPE outside its envelope (1 <= n_items <= 36864,
 * 1 <= hidden <= 4096, 1 <= latent <= 4096, 1 <= n_rows < 2^31, 1 <= batch <= 2^22, 1 <= k <= min(128, n_items), metric 0 or 1) and
 * for anything a later GEMM launch would refuse on any tile - with the launches banded as the entry point does, nothing inside the
 * envelope is - else SDRM_OK.  Pure function: callable without a GPU. */
int sdrm_debug_vae_eval_args(int n_items, int hidden, int latent, int64_t n_rows, int batch, int k, int metric);

/* Tile shapes of the MFMA GEMM template, as numbered by sdrm_debug_set_tile / the `cfg` arguments below:
 *   0 = 64x64x16 (default), 1 = 64x64x32, 2 = 64x128x16, 3 = 128x128x16 on v_mfma_f32_32x32x2_f32,
 *   4 = 32x32x32 on v_mfma_f32_16x16x4_f32. */
enum { SDRM_TILE_AUTO = -1, SDRM_TILE_COUNT = 5 };

/* Forces the GEMM tile shape of every launch of this engine (SDRM_TILE_AUTO = automatic: 64x64x16, or 32x32x32 for NT
 * launches of at most `nt32` rows, see sdrm_debug_set_nt32_rows); also env SDRM_TILE, read by sdrm_create.  Refused
 * (SDRM_ERR_STATE) between sdrm_train_backward_begin and _finish and inside a sampling call; a train forward still
 * waiting for its backward is dropped (the slope partial layout of a backward is fixed by the tile of its forward). */
int sdrm_debug_set_tile(sdrm_engine* e, int cfg);
/* Row thresholds of the automatic tile choice: NT launches of at most max_rows rows (sampling, plain forward; default
 * 4096) / max_rows_train stacked rows (train step; default 8192) run on the 32x32x32 tile.  A negative value leaves
 * that threshold alone.  Also env SDRM_NT32_MAX_ROWS / SDRM_NT32_MAX_ROWS_TRAIN. */
int sdrm_debug_set_nt32_rows(sdrm_engine* e, int max_rows, int max_rows_train);
/* The LDS-resident kernels used when the padded widths are <= 64 (csrc/skinny.h, csrc/skinny_step.h, csrc/skinny_fwd4.h):
 * 1 (default) on, the train forward owning 4 users per work-group (4x4x1 MFMAs); 2 on, with the 16-user train forward (what shapes
 * whose LDS image does not fit take anyway); 0 off: narrow nets go through the general per-layer GEMM path. */
int sdrm_debug_set_skinny(sdrm_engine* e, int on);
/* Row-owned train forward (csrc/rowchain.h: staging, every layer and the loss partial sums of a 96-row group of stacked rows in
 * ONE work-group per CU; nets with L == W and a padded width of 128..352): 0 never, 1 (default) when the batch fills whole
 * rounds of the chip (one round: at least 154 groups of 32 users; more: the last round at least five sixths full), 2 whenever the net allows
 * (tests); also env SDRM_ROWCHAIN.  A forced tile (sdrm_debug_set_tile) switches it off.  Results agree with the per-layer path
 * to fp32 summation order; the stacked rows of that step are in the GROUPED order (elementwise.h), which sdrm_get_train_outputs
 * / sdrm_get_preacts undo.  Refused between sdrm_train_backward_begin and _finish; drops a pending train forward. */
int sdrm_debug_set_rowchain(sdrm_engine* e, int mode);
/* The row-owned train step on 48-row work-groups (csrc/rows48.h: the P, S, Q rows of 16 users per work-group through staging,
 * every layer and the loss sums, then through the loss seeds and every layer's input gradient; the nets of the row-owned forward):
 * 0 never, 1 (default) when the batch's 16-user groups fill most of one round of the chip (160..256 groups: 2545..4096 users) and
 * the 96-row kernels do not take the batch, 2 whenever the net allows (tests); also env SDRM_ROWS48.  sdrm_debug_set_rowchain(e, 2)
 * and a forced tile take precedence.  The stacked rows of such a step are grouped by 16 users (elementwise.h).  Refused between
 * sdrm_train_backward_begin and _finish; drops a pending train forward. */
int sdrm_debug_set_rows48(sdrm_engine* e, int mode);
/* Column-split row groups of that step (csrc/rows48.h): G work-groups of ONE XCD share a 48-row group - each owns 1 / G of every
 * layer's output columns and pulls the rest of the next layer's input through that XCD's L2 (work-group-scope atomics + sc1 loads,
 * no device-scope fence) - so that batches of at most 2048 users fill the chip in 6 launches instead of 11: 0 never, 1 (default) by
 * size (1281..2048 users: 2 work-groups per group), 2 / 4 that many whenever groups x G fit the 256 CUs (every
 * work-group of such a launch must be resident at once); also env SDRM_ROWS48_SPLIT.  Needs the chip's block -> XCD mapping
 * (checked by sdrm_create: sdrm_debug_rows48_split_available).  A hand-shake that times out (30 ms) is reported by the next train
 * call on the handle as SDRM_ERR_HIP and switches the path off for the handle. */
int sdrm_debug_set_rows48_split(sdrm_engine* e, int mode);
int sdrm_debug_rows48_split_available(const sdrm_engine* e);
/* The shared-tile form of the 48-row kernels (csrc/rows48.h; nets whose padded width is 4 q + 2 column tiles of 16 - 352 is 22 -, one
 * work-group per row group): the four waves own q tiles each and the waves of a pair split the K-steps of one more, instead of
 * multiplying two tiles of zeros in the last wave: 1 (default) on, 0 the plain form; also env SDRM_ROWS48_SHARE.  The same sums in
 * another order for the shared tiles' columns (two partial sums over alternate K-steps). */
int sdrm_debug_set_rows48_share(sdrm_engine* e, int on);
/* Reverse-sampling steps without kernel boundaries between the layers (csrc/sample_persist.h: one launch per sdrm_sample_steps call
 * runs its `count` steps - every layer on the 32x32 tile, the reverse update in the out layer's epilogue - with the column tiles of
 * a row tile synchronised through ONE XCD's L2): full-resolution PHILOX sampling of a net with L == W; 0 never, 1 (default) for at
 * most 352 rows (one work-group per CU: measured 12.1 against 16.5 us per step at 339 rows; at 679 rows - the 8-GPU shard of the 5429
 * sampled users - the fullest XCDs hold 33 work-groups for 32 CUs and it ties, 16.0 against 16.4), 2 whenever every work-group of the launch is resident at once
 * (at most two 32x32 tiles per CU on the fullest XCD); also env SDRM_SAMPLE_PERSIST.  Results are those of the per-layer path with
 * the fused reverse update (same tile body, same epilogue).  Refused inside a sampling call. */
int sdrm_debug_set_sample_persist(sdrm_engine* e, int mode);
/* Fault injection for that path: the NEXT column-split launch waits for a count its group never reaches (its base is moved up by
 * `skew`), so every work-group of it runs into the 30 ms bound of its first hand-shake, raises the abort word and returns; the
 * next train call on the handle then reports SDRM_ERR_HIP and the handle continues on the per-layer path. */
int sdrm_debug_split_skew(sdrm_engine* e, unsigned skew);
/* Strip-owned weight gradients (csrc/wgrad2.h: every weight gradient of a step in one balanced round of one work-group per CU,
 * bias gradients from the ones column of the layer inputs) behind the row-owned forward: 1 (default) on, 0 the batched 64x64-tile
 * split-K launch; also env SDRM_WGRAD_STRIPS.  Takes effect with the next train forward. */
int sdrm_debug_set_wgrad_strips(sdrm_engine* e, int on);
/* Row-owned input gradients (csrc/dgrad_rows.h: one work-group per CU owns 96 stacked rows and every column of a layer's input
 * gradient, operands straight from global memory, PReLU' and the slope partial sums on 16-byte quads) behind the row-owned
 * forward: 1 (default) the loss value, the gradient seeds and every layer's dgrad in ONE launch (k_dgrad_chain: rows never meet, a
 * work-group runs down the chain on its own), 2 k_loss_seed + one k_dgrad_rows launch per layer, 0 k_loss_seed + the 64x64-tile
 * launches; also env SDRM_DGRAD_ROWS.  Drops a pending train forward (a row-owned forward stores no pre-activations when these
 * kernels follow: they read the activations). */
int sdrm_debug_set_dgrad_rows(sdrm_engine* e, int mode);
/* 1 when this engine's shape qualifies for the row-owned forward (its fragment-packed weight copies exist). */
int sdrm_debug_rowchain_available(const sdrm_engine* e);
/* Fusion of the DDPM reverse update into the out-layer GEMM epilogue (full-resolution sampling with on-device Philox;
 * every other case uses the stand-alone k_reverse_update): 0 never, 1 (default) for launches of at most 4096 rows - the
 * shards of a multi-GPU run, which run on the 32x32 tile where one launch less per reverse step is worth more than the
 * epilogue's Philox work - 2 always; also env SDRM_FUSE_REV.  Results are identical up to the rounding of the update
 * arithmetic.  Not refused inside a sampling call: the per-layer launches of that call follow the new mode from their next step on;
 * whether the call may take the persistent kernel (mode 0 rules it out) was decided by its sdrm_sample_begin and stays. */
int sdrm_debug_set_fused_reverse(sdrm_engine* e, int mode);
/* Row chains of a sampling call (csrc/sdrm_hip.hip: independent row ranges run on separate HIP streams so that one
 * chain's launch gaps are filled by another's kernels): -1 = by size (default: sdrm_debug_chains), 1..4 forced; also env SDRM_CHAINS.
 * Rows are independent and randoms are keyed by row: every chain count computes the same call; the tile and the fusion of the reverse
 * update go by a chain's row count, so the last bits may differ between chain counts (never between two runs of one). */
int sdrm_debug_set_chains(sdrm_engine* e, int chains);
/* The number of row chains of the sampling call in progress (or of the last one); by size: two once the call has 2560 x 352 elements
 * per layer (ML-1M: n >= 2560 rows).  While an event profile is recorded (sdrm_profile_begin) the chains run one after the other.
 * How chains and train steps queued between sampling steps share the chip (csrc/sdrm_hip.hip: ChainSched) has two
 * environment switches for A/B runs, read at sdrm_create: SDRM_DETACH=0 keeps the one chain of a small call on the caller's stream
 * (default: on an auxiliary stream, beside train steps of the per-layer path), SDRM_HOLD_EARLY=0 makes the chains wait for the end of a
 * row-owned train step (default: for its weight gradients; the tail runs beside them). */
int sdrm_debug_chains(const sdrm_engine* e);

/* What ran last on this handle, read back from the engine's own records (host code only: no device work, nothing changes).
 * train_path / parts / dgrad: the plan of the last sdrm_train_forward, alone or inside a sdrm_train_step - the kernel path, the work-groups
 * per 48-row group (1, or 2 / 4 column-split; 1 on every other path) and the form of its input gradients.  sample_path: what the last
 * sdrm_sample_begin decided (SDRM_SAMPLE_PATH_PERSIST: the persistent kernel while no hand-shake has timed out, else a launch per
 * layer).  Before the first train forward / sampling call the values are those of a per-layer step.  Any out pointer may be NULL.
 * Lets a test of the size rules assert which path a batch really took, so that a retuned threshold fails the test instead of
 * quietly moving what it covers. */
enum { SDRM_PLAN_PER_LAYER = 0,    /* one launch per layer (64x64 / 32x32 tiles) */
       SDRM_PLAN_SKINNY = 1,       /* the narrow nets' step (csrc/skinny_step.h) */
       SDRM_PLAN_ROW96 = 2,        /* row-owned, 96-row work-groups (csrc/rowchain.h) */
       SDRM_PLAN_ROW48 = 3 };      /* row-owned, 48-row work-groups (csrc/rows48.h); parts > 1: column-split */
enum { SDRM_PLAN_DGRAD_TILES = 0,            /* k_loss_seed + a tile GEMM per layer */
       SDRM_PLAN_DGRAD_ROWS_PER_LAYER = 1,   /* k_loss_seed + a row-owned launch per layer (csrc/dgrad_rows.h) */
       SDRM_PLAN_DGRAD_CHAIN = 2,            /* the seeds and every layer in one row-owned launch */
       SDRM_PLAN_DGRAD_SKINNY_OWN = 3 };     /* inside the narrow nets' backward kernel */
enum { SDRM_SAMPLE_PATH_SKINNY = 0,      /* the narrow nets' one launch for the whole loop (csrc/skinny.h) */
       SDRM_SAMPLE_PATH_PERSIST = 1,     /* reverse steps without kernel boundaries (csrc/sample_persist.h) */
       SDRM_SAMPLE_PATH_PER_LAYER = 2 }; /* one launch per layer */
int sdrm_debug_last_plan(const sdrm_engine* e, int* train_path, int* parts, int* dgrad, int* sample_path);
/* What the last train forward staged, read only (every kernel path leaves both: the staging of a step is one definition, csrc/train_math.h):
 * staged [3][B][L] float32 - the layer-0 inputs of the P, S and Q pass (q_sample and the three dropout masks applied), in user order
 * whatever the stacked row order of the path - and t [B] int32, the users' timesteps; DEVICE pointers, either may be NULL.  Enqueued
 * on `stream`; SDRM_ERR_STATE before the first forward.  Valid until the next train forward on the handle (the backward reads, never
 * writes, what this returns). */
int sdrm_debug_get_staged(const sdrm_engine* e, float* staged, int* t, void* stream);

/* Gradient all-reduces of sdrm_train_step_sharded: 1 (default) = one all-reduce of the whole flat gradient after the one-call
 * backward; 2 = the two buckets of sdrm_grad_buckets, the first overlapped with the upper layers' weight gradients on the
 * auxiliary stream (pays when the first bucket's all-reduce takes longer than the ~40 us the hand-offs cost); also env
 * SDRM_AR_BUCKETS.  The result is the same bit for bit. */
int sdrm_debug_set_gradient_buckets(sdrm_engine* e, int buckets);

/* The on-device generator's draws as the staging kernels consume them (csrc/philox.h): for rows row0 .. row0 + rows - 1 and column
 * quads 0 .. quads - 1, one Philox4x32-10 call keyed by (seed, step, purpose) each: normals [rows, 4 * quads] float32 (two
 * Box-Muller pairs per call) and, when lowbits is not NULL, [rows, 4 * quads] uint8 holding bits 0..2 of the call's four words
 * (the dropout keep bits of the three passes of a train step).  purpose: 1 = train step elements, 3 = sampling start noise,
 * 4 | (i << 8) = reverse step i.  For the statistical tests of the generator (tests/test_philox_stats.py). */
int sdrm_debug_philox_draws(sdrm_engine* e, uint64_t seed, uint32_t purpose, uint32_t step, int64_t row0, int rows, int quads,
                            float* normals, uint8_t* lowbits, void* stream);

/* The engine's ncclComm_t (NULL without one): lets a test hand a communicator made elsewhere to sdrm_allreduce_init. */
void* sdrm_debug_comm_handle(const sdrm_engine* e);

/* Host-side planning of a split-K weight-gradient launch with the default settings (no device work): for a reduction
 * over `rows` stacked rows into ONE [n_out, k_in] gradient, the number of K-slices (slabs) and the rows per slice the
 * engine would use (a step's gradients are planned together: one slice count for all - one round of the resident
 * work-groups when that gives eight slices or more of at most 1024 rows, else about 2.2 rounds).  Invariants: rows_per_slice is a multiple of 32, slices * rows_per_slice >= rows > (slices - 1) *
 * rows_per_slice, slices <= 64, at least four K-steps of 32 rows per slice when the rows allow, and slices * tiles does not
 * exceed the 2816 work-group target unless a single slice already does. */
int sdrm_debug_plan_wgrad(int rows, int n_out, int k_in, int* slices, int* rows_per_slice);

/* C[M,N] = A[M,K] * B^T (variant 0, B is [N,K]), A * B (variant 1, B is [K,N]), A^T * B (variant 2, A is [K,M], B is
 * [K,N]) through the same MFMA kernel the engine uses, on tile shape `cfg` (0..4).  All dims must be multiples of 32.
 * Stages the operands in zero-padded scratch and synchronises. */
int sdrm_debug_gemm(int variant, int cfg, const float* A, const float* B, float* C, int M, int N, int K, void* stream);
/* Same kernel timed: `reps` launches on zero-filled scratch operands, mean microseconds per launch by HIP events on
 * `stream` (tools/gemm_tune.py). */
int sdrm_debug_gemm_time(int variant, int cfg, int M, int N, int K, int reps, float* us_out, void* stream);

/* The host side of sdrm_svd_fit that needs no device: SDRM_OK, or SDRM_ERR_SHAPE for a call outside its envelope (k < 1, k + 10 > 32,
 * min of m and n below 32, m or n above 2^22, nnz outside 0 .. 2^40 - 1, n_iter outside 0 .. 10000). */
int sdrm_debug_svd_args(int64_t m, int64_t n, int64_t nnz, int k, int n_iter);
/* The same of sdrm_csr_transpose: SDRM_ERR_SHAPE for m or n outside 1 .. 2^22, capacity outside 0 .. 2^40 - 1, or a bit table of
 * ceil(m / 64) x n words above 2^26. */
int sdrm_debug_csr_transpose_args(int64_t m, int64_t n, int64_t capacity);
/* The mark pass of the CSR transpose, csrc/csr_transpose.h: 0 (default) by the matrix's width - column tiles in LDS up to 9 tiles of
 * 4096 columns, 64-bit global atomics beyond -, 1 always global atomics, 2 always LDS tiles.  The result is the same bytes. */
int sdrm_debug_set_csrt_mark(sdrm_engine* e, int mode);
/* One stage of the fit on the caller's panels (csrc/svd_eval.h), for the stage tests: y_prod [n_rows, 32] = A q for the CSR matrix
 * A [n_rows, n_cols] (data null: all ones; hand in the CSC arrays with n_rows and n_cols swapped for the product with the transpose) and
 * q [n_cols, 32]; y_orth [n_rows, 32] = y_prod orthonormalised (CholeskyQR twice).  All three panels float32 on the device, 16-byte
 * aligned.  Synchronises `stream`; a breakdown is SDRM_ERR_ARG as in the fit (y_orth is then all zeros). */
int sdrm_debug_svd_stage(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t n_cols,
                         int64_t nnz, const float* q, float* y_prod, float* y_orth, void* stream);

/* The host side of sdrm_neumf_scores that needs no device: SDRM_OK, or SDRM_ERR_SHAPE for a call outside its envelope (factor outside
 * {8, 16, 32}, a table without rows, no listed user or item, more than 2^20 - 16 listed users, more than 2^22 listed items, users x items at or
 * above 2^40). */
int sdrm_debug_neumf_args(int n_users, int n_items, int factor, int64_t listed_users, int64_t listed_items);

/* The host side of sdrm_neumf_train_steps that needs no device: SDRM_OK, SDRM_ERR_SHAPE for a call outside its envelope (factor outside
 * {8, 16} - 32 is not built for training -, a table without rows, n outside 1 .. 2^31 - 1, batch outside 1 .. 1024), or SDRM_ERR_ARG
 * (step0 < 0, p_drop outside [0, 1) or not a number). */
int sdrm_debug_neumf_train_args(int n_users, int n_items, int factor, int64_t n, int batch, int64_t step0, float p_drop);

/* The host side of sdrm_neumf_epoch_draw that needs no device: SDRM_OK, or SDRM_ERR_SHAPE for a call outside its envelope (n outside
 * 2 .. 2^30, n_hold outside 1 .. n - 1, capacity below 2 (n - n_hold), with_present != 0 and n_users < 1). */
int sdrm_debug_neumf_draw_args(int64_t n, int64_t n_hold, int64_t capacity, int with_present, int n_users);

/* The host side of sdrm_neumf_triples that needs no device: SDRM_OK, SDRM_ERR_ARG (null parts, a part with a null indptr, or with null
 * indices and capacity > 0) or SDRM_ERR_SHAPE for a call outside its envelope, as listed at sdrm_neumf_triples.  The part's pointers are
 * compared with null only, never followed. */
int sdrm_debug_neumf_triples_args(const sdrm_triple_part* parts, int n_parts, int n_items, int64_t capacity_out);

/* The host side of sdrm_neumf_rank_problem that needs no device: SDRM_OK, SDRM_ERR_ARG (null parts, a part with a null indptr, or with
 * null indices and capacity > 0) or SDRM_ERR_SHAPE for a call outside its envelope, as listed at sdrm_neumf_rank_problem.  The part's
 * pointers are compared with null only, never followed. */
int sdrm_debug_neumf_rank_args(const sdrm_triple_part* parts, int n_parts, int n_items, int64_t n_heldout, int64_t n_rows, int64_t capacity_cols,
                               int64_t capacity_seen, int64_t capacity_relevant);

/* The host side of sdrm_mlp_train_steps that needs no device: SDRM_OK, SDRM_ERR_SHAPE for a call outside its envelope (n_items outside
 * 1 .. 36864, n_users < 2, batch outside 1 .. 16, n outside 1 .. 2^31 - 1, step0 < 0, p_drop outside [0, 1) or not a number), or
 * SDRM_ERR_ARG: with_grads for more than one step (n > batch) and, when `addr` is given - the base addresses of p[9], m[9], v[9] and, with
 * with_grads, of the nine gradient tensors, n_addr = 27 or 36 of them - a null address, one off the 16-byte grid, two tensors that share a
 * byte, or another n_addr. */
int sdrm_debug_mlp_train_args(int n_users, int n_items, int64_t n, int batch, int64_t step0, float p_drop, int with_grads, const uint64_t* addr,
                              int n_addr);

/* The host side of sdrm_mlp_eval that needs no device: SDRM_OK, or SDRM_ERR_SHAPE for a call outside its envelope (n_items outside 1 .. 36864,
 * n_users < 2, batch outside 1 .. 4096, n < 1, n_rows < 1, nnz < 0, without a row list - rows_listed == 0 - a range row0 .. row0 + n - 1 that
 * starts below 0 or ends behind n_rows, n x n_items at or above 2^40, neither with_out nor with_sse, and, when `addr` is given - the base
 * addresses of the nine tensors, n_addr = 9 - one off the 16-byte grid); SDRM_ERR_ARG for a null address or another n_addr. */
int sdrm_debug_mlp_eval_args(int n_users, int n_items, int64_t nnz, int64_t n_rows, int rows_listed, int64_t row0, int64_t n, int batch, int with_out,
                             int with_sse, const uint64_t* addr, int n_addr);

#ifdef __cplusplus
}
#endif
#endif /* SDRM_HIP_DEBUG_H */
