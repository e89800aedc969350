/*
 * sdrm_hip.h — C ABI of libsdrm_hip.so, the MI355X (gfx950) denoising engine for SDRM.
 *
 * The reference (Multi-resolution-diffusion-recommender/SDRM) is pure Python on PyTorch and has
 * no FFI layer; the boundary this library replaces is the Python call surface of
 * /root/reference/train_SDRM.py as consumed by main.py:148-175 and
 * hyperparameter_search.py:147,386,691.  Each entry point below cites the
 * reference lines whose device work it replaces.  The Python shim that keeps the
 * reference's names (`train_SDRM`, `sample_ddpm`, `SDRM.forward`, ...) lives in
 * sdrm_amd/train_SDRM.py and binds these symbols with ctypes.
 *
 * Conventions
 *  - Every `const float*` / `float*` / `const int64_t*` / `const uint8_t*` argument whose name does
 *    not end in `_host` is a DEVICE pointer owned by the caller (e.g. `tensor.data_ptr()` of a
 *    contiguous ROCm torch tensor).  The library owns only handle-internal buffers and never
 *    allocates in a step call.
 *  - `stream` is a `hipStream_t` passed as `void*` (NULL = the default stream).  All work is
 *    enqueued on it and nothing synchronises unless stated.  It may be a non-blocking stream with work of the caller's still
 *    pending, beside a busy default stream: inputs need only be ready in `stream` order, and outputs are final in `stream` order
 *    (tests/test_stream_order.py holds every entry point to this).  One exception covers every entry point with library-owned,
 *    grow-only scratch: a call whose scratch must GROW - the first one of its family on a handle, and each larger one - waits for
 *    the device before it frees the old buffer and for the zeroing of the new one; a call that fits does not wait.
 *  - All arithmetic is fp32; `t` / `Tj` are int64 as in the reference (`torch.randint`, :327).
 *  - Return value: 0 on success, negative `sdrm_status` otherwise; never throws.  The message of the
 *    last failure on a handle is returned by sdrm_last_error().
 *  - A handle is not thread-safe; distinct handles are independent: all tile / path selection state lives in the
 *    handle (read from the SDRM_* environment variables once, in sdrm_create), none of it is process-global.
 *  - Test and tuning hooks (sdrm_debug_*) are declared in sdrm_hip_debug.h, not here.
 *
 * Parameter order of every "flat" vector (P floats) = SDRM.named_parameters() of the reference
 * (train_SDRM.py:86-95):
 *   emb_layer.weight[T,T] emb_layer.bias[T] dnn.0.weight[W,L+T] dnn.0.bias[W] dnn.1.weight[1]
 *   (H>=1: dnn.2.weight[W,W] dnn.2.bias[W] dnn.3.weight[1])  dnn.{2+2H}.weight[L,W] dnn.{2+2H}.bias[L]
 * The H hidden layers share ONE weight/bias/slope (train_SDRM.py:94, quirk Q1).
 */
#ifndef SDRM_HIP_H
#define SDRM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdrm_engine sdrm_engine;

enum sdrm_status {
  SDRM_OK = 0,
  SDRM_ERR_ARG = -1,    /* null pointer / bad enum */
  SDRM_ERR_SHAPE = -2,  /* rows > max_rows, L/W/T/H outside the supported envelope */
  SDRM_ERR_HIP = -3,    /* a HIP runtime call failed */
  SDRM_ERR_STATE = -4,  /* call order violated (e.g. backward before forward) */
  SDRM_ERR_NOMEM = -5,
  SDRM_ERR_RCCL = -6,   /* librccl could not be loaded, or an RCCL call failed */
  SDRM_ERR_DEVICE = -7  /* the device is not the chip this library is built for (gfx950, 256 compute units) */
};

/* Where the randomness of a call comes from (SURVEY.md §8b "two RNG modes"). */
enum sdrm_rng_mode {
  SDRM_RNG_EXPLICIT = 0, /* caller supplies noise / t / dropout keep-masks / z (parity mode) */
  SDRM_RNG_PHILOX = 1    /* counter-based Philox4x32-10 keyed by (seed, step, GLOBAL row, column) */
};

/* Explicit randoms of one train step.  Replaces the draws at train_SDRM.py:326-327 and the three
 * F.dropout masks of :100 (one per forward pass, order P, S, Q — :331, :193, :195). */
typedef struct sdrm_train_randoms {
  const float* noise;    /* [B,L] eps, ALREADY multiplied by noise_divider (:326) */
  const int64_t* t;      /* [B] timesteps in 1..T (:327) */
  const uint8_t* keep;   /* [3,B,L] 1 = element survives dropout (then scaled by 2) */
} sdrm_train_randoms;

/* ---- lifetime ------------------------------------------------------------------------------- */

/* Builds an engine for an eps-predictor SDRM(N_ITEMS=L, EMB_DIM=T, LATENT_DIM=W, n_hidden_layers=H)
 * (train_SDRM.py:86-95, :305) able to process up to max_rows rows per call, with Adam state
 * (train_SDRM.py:309) and the DDPM schedule for beta1=1e-4, beta2=0.02 (train_SDRM.py:275-276,
 * 300-303).  Parameters start at zero: call sdrm_set_params.  Envelope: 1<=L,W<=4096, 2<=T<=1020,
 * 0<=H<=16 (the reference's search space, hyperparameter_search.py:103-113, is L=W<=1000, T<=198, H<=5).
 * The device must be a gfx950 with 256 compute units (MI355X in SPX mode): the one-round launches (one work-group per CU) and
 * the work-group -> XCD mapping are sized for it, anything else is refused with SDRM_ERR_DEVICE rather than run mis-balanced. */
int sdrm_create(int L, int W, int T, int H, int max_rows, int device_id, sdrm_engine** out);
int sdrm_destroy(sdrm_engine* e);
const char* sdrm_last_error(const sdrm_engine* e);
int64_t sdrm_param_count(const sdrm_engine* e);

/* ---- schedule (train_SDRM.py:296-303; module globals b_t/a_t/ab_t, quirk Q10) ---------------- */
/* sdrm_set_schedule takes no stream: it WAITS FOR THE DEVICE (every stream), then rewrites the tables with blocking copies.  Work queued
 * before the call, on any stream, uses the old schedule; work queued after it the new one.  A once-per-run call. */
int sdrm_set_schedule(sdrm_engine* e, float beta1, float beta2);
/* Copies beta, alpha, alpha-bar ([T+1] each) to HOST arrays. */
int sdrm_get_schedule(const sdrm_engine* e, float* beta_host, float* alpha_host, float* alphabar_host);

/* ---- parameters / optimiser state (nn.Module.state_dict / torch.optim.Adam state) ------------ */
int sdrm_set_params(sdrm_engine* e, const float* flat, void* stream);
int sdrm_get_params(const sdrm_engine* e, float* flat, void* stream);
/* The live parameters in place: DEVICE pointer to the library's flat master vector [P] (what nn.Module.parameters() hands out in
 * the reference, hyperparameter_search.py:53: views, not copies).  Valid until sdrm_destroy.  READ-ONLY for the caller: the
 * kernels read padded / transposed / fragment-packed compute copies that only sdrm_set_params and the train step refresh. */
const float* sdrm_params_ptr(const sdrm_engine* e);
/* Gradient of the last backward, flat [P] (what autograd leaves in p.grad after :336).  If that backward was
 * given a caller buffer (`grad`), this reads from it: the buffer must still be alive. */
int sdrm_get_grads(const sdrm_engine* e, float* flat, void* stream);
/* Adam first/second moments, flat [P] each, and the global step counter (Q8). */
int sdrm_get_adam_state(const sdrm_engine* e, float* exp_avg, float* exp_avg_sq, int64_t* step_host, void* stream);
int sdrm_set_adam_state(sdrm_engine* e, const float* exp_avg, const float* exp_avg_sq, int64_t step, void* stream);
int sdrm_adam_reset(sdrm_engine* e, void* stream);

/* ---- training step, split in the three phases the user-sharded (multi-GPU) step needs --------- *
 * Replaces train_SDRM.py:326-337 for one batch of B rows (this rank's shard).
 *
 * (1) sdrm_train_forward: q_sample (:203,:328) + the three eps-net forwards P=f(x_pert,t),
 *     S=f(x0,t), Q=f(x0+0.1*eps,t) (:331,:193-195) + the rank-local partial sums of the loss
 *     (:196-198): sums[0..4] = { sum D^2, sum (R-S)^2, sum R, sum R^2, count } in float64, where
 *     R = P-x0, D = (Q-S)/mu^2 - R.  Multi-GPU callers all-reduce(sum) these 5 doubles.
 *     row0 = global index of this shard's first row (keys the Philox streams; 0 on one GPU),
 *     seed/step key the PHILOX mode; `rnd` is used in EXPLICIT mode (may be NULL in PHILOX mode).
 * (2) sdrm_train_backward: loss value (:198) and closed-form gradient seeds from the GLOBAL sums,
 *     backward through the three passes, gradient accumulation over passes and over the H shared
 *     hidden applications; writes this rank's flat gradient [P] to `grad` (device; may be NULL to
 *     keep it internal) and the global loss to `loss` (device float; may be NULL).  Multi-GPU
 *     callers all-reduce(sum) `grad`.
 * (3) sdrm_adam_step: torch.optim.Adam(lr, betas=(0.9,0.999), eps=1e-8, weight_decay=1e-4) with
 *     coupled L2 (:309, :337), on `grad` (device, flat [P]; NULL = the internal gradient).
 *     lr is the caller's per-epoch value DIFF_LR*(1-ep/EPOCHS) (:316).
 */
int sdrm_train_forward(sdrm_engine* e, const float* x0, int B, int64_t row0, int mode,
                       const sdrm_train_randoms* rnd, uint64_t seed, uint64_t step, float noise_divider,
                       double* sums, void* stream);
int sdrm_train_backward(sdrm_engine* e, const double* sums, float* grad, float* loss, void* stream);
/* Phase 2 in two calls, for callers that overlap the gradient exchange with the backward (no reference
 * counterpart: the reference is single-device).  `begin` runs the loss seeds, the dgrad chain, the layer-0
 * weight gradient and the embedding backward and finalises the FIRST bucket of `grad` in `stream` order; `finish`
 * runs the weight gradients of the upper layers and finalises the SECOND bucket.  sdrm_grad_buckets returns the two [offset, length) ranges of the flat gradient (first: emb_layer.*,
 * dnn.0.weight, dnn.0.bias; second: everything from dnn.1 (the first PReLU slope) on).  Same `grad` in both calls.
 * sdrm_train_backward == begin + finish. */
int sdrm_train_backward_begin(sdrm_engine* e, const double* sums, float* grad, float* loss, void* stream);
int sdrm_train_backward_finish(sdrm_engine* e, float* grad, void* stream);
int sdrm_grad_buckets(const sdrm_engine* e, int64_t* first_off, int64_t* first_len, int64_t* second_off,
                      int64_t* second_len);
int sdrm_adam_step(sdrm_engine* e, const float* grad, float lr, void* stream);
/* Single-GPU convenience: (1)+(2)+(3) back to back on `stream`. */
int sdrm_train_step(sdrm_engine* e, const float* x0, int B, float lr, int mode, const sdrm_train_randoms* rnd,
                    uint64_t seed, uint64_t step, float noise_divider, float* loss, void* stream);
/* ---- multi-GPU: the user-sharded train step with its exchange inside the library ---------- *
 * No reference counterpart (the reference is single-device, train_SDRM.py:18): rows (users) of the global batch are
 * partitioned over one process per GPU; parameters, Adam state and schedule are replicated.  Per step two things cross
 * GPUs, both as RCCL all-reduce(sum) issued by the library itself: the 5 float64 loss sums (var(R) and both mse means of
 * train_SDRM.py:196-198 are over the GLOBAL batch) and the flat gradient [P] - by default in one all-reduce after the
 * backward; optionally (sdrm_hip_debug.h) in the two buckets of sdrm_grad_buckets, the first one overlapped with the upper
 * layers' weight gradients on an auxiliary stream.  Sampling needs no exchange.
 *
 * librccl is loaded at run time (dlopen "librccl.so.1", or $SDRM_RCCL_LIB); a process that already holds one - e.g. a
 * PyTorch process - shares that instance.  Either
 *   sdrm_comm_unique_id (rank 0; ship the 128 bytes to the other ranks by any channel) + sdrm_comm_init_rank (all ranks;
 *   the library owns the communicator), or
 *   sdrm_allreduce_init (adopts a ncclComm_t the caller made with the same librccl; not destroyed by the library).
 * aux_stream: a hipStream_t for the overlapped bucket (NULL = the library creates one). */
enum { SDRM_COMM_ID_BYTES = 128 };
int sdrm_comm_unique_id(void* id_host);
/* 1 when librccl can be resolved in this process (what sdrm_comm_unique_id / sdrm_comm_init_rank need), else 0: a purely local
 * check, so that the ranks of a job can agree on the exchange BEFORE any of them enters the collective ncclCommInitRank. */
int sdrm_comm_available(void);
int sdrm_comm_init_rank(sdrm_engine* e, int nranks, int rank, const void* id_host);
int sdrm_allreduce_init(sdrm_engine* e, void* rccl_comm, void* aux_stream);
int sdrm_comm_info(const sdrm_engine* e, int* nranks, int* rank);   /* nranks 0 / rank -1: no communicator */
int sdrm_comm_destroy(sdrm_engine* e);                             /* also done by sdrm_destroy */
/* sdrm_train_forward (this rank's rows, first global row row0) -> all-reduce of the loss sums -> sdrm_train_backward ->
 * all-reduce of the flat gradient -> sdrm_adam_step (two-bucket form: sdrm_train_backward_begin -> all-reduce of the first
 * bucket beside sdrm_train_backward_finish -> all-reduce of the second bucket -> sdrm_adam_step).
 * `loss` (device float, may be NULL) receives the GLOBAL loss.  With one rank it equals sdrm_train_step bit for bit. */
int sdrm_train_step_sharded(sdrm_engine* e, const float* x0, int B, int64_t row0, float lr, int mode,
                            const sdrm_train_randoms* rnd, uint64_t seed, uint64_t step, float noise_divider, float* loss,
                            void* stream);
/* Outputs of the last sdrm_train_forward: P,S,Q as [3,B,L] (parity tests). */
int sdrm_get_train_outputs(const sdrm_engine* e, float* psq, void* stream);

/* ---- plain forward: SDRM.forward(x, t) (train_SDRM.py:97-103), dropout always on (Q2) ---------- *
 * keep [n,L] (EXPLICIT) or Philox(seed, step, row0+row, col).  Used by callers that run their own
 * sampler (hyperparameter_search.py:67,78). */
int sdrm_forward(sdrm_engine* e, const float* x, const int64_t* t, int n, int mode, const uint8_t* keep,
                 uint64_t seed, uint64_t step, int64_t row0, float* out, void* stream);

/* ---- reverse sampling: sample_ddpm latent loop (train_SDRM.py:37-59) + denoise_add_noise (:20-25) *
 * Runs i = T..1 over n rows and writes the final latents x_0 to out[n,L] (the caller then applies
 * vae.decode, :49/:61).  Tj == NULL -> full resolution (:50-59).  Tj != NULL -> multi-resolution
 * (:37-48): row j runs i = Tj[j]..1; rows are independent, so this equals the reference's per-user
 * batch-1 loop (Q11).  EXPLICIT mode: xT[n,L] start noise (:38/:51), z[T+1,n,L] with z[i] the noise
 * injected at step i ALREADY multiplied by noise_divider (z[1] is ignored: no noise at i==1, Q9),
 * keep[T+1,n,L] dropout keep-masks per step.  PHILOX mode: all of those (and Tj when
 * `multires` != 0) are drawn on device; Tj_out (device int64 [n], may be NULL) receives the drawn
 * start steps.  A caller's Tj (EXPLICIT mode, Tj != NULL) is read back to order the rows on the host: that one form synchronises
 * `stream` once, in sdrm_sample / sdrm_sample_begin; no other form of the call waits. */
int sdrm_sample(sdrm_engine* e, int n, float noise_divider, int multires, int mode, const float* xT,
                const float* z, const uint8_t* keep, const int64_t* Tj, uint64_t seed, uint64_t call_id,
                int64_t row0, float* out, int64_t* Tj_out, void* stream);

/* The same loop in resumable form (sdrm_sample == begin + steps(all) + end).  A sampling call uses the parameters as
 * they are at sdrm_sample_begin (the sampler reads its own snapshot of the net; a narrow net's whole reverse loop is one launch
 * that sdrm_sample_begin itself issues): sdrm_set_params or train steps issued after the begin, between its sdrm_sample_steps
 * calls, do not change its result.  The streams of the begin / steps / end calls of one sampling call must be the same or
 * ordered by the caller.  The EXPLICIT-mode pointers must stay valid until sdrm_sample_end.  sdrm_sample_steps runs at most `count` reverse
 * steps; sdrm_sample_remaining returns the next step index i (0 = loop finished).
 * The steps are queued, not necessarily on `stream`: the engine runs row ranges of a call as chains of launches on streams of its own
 * (ordered after everything queued on `stream` at the first sdrm_sample_steps; folded back into `stream` by sdrm_sample_end and by every
 * other entry point that touches the sampler's state), so a train step queued between two sdrm_sample_steps calls may execute beside
 * the call's launches.  Neither sees the other: the call's result and the train steps' are those of the sequential order, bit for bit. */
int sdrm_sample_begin(sdrm_engine* e, int n, float noise_divider, int multires, int mode, const float* xT,
                      const float* z, const uint8_t* keep, const int64_t* Tj, uint64_t seed, uint64_t call_id,
                      int64_t row0, int64_t* Tj_out, void* stream);
int sdrm_sample_steps(sdrm_engine* e, int count, void* stream);
int sdrm_sample_remaining(const sdrm_engine* e);
int sdrm_sample_end(sdrm_engine* e, float* out, void* stream);

/* One reverse step on caller-owned state, for callers that drive the loop themselves:
 * x <- denoise_add_noise(x, i, f(x, i), z) (train_SDRM.py:56-59).  z may be NULL (= 0, the i==1 case). */
int sdrm_reverse_step(sdrm_engine* e, float* x, int n, int i, const float* z, const uint8_t* keep, void* stream);

/* q_sample alone: perturb_input(x, t, noise) (train_SDRM.py:202-203). */
int sdrm_perturb_input(sdrm_engine* e, const float* x, const int64_t* t, const float* noise, int n, float* out,
                       void* stream);

/* Pre-activations of eps-net layer `layer` (0..H) from the last sdrm_train_forward, as [3,B,W]
 * (pass order P,S,Q).  Parity tests use their signs to evaluate the oracle with the same PReLU
 * derivative choice at pre-activations that are zero within fp32 rounding (DESIGN.md "kink flips").
 * Valid from that forward until the parameters change: some paths keep activations only and rebuild the
 * pre-activations from the PReLU slopes of the forward, so after sdrm_adam_step, a whole sdrm_train_step /
 * sdrm_train_step_sharded (their tail applies Adam) or sdrm_set_params the call returns SDRM_ERR_STATE
 * and writes nothing - on every path, whether that forward stored them or not. */
int sdrm_get_preacts(const sdrm_engine* e, int layer, float* out, void* stream);

/* ---- introspection for bench.py / profiling ---------------------------------------------------- */
/* Per-kernel timing with HIP events recorded on the launch stream around every GEMM launch.
 * sdrm_profile_begin enables it (capacity = max launches recorded), sdrm_profile_end synchronises the
 * stream and aggregates per kernel class; sdrm_profile_get returns, for class `cls`
 * (0..sdrm_profile_classes()-1), the summed duration [ms], the launch count and the summed
 * ALGORITHMIC flops (2*rows*N*K on the unpadded dims).  Adds two event records per launch, so it is
 * used in a separate pass, never inside the throughput-timed region. */
int sdrm_profile_begin(sdrm_engine* e, int capacity);
/* Restricts the bracketing to ONE kernel class (cls < 0: all classes again).  Every bracketed launch puts two marker packets on
 * the stream, and the markers of neighbouring launches inflate each other's intervals (+3..5 us per launch, +10 us on the
 * largest one): bench.py finds the dominant class with all classes bracketed, then times that class alone. */
int sdrm_profile_only(sdrm_engine* e, int cls);
int sdrm_profile_end(sdrm_engine* e, void* stream);
int sdrm_profile_classes(void);
const char* sdrm_profile_name(int cls);
int sdrm_profile_get(const sdrm_engine* e, int cls, double* total_ms, int64_t* launches, double* flops);

/* Kernel launches issued through this handle since sdrm_create (memcpy / memset nodes not counted): bench.py reports
 * launches per step beside the roofline of the latency-bound configurations. */
int64_t sdrm_launch_count(const sdrm_engine* e);
/* Name of the GEMM kernel variant family in use and tile geometry, as a static string. */
const char* sdrm_build_info(void);
/* Hex SHA-256 of the sources this binary was compiled from (sdrm_amd/csrc/ and include/, as sdrm_amd/_build.py hashes
 * them).  The Python loader refuses, or rebuilds, a library whose hash differs from the sources next to it. */
const char* sdrm_source_hash(void);
/* Sparse batch feed (reference: dataloaders.py:46-79 builds a COO tensor per batch on the host, train_SDRM.py:323
 * densifies it before vae.encode).  The CSR matrix of the whole feed [n_rows, n_items] stays on the device (int64
 * indptr, int32 column indices, float32 data or null for all-ones); out [b, n_items] float32 receives the dense rows
 * rows[0..b) (device int64 array; the caller's epoch permutation) or, when rows is null, rows row0 .. row0+b-1
 * (checked on the host against n_rows).  The caller's CSR is not trusted with the address of a store: on the device every
 * row id is checked against [0, n_rows), every indptr pair for order, every column index against [0, n_items); an offending
 * row / entry is left zero and recorded in the handle's feed status word, which sdrm_feed_status reports. */
int sdrm_csr_rows_to_dense(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows,
                           const int64_t* rows, int64_t row0, int b, int n_items, float* out, void* stream);
/* SDRM_OK, or SDRM_ERR_ARG (message: what was out of range) if any sdrm_csr_rows_to_dense launch since the last call met an
 * out-of-range row id, indptr pair or column index; clears the record.  Synchronises `stream` (call it once per epoch, not per
 * batch). */
int sdrm_feed_status(sdrm_engine* e, void* stream);

/* Equal-sparsity binarisation of sampled data on the device (reference: main.py:177-180,
 *   threshold = np.quantile(M.flatten(), SPARSITY); M_equal_sparsity = (M >= threshold)):
 * x [n] float32 (the flattened [users, items] matrix, 16-byte aligned), q in [0,1].  threshold (device float*, may
 * be null) receives exactly what np.quantile (numpy 2.x, method "linear": float32 virtual index, float32 lerp
 * between the two neighbouring order statistics) returns for a float32 array; out (device uint8[n], 4-byte
 * aligned, may be null) receives x >= threshold.  Inputs must not contain NaN. */
int sdrm_equal_sparsity(sdrm_engine* e, const float* x, int64_t n, double q, uint8_t* out, float* threshold, void* stream);
/* The same result as a canonical CSR matrix made on the device, either side (reference: main.py:177-180 and the NeuMF branch's
 * other tail, :259-270, `(F <= np.quantile(F.flatten(), 1 - SPARSITY))`, both turned into csr_matrix / (row, col) form downstream):
 * x [n_rows, n_cols] float32 row-major (16-byte aligned at its base; rows need not be), q in [0,1], side 0: x >= threshold,
 * side 1: x <= threshold, threshold exactly sdrm_equal_sparsity's.  No dense matrix exists: one sweep over x writes a bit mask
 * (ceil(n_cols / 64) 64-bit words per row, engine workspace, grow-only) and integer row counts, a scan makes indptr, and the
 * column indices are written from the mask alone.  No data array: the matrix is all ones (the convention of the CSR inputs above).
 * The call is split because nnz is not bounded by the rank (ties at the threshold add any number of elements):
 * sdrm_equal_sparsity_csr_begin computes the threshold (device float*, may be null), the mask and indptr (device int64
 *   [n_rows + 1]), synchronises `stream` ONCE and returns nnz = indptr[n_rows] in *nnz_host (host) - 8 bytes read back
 *   instead of n_rows x n_cols.  A second begin replaces a pending one.  SDRM_ERR_SHAPE: n_rows < 1, n_cols outside [1, 2^31),
 *   or more than 2^31 mask words; SDRM_ERR_ARG: a null pointer, q outside [0,1], side outside {0, 1}, x not 16-byte aligned.
 * sdrm_equal_sparsity_csr_end fills indices[0 .. nnz) (device int32; ascending columns within a row, rows in order) from the
 *   pending mask and ends the call; no store lands outside [0, nnz).  SDRM_ERR_STATE without a pending begin; SDRM_ERR_ARG if
 *   capacity < nnz (nothing is written and the begin stays pending).  Inputs must not contain NaN. */
int sdrm_equal_sparsity_csr_begin(sdrm_engine* e, const float* x, int64_t n_rows, int64_t n_cols, double q, int side,
                                  int64_t* indptr, float* threshold, int64_t* nnz_host, void* stream);
int sdrm_equal_sparsity_csr_end(sdrm_engine* e, int32_t* indices, int64_t capacity, void* stream);

/* A device-resident CSR matrix [n_rows, n_cols] to its CSC form, the CSR of the transpose (csrc/csr_transpose.h).  The input's
 * contract is sdrm_csr_rows_to_dense's: device arrays, data null for all ones.  `capacity` is the number of elements of indices (and
 * of data, rowidx and cdata).  indptr holds absolute offsets and need not start at 0: a row range of a larger matrix is a pointer
 * offset.  Columns within a row must be distinct; they need not be sorted.
 *   colptr [n_cols + 1] (device int64) starts at 0; rowidx (device int32) ascends within every column and cdata[q] is the value of the
 *   entry rowidx[q] names; cdata is null exactly when data is.  For a canonical input this is what scipy's tocsc() + sort_indices()
 *   gives, byte for byte.  Elements at and behind colptr[n_cols] are unspecified.
 * The result is the same from call to call and does not depend on what earlier calls left in scratch (a bit table of
 * ceil(n_rows / 64) x n_cols 64-bit words and as many 4-byte offsets, library-owned, grow-only, cleared on the stream by every call).
 * Integer atomics only.  Nothing is read back and nothing synchronises, except the device synchronise when the scratch must grow.
 * Range checks, into the status word sdrm_feed_status reports: an indptr pair that is negative, out of order or reaches behind
 * `capacity` makes its row contribute nothing; a column outside [0, n_cols) is skipped; a row that holds a column twice raises a
 * bit of its own - the output is then not the transpose.  No load or store uses an unchecked index, no store lands outside
 * [0, capacity) of rowidx / cdata or [0, n_cols] of colptr for any input.
 * Refused before any launch: SDRM_ERR_ARG for a null handle or required pointer, or values on one side only; SDRM_ERR_SHAPE for
 * n_rows or n_cols outside 1 .. 2^22, capacity outside 0 .. 2^40 - 1, or ceil(n_rows / 64) x n_cols above 2^26. */
int sdrm_csr_transpose(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t n_cols,
                       int64_t capacity, int64_t* colptr, int32_t* rowidx, float* cdata, void* stream);

/* Up to 8 device-resident CSR matrices of n_cols columns, one under the other (csrc/csr_transpose.h).  A part's indptr
 * [n_rows + 1] holds absolute offsets; its true entry count lives on the device (indptr[n_rows] - indptr[0]) and `capacity` is only
 * the size of its indices (and data) array - the convention of sdrm_holdout_split's outputs, which stack as they are.
 *   indptr_out [sum n_rows + 1] (device int64) starts at 0; the rows appear in part order with their entries in their own order.
 *   data_out is null when every part's data is null; otherwise it is required and an all-ones part contributes 1.0f.
 * Rows are checked the way sdrm_holdout_split checks them (the output may feed sdrm_rank_metrics): a row whose indptr pair is
 * negative, out of order, reaches behind its part's capacity or spans more than n_cols entries, and a row with a column outside
 * [0, n_cols), is EMPTY in the output and recorded in the status word sdrm_feed_status reports.  The parts' running bases are scanned
 * on the device: nothing is read back, nothing synchronises (except when the grow-only scratch of 12 bytes per row must grow).
 * No store lands outside [0, capacity_out).
 * SDRM_ERR_SHAPE: n_parts outside 1 .. 8, n_cols outside 1 .. 2^22, total rows outside 1 .. 2^22, capacity_out below the sum of the
 * parts' capacities (the host cannot know less); SDRM_ERR_ARG: a null pointer, or data_out not as described. */
typedef struct sdrm_csr_part {
  const int64_t* indptr; const int32_t* indices; const float* data;
  int64_t n_rows; int64_t capacity;
} sdrm_csr_part;
int sdrm_csr_vstack(sdrm_engine* e, const sdrm_csr_part* parts, int n_parts, int n_cols, int64_t* indptr_out, int32_t* indices_out,
                    float* data_out, int64_t capacity_out, void* stream);

/* The NeuMF evaluator's (user, item, label) triples from up to 8 device-resident CSR parts (reference: main.py:218-283, the frames of
 * the two tails of the synthetic matrix and of the validation users' training half, concatenated; csrc/neumf_triples.h; restated in
 * tests/neumf_triples_ref.py).  Only a part's PATTERN is read: indptr [n_rows + 1] holds absolute offsets and need not start at 0 (a row
 * range of a larger matrix is a pointer offset), `capacity` is the number of elements of indices, as in sdrm_csr_part.  Row r of a part
 * is user user0 + r, and every triple of a part carries the part's label, 0 or 1.
 * The order, which is the definition: the parts in the order given; within a part the rows ascending; within a row the entries in
 *   their stored order.  Entry j of row r of part p becomes the record (parts[p].user0 + r, indices[j], parts[p].label), three int32.
 *   triples_out [capacity_out][3] is dense - a row without entries, or an emptied one, leaves no hole - and rows m .. capacity_out - 1
 *   are left as they were.  It is the buffer sdrm_neumf_epoch_draw reads.
 * Row checks, exactly sdrm_csr_vstack's: a row whose indptr pair is negative, out of order, reaches behind its part's capacity or spans
 *   more than n_items entries is EMPTY in the output and raises the status word sdrm_feed_status reports under sdrm_csr_vstack's indptr
 *   bit; a row that holds a column outside [0, n_items) is EMPTY too and raises the column bit.  Should the checked lengths add up
 *   to more than capacity_out (parts whose rows share entries), the triples behind capacity_out are dropped, m is capacity_out and the
 *   indptr bit is raised.  No load or store uses an unchecked index; no store lands outside [0, capacity_out) of triples_out,
 *   [0, n_items) of item_present or [0, 4) of counts_dev, for any input.
 * counts_dev: DEVICE int64 [4], written by the call: m; the number of label-1 triples; max user + 1 and max item + 1 over the emitted
 *   triples (both 0 when m is 0) - what main.py:283 takes for n_users and n_items.
 * item_present: null, or DEVICE uint8 [n_items]: the call zeroes it and sets byte i for every emitted item i - the ranking's column list
 *   without the triples crossing to the host.
 * Three launches behind three memsets, all enqueued on `hip_stream` - the caller's stream, under the contract of every `stream` argument
 *   of this header (Conventions); nothing is read back and nothing synchronises (except the device
 *   synchronise when the grow-only scratch of 20 bytes per row must grow).  Integer atomics only, for the three counts behind m; the
 *   scratch is cleared on the stream by every call: the same bytes on every run, whatever earlier calls left behind.
 * Refused before any launch, nothing written: SDRM_ERR_ARG for a null handle, null parts, triples_out or counts_dev, a part with a null
 *   indptr, or with null indices and capacity > 0; SDRM_ERR_SHAPE for n_parts outside 1 .. 8, n_items outside 1 .. 2^22, total rows
 *   outside 1 .. 2^22 (a part may have none), a label outside {0, 1}, user0 < 0 or user0 + n_rows above 2^31 - 1, a negative capacity,
 *   capacity_out below the sum of the parts' capacities (the host cannot know less) or above 2^30 (sdrm_neumf_epoch_draw's bound on n). */
typedef struct sdrm_triple_part {
  const int64_t* indptr; const int32_t* indices;
  int64_t n_rows; int64_t capacity;
  int32_t user0; int32_t label;
} sdrm_triple_part;
int sdrm_neumf_triples(sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, int32_t* triples_out, int64_t capacity_out,
                       uint8_t* item_present, int64_t* counts_dev, void* hip_stream);

/* The NeuMF evaluator's ranking problem, built on the device from the parts sdrm_neumf_triples read (reference:
 * neural_cf_benchmark_pt.py:294-326, the testing block: the two merges in pandas and the two CSR matrices rebuilt through Python dicts;
 * here what sdrm_amd/neumf.py's RankingProblem.from_parts builds on the host with scipy - one csr + csr per part, np.isin, searchsorted,
 * sum_duplicates, sort_indices; csrc/neumf_rank.h; restated in tests/neumf_rank_ref.py).  parts / n_parts / n_items: as sdrm_neumf_triples
 * takes them, only the PATTERN is read.  item_present: DEVICE uint8 [n_items], the bytes that call wrote (any non-zero byte counts).
 * heldout: DEVICE int32 [n_heldout][3] (user, item, label), null only with n_heldout 0.  n_rows: the number of user ids.
 * The outputs, which are the definition:
 *   cols_out [capacity_cols >= n_items]: the item ids i with item_present[i] != 0, ascending, C of them; col_of[i] is the place of i in
 *     it, -1 for an absent item.  Elements C .. are left as they were.
 *   seen: a canonical CSR [n_rows, C], int64 indptr [n_rows + 1] from 0, int32 indices, no data; ROWS ARE DENSE BY USER ID, row u is user u:
 *     the ascending, duplicate-free union, over every part p with user0_p <= u < user0_p + n_rows_p, of col_of[] of the present items of
 *     that part's row u - user0_p, whatever the part's label.  A user no part covers has an empty row.  capacity_seen is at least the sum
 *     of the parts' capacities; elements behind indptr[n_rows] are left as they were.
 *   relevant: the same form from the held-out triples with label > 0 whose item is present, duplicates merged; capacity_relevant is at
 *     least n_heldout.  A triple, whatever its label, whose user is outside [0, n_rows) is dropped and raises the row bit of the status
 *     word sdrm_feed_status reports, one whose item is outside [0, n_items) is dropped and raises the column bit; a triple whose item is
 *     in range but absent is dropped silently, as the reference drops a held-out item that never occurs in training.
 * Part rows are checked exactly as sdrm_neumf_triples checks them - an indptr pair that is negative, out of order, reaches behind its
 *   part's capacity or spans more than n_items entries (sdrm_csr_vstack's indptr bit), a column outside [0, n_items) (the column bit) -
 *   and an offending row contributes nothing.  A part row with entries whose user is n_rows or above contributes nothing and raises the
 *   row bit.  Should part rows that share entries make seen longer than capacity_seen, the columns behind it are dropped, the count says
 *   capacity_seen and the indptr bit is raised.  No load or store uses an unchecked index.
 * counts_dev: DEVICE int64 [4], written by the call: C; seen's entries; relevant's entries; the held-out triples dropped for a range defect.
 * Order: two memsets (the scratch - two bit tables of n_rows x ceil(n_items / 64) 64-bit words over raw item ids and 20 bytes per user
 *   and 4 per item - and counts_dev) lead seven launches (six with n_heldout 0), all enqueued on `hip_stream` - the caller's stream, under the
 *   contract of every `stream` argument of this header (Conventions); nothing is read back and nothing synchronises (except the device
 *   synchronise when the grow-only scratch must grow).  64-bit integer atomic ORs into the cleared tables - one per run of a part row's
 *   entries that fall into one word, one per held-out triple - and one integer add: the same bytes on every run.
 * Refused before any launch, nothing written: SDRM_ERR_ARG for a null handle or pointer, a part with a null indptr, or with null indices
 *   and capacity > 0; SDRM_ERR_SHAPE for n_parts outside 1 .. 8, n_items, n_rows or the parts' total rows outside 1 .. 2^22, one bit table
 *   above 2^31 bytes, n_heldout outside 0 .. 2^30, a part as sdrm_neumf_triples refuses it (label, user0, n_rows, capacity), capacity_cols
 *   below n_items, capacity_seen below the sum of the parts' capacities, capacity_relevant below n_heldout. */
int sdrm_neumf_rank_problem(sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, const uint8_t* item_present,
                            const int32_t* heldout, int64_t n_heldout, int64_t n_rows, int32_t* cols_out, int64_t capacity_cols,
                            int64_t* seen_indptr, int32_t* seen_indices, int64_t capacity_seen, int64_t* relevant_indptr,
                            int32_t* relevant_indices, int64_t capacity_relevant, int64_t* counts_dev, void* hip_stream);

/* A ranking's users from a mask (reference: neural_cf_benchmark_pt.py:215-217, the users of the epoch's 20 %; here np.flatnonzero of the
 * bytes sdrm_neumf_epoch_draw leaves in `present`, on the device): users_out [n_rows] receives the ids u with mask[u] != 0, ascending,
 * U of them (elements U .. are left as they were), and count_dev, DEVICE int64 [1], receives U.  One launch of one work-group on
 * `hip_stream` (the caller's stream, as above); nothing is read back.  SDRM_ERR_ARG: a null pointer; SDRM_ERR_SHAPE: n_rows outside 1 .. 2^22. */
int sdrm_neumf_rank_users(sdrm_engine* e, const uint8_t* mask, int64_t n_rows, int32_t* users_out, int64_t* count_dev, void* hip_stream);

/* The VAE decode hook on the device (reference: train_SDRM.py:212-214 `decoder = Linear(latent, hidden) -> Tanh ->
 * Linear(hidden, N_ITEMS)`, :252-254 `VAE.decode`, called by sample_ddpm at :49 / :61 on the sampled latents): two launches of
 * the engine's fp32 MFMA GEMM with the bias + tanh / bias epilogues.  The struct holds DEVICE pointers to the four nn.Linear
 * tensors as PyTorch stores them (weight [out, in] row-major).  z [n, latent] float32 -> out [n, n_items] float32.  Scratch
 * (padded copies of z and of the weights, the hidden activations) is library-owned and grows on demand - this is a
 * once-per-sampling call, not a step call. */
typedef struct sdrm_vae_decoder {
  const float* w1; const float* b1;   /* decoder[0]: [hidden, latent], [hidden] */
  const float* w2; const float* b2;   /* decoder[2]: [n_items, hidden], [n_items] */
  int latent, hidden, n_items;
} sdrm_vae_decoder;
int sdrm_vae_decode(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, int n, float* out, void* stream);
/* The VAE encode hook on the device, FROZEN and in EVAL MODE only (reference: train_SDRM.py:210-212 `encoder = Linear(N_ITEMS,
 * hidden) -> Tanh -> Linear(hidden, 2*latent)`, :241-250 `VAE.encode` with is_training == 0 and dropout off, called per batch at :323):
 *   z  = mu = W2[:L] tanh(W1 x / max(|x|_2, 1e-12) + b1) + b2[:L]
 *   kl = -0.5 * mean over rows of sum(1 + logvar - mu^2 - exp(logvar)),   logvar = rows L..2L of the second Linear.
 * Dropout, the reparameterisation draw (the reference multiplies it by is_training == 0) and anything backward are out of scope: a
 * VAE in train mode is not this function.
 * sdrm_vae_encoder_load stages the encoder once into library-owned buffers (W1 transposed [n_items, hidden padded to 4] for the CSR
 * form, zero-padded tiled copies of W1 and W2 for the GEMM, the biases); the struct holds DEVICE pointers to the four nn.Linear tensors
 * as PyTorch stores them, free again once the call is ordered on `stream`.  A second load replaces the first.  Envelope: 1 <= latent <=
 * 4096, 1 <= hidden <= 16384, 1 <= n_items <= 2^20.  Both encode calls return SDRM_ERR_STATE while no encoder is loaded.
 * sdrm_vae_encode: x [n, n_items] float32 dense (n_items is the loaded encoder's) -> z [n, latent]; one staging launch (L2
 * normalisation) and two launches of the fp32 MFMA GEMM.
 * sdrm_vae_encode_csr: the same z for the CSR rows rows[0..b) (or row0 .. row0+b-1 when rows is null) of a device-resident matrix
 * [n_rows, n_items], under the contract of sdrm_csr_rows_to_dense (int64 indptr, int32 indices, float32 data or null for all ones;
 * canonical CSR: no column twice in a row; stored zeros are legal).  The first Linear is a gather of the rows of W1 transposed that
 * the row's entries name, summed in CSR order: no dense batch exists, and a row's z does not depend on where it sits in the batch, bit
 * for bit.  Row ids, indptr pairs and column indices are range-checked on the device into the same status word: an offending entry
 * contributes nothing, an offending row is encoded as an empty row, and sdrm_feed_status reports it.
 * kl (device float) may be null: then only the mu half of the second Linear is computed.  Scratch is library-owned and grow-only. */
typedef struct sdrm_vae_encoder {
  const float* w1; const float* b1;   /* encoder[0]: [hidden, n_items], [hidden] */
  const float* w2; const float* b2;   /* encoder[2]: [2*latent, hidden], [2*latent] */
  int n_items, hidden, latent;
} sdrm_vae_encoder;
int sdrm_vae_encoder_load(sdrm_engine* e, const sdrm_vae_encoder* enc, void* stream);
int sdrm_vae_encode(sdrm_engine* e, const float* x, int n, float* z, float* kl, void* stream);
int sdrm_vae_encode_csr(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows,
                        const int64_t* rows, int64_t row0, int b, float* z, float* kl, void* stream);
/* The loss head of the VAE pre-stage on the device (reference: train_SDRM.py:141-142,
 *   neg_ll = -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X, dim=1)), and the gradient autograd derives from it), for the batch
 * whose interaction rows X are the CSR rows rows[0..b) (or row0 .. row0+b-1 when rows is null) of a device-resident matrix
 * [n_rows, n_items] under the contract of sdrm_vae_encode_csr (int64 indptr, int32 indices, float32 data or null for all ones;
 * canonical CSR: no column twice in a row; stored zeros are legal).  No dense X exists.  logits [b, n_items] float32 row-major, its
 * base 16-byte aligned (rows need not be).  With x_p the stored values of the batch row's CSR row and s_r their sum:
 *   sdrm_multinomial_nll_csr:       lse[r] = log sum_i exp(logits[r,i])  (max-subtracted, fp32; device float [b]),
 *                                   *loss  = -(1/b) sum_r sum_p x_p (logits[r, col_p] - lse[r])  (device float; fp32 terms summed in
 *                                   float64 in a fixed order: per work-group partials, then one work-group; no atomics).
 *   sdrm_multinomial_nll_csr_grad:  grad[r,i] = scale (exp(logits[r,i] - lse[r]) s_r - X[r,i]) / b, with lse as the first call left it;
 *                                   scale is a DEVICE float, the upstream gradient (null: 1).
 * The first call reads the logits once (and the row's stored columns once more for the terms), the second reads them once and writes
 * grad once.  grad (16-byte aligned) may be the logits buffer itself - exactly it, any other overlap is SDRM_ERR_ARG: every element
 * is read before it is written, by the thread that writes it.
 * Bit-level promises: lse[r] and row r of grad are functions of logits row r, CSR row rows[r], b and scale alone - the same bits
 * wherever the row sits in the batch, with rows or row0 addressing, in place or out of place, and for data == null against explicit
 * ones; *loss is the same bits from call to call on the same inputs.
 * Row ids, indptr pairs and column indices are range-checked on the device into the status word sdrm_feed_status reports: an
 * offending entry contributes nothing to s_r, to the loss or to grad; an offending row counts as an empty row (its term is 0, its
 * grad row all zeros; its lse is still that of its logits).  No load or store uses an unchecked index.
 * Envelope: 1 <= b, 1 <= n_items <= 2^20, b * n_items < 2^40 (SDRM_ERR_SHAPE otherwise, and for a contiguous range that ends behind
 * n_rows); a null required pointer or a misaligned logits / grad is SDRM_ERR_ARG.  Non-finite logits are outside the contract.
 * Scratch (the float64 partials, a fixed 16 KB of the handle) is library-owned.  Neither call synchronises the stream. */
int sdrm_multinomial_nll_csr(sdrm_engine* e, const float* logits, const int64_t* indptr, const int32_t* indices, const float* data,
                             int64_t n_rows, const int64_t* rows, int64_t row0, int b, int n_items, float* lse, float* loss, void* stream);
int sdrm_multinomial_nll_csr_grad(sdrm_engine* e, const float* logits, const float* lse, const int64_t* indptr, const int32_t* indices,
                                  const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b, int n_items,
                                  const float* scale, float* grad, void* stream);
/* The input layer of the VAE encoder in TRAIN mode, both directions, straight from a device-resident feed (reference:
 * train_SDRM.py:242-244, `h = self.encoder(self.dropout(F.normalize(x, p=2, dim=1)))` - the normalisation, the dropout and the FIRST
 * Linear of the encoder - and, of :148 `loss.backward()`, that Linear's weight gradient).  No dense batch exists in either direction.
 *   x~[r,c]  = keep(R_r, c) * scale * x[r,c] / max(|x[r,:]|_2, 1e-12)     R_r the feed row of batch row r; the norm covers dropped entries
 *   pre[r,:] = sum_c x~[r,c] W1[:,c] + b1                                  (no tanh: everything behind the pre-activation is the caller's)
 *   dW1[:,c] = sum_r x~[r,c] dpre[r,:]
 * Dropout: the keep decision of (feed row R, column c) is word c & 3 of Philox4x32-10 with counter (R, c >> 2, 7, step) and key
 * `seed` (csrc/philox.h, PURPOSE_VAE_DROP); keep iff word >= thr, thr = floor((double)p_drop * 2^32); kept values are multiplied by
 * scale = (float)(1 / (1 - (double)p_drop)).  p_drop is a float in [0, 1) (0: nothing is drawn).  The decision depends on (seed,
 * step, R, c) alone - not on where the row sits in a batch - and the backward regenerates it: no mask is stored.
 * sdrm_vae_input_layer_fwd: w1 [hidden, n_items], b1 [hidden] as nn.Linear stores them (device, read by this call: W1 is transposed
 *   into scratch of the handle on EVERY call, it changes with every optimiser step; an encoder staged by sdrm_vae_encoder_load is not
 *   touched); the batch is the CSR rows rows[0..b) (or row0 .. row0+b-1 when rows is null) of the feed [n_rows, n_items] under the
 *   contract of sdrm_vae_encode_csr.  Out: pre [b, hidden] contiguous and rowscale [b] = scale / max(|x[r,:]|_2, 1e-12), which the
 *   backward takes.  A row's pre and rowscale have the same bits at any batch position and batch size, through rows or row0, and for
 *   data == null against explicit ones.
 * sdrm_vae_input_layer_wgrad: dpre [b, hidden] contiguous, rowscale [b] as the forward left it; the feed as CSC (int64 colptr
 *   [n_items + 1], int32 rowidx ascending within a column, float32 data or null); pos int32 [n_rows], the place of every feed row in
 *   the epoch's order (the inverse of the permutation whose slice lo .. lo+b-1 was the forward's `rows`; null: the identity, batch =
 *   rows lo .. lo+b-1).  Feed row R is in the batch iff 0 <= pos[R] - lo < b, and that difference is its row of dpre.  Out: dw1
 *   [hidden, n_items] contiguous, EVERY element written exactly once (zero where the batch has no kept entry): no memset, no atomic.
 *   A column's sum runs over its members in ascending feed row: the same bits from call to call and under any order of the batch.
 *   Cost: one walk over the whole feed's rowidx per call, whatever b is.
 * Range checks, into the status word sdrm_feed_status reports: row ids, indptr / colptr pairs, column and row indices; an offending
 * entry contributes nothing, an offending row or column counts as empty.  No load or store uses an unchecked index.
 * Envelope (SDRM_ERR_SHAPE otherwise): 1 <= n_items <= 2^20, 1 <= hidden <= 4096, 1 <= n_rows < 2^31, 1 <= b <= 2^22, row0 / lo >= 0,
 * a contiguous range inside the feed, p_drop in [0, 1).  A null required pointer is SDRM_ERR_ARG.  Neither call synchronises. */
int sdrm_vae_input_layer_fwd(sdrm_engine* e, const float* w1, const float* b1, int n_items, int hidden, const int64_t* indptr,
                             const int32_t* indices, const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b,
                             uint64_t seed, uint32_t step, float p_drop, float* pre, float* rowscale, void* stream);
int sdrm_vae_input_layer_wgrad(sdrm_engine* e, const float* dpre, const float* rowscale, int hidden, const int64_t* colptr,
                               const int32_t* rowidx, const float* data, int64_t n_rows, int n_items, const int32_t* pos, int64_t lo,
                               int b, uint64_t seed, uint32_t step, float p_drop, float* dw1, void* stream);
/* The VAE encoder BEHIND its first pre-activation in TRAIN mode, both directions (reference: train_SDRM.py:244-250 with is_training == 1 -
 * the Tanh and the second Linear of `self.encoder`, `chunk`, the KL line and `mu + eps * exp(0.5 * logvar)` - and their share of :148).
 * It takes the `pre` that sdrm_vae_input_layer_fwd left; float32 throughout, L = latent, H = hidden, R_r the feed row of batch row r:
 *   h1   = tanh(pre)                                    [b, H]
 *   out2 = h1 W2^T + b2 = [mu | lv]                     [b, 2L]      W2 [2L, H], b2 [2L] as nn.Linear stores them
 *   eps[r, j] = normal j & 3 of the column quad j >> 2: words = Philox4x32-10 with counter (R_r, j >> 2, 9, step) and key `seed`
 *          (csrc/philox.h, PURPOSE_VAE_EPS); (n0, n1) = box_muller(x, y), (n2, n3) = box_muller(z, w)
 *   z    = mu + eps exp(0.5 lv)                         [b, L]
 *   kl   = -0.5 / b sum_r sum_j (lv - mu^2 - expm1(lv))  fp32 terms summed in float64 in a fixed order (per-work-group partials, then
 *          one work-group): no floating-point atomic
 *   dmu  = gz + gkl mu / b        dlv = 0.5 gz eps exp(0.5 lv) + 0.5 gkl expm1(lv) / b        dout2 = [dmu | dlv]
 *   dW2  = dout2^T h1             db2 = sum_r dout2[r, :]                                      dpre  = (dout2 W2) (1 - h1^2)
 * The draw depends on (seed, step, R_r, j) alone - not on where the row sits in a batch, on the batch size or on torch's generator.
 * sdrm_vae_latent_fwd: pre [b, hidden], w2 [2 latent, hidden], b2 [2 latent] contiguous (device, read by this call: W2 and b2 are
 *   padded into scratch of the handle on EVERY call, they change with every optimiser step; an encoder staged by
 *   sdrm_vae_encoder_load is not touched).  rows: int64 device array [b] of feed rows, or null for row0 .. row0 + b - 1; it names the
 *   rows for the Philox counter only - no feed is read.  draw != 0: eps [b, latent] is drawn and WRITTEN; draw == 0: eps is an INPUT
 *   and is not written (how tests, and callers who want torch's draws, inject their own; rows, row0, seed and step are then unused).
 *   Out, all caller-owned and contiguous: h1 [b, hidden], out2 [b, 2 latent], eps, z [b, latent], kl (one device float).  The
 *   backward takes h1, out2 and eps from the caller, so two forwards may precede their backwards.
 * sdrm_vae_latent_bwd: h1, out2, eps as a forward left them, w2 as that forward read it; gz [b, latent] and gkl (ONE device float),
 *   the upstream gradients of z and kl - either may be null, which means zero.  Out: dpre [b, hidden], dw2 [2 latent, hidden], db2
 *   [2 latent] contiguous, EVERY element written exactly once: no memset, no atomic, the same bits from call to call.
 * Launches: 4 forward (staging, GEMM, reparameterisation + KL partials, KL sum), 5 backward (staging, seed, weight-gradient GEMM,
 * dgrad GEMM, unpadding); the GEMMs are csrc/gemm.h's fp32 MFMA family and follow sdrm_debug_set_tile.
 * Envelope (SDRM_ERR_SHAPE otherwise): 1 <= hidden <= 4096, 1 <= latent <= 4096, 1 <= b <= 2^22, feed rows in [0, 2^31) (row0 .. row0
 * + b - 1 is checked on the host; an id of `rows` outside that range raises the feed status word's row bit, sdrm_feed_status, and its
 * counter is the id's low 32 bits).  A null required pointer is SDRM_ERR_ARG.  Neither call synchronises or reads back. */
int sdrm_vae_latent_fwd(sdrm_engine* e, const float* pre, const float* w2, const float* b2, int hidden, int latent, const int64_t* rows,
                        int64_t row0, int b, uint64_t seed, uint32_t step, int draw, float* h1, float* out2, float* eps, float* z, float* kl,
                        void* stream);
int sdrm_vae_latent_bwd(sdrm_engine* e, const float* h1, const float* out2, const float* eps, const float* w2, int hidden, int latent, int b,
                        const float* gz, const float* gkl, float* dpre, float* dw2, float* db2, void* stream);
/* The VAE decoder and the multinomial loss in TRAIN mode, both directions (reference: train_SDRM.py:252-254 `decode`, :141-142 the loss
 * line, and their share of :148), for the batch whose interaction rows are the CSR rows rows[0..b) (or row0 .. row0+b-1 when rows is null)
 * of a device-resident matrix [n_rows, n_items] under the contract of sdrm_multinomial_nll_csr.  float32 throughout, L = latent,
 * H = hidden, I = n_items; `dec` is sdrm_vae_decode's struct: w1 = W3 [H, L], b1 = b3 [H], w2 = W4 [I, H], b2 = b4 [I] as nn.Linear
 * stores them:
 *   h3     = tanh(z W3^T + b3)                         [b, H]
 *   logits = h3 W4^T + b4                              [b, I]
 *   lse[r] = log sum_i exp(logits[r,i])                (max-subtracted, fp32, over exactly I columns)
 *   loss   = -(1/b) sum_r sum_p x_p (logits[r,col_p] - lse[r])      (fp32 terms, float64 sums in a fixed order)
 *   g      = scale (exp(logits - lse) s_r - X) / b     [b, I]       s_r = sum_p x_p;  scale: ONE device float or null (= 1)
 *   dW4 = g^T h3     db4 = sum_r g[r,:]     dpre3 = (g W4)(1 - h3^2)
 *   dW3 = dpre3^T z  db3 = sum_r dpre3[r,:] dz    = dpre3 W3
 * sdrm_vae_decoder_nll_fwd: z [b, L] contiguous.  Out, all caller-owned and contiguous: h3 [b, H], logits [b, I] (base 16-byte
 *   aligned), lse [b], loss (one device float).  The four tensors are read and padded into scratch of the handle on EVERY call (they
 *   change with every optimiser step); the scratch of sdrm_vae_decode and an encoder staged by sdrm_vae_encoder_load are not touched.
 * sdrm_vae_decoder_nll_bwd: z, h3, logits, lse as a forward left them, W3 and W4 as that forward read them (b1 / b2 of `dec` are not
 *   read), the same batch - so two forwards may precede their backwards.  The inputs are not written; g and dpre3 live in padded
 *   scratch of the handle, whose padding this call writes itself.  Out: dz [b, L] (may be null: then the last dgrad is not launched),
 *   dw3 [H, L], db3 [H], dw4 [I, H], db4 [I] contiguous, EVERY element written exactly once: no memset, no atomic, the same bits
 *   from call to call on the same inputs.
 * Range checks as in sdrm_multinomial_nll_csr: an offending entry contributes nothing to s_r, the loss or g; an offending row counts
 * as an empty row (its g row is zero, its lse still that of its logits); the verdict waits in the word sdrm_feed_status reports.
 * Launches: 6 forward (staging, GEMM + tanh, h3 unpadded, GEMM + bias, loss rows, loss sum), 7 backward (staging with both weight
 * transposes, loss gradient, weight-gradient GEMM of W4, dgrad GEMM through the tanh, weight-gradient GEMM of W3, dgrad GEMM to z,
 * unpadding) - 6 without dz; the GEMMs are csrc/gemm.h's fp32 MFMA family and follow sdrm_debug_set_tile.  A batch of more rows than
 * one weight-gradient K chunk (8192, fewer where (chunk + 64) x n_items padded to 32 x 4 bytes would reach 2^32) makes one slab per
 * chunk, added in slab order; a product beyond the exact range of the GEMM's tile arithmetic goes out in bands, one launch each.
 * Envelope (SDRM_ERR_SHAPE otherwise, before any launch): 1 <= latent <= 4096, 1 <= hidden <= 4096, 1 <= n_items <= 2^20, 1 <= b <=
 * 2^22, b x n_items < 2^40, n_rows >= 1, row0 >= 0 and a contiguous range inside the matrix.  A null required pointer or a logits
 * base off 16 bytes is SDRM_ERR_ARG.  Both calls join the sampler's chains; neither synchronises or reads back. */
int sdrm_vae_decoder_nll_fwd(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, const int64_t* indptr, const int32_t* indices,
                             const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b, float* h3, float* logits,
                             float* lse, float* loss, void* stream);
int sdrm_vae_decoder_nll_bwd(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, const float* h3, const float* logits, const float* lse,
                             const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, const int64_t* rows,
                             int64_t row0, int b, const float* scale, float* dz, float* dw3, float* db3, float* dw4, float* db4, void* stream);
/* Adam over caller-owned tensors in ONE launch, and the loss value of a pre-stage step (reference: train_SDRM.py:126
 * `torch.optim.Adam(model.parameters(), lr)`, :143-150 `loss = neg_ll + anneal * kl + model.get_l2_reg()` ... `optimizer.step()`, :262-268
 * get_l2_reg).  Per tensor p, g, m, v: float32, contiguous, n elements each, on the device; p, m, v are updated in place, g is read only:
 *   g' = g + 2 l2_coef p        (the gradient of the loss term l2_coef * sum(p^2), folded in; l2_coef = weight_decay for a `.weight`, 0 for a bias)
 *   m = beta1 m + (1 - beta1) g'        v = beta2 v + (1 - beta2) g'^2
 *   p -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * torch.optim.Adam's update in its default form (no amsgrad, not maximize), in fp32 with contraction off and the hardware's sqrt / rcp
 * (1 ulp each: csrc/elementwise.h adam_math, the eps-net's own); the two bias corrections are formed on the host in double from the
 * float betas.  `step` >= 1 is the count AFTER this update and is the caller's number: nothing of the optimizer lives in the handle,
 * two optimizers may share an engine.  Work is dealt in chunks of 4096 elements, one work-group each: a tensor of n elements is
 * ceil(n / 4096) chunks, 16 tensors go into one launch, more go out as successive launches of the same kernel.  A tensor whose four
 * pointers are 16-byte aligned is read and written with 16-byte accesses (its last partial quad by dwords), any other by dwords; no
 * access falls outside [ptr, ptr + n).
 * l2_partials (device, float64, l2_capacity elements; may be null): when given and some l2_coef > 0, slot c of it receives sum(p^2) over
 * chunk c of the table - the weights BEFORE the update, 0 for a chunk of a tensor with l2_coef == 0 - summed in float64 in a fixed order
 * (no atomic): every slot below the chunk count is written, none is read, the buffer needs no zeroing.  With every l2_coef == 0 nothing
 * is summed and the buffer is not touched.
 * sdrm_vae_loss_slot: *out = (*neg_ll + anneal * *kl) + (float)(weight_decay * sum(l2_partials[0 .. n_partials))) from device scalars, in
 * torch's parenthesisation of `neg_ll + anneal * kl + l2` on float32 with contraction off; the partials are added in float64 in a fixed
 * order by one work-group.  l2_partials == null: the last term is +0.0f (what get_l2_reg returns for weight_decay == 0), and the value
 * equals torch's for the same two scalars to the bit.  `out` is ONE float on the device, e.g. a slot of a per-epoch loss buffer.
 * Refusals, before any launch: a null pointer, step < 1, a negative l2_coef, or two of the 4 x n_tensors ranges [ptr, ptr + n) sharing
 * a byte (ranges that only touch are fine) are SDRM_ERR_ARG; n_tensors <= 0, n outside 1 .. 2^40, more than 2^30 chunks, l2_capacity
 * below the chunk count while l2_partials is given and some l2_coef > 0, or n_partials < 1 with l2_partials given are SDRM_ERR_SHAPE.
 * Both calls are deterministic from call to call, use no atomics, do not synchronise and read nothing back. */
typedef struct sdrm_vae_adam_tensor { float* p; const float* g; float* m; float* v; int64_t n; float l2_coef; } sdrm_vae_adam_tensor;
int sdrm_vae_adam_step(sdrm_engine* e, const sdrm_vae_adam_tensor* t, int n_tensors, int64_t step, float lr, float beta1, float beta2,
                       float eps, double* l2_partials, int64_t l2_capacity, void* stream);
int sdrm_vae_loss_slot(sdrm_engine* e, const float* neg_ll, const float* kl, float anneal, const double* l2_partials, int64_t n_partials,
                       float weight_decay, float* out, void* stream);
/* Per-user hold-out split on the device, CSR in, two CSRs out (reference: utilities.py:174-236,
 * split_train_test_proportion_from_csr_matrix with ignore_zeros=False, which train_SDRM.py:161 calls once per pre-stage epoch): of
 * the n stored entries of a user with n >= 2, m = ceil(test_prop * n) chosen uniformly without replacement go to the held-out
 * matrix and the others to the train matrix; both are all ones (there is no data array, in or out: every stored entry of the input
 * counts as an interaction, stored zeros included) with columns in CSR order.  Where the reference DROPS a user with fewer than two
 * entries, that user is an EMPTY ROW in both outputs here: row numbers stay the input's, and sdrm_rank_metrics gives such a user nan,
 * which the pre-stage's nanmean ignores - the same users count.
 * The reference's MT19937 np.random.choice stream is not reproduced.  The draw is defined by sort keys (csrc/philox.h,
 * PURPOSE_HOLDOUT = 8): entry p (0-based place inside feed row u) has
 *   w_p     = word p & 3 of Philox4x32-10 with counter (u, p >> 2, 8, draw) and key `seed`,
 *   rank(p) = #{q : w_q < w_p or (w_q == w_p and q < p)},   and is held out iff rank(p) < m_u,
 *   m_u     = n_u < 2 ? 0 : min(n_u, (int64)ceil(test_prop * (double)n_u))      (the product in double: Python's math.ceil(test_prop * n)).
 * The m smallest of iid keys are a uniform m-subset (the tie-break by place on equal 32-bit words is a bias of order n^2 2^-32).  The
 * split of row u depends on (seed, draw, u, n_u) and the row's columns alone - not on n_rows or any other row.
 * In: indptr [n_rows + 1] int64, indices [nnz] int32 (device).  Out: train_indptr, held_indptr [n_rows + 1] int64; train_indices,
 * held_indices int32 of capacity nnz, filled on [0, x_indptr[n_rows]) and untouched behind (every store is checked against nnz).
 * The call does not synchronise and reads nothing back; the outputs are the same bits on every call.
 * Range checks, into the status word sdrm_feed_status reports: a row whose indptr pair is out of order or reaches outside [0, nnz],
 * that is longer than n_items, or that holds a column outside [0, n_items) is recorded and is an empty row in both outputs.  The
 * outputs therefore hold checked column indices and ordered offsets only: sdrm_rank_metrics and sdrm_csr_rows_to_dense may take
 * them as they are.  No load or store uses an unchecked index.
 * Envelope (SDRM_ERR_SHAPE otherwise): 1 <= n_items <= 2^20, 1 <= n_rows < 2^31, 0 <= nnz < 2^40, 0 < test_prop < 1.  A null
 * pointer is SDRM_ERR_ARG (with nnz == 0 the index arrays are never touched but must still be given).  Scratch (two counts per
 * row) is library-owned and grow-only.  The ranking is quadratic in the row length. */
int sdrm_holdout_split(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int n_items, int64_t nnz,
                       double test_prop, uint64_t seed, uint32_t draw, int64_t* train_indptr, int32_t* train_indices,
                       int64_t* held_indptr, int32_t* held_indices, void* stream);
/* Recall@k and NDCG@k of a score matrix against held-out interactions (reference: utilities.py:116-171,
 * mask_training_examples + recall_at_k_batch + NDCG_binary_at_k_batch, as svd_benchmark.py:58-66 chains them).
 * scores [U, I] float32 row-major; held_* / train_* are CSR index arrays over the same U rows (int64 indptr [U+1],
 * int32 column indices; every stored entry counts as an interaction); train_* may both be null (no masking,
 * otherwise those items score -inf).  ks_host: nk <= 8 cut-offs (HOST array, each 1 <= k <= min(128, I)).
 * tp [kmax] = 1/log2(r+2) and idcg [kmax+1] = sum(tp[:m]) are float64 DEVICE tables computed by the caller with numpy
 * so that the constants are the reference's own.  recall, ndcg: [nk, U] float64 (nan where a user has nothing held
 * out, like the reference's 0/0).  Ties in the scores rank towards the lower item index (the reference's
 * argpartition leaves them unspecified). */
int sdrm_rank_metrics(sdrm_engine* e, const float* scores, int U, int I, const int64_t* held_indptr,
                      const int32_t* held_indices, const int64_t* train_indptr, const int32_t* train_indices,
                      const int32_t* ks_host, int nk, const double* tp, const double* idcg, double* recall, double* ndcg,
                      void* stream);
/* sdrm_rank_metrics with a row map, for any caller whose score rows are a selection of the rows of two resident matrices (reference:
 * the same utilities.py:116-171; for the NeuMF evaluator neural_cf_benchmark_pt.py:294-332, where sdrm_amd/neumf.py's rank_all_items
 * selected the rows on the host, uploaded both selections and re-footed the NDCG there).  scores [U, I]; held_* / train_* are CSR index
 * arrays over n_rows rows (int64 indptr [n_rows + 1], int32 columns, held_nnz / train_nnz the capacities of the index arrays) and score
 * row q ranks against CSR row rows[q] of both (rows: DEVICE int32 [U], any order, repeats allowed).  Nothing is trusted: rows[q] outside
 * [0, n_rows) is an empty row and raises the row bit of the status word sdrm_feed_status reports; an indptr pair that is out of order or
 * reaches outside [0, nnz] is an empty row (the indptr bit), an entry with a column outside [0, I) is skipped, a held one does not count
 * as held (the column bit).  ks_host, tp, idcg, recall, ndcg, the bound I <= 36864, the k rules and the ties: sdrm_rank_metrics'.
 * full_idcg == 0: sdrm_rank_metrics' NDCG, dcg / idcg[min(n_true, k)], nan without a held-out item.  full_idcg != 0: the NeuMF footing -
 *   the reference's held-out matrix stores every pair of the cartesian product, so its ideal DCG counts min(I, k) items for every user
 *   and a user without a relevant item has NDCG 0.  The device makes the three float64 operations rank_all_items made on the host, in
 *   its order, so the bits are its bits: t = dcg / idcg[min(n_true, k)]; ndcg = n_true > 0 ? t * idcg[min(n_true, k)] / idcg[min(I, k)]
 *   : 0.0 - not the shortcut dcg / idcg[min(I, k)].  Recall is the same either way: nan without a relevant item.
 * One launch on `hip_stream` (the caller's stream, under the contract of every `stream` argument of this header); nothing is read back.
 * SDRM_ERR_ARG: a null pointer (train_* may both be null), nk outside 1 .. 8, a k outside [1, min(128, I)]; SDRM_ERR_SHAPE: U < 1, I
 * outside 1 .. 36864, n_rows < 1, a negative capacity. */
int sdrm_rank_metrics_rows(sdrm_engine* e, const float* scores, int U, int I, const int32_t* rows, int64_t n_rows, const int64_t* held_indptr,
                           const int32_t* held_indices, int64_t held_nnz, const int64_t* train_indptr, const int32_t* train_indices,
                           int64_t train_nnz, const int32_t* ks_host, int nk, const double* tp, const double* idcg, double* recall, double* ndcg,
                           int full_idcg, void* hip_stream);
/* The evaluation half of a VAE pre-stage epoch on the device (reference: train_SDRM.py:160-177 with is_training == 0 and dropout
 * off), one call for all users of a hold-out split.  enc / dec are the eight LIVE nn.Linear tensors as nn.Linear stores them (their
 * n_items, hidden and latent must agree); train_* / held_* are the two CSR index pairs sdrm_holdout_split leaves (int64 indptr
 * [n_rows + 1], int32 indices of capacity *_nnz; every stored entry counts as 1).  For user u, with T_u the columns of the train
 * part and H_u those of the held part:
 *   x = 1_{T_u} / max(sqrt(|T_u|), 1e-12),  h1 = tanh(W1 x + b1),  z = W2[:L] h1 + b2[:L],  h3 = tanh(W3 z + b3),  s = W4 h3 + b4,
 *   scores[u] = Recall@k (metric 0) or NDCG@k (metric 1) of s against H_u with the items of T_u at -inf
 * - the last line being sdrm_rank_metrics' definition (tie rule, nan for a user with nothing held out, tp [k] and idcg [k + 1] float64
 * device tables as that call takes them).  The logvar rows of W2, the KL and the reparameterisation draw are never computed.
 * scores: float64 [n_rows], every element written exactly once.  logits: null, or float32 [n_rows, n_items] contiguous, which then
 * receives s of every user; when null, nothing of that size leaves the handle's scratch.
 * The weights are staged ONCE per call (two launches: seven tensors padded, W1 transposed) into scratch of their own - an encoder
 * staged by sdrm_vae_encoder_load and the scratch of the train-mode entry points are not touched -, then the call loops over batches
 * of `batch` users (the last may be short), five launches each: the eval-mode gather of the first Linear straight from the train
 * part's rows (no dense input batch), three MFMA GEMMs (they follow sdrm_debug_set_tile) and the ranking.  A GEMM of more than 65535
 * tiles goes out in row bands, one launch each.  The call does not synchronise, reads nothing back, joins the sampler chains like its
 * neighbours, and gives the same bits on every call.
 * Range checks, into the status word sdrm_feed_status reports: no load or store uses an unchecked index.  An indptr pair that is
 * negative, out of order or reaches behind *_nnz is an empty row, in the gather and in the ranking alike (such a user's logits are
 * those of a user without train entries, and nothing of that user is masked); a train entry with a column outside [0, n_items)
 * contributes nothing and masks nothing; a held entry outside it is neither ranked nor counted.
 * Envelope (SDRM_ERR_SHAPE otherwise): 1 <= n_items <= 36864 (the ranking's LDS row), 1 <= hidden, latent <= 4096, 1 <= n_rows <
 * 2^31, 1 <= batch <= 2^22, 1 <= k <= min(128, n_items), metric in {0, 1}, *_nnz >= 0, every tile x K span of the GEMMs below 2^32
 * bytes.  A null required pointer is SDRM_ERR_ARG.  No launch is made by a refused call. */
int sdrm_vae_eval_holdout(sdrm_engine* e, const sdrm_vae_encoder* enc, const sdrm_vae_decoder* dec, const int64_t* train_indptr,
                          const int32_t* train_indices, int64_t train_nnz, const int64_t* held_indptr, const int32_t* held_indices,
                          int64_t held_nnz, int64_t n_rows, int batch, int k, const double* tp, const double* idcg, int metric,
                          double* scores, float* logits, void* stream);

/* Rank-k truncated SVD of a sparse matrix on the device, and the scores of its rank-k reconstruction (reference: svd_benchmark.py:17-70,
 * `TruncatedSVD(n_components=20, n_iter=100)` fitted on the stacked matrix, `inverse_transform(fit_transform(.))` as the score matrix).
 * sklearn's randomized SVD is a subspace iteration; this is the same iteration on a panel of 32 columns (csrc/svd_eval.h):
 *   Q [n, 32] = the start panel;  n_iter times: Y = A Q, Y <- orth(Y), Q = A^T Y, Q <- orth(Q);  then Y = A Q, Y <- orth(Y), Z = A^T Y
 *   host, float64: the eigenvectors of Z^T Z (= B B^T for B = Y^T A) rotate Z into the top k right singular directions; normalised, they
 *   are the rows of components, and singular_values are the square roots of the eigenvalues.
 * The products are gathers in float32, every output element summed in the order of its row's entries (no atomic: the same bits on every
 * call); orth is CholeskyQR applied twice with the Gram matrix, the factorisation and the sums of Y R^-1 in float64.  7 launches per
 * half-iteration.  The sign of a component is whatever the iteration leaves (sklearn's svd_flip is not applied).
 * sdrm_svd_fit: the matrix A [m, n] in BOTH forms, device-resident under the contract of sdrm_csr_rows_to_dense - CSR (indptr [m + 1]
 *   int64, indices [nnz] int32, data [nnz] float32 or null for all ones) and CSC (colptr [n + 1], rowidx [nnz], cdata: the CSR of the
 *   transpose; data and cdata are both given or both null).  q0: null - the start panel is drawn on the device, normals 4 j .. 4 j + 3 of
 *   row i from Philox4x32-10 with counter (i, j, 10, draw) and key `seed` -, or a device float32 [n, 32] that is used instead (how tests
 *   inject theirs; seed and draw are then unused).  Out: components [k, n] float32 on the device, singular_values_host [k] float64 on the
 *   HOST, descending.  The call synchronises `stream`: ONE read-back (Z, 128 n bytes, with the status word), the small problem on the host,
 *   one upload of components.
 *   SDRM_ERR_SHAPE, before any launch: k < 1, k + 10 > 32 (the reference's 10 oversampling columns must fit the panel), min(m, n) < 32,
 *   m or n above 2^22, nnz outside 0 .. 2^40 - 1, n_iter outside 0 .. 10000.  A null required pointer is SDRM_ERR_ARG.
 *   BREAKDOWN is SDRM_ERR_ARG as well (the matrix handed in cannot be factored; the message says so): a panel whose columns are numerically
 *   dependent - a matrix of rank < 32, or values that are not finite - shows as a Cholesky pivot at or below 2^-40 of the largest diagonal
 *   entry of the Gram matrix (the derivation is in csrc/svd_eval.h).  It raises a status word on the device and zeroes the panel, so the
 *   rest of the fit meets no NaN and stores nothing outside the handle's scratch; components and singular_values_host are not written.
 *   The word is cleared by the refusal and by the next fit: the next call on the same handle works.
 * sdrm_svd_scores: scores [b, n_items] float32 contiguous = (A_rows V^T) V for the CSR rows rows[0..b) (or row0 .. row0+b-1 when rows is
 *   null) of a device-resident matrix [n_rows, n_items] and V = components [k, n_items]: V is transposed into scratch, the rows' k
 *   coordinates are gathered by the fit's product kernel, and the expansion writes every element of scores exactly once.  Three launches,
 *   no synchronisation.  Seen items are NOT masked: sdrm_rank_metrics does that.
 *   SDRM_ERR_SHAPE: k outside 1 .. 22, b or n_items above 2^22, b x n_items at or above 2^40, a contiguous range that ends behind n_rows.
 * Range checks of both calls, into the status word sdrm_feed_status reports: row ids, indptr / colptr pairs (negative, out of order or
 * reaching behind nnz: the row is empty), column / row indices outside the matrix (the entry is skipped).  A row that fails is a zero
 * row of the product and of scores.  No load or store uses an unchecked index.  Scratch is library-owned and grow-only. */
int sdrm_svd_fit(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, const int64_t* colptr, const int32_t* rowidx,
                 const float* cdata, int64_t m, int64_t n, int64_t nnz, int k, int n_iter, uint64_t seed, uint32_t draw, const float* q0,
                 float* components, double* singular_values_host, void* stream);
int sdrm_svd_scores(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t nnz,
                    const int64_t* rows, int64_t row0, int b, int n_items, const float* components, int k, float* scores, void* stream);

/* Non-negative matrix factorisation of a sparse matrix on the device, and the scores of its reconstruction (reference:
 * svd_benchmark.py:49-54 with nnmf=True, `NMF(n_components=15, max_iter=50)` fitted on the stacked matrix, `inverse_transform(fit_transform(.))`
 * as the score matrix; sklearn's defaults: the `cd` solver, no regularisation, no shuffle, tol = 1e-4, init = NNDSVDa).  csrc/nmf.h.
 * Everything is float64.  A factor is stored row-major with a row stride of 16 doubles, 16-byte aligned: W [m][16], Ht = H^T [n][16]; the
 * columns k .. 15 are zero on entry and on exit and are never read into a result.  The matrix X [m, n] is device-resident under the contract
 * of sdrm_svd_fit: CSR (indptr [m + 1] int64, indices [nnz] int32, data [nnz] float32 or null for all ones) and, for the fit, CSC as well.
 * sdrm_nmf_fit: W and Ht are the start on entry (sklearn's init='custom') and the result on exit.  Iteration i = 1 .. max_iter updates W, then
 *   H, by one cyclic sweep of coordinate descent each (`_update_coordinate_descent`: the product X Ht gathered in CSR order, the Gram matrix
 *   Ht^T Ht from per-work-group partials added in block order, then per row, t ascending: grad = -XHt[t] + sum_r HHt[t][r] W[r]; the
 *   projected gradient pg = grad, or min(0, grad) where W[t] == 0, adds |pg| to the violation; W[t] = max(W[t] - grad / HHt[t][t], 0) unless
 *   HHt[t][t] == 0).  Every sum is one fused chain in a fixed order, nothing is atomic: the same bits on every call.  After iteration i the
 *   device forms v_i = violation of both halves, stores it in violations_dev[i - 1], and stops when v_1 == 0 or v_i / v_1 <= tol: *n_iter_dev
 *   = i, the factors are those of iteration i, the launches behind it return at once and violations_dev[i ..] stay 0.  Without a stop
 *   *n_iter_dev = max_iter.  n_iter_dev: a device int32; violations_dev: device float64 [max_iter].  Five launches per iteration, all
 *   queued by the one call: NO synchronisation and no read-back.
 *   SDRM_ERR_SHAPE, before any launch: k outside 1 .. 16, max_iter outside 1 .. 10000, tol < 0 (or NaN), m or n outside 1 .. 2^22, nnz
 *   outside 0 .. 2^40 - 1.  A null pointer, data without cdata or a factor off the 16-byte grid is SDRM_ERR_ARG.
 * sdrm_nmf_init: W0 [m][16], Ht0 [n][16] = `_initialize_nmf(X, k, init='nndsvda')` with the truncated SVD that sdrm_svd_fit leaves -
 *   components [k, n] float32 on the device, singular_values_host [k] on the HOST - in the place of sklearn's randomized one: U = X V^T /
 *   sigma by the fit's product kernel in float64; component 0 is sqrt(sigma_0) |u_0|, sqrt(sigma_0) |v_0|; component j >= 1 the positive or
 *   the negative parts of (u_j, v_j), whichever pair has the larger product of norms (the negative pair on a tie), normalised and scaled by
 *   sqrt(sigma_j x that product); an entry below 1e-6 becomes 0 and every zero becomes X.mean() - (entries) / (m n) for all-ones data, else
 *   the sum of the values in a fixed order over m n.  The sign of a component does not matter.  Six launches, no synchronisation.
 *   SDRM_ERR_SHAPE as above; a singular value that is not positive and finite is SDRM_ERR_ARG.
 * sdrm_nmf_scores: scores [b, n_items] float32 contiguous, scores[r][j] = sum_{c < k} W[row_r][c] Ht[j][c], c ascending, added in float64
 *   and rounded once, for the rows rows[0..b) of W [n_rows][16] (or row0 .. row0+b-1 when rows is null).  One launch, every element written
 *   exactly once, no synchronisation.  Seen items are NOT masked: sdrm_rank_metrics does that.
 *   SDRM_ERR_SHAPE: k outside 1 .. 16, b, n_items or n_rows outside 1 .. 2^22, b x n_items at or above 2^40, a contiguous range that ends
 *   behind n_rows.
 * Range checks of all three, into the status word sdrm_feed_status reports: row ids, indptr / colptr pairs (negative, out of order or reaching
 * behind nnz: the row is empty), column / row indices outside the matrix (the entry is skipped); a listed row of sdrm_nmf_scores outside
 * [0, n_rows) is a zero row.  No load or store uses an unchecked index.  Scratch is library-owned and grow-only. */
int sdrm_nmf_fit(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, const int64_t* colptr, const int32_t* rowidx,
                 const float* cdata, int64_t m, int64_t n, int64_t nnz, int k, int max_iter, double tol, double* W, double* Ht, int32_t* n_iter_dev,
                 double* violations_dev, void* stream);
int sdrm_nmf_init(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t m, int64_t n, int64_t nnz, int k,
                  const float* components, const double* singular_values_host, double* W0, double* Ht0, void* stream);
int sdrm_nmf_scores(sdrm_engine* e, const double* W, const double* Ht, int64_t n_rows, int k, const int64_t* rows, int64_t row0, int b, int n_items,
                    float* scores, void* stream);

/* The NeuMF evaluator's forward on the device, EVAL MODE only (reference: neural_cf_benchmark_pt.py:125-144, `NCF.forward` of the
 * 'NeuMF-end' model with dropout off; csrc/neumf.h).  For a user u and an item i, factor F, three MLP layers:
 *   g = Pg[u] * Qg[i];  h1 = relu(W1 [Pm[u]; Qm[i]] + b1);  h2 = relu(W2 h1 + b2);  h3 = relu(W3 h2 + b3);  y = wp [g; h3] + bp
 * The struct holds DEVICE pointers to the twelve tensors of the live module as PyTorch stores them (float32, contiguous; a Linear's
 * weight is [out, in] row-major); they are read by the call, nothing is copied or re-packed on the host, and they are free again once
 * the call is ordered on `stream`.  factor must be 8, 16 or 32 (SDRM_ERR_SHAPE before any launch otherwise).
 * Arithmetic: fp32, every output element of every layer one fmaf chain in ascending k from its bias; layer 1 is split into a per-user and
 * a per-item half (staged once per listed id: one launch) whose sum enters the relu.  A logit has the same bits from either entry point,
 * at any position of a list and however a call is split.
 * Ids are int32 and are range-checked on the device into the status word sdrm_feed_status reports: a user id outside [0, n_users)
 * raises the row bit, an item id outside [0, n_items) the column bit; the offending row / column / logit is written as ZERO, adds
 * nothing to the loss, and no load uses the id.  Scratch is library-owned and grow-only: a call whose
 * scratch must grow - the first one, and each one with more listed ids or pairs than any before it on the handle - synchronises the
 * DEVICE and frees the old buffer before it allocates (such a call cannot run under graph capture); a call that fits does not synchronise.
 * sdrm_neumf_scores replaces :219-233 and :299-310 (the cartesian product of the validation users and the training items pushed through
 *   the model in batches of 10000 and moved to a Python list): out [n_listed_users, n_listed_items] float32 row-major, the matrix
 *   sdrm_rank_metrics takes, for users[0 .. n_listed_users) (any order, repeats allowed) and items[0 .. n_listed_items) - or, with items
 *   null, the items 0 .. n_items - 1 (n_listed_items must then be n_items).  Two launches.
 *   SDRM_ERR_SHAPE: no listed user or item, more than 2^20 - 16 listed users (16 per work-group on grid.y), more than 2^22 listed items, users x items at or above 2^40.
 * sdrm_neumf_pair_loss replaces :209-210 (the validation triples through the model and BCEWithLogitsLoss): for the n pairs (users[j],
 *   items[j]) logits [n] (may be null) and, with labels [n] float32, *loss_sum (a DEVICE double, may be null) = the sum over j of
 *   max(x, 0) - x y + log1p(exp(-|x|)), the numerator of BCEWithLogitsLoss's mean: fp32 terms, per-work-group float64 partials and a fixed
 *   final tree - no atomic, the same bits on every run.  Pairs are staged 65536 at a time: two launches per such chunk and one for the sum.
 *   SDRM_ERR_ARG: loss_sum without labels, or neither output; SDRM_ERR_SHAPE: n outside 1 .. 2^31 - 1. */
typedef struct sdrm_neumf {
  const float* embed_user_gmf; const float* embed_item_gmf;   /* Pg [n_users, F], Qg [n_items, F] */
  const float* embed_user_mlp; const float* embed_item_mlp;   /* Pm [n_users, 4F], Qm [n_items, 4F] */
  const float* w1; const float* b1;                           /* MLP_layers.1: [4F, 8F], [4F] */
  const float* w2; const float* b2;                           /* MLP_layers.4: [2F, 4F], [2F] */
  const float* w3; const float* b3;                           /* MLP_layers.7: [F, 2F], [F] */
  const float* wp; const float* bp;                           /* predict_layer: [1, 2F], [1] */
  int n_users, n_items, factor;
} sdrm_neumf;
int sdrm_neumf_scores(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, int n_listed_users, const int32_t* items, int n_listed_items,
                      float* out, void* stream);
int sdrm_neumf_pair_loss(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, const int32_t* items, const float* labels, int64_t n,
                         float* logits, double* loss_sum, void* stream);

/* The NeuMF evaluator's TRAIN steps on the device (reference: neural_cf_benchmark_pt.py:186-200, the batch loop of an epoch - `model.zero_grad()`,
 * `model(X[:, 0], X[:, 1])` in TRAIN mode :125-144, `BCEWithLogitsLoss` :197, `loss.backward()` :199 and `optimizer.step()` :200 of the
 * `optim.Adam` of :169; csrc/neumf_train.h).  With s = 1 / (1 - p_drop) and k0, k1, k2 the keep decisions of the three Dropout modules:
 *   a0 = k0 s [Pm[u]; Qm[i]];  a1 = k1 s relu(W1 a0 + b1);  a2 = k2 s relu(W2 a1 + b2);  h3 = relu(W3 a2 + b3);  g = Pg[u] * Qg[i]
 *   y = wp [g; h3] + bp;  loss = mean_j(max(y, 0) - y l + log1p(exp(-|y|)));  dy_j = (sigmoid(y_j) - l_j) / b
 * followed by the gradients of all twelve tensors and torch.optim.Adam's default DENSE update of all twelve (a table row outside the batch
 * still moves while its moments are non-zero), Adam's step count for step t of the call being step0 + t + 1.
 * The struct holds DEVICE pointers to the twelve LIVE tensors p (updated in place) and to their moments m = exp_avg, v = exp_avg_sq (the
 * same shapes, updated in place), in the order of sdrm_neumf's fields (= `state_dict()`): float32, contiguous, no two of them sharing a
 * byte (SDRM_ERR_ARG).  factor is 8 or 16; factor 32 is NOT built for training and is SDRM_ERR_SHAPE.
 * sdrm_neumf_train_steps replaces :186-200 for a whole pass over triples [n][3] int32 (user, item, label 0 / 1) on the device: ceil(n / batch)
 *   consecutive steps over the array in order, the last one partial, 1 <= batch <= 1024, 1 <= n <= 2^31 - 1.  Four launches per step, all
 *   enqueued on `stream`; nothing is read back and no step waits for the host.  Scratch is library-owned and grow-only: a call whose scratch
 *   must grow - the first one, and each one with larger tables than any before it on the handle - synchronises the DEVICE and frees the old
 *   buffer before it allocates (such a call cannot run under graph capture); a call that fits does not synchronise.
 *   Arithmetic is fp32; every sum (a weight gradient over the batch, the gradient of a table row that several pairs share, in ascending
 *   pair order, the loss: fp32 terms, float64 sum by a fixed tree) has a fixed order and there is no floating-point atomic: the same
 *   bits on every run, and a call over the whole array gives the bits of one call per batch.
 *   Ids are range-checked on the device: a pair with a user outside [0, n_users) or an item outside [0, n_items) raises the feed status word
 *   (sdrm_feed_status: "row" for a user, "column" for an item), contributes nothing to the loss or to any gradient and still counts in the
 *   divisor b; no load or store uses the id.
 *   Dropout: mode SDRM_RNG_EXPLICIT reads keep [n][14 factor] uint8 (per pair: 8 factor bytes of k0, 4 factor of k1, 2 factor of k2; non-zero
 *   = kept); SDRM_RNG_PHILOX ignores keep: column c of the pair at position j of `triples` is kept iff word c & 3 of Philox4x32-10 with
 *   counter (j, c >> 2, 10, call_id) and key seed is >= floor(p_drop 2^32), 0 <= p_drop < 1 - so a call is a function of (seed, call_id)
 *   and of nothing the host drew.
 *   losses: DEVICE double [ceil(n / batch)] that receives each step's loss, or null.  grads: HOST array of twelve DEVICE pointers that
 *   receive the dense gradients of the LAST step of the call (each the size of its tensor), or null.
 *   SDRM_ERR_ARG: a null pointer, EXPLICIT without keep, an unknown mode, step0 < 0, p_drop outside [0, 1), overlapping tensors;
 *   SDRM_ERR_SHAPE: factor outside {8, 16}, a table without rows, n or batch outside their ranges.  Refused calls launch nothing. */
typedef struct sdrm_neumf_train { float* p[12]; float* m[12]; float* v[12]; int n_users, n_items, factor; } sdrm_neumf_train;
int sdrm_neumf_train_steps(sdrm_engine* e, const sdrm_neumf_train* s, const int32_t* triples, int64_t n, int batch, int64_t step0, float lr,
                           float beta1, float beta2, float eps, float p_drop, int mode, const uint8_t* keep, uint64_t seed, uint32_t call_id,
                           double* losses, float* const* grads, void* stream);

/* An epoch's data preparation of the NeuMF evaluator on the device (reference: neural_cf_benchmark_pt.py:180-184 - `train_test_split` of the
 * training triples 80/20, the label-0 rows of the 80 % drawn again with replacement, one per label-1 row, the concatenation shuffled;
 * csrc/neumf_draw.h).  The reference's draws are unseeded; this call's are a function of (seed, epoch) and the triples alone, so that
 * tests/neumf_draw_ref.py restates it exactly in numpy.  triples [n][3] int32 (user, item, label) stay on the device across epochs.
 * The keyed permutation perm(n, seed, epoch, draw) of 0 .. n-1, n >= 1:  b = max(1, bit_length(n - 1)), h = (b + 1) / 2, mask = 2^h - 1 (the
 *   domain 4^h >= n).  For a value x: L = x >> h, R = x & mask; six rounds r = 0 .. 5 of (L, R) <- (R, L ^ (W & mask)), W = word 0 of
 *   Philox4x32-10 with counter (R, r, 12 | draw << 8, epoch) and key seed; then x = L << h | R.  perm(i) starts at x = i and repeats that map
 *   until x < n (cycle walking): a bijection of [0, n) - the construction of thrust::shuffle.  It is a good shuffle for batches and splits,
 *   every element is equally likely at every place, but it is NOT uniform over the n! orders (at tiny n it reaches only part of them).
 *   The device loop is bounded at 1024 applications; a lane that reaches the bound makes the call fail with SDRM_ERR_STATE, and nothing is
 *   promised about the outputs then (the longest walk seen over n up to 1.3 M was 43).
 * The draw, with n_part = n - n_hold:
 *   hold[j] = T[perm(n; draw 0)(j)], j < n_hold;   part[q] = T[perm(n; draw 0)(n_hold + q)], q < n_part;
 *   g_0 < g_1 < ... the places q where part[q] has label 0, n_neg of them; n_pos the number of places with label 1 (any other label counts
 *   in neither and passes through);   n_extra = n_pos if n_neg > 0, else 0;
 *   extra[k] = part[g_r], r = (w n_neg) >> 32, w = word k & 3 of Philox4x32-10 with counter (k >> 2, 0, 12 | 1 << 8, epoch) and key seed;
 *   m = n_part + n_extra;   out[p] = (part ++ extra)[perm(m; draw 2)(p)], p < m.
 * hold [n_hold][3] and out [capacity][3] (rows m .. capacity - 1 are left as they were) receive whole triples, verbatim.
 * present: null, or uint8 [n_users]: the call zeroes it and sets byte u for every user id u in [0, n_users) that occurs in hold; a hold
 *   triple with a user id outside that range raises the "row" bit of the feed status word (sdrm_feed_status), is not marked and is still
 *   copied verbatim (sdrm_neumf_train_steps range-checks its own ids).  With present null, n_users is ignored.
 * counts_host: HOST int64 [3] that receives n_pos, n_neg, m.
 * The call takes NO stream and is DEVICE-SYNCHRONOUS, like sdrm_set_schedule: it waits for the device (every stream) before its first
 *   launch, runs its four launches on a stream of the library's own and waits for them before it returns.  So inputs written by work queued
 *   earlier on any stream are seen, and the outputs and counts are complete on return: the host sizes the train call from m.  It cannot
 *   run under graph capture.  Scratch is library-owned and grow-only, as for sdrm_neumf_train_steps.  Integer work only: the same bytes on
 *   every run.
 * SDRM_ERR_SHAPE, before any launch: n outside 2 .. 2^30 (2 n_part stays an int32 index), n_hold outside 1 .. n - 1, capacity below
 *   2 (n - n_hold), n_users < 1 with present.  SDRM_ERR_ARG: a null handle, triples, hold, out or counts_host.  Refused calls launch and
 *   write nothing. */
int sdrm_neumf_epoch_draw(sdrm_engine* e, const int32_t* triples, int64_t n, int64_t n_hold, uint64_t seed, uint32_t epoch, int32_t* hold,
                          int32_t* out, int64_t capacity, uint8_t* present, int n_users, int64_t* counts_host);

/* The MLP evaluator's TRAIN steps on the device (reference: mlp_benchmark.py:37-62 the model, :85-110 `model.fit` with Keras's Adam and
 * `binary_crossentropy`; restated, with the Keras facts it rests on, in sdrm_amd/mlp_eval.py; csrc/mlp_train.h).  The input rows are 0 / 1,
 * given as the PATTERN of a device CSR matrix [n_rows, n_items] (an entry means 1).  With s = 1 / (1 - p_drop) and k1, k2, k3 the keep
 * decisions of the three Dropout layers:
 *   a0[r, 8j + f] = E[x_rj][f];  a1 = k1 s relu(a0 W1 + b1);  a2 = k2 s relu(a1 W2 + b2);  a3 = k3 s relu(a2 W3 + b3);  y = a3 W4 + b4
 *   loss = sum(max(y, 0) - y x + log1p(exp(-|y|))) / (b n_items);  dy = (sigmoid(y) - x) / (b n_items)
 * followed by the gradients of all nine tensors and Keras's Adam: alpha = lr sqrt(1 - beta2^t) / (1 - beta1^t), m += (g - m)(1 - beta1),
 * v += (g^2 - v)(1 - beta2), p -= alpha m / (sqrt(v) + eps), t = step0 + 1 for the first step of the call.  Of E only rows 0 and 1 are read
 * and updated (Keras's sparse embedding update).
 * The struct holds DEVICE pointers to the nine LIVE tensors p (updated in place) and to their moments m, v (the same shapes, updated in
 * place) in Keras's `get_weights()` order and layout, kernels [in][out]: E [n_users][8], W1 [8 n_items][512], b1 [512], W2 [512][256],
 * b2 [256], W3 [256][256], b3 [256], W4 [256][n_items], b4 [n_items]: float32, contiguous, every base on the 16-byte grid, no two of
 * them sharing a byte.
 * sdrm_mlp_train_steps runs ceil(n / batch) consecutive steps over rows [n] (int64 row ids of the CSR matrix, DEVICE) in order, the last
 *   one partial, all enqueued on `stream`; nothing is read back and no step waits for the host.  Neither the dense input [b][8 n_items]
 *   nor the gradient of W1 exists in memory (but in grads_out): a step is ONE read-modify-write pass over W1 and its moments.  Scratch
 *   is library-owned and grow-only, as for sdrm_neumf_train_steps.  Values are fp32, every sum is accumulated in float64 in a fixed
 *   order and rounded once, there is no floating-point atomic: the same bits on every run, and a call over n rows gives the bits of
 *   one call per batch.
 *   A row id outside [0, n_rows), an indptr pair out of order (such a row adds nothing to the loss or to any gradient) and a column
 *   outside [0, n_items) (skipped) raise the feed status word (sdrm_feed_status); the divisor b n_items still counts them.
 *   Dropout: mode SDRM_RNG_EXPLICIT reads keep [n][1024] uint8 (per row 512 bytes of k1, 256 of k2, 256 of k3; non-zero = kept);
 *   SDRM_RNG_PHILOX ignores keep: column c of the row at place j of `rows` is kept iff word c & 3 of Philox4x32-10 with counter
 *   (j, c >> 2, 11, call_id) and key seed is >= floor(p_drop 2^32).
 *   losses: DEVICE double [ceil(n / batch)], each step's loss.  grads_out: null, or a HOST array of nine DEVICE pointers (the tensors'
 *   shapes, the same alignment and no shared byte) that receive the gradients the update used - allowed for a call of ONE step only.
 *   SDRM_ERR_SHAPE: n_items outside 1 .. 36864, n_users < 2, batch outside 1 .. 16, n outside 1 .. 2^31 - 1, step0 < 0, p_drop outside
 *   [0, 1), n_rows < 1; SDRM_ERR_ARG: a null pointer, EXPLICIT without keep, an unknown mode, grads_out with more than one step, a tensor
 *   off the 16-byte grid, two tensors that share a byte.  Refused calls launch nothing. */
typedef struct sdrm_mlp_train { float* p[9]; float* m[9]; float* v[9]; int n_users, n_items; } sdrm_mlp_train;
int sdrm_mlp_train_steps(sdrm_engine* e, const sdrm_mlp_train* s, const int64_t* indptr, const int32_t* indices, int64_t n_rows, const int64_t* rows,
                         int64_t n, int batch, int64_t step0, float lr, float beta1, float beta2, float eps, float p_drop, int mode,
                         const uint8_t* keep, uint64_t seed, uint32_t call_id, double* losses, float* const* grads_out, void* stream);

/* The MLP evaluator's EVAL-MODE forward on the device (reference: mlp_benchmark.py:92 the `RootMeanSquaredError` metric, :109 the per-epoch
 * validation pass of `model.fit`, :114 `model.predict`; restated in sdrm_amd/mlp_eval.py; csrc/mlp_eval.h).  In inference the dropouts are
 * the identity; the input rows are 0 / 1, given as the PATTERN of a device CSR matrix [n_rows, n_items] with nnz entries:
 *   a1 = relu(b1 + sum_j E[x_rj] W1[8j ..]);  a2 = relu(a1 W2 + b2);  a3 = relu(a2 W3 + b3);  y = a3 W4 + b4;  p = sigmoid(y)
 * The struct holds DEVICE pointers to the nine LIVE tensors in sdrm_mlp_train's order and layout, every base on the 16-byte grid; they are
 * READ, nothing is re-packed on the host, and they are free again once the call is ordered on `stream`.
 * sdrm_mlp_eval evaluates the n rows rows[0 .. n) (DEVICE int64 row ids; any order, repeats allowed) or, with rows null, the rows row0 ..
 *   row0 + n - 1, looping over batches of `batch` rows itself.  out: null, or DEVICE float32 [n, n_items] contiguous that receives p (kind 0) or
 *   y (kind 1).  sse: null, or ONE DEVICE float64 that receives the sum over the n x n_items elements of (p - x)^2 - probabilities whatever
 *   `kind` says - the numerator of the RMSE.  With out null nothing of size n x n_items exists: one [batch][n_items] scratch buffer is reused.
 *   W1 is read ONCE per call: one pass folds it into a row per item, D[j] = sum_f (E[1][f] - E[0][f]) W1[8j + f] (float64 sums, rounded
 *   once), and the sums B_f = sum_j W1[8j + f]; a row's first layer is then a sum of its entries' rows of D in fp32.  Layers 2, 3 and the
 *   output layer are the fp32-MFMA GEMMs on weights staged once per call.  The SSE is SSE_r = sum_j p_rj^2 - sum_{j in row r} (2 p_rj - 1)
 *   per row in float64, the rows added in a fixed order by the call's last launch.  No floating-point atomic: two runs of a call give the
 *   same bits, and a row's output has the same bits wherever it stands in any call made with the same `batch` (the tile goes by `batch`).
 *   Launches: 7 per call (8 with sse) and 5 per batch - more only where the output layer goes out in row bands, never for a batch of
 *   at most 1792 rows; all enqueued on `stream`, nothing is read back and nothing synchronises.  Scratch is library-owned and grow-only,
 *   as for sdrm_neumf_train_steps.
 *   Range checks, into the status word sdrm_feed_status reports: a row id outside [0, n_rows), or an indptr pair that is negative, out of
 *   order or reaches behind nnz, makes a DEAD row - its row of out is zero and it adds nothing to sse; a column outside [0, n_items) is
 *   skipped by the first layer and by sse.  The columns of a row must be distinct.  No load or store uses an unchecked index.
 *   SDRM_ERR_SHAPE: n_items outside 1 .. 36864, n_users < 2, batch outside 1 .. 4096, n < 1, n_rows < 1, a contiguous range that starts below
 *   0 or ends behind n_rows, nnz < 0, n x n_items at or above 2^40, out and sse both null, a tensor off the 16-byte grid; SDRM_ERR_ARG: a
 *   null pointer, kind outside {0, 1}.  Refused calls launch nothing. */
typedef struct sdrm_mlp_eval_w { const float* p[9]; int n_users, n_items; } sdrm_mlp_eval_w;
int sdrm_mlp_eval(sdrm_engine* e, const sdrm_mlp_eval_w* w, const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows,
                  const int64_t* rows, int64_t row0, int64_t n, int batch, int kind, float* out, double* sse, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SDRM_HIP_H */
