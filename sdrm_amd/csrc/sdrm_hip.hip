// libsdrm_hip.so — C ABI (include/sdrm_hip.h) over the gfx950 kernels in gemm.h / elementwise.h.
// Host logic only: buffer ownership, launch orchestration of the train step / sampler, error codes.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <set>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/sdrm_hip.h"
#include "../../include/sdrm_hip_debug.h"
#include "compact.h"
#include "csr_transpose.h"
#include "decode.h"
#include "decoder_train.h"
#include "elementwise.h"
#include "encode.h"
#include "eval_half.h"
#include "exchange.h"
#include "feed.h"
#include "gemm.h"
#include "holdout.h"
#include "input_layer.h"
#include "latent.h"
#include "neumf.h"
#include "mlp_train.h"
#include "mlp_eval.h"
#include "neumf_draw.h"
#include "neumf_train.h"
#include "neumf_rank.h"
#include "neumf_triples.h"
#include "nll.h"
#include "nmf.h"
#include "rank.h"
#include "rowchain.h"
#include "rows48.h"
#include "sample_persist.h"
#include "select.h"
#include "skinny.h"
#include "skinny_step.h"
#include "skinny_fwd4.h"
#include "svd_eval.h"
#include "tail.h"
#include "vae_adam.h"
#include "dgrad_rows.h"
#include "wgrad2.h"

using namespace sdrm;

namespace {

constexpr int BM = 64;              // row padding granule = rows of the default tile (the 128-row alternates read into
                                    // the slack every buffer carries, and write rows nobody reads)
constexpr int S_MAX = 64;          // max split-K slabs per weight-gradient GEMM
constexpr int LOSS_BLOCKS = 256;

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

}  // namespace

// Tile / path selection of ONE engine: read from the environment once, in sdrm_create, changed afterwards only by the
// sdrm_debug_* setters of that handle (include/sdrm_hip_debug.h).  Nothing here is process-global: two engines on two
// threads never see each other's settings.
struct Tuning {
  int force_cfg = -1;            // SDRM_TILE: -1 = automatic, 0..4 forced tile shape
  int chains = -1;               // SDRM_CHAINS: sampler row chains, -1 = by size, 1..4 forced
  int detach = 1;                // SDRM_DETACH: the one chain of a small sampling call runs on an auxiliary stream (ChainSched)
  int hold_early = 1;            // SDRM_HOLD_EARLY: the chains of a sampling call wait for the weight gradients of a row-owned train step
                                 // queued between two of its steps (1) or for the whole step (0): chains_wgrads_queued
  int fuse_rev = 1;              // SDRM_FUSE_REV: reverse update fused into the out-layer GEMM epilogue (full-resolution PHILOX
                                 // sampling): 0 never, 1 for launches of at most FUSE_REV_MAX_ROWS rows, 2 always
  int skinny = 1;                // (2: with the 16-user train forward instead of the 4-user one) LDS-resident kernels for nets with padded widths <= 64 (persistent sampler, fused train
                                 // forward and dgrad chain)
  int nt32_max_rows = 4096;      // SDRM_NT32_MAX_ROWS: sampling / plain-forward NT launches of at most this many rows use the 32x32 tile
  int nt32_max_rows_train = 8192;  // SDRM_NT32_MAX_ROWS_TRAIN: the same for the train step's launches (stacked rows = 3 x batch):
                                 // 6144 stacked rows (a 4-GPU shard of the 8192 batch) 234 -> 226 us per step on the 32x32 tile,
                                 // 12288 a tie; the sampling launch of 5429 rows is faster on 64x64 (18.5 k vs 17.5 k steps/s)
  int wgrad_blocks = 2816;       // SDRM_WGRAD_BLOCKS: work-groups the batched weight-gradient launch of a step aims for (2.2 rounds of 5 per CU) ...
  int wgrad_round = 1280;        // SDRM_WGRAD_ROUND: ... unless ONE round (this many work-groups) already gives eight slices or more
  int wgrad_slices = 0;          // SDRM_WGRAD_SLICES: > 0 forces the K-slice count of every weight-gradient problem (tuning aid)
  int ar_buckets = 1;            // SDRM_AR_BUCKETS: gradient all-reduces of sdrm_train_step_sharded: 1 (after the whole backward) or 2 (overlapped)
  int dgrad_rows = 1;            // SDRM_DGRAD_ROWS: row-owned input gradients (csrc/dgrad_rows.h) behind the row-owned forward: 0 off,
                                 // 1 the whole chain (loss seeds + every layer) in one launch, 2 k_loss_seed + one launch per layer
  int strips = 1;                // SDRM_WGRAD_STRIPS: strip-owned weight gradients (csrc/wgrad2.h) behind the row-owned forward: 0 off
  int rows48 = 1;                // SDRM_ROWS48: the row-owned train step on 48-row work-groups (csrc/rows48.h: 16 users' P, S, Q rows; the
                                 // same nets as rowchain) for batches that do not fill the chip with 96-row work-groups: 0 never, 1 when
                                 // the batch's 16-user groups fill most of one round of the chip (see use_rows48), 2 whenever the net allows
  int rows48_share = 7;          // (bit 0: the forward, bit 1: the dgrad chain, bit 2: the forward's deferred-store sweep) SDRM_ROWS48_SHARE: the shared-tile form of the 48-row kernels (csrc/rows48.h: widths of 4 q + 2 column tiles - 352 is
                                 // 22 - no wave multiplies tiles beyond the layer; the waves of a pair split one tile's K-steps): 1 on, 0 the plain form
  int smp_persist = 1;           // SDRM_SAMPLE_PERSIST: reverse steps without kernel boundaries between the layers (csrc/sample_persist.h; full
                                 // resolution, PHILOX, L == W, one row chain): 0 never, 1 for at most SMP_PERSIST_MAX_ROWS (352) rows, 2 whenever it fits
  int split = 1;                 // SDRM_ROWS48_SPLIT: column-split row groups of that step (G work-groups of one XCD share a 48-row group and
                                 // exchange the activations through that XCD's L2, csrc/rows48.h) for batches of at most 2048 users:
                                 // 0 never, 1 by size (see rows48_parts), 2 / 4: that many work-groups per group whenever the grid fits the chip
  int rowchain = 1;              // SDRM_ROWCHAIN: row-owned train forward (csrc/rowchain.h) for nets with L == W, padded width 128..352:
                                 // 0 never, 1 when the batch fills whole rounds of one 96-row work-group per CU, 2 whenever the net allows
};

// The kernel path of ONE train step: decided once, by plan_step() in sdrm_train_forward, and frozen there.  The backward,
// sdrm_get_train_outputs and sdrm_get_preacts read it; none of them looks at the tuning values again, so what the forward left
// in the buffers and what the backward expects there cannot disagree (a sdrm_debug_set_* call takes effect at the next forward).
struct StepPlan {
  enum Path { PER_LAYER, SKINNY, ROW96, ROW48 };   // one launch per layer (64x64 / 32x32 tiles); the narrow nets' step (csrc/skinny_step.h);
                                                   // row-owned on 96-row (csrc/rowchain.h) / 48-row (csrc/rows48.h) work-groups
  enum Dgrad { TILES, ROWS_PER_LAYER, CHAIN, SKINNY_OWN };   // k_loss_seed + a tile GEMM per layer; k_loss_seed + a row-owned launch per layer
                                                   // (csrc/dgrad_rows.h); seeds + every layer in ONE row-owned launch; inside k_skinny_bwd
  Path path = PER_LAYER;
  Dgrad dgrad = TILES;
  int B = 0;                         // users of the step
  int parts = 1;                     // work-groups per row group (ROW48: 1, or 2 / 4 column-split)
  int groups = 0, users_per_group = 1;   // user groups of the stacked rows (PER_LAYER: every user its own)
  int rows = 0, MP = 0;              // stacked rows the forward really writes (whole groups), and the same rounded up to the tile
  int order = 0;                     // stacked row order (elementwise.h: stacked_row): 0 plain, 1 grouped by 32 users, 2 by 16
  int loss_parts = 0;                // loss partials the forward leaves (the narrow nets': G or 4 G, known once its forward is launched)
  bool acts_stored = false;          // the forward stores the activations prelu(pre[k]) in `act` beside pre[k] ...
  bool strips_ok = false;            // ... and a one-call backward may take the strip-owned weight gradients (csrc/wgrad2.h)
  // the row-owned dgrads read the activations: the forward need not store pre-activations (rowchain.h: skip_pre)
  bool skip_pre() const { return acts_stored && (dgrad == ROWS_PER_LAYER || dgrad == CHAIN); }
};

// ONE sampling call: what sdrm_sample_begin was given and what it decided from everything that is fixed for the call, written there
// in one place and read by every later entry point of the call.  sdrm_sample_steps counts i_next down; nothing else changes until the
// next sdrm_sample_begin (sdrm_debug_chains reports `chains` of the last call after it has ended).
struct SampleCall {
  enum Path { SKINNY, PERSIST, PER_LAYER };   // the narrow nets' one launch for the whole loop (csrc/skinny.h), issued by sdrm_sample_begin;
                                              // reverse steps without kernel boundaries (csrc/sample_persist.h: sample_persist_fits), taken
                                              // while the abort word is clear (persist_now), else as PER_LAYER; one launch per layer
  bool active = false;
  int n = 0, multires = 0, mode = 0; float nd = 1.f; const float *xT = nullptr, *z = nullptr; const uint8_t* keep = nullptr;   // the
  uint64_t seed = 0, call_id = 0; int64_t row0 = 0;                                                            // arguments of the call
  int MP = 0, i_next = 0;                     // n rounded up to the row granule; the next reverse step, 0: none left
  Path path = PER_LAYER;
  int chains = 1, chunk = 0;                  // row chains (chains_for) and the rows of each but the last
  // multi-resolution: active prefix per step (every row when full resolution), slot -> row, Tj by slot and by row
  std::vector<int> nact, perm;
  std::vector<int64_t> tj_sorted, tj_orig;
  uint32_t persist_phase = 0;                 // what the persistent kernel's row-tile counters (xcntS) stand at, in phases
};

// Where the row chains of the sampling call run and what their next launches wait for: touched by the chains_* functions and
// chains_join only (the rules, and what was measured, stand above them).
struct ChainSched {
  enum State { ON_CALLER,      // every chain on the caller's stream, nothing pending
               DETACH_ARMED,   // a train step was queued beside a small call: ev_fork marks the point behind the call's last step
               FORKED };       // chains on auxiliary streams, pending: joined by the next entry point that needs the result
  State state = ON_CALLER;
  bool detached = false;       // the ONE chain of a small call runs on aux[0], till the call ends (else: chain 0 on the caller's stream, c on aux[c - 1])
  // the train steps queued since the last sampling step
  bool train_queued = false;   // there was one: the chains' next launches come behind it
  bool train_row_owned = false;   // one of them was row-owned (one work-group per CU): the chains wait for such a step
  bool hold_marked = false;    // ev_hold is recorded behind its weight gradients
};

constexpr int PROF_SLOTS = 56;   // room for the profile classes (ProfClass below holds PC_COUNT to it)

// The library-owned device scratch of the utility entry points (sdrm_engine::scratch, reached through scratch<T>() only): one slot per
// buffer, every slot grow-only and owned by ONE family of entry points, so nothing a family leaves behind is touched by another.  Two
// promises of include/sdrm_hip.h rest on that: the encoder staged by sdrm_vae_encoder_load (ENC_W1T .. ENC_B2) survives every other
// call, and the workspace of a pending sdrm_equal_sparsity_csr_begin (CSR_WS) survives until its _end.
enum Scratch {
  // sdrm_vae_decode: padded latents, weights, hidden activations
  SCR_DEC_Z = 0, SCR_DEC_W1, SCR_DEC_B1, SCR_DEC_HID, SCR_DEC_W2, SCR_DEC_B2,
  // the frozen VAE encoder staged by sdrm_vae_encoder_load (csrc/encode.h): W1^T [items][Hq] | tiled W1, b1, W2, b2; and the encode calls'
  // normalised rows, hidden activations, [n][2 latent], densified rows, partial sums of the kl (k_encode_kl_rows, [KL_PARTS] float64)
  SCR_ENC_W1T, SCR_ENC_W1, SCR_ENC_B1, SCR_ENC_W2, SCR_ENC_B2, SCR_ENC_XN, SCR_ENC_HID, SCR_ENC_OUT2, SCR_ENC_DENSE, SCR_ENC_PART,
  // the train-mode input layer (csrc/input_layer.h): this call's W1^T [items][Hq] | dpre padded to [b][Hq] (hidden off the 16-byte grid only)
  SCR_IL_W1T, SCR_IL_DPRE,
  // the train-mode latent head (csrc/latent.h), this call's operands (h1, out2, eps are the caller's): h1 [MP][Hp] | W2 [L2r][Hp], b2 [L2r] |
  // W2^T [Hr][L2p] | dout2 [MP][L2p] | weight-gradient slabs [S][L2p][Hp], bias sums [S][L2p] | partial sums of its kl (k_latent_reparam)
  SCR_LAT_H, SCR_LAT_W2, SCR_LAT_B2, SCR_LAT_W2T, SCR_LAT_DOUT2, SCR_LAT_SLAB, SCR_LAT_DBIAS, SCR_LAT_PART,
  // the train-mode decoder and loss head (csrc/decoder_train.h), every one written by the call that reads it (h3, logits, lse are the
  // caller's): z [MP][Lp], W3 [Hr][Lp], b3 [Hr], h3 [MP][Hp], W4 [Ir][Hp], b4 [Ir] | W4^T [Hr][Ip], W3^T [Lr][Hp], zero bias [Lr], g [MP][Ip],
  // dpre3 [MP][Hp], slabs [S][Ip][Hp] + bias sums [S][Ip] of dW4, slabs [S][Hp][Lp] + bias sums [S][Hp] of dW3
  SCR_DH_Z, SCR_DH_W3, SCR_DH_B3, SCR_DH_H3, SCR_DH_W4, SCR_DH_B4, SCR_DH_W4T, SCR_DH_W3T, SCR_DH_ZB, SCR_DH_G, SCR_DH_DP3, SCR_DH_SLAB4,
  SCR_DH_DB4, SCR_DH_SLAB3, SCR_DH_DB3,
  // sdrm_vae_eval_holdout (csrc/eval_half.h), the live weights staged by that call and its batches' hand-overs: W1^T [items][Hq], b1 [Hr],
  // W2[:L] [Lr][Hp], b2[:L] [Lr], W3 [Hr][Lp], b3 [Hr], W4 [Ir][Hp], b4 [Ir] | h1 [MP][Hp], z [MP][Lp], h3 [MP][Hp], logits [batch][items]
  // (when the caller gives none)
  SCR_EV_W1T, SCR_EV_B1, SCR_EV_W2, SCR_EV_B2, SCR_EV_W3, SCR_EV_B3, SCR_EV_W4, SCR_EV_B4, SCR_EV_H1, SCR_EV_Z, SCR_EV_H3, SCR_EV_LOGITS,
  SCR_HOLD_CNT,      // sdrm_holdout_split (csrc/holdout.h): uint32 [2][rows] entries n_u and held entries m_u of every row
  // sdrm_svd_fit / sdrm_svd_scores (csrc/svd_eval.h): the fit's panels Q [n][32] | Y [m][32]; the scores' V^T [n][32] | T [b][32]; the Gram
  // partials [SVD_GRAM_PARTS][32][32] with R^-1 [32][32] behind them (float64); the fit's status word (bit 0: breakdown)
  SCR_SVD_PANEL, SCR_SVD_VT, SCR_SVD_PART, SCR_SVD_FLAG,
  // sdrm_neumf_scores / sdrm_neumf_pair_loss (csrc/neumf.h): W2t | W3t | the staged user and item sides; the validity words of both sides
  // (int); the pair kernel's per-block loss partials (float64)
  SCR_NEUMF_WS, SCR_NEUMF_VALID, SCR_NEUMF_PART,
  // sdrm_neumf_train_steps (csrc/neumf_train.h): the step's column-major workspace [NtCols::COUNT][NT_LD] with the dense gradients of the
  // eight tower tensors behind it | the dense gradients of the four embedding tables, ALL ZERO between two calls (a step writes the rows
  // its pairs name and zeroes them again): nothing else may ever be carved out of that slot
  SCR_NEUMF_TRAIN_WS, SCR_NEUMF_TRAIN_TAB,
  // sdrm_neumf_epoch_draw (csrc/neumf_draw.h), 8-byte words, every piece written by the call that reads it: [counts int64 [3] | status word |
  // label-0 mask words | part_src int32 [n_part] | neg_src int32 [n_part] | work-group counts uint32 [2][blocks] | their scan uint32 [blocks]]
  SCR_NEUMF_DRAW_WS,
  // sdrm_mlp_train_steps (csrc/mlp_train.h), 8-byte words: [B_f of the weights, two copies | the W1 pass's partial B_f and dE[1] | the gather's
  // partial sums | loss partials | a1, a2, a3, dz1, dz2, dz3, dy (float) | live words | item mask]
  SCR_MLP_TRAIN_WS,
  // sdrm_mlp_eval (csrc/mlp_eval.h), 8-byte words, every piece written by the call that reads it: [B_f | the fold's partial B_f | the rows' SSE
  // | D [items][512], base, the zero slope, W2^T, W3^T, W4^T [Ir][256], b4 [Ir], a1, a2, a3 [MP][.] (float) | the batch's [batch][items] output
  // (when the caller gives none)]
  SCR_MLP_EVAL_WS,
  SCR_CSR_WS,        // sdrm_equal_sparsity_csr_begin / _end (csrc/compact.h), 8-byte words: [mask words | row offsets int64 | row counts uint32]
  // sdrm_csr_transpose / sdrm_csr_vstack (csrc/csr_transpose.h), 8-byte words: [checked | total | bit table | colptr int64 | offsets uint32 |
  // column counts uint32] and [total | indptr int64 | row lengths uint32]
  SCR_CSRT_WS, SCR_STACK_WS,
  // sdrm_neumf_triples (csrc/neumf_triples.h), 8-byte words, cleared on the stream by every call: [total | row bases int64 [rows + 1], twice
  // (k_csr_scan writes two copies) | row lengths uint32]
  SCR_TRIPLE_WS,
  // sdrm_neumf_rank_problem (csrc/neumf_rank.h), 8-byte words, cleared on the stream by every call: [totals int64 [2] | bit table of seen,
  // of relevant [n_rows][wpr] | row offsets int64 [n_rows + 1] of seen, of relevant (the scan's own copies) | row lengths uint32 [n_rows] of
  // seen, of relevant | col_of int32 [n_items]]
  SCR_RANK_WS,
  // sdrm_nmf_fit (csrc/nmf.h), float64: [the fit's state (2) | Gram partials [NMF_PARTS][16][16] | the product [max(m, n)][16] | violation
  // partials of the W half, of the H half]; sdrm_nmf_init, float64: [mean, sigma [16] (32) | norm partials of U, of V [NMF_PARTS][2][16] each
  // | V^T [n][16] | X V^T [m][16]]
  SCR_NMF_FIT, SCR_NMF_INIT,
  SCR_COUNT
};

struct sdrm_engine {
  int L, W, T, H, max_rows, device;
  Tuning tune;
  int LP, WP, TP, K0, MPmax;
  int64_t P;
  int64_t off_we, off_be, off_w0, off_b0, off_a0, off_wh, off_bh, off_ah, off_wo, off_bo;
  // flat master copies
  float *p = nullptr, *m = nullptr, *v = nullptr, *g = nullptr;
  // padded compute copies
  float *W0c = nullptr, *b0c = nullptr, *Whc = nullptr, *bhc = nullptr, *Woc = nullptr, *boc = nullptr;
  float *WhcT = nullptr, *WocT = nullptr;   // transposed copies [in][out]: dgrad is then an NT GEMM like the forwards
  float *WhfT = nullptr, *WofT = nullptr;                 // the same of the transposes ([k = out][n = in]) for the row-owned dgrads
  float *W0f = nullptr, *Whf = nullptr, *Wof = nullptr;   // fragment-packed copies [WP/16][WP/16][64][4] for the row-owned forward
                                                          // (layer 0: the latent columns only); null when the net does not qualify
  StepPlan plan;                     // what the last train_forward ran on (plan_step)
  // column-split row groups: hand-shake counters of the forward / of the dgrad chain [256 groups][32], never reset while the
  // launch geometry stays the same (xgeo); the abort word lives in host-visible memory (xabort_host / its device alias)
  unsigned *xcntF = nullptr, *xcntC = nullptr;
  unsigned *xabort_host = nullptr, *xabort_dev = nullptr;
  uint32_t xepochF = 0, xepochC = 0;
  int xgeoF = 0, xgeoC = 0;           // (parts << 16 | groups) of the launches the counters have counted
  bool xcd_ok = false;               // the probe launch of sdrm_create found work-group b on XCD b & 7
  unsigned* xcntS = nullptr;         // the persistent sampler's row-tile counters [256][32] (SampleCall::persist_phase: what they stand at)
  unsigned xskew = 0;                // test hook (sdrm_debug_split_skew): added once to the next split launch's counter base
  bool tables_fresh = false;         // B0tab / the C0^T columns of W0c belong to the current parameters
  float* act = nullptr;              // activations prelu(pre[k]) [H+1][MPmax][WP], written by the row-owned forward beside pre[k]:
                                     // the weight gradients of that step read their operand without PReLU on load
  int ones_col = -1;                 // pad column round_up(W, 4) < WP of the layer inputs that carries 1.0 (the padded biases put it there,
                                     // the row-owned forward's staging into U): column ones_col of a weight-gradient slab is then the
                                     // bias gradient (csrc/wgrad2.h); -1: none
  bool bwd_strips = false;           // this backward's weight gradients: the strip-owned launch (bias gradients in slab column ones_col)
  float *temb = nullptr, *tembP = nullptr, *B0tab = nullptr;   // time-embedding table [T+1][T]; the same with rows padded to TP (the
                                                               // trailing columns of the train step's layer-0 operand); b0 + C0[t]
  float *sched = nullptr;  // [8][T+1]: beta alpha alphabar sqrt_ab one_minus_ab
  float *Us = nullptr;               // sampler's own layer-0 input [rows][LP] (survives train steps between sample_steps calls)
  float *smp_pre = nullptr, *smp_Y = nullptr;   // ... and its own layer buffers / eps-net output: a train step between two sampling steps
                                     // shares nothing with the call in progress (sdrm_train_forward: no join of the row chains)
  float *U = nullptr, *pre = nullptr, *Y = nullptr, *dY = nullptr, *dA = nullptr, *X = nullptr;
  float *slab0 = nullptr, *slabH = nullptr, *slabO = nullptr, *db0s = nullptr, *dbHs = nullptr, *dbOs = nullptr;
  float *alpha_part = nullptr;
  int alpha_part_stride = 0;
  double *loss_part = nullptr, *sums = nullptr;
  float *WeP = nullptr, *W0eP = nullptr;    // narrow nets with T <= 128: padded copies of emb_layer.weight [TPe][TPe] and of W0e [WP][TPe]
  int TPe = 0;                              // (TPe = T rounded up to 16): the forward makes its own rows of the time-embedding table
  float *Mred = nullptr, *snap = nullptr;   // the tail's hand-over to its second launch (csrc/tail.h): M [W][TP]; We | be | W0e before the update
  int *tdev = nullptr;
  int64_t *Tj_dev = nullptr;
  int *rowid_dev = nullptr;
  const float* grad_src = nullptr;   // where the last backward wrote the flat gradient (internal g or the caller's buffer)
  float *rev_dev = nullptr;          // [3][T+1] reverse-step coefficients c1, sqrt(alpha), sqrt(beta)
  SelectState* sel = nullptr;        // radix-select workspace of sdrm_equal_sparsity
  // sdrm_equal_sparsity_csr_begin / _end (csrc/compact.h): the call pending between the two (its workspace: SCR_CSR_WS)
  int64_t *csr_nnz_host = nullptr, *csr_nnz_dev = nullptr;   // nnz of the scan, in host memory the device writes (and its device alias)
  struct CsrPending { bool active = false; int64_t n_rows = 0, nnz = 0; int wpr = 0; size_t off_ptr = 0; } csr;
  float* one_dev = nullptr;          // 1.0f (identity PReLU slope for layer 0 inside the batched weight-gradient launch)
  unsigned* feed_flag = nullptr;     // status word of the sparse batch feed (csrc/feed.h: out-of-range row ids / column indices)
  std::vector<float> h_beta, h_alpha, h_alphabar;
  int64_t adam_t = 0;
  // state of the last train_forward
  const float* fwd_x0 = nullptr;    // its batch (the backward's loss seeds read it again)
  bool fwd_done = false;
  bool fwd_params_live = false;     // no parameter has changed since that forward (sdrm_get_preacts rebuilds from the live PReLU slopes)
  int last_S = 1, last_dgrad_blocks = 0;
  bool bwd_begun = false;
  int bwd_S0 = 1, bwd_SH = 1, bwd_SO = 1, bwd_kc0 = 0, bwd_kcH = 0, bwd_kcO = 0, bwd_dgrad_blocks = 0;
  int bwd_hidden_apps = 0;           // slab sets of the shared hidden layer's weight gradient per K-slice: H (one per application), or 1 (already summed)
  int bwd_cfg_w = 0;                 // tile of the split-K launches, fixed by backward_chain for the whole backward
  struct { void* p = nullptr; size_t cap = 0; } scratch[SCR_COUNT];   // the pool (enum Scratch); cap in elements of the slot's one type
  bool enc_loaded = false;
  double* nll_part = nullptr;        // partial sums of the multinomial loss (k_nll_rows), [NLL_PARTS]
  int csrt_mark_mode = 0;            // sdrm_debug_set_csrt_mark: 0 by the matrix's width, 1 global atomics, 2 LDS tiles
  int enc_items = 0, enc_hidden = 0, enc_latent = 0;
  Exchange xch;                      // RCCL communicator of the user-sharded step (sdrm_comm_init_rank / sdrm_allreduce_init)
  mutable int64_t n_launches = 0;    // kernel launches issued through this handle since sdrm_create
  // The sampler's own copy of everything it reads of the net (padded weights, biases, the folded bias table b0 + C0[i], the two
  // PReLU slopes), taken by sdrm_sample_begin: a sampling call is a function of the parameters at its begin, whatever
  // sdrm_set_params or train steps do between its sdrm_sample_steps calls (the persistent narrow-net sampler, one launch
  // for the whole loop, is issued by sdrm_sample_begin itself and so reads the parameters of that moment).
  float* smp_w = nullptr;
  size_t smp_off[7] = {0, 0, 0, 0, 0, 0, 0};   // W0c, Whc, Woc, bhc, boc, B0tab, slopes
  SampleCall call;
  // sampler row chains: row ranges of one sampling call on streams of their own (ChainSched)
  hipStream_t aux[3] = {nullptr, nullptr, nullptr};
  hipStream_t draw_stream = nullptr;   // sdrm_neumf_epoch_draw's own stream (a device-synchronous call: made on its first call)
  hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
  hipEvent_t ev_hold = nullptr;      // behind the weight gradients of a train step that runs between two sampling steps (chains_wgrads_queued)
  ChainSched chain_sched;
  // event profiling (bench only)
  bool prof_on = false;
  int prof_cap = 0;
  int prof_only = -1;                   // >= 0: only launches of this class are bracketed (sdrm_profile_only)
  std::vector<hipEvent_t> prof_ev;      // 2 per recorded launch
  std::vector<int> prof_cls;
  std::vector<double> prof_flops;
  double prof_ms[PROF_SLOTS] = {0};
  double prof_fl[PROF_SLOTS] = {0};
  int64_t prof_n[PROF_SLOTS] = {0};
  std::string err;
};

constexpr int NLL_PARTS = 2048;   // most work-groups of k_nll_rows (8 per CU): the float64 partials k_nll_sum adds (csrc/nll.h)

enum ProfClass { PC_FWD_L0 = 0, PC_FWD_HIDDEN, PC_FWD_OUT, PC_DGRAD, PC_WGRAD, PC_WGRAD_L0, PC_SMP_L0, PC_SMP_HIDDEN,
                 PC_SMP_OUT, PC_ROW_FWD, PC_WGRAD_STRIPS, PC_DGRAD_ROWS, PC_SMP_PERSIST, PC_NLL, PC_INPUT_LAYER, PC_HOLDOUT, PC_LATENT, PC_DECODER, PC_VAE_ADAM, PC_EVAL_HALF, PC_SVD_SPMM, PC_SVD_GRAM, PC_SVD_CHOL, PC_SVD_APPLY, PC_SVD_EXPAND, PC_NEUMF_STAGE, PC_NEUMF_SCORES, PC_NEUMF_PAIRS, PC_NEUMF_TRAIN_PAIRS, PC_NEUMF_TRAIN_GRADS, PC_NEUMF_TRAIN_ADAM, PC_NEUMF_TRAIN_CLEAR, PC_CSRT_MARK, PC_CSRT_COLSCAN, PC_CSRT_SCAN, PC_CSRT_FILL, PC_CSR_VSTACK, PC_NMF_STEP, PC_NMF_INIT, PC_NMF_EXPAND, PC_MLP_FWD, PC_MLP_BWD, PC_MLP_W1, PC_MLP_FOLD, PC_MLP_EVAL, PC_NEUMF_DRAW_SPLIT, PC_NEUMF_DRAW_SCAN, PC_NEUMF_DRAW_NEG, PC_NEUMF_DRAW_OUT, PC_NEUMF_TRIPLES, PC_NEUMF_RANK_PROBLEM, PC_NEUMF_RANK_USERS, PC_RANK_ROWS, PC_COUNT };
static_assert(PC_COUNT <= PROF_SLOTS, "sdrm_engine::prof_ms / prof_fl / prof_n hold one slot per class");
// the template arguments are <LOADA,LOADB,XFA,XFB,EPI> of gemm_kernel (what rocprofv3 prints after the tile type)
static const char* kProfNames[PC_COUNT] = {
    "train: gemm_kernel<0,0,0,0,9> fwd layer0 (row-table bias)", "train: gemm_kernel<0,0,1,0,0> fwd hidden (prelu-in, bias)",
    "train: gemm_kernel<0,0,1,0,1> fwd out (prelu-in, tanh)",
    "train: gemm_kernel<0,0,0,0,3> dgrad (prelu' epilogue)",
    "train: gemm_batch_kernel<1,1,0,1,4> wgrad of all layers in one launch (prelu-in, split-K slabs)",
    "train: gemm_kernel<1,1,0,0,4> wgrad layer0 (split-K slabs)",
    "sample: gemm_kernel<0,0,0,0,10> fwd layer0 (bias table, prelu epilogue)", "sample: gemm_kernel<0,0,0,0,10> fwd hidden (bias, prelu epilogue)",
    "sample: gemm_kernel<0,0,0,0,1> fwd out (tanh)",
    "train: k_row_fwd row-owned forward (staging + all layers + loss partial sums, one work-group per CU)",
    "train: k_wgrad_strips weight gradients of all layers (strip-owned split-K, one work-group per CU)",
    "train: k_dgrad_chain / k_dgrad_rows input gradients (row-owned, prelu' epilogue, one work-group per CU; the chain: loss seeds + every layer in one launch)",
    "sample: k_sample_persist reverse steps without kernel boundaries (all layers + reverse update per step, row tiles synchronised through one XCD's L2)",
    "loss head: k_nll_rows / k_nll_grad multinomial NLL of logits against CSR rows and its gradient (one work-group per row, HBM-bound)",
    "input layer: k_input_fwd / k_input_wgrad train-mode first Linear of the VAE encoder from CSR rows and its weight gradient from CSC columns",
    "hold-out: k_holdout_counts / k_holdout_scan / k_holdout_split per-user hold-out split of a CSR matrix into two (keys ranked per row, a wave or a work-group per row)",
    "latent head: k_latent_stage / gemm_kernel<0,0,0,0,7> / k_latent_reparam forward, k_latent_stage_bwd / k_latent_seed / gemm_kernel<1,1,0,0,4> / gemm_kernel<0,0,0,0,11> / k_latent_unpad backward of the VAE encoder behind its first pre-activation in train mode",
    "decoder head: k_pad2d / gemm_kernel<0,0,0,0,1> / k_dechead_h3 / gemm_kernel<0,0,0,0,7> / k_nll_rows / k_nll_sum forward, k_dechead_stage_bwd / k_dechead_grad / gemm_kernel<1,1,0,0,4> / gemm_kernel<0,0,0,0,11> / gemm_kernel<0,0,0,0,7> / k_dechead_unpad backward of the VAE decoder and the multinomial loss in train mode",
    "optimizer: k_vae_adam / k_vae_loss_slot Adam over the VAE pre-stage's parameter tensors in one launch (with the L2 partial sums) and the step's loss value into its slot",
    "evaluation half: k_pad2d / k_encode_w1t staging once per call, then per batch k_encode_csr_checked / gemm_kernel<0,0,0,0,0> / gemm_kernel<0,0,0,0,1> / gemm_kernel<0,0,0,0,7> / k_rank_metrics_checked: the VAE's eval-mode forward from the CSR rows of a hold-out split and Recall@k / NDCG@k of its scores",
    "svd evaluator: k_svd_spmm sparse x [., 32] panel product from CSR / CSC rows (fixed summation order)",
    "svd evaluator: k_svd_gram float64 partials of the panel's Gram matrix",
    "svd evaluator: k_svd_chol partials summed, 32 x 32 Cholesky factor and its inverse in float64 (one work-group)",
    "svd evaluator: k_svd_apply panel times R^-1, row by row",
    "svd evaluator: k_svd_start / k_svd_vt / k_svd_expand start panel, V^T staging and the rank-k expansion into dense scores",
    "neumf evaluator: k_neumf_stage layer 1 split per listed user / item, the GMF rows, W2 and W3 transposed",
    "neumf evaluator: k_neumf_scores eval-mode forward of all listed users x listed items (fp32 vector FMAs, scalar weight operands)",
    "neumf evaluator: k_neumf_pairs / k_neumf_loss_sum eval-mode forward of listed pairs and the BCE-with-logits numerator (float64 partials, fixed order)",
    "neumf train step: k_nt_pairs train-mode forward with dropout, loss terms and the backward down to the embedding rows, a lane per pair (fp32 vector FMAs, scalar weight operands)",
    "neumf train step: k_nt_grads weight and bias gradients of the tower (fixed pair order), the dense table-gradient rows of the batch, the loss (float64, fixed tree)",
    "neumf train step: k_vae_adam dense Adam over the twelve tensors in one launch",
    "neumf train step: k_nt_clear the batch's rows of the dense table gradients zeroed again",
    "csr transpose: k_csrt_mark_lds / k_csrt_mark one pass over the entries, a row's bit into the row-blocked bit table (LDS column tiles, or 64-bit global atomics into a table cleared first), the count of checked entries",
    "csr transpose: k_csrt_colscan a thread per column, running popcounts over the row blocks and the column counts",
    "csr transpose: k_csr_scan column counts -> colptr (one work-group)",
    "csr transpose: k_csrt_fill one pass over the entries, row index and value to the place the bit table gives",
    "csr vstack: k_stack_counts / k_csr_scan / k_stack_copy checked row lengths, indptr, and the copy of up to 8 CSR parts one under the other",
    "nmf evaluator: k_nmf_prod / k_nmf_sweep / k_nmf_stop sparse x [., 16] float64 product with the Gram partials, the coordinate-descent sweep (a lane per row) and the stop rule",
    "nmf evaluator: k_nmf_vt / k_nmf_mean / k_nmf_norms / k_nmf_init the NNDSVDa start from the truncated SVD's factors",
    "nmf evaluator: k_nmf_expand the rank-k expansion W H into dense float32 scores (float64 sums, rounded once)",
    "mlp train step: k_mlp_mask / k_mlp_gather / k_mlp_z1 / k_mlp_fwd train-mode forward from CSR rows with the three dropouts, the loss terms and dy",
    "mlp train step: k_mlp_dgrad / k_mlp_adam / k_mlp_embed / k_mlp_bsum input gradients, Keras's Adam on W2 .. b4 and on E's two rows with the gradient made inside the pass, the loss, B_f",
    "mlp train step: k_mlp_w1 the one read-modify-write pass over W1 and its moments (gradient per element from S and T_j, Keras's Adam, partial B_f and dE[1])",
    "mlp evaluation: k_mlp_fold the one read-only pass over W1 that leaves D [items][512] and the partial B_f",
    "mlp evaluation: k_mlp_bsum / k_mlp_base / k_pad2d / k_encode_w1t staging once per call, then per batch k_mlp_rows_relu / gemm_kernel<0,0,0,0,10> x2 / gemm_kernel<0,0,0,0,7> or <0,0,0,0,12> / k_mlp_sse, and k_mlp_sse_sum: the eval-mode forward from CSR rows, probabilities or logits, and the sum of squared errors",
    "neumf epoch draw: k_draw_split the hold-out rows gathered through the keyed Feistel permutation and `present` marked; the source places, label-0 mask words and work-group counts of the other rows",
    "neumf epoch draw: k_draw_scan exclusive scan of the work-groups' label-0 counts with a carry, n_pos, n_neg and m (one work-group)",
    "neumf epoch draw: k_draw_neg the source places of the label-0 rows in ascending order, from the mask words and the scanned offsets",
    "neumf epoch draw: k_draw_out the shuffled rows gathered through the second permutation, the extra rows' Philox draws among the label-0 rows",
    "neumf triples: k_triple_counts / k_csr_scan / k_triple_fill checked row lengths, the rows' bases, and the (user, item, label) records of up to 8 CSR parts with item_present and the four counts",
    "neumf ranking problem: k_rank_cols / k_rank_mark_parts / k_rank_mark_held / k_rank_counts / k_csr_scan x2 / k_rank_fill the columns, the seen and the relevant CSR matrix by user id from up to 8 CSR parts and the held-out triples (one bit table each, 64-bit integer atomics)",
    "neumf ranking users: k_rank_users a uint8 mask compacted into the ascending user list and its length (one work-group)",
    "rank metrics by rows: k_rank_metrics_rows the checked ranking body with a row map into both CSR matrices and the NeuMF footing of the NDCG"};

namespace {

#define HIP_TRY(e, call)                                                                   \
  do {                                                                                     \
    hipError_t _st = (call);                                                               \
    if (_st != hipSuccess) {                                                               \
      (e)->err = std::string(#call) + ": " + hipGetErrorString(_st);                       \
      return SDRM_ERR_HIP;                                                                 \
    }                                                                                      \
  } while (0)

// every kernel launch goes through here: the handle counts them (sdrm_launch_count: launches per step for bench.py)
#define SDRM_LAUNCH(eng, ...)                      \
  do {                                             \
    if (eng) ++(eng)->n_launches;                  \
    hipLaunchKernelGGL(__VA_ARGS__);               \
  } while (0)

int fail(sdrm_engine* e, int code, const std::string& msg) {
  if (e) e->err = msg;
  return code;
}

// The batch of CSR rows of an entry point (csrc/csr_batch.h): the checks that all of them make, and the kernels' descriptor.  The
// caller has looked at `e` and keeps the limits that are its own.
int csr_batch(sdrm_engine* e, const char* who, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows,
              const int64_t* rows, int64_t row0, int b, int n_items, CsrBatch* out) {
  if (!indptr || !indices) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (b < 1 || n_items < 1 || n_rows < 1 || row0 < 0) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": b < 1, n_items < 1, n_rows < 1 or row0 < 0");
  if (!rows && row0 + b > n_rows) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": rows row0 .. row0 + b - 1 end behind the matrix");
  *out = CsrBatch{indptr, indices, data, rows, row0, n_rows, b, n_items, e->feed_flag};
  return SDRM_OK;
}

constexpr size_t SLACK = 4096;  // elements of zeroed tail on every buffer: unguarded tile loads may run past a matrix

// Dynamic LDS above 48 KB needs the kernel's limit raised.  Raised ONCE per kernel and process, to the whole 160 KB of a CU (less
// what a kernel declares statically: its caller says so in `bytes`): a per-launch call is host time on every step of the narrow
// nets, and a per-engine value would let a second engine with a smaller image lower the limit under a first one with a larger image.
constexpr int LDS_MAX_BYTES = 160 * 1024;
hipError_t allow_full_lds(const void* kernel, int bytes = LDS_MAX_BYTES) {
  static std::mutex mu;
  static std::set<const void*> done;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count(kernel)) return hipSuccess;
  const hipError_t st = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
  if (st == hipSuccess) done.insert(kernel);
  return st;
}

// The zeroing goes to the default stream and hipMemset does not wait for it: behind a busy default stream it would land on a buffer that a
// caller's non-blocking stream has long written (tests/test_stream_order.py met it in the mask of sdrm_equal_sparsity_csr_begin).  So
// the allocation waits for it - a call whose scratch grows may synchronise (include/sdrm_hip.h, Conventions).
template <typename Tp>
hipError_t dalloc(Tp** p, size_t n) {
  hipError_t st = hipMalloc((void**)p, (n + SLACK) * sizeof(Tp));
  if (st != hipSuccess) return st;
  st = hipMemset(*p, 0, (n + SLACK) * sizeof(Tp));
  if (st != hipSuccess) return st;
  return hipStreamSynchronize(nullptr);
}

// One buffer of the scratch pool (enum Scratch), as elements of Tp: *out holds n of them afterwards (and SLACK zeroed ones behind).
// Grow-only: a buffer that is too small is freed behind a device synchronise (a launch may still read it) and its contents are not
// kept.  scratch_at: the buffer as it stands (null before its first scratch()).
template <typename Tp>
int scratch(sdrm_engine* e, Scratch slot, size_t n, Tp** out) {
  auto& s = e->scratch[slot];
  if (n > s.cap) {
    if (s.p) { HIP_TRY(e, hipDeviceSynchronize()); HIP_TRY(e, hipFree(s.p)); s.p = nullptr; s.cap = 0; }
    HIP_TRY(e, dalloc((Tp**)&s.p, n));
    s.cap = n;
  }
  *out = (Tp*)s.p;
  return SDRM_OK;
}
template <typename Tp = float>
Tp* scratch_at(const sdrm_engine* e, Scratch slot) { return (Tp*)e->scratch[slot].p; }

float* pre_buf(sdrm_engine* e, int k) { return e->pre + (size_t)k * e->MPmax * e->WP; }
float* smp_buf(sdrm_engine* e, int k) { return e->smp_pre + (size_t)k * e->MPmax * e->WP; }   // the sampler's layer buffers
float* dpre_buf(sdrm_engine* e, int k) { return e->dA + (size_t)k * e->MPmax * e->WP; }   // d loss / d pre-activation k
const float* slope_ptr(sdrm_engine* e, int layer) { return e->p + (layer == 0 ? e->off_a0 : e->off_ah); }

// ---- GEMM launch helpers ----------------------------------------------------------------------
struct Prof { sdrm_engine* e; int cls; double flops; };

// ONE launch between the two events of an event profile (sdrm_profile_begin): recorded only while the profile is on, has room,
// and takes this class (sdrm_profile_only); a null engine (the sdrm_debug_gemm* entry points) records nothing.  `launch` issues
// the kernel and returns its status.
template <class Launch>
hipError_t profiled(sdrm_engine* e, int cls, double flops, hipStream_t st, Launch&& launch) {
  const bool rec = e && e->prof_on && (int)e->prof_cls.size() < e->prof_cap && (e->prof_only < 0 || e->prof_only == cls);
  size_t slot = 0;
  if (rec) {
    slot = e->prof_cls.size();
    e->prof_cls.push_back(cls);
    e->prof_flops.push_back(flops);
    const hipError_t st0 = hipEventRecord(e->prof_ev[2 * slot], st);
    if (st0 != hipSuccess) return st0;
  }
  hipError_t rc = launch();
  if (rec && rc == hipSuccess) rc = hipEventRecord(e->prof_ev[2 * slot + 1], st);
  return rc;
}
// ... for the launch helpers that return SDRM_* codes: the status of profiled(), with the kernel's name in the message
int hip_rc(sdrm_engine* e, const char* kernel, hipError_t st) {
  return st == hipSuccess ? SDRM_OK : fail(e, SDRM_ERR_HIP, std::string(kernel) + ": " + hipGetErrorString(st));
}
// ONE kernel launch as its own interval of class `cls` (with its flops, if it counts any): counted like every launch, the kernel's name
// in the message of a HIP error.  PC_NONE: a launch that no profile brackets - profiled() is not called at all (it records every class
// while sdrm_profile_only is off).
constexpr int PC_NONE = -1;
struct LaunchClass { int cls; double flops; LaunchClass(int c, double f = 0.0) : cls(c), flops(f) {} };
template <class... Params, class... Args>
int launch_k(sdrm_engine* e, LaunchClass lc, const char* name, void (*kernel)(Params...), dim3 grid, dim3 block, size_t lds, hipStream_t st,
             const Args&... args) {
  const auto go = [&] { SDRM_LAUNCH(e, kernel, grid, block, lds, st, args...); return hipGetLastError(); };
  return hip_rc(e, name, lc.cls == PC_NONE ? go() : profiled(e, lc.cls, lc.flops, st, go));
}

// Runtime value -> template argument: f is a generic callable that takes the value as a std::integral_constant (VAL reads it back
// as a constant expression).  with_int_in tries LO + I for every I of the sequence; a value outside calls nothing and returns false.
#define VAL(c) (decltype(c)::value)
template <int LO, int... I, class F>
bool with_int_in(int v, std::integer_sequence<int, I...>, int& rc, F&& f) {
  return ((v == LO + I && ((rc = f(std::integral_constant<int, LO + I>{})), true)) || ...);
}
template <class F>
int with_bool(bool b, F&& f) { return b ? f(std::true_type{}) : f(std::false_type{}); }

// The column tiles CT = WP / 32 of the row-owned kernels and the strip widths of k_wgrad_strips: 4 .. 11, the widths the
// fragment-packed weight copies exist for (sdrm_create).  tests/test_isa_lint.py holds the instantiations made here to its lists.
constexpr int CT_MIN = 4, CT_MAX = 11;
template <class F>
int with_col_tiles(sdrm_engine* e, F&& f) {
  int rc = SDRM_OK;
  if (with_int_in<CT_MIN>(e->WP / 32, std::make_integer_sequence<int, CT_MAX - CT_MIN + 1>{}, rc, f)) return rc;
  return fail(e, SDRM_ERR_SHAPE, "row-owned kernels: padded width outside 128..352");
}

#ifdef SDRM_STAMPS
unsigned long long* g_wgrad_stamps = nullptr;   // diagnostic build: 8 stamp slots per work-group of the batched wgrad launch
int g_wgrad_stamps_cap = 0, g_wgrad_stamps_n = 0;
int g_stamp_class = -1;                         // -1: the batched wgrad launch; else the NT launches of this profile class
#endif


// Tile shapes (tools/gemm_tune.py, profiles/r01_gemm_tile_sweep_c.txt).  K is only ~350 deep, so a work-group is ~22
// K-steps long and what hides its prologue, epilogue and per-K-step barrier is many co-resident work-groups, not a
// big tile: 64x64x16 (20 KB of LDS, <= 80 VGPRs -> six per CU) for the large launches, 32x32x32 on the 16-wide MFMA
// for NT launches of up to 4096 rows (choose_cfg), the others are tuning alternates (SDRM_TILE).
typedef TileCfg<64, 64, 2, 2, 4, 16> Cfg0;     //  64x 64x16  (default)
typedef TileCfg<64, 64, 2, 2, 4, 32, 32, 1> Cfg1;  //  64x 64x32, one prefetch set
typedef TileCfg<64, 128, 2, 2, 4, 16> Cfg2;    //  64x128x16
typedef TileCfg<128, 128, 2, 2, 4, 16> Cfg3;   // 128x128x16
typedef TileCfg<32, 32, 2, 2, 4, 32, 16> Cfg4; //  32x 32x32 on v_mfma_f32_16x16x4_f32 (NT launches of <= 4096 rows)
constexpr int N_TILE_CFGS = 5;   // (a 192x64x16 tile - exactly one round of three fat work-groups per CU at 24576 x 352 - measured 3 % slower:
                                 //  profiles/r02_gemm_stagger_and_waveflip.txt)
const int kCfgBM[N_TILE_CFGS] = {64, 64, 64, 128, 32};
const int kCfgBN[N_TILE_CFGS] = {64, 64, 128, 128, 32};
constexpr int FUSE_REV_MAX_ROWS = 4096;   // = the launches that run on the 32x32 tile (4 accumulator rows per lane: two Philox calls);
                                          // measured (tools/shard_probe.py): 679 / 1358 / 2715 rows 21.1 / 24.9 / 36.6 -> 18.8 / 22.6 / 33.7 us per step;
                                          // on the 64x64 tile (16 rows per lane) 5429 rows 54.3 -> 56.9

// Tile of a split-K (weight-gradient) launch: the forced one, else the default.
int pick_cfg(const Tuning& t) { return (t.force_cfg >= 0 && t.force_cfg < N_TILE_CFGS) ? t.force_cfg : 0; }

// Tile for an unsplit (NT) launch of M rows; `nt32_rows` is the caller's threshold (Tuning::nt32_max_rows for sampling
// and plain forwards, ::nt32_max_rows_train for the train step).  With the k-minor LDS image and ds_read_b128
// fragments the 32x32x32 tile on the 16-wide MFMA has no ragged tile (352 = 11 x 32), four times the work-groups and a
// quarter of the dependent MFMA chain per wave.  Stand-alone (tools/gemm_tune.py, operands hot in L2) it matches or
// beats 64x64x16 at every size; inside the step, where every operand was just written by the previous launch, it wins
// up to a few thousand rows and loses above (tools/shard_probe.py, sample step at 679 / 1358 / 2715 / 5429 rows:
// 19.3 / 25.6 / 36.9 / 60.1 us against 23.5 / 31.6 / 49.9 / 54.2; train step at 3072 / 6144 / 12288 / 24576 stacked
// rows: 156 / 235 / 375 / 683 against 170 / 235 / 363 / 629) - the 64x64 tile moves half the operand bytes per flop.
// (64x32 and 32x64 tiles on the 16-wide MFMA were tried for the large launches: 644 / 661 us per train step against 618; round 5 tried
// 64x32x32, 32x64x32 and 64x64x32 on the 16-wide MFMA again where the 32x32 tile runs today - ML-100k's NT launches 350.5 / 345.6 / 378.5 us
// per train step against 348.0, the sampler's two chains at 5429 rows 46.3 / 45.7 / 58.9 us per step against 44.0, one chain at 679
// rows 22.1 / 21.0 / 32.7 against 16.7: profiles/r05_nt_tiles.txt.  The operand bytes per flop are not what bounds these launches.)
int choose_cfg(const Tuning& t, int M, int nt32_rows) {
  if (t.force_cfg >= 0 && t.force_cfg < N_TILE_CFGS) return t.force_cfg;
  return M <= nt32_rows ? 4 : 0;
}

int max_gemm_blocks(int M, int N) {
  int best = 0;
  for (int c = 0; c < N_TILE_CFGS; ++c) {
    const int b = ((M + kCfgBM[c] - 1) / kCfgBM[c]) * ((N + kCfgBN[c] - 1) / kCfgBN[c]);
    if (b > best) best = b;
  }
  return best;
}

// The tile loads address one tile x one K chunk with 32-bit offsets behind a 64-bit base (gemm.h: tile_resource): whether the spans of a
// launch on a bm x bn tile stay below 2^32 bytes.  launch_gemm_cfg's test; the sdrm_debug_*_args envelopes ask it for every tile.
bool gemm_span_ok(int bm, int bn, bool a_kcontig, bool b_kcontig, int lda, int ldb, int kchunk) {
  const uint64_t kc = (uint64_t)std::max(kchunk, 1) + 64;
  const uint64_t spanA = a_kcontig ? ((uint64_t)bm * lda + kc) : kc * lda;
  const uint64_t spanB = b_kcontig ? ((uint64_t)bn * ldb + kc) : kc * ldb;
  return spanA * 4 < (1ull << 32) && spanB * 4 < (1ull << 32);
}
bool gemm_span_ok(int cfg, bool kcontig, int lda, int ldb, int kchunk) {
  return gemm_span_ok(kCfgBM[cfg], kCfgBN[cfg], kcontig, kcontig, lda, ldb, kchunk);
}

template <class Cfg, int LA, int LB, int XA, int XB, int EPI>
hipError_t launch_gemm_cfg(GemmArgs& a, int M, int N, int splits, hipStream_t st, Prof pr) {
  const int tiles_m = (M + Cfg::BM - 1) / Cfg::BM, tiles_n = (N + Cfg::BN - 1) / Cfg::BN;
  if (!gemm_set_grid(a, tiles_m, tiles_n, splits)) return hipErrorInvalidValue;   // beyond the exact range of the magic divisions
  if (!gemm_span_ok(Cfg::BM, Cfg::BN, LA == LD_KCONTIG, LB == LD_KCONTIG, a.lda, a.ldb, a.kchunk)) return hipErrorInvalidValue;
  dim3 grid(EPI == EPI_SLAB ? (unsigned)(a.nblocks * splits) : (unsigned)a.nblocks, 1, 1);
  return profiled(pr.e, pr.cls, pr.flops, st, [&] {
#ifdef SDRM_STAMPS
    if (g_wgrad_stamps && g_stamp_class >= 0 && pr.e && pr.cls == g_stamp_class && (int)grid.x <= g_wgrad_stamps_cap) {
      a.stamps = g_wgrad_stamps;
      g_wgrad_stamps_n = (int)grid.x;
    }
#endif
    SDRM_LAUNCH(pr.e, (gemm_kernel<Cfg, LA, LB, XA, XB, EPI>), grid, dim3(NTHREADS), 0, st, a);
    return hipGetLastError();
  });
}

template <int LA, int LB, int XA, int XB, int EPI>
hipError_t launch_gemm(GemmArgs& a, int M, int N, int splits, hipStream_t st, Prof pr, int cfg) {
  switch (cfg) {
    case 1: return launch_gemm_cfg<Cfg1, LA, LB, XA, XB, EPI>(a, M, N, splits, st, pr);
    case 2: return launch_gemm_cfg<Cfg2, LA, LB, XA, XB, EPI>(a, M, N, splits, st, pr);
    case 3: return launch_gemm_cfg<Cfg3, LA, LB, XA, XB, EPI>(a, M, N, splits, st, pr);
    case 4: return launch_gemm_cfg<Cfg4, LA, LB, XA, XB, EPI>(a, M, N, splits, st, pr);
    default: return launch_gemm_cfg<Cfg0, LA, LB, XA, XB, EPI>(a, M, N, splits, st, pr);
  }
}

// forward Linear: C[M,N] = act(xf(A)[M,K] * Wc[N,K]^T + bias)
template <int XA, int EPI>
hipError_t gemm_forward(GemmArgs a, const float* A, int lda, const float* Wc, int ldw, int M, int N, int K,
                        hipStream_t st, Prof pr, int cfg) {
  a.A = A; a.lda = lda; a.limA = M;
  a.B = Wc; a.ldb = ldw; a.limB = N;
  a.K = K; a.kchunk = K;
  return launch_gemm<LD_KCONTIG, LD_KCONTIG, XA, XF_NONE, EPI>(a, M, N, 1, st, pr, cfg);
}

// dgrad: C[M,Kin] = (dC[M,Nout] * W[Nout,Kin]) * prelu'(aux), against the transposed copy WT[Kin][Nout] (NT form)
hipError_t gemm_dgrad(sdrm_engine* e, const float* dC, int lddc, const float* WT, int ldwt, int M, int Nout, int Kin,
                      float* out, const float* aux, const float* slopeE, float* partial, hipStream_t st, double flops,
                      int cfg) {
  GemmArgs a{};
  a.A = dC; a.lda = lddc; a.limA = M;
  a.B = WT; a.ldb = ldwt; a.limB = Kin;
  a.C = out; a.ldc = e->WP;
  a.K = Nout; a.kchunk = Nout;
  a.aux = aux; a.ldaux = e->WP; a.slopeE = slopeE; a.slope_partial = partial;
  return launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI_DPRELU>(a, M, Kin, 1, st, Prof{e, PC_DGRAD, flops}, cfg);
}

// wgrad: slab[s][Nout,Kin] = dC[rows s][.,Nout]^T * xf(Act)[rows s][., Kin] ; dbias[s][Nout] = column sums of dC
template <int XB>
hipError_t gemm_wgrad(const float* dC, int lddc, int Nout, const float* Act, int ldact, int Kin, const float* slopeB,
                      int Mrows, int S, int kchunk, float* slab, float* dbias, hipStream_t st, Prof pr, int cfg) {
  GemmArgs a{};
  a.A = dC; a.lda = lddc; a.limA = Nout;
  a.B = Act; a.ldb = ldact; a.limB = Kin;
  a.C = slab; a.ldc = Kin;
  a.K = Mrows; a.kchunk = kchunk;
  a.slopeB = slopeB;
  a.slab_stride = (size_t)Nout * Kin;
  a.dbias = dbias; a.dbias_stride = Nout;
  return launch_gemm<LD_MCONTIG, LD_MCONTIG, XF_NONE, XB, EPI_SLAB>(a, Nout, Kin, S, st, pr, cfg);
}

// gemm_set_grid keeps a launch's tile count inside the exact range of its magic divisions (nb < 2^31, nb x tiles_n < 2^32,
// nb^2 x slices < 2^32).  A product of the VAE entry points' envelope can leave that range - 2^22 rows, or 2^20 output columns - so these
// two give the most rows (NT launch, N columns) / output columns (split-K launch, Kin columns, S slices) of ONE launch on tile `cfg`, whole
// tiles, and the helpers below send a larger product out in bands of that size.  0: not even one tile row fits.
int gemm_nt_band_rows(int cfg, int N) {
  const uint64_t tn = (uint64_t)((N + kCfgBN[cfg] - 1) / kCfgBN[cfg]);
  const uint64_t t = std::min<uint64_t>(65535 / tn, ((1ull << 32) - 1) / (tn * tn));
  return (int)t * kCfgBM[cfg];
}
int gemm_wgrad_band_cols(int cfg, int Kin, int S) {
  const uint64_t tn = (uint64_t)((Kin + kCfgBN[cfg] - 1) / kCfgBN[cfg]);
  uint64_t nb = (uint64_t)std::sqrt((double)((1ull << 32) - 1) / (double)S);   // the most tiles with nb^2 x S < 2^32
  while (nb * nb * (uint64_t)S >= (1ull << 32)) --nb;
  while ((nb + 1) * (nb + 1) * (uint64_t)S < (1ull << 32)) ++nb;
  return (int)std::min<uint64_t>(nb / tn, 1u << 20) * kCfgBM[cfg];
}

// C[M, N] = epilogue(A[M, K] B[N, K]^T) in row bands; `a` carries B, C, K and the epilogue's operands, rows_valid counts from row 0
template <int EPI>
int gemm_nt_banded(sdrm_engine* e, const GemmArgs& a, const float* A, int lda, int M, int N, int rows_valid, hipStream_t st, Prof pr, int cfg) {
  const int band = gemm_nt_band_rows(cfg, N);
  if (band < 1) return fail(e, SDRM_ERR_SHAPE, "decoder head: no tile row of this product fits one launch");
  for (int m0 = 0; m0 < M; m0 += band) {
    GemmArgs x = a;
    const int m = std::min(band, M - m0);
    x.A = A + (size_t)m0 * lda; x.lda = lda; x.limA = m; x.limB = N;
    x.C = a.C + (size_t)m0 * a.ldc;
    if (a.aux) x.aux = a.aux + (size_t)m0 * a.ldaux;
    x.kchunk = a.K;
    x.rows_valid = std::max(0, std::min(rows_valid - m0, m));
    HIP_TRY(e, (launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI>(x, m, N, 1, st, pr, cfg)));
  }
  return SDRM_OK;
}

// gemm_wgrad in bands of output columns: slab [S][Nout][Kin] and dbias [S][Nout] keep their whole strides
int gemm_wgrad_banded(sdrm_engine* e, const float* dC, int Nout, const float* Act, int Kin, int Mrows, int S, int kchunk, float* slab,
                      float* dbias, hipStream_t st, Prof pr, int cfg) {
  const int band = gemm_wgrad_band_cols(cfg, Kin, S);
  if (band < 1) return fail(e, SDRM_ERR_SHAPE, "decoder head: no tile row of this weight gradient fits one launch");
  for (int n0 = 0; n0 < Nout; n0 += band) {
    GemmArgs a{};
    a.A = dC + n0; a.lda = Nout; a.limA = std::min(band, Nout - n0);
    a.B = Act; a.ldb = Kin; a.limB = Kin;
    a.C = slab + (size_t)n0 * Kin; a.ldc = Kin;
    a.K = Mrows; a.kchunk = kchunk;
    a.slab_stride = (size_t)Nout * Kin;
    a.dbias = dbias + n0; a.dbias_stride = Nout;
    HIP_TRY(e, (launch_gemm<LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_SLAB>(a, a.limA, Kin, S, st, pr, cfg)));
  }
  return SDRM_OK;
}

// work-groups of 256 threads for `items` work items: at least 1, at most 2048 (the kernels stride)
unsigned blocks_for(int64_t items) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(2048, (items + 255) / 256)); }

// One weight gradient of a batched launch (gemm_batch_kernel): the arguments gemm_wgrad would pass, with the grid
// bookkeeping launch_gemm_cfg does, for the default tile.  slopeB must be non-null: layer 0, whose operand is not a
// stored pre-activation, passes a slope of exactly 1 (v > 0 ? v : 1*v is v bit for bit).
struct WgradSpec {
  const float* dC; int lddc, Nout; const float* Act; int ldact, Kin; const float* slopeB; int S, kchunk; float* slab; float* dbias;
};

hipError_t launch_wgrad_batch(sdrm_engine* e, const WgradSpec* w, int n, int Mrows, hipStream_t st, Prof pr, bool plain_b = false) {
  GemmBatch b{};
  b.n = n;
  int grid = 0;
  for (int k = 0; k < n; ++k) {
    GemmArgs& a = b.p[k];
    a.A = w[k].dC; a.lda = w[k].lddc; a.limA = w[k].Nout;
    a.B = w[k].Act; a.ldb = w[k].ldact; a.limB = w[k].Kin;
    a.C = w[k].slab; a.ldc = w[k].Kin;
    a.K = Mrows; a.kchunk = w[k].kchunk;
    a.slopeB = w[k].slopeB;
    a.slab_stride = (size_t)w[k].Nout * w[k].Kin;
    a.dbias = w[k].dbias; a.dbias_stride = w[k].Nout;
    const int tiles_m = (w[k].Nout + Cfg0::BM - 1) / Cfg0::BM, tiles_n = (w[k].Kin + Cfg0::BN - 1) / Cfg0::BN;
    if (!gemm_set_grid(a, tiles_m, tiles_n, w[k].S)) return hipErrorInvalidValue;
    // 32-bit offsets inside one K chunk (gemm.h: tile_resource): both operands are M-contiguous here
    if (((uint64_t)std::max(a.kchunk, 1) + 64) * (uint64_t)std::max(a.lda, a.ldb) * 4 >= (1ull << 32)) return hipErrorInvalidValue;
    b.start[k] = grid;
#ifdef SDRM_STAMPS
    a.stamps = (g_wgrad_stamps && g_stamp_class < 0) ? g_wgrad_stamps + 8 * (size_t)grid : nullptr;
#endif
    grid += round_up(a.nblocks * w[k].S, 8);   // a multiple of 8: the XCD of a work-group is the same inside its problem
  }
  b.start[n] = grid;
#ifdef SDRM_STAMPS
  if (grid > g_wgrad_stamps_cap) for (int k = 0; k < n; ++k) b.p[k].stamps = nullptr;
  else if (g_stamp_class < 0) g_wgrad_stamps_n = grid;
#endif
  return profiled(e, pr.cls, pr.flops, st, [&] {
    // plain_b: every B operand is stored as the kernel needs it (activations written by the row-owned forward): no PReLU on load
    if (plain_b)
      SDRM_LAUNCH(e, (gemm_batch_kernel<Cfg0, LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_SLAB>), dim3((unsigned)grid),
                         dim3(NTHREADS), 0, st, b);
    else
      SDRM_LAUNCH(e, (gemm_batch_kernel<Cfg0, LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_PRELU, EPI_SLAB>), dim3((unsigned)grid),
                         dim3(NTHREADS), 0, st, b);
    return hipGetLastError();
  });
}

// Split-K plan of a backward's weight gradients: ONE slice count for all of them (so the one-call and the two-call backward
// add the same partial sums in the same order), chosen so that the batched launch is ONE round of what the device holds at
// once (5 work-groups per CU, 1280 on MI355X) when that cuts the reduction eight ways or more with slices of at most 1024
// rows, and 2.2 rounds (2816 work-groups) otherwise.  Measured on one box, train step in us
// (profiles/r02_wgrad_slices_any_count.txt): ML-1M, 114 tiles, 24576 rows: 11 slices (one round) 572, 22 / 24 slices 573 /
// 573, 10 / 12 / 13 slices (just under / over a round) 586-588 - equal times, but the 2240-row slices of the one-round
// plan do not fit an XCD's L2 and double the launch's HBM traffic, so this size takes 24; the same net at the row counts
// of a 4- / 8-GPU shard: 11 slices 204.0 / 139.7, 24 slices 207.8 / 144.3 (a slice of 128 rows is mostly prologue and
// epilogue); ML-100k, 702 tiles: 4 slices 356, 3: 359, 1-2: 361, 8 (round 1's multiple of 8): 369.
// The (slice, tile) units are dealt to the XCDs in contiguous runs (gemm.h), so any slice count fills the chip evenly.
void pick_splits(const Tuning& tn, int Mrows, int tiles_total, int& S, int& kchunk) {
  const int BK = 32;
  int max_by_rows = Mrows / (4 * BK);  // at least 4 K-steps of 32 rows per work-group
  if (max_by_rows < 1) max_by_rows = 1;
  const int tiles = tiles_total < 1 ? 1 : tiles_total;
  // one round when that cuts the reduction eight ways or more AND a slice stays within 1024 rows - the tiles of a slice share
  // its operand strips through one XCD's 4 MB L2: at 24576 rows 11 slices of 2240 rows take the same 204 us as 24 slices of
  // 1024 but move 653 MB instead of 334 MB (PMC) - else 2.2 rounds (floor: one block more is a round more)
  S = tn.wgrad_round / tiles;
  if (S < 8 || round_up((Mrows + S - 1) / S, BK) > 1024) S = tn.wgrad_blocks / tiles;
  if (S < 1) S = 1;
  if (tn.wgrad_slices > 0) S = tn.wgrad_slices;
  if (S > S_MAX) S = S_MAX;
  if (S > max_by_rows) S = max_by_rows;
  kchunk = round_up((Mrows + S - 1) / S, BK);
  S = (Mrows + kchunk - 1) / kchunk;
}

int wgrad_tiles(const Tuning& tn, int Nout, int Kin) {
  const int c = pick_cfg(tn);
  return ((Nout + kCfgBM[c] - 1) / kCfgBM[c]) * ((Kin + kCfgBN[c] - 1) / kCfgBN[c]);
}

// the parameter tensors and their compute copies, as k_adam (sdrm_adam_step, sdrm_set_params) walks them
void build_jobs(sdrm_engine* e, JobTable& tab) {
  const int L = e->L, W = e->W, T = e->T, H = e->H;
  int n = 0;
  auto add = [&](int64_t off, int rows, int cols, int flat_ld, int ncols, float* dst, int dst_ld, float* dstT = nullptr, int dstT_ld = 0) -> Job& {
    Job& j = tab.j[n++];
    j.flat_off = off; j.rows = rows; j.cols = cols; j.flat_ld = flat_ld; j.ncols = ncols;
    j.dst = dst; j.dst_ld = dst_ld; j.dstT = dstT; j.dstT_ld = dstT_ld; j.dst2 = nullptr; j.dst2_ld = 0;
    j.dstF = nullptr; j.dstFT = nullptr; j.fnct = e->WP / 16; j.fklast = -1; j.fklastT = -1;
    return j;
  };
  add(e->off_we, T, T, T, e->WeP ? T : 0, e->WeP, e->TPe);   // emb_layer.weight (a padded copy for the narrow nets' forward only)
  add(e->off_be, 1, T, T, 0, nullptr, 0);                    // emb_layer.bias
  {
    Job& j = add(e->off_w0, W, L + T, L + T, L, e->W0c, e->K0);
    j.dstF = e->W0f; j.fklast = rc_light_klast(L, e->LP);
    j.dst2 = e->W0eP; j.dst2_ld = e->TPe;
  }
  add(e->off_b0, 1, W, W, W, e->b0c, 0);
  add(e->off_a0, 1, 1, 1, 1, nullptr, 0);
  if (H >= 1) {
    Job& j = add(e->off_wh, W, W, W, W, e->Whc, e->WP, e->WhcT, e->WP);
    j.dstF = e->Whf; j.dstFT = e->WhfT; j.fklast = j.fklastT = rc_light_klast(W, e->WP);
    add(e->off_bh, 1, W, W, W, e->bhc, 0);
    add(e->off_ah, 1, 1, 1, 1, nullptr, 0);
  }
  {
    Job& j = add(e->off_wo, L, W, W, W, e->Woc, e->WP, e->WocT, e->LP);
    j.dstF = e->Wof; j.dstFT = e->WofT; j.fklast = rc_light_klast(W, e->WP); j.fklastT = rc_light_klast(L, e->LP);
  }
  add(e->off_bo, 1, L, L, L, e->boc, 0);
  tab.n = n;
}

// Adam's bias corrections of step `step` >= 1 for the given betas (the eps-net's: e->adam_t, 0.9, 0.999 - train_SDRM.py:337; torch.optim.Adam: step_size = lr / (1 - b1^k), denominators
// scaled by sqrt(1 - b2^k))
void adam_scalars(int64_t step, float lr, double beta1, double beta2, float& step_size, float& bc2_sqrt) {
  const double k = (double)step;
  const double bc1 = 1.0 - std::pow(beta1, k), bc2 = 1.0 - std::pow(beta2, k);
  step_size = (float)((double)lr / bc1);
  bc2_sqrt = (float)std::sqrt(bc2);
}

int launch_adam(sdrm_engine* e, const float* grad, float lr, int update, hipStream_t st) {
  JobTable tab;
  build_jobs(e, tab);
  AdamArgs a{};
  a.p = e->p; a.m = e->m; a.v = e->v; a.g = grad ? grad : e->g;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f; a.wd = 1e-4f; a.update = update;
  if (update) adam_scalars(e->adam_t, lr, 0.9, 0.999, a.step_size, a.bc2_sqrt);
  // enough work-groups that the largest tensor is one or two passes per thread (a pass is a chain of dependent loads)
  int64_t biggest = 0;
  for (int k = 0; k < tab.n; ++k) biggest = std::max<int64_t>(biggest, (int64_t)tab.j[k].rows * tab.j[k].cols);
  const int gx = (int)std::min<int64_t>(1024, std::max<int64_t>(1, (biggest + 511) / 512));
  dim3 grid(gx, tab.n);
  SDRM_LAUNCH(e, k_adam, grid, dim3(256), 0, st, tab, a);
  HIP_TRY(e, hipGetLastError());
  e->tables_fresh = false;
  e->fwd_params_live = false;
  return SDRM_OK;
}

// Strip-owned weight gradients (csrc/wgrad2.h): every weight gradient of the step in one balanced round of one work-group per CU.
// Taken by the one-call backward when the forward was a row-owned one (StepPlan::strips_ok: the operands are stored as the kernel
// reads them - activations, a ones column for the bias gradients) and the slices stay within the slab count.
int launch_wgrad_strips(sdrm_engine* e, double flops, hipStream_t st) {
  const int H = e->H;
  Wg2Args a{};
  int ktiles[WG2_MAX_PROBLEMS], n = 0;
  auto problem = [&](const float* A, int lda, const float* B, int ldb, float* slab, int kin, size_t slab_rows) {
    a.p[n].A = A; a.p[n].lda = lda; a.p[n].B = B; a.p[n].ldb = ldb; a.p[n].slab = slab; a.p[n].ldc = kin;
    a.p[n].slab_stride = slab_rows * (size_t)kin;
    ktiles[n++] = kin / 32;
  };
  auto actk = [&](int k) { return e->act + (size_t)k * e->MPmax * e->WP; };
  problem(dpre_buf(e, 0), e->WP, e->U, e->K0, e->slab0, e->K0, (size_t)e->WP);
  problem(e->dY, e->LP, actk(H), e->WP, e->slabO, e->WP, (size_t)e->LP);
  const int units = [&] { int t = e->K0 / 32 + (H + 1) * (e->WP / 32); return (t + 3) / 4; }();
  int S = 256 / units;
  if (S < 1) S = 1;
  if (S > S_MAX) S = S_MAX;
  const int MP = e->plan.rows;   // the rows the forward wrote (whole groups, a multiple of 16): the padding behind them is not summed over
  const int kchunk = round_up((MP + S - 1) / S, WG2_BK);
  const int slices = (MP + kchunk - 1) / kchunk;
  for (int k = H; k >= 1; --k)   // the shared hidden layer: one problem per application, slabs [application][slice]
    problem(dpre_buf(e, k), e->WP, actk(k - 1), e->WP, e->slabH + (size_t)(k - 1) * slices * e->WP * e->WP, e->WP, (size_t)e->WP);
  if (wg2_plan(ktiles, n, a) != units) return fail(e, SDRM_ERR_SHAPE, "strip-owned weight gradients: plan does not fit");
  a.slices = slices; a.rows = MP; a.kchunk = kchunk;
  e->bwd_S0 = e->bwd_SH = e->bwd_SO = slices;
  e->bwd_strips = true;
  return with_col_tiles(e, [&](auto nt) {
    return hip_rc(e, "k_wgrad_strips", profiled(e, PC_WGRAD_STRIPS, flops, st, [&] {
      SDRM_LAUNCH(e, (k_wgrad_strips<VAL(nt)>), dim3((unsigned)(a.units * a.slices)), dim3(NTHREADS), 0, st, a);
      return hipGetLastError();
    }));
  });
}

EmbTabArgs emb_args(sdrm_engine* e) {
  EmbTabArgs a{};
  a.temb = e->temb; a.We = e->p + e->off_we; a.be = e->p + e->off_be; a.W0 = e->p + e->off_w0; a.b0 = e->p + e->off_b0;
  a.W0c = e->W0c; a.B0tab = e->B0tab;
  a.L = e->L; a.W = e->W; a.T = e->T; a.LP = e->LP; a.WP = e->WP; a.K0 = e->K0;
  a.ones_col = e->ones_col;
  return a;
}

// The time-embedding tables of the current parameters: B0tab[t] = b0 + C0[t] (what layer 0 of a train step or of a sampling step
// adds per row) and C0^T in the trailing columns of W0c (what the plain forward multiplies its one-hot(t) columns with).
int emb_tables(sdrm_engine* e, hipStream_t st, const float* warm = nullptr, size_t warm_floats = 0) {
  EmbTabArgs a = emb_args(e);
  a.warm = warm; a.warm_lines = warm ? (unsigned)std::min<size_t>(warm_floats / 32, 1u << 24) : 0u;
  SDRM_LAUNCH(e, k_emb_tables, dim3(e->T + 1), dim3(1024), 2 * e->T * sizeof(float), st, a);
  HIP_TRY(e, hipGetLastError());
  e->tables_fresh = true;
  return SDRM_OK;
}
// ... made only when the parameters changed since they were last made (sdrm_set_params, sdrm_adam_step, every train step: the tail
// updates the parameters and clears `tables_fresh`; the tables are then made by the next consumer - k_emb_tables in front of the
// row-owned forward, the leading blocks of k_prep_train, the narrow nets' forward itself when T <= 128, or this launch: narrow
// nets with T > 128 and the sampler pay it as a launch of its own)
// (Round 5 also made the next row-owned step's tables AHEAD - on aux[2], behind the tail of the last train step, beside the first sampling
// step that follows it in bench.py's walk: 8967 -> 8907 steps/s in the driver's form, 9069 -> 8994 with the default windows; the fork, the
// join and a forward that finds its batch cold cost more than the 10 us launch saved.  profiles/r05_walk_transitions.txt)
int ensure_tables(sdrm_engine* e, hipStream_t st) { return e->tables_fresh ? SDRM_OK : emb_tables(e, st); }

bool skinny_net(const sdrm_engine* e) { return e->tune.skinny && e->LP <= 64 && e->WP <= 64; }
// The forms <NL, NW> of the narrow nets' kernels (csrc/skinny.h, skinny_step.h, skinny_fwd4.h): the 16-column tiles with real columns
// of the latent and of the hidden width, 1..4 each (more: the form of 4)
template <class F>
int with_skinny_form(sdrm_engine* e, F&& f) {
  const auto tiles = std::make_integer_sequence<int, 4>{};
  int rc = SDRM_OK;
  with_int_in<1>(std::min((e->L + 15) / 16, 4), tiles, rc, [&](auto nl) {
    return with_int_in<1>(std::min((e->W + 15) / 16, 4), tiles, rc, [&](auto nw) { return f(nl, nw); }), rc;
  });
  return rc;
}

// Row-owned train forward (rowchain.h): one 96-row work-group per CU.  It replaces staging + H + 2 GEMM launches + the loss
// partial sums when the batch fills whole rounds of the chip's 256 CUs (measured at B = 8192, L = 340: 169 us against
// 182 + 18.7 + 11.7 us); a last round that leaves more than a sixth of the CUs idle loses to the per-layer path.
// row-owned dgrads (dgrad_rows.h): the stacked rows are whole 96-row work-groups (the grouped order of the row-owned forward),
// reduction axis == output axis == the padded width (LP == WP: L == W).  Whether they follow a forward is decided with the
// forward, in plan_step (StepPlan::dgrad): they read activations, so that forward need not store pre-activations (rowchain.h: skip_pre).

// The forms <CT, LIGHT> of the row-owned kernels: CT column tiles, LIGHT the weight copies' compact last K-step (elementwise.h;
// L == W on these paths: one answer for every layer).
template <class F>
int with_row_form(sdrm_engine* e, F&& f) {
  return with_col_tiles(e, [&](auto ct) { return with_bool(rc_light_klast(e->W, e->WP) >= 0, [&](auto light) { return f(ct, light); }); });
}

// out[MP][WP] = (G[MP][WP] * W) * prelu'(pre), W given as the fragment-packed [k = out][n = in] copy
DgradRowsArgs dgrad_rows_args(const sdrm_engine* e, const float* G, const float* WfT, const float* pre, const float* slope, float* out,
                              float* partial) {
  DgradRowsArgs a{};
  a.G = G; a.ldg = e->WP; a.WfT = WfT; a.pre = pre; a.ldp = e->WP; a.slope = slope; a.out = out; a.ldo = e->WP; a.slope_part = partial;
  // the layer's activations sit at the same place of the `act` buffer as its pre-activations in `pre`
  a.act = e->act ? e->act + (pre - e->pre) : nullptr; a.from_act = (e->plan.skip_pre() && a.act) ? 1 : 0;
  return a;
}

int launch_dgrad_rows(sdrm_engine* e, const float* G, const float* WfT, const float* pre, const float* slope, float* out, float* partial,
                      int groups, double flops, hipStream_t st) {
  const DgradRowsArgs a = dgrad_rows_args(e, G, WfT, pre, slope, out, partial);
  return with_row_form(e, [&](auto ct, auto light) {
    return hip_rc(e, "k_dgrad_rows", profiled(e, PC_DGRAD_ROWS, flops, st, [&] {
      SDRM_LAUNCH(e, (k_dgrad_rows<VAL(ct), VAL(light)>), dim3((unsigned)groups), dim3(NTHREADS), 0, st, a);
      return hipGetLastError();
    }));
  });
}

// the layers of the row-owned chain, output layer first (the 96-row and the 48-row chain alike)
void dgrad_chain_args(sdrm_engine* e, const SeedArgs& seed, DgradChainArgs& ca) {
  const int H = e->H;
  ca.seed = seed; ca.nlayers = H + 1;
  ca.layer[0] = dgrad_rows_args(e, e->dY, e->WofT, pre_buf(e, H), slope_ptr(e, H), dpre_buf(e, H), e->alpha_part + (size_t)H * e->alpha_part_stride);
  for (int k = H; k >= 1; --k)
    ca.layer[H + 1 - k] = dgrad_rows_args(e, dpre_buf(e, k), e->WhfT, pre_buf(e, k - 1), slope_ptr(e, k - 1), dpre_buf(e, k - 1),
                                          e->alpha_part + (size_t)(k - 1) * e->alpha_part_stride);
}

// loss value + gradient seeds + every layer's dgrad in one launch (k_dgrad_chain)
int launch_dgrad_chain(sdrm_engine* e, const DgradChainArgs& a, int groups, double flops, hipStream_t st) {
  return with_row_form(e, [&](auto ct, auto light) {
    return hip_rc(e, "k_dgrad_chain", profiled(e, PC_DGRAD_ROWS, flops, st, [&] {
      SDRM_LAUNCH(e, (k_dgrad_chain<VAL(ct), VAL(light)>), dim3((unsigned)groups), dim3(NTHREADS), 0, st, a);
      return hipGetLastError();
    }));
  });
}

bool use_rowchain(const sdrm_engine* e, int B) {
  if (!e->W0f || e->tune.rowchain <= 0 || e->tune.force_cfg >= 0) return false;   // a forced tile means: the per-layer kernels
  if (e->tune.rowchain >= 2) return true;
  const int G = (B + RC_USERS - 1) / RC_USERS;
  const int rounds = (G + 255) / 256;
  // one round: from 154 groups (B = 4897) on the three row-owned launches beat the per-layer path's eleven although two fifths of
  // the CUs idle (round 5, tools/rows48_probe.py: B = 5120 383 against 397 us, B = 6144 406 against 462); several rounds: the
  // last one at least five sixths full
  return rounds == 1 ? G >= 154 : G * 6 >= rounds * 256 * 5;
}

// ---- the row chains of a sampling call ----------------------------------------------------------
// Rows are independent through the whole reverse loop, so a row range can run as a chain of launches on a stream of its own; the
// ramp and drain of one chain's launch are then filled by the other's.  Measured in round 5 (tools/ab/chain_ab.py,
// profiles/r05_sampler_chains.txt; us per reverse step of the ML-1M net, whole calls): two chains win from ~2700 rows on - 2715 rows
// 30.4 -> 27.3, 4096 rows 40.3 -> 36.1, 5429 rows 48.8 -> 44.4, 8192 rows 67.3 -> 59.5 - and lose below (1358 rows 20.1 -> 22.9: a
// launch of half the rows no longer fills the chip).  Three chains: 42.6 at 5429 rows, worse elsewhere, and worse inside a job that
// trains between sampling steps; more than two are not what the host's launch rate bounds (tools/ab/chain_threads.py: one host
// thread per chain gives the same 43.4; a captured graph with forked streams replays at 65).
// The rule: two chains once the call has 2560 x 352 elements per layer, i.e. each chain's launch still has ~130 work-groups.
int chains_for(const Tuning& t, int n, int WP) {
  if (t.chains >= 1) return t.chains > 4 ? 4 : t.chains;
  return (size_t)n * (size_t)WP >= (size_t)2560 * 352 ? 2 : 1;
}

// the abort word of the XCD-local launches lives in host-mapped memory the GPU writes: read it as volatile
inline unsigned xabort_read(const sdrm_engine* e) { return e->xabort_host ? *(volatile const unsigned*)e->xabort_host : 0u; }
// The call's path is PERSIST and the abort word - the one input of that path that stays live - is clear.
bool persist_now(const sdrm_engine* e) { return e->call.path == SampleCall::PERSIST && xabort_read(e) == 0u; }

// ChainSched, one function per event.  ON_CALLER -> FORKED at the first steps of a call of several chains, ON_CALLER -> DETACH_ARMED ->
// FORKED for the one chain of a small call, FORKED -> ON_CALLER at every join:
//  * Chain 0 of several runs on the caller's stream, the others on auxiliary streams; they are joined lazily (chains_join).
//  * A small call is one chain on the caller's stream - on a stream of its own a plain call is ~3 us per step SLOWER
//    (tools/ab/detach_ab.py: 679 rows 17.0 -> 19.7, ML-100k 58.1 -> 62.4) - until a train step is queued beside it: from then on the
//    chain is detached, it runs on aux[0] and the caller's stream carries the train steps.  A train step of the per-layer path - eleven
//    dependent launches of 5-13 us on a mostly idle chip - and the four launches of a small sampling step are both latency chains, and
//    two latency chains on two streams fill each other's gaps.
//  * A train step between two sampling steps (bench.py's walk) does not join the chains: the call reads its own snapshot of the net
//    and runs in buffers of its own - Us, X, smp_pre, smp_Y - so what the chains have queued may finish beside the start of the step.
//    Behind a per-layer step their next launches wait for nothing; behind a ROW-OWNED one for its last MFMA kernel, the weight
//    gradients (SDRM_HOLD_EARLY=0: for all that is queued when they are launched) - one cross-stream dependency per train step instead
//    of a join and a fork.  With none, a launch of one work-group per CU finds some CUs busy with the other stream's work-groups and ends
//    a whole work-group time later: 8850 -> 8565 steps/s.  What follows the weight gradients - the tail's two launches - is latency- and
//    HBM-bound on a fraction of the chip; the chains' next GEMMs run beside it (the tail writes the live parameters).
//  * While an event profile is recorded (sdrm_profile_begin) the chains run one after the other on the caller's stream: intervals of
//    launches that share the chip would overlap and say nothing about either kernel.
int chains_on_aux(const sdrm_engine* e) { return e->chain_sched.detached ? 1 : e->call.chains - 1; }

// Chains still running on the auxiliary streams are folded back into `st` before anything else touches the engine's buffers or parameters.
int chains_join(sdrm_engine* e, hipStream_t st) {
  e->bwd_begun = false;   // a backward that was begun but never finished is abandoned
  if (e->chain_sched.state != ChainSched::FORKED) return SDRM_OK;
  for (int c = 0; c < chains_on_aux(e); ++c) {
    HIP_TRY(e, hipEventRecord(e->ev_join[c], e->aux[c]));
    HIP_TRY(e, hipStreamWaitEvent(st, e->ev_join[c], 0));
  }
  e->chain_sched.state = ChainSched::ON_CALLER;
  return SDRM_OK;
}

// sdrm_sample_begin: the chains of the call before are joined (by that call's count), the new call starts on the caller's stream
int chains_begin(sdrm_engine* e, hipStream_t st) {
  if (int jr = chains_join(e, st)) return jr;
  e->chain_sched.state = ChainSched::ON_CALLER;
  e->chain_sched.detached = false;
  return SDRM_OK;
}

// A train forward is about to be queued on `st`, in front of its launches (no join: see above).  Beside a small call that is still on
// the caller's stream the detach is armed: the mark behind the call's last step is taken now.
int chains_train_forward(sdrm_engine* e, hipStream_t st) {
  ChainSched& s = e->chain_sched;
  const SampleCall& c = e->call;
  if (!s.train_queued) s.train_row_owned = false;   // (kept over several train steps in a row)
  s.train_queued = true; s.hold_marked = false;
  if (e->tune.detach > 0 && c.active && c.path != SampleCall::SKINNY && c.i_next >= 1 && c.chains == 1 && !s.detached &&
      s.state == ChainSched::ON_CALLER && !e->prof_on && !persist_now(e)) {
    HIP_TRY(e, hipEventRecord(e->ev_fork, st));
    s.state = ChainSched::DETACH_ARMED;
  }
  return SDRM_OK;
}
void chains_train_row_owned(sdrm_engine* e) { e->chain_sched.train_row_owned = true; }   // ... and it was a row-owned one, launched

// The weight gradients of that step - its last MFMA kernel - are queued on `st`: the point pending chains wait for
int chains_wgrads_queued(sdrm_engine* e, hipStream_t st) {
  if (e->chain_sched.state != ChainSched::FORKED || !e->tune.hold_early || !e->chain_sched.train_row_owned) return SDRM_OK;
  HIP_TRY(e, hipEventRecord(e->ev_hold, st));
  e->chain_sched.hold_marked = true;
  return SDRM_OK;
}

// Is a small call running beside this train step, on its detached chain or about to be (rows48_parts)?
bool chains_small_call_beside(const sdrm_engine* e) {
  return e->call.active && (e->chain_sched.state == ChainSched::DETACH_ARMED || (e->chain_sched.state == ChainSched::FORKED && e->chain_sched.detached));
}

// In front of the launches of one sdrm_sample_steps: on[c] = the stream of chain c
int chains_streams(sdrm_engine* e, hipStream_t st, hipStream_t (&on)[4]) {
  ChainSched& s = e->chain_sched;
  auto aux_wait = [&](hipEvent_t ev) -> int {
    for (int c = 0; c < chains_on_aux(e); ++c) HIP_TRY(e, hipStreamWaitEvent(e->aux[c], ev, 0));
    return SDRM_OK;
  };
  // pending chains behind a row-owned train step: its own mark if it left one, else everything queued on `st` so far
  auto hold = [&]() -> int {
    if (!s.train_queued || !s.train_row_owned) return SDRM_OK;
    if (s.hold_marked) { s.hold_marked = false; return aux_wait(e->ev_hold); }
    HIP_TRY(e, hipEventRecord(e->ev_fork, st));
    return aux_wait(e->ev_fork);
  };
  if (e->prof_on) {
    if (s.state == ChainSched::DETACH_ARMED) s.state = ChainSched::ON_CALLER;
    if (int jr = chains_join(e, st)) return jr;
  } else if (s.state == ChainSched::DETACH_ARMED) {   // the first steps behind a train step that was queued beside this small call
    s.detached = true;
    if (int rc = aux_wait(e->ev_fork)) return rc;
    s.state = ChainSched::FORKED;
    if (int rc = hold()) return rc;
  } else if (s.state == ChainSched::FORKED) {
    if (int rc = hold()) return rc;
  } else if (chains_on_aux(e) > 0) {   // fork: the chains on auxiliary streams start after everything queued on `st` so far
    HIP_TRY(e, hipEventRecord(e->ev_fork, st));
    if (int rc = aux_wait(e->ev_fork)) return rc;
    s.state = ChainSched::FORKED;
  }
  s.train_queued = false;
  for (int c = 0; c < 4; ++c) on[c] = e->prof_on ? st : s.detached ? e->aux[0] : c == 0 ? st : e->aux[c - 1];
  return SDRM_OK;
}

// The same step on 48-row work-groups (csrc/rows48.h), for batches the 96-row kernels would leave CUs idle with.  Returns the
// work-groups per 16-user row group, 0: not this path.
//   1: the groups of the batch fill most of ONE round of the chip (160..256 groups: 2545..4096 users; two work-groups fit a CU, but
//      a second round's worth then shares the matrix pipes: no faster than the per-layer path);
//   2 / 4 (column-split groups, exchanged through one XCD's L2): batches of at most 2048 / 1024 users, whose groups x parts fit the
//      chip's 256 CUs - every work-group of such a launch must be resident at once; by size only 2, for 1281 .. 2048 users.
int rows48_grid(int groups, int parts) { return parts == 1 ? groups : 8 * parts * ((groups + 7) / 8); }
int rows48_parts(const sdrm_engine* e, int B) {
  if (!e->W0f || e->tune.rows48 <= 0 || e->tune.force_cfg >= 0 || e->tune.rowchain >= 2) return 0;
  const int G = (B + R48_USERS - 1) / R48_USERS;
  const bool can_split = e->xcd_ok && e->tune.split > 0 && e->xabort_host && xabort_read(e) == 0u;
  if (can_split && e->tune.split >= 2) {
    const int parts = e->tune.split >= 4 ? 4 : 2;
    if (rows48_grid(G, parts) <= 256) return parts;
    if (parts == 4 && rows48_grid(G, 2) <= 256) return 2;
  }
  if (e->tune.rows48 >= 2) return 1;
  // (measured, tools/rows48_probe.py, profiles/r05_rows48_probe.txt: two work-groups per group beat the per-layer path from ~1300
  // users on - B = 2048: 174 against 201 us, B = 1536: 164 against 170 - four per group do not: B = 1024: 140 against 131, the
  // redundant staging and the two hand-shakes per kernel cost what the five launches saved)
  // ... unless a small sampling call is in progress on its detached chain (ChainSched): beside it the eleven launches of the per-layer
  // path, which it may run along with, beat the column-split kernels, which hold it (tools/ab/walk_host.py, one rank of four - 2048 users,
  // 1358 sampled rows - in bench.py's walk: 25.2 k -> 27.1 k steps/s).  The two paths differ in the last bits of a step.
  if (can_split && e->tune.split == 1 && G > 80 && rows48_grid(G, 2) <= 256) return chains_small_call_beside(e) ? 0 : 2;   // 1281 .. 2048 users
  return (G >= 160 && G <= 256) ? 1 : 0;   // (2545 .. 4096 users; measured: 2560 users 231 against 235 us, 2688 231 / 241, 2432 228 / 224)
}

// The plan of a train step of B users: which kernels run it (the size rules above, asked here and nowhere else), what its forward
// leaves in the buffers, and what its backward does with that.
StepPlan plan_step(const sdrm_engine* e, int B) {
  StepPlan p;
  p.B = B;
  auto grouped = [&](StepPlan::Path path, int order, int users, int rows_per_group) {
    p.path = path; p.order = order; p.users_per_group = users;
    p.groups = (B + users - 1) / users;
    p.rows = p.groups * rows_per_group;
    p.loss_parts = p.groups;
  };
  if (skinny_net(e)) {
    grouped(StepPlan::SKINNY, 2, SK_USERS, SK_ROWS);
    p.dgrad = StepPlan::SKINNY_OWN;
  } else if (use_rowchain(e, B)) {
    grouped(StepPlan::ROW96, 1, RC_USERS, RC_ROWS);
  } else if (const int parts = rows48_parts(e, B)) {
    grouped(StepPlan::ROW48, 2, R48_USERS, R48_ROWS);
    p.parts = parts;
    p.loss_parts = p.groups * parts;
  } else {
    p.groups = B;
    p.rows = round_up(3 * B, BM);
    p.loss_parts = LOSS_BLOCKS;
  }
  p.MP = round_up(p.rows, BM);
  if (p.path == StepPlan::ROW96 || p.path == StepPlan::ROW48) {
    p.acts_stored = true;
    p.strips_ok = e->ones_col >= 0 && e->tune.strips > 0 && e->H + 2 <= WG2_MAX_PROBLEMS && e->WP >= 128 && e->WP <= 352;
    // the envelope of the row-owned dgrads: the transposed fragment-packed copies, one padded width for every axis; the chains keep
    // every layer's arguments in one struct; the 96-row kernels want the padded rows to be whole work-groups (the 48-row chain
    // clears the padding rows behind its last group itself, and has no launch-per-layer form: tune.dgrad_rows == 2 runs its chain too)
    const bool rows_ok = e->WhfT && e->tune.dgrad_rows > 0 && e->LP == e->WP && e->WP >= 128 && e->WP <= 352;
    const bool chain_fits = e->H + 1 <= DR_MAX_LAYERS;
    if (rows_ok && p.path == StepPlan::ROW48 && chain_fits) p.dgrad = StepPlan::CHAIN;
    if (rows_ok && p.path == StepPlan::ROW96 && p.MP % RC_ROWS == 0)
      p.dgrad = (e->tune.dgrad_rows == 1 && chain_fits) ? StepPlan::CHAIN : StepPlan::ROWS_PER_LAYER;
  }
  return p;
}

// the hand-shake counters of a column-split launch: they count on from launch to launch while the geometry stays the same
int split_sync(sdrm_engine* e, bool chain, int groups, int parts, int phases, hipStream_t st, unsigned** cnt, unsigned* base) {
  unsigned*& c = chain ? e->xcntC : e->xcntF;
  uint32_t& epoch = chain ? e->xepochC : e->xepochF;
  int& geo = chain ? e->xgeoC : e->xgeoF;
  const int now = (parts << 16) | groups | (phases << 24);
  if (geo != now || epoch >= 0x7fffffffu / (uint32_t)(phases * parts + 1)) {
    HIP_TRY(e, hipMemsetAsync(c, 0, (size_t)256 * 32 * sizeof(unsigned), st));
    epoch = 0; geo = now;
  }
  *cnt = c;
  *base = epoch * (uint32_t)(phases * parts) + e->xskew;
  if (e->xskew) { e->xskew = 0; geo = 0; }   // (the counters of a skewed launch are worthless: start over with the next one)
  ++epoch;
  return SDRM_OK;
}

// a timed-out hand-shake of an earlier column-split launch (csrc/rows48.h): reported by the next call, the path switched off
int split_status(sdrm_engine* e) {
  if (xabort_read(e) == 0u) return SDRM_OK;
  *(volatile unsigned*)e->xabort_host = 0u;   // reported once; the counters start over should the path ever be switched on again
  e->xgeoF = e->xgeoC = 0;
  e->tune.split = 0;
  e->fwd_done = false;
  return fail(e, SDRM_ERR_HIP, "a column-split row-group launch (csrc/rows48.h) timed out waiting for a work-group of its group: the results of "
                               "that train step are invalid; the path is switched off for this handle");
}

// The forms <CT, LIGHT, PARTS, SHARE> of the 48-row kernels (csrc/rows48.h): 1 / 2 / 4 work-groups per row group, and the shared-tile
// form - for one work-group per group and 2 CT = 4 q + 2 column tiles (odd CT) only, where `share` asks for it.  Not the full
// product: a form nobody launches is a kernel nobody lints (tests/test_isa_lint.py).
template <class F>
int with_rows48_form(sdrm_engine* e, int parts, bool share, F&& f) {
  return with_row_form(e, [&](auto ct, auto light) {
    if constexpr (VAL(ct) % 2 == 1)
      if (parts == 1 && share) return f(ct, light, std::integral_constant<int, 1>{}, std::true_type{});
    if (parts == 4) return f(ct, light, std::integral_constant<int, 4>{}, std::false_type{});
    if (parts == 2) return f(ct, light, std::integral_constant<int, 2>{}, std::false_type{});
    return f(ct, light, std::integral_constant<int, 1>{}, std::false_type{});
  });
}

int launch_rows48_chain(sdrm_engine* e, DgradChain48Args& a, int G, int parts, double flops, hipStream_t st) {
  if (parts > 1) {
    if (int rc = split_sync(e, true, G, parts, std::max(1, a.c.nlayers - 1), st, &a.xcnt, &a.xbase)) return rc;
    a.xabort = e->xabort_dev; a.ngroups = G;
  }
  const int grid = rows48_grid(G, parts);
  return with_rows48_form(e, parts, (e->tune.rows48_share & 2) != 0, [&](auto ct, auto light, auto np, auto share) {
    return hip_rc(e, "k_rows48_dgrad_chain", profiled(e, PC_DGRAD_ROWS, flops, st, [&] {
      SDRM_LAUNCH(e, (k_rows48_dgrad_chain<VAL(ct), VAL(light), VAL(np), VAL(share)>), dim3((unsigned)grid), dim3(NTHREADS), 0, st, a);
      return hipGetLastError();
    }));
  });
}

// the row-owned forward of the step `p` plans: staging, every layer and the loss partial sums of p.groups user groups in one launch
int launch_row_forward(sdrm_engine* e, const StepPlan& p, const float* x0, int64_t row0, int mode, const sdrm_train_randoms* rnd,
                       uint64_t seed, uint64_t step, float nd, hipStream_t st) {
  const int n = e->T + 1, G = p.groups;
  RowChainArgs a{};
  a.x0 = x0;
  if (mode == SDRM_RNG_EXPLICIT) { a.noise = rnd->noise; a.t = rnd->t; a.keep = rnd->keep; }
  a.sqrt_ab = e->sched + 3 * n; a.one_minus_ab = e->sched + 4 * n; a.tembP = e->tembP;
  a.B = p.B; a.L = e->L; a.T = e->T; a.H = e->H;
  a.mode = mode; a.seed_lo = (uint32_t)seed; a.seed_hi = (uint32_t)(seed >> 32); a.step = (uint32_t)step; a.row0 = row0; a.nd = nd;
  a.W0f = e->W0f; a.Whf = e->Whf; a.Wof = e->Wof; a.bh = e->bhc; a.bo = e->boc; a.B0tab = e->B0tab; a.ldtab = e->WP;
  a.slope0 = slope_ptr(e, 0); a.slopeh = e->H > 0 ? slope_ptr(e, 1) : slope_ptr(e, 0);
  a.U = e->U; a.K0 = e->K0; a.LPs = e->LP; a.tdev = e->tdev; a.ones_col = e->ones_col;
  a.light = rc_light_klast(e->W, e->WP) >= 0 ? 1 : 0;   // L == W on this path: one answer for every layer
  a.pre = e->pre; a.pre_stride = (size_t)e->MPmax * e->WP; a.ldp = e->WP; a.Y = e->Y; a.ldy = e->LP;
  a.act = e->act;
  a.loss_part = e->loss_part;
  a.sweep = (e->tune.rows48_share & 4) ? 1 : 0;
  a.skip_pre = p.skip_pre() ? 1 : 0;
  // profile class: the algorithmic flops of the H + 2 layers of the three passes (staging, loss sums and the streamed copies ride along)
  const double flops = 2.0 * 3 * a.B * ((double)e->W * e->L + (double)e->H * e->W * e->W + (double)e->L * e->W);
  if (p.path == StepPlan::ROW48) {
    if (p.parts > 1) {
      if (int rc = split_sync(e, false, G, p.parts, e->H + 1, st, &a.xcnt, &a.xbase)) return rc;
      a.xabort = e->xabort_dev; a.ngroups = G;
    }
    const int grid = rows48_grid(G, p.parts);
    return with_rows48_form(e, p.parts, (e->tune.rows48_share & 1) != 0, [&](auto ct, auto light, auto np, auto share) {
      return hip_rc(e, "k_rows48_fwd", profiled(e, PC_ROW_FWD, flops, st, [&] {
        SDRM_LAUNCH(e, (k_rows48_fwd<VAL(ct), VAL(light), VAL(np), VAL(share)>), dim3((unsigned)grid), dim3(NTHREADS), 0, st, a);
        return hipGetLastError();
      }));
    });
  }
  return with_row_form(e, [&](auto ct, auto light) {
    return hip_rc(e, "k_row_fwd", profiled(e, PC_ROW_FWD, flops, st, [&] {
      // two kernels: the one that draws its randoms itself, and the one that reads the step's noise / t / keep arrays (csrc/rowchain.h)
      if (mode == SDRM_RNG_EXPLICIT) SDRM_LAUNCH(e, (k_row_fwd_explicit<VAL(ct), VAL(light)>), dim3((unsigned)G), dim3(NTHREADS), 0, st, a);
      else SDRM_LAUNCH(e, (k_row_fwd<VAL(ct), VAL(light)>), dim3((unsigned)G), dim3(NTHREADS), 0, st, a);
      return hipGetLastError();
    }));
  });
}

// the narrow nets' train step (csrc/skinny_step.h): forward (which = 0) / backward (which = 1) over G = ceil(B / 16) user groups
SkStepArgs sk_step_args(sdrm_engine* e, int B) {
  SkStepArgs a{};
  const int n = e->T + 1;
  a.W0c = e->W0c; a.K0 = e->K0; a.Whc = e->Whc; a.Woc = e->Woc; a.bh = e->bhc; a.bo = e->boc;
  a.WhcT = e->WhcT; a.WocT = e->WocT; a.B0tab = e->B0tab;
  a.WeP = e->WeP; a.W0eP = e->W0eP; a.be = e->p + e->off_be; a.b0 = e->b0c; a.TPe = e->TPe; a.intab = e->WeP ? 1 : 0;
  a.slope0 = slope_ptr(e, 0); a.slopeh = e->H > 0 ? slope_ptr(e, 1) : slope_ptr(e, 0);
  a.sqrt_ab = e->sched + 3 * n; a.one_minus_ab = e->sched + 4 * n; a.tembP = e->tembP;
  a.B = B; a.L = e->L; a.W = e->W; a.T = e->T; a.H = e->H; a.G = (B + SK_USERS - 1) / SK_USERS;
  a.LPs = e->LP; a.WPs = e->WP; a.TPs = e->TP;
  a.U = e->U; a.tdev = e->tdev; a.pre = e->pre; a.pre_stride = (size_t)e->MPmax * e->WP; a.Y = e->Y;
  a.loss_part = e->loss_part; a.NP = a.G;
  a.slab0 = e->slab0; a.slabH = e->slabH; a.slabO = e->slabO; a.db0s = e->db0s; a.dbHs = e->dbHs; a.dbOs = e->dbOs;
  a.alpha_part = e->alpha_part; a.alpha_part_stride = e->alpha_part_stride;
  return a;
}

template <int NL, int NW>
int launch_sk_step_nlnw(sdrm_engine* e, const SkStepArgs& ka, int which, int grid, hipStream_t st) {
  typedef SkCfg<NL, NW> C;
  const size_t lds = (which == 0 ? sk_fwd_lds_floats<NL, NW>(ka.intab ? ka.TPe : 0) : sk_bwd_lds_floats<NL, NW>(ka.TPs)) * sizeof(float);
  if (lds > 48 * 1024) HIP_TRY(e, allow_full_lds(which == 0 ? (const void*)k_skinny_fwd<NL, NW> : (const void*)k_skinny_bwd<NL, NW>));
  if (which == 0) SDRM_LAUNCH(e, (k_skinny_fwd<NL, NW>), dim3((unsigned)grid), dim3(C::NTHR), lds, st, ka);
  else SDRM_LAUNCH(e, (k_skinny_bwd<NL, NW>), dim3((unsigned)grid), dim3(C::NTHR), lds, st, ka);
  HIP_TRY(e, hipGetLastError());
  return SDRM_OK;
}

// the narrow nets' forward on 4-row MFMA units (csrc/skinny_fwd4.h): one work-group per 4 users; false: the shape's LDS image does
// not fit (the caller takes k_skinny_fwd)
template <int NL, int NW>
int launch_sk_fwd4_nlnw(sdrm_engine* e, const SkStepArgs& ka, hipStream_t st, bool* done) {
  const size_t lds = sk4_fwd_lds_floats<NL, NW>(ka.intab ? ka.TPe : 0) * sizeof(float);
  *done = false;
  if (lds > 160 * 1024) return SDRM_OK;
  if (lds > 48 * 1024) HIP_TRY(e, allow_full_lds((const void*)k_skinny_fwd4<NL, NW>));
  SDRM_LAUNCH(e, (k_skinny_fwd4<NL, NW>), dim3((unsigned)std::min(ka.NP, 8192)), dim3(SK4_THREADS), lds, st, ka);
  HIP_TRY(e, hipGetLastError());
  *done = true;
  return SDRM_OK;
}

int launch_sk_fwd4(sdrm_engine* e, const SkStepArgs& ka, hipStream_t st, bool* done) {
  return with_skinny_form(e, [&](auto nl, auto nw) { return launch_sk_fwd4_nlnw<VAL(nl), VAL(nw)>(e, ka, st, done); });
}

int launch_sk_step(sdrm_engine* e, const SkStepArgs& ka, int which, int grid, hipStream_t st) {
  return with_skinny_form(e, [&](auto nl, auto nw) { return launch_sk_step_nlnw<VAL(nl), VAL(nw)>(e, ka, which, grid, st); });
}

// eps-net layers 1..H and the output pre-activation inputs; layer 0 is launched by the caller
// (its bias / K differ between training and sampling).
// post_act (the sampler): every buffer holds the layer's ACTIVATION - the producer's epilogue applied PReLU, the operand is
// loaded as it is; otherwise (training, which needs the pre-activations for its backward) PReLU is applied on operand load.
// what a forward reads of the net: the live compute copies, or the sampler's snapshot of them
struct NetView { const float *W0c, *Whc, *Woc, *bhc, *boc, *B0tab, *slope0, *slopeh; };
NetView snapshot_view(const sdrm_engine* e) {
  const float* b = e->smp_w;
  return NetView{b + e->smp_off[0], b + e->smp_off[1], b + e->smp_off[2], b + e->smp_off[3], b + e->smp_off[4], b + e->smp_off[5],
                 b + e->smp_off[6], b + e->smp_off[6] + 1};
}

int hidden_forward(sdrm_engine* e, int MP, int rows, hipStream_t st, int cfg, int r0 = 0, int cls = PC_FWD_HIDDEN,
                   bool post_act = false, const NetView* nv = nullptr) {
  const double fl = 2.0 * rows * (double)e->W * e->W;
  const size_t ro = (size_t)r0 * e->WP;
  for (int k = 1; k <= e->H; ++k) {
    if (post_act) {
      GemmArgs a{};
      // (nv: a sampling step - the snapshot's weights, the sampler's own layer buffers)
      a.C = (nv ? smp_buf(e, k) : pre_buf(e, k)) + ro; a.ldc = e->WP; a.bias = nv ? nv->bhc : e->bhc; a.slopeE = nv ? nv->slopeh : slope_ptr(e, k);
      HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_PRELU>(a, (nv ? smp_buf(e, k - 1) : pre_buf(e, k - 1)) + ro, e->WP, nv ? nv->Whc : e->Whc, e->WP, MP, e->WP, e->WP,
                                                         st, Prof{e, cls, fl}, cfg)));
      continue;
    }
    GemmArgs a{};
    a.C = pre_buf(e, k) + ro; a.ldc = e->WP; a.bias = e->bhc; a.slopeA = slope_ptr(e, k - 1);
    HIP_TRY(e, (gemm_forward<XF_PRELU, EPI_BIAS>(a, pre_buf(e, k - 1) + ro, e->WP, e->Whc, e->WP, MP, e->WP, e->WP, st,
                                                 Prof{e, cls, fl}, cfg)));
  }
  return SDRM_OK;
}

int upload_schedule(sdrm_engine* e, float beta1, float beta2) {
  const int T = e->T, n = T + 1;
  // fp32 arithmetic in the reference's op order (train_SDRM.py:300-303): linspace, affine, 1-b, log, cumsum, exp
  std::vector<float> b(n), al(n), ab(n), sq(n), om(n);
  const float step = 1.0f / (float)T;  // torch.linspace(0,1,T+1): start + i*step for the lower half, end - (n-1-i)*step above
  float run = 0.f;
  for (int i = 0; i < n; ++i) {
    const float lin = (i < n / 2) ? (0.f + step * (float)i) : (1.f - step * (float)(n - 1 - i));
    b[i] = (beta2 - beta1) * lin + beta1;
    al[i] = 1.f - b[i];
    run += std::log(al[i]);
    ab[i] = std::exp(run);
  }
  ab[0] = 1.f;
  for (int i = 0; i < n; ++i) { sq[i] = std::sqrt(ab[i]); om[i] = 1.f - ab[i]; }
  e->h_beta = b; e->h_alpha = al; e->h_alphabar = ab;
  HIP_TRY(e, hipMemcpy(e->sched + 0 * n, b.data(), n * 4, hipMemcpyHostToDevice));
  HIP_TRY(e, hipMemcpy(e->sched + 1 * n, al.data(), n * 4, hipMemcpyHostToDevice));
  HIP_TRY(e, hipMemcpy(e->sched + 2 * n, ab.data(), n * 4, hipMemcpyHostToDevice));
  HIP_TRY(e, hipMemcpy(e->sched + 3 * n, sq.data(), n * 4, hipMemcpyHostToDevice));
  HIP_TRY(e, hipMemcpy(e->sched + 4 * n, om.data(), n * 4, hipMemcpyHostToDevice));
  if (e->rev_dev) {   // (1-alpha)/sqrt(1-alphabar), sqrt(alpha), sqrt(beta) per step, fp32 like the reference (:23-24)
    std::vector<float> rev(3 * (size_t)n, 0.f);
    for (int i = 1; i < n; ++i) {
      rev[i] = (1.f - al[i]) / std::sqrt(1.f - ab[i]);
      rev[n + i] = std::sqrt(al[i]);
      rev[2 * n + i] = std::sqrt(b[i]);
    }
    HIP_TRY(e, hipMemcpy(e->rev_dev, rev.data(), rev.size() * 4, hipMemcpyHostToDevice));
  }
  return SDRM_OK;
}

int upload_temb(sdrm_engine* e) {
  const int T = e->T, half = T / 2;
  std::vector<float> tab((size_t)(T + 1) * T, 0.f), freqs(half);
  // train_SDRM.py:105-112 in fp32: exp(-ln(1e4) * k / half)
  const float nl = -(float)std::log(10000.0);
  for (int k = 0; k < half; ++k) freqs[k] = std::exp(nl * (float)k / (float)half);
  for (int t = 0; t <= T; ++t)
    for (int k = 0; k < half; ++k) {
      const float arg = (float)t * freqs[k];
      tab[(size_t)t * T + k] = std::cos(arg);
      tab[(size_t)t * T + half + k] = std::sin(arg);
    }
  HIP_TRY(e, hipMemcpy(e->temb, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));
  // rows padded to TP floats: what the train step's staging copies into the trailing columns of the layer-0 operand
  HIP_TRY(e, hipMemcpy2D(e->tembP, (size_t)e->TP * 4, tab.data(), (size_t)T * 4, (size_t)T * 4, (size_t)(T + 1), hipMemcpyHostToDevice));
  return SDRM_OK;
}

void reverse_coeffs(const sdrm_engine* e, int i, float& c1, float& sa, float& sb) {
  const float a = e->h_alpha[i], ab = e->h_alphabar[i], b = e->h_beta[i];
  c1 = (1.f - a) / std::sqrt(1.f - ab);
  sa = std::sqrt(a);
  sb = std::sqrt(b);
}

}  // namespace

// =================================================================================================
extern "C" {

int sdrm_debug_set_rowchain(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  if (e->bwd_begun) return fail(e, SDRM_ERR_STATE, "sdrm_debug_set_rowchain: a two-call backward is in progress");
  e->fwd_done = false;   // a pending forward's stacked row order belongs to the old setting
  e->tune.rowchain = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return SDRM_OK;
}

int sdrm_debug_set_rows48(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  if (e->bwd_begun) return fail(e, SDRM_ERR_STATE, "sdrm_debug_set_rows48: between sdrm_train_backward_begin and _finish");
  e->fwd_done = false;   // a pending forward's stacked row order belongs to the old setting
  e->tune.rows48 = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return SDRM_OK;
}

int sdrm_debug_set_rows48_split(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  if (e->bwd_begun) return fail(e, SDRM_ERR_STATE, "sdrm_debug_set_rows48_split: between sdrm_train_backward_begin and _finish");
  if (mode != 0 && mode != 1 && mode != 2 && mode != 4) return fail(e, SDRM_ERR_ARG, "sdrm_debug_set_rows48_split: 0, 1, 2 or 4");
  e->fwd_done = false;
  e->tune.split = mode;
  return SDRM_OK;
}

int sdrm_debug_rows48_split_available(const sdrm_engine* e) { return e && e->W0f && e->xcd_ok ? 1 : 0; }

int sdrm_debug_set_rows48_share(sdrm_engine* e, int on) {
  if (!e) return SDRM_ERR_ARG;
  e->tune.rows48_share = on == 1 ? 7 : (on == 2 ? 5 : (on == 3 ? 2 : 0));   // 1: forward (with its sweep) and chain, 2: the forward only, 3: the chain only
  return SDRM_OK;
}

int sdrm_debug_set_sample_persist(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  if (e->call.active) return fail(e, SDRM_ERR_STATE, "sdrm_debug_set_sample_persist: inside a sampling call");
  e->tune.smp_persist = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return SDRM_OK;
}

int sdrm_debug_split_skew(sdrm_engine* e, unsigned skew) {
  if (!e) return SDRM_ERR_ARG;
  e->xskew = skew;
  return SDRM_OK;
}

int sdrm_debug_rowchain_available(const sdrm_engine* e) { return e && e->W0f ? 1 : 0; }

int sdrm_debug_set_wgrad_strips(sdrm_engine* e, int on) {
  if (!e) return SDRM_ERR_ARG;
  e->tune.strips = on ? 1 : 0;
  return SDRM_OK;
}

int sdrm_debug_set_dgrad_rows(sdrm_engine* e, int on) {
  if (!e) return SDRM_ERR_ARG;
  e->fwd_done = false;   // a pending row-owned forward chose what it stores (pre-activations or not) by the old setting
  e->tune.dgrad_rows = on < 0 ? 0 : (on > 2 ? 2 : on);
  return SDRM_OK;
}

int sdrm_debug_set_skinny(sdrm_engine* e, int on) {
  if (!e) return SDRM_ERR_ARG;
  e->tune.skinny = on < 0 ? 0 : (on > 2 ? 2 : on);
  return SDRM_OK;
}

int sdrm_debug_set_csrt_mark(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  e->csrt_mark_mode = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return SDRM_OK;
}

int sdrm_debug_plan_wgrad(int rows, int n_out, int k_in, int* slices, int* rows_per_slice) {
  if (!slices || !rows_per_slice || rows < 1 || n_out < 1 || k_in < 1) return SDRM_ERR_ARG;
  pick_splits(Tuning{}, rows, wgrad_tiles(Tuning{}, n_out, k_in), *slices, *rows_per_slice);
  return SDRM_OK;
}

int sdrm_debug_philox_draws(sdrm_engine* e, uint64_t seed, uint32_t purpose, uint32_t step, int64_t row0, int rows, int quads,
                            float* normals, uint8_t* lowbits, void* stream) {
  if (!e || !normals || rows < 1 || quads < 1) return fail(e, SDRM_ERR_ARG, "sdrm_debug_philox_draws: bad argument");
  const size_t total = (size_t)rows * quads;
  SDRM_LAUNCH(e, k_philox_draws, dim3((unsigned)std::min<size_t>(8192, (total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
              (uint32_t)seed, (uint32_t)(seed >> 32), purpose, step, row0, rows, quads, normals, lowbits);
  HIP_TRY(e, hipGetLastError());
  return SDRM_OK;
}

int sdrm_debug_set_fused_reverse(sdrm_engine* e, int mode) {
  if (!e) return SDRM_ERR_ARG;
  e->tune.fuse_rev = mode < 0 ? 0 : (mode > 2 ? 2 : mode);
  return SDRM_OK;
}

int sdrm_debug_set_gradient_buckets(sdrm_engine* e, int buckets) {
  if (!e || (buckets != 1 && buckets != 2)) return SDRM_ERR_ARG;
  e->tune.ar_buckets = buckets;
  return SDRM_OK;
}

int sdrm_debug_set_chains(sdrm_engine* e, int chains) {
  if (!e) return SDRM_ERR_ARG;
  e->tune.chains = chains;
  return SDRM_OK;
}

int sdrm_debug_chains(const sdrm_engine* e) { return e ? e->call.chains : 0; }

// the names of include/sdrm_hip_debug.h are the enumerators of StepPlan / SampleCall
static_assert(SDRM_PLAN_PER_LAYER == (int)StepPlan::PER_LAYER && SDRM_PLAN_SKINNY == (int)StepPlan::SKINNY &&
              SDRM_PLAN_ROW96 == (int)StepPlan::ROW96 && SDRM_PLAN_ROW48 == (int)StepPlan::ROW48, "sdrm_hip_debug.h: train paths");
static_assert(SDRM_PLAN_DGRAD_TILES == (int)StepPlan::TILES && SDRM_PLAN_DGRAD_ROWS_PER_LAYER == (int)StepPlan::ROWS_PER_LAYER &&
              SDRM_PLAN_DGRAD_CHAIN == (int)StepPlan::CHAIN && SDRM_PLAN_DGRAD_SKINNY_OWN == (int)StepPlan::SKINNY_OWN, "sdrm_hip_debug.h: dgrads");
static_assert(SDRM_SAMPLE_PATH_SKINNY == (int)SampleCall::SKINNY && SDRM_SAMPLE_PATH_PERSIST == (int)SampleCall::PERSIST &&
              SDRM_SAMPLE_PATH_PER_LAYER == (int)SampleCall::PER_LAYER, "sdrm_hip_debug.h: sampling paths");

int sdrm_debug_last_plan(const sdrm_engine* e, int* train_path, int* parts, int* dgrad, int* sample_path) {
  if (!e) return SDRM_ERR_ARG;
  if (train_path) *train_path = (int)e->plan.path;
  if (parts) *parts = e->plan.parts;
  if (dgrad) *dgrad = (int)e->plan.dgrad;
  if (sample_path) *sample_path = (int)e->call.path;
  return SDRM_OK;
}

int sdrm_debug_set_tile(sdrm_engine* e, int cfg) {
  if (!e) return SDRM_ERR_ARG;
  if (e->bwd_begun || e->call.active)
    return fail(e, SDRM_ERR_STATE, "sdrm_debug_set_tile: a two-call backward or a sampling call is in progress");
  e->fwd_done = false;   // the slope-partial layout of a backward is fixed by its forward's tile: a pending forward is dropped
  e->tune.force_cfg = cfg;
  return SDRM_OK;
}

int sdrm_debug_set_nt32_rows(sdrm_engine* e, int max_rows, int max_rows_train) {
  if (!e) return SDRM_ERR_ARG;
  if (max_rows >= 0) e->tune.nt32_max_rows = max_rows;
  if (max_rows_train >= 0) e->tune.nt32_max_rows_train = max_rows_train;
  return SDRM_OK;
}

#ifndef SDRM_SOURCE_HASH
#define SDRM_SOURCE_HASH "unhashed"
#endif
// "SDRM_SOURCE_HASH=<hex>" is also what sdrm_amd/_build.py looks for in the file to decide whether the binary belongs to
// the sources next to it.
static const char kSourceHashMarker[] = "SDRM_SOURCE_HASH=" SDRM_SOURCE_HASH;
const char* sdrm_source_hash(void) { return kSourceHashMarker + sizeof("SDRM_SOURCE_HASH=") - 1; }

const char* sdrm_build_info(void) {
  return "gfx950 fp32 v_mfma_f32_32x32x2_f32; block tile 64x64x16 (32x32x32 on v_mfma_f32_16x16x4_f32 for NT launches of at "
         "most 4096 rows, 8192 stacked rows in the train step), 4 waves, two LDS stages + register-double-buffered fragments, "
         "pipeline pieces in the MFMA shadows, k-minor LDS + ds_read_b128 for NT; split-K slabs for wgrad; persistent "
         "LDS-resident kernels for widths <= 64; one-round grids sized for 256 compute units in 8 XCDs (sdrm_create refuses any "
         "other device); sources " SDRM_SOURCE_HASH;
}

const char* sdrm_last_error(const sdrm_engine* e) { return e ? e->err.c_str() : "null engine"; }

// The chip this library is written for: gfx950 with all 256 compute units in one device (MI355X, SPX mode).  The one-round grids
// (k_row_fwd, k_dgrad_chain, k_wgrad_strips: one work-group per CU), the split-K plans (1280 resident work-groups) and the
// work-group -> XCD mapping (block b on XCD b & 7, xcd_remap) are sized for exactly that; on another CU count they would run,
// silently mis-balanced.  sdrm_create refuses instead (SDRM_ALLOW_ANY_DEVICE=1 lifts the CU-count check for experiments).
constexpr int SDRM_TARGET_CUS = 256;
int sdrm_debug_device_check(const char* gcn_arch, int compute_units) {
  if (!gcn_arch) return SDRM_ERR_ARG;
  if (std::strncmp(gcn_arch, "gfx950", 6) != 0 || (gcn_arch[6] != '\0' && gcn_arch[6] != ':')) return SDRM_ERR_DEVICE;
  return compute_units == SDRM_TARGET_CUS ? SDRM_OK : SDRM_ERR_DEVICE;
}
int64_t sdrm_param_count(const sdrm_engine* e) { return e ? e->P : -1; }

int sdrm_create(int L, int W, int T, int H, int max_rows, int device_id, sdrm_engine** out) {
  if (!out) return SDRM_ERR_ARG;
  *out = nullptr;
  if (L < 1 || L > 4096 || W < 1 || W > 4096 || T < 2 || T > 1024 || H < 0 || H > 16 || max_rows < 1 ||
      max_rows > (1 << 22))
    return SDRM_ERR_SHAPE;
  // k_tail_emb (csrc/tail.h) keeps TE_JT rows of emb_layer.weight beside a [TE_RB][TP] block of M in LDS: the image grows with T and
  // passes the CU's 160 KB at T = 1021 (the reference's search space ends at T = 198, hyperparameter_search.py:108)
  if (tail_emb_lds_floats(T, round_up(T + 1, 32)) * sizeof(float) > 160 * 1024) return SDRM_ERR_SHAPE;
  sdrm_engine* e = new sdrm_engine();
  // the only place the environment is read: the settings then belong to this handle
  if (const char* env = std::getenv("SDRM_TILE")) e->tune.force_cfg = std::atoi(env);
  if (const char* env = std::getenv("SDRM_CHAINS")) e->tune.chains = std::atoi(env);
  if (const char* env = std::getenv("SDRM_HOLD_EARLY")) e->tune.hold_early = std::atoi(env);
  if (const char* env = std::getenv("SDRM_DETACH")) e->tune.detach = std::atoi(env);
  if (const char* env = std::getenv("SDRM_FUSE_REV")) e->tune.fuse_rev = std::atoi(env);
  if (const char* env = std::getenv("SDRM_NT32_MAX_ROWS")) e->tune.nt32_max_rows = std::atoi(env);
  if (const char* env = std::getenv("SDRM_NT32_MAX_ROWS_TRAIN")) e->tune.nt32_max_rows_train = std::atoi(env);
  if (const char* env = std::getenv("SDRM_WGRAD_BLOCKS")) e->tune.wgrad_blocks = std::max(1, std::atoi(env));
  if (const char* env = std::getenv("SDRM_WGRAD_ROUND")) e->tune.wgrad_round = std::max(1, std::atoi(env));
  if (const char* env = std::getenv("SDRM_AR_BUCKETS")) e->tune.ar_buckets = std::atoi(env);
  if (const char* env = std::getenv("SDRM_WGRAD_SLICES")) e->tune.wgrad_slices = std::min(S_MAX, std::max(0, std::atoi(env)));
  if (const char* env = std::getenv("SDRM_ROWCHAIN")) e->tune.rowchain = std::atoi(env);
  if (const char* env = std::getenv("SDRM_ROWS48")) e->tune.rows48 = std::atoi(env);
  if (const char* env = std::getenv("SDRM_ROWS48_SPLIT")) e->tune.split = std::atoi(env);
  if (const char* env = std::getenv("SDRM_SAMPLE_PERSIST")) e->tune.smp_persist = std::atoi(env);
  if (const char* env = std::getenv("SDRM_ROWS48_SHARE")) e->tune.rows48_share = std::atoi(env);
  if (const char* env = std::getenv("SDRM_WGRAD_STRIPS")) e->tune.strips = std::atoi(env);
  if (const char* env = std::getenv("SDRM_DGRAD_ROWS")) e->tune.dgrad_rows = std::atoi(env);
  e->L = L; e->W = W; e->T = T; e->H = H; e->max_rows = max_rows; e->device = device_id;
  e->LP = round_up(L, 32); e->WP = round_up(W, 32); e->TP = round_up(T + 1, 32); e->K0 = e->LP + e->TP;
  e->MPmax = round_up(RC_ROWS * ((max_rows + RC_USERS - 1) / RC_USERS), 128);   // either stacked row order fits
  int64_t o = 0;
  e->off_we = o; o += (int64_t)T * T;
  e->off_be = o; o += T;
  e->off_w0 = o; o += (int64_t)W * (L + T);
  e->off_b0 = o; o += W;
  e->off_a0 = o; o += 1;
  if (H >= 1) {
    e->off_wh = o; o += (int64_t)W * W;
    e->off_bh = o; o += W;
    e->off_ah = o; o += 1;
  } else {
    e->off_wh = e->off_bh = e->off_ah = -1;
  }
  e->off_wo = o; o += (int64_t)L * W;
  e->off_bo = o; o += L;
  e->P = o;
  *out = e;  // handed out even on failure below so the caller can read the message and destroy
  HIP_TRY(e, hipSetDevice(device_id));
  {
    hipDeviceProp_t prop;
    HIP_TRY(e, hipGetDeviceProperties(&prop, device_id));
    const char* any = std::getenv("SDRM_ALLOW_ANY_DEVICE");
    const bool lifted = any && std::atoi(any) != 0;
    if (sdrm_debug_device_check(prop.gcnArchName, lifted ? SDRM_TARGET_CUS : prop.multiProcessorCount) != SDRM_OK)
      return fail(e, SDRM_ERR_DEVICE, std::string("sdrm_create: device ") + std::to_string(device_id) + " is " + prop.gcnArchName + " with " +
                                          std::to_string(prop.multiProcessorCount) + " compute units; this library is built for gfx950 with " +
                                          std::to_string(SDRM_TARGET_CUS) + " (MI355X, SPX mode): its one-round grids and XCD mapping assume them");
  }
  const size_t MP = e->MPmax;
  const int n = T + 1;
  HIP_TRY(e, dalloc(&e->p, e->P)); HIP_TRY(e, dalloc(&e->m, e->P));
  HIP_TRY(e, dalloc(&e->v, e->P)); HIP_TRY(e, dalloc(&e->g, e->P));
  HIP_TRY(e, dalloc(&e->W0c, (size_t)round_up(e->WP, 128) * e->K0)); HIP_TRY(e, dalloc(&e->b0c, e->WP));
  HIP_TRY(e, dalloc(&e->Whc, (size_t)round_up(e->WP, 128) * e->WP)); HIP_TRY(e, dalloc(&e->bhc, e->WP));
  HIP_TRY(e, dalloc(&e->Woc, (size_t)round_up(e->LP, 128) * e->WP)); HIP_TRY(e, dalloc(&e->boc, e->LP));
  HIP_TRY(e, dalloc(&e->WhcT, (size_t)round_up(e->WP, 128) * e->WP)); HIP_TRY(e, dalloc(&e->WocT, (size_t)round_up(e->WP, 128) * e->LP));
  if (L == W && e->WP >= 128 && e->WP <= 352) {   // the row-owned forward's shape envelope (rowchain.h); L == W (every call site of the
                                                  // reference): the ones column round_up(W, 4) must be a pad column of U as well
    HIP_TRY(e, dalloc(&e->W0f, (size_t)e->WP * e->WP)); HIP_TRY(e, dalloc(&e->Whf, (size_t)e->WP * e->WP));
    HIP_TRY(e, dalloc(&e->Wof, (size_t)e->WP * e->WP));
    HIP_TRY(e, dalloc(&e->WhfT, (size_t)e->WP * e->WP)); HIP_TRY(e, dalloc(&e->WofT, (size_t)e->WP * e->WP));
    HIP_TRY(e, dalloc(&e->act, (size_t)(H + 1) * e->MPmax * e->WP));
    if (round_up(W, 4) < e->WP) e->ones_col = round_up(W, 4);
  }
  HIP_TRY(e, dalloc(&e->temb, (size_t)n * T)); HIP_TRY(e, dalloc(&e->tembP, (size_t)n * e->TP));
  HIP_TRY(e, dalloc(&e->B0tab, (size_t)n * e->WP)); HIP_TRY(e, dalloc(&e->sched, (size_t)8 * n));
  HIP_TRY(e, dalloc(&e->rev_dev, (size_t)3 * n));
  {
    const size_t sz[7] = {(size_t)round_up(e->WP, 128) * e->K0, (size_t)round_up(e->WP, 128) * e->WP, (size_t)round_up(e->LP, 128) * e->WP,
                          (size_t)e->WP, (size_t)e->LP, (size_t)n * e->WP, 4};
    size_t tot = 0;
    for (int k = 0; k < 7; ++k) { e->smp_off[k] = tot; tot += (sz[k] + 63) / 64 * 64; }   // 256-byte aligned pieces
    HIP_TRY(e, dalloc(&e->smp_w, tot));
  }
  HIP_TRY(e, dalloc(&e->sel, 1));
  HIP_TRY(e, dalloc(&e->one_dev, 4));
  HIP_TRY(e, dalloc(&e->feed_flag, 4));
  HIP_TRY(e, dalloc(&e->nll_part, NLL_PARTS));
  if (e->W0f) {
    // column-split row groups (csrc/rows48.h): hand-shake counters, the host-visible abort word, and the check of the one property
    // of the chip the path rests on - work-group b of a launch runs on XCD b & 7 - with a probe launch
    HIP_TRY(e, dalloc(&e->xcntF, (size_t)256 * 32)); HIP_TRY(e, dalloc(&e->xcntC, (size_t)256 * 32));
    HIP_TRY(e, dalloc(&e->xcntS, (size_t)256 * 32));
    HIP_TRY(e, hipHostMalloc((void**)&e->xabort_host, sizeof(unsigned), hipHostMallocMapped));
    *e->xabort_host = 0u;
    HIP_TRY(e, hipHostGetDevicePointer((void**)&e->xabort_dev, e->xabort_host, 0));
    unsigned* probe = nullptr;
    constexpr int NPROBE = 512;
    HIP_TRY(e, dalloc(&probe, NPROBE));
    hipLaunchKernelGGL(k_xcc_probe, dim3(NPROBE), dim3(64), 0, 0, probe);
    std::vector<unsigned> xcc(NPROBE);
    HIP_TRY(e, hipMemcpy(xcc.data(), probe, NPROBE * sizeof(unsigned), hipMemcpyDeviceToHost));
    HIP_TRY(e, hipFree(probe));
    bool ok = true;
    std::set<unsigned> ids;
    for (int b = 0; b < NPROBE; ++b) ok = ok && (xcc[b] & 0xfu) == (xcc[b & 7] & 0xfu);
    for (int x = 0; x < 8; ++x) ids.insert(xcc[x] & 0xfu);
    e->xcd_ok = ok && ids.size() == 8;
  }
  {
    const float one = 1.0f;
    HIP_TRY(e, hipMemcpy(e->one_dev, &one, 4, hipMemcpyHostToDevice));
    // the ones column: pad entry ones_col of the hidden layer's padded bias is 1 (its weight row there is zero, so the
    // pre-activation and the activation of that pad column are 1 in every row; the next layer's weight column there is zero, so
    // nothing else changes); layer 0's comes from B0tab (k_emb_tables), U's from the row-owned forward's staging
    if (e->ones_col >= 0) HIP_TRY(e, hipMemcpy(e->bhc + e->ones_col, &one, 4, hipMemcpyHostToDevice));
  }
  HIP_TRY(e, dalloc(&e->U, MP * e->K0)); HIP_TRY(e, dalloc(&e->pre, (size_t)(H + 1) * MP * e->WP));
  HIP_TRY(e, dalloc(&e->Y, MP * e->LP)); HIP_TRY(e, dalloc(&e->dY, MP * e->LP));
  HIP_TRY(e, dalloc(&e->dA, (size_t)(H + 1) * MP * e->WP));   // dpre_buf(0..H)
  HIP_TRY(e, dalloc(&e->X, MP * e->LP)); HIP_TRY(e, dalloc(&e->Us, MP * e->LP));
  HIP_TRY(e, dalloc(&e->smp_pre, (size_t)(H + 1) * MP * e->WP)); HIP_TRY(e, dalloc(&e->smp_Y, MP * e->LP));
  HIP_TRY(e, dalloc(&e->slab0, (size_t)S_MAX * e->WP * e->K0)); HIP_TRY(e, dalloc(&e->db0s, (size_t)S_MAX * e->WP));
  HIP_TRY(e, dalloc(&e->slabO, (size_t)S_MAX * e->LP * e->WP)); HIP_TRY(e, dalloc(&e->dbOs, (size_t)S_MAX * e->LP));
  if (H >= 1) {
    HIP_TRY(e, dalloc(&e->slabH, (size_t)H * S_MAX * e->WP * e->WP));
    HIP_TRY(e, dalloc(&e->dbHs, (size_t)H * S_MAX * e->WP));
  }
  e->alpha_part_stride = std::max(max_gemm_blocks((int)MP, e->WP), (int)MP / 16);
  HIP_TRY(e, dalloc(&e->alpha_part, (size_t)(H + 1) * e->alpha_part_stride));
  HIP_TRY(e, dalloc(&e->loss_part, (size_t)4 * std::max<size_t>(LOSS_BLOCKS, 4 * (MP / SK_ROWS + 1)))); HIP_TRY(e, dalloc(&e->sums, 8));
  if (e->LP <= 64 && e->WP <= 64 && T <= 128) {
    e->TPe = round_up(T, 16);
    HIP_TRY(e, dalloc(&e->WeP, (size_t)e->TPe * e->TPe)); HIP_TRY(e, dalloc(&e->W0eP, (size_t)e->WP * e->TPe));
  }
  HIP_TRY(e, dalloc(&e->Mred, (size_t)W * e->TP)); HIP_TRY(e, dalloc(&e->snap, (size_t)T * T + T + (size_t)W * T));
  HIP_TRY(e, allow_full_lds((const void*)k_tail_emb));
  HIP_TRY(e, dalloc(&e->tdev, max_rows)); HIP_TRY(e, dalloc(&e->Tj_dev, max_rows)); HIP_TRY(e, dalloc(&e->rowid_dev, max_rows));
  HIP_TRY(e, hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  HIP_TRY(e, hipEventCreateWithFlags(&e->ev_hold, hipEventDisableTiming));
  for (int c = 0; c < 3; ++c) {
    HIP_TRY(e, hipStreamCreateWithFlags(&e->aux[c], hipStreamNonBlocking));
    HIP_TRY(e, hipEventCreateWithFlags(&e->ev_join[c], hipEventDisableTiming));
  }
  int rc = upload_schedule(e, 1e-4f, 0.02f);
  if (rc) return rc;
  rc = upload_temb(e);
  if (rc) return rc;
  HIP_TRY(e, hipDeviceSynchronize());
  return SDRM_OK;
}

int sdrm_destroy(sdrm_engine* e) {
  if (!e) return SDRM_ERR_ARG;
  (void)hipSetDevice(e->device);
  void* bufs[] = {e->p, e->m, e->v, e->g, e->W0c, e->b0c, e->Whc, e->bhc, e->Woc, e->boc, e->temb, e->tembP, e->B0tab,
                  e->sched, e->U, e->pre, e->Y, e->dY, e->dA, e->X, e->slab0, e->slabH, e->slabO, e->db0s,
                  e->dbHs, e->dbOs, e->alpha_part, e->loss_part, e->sums, e->Mred, e->snap, e->WeP, e->W0eP, e->tdev, e->Tj_dev, e->rowid_dev, e->rev_dev, e->Us, e->WhcT, e->WocT, e->sel, e->one_dev, e->feed_flag, e->smp_w, e->W0f, e->Whf, e->Wof, e->act, e->WhfT, e->WofT, e->smp_pre, e->smp_Y};
  for (void* b : bufs)
    if (b) (void)hipFree(b);
  if (e->xcntF) (void)hipFree(e->xcntF);
  if (e->xcntC) (void)hipFree(e->xcntC);
  if (e->xcntS) (void)hipFree(e->xcntS);
  for (hipEvent_t ev : e->prof_ev) (void)hipEventDestroy(ev);
  (void)hipDeviceSynchronize();
  if (e->xabort_host) (void)hipHostFree(e->xabort_host);
  (void)sdrm_comm_destroy(e);
  for (const auto& s : e->scratch)
    if (s.p) (void)hipFree(s.p);
  if (e->nll_part) (void)hipFree(e->nll_part);
  if (e->csr_nnz_host) (void)hipHostFree(e->csr_nnz_host);
  if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
  if (e->ev_hold) (void)hipEventDestroy(e->ev_hold);
  for (int c = 0; c < 3; ++c) {
    if (e->ev_join[c]) (void)hipEventDestroy(e->ev_join[c]);
    if (e->aux[c]) (void)hipStreamDestroy(e->aux[c]);
  }
  if (e->draw_stream) (void)hipStreamDestroy(e->draw_stream);
  delete e;
  return SDRM_OK;
}

int sdrm_set_schedule(sdrm_engine* e, float beta1, float beta2) {
  if (!e) return SDRM_ERR_ARG;
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipDeviceSynchronize());
  return upload_schedule(e, beta1, beta2);
}

int sdrm_get_schedule(const sdrm_engine* e, float* b, float* a, float* ab) {
  if (!e || !b || !a || !ab) return SDRM_ERR_ARG;
  const size_t n = (size_t)e->T + 1;
  std::memcpy(b, e->h_beta.data(), n * 4);
  std::memcpy(a, e->h_alpha.data(), n * 4);
  std::memcpy(ab, e->h_alphabar.data(), n * 4);
  return SDRM_OK;
}

int sdrm_set_params(sdrm_engine* e, const float* flat, void* stream) {
  if (!e || !flat) return fail(e, SDRM_ERR_ARG, "sdrm_set_params: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  HIP_TRY(e, hipMemcpyAsync(e->p, flat, e->P * 4, hipMemcpyDeviceToDevice, st));
  return launch_adam(e, nullptr, 0.f, 0, st);  // re-pack only
}

int sdrm_get_params(const sdrm_engine* e, float* flat, void* stream) {
  if (!e || !flat) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  HIP_TRY(me, hipMemcpyAsync(flat, e->p, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SDRM_OK;
}

const float* sdrm_params_ptr(const sdrm_engine* e) { return e ? e->p : nullptr; }

int sdrm_get_grads(const sdrm_engine* e, float* flat, void* stream) {
  if (!e || !flat) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  HIP_TRY(me, hipMemcpyAsync(flat, e->grad_src ? e->grad_src : e->g, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SDRM_OK;
}

int sdrm_get_adam_state(const sdrm_engine* e, float* m, float* v, int64_t* step_host, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  if (m) HIP_TRY(me, hipMemcpyAsync(m, e->m, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (v) HIP_TRY(me, hipMemcpyAsync(v, e->v, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (step_host) *step_host = e->adam_t;
  return SDRM_OK;
}

int sdrm_set_adam_state(sdrm_engine* e, const float* m, const float* v, int64_t step, void* stream) {
  if (!e || step < 0) return fail(e, SDRM_ERR_ARG, "sdrm_set_adam_state: bad argument");
  if (m) HIP_TRY(e, hipMemcpyAsync(e->m, m, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  if (v) HIP_TRY(e, hipMemcpyAsync(e->v, v, e->P * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  e->adam_t = step;
  return SDRM_OK;
}

int sdrm_adam_reset(sdrm_engine* e, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  HIP_TRY(e, hipMemsetAsync(e->m, 0, e->P * 4, (hipStream_t)stream));
  HIP_TRY(e, hipMemsetAsync(e->v, 0, e->P * 4, (hipStream_t)stream));
  e->adam_t = 0;
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// fold_sums (sdrm_train_step): the backward folds the loss partials itself - no k_loss_sums launch here
static int train_forward_impl(sdrm_engine* e, const float* x0, int B, int64_t row0, int mode, const sdrm_train_randoms* rnd,
                              uint64_t seed, uint64_t step, float nd, double* sums, void* stream, bool fold_sums) {
  if (!e || !x0) return fail(e, SDRM_ERR_ARG, "sdrm_train_forward: null pointer");
  if (B < 1 || B > e->max_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_train_forward: B outside [1, max_rows]");
  if (mode == SDRM_RNG_EXPLICIT && (!rnd || !rnd->noise || !rnd->t || !rnd->keep))
    return fail(e, SDRM_ERR_ARG, "sdrm_train_forward: EXPLICIT mode needs noise, t and keep");
  if (mode != SDRM_RNG_EXPLICIT && mode != SDRM_RNG_PHILOX) return fail(e, SDRM_ERR_ARG, "bad rng mode");
  hipStream_t st = (hipStream_t)stream;
  e->bwd_begun = false;   // a backward that was begun but never finished is abandoned
  if (int cr = chains_train_forward(e, st)) return cr;   // (no chains_join: a sampling call in progress shares nothing with this step)
  e->fwd_done = false;
  e->fwd_params_live = true;
  if (int xs = split_status(e)) return xs;
  e->plan = plan_step(e, B);
  StepPlan& p = e->plan;
  if (p.path == StepPlan::SKINNY) {
    // narrow net (csrc/skinny_step.h): staging, all layers and the loss partial sums of 16 users' P, S, Q rows per work-group in
    // ONE launch; the tables B0tab = b0 + C0[t] come from the last step's tail (or are made now, after a parameter upload)
    int rc = e->WeP ? SDRM_OK : ensure_tables(e, st);   // (T <= 128: the forward makes its users' rows of the table itself)
    if (rc) return rc;
    SkStepArgs ka = sk_step_args(e, B);
    ka.x0 = x0;
    if (mode == SDRM_RNG_EXPLICIT) { ka.noise = rnd->noise; ka.t = rnd->t; ka.keep = rnd->keep; }
    ka.mode = mode; ka.seed_lo = (uint32_t)seed; ka.seed_hi = (uint32_t)(seed >> 32); ka.step = (uint32_t)step;
    ka.row0 = row0; ka.nd = nd;
    bool done4 = false;
    if (e->tune.skinny == 1) {   // 4 users per work-group (csrc/skinny_fwd4.h); 2: the 16-user forward
      ka.NP = 4 * ka.G;
      rc = launch_sk_fwd4(e, ka, st, &done4);
      if (rc) return rc;
    }
    if (!done4) {
      ka.NP = ka.G;
      rc = launch_sk_step(e, ka, 0, ka.G, st);
      if (rc) return rc;
    }
    p.loss_parts = ka.NP;
  } else if (p.path == StepPlan::ROW96 || p.path == StepPlan::ROW48) {
    // row-owned forward (rowchain.h; rows48.h: the same on 48-row work-groups, p.parts of them per row group): the step's tables,
    // then staging + every layer + the loss partial sums in ONE launch.  In front of the 48-row kernels the tables launch also
    // pulls the batch into L2 (their staging asks for a thread's x0 quads one after the other); the 96-row forward requests every
    // quad of a thread at once and is no faster behind the warm-up, so its tables launch goes without
    const bool warm = p.path == StepPlan::ROW48;
    int rc = emb_tables(e, st, warm ? x0 : nullptr, warm ? (size_t)B * e->L : 0);
    if (rc) return rc;
    rc = launch_row_forward(e, p, x0, row0, mode, rnd, seed, step, nd, st);
    if (rc) return rc;
    chains_train_row_owned(e);
  } else {
    const int MP = p.MP, n = e->T + 1;
    const int cfg = choose_cfg(e->tune, MP, e->tune.nt32_max_rows_train);   // one tile for every NT launch of the step
    PrepTrainArgs pa{};
    pa.x0 = x0;
    if (mode == SDRM_RNG_EXPLICIT) { pa.noise = rnd->noise; pa.t = rnd->t; pa.keep = rnd->keep; }
    pa.sqrt_ab = e->sched + 3 * n; pa.one_minus_ab = e->sched + 4 * n; pa.tembP = e->tembP;
    pa.U = e->U; pa.tdev = e->tdev;
    pa.B = B; pa.L = e->L; pa.LP = e->LP; pa.K0 = e->K0; pa.T = e->T; pa.MP = MP;
    pa.mode = mode; pa.seed_lo = (uint32_t)seed; pa.seed_hi = (uint32_t)(seed >> 32); pa.step = (uint32_t)step;
    pa.row0 = row0; pa.nd = nd;
    {
      // the step's tables ride on the staging launch: C0^T in the trailing columns of W0c (what the plain sdrm_forward multiplies its
      // one-hot(t) columns with) and B0tab = b0 + C0[t], which layer 0 below adds per row
      pa.emb = emb_args(e);
      e->tables_fresh = true;
      pa.emb_row0 = B + (MP - 3 * B);
      pa.emb_chunks = (e->WP + 63) / 64;
      pa.emb_blocks = (e->T + 1) * pa.emb_chunks;
      const int main_blocks = (int)(((int64_t)pa.emb_row0 * (e->K0 / 4) + 255) / 256);
      SDRM_LAUNCH(e, k_prep_train, dim3(pa.emb_blocks + main_blocks), dim3(256), 2 * e->T * sizeof(float), st, pa);
      HIP_TRY(e, hipGetLastError());
    }
    {
      // Layer 0 contracts over the latent columns only (K = LP instead of LP + TP: a fifth less work at ML-1M): every row's
      // time-embedding term is a row of B0tab, added in the epilogue.  The trailing columns of U carry temb[t_row] (round 4; before: a
      // one-hot(t)): the layer-0 weight gradient multiplies them to deliver M = dpre0^T * temb (csrc/tail.h).
      GemmArgs a{};
      a.C = pre_buf(e, 0); a.ldc = e->WP; a.bias = e->B0tab; a.ldtab = e->WP; a.trow = e->tdev; a.trow_B = B;
      HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_ROWTAB>(a, e->U, e->K0, e->W0c, e->K0, MP, e->WP, e->LP, st,
                                                         Prof{e, PC_FWD_L0, 2.0 * 3 * B * (double)e->W * e->L}, cfg)));   // K = the latents: the time-embedding term is a table row
    }
    int rc = hidden_forward(e, MP, 3 * B, st, cfg);
    if (rc) return rc;
    {
      GemmArgs a{};
      a.C = e->Y; a.ldc = e->LP; a.bias = e->boc; a.slopeA = slope_ptr(e, e->H);
      a.rows_valid = MP; a.cols_valid = e->LP;
      HIP_TRY(e, (gemm_forward<XF_PRELU, EPI_BIAS_TANH>(a, pre_buf(e, e->H), e->WP, e->Woc, e->WP, MP, e->LP, e->WP, st,
                                                        Prof{e, PC_FWD_OUT, 2.0 * 3 * B * (double)e->L * e->W}, cfg)));
    }
    LossArgs la{};
    la.Y = e->Y; la.x0 = x0; la.B = B; la.L = e->L; la.LP = e->LP; la.part = e->loss_part;
    SDRM_LAUNCH(e, k_loss_partials, dim3(LOSS_BLOCKS), dim3(1024), 0, st, la);
    HIP_TRY(e, hipGetLastError());
  }
  if (!fold_sums) {
    SDRM_LAUNCH(e, k_loss_sums, dim3(1), dim3(256), 0, st, (const double*)e->loss_part, p.loss_parts, (double)B * (double)e->L,
                       sums ? sums : e->sums);
    HIP_TRY(e, hipGetLastError());
  }
  e->fwd_x0 = x0; e->fwd_done = true;
  return SDRM_OK;
}

int sdrm_train_forward(sdrm_engine* e, const float* x0, int B, int64_t row0, int mode, const sdrm_train_randoms* rnd,
                       uint64_t seed, uint64_t step, float nd, double* sums, void* stream) {
  return train_forward_impl(e, x0, B, row0, mode, rnd, seed, step, nd, sums, stream, false);
}

// Backward in two calls, so that a data-parallel caller can all-reduce one gradient bucket while the other is
// still being computed.  `begin` runs the chain every other kernel waits for (loss seeds, the dgrads down to
// layer 0), then the layer-0 weight gradient, its slab reduction and the small, latency-bound embedding
// backward: when it returns, the FIRST bucket (flat[0, off_a0): emb_layer.*, dnn.0.weight/bias) is final in
// stream order.  `finish` runs the weight gradients of the upper layers - two thirds of the wgrad flops,
// nothing but Adam depends on them - and reduces the second bucket (slopes, hidden and output layer).
// (Forking the upper wgrads to a second stream so that they also overlap the embedding backward on ONE GPU was
// measured: the two cross-stream event waits cost more than the ~45 us they hide, 642 vs 627 us per step.)
namespace {

// loss seeds, the dgrad chain down to layer 0, and the layer-0 weight gradient (whose time-embedding columns deliver M, csrc/tail.h)
int backward_chain(sdrm_engine* e, const double* sums, float* loss, hipStream_t st, bool with_wgrad0, bool fold_sums) {
  const StepPlan& p = e->plan;
  const int B = p.B, MP = p.MP, H = e->H;
  e->bwd_strips = false;
  SeedArgs sa{};
  sa.sums = fold_sums ? nullptr : (sums ? sums : e->sums); sa.Y = e->Y; sa.x0 = e->fwd_x0; sa.dY = e->dY; sa.loss = loss;
  sa.B = B; sa.L = e->L; sa.LP = e->LP; sa.MP = MP; sa.grouped = p.order;
  sa.part = e->loss_part;
  sa.nblk = p.loss_parts;
  sa.count = (double)B * (double)e->L;
  // the row-owned chain (dgrad_rows.h) and the narrow nets' backward compute the seeds themselves; every other form launches k_loss_seed
  if (p.dgrad == StepPlan::TILES || p.dgrad == StepPlan::ROWS_PER_LAYER) {
    const int nslots = p.groups * p.users_per_group;
    const unsigned need = (unsigned)(((size_t)(nslots + (MP - 3 * nslots)) * (e->LP / 4) + 255) / 256);
    dim3 grid(std::min(need, 2048u));   // grid-stride beyond: see k_loss_seed
    SDRM_LAUNCH(e, k_loss_seed, grid, dim3(256), 0, st, sa);
    HIP_TRY(e, hipGetLastError());
  }
  int S0, kc0;
  pick_splits(e->tune, MP, wgrad_tiles(e->tune, e->WP, e->K0) + H * wgrad_tiles(e->tune, e->WP, e->WP) + wgrad_tiles(e->tune, e->LP, e->WP),
              S0, kc0);
  const int cfg_w = pick_cfg(e->tune);   // tile of every split-K launch of this backward (backward_wgrads reuses it)
  e->bwd_cfg_w = cfg_w;
  const double flO = 2.0 * 3 * B * (double)e->L * e->W, flH = 2.0 * 3 * B * (double)e->W * e->W;
  const double fl0 = 2.0 * 3 * B * (double)e->W * (e->L + e->T);
  e->bwd_hidden_apps = H;
  int dgrad_blocks = 0;   // work-groups of a dgrad launch: each leaves one slope partial per layer
  switch (p.dgrad) {
    case StepPlan::SKINNY_OWN: {
      // narrow net (csrc/skinny_step.h): the sums' fold, the loss value, the seeds, the whole dgrad chain AND every weight / bias /
      // slope gradient of a work-group's users in one launch; one slab set per work-group (the hidden layer's applications already
      // summed), at most S_MAX of them - a work-group then walks several groups of users
      SkStepArgs ka = sk_step_args(e, B);
      ka.NP = p.loss_parts;
      ka.x0 = e->fwd_x0; ka.sums = sa.sums; ka.count = sa.count; ka.loss = loss;
      const int S = std::min(ka.G, S_MAX);
      int rc = launch_sk_step(e, ka, 1, S, st);
      if (rc) return rc;
      e->bwd_S0 = e->bwd_SH = e->bwd_SO = S; e->bwd_hidden_apps = 1; e->bwd_dgrad_blocks = S;
      e->bwd_kc0 = e->bwd_kcH = e->bwd_kcO = 0;
      return SDRM_OK;
    }
    case StepPlan::CHAIN: {
      // one work-group per 96 stacked rows - or `parts` per 48 (csrc/rows48.h) - runs the whole chain: one slope partial per work-group and layer
      DgradChain48Args c8{};
      dgrad_chain_args(e, sa, c8.c);
      c8.pad_rows = MP - p.rows;
      dgrad_blocks = p.groups * p.parts;
      int rc = p.path == StepPlan::ROW48 ? launch_rows48_chain(e, c8, p.groups, p.parts, flO + H * flH, st)
                                         : launch_dgrad_chain(e, c8.c, p.groups, flO + H * flH, st);
      if (rc) return rc;
      break;
    }
    case StepPlan::ROWS_PER_LAYER: {
      // one work-group per 96 stacked rows (and layer): one slope partial per work-group
      dgrad_blocks = p.groups;
      int rc = launch_dgrad_rows(e, e->dY, e->WofT, pre_buf(e, H), slope_ptr(e, H), dpre_buf(e, H),
                                 e->alpha_part + (size_t)H * e->alpha_part_stride, p.groups, flO, st);
      for (int k = H; k >= 1 && !rc; --k)
        rc = launch_dgrad_rows(e, dpre_buf(e, k), e->WhfT, pre_buf(e, k - 1), slope_ptr(e, k - 1), dpre_buf(e, k - 1),
                               e->alpha_part + (size_t)(k - 1) * e->alpha_part_stride, p.groups, flH, st);
      if (rc) return rc;
      break;
    }
    case StepPlan::TILES: {
      // every dgrad writes [MP,WP]: one tile shape for all of them, so the slope partial counts agree
      const int cfg_d = choose_cfg(e->tune, MP, e->tune.nt32_max_rows_train);
      dgrad_blocks = ((MP + kCfgBM[cfg_d] - 1) / kCfgBM[cfg_d]) * ((e->WP + kCfgBN[cfg_d] - 1) / kCfgBN[cfg_d]);
      // dpre[k] = gradient w.r.t. pre-activation k (kept for the weight gradients that run later)
      HIP_TRY(e, gemm_dgrad(e, e->dY, e->LP, e->WocT, e->LP, MP, e->LP, e->WP, dpre_buf(e, H), pre_buf(e, H), slope_ptr(e, H),
                            e->alpha_part + (size_t)H * e->alpha_part_stride, st, flO, cfg_d));
      for (int k = H; k >= 1; --k)
        HIP_TRY(e, gemm_dgrad(e, dpre_buf(e, k), e->WP, e->WhcT, e->WP, MP, e->WP, e->WP, dpre_buf(e, k - 1), pre_buf(e, k - 1),
                              slope_ptr(e, k - 1), e->alpha_part + (size_t)(k - 1) * e->alpha_part_stride, st, flH, cfg_d));
      break;
    }
  }
  // layer 0 (no latent dgrad: XT.grad is never read, Q7)
  if (with_wgrad0)
    HIP_TRY(e, (gemm_wgrad<XF_NONE>(dpre_buf(e, 0), e->WP, e->WP, e->U, e->K0, e->K0, nullptr, MP, S0, kc0, e->slab0, e->db0s, st,
                                    Prof{e, PC_WGRAD_L0, fl0}, cfg_w)));
  // ONE slice count for every weight gradient of this backward (pick_splits)
  e->bwd_S0 = e->bwd_SH = e->bwd_SO = S0; e->bwd_kc0 = e->bwd_kcH = e->bwd_kcO = kc0;
  e->bwd_dgrad_blocks = dgrad_blocks;
  return SDRM_OK;
}

// weight gradients of the output and hidden layers (two thirds of the wgrad flops, only Adam waits for them), and, for
// the one-call backward, of layer 0 as well: ONE batched launch (gemm_batch_kernel) - every input is ready once the
// dgrad chain is done.  More problems than a batch holds (H > 6) go in several batches; a forced tile shape
// (SDRM_TILE) falls back to one launch per layer.
int backward_wgrads(sdrm_engine* e, hipStream_t st, bool with_wgrad0) {
  const StepPlan& p = e->plan;
  if (p.path == StepPlan::SKINNY) return SDRM_OK;   // the narrow nets' backward launch has left every weight gradient in its slabs
  const int B = p.B, MP = p.MP, H = e->H, SH = e->bwd_SH, SO = e->bwd_SO;
  const double flO = 2.0 * 3 * B * (double)e->L * e->W, flH = 2.0 * 3 * B * (double)e->W * e->W;
  const double fl0 = 2.0 * 3 * B * (double)e->W * (e->L + e->T);
  if (e->bwd_cfg_w > 0) {   // a forced tile other than the default: the batched kernel is built for the default only
    const int cfg_w = e->bwd_cfg_w;
    if (with_wgrad0)
      HIP_TRY(e, (gemm_wgrad<XF_NONE>(dpre_buf(e, 0), e->WP, e->WP, e->U, e->K0, e->K0, nullptr, MP, e->bwd_S0, e->bwd_kc0, e->slab0,
                                      e->db0s, st, Prof{e, PC_WGRAD_L0, fl0}, cfg_w)));
    HIP_TRY(e, (gemm_wgrad<XF_PRELU>(e->dY, e->LP, e->LP, pre_buf(e, H), e->WP, e->WP, slope_ptr(e, H), MP, SO, e->bwd_kcO,
                                     e->slabO, e->dbOs, st, Prof{e, PC_WGRAD, flO}, cfg_w)));
    for (int k = H; k >= 1; --k)
      HIP_TRY(e, (gemm_wgrad<XF_PRELU>(dpre_buf(e, k), e->WP, e->WP, pre_buf(e, k - 1), e->WP, e->WP, slope_ptr(e, k - 1), MP, SH,
                                       e->bwd_kcH, e->slabH + (size_t)(k - 1) * SH * e->WP * e->WP,
                                       e->dbHs + (size_t)(k - 1) * SH * e->WP, st, Prof{e, PC_WGRAD, flH}, cfg_w)));
    return SDRM_OK;
  }
  if (with_wgrad0 && p.strips_ok) return launch_wgrad_strips(e, fl0 + flO + H * flH, st);
  std::vector<WgradSpec> w;
  std::vector<double> fl;
  if (with_wgrad0) {
    w.push_back(WgradSpec{dpre_buf(e, 0), e->WP, e->WP, e->U, e->K0, e->K0, e->one_dev, e->bwd_S0, e->bwd_kc0, e->slab0, e->db0s});
    fl.push_back(fl0);
  }
  // operand of the upper layers' weight gradients: the stored pre-activation (PReLU on load), or the activation itself
  const bool plain = p.acts_stored;
  auto opnd = [&](int k) { return plain ? e->act + (size_t)k * e->MPmax * e->WP : pre_buf(e, k); };
  w.push_back(WgradSpec{e->dY, e->LP, e->LP, opnd(H), e->WP, e->WP, slope_ptr(e, H), SO, e->bwd_kcO, e->slabO, e->dbOs});
  fl.push_back(flO);
  for (int k = H; k >= 1; --k) {
    w.push_back(WgradSpec{dpre_buf(e, k), e->WP, e->WP, opnd(k - 1), e->WP, e->WP, slope_ptr(e, k - 1), SH, e->bwd_kcH,
                          e->slabH + (size_t)(k - 1) * SH * e->WP * e->WP, e->dbHs + (size_t)(k - 1) * SH * e->WP});
    fl.push_back(flH);
  }
  for (size_t lo = 0; lo < w.size(); lo += GEMM_BATCH_MAX) {
    const int n = (int)std::min<size_t>(GEMM_BATCH_MAX, w.size() - lo);
    double f = 0.0;
    for (int k = 0; k < n; ++k) f += fl[lo + k];
    HIP_TRY(e, launch_wgrad_batch(e, w.data() + lo, n, MP, st, Prof{e, PC_WGRAD, f}, plain));
  }
  return SDRM_OK;
}

enum { BUCKET_FIRST = 1, BUCKET_SECOND = 2, BUCKET_BOTH = 3 };

// The tail of a backward (csrc/tail.h): slabs -> flat gradient (written where the caller wants it, e.g. a DDP bucket - no copy
// afterwards), the embedding path's gradients from the time-embedding columns of the layer-0 slabs, and - `update` (the
// single-GPU step) - Adam straight from the sums with the re-pack of the compute copies: ONE launch for everything that needs
// only the slabs, a second for the embedding path (FIRST bucket: W0e and emb_layer.*, out of what the first launch left).
int backward_tail(sdrm_engine* e, float* gout, int which, bool update, float lr, hipStream_t st) {
  const int L = e->L, W = e->W, T = e->T, H = e->H;
  const int S0 = e->bwd_S0, SH = e->bwd_SH, SO = e->bwd_SO;
  const int bias_col = e->bwd_strips ? e->ones_col : -1;   // strip-owned weight gradients: the bias gradient is slab column ones_col
  TailArgs a{};
  int n = 0, blocks = 0;
  auto add = [&](int kind, int64_t off, int rows, int cols, int flat_ld, const float* src, int src_ld, size_t slab_stride, int nslabs,
                 int nblocks) -> TailJob& {
    TailJob& j = a.j[n];
    j.kind = kind; j.flat_off = off; j.rows = rows; j.cols = cols; j.flat_ld = flat_ld;
    j.src = src; j.src_ld = src_ld; j.slab_stride = slab_stride; j.nslabs = nslabs; j.inner = 1; j.nblocks = nblocks; j.lanes = 4;
    j.red = nullptr; j.red_ld = 0;
    j.dst = j.dstT = j.dstF = j.dstFT = nullptr; j.dst_ld = j.dstT_ld = 0; j.fnct = e->WP / 16; j.fklast = j.fklastT = -1;
    a.start[n++] = blocks;
    blocks += nblocks;
    return j;
  };
  // a weight's sub-tiles (csrc/tail.h): 16 x 16 with four lanes per column quad (each a quarter of the slabs) when there are more
  // than 32 slabs, 16 x 32 with two up to 32, 32 x 32 with one up to eight
  auto mat = [&](int64_t off, int rows, int cols, int flat_ld, const float* src, int src_ld, size_t slab_stride, int nslabs) -> TailJob& {
    const int lanes = nslabs > 32 ? 4 : (nslabs > 8 ? 2 : 1), tsr = lanes == 1 ? 32 : 16, tsc = lanes == 4 ? 16 : 32;
    TailJob& j = add(TJ_MAT, off, rows, cols, flat_ld, src, src_ld, slab_stride, nslabs, ((rows + tsr - 1) / tsr) * ((cols + tsc - 1) / tsc));
    j.lanes = lanes;
    return j;
  };
  auto vec = [&](int64_t off, int len, const float* col_src, int col_ld, size_t col_stride, const float* sum_src, size_t sum_stride, int nslabs,
                 float* dst) -> TailJob& {
    TailJob& j = bias_col >= 0 ? add(TJ_VEC, off, len, 1, 1, col_src + bias_col, col_ld, col_stride, nslabs, (len + 63) / 64)
                               : add(TJ_VEC, off, len, 1, 1, sum_src, 1, sum_stride, nslabs, (len + 63) / 64);   // 64 entries per work-group
    j.dst = dst;
    return j;
  };
  auto snap = [&](int64_t off, int rows, int cols, int flat_ld, float* dst, int dst_ld) {
    TailJob& j = add(TJ_SNAP, off, rows, cols, flat_ld, nullptr, 0, 0, 0, rows * ((cols + TAIL_THREADS * 8 - 1) / (TAIL_THREADS * 8)));   // pieces of 2048 elements of a row
    j.red = dst; j.red_ld = dst_ld;
  };
  if (which & BUCKET_FIRST) {
    {
      TailJob& j = mat(e->off_w0, W, L, L + T, e->slab0, e->K0, (size_t)e->WP * e->K0, S0);
      j.dst = e->W0c; j.dst_ld = e->K0; j.dstF = e->W0f; j.fklast = rc_light_klast(L, e->LP);
    }
    vec(e->off_b0, W, e->slab0, e->K0, (size_t)e->WP * e->K0, e->db0s, (size_t)e->WP, S0, e->b0c);
    // for the second launch: M = the time-embedding columns of the layer-0 slabs, summed; emb_layer.* and W0e as they are now
    {
      TailJob& j = mat(0, W, T, 0, e->slab0 + e->LP, e->K0, (size_t)e->WP * e->K0, S0);
      j.red = e->Mred; j.red_ld = e->TP;
    }
    snap(e->off_we, 1, T * T + T, 0, e->snap, 0);
    snap(e->off_w0 + L, W, T, L + T, e->snap + (size_t)T * T + T, T);
  }
  if (which & BUCKET_SECOND) {
    // PReLU slopes: per-work-group partials of the dgrad epilogues, [application][alpha_part_stride]
    {
      TailJob& j = add(TJ_SCALAR, e->off_a0, 1, 1, 1, e->alpha_part, 0, (size_t)e->alpha_part_stride, 1, 1);
      j.inner = e->bwd_dgrad_blocks;
    }
    if (H >= 1) {
      const int HS = e->bwd_hidden_apps * SH;   // slab sets of the shared hidden layer: one per application and K-slice, or per K-slice
      TailJob& j = mat(e->off_wh, W, W, W, e->slabH, e->WP, (size_t)e->WP * e->WP, HS);
      j.dst = e->Whc; j.dst_ld = e->WP; j.dstT = e->WhcT; j.dstT_ld = e->WP; j.dstF = e->Whf; j.dstFT = e->WhfT;
      j.fklast = j.fklastT = rc_light_klast(W, e->WP);
      vec(e->off_bh, W, e->slabH, e->WP, (size_t)e->WP * e->WP, e->dbHs, (size_t)e->WP, HS, e->bhc);
      TailJob& s = add(TJ_SCALAR, e->off_ah, 1, 1, 1, e->alpha_part + e->alpha_part_stride, 0, (size_t)e->alpha_part_stride, H, 1);
      s.inner = e->bwd_dgrad_blocks;
    }
    {
      TailJob& j = mat(e->off_wo, L, W, W, e->slabO, e->WP, (size_t)e->LP * e->WP, SO);
      j.dst = e->Woc; j.dst_ld = e->WP; j.dstT = e->WocT; j.dstT_ld = e->LP; j.dstF = e->Wof; j.dstFT = e->WofT;
      j.fklast = rc_light_klast(W, e->WP); j.fklastT = rc_light_klast(L, e->LP);
    }
    vec(e->off_bo, L, e->slabO, e->WP, (size_t)e->LP * e->WP, e->dbOs, (size_t)e->LP, SO, e->boc);
  }
  a.start[n] = blocks;
  a.n = n;
  a.p = e->p; a.m = e->m; a.v = e->v; a.g = gout;
  a.L = L; a.W = W; a.T = T; a.LP = e->LP; a.TP = e->TP;
  a.off_we = e->off_we; a.off_be = e->off_be; a.off_w0 = e->off_w0; a.off_b0 = e->off_b0;
  a.Mred = e->Mred; a.snap = e->snap; a.WeP = e->WeP; a.W0eP = e->W0eP; a.TPe = e->TPe;
  a.b1 = 0.9f; a.b2 = 0.999f; a.eps = 1e-8f; a.wd = 1e-4f; a.update = update ? 1 : 0;
  if (update) adam_scalars(e->adam_t, lr, 0.9, 0.999, a.step_size, a.bc2_sqrt);
  int per_lane = 0;   // most slabs any lane of a weight job sums
  for (int q = 0; q < n; ++q)
    if (a.j[q].kind == TJ_MAT) per_lane = std::max(per_lane, (a.j[q].nslabs + a.j[q].lanes - 1) / a.j[q].lanes);
  if (per_lane <= 8) SDRM_LAUNCH(e, k_tail<8>, dim3((unsigned)blocks), dim3(TAIL_THREADS), 0, st, a);
  else SDRM_LAUNCH(e, k_tail<16>, dim3((unsigned)blocks), dim3(TAIL_THREADS), 0, st, a);
  HIP_TRY(e, hipGetLastError());
  if (update) { e->tables_fresh = false; e->fwd_params_live = false; }
  if (which & BUCKET_FIRST) {
    const int eb = tail_emb_blocks_a(W, T) + tail_emb_blocks_b(T) + tail_emb_blocks_c(T);
    SDRM_LAUNCH(e, k_tail_emb, dim3((unsigned)eb), dim3(256), tail_emb_lds_floats(T, e->TP) * sizeof(float), st, a);
    HIP_TRY(e, hipGetLastError());
  }
  return SDRM_OK;
}

}  // namespace

int sdrm_train_backward_begin(sdrm_engine* e, const double* sums, float* grad, float* loss, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!e->fwd_done) return fail(e, SDRM_ERR_STATE, "sdrm_train_backward: no forward to back-propagate");
  hipStream_t st = (hipStream_t)stream;
  e->bwd_begun = false;
  float* gout = grad ? grad : e->g;
  e->grad_src = gout;
  int rc = backward_chain(e, sums, loss, st, true, false);
  if (!rc) rc = backward_tail(e, gout, BUCKET_FIRST, false, 0.f, st);
  if (rc) return rc;
  e->bwd_begun = true;
  return SDRM_OK;
}

int sdrm_train_backward_finish(sdrm_engine* e, float* grad, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!e->fwd_done || !e->bwd_begun) return fail(e, SDRM_ERR_STATE, "sdrm_train_backward_finish: sdrm_train_backward_begin not run");
  hipStream_t st = (hipStream_t)stream;
  float* gout = grad ? grad : e->g;
  if (gout != e->grad_src) return fail(e, SDRM_ERR_ARG, "sdrm_train_backward_finish: different gradient buffer than begin");
  int rc = backward_wgrads(e, st, false);
  if (!rc) rc = chains_wgrads_queued(e, st);
  if (!rc) rc = backward_tail(e, gout, BUCKET_SECOND, false, 0.f, st);
  e->bwd_begun = false;
  return rc;
}

// the whole backward in one call: same kernels, one tail for both buckets; `fused_lr` (the single-GPU step): Adam applied by the
// tail itself, straight from the slab sums (the flat gradient is still written: sdrm_get_grads)
// (Round 5 measured the single-GPU tail as two concurrent halves - the hidden / output layers' jobs on an auxiliary stream beside layer 0's
// jobs + k_tail_emb, optionally + the next step's k_emb_tables: the fork and the join cost more than the overlap gains on this runtime,
// train step 450.7 -> 467.3 / 457.4 us at B = 8192, 72.8 -> 98.9 at B = 160, ADM 47.2 -> 66.4: profiles/r05_tail_split.txt.)
static int train_backward_impl(sdrm_engine* e, const double* sums, float* grad, float* loss, hipStream_t st, const float* fused_lr,
                               bool fold_sums) {
  e->bwd_begun = false;
  float* gout = grad ? grad : e->g;
  e->grad_src = gout;
  int rc = backward_chain(e, sums, loss, st, false, fold_sums);
  if (!rc) rc = backward_wgrads(e, st, true);
  if (!rc) rc = chains_wgrads_queued(e, st);
  if (!rc) rc = backward_tail(e, gout, BUCKET_BOTH, fused_lr != nullptr, fused_lr ? *fused_lr : 0.f, st);
  return rc;
}

int sdrm_train_backward(sdrm_engine* e, const double* sums, float* grad, float* loss, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!e->fwd_done) return fail(e, SDRM_ERR_STATE, "sdrm_train_backward: no forward to back-propagate");
  return train_backward_impl(e, sums, grad, loss, (hipStream_t)stream, nullptr, false);
}

int sdrm_grad_buckets(const sdrm_engine* e, int64_t* first_off, int64_t* first_len, int64_t* second_off, int64_t* second_len) {
  if (!e || !first_off || !first_len || !second_off || !second_len) return SDRM_ERR_ARG;
  *first_off = 0; *first_len = e->off_a0;
  *second_off = e->off_a0; *second_len = e->P - e->off_a0;
  return SDRM_OK;
}

int sdrm_adam_step(sdrm_engine* e, const float* grad, float lr, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (int jr = chains_join(e, (hipStream_t)stream)) return jr;
  e->adam_t += 1;
  return launch_adam(e, grad, lr, 1, (hipStream_t)stream);
}

int sdrm_train_step(sdrm_engine* e, const float* x0, int B, float lr, int mode, const sdrm_train_randoms* rnd,
                    uint64_t seed, uint64_t step, float nd, float* loss, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  // one process, one GPU: nobody needs the five sums between the forward and the backward (fold_sums: the seed kernel folds the
  // loss partials itself) ...
  int rc = train_forward_impl(e, x0, B, 0, mode, rnd, seed, step, nd, nullptr, stream, true);
  if (rc) return rc;
  e->adam_t += 1;         // ... nor the flat gradient between the backward and Adam: the tail applies it (csrc/tail.h)
  rc = train_backward_impl(e, nullptr, nullptr, loss, (hipStream_t)stream, &lr, true);
  if (rc) e->adam_t -= 1;
  return rc;
}

// ---------------------------------------------------------------------------------------------
// The exchange step of the user-sharded train step, RCCL called from inside the library.
#define NCCL_TRY(e, api, call)                                                                  \
  do {                                                                                          \
    ncclResult_t _r = (call);                                                                   \
    if (_r != ncclSuccess) {                                                                    \
      (e)->err = std::string(#call) + ": " + (api)->GetErrorString(_r);                         \
      return SDRM_ERR_RCCL;                                                                     \
    }                                                                                           \
  } while (0)

int sdrm_comm_available(void) { return rccl_api(nullptr) != nullptr ? 1 : 0; }

int sdrm_comm_unique_id(void* id_host) {
  if (!id_host) return SDRM_ERR_ARG;
  const RcclApi* api = rccl_api(nullptr);
  if (!api) return SDRM_ERR_RCCL;
  static_assert(sizeof(ncclUniqueId) == SDRM_COMM_ID_BYTES, "ncclUniqueId size");
  ncclUniqueId id;
  if (api->GetUniqueId(&id) != ncclSuccess) return SDRM_ERR_RCCL;
  std::memcpy(id_host, &id, sizeof(id));
  return SDRM_OK;
}

namespace {
int exchange_streams(sdrm_engine* e, void* aux_stream) {
  Exchange& x = e->xch;
  if (aux_stream) { x.aux = (hipStream_t)aux_stream; x.aux_owned = false; }
  else { HIP_TRY(e, hipStreamCreateWithFlags(&x.aux, hipStreamNonBlocking)); x.aux_owned = true; }
  HIP_TRY(e, hipEventCreateWithFlags(&x.ev_bucket, hipEventDisableTiming));
  HIP_TRY(e, hipEventCreateWithFlags(&x.ev_done, hipEventDisableTiming));
  return SDRM_OK;
}
}  // namespace

int sdrm_comm_init_rank(sdrm_engine* e, int nranks, int rank, const void* id_host) {
  if (!e || !id_host || nranks < 1 || rank < 0 || rank >= nranks) return fail(e, SDRM_ERR_ARG, "sdrm_comm_init_rank: bad argument");
  if (e->xch.comm) return fail(e, SDRM_ERR_STATE, "sdrm_comm_init_rank: this engine already has a communicator");
  std::string why;
  const RcclApi* api = rccl_api(&why);
  if (!api) return fail(e, SDRM_ERR_RCCL, why);
  HIP_TRY(e, hipSetDevice(e->device));
  ncclUniqueId id;
  std::memcpy(&id, id_host, sizeof(id));
  ncclComm_t comm = nullptr;
  NCCL_TRY(e, api, api->CommInitRank(&comm, nranks, id, rank));
  e->xch.comm = comm; e->xch.comm_owned = true; e->xch.nranks = nranks; e->xch.rank = rank;
  return exchange_streams(e, nullptr);
}

int sdrm_allreduce_init(sdrm_engine* e, void* rccl_comm, void* aux_stream) {
  if (!e || !rccl_comm) return fail(e, SDRM_ERR_ARG, "sdrm_allreduce_init: null pointer");
  if (e->xch.comm) return fail(e, SDRM_ERR_STATE, "sdrm_allreduce_init: this engine already has a communicator");
  std::string why;
  const RcclApi* api = rccl_api(&why);
  if (!api) return fail(e, SDRM_ERR_RCCL, why);
  ncclComm_t comm = (ncclComm_t)rccl_comm;
  int n = 0, r = -1;
  NCCL_TRY(e, api, api->CommCount(comm, &n));
  NCCL_TRY(e, api, api->CommUserRank(comm, &r));
  e->xch.comm = comm; e->xch.comm_owned = false; e->xch.nranks = n; e->xch.rank = r;
  return exchange_streams(e, aux_stream);
}

int sdrm_comm_info(const sdrm_engine* e, int* nranks, int* rank) {
  if (!e) return SDRM_ERR_ARG;
  if (nranks) *nranks = e->xch.comm ? e->xch.nranks : 0;
  if (rank) *rank = e->xch.comm ? e->xch.rank : -1;
  return SDRM_OK;
}

void* sdrm_debug_comm_handle(const sdrm_engine* e) { return e ? (void*)e->xch.comm : nullptr; }

int sdrm_comm_destroy(sdrm_engine* e) {
  if (!e) return SDRM_ERR_ARG;
  Exchange& x = e->xch;
  if (!x.comm) return SDRM_OK;
  (void)hipSetDevice(e->device);
  (void)hipDeviceSynchronize();
  if (x.comm_owned)
    if (const RcclApi* api = rccl_api(nullptr)) (void)api->CommDestroy(x.comm);
  if (x.ev_bucket) (void)hipEventDestroy(x.ev_bucket);
  if (x.ev_done) (void)hipEventDestroy(x.ev_done);
  if (x.aux && x.aux_owned) (void)hipStreamDestroy(x.aux);
  x = Exchange{};
  return SDRM_OK;
}

// One user-sharded train step, exchange included (what a non-Python caller needs: sdrm_amd/parallel.py does the same
// with torch.distributed between the three phases).  Order on `stream` unless noted:
//   forwards + local loss sums -> all-reduce(5 doubles) -> loss seeds, dgrad chain, layer-0 weight gradient, first
//   bucket final -> [aux stream: all-reduce(first bucket)] beside the upper layers' weight gradients -> second bucket
//   final -> [aux: all-reduce(second bucket)] -> Adam.
// Every collective of the communicator is ordered against the next by stream dependencies, on every rank alike.
int sdrm_train_step_sharded(sdrm_engine* e, const float* x0, int B, int64_t row0, float lr, int mode,
                            const sdrm_train_randoms* rnd, uint64_t seed, uint64_t step, float nd, float* loss, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  Exchange& x = e->xch;
  if (!x.comm) return fail(e, SDRM_ERR_STATE, "sdrm_train_step_sharded: no communicator (sdrm_comm_init_rank / sdrm_allreduce_init)");
  const RcclApi* api = rccl_api(nullptr);
  if (!api) return fail(e, SDRM_ERR_RCCL, "librccl is gone");
  hipStream_t st = (hipStream_t)stream;
  int rc = sdrm_train_forward(e, x0, B, row0, mode, rnd, seed, step, nd, e->sums, stream);
  if (rc) return rc;
  NCCL_TRY(e, api, api->AllReduce(e->sums, e->sums, 5, ncclDouble, ncclSum, x.comm, st));
  // Default: ONE all-reduce of the whole gradient after the one-call backward (all weight gradients in one batched launch).
  // The two-bucket form below hides the first bucket's all-reduce behind the upper layers' weight gradients, but its event
  // hand-offs and split launches cost 36-45 us per step by themselves (one-rank communicator, where the collectives are
  // free: tools/exchange_probe.py, profiles/r02_exchange_probe.txt) - more than a 0.6 MB all-reduce between GPUs of one
  // node takes.  sdrm_debug_set_gradient_buckets(e, 2) / SDRM_AR_BUCKETS=2 selects it for nets whose gradient is large
  // enough for the overlap to pay.
  const int buckets = e->tune.ar_buckets == 2 ? 2 : 1;
  if (buckets == 1) {
    rc = sdrm_train_backward(e, e->sums, nullptr, loss, stream);
    if (rc) return rc;
    NCCL_TRY(e, api, api->AllReduce(e->g, e->g, (size_t)e->P, ncclFloat, ncclSum, x.comm, st));
    return sdrm_adam_step(e, nullptr, lr, stream);
  }
  rc = sdrm_train_backward_begin(e, e->sums, nullptr, loss, stream);
  if (rc) return rc;
  const int64_t n0 = e->off_a0, n1 = e->P - e->off_a0;
  HIP_TRY(e, hipEventRecord(x.ev_bucket, st));
  HIP_TRY(e, hipStreamWaitEvent(x.aux, x.ev_bucket, 0));
  NCCL_TRY(e, api, api->AllReduce(e->g, e->g, (size_t)n0, ncclFloat, ncclSum, x.comm, x.aux));
  rc = sdrm_train_backward_finish(e, nullptr, stream);
  if (rc) return rc;
  HIP_TRY(e, hipEventRecord(x.ev_bucket, st));
  HIP_TRY(e, hipStreamWaitEvent(x.aux, x.ev_bucket, 0));
  NCCL_TRY(e, api, api->AllReduce(e->g + n0, e->g + n0, (size_t)n1, ncclFloat, ncclSum, x.comm, x.aux));
  HIP_TRY(e, hipEventRecord(x.ev_done, x.aux));
  HIP_TRY(e, hipStreamWaitEvent(st, x.ev_done, 0));
  return sdrm_adam_step(e, nullptr, lr, stream);
}

int sdrm_get_train_outputs(const sdrm_engine* e, float* psq, void* stream) {
  if (!e || !psq) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  if (!e->fwd_done) return fail(me, SDRM_ERR_STATE, "sdrm_get_train_outputs: no forward yet");
  SDRM_LAUNCH(e, k_unpad_psq, dim3(256), dim3(256), 0, (hipStream_t)stream, (const float*)e->Y, e->plan.B, e->L,
                     e->LP, e->plan.order, psq);
  HIP_TRY(me, hipGetLastError());
  return SDRM_OK;
}

// test hook: the staged layer-0 inputs (the latent columns of U, in user order) and the timesteps of the last train forward
int sdrm_debug_get_staged(const sdrm_engine* e, float* staged, int* t, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  if (!e->fwd_done) return fail(me, SDRM_ERR_STATE, "sdrm_debug_get_staged: no forward yet");
  if (staged) {
    SDRM_LAUNCH(e, k_unpad_psq, dim3(256), dim3(256), 0, (hipStream_t)stream, (const float*)e->U, e->plan.B, e->L, e->K0, e->plan.order, staged);
    HIP_TRY(me, hipGetLastError());
  }
  if (t) HIP_TRY(me, hipMemcpyAsync(t, e->tdev, (size_t)e->plan.B * sizeof(int), hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
static int forward_rows(sdrm_engine* e, const float* x, const int64_t* t, int t_uniform, int n, int mode,
                        const uint8_t* keep, uint64_t seed, uint64_t step, int64_t row0, float* out, int ldout,
                        int cols_valid, hipStream_t st) {
  if (int jr = chains_join(e, st)) return jr;
  const int MP = round_up(n, BM);
  const int cfg = choose_cfg(e->tune, MP, e->tune.nt32_max_rows);
  PrepFwdArgs pa{};
  pa.x = x; pa.t = t; pa.t_uniform = t_uniform; pa.keep = keep; pa.U = e->U;
  pa.n = n; pa.L = e->L; pa.LP = e->LP; pa.K0 = e->K0; pa.T = e->T; pa.MP = MP;
  pa.mode = mode; pa.seed_lo = (uint32_t)seed; pa.seed_hi = (uint32_t)(seed >> 32); pa.step = (uint32_t)step;
  pa.row0 = row0;
  pa.bpr = (e->K0 / 2 + 255) / 256;
  dim3 grid((unsigned)((size_t)pa.bpr * MP));
  SDRM_LAUNCH(e, k_prep_forward, grid, dim3(256), 0, st, pa);
  HIP_TRY(e, hipGetLastError());
  int rc = ensure_tables(e, st);
  if (rc) return rc;
  {
    GemmArgs a{};
    a.C = pre_buf(e, 0); a.ldc = e->WP; a.bias = e->b0c;
    HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS>(a, e->U, e->K0, e->W0c, e->K0, MP, e->WP, e->K0, st,
                                                Prof{e, PC_FWD_L0, 2.0 * n * (double)e->W * (e->L + e->T)}, cfg)));
  }
  rc = hidden_forward(e, MP, n, st, cfg);
  if (rc) return rc;
  GemmArgs a{};
  a.C = out; a.ldc = ldout; a.bias = e->boc; a.slopeA = slope_ptr(e, e->H);
  a.rows_valid = n; a.cols_valid = cols_valid;
  HIP_TRY(e, (gemm_forward<XF_PRELU, EPI_BIAS_TANH_G>(a, pre_buf(e, e->H), e->WP, e->Woc, e->WP, MP, e->LP, e->WP, st,
                                                    Prof{e, PC_FWD_OUT, 2.0 * n * (double)e->L * e->W}, cfg)));
  return SDRM_OK;
}

int sdrm_forward(sdrm_engine* e, const float* x, const int64_t* t, int n, int mode, const uint8_t* keep, uint64_t seed,
                 uint64_t step, int64_t row0, float* out, void* stream) {
  if (!e || !x || !t || !out) return fail(e, SDRM_ERR_ARG, "sdrm_forward: null pointer");
  if (n < 1 || n > 3 * e->max_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_forward: n outside [1, 3*max_rows]");
  if (mode == SDRM_RNG_EXPLICIT && !keep) return fail(e, SDRM_ERR_ARG, "sdrm_forward: EXPLICIT mode needs keep");
  e->fwd_done = false;
  return forward_rows(e, x, t, 0, n, mode, keep, seed, step, row0, out, e->L, e->L, (hipStream_t)stream);
}

int sdrm_reverse_step(sdrm_engine* e, float* x, int n, int i, const float* z, const uint8_t* keep, void* stream) {
  if (!e || !x || !keep) return fail(e, SDRM_ERR_ARG, "sdrm_reverse_step: null pointer");
  if (n < 1 || n > 3 * e->max_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_reverse_step: n outside [1, 3*max_rows]");
  if (i < 1 || i > e->T) return fail(e, SDRM_ERR_ARG, "sdrm_reverse_step: step outside [1, T]");
  hipStream_t st = (hipStream_t)stream;
  e->fwd_done = false;
  int rc = forward_rows(e, x, nullptr, i, n, SDRM_RNG_EXPLICIT, keep, 0, 0, 0, e->Y, e->LP, e->LP, st);
  if (rc) return rc;
  float c1, sa, sb;
  reverse_coeffs(e, i, c1, sa, sb);
  SDRM_LAUNCH(e, k_reverse_apply, dim3(256), dim3(256), 0, st, x, (const float*)e->Y, e->LP, z, n, e->L, c1, sa, sb);
  HIP_TRY(e, hipGetLastError());
  return SDRM_OK;
}

int sdrm_perturb_input(sdrm_engine* e, const float* x, const int64_t* t, const float* noise, int n, float* out,
                       void* stream) {
  if (!e || !x || !t || !noise || !out || n < 1) return fail(e, SDRM_ERR_ARG, "sdrm_perturb_input: bad argument");
  const int nn = e->T + 1;
  SDRM_LAUNCH(e, k_perturb, dim3(256), dim3(256), 0, (hipStream_t)stream, x, t, noise,
                     (const float*)(e->sched + 3 * nn), (const float*)(e->sched + 4 * nn), n, e->L, e->T, out);
  HIP_TRY(e, hipGetLastError());
  return SDRM_OK;
}

namespace {
// The narrow-net sampler: ONE persistent launch runs the whole reverse loop (rows are independent across all timesteps).  It is
// issued by sdrm_sample_begin, on that call's stream, so the call reads the parameters as they are at its begin - the same
// contract as the snapshot of the per-layer path; sdrm_sample_steps is then only book-keeping for the resumable API.
int launch_skinny_sampler(sdrm_engine* e, const SampleCall& s, hipStream_t st) {
  SkinnyArgs ka{};
  ka.W0c = e->W0c; ka.K0 = e->K0; ka.Whc = e->Whc; ka.Woc = e->Woc; ka.bh = e->bhc; ka.bo = e->boc;
  ka.B0tab = e->B0tab; ka.slope0 = slope_ptr(e, 0); ka.slopeh = e->H > 0 ? slope_ptr(e, 1) : slope_ptr(e, 0);
  ka.rev = e->rev_dev; ka.xT = s.xT; ka.Z = s.z; ka.keep = s.keep;
  ka.Tj = s.multires ? e->Tj_dev : nullptr; ka.rowid = s.multires ? e->rowid_dev : nullptr;
  ka.out = e->X; ka.n = s.n; ka.L = e->L; ka.W = e->W; ka.T = e->T; ka.H = e->H;
  ka.mode = s.mode; ka.seed_lo = (uint32_t)s.seed; ka.seed_hi = (uint32_t)(s.seed >> 32);
  ka.call_id = (uint32_t)s.call_id; ka.row0 = s.row0; ka.nd = s.nd;
  ka.LPs = e->LP; ka.WPs = e->WP;
  return with_skinny_form(e, [&](auto nl, auto nw) {   // 16 rows per work-group, one wave per column tile
    SDRM_LAUNCH(e, (k_skinny_sample<VAL(nl), VAL(nw)>), dim3((s.n + 15) / 16), dim3(64 * std::max(VAL(nl), VAL(nw))), 0, st, ka);
    HIP_TRY(e, hipGetLastError());
    return SDRM_OK;
  });
}

// The other paths: the call's snapshot of the net (see sdrm_engine::smp_w: one launch for all of its pieces), the sampler state X and the first
// step's layer-0 input Us; the persistent sampler's counters start every call at zero (row tiles differ from call to call)
int launch_sample_init(sdrm_engine* e, const SampleCall& s, hipStream_t st) {
  float* b = e->smp_w;
  CopySegs cs{};
  auto seg = [&](int i, int k, const float* src, size_t n_, size_t extra = 0) {
    cs.src[i] = src; cs.dst[i] = b + e->smp_off[k] + extra; cs.n[i] = src ? (unsigned)n_ : 0u;
  };
  seg(0, 0, e->W0c, (size_t)e->WP * e->K0);
  seg(1, 1, e->H >= 1 ? e->Whc : nullptr, (size_t)e->WP * e->WP);
  seg(2, 2, e->Woc, (size_t)e->LP * e->WP);
  seg(3, 3, e->H >= 1 ? e->bhc : nullptr, (size_t)e->WP);
  seg(4, 4, e->boc, (size_t)e->LP);
  seg(5, 5, e->B0tab, (size_t)(e->T + 1) * e->WP);
  seg(6, 6, slope_ptr(e, 0), 1);
  seg(7, 6, e->H >= 1 ? slope_ptr(e, 1) : nullptr, 1, 1);
  SDRM_LAUNCH(e, k_copy_segments, dim3(64, 8), dim3(256), 0, st, cs);
  HIP_TRY(e, hipGetLastError());
  SampleInitArgs ia{};
  ia.xT = s.xT; ia.keep = s.keep; ia.Tj = s.multires ? e->Tj_dev : nullptr; ia.rowid = s.multires ? e->rowid_dev : nullptr;
  ia.X = e->X; ia.U = e->Us; ia.n = s.n; ia.L = e->L; ia.LP = e->LP; ia.K0 = e->LP; ia.MP = s.MP; ia.T = e->T;
  ia.mode = s.mode; ia.seed_lo = (uint32_t)s.seed; ia.seed_hi = (uint32_t)(s.seed >> 32);
  ia.call_id = (uint32_t)s.call_id; ia.row0 = s.row0;
  ia.bpr = (e->LP / 4 + 255) / 256;
  dim3 grid((unsigned)((size_t)ia.bpr * s.MP));
  SDRM_LAUNCH(e, k_sample_init, grid, dim3(256), 0, st, ia);
  HIP_TRY(e, hipGetLastError());
  if (e->xcntS) HIP_TRY(e, hipMemsetAsync(e->xcntS, 0, (size_t)256 * 32 * sizeof(unsigned), st));
  return SDRM_OK;
}

// Reverse steps in one launch (csrc/sample_persist.h): full resolution, PHILOX (the reverse update rides in the out layer's
// epilogue), a net whose layers share one tiling (L == W), one row chain, a forced tile only if it is the 32x32 one, the chip's
// block -> XCD mapping, and every work-group resident at once: 32x32 tiles, at most two per CU on the fullest XCD.
// by size: up to 11 row tiles of 32 (at most two row tiles = 22 work-groups per XCD: one per CU).  Measured (tools/sample_persist_probe.py,
// profiles/r05_sample_persist_probe.txt): n = 339: 12.1 us per step for a whole call in one launch against 16.5 for the three
// launches per step (15.7 driven one step per call); n = 679 - the 8-GPU shard: 22 row tiles put 33 work-groups on six XCDs' 32
// CUs, the doubled CU sets every phase - 16.0 against 16.4 (19.9 one step per call), n = 1024: 18.8 against 17.7: not taken there
// Asked once per call, by sdrm_sample_begin (the tile's and smp_persist's setters refuse inside one; fuse_rev as it is then): the abort word is persist_now's.
constexpr int SMP_PERSIST_MAX_ROWS = 352;
bool sample_persist_fits(const sdrm_engine* e, int n, int MP, int multires, int mode, int chains) {
  if (e->tune.smp_persist <= 0 || !e->xcd_ok || !e->xcntS || !e->xabort_host) return false;
  if (multires || mode != SDRM_RNG_PHILOX || e->LP != e->WP || chains != 1) return false;
  if (e->tune.force_cfg >= 0 && e->tune.force_cfg != 4) return false;
  if (e->tune.fuse_rev == 0) return false;   // (a caller who asked for the stand-alone reverse update gets the per-layer path)
  const int tiles_m = MP / 32, tiles_n = e->WP / 32;
  const int per_xcd = ((tiles_m + 7) / 8) * tiles_n;
  if (per_xcd > 64 || tiles_m > 256) return false;
  return e->tune.smp_persist >= 2 || n <= SMP_PERSIST_MAX_ROWS;
}
}  // namespace

int sdrm_sample_begin(sdrm_engine* e, int n, float nd, int multires, int mode, const float* xT, const float* z,
                      const uint8_t* keep, const int64_t* Tj, uint64_t seed, uint64_t call_id, int64_t row0,
                      int64_t* Tj_out, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  SampleCall& c = e->call;
  c.active = false;
  if (n < 1 || n > 3 * e->max_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_sample: n outside [1, 3*max_rows]");
  if (mode == SDRM_RNG_EXPLICIT && (!xT || !z || !keep || (multires && !Tj)))
    return fail(e, SDRM_ERR_ARG, "sdrm_sample: EXPLICIT mode needs xT, z, keep (and Tj for multi-resolution)");
  if (mode != SDRM_RNG_EXPLICIT && mode != SDRM_RNG_PHILOX) return fail(e, SDRM_ERR_ARG, "bad rng mode");
  if (multires && n > e->max_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_sample: multi-resolution n > max_rows");
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_begin(e, st)) return jr;
  const int T = e->T;
  e->fwd_done = false;
  int rc = ensure_tables(e, st);
  if (rc) return rc;
  int i_first = T;
  c.nact.assign(T + 2, n);                            // nact[i] = rows with Tj >= i (all rows when full resolution)
  if (multires) {
    // Start steps on the host: drawn with the same Philox call the device would make (PHILOX), or copied
    // back (EXPLICIT; one sync per sampling call).  Slots are then ordered by descending Tj.
    std::vector<int64_t> tj(n);
    if (mode == SDRM_RNG_PHILOX) {
      for (int r = 0; r < n; ++r) {
        const U4 w = philox4x32_10((uint32_t)(row0 + r), 0u, PURPOSE_SAMPLE_TJ, (uint32_t)call_id, (uint32_t)seed,
                                   (uint32_t)(seed >> 32));
        tj[r] = 1 + (int64_t)bounded(w.x, (uint32_t)(T - 1 > 1 ? T - 1 : 1));   // np.random.randint(1, T), :42
      }
    } else {
      HIP_TRY(e, hipMemcpyAsync(tj.data(), Tj, (size_t)n * 8, hipMemcpyDeviceToHost, st));
      HIP_TRY(e, hipStreamSynchronize(st));
      for (int r = 0; r < n; ++r) tj[r] = tj[r] < 0 ? 0 : (tj[r] > T ? T : tj[r]);
    }
    c.perm.resize(n);
    for (int r = 0; r < n; ++r) c.perm[r] = r;
    std::stable_sort(c.perm.begin(), c.perm.end(), [&](int a, int b) { return tj[a] > tj[b]; });
    c.tj_sorted.resize(n);
    for (int s = 0; s < n; ++s) c.tj_sorted[s] = tj[c.perm[s]];
    std::vector<int> hist(T + 2, 0);
    for (int r = 0; r < n; ++r) hist[(int)tj[r]]++;
    int acc = 0;
    for (int i = T; i >= 0; --i) { acc += hist[i]; c.nact[i] = acc; }
    i_first = (int)c.tj_sorted[0];
    HIP_TRY(e, hipMemcpyAsync(e->rowid_dev, c.perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(e, hipMemcpyAsync(e->Tj_dev, c.tj_sorted.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    if (Tj_out) {
      c.tj_orig = tj;
      HIP_TRY(e, hipMemcpyAsync(Tj_out, c.tj_orig.data(), (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
  }
  // the record of the call
  c.n = n; c.multires = multires; c.mode = mode; c.nd = nd;
  c.xT = xT; c.z = z; c.keep = keep;
  c.seed = seed; c.call_id = call_id; c.row0 = row0;
  c.MP = round_up(n, BM);
  const int chains = chains_for(e->tune, n, e->WP);
  c.chunk = round_up((n + chains - 1) / chains, BM);
  c.chains = (n + c.chunk - 1) / c.chunk;
  c.path = skinny_net(e) ? SampleCall::SKINNY
           : sample_persist_fits(e, n, c.MP, multires, mode, c.chains) ? SampleCall::PERSIST : SampleCall::PER_LAYER;
  c.i_next = i_first;
  c.persist_phase = 0;
  c.active = true;
  rc = c.path == SampleCall::SKINNY ? launch_skinny_sampler(e, c, st) : launch_sample_init(e, c, st);
  if (rc) c.active = false;
  return rc;
}

namespace {
// count reverse steps from i_next on, in one launch
int launch_sample_persist(sdrm_engine* e, SampleCall& s, int count, hipStream_t st) {
  const NetView nv = snapshot_view(e);
  const int MP = s.MP, tiles_m = MP / 32, tiles_n = e->WP / 32;
  SamplePersistArgs P{};
  auto layer = [&](GemmArgs& a, const float* A, int lda, const float* Wc, int ldw, float* C, int ldc, int K) {
    a.A = A; a.lda = lda; a.limA = MP; a.B = Wc; a.ldb = ldw; a.limB = e->WP; a.K = K; a.kchunk = K; a.C = C; a.ldc = ldc;
    return gemm_set_grid(a, tiles_m, tiles_n, 1);
  };
  bool ok = layer(P.l0, e->Us, e->LP, nv.W0c, e->K0, smp_buf(e, 0), e->WP, e->LP);
  P.l0.slopeE = nv.slope0;
  ok = ok && layer(P.lh, smp_buf(e, 0), e->WP, nv.Whc, e->WP, smp_buf(e, 1), e->WP, e->WP);
  P.lh.bias = nv.bhc; P.lh.slopeE = nv.slopeh;
  ok = ok && layer(P.lo, smp_buf(e, e->H), e->WP, nv.Woc, e->WP, e->smp_Y, e->LP, e->WP);
  if (!ok) return fail(e, SDRM_ERR_SHAPE, "persistent sampler: grid beyond the tile arithmetic");
  GemmArgs& a = P.lo;
  a.bias = nv.boc; a.rows_valid = MP; a.cols_valid = e->LP;
  a.revX = e->X; a.revU = e->Us; a.rev_ldx = e->LP; a.rev_s0 = 0; a.rev_n = s.n; a.rev_L = e->L; a.rev_nd = s.nd;
  a.rev_seed_lo = (uint32_t)s.seed; a.rev_seed_hi = (uint32_t)(s.seed >> 32); a.rev_call_id = (uint32_t)s.call_id; a.rev_row0 = s.row0;
  P.pre_stride = (size_t)e->MPmax * e->WP;
  P.B0tab = nv.B0tab; P.ldtab = e->WP; P.rev = e->rev_dev;
  P.T = e->T; P.H = e->H; P.i_first = s.i_next; P.count = count;
  P.row_tiles = tiles_m; P.tiles_n = tiles_n;
  P.cnt = e->xcntS; P.base = s.persist_phase * (uint32_t)tiles_n; P.abort_ = e->xabort_dev;
  const int steps = std::min(count, s.i_next);
  s.persist_phase += (uint32_t)(steps * (e->H + 2));
  const int grid = 8 * tiles_n * ((tiles_m + 7) / 8);
  const double flops = 2.0 * s.n * ((double)e->W * e->L + (double)e->H * e->W * e->W + (double)e->L * e->W) * steps;
  const int rc = hip_rc(e, "k_sample_persist", profiled(e, PC_SMP_PERSIST, flops, st, [&] {
    SDRM_LAUNCH(e, (k_sample_persist<Cfg4>), dim3((unsigned)grid), dim3(NTHREADS), 0, st, P);
    return hipGetLastError();
  }));
  if (rc) return rc;
  s.i_next -= steps;
  return SDRM_OK;
}

// Reverse step i of the rows [s0, s1) of one chain, on the chain's stream: layer 0, the hidden layers, the out layer, and the
// reverse update where it does not ride in the out layer's epilogue
int sample_chain_step(sdrm_engine* e, const SampleCall& s, const NetView& nv, int i, int s0, int s1, hipStream_t sc) {
  const int L = e->L, rows = s1 - s0, MP = round_up(rows, BM);
  const size_t nL = (size_t)s.n * L;
  const int cfg = choose_cfg(e->tune, MP, e->tune.nt32_max_rows);
  // the sampler keeps ACTIVATIONS in the layer buffers (EPI_BIAS_PRELU): no backward will ask for the pre-activations
  GemmArgs a0{};
  a0.C = smp_buf(e, 0) + (size_t)s0 * e->WP; a0.ldc = e->WP; a0.bias = nv.B0tab + (size_t)i * e->WP; a0.slopeE = nv.slope0;
  HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_PRELU>(a0, e->Us + (size_t)s0 * e->LP, e->LP, nv.W0c, e->K0, MP, e->WP, e->LP, sc,
                                                    Prof{e, PC_SMP_L0, 2.0 * rows * (double)e->W * e->L}, cfg)));
  int rc = hidden_forward(e, MP, rows, sc, cfg, s0, PC_SMP_HIDDEN, true, &nv);
  if (rc) return rc;
  float c1, sqrt_alpha, sqrt_beta;
  reverse_coeffs(e, i, c1, sqrt_alpha, sqrt_beta);
  // (round 5: multi-resolution steps too - their active prefix is a launch like any other, the epilogue keys Philox by the slot's
  // original row; EXPLICIT randoms keep the stand-alone kernel)
  const bool fused = s.mode == SDRM_RNG_PHILOX && (e->tune.fuse_rev == 2 || (e->tune.fuse_rev == 1 && rows <= FUSE_REV_MAX_ROWS));
  GemmArgs a{};
  a.C = e->smp_Y + (size_t)s0 * e->LP; a.ldc = e->LP; a.bias = nv.boc;
  a.rows_valid = MP; a.cols_valid = e->LP;
  const Prof pr{e, PC_SMP_OUT, 2.0 * rows * (double)e->L * e->W};
  if (fused) {
    // eps_hat never reaches memory: the epilogue applies denoise_add_noise to the sampler state and writes the
    // next step's dropped-out input (one launch less per reverse step)
    a.revX = e->X; a.revU = e->Us; a.rev_ldx = e->LP; a.rev_s0 = s0; a.rev_n = s1; a.rev_L = L; a.rev_step = i;
    a.rev_c1 = c1; a.rev_sqrt_alpha = sqrt_alpha; a.rev_sqrt_beta = sqrt_beta; a.rev_nd = s.nd;
    a.rev_seed_lo = (uint32_t)s.seed; a.rev_seed_hi = (uint32_t)(s.seed >> 32); a.rev_call_id = (uint32_t)s.call_id;
    a.rev_row0 = s.row0; a.rev_rowid = s.multires ? e->rowid_dev : nullptr;
    HIP_TRY(e, (gemm_forward<XF_NONE, EPI_TANH_REV>(a, smp_buf(e, e->H) + (size_t)s0 * e->WP, e->WP, nv.Woc, e->WP, MP, e->LP, e->WP, sc, pr, cfg)));
    return SDRM_OK;
  }
  HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_TANH>(a, smp_buf(e, e->H) + (size_t)s0 * e->WP, e->WP, nv.Woc, e->WP, MP, e->LP, e->WP, sc, pr, cfg)));
  ReverseArgs ra{};
  ra.X = e->X; ra.Y = e->smp_Y; ra.U = e->Us;
  ra.Z = (s.mode == SDRM_RNG_EXPLICIT && i > 1) ? s.z + (size_t)i * nL : nullptr;
  ra.keep_next = (s.mode == SDRM_RNG_EXPLICIT && i > 1) ? s.keep + (size_t)(i - 1) * nL : nullptr;
  ra.Tj = s.multires ? e->Tj_dev : nullptr;
  ra.rowid = s.multires ? e->rowid_dev : nullptr;
  ra.s0 = s0; ra.n = s1; ra.L = L; ra.LP = e->LP; ra.K0 = e->LP; ra.step_i = i; ra.nd = s.nd;
  ra.c1 = c1; ra.sqrt_alpha = sqrt_alpha; ra.sqrt_beta = sqrt_beta;
  ra.mode = s.mode; ra.seed_lo = (uint32_t)s.seed; ra.seed_hi = (uint32_t)(s.seed >> 32);
  ra.call_id = (uint32_t)s.call_id; ra.row0 = s.row0;
  ra.bpr = ((L + 3) / 4 + 255) / 256;
  ra.rpb = std::max(1, 256 / ((L + 3) / 4));
  const unsigned rev_grid = ra.rpb > 1 ? (unsigned)((rows + ra.rpb - 1) / ra.rpb) : (unsigned)((size_t)ra.bpr * rows);
  SDRM_LAUNCH(e, k_reverse_update, dim3(rev_grid), dim3(256), 0, sc, ra);
  HIP_TRY(e, hipGetLastError());
  return SDRM_OK;
}
}  // namespace

int sdrm_sample_steps(sdrm_engine* e, int count, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  SampleCall& s = e->call;
  if (!s.active) return fail(e, SDRM_ERR_STATE, "sdrm_sample_steps: no sampling call in progress");
  hipStream_t st = (hipStream_t)stream;
  if (s.path == SampleCall::SKINNY) {
    // (launch_skinny_sampler ran the whole loop: the step counter is only book-keeping for the resumable API)
    s.i_next = s.i_next > count ? s.i_next - count : 0;
    return SDRM_OK;
  }
  // A train forward that was waiting for its backward is dropped (the documented rule of the two-call train API).  Whole train steps may
  // run between sdrm_sample_steps calls (bench.py interleaves them): the call reads its own snapshot of the net and has layer buffers of
  // its own - smp_pre, smp_Y - so they change nothing of it.
  e->fwd_done = false;
  e->bwd_begun = false;
  if (count > 0 && s.i_next >= 1 && persist_now(e)) return launch_sample_persist(e, s, count, st);
  hipStream_t on[4];
  if (int cr = chains_streams(e, st, on)) return cr;
  const NetView nv = snapshot_view(e);
  for (int done = 0; done < count && s.i_next >= 1; ++done, --s.i_next) {
    const int i = s.i_next;
    const int na = s.nact[i];                      // active prefix at this step
    for (int c = 0; c < s.chains; ++c) {
      const int s0 = c * s.chunk, s1 = std::min(na, s0 + s.chunk);
      if (s1 <= s0) break;
      if (int rc = sample_chain_step(e, s, nv, i, s0, s1, on[c])) return rc;
    }
  }
  return SDRM_OK;
}

int sdrm_sample_remaining(const sdrm_engine* e) { return (e && e->call.active) ? e->call.i_next : 0; }

int sdrm_sample_end(sdrm_engine* e, float* out, void* stream) {
  if (!e || !out) return SDRM_ERR_ARG;
  if (!e->call.active) return fail(e, SDRM_ERR_STATE, "sdrm_sample_end: no sampling call in progress");
  if (e->call.i_next >= 1) return fail(e, SDRM_ERR_STATE, "sdrm_sample_end: reverse steps still pending");
  if (int jr = chains_join(e, (hipStream_t)stream)) return jr;
  if (xabort_read(e) != 0u) {   // a hand-shake of the persistent sampler (or of a split train step) timed out
    *(volatile unsigned*)e->xabort_host = 0u;
    e->tune.smp_persist = 0; e->tune.split = 0; e->xgeoF = e->xgeoC = 0;
    e->call.active = false;
    return fail(e, SDRM_ERR_HIP, "a launch that synchronises work-groups through an XCD's L2 (csrc/sample_persist.h, csrc/rows48.h) timed out: "
                                 "the sampling call's result is invalid; those paths are switched off for this handle");
  }
  if (e->call.path == SampleCall::SKINNY)   // the persistent kernel wrote dense [n,L] rows in original order
    HIP_TRY(e, hipMemcpyAsync(out, e->X, (size_t)e->call.n * e->L * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  else
    SDRM_LAUNCH(e, k_unpad_rows, dim3((unsigned)std::min<size_t>(4096, ((size_t)e->call.n * e->L + 255) / 256)), dim3(256), 0,
                (hipStream_t)stream, (const float*)e->X, e->LP, out, e->call.n, e->L,
                (const int*)(e->call.multires ? e->rowid_dev : nullptr));
  HIP_TRY(e, hipGetLastError());
  e->call.active = false;
  return SDRM_OK;
}

int sdrm_sample(sdrm_engine* e, int n, float nd, int multires, int mode, const float* xT, const float* z,
                const uint8_t* keep, const int64_t* Tj, uint64_t seed, uint64_t call_id, int64_t row0, float* out,
                int64_t* Tj_out, void* stream) {
  if (!e || !out) return fail(e, SDRM_ERR_ARG, "sdrm_sample: null pointer");
  int rc = sdrm_sample_begin(e, n, nd, multires, mode, xT, z, keep, Tj, seed, call_id, row0, Tj_out, stream);
  if (rc) return rc;
  rc = sdrm_sample_steps(e, e->T + 1, stream);
  if (rc) return rc;
  return sdrm_sample_end(e, out, stream);
}

int sdrm_get_preacts(const sdrm_engine* e, int layer, float* out, void* stream) {
  if (!e || !out) return SDRM_ERR_ARG;
  sdrm_engine* me = const_cast<sdrm_engine*>(e);
  if (!e->fwd_done) return fail(me, SDRM_ERR_STATE, "sdrm_get_preacts: no train forward yet");
  if (layer < 0 || layer > e->H) return fail(me, SDRM_ERR_ARG, "sdrm_get_preacts: layer outside [0,H]");
  // A forward that skipped the stores (skip_pre) left activations only: k_unpad_pre rebuilds v = h / slope and picks `act` or `pre` by the
  // slope AS IT IS NOW.  Once Adam (sdrm_adam_step, the fused tail of sdrm_train_step) or sdrm_set_params has moved the slopes that is
  // another number, or a buffer the forward never wrote: the forward's pre-activations are gone.
  if (!e->fwd_params_live)
    return fail(me, SDRM_ERR_STATE, "sdrm_get_preacts: the parameters have changed since the train forward (Adam step or sdrm_set_params): "
                                    "its pre-activations are gone");
  const float* actl = (e->plan.skip_pre() && e->act) ? e->act + (size_t)layer * e->MPmax * e->WP : nullptr;
  SDRM_LAUNCH(e, k_unpad_pre, dim3(256), dim3(256), 0, (hipStream_t)stream, (const float*)pre_buf(me, layer), actl,
                     (const float*)slope_ptr(me, layer), e->plan.B, e->W, e->WP, e->plan.order, out);
  HIP_TRY(me, hipGetLastError());
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// Sparse batch feed (dataloaders.py:46-79, train_SDRM.py:323), csrc/feed.h.
int sdrm_csr_rows_to_dense(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows,
                           const int64_t* rows, int64_t row0, int b, int n_items, float* out, void* stream) {
  if (!e || !out) return fail(e, SDRM_ERR_ARG, "sdrm_csr_rows_to_dense: null pointer");
  FeedArgs a{};
  if (int rc = csr_batch(e, "sdrm_csr_rows_to_dense", indptr, indices, data, n_rows, rows, row0, b, n_items, &a.csr)) return rc;
  a.out = out;
  return launch_k(e, PC_NONE, "k_csr_rows_to_dense", k_csr_rows_to_dense, dim3(b), dim3(256), 0, (hipStream_t)stream, a);
}

// what the feed launches since the last call found (synchronises `stream`), and clears it
int sdrm_feed_status(sdrm_engine* e, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  unsigned flag = 0;
  HIP_TRY(e, hipMemcpyAsync(&flag, e->feed_flag, sizeof(flag), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
  if (!flag) return SDRM_OK;
  HIP_TRY(e, hipMemsetAsync(e->feed_flag, 0, sizeof(flag), (hipStream_t)stream));
  std::string msg = "the CSR feed met";
  for (const FeedStatusText& t : FEED_STATUS_TEXT)
    if (flag & t.bit) msg += t.text;
  return fail(e, SDRM_ERR_ARG, msg);
}

// ---------------------------------------------------------------------------------------------
// Equal-sparsity binarisation of sampled data (main.py:177-180), csrc/select.h.
namespace {

// np.quantile(a, q) for float32 `a` and a Python-float q (numpy 2.x: q and the virtual index take a's dtype):
//   virtual = float32(n-1) * float32(q); previous = floor(virtual); next = previous + 1; gamma = virtual - previous
// (volatile: every operation rounds to float32, no contraction)
void quantile_ranks(int64_t n, double q, int64_t& r0, int64_t& r1, float& gamma) {
  volatile float q32 = (float)q;
  volatile float nm1 = (float)(n - 1);
  volatile float virt = nm1 * q32;
  if (virt >= nm1) { r0 = r1 = n - 1; gamma = 0.f; }
  else if (virt < 0.f) { r0 = r1 = 0; gamma = 0.f; }
  else {
    const float prev = std::floor(virt);
    volatile float g = virt - prev;
    gamma = g;
    r0 = (int64_t)prev; r1 = r0 + 1;
    if (r0 > n - 1) r0 = n - 1;
    if (r1 > n - 1) r1 = n - 1;
  }
}

// The three select sweeps, then the threshold and the binarise sweep.
int select_and_binarize(sdrm_engine* e, const float* x, int64_t n, float gamma, uint8_t* out, float* threshold, hipStream_t st) {
  const int blocks = (int)std::min<int64_t>(2048, (n / 4 + 255) / 256 + 1);
  for (int pass = 0; pass < SEL_PASSES; ++pass) {
    if (int rc = launch_k(e, PC_NONE, "k_select_hist", pass == 0 ? k_select_hist<4> : k_select_hist<1>, dim3(blocks), dim3(256), 0, st, x, n, e->sel, pass))
      return rc;
    if (int rc = launch_k(e, PC_NONE, "k_select_pick", k_select_pick, dim3(1), dim3(256), 0, st, e->sel, pass, gamma)) return rc;
  }
  if (threshold) HIP_TRY(e, hipMemcpyAsync(threshold, &e->sel->threshold, 4, hipMemcpyDeviceToDevice, st));
  if (out) return launch_k(e, PC_NONE, "k_binarize_ge", k_binarize_ge, dim3(blocks), dim3(256), 0, st, x, n, &e->sel->threshold, out);
  return SDRM_OK;
}

// The VAE-shaped entry points' limits, the same for every one of them (ENC_GATHER_MAX_Q and EVAL_MAX_ITEMS below are limits of their own)
constexpr int VAE_MAX_HIDDEN = 4096, VAE_MAX_LATENT = 4096;   // (hidden: ENC_GATHER_MAX_Q float4 slices in the gather kernels' registers)
constexpr int MAX_ITEMS = 1 << 20, MAX_BATCH_ROWS = 1 << 22;

// The padded extents of a VAE-shaped call, by three rules: K and N of the GEMMs go to 32 (Hp, Lp, L2p, Ip; Kb: the batch as the K of a
// weight gradient); the rows of an operand go to the largest tile, 128 (Hr, Lr, L2r, Ir; MP: the batch where it is a buffer's rows); the
// batch as a launch's M goes to the default tile, 64 (rows64).  Hq is `hidden` on the float4 grid of the gather kernels; L2 = 2 latent,
// the encoder's mu | logvar.  An extent that a call does not have goes in as 0.
struct VaeDims { int Hq, Hp, Hr, Lp, Lr, L2, L2p, L2r, Ip, Ir, MP, rows64, Kb; };
VaeDims vae_dims(int n_items, int hidden, int latent, int b) {
  VaeDims d;
  d.Hq = round_up(hidden, 4); d.Hp = round_up(hidden, 32); d.Hr = round_up(d.Hp, 128);
  d.Lp = round_up(latent, 32); d.Lr = round_up(d.Lp, 128);
  d.L2 = 2 * latent; d.L2p = round_up(d.L2, 32); d.L2r = round_up(d.L2p, 128);
  d.Ip = round_up(n_items, 32); d.Ir = round_up(d.Ip, 128);
  d.MP = round_up(b, 128); d.rows64 = round_up(b, BM); d.Kb = round_up(b, 32);
  return d;
}

// Split-K plan of a weight gradient over Kb batch rows, in slabs of at most `chunk` rows
struct SplitK { int kchunk, S; };
SplitK split_k(int Kb, int chunk) {
  const int kc = std::min(Kb, chunk);
  return SplitK{kc, (Kb + kc - 1) / kc};
}

// The segments of ONE k_pad2d launch: src [rows, cols] -> dst [rowsP, colsP], zero-padded
struct PadList {
  PadSegs sg{};
  int64_t most = 0;
  int k = 0;
  void add(const float* src, int rows, int cols, float* dst, int rowsP, int colsP) {
    sg.src[k] = src; sg.dst[k] = dst; sg.rows[k] = rows; sg.cols[k] = cols; sg.rowsP[k] = rowsP; sg.colsP[k] = colsP;
    most = std::max<int64_t>(most, (int64_t)rowsP * (colsP / 4));
    ++k;
  }
  int launch(sdrm_engine* e, LaunchClass lc, hipStream_t st) const {   // (no lower bound of 1 on the grid: a list is never empty)
    return launch_k(e, lc, "k_pad2d", k_pad2d, dim3((unsigned)std::min<int64_t>(2048, (most + 255) / 256), (unsigned)k), dim3(256), 0, st, sg);
  }
};

// decoder(z) = Linear(hidden, items)(tanh(Linear(latent, hidden)(z)))   (train_SDRM.py:212-214, :252-254): one staging launch, two GEMMs
int decode_launches(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, int n, float* out, hipStream_t st) {
  const VaeDims d = vae_dims(dec->n_items, dec->hidden, dec->latent, n);
  float *zp, *w1p, *b1p, *hid, *w2p, *b2p;
  int rc;
  if ((rc = scratch(e, SCR_DEC_Z, (size_t)d.MP * d.Lp, &zp)) || (rc = scratch(e, SCR_DEC_W1, (size_t)d.Hr * d.Lp, &w1p)) ||
      (rc = scratch(e, SCR_DEC_B1, d.Hr, &b1p)) || (rc = scratch(e, SCR_DEC_HID, (size_t)d.MP * d.Hp, &hid)) ||
      (rc = scratch(e, SCR_DEC_W2, (size_t)d.Ir * d.Hp, &w2p)) || (rc = scratch(e, SCR_DEC_B2, d.Ir, &b2p)))
    return rc;
  PadList pad;
  pad.add(z, n, dec->latent, zp, d.MP, d.Lp);
  pad.add(dec->w1, dec->hidden, dec->latent, w1p, d.Hr, d.Lp);
  pad.add(dec->b1, 1, dec->hidden, b1p, 1, d.Hr);
  pad.add(dec->w2, dec->n_items, dec->hidden, w2p, d.Ir, d.Hp);
  pad.add(dec->b2, 1, dec->n_items, b2p, 1, d.Ir);
  if ((rc = pad.launch(e, PC_NONE, st))) return rc;
  const int cfg = choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows);
  {
    GemmArgs a{};
    a.C = hid; a.ldc = d.Hp; a.bias = b1p;
    HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_TANH>(a, zp, d.Lp, w1p, d.Lp, d.rows64, d.Hp, d.Lp, st, Prof{nullptr, 0, 0.0}, cfg)));
  }
  GemmArgs a{};
  a.C = out; a.ldc = dec->n_items; a.bias = b2p;
  a.rows_valid = n; a.cols_valid = dec->n_items;
  HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_G>(a, hid, d.Hp, w2p, d.Hp, d.rows64, d.Ip, d.Hp, st, Prof{nullptr, 0, 0.0}, cfg)));
  return SDRM_OK;
}

// the four tensors of a decoder / an encoder are there (bwd: the backward reads no bias)
bool dec_tensors(const sdrm_vae_decoder* d, bool biases = true) { return d && d->w1 && d->w2 && (!biases || (d->b1 && d->b2)); }
bool enc_tensors(const sdrm_vae_encoder* d) { return d && d->w1 && d->b1 && d->w2 && d->b2; }

int check_decoder(sdrm_engine* e, const sdrm_vae_decoder* d, const float* z, int n, const char* who) {
  if (!e || !dec_tensors(d) || !z) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (n < 1 || n > MAX_BATCH_ROWS || d->latent < 1 || d->latent > VAE_MAX_LATENT || d->hidden < 1 || d->hidden > 16384 || d->n_items < 1 ||
      d->n_items > MAX_ITEMS)
    return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": n, latent, hidden or n_items outside the supported envelope");
  return SDRM_OK;
}

}  // namespace

int sdrm_vae_decode(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, int n, float* out, void* stream) {
  if (int rc = check_decoder(e, dec, z, n, "sdrm_vae_decode")) return rc;
  if (!out) return fail(e, SDRM_ERR_ARG, "sdrm_vae_decode: null output");
  if (int jr = chains_join(e, (hipStream_t)stream)) return jr;
  return decode_launches(e, dec, z, n, out, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------
// VAE encode hook, frozen and in eval mode (train_SDRM.py:241-250, called at :323), csrc/encode.h.
namespace {

constexpr int KL_PARTS = 512;    // work-groups of k_encode_kl_rows / k_latent_reparam: the float64 partials k_encode_kl_sum adds
constexpr int ENC_GATHER_MAX_Q = 1024;   // float4 slices of the hidden vector k_encode_csr holds in registers (256 threads x 4): hidden <= 4096

// The second Linear on the hidden activations SCR_ENC_HID [rows64][Hp], and the kl.  kl null: only the mu rows of W2, straight into z.
int encode_tail(sdrm_engine* e, int n, float* z, float* kl, hipStream_t st) {
  const VaeDims d = vae_dims(e->enc_items, e->enc_hidden, e->enc_latent, n);
  const int L = e->enc_latent;
  const int cfg = choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows);
  const float *hid = scratch_at(e, SCR_ENC_HID), *w2 = scratch_at(e, SCR_ENC_W2);
  GemmArgs a{};
  a.bias = scratch_at(e, SCR_ENC_B2);
  a.rows_valid = n;
  if (!kl) {
    a.C = z; a.ldc = L; a.cols_valid = L;
    HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_G>(a, hid, d.Hp, w2, d.Hp, d.rows64, d.Lp, d.Hp, st, Prof{nullptr, 0, 0.0}, cfg)));
    return SDRM_OK;
  }
  float* out2;
  if (int rc = scratch(e, SCR_ENC_OUT2, (size_t)n * d.L2, &out2)) return rc;
  a.C = out2; a.ldc = d.L2; a.cols_valid = d.L2;
  HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_G>(a, hid, d.Hp, w2, d.Hp, d.rows64, d.L2p, d.Hp, st, Prof{nullptr, 0, 0.0}, cfg)));
  const int parts = std::min(n, KL_PARTS);
  double* part = scratch_at<double>(e, SCR_ENC_PART);
  if (int rc = launch_k(e, PC_NONE, "k_encode_kl_rows", k_encode_kl_rows, dim3(parts), dim3(256), 0, st, out2, n, L, z, part)) return rc;
  return launch_k(e, PC_NONE, "k_encode_kl_sum", k_encode_kl_sum, dim3(1), dim3(256), 0, st, part, parts, n, kl);
}

// x [n, n_items] dense -> z (, kl): normalise + pad, Linear + tanh, tail
int encode_dense_launches(sdrm_engine* e, const float* x, int n, float* z, float* kl, hipStream_t st) {
  const VaeDims d = vae_dims(e->enc_items, e->enc_hidden, e->enc_latent, n);
  float *xn, *hid;
  int rc;
  if ((rc = scratch(e, SCR_ENC_XN, (size_t)d.MP * d.Ip, &xn)) || (rc = scratch(e, SCR_ENC_HID, (size_t)d.MP * d.Hp, &hid))) return rc;
  if ((rc = launch_k(e, PC_NONE, "k_encode_norm_rows", k_encode_norm_rows, dim3(n), dim3(256), 0, st, x, e->enc_items, xn, d.Ip))) return rc;
  GemmArgs a{};
  a.C = hid; a.ldc = d.Hp; a.bias = scratch_at(e, SCR_ENC_B1);
  HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_TANH>(a, xn, d.Ip, scratch_at(e, SCR_ENC_W1), d.Ip, d.rows64, d.Hp, d.Ip, st, Prof{nullptr, 0, 0.0},
                                                   choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows))));
  return encode_tail(e, n, z, kl, st);
}

// One launch of a row-owned gather kernel (csrc/csr_batch.h) over the rows of a batch.  The gather shape goes by the q float4 slices
// of the hidden vector alone: TPR threads own a row, NV slices each, U entries in flight.  kernel_of(TPR, NV, U) names the kernel.
extern "C++" template <class Args, class KernelOf>
int launch_gather_rows(sdrm_engine* e, LaunchClass lc, const char* name, int q, const Args& a, hipStream_t st, KernelOf&& kernel_of) {
  const auto go = [&](auto tpr, auto nv, auto u) {
    constexpr int rpw = 256 / VAL(tpr);
    return launch_k(e, lc, name, kernel_of(tpr, nv, u), dim3((unsigned)((a.csr.b + rpw - 1) / rpw)), dim3(256), 0, st, a);
  };
  using std::integral_constant;
  if (q <= 64) return go(integral_constant<int, 64>{}, integral_constant<int, 1>{}, integral_constant<int, 8>{});   // one wave per row, four rows per work-group (ADM: hidden 200)
  if (q <= 256) return go(integral_constant<int, 256>{}, integral_constant<int, 1>{}, integral_constant<int, 8>{});   // one work-group per row (ML-1M 600, ML-100k 930)
  if (q <= 512) return go(integral_constant<int, 256>{}, integral_constant<int, 2>{}, integral_constant<int, 4>{});
  return go(integral_constant<int, 256>{}, integral_constant<int, 4>{}, integral_constant<int, 2>{});
}

int check_encoder(sdrm_engine* e, const sdrm_vae_encoder* d, const char* who) {
  if (!e) return SDRM_ERR_ARG;
  if (!enc_tensors(d)) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (d->latent < 1 || d->latent > VAE_MAX_LATENT || d->hidden < 1 || d->hidden > 16384 || d->n_items < 1 || d->n_items > MAX_ITEMS)
    return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": latent, hidden or n_items outside the supported envelope");
  return SDRM_OK;
}

// W1 [hidden][items] -> W1^T [items][Hq], the gather kernels' operand
int launch_w1t(sdrm_engine* e, LaunchClass lc, const float* w1, int hidden, int n_items, float* w1t, int Hq, hipStream_t st) {
  return launch_k(e, lc, "k_encode_w1t", k_encode_w1t, dim3((unsigned)((n_items + 31) / 32), (unsigned)((Hq + 31) / 32)), dim3(256), 0, st, w1,
                  hidden, n_items, w1t, Hq);
}

}  // namespace

int sdrm_vae_encoder_load(sdrm_engine* e, const sdrm_vae_encoder* enc, void* stream) {
  if (int rc = check_encoder(e, enc, "sdrm_vae_encoder_load")) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(enc->n_items, enc->hidden, enc->latent, 0);
  e->enc_loaded = false;
  float *w1t, *w1p, *b1p, *w2p, *b2p;
  double* part;
  int rc;
  if ((rc = scratch(e, SCR_ENC_W1T, (size_t)enc->n_items * d.Hq, &w1t)) || (rc = scratch(e, SCR_ENC_W1, (size_t)d.Hr * d.Ip, &w1p)) ||
      (rc = scratch(e, SCR_ENC_B1, d.Hr, &b1p)) || (rc = scratch(e, SCR_ENC_W2, (size_t)d.L2r * d.Hp, &w2p)) ||
      (rc = scratch(e, SCR_ENC_B2, d.L2r, &b2p)) || (rc = scratch(e, SCR_ENC_PART, KL_PARTS, &part)))
    return rc;
  PadList pad;
  pad.add(enc->w1, enc->hidden, enc->n_items, w1p, d.Hr, d.Ip);
  pad.add(enc->b1, 1, enc->hidden, b1p, 1, d.Hr);
  pad.add(enc->w2, d.L2, enc->hidden, w2p, d.L2r, d.Hp);
  pad.add(enc->b2, 1, d.L2, b2p, 1, d.L2r);
  if ((rc = pad.launch(e, PC_NONE, st))) return rc;
  if ((rc = launch_w1t(e, PC_NONE, enc->w1, enc->hidden, enc->n_items, w1t, d.Hq, st))) return rc;
  e->enc_items = enc->n_items; e->enc_hidden = enc->hidden; e->enc_latent = enc->latent;
  e->enc_loaded = true;
  return SDRM_OK;
}

int sdrm_vae_encode(sdrm_engine* e, const float* x, int n, float* z, float* kl, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!x || !z) return fail(e, SDRM_ERR_ARG, "sdrm_vae_encode: null pointer");
  if (!e->enc_loaded) return fail(e, SDRM_ERR_STATE, "sdrm_vae_encode: no encoder loaded (sdrm_vae_encoder_load)");
  if (n < 1 || n > MAX_BATCH_ROWS) return fail(e, SDRM_ERR_SHAPE, "sdrm_vae_encode: n outside 1 .. 2^22");
  if (int jr = chains_join(e, (hipStream_t)stream)) return jr;
  return encode_dense_launches(e, x, n, z, kl, (hipStream_t)stream);
}

int sdrm_vae_encode_csr(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows,
                        const int64_t* rows, int64_t row0, int b, float* z, float* kl, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!z) return fail(e, SDRM_ERR_ARG, "sdrm_vae_encode_csr: null pointer");
  if (!e->enc_loaded) return fail(e, SDRM_ERR_STATE, "sdrm_vae_encode_csr: no encoder loaded (sdrm_vae_encoder_load)");
  EncodeCsrArgs a{};
  if (int rc = csr_batch(e, "sdrm_vae_encode_csr", indptr, indices, data, n_rows, rows, row0, b, e->enc_items, &a.csr)) return rc;
  if (b > MAX_BATCH_ROWS) return fail(e, SDRM_ERR_SHAPE, "sdrm_vae_encode_csr: b outside 1 .. 2^22");
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(e->enc_items, e->enc_hidden, e->enc_latent, b);
  const int q = d.Hq / 4;
  if (q > ENC_GATHER_MAX_Q) {   // a hidden vector wider than the gather kernel's registers: densify into scratch, then the dense form
    float* dense;
    if (int rc = scratch(e, SCR_ENC_DENSE, (size_t)b * e->enc_items, &dense)) return rc;
    if (int rc = sdrm_csr_rows_to_dense(e, indptr, indices, data, n_rows, rows, row0, b, e->enc_items, dense, stream)) return rc;
    return encode_dense_launches(e, dense, b, z, kl, st);
  }
  if (int rc = scratch(e, SCR_ENC_HID, (size_t)d.MP * d.Hp, &a.hid)) return rc;
  a.w1t = scratch_at(e, SCR_ENC_W1T); a.b1 = scratch_at(e, SCR_ENC_B1); a.Hq = d.Hq; a.Hp = d.Hp;
  if (int rc = launch_gather_rows(e, PC_NONE, "k_encode_csr", q, a, st, [](auto tpr, auto nv, auto u) { return k_encode_csr<VAL(tpr), VAL(nv), VAL(u)>; }))
    return rc;
  return encode_tail(e, b, z, kl, st);
}

// ---------------------------------------------------------------------------------------------
// The VAE encoder behind its first pre-activation in TRAIN mode (train_SDRM.py:244-250 with is_training == 1: Tanh, the second Linear,
// chunk, the KL, the reparameterisation; and their share of :148), csrc/latent.h.  The frozen encoder above is not touched.
constexpr int LATENT_WGRAD_KCHUNK = 8192;   // most batch rows of one weight-gradient slab (the pre-stage's batches are a few hundred: one slab)

// The host side of both entry points that needs no device: the envelope (`contiguous` != 0: the feed rows are row0 .. row0 + b - 1).
int sdrm_debug_latent_args(int hidden, int latent, int b, int64_t row0, int contiguous) {
  if (hidden < 1 || hidden > VAE_MAX_HIDDEN || latent < 1 || latent > VAE_MAX_LATENT || b < 1 || b > MAX_BATCH_ROWS) return SDRM_ERR_SHAPE;
  if (contiguous && (row0 < 0 || row0 + b > ((int64_t)1 << 31))) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

namespace {

const char* const kLatentEnvelope = ": hidden outside 1 .. 4096, latent outside 1 .. 4096, b outside 1 .. 2^22, or feed rows row0 .. row0 + b - 1 "
                                    "outside [0, 2^31)";

}  // namespace

int sdrm_vae_latent_fwd(sdrm_engine* e, const float* pre, const float* w2, const float* b2, int hidden, int latent, const int64_t* rows,
                        int64_t row0, int b, uint64_t seed, uint32_t step, int draw, float* h1, float* out2, float* eps, float* z, float* kl,
                        void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!pre || !w2 || !b2 || !h1 || !out2 || !eps || !z || !kl) return fail(e, SDRM_ERR_ARG, "sdrm_vae_latent_fwd: null pointer");
  if (int rc = sdrm_debug_latent_args(hidden, latent, b, row0, rows == nullptr)) return fail(e, rc, std::string("sdrm_vae_latent_fwd") + kLatentEnvelope);
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(0, hidden, latent, b);
  LatentStageArgs sa{};
  LatentReparamArgs ra{};
  int rc;
  if ((rc = scratch(e, SCR_LAT_H, (size_t)d.MP * d.Hp, &sa.hp)) || (rc = scratch(e, SCR_LAT_W2, (size_t)d.L2r * d.Hp, &sa.w2p)) ||
      (rc = scratch(e, SCR_LAT_B2, d.L2r, &sa.b2p)) || (rc = scratch(e, SCR_LAT_PART, KL_PARTS, &ra.part)))
    return rc;
  // 1: h1 = tanh(pre) into the caller's buffer and the padded operand; W2 and b2 padded (they change with every optimiser step)
  sa.pre = pre; sa.h1 = h1; sa.b = b; sa.H = hidden; sa.MP = d.MP; sa.Hp = d.Hp;
  sa.w2 = w2; sa.L2 = d.L2; sa.L2r = d.L2r;
  sa.b2 = b2;
  if ((rc = launch_k(e, PC_LATENT, "k_latent_stage", k_latent_stage, dim3(blocks_for((int64_t)std::max(d.MP, d.L2r) * (d.Hp / 4)), 3), dim3(256), 0,
                     st, sa)))
    return rc;
  // 2: out2 = h1 W2^T + b2, bounds-checked into the caller's [b][2L]
  {
    GemmArgs a{};
    a.C = out2; a.ldc = d.L2; a.bias = sa.b2p;
    a.rows_valid = b; a.cols_valid = d.L2;
    HIP_TRY(e, (gemm_forward<XF_NONE, EPI_BIAS_G>(a, sa.hp, d.Hp, sa.w2p, d.Hp, d.rows64, d.L2p, d.Hp, st, Prof{e, PC_LATENT, 2.0 * b * d.L2 * hidden},
                                                   choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows))));
  }
  // 3: the draw, z and the KL partials; 4: their sum
  const int parts = std::min(b, KL_PARTS);
  ra.out2 = out2; ra.rows = rows; ra.row0 = row0; ra.b = b; ra.L = latent;
  ra.k0 = (uint32_t)seed; ra.k1 = (uint32_t)(seed >> 32); ra.step = step; ra.draw = draw;
  ra.eps = eps; ra.z = z; ra.flag = e->feed_flag;
  if ((rc = launch_k(e, PC_LATENT, "k_latent_reparam", k_latent_reparam, dim3((unsigned)parts), dim3(256), 0, st, ra))) return rc;
  return launch_k(e, PC_LATENT, "k_encode_kl_sum", k_encode_kl_sum, dim3(1), dim3(256), 0, st, ra.part, parts, b, kl);
}

int sdrm_vae_latent_bwd(sdrm_engine* e, const float* h1, const float* out2, const float* eps, const float* w2, int hidden, int latent, int b,
                        const float* gz, const float* gkl, float* dpre, float* dw2, float* db2, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!h1 || !out2 || !eps || !w2 || !dpre || !dw2 || !db2) return fail(e, SDRM_ERR_ARG, "sdrm_vae_latent_bwd: null pointer");
  if (int rc = sdrm_debug_latent_args(hidden, latent, b, 0, 0)) return fail(e, rc, std::string("sdrm_vae_latent_bwd") + kLatentEnvelope);
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(0, hidden, latent, b);
  const SplitK sk = split_k(d.Kb, LATENT_WGRAD_KCHUNK);
  float *hp, *w2t, *dp, *slab, *dbias;
  int rc;
  if ((rc = scratch(e, SCR_LAT_H, (size_t)d.MP * d.Hp, &hp)) || (rc = scratch(e, SCR_LAT_W2T, (size_t)d.Hr * d.L2p, &w2t)) ||
      (rc = scratch(e, SCR_LAT_DOUT2, (size_t)d.MP * d.L2p, &dp)) || (rc = scratch(e, SCR_LAT_SLAB, (size_t)sk.S * d.L2p * d.Hp, &slab)) ||
      (rc = scratch(e, SCR_LAT_DBIAS, (size_t)sk.S * d.L2p, &dbias)))
    return rc;
  // 1: W2^T (the NT dgrad's operand) and the padded h1 (the weight gradient's operand, the dgrad epilogue's aux)
  LatentStageBwdArgs sa{};
  sa.w2 = w2; sa.w2t = w2t; sa.L2 = d.L2; sa.H = hidden; sa.L2p = d.L2p; sa.Hr = d.Hr;
  sa.h1 = h1; sa.hp = hp; sa.b = b; sa.MP = d.MP; sa.Hp = d.Hp;
  sa.tiles_l = d.L2p / 32; sa.tiles = (d.Hr / 32) * sa.tiles_l;
  if ((rc = launch_k(e, PC_LATENT, "k_latent_stage_bwd", k_latent_stage_bwd, dim3((unsigned)sa.tiles + blocks_for((int64_t)d.MP * (d.Hp / 4))),
                     dim3(256), 0, st, sa)))
    return rc;
  // 2: dout2 = [dmu | dlv], padded
  LatentSeedArgs ga{};
  ga.out2 = out2; ga.eps = eps; ga.gz = gz; ga.gkl = gkl; ga.b = b; ga.L = latent; ga.MP = d.MP; ga.L2p = d.L2p; ga.dp = dp;
  if ((rc = launch_k(e, PC_LATENT, "k_latent_seed", k_latent_seed, dim3(blocks_for((int64_t)d.MP * (d.L2p / 4))), dim3(256), 0, st, ga))) return rc;
  // 3: dW2 = dout2^T h1 into slabs, db2 = column sums of dout2 (the reduction runs over the batch rows: M-contiguous operands)
  HIP_TRY(e, (gemm_wgrad<XF_NONE>(dp, d.L2p, d.L2p, hp, d.Hp, d.Hp, nullptr, d.Kb, sk.S, sk.kchunk, slab, dbias, st,
                                  Prof{e, PC_LATENT, 2.0 * b * d.L2 * hidden}, pick_cfg(e->tune))));
  // 4: dpre = (dout2 W2) (1 - h1^2), bounds-checked into the caller's [b][hidden]
  {
    GemmArgs a{};
    a.A = dp; a.lda = d.L2p; a.limA = d.rows64;
    a.B = w2t; a.ldb = d.L2p; a.limB = d.Hp;
    a.C = dpre; a.ldc = hidden; a.rows_valid = b; a.cols_valid = hidden;
    a.K = d.L2p; a.kchunk = d.L2p;
    a.aux = hp; a.ldaux = d.Hp;
    HIP_TRY(e, (launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI_DTANH_G>(a, d.rows64, d.Hp, 1, st, Prof{e, PC_LATENT, 2.0 * b * d.L2 * hidden},
                                                                                    choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows))));
  }
  // 5: the slabs and bias sums into the caller's dw2 [2L][hidden] and db2 [2L]
  LatentUnpadArgs ua{};
  ua.slab = slab; ua.dbias = dbias; ua.S = sk.S; ua.L2 = d.L2; ua.H = hidden; ua.L2p = d.L2p; ua.Hp = d.Hp; ua.dw2 = dw2; ua.db2 = db2;
  return launch_k(e, PC_LATENT, "k_latent_unpad", k_latent_unpad, dim3(blocks_for((int64_t)d.L2 * ((hidden + 3) / 4) + d.L2)), dim3(256), 0, st, ua);
}

// ---------------------------------------------------------------------------------------------
// The VAE decoder and the multinomial loss head in TRAIN mode (train_SDRM.py:252-254 and :141-142, and their share of :148),
// csrc/decoder_train.h.  The scratch of sdrm_vae_decode and a loaded frozen encoder are not touched.
constexpr int DECHEAD_WGRAD_KCHUNK = 8192;   // most batch rows of one weight-gradient slab (the pre-stage's batches are a few hundred: one slab)

namespace {

// Batch rows of one slab of the dW4 weight gradient: launch_gemm_cfg refuses a launch whose K chunk (+ 64) times the operand's row
// stride reaches 2^32 bytes, and g's stride is Ip - so the chunk follows from Ip (8192 up to Ip = 130048, 928 at Ip = 2^20).
int dh_kchunk4(int Ip) {
  const int64_t kc = (((int64_t)1 << 30) - 1) / Ip - 64;   // (kc + 64) * Ip * 4 < 2^32
  return (int)std::min<int64_t>(DECHEAD_WGRAD_KCHUNK, kc / 32 * 32);
}
// the split-K plans of dW4 and dW3
SplitK dh_split4(const VaeDims& d) { return split_k(d.Kb, dh_kchunk4(d.Ip)); }
SplitK dh_split3(const VaeDims& d) { return split_k(d.Kb, DECHEAD_WGRAD_KCHUNK); }

const char* const kDecheadEnvelope = ": latent outside 1 .. 4096, hidden outside 1 .. 4096, n_items outside 1 .. 2^20, b outside 1 .. 2^22, b x n_items >= 2^40, "
                                     "n_rows < 1, row0 < 0, or rows row0 .. row0 + b - 1 end behind the matrix";

}  // namespace

// The host side of both entry points that needs no device: the envelope, and every test a later launch would make on any tile
// (`contiguous` != 0: the batch is the feed rows row0 .. row0 + b - 1).
int sdrm_debug_decoder_nll_args(int latent, int hidden, int n_items, int b, int64_t row0, int64_t n_rows, int contiguous) {
  if (latent < 1 || latent > VAE_MAX_LATENT || hidden < 1 || hidden > VAE_MAX_HIDDEN || n_items < 1 || n_items > MAX_ITEMS || b < 1 ||
      b > MAX_BATCH_ROWS || (int64_t)b * n_items >= ((int64_t)1 << 40) || n_rows < 1 || row0 < 0)
    return SDRM_ERR_SHAPE;
  if (contiguous && row0 + b > n_rows) return SDRM_ERR_SHAPE;
  const VaeDims d = vae_dims(n_items, hidden, latent, b);
  const SplitK s4 = dh_split4(d), s3 = dh_split3(d);
  if (s4.kchunk < 32) return SDRM_ERR_SHAPE;
  for (int cfg = 0; cfg < N_TILE_CFGS; ++cfg) {
    // forward: z W3^T, h3 W4^T; backward: g W4 (K = Ip), dpre3 W3 (K = Hp); the two weight gradients
    if (gemm_nt_band_rows(cfg, d.Hp) < 1 || gemm_nt_band_rows(cfg, d.Ip) < 1 || gemm_nt_band_rows(cfg, d.Lp) < 1) return SDRM_ERR_SHAPE;
    if (!gemm_span_ok(cfg, true, d.Lp, d.Lp, d.Lp) || !gemm_span_ok(cfg, true, d.Hp, d.Hp, d.Hp) || !gemm_span_ok(cfg, true, d.Ip, d.Ip, d.Ip))
      return SDRM_ERR_SHAPE;
    if (gemm_wgrad_band_cols(cfg, d.Hp, s4.S) < 1 || gemm_wgrad_band_cols(cfg, d.Lp, s3.S) < 1) return SDRM_ERR_SHAPE;
    if (!gemm_span_ok(cfg, false, d.Ip, d.Hp, s4.kchunk) || !gemm_span_ok(cfg, false, d.Hp, d.Lp, s3.kchunk)) return SDRM_ERR_SHAPE;
  }
  return SDRM_OK;
}

int sdrm_vae_decoder_nll_fwd(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, const int64_t* indptr, const int32_t* indices,
                             const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b, float* h3, float* logits,
                             float* lse, float* loss, void* stream) {
  const char* who = "sdrm_vae_decoder_nll_fwd";
  if (!e) return SDRM_ERR_ARG;
  if (!dec_tensors(dec) || !z || !indptr || !indices || !h3 || !logits || !lse || !loss) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if ((uintptr_t)logits & 15u) return fail(e, SDRM_ERR_ARG, std::string(who) + ": logits must be 16-byte aligned");
  const int L = dec->latent, H = dec->hidden, I = dec->n_items;
  if (int rc = sdrm_debug_decoder_nll_args(L, H, I, b, row0, n_rows, rows == nullptr)) return fail(e, rc, std::string(who) + kDecheadEnvelope);
  NllArgs na{};
  if (int rc = csr_batch(e, who, indptr, indices, data, n_rows, rows, row0, b, I, &na.csr)) return rc;
  na.logits = logits;
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(I, H, L, b);
  float *zp, *w3p, *b3p, *h3p, *w4p, *b4p;
  int rc;
  if ((rc = scratch(e, SCR_DH_Z, (size_t)d.MP * d.Lp, &zp)) || (rc = scratch(e, SCR_DH_W3, (size_t)d.Hr * d.Lp, &w3p)) ||
      (rc = scratch(e, SCR_DH_B3, d.Hr, &b3p)) || (rc = scratch(e, SCR_DH_H3, (size_t)d.MP * d.Hp, &h3p)) ||
      (rc = scratch(e, SCR_DH_W4, (size_t)d.Ir * d.Hp, &w4p)) || (rc = scratch(e, SCR_DH_B4, d.Ir, &b4p)))
    return rc;
  // 1: z and the four tensors padded (the weights change with every optimiser step)
  {
    PadList pad;
    pad.add(z, b, L, zp, d.MP, d.Lp);
    pad.add(dec->w1, H, L, w3p, d.Hr, d.Lp);
    pad.add(dec->b1, 1, H, b3p, 1, d.Hr);
    pad.add(dec->w2, I, H, w4p, d.Ir, d.Hp);
    pad.add(dec->b2, 1, I, b4p, 1, d.Ir);
    if ((rc = pad.launch(e, PC_DECODER, st))) return rc;
  }
  const int cfg = choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows);
  // 2: h3 = tanh(z W3^T + b3) into the padded [MP][Hp], the second GEMM's A operand (the launch decode_launches makes; columns behind
  //    H are tanh(0) = 0 - W3's pad rows and b3's pad are zero -, rows behind b feed only output rows that 4 drops)
  {
    GemmArgs a{};
    a.B = w3p; a.ldb = d.Lp; a.C = h3p; a.ldc = d.Hp; a.K = d.Lp; a.bias = b3p;
    if ((rc = gemm_nt_banded<EPI_BIAS_TANH>(e, a, zp, d.Lp, d.rows64, d.Hp, b, st, Prof{e, PC_DECODER, 2.0 * b * (double)H * L}, cfg))) return rc;
  }
  // 3: its b rows and H columns into the caller's h3 [b][H]
  {
    const DecH3Args ha{h3p, h3, b, H, d.Hp};
    if ((rc = launch_k(e, PC_DECODER, "k_dechead_h3", k_dechead_h3, dim3(blocks_for((int64_t)b * ((H + 3) / 4))), dim3(256), 0, st, ha))) return rc;
  }
  // 4: logits = h3 W4^T + b4, bounds-checked into the caller's [b][I]
  {
    GemmArgs a{};
    a.B = w4p; a.ldb = d.Hp; a.C = logits; a.ldc = I; a.K = d.Hp; a.bias = b4p; a.cols_valid = I;
    if ((rc = gemm_nt_banded<EPI_BIAS_G>(e, a, h3p, d.Hp, d.rows64, d.Ip, b, st, Prof{e, PC_DECODER, 2.0 * b * (double)I * H}, cfg))) return rc;
  }
  // 5: lse and the loss terms over exactly I columns of the caller's logits (csrc/nll.h); 6: their sum
  const int parts = std::min(b, NLL_PARTS);
  if ((rc = launch_k(e, PC_DECODER, "k_nll_rows", k_nll_rows, dim3((unsigned)parts), dim3(256), 0, st, na, lse, e->nll_part))) return rc;
  return launch_k(e, PC_DECODER, "k_nll_sum", k_nll_sum, dim3(1), dim3(256), 0, st, e->nll_part, parts, b, loss);
}

int sdrm_vae_decoder_nll_bwd(sdrm_engine* e, const sdrm_vae_decoder* dec, const float* z, const float* h3, const float* logits, const float* lse,
                             const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, const int64_t* rows,
                             int64_t row0, int b, const float* scale, float* dz, float* dw3, float* db3, float* dw4, float* db4, void* stream) {
  const char* who = "sdrm_vae_decoder_nll_bwd";
  if (!e) return SDRM_ERR_ARG;
  if (!dec_tensors(dec, false) || !z || !h3 || !logits || !lse || !indptr || !indices || !dw3 || !db3 || !dw4 || !db4)
    return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if ((uintptr_t)logits & 15u) return fail(e, SDRM_ERR_ARG, std::string(who) + ": logits must be 16-byte aligned");
  const int L = dec->latent, H = dec->hidden, I = dec->n_items;
  if (int rc = sdrm_debug_decoder_nll_args(L, H, I, b, row0, n_rows, rows == nullptr)) return fail(e, rc, std::string(who) + kDecheadEnvelope);
  DecGradArgs ga{};
  if (int rc = csr_batch(e, who, indptr, indices, data, n_rows, rows, row0, b, I, &ga.csr)) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const VaeDims d = vae_dims(I, H, L, b);
  const SplitK s4 = dh_split4(d), s3 = dh_split3(d);
  float *zp, *h3p, *w4t, *w3t, *zb, *g, *dp3, *slab4, *dbs4, *slab3, *dbs3;
  int rc;
  if ((rc = scratch(e, SCR_DH_Z, (size_t)d.MP * d.Lp, &zp)) || (rc = scratch(e, SCR_DH_H3, (size_t)d.MP * d.Hp, &h3p)) ||
      (rc = scratch(e, SCR_DH_W4T, (size_t)d.Hr * d.Ip, &w4t)) || (rc = scratch(e, SCR_DH_W3T, (size_t)d.Lr * d.Hp, &w3t)) ||
      (rc = scratch(e, SCR_DH_ZB, d.Lr, &zb)) || (rc = scratch(e, SCR_DH_G, (size_t)d.MP * d.Ip, &g)) ||
      (rc = scratch(e, SCR_DH_DP3, (size_t)d.MP * d.Hp, &dp3)) || (rc = scratch(e, SCR_DH_SLAB4, (size_t)s4.S * d.Ip * d.Hp, &slab4)) ||
      (rc = scratch(e, SCR_DH_DB4, (size_t)s4.S * d.Ip, &dbs4)) || (rc = scratch(e, SCR_DH_SLAB3, (size_t)s3.S * d.Hp * d.Lp, &slab3)) ||
      (rc = scratch(e, SCR_DH_DB3, (size_t)s3.S * d.Hp, &dbs3)))
    return rc;
  // 1: W4^T and W3^T (the NT dgrads' operands), h3 and z padded (the weight gradients' operands), the last dgrad's zero bias
  DecStageBwdArgs sa{};
  sa.t4 = DecTranspose{dec->w2, w4t, I, H, d.Ip, d.Ip / 32};
  sa.t3 = DecTranspose{dec->w1, w3t, H, L, d.Hp, d.Hp / 32};
  sa.tiles4 = (int64_t)(d.Hr / 32) * (d.Ip / 32); sa.tiles = sa.tiles4 + (int64_t)(d.Lr / 32) * (d.Hp / 32);
  sa.h3 = h3; sa.h3p = h3p; sa.b = b; sa.H = H; sa.MP = d.MP; sa.Hp = d.Hp;
  sa.z = z; sa.zp = zp; sa.L = L; sa.Lp = d.Lp;
  sa.zb = zb; sa.Lr = d.Lr;
  if ((rc = launch_k(e, PC_DECODER, "k_dechead_stage_bwd", k_dechead_stage_bwd,
                     dim3((unsigned)sa.tiles + blocks_for((int64_t)d.MP * ((d.Hp + d.Lp) / 4) + d.Lr / 4)), dim3(256), 0, st, sa)))
    return rc;
  // 2: g = scale (softmax s_r - X) / b into [MP][Ip], zero behind b rows / I columns
  ga.logits = logits; ga.lse = lse; ga.scale = scale; ga.g = g; ga.MP = d.MP; ga.Ip = d.Ip;
  if ((rc = launch_k(e, PC_DECODER, "k_dechead_grad", k_dechead_grad, dim3((unsigned)std::min(d.MP, 1 << 16)), dim3(256), 0, st, ga))) return rc;
  const int cfg_w = pick_cfg(e->tune), cfg = choose_cfg(e->tune, d.rows64, e->tune.nt32_max_rows);
  // 3: dW4 = g^T h3 into slabs, db4 = column sums of g (the reduction runs over the batch rows: M-contiguous operands)
  if ((rc = gemm_wgrad_banded(e, g, d.Ip, h3p, d.Hp, d.Kb, s4.S, s4.kchunk, slab4, dbs4, st, Prof{e, PC_DECODER, 2.0 * b * (double)I * H}, cfg_w)))
    return rc;
  // 4: dpre3 = (g W4)(1 - h3^2) into [MP][Hp]: all rows64 rows and Hp columns are stored - behind b rows g is zero, behind H columns
  //    W4^T is: the products are zeros, written by this call
  {
    GemmArgs a{};
    a.B = w4t; a.ldb = d.Ip; a.C = dp3; a.ldc = d.Hp; a.K = d.Ip; a.aux = h3p; a.ldaux = d.Hp; a.cols_valid = d.Hp;
    if ((rc = gemm_nt_banded<EPI_DTANH_G>(e, a, g, d.Ip, d.rows64, d.Hp, d.rows64, st, Prof{e, PC_DECODER, 2.0 * b * (double)I * H}, cfg))) return rc;
  }
  // 5: dW3 = dpre3^T z into slabs, db3 = column sums of dpre3
  if ((rc = gemm_wgrad_banded(e, dp3, d.Hp, zp, d.Lp, d.Kb, s3.S, s3.kchunk, slab3, dbs3, st, Prof{e, PC_DECODER, 2.0 * b * (double)H * L}, cfg_w)))
    return rc;
  // 6: dz = dpre3 W3, bounds-checked into the caller's [b][L] (the bias epilogue on a bias of zeros)
  if (dz) {
    GemmArgs a{};
    a.B = w3t; a.ldb = d.Hp; a.C = dz; a.ldc = L; a.K = d.Hp; a.bias = zb; a.cols_valid = L;
    if ((rc = gemm_nt_banded<EPI_BIAS_G>(e, a, dp3, d.Hp, d.rows64, d.Lp, b, st, Prof{e, PC_DECODER, 2.0 * b * (double)H * L}, cfg))) return rc;
  }
  // 7: the slabs and bias sums into the caller's dw4 [I][H], db4 [I], dw3 [H][L], db3 [H]
  DecUnpadArgs ua{};
  ua.seg[0] = DecUnpadSeg{slab4, dbs4, s4.S, I, H, d.Ip, d.Hp, dw4, db4};
  ua.seg[1] = DecUnpadSeg{slab3, dbs3, s3.S, H, L, d.Hp, d.Lp, dw3, db3};
  return launch_k(e, PC_DECODER, "k_dechead_unpad", k_dechead_unpad, dim3(blocks_for((int64_t)I * ((H + 3) / 4) + I), 2), dim3(256), 0, st, ua);
}

// ---------------------------------------------------------------------------------------------
// Adam over caller-owned tensors and the loss value of a pre-stage step (train_SDRM.py:126, :143-150), csrc/vae_adam.h.
// The host side that needs no device: every refusal of sdrm_vae_adam_step, on integers, and the chunk count of the table.
int sdrm_debug_vae_adam_args(const uint64_t* addr, const int64_t* n, const float* l2_coef, int n_tensors, int64_t step, int has_partials,
                             int64_t l2_capacity, int64_t* chunks_out) {
  if (!addr || !n || !l2_coef) return SDRM_ERR_ARG;
  if (n_tensors <= 0) return SDRM_ERR_SHAPE;
  if (step < 1) return SDRM_ERR_ARG;
  int64_t chunks = 0;
  bool any_l2 = false;
  for (int i = 0; i < n_tensors; ++i) {
    for (int j = 0; j < 4; ++j)
      if (addr[4 * i + j] == 0) return SDRM_ERR_ARG;
    if (n[i] <= 0 || n[i] > ((int64_t)1 << 40)) return SDRM_ERR_SHAPE;
    if (!(l2_coef[i] >= 0.f)) return SDRM_ERR_ARG;   // (a nan as well)
    any_l2 = any_l2 || l2_coef[i] > 0.f;
    chunks += (n[i] + VADAM_CHUNK - 1) / VADAM_CHUNK;
    if (chunks > ((int64_t)1 << 30)) return SDRM_ERR_SHAPE;
  }
  if (has_partials && any_l2 && l2_capacity < chunks) return SDRM_ERR_SHAPE;
  // no two of the 4 x n_tensors ranges [ptr, ptr + n) may share a byte (ranges that only touch are fine)
  std::vector<std::pair<uint64_t, uint64_t>> span((size_t)4 * n_tensors);
  for (int i = 0; i < n_tensors; ++i)
    for (int j = 0; j < 4; ++j) {
      const uint64_t lo = addr[4 * i + j], bytes = (uint64_t)n[i] * sizeof(float);
      if (lo + bytes < lo) return SDRM_ERR_ARG;   // wraps the address space
      span[(size_t)4 * i + j] = {lo, lo + bytes};
    }
  std::sort(span.begin(), span.end());
  for (size_t k = 1; k < span.size(); ++k)
    if (span[k].first < span[k - 1].second) return SDRM_ERR_ARG;
  if (chunks_out) *chunks_out = chunks;
  return SDRM_OK;
}

int sdrm_vae_adam_step(sdrm_engine* e, const sdrm_vae_adam_tensor* t, int n_tensors, int64_t step, float lr, float beta1, float beta2,
                       float eps, double* l2_partials, int64_t l2_capacity, void* stream) {
  const char* who = "sdrm_vae_adam_step";
  if (!e) return SDRM_ERR_ARG;
  if (!t) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (n_tensors <= 0) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": n_tensors <= 0");
  std::vector<uint64_t> addr((size_t)4 * n_tensors);
  std::vector<int64_t> n(n_tensors);
  std::vector<float> coef(n_tensors);
  for (int i = 0; i < n_tensors; ++i) {
    addr[4 * i] = (uint64_t)(uintptr_t)t[i].p; addr[4 * i + 1] = (uint64_t)(uintptr_t)t[i].g;
    addr[4 * i + 2] = (uint64_t)(uintptr_t)t[i].m; addr[4 * i + 3] = (uint64_t)(uintptr_t)t[i].v;
    n[i] = t[i].n; coef[i] = t[i].l2_coef;
  }
  int64_t chunks = 0;
  if (int rc = sdrm_debug_vae_adam_args(addr.data(), n.data(), coef.data(), n_tensors, step, l2_partials != nullptr, l2_capacity, &chunks))
    return fail(e, rc, std::string(who) + ": a null pointer, step < 1, a negative l2_coef or two of the ranges [ptr, ptr + n) overlapping (SDRM_ERR_ARG); "
                                          "n outside 1 .. 2^40, more than 2^30 chunks of 4096 elements, or l2_capacity below the chunk count (SDRM_ERR_SHAPE)");
  bool any_l2 = false;
  for (int i = 0; i < n_tensors; ++i) any_l2 = any_l2 || coef[i] > 0.f;
  VAdamArgs a{};
  adam_scalars(step, lr, (double)beta1, (double)beta2, a.step_size, a.bc2_sqrt);
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.l2_partials = any_l2 ? l2_partials : nullptr;
  hipStream_t st = (hipStream_t)stream;
  unsigned chunk0 = 0;
  for (int i0 = 0; i0 < n_tensors; i0 += VADAM_MAX_TENSORS) {
    VAdamTable tab{};
    tab.n = std::min(VADAM_MAX_TENSORS, n_tensors - i0);
    unsigned c = 0;
    for (int k = 0; k < tab.n; ++k) {
      const sdrm_vae_adam_tensor& s = t[i0 + k];
      VAdamTensor& d = tab.t[k];
      d.p = s.p; d.g = s.g; d.m = s.m; d.v = s.v; d.n = s.n;
      d.wd2 = 2.f * s.l2_coef;
      d.first_chunk = c;
      d.vector_ok = (((uintptr_t)s.p | (uintptr_t)s.g | (uintptr_t)s.m | (uintptr_t)s.v) & 15u) == 0;
      c += (unsigned)((s.n + VADAM_CHUNK - 1) / VADAM_CHUNK);
    }
    a.chunk0 = chunk0;
    if (int rc = launch_k(e, PC_VAE_ADAM, "k_vae_adam", k_vae_adam, dim3(c), dim3(256), 0, st, tab, a)) return rc;
    chunk0 += c;
  }
  return SDRM_OK;
}

int sdrm_vae_loss_slot(sdrm_engine* e, const float* neg_ll, const float* kl, float anneal, const double* l2_partials, int64_t n_partials,
                       float weight_decay, float* out, void* stream) {
  const char* who = "sdrm_vae_loss_slot";
  if (!e) return SDRM_ERR_ARG;
  if (!neg_ll || !kl || !out) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (l2_partials && n_partials < 1) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": l2_partials given with n_partials < 1");
  return launch_k(e, PC_VAE_ADAM, "k_vae_loss_slot", k_vae_loss_slot, dim3(1), dim3(256), 0, (hipStream_t)stream, neg_ll, kl, anneal, l2_partials,
                  n_partials, weight_decay, out);
}

// ---------------------------------------------------------------------------------------------
// Loss head of the VAE pre-stage (train_SDRM.py:141-142), csrc/nll.h.
namespace {

constexpr int NLL_GRAD_BLOCKS = 1 << 16;   // most work-groups of k_nll_grad; either kernel strides over the rows behind its grid

// the checks of both entry points, and their kernels' arguments
int nll_args(sdrm_engine* e, const char* who, const float* logits, const int64_t* indptr, const int32_t* indices, const float* data,
             int64_t n_rows, const int64_t* rows, int64_t row0, int b, int n_items, NllArgs* a) {
  const std::string w(who);
  if (!logits) return fail(e, SDRM_ERR_ARG, w + ": null pointer");
  if ((uintptr_t)logits & 15u) return fail(e, SDRM_ERR_ARG, w + ": logits must be 16-byte aligned");
  if (int rc = csr_batch(e, who, indptr, indices, data, n_rows, rows, row0, b, n_items, &a->csr)) return rc;
  if (n_items > MAX_ITEMS || (int64_t)b * n_items >= ((int64_t)1 << 40))
    return fail(e, SDRM_ERR_SHAPE, w + ": n_items outside 1 .. 2^20 or b x n_items >= 2^40");
  a->logits = logits;
  return SDRM_OK;
}

}  // namespace

int sdrm_multinomial_nll_csr(sdrm_engine* e, const float* logits, const int64_t* indptr, const int32_t* indices, const float* data,
                             int64_t n_rows, const int64_t* rows, int64_t row0, int b, int n_items, float* lse, float* loss, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!lse || !loss) return fail(e, SDRM_ERR_ARG, "sdrm_multinomial_nll_csr: null pointer");
  NllArgs a{};
  if (int rc = nll_args(e, "sdrm_multinomial_nll_csr", logits, indptr, indices, data, n_rows, rows, row0, b, n_items, &a)) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int parts = std::min(b, NLL_PARTS);
  if (int rc = launch_k(e, PC_NLL, "k_nll_rows", k_nll_rows, dim3((unsigned)parts), dim3(256), 0, st, a, lse, e->nll_part)) return rc;
  return launch_k(e, PC_NONE, "k_nll_sum", k_nll_sum, dim3(1), dim3(256), 0, st, e->nll_part, parts, b, loss);
}

int sdrm_multinomial_nll_csr_grad(sdrm_engine* e, const float* logits, const float* lse, const int64_t* indptr, const int32_t* indices,
                                  const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b, int n_items,
                                  const float* scale, float* grad, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!lse || !grad) return fail(e, SDRM_ERR_ARG, "sdrm_multinomial_nll_csr_grad: null pointer");
  if ((uintptr_t)grad & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_multinomial_nll_csr_grad: grad must be 16-byte aligned");
  NllArgs a{};
  if (int rc = nll_args(e, "sdrm_multinomial_nll_csr_grad", logits, indptr, indices, data, n_rows, rows, row0, b, n_items, &a)) return rc;
  const uintptr_t lo = (uintptr_t)logits, go = (uintptr_t)grad, bytes = (uintptr_t)b * (uintptr_t)n_items * sizeof(float);
  if (lo != go && lo < go + bytes && go < lo + bytes)
    return fail(e, SDRM_ERR_ARG, "sdrm_multinomial_nll_csr_grad: grad overlaps logits (only grad == logits may alias)");
  return launch_k(e, PC_NLL, "k_nll_grad", k_nll_grad, dim3((unsigned)std::min(b, NLL_GRAD_BLOCKS)), dim3(256), 0, (hipStream_t)stream, a, lse, scale,
                  grad);
}

// ---------------------------------------------------------------------------------------------
// Input layer of the VAE encoder in train mode (train_SDRM.py:242-244, first Linear; its weight's share of :148), csrc/input_layer.h.

// The host side of both entry points that needs no device: the envelope, and the dropout threshold and scale of a float p_drop.
int sdrm_debug_input_layer_args(int n_items, int hidden, int64_t n_rows, int64_t first, int b, int contiguous, float p_drop,
                                uint32_t* thr, float* scale) {
  if (n_items < 1 || n_items > MAX_ITEMS || hidden < 1 || hidden > VAE_MAX_HIDDEN || n_rows < 1 || n_rows > (int64_t)INT32_MAX ||
      b < 1 || b > MAX_BATCH_ROWS || first < 0)
    return SDRM_ERR_SHAPE;
  if (contiguous && first + b > n_rows) return SDRM_ERR_SHAPE;
  if (!(p_drop >= 0.f && p_drop < 1.f)) return SDRM_ERR_SHAPE;   // (a NaN fails both compares)
  const double p = (double)p_drop;
  if (thr) *thr = (uint32_t)std::floor(p * 4294967296.0);
  if (scale) *scale = (float)(1.0 / (1.0 - p));
  return SDRM_OK;
}

namespace {

DropArgs drop_args(uint64_t seed, uint32_t step, uint32_t thr) {
  DropArgs d;
  d.k0 = (uint32_t)seed; d.k1 = (uint32_t)(seed >> 32); d.step = step; d.thr = thr;
  return d;
}

int launch_input_wgrad(sdrm_engine* e, void (*kernel)(const InputWgradArgs), dim3 grid, size_t lds, const InputWgradArgs& a, hipStream_t st) {
  // the kernel's static LDS (the chunk, 2 KB) comes on top of the tile
  if (const hipError_t rc = allow_full_lds(reinterpret_cast<const void*>(kernel), LDS_MAX_BYTES - 4096)) return hip_rc(e, "k_input_wgrad", rc);
  return launch_k(e, PC_INPUT_LAYER, "k_input_wgrad", kernel, grid, dim3(256), lds, st, a);
}

}  // namespace

int sdrm_vae_input_layer_fwd(sdrm_engine* e, const float* w1, const float* b1, int n_items, int hidden, const int64_t* indptr,
                             const int32_t* indices, const float* data, int64_t n_rows, const int64_t* rows, int64_t row0, int b,
                             uint64_t seed, uint32_t step, float p_drop, float* pre, float* rowscale, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!w1 || !b1 || !pre || !rowscale) return fail(e, SDRM_ERR_ARG, "sdrm_vae_input_layer_fwd: null pointer");
  InputFwdArgs a{};
  if (int rc = csr_batch(e, "sdrm_vae_input_layer_fwd", indptr, indices, data, n_rows, rows, row0, b, n_items, &a.csr)) return rc;
  uint32_t thr;
  float scale;
  if (int rc = sdrm_debug_input_layer_args(n_items, hidden, n_rows, row0, b, rows == nullptr, p_drop, &thr, &scale))
    return fail(e, rc, "sdrm_vae_input_layer_fwd: n_items outside 1 .. 2^20, hidden outside 1 .. 4096, n_rows outside 1 .. 2^31 - 1, b outside "
                       "1 .. 2^22, row0 < 0, rows row0 .. row0 + b - 1 end behind the matrix, or p_drop outside [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const int Hq = vae_dims(n_items, hidden, 0, b).Hq;
  float* w1t;
  if (int rc = scratch(e, SCR_IL_W1T, (size_t)n_items * Hq, &w1t)) return rc;
  // W1 changes with every optimiser step: the transposed copy is this call's
  if (int rc = launch_w1t(e, PC_NONE, w1, hidden, n_items, w1t, Hq, st)) return rc;
  a.w1t = w1t; a.b1 = b1; a.hidden = hidden; a.Hq = Hq;
  a.drop = drop_args(seed, step, thr); a.scale = scale; a.pre = pre; a.rowscale = rowscale;
  return launch_gather_rows(e, PC_INPUT_LAYER, "k_input_fwd", Hq / 4, a, st, [](auto tpr, auto nv, auto u) { return k_input_fwd<VAL(tpr), VAL(nv), VAL(u)>; });
}

int sdrm_vae_input_layer_wgrad(sdrm_engine* e, const float* dpre, const float* rowscale, int hidden, const int64_t* colptr,
                               const int32_t* rowidx, const float* data, int64_t n_rows, int n_items, const int32_t* pos, int64_t lo,
                               int b, uint64_t seed, uint32_t step, float p_drop, float* dw1, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!dpre || !rowscale || !colptr || !rowidx || !dw1) return fail(e, SDRM_ERR_ARG, "sdrm_vae_input_layer_wgrad: null pointer");
  uint32_t thr;
  float scale;
  if (int rc = sdrm_debug_input_layer_args(n_items, hidden, n_rows, lo, b, 1, p_drop, &thr, &scale))
    return fail(e, rc, "sdrm_vae_input_layer_wgrad: n_items outside 1 .. 2^20, hidden outside 1 .. 4096, n_rows outside 1 .. 2^31 - 1, b outside "
                       "1 .. 2^22, lo < 0, places lo .. lo + b - 1 end behind the feed, or p_drop outside [0, 1)");
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const int Hq = vae_dims(n_items, hidden, 0, b).Hq, q = Hq / 4;
  InputWgradArgs a{};
  a.dpre = dpre; a.ldd = hidden;
  if ((hidden & 3) || ((uintptr_t)dpre & 15u)) {   // rows off the 16-byte grid: a padded copy [b][Hq]
    float* dp;
    if (int rc = scratch(e, SCR_IL_DPRE, (size_t)b * Hq, &dp)) return rc;
    PadList pad;
    pad.add(dpre, b, hidden, dp, b, Hq);
    if (int rc = pad.launch(e, PC_NONE, st)) return rc;
    a.dpre = dp; a.ldd = Hq;
  }
  a.rowscale = rowscale; a.colptr = colptr; a.rowidx = rowidx; a.data = data; a.pos = pos; a.lo = lo; a.n_rows = n_rows; a.b = b;
  a.n_items = n_items; a.hidden = hidden; a.Hq = Hq; a.flag = e->feed_flag; a.drop = drop_args(seed, step, thr); a.dw1 = dw1;
  const unsigned tiles = (unsigned)((n_items + IL_CT - 1) / IL_CT);
  // the LDS tile [16][ld]: ld = the pass's share of Hq + 4 floats (<= 131 KB at 2048 of them)
  const auto lds = [&](int span) { return (size_t)IL_CT * (size_t)(std::min(Hq, span) + 4) * sizeof(float); };
  if (q <= 64) return launch_input_wgrad(e, k_input_wgrad<64, 1, 4>, dim3(tiles, 1), lds(256), a, st);      // one wave per column
  if (q <= 256) return launch_input_wgrad(e, k_input_wgrad<256, 1, 4>, dim3(tiles, 1), lds(1024), a, st);   // the work-group per column
  return launch_input_wgrad(e, k_input_wgrad<256, 2, 2>, dim3(tiles, (unsigned)((Hq + 2047) / 2048)), lds(2048), a, st);
}

// ---------------------------------------------------------------------------------------------
// Per-user hold-out split of the VAE pre-stage's evaluation half (utilities.py:174-236), csrc/holdout.h.

// The host side that needs no device: the envelope, and m_u of a row of n_u entries.
int sdrm_debug_holdout_args(int n_items, int64_t n_rows, int64_t nnz, double test_prop, int64_t n_u, int64_t* m_out) {
  if (n_items < 1 || n_items > MAX_ITEMS || n_rows < 1 || n_rows > (int64_t)INT32_MAX || nnz < 0 || nnz >= ((int64_t)1 << 40))
    return SDRM_ERR_SHAPE;
  if (!(test_prop > 0.0 && test_prop < 1.0)) return SDRM_ERR_SHAPE;   // (a NaN fails both compares)
  if (m_out) *m_out = holdout_m(test_prop, n_u);
  return SDRM_OK;
}

int sdrm_holdout_split(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, int64_t n_rows, int n_items, int64_t nnz,
                       double test_prop, uint64_t seed, uint32_t draw, int64_t* train_indptr, int32_t* train_indices,
                       int64_t* held_indptr, int32_t* held_indices, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !train_indptr || !train_indices || !held_indptr || !held_indices)
    return fail(e, SDRM_ERR_ARG, "sdrm_holdout_split: null pointer");
  if (int rc = sdrm_debug_holdout_args(n_items, n_rows, nnz, test_prop, 0, nullptr))
    return fail(e, rc, "sdrm_holdout_split: n_items outside 1 .. 2^20, n_rows outside 1 .. 2^31 - 1, nnz outside 0 .. 2^40 - 1 or test_prop outside (0, 1)");
  hipStream_t st = (hipStream_t)stream;
  HoldoutArgs a{};
  if (int rc = scratch(e, SCR_HOLD_CNT, 2 * (size_t)n_rows, &a.cnt)) return rc;
  a.indptr = indptr; a.indices = indices; a.n_rows = n_rows; a.nnz = nnz; a.n_items = n_items; a.test_prop = test_prop;
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.draw = draw;
  a.train_indptr = train_indptr; a.train_indices = train_indices; a.held_indptr = held_indptr; a.held_indices = held_indices;
  a.flag = e->feed_flag;
  const unsigned waves = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 1 << 20);   // the kernels stride over the rows behind their grids
  const unsigned groups = (unsigned)std::min<int64_t>(n_rows, 1 << 16);
  return hip_rc(e, "k_holdout_split", profiled(e, PC_HOLDOUT, 0.0, st, [&] {
    SDRM_LAUNCH(e, k_holdout_counts, dim3(waves), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_holdout_scan, dim3(2), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_holdout_split<64>, dim3(waves), dim3(256), 0, st, a);    // rows of at most HOLD_WAVE_MAX entries: a wave each
    SDRM_LAUNCH(e, k_holdout_split<256>, dim3(groups), dim3(256), 0, st, a);  // longer rows: a work-group each
    return hipGetLastError();
  }));
}

int sdrm_equal_sparsity(sdrm_engine* e, const float* x, int64_t n, double q, uint8_t* out, float* threshold, void* stream) {
  if (!e || !x) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity: null pointer");
  if (n < 1) return fail(e, SDRM_ERR_SHAPE, "sdrm_equal_sparsity: n < 1");
  if (!(q >= 0.0 && q <= 1.0)) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity: q outside [0,1]");
  if (((uintptr_t)x & 15u) || (out && ((uintptr_t)out & 3u)))
    return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity: x must be 16-byte and out 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  int64_t r0, r1;
  float gamma;
  quantile_ranks(n, q, r0, r1, gamma);
  if (int rc = launch_k(e, PC_NONE, "k_select_init", k_select_init, dim3(8), dim3(256), 0, st, e->sel, r0, r1)) return rc;
  return select_and_binarize(e, x, n, gamma, out, threshold, st);
}

// ---------------------------------------------------------------------------------------------
// The same result as a canonical CSR matrix made on the device, either side (main.py:177-180, :259-270), csrc/compact.h.
int sdrm_equal_sparsity_csr_begin(sdrm_engine* e, const float* x, int64_t n_rows, int64_t n_cols, double q, int side,
                                  int64_t* indptr, float* threshold, int64_t* nnz_host, void* stream) {
  // (the handle is looked at last: every refusal below can be had without a device)
  if (!x || !indptr || !nnz_host) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_begin: null pointer");
  if (n_rows < 1 || n_cols < 1 || n_cols >= ((int64_t)1 << 31))
    return fail(e, SDRM_ERR_SHAPE, "sdrm_equal_sparsity_csr_begin: n_rows < 1 or n_cols outside [1, 2^31)");
  if (!(q >= 0.0 && q <= 1.0)) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_begin: q outside [0,1]");
  if (side != 0 && side != 1) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_begin: side is 0 (>=) or 1 (<=)");
  if ((uintptr_t)x & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_begin: x must be 16-byte aligned");
  const int64_t wpr = (n_cols + 63) / 64;
  if (n_rows > (((int64_t)1 << 31) - 256) / wpr)   // the mask is indexed with 32 bits (2^31 words: a matrix of 512 GB and more)
    return fail(e, SDRM_ERR_SHAPE, "sdrm_equal_sparsity_csr_begin: more than 2^31 mask words");
  if (!e) return SDRM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  e->csr.active = false;   // a second begin replaces a pending one
  const size_t words = (size_t)(n_rows * wpr), off_ptr = words, off_cnt = off_ptr + (size_t)n_rows + 1;
  const size_t need = off_cnt + ((size_t)n_rows + 1) / 2;
  uint64_t* ws;
  if (int rc = scratch(e, SCR_CSR_WS, need, &ws)) return rc;
  if (!e->csr_nnz_host) {
    HIP_TRY(e, hipHostMalloc((void**)&e->csr_nnz_host, sizeof(int64_t), hipHostMallocMapped));
    HIP_TRY(e, hipHostGetDevicePointer((void**)&e->csr_nnz_dev, e->csr_nnz_host, 0));
  }
  const int64_t n = n_rows * n_cols;
  int64_t r0, r1;
  float gamma;
  quantile_ranks(n, q, r0, r1, gamma);
  if (int rc = launch_k(e, PC_NONE, "k_select_init", k_select_init, dim3(8), dim3(256), 0, st, e->sel, r0, r1)) return rc;
  if (int rc = select_and_binarize(e, x, n, gamma, nullptr, threshold, st)) return rc;
  uint32_t* counts = reinterpret_cast<uint32_t*>(ws + off_cnt);
  int64_t* own = reinterpret_cast<int64_t*>(ws + off_ptr);
  HIP_TRY(e, hipMemsetAsync(counts, 0, (size_t)n_rows * sizeof(uint32_t), st));
  const dim3 grid((unsigned)((words + 4 * CSR_MASK_WORDS - 1) / (4 * CSR_MASK_WORDS)));   // four waves per work-group
  if (int rc = launch_k(e, PC_NONE, "k_csr_mask", side == 0 ? k_csr_mask<0> : k_csr_mask<1>, grid, dim3(256), 0, st, x, (int)n_cols, (int)wpr,
                        (uint32_t)words, &e->sel->threshold, ws, counts))
    return rc;
  *e->csr_nnz_host = -1;
  if (int rc = launch_k(e, PC_NONE, "k_csr_scan", k_csr_scan, dim3(1), dim3(256), 0, st, counts, n_rows, own, indptr, e->csr_nnz_dev)) return rc;
  HIP_TRY(e, hipStreamSynchronize(st));
  const int64_t nnz = *(volatile int64_t*)e->csr_nnz_host;
  if (nnz < 0 || nnz > n) return fail(e, SDRM_ERR_STATE, "sdrm_equal_sparsity_csr_begin: the row counts do not add up");
  *nnz_host = nnz;
  e->csr.active = true; e->csr.n_rows = n_rows; e->csr.nnz = nnz; e->csr.wpr = (int)wpr; e->csr.off_ptr = off_ptr;
  return SDRM_OK;
}

int sdrm_equal_sparsity_csr_end(sdrm_engine* e, int32_t* indices, int64_t capacity, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!e->csr.active) return fail(e, SDRM_ERR_STATE, "sdrm_equal_sparsity_csr_end: no sdrm_equal_sparsity_csr_begin is pending");
  // (a refused call leaves the begin pending: the caller may come back with a buffer that fits)
  if (capacity < e->csr.nnz) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_end: capacity < nnz");
  if (!indices && e->csr.nnz > 0) return fail(e, SDRM_ERR_ARG, "sdrm_equal_sparsity_csr_end: null pointer");
  const auto& c = e->csr;
  if (c.nnz > 0) {
    const uint64_t* ws = scratch_at<uint64_t>(e, SCR_CSR_WS);
    const int64_t* own = reinterpret_cast<const int64_t*>(ws + c.off_ptr);
    // rows per work-group: 4 (a wave per row) for the wide matrices (3125 columns: 49 words, 8582: 135), 16 for rows of at most 32 words
    // (843 x 1008: 16 words), where a wave per row would leave three lanes in four without a word
    const int rpw = c.wpr > 32 ? 4 : 16;
    const unsigned blocks = (unsigned)std::min<int64_t>((c.n_rows + rpw - 1) / rpw, 65536);
    if (int rc = launch_k(e, PC_NONE, "k_csr_fill", c.wpr > 32 ? k_csr_fill<64> : k_csr_fill<16>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, ws,
                          own, c.n_rows, c.wpr, indices, c.nnz))
      return rc;
  }
  e->csr.active = false;
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// A device CSR to its CSC form, and CSR parts one under the other (csrc/csr_transpose.h).

// The host side that needs no device: the envelope of sdrm_csr_transpose.
int sdrm_debug_csr_transpose_args(int64_t m, int64_t n, int64_t capacity) {
  if (m < 1 || m > CSRT_MAX_DIM || n < 1 || n > CSRT_MAX_DIM || capacity < 0 || capacity >= ((int64_t)1 << 40)) return SDRM_ERR_SHAPE;
  if (((m + 63) / 64) * n > CSRT_MAX_WORDS) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_csr_transpose(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t n_cols,
                       int64_t capacity, int64_t* colptr, int32_t* rowidx, float* cdata, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !colptr || !rowidx) return fail(e, SDRM_ERR_ARG, "sdrm_csr_transpose: null pointer");
  if ((data == nullptr) != (cdata == nullptr)) return fail(e, SDRM_ERR_ARG, "sdrm_csr_transpose: the values of the input and of the output go together");
  if (int rc = sdrm_debug_csr_transpose_args(n_rows, n_cols, capacity))
    return fail(e, rc, "sdrm_csr_transpose: n_rows or n_cols outside 1 .. 2^22, capacity outside 0 .. 2^40 - 1, or ceil(n_rows / 64) x n_cols above 2^26 "
                       "(the bit table's envelope: Engine.csc_to_device takes such a matrix on the host)");
  hipStream_t st = (hipStream_t)stream;
  const size_t blocks = (size_t)((n_rows + 63) / 64), words = blocks * (size_t)n_cols;
  const size_t off_table = 2, off_ptr = off_table + words, off_off = off_ptr + (size_t)n_cols + 1, off_cnt = off_off + (words + 1) / 2;
  uint64_t* ws;
  if (int rc = scratch(e, SCR_CSRT_WS, off_cnt + ((size_t)n_cols + 1) / 2, &ws)) return rc;
  int64_t* own = reinterpret_cast<int64_t*>(ws + off_ptr);
  CsrTransposeArgs a{};
  a.csr = CsrBatch{indptr, indices, data, nullptr, 0, n_rows, (int)n_rows, (int)n_cols, e->feed_flag};
  a.capacity = capacity;
  a.checked = reinterpret_cast<unsigned long long*>(ws);
  a.total = reinterpret_cast<const int64_t*>(ws + 1);
  a.table = ws + off_table;
  a.off = reinterpret_cast<uint32_t*>(ws + off_off);
  a.counts = reinterpret_cast<uint32_t*>(ws + off_cnt);
  a.colptr = own;
  a.blocks = (int)blocks;
  a.rowidx = rowidx; a.cdata = cdata;
  // The count of checked entries, the total and the bit table are this call's own, made anew on the stream every time: the LDS-tile
  // form of the mark pass stores every word of the table, the global-atomic form ORs into a cleared one.
  const int64_t tiles = (n_cols + CSRT_TILE - 1) / CSRT_TILE;
  const bool lds = e->csrt_mark_mode == 2 || (e->csrt_mark_mode == 0 && tiles <= CSRT_LDS_MAX_TILES);
  HIP_TRY(e, hipMemsetAsync(ws, 0, off_table * sizeof(uint64_t), st));
  const unsigned waves = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 1 << 16);   // the row kernels stride over the rows behind their grids
  HIP_TRY(e, profiled(e, PC_CSRT_MARK, 0.0, st, [&] {   // (the clearing is the global form's cost: inside its interval)
    if (lds) {
      SDRM_LAUNCH(e, k_csrt_mark_lds, dim3((unsigned)blocks, (unsigned)tiles), dim3(256), 0, st, a);
    } else {
      const hipError_t rc = hipMemsetAsync(a.table, 0, words * sizeof(uint64_t), st);
      if (rc != hipSuccess) return rc;
      SDRM_LAUNCH(e, k_csrt_mark, dim3(waves), dim3(256), 0, st, a);
    }
    return hipGetLastError();
  }));
  if (int rc = launch_k(e, PC_CSRT_COLSCAN, "k_csrt_colscan", k_csrt_colscan, dim3((unsigned)((n_cols + 255) / 256)), dim3(256), 0, st, a)) return rc;
  if (int rc = launch_k(e, PC_CSRT_SCAN, "k_csr_scan", k_csr_scan, dim3(1), dim3(256), 0, st, a.counts, n_cols, own, colptr,
                        reinterpret_cast<int64_t*>(ws + 1)))
    return rc;
  return launch_k(e, PC_CSRT_FILL, "k_csrt_fill", k_csrt_fill, dim3(waves), dim3(256), 0, st, a);
}

int sdrm_csr_vstack(sdrm_engine* e, const sdrm_csr_part* parts, int n_parts, int n_cols, int64_t* indptr_out, int32_t* indices_out,
                    float* data_out, int64_t capacity_out, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!parts || !indptr_out || !indices_out) return fail(e, SDRM_ERR_ARG, "sdrm_csr_vstack: null pointer");
  if (n_parts < 1 || n_parts > CSR_STACK_MAX) return fail(e, SDRM_ERR_SHAPE, "sdrm_csr_vstack: n_parts outside 1 .. 8");
  if (n_cols < 1 || n_cols > CSRT_MAX_DIM) return fail(e, SDRM_ERR_SHAPE, "sdrm_csr_vstack: n_cols outside 1 .. 2^22");
  CsrStackArgs a{};
  int64_t rows = 0, cap = 0;
  bool values = false;
  for (int k = 0; k < n_parts; ++k) {
    const sdrm_csr_part& p = parts[k];
    if (!p.indptr || !p.indices) return fail(e, SDRM_ERR_ARG, "sdrm_csr_vstack: null pointer in a part");
    if (p.n_rows < 0 || p.n_rows > CSRT_MAX_DIM || p.capacity < 0 || p.capacity >= ((int64_t)1 << 40))
      return fail(e, SDRM_ERR_SHAPE, "sdrm_csr_vstack: a part's n_rows outside 0 .. 2^22 or its capacity outside 0 .. 2^40 - 1");
    a.part[k] = CsrStackPart{p.indptr, p.indices, p.data, p.capacity};
    a.first[k] = rows;
    rows += p.n_rows; cap += p.capacity;
    values |= p.data != nullptr;
  }
  for (int k = n_parts; k <= CSR_STACK_MAX; ++k) a.first[k] = rows;
  if (rows < 1 || rows > CSRT_MAX_DIM) return fail(e, SDRM_ERR_SHAPE, "sdrm_csr_vstack: total rows outside 1 .. 2^22");
  if (capacity_out < cap) return fail(e, SDRM_ERR_SHAPE, "sdrm_csr_vstack: capacity_out below the sum of the parts' capacities");
  if (values != (data_out != nullptr))
    return fail(e, SDRM_ERR_ARG, "sdrm_csr_vstack: data_out is required when a part has values, and null when none has");
  hipStream_t st = (hipStream_t)stream;
  const size_t off_ptr = 1, off_cnt = off_ptr + (size_t)rows + 1;
  uint64_t* ws;
  if (int rc = scratch(e, SCR_STACK_WS, off_cnt + ((size_t)rows + 1) / 2, &ws)) return rc;
  int64_t* own = reinterpret_cast<int64_t*>(ws + off_ptr);
  a.n_parts = n_parts; a.n_cols = n_cols;
  a.cnt = reinterpret_cast<uint32_t*>(ws + off_cnt);
  a.rowptr = own;
  a.indices_out = indices_out; a.data_out = data_out; a.capacity_out = capacity_out;
  a.flag = e->feed_flag;
  const unsigned waves = (unsigned)std::min<int64_t>((rows + 3) / 4, 1 << 16);
  return hip_rc(e, "k_stack_copy", profiled(e, PC_CSR_VSTACK, 0.0, st, [&] {
    SDRM_LAUNCH(e, k_stack_counts, dim3(waves), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_csr_scan, dim3(1), dim3(256), 0, st, (const uint32_t*)a.cnt, rows, own, indptr_out, reinterpret_cast<int64_t*>(ws));
    SDRM_LAUNCH(e, k_stack_copy, dim3(waves), dim3(256), 0, st, a);
    return hipGetLastError();
  }));
}

// ---------------------------------------------------------------------------------------------
// The NeuMF evaluator's triples from device CSR parts (main.py:218-283), csrc/neumf_triples.h.

// The host side that needs no device: everything sdrm_neumf_triples refuses but the handle and the two output pointers.
int sdrm_debug_neumf_triples_args(const sdrm_triple_part* parts, int n_parts, int n_items, int64_t capacity_out) {
  if (!parts) return SDRM_ERR_ARG;
  if (n_parts < 1 || n_parts > CSR_STACK_MAX) return SDRM_ERR_SHAPE;
  if (n_items < 1 || n_items > CSRT_MAX_DIM) return SDRM_ERR_SHAPE;
  int64_t rows = 0, cap = 0;
  for (int k = 0; k < n_parts; ++k) {
    const sdrm_triple_part& p = parts[k];
    if (p.n_rows < 0 || p.n_rows > CSRT_MAX_DIM || p.capacity < 0 || p.capacity > TRIPLE_MAX_OUT) return SDRM_ERR_SHAPE;
    if (!p.indptr || (!p.indices && p.capacity > 0)) return SDRM_ERR_ARG;
    if (p.label != 0 && p.label != 1) return SDRM_ERR_SHAPE;
    if (p.user0 < 0 || (int64_t)p.user0 + p.n_rows > (int64_t)0x7fffffff) return SDRM_ERR_SHAPE;
    rows += p.n_rows; cap += p.capacity;
  }
  if (rows < 1 || rows > CSRT_MAX_DIM) return SDRM_ERR_SHAPE;
  if (capacity_out < cap || capacity_out > TRIPLE_MAX_OUT) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_neumf_triples(sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, int32_t* triples_out, int64_t capacity_out,
                       uint8_t* item_present, int64_t* counts_dev, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!parts || !triples_out || !counts_dev) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_triples: null pointer");
  if (int rc = sdrm_debug_neumf_triples_args(parts, n_parts, n_items, capacity_out))
    return fail(e, rc, rc == SDRM_ERR_ARG ? "sdrm_neumf_triples: a part without indptr, or without indices and capacity > 0"
                                          : "sdrm_neumf_triples: n_parts outside 1 .. 8, n_items or total rows outside 1 .. 2^22, a label outside {0, 1}, user0 < 0 or "
                                            "user0 + n_rows above 2^31 - 1, a part's n_rows or capacity out of range, or capacity_out below the sum of the "
                                            "parts' capacities or above 2^30");
  TripleArgs a{};
  int64_t rows = 0;
  for (int k = 0; k < n_parts; ++k) {
    const sdrm_triple_part& p = parts[k];
    a.part[k] = TriplePart{p.indptr, p.indices, p.n_rows, p.capacity, p.user0, p.label};
    a.first[k] = rows;
    rows += p.n_rows;
  }
  for (int k = n_parts; k <= CSR_STACK_MAX; ++k) a.first[k] = rows;
  hipStream_t st = (hipStream_t)stream;
  const size_t off_base = 1, off_copy = off_base + (size_t)rows + 1, off_cnt = off_copy + (size_t)rows + 1, words = off_cnt + ((size_t)rows + 1) / 2;
  uint64_t* ws;
  if (int rc = scratch(e, SCR_TRIPLE_WS, words, &ws)) return rc;
  int64_t* base = reinterpret_cast<int64_t*>(ws + off_base);
  a.n_parts = n_parts; a.n_items = n_items;
  a.cnt = reinterpret_cast<uint32_t*>(ws + off_cnt);
  a.base = base;
  a.out = triples_out; a.capacity_out = capacity_out;
  a.present = item_present;
  a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
  a.flag = e->feed_flag;
  const unsigned waves = (unsigned)std::min<int64_t>((rows + 3) / 4, 1 << 16);
  const unsigned groups = (unsigned)((rows + TRIPLE_ROWS - 1) / TRIPLE_ROWS);   // (at most 2^18)
  return hip_rc(e, "k_triple_fill", profiled(e, PC_NEUMF_TRIPLES, 0.0, st, [&] {
    // the scratch, the counts and the item bytes are this call's own, made anew on the stream every time
    hipError_t rc = hipMemsetAsync(ws, 0, words * sizeof(uint64_t), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), st);
    if (rc == hipSuccess && item_present) rc = hipMemsetAsync(item_present, 0, (size_t)n_items, st);
    if (rc != hipSuccess) return rc;
    SDRM_LAUNCH(e, k_triple_counts, dim3(waves), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_csr_scan, dim3(1), dim3(256), 0, st, (const uint32_t*)a.cnt, rows, base, reinterpret_cast<int64_t*>(ws + off_copy),
                reinterpret_cast<int64_t*>(ws));
    SDRM_LAUNCH(e, k_triple_fill, dim3(groups), dim3(256), 0, st, a);
    return hipGetLastError();
  }));
}

// ---------------------------------------------------------------------------------------------
// The NeuMF evaluator's ranking problem from device CSR parts and held-out triples (neural_cf_benchmark_pt.py:294-326), csrc/neumf_rank.h.

// The host side that needs no device: everything sdrm_neumf_rank_problem refuses but the handle and the data pointers beside the parts'.
int sdrm_debug_neumf_rank_args(const sdrm_triple_part* parts, int n_parts, int n_items, int64_t n_heldout, int64_t n_rows, int64_t capacity_cols,
                               int64_t capacity_seen, int64_t capacity_relevant) {
  if (!parts) return SDRM_ERR_ARG;
  if (n_parts < 1 || n_parts > CSR_STACK_MAX) return SDRM_ERR_SHAPE;
  if (n_items < 1 || n_items > RANKP_MAX_DIM) return SDRM_ERR_SHAPE;
  if (n_rows < 1 || n_rows > RANKP_MAX_DIM) return SDRM_ERR_SHAPE;
  if (n_heldout < 0 || n_heldout > RANKP_MAX_HELD) return SDRM_ERR_SHAPE;
  if (n_rows * (((int64_t)n_items + 63) / 64) * 8 > RANKP_MAX_TABLE) return SDRM_ERR_SHAPE;
  int64_t rows = 0, cap = 0;
  for (int k = 0; k < n_parts; ++k) {
    const sdrm_triple_part& p = parts[k];
    if (p.n_rows < 0 || p.n_rows > RANKP_MAX_DIM || p.capacity < 0 || p.capacity > TRIPLE_MAX_OUT) return SDRM_ERR_SHAPE;
    if (!p.indptr || (!p.indices && p.capacity > 0)) return SDRM_ERR_ARG;
    if (p.label != 0 && p.label != 1) return SDRM_ERR_SHAPE;
    if (p.user0 < 0 || (int64_t)p.user0 + p.n_rows > (int64_t)0x7fffffff) return SDRM_ERR_SHAPE;
    rows += p.n_rows; cap += p.capacity;
  }
  if (rows < 1 || rows > RANKP_MAX_DIM) return SDRM_ERR_SHAPE;
  if (capacity_cols < n_items || capacity_seen < cap || capacity_relevant < n_heldout) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_neumf_rank_problem(sdrm_engine* e, const sdrm_triple_part* parts, int n_parts, int n_items, const uint8_t* item_present,
                            const int32_t* heldout, int64_t n_heldout, int64_t n_rows, int32_t* cols_out, int64_t capacity_cols,
                            int64_t* seen_indptr, int32_t* seen_indices, int64_t capacity_seen, int64_t* relevant_indptr,
                            int32_t* relevant_indices, int64_t capacity_relevant, int64_t* counts_dev, void* stream) {
  const char* who = "sdrm_neumf_rank_problem";
  if (!e) return SDRM_ERR_ARG;
  if (!parts || !item_present || !cols_out || !seen_indptr || !seen_indices || !relevant_indptr || !relevant_indices || !counts_dev ||
      (!heldout && n_heldout > 0))
    return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (int rc = sdrm_debug_neumf_rank_args(parts, n_parts, n_items, n_heldout, n_rows, capacity_cols, capacity_seen, capacity_relevant))
    return fail(e, rc, std::string(who) + (rc == SDRM_ERR_ARG ? ": a part without indptr, or without indices and capacity > 0"
                                                                : ": n_parts outside 1 .. 8, n_items, n_rows or the parts' total rows outside 1 .. 2^22, a bit table "
                                                                  "n_rows x ceil(n_items / 64) x 8 above 2^31 bytes, n_heldout outside 0 .. 2^30, a part as "
                                                                  "sdrm_neumf_triples refuses it, or a capacity below n_items (cols), the sum of the parts' capacities "
                                                                  "(seen) or n_heldout (relevant)"));
  RankProblemArgs a{};
  int64_t rows = 0;
  for (int k = 0; k < n_parts; ++k) {
    const sdrm_triple_part& p = parts[k];
    a.part[k] = TriplePart{p.indptr, p.indices, p.n_rows, p.capacity, p.user0, p.label};
    a.first[k] = rows;
    rows += p.n_rows;
  }
  for (int k = n_parts; k <= CSR_STACK_MAX; ++k) a.first[k] = rows;
  hipStream_t st = (hipStream_t)stream;
  const int wpr = (n_items + 63) / 64;
  const size_t table = (size_t)n_rows * (size_t)wpr, ptr = (size_t)n_rows + 1, cnt = ((size_t)n_rows + 1) / 2;
  const size_t off_tab = 2, off_ptr = off_tab + 2 * table, off_cnt = off_ptr + 2 * ptr, off_col = off_cnt + 2 * cnt;
  const size_t words = off_col + ((size_t)n_items + 1) / 2;
  uint64_t* ws;
  if (int rc = scratch(e, SCR_RANK_WS, words, &ws)) return rc;
  a.n_parts = n_parts; a.n_items = n_items; a.flag = e->feed_flag;
  a.n_rows = n_rows; a.wpr = wpr;
  a.present = item_present; a.held = heldout; a.n_held = n_heldout;
  int64_t* own[2];
  for (int t = 0; t < 2; ++t) {
    a.table[t] = ws + off_tab + (size_t)t * table;
    own[t] = reinterpret_cast<int64_t*>(ws + off_ptr + (size_t)t * ptr);
    a.own[t] = own[t];
    a.cnt[t] = reinterpret_cast<uint32_t*>(ws + off_cnt + (size_t)t * cnt);
  }
  a.col_of = reinterpret_cast<int32_t*>(ws + off_col);
  a.cols = cols_out;
  a.indices[0] = seen_indices; a.capacity[0] = capacity_seen;
  a.indices[1] = relevant_indices; a.capacity[1] = capacity_relevant;
  a.counts = reinterpret_cast<unsigned long long*>(counts_dev);
  const unsigned part_waves = (unsigned)std::min<int64_t>((rows + 3) / 4, 1 << 16);
  const unsigned row_waves = (unsigned)std::min<int64_t>((n_rows + 3) / 4, 1 << 16);
  const unsigned count_waves = (unsigned)std::min<int64_t>((2 * n_rows + 3) / 4, 1 << 16);
  return hip_rc(e, "k_rank_fill", profiled(e, PC_NEUMF_RANK_PROBLEM, 0.0, st, [&] {
    // the scratch (the two bit tables first of all) and the counts are this call's own, made anew on the stream every time
    hipError_t rc = hipMemsetAsync(ws, 0, words * sizeof(uint64_t), st);
    if (rc == hipSuccess) rc = hipMemsetAsync(counts_dev, 0, 4 * sizeof(int64_t), st);
    if (rc != hipSuccess) return rc;
    SDRM_LAUNCH(e, k_rank_cols, dim3(1), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_rank_mark_parts, dim3(part_waves), dim3(256), 0, st, a);
    if (n_heldout > 0) SDRM_LAUNCH(e, k_rank_mark_held, dim3((unsigned)((n_heldout + 255) / 256)), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_rank_counts, dim3(count_waves), dim3(256), 0, st, a);
    SDRM_LAUNCH(e, k_csr_scan, dim3(1), dim3(256), 0, st, (const uint32_t*)a.cnt[0], n_rows, own[0], seen_indptr, reinterpret_cast<int64_t*>(ws));
    SDRM_LAUNCH(e, k_csr_scan, dim3(1), dim3(256), 0, st, (const uint32_t*)a.cnt[1], n_rows, own[1], relevant_indptr, reinterpret_cast<int64_t*>(ws + 1));
    SDRM_LAUNCH(e, k_rank_fill, dim3(row_waves, 2), dim3(256), 0, st, a);
    return hipGetLastError();
  }));
}

int sdrm_neumf_rank_users(sdrm_engine* e, const uint8_t* mask, int64_t n_rows, int32_t* users_out, int64_t* count_dev, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!mask || !users_out || !count_dev) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_rank_users: null pointer");
  if (n_rows < 1 || n_rows > RANKP_MAX_DIM) return fail(e, SDRM_ERR_SHAPE, "sdrm_neumf_rank_users: n_rows outside 1 .. 2^22");
  return launch_k(e, PC_NEUMF_RANK_USERS, "k_rank_users", k_rank_users, dim3(1), dim3(256), 0, (hipStream_t)stream, mask, n_rows, users_out,
                  reinterpret_cast<unsigned long long*>(count_dev));
}

// ---------------------------------------------------------------------------------------------
// Recall@k / NDCG@k against held-out interactions (utilities.py:116-171), csrc/rank.h.
int sdrm_rank_metrics(sdrm_engine* e, const float* scores, int U, int I, const int64_t* held_indptr,
                      const int32_t* held_indices, const int64_t* train_indptr, const int32_t* train_indices,
                      const int32_t* ks_host, int nk, const double* tp, const double* idcg, double* recall, double* ndcg,
                      void* stream) {
  if (!e || !scores || !held_indptr || !held_indices || !ks_host || !tp || !idcg || !recall || !ndcg)
    return fail(e, SDRM_ERR_ARG, "sdrm_rank_metrics: null pointer");
  if ((train_indptr == nullptr) != (train_indices == nullptr))
    return fail(e, SDRM_ERR_ARG, "sdrm_rank_metrics: train_indptr and train_indices go together");
  if (U < 1 || I < 1 || I > 36864) return fail(e, SDRM_ERR_SHAPE, "sdrm_rank_metrics: U < 1 or I outside [1, 36864]");
  if (nk < 1 || nk > RANK_MAX_NK) return fail(e, SDRM_ERR_ARG, "sdrm_rank_metrics: nk outside [1, 8]");
  RankArgs a{};
  a.scores = scores; a.U = U; a.I = I;
  a.held_indptr = held_indptr; a.held_indices = held_indices;
  a.train_indptr = train_indptr; a.train_indices = train_indices;
  a.nk = nk; a.kmax = 0;
  for (int q = 0; q < nk; ++q) {
    if (ks_host[q] < 1 || ks_host[q] > RANK_MAX_K || ks_host[q] > I)
      return fail(e, SDRM_ERR_ARG, "sdrm_rank_metrics: k outside [1, min(128, I)]");
    a.ks[q] = ks_host[q];
    if (ks_host[q] > a.kmax) a.kmax = ks_host[q];
  }
  a.tp = tp; a.idcg = idcg; a.recall = recall; a.ndcg = ndcg;
  const size_t lds = (size_t)I * sizeof(float);
  if (lds > 48 * 1024)
    HIP_TRY(e, hipFuncSetAttribute((const void*)k_rank_metrics, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  return launch_k(e, PC_NONE, "k_rank_metrics", k_rank_metrics, dim3(U), dim3(256), lds, (hipStream_t)stream, a);
}

// The same ranking with a row map into both matrices, every offset and column checked, and the NeuMF footing of the NDCG on request
// (k_rank_metrics_rows, csrc/neumf_rank.h).
int sdrm_rank_metrics_rows(sdrm_engine* e, const float* scores, int U, int I, const int32_t* rows, int64_t n_rows, const int64_t* held_indptr,
                           const int32_t* held_indices, int64_t held_nnz, const int64_t* train_indptr, const int32_t* train_indices,
                           int64_t train_nnz, const int32_t* ks_host, int nk, const double* tp, const double* idcg, double* recall, double* ndcg,
                           int full_idcg, void* stream) {
  const char* who = "sdrm_rank_metrics_rows";
  if (!e) return SDRM_ERR_ARG;
  if (!scores || !rows || !held_indptr || !held_indices || !ks_host || !tp || !idcg || !recall || !ndcg)
    return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if ((train_indptr == nullptr) != (train_indices == nullptr))
    return fail(e, SDRM_ERR_ARG, std::string(who) + ": train_indptr and train_indices go together");
  if (U < 1 || I < 1 || I > 36864) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": U < 1 or I outside [1, 36864]");
  if (n_rows < 1 || held_nnz < 0 || train_nnz < 0) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": n_rows < 1 or a negative index capacity");
  if (nk < 1 || nk > RANK_MAX_NK) return fail(e, SDRM_ERR_ARG, std::string(who) + ": nk outside [1, 8]");
  RankArgs a{};
  a.scores = scores; a.U = U; a.I = I;
  a.held_indptr = held_indptr; a.held_indices = held_indices;
  a.train_indptr = train_indptr; a.train_indices = train_indices;
  a.nk = nk; a.kmax = 0;
  for (int q = 0; q < nk; ++q) {
    if (ks_host[q] < 1 || ks_host[q] > RANK_MAX_K || ks_host[q] > I)
      return fail(e, SDRM_ERR_ARG, std::string(who) + ": k outside [1, min(128, I)]");
    a.ks[q] = ks_host[q];
    if (ks_host[q] > a.kmax) a.kmax = ks_host[q];
  }
  a.tp = tp; a.idcg = idcg; a.recall = recall; a.ndcg = ndcg;
  const RankCheck ck{held_nnz, train_nnz, e->feed_flag};
  const RankRows rm{rows, n_rows, full_idcg != 0};
  const size_t lds = (size_t)I * sizeof(float);
  if (lds > 48 * 1024) HIP_TRY(e, allow_full_lds((const void*)k_rank_metrics_rows, 36864 * (int)sizeof(float)));
  return launch_k(e, PC_RANK_ROWS, "k_rank_metrics_rows", k_rank_metrics_rows, dim3(U), dim3(256), lds, (hipStream_t)stream, a, ck, rm);
}

// ---------------------------------------------------------------------------------------------
// Rank-k truncated SVD of a sparse matrix and the scores of its reconstruction (svd_benchmark.py:17-70), csrc/svd_eval.h.
namespace {

constexpr int64_t SVD_MAX_DIM = (int64_t)1 << 22;
const char* const kSvdEnvelope = ": k outside 1 .. 22 (k + 10 columns must fit the panel of 32), min(m, n) < 32, m or n above 2^22, nnz outside 0 .. 2^40 - 1 "
                                 "or n_iter outside 0 .. 10000";

// the Gram partials with R^-1 behind them, and the status word: made once, at their fixed sizes
int svd_scratch(sdrm_engine* e, unsigned** flag) {
  double* part;
  if (int rc = scratch(e, SCR_SVD_PART, (size_t)(SVD_GRAM_PARTS + 1) * SVD_PW * SVD_PW, &part)) return rc;
  return scratch(e, SCR_SVD_FLAG, 4, flag);
}

// y [c.b][32] = (the rows of c) q
int svd_spmm(sdrm_engine* e, const CsrBatch& c, int64_t nnz, const float* q, float* y, hipStream_t st) {
  const SvdSpmmArgs a{c, nnz, q, y};
  return launch_k(e, PC_SVD_SPMM, "k_svd_spmm", k_svd_spmm, dim3((unsigned)((c.b + 31) / 32)), dim3(256), 0, st, a);
}

// y [rows][32] <- orth(y): CholeskyQR twice, three launches each
int svd_orth(sdrm_engine* e, float* y, int rows, hipStream_t st) {
  const int parts = std::min(SVD_GRAM_PARTS, (rows + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS);
  double* part = scratch_at<double>(e, SCR_SVD_PART);
  double* rinv = part + (size_t)SVD_GRAM_PARTS * SVD_PW * SVD_PW;
  for (int pass = 0; pass < 2; ++pass) {
    if (int rc = launch_k(e, PC_SVD_GRAM, "k_svd_gram", k_svd_gram, dim3((unsigned)parts), dim3(256), 0, st, y, rows, part)) return rc;
    if (int rc = launch_k(e, PC_SVD_CHOL, "k_svd_chol", k_svd_chol, dim3(1), dim3(256), 0, st, part, parts, rinv, scratch_at<unsigned>(e, SCR_SVD_FLAG)))
      return rc;
    if (int rc = launch_k(e, PC_SVD_APPLY, "k_svd_apply", k_svd_apply, dim3((unsigned)((rows + 31) / 32)), dim3(256), 0, st, y, rows, rinv)) return rc;
  }
  return SDRM_OK;
}

// Eigen-decomposition of the symmetric a [n][n] by cyclic Jacobi rotations (float64): the eigenvalues end on a's diagonal, column j of v
// is the eigenvector of a[j][j].
void jacobi_eigh(std::vector<double>& a, std::vector<double>& v, int n) {
  v.assign((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 64; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int p = 0; p < n; ++p) {
      diag += a[(size_t)p * n + p] * a[(size_t)p * n + p];
      for (int q = p + 1; q < n; ++q) off += a[(size_t)p * n + q] * a[(size_t)p * n + q];
    }
    if (!(off > 1e-32 * diag)) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double theta = (a[(size_t)q * n + q] - a[(size_t)p * n + p]) / (2.0 * apq);
        const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < n; ++k) {
          const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
          v[(size_t)k * n + p] = c * vkp - s * vkq;
          v[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
}

// The closing small problem on the host, float64: z [n][32] = A^T Y = B^T.  eigh(B B^T = z^T z), the top k eigenvectors u rotated into
// the rows z u of V and normalised (float32 [k][n]), sigma = sqrt(eigenvalue).  False when a direction has no length or is not finite.
bool svd_close(const std::vector<float>& z, int64_t n, int k, std::vector<float>& V, double* sigma) {
  std::vector<double> g((size_t)SVD_PW * SVD_PW, 0.0), u;
  for (int64_t r = 0; r < n; ++r) {
    const float* zr = &z[(size_t)r * SVD_PW];
    for (int i = 0; i < SVD_PW; ++i)
      for (int j = i; j < SVD_PW; ++j) g[(size_t)i * SVD_PW + j] += (double)zr[i] * (double)zr[j];
  }
  for (int i = 0; i < SVD_PW; ++i)
    for (int j = 0; j < i; ++j) g[(size_t)i * SVD_PW + j] = g[(size_t)j * SVD_PW + i];
  for (double x : g)
    if (!std::isfinite(x)) return false;
  jacobi_eigh(g, u, SVD_PW);
  int order[SVD_PW];
  for (int i = 0; i < SVD_PW; ++i) order[i] = i;
  std::stable_sort(order, order + SVD_PW, [&](int x, int y) { return g[(size_t)x * SVD_PW + x] > g[(size_t)y * SVD_PW + y]; });
  V.assign((size_t)k * n, 0.f);
  std::vector<double> row((size_t)n);
  for (int c = 0; c < k; ++c) {
    const int col = order[c];
    double norm2 = 0.0;
    for (int64_t r = 0; r < n; ++r) {
      double s = 0.0;
      for (int i = 0; i < SVD_PW; ++i) s += (double)z[(size_t)r * SVD_PW + i] * u[(size_t)i * SVD_PW + col];
      row[(size_t)r] = s;
      norm2 += s * s;
    }
    if (!(norm2 > 0.0) || !std::isfinite(norm2)) return false;
    const double inv = 1.0 / std::sqrt(norm2);
    for (int64_t r = 0; r < n; ++r) V[(size_t)c * n + r] = (float)(row[(size_t)r] * inv);
    sigma[c] = std::sqrt(std::max(g[(size_t)col * SVD_PW + col], 0.0));
  }
  return true;
}

const char* const kSvdBreakdown = ": breakdown - a panel of 32 columns became numerically dependent (a Cholesky pivot at or below 2^-40 of the "
                                  "largest diagonal entry of its Gram matrix): the matrix has numerical rank below 32, or holds values that are not finite";

// the fit's status word as it stands once `st` has drained; a raised one is cleared for the next call
int svd_breakdown(sdrm_engine* e, const char* who, hipStream_t st, unsigned flag) {
  if (!(flag & SVD_BREAKDOWN)) return SDRM_OK;
  HIP_TRY(e, hipMemsetAsync(scratch_at<unsigned>(e, SCR_SVD_FLAG), 0, sizeof(unsigned), st));
  return fail(e, SDRM_ERR_ARG, std::string(who) + kSvdBreakdown);
}

}  // namespace

// The host side that needs no device: the envelope of sdrm_svd_fit.
int sdrm_debug_svd_args(int64_t m, int64_t n, int64_t nnz, int k, int n_iter) {
  if (k < 1 || k + 10 > SVD_PW || std::min(m, n) < SVD_PW || m > SVD_MAX_DIM || n > SVD_MAX_DIM || nnz < 0 || nnz >= ((int64_t)1 << 40) ||
      n_iter < 0 || n_iter > 10000)
    return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_svd_fit(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, const int64_t* colptr, const int32_t* rowidx,
                 const float* cdata, int64_t m, int64_t n, int64_t nnz, int k, int n_iter, uint64_t seed, uint32_t draw, const float* q0,
                 float* components, double* singular_values_host, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !colptr || !rowidx || !components || !singular_values_host) return fail(e, SDRM_ERR_ARG, "sdrm_svd_fit: null pointer");
  if ((data == nullptr) != (cdata == nullptr)) return fail(e, SDRM_ERR_ARG, "sdrm_svd_fit: the values of the CSR and of the CSC form go together");
  if (int rc = sdrm_debug_svd_args(m, n, nnz, k, n_iter)) return fail(e, rc, std::string("sdrm_svd_fit") + kSvdEnvelope);
  hipStream_t st = (hipStream_t)stream;
  unsigned* dflag;
  float* Q;
  int rc;
  if ((rc = svd_scratch(e, &dflag)) || (rc = scratch(e, SCR_SVD_PANEL, (size_t)(m + n) * SVD_PW, &Q))) return rc;
  float* Y = Q + (size_t)n * SVD_PW;
  const CsrBatch by_rows{indptr, indices, data, nullptr, 0, m, (int)m, (int)n, e->feed_flag};
  const CsrBatch by_cols{colptr, rowidx, cdata, nullptr, 0, n, (int)n, (int)m, e->feed_flag};
  HIP_TRY(e, hipMemsetAsync(dflag, 0, sizeof(unsigned), st));
  if (q0) {
    HIP_TRY(e, hipMemcpyAsync(Q, q0, (size_t)n * SVD_PW * sizeof(float), hipMemcpyDeviceToDevice, st));
  } else if ((rc = launch_k(e, PC_SVD_EXPAND, "k_svd_start", k_svd_start, dim3((unsigned)std::min<int64_t>(4096, (n * 8 + 255) / 256)), dim3(256), 0, st,
                            Q, (int)n, (uint32_t)seed, (uint32_t)(seed >> 32), draw))) {
    return rc;
  }
  for (int it = 0; it <= n_iter; ++it) {
    if ((rc = svd_spmm(e, by_rows, nnz, Q, Y, st)) || (rc = svd_orth(e, Y, (int)m, st)) ||
        (rc = svd_spmm(e, by_cols, nnz, Y, Q, st)) ||   // the last one stays as it is: Z = A^T Y
        (it < n_iter && (rc = svd_orth(e, Q, (int)n, st))))
      return rc;
  }
  std::vector<float> z((size_t)n * SVD_PW), V;
  unsigned flag = 0;
  HIP_TRY(e, hipMemcpyAsync(z.data(), Q, z.size() * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipMemcpyAsync(&flag, dflag, sizeof(flag), hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipStreamSynchronize(st));
  if (int rc = svd_breakdown(e, "sdrm_svd_fit", st, flag)) return rc;
  if (!svd_close(z, n, k, V, singular_values_host)) return fail(e, SDRM_ERR_ARG, std::string("sdrm_svd_fit") + kSvdBreakdown);
  HIP_TRY(e, hipMemcpyAsync(components, V.data(), V.size() * sizeof(float), hipMemcpyHostToDevice, st));
  HIP_TRY(e, hipStreamSynchronize(st));   // V is this call's own
  return SDRM_OK;
}

int sdrm_svd_scores(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t nnz,
                    const int64_t* rows, int64_t row0, int b, int n_items, const float* components, int k, float* scores, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!components || !scores) return fail(e, SDRM_ERR_ARG, "sdrm_svd_scores: null pointer");
  CsrBatch c;
  if (int rc = csr_batch(e, "sdrm_svd_scores", indptr, indices, data, n_rows, rows, row0, b, n_items, &c)) return rc;
  if (k < 1 || k > SVD_KMAX || n_items > SVD_MAX_DIM || b > SVD_MAX_DIM || nnz < 0 || nnz >= ((int64_t)1 << 40) ||
      (int64_t)b * n_items >= ((int64_t)1 << 40))
    return fail(e, SDRM_ERR_SHAPE, "sdrm_svd_scores: k outside 1 .. 22, b or n_items above 2^22, nnz outside 0 .. 2^40 - 1 or b x n_items at or above 2^40");
  hipStream_t st = (hipStream_t)stream;
  float* Vt;
  if (int rc = scratch(e, SCR_SVD_VT, ((size_t)n_items + (size_t)b) * SVD_PW, &Vt)) return rc;
  float* T = Vt + (size_t)n_items * SVD_PW;
  if (int rc = launch_k(e, PC_SVD_EXPAND, "k_svd_vt", k_svd_vt, dim3((unsigned)std::min<int64_t>(4096, ((int64_t)n_items * SVD_PW + 255) / 256)), dim3(256),
                        0, st, components, k, n_items, Vt))
    return rc;
  if (int rc = svd_spmm(e, c, nnz, Vt, T, st)) return rc;
  const SvdExpandArgs a{T, components, k, n_items, b, scores};
  return launch_k(e, PC_SVD_EXPAND, "k_svd_expand", k_svd_expand,
                  dim3((unsigned)((n_items + 255) / 256), (unsigned)std::min(4096, (b + SVD_ROW_TILE - 1) / SVD_ROW_TILE)), dim3(256), 0, st, a);
}

// One product and one orthonormalisation on the caller's panels (include/sdrm_hip_debug.h).
int sdrm_debug_svd_stage(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t n_rows, int64_t n_cols,
                         int64_t nnz, const float* q, float* y_prod, float* y_orth, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !q || !y_prod || !y_orth) return fail(e, SDRM_ERR_ARG, "sdrm_debug_svd_stage: null pointer");
  if (((uintptr_t)q | (uintptr_t)y_prod | (uintptr_t)y_orth) & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_debug_svd_stage: the panels must be 16-byte aligned");
  if (n_rows < 1 || n_rows > SVD_MAX_DIM || n_cols < 1 || n_cols > SVD_MAX_DIM || nnz < 0 || nnz >= ((int64_t)1 << 40))
    return fail(e, SDRM_ERR_SHAPE, "sdrm_debug_svd_stage: n_rows or n_cols outside 1 .. 2^22 or nnz outside 0 .. 2^40 - 1");
  hipStream_t st = (hipStream_t)stream;
  unsigned* dflag;
  if (int rc = svd_scratch(e, &dflag)) return rc;
  const CsrBatch c{indptr, indices, data, nullptr, 0, n_rows, (int)n_rows, (int)n_cols, e->feed_flag};
  HIP_TRY(e, hipMemsetAsync(dflag, 0, sizeof(unsigned), st));
  if (int rc = svd_spmm(e, c, nnz, q, y_prod, st)) return rc;
  HIP_TRY(e, hipMemcpyAsync(y_orth, y_prod, (size_t)n_rows * SVD_PW * sizeof(float), hipMemcpyDeviceToDevice, st));
  if (int rc = svd_orth(e, y_orth, (int)n_rows, st)) return rc;
  unsigned flag = 0;
  HIP_TRY(e, hipMemcpyAsync(&flag, dflag, sizeof(flag), hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipStreamSynchronize(st));
  return svd_breakdown(e, "sdrm_debug_svd_stage", st, flag);
}

// ---------------------------------------------------------------------------------------------
// NMF of a sparse matrix by coordinate descent from an NNDSVDa start, and the scores of its reconstruction (svd_benchmark.py:49-54 with
// nnmf=True), csrc/nmf.h.
namespace {

constexpr int64_t NMF_MAX_DIM = (int64_t)1 << 22;
const char* const kNmfEnvelope = ": k outside 1 .. 16, m or n outside 1 .. 2^22 or nnz outside 0 .. 2^40 - 1";

int nmf_parts(int64_t rows) { return (int)std::min<int64_t>(NMF_PARTS, (rows + NMF_GRAM_ROWS - 1) / NMF_GRAM_ROWS); }

int nmf_dims(int64_t m, int64_t n, int64_t nnz, int k) {
  return (k < 1 || k > NMF_LD || m < 1 || n < 1 || m > NMF_MAX_DIM || n > NMF_MAX_DIM || nnz < 0 || nnz >= ((int64_t)1 << 40)) ? SDRM_ERR_SHAPE : SDRM_OK;
}

// out [c.b][16] = (the rows of c) f, and with `gram` the partials of f^T f behind it in the same launch
int nmf_prod(sdrm_engine* e, const CsrBatch& c, int64_t nnz, const double* f, double* out, double* gram, const NmfState* state, hipStream_t st) {
  const int pb = (c.b + 31) / 32, gb = gram ? nmf_parts(c.n_items) : 0;
  const NmfProdArgs a{c, nnz, f, out, pb, gram, state};
  return launch_k(e, PC_NMF_STEP, "k_nmf_prod", k_nmf_prod, dim3((unsigned)(pb + gb)), dim3(256), 0, st, a);
}

// `_update_coordinate_descent` of the factor w [c.b][16] against f [c.n_items][16]: two launches
int nmf_half(sdrm_engine* e, const CsrBatch& c, int64_t nnz, const double* f, double* w, int k, double* xh, double* gram, double* viol,
             const NmfState* state, hipStream_t st) {
  if (int rc = nmf_prod(e, c, nnz, f, xh, gram, state, st)) return rc;
  const NmfSweepArgs a{w, xh, gram, nmf_parts(c.n_items), c.b, k, viol, state};
  return launch_k(e, PC_NMF_STEP, "k_nmf_sweep", k_nmf_sweep, dim3((unsigned)((c.b + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace

int sdrm_nmf_fit(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, const int64_t* colptr, const int32_t* rowidx,
                 const float* cdata, int64_t m, int64_t n, int64_t nnz, int k, int max_iter, double tol, double* W, double* Ht, int32_t* n_iter_dev,
                 double* violations_dev, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !colptr || !rowidx || !W || !Ht || !n_iter_dev || !violations_dev) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_fit: null pointer");
  if ((data == nullptr) != (cdata == nullptr)) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_fit: the values of the CSR and of the CSC form go together");
  if (((uintptr_t)W | (uintptr_t)Ht) & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_fit: the factors must be 16-byte aligned");
  if (nmf_dims(m, n, nnz, k) || max_iter < 1 || max_iter > 10000 || !(tol >= 0.0))
    return fail(e, SDRM_ERR_SHAPE, std::string("sdrm_nmf_fit") + kNmfEnvelope + ", max_iter outside 1 .. 10000 or tol < 0");
  hipStream_t st = (hipStream_t)stream;
  const int64_t wide = std::max(m, n);
  const size_t bw = (size_t)((m + 255) / 256), bh = (size_t)((n + 255) / 256);
  double* ws;
  if (int rc = scratch(e, SCR_NMF_FIT, 2 + (size_t)NMF_PARTS * NMF_LD * NMF_LD + (size_t)wide * NMF_LD + bw + bh, &ws)) return rc;
  NmfState* state = reinterpret_cast<NmfState*>(ws);
  double* gram = ws + 2;
  double* xh = gram + (size_t)NMF_PARTS * NMF_LD * NMF_LD;
  double* viol_w = xh + (size_t)wide * NMF_LD;
  double* viol_h = viol_w + bw;
  const CsrBatch by_rows{indptr, indices, data, nullptr, 0, m, (int)m, (int)n, e->feed_flag};
  const CsrBatch by_cols{colptr, rowidx, cdata, nullptr, 0, n, (int)n, (int)m, e->feed_flag};
  HIP_TRY(e, hipMemsetAsync(state, 0, sizeof(NmfState), st));
  HIP_TRY(e, hipMemsetAsync(violations_dev, 0, (size_t)max_iter * sizeof(double), st));
  HIP_TRY(e, hipMemsetAsync(n_iter_dev, 0, sizeof(int32_t), st));
  for (int it = 1; it <= max_iter; ++it) {
    int rc;
    if ((rc = nmf_half(e, by_rows, nnz, Ht, W, k, xh, gram, viol_w, state, st)) ||
        (rc = nmf_half(e, by_cols, nnz, W, Ht, k, xh, gram, viol_h, state, st)) ||
        (rc = launch_k(e, PC_NMF_STEP, "k_nmf_stop", k_nmf_stop, dim3(1), dim3(256), 0, st, (const double*)viol_w, (int)bw, (const double*)viol_h, (int)bh, it,
                       max_iter, tol, state, (int*)n_iter_dev, violations_dev)))
      return rc;
  }
  return SDRM_OK;
}

int sdrm_nmf_init(sdrm_engine* e, const int64_t* indptr, const int32_t* indices, const float* data, int64_t m, int64_t n, int64_t nnz, int k,
                  const float* components, const double* singular_values_host, double* W0, double* Ht0, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!indptr || !indices || !components || !singular_values_host || !W0 || !Ht0) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_init: null pointer");
  if (((uintptr_t)W0 | (uintptr_t)Ht0) & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_init: the factors must be 16-byte aligned");
  if (nmf_dims(m, n, nnz, k)) return fail(e, SDRM_ERR_SHAPE, std::string("sdrm_nmf_init") + kNmfEnvelope);
  NmfSigma sigma, ones;
  for (int c = 0; c < NMF_LD; ++c) {
    ones.s[c] = 1.0;
    sigma.s[c] = c < k ? singular_values_host[c] : 1.0;
    if (!(sigma.s[c] > 0.0) || !std::isfinite(sigma.s[c])) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_init: a singular value that is not positive and finite");
  }
  hipStream_t st = (hipStream_t)stream;
  const int pu = nmf_parts(m), pv = nmf_parts(n);
  double* ws;
  if (int rc = scratch(e, SCR_NMF_INIT, 32 + 2 * (size_t)NMF_PARTS * 32 + (size_t)(m + n) * NMF_LD, &ws)) return rc;
  double* mean = ws;
  double* part_u = ws + 32;
  double* part_v = part_u + (size_t)NMF_PARTS * 32;
  double* vt = part_v + (size_t)NMF_PARTS * 32;
  double* u = vt + (size_t)n * NMF_LD;
  const CsrBatch by_rows{indptr, indices, data, nullptr, 0, m, (int)m, (int)n, e->feed_flag};
  int rc;
  if ((rc = launch_k(e, PC_NMF_INIT, "k_nmf_vt", k_nmf_vt, dim3((unsigned)std::min<int64_t>(4096, (n * NMF_LD + 255) / 256)), dim3(256), 0, st, components, k,
                     (int)n, vt)) ||
      (rc = nmf_prod(e, by_rows, nnz, vt, u, nullptr, nullptr, st)) ||
      (rc = launch_k(e, PC_NMF_INIT, "k_nmf_mean", k_nmf_mean, dim3(1), dim3(256), 0, st, indptr, data, m, n, nnz, mean)) ||
      (rc = launch_k(e, PC_NMF_INIT, "k_nmf_norms", k_nmf_norms, dim3((unsigned)pu), dim3(256), 0, st, (const double*)u, (int)m, k, sigma, part_u)) ||
      (rc = launch_k(e, PC_NMF_INIT, "k_nmf_norms", k_nmf_norms, dim3((unsigned)pv), dim3(256), 0, st, (const double*)vt, (int)n, k, ones, part_v)))
    return rc;
  const int blocks_w = (int)((m + 255) / 256);
  const NmfInitArgs a{u, vt, sigma, part_u, part_v, mean, (int)m, (int)n, k, pu, pv, blocks_w, W0, Ht0};
  return launch_k(e, PC_NMF_INIT, "k_nmf_init", k_nmf_init, dim3((unsigned)(blocks_w + (n + 255) / 256)), dim3(256), 0, st, a);
}

int sdrm_nmf_scores(sdrm_engine* e, const double* W, const double* Ht, int64_t n_rows, int k, const int64_t* rows, int64_t row0, int b, int n_items,
                    float* scores, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!W || !Ht || !scores) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_scores: null pointer");
  if (((uintptr_t)W | (uintptr_t)Ht) & 15u) return fail(e, SDRM_ERR_ARG, "sdrm_nmf_scores: the factors must be 16-byte aligned");
  if (k < 1 || k > NMF_LD || b < 1 || n_items < 1 || n_rows < 1 || row0 < 0 || n_items > NMF_MAX_DIM || b > NMF_MAX_DIM || n_rows > NMF_MAX_DIM ||
      (int64_t)b * n_items >= ((int64_t)1 << 40))
    return fail(e, SDRM_ERR_SHAPE, "sdrm_nmf_scores: k outside 1 .. 16, b, n_items or n_rows outside 1 .. 2^22, row0 < 0 or b x n_items at or above 2^40");
  if (!rows && row0 + b > n_rows) return fail(e, SDRM_ERR_SHAPE, "sdrm_nmf_scores: rows row0 .. row0 + b - 1 end behind the factor");
  const NmfExpandArgs a{W, Ht, rows, row0, n_rows, k, n_items, b, scores, e->feed_flag};
  return launch_k(e, PC_NMF_EXPAND, "k_nmf_expand", k_nmf_expand,
                  dim3((unsigned)((n_items + 255) / 256), (unsigned)std::min(4096, (b + NMF_ROW_TILE - 1) / NMF_ROW_TILE)), dim3(256), 0, (hipStream_t)stream, a);
}

// ---------------------------------------------------------------------------------------------
// The NeuMF evaluator's eval-mode forward (neural_cf_benchmark_pt.py:125-144 as :203-246 and :294-332 call it), csrc/neumf.h: layer 1
// staged per listed id, then all listed users x listed items, or listed pairs with the BCE-with-logits numerator.
namespace {

constexpr int64_t NEUMF_MAX_USERS = ((int64_t)1 << 20) - 16;   // listed users of one sdrm_neumf_scores call: 16 per work-group on grid.y, 65535 at most
constexpr int64_t NEUMF_MAX_ITEMS = (int64_t)1 << 22;   // listed items of one call
const char* const kNeumfEnvelope = ": factor outside {8, 16, 32}, a table without rows, no listed user or item, more than 2^20 - 16 listed users, more "
                                   "than 2^22 listed items, or users x items at or above 2^40";

bool neumf_complete(const sdrm_neumf* w) {
  return w && w->embed_user_gmf && w->embed_item_gmf && w->embed_user_mlp && w->embed_item_mlp && w->w1 && w->b1 && w->w2 && w->b2 && w->w3 &&
         w->b3 && w->wp && w->bp;
}

struct NeumfStaged { const float *w2t, *w3t, *ua, *ibt; const int *uvalid, *ivalid; int64_t ld; };

extern "C++" {   // (the ABI's extern "C" block is open: templates need C++ linkage)

// One staging launch for nu listed users and ni listed items; pairs: the user side in the transposed form as well (nu == ni then).
template <int F>
int neumf_stage(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, int nu, bool pairs, const int32_t* items, int ni, hipStream_t st,
                NeumfStaged* out) {
  constexpr int ROW = NeumfShape<F>::ROW;
  const int64_t ldu = ((int64_t)nu + 63) / 64 * 64, ldi = ((int64_t)ni + 63) / 64 * 64;
  const size_t n_w2 = (size_t)8 * F * F, n_w3 = (size_t)2 * F * F;
  const size_t n_u = pairs ? (size_t)ROW * ldu : (size_t)nu * ROW;
  float* w2t;
  int* valid;
  if (int rc = scratch(e, SCR_NEUMF_WS, n_w2 + n_w3 + n_u + (size_t)ROW * ldi, &w2t)) return rc;
  if (int rc = scratch(e, SCR_NEUMF_VALID, (size_t)nu + ni, &valid)) return rc;
  float* w3t = w2t + n_w2;
  float* ua = w3t + n_w3;
  float* ibt = ua + n_u;
  NeumfStageArgs a;
  a.side[0] = NeumfStageSide{w->embed_user_mlp, w->embed_user_gmf, users, nu, w->n_users, ua, valid, ldu, pairs ? 1 : 0, 0, FEED_BAD_ROW};
  a.side[1] = NeumfStageSide{w->embed_item_mlp, w->embed_item_gmf, items, ni, w->n_items, ibt, valid + nu, ldi, 1, 4 * F, FEED_BAD_COL};
  a.w1 = w->w1; a.b1 = w->b1; a.w2 = w->w2; a.w3 = w->w3;
  a.w2t = w2t; a.w3t = w3t;
  a.flag = e->feed_flag;
  a.blocks[0] = (int)(((int64_t)nu * ROW + 255) / 256);
  a.blocks[1] = (int)(((int64_t)ni * ROW + 255) / 256);
  const unsigned grid = (unsigned)a.blocks[0] + (unsigned)a.blocks[1] + (unsigned)((10 * F * F + 255) / 256);
  *out = NeumfStaged{w2t, w3t, ua, ibt, valid, valid + nu, ldi};
  return launch_k(e, {PC_NEUMF_STAGE, 2.0 * 16 * F * F * ((double)nu + ni)}, "k_neumf_stage", k_neumf_stage<F>, dim3(grid), dim3(256), 0, st, a);
}

template <int F>
int neumf_scores(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, int nu, const int32_t* items, int ni, float* out, hipStream_t st) {
  NeumfStaged s;
  if (int rc = neumf_stage<F>(e, w, users, nu, false, items, ni, st, &s)) return rc;
  const dim3 grid((unsigned)((ni + NEUMF_ITEM_TILE - 1) / NEUMF_ITEM_TILE), (unsigned)((nu + NEUMF_USER_TILE - 1) / NEUMF_USER_TILE));
  return launch_k(e, {PC_NEUMF_SCORES, 2.0 * (10.0 * F * F + 2.0 * F) * nu * ni}, "k_neumf_scores", k_neumf_scores<F>, grid, dim3(256), 0, st, s.ua,
                  s.uvalid, s.ibt, s.ivalid, s.ld, s.w2t, w->b2, s.w3t, w->b3, w->wp, w->bp, nu, ni, out);
}

template <int F>
int neumf_pairs(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, const int32_t* items, const float* labels, int64_t n, float* logits,
                double* loss_sum, hipStream_t st) {
  const int64_t n_part = (n + 255) / 256;
  double* parts = nullptr;
  if (loss_sum)
    if (int rc = scratch(e, SCR_NEUMF_PART, (size_t)n_part, &parts)) return rc;
  for (int64_t off = 0; off < n; off += NEUMF_PAIR_CHUNK) {
    const int m = (int)std::min<int64_t>(NEUMF_PAIR_CHUNK, n - off);
    NeumfStaged s;
    if (int rc = neumf_stage<F>(e, w, users + off, m, true, items + off, m, st, &s)) return rc;
    const float* lab = labels ? labels + off : nullptr;
    float* lg = logits ? logits + off : nullptr;
    double* part = loss_sum ? parts + off / 256 : nullptr;
    if (int rc = launch_k(e, {PC_NEUMF_PAIRS, 2.0 * (10.0 * F * F + 2.0 * F) * m}, "k_neumf_pairs", k_neumf_pairs<F>, dim3((unsigned)((m + 255) / 256)),
                          dim3(256), 0, st, s.ua, s.uvalid, s.ibt, s.ivalid, s.ld, s.w2t, w->b2, s.w3t, w->b3, w->wp, w->bp, lab, m, lg, part))
      return rc;
  }
  if (loss_sum) return launch_k(e, PC_NEUMF_PAIRS, "k_neumf_loss_sum", k_neumf_loss_sum, dim3(1), dim3(256), 0, st, parts, (int)n_part, loss_sum);
  return SDRM_OK;
}

}  // extern "C++"

}  // namespace

// The host side that needs no device: the envelope of sdrm_neumf_scores (listed users x listed items; a pair call hands in n and 1).
int sdrm_debug_neumf_args(int n_users, int n_items, int factor, int64_t listed_users, int64_t listed_items) {
  if (factor != 8 && factor != 16 && factor != 32) return SDRM_ERR_SHAPE;
  if (n_users < 1 || n_items < 1 || listed_users < 1 || listed_items < 1) return SDRM_ERR_SHAPE;
  if (listed_users > NEUMF_MAX_USERS || listed_items > NEUMF_MAX_ITEMS || listed_users * listed_items >= ((int64_t)1 << 40)) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_neumf_scores(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, int n_listed_users, const int32_t* items, int n_listed_items,
                      float* out, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!neumf_complete(w) || !users || !out) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_scores: null pointer");
  if (int rc = sdrm_debug_neumf_args(w->n_users, w->n_items, w->factor, n_listed_users, n_listed_items))
    return fail(e, rc, std::string("sdrm_neumf_scores") + kNeumfEnvelope);
  if (!items && n_listed_items != w->n_items) return fail(e, SDRM_ERR_SHAPE, "sdrm_neumf_scores: without an item list the columns are all n_items items");
  hipStream_t st = (hipStream_t)stream;
  switch (w->factor) {
    case 8: return neumf_scores<8>(e, w, users, n_listed_users, items, n_listed_items, out, st);
    case 16: return neumf_scores<16>(e, w, users, n_listed_users, items, n_listed_items, out, st);
    default: return neumf_scores<32>(e, w, users, n_listed_users, items, n_listed_items, out, st);
  }
}

int sdrm_neumf_pair_loss(sdrm_engine* e, const sdrm_neumf* w, const int32_t* users, const int32_t* items, const float* labels, int64_t n,
                         float* logits, double* loss_sum, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  if (!neumf_complete(w) || !users || !items) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_pair_loss: null pointer");
  if (!logits && !loss_sum) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_pair_loss: neither logits nor loss_sum is asked for");
  if (loss_sum && !labels) return fail(e, SDRM_ERR_ARG, "sdrm_neumf_pair_loss: the loss needs labels");
  if (n < 1 || n > (int64_t)0x7fffffff || sdrm_debug_neumf_args(w->n_users, w->n_items, w->factor, 1, 1) != SDRM_OK)
    return fail(e, SDRM_ERR_SHAPE, "sdrm_neumf_pair_loss: factor outside {8, 16, 32}, a table without rows, or n outside 1 .. 2^31 - 1");
  hipStream_t st = (hipStream_t)stream;
  switch (w->factor) {
    case 8: return neumf_pairs<8>(e, w, users, items, labels, n, logits, loss_sum, st);
    case 16: return neumf_pairs<16>(e, w, users, items, labels, n, logits, loss_sum, st);
    default: return neumf_pairs<32>(e, w, users, items, labels, n, logits, loss_sum, st);
  }
}

// ---------------------------------------------------------------------------------------------
// The NeuMF evaluator's train steps (neural_cf_benchmark_pt.py:186-200: the batch loop with zero_grad, the train-mode forward, BCEWithLogitsLoss,
// backward and optimizer.step()), csrc/neumf_train.h: per step k_nt_pairs, k_nt_grads, k_vae_adam, k_nt_clear; a whole call is enqueued
// without a host synchronisation.
namespace {

constexpr int NT_TENSORS = 12;

extern "C++" {

template <int F>
int neumf_train_steps(sdrm_engine* e, const sdrm_neumf_train* s, const int32_t* triples, int64_t n, int batch, int64_t step0, float lr, float beta1,
                      float beta2, float eps, float p_drop, const uint8_t* keep, uint64_t seed, uint32_t call_id, double* losses,
                      float* const* grads, hipStream_t st) {
  using Cols = NtCols<F>;
  const int64_t nu = s->n_users, ni = s->n_items;
  const int64_t count[NT_TENSORS] = {nu * F, ni * F, nu * 4 * F, ni * 4 * F, 32 * F * F, 4 * F, 8 * F * F, 2 * F, 2 * F * F, F, 2 * F, 1};
  // dense gradients: the four tables in their own slot (all zero between calls), the eight tower tensors behind the step's workspace;
  // every one starts on a 16-byte boundary (k_vae_adam's 16-byte accesses)
  size_t off[NT_TENSORS], tab = 0, tower = (size_t)Cols::COUNT * NT_LD;
  for (int i = 0; i < NT_TENSORS; ++i) {
    size_t& at = i < 4 ? tab : tower;
    off[i] = at;
    at += ((size_t)count[i] + 3) / 4 * 4;
  }
  float *ws, *gt;
  if (int rc = scratch(e, SCR_NEUMF_TRAIN_WS, tower, &ws)) return rc;
  if (int rc = scratch(e, SCR_NEUMF_TRAIN_TAB, tab, &gt)) return rc;
  float* g[NT_TENSORS];
  for (int i = 0; i < NT_TENSORS; ++i) g[i] = (i < 4 ? gt : ws) + off[i];
  // Adam's table, the same for every step of the call; its refusals (a range of p, m, v or g sharing a byte with another) before any launch
  {
    uint64_t addr[4 * NT_TENSORS];
    float coef[NT_TENSORS] = {0};
    for (int i = 0; i < NT_TENSORS; ++i) {
      addr[4 * i] = (uint64_t)(uintptr_t)s->p[i]; addr[4 * i + 1] = (uint64_t)(uintptr_t)g[i];
      addr[4 * i + 2] = (uint64_t)(uintptr_t)s->m[i]; addr[4 * i + 3] = (uint64_t)(uintptr_t)s->v[i];
    }
    if (int rc = sdrm_debug_vae_adam_args(addr, count, coef, NT_TENSORS, step0 + 1, 0, 0, nullptr))
      return fail(e, rc, "sdrm_neumf_train_steps: two of the parameter / moment tensors share a byte, or a table of more than 2^40 elements");
  }
  VAdamTable tabl{};
  tabl.n = NT_TENSORS;
  unsigned chunks = 0;
  for (int i = 0; i < NT_TENSORS; ++i) {
    VAdamTensor& d = tabl.t[i];
    d.p = s->p[i]; d.g = g[i]; d.m = s->m[i]; d.v = s->v[i]; d.n = count[i];
    d.wd2 = 0.f;
    d.first_chunk = chunks;
    d.vector_ok = (((uintptr_t)d.p | (uintptr_t)d.g | (uintptr_t)d.m | (uintptr_t)d.v) & 15u) == 0;
    chunks += (unsigned)((count[i] + VADAM_CHUNK - 1) / VADAM_CHUNK);
  }
  const double p = (double)p_drop;
  NtPairArgs pa{};
  pa.ws = ws; pa.flag = e->feed_flag; pa.n_users = s->n_users; pa.n_items = s->n_items;
  pa.k0 = (uint32_t)seed; pa.k1 = (uint32_t)(seed >> 32); pa.call_id = call_id;
  pa.thr = (uint32_t)std::floor(p * 4294967296.0);
  pa.s = (float)(1.0 / (1.0 - p));
  NtGradArgs ga{};
  const int in[4] = {8 * F, 4 * F, 2 * F, 2 * F}, out[4] = {4 * F, 2 * F, F, 1};
  const int colA[4] = {Cols::A0, Cols::A1, Cols::A2, Cols::AP}, colD[4] = {Cols::DZ1, Cols::DZ2, Cols::DZ3, Cols::DY};
  int wb = 0;
  for (int l = 0; l < 4; ++l) {
    ga.layer[l] = NtLayerJob{ws + (size_t)colA[l] * NT_LD, ws + (size_t)colD[l] * NT_LD, g[4 + 2 * l], g[5 + 2 * l], in[l], out[l], wb};
    wb += (out[l] * (in[l] + 1) + 255) / 256;
  }
  ga.w_blocks = wb;
  const int* uid = reinterpret_cast<const int*>(ws + (size_t)Cols::UID * NT_LD);
  const int* iid = reinterpret_cast<const int*>(ws + (size_t)Cols::IID * NT_LD);
  ga.ids[0] = uid; ga.ids[1] = iid;
  ga.D[0] = ws + (size_t)Cols::DU * NT_LD; ga.D[1] = ws + (size_t)Cols::DI * NT_LD;
  ga.g_mlp[0] = g[2]; ga.g_mlp[1] = g[3]; ga.g_gmf[0] = g[0]; ga.g_gmf[1] = g[1];
  ga.lt = ws + (size_t)Cols::LT * NT_LD;
  const int64_t steps = (n + batch - 1) / batch;
  for (int64_t t = 0; t < steps; ++t) {
    const int64_t j0 = t * batch;
    const int b = (int)std::min<int64_t>(batch, n - j0);
    pa.triples = triples + 3 * j0;
    pa.keep = keep ? keep + (size_t)j0 * 14 * F : nullptr;
    pa.b = b; pa.j0 = (uint32_t)j0;
    const double fl_pair = 2.0 * (2.0 * 42.0 * F * F + 4.0 * F);
    if (int rc = launch_k(e, {PC_NEUMF_TRAIN_PAIRS, fl_pair * b}, "k_nt_pairs", k_nt_pairs<F>, dim3((unsigned)((b + NT_PAIR_BLOCK - 1) / NT_PAIR_BLOCK)),
                          dim3(NT_PAIR_BLOCK), 0, st, (const float*)s->p[0], (const float*)s->p[1], (const float*)s->p[2], (const float*)s->p[3],
                          (const float*)s->p[4], (const float*)s->p[5], (const float*)s->p[6], (const float*)s->p[7], (const float*)s->p[8],
                          (const float*)s->p[9], (const float*)s->p[10], (const float*)s->p[11], pa))
      return rc;
    ga.b = b;
    ga.row_blocks = (b * 5 * F + 255) / 256;
    ga.loss = losses ? losses + t : nullptr;
    const unsigned gblocks = (unsigned)(wb + 2 * ga.row_blocks + (losses ? 1 : 0));
    if (int rc = launch_k(e, {PC_NEUMF_TRAIN_GRADS, 2.0 * (42.0 * F * F + 2.0 * F) * b}, "k_nt_grads", k_nt_grads<F>, dim3(gblocks), dim3(256), 0, st, ga))
      return rc;
    if (grads && t == steps - 1)
      for (int i = 0; i < NT_TENSORS; ++i) HIP_TRY(e, hipMemcpyAsync(grads[i], g[i], (size_t)count[i] * sizeof(float), hipMemcpyDeviceToDevice, st));
    VAdamArgs aa{};
    adam_scalars(step0 + t + 1, lr, (double)beta1, (double)beta2, aa.step_size, aa.bc2_sqrt);
    aa.b1 = beta1; aa.b2 = beta2; aa.eps = eps;
    if (int rc = launch_k(e, PC_NEUMF_TRAIN_ADAM, "k_vae_adam", k_vae_adam, dim3(chunks), dim3(256), 0, st, tabl, aa)) return rc;
    if (int rc = launch_k(e, PC_NEUMF_TRAIN_CLEAR, "k_nt_clear", k_nt_clear<F>, dim3((unsigned)((2 * b * 5 * F + 255) / 256)), dim3(256), 0, st, uid, iid,
                          g[2], g[0], g[3], g[1], b))
      return rc;
  }
  return SDRM_OK;
}

}  // extern "C++"

}  // namespace

// The host side that needs no device: the envelope of sdrm_neumf_train_steps.
int sdrm_debug_neumf_train_args(int n_users, int n_items, int factor, int64_t n, int batch, int64_t step0, float p_drop) {
  if (factor != 8 && factor != 16) return SDRM_ERR_SHAPE;   // (32 as well: csrc/neumf_train.h)
  if (n_users < 1 || n_items < 1 || n < 1 || n > (int64_t)0x7fffffff || batch < 1 || batch > NT_LD) return SDRM_ERR_SHAPE;
  if (step0 < 0 || step0 > ((int64_t)1 << 52)) return SDRM_ERR_ARG;
  if (!(p_drop >= 0.f && p_drop < 1.f)) return SDRM_ERR_ARG;   // (a NaN fails both compares)
  return SDRM_OK;
}

int sdrm_neumf_train_steps(sdrm_engine* e, const sdrm_neumf_train* s, const int32_t* triples, int64_t n, int batch, int64_t step0, float lr, float beta1,
                           float beta2, float eps, float p_drop, int mode, const uint8_t* keep, uint64_t seed, uint32_t call_id, double* losses,
                           float* const* grads, void* stream) {
  const char* who = "sdrm_neumf_train_steps";
  if (!e) return SDRM_ERR_ARG;
  if (!s || !triples) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  for (int i = 0; i < NT_TENSORS; ++i)
    if (!s->p[i] || !s->m[i] || !s->v[i] || (grads && !grads[i])) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null tensor pointer");
  if (mode != SDRM_RNG_EXPLICIT && mode != SDRM_RNG_PHILOX) return fail(e, SDRM_ERR_ARG, std::string(who) + ": mode is neither SDRM_RNG_EXPLICIT nor SDRM_RNG_PHILOX");
  if (mode == SDRM_RNG_EXPLICIT && !keep) return fail(e, SDRM_ERR_ARG, std::string(who) + ": SDRM_RNG_EXPLICIT needs keep [n][14 factor]");
  if (int rc = sdrm_debug_neumf_train_args(s->n_users, s->n_items, s->factor, n, batch, step0, p_drop))
    return fail(e, rc, std::string(who) + ": factor outside {8, 16} (32 is not built: csrc/neumf_train.h), a table without rows, n outside 1 .. 2^31 - 1 or "
                                          "batch outside 1 .. 1024 (SDRM_ERR_SHAPE); step0 < 0 or p_drop outside [0, 1) (SDRM_ERR_ARG)");
  const uint8_t* k = mode == SDRM_RNG_EXPLICIT ? keep : nullptr;
  hipStream_t st = (hipStream_t)stream;
  if (s->factor == 8) return neumf_train_steps<8>(e, s, triples, n, batch, step0, lr, beta1, beta2, eps, p_drop, k, seed, call_id, losses, grads, st);
  return neumf_train_steps<16>(e, s, triples, n, batch, step0, lr, beta1, beta2, eps, p_drop, k, seed, call_id, losses, grads, st);
}

// ---------------------------------------------------------------------------------------------
// An epoch's split, negatives and shuffle of the NeuMF evaluator (neural_cf_benchmark_pt.py:180-184), csrc/neumf_draw.h.  A
// device-synchronous call on a stream of the library's own: it hands three counts to the host, which sizes the train call from them.

// The host side that needs no device: the envelope.
int sdrm_debug_neumf_draw_args(int64_t n, int64_t n_hold, int64_t capacity, int with_present, int n_users) {
  if (n < 2 || n > ((int64_t)1 << 30)) return SDRM_ERR_SHAPE;          // (2 n_part stays an int32 index)
  if (n_hold < 1 || n_hold >= n) return SDRM_ERR_SHAPE;
  if (capacity < 2 * (n - n_hold)) return SDRM_ERR_SHAPE;
  if (with_present && n_users < 1) return SDRM_ERR_SHAPE;
  return SDRM_OK;
}

int sdrm_neumf_epoch_draw(sdrm_engine* e, const int32_t* triples, int64_t n, int64_t n_hold, uint64_t seed, uint32_t epoch, int32_t* hold,
                          int32_t* out, int64_t capacity, uint8_t* present, int n_users, int64_t* counts_host) {
  const char* who = "sdrm_neumf_epoch_draw";
  if (!e) return SDRM_ERR_ARG;
  if (!triples || !hold || !out || !counts_host) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (int rc = sdrm_debug_neumf_draw_args(n, n_hold, capacity, present != nullptr, n_users))
    return fail(e, rc, std::string(who) + ": n outside 2 .. 2^30, n_hold outside 1 .. n - 1, capacity below 2 (n - n_hold), or present with n_users < 1");
  HIP_TRY(e, hipSetDevice(e->device));
  HIP_TRY(e, hipDeviceSynchronize());     // every stream: whatever wrote the triples is done, whatever reads the outputs has not begun
  if (!e->draw_stream) HIP_TRY(e, hipStreamCreateWithFlags(&e->draw_stream, hipStreamNonBlocking));
  hipStream_t st = e->draw_stream;
  DrawArgs a{};
  a.T = (const DrawTriple*)triples; a.n = (uint32_t)n; a.n_hold = (uint32_t)n_hold; a.n_part = (uint32_t)(n - n_hold);
  a.k0 = (uint32_t)seed; a.k1 = (uint32_t)(seed >> 32); a.epoch = epoch;
  a.hold = (DrawTriple*)hold; a.out = (DrawTriple*)out; a.present = present; a.n_users = present ? n_users : 0;
  a.hold_blocks = (a.n_hold + 255u) / 256u; a.part_blocks = (a.n_part + 255u) / 256u;
  const size_t w_head = 4, w_mask = ((size_t)a.n_part + 63) / 64, w_src = ((size_t)a.n_part + 1) / 2, w_blk = ((size_t)a.part_blocks + 1) / 2;
  uint64_t* ws = nullptr;
  if (int rc = scratch(e, SCR_NEUMF_DRAW_WS, w_head + w_mask + 2 * w_src + 3 * w_blk, &ws)) return rc;
  a.counts = (int64_t*)ws; a.status = (unsigned*)(ws + 3);
  a.mask0 = ws + w_head;
  a.part_src = (int32_t*)(a.mask0 + w_mask); a.neg_src = (int32_t*)(a.mask0 + w_mask + w_src);
  a.cnt = (uint32_t*)(a.mask0 + w_mask + 2 * w_src); a.off0 = (uint32_t*)(a.mask0 + w_mask + 2 * w_src + 2 * w_blk);
  a.flag = e->feed_flag;
  HIP_TRY(e, hipMemsetAsync(ws, 0, w_head * sizeof(uint64_t), st));
  if (present) HIP_TRY(e, hipMemsetAsync(present, 0, (size_t)n_users, st));
  if (int rc = launch_k(e, PC_NEUMF_DRAW_SPLIT, "k_draw_split", k_draw_split, dim3(a.hold_blocks + a.part_blocks), dim3(256), 0, st, a)) return rc;
  if (int rc = launch_k(e, PC_NEUMF_DRAW_SCAN, "k_draw_scan", k_draw_scan, dim3(1), dim3(256), 0, st, a)) return rc;
  if (int rc = launch_k(e, PC_NEUMF_DRAW_NEG, "k_draw_neg", k_draw_neg, dim3(a.part_blocks), dim3(256), 0, st, a)) return rc;
  if (int rc = launch_k(e, PC_NEUMF_DRAW_OUT, "k_draw_out", k_draw_out, dim3((2u * a.n_part + 255u) / 256u), dim3(256), 0, st, a)) return rc;
  int64_t head[4] = {0, 0, 0, 0};
  HIP_TRY(e, hipMemcpyAsync(head, ws, sizeof(head), hipMemcpyDeviceToHost, st));
  HIP_TRY(e, hipStreamSynchronize(st));
  if ((unsigned)head[3] & DRAW_STATUS_WALK)
    return fail(e, SDRM_ERR_STATE, std::string(who) + ": a lane walked its permutation's cycle " + std::to_string(DRAW_MAX_WALKS) + " times without coming back inside; the outputs are not the draw");
  counts_host[0] = head[0]; counts_host[1] = head[1]; counts_host[2] = head[2];
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// The MLP evaluator's train steps (mlp_benchmark.py:85-110: the batch loop of `model.fit`), csrc/mlp_train.h; a whole call is enqueued
// without a host synchronisation.
namespace {

constexpr int MLP_TENSORS = 9;

// elements of E, W1, b1, W2, b2, W3, b3, W4, b4
void mlp_counts(int n_users, int n_items, int64_t (&count)[MLP_TENSORS]) {
  const int64_t I = n_items;
  const int64_t c[MLP_TENSORS] = {(int64_t)n_users * MLP_F, I * MLP_F * MLP_H1, MLP_H1, (int64_t)MLP_H1 * MLP_H2, MLP_H2, (int64_t)MLP_H2 * MLP_H3, MLP_H3,
                                  (int64_t)MLP_H3 * I, I};
  for (int i = 0; i < MLP_TENSORS; ++i) count[i] = c[i];
}

}  // namespace

// The host side that needs no device: the envelope of sdrm_mlp_train_steps and, with `addr`, the checks of its tensors' addresses.
int sdrm_debug_mlp_train_args(int n_users, int n_items, int64_t n, int batch, int64_t step0, float p_drop, int with_grads, const uint64_t* addr,
                              int n_addr) {
  if (n_items < 1 || n_items > MLP_MAX_ITEMS || n_users < 2 || batch < 1 || batch > MLP_MAX_BATCH || n < 1 || n > (int64_t)0x7fffffff)
    return SDRM_ERR_SHAPE;
  if (step0 < 0 || step0 > ((int64_t)1 << 52) || !(p_drop >= 0.f && p_drop < 1.f)) return SDRM_ERR_SHAPE;   // (a NaN fails both compares)
  if (with_grads && n > batch) return SDRM_ERR_ARG;   // the gradients of ONE step
  if (!addr) return SDRM_OK;
  if (n_addr != (with_grads ? 4 : 3) * MLP_TENSORS) return SDRM_ERR_ARG;
  int64_t count[MLP_TENSORS];
  mlp_counts(n_users, n_items, count);
  std::vector<std::pair<uint64_t, uint64_t>> span;
  for (int i = 0; i < n_addr; ++i) {
    if (!addr[i] || (addr[i] & 15u)) return SDRM_ERR_ARG;   // null, or off the 16-byte grid
    span.emplace_back(addr[i], addr[i] + (uint64_t)count[i % MLP_TENSORS] * sizeof(float));
  }
  std::sort(span.begin(), span.end());
  for (size_t i = 1; i < span.size(); ++i)
    if (span[i].first < span[i - 1].second) return SDRM_ERR_ARG;   // two tensors share a byte
  return SDRM_OK;
}

int sdrm_mlp_train_steps(sdrm_engine* e, const sdrm_mlp_train* s, const int64_t* indptr, const int32_t* indices, int64_t n_rows, const int64_t* rows,
                         int64_t n, int batch, int64_t step0, float lr, float beta1, float beta2, float eps, float p_drop, int mode,
                         const uint8_t* keep, uint64_t seed, uint32_t call_id, double* losses, float* const* grads_out, void* stream) {
  const char* who = "sdrm_mlp_train_steps";
  if (!e) return SDRM_ERR_ARG;
  if (!s || !indptr || !indices || !rows || !losses) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (mode != SDRM_RNG_EXPLICIT && mode != SDRM_RNG_PHILOX) return fail(e, SDRM_ERR_ARG, std::string(who) + ": mode is neither SDRM_RNG_EXPLICIT nor SDRM_RNG_PHILOX");
  if (mode == SDRM_RNG_EXPLICIT && !keep) return fail(e, SDRM_ERR_ARG, std::string(who) + ": SDRM_RNG_EXPLICIT needs keep [n][1024]");
  if (n_rows < 1) return fail(e, SDRM_ERR_SHAPE, std::string(who) + ": a CSR matrix without rows");
  uint64_t addr[4 * MLP_TENSORS];
  for (int i = 0; i < MLP_TENSORS; ++i) {
    addr[i] = (uint64_t)(uintptr_t)s->p[i]; addr[MLP_TENSORS + i] = (uint64_t)(uintptr_t)s->m[i]; addr[2 * MLP_TENSORS + i] = (uint64_t)(uintptr_t)s->v[i];
    addr[3 * MLP_TENSORS + i] = grads_out ? (uint64_t)(uintptr_t)grads_out[i] : 0;
  }
  if (int rc = sdrm_debug_mlp_train_args(s->n_users, s->n_items, n, batch, step0, p_drop, grads_out != nullptr, addr, (grads_out ? 4 : 3) * MLP_TENSORS))
    return fail(e, rc, std::string(who) + ": n_items outside 1 .. 36864, n_users < 2, batch outside 1 .. 16, n outside 1 .. 2^31 - 1, step0 < 0 or p_drop "
                                          "outside [0, 1) (SDRM_ERR_SHAPE); grads_out with more than one step, a null tensor, a tensor off the 16-byte grid "
                                          "or two tensors that share a byte (SDRM_ERR_ARG)");
  hipStream_t st = (hipStream_t)stream;
  const int I = s->n_items;
  int64_t count[MLP_TENSORS];
  mlp_counts(s->n_users, I, count);
  // the workspace: 8-byte words first
  const int w1_blocks = (I + MLP_W1_ITEMS - 1) / MLP_W1_ITEMS, out_blocks = (I + 63) / 64;
  const size_t BF = (size_t)MLP_F * MLP_H1;
  size_t at = 0;
  const auto take = [&](size_t words) { const size_t o = at; at += (words + 1) / 2 * 2; return o; };   // (every piece on the 16-byte grid)
  const size_t o_bsum = take(2 * BF), o_bpart = take((size_t)w1_blocks * BF), o_e1 = take((size_t)w1_blocks * MLP_F),
               o_zpart = take((size_t)MLP_MAX_BATCH * MLP_GCH * MLP_H1), o_loss = take((size_t)out_blocks);
  const auto take_f = [&](size_t floats) { return take((floats + 1) / 2); };
  const size_t o_a1 = take_f(MLP_MAX_BATCH * MLP_H1), o_a2 = take_f(MLP_MAX_BATCH * MLP_H2), o_a3 = take_f(MLP_MAX_BATCH * MLP_H3),
               o_dz1 = take_f(MLP_MAX_BATCH * MLP_H1), o_dz2 = take_f(MLP_MAX_BATCH * MLP_H2), o_dz3 = take_f(MLP_MAX_BATCH * MLP_H3),
               o_dy = take_f((size_t)MLP_MAX_BATCH * I), o_live = take_f(MLP_MAX_BATCH), o_mask = take_f((size_t)I);
  double* ws;
  if (int rc = scratch(e, SCR_MLP_TRAIN_WS, at, &ws)) return rc;
  double *bsum = ws + o_bsum, *bpart = ws + o_bpart, *e1part = ws + o_e1, *zpart = ws + o_zpart, *losspart = ws + o_loss;
  const auto fl = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *a1 = fl(o_a1), *a2 = fl(o_a2), *a3 = fl(o_a3), *dz1 = fl(o_dz1), *dz2 = fl(o_dz2), *dz3 = fl(o_dz3), *dy = fl(o_dy);
  int* live = reinterpret_cast<int*>(ws + o_live);
  unsigned* mask = reinterpret_cast<unsigned*>(ws + o_mask);
  float* const* P = s->p; float* const* M = s->m; float* const* V = s->v;
  float* G[MLP_TENSORS];
  for (int i = 0; i < MLP_TENSORS; ++i) G[i] = grads_out ? grads_out[i] : nullptr;

  const double p = (double)p_drop;
  MlpDrop drop{};
  drop.k0 = (uint32_t)seed; drop.k1 = (uint32_t)(seed >> 32); drop.call_id = call_id;
  drop.thr = (uint32_t)std::floor(p * 4294967296.0);
  drop.s = (float)(1.0 / (1.0 - p));
  const LaunchClass pc(PC_MLP_FWD), pcb(PC_MLP_BWD), pcw(PC_MLP_W1);

  // B_f of the weights as they stand: the W1 pass in its read-only form, then the sum of its partials
  MlpW1Args wa{};
  wa.W = P[1]; wa.mW = M[1]; wa.vW = V[1]; wa.gW = G[1]; wa.B = P[2]; wa.mB = M[2]; wa.vB = V[2]; wa.gB = G[2];
  wa.E = P[0]; wa.dz1 = dz1; wa.mask = mask; wa.bpart = bpart; wa.e1part = e1part; wa.n_items = I;
  if (int rc = launch_k(e, pcw, "k_mlp_w1<false>", k_mlp_w1<false>, dim3((unsigned)w1_blocks), dim3(128), 0, st, wa)) return rc;
  if (int rc = launch_k(e, pcb, "k_mlp_bsum", k_mlp_bsum, dim3((unsigned)(BF / 16)), dim3(256), 0, st, (const double*)bpart, w1_blocks, bsum)) return rc;
  if (G[0]) HIP_TRY(e, hipMemsetAsync(G[0], 0, (size_t)count[0] * sizeof(float), st));   // (rows 2 .. of dE: a 0 / 1 input names none of them)

  const int64_t steps = (n + batch - 1) / batch;
  for (int64_t t = 0; t < steps; ++t) {
    const int64_t j0 = t * batch;
    const int b = (int)std::min<int64_t>(batch, n - j0);
    double* bcur = bsum + (size_t)(t & 1) * BF;
    double* bnext = bsum + (size_t)((t + 1) & 1) * BF;
    const CsrBatch cb{indptr, indices, nullptr, rows + j0, 0, n_rows, b, I, e->feed_flag};
    drop.keep = mode == SDRM_RNG_EXPLICIT ? keep + (size_t)j0 * MLP_KEEP_COLS : nullptr;
    drop.j0 = (uint32_t)j0;
    MlpAdam ad{};
    {
      const double k = (double)(step0 + t + 1), b1d = (double)beta1, b2d = (double)beta2;
      ad.alpha = (float)((double)lr * std::sqrt(1.0 - std::pow(b2d, k)) / (1.0 - std::pow(b1d, k)));
      ad.omb1 = (float)(1.0 - b1d); ad.omb2 = (float)(1.0 - b2d); ad.eps = eps;
    }
    HIP_TRY(e, hipMemsetAsync(mask, 0, (size_t)I * sizeof(unsigned), st));
    if (int rc = launch_k(e, pc, "k_mlp_mask", k_mlp_mask, dim3((unsigned)b), dim3(256), 0, st, cb, mask, live)) return rc;
    if (int rc = launch_k(e, pc, "k_mlp_gather", k_mlp_gather, dim3(MLP_GCH, (unsigned)b), dim3(128), 0, st, cb, (const float*)P[0], (const float*)P[1], zpart))
      return rc;
    if (int rc = launch_k(e, pc, "k_mlp_z1", k_mlp_z1, dim3((unsigned)(b * MLP_H1 / 256)), dim3(256), 0, st, (const float*)P[0], (const float*)P[2],
                          (const double*)bcur, (const double*)zpart, drop, a1))
      return rc;
    // layers 2, 3 and the output layer
    MlpFwdArgs fa{};
    fa.b = b; fa.d = drop; fa.mask = mask; fa.live = live; fa.losspart = losspart;
    fa.A = a1; fa.W = P[3]; fa.bias = P[4]; fa.out = a2; fa.IN = MLP_H1; fa.OUT = MLP_H2; fa.drop0 = MLP_H1;
    if (int rc = launch_k(e, pc, "k_mlp_fwd<false>", k_mlp_fwd<false>, dim3(MLP_H2 / 64), dim3(256), 0, st, fa)) return rc;
    fa.A = a2; fa.W = P[5]; fa.bias = P[6]; fa.out = a3; fa.IN = MLP_H2; fa.OUT = MLP_H3; fa.drop0 = MLP_H1 + MLP_H2;
    if (int rc = launch_k(e, pc, "k_mlp_fwd<false>", k_mlp_fwd<false>, dim3(MLP_H3 / 64), dim3(256), 0, st, fa)) return rc;
    fa.A = a3; fa.W = P[7]; fa.bias = P[8]; fa.out = dy; fa.IN = MLP_H3; fa.OUT = I; fa.drop0 = 0;
    if (int rc = launch_k(e, pc, "k_mlp_fwd<true>", k_mlp_fwd<true>, dim3((unsigned)out_blocks), dim3(256), 0, st, fa)) return rc;
    // down the layers: the input gradient from the kernel before its update, then the kernel's Adam pass with its gradient inside
    const float* Ain[3] = {a3, a2, a1};
    const float* Dn[3] = {dy, dz3, dz2};
    float* dzo[3] = {dz3, dz2, dz1};
    const int in[3] = {MLP_H3, MLP_H2, MLP_H1}, out[3] = {I, MLP_H3, MLP_H2}, wi[3] = {7, 5, 3};
    for (int l = 0; l < 3; ++l) {
      const MlpDgradArgs da{Dn[l], P[wi[l]], Ain[l], dzo[l], b, in[l], out[l], drop.s};
      if (int rc = launch_k(e, pcb, "k_mlp_dgrad", k_mlp_dgrad, dim3((unsigned)in[l]), dim3(256), 0, st, da)) return rc;
      MlpAdamArgs aa{};
      aa.A = Ain[l]; aa.DZ = Dn[l]; aa.b = b; aa.IN = in[l]; aa.OUT = out[l]; aa.adam = ad;
      aa.W = P[wi[l]]; aa.mW = M[wi[l]]; aa.vW = V[wi[l]]; aa.gW = G[wi[l]];
      aa.B = P[wi[l] + 1]; aa.mB = M[wi[l] + 1]; aa.vB = V[wi[l] + 1]; aa.gB = G[wi[l] + 1];
      if (int rc = launch_k(e, pcb, "k_mlp_adam", k_mlp_adam, dim3((unsigned)((out[l] + 255) / 256), (unsigned)(in[l] / MLP_ADAM_ROWS)), dim3(256), 0, st, aa))
        return rc;
    }
    wa.b = b; wa.adam = ad;
    if (int rc = launch_k(e, pcw, "k_mlp_w1<true>", k_mlp_w1<true>, dim3((unsigned)w1_blocks), dim3(128), 0, st, wa)) return rc;
    MlpEmbedArgs ea{};
    ea.E = P[0]; ea.mE = M[0]; ea.vE = V[0]; ea.gE = G[0]; ea.e1part = e1part; ea.parts = w1_blocks; ea.bsum = bcur; ea.dz1 = dz1;
    ea.losspart = losspart; ea.loss_parts = out_blocks; ea.loss = losses + t; ea.b = b; ea.n_items = I; ea.adam = ad;
    if (int rc = launch_k(e, pcb, "k_mlp_embed", k_mlp_embed, dim3(1), dim3(256), 0, st, ea)) return rc;
    if (int rc = launch_k(e, pcb, "k_mlp_bsum", k_mlp_bsum, dim3((unsigned)(BF / 16)), dim3(256), 0, st, (const double*)bpart, w1_blocks, bnext)) return rc;
  }
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// The MLP evaluator's eval-mode forward, validation SSE and predict (mlp_benchmark.py:92, :109, :114), csrc/mlp_eval.h.
namespace {

constexpr int MLP_EVAL_MAX_BATCH = 4096;

const char* const kMlpEvalEnvelope = ": n_items outside 1 .. 36864, n_users < 2, batch outside 1 .. 4096, n < 1, a row range that starts below 0 or ends behind "
                                     "n_rows, n_rows < 1, a negative nnz, n x n_items at or above 2^40, neither out nor sse, or a tensor off the 16-byte grid "
                                     "(SDRM_ERR_SHAPE); a null tensor or another count of addresses (SDRM_ERR_ARG)";

}  // namespace

// The host side that needs no device: the envelope of sdrm_mlp_eval and, with `addr`, the checks of its nine tensors' addresses.
int sdrm_debug_mlp_eval_args(int n_users, int n_items, int64_t nnz, int64_t n_rows, int rows_listed, int64_t row0, int64_t n, int batch, int with_out,
                             int with_sse, const uint64_t* addr, int n_addr) {
  if (n_items < 1 || n_items > MLP_MAX_ITEMS || n_users < 2 || batch < 1 || batch > MLP_EVAL_MAX_BATCH || n < 1 || n_rows < 1 || nnz < 0)
    return SDRM_ERR_SHAPE;
  if (!rows_listed && (row0 < 0 || row0 > n_rows || n > n_rows - row0)) return SDRM_ERR_SHAPE;
  if (n > (((int64_t)1 << 40) - 1) / n_items) return SDRM_ERR_SHAPE;   // n x n_items < 2^40
  if (!with_out && !with_sse) return SDRM_ERR_SHAPE;
  for (int cfg = 0; cfg < N_TILE_CFGS; ++cfg) {   // the three GEMM launches on any tile (K = 512, 256, 256; A's stride equal to K)
    if (gemm_nt_band_rows(cfg, MLP_H2) < 1 || gemm_nt_band_rows(cfg, round_up(n_items, 32)) < 1) return SDRM_ERR_SHAPE;
    if (!gemm_span_ok(cfg, true, MLP_H1, MLP_H1, MLP_H1) || !gemm_span_ok(cfg, true, MLP_H2, MLP_H2, MLP_H2)) return SDRM_ERR_SHAPE;
  }
  if (!addr) return SDRM_OK;
  if (n_addr != MLP_TENSORS) return SDRM_ERR_ARG;
  for (int i = 0; i < n_addr; ++i) {
    if (!addr[i]) return SDRM_ERR_ARG;
    if (addr[i] & 15u) return SDRM_ERR_SHAPE;
  }
  return SDRM_OK;
}

int sdrm_mlp_eval(sdrm_engine* e, const sdrm_mlp_eval_w* w, const int64_t* indptr, const int32_t* indices, int64_t nnz, int64_t n_rows,
                  const int64_t* rows, int64_t row0, int64_t n, int batch, int kind, float* out, double* sse, void* stream) {
  const char* who = "sdrm_mlp_eval";
  if (!e) return SDRM_ERR_ARG;
  if (!w || !indptr || !indices) return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  if (kind != 0 && kind != 1) return fail(e, SDRM_ERR_ARG, std::string(who) + ": kind is neither 0 (probabilities) nor 1 (logits)");
  uint64_t addr[MLP_TENSORS];
  for (int i = 0; i < MLP_TENSORS; ++i) addr[i] = (uint64_t)(uintptr_t)w->p[i];
  if (int rc = sdrm_debug_mlp_eval_args(w->n_users, w->n_items, nnz, n_rows, rows != nullptr, row0, n, batch, out != nullptr, sse != nullptr, addr,
                                        MLP_TENSORS))
    return fail(e, rc, std::string(who) + kMlpEvalEnvelope);
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const int I = w->n_items, Ip = round_up(I, 32), Ir = round_up(Ip, 128);
  const int bmax = (int)std::min<int64_t>(batch, n), MP = round_up(bmax, 128);
  const int fold_blocks = (I + MLP_W1_ITEMS - 1) / MLP_W1_ITEMS;
  const size_t BF = (size_t)MLP_F * MLP_H1;
  // the workspace: 8-byte words first, every piece on the 16-byte grid
  size_t at = 0;
  const auto take = [&](size_t words) { const size_t o = at; at += (words + 1) / 2 * 2; return o; };
  const auto take_f = [&](size_t floats) { return take((floats + 1) / 2); };
  const size_t o_bsum = take(BF), o_bpart = take((size_t)fold_blocks * BF), o_rowsse = take(sse ? (size_t)n : 0);
  const size_t o_D = take_f((size_t)I * MLP_H1), o_base = take_f(MLP_H1), o_zero = take_f(4), o_w2 = take_f((size_t)MLP_H2 * MLP_H1),
               o_w3 = take_f((size_t)MLP_H3 * MLP_H2), o_w4 = take_f((size_t)Ir * MLP_H3), o_b4 = take_f(Ir), o_a1 = take_f((size_t)MP * MLP_H1),
               o_a2 = take_f((size_t)MP * MLP_H2), o_a3 = take_f((size_t)MP * MLP_H3), o_out = take_f(out ? 0 : (size_t)bmax * I);
  double* ws;
  if (int rc = scratch(e, SCR_MLP_EVAL_WS, at, &ws)) return rc;
  double *bsum = ws + o_bsum, *bpart = ws + o_bpart, *rowsse = sse ? ws + o_rowsse : nullptr;
  const auto fl = [&](size_t o) { return reinterpret_cast<float*>(ws + o); };
  float *D = fl(o_D), *base = fl(o_base), *zero = fl(o_zero), *w2t = fl(o_w2), *w3t = fl(o_w3), *w4t = fl(o_w4), *b4p = fl(o_b4), *a1 = fl(o_a1),
        *a2 = fl(o_a2), *a3 = fl(o_a3), *own_out = out ? nullptr : fl(o_out);
  const float* const* P = w->p;
  const LaunchClass pc(PC_MLP_EVAL);
  int rc;
  // once per call: the fold of W1, B_f, base; the zero slope; b4 padded, the three Keras kernels transposed
  {
    const MlpFoldArgs fa{P[1], P[0], D, bpart, I};
    if ((rc = launch_k(e, LaunchClass(PC_MLP_FOLD), "k_mlp_fold", k_mlp_fold, dim3((unsigned)fold_blocks), dim3(128), 0, st, fa))) return rc;
    if ((rc = launch_k(e, pc, "k_mlp_bsum", k_mlp_bsum, dim3((unsigned)(BF / 16)), dim3(256), 0, st, (const double*)bpart, fold_blocks, bsum))) return rc;
    if ((rc = launch_k(e, pc, "k_mlp_base", k_mlp_base, dim3(1), dim3(MLP_H1), 0, st, P[0], P[2], (const double*)bsum, base))) return rc;
    HIP_TRY(e, hipMemsetAsync(zero, 0, 4 * sizeof(float), st));
    PadList pad;
    pad.add(P[8], 1, I, b4p, 1, Ir);
    if ((rc = pad.launch(e, pc, st)) || (rc = launch_w1t(e, pc, P[3], MLP_H1, MLP_H2, w2t, MLP_H1, st)) ||
        (rc = launch_w1t(e, pc, P[5], MLP_H2, MLP_H3, w3t, MLP_H2, st)) || (rc = launch_w1t(e, pc, P[7], MLP_H3, I, w4t, MLP_H3, st)))
      return rc;
  }
  // the tile goes by `batch` alone, so that a row has the same bits in every call made with the same batch
  const int cfg = choose_cfg(e->tune, round_up(batch, BM), e->tune.nt32_max_rows);
  for (int64_t j0 = 0; j0 < n; j0 += batch) {
    const int b = (int)std::min<int64_t>(batch, n - j0);
    const int rows64 = round_up(b, BM);
    const CsrBatch cb{indptr, indices, nullptr, rows ? rows + j0 : nullptr, rows ? 0 : row0 + j0, n_rows, b, I, e->feed_flag};
    // 1: a1 = relu(base + the row's rows of D) into the padded operand
    {
      EncodeCsrArgs a{};
      a.csr = cb; a.w1t = D; a.b1 = base; a.Hq = MLP_H1; a.Hp = MLP_H1; a.hid = a1; a.nnz = nnz;
      if ((rc = launch_gather_rows(e, pc, "k_mlp_rows_relu", MLP_H1 / 4, a, st,
                                   [](auto tpr, auto nv, auto u) { return k_mlp_rows_relu<VAL(tpr), VAL(nv), VAL(u)>; })))
        return rc;
    }
    // 2, 3: a2 = relu(a1 W2 + b2), a3 = relu(a2 W3 + b3): PReLU with a zero slope
    {
      GemmArgs a{};
      a.B = w2t; a.ldb = MLP_H1; a.C = a2; a.ldc = MLP_H2; a.K = MLP_H1; a.bias = P[4]; a.slopeE = zero;
      if ((rc = gemm_nt_banded<EPI_BIAS_PRELU>(e, a, a1, MLP_H1, rows64, MLP_H2, b, st, Prof{e, PC_MLP_EVAL, 2.0 * b * (double)MLP_H1 * MLP_H2}, cfg))) return rc;
    }
    {
      GemmArgs a{};
      a.B = w3t; a.ldb = MLP_H2; a.C = a3; a.ldc = MLP_H3; a.K = MLP_H2; a.bias = P[6]; a.slopeE = zero;
      if ((rc = gemm_nt_banded<EPI_BIAS_PRELU>(e, a, a2, MLP_H2, rows64, MLP_H3, b, st, Prof{e, PC_MLP_EVAL, 2.0 * b * (double)MLP_H2 * MLP_H3}, cfg))) return rc;
    }
    // 4: the output layer, bounds-checked into the batch's [b][I]: the caller's rows j0 .., or the scratch (always probabilities)
    float* s_out = out ? out + (size_t)j0 * I : own_out;
    const bool logits = out && kind == 1;
    {
      GemmArgs a{};
      a.B = w4t; a.ldb = MLP_H3; a.C = s_out; a.ldc = I; a.K = MLP_H3; a.bias = b4p; a.cols_valid = I;
      const Prof pr{e, PC_MLP_EVAL, 2.0 * b * (double)I * MLP_H3};
      if ((rc = logits ? gemm_nt_banded<EPI_BIAS_G>(e, a, a3, MLP_H3, rows64, Ip, b, st, pr, cfg)
                       : gemm_nt_banded<EPI_BIAS_SIGMOID_G>(e, a, a3, MLP_H3, rows64, Ip, b, st, pr, cfg)))
        return rc;
    }
    // 5: dead rows zeroed, the rows' SSE
    {
      const MlpSseArgs a{cb, nnz, s_out, rowsse ? rowsse + j0 : nullptr, logits ? 1 : 0};
      if ((rc = launch_k(e, pc, "k_mlp_sse", k_mlp_sse, dim3((unsigned)b), dim3(256), 0, st, a))) return rc;
    }
  }
  if (sse) return launch_k(e, pc, "k_mlp_sse_sum", k_mlp_sse_sum, dim3(1), dim3(256), 0, st, (const double*)rowsse, n, sse);
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
// The evaluation half of a VAE pre-stage epoch (train_SDRM.py:160-177), csrc/eval_half.h: the live weights staged once, then per
// batch of users the eval-mode forward straight from the train part's CSR rows and the ranking against the held part.
namespace {

constexpr int EVAL_MAX_ITEMS = 36864;   // k_rank_metrics' LDS row

const char* const kEvalEnvelope = ": n_items outside 1 .. 36864, hidden or latent outside 1 .. 4096, n_rows outside 1 .. 2^31 - 1, batch outside 1 .. 2^22, "
                                  "k outside 1 .. min(128, n_items), metric not 0 (recall) or 1 (ndcg), a negative nnz, or the encoder's and the decoder's sizes differ";

}  // namespace

// The host side that needs no device: the envelope, and the tests that the three GEMM launches of sdrm_vae_eval_holdout make on any
// tile (A's stride equal to K, as those launches have it; a launch of another form added to the call needs its own line here).
int sdrm_debug_vae_eval_args(int n_items, int hidden, int latent, int64_t n_rows, int batch, int k, int metric) {
  if (n_items < 1 || n_items > EVAL_MAX_ITEMS || hidden < 1 || hidden > VAE_MAX_HIDDEN || latent < 1 || latent > VAE_MAX_LATENT || n_rows < 1 ||
      n_rows > (int64_t)INT32_MAX || batch < 1 || batch > MAX_BATCH_ROWS || k < 1 || k > RANK_MAX_K || k > n_items || (metric != 0 && metric != 1))
    return SDRM_ERR_SHAPE;
  const VaeDims d = vae_dims(n_items, hidden, latent, batch);
  for (int cfg = 0; cfg < N_TILE_CFGS; ++cfg) {
    // h1 W2[:L]^T (K = Hp), z W3^T (K = Lp), h3 W4^T (K = Hp): a row band of each fits a launch, and a tile x K span stays below 2^32 bytes
    if (gemm_nt_band_rows(cfg, d.Lp) < 1 || gemm_nt_band_rows(cfg, d.Hp) < 1 || gemm_nt_band_rows(cfg, d.Ip) < 1) return SDRM_ERR_SHAPE;
    if (!gemm_span_ok(cfg, true, d.Hp, d.Hp, d.Hp) || !gemm_span_ok(cfg, true, d.Lp, d.Lp, d.Lp)) return SDRM_ERR_SHAPE;
  }
  return SDRM_OK;
}

int sdrm_vae_eval_holdout(sdrm_engine* e, const sdrm_vae_encoder* enc, const sdrm_vae_decoder* dec, const int64_t* train_indptr,
                          const int32_t* train_indices, int64_t train_nnz, const int64_t* held_indptr, const int32_t* held_indices,
                          int64_t held_nnz, int64_t n_rows, int batch, int k, const double* tp, const double* idcg, int metric, double* scores,
                          float* logits, void* stream) {
  const char* who = "sdrm_vae_eval_holdout";
  if (!e) return SDRM_ERR_ARG;
  if (!enc_tensors(enc) || !dec_tensors(dec) || !train_indptr || !train_indices || !held_indptr || !held_indices || !tp || !idcg || !scores)
    return fail(e, SDRM_ERR_ARG, std::string(who) + ": null pointer");
  const int I = enc->n_items, H = enc->hidden, L = enc->latent;
  if (dec->n_items != I || dec->hidden != H || dec->latent != L || train_nnz < 0 || held_nnz < 0)
    return fail(e, SDRM_ERR_SHAPE, std::string(who) + kEvalEnvelope);
  if (int rc = sdrm_debug_vae_eval_args(I, H, L, n_rows, batch, k, metric)) return fail(e, rc, std::string(who) + kEvalEnvelope);
  hipStream_t st = (hipStream_t)stream;
  if (int jr = chains_join(e, st)) return jr;
  const int bmax = (int)std::min<int64_t>(batch, n_rows);
  const VaeDims d = vae_dims(I, H, L, bmax);
  float *w1t, *b1p, *w2p, *b2p, *w3p, *b3p, *w4p, *b4p, *h1, *zp, *h3, *own_logits = nullptr;
  int rc;
  if ((rc = scratch(e, SCR_EV_W1T, (size_t)I * d.Hq, &w1t)) || (rc = scratch(e, SCR_EV_B1, d.Hr, &b1p)) ||
      (rc = scratch(e, SCR_EV_W2, (size_t)d.Lr * d.Hp, &w2p)) || (rc = scratch(e, SCR_EV_B2, d.Lr, &b2p)) ||
      (rc = scratch(e, SCR_EV_W3, (size_t)d.Hr * d.Lp, &w3p)) || (rc = scratch(e, SCR_EV_B3, d.Hr, &b3p)) ||
      (rc = scratch(e, SCR_EV_W4, (size_t)d.Ir * d.Hp, &w4p)) || (rc = scratch(e, SCR_EV_B4, d.Ir, &b4p)) ||
      (rc = scratch(e, SCR_EV_H1, (size_t)d.MP * d.Hp, &h1)) || (rc = scratch(e, SCR_EV_Z, (size_t)d.MP * d.Lp, &zp)) ||
      (rc = scratch(e, SCR_EV_H3, (size_t)d.MP * d.Hp, &h3)))
    return rc;
  if (!logits && (rc = scratch(e, SCR_EV_LOGITS, (size_t)bmax * I, &own_logits))) return rc;
  const size_t lds = (size_t)I * sizeof(float);
  if (lds > 48 * 1024) HIP_TRY(e, allow_full_lds((const void*)k_rank_metrics_checked, EVAL_MAX_ITEMS * (int)sizeof(float)));
  // staging, once per call (the weights change with every optimiser step): seven tensors padded in one launch, W1 transposed in a second
  {
    PadList pad;
    pad.add(enc->b1, 1, H, b1p, 1, d.Hr);
    pad.add(enc->w2, L, H, w2p, d.Lr, d.Hp);   // the mu rows: the first L of [2 L][H]
    pad.add(enc->b2, 1, L, b2p, 1, d.Lr);
    pad.add(dec->w1, H, L, w3p, d.Hr, d.Lp);
    pad.add(dec->b1, 1, H, b3p, 1, d.Hr);
    pad.add(dec->w2, I, H, w4p, d.Ir, d.Hp);
    pad.add(dec->b2, 1, I, b4p, 1, d.Ir);
    if ((rc = pad.launch(e, PC_EVAL_HALF, st)) || (rc = launch_w1t(e, PC_EVAL_HALF, enc->w1, H, I, w1t, d.Hq, st))) return rc;
  }
  for (int64_t row0 = 0; row0 < n_rows; row0 += batch) {
    const int b = (int)std::min<int64_t>(batch, n_rows - row0);
    const int rows64 = round_up(b, BM);
    const int cfg = choose_cfg(e->tune, rows64, e->tune.nt32_max_rows);
    // 1: h1 = tanh(W1 x / |x| + b1) by gather from the train part's rows, into the padded operand (columns behind H: zero)
    {
      EncodeCsrArgs a{};
      a.csr = CsrBatch{train_indptr, train_indices, nullptr, nullptr, row0, n_rows, b, I, e->feed_flag};
      a.w1t = w1t; a.b1 = b1p; a.Hq = d.Hq; a.Hp = d.Hp; a.hid = h1; a.nnz = train_nnz;
      if ((rc = launch_gather_rows(e, PC_EVAL_HALF, "k_encode_csr_checked", d.Hq / 4, a, st,
                                   [](auto tpr, auto nv, auto u) { return k_encode_csr_checked<VAL(tpr), VAL(nv), VAL(u)>; })))
        return rc;
    }
    // 2: z = h1 W2[:L]^T + b2[:L] into the padded [MP][Lp] (W2's pad rows and b2's pad are zero: columns behind L are 0)
    {
      GemmArgs a{};
      a.B = w2p; a.ldb = d.Hp; a.C = zp; a.ldc = d.Lp; a.K = d.Hp; a.bias = b2p;
      if ((rc = gemm_nt_banded<EPI_BIAS>(e, a, h1, d.Hp, rows64, d.Lp, b, st, Prof{e, PC_EVAL_HALF, 2.0 * b * (double)L * H}, cfg))) return rc;
    }
    // 3: h3 = tanh(z W3^T + b3) into the padded [MP][Hp]
    {
      GemmArgs a{};
      a.B = w3p; a.ldb = d.Lp; a.C = h3; a.ldc = d.Hp; a.K = d.Lp; a.bias = b3p;
      if ((rc = gemm_nt_banded<EPI_BIAS_TANH>(e, a, zp, d.Lp, rows64, d.Hp, b, st, Prof{e, PC_EVAL_HALF, 2.0 * b * (double)H * L}, cfg))) return rc;
    }
    // 4: s = h3 W4^T + b4, bounds-checked into the batch's [b][I]: the scratch, or the caller's rows row0 ..
    float* s_out = logits ? logits + (size_t)row0 * I : own_logits;
    {
      GemmArgs a{};
      a.B = w4p; a.ldb = d.Hp; a.C = s_out; a.ldc = I; a.K = d.Hp; a.bias = b4p; a.cols_valid = I;
      if ((rc = gemm_nt_banded<EPI_BIAS_G>(e, a, h3, d.Hp, rows64, d.Ip, b, st, Prof{e, PC_EVAL_HALF, 2.0 * b * (double)I * H}, cfg))) return rc;
    }
    // 5: the chosen metric of the batch's users into scores[row0 ..] (the indptr arrays hold absolute offsets: a row range is a pointer offset)
    {
      RankArgs a{};
      a.scores = s_out; a.U = b; a.I = I;
      a.held_indptr = held_indptr + row0; a.held_indices = held_indices;
      a.train_indptr = train_indptr + row0; a.train_indices = train_indices;
      a.nk = 1; a.kmax = k; a.ks[0] = k;
      a.tp = tp; a.idcg = idcg;
      a.recall = metric == 0 ? scores + row0 : nullptr;
      a.ndcg = metric == 1 ? scores + row0 : nullptr;
      const RankCheck ck{held_nnz, train_nnz, e->feed_flag};
      if ((rc = launch_k(e, PC_EVAL_HALF, "k_rank_metrics_checked", k_rank_metrics_checked, dim3((unsigned)b), dim3(256), lds, st, a, ck))) return rc;
    }
  }
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
int64_t sdrm_launch_count(const sdrm_engine* e) { return e ? e->n_launches : -1; }
int sdrm_profile_classes(void) { return PC_COUNT; }
const char* sdrm_profile_name(int cls) { return (cls >= 0 && cls < PC_COUNT) ? kProfNames[cls] : ""; }

int sdrm_profile_begin(sdrm_engine* e, int capacity) {
  if (!e || capacity < 1) return SDRM_ERR_ARG;
  while ((int)e->prof_ev.size() < 2 * capacity) {
    hipEvent_t ev;
    HIP_TRY(e, hipEventCreate(&ev));
    e->prof_ev.push_back(ev);
  }
  e->prof_cap = capacity;
  e->prof_cls.clear();
  e->prof_flops.clear();
  for (int i = 0; i < PROF_SLOTS; ++i) { e->prof_ms[i] = 0; e->prof_fl[i] = 0; e->prof_n[i] = 0; }
  e->prof_on = true;
  return SDRM_OK;
}

int sdrm_profile_only(sdrm_engine* e, int cls) {
  if (!e || cls >= PC_COUNT) return SDRM_ERR_ARG;
  e->prof_only = cls < 0 ? -1 : cls;
  return SDRM_OK;
}

int sdrm_profile_end(sdrm_engine* e, void* stream) {
  if (!e) return SDRM_ERR_ARG;
  e->prof_on = false;
  if (int jr = chains_join(e, (hipStream_t)stream)) return jr;
  HIP_TRY(e, hipStreamSynchronize((hipStream_t)stream));
  for (size_t i = 0; i < e->prof_cls.size(); ++i) {
    float ms = 0.f;
    HIP_TRY(e, hipEventElapsedTime(&ms, e->prof_ev[2 * i], e->prof_ev[2 * i + 1]));
    const int c = e->prof_cls[i];
    e->prof_ms[c] += ms; e->prof_fl[c] += e->prof_flops[i]; e->prof_n[c] += 1;
  }
  return SDRM_OK;
}

int sdrm_profile_get(const sdrm_engine* e, int cls, double* total_ms, int64_t* launches, double* flops) {
  if (!e || cls < 0 || cls >= PC_COUNT) return SDRM_ERR_ARG;
  if (total_ms) *total_ms = e->prof_ms[cls];
  if (launches) *launches = e->prof_n[cls];
  if (flops) *flops = e->prof_fl[cls];
  return SDRM_OK;
}

// ---------------------------------------------------------------------------------------------
int sdrm_debug_gemm(int variant, int cfg, const float* A, const float* B, float* C, int M, int N, int K, void* stream) {
  if (!A || !B || !C || cfg < 0 || cfg >= N_TILE_CFGS) return SDRM_ERR_ARG;
  if (M % 32 || N % 32 || K % 32 || variant < 0 || variant > 2) return SDRM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  // The kernel reads whole tiles without bounds checks, so stage the caller's matrices in zero-padded
  // scratch (test hook only: allocates and synchronises).
  const int Mp = round_up(M, 128), Np = round_up(N, 128), Kp = round_up(K, 128);
  const int ar = variant == 2 ? Kp : Mp, ac = variant == 2 ? Mp : K;     // A as stored: [M,K] or [K,M]
  const int br = variant == 0 ? Np : Kp, bc = variant == 0 ? K : Np;     // B as stored: [N,K] or [K,N]
  float *dA = nullptr, *dB = nullptr, *dC = nullptr;
  if (dalloc(&dA, (size_t)ar * ac) != hipSuccess || dalloc(&dB, (size_t)br * bc) != hipSuccess ||
      dalloc(&dC, (size_t)Mp * Np) != hipSuccess)
    return SDRM_ERR_NOMEM;
  const int a_rows = variant == 2 ? K : M, a_cols = variant == 2 ? M : K;
  const int b_rows = variant == 0 ? N : K, b_cols = variant == 0 ? K : N;
  hipError_t rc = hipMemcpy2DAsync(dA, (size_t)ac * 4, A, (size_t)a_cols * 4, (size_t)a_cols * 4, a_rows, hipMemcpyDeviceToDevice, st);
  if (rc == hipSuccess)
    rc = hipMemcpy2DAsync(dB, (size_t)bc * 4, B, (size_t)b_cols * 4, (size_t)b_cols * 4, b_rows, hipMemcpyDeviceToDevice, st);
  GemmArgs a{};
  a.C = dC; a.ldc = Np; a.K = K; a.kchunk = K;
  a.A = dA; a.lda = ac; a.limA = M; a.B = dB; a.ldb = bc; a.limB = N;
  if (rc == hipSuccess) {
    const Prof np{nullptr, 0, 0.0};
    if (variant == 0) rc = launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
    else if (variant == 1) rc = launch_gemm<LD_KCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
    else rc = launch_gemm<LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
  }
  if (rc == hipSuccess)
    rc = hipMemcpy2DAsync(C, (size_t)N * 4, dC, (size_t)Np * 4, (size_t)N * 4, M, hipMemcpyDeviceToDevice, st);
  if (rc == hipSuccess) rc = hipStreamSynchronize(st);
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
  return rc == hipSuccess ? SDRM_OK : SDRM_ERR_HIP;
}

/* Timing variant of the hook for tools/gemm_tune.py: same kernel, `reps` launches on pre-padded scratch,
 * returns the mean microseconds per launch measured with HIP events on `stream`. */
#ifdef SDRM_STAMPS
// diagnostic build: stamps of the engine's own batched weight-gradient launch (the last one run)
extern "C" int sdrm_debug_stamp_class(int cls) { g_stamp_class = cls; return SDRM_OK; }
extern "C" int sdrm_debug_wgrad_stamps_begin(int max_blocks) {
  if (g_wgrad_stamps) (void)hipFree(g_wgrad_stamps);
  g_wgrad_stamps = nullptr;
  if (dalloc(&g_wgrad_stamps, (size_t)8 * max_blocks) != hipSuccess) return SDRM_ERR_NOMEM;
  g_wgrad_stamps_cap = max_blocks; g_wgrad_stamps_n = 0;
  return SDRM_OK;
}
extern "C" int sdrm_debug_wgrad_stamps_read(unsigned long long* host_out, int max_blocks) {
  if (!g_wgrad_stamps || hipDeviceSynchronize() != hipSuccess) return SDRM_ERR_STATE;
  const int nb = g_wgrad_stamps_n < max_blocks ? g_wgrad_stamps_n : max_blocks;
  if (hipMemcpy(host_out, g_wgrad_stamps, (size_t)nb * 64, hipMemcpyDeviceToHost) != hipSuccess) return SDRM_ERR_HIP;
  return nb;
}
// host_out: 8 slots per block (gemm.h); `warm` launches first, back to back, so that the clock the stamps see is the one
// the chip holds under this load (MI355X_MICROARCH.md, DVFS give-back item 6: >= 2 s)
extern "C" int sdrm_debug_gemm_stamps(int variant, int cfg, int M, int N, int K, unsigned long long* host_out, int max_blocks,
                                      int warm) {
  if (cfg < 0 || cfg >= N_TILE_CFGS) return SDRM_ERR_ARG;
  const int Mp = round_up(M, 128), Np = round_up(N, 128), Kp = round_up(K, 128);
  const int ar = variant == 2 ? Kp : Mp, ac = variant == 2 ? Mp : K;
  const int br = variant == 0 ? Np : Kp, bc = variant == 0 ? K : Np;
  float *dA = nullptr, *dB = nullptr, *dC = nullptr;
  unsigned long long* dS = nullptr;
  if (dalloc(&dA, (size_t)ar * ac) != hipSuccess || dalloc(&dB, (size_t)br * bc) != hipSuccess ||
      dalloc(&dC, (size_t)Mp * Np) != hipSuccess || dalloc(&dS, (size_t)8 * max_blocks) != hipSuccess)
    return SDRM_ERR_NOMEM;
  GemmArgs a{};
  a.C = dC; a.ldc = Np; a.K = K; a.kchunk = K; a.stamps = dS;
  a.A = dA; a.lda = ac; a.limA = M; a.B = dB; a.ldb = bc; a.limB = N;
  hipError_t rc = hipSuccess;
  for (int i = 0; i < 3 + (warm > 0 ? warm : 0) && rc == hipSuccess; ++i) {
    const Prof np{nullptr, 0, 0.0};
    if (variant == 0) rc = launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, nullptr, np, cfg);
    else if (variant == 1) rc = launch_gemm<LD_KCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, nullptr, np, cfg);
    else rc = launch_gemm<LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, nullptr, np, cfg);
  }
  if (rc == hipSuccess) rc = hipDeviceSynchronize();
  const int nb = a.nblocks < max_blocks ? a.nblocks : max_blocks;
  if (rc == hipSuccess) rc = hipMemcpy(host_out, dS, (size_t)nb * 64, hipMemcpyDeviceToHost);
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC); (void)hipFree(dS);
  return rc == hipSuccess ? nb : SDRM_ERR_HIP;
}
#endif

int sdrm_debug_gemm_time(int variant, int cfg, int M, int N, int K, int reps, float* us_out, void* stream) {
  if (!us_out || reps < 1 || M % 32 || N % 32 || K % 32 || variant < 0 || variant > 2 || cfg < 0 || cfg >= N_TILE_CFGS) return SDRM_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  const int Mp = round_up(M, 128), Np = round_up(N, 128), Kp = round_up(K, 128);
  const int ar = variant == 2 ? Kp : Mp, ac = variant == 2 ? Mp : K;
  const int br = variant == 0 ? Np : Kp, bc = variant == 0 ? K : Np;
  float *dA = nullptr, *dB = nullptr, *dC = nullptr;
  if (dalloc(&dA, (size_t)ar * ac) != hipSuccess || dalloc(&dB, (size_t)br * bc) != hipSuccess ||
      dalloc(&dC, (size_t)Mp * Np) != hipSuccess)
    return SDRM_ERR_NOMEM;
  GemmArgs a{};
  a.C = dC; a.ldc = Np; a.K = K; a.kchunk = K;
  a.A = dA; a.lda = ac; a.limA = M; a.B = dB; a.ldb = bc; a.limB = N;
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  hipError_t rc = hipSuccess;
  for (int i = 0; i < reps + 3 && rc == hipSuccess; ++i) {
    if (i == 3) (void)hipEventRecord(e0, st);
    const Prof np{nullptr, 0, 0.0};
    if (variant == 0) rc = launch_gemm<LD_KCONTIG, LD_KCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
    else if (variant == 1) rc = launch_gemm<LD_KCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
    else rc = launch_gemm<LD_MCONTIG, LD_MCONTIG, XF_NONE, XF_NONE, EPI_PLAIN>(a, M, N, 1, st, np, cfg);
  }
  (void)hipEventRecord(e1, st);
  if (rc == hipSuccess) rc = hipStreamSynchronize(st);
  float ms = 0.f;
  if (rc == hipSuccess) rc = hipEventElapsedTime(&ms, e0, e1);
  *us_out = ms * 1e3f / reps;
  (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
  (void)hipFree(dA); (void)hipFree(dB); (void)hipFree(dC);
  return rc == hipSuccess ? SDRM_OK : SDRM_ERR_HIP;
}

}  // extern "C"
