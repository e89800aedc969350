// The evaluation half of a VAE pre-stage epoch on the engine (train_SDRM.py:160-177 with is_training == 0 and dropout off): for every
// user u of a hold-out split, with T_u the columns of the train part and H_u those of the held part (every stored entry counts as 1),
//   x = 1_{T_u} / max(sqrt(|T_u|), 1e-12),  h1 = tanh(W1 x + b1),  z = W2[:L] h1 + b2[:L],  h3 = tanh(W3 z + b3),  s = W4 h3 + b4,
//   score_u = Recall@k or NDCG@k of s against H_u with the items of T_u at -inf                      (sdrm_rank_metrics' definition).
// The logvar rows of W2, the KL and the reparameterisation draw are never computed.  sdrm_vae_eval_holdout (csrc/sdrm_hip.hip) takes the
// LIVE weights, stages them once per call into scratch of its own (EV_* below: W1^T [n_items][Hq] by k_encode_w1t, the other seven
// tensors on the GEMM family's padded strides by ONE k_pad2d launch) and then runs, per batch of users, five launches that exist
// already - nothing here is a second copy of one of them:
//   1  k_encode_csr_checked (below)        the body of k_encode_csr (csrc/encode.h): normalise + first Linear as a sum of W1^T rows + bias +
//                                          tanh, into the padded operand [rows64][Hp]; every offset held against the train part's nnz
//   2  gemm_kernel<.., EPI_BIAS>           mu rows of W2, into the padded z [rows64][Lp] (columns behind L: 0 + 0)
//   3  gemm_kernel<.., EPI_BIAS_TANH>      into the padded h3 [rows64][Hp]
//   4  gemm_kernel<.., EPI_BIAS_G>         bounds-checked into the batch's [b][n_items] logits (scratch, or the caller's rows)
//   5  k_rank_metrics_checked (below)      the body of k_rank_metrics (csrc/rank.h) with every offset and column range-checked
// What is new on the device are the CHECKED instantiations of the gather's and the ranking's bodies: the call is public and must not
// assume that its two CSRs come from sdrm_holdout_split, and unlike the feed entry points it is given both nnz.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode.h"
#include "rank.h"

namespace sdrm {

// Launch 1: k_encode_csr's body (csrc/encode.h) with the upper end of every train indptr pair held against a.nnz as well, so that the
// gather loads no index behind the caller's array.  A pair that fails is the empty row here and in launch 5 alike: the user's logits are
// those of a user without train entries, nothing of that user is masked, and FEED_BAD_PTR is raised.
template <int TPR, int NV, int U>
__global__ __launch_bounds__(256) void k_encode_csr_checked(const EncodeCsrArgs a) { encode_csr_rows<TPR, NV, U, true>(a); }

// One work-group per user of the batch: a.scores is the batch's [U][I] logits, the indptr arrays start at the batch's first row (they
// hold absolute offsets), a.recall / a.ndcg at its first user; the one that is null is not written.
__global__ __launch_bounds__(256) void k_rank_metrics_checked(const RankArgs a, const RankCheck ck) { rank_metrics_user<true>(a, ck); }

}  // namespace sdrm
