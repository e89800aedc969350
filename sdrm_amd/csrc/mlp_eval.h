// The MLP evaluator's EVAL-MODE forward on the device (reference: mlp_benchmark.py:92 the RMSE metric, :109 the per-epoch validation pass
// of `model.fit`, :114 `model.predict`; restated in sdrm_amd/mlp_eval.py; the train half is csrc/mlp_train.h, whose constants and layout
// this file shares).  In inference the three dropouts are the identity, so for a row r of the 0 / 1 matrix, given as a CSR pattern:
//   z1[r] = base + sum_{j in row r} D[j]      D[j] = sum_f (E[1][f] - E[0][f]) W1[8j + f]     (512 floats per item)
//   base  = b1 + sum_f E[0][f] B_f            B_f  = sum_j W1[8j + f]
//   a1 = relu(z1)   a2 = relu(a1 W2 + b2)   a3 = relu(a2 W3 + b3)   y = a3 W4 + b4   p = sigmoid(y)
// A call reads W1 ONCE (k_mlp_fold), where the train step's gather moves 16 KB per stored entry: an evaluation call has hundreds to
// thousands of rows.  The launches of sdrm_mlp_eval (csrc/sdrm_hip.hip):
//   once per call
//     k_mlp_fold      the pass over W1: D [n_items][512] fp32 - a row per item, the W1^T [n_items][Hq] form the row gather takes - and
//                     the per-work-group float64 partials of B_f in k_mlp_w1<false>'s layout
//     k_mlp_bsum      (csrc/mlp_train.h) the partials in its fixed order
//     k_mlp_base      base [512], one work-group
//     k_pad2d         b4 onto the GEMM family's padded stride
//     k_encode_w1t x3 the Keras kernels W2, W3, W4 ([in][out]) transposed into the [out][in] operands of the NT GEMMs
//   per batch of rows
//     k_mlp_rows_relu encode_csr_rows (csrc/encode.h) with the ReLU and no scaling: a1 into the padded operand [rows64][512], every
//                     offset held against nnz
//     gemm_kernel<.., EPI_BIAS_PRELU> x2   layers 2 and 3 with a zero slope (a ReLU), into padded operands
//     gemm_kernel<.., EPI_BIAS_G> or <.., EPI_BIAS_SIGMOID_G>   the output layer, bounds-checked into the batch's unpadded [b][n_items]
//     k_mlp_sse       a work-group per row: a dead row's output zeroed, and (when asked) SSE_r = sum_j p_rj^2 - sum_{j in row r} (2 p_rj - 1),
//                     which is sum_j (p_rj - x_rj)^2 without a dense x
//   last, when the SSE is asked for
//     k_mlp_sse_sum   the rows' values in row order (256 consecutive stretches, then those in order), one float64
// Values are fp32; D's eight-term sums and every sum of the SSE are float64 in a fixed order.  No floating-point atomic: two runs of
// a call give the same bits, and a row's output is a function of that row and the tile configuration alone.
// A row id outside the matrix or an indptr pair that is negative, out of order or reaches behind nnz is a DEAD row (output zero, no
// SSE); a column outside [0, n_items) is skipped by the gather and by the SSE: both raise the feed status word.  No address is taken
// from the feed unchecked.  Plain HIP, vector / plain C++ stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "encode.h"
#include "mlp_train.h"

namespace sdrm {

// The pass over W1: grid ceil(I / MLP_W1_ITEMS), block 128, thread t owns columns 4t .. 4t + 3 of every row of the work-group's items
// (k_mlp_w1's split).  Two items' 16 loads of 16 bytes are issued before the first is used.  bpart's sums run over j ascending, as
// k_mlp_w1<false>'s do: the same bits.
struct MlpFoldArgs {
  const float* W;    // W1 [8 I][512]
  const float* E;    // [n_users][8], rows 0 and 1 read
  float* D;          // [I][512]
  double* bpart;     // [work-groups][8][512]
  int n_items;
};
__global__ __launch_bounds__(128) void k_mlp_fold(const MlpFoldArgs a) {
  const int t = threadIdx.x;
  const int j0 = blockIdx.x * MLP_W1_ITEMS, j1 = j0 + MLP_W1_ITEMS < a.n_items ? j0 + MLP_W1_ITEMS : a.n_items;
  double de[MLP_F];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) de[f] = (double)a.E[MLP_F + f] - (double)a.E[f];
  double bacc[MLP_F][4];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) bacc[f][q] = 0.0;
  }
  const float4* __restrict__ W4p = reinterpret_cast<const float4*>(a.W);
  float4* __restrict__ D4 = reinterpret_cast<float4*>(a.D);
  for (int j = j0; j < j1; j += 2) {
    const bool two = j + 1 < j1;   // (uniform)
    float4 w[2][MLP_F];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const size_t row0 = (size_t)(two || i == 0 ? j + i : j) * MLP_F * (MLP_H1 / 4) + t;   // (a lone last item is read twice, used once)
#pragma unroll
      for (int f = 0; f < MLP_F; ++f) w[i][f] = W4p[row0 + f * (MLP_H1 / 4)];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      if (i == 1 && !two) break;
      double d[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int f = 0; f < MLP_F; ++f) {
        const float wv[4] = {w[i][f].x, w[i][f].y, w[i][f].z, w[i][f].w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          d[q] = fma(de[f], (double)wv[q], d[q]);
          bacc[f][q] += (double)wv[q];
        }
      }
      D4[(size_t)(j + i) * (MLP_H1 / 4) + t] = make_float4((float)d[0], (float)d[1], (float)d[2], (float)d[3]);
    }
  }
  double* bp = a.bpart + (size_t)blockIdx.x * MLP_F * MLP_H1 + 4 * t;
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) bp[f * MLP_H1 + q] = bacc[f][q];
  }
}

// base[c] = b1[c] + sum_f E[0][f] B_f[c] (k_mlp_z1's chain, rounded once): grid 1, block 512
__global__ __launch_bounds__(512) void k_mlp_base(const float* __restrict__ E, const float* __restrict__ b1, const double* __restrict__ bsum,
                                                  float* __restrict__ base) {
  const int c = threadIdx.x;
  double z = (double)b1[c];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) z = fma((double)E[f], bsum[f * MLP_H1 + c], z);
  base[c] = (float)z;
}

// a1 = relu(base + sum of the row's rows of D): the body of k_encode_csr_checked with the ReLU in the place of normalise + tanh
template <int TPR, int NV, int U>
__global__ __launch_bounds__(256) void k_mlp_rows_relu(const EncodeCsrArgs a) { encode_csr_rows<TPR, NV, U, true, ENC_ACT_RELU>(a); }

// grid b, block 256: row r of the batch.  out: the batch's [b][n_items] (probabilities, or logits with `logits` set).  A dead row's
// output is zeroed.  rowsse null: nothing else; else rowsse[r] = sum_j p^2 - sum_{checked entries} (2 p - 1), float64: every thread
// its columns / entries t, t + 256, .. in ascending order, then the tree.
struct MlpSseArgs {
  CsrBatch csr;
  int64_t nnz;
  float* out;
  double* rowsse;   // this batch's slots, or null
  int logits;
};
__global__ __launch_bounds__(256) void k_mlp_sse(const MlpSseArgs a) {
  __shared__ double red[256];
  const int r = blockIdx.x, t = threadIdx.x, I = a.csr.n_items;
  // csr_row_span's tests and the gather's against nnz, spelt out: a DEAD row and an empty one must be told apart here (the gather has
  // raised the word)
  const int64_t src = a.csr.rows ? a.csr.rows[r] : a.csr.row0 + r;
  bool dead = src < 0 || src >= a.csr.n_rows;
  CsrSpan s{src, 0, 0};
  if (!dead) {
    s.p0 = a.csr.indptr[src]; s.p1 = a.csr.indptr[src + 1];
    dead = s.p0 < 0 || s.p1 < s.p0 || s.p1 > a.nnz;
  }
  float* __restrict__ row = a.out + (size_t)r * I;
  if (dead) {   // (uniform)
    for (int c = t; c < I; c += 256) row[c] = 0.f;
    if (a.rowsse && t == 0) a.rowsse[r] = 0.0;
    return;
  }
  if (!a.rowsse) return;
  double acc = 0.0;
  for (int c = t; c < I; c += 256) {
    const float p = a.logits ? sigmoid_f(row[c]) : row[c];
    acc = fma((double)p, (double)p, acc);
  }
  bool bad = false;
  for (int64_t q = s.p0 + t; q < s.p1; q += 256) {
    int32_t col; float val;
    if (!csr_entry(a.csr, q, bad, col, val)) continue;
    const float p = a.logits ? sigmoid_f(row[col]) : row[col];
    acc -= 2.0 * (double)p - 1.0;
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  const double z = encode_block_sum(acc, red);
  if (t == 0) a.rowsse[r] = z;
}

// *sse = the n per-row values: thread t adds its stretch of ceil(n / 256) consecutive rows in order, thread 0 the 256 stretches in order
__global__ __launch_bounds__(256) void k_mlp_sse_sum(const double* __restrict__ rowsse, int64_t n, double* __restrict__ sse) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int64_t len = (n + 255) / 256, q0 = t * len, q1 = q0 + len < n ? q0 + len : n;
  double s = 0.0;
  for (int64_t q = q0; q < q1; ++q) s += rowsse[q];
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    double z = 0.0;
    for (int i = 0; i < 256; ++i) z += red[i];
    *sse = z;
  }
}

}  // namespace sdrm
