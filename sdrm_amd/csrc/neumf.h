// The NeuMF evaluator's forward on the device: NeuMF-end in EVAL MODE (reference: neural_cf_benchmark_pt.py:125-144 with dropout off, as
// the per-epoch evaluation :203-246 and the testing block :294-332 call it).  For a user u and an item i, factor F, three MLP layers:
//   g  = Pg[u] * Qg[i]                       (F products)
//   h1 = relu(W1 [Pm[u]; Qm[i]] + b1)        (8F -> 4F)
//   h2 = relu(W2 h1 + b2)                    (4F -> 2F)
//   h3 = relu(W3 h2 + b3)                    (2F -> F)
//   y  = wp [g; h3] + bp                     (2F -> 1)
// Layer 1 is linear in the concatenation, so it is split and staged per listed id, not per pair:
//   k_neumf_stage   A[u] = b1 + W1[:, :4F] Pm[u] for the listed users, B[i] = W1[:, 4F:] Qm[i] for the listed items, with Pg[u] / Qg[i]
//                   copied behind them (5F floats per id), a validity word per id, and W2, W3 transposed (W2t [4F][2F], W3t [2F][F]: the
//                   towers walk k outermost and want the 2F / F weights of one k side by side).  One launch.  An id outside its table
//                   raises the feed status word (FEED_BAD_ROW for a user, FEED_BAD_COL for an item), stages a zero row and reads nothing.
//   h1 = relu(A[u] + B[i]) then costs 4F adds per pair instead of 8F x 4F multiply-adds: of the 42F^2 + 2F multiply-adds of a pair,
//   10F^2 + 2F remain (8F^2 of layer 2, 2F^2 of layer 3, 2F of the predict layer) beside the F GMF products.
//   k_neumf_scores  dense out[U][I] for listed users x listed items.  A lane owns ONE ITEM (its B column comes from the transposed
//                   staging by coalesced loads and its stores are coalesced along the row), a work-group owns 256 items x 16 users and
//                   walks the users NU at a time.  Everything else a lane multiplies with is wave-uniform: A[u] and Pg[u] (row-major
//                   staging, uniform row), W2t, W3t, wp, the biases - const __restrict__ kernel arguments at uniform addresses, which
//                   the compiler turns into scalar loads and scalar FMA operands.  NU users share each weight operand.
//   k_neumf_pairs   n listed pairs, a lane owns one pair: both sides staged per pair in the transposed form; logits, and the per-block
//                   float64 partial of the BCE-with-logits numerator  max(x, 0) - x y + log1p(exp(-|x|)).
//   k_neumf_loss_sum  the partials added in a fixed order by one work-group: no float atomic, the same bits on every run.
// Arithmetic: fp32; every output element of every layer is ONE fmaf chain in ascending k that starts from the bias (B[i], which has no
// bias, starts from +0).  All three kernels call the same chain (neumf_tower / the staging loop), so a logit has the same bits whichever
// kernel made it, wherever its pair sits in a tile, and however a call was split.  fp32 vector FMAs: on gfx950 the fp32 MFMA rate equals
// the fp32 vector rate, and 4F x 2F per pair with per-pair operands is no GEMM.
// No address is trusted (csrc/csr_batch.h): ids are checked in the staging kernel, the towers read staged rows only, tail lanes clamp
// their loads to the last valid row / column and store nothing.  Plain HIP, vector / plain C++ stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"

namespace sdrm {

constexpr int NEUMF_ITEM_TILE = 256;    // items of a work-group of k_neumf_scores (one per lane)
constexpr int NEUMF_USER_TILE = 16;     // users of a work-group of k_neumf_scores
constexpr int NEUMF_PAIR_CHUNK = 1 << 16;   // pairs staged at a time by sdrm_neumf_pair_loss (a multiple of 256)
template <int F> struct NeumfShape {
  static constexpr int NU = F == 8 ? 4 : F == 16 ? 2 : 1;   // users per pass: 2F x NU = 64 accumulators of layer 2 in all three shapes
  static constexpr int ROW = 5 * F;                          // floats staged per id: 4F of the split layer 1, F of the GMF table
};

struct NeumfStageSide {
  const float* emb_mlp;    // [n_rows][4F]
  const float* emb_gmf;    // [n_rows][F]
  const int32_t* ids;      // [n] (null: 0 .. n - 1)
  int n, n_rows;
  float* out;              // transposed: [5F][ld], else [n][5F]
  int* valid;              // [n] 1 / 0
  int64_t ld;
  int transposed, w1_off;  // W1's column offset of this side (0 users, 4F items)
  unsigned bad_bit;
};
struct NeumfStageArgs {
  NeumfStageSide side[2];  // users, items
  const float *w1, *b1, *w2, *w3;
  float *w2t, *w3t;
  unsigned* flag;
  int blocks[2];           // work-groups of the two sides; the transposes follow
};

template <int F>
__global__ __launch_bounds__(256) void k_neumf_stage(const NeumfStageArgs a) {
  constexpr int ROW = NeumfShape<F>::ROW;
  int blk = blockIdx.x, s = 0;
  if (blk >= a.blocks[0]) { blk -= a.blocks[0]; s = 1; }
  if (s == 1 && blk >= a.blocks[1]) {   // W2 [2F][4F] -> W2t [4F][2F], W3 [F][2F] -> W3t [2F][F]
    const int e = (blk - a.blocks[1]) * 256 + threadIdx.x;
    if (e < 8 * F * F) { const int k = e / (2 * F), o = e % (2 * F); a.w2t[e] = a.w2[o * 4 * F + k]; }
    else if (e < 10 * F * F) { const int e3 = e - 8 * F * F, k = e3 / F, o = e3 % F; a.w3t[e3] = a.w3[o * 2 * F + k]; }
    return;
  }
  const NeumfStageSide& sd = a.side[s];
  const int64_t e = (int64_t)blk * 256 + threadIdx.x;
  const int r = (int)(e / ROW), o = (int)(e % ROW);
  if (r >= sd.n) return;
  const int id = sd.ids ? sd.ids[r] : r;
  const bool ok = id >= 0 && id < sd.n_rows;
  float v = 0.f;
  if (ok) {
    if (o < 4 * F) {
      v = s == 0 ? a.b1[o] : 0.f;
      const float* __restrict__ w = a.w1 + (size_t)o * 8 * F + sd.w1_off;
      const float* __restrict__ x = sd.emb_mlp + (size_t)id * 4 * F;
#pragma unroll 8
      for (int k = 0; k < 4 * F; ++k) v = fmaf(w[k], x[k], v);
    } else {
      v = sd.emb_gmf[(size_t)id * F + (o - 4 * F)];
    }
  }
  if (o == 0) {
    sd.valid[r] = ok ? 1 : 0;
    if (!ok) atomicOr(a.flag, sd.bad_bit);
  }
  sd.out[sd.transposed ? (size_t)o * sd.ld + r : (size_t)r * ROW + o] = v;
}

// Layers 2, 3 and the predict layer of NU pairs that share their weight operands.  h1(j, k): relu(A + B)[k] of pair j; g(j, k): its
// GMF product.  Every accumulator is one fmaf chain in ascending k from its bias.
template <int F, int NU, class H1, class G>
__device__ __forceinline__ void neumf_tower(const float* __restrict__ w2t, const float* __restrict__ b2, const float* __restrict__ w3t,
                                            const float* __restrict__ b3, const float* __restrict__ wp, const float* __restrict__ bp,
                                            H1 h1, G g, float (&y)[NU]) {
  float h2[NU][2 * F];
#pragma unroll
  for (int o = 0; o < 2 * F; ++o) {
    const float b = b2[o];
#pragma unroll
    for (int j = 0; j < NU; ++j) h2[j][o] = b;
  }
#pragma unroll 2
  for (int k = 0; k < 4 * F; ++k) {
    float x[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) x[j] = h1(j, k);
    const float* __restrict__ w = w2t + k * 2 * F;
#pragma unroll
    for (int o = 0; o < 2 * F; ++o) {
      const float wv = w[o];
#pragma unroll
      for (int j = 0; j < NU; ++j) h2[j][o] = fmaf(wv, x[j], h2[j][o]);
    }
  }
  float h3[NU][F];
#pragma unroll
  for (int o = 0; o < F; ++o) {
    const float b = b3[o];
#pragma unroll
    for (int j = 0; j < NU; ++j) h3[j][o] = b;
  }
#pragma unroll
  for (int k = 0; k < 2 * F; ++k) {
    float x[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) x[j] = fmaxf(h2[j][k], 0.f);
#pragma unroll
    for (int o = 0; o < F; ++o) {
      const float wv = w3t[k * F + o];
#pragma unroll
      for (int j = 0; j < NU; ++j) h3[j][o] = fmaf(wv, x[j], h3[j][o]);
    }
  }
  const float b = bp[0];
#pragma unroll
  for (int j = 0; j < NU; ++j) y[j] = b;
#pragma unroll
  for (int k = 0; k < F; ++k) {
    const float wv = wp[k];
#pragma unroll
    for (int j = 0; j < NU; ++j) y[j] = fmaf(wv, g(j, k), y[j]);
  }
#pragma unroll
  for (int k = 0; k < F; ++k) {
    const float wv = wp[F + k];
#pragma unroll
    for (int j = 0; j < NU; ++j) y[j] = fmaf(wv, fmaxf(h3[j][k], 0.f), y[j]);
  }
}

// out [U][I]: blockIdx.x owns 256 items, blockIdx.y 16 users.  ua [U][5F] row-major (uniform rows), ibt [5F][ld] transposed.
template <int F>
__global__ __launch_bounds__(256) void k_neumf_scores(const float* __restrict__ ua, const int* __restrict__ uvalid, const float* __restrict__ ibt,
                                                      const int* __restrict__ ivalid, int64_t ld, const float* __restrict__ w2t,
                                                      const float* __restrict__ b2, const float* __restrict__ w3t, const float* __restrict__ b3,
                                                      const float* __restrict__ wp, const float* __restrict__ bp, int U, int I,
                                                      float* __restrict__ out) {
  constexpr int NU = NeumfShape<F>::NU, ROW = NeumfShape<F>::ROW;
  const int c = blockIdx.x * NEUMF_ITEM_TILE + threadIdx.x;
  const int cc = c < I ? c : I - 1;   // a tail lane computes its neighbour's column and stores nothing
  const bool iv = ivalid[cc] != 0;
  const float* __restrict__ bcol = ibt + cc;
  const int u0 = blockIdx.y * NEUMF_USER_TILE;
  const int u1 = u0 + NEUMF_USER_TILE < U ? u0 + NEUMF_USER_TILE : U;
  for (int u = u0; u < u1; u += NU) {
    const float* __restrict__ arow[NU];
#pragma unroll
    for (int j = 0; j < NU; ++j) arow[j] = ua + (size_t)(u + j < U ? u + j : U - 1) * ROW;
    float y[NU];
    neumf_tower<F, NU>(
        w2t, b2, w3t, b3, wp, bp, [&](int j, int k) { return fmaxf(arow[j][k] + bcol[(size_t)k * ld], 0.f); },
        [&](int j, int k) { return arow[j][4 * F + k] * bcol[(size_t)(4 * F + k) * ld]; }, y);
    if (c < I) {
#pragma unroll
      for (int j = 0; j < NU; ++j)
        if (u + j < u1) out[(size_t)(u + j) * I + c] = iv && uvalid[u + j] != 0 ? y[j] : 0.f;
    }
  }
}

// n listed pairs, both sides staged per pair in the transposed form [5F][ld].  logits, labels and part may each be null; part[block] is
// the block's float64 sum of the pairs' loss terms, added by a fixed tree.
template <int F>
__global__ __launch_bounds__(256) void k_neumf_pairs(const float* __restrict__ uat, const int* __restrict__ uvalid, const float* __restrict__ ibt,
                                                     const int* __restrict__ ivalid, int64_t ld, const float* __restrict__ w2t,
                                                     const float* __restrict__ b2, const float* __restrict__ w3t, const float* __restrict__ b3,
                                                     const float* __restrict__ wp, const float* __restrict__ bp,
                                                     const float* __restrict__ labels, int n, float* __restrict__ logits,
                                                     double* __restrict__ part) {
  __shared__ double red[256];
  const int p = blockIdx.x * 256 + threadIdx.x;
  const int pp = p < n ? p : n - 1;
  const float* __restrict__ acol = uat + pp;
  const float* __restrict__ bcol = ibt + pp;
  float y[1];
  neumf_tower<F, 1>(
      w2t, b2, w3t, b3, wp, bp, [&](int, int k) { return fmaxf(acol[(size_t)k * ld] + bcol[(size_t)k * ld], 0.f); },
      [&](int, int k) { return acol[(size_t)(4 * F + k) * ld] * bcol[(size_t)(4 * F + k) * ld]; }, y);
  const bool ok = p < n && uvalid[pp] != 0 && ivalid[pp] != 0;
  const float x = ok ? y[0] : 0.f;
  if (logits && p < n) logits[p] = x;
  if (part) {   // (uniform over the grid)
    float t = 0.f;
    if (ok) t = fmaxf(x, 0.f) - x * labels[pp] + log1pf(expf(-fabsf(x)));
    red[threadIdx.x] = (double)t;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
  }
}

// *sum = part[0] + .. + part[n_part - 1]: thread t adds part[t], part[t + 256], .. in that order, then the same fixed tree.
__global__ __launch_bounds__(256) void k_neumf_loss_sum(const double* __restrict__ part, int n_part, double* __restrict__ sum) {
  __shared__ double red[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_part; i += 256) s += part[i];
  red[threadIdx.x] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *sum = red[0];
}

}  // namespace sdrm
