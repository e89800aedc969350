// The NeuMF evaluator's TRAIN step on the device: NeuMF-end in TRAIN MODE (reference: neural_cf_benchmark_pt.py:125-144 with dropout on,
// as the train loop :195-200 calls it: forward, BCEWithLogitsLoss, backward, Adam).  For the pairs j = 0 .. b - 1 of a batch, factor F:
//   x0 = [Pm[u_j]; Qm[i_j]]   a0 = k0 s x0            (8F)
//   z1 = W1 a0 + b1           a1 = k1 s relu(z1)      (4F)
//   z2 = W2 a1 + b2           a2 = k2 s relu(z2)      (2F)
//   z3 = W3 a2 + b3           h3 = relu(z3)           (F)
//   g  = Pg[u_j] * Qg[i_j]    y  = wp [g; h3] + bp
//   loss = mean_j(max(y, 0) - y l + log1p(exp(-|y|)))   dy_j = (sigmoid(y_j) - l_j) / b
// with s = 1 / (1 - p_drop) and k0 / k1 / k2 the keep decisions of the three Dropout modules.  The layer-1 split of the evaluator
// (csrc/neumf.h) does not apply: dropout sits on the concatenated input of every pair, so layer 1 is a full 8F x 4F product per pair.
// FACTORS: 8 (what the driver uses; the shapes below are chosen for it) and 16 through the same template.  Factor 32 is REFUSED by the
// entry point (SDRM_ERR_SHAPE): a lane would hold 256 layer-1 inputs in registers and a weight-gradient work-group 256 operand rows in
// LDS, neither of which this cut of the work is made for.
// A step is four launches:
//   k_nt_pairs  a lane owns ONE PAIR (one wave per work-group, so a batch of 256 spreads over four compute units): ids range-checked
//               once (FEED_BAD_ROW for a user, FEED_BAD_COL for an item; such a pair loads row 0, stores zeros everywhere and so adds
//               nothing to the loss or to any gradient - the divisor b still counts it), gather, the three dropout layers, the tower,
//               the loss term, dy, and the backward through the tower down to the two embedding rows.  Every weight a lane multiplies
//               with is wave-uniform (const __restrict__ kernel arguments at uniform addresses: scalar loads, scalar FMA operands, as
//               in csrc/neumf.h); the lane's own operands of a layer sit in registers (constant indices: the k loop is unrolled), the
//               outputs of a layer are walked four at a time by a rolled loop and go to the step's workspace, column-major [column][NT_LD]
//               so that the 64 lanes store one line, from where the lane reads them back as the next layer's operands.  What the
//               gradient launch needs is exactly what lies there afterwards: the layer inputs a0, a1, a2, [g; h3], the seeds dz1, dz2,
//               dz3, dy, the per-pair gradients of the two embedding rows (4F MLP + F GMF floats a side), the loss terms, the checked ids.
//               ReLU' and the dropout of a layer are read off its stored input: a_k > 0 iff the value was kept and its z was > 0.
//   k_nt_grads  three kinds of work-groups in one launch.  (1) weight gradients: 256 adjacent elements of one layer's [OUT][IN + 1]
//               (column IN is the bias), the layer's operand rows staged through LDS 64 pairs at a time, each element ONE compensated
//               (Kahan) fp32 sum over the pairs in ascending order: a plain fp32 chain over 256 signed terms loses four to eight times
//               what torch's blocked sums lose on the bias gradients, the compensated one loses nothing beyond its inputs' rounding.
//               (2) table rows: a thread owns (pair, column) of a side; the FIRST pair of the batch that names a row sums the contributions of every pair naming it, in ascending pair order, and writes the row of the
//               dense table gradient - later pairs of the same id write nothing.  (3) the loss: the b fp32 terms added in float64 by
//               a fixed tree (thread t takes t, t + 256, .., then k_neumf_loss_sum's tree), divided by b.
//   k_vae_adam  (csrc/vae_adam.h) torch.optim.Adam's dense form over all twelve tensors in one launch, l2 = 0.  Dense: a table row that
//               is not in the batch still moves while its moments are non-zero.
//   k_nt_clear  the rows the step wrote into the dense table gradients, zeroed again: the tables are never memset per step.
// Arithmetic is fp32, every reduction has a fixed order, there is no floating-point atomic: two runs give the same bits.
// Dropout, both modes by the same decision "keep iff word >= floor(p_drop 2^32)" (the scheme of PURPOSE_VAE_DROP): column c of the
// 14F columns of a pair (k0: 0 .. 8F - 1, k1: the next 4F, k2: the next 2F) at position j of the CALL's triple array is, in PHILOX
// mode, word c & 3 of Philox4x32-10 with counter (j, c >> 2, PURPOSE_NEUMF_DROP, call_id) and key seed; in EXPLICIT mode byte
// keep[j][c] != 0.  The backward regenerates the layer-0 decisions; the others are read off the stored activations.
// No address is trusted (csrc/csr_batch.h).  Plain HIP, vector / plain C++ stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "philox.h"

namespace sdrm {

constexpr int NT_LD = 1024;         // pairs of a step at most = the leading dimension of the step's column-major workspace
constexpr int NT_PAIR_BLOCK = 64;   // pairs of a work-group of k_nt_pairs (one wave)
constexpr int NT_CHUNK = 64;        // pairs staged at a time by a weight-gradient work-group

// columns of the step's workspace (4-byte words, NT_LD a column)
template <int F> struct NtCols {
  static constexpr int A0 = 0, A1 = A0 + 8 * F, A2 = A1 + 4 * F, AP = A2 + 2 * F;          // layer inputs: a0, a1, a2, [g; h3]
  static constexpr int DZ1 = AP + 2 * F, DZ2 = DZ1 + 4 * F, DZ3 = DZ2 + 2 * F, DY = DZ3 + F;   // seeds
  static constexpr int DU = DY + 1, DI = DU + 5 * F;                                       // per-pair row gradients: [4F MLP | F GMF] a side
  static constexpr int LT = DI + 5 * F, UID = LT + 1, IID = UID + 1, COUNT = IID + 1;      // loss terms; checked ids (int, -1: dead pair)
};

struct NtDrop {
  const uint8_t* row;   // EXPLICIT: this pair's 14F bytes; null: PHILOX
  uint32_t j, k0, k1, call_id, thr;
};

// the keep decisions of columns 4q .. 4q + 3 of a pair
__device__ __forceinline__ void nt_keep4(const NtDrop& d, int q, bool (&k)[4]) {
  if (d.row) {
#pragma unroll
    for (int t = 0; t < 4; ++t) k[t] = d.row[4 * q + t] != 0;
  } else {
    const U4 w = philox4x32_10(d.j, (uint32_t)q, PURPOSE_NEUMF_DROP, d.call_id, d.k0, d.k1);
    k[0] = w.x >= d.thr; k[1] = w.y >= d.thr; k[2] = w.z >= d.thr; k[3] = w.w >= d.thr;
  }
}

struct NtPairArgs {
  const int32_t* triples;   // this step's [b][3]: user, item, label
  const uint8_t* keep;      // this step's [b][14F], or null (PHILOX)
  float* ws;                // the step's workspace [NtCols::COUNT][NT_LD]
  unsigned* flag;
  int b, n_users, n_items;
  uint32_t j0;              // position of the step's first pair in the call's triple array
  uint32_t k0, k1, call_id, thr;
  float s;                  // 1 / (1 - p_drop)
};

// The FORWARD's dot products are compensated fp32 dot products (Ogita / Rump / Oishi's Dot2: the product's rounding error from one fma,
// the addition's from TwoSum, both collected in a second fp32 word that is added once at the end): a z is then the correctly rounded
// fp32 value of bias + sum_k w_k a_k in all but rare cases, as if it had been summed in twice the precision, in fp32 operations only
// and in ascending k.  The logit's accuracy is what the loss and, through sigmoid'(y), every gradient rest on: a plain fmaf chain over
// the 128 inputs of layer 1 at F = 16 loses about four times what torch's blocked GEMM loses, runs of 16 as much as torch - and the
// loss of a step is held to 4 x the reference's own deviation, which on a lucky step is an eighth of float32's half-ulp.  With exact
// dot products what is left in the logit is the one rounding of each stored activation.
// One term: (s, c) += w x.  Contraction is off: TwoSum needs t = fl(s + p) with p the ROUNDED product.
__device__ __forceinline__ void nt_dot2_step(float w, float x, float& s, float& c) {
#pragma clang fp contract(off)
  const float p = w * x;
  const float e = fmaf(w, x, -p);   // exact: w x - p
  const float t = s + p;
  const float bb = t - s;
  const float err = (s - (t - bb)) + (p - bb);   // exact: (s + p) - t
  s = t;
  c += e + err;
}

// The BACKWARD's dot products are cut into runs of NT_RUN terms: each run is one fmaf chain in ascending index from +0, the runs are
// added by a fixed pairwise tree.  The order is fixed: the same bits on every run and in every split of a call.
constexpr int NT_RUN = 16;
template <int N> struct NtRuns {
  static constexpr int LEN = N < NT_RUN ? N : NT_RUN, COUNT = N / LEN;   // (N is F or 2F, 4F, 8F: COUNT is a power of two)
};
template <int NC>
__device__ __forceinline__ float nt_tree(float (&p)[NC]) {
#pragma unroll
  for (int st = 1; st < NC; st *= 2) {
#pragma unroll
    for (int c = 0; c + st < NC; c += 2 * st) p[c] += p[c + st];
  }
  return p[0];
}

// One layer forward for the lane's pair: OUT outputs four at a time from IN operands in registers; out = keep ? relu(z) s : 0 (DROP),
// relu(z) otherwise, stored to column col0 + o.
template <int IN, int OUT, bool DROP>
__device__ __forceinline__ void nt_layer_fwd(const float* __restrict__ w, const float* __restrict__ bias, const float (&x)[IN], const NtDrop& d,
                                             int quad0, float s, bool live, float* __restrict__ ws, int col0) {
#pragma unroll 1
  for (int oq = 0; oq < OUT / 4; ++oq) {
    float z[4], lo[4];   // four independent compensated chains, interleaved
#pragma unroll
    for (int t = 0; t < 4; ++t) { z[t] = bias[4 * oq + t]; lo[t] = 0.f; }
#pragma unroll
    for (int k = 0; k < IN; ++k) {
#pragma unroll
      for (int t = 0; t < 4; ++t) nt_dot2_step(w[(4 * oq + t) * IN + k], x[k], z[t], lo[t]);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) z[t] += lo[t];
    bool kp[4] = {true, true, true, true};
    if (DROP) nt_keep4(d, quad0 + oq, kp);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const float h = fmaxf(z[t], 0.f);
      const float v = DROP ? (kp[t] ? h * s : 0.f) : h;
      ws[(size_t)(col0 + 4 * oq + t) * NT_LD] = live ? v : 0.f;
    }
  }
}

// One layer backward: da[k] = sum_o w[o][k] dz[o] (runs over o, as above) for the IN inputs four at a time from the OUT seeds in registers.
template <int IN, int OUT>
__device__ __forceinline__ void nt_layer_dgrad4(const float* __restrict__ w, const float (&dz)[OUT], int kq, float (&acc)[4]) {
  using R = NtRuns<OUT>;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    float part[R::COUNT];
#pragma unroll
    for (int c = 0; c < R::COUNT; ++c) {
      part[c] = 0.f;
#pragma unroll
      for (int oo = 0; oo < R::LEN; ++oo) part[c] = fmaf(w[(c * R::LEN + oo) * IN + 4 * kq + t], dz[c * R::LEN + oo], part[c]);
    }
    acc[t] = nt_tree<R::COUNT>(part);
  }
}

template <int N>
__device__ __forceinline__ void nt_load_cols(const float* __restrict__ ws, int col0, float (&x)[N]) {
#pragma unroll
  for (int k = 0; k < N; ++k) x[k] = ws[(size_t)(col0 + k) * NT_LD];
}

template <int F>
__global__ __launch_bounds__(NT_PAIR_BLOCK) void k_nt_pairs(const float* __restrict__ pg, const float* __restrict__ qg, const float* __restrict__ pm,
                                                            const float* __restrict__ qm, const float* __restrict__ w1, const float* __restrict__ b1,
                                                            const float* __restrict__ w2, const float* __restrict__ b2, const float* __restrict__ w3,
                                                            const float* __restrict__ b3, const float* __restrict__ wp, const float* __restrict__ bp,
                                                            const NtPairArgs a) {
  using C = NtCols<F>;
  const int j = blockIdx.x * NT_PAIR_BLOCK + threadIdx.x;
  if (j >= a.b) return;
  float* __restrict__ ws = a.ws + j;
  const int u = a.triples[(size_t)3 * j], i = a.triples[(size_t)3 * j + 1];
  const float lab = (float)a.triples[(size_t)3 * j + 2];
  const bool uok = u >= 0 && u < a.n_users, iok = i >= 0 && i < a.n_items, live = uok && iok;
  if (!uok) atomicOr(a.flag, (unsigned)FEED_BAD_ROW);
  if (!iok) atomicOr(a.flag, (unsigned)FEED_BAD_COL);
  const size_t ur = live ? (size_t)u : 0, ir = live ? (size_t)i : 0;   // (a dead pair reads row 0 and stores zeros)
  reinterpret_cast<int*>(ws)[(size_t)C::UID * NT_LD] = live ? u : -1;
  reinterpret_cast<int*>(ws)[(size_t)C::IID * NT_LD] = live ? i : -1;
  const NtDrop d{a.keep ? a.keep + (size_t)j * 14 * F : nullptr, a.j0 + (uint32_t)j, a.k0, a.k1, a.call_id, a.thr};
  const float s = a.s;

  {   // layer 1 from the gathered rows
    float a0[8 * F];
    const float* __restrict__ xu = pm + ur * 4 * F;
    const float* __restrict__ xi = qm + ir * 4 * F;
#pragma unroll
    for (int q = 0; q < 2 * F; ++q) {
      bool kp[4];
      nt_keep4(d, q, kp);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int c = 4 * q + t;
        const float x = c < 4 * F ? xu[c] : xi[c - 4 * F];
        a0[c] = kp[t] ? x * s : 0.f;
        ws[(size_t)(C::A0 + c) * NT_LD] = live ? a0[c] : 0.f;
      }
    }
    nt_layer_fwd<8 * F, 4 * F, true>(w1, b1, a0, d, 2 * F, s, live, ws, C::A1);
  }
  {
    float a1[4 * F];
    nt_load_cols<4 * F>(ws, C::A1, a1);
    nt_layer_fwd<4 * F, 2 * F, true>(w2, b2, a1, d, 3 * F, s, live, ws, C::A2);
  }
  {
    float a2[2 * F];
    nt_load_cols<2 * F>(ws, C::A2, a2);
    nt_layer_fwd<2 * F, F, false>(w3, b3, a2, d, 0, s, live, ws, C::AP + F);
  }
  // the GMF branch, the logit, the loss term and dy
  float pu[F], qi[F], h3[F];
  nt_load_cols<F>(ws, C::AP + F, h3);
  float y = bp[0], ylo = 0.f;   // the predict layer: one compensated chain from the bias, the GMF half first
#pragma unroll
  for (int k = 0; k < F; ++k) {
    pu[k] = pg[ur * F + k];
    qi[k] = qg[ir * F + k];
    const float g = pu[k] * qi[k];
    ws[(size_t)(C::AP + k) * NT_LD] = live ? g : 0.f;
    nt_dot2_step(wp[k], g, y, ylo);
  }
#pragma unroll
  for (int k = 0; k < F; ++k) nt_dot2_step(wp[F + k], h3[k], y, ylo);
  y += ylo;
  // the loss term: an fp32 value, the correctly rounded one - its three parts are evaluated in float64 from the fp32 logit, so that the
  // terms of a batch of near-equal logits (the first steps of a fresh model) do not share one transcendental's rounding
  const double yd = (double)y;
  const float term = (float)(fmax(yd, 0.0) - yd * (double)lab + log1p(exp(-fabs(yd))));
  ws[(size_t)C::LT * NT_LD] = live ? term : 0.f;
  // sigmoid(y) - l without the cancellation at a saturated logit: (1 - l) sigmoid(y) - l sigmoid(-y), both sigmoids from t = exp(-|y|)
  // (for a label of 0 or 1 one of the two terms is exactly zero)
  const float et = expf(-fabsf(y));
  const float sig_hi = 1.f / (1.f + et), sig_lo = et / (1.f + et);   // sigmoid(|y|), sigmoid(-|y|)
  const float sp = y >= 0.f ? sig_hi : sig_lo, sn = y >= 0.f ? sig_lo : sig_hi;
  const float dy = live ? ((1.f - lab) * sp - lab * sn) / (float)a.b : 0.f;
  ws[(size_t)C::DY * NT_LD] = dy;
  // backward: the predict layer's two halves
  float dz3[F];
#pragma unroll
  for (int k = 0; k < F; ++k) {
    const float dg = dy * wp[k];
    ws[(size_t)(C::DU + 4 * F + k) * NT_LD] = live ? dg * qi[k] : 0.f;
    ws[(size_t)(C::DI + 4 * F + k) * NT_LD] = live ? dg * pu[k] : 0.f;
    dz3[k] = h3[k] > 0.f ? dy * wp[F + k] : 0.f;
    ws[(size_t)(C::DZ3 + k) * NT_LD] = dz3[k];
  }
  // ... and down the tower
#pragma unroll 1
  for (int kq = 0; kq < 2 * F / 4; ++kq) {
    float acc[4];
    nt_layer_dgrad4<2 * F, F>(w3, dz3, kq, acc);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const size_t c = (size_t)(4 * kq + t) * NT_LD;
      ws[(size_t)C::DZ2 * NT_LD + c] = ws[(size_t)C::A2 * NT_LD + c] > 0.f ? acc[t] * s : 0.f;
    }
  }
  {
    float dz2[2 * F];
    nt_load_cols<2 * F>(ws, C::DZ2, dz2);
#pragma unroll 1
    for (int kq = 0; kq < 4 * F / 4; ++kq) {
      float acc[4];
      nt_layer_dgrad4<4 * F, 2 * F>(w2, dz2, kq, acc);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const size_t c = (size_t)(4 * kq + t) * NT_LD;
        ws[(size_t)C::DZ1 * NT_LD + c] = ws[(size_t)C::A1 * NT_LD + c] > 0.f ? acc[t] * s : 0.f;
      }
    }
  }
  {
    float dz1[4 * F];
    nt_load_cols<4 * F>(ws, C::DZ1, dz1);
#pragma unroll 1
    for (int kq = 0; kq < 8 * F / 4; ++kq) {
      float acc[4];
      nt_layer_dgrad4<8 * F, 4 * F>(w1, dz1, kq, acc);
      bool kp[4];
      nt_keep4(d, kq, kp);
      const int col0 = kq < F ? C::DU + 4 * kq : C::DI + 4 * (kq - F);   // the first 4F inputs are the user's row, the others the item's
#pragma unroll
      for (int t = 0; t < 4; ++t) ws[(size_t)(col0 + t) * NT_LD] = live && kp[t] ? acc[t] * s : 0.f;
    }
  }
}

// acc += y where y is the next term less what was lost so far; `lost` becomes what THIS addition rounds away.  The order of the three
// operations is the algorithm: contraction may not reassociate them (and fp contraction does not).
__device__ __forceinline__ void nt_kahan_add(float& acc, float& lost, float y) {
  const float t = acc + y;
  lost = (t - acc) - y;
  acc = t;
}

struct NtLayerJob {
  const float* A;    // inputs  [IN][NT_LD]
  const float* DZ;   // seeds   [OUT][NT_LD]
  float* dW;         // [OUT][IN]
  float* db;         // [OUT]
  int IN, OUT, first_block;
};
struct NtGradArgs {
  NtLayerJob layer[4];   // layers 1, 2, 3 and the predict layer
  int w_blocks;          // work-groups of the weight gradients; the table rows follow, then the loss
  const int* ids[2];     // checked ids of the users / the items [b] (-1: dead pair)
  const float* D[2];     // per-pair row gradients of the side [5F][NT_LD]
  float* g_mlp[2];       // dense table gradients [n_rows][4F]
  float* g_gmf[2];       // [n_rows][F]
  int row_blocks;        // work-groups of ONE side
  const float* lt;       // loss terms [b]
  double* loss;          // this step's slot, or null: no such work-group
  int b;
};

template <int F>
__global__ __launch_bounds__(256) void k_nt_grads(const NtGradArgs a) {
  constexpr int LDS_LD = NT_CHUNK + 1;   // (odd: the 64 lanes of a wave read 64 rows of one column without a bank conflict beyond the wave's two halves)
  constexpr int DROWS = 18;              // rows of seeds 256 adjacent elements of [OUT][IN + 1] can span: IN + 1 >= 17
  __shared__ float As[8 * F * LDS_LD];
  __shared__ float Ds[DROWS * LDS_LD];
  __shared__ int ids[NT_LD];
  __shared__ double red[256];
  const int blk = blockIdx.x, t = threadIdx.x, b = a.b;
  if (blk < a.w_blocks) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (a.layer[q].first_block <= blk) l = q;
    const NtLayerJob& L = a.layer[l];
    const int IN = L.IN, W = IN + 1, total = L.OUT * W;
    const int e0 = (blk - L.first_block) * 256, e = e0 + t;
    const int o_lo = e0 / W;
    const int e_hi = e0 + 255 < total - 1 ? e0 + 255 : total - 1;
    const int n_o = e_hi / W - o_lo + 1;   // <= DROWS
    const bool mine = e < total;
    const int o = mine ? e / W : o_lo, k = mine ? e % W : 0;
    float acc = 0.f, lost = 0.f;   // compensated (Kahan) sum: `lost` is what the additions so far have rounded away
    for (int j0 = 0; j0 < b; j0 += NT_CHUNK) {
      const int jn = b - j0 < NT_CHUNK ? b - j0 : NT_CHUNK;
      __syncthreads();
      for (int idx = t; idx < IN * NT_CHUNK; idx += 256) {
        const int r = idx / NT_CHUNK, jj = idx % NT_CHUNK;
        As[r * LDS_LD + jj] = jj < jn ? L.A[(size_t)r * NT_LD + j0 + jj] : 0.f;
      }
      for (int idx = t; idx < n_o * NT_CHUNK; idx += 256) {
        const int r = idx / NT_CHUNK, jj = idx % NT_CHUNK;
        Ds[r * LDS_LD + jj] = jj < jn ? L.DZ[(size_t)(o_lo + r) * NT_LD + j0 + jj] : 0.f;
      }
      __syncthreads();
      const float* __restrict__ dr = Ds + (o - o_lo) * LDS_LD;
      if (k < IN) {
        const float* __restrict__ ar = As + k * LDS_LD;
        for (int jj = 0; jj < jn; ++jj) nt_kahan_add(acc, lost, fmaf(dr[jj], ar[jj], -lost));   // (the product enters unrounded)
      } else {
        for (int jj = 0; jj < jn; ++jj) nt_kahan_add(acc, lost, dr[jj] - lost);
      }
    }
    if (mine) {
      if (k < IN) L.dW[(size_t)o * IN + k] = acc;
      else L.db[o] = acc;
    }
    return;
  }
  const int rb = blk - a.w_blocks;
  if (rb < 2 * a.row_blocks) {
    const int side = rb / a.row_blocks;
    const int* __restrict__ gid = a.ids[side];
    for (int q = t; q < b; q += 256) ids[q] = gid[q];
    __syncthreads();
    const int e = (rb % a.row_blocks) * 256 + t;
    const int j = e / (5 * F), c = e % (5 * F);
    if (j >= b) return;
    const int id = ids[j];
    if (id < 0) return;
    for (int q = 0; q < j; ++q)
      if (ids[q] == id) return;   // an earlier pair names the row: it owns the sum
    const float* __restrict__ col = a.D[side] + (size_t)c * NT_LD;
    float acc = 0.f;
    for (int q = j; q < b; ++q)
      if (ids[q] == id) acc += col[q];
    if (c < 4 * F) a.g_mlp[side][(size_t)id * 4 * F + c] = acc;
    else a.g_gmf[side][(size_t)id * F + (c - 4 * F)] = acc;
    return;
  }
  // the loss: thread t adds the terms t, t + 256, .. in that order, then k_neumf_loss_sum's tree
  double s = 0.0;
  for (int q = t; q < b; q += 256) s += (double)a.lt[q];
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) *a.loss = red[0] / (double)b;
}

// the rows of the dense table gradients that the step's pairs name, zeroed again (a row named twice is zeroed twice)
template <int F>
__global__ __launch_bounds__(256) void k_nt_clear(const int* __restrict__ uid, const int* __restrict__ iid, float* __restrict__ gu_mlp,
                                                  float* __restrict__ gu_gmf, float* __restrict__ gi_mlp, float* __restrict__ gi_gmf, int b) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  const int side = e / (b * 5 * F), r = e % (b * 5 * F);
  if (side > 1) return;
  const int j = r / (5 * F), c = r % (5 * F);
  const int id = side == 0 ? uid[j] : iid[j];
  if (id < 0) return;
  float* mlp = side == 0 ? gu_mlp : gi_mlp;
  float* gmf = side == 0 ? gu_gmf : gi_gmf;
  if (c < 4 * F) mlp[(size_t)id * 4 * F + c] = 0.f;
  else gmf[(size_t)id * F + (c - 4 * F)] = 0.f;
}

}  // namespace sdrm
