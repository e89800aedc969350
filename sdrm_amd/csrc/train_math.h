// The arithmetic of a train step that every kernel path shares, written once (gfx950): the timestep draw, the per-quad randoms,
// the three staged inputs, the loss terms, the loss coefficients and the closed-form gradient seeds.  This file and
// oracle/philox_ref.py are the two places where a change to the randoms or to the loss is made.
// Reference lines (:n) are into the reference's train_SDRM.py.
//
// The contract (PHILOX mode; philox.h has the generator, oracle/philox_ref.py restates all of this in numpy):
//   * timestep of global row r (:327):  word x of the call (r, 0, PURPOSE_TRAIN_T, step), t = 1 + bounded(x, T), clamped to [0, T];
//   * one call per (global row, COLUMN QUAD) with PURPOSE_TRAIN_ELEM - counter word 1 is the quad, column / 4 - gives the four
//     words (x, y, z, w) of columns 4 q .. 4 q + 3:
//       - normals: box_muller(x, y) and box_muller(z, w) on the UPPER 24 bits of each word, times the noise scale nd; the three
//         passes of a user share them (:326);
//       - dropout (:100): the keep bit of pass p (0 = P, 1 = S, 2 = Q) of column j is bit p of word j.
//   EXPLICIT mode reads t [B], noise [B, L] and keep [3, B, L] instead.
//   * staged inputs (:328-333, :193-195):  P = 2 keep1 (sqrt(abar_t) x + (1 - abar_t) e),  S = 2 keep2 x,  Q = 2 keep3 (x + mu e);
//   * loss (:196-198):  R = P - x,  D = (Q - S) / mu^2 - R;  sums over the batch of D^2, (R - S)^2, R, R^2 and the count N give
//     loss = 0.5 (A + C) / (1e-8 + V) with A = mean D^2, C = mean (R - S)^2, V = the unbiased variance of R;
//   * seeds: d loss / d (P, S, Q) in closed form, times tanh' = 1 - y^2.
//
// Two things differ between the call sites ON PURPOSE, and every call site keeps the form it has always had (the paths are
// compared bit for bit with themselves across runs and shards, never with each other below the parity bars):
//   * 1 / mu^2.  RECIP = false, a division: k_prep_train's companions k_loss_partials and k_loss_seed (elementwise.h) and the
//     narrow-net kernels k_skinny_fwd, k_skinny_fwd4, k_skinny_bwd - a few elements per lane.  RECIP = true, a multiply by
//     1.f / MU2: the row-owned kernels k_row_fwd, k_rows48_fwd (rowchain.h, rows48.h: loss sums) and k_dgrad_chain,
//     k_rows48_dgrad_chain (dgrad_rows.h, rows48.h: seeds) - an IEEE division is ten instructions, 132 times per lane there.
//   * the fold of the forward's loss partials into the five sums.  block_sum4_seq (elementwise.h; k_loss_seed) and block_sum
//     per sum (the two chain kernels) are k_loss_sums' tree: waves in order.  k_skinny_bwd emulates that tree on wave 0 (its
//     work-group may have three waves).  block_sum4 (rowchain.h) is the row-owned forwards' own pairwise tree over four waves,
//     for the partials they WRITE.
// One kernel does not call the helpers: k_skinny_bwd keeps loss_coef and loss_seed<false> written out (skinny_step.h says why).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "philox.h"

namespace sdrm {

constexpr float MU = 0.1f;          // score_matching_loss(..., mu=.1), :333
constexpr float MU2 = 0.01f;        // mu ** 2, :196

// The helpers take the step's inputs as plain values (the fields of PrepTrainArgs, RowChainArgs, SkStepArgs of the same names),
// never a kernel's argument struct by reference and no register arrays of a whole thread: either changes the register allocation
// of a row-owned kernel as a whole, up to more VGPRs or scratch (measured: profiles/train_math_refactor.txt).  That is also why
// the staging and epilogue of k_row_fwd / k_rows48_fwd and the seed stage of the two chain kernels stay two texts each.

// the timestep of user `usr` (< B; the caller guards, stores it to tdev and picks the value of an empty slot)
__device__ __forceinline__ int train_timestep(int mode, const int64_t* t, int64_t row0, int usr, uint32_t step, uint32_t seed_lo,
                                              uint32_t seed_hi, int T) {
  int t0;
  if (mode == 0) {
    t0 = (int)t[usr];
  } else {
    const U4 w = philox4x32_10((uint32_t)(row0 + usr), 0u, PURPOSE_TRAIN_T, step, seed_lo, seed_hi);
    t0 = 1 + (int)bounded(w.x, (uint32_t)T);
  }
  return min(max(t0, 0), T);
}

// the raw words of (user, column quad): split from their decode so that a thread can issue all its calls in one straight-line
// block (a call is a serial chain of 10 rounds: rowchain.h, k_row_fwd's staging)
__device__ __forceinline__ U4 train_quad_draw(int64_t row0, int usr, int quad, uint32_t step, uint32_t seed_lo, uint32_t seed_hi) {
  return philox4x32_10((uint32_t)(row0 + usr), (uint32_t)quad, PURPOSE_TRAIN_ELEM, step, seed_lo, seed_hi);
}
// ... decoded: the quad's four scaled normals, and the four words whose bits 0 .. 2 are the columns' keep bits
__device__ __forceinline__ void train_quad_decode(const U4& w, float nd, float (&e)[4], uint32_t (&bits)[4]) {
  box_muller(w.x, w.y, e[0], e[1]);
  box_muller(w.z, w.w, e[2], e[3]);
#pragma unroll
  for (int j = 0; j < 4; ++j) e[j] *= nd;
  bits[0] = w.x; bits[1] = w.y; bits[2] = w.z; bits[3] = w.w;
}

// one element's three staged inputs (a lane that holds P, S and Q together)
__device__ __forceinline__ void stage_element(float x, float e, float sa, float om, bool k1, bool k2, bool k3, float& vP, float& vS,
                                              float& vQ) {
  vP = k1 ? 2.f * (sa * x + om * e) : 0.f;
  vS = k2 ? 2.f * x : 0.f;
  vQ = k3 ? 2.f * (x + MU * e) : 0.f;
}
// ... and the input of ONE pass (the narrow nets: a wave per pass)
__device__ __forceinline__ float stage_element_pass(int pass, float x, float e, float sa, float om, bool keep) {
  const float v = pass == 0 ? sa * x + om * e : (pass == 1 ? x : x + MU * e);
  return keep ? 2.f * v : 0.f;
}

// v / mu^2 in the call site's form (see the head of this file); V: float or a vector of floats
template <bool RECIP, class V>
__device__ __forceinline__ V over_mu2(V v) {
  if constexpr (RECIP) return v * (1.f / MU2);
  else return v / MU2;
}

// one element's four loss terms D^2, (R - S)^2, R, R^2, added to the caller's sums (Acc: float - a quad's or a lane's sums, which
// then go to the double sums - or double: the narrow-net kernels add every element in double)
template <bool RECIP, class Acc>
__device__ __forceinline__ void loss_terms(float P, float S, float Q, float x, Acc& sD, Acc& sC, Acc& sR, Acc& sR2) {
  const float R = P - x;
  const float D = over_mu2<RECIP>(Q - S) - R;
  const float RS = R - S;
  sD += (Acc)(D * D); sC += (Acc)(RS * RS); sR += (Acc)R; sR2 += (Acc)(R * R);
}

// the five sums -> the seeds' coefficients and the loss value
struct LossCoef { float cD, cV, rbar, loss; };
__device__ __forceinline__ LossCoef loss_coef(double s0, double s1, double s2, double s3, double N) {
  const double A = s0 / N, C = s1 / N, Rbar = s2 / N;
  // unbiased variance; a single element gives 0/0 = NaN exactly as torch.var does (train_SDRM.py:198)
  const double V = (N > 1.0) ? (s3 - N * Rbar * Rbar) / (N - 1.0) : __builtin_nan("");
  const double den = 1e-8 + V;
  const double k = 0.5 / den;
  LossCoef c;
  c.cD = (float)(2.0 * k / N);
  c.cV = (float)(-(0.5 * (A + C) / (den * den)) * 2.0 / (N - 1.0));
  c.rbar = (float)Rbar;
  c.loss = (float)(0.5 * (A + C) / den);
  return c;
}

// the seeds of one element (V = float) or of four columns at once (V = f32x4: the compiler pairs it into v_pk_mul / v_pk_add /
// v_pk_fma, two elements per instruction)
template <bool RECIP, class V>
__device__ __forceinline__ void loss_seed(V P, V S, V Q, V X, const LossCoef& k, V& gP, V& gS, V& gQ) {
  const V R = P - X;
  const V D = over_mu2<RECIP>(Q - S) - R;
  const V gD = k.cD * D;
  const V gC = k.cD * (R - S);
  const V gV = k.cV * (R - k.rbar);
  const V gDm = over_mu2<RECIP>(gD);
  gP = (-gD + gC + gV) * (1.f - P * P);
  gQ = gDm * (1.f - Q * Q);
  // (the division form negates gD before it divides, as its call sites always have: the same bits, another instruction sequence)
  gS = ((RECIP ? -gDm : over_mu2<RECIP>(-gD)) - gC) * (1.f - S * S);
}
// ... of the quad at columns col .. col + 3 (col < L), zero in the columns >= L
template <bool RECIP, class V4>
__device__ __forceinline__ void loss_seed_quad(V4 P, V4 S, V4 Q, V4 X, const LossCoef& k, int col, int L, V4& gP, V4& gS, V4& gQ) {
  loss_seed<RECIP>(P, S, Q, X, k, gP, gS, gQ);
#pragma unroll
  for (int i = 1; i < 4; ++i)
    if (col + i >= L) { gP[i] = 0.f; gQ[i] = 0.f; gS[i] = 0.f; }
}

}  // namespace sdrm
