// The MLP evaluator's TRAIN step on the device (reference: mlp_benchmark.py:37-62 the model, :85-110 compile and fit; restated in
// sdrm_amd/mlp_eval.py, which names the Keras facts).  For the rows r = 0 .. b - 1 of a batch (b <= 16), I items, the input 0 / 1:
//   a0[r, 8j + f] = E[x_rj][f]                                   (8 I, never in memory)
//   z1 = a0 W1 + b1      a1 = k1 s relu(z1)                      (512)
//   z2 = a1 W2 + b2      a2 = k2 s relu(z2)                      (256)
//   z3 = a2 W3 + b3      a3 = k3 s relu(z3)                      (256)
//   y  = a3 W4 + b4      loss = sum(max(y, 0) - y x + log1p(exp(-|y|))) / (b I)      dy = (sigmoid(y) - x) / (b I)
// followed by the gradients of all nine tensors and Keras's Adam.  Kernels are [in][out] as Keras stores them: W1's row 8j + f is 512
// contiguous floats and item j owns eight adjacent rows.
// What makes the step one pass over W1 and its moments:
//   forward   z1[r] = b1 + sum_f E[0][f] B_f + sum_{j in row r} sum_f (E[1][f] - E[0][f]) W1[8j + f],   B_f = sum_j W1[8j + f]  [512]
//             B_f of the weights as they stand is LEFT BEHIND by the update pass of the step before (the first step of a call makes it
//             with the same kernel in its read-only form, so a call of n steps gives the bits of n calls of one step).
//   backward  S = sum_r dz1[r], T_j = sum_{r: j in row r} dz1[r]:  dW1[8j + f] = E[0][f] S + (E[1][f] - E[0][f]) T_j  - made per element
//             inside the Adam pass and never stored (but into grads_out).  From the row BEFORE its update the pass also takes
//             sum_c T_j[c] W1[8j + f][c], whose sum over j is dE[1][f]; dE[0][f] = sum_c S[c] B_f[c] - dE[1][f].
// A step is these launches (and one memset of the item mask):
//   k_mlp_mask    a work-group per row: the row's span checked (csrc/csr_batch.h's status bits), its `live` word, bit r of mask[j] for
//                 every checked entry j (an integer atomicOr: the result does not depend on the order)
//   k_mlp_gather  (row, chunk of the row's entries): the gather of the forward, MLP_GCH partial sums per row
//   k_mlp_z1      z1 from the base vector and the partial sums in chunk order; a1
//   k_mlp_fwd     layers 2, 3 and the output layer (with the loss terms, dy and the loss partial sums), 64 columns a work-group
//   k_mlp_dgrad   dz3, dz2, dz1: a work-group per input unit, from the kernels BEFORE their update
//   k_mlp_adam    W4 b4, W3 b3, W2 b2: every gradient element a sum over the rows in ascending order inside its Adam update
//   k_mlp_w1      the pass over W1, m, v (and b1) described above; per work-group the partial B_f of the NEW weights and of dE[1]
//   k_mlp_embed   dE, Adam on rows 0 and 1 of E (the only rows a 0 / 1 input names; Keras's sparse update leaves the others alone), the loss
//   k_mlp_bsum    the partial B_f added in work-group order
// Values are fp32.  Every SUM (a dot product of a layer, the gather, B_f, a gradient element's terms over the rows) is accumulated in
// float64 in a fixed order and rounded to fp32 once: the step is bound by the bytes of W1, m and v, not by arithmetic, and the tests
// hold every gradient to a few times the rounding of a float32 reference.  No floating-point atomic: the same bits on every run.
// A row id outside the matrix, an indptr pair out of order (dead row: dy = 0, so it adds nothing to the loss or to any gradient) and
// a column outside [0, I) (skipped) raise the feed status word; the divisor b I still counts them.  No address is taken from the feed
// unchecked.  Plain HIP, vector / plain C++ stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "elementwise.h"
#include "philox.h"

namespace sdrm {

constexpr int MLP_F = 8, MLP_H1 = 512, MLP_H2 = 256, MLP_H3 = 256;
constexpr int MLP_MAX_BATCH = 16, MLP_KEEP_COLS = MLP_H1 + MLP_H2 + MLP_H3, MLP_MAX_ITEMS = 36864;
constexpr int MLP_GCH = 16;        // partial sums of a row's gather (a row of n entries: chunks of ceil(n / MLP_GCH) entries)
constexpr int MLP_W1_ITEMS = 16;   // items of a work-group of k_mlp_w1
constexpr int MLP_BS_SPLIT = 16;   // strided groups k_mlp_bsum adds a column's partials in

// Keras's Adam for one element: alpha = lr sqrt(1 - b2^t) / (1 - b1^t) (the host's), omb = 1 - beta.
struct MlpAdam { float alpha, omb1, omb2, eps; };
__device__ __forceinline__ float mlp_adam(const MlpAdam& a, float w, float g, float& m, float& v) {
  return adam_math_keras(w, g, m, v, a.alpha, a.omb1, a.omb2, a.eps);
}

struct MlpDrop {
  const uint8_t* keep;   // EXPLICIT: this step's [b][MLP_KEEP_COLS] bytes; null: PHILOX
  uint32_t j0, k0, k1, call_id, thr;
  float s;               // 1 / (1 - p_drop)
};
// the keep decision of column c (0 .. 1023: k1 | k2 | k3) of the step's row r
__device__ __forceinline__ bool mlp_keep(const MlpDrop& d, int r, int c) {
  if (d.keep) return d.keep[(size_t)r * MLP_KEEP_COLS + c] != 0;
  const U4 w = philox4x32_10(d.j0 + (uint32_t)r, (uint32_t)(c >> 2), PURPOSE_MLP_DROP, d.call_id, d.k0, d.k1);
  const uint32_t word = (c & 3) == 0 ? w.x : (c & 3) == 1 ? w.y : (c & 3) == 2 ? w.z : w.w;
  return word >= d.thr;
}

// The checked span of the step's row r: false for a row id outside the matrix or an indptr pair out of order (thread `owner` == 0 raises
// the status word).
__device__ __forceinline__ bool mlp_row_span(const CsrBatch& c, int r, int owner, int64_t& p0, int64_t& p1) {
  p0 = p1 = 0;
  const int64_t src = c.rows[r];
  if (src < 0 || src >= c.n_rows) {
    if (owner == 0) atomicOr(c.flag, (unsigned)FEED_BAD_ROW);
    return false;
  }
  const int64_t q0 = c.indptr[src], q1 = c.indptr[src + 1];
  if (q0 < 0 || q1 < q0) {
    if (owner == 0) atomicOr(c.flag, (unsigned)FEED_BAD_PTR);
    return false;
  }
  p0 = q0; p1 = q1;
  return true;
}

// grid b, block 256
__global__ __launch_bounds__(256) void k_mlp_mask(const CsrBatch c, unsigned* __restrict__ mask, int* __restrict__ live) {
  const int r = blockIdx.x, t = threadIdx.x;
  int64_t p0, p1;
  const bool ok = mlp_row_span(c, r, t, p0, p1);
  if (t == 0) live[r] = ok ? 1 : 0;
  bool bad = false;
  for (int64_t p = p0 + t; p < p1; p += 256) {
    const int32_t col = c.indices[p];
    if (col < 0 || col >= c.n_items) bad = true;
    else atomicOr(mask + col, 1u << r);
  }
  if (bad) atomicOr(c.flag, (unsigned)FEED_BAD_COL);
}

// grid (MLP_GCH, b), block 128: thread t owns columns 4t .. 4t + 3.  zpart [b][MLP_GCH][512] float64.
__global__ __launch_bounds__(128) void k_mlp_gather(const CsrBatch c, const float* __restrict__ E, const float* __restrict__ W1,
                                                    double* __restrict__ zpart) {
  const int r = blockIdx.y, slot = blockIdx.x, t = threadIdx.x;
  int64_t p0, p1;
  mlp_row_span(c, r, 1, p0, p1);   // (k_mlp_mask has raised the word)
  const int64_t len = (p1 - p0 + MLP_GCH - 1) / MLP_GCH;
  const int64_t q0 = p0 + slot * len, q1 = q0 + len < p1 ? q0 + len : p1;
  double dE[MLP_F];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) dE[f] = (double)E[MLP_F + f] - (double)E[f];
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int64_t p = q0; p < q1; ++p) {
    const int32_t col = c.indices[p];
    if (col < 0 || col >= c.n_items) continue;
    const float4* __restrict__ row = reinterpret_cast<const float4*>(W1 + (size_t)col * MLP_F * MLP_H1) + t;
    float4 w[MLP_F];
#pragma unroll
    for (int f = 0; f < MLP_F; ++f) w[f] = row[f * (MLP_H1 / 4)];
#pragma unroll
    for (int f = 0; f < MLP_F; ++f) {
      acc[0] = fma(dE[f], (double)w[f].x, acc[0]);
      acc[1] = fma(dE[f], (double)w[f].y, acc[1]);
      acc[2] = fma(dE[f], (double)w[f].z, acc[2]);
      acc[3] = fma(dE[f], (double)w[f].w, acc[3]);
    }
  }
  double* out = zpart + ((size_t)r * MLP_GCH + slot) * MLP_H1 + 4 * t;
#pragma unroll
  for (int q = 0; q < 4; ++q) out[q] = acc[q];
}

// grid b * 512 / 256, block 256: a1 [b][512]
__global__ __launch_bounds__(256) void k_mlp_z1(const float* __restrict__ E, const float* __restrict__ b1, const double* __restrict__ bsum,
                                                const double* __restrict__ zpart, const MlpDrop d, float* __restrict__ a1) {
  const int idx = blockIdx.x * 256 + threadIdx.x, r = idx / MLP_H1, c = idx % MLP_H1;
  double z = (double)b1[c];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) z = fma((double)E[f], bsum[f * MLP_H1 + c], z);
#pragma unroll
  for (int q = 0; q < MLP_GCH; ++q) z += zpart[((size_t)r * MLP_GCH + q) * MLP_H1 + c];
  const float zf = (float)z;
  a1[idx] = zf > 0.f && mlp_keep(d, r, c) ? zf * d.s : 0.f;
}

// One dense layer forward for the step's rows: block 256 = 64 output columns x 4 quarters of the inputs, grid ceil(OUT / 64).
// LOSS = false: out[r][col] = keep && z > 0 ? z s : 0 with the keep columns from drop0.
// LOSS = true (the output layer): out = dy [b][OUT], and the work-group's sum of the loss terms into losspart[blockIdx.x].
struct MlpFwdArgs {
  const float* A;      // [b][IN]
  const float* W;      // [IN][OUT]
  const float* bias;   // [OUT]
  float* out;          // [b][OUT]
  int b, IN, OUT, drop0;
  MlpDrop d;
  const unsigned* mask; const int* live; double* losspart;   // LOSS only
};
template <bool LOSS>
__global__ __launch_bounds__(256) void k_mlp_fwd(const MlpFwdArgs a) {
  __shared__ double buf[4 * 64 * MLP_MAX_BATCH];   // 32 KB: the staged inputs [16][IN <= 512] as floats, then the quarters' sums
  float* As = reinterpret_cast<float*>(buf);
  const int t = threadIdx.x, q = t >> 6, l = t & 63, IN = a.IN, OUT = a.OUT;
  for (int i = t; i < MLP_MAX_BATCH * IN; i += 256) As[i] = i < a.b * IN ? a.A[i] : 0.f;
  __syncthreads();
  const int col = blockIdx.x * 64 + l, colc = col < OUT ? col : OUT - 1;
  double acc[MLP_MAX_BATCH];
#pragma unroll
  for (int r = 0; r < MLP_MAX_BATCH; ++r) acc[r] = 0.0;
  const int kq = IN / 4;
  const float* __restrict__ wp = a.W + (size_t)q * kq * OUT + colc;
#pragma unroll 4
  for (int k = 0; k < kq; ++k) {
    const double w = (double)wp[(size_t)k * OUT];
#pragma unroll
    for (int r = 0; r < MLP_MAX_BATCH; ++r) acc[r] = fma((double)As[r * IN + q * kq + k], w, acc[r]);
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < MLP_MAX_BATCH; ++r) buf[(q * MLP_MAX_BATCH + r) * 64 + l] = acc[r];
  __syncthreads();
  double terms = 0.0;
  const double div = (double)a.b * (double)OUT;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = t + 256 * i, r = o >> 6, ll = o & 63, cc = blockIdx.x * 64 + ll;
    if (r >= a.b || cc >= OUT) continue;
    double z = (double)a.bias[cc];
#pragma unroll
    for (int qq = 0; qq < 4; ++qq) z += buf[(qq * MLP_MAX_BATCH + r) * 64 + ll];
    const float zf = (float)z;
    if (!LOSS) {
      a.out[(size_t)r * OUT + cc] = zf > 0.f && mlp_keep(a.d, r, a.drop0 + cc) ? zf * a.d.s : 0.f;
    } else {
      // the loss term and dy from the fp32 logit, in float64: (1 - x) sigmoid(y) - x sigmoid(-y), both sigmoids from exp(-|y|)
      const double y = (double)zf, x = (double)((a.mask[cc] >> r) & 1u);
      const double et = exp(-fabs(y)), hi = 1.0 / (1.0 + et), lo = et / (1.0 + et);
      const double sp = y >= 0.0 ? hi : lo, sn = y >= 0.0 ? lo : hi;
      const bool live = a.live[r] != 0;
      if (live) terms += fmax(y, 0.0) - y * x + log1p(et);
      a.out[(size_t)r * OUT + cc] = live ? (float)(((1.0 - x) * sp - x * sn) / div) : 0.f;
    }
  }
  if (LOSS) {
    __syncthreads();
    buf[t] = terms;
    __syncthreads();
#pragma unroll
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) buf[t] += buf[t + w];
      __syncthreads();
    }
    if (t == 0) a.losspart[blockIdx.x] = buf[0];
  }
}

// dz[r][k] = Ain[r][k] > 0 ? s sum_c D[r][c] W[k][c] : 0 for the step's rows: grid IN (a work-group per input unit k), block 256.
// (Ain > 0 iff the unit was kept and its z was positive.)
struct MlpDgradArgs {
  const float* D;     // [b][OUT]
  const float* W;     // [IN][OUT], before its update
  const float* Ain;   // [b][IN]
  float* dz;          // [b][IN]
  int b, IN, OUT;
  float s;
};
__global__ __launch_bounds__(256) void k_mlp_dgrad(const MlpDgradArgs a) {
  __shared__ double red[MLP_MAX_BATCH][256];
  const int k = blockIdx.x, t = threadIdx.x, OUT = a.OUT, b = a.b;
  double acc[MLP_MAX_BATCH];
#pragma unroll
  for (int r = 0; r < MLP_MAX_BATCH; ++r) acc[r] = 0.0;
  const float* __restrict__ wrow = a.W + (size_t)k * OUT;
  for (int c = t; c < OUT; c += 256) {
    const double w = (double)wrow[c];
#pragma unroll
    for (int r = 0; r < MLP_MAX_BATCH; ++r)
      if (r < b) acc[r] = fma((double)a.D[(size_t)r * OUT + c], w, acc[r]);
  }
#pragma unroll
  for (int r = 0; r < MLP_MAX_BATCH; ++r) red[r][t] = acc[r];
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
#pragma unroll
      for (int r = 0; r < MLP_MAX_BATCH; ++r) red[r][t] += red[r][t + w];
    }
    __syncthreads();
  }
  if (t < b) a.dz[(size_t)t * a.IN + k] = a.Ain[(size_t)t * a.IN + k] > 0.f ? (float)(red[t][0] * (double)a.s) : 0.f;
}

// Adam on a dense kernel W [IN][OUT] and its bias, the gradient made on the way: g[k][c] = sum_r A[r][k] DZ[r][c], r ascending, float64,
// rounded once.  grid (ceil(OUT / 256), IN / MLP_ADAM_ROWS), block 256: thread = column c, the work-group's rows k in turn; the
// work-groups of grid row 0 take the bias (g = sum_r DZ[r][c]) as well.
constexpr int MLP_ADAM_ROWS = 32;
struct MlpAdamArgs {
  const float* A;    // [b][IN]
  const float* DZ;   // [b][OUT]
  float *W, *mW, *vW, *gW;   // [IN][OUT]; gW null: the gradient is not stored
  float *B, *mB, *vB, *gB;   // [OUT]
  int b, IN, OUT;
  MlpAdam adam;
};
__global__ __launch_bounds__(256) void k_mlp_adam(const MlpAdamArgs a) {
  __shared__ float As[MLP_MAX_BATCH][MLP_ADAM_ROWS];
  const int t = threadIdx.x, c = blockIdx.x * 256 + t, k0 = blockIdx.y * MLP_ADAM_ROWS, OUT = a.OUT, b = a.b;
  for (int i = t; i < MLP_MAX_BATCH * MLP_ADAM_ROWS; i += 256) {
    const int r = i / MLP_ADAM_ROWS, kk = i % MLP_ADAM_ROWS;
    As[r][kk] = r < b ? a.A[(size_t)r * a.IN + k0 + kk] : 0.f;
  }
  __syncthreads();
  if (c >= OUT) return;
  double dz[MLP_MAX_BATCH];
#pragma unroll
  for (int r = 0; r < MLP_MAX_BATCH; ++r) dz[r] = r < b ? (double)a.DZ[(size_t)r * OUT + c] : 0.0;
  if (blockIdx.y == 0) {
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < MLP_MAX_BATCH; ++r) g += dz[r];
    float m = a.mB[c], v = a.vB[c];
    a.B[c] = mlp_adam(a.adam, a.B[c], (float)g, m, v);
    a.mB[c] = m; a.vB[c] = v;
    if (a.gB) a.gB[c] = (float)g;
  }
#pragma unroll 4
  for (int kk = 0; kk < MLP_ADAM_ROWS; ++kk) {
    const size_t at = (size_t)(k0 + kk) * OUT + c;
    const float w = a.W[at];
    float m = a.mW[at], v = a.vW[at];
    double g = 0.0;
#pragma unroll
    for (int r = 0; r < MLP_MAX_BATCH; ++r) g = fma((double)As[r][kk], dz[r], g);
    a.W[at] = mlp_adam(a.adam, w, (float)g, m, v);
    a.mW[at] = m; a.vW[at] = v;
    if (a.gW) a.gW[at] = (float)g;
  }
}

// The pass over W1: grid ceil(I / MLP_W1_ITEMS), block 128, thread t owns columns 4t .. 4t + 3 of every row of the work-group's items.
// UPDATE = false: nothing but bpart (the first step of a call).
struct MlpW1Args {
  float *W, *mW, *vW, *gW;      // [8 I][512]; gW null: the gradient is not stored
  float *B, *mB, *vB, *gB;      // b1 [512]
  const float* E;               // [n_users][8], rows 0 and 1 read
  const float* dz1;             // [b][512]
  const unsigned* mask;         // [I]
  double* bpart;                // [work-groups][8][512]: sum of the work-group's rows 8j + f AFTER the update
  double* e1part;               // [work-groups][8]: sum over the work-group's items j of sum_c T_j[c] W1[8j + f][c] BEFORE the update
  int b, n_items;
  MlpAdam adam;
};
template <bool UPDATE>
__global__ __launch_bounds__(128) void k_mlp_w1(const MlpW1Args a) {
  __shared__ double red[MLP_F][128];
  const int t = threadIdx.x, b = a.b;
  const int j0 = blockIdx.x * MLP_W1_ITEMS, j1 = j0 + MLP_W1_ITEMS < a.n_items ? j0 + MLP_W1_ITEMS : a.n_items;
  double S[4] = {0.0, 0.0, 0.0, 0.0}, e1[MLP_F];
  double bacc[MLP_F][4];
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) {
    e1[f] = 0.0;
#pragma unroll
    for (int q = 0; q < 4; ++q) bacc[f][q] = 0.0;
  }
  if (UPDATE) {
    for (int r = 0; r < b; ++r) {
      const float4 d = reinterpret_cast<const float4*>(a.dz1 + (size_t)r * MLP_H1)[t];
      S[0] += (double)d.x; S[1] += (double)d.y; S[2] += (double)d.z; S[3] += (double)d.w;
    }
    if (blockIdx.x == 0) {   // b1: g = S
      const float4 w = reinterpret_cast<const float4*>(a.B)[t];
      float4 m = reinterpret_cast<const float4*>(a.mB)[t], v = reinterpret_cast<const float4*>(a.vB)[t];
      const float4 g = make_float4((float)S[0], (float)S[1], (float)S[2], (float)S[3]);
      float4 n;
      n.x = mlp_adam(a.adam, w.x, g.x, m.x, v.x); n.y = mlp_adam(a.adam, w.y, g.y, m.y, v.y);
      n.z = mlp_adam(a.adam, w.z, g.z, m.z, v.z); n.w = mlp_adam(a.adam, w.w, g.w, m.w, v.w);
      reinterpret_cast<float4*>(a.B)[t] = n;
      reinterpret_cast<float4*>(a.mB)[t] = m;
      reinterpret_cast<float4*>(a.vB)[t] = v;
      if (a.gB) reinterpret_cast<float4*>(a.gB)[t] = g;
    }
  }
  for (int j = j0; j < j1; ++j) {
    double T[4] = {0.0, 0.0, 0.0, 0.0};
    unsigned mk = 0;
    if (UPDATE) {
      mk = a.mask[j];
      for (int r = 0; r < b; ++r) {
        if (!((mk >> r) & 1u)) continue;   // (wave-uniform)
        const float4 d = reinterpret_cast<const float4*>(a.dz1 + (size_t)r * MLP_H1)[t];
        T[0] += (double)d.x; T[1] += (double)d.y; T[2] += (double)d.z; T[3] += (double)d.w;
      }
    }
    const size_t row0 = (size_t)j * MLP_F * (MLP_H1 / 4) + t;   // in float4
    float4 w[MLP_F], m[MLP_F], v[MLP_F];
#pragma unroll
    for (int f = 0; f < MLP_F; ++f) {
      w[f] = reinterpret_cast<const float4*>(a.W)[row0 + f * (MLP_H1 / 4)];
      if (UPDATE) {
        m[f] = reinterpret_cast<const float4*>(a.mW)[row0 + f * (MLP_H1 / 4)];
        v[f] = reinterpret_cast<const float4*>(a.vW)[row0 + f * (MLP_H1 / 4)];
      }
    }
#pragma unroll
    for (int f = 0; f < MLP_F; ++f) {
      float wv[4] = {w[f].x, w[f].y, w[f].z, w[f].w};
      if (UPDATE) {
        const double e0 = (double)a.E[f], de = (double)a.E[MLP_F + f] - e0;
        float mv[4] = {m[f].x, m[f].y, m[f].z, m[f].w}, vv[4] = {v[f].x, v[f].y, v[f].z, v[f].w}, g[4];
        if (mk) e1[f] += (T[0] * (double)wv[0] + T[1] * (double)wv[1]) + (T[2] * (double)wv[2] + T[3] * (double)wv[3]);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          g[q] = (float)fma(de, T[q], e0 * S[q]);
          wv[q] = mlp_adam(a.adam, wv[q], g[q], mv[q], vv[q]);
        }
        const size_t at = row0 + f * (MLP_H1 / 4);
        reinterpret_cast<float4*>(a.W)[at] = make_float4(wv[0], wv[1], wv[2], wv[3]);
        reinterpret_cast<float4*>(a.mW)[at] = make_float4(mv[0], mv[1], mv[2], mv[3]);
        reinterpret_cast<float4*>(a.vW)[at] = make_float4(vv[0], vv[1], vv[2], vv[3]);
        if (a.gW) reinterpret_cast<float4*>(a.gW)[at] = make_float4(g[0], g[1], g[2], g[3]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) bacc[f][q] += (double)wv[q];
    }
  }
  double* bp = a.bpart + (size_t)blockIdx.x * MLP_F * MLP_H1 + 4 * t;
#pragma unroll
  for (int f = 0; f < MLP_F; ++f) {
#pragma unroll
    for (int q = 0; q < 4; ++q) bp[f * MLP_H1 + q] = bacc[f][q];
  }
  if (UPDATE) {
#pragma unroll
    for (int f = 0; f < MLP_F; ++f) red[f][t] = e1[f];
    __syncthreads();
#pragma unroll
    for (int w = 64; w > 0; w >>= 1) {
      if (t < w) {
#pragma unroll
        for (int f = 0; f < MLP_F; ++f) red[f][t] += red[f][t + w];
      }
      __syncthreads();
    }
    if (t < MLP_F) a.e1part[(size_t)blockIdx.x * MLP_F + t] = red[t][0];
  }
}

// bsum[i] = sum over the work-groups q of bpart[q][i], i < 4096: MLP_BS_SPLIT strided groups (q = g, g + 16, ..), each in ascending order,
// then the groups in order.  grid 4096 / 16, block 256 = 16 groups x 16 elements.
__global__ __launch_bounds__(256) void k_mlp_bsum(const double* __restrict__ bpart, int parts, double* __restrict__ bsum) {
  __shared__ double red[MLP_BS_SPLIT][16];
  const int t = threadIdx.x, g = t >> 4, l = t & 15, i = blockIdx.x * 16 + l;
  double s = 0.0;
#pragma unroll 4
  for (int q = g; q < parts; q += MLP_BS_SPLIT) s += bpart[(size_t)q * (MLP_F * MLP_H1) + i];
  red[g][l] = s;
  __syncthreads();
  if (t < 16) {
    double z = 0.0;
#pragma unroll
    for (int gg = 0; gg < MLP_BS_SPLIT; ++gg) z += red[gg][t];
    bsum[i] = z;
  }
}

// One work-group of 256: dE[1][f] = sum of e1part in work-group order (32 strided groups, then in order), dE[0][f] = sum_c S[c] B_f[c] -
// dE[1][f] with B_f of the weights BEFORE the update; Adam on E's rows 0 and 1; the loss = sum of losspart / (b I).
struct MlpEmbedArgs {
  float *E, *mE, *vE, *gE;   // [n_users][8]; gE null or zeroed by the host: rows 0 and 1 are written
  const double* e1part; int parts;
  const double* bsum;        // [8][512]
  const float* dz1;          // [b][512]
  const double* losspart; int loss_parts;
  double* loss;              // this step's slot, or null
  int b, n_items;
  MlpAdam adam;
};
__global__ __launch_bounds__(256) void k_mlp_embed(const MlpEmbedArgs a) {
  __shared__ double red[256];
  __shared__ double S[MLP_H1];
  __shared__ double e1[MLP_F], eall[MLP_F];
  const int t = threadIdx.x;
  for (int c = t; c < MLP_H1; c += 256) {
    double s = 0.0;
    for (int r = 0; r < a.b; ++r) s += (double)a.dz1[(size_t)r * MLP_H1 + c];
    S[c] = s;
  }
  {   // e1part: thread = (group t / 8 of 32, f = t % 8)
    const int f = t & 7;
    double s = 0.0;
    for (int q = t >> 3; q < a.parts; q += 32) s += a.e1part[(size_t)q * MLP_F + f];
    red[t] = s;
  }
  __syncthreads();
  if (t < MLP_F) {
    double z = 0.0;
    for (int g = 0; g < 32; ++g) z += red[g * 8 + t];
    e1[t] = z;
  }
  __syncthreads();
  {   // S . B_f: thread = (f = t / 32, 32 strided partial sums)
    const int f = t >> 5, l = t & 31;
    double s = 0.0;
    for (int c = l; c < MLP_H1; c += 32) s = fma(S[c], a.bsum[f * MLP_H1 + c], s);
    red[t] = s;
  }
  __syncthreads();
  if (t < MLP_F) {
    double z = 0.0;
    for (int l = 0; l < 32; ++l) z += red[t * 32 + l];
    eall[t] = z;
  }
  __syncthreads();
  if (t < 2 * MLP_F) {
    const int f = t & 7;
    const float g = (float)(t < MLP_F ? eall[f] - e1[f] : e1[f]);
    float m = a.mE[t], v = a.vE[t];
    a.E[t] = mlp_adam(a.adam, a.E[t], g, m, v);
    a.mE[t] = m; a.vE[t] = v;
    if (a.gE) a.gE[t] = g;
  }
  if (!a.loss) return;   // (uniform)
  __syncthreads();
  double s = 0.0;
  for (int q = t; q < a.loss_parts; q += 256) s += a.losspart[q];
  red[t] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) *a.loss = red[0] / ((double)a.b * (double)a.n_items);
}

}  // namespace sdrm
