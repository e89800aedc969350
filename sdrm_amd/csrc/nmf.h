// Non-negative matrix factorisation of a sparse matrix on the device, and the scores of its reconstruction (reference: svd_benchmark.py:49-54,
// `NMF(n_components=15, max_iter=50)` + `inverse_transform(fit_transform(.))`; sklearn's default solver is `cd`, coordinate descent, and its
// default start is NNDSVDa).  Everything is float64: the factors are m x 15 and n x 15 numbers and every kernel is latency- or gather-bound.
// Factors are stored row-major with a row stride of NMF_LD = 16 doubles, W [m][16] and Ht [n][16]; columns k .. 15 are zero and are never
// read into a result (the loops over components stop at k).
//
// One half-iteration is sklearn's `_update_coordinate_descent(X, W, Ht)`, three bodies in two launches:
//   k_nmf_prod    work-groups [0, prod_blocks): XHt[r][0:16] = sum_p value_p Ht[col_p][0:16] over the entries of CSR row r in CSR ORDER, ONE
//                 FUSED chain (fma) per output element: no atomic, the same bits on every run.  Modelled on k_svd_spmm: 8 lanes own a row (a
//                 double2 slice of the 16 columns each, 32 rows per work-group), load 8 entries of it coalesced, hand them round with 8-wide
//                 shuffles and issue the 8 16-byte loads of Ht before the FMAs that consume them.  data == null: all ones.  Row ids, indptr
//                 pairs (against nnz as well) and column indices are range-checked (csrc/csr_batch.h): an offender is skipped and raises the
//                 feed status word.
//                 work-groups behind them: the Gram matrix HHt = Ht^T Ht [16][16] as per-work-group partials: work-group g takes the tiles
//                 g, g + G, .. of 64 rows in that order, a thread owns one element and adds the rows of a tile in row order (fma).
//   k_nmf_sweep   prologue: EVERY work-group adds the Gram partials in block order into LDS.  Then one lane per row, W's row and the row of
//                 XHt in registers, HHt a uniform LDS operand; for t = 0 .. k-1 in order:
//                     grad = -XHt[t] + sum_r HHt[t][r] W[r]  (r ascending, fma);  pg = W[t] == 0 ? min(0, grad) : grad;  violation += |pg|;
//                     if HHt[t][t] != 0:  W[t] = max(W[t] - grad / HHt[t][t], 0)
//                 The rows' violations are added by a fixed tree inside the work-group into one partial per work-group.
// The H update is the same two launches on the CSC arrays (the CSR of X^T) with the roles of W and Ht swapped.
//   k_nmf_stop    one work-group, behind the H half of iteration i: the partials of both halves added in block order (a thread adds a
//                 contiguous run of blocks ascending, thread 0 adds the 256 runs ascending), v_i = viol_W + viol_H into violations[i-1], v_1
//                 kept, and `done` raised with n_iter = i when v_1 == 0 or v_i / v_1 <= tol.  EVERY launch of the fit reads `done` first
//                 and returns at once when it is set: a whole fit is queued without a host round trip, and the factors are exactly those
//                 of the stopping iteration.  Without a stop the last iteration writes n_iter = max_iter.
// The start, sklearn's `_initialize_nmf(init='nndsvda')` from the factors of sdrm_svd_fit:
//   k_nmf_vt      components [k][n] float32 -> V^T [n][16] float64, zero-padded (U sigma = X V^T is then k_nmf_prod without Gram work-groups)
//   k_nmf_mean    X.mean(): (entries of the matrix) / (m n) for all-ones data, else the sum of `data` over the stretch indptr[0] .. indptr[m]
//                 in a fixed order (a thread a contiguous run, thread 0 the 256 runs), divided by m n
//   k_nmf_norms   per column j < k the squared norms of the positive and of the negative part, per-work-group partials in a fixed tile order
//   k_nmf_init    prologue: every work-group adds those partials in block order and picks per component: 0: sqrt(sigma_0) |u_0|, sqrt(sigma_0)
//                 |v_0|;  j >= 1: the pair (positive or negative parts of u_j, v_j) with the larger product of norms - the negative pair on
//                 a tie, sklearn's `m_p > m_n` is strict -, each part divided by its norm and scaled by sqrt(sigma_j x product).  Entries
//                 below 1e-6 (`_initialize_nmf`'s eps, which NMF leaves at its default) become 0, every zero then becomes X.mean().  A part
//                 of norm zero gives zeros (sklearn divides by it).  The sign of a component does not matter: svd_fit's unflipped signs are fine.
// The scores:
//   k_nmf_expand  scores[r][j] = sum_{c < k} W[row_r][c] H[c][j], c ascending, in float64 (fma), rounded ONCE to float32 and written exactly
//                 once per element in k_svd_expand's store pattern: a thread holds row j of Ht in registers and writes column j of a tile of
//                 16 rows.  A row id outside [0, m) gives a zero row and raises the feed status word.
// Plain HIP, vector / plain C++ stores only, no atomics on data, no grid barrier, no spin-wait (tests/test_isa_lint.py has nothing to hold).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"

namespace sdrm {

constexpr int NMF_LD = 16;            // row stride of the factors, and the most components
constexpr int NMF_GRAM_ROWS = 64;     // rows of a Gram tile
constexpr int NMF_PARTS = 64;         // most work-groups of the Gram and of k_nmf_norms: every sweep work-group adds that many partials
constexpr int NMF_ROW_TILE = 16;      // rows of a tile of k_nmf_expand
constexpr double NMF_INIT_EPS = 1e-6; // `_initialize_nmf(eps=1e-6)`

struct NmfState { double v1; int done; int pad; };   // of one fit: the first iteration's violation and the stop word

struct NmfProdArgs {
  CsrBatch csr;        // the rows of the product (for X^T: the CSC arrays, n_rows = columns of X, n_items = rows of X)
  int64_t nnz;         // entries of csr.indices: an indptr pair that reaches behind them is an empty row
  const double* f;     // [csr.n_items][16] the gathered factor; the Gram work-groups take f^T f
  double* out;         // [csr.b][16]
  int prod_blocks;     // work-groups [0, prod_blocks) are the product's, those behind them the Gram's
  double* g_part;      // [Gram work-groups][16][16]
  const NmfState* st;  // null: no stop word to look at
};

__global__ __launch_bounds__(256) void k_nmf_prod(const NmfProdArgs a) {
  __shared__ __attribute__((aligned(16))) double tile[NMF_GRAM_ROWS][NMF_LD];
  if (a.st && a.st->done) return;
  const double2* __restrict__ f2 = reinterpret_cast<const double2*>(a.f);
  if ((int)blockIdx.x >= a.prod_blocks) {   // ---- Gram partial of work-group g
    const int g = (int)blockIdx.x - a.prod_blocks, G = (int)gridDim.x - a.prod_blocks;
    const int t = threadIdx.x, i = t >> 4, j = t & 15;
    const int rows = a.csr.n_items;
    const int tiles = (rows + NMF_GRAM_ROWS - 1) / NMF_GRAM_ROWS;
    double acc = 0.0;
    for (int k = g; k < tiles; k += G) {
      __syncthreads();   // the previous tile has been read
      for (int e = t; e < NMF_GRAM_ROWS * 8; e += 256) {
        const int64_t row = (int64_t)k * NMF_GRAM_ROWS + (e >> 3);
        const double2 v = row < rows ? f2[(size_t)row * 8 + (e & 7)] : make_double2(0.0, 0.0);
        *reinterpret_cast<double2*>(&tile[e >> 3][(e & 7) * 2]) = v;
      }
      __syncthreads();
      for (int rr = 0; rr < NMF_GRAM_ROWS; ++rr) acc = fma(tile[rr][i], tile[rr][j], acc);
    }
    a.g_part[(size_t)g * (NMF_LD * NMF_LD) + t] = acc;
    return;
  }
  const int lane = threadIdx.x & 7;
  const int r = blockIdx.x * 32 + (threadIdx.x >> 3);
  if (r >= a.csr.b) return;   // (the 8 lanes of a row leave together: the shuffles below stay inside a row's lanes)
  CsrSpan s = csr_row_span(a.csr, r, lane);
  if (s.p1 > a.nnz) {
    if (lane == 0) atomicOr(a.csr.flag, (unsigned)FEED_BAD_PTR);
    s.p0 = s.p1 = 0;
  }
  double2 acc = make_double2(0.0, 0.0);
  bool bad = false;
  for (int64_t p = s.p0; p < s.p1; p += 8) {
    const int cnt = (int)((s.p1 - p) < 8 ? (s.p1 - p) : 8);
    int col = -1;   // -1: nothing to add (behind the row's end, or a column outside the matrix)
    float val = 0.f;
    if (lane < cnt) {
      int32_t c;
      float v;
      if (csr_entry(a.csr, p + lane, bad, c, v)) { col = c; val = v; }
    }
    double2 w[8];
    double vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int cu = __shfl(col, u, 8);
      vv[u] = (double)__shfl(val, u, 8);
      w[u] = cu >= 0 ? f2[(size_t)cu * 8 + lane] : make_double2(0.0, 0.0);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x = fma(vv[u], w[u].x, acc.x);
      acc.y = fma(vv[u], w[u].y, acc.y);
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  reinterpret_cast<double2*>(a.out)[(size_t)r * 8 + lane] = acc;
}

// s = x[0] + .. + x[255] by a fixed tree, into x[0] (all 256 threads call it; x is LDS)
__device__ __forceinline__ void nmf_tree_sum(double* x, int t) {
  for (int w = 128; w >= 1; w >>= 1) {
    __syncthreads();
    if (t < w) x[t] += x[t + w];
  }
  __syncthreads();
}

struct NmfSweepArgs {
  double* w;             // [rows][16] the factor this half updates, in place
  const double* xh;      // [rows][16] k_nmf_prod's product
  const double* g_part;  // [g_parts][16][16]
  int g_parts, rows, k;
  double* viol_part;     // [work-groups of this launch]
  const NmfState* st;
};

__global__ __launch_bounds__(256) void k_nmf_sweep(const NmfSweepArgs a) {
  __shared__ double H[NMF_LD][NMF_LD];
  __shared__ double red[256];
  if (a.st->done) return;
  const int t = threadIdx.x;
  {
    double s = 0.0;
    for (int p = 0; p < a.g_parts; ++p) s += a.g_part[(size_t)p * (NMF_LD * NMF_LD) + t];   // block order
    H[t >> 4][t & 15] = s;
  }
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * 256 + t;
  double viol = 0.0;
  if (row < a.rows) {
    double W[NMF_LD], X[NMF_LD];
    double2* w2 = reinterpret_cast<double2*>(a.w) + (size_t)row * 8;
    const double2* x2 = reinterpret_cast<const double2*>(a.xh) + (size_t)row * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double2 v = w2[c], x = x2[c];
      W[2 * c] = v.x; W[2 * c + 1] = v.y;
      X[2 * c] = x.x; X[2 * c + 1] = x.y;
    }
#pragma unroll
    for (int c = 0; c < NMF_LD; ++c) {
      if (c < a.k) {
        double grad = -X[c];
#pragma unroll
        for (int r = 0; r < NMF_LD; ++r)
          if (r < a.k) grad = fma(H[c][r], W[r], grad);
        const double pg = W[c] == 0.0 ? fmin(0.0, grad) : grad;
        viol += fabs(pg);
        const double hess = H[c][c];
        if (hess != 0.0) W[c] = fmax(W[c] - grad / hess, 0.0);
      }
    }
#pragma unroll
    for (int c = 0; c < 8; ++c) w2[c] = make_double2(W[2 * c], W[2 * c + 1]);
  }
  red[t] = viol;
  nmf_tree_sum(red, t);
  if (t == 0) a.viol_part[blockIdx.x] = red[0];
}

// x[0] + .. + x[n-1]: thread t adds the run [t c, (t + 1) c) ascending (c = ceil(n / 256)), thread 0 the 256 runs ascending.  The result is
// valid in thread 0 only.  All 256 threads call it.
__device__ __forceinline__ double nmf_run_sum(const double* __restrict__ x, int64_t n, double* red, int t) {
  const int64_t c = (n + 255) / 256;
  const int64_t lo = t * c, hi = lo + c < n ? lo + c : n;
  double s = 0.0;
  for (int64_t p = lo; p < hi; ++p) s += x[p];
  __syncthreads();   // red is free again
  red[t] = s;
  __syncthreads();
  double tot = 0.0;
  if (t == 0)
    for (int u = 0; u < 256; ++u) tot += red[u];
  return tot;
}

__global__ __launch_bounds__(256) void k_nmf_stop(const double* __restrict__ viol_w, int parts_w, const double* __restrict__ viol_h, int parts_h, int it,
                                                  int max_iter, double tol, NmfState* st, int* __restrict__ n_iter, double* __restrict__ violations) {
  __shared__ double red[256];
  if (st->done) return;
  const int t = threadIdx.x;
  const double vw = nmf_run_sum(viol_w, parts_w, red, t);
  const double vh = nmf_run_sum(viol_h, parts_h, red, t);
  if (t != 0) return;
  const double v = vw + vh;
  violations[it - 1] = v;
  if (it == 1) st->v1 = v;
  const double v1 = it == 1 ? v : st->v1;
  if (v1 == 0.0 || v / v1 <= tol) {
    st->done = 1;
    *n_iter = it;
  } else if (it == max_iter) {
    *n_iter = it;
  }
}

// vt [n][16] float64 = v [k][n]^T, columns k .. 15 zero.
__global__ __launch_bounds__(256) void k_nmf_vt(const float* __restrict__ v, int k, int n, double* __restrict__ vt) {
  const int64_t total = (int64_t)n * NMF_LD;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c = (int)(idx & 15);
    const int64_t j = idx >> 4;
    vt[idx] = c < k ? (double)v[(size_t)c * n + j] : 0.0;
  }
}

// *mean = X.mean() of the matrix [m, n] (header comment).  One work-group.  The stretch of entries is clamped to [0, nnz].
__global__ __launch_bounds__(256) void k_nmf_mean(const int64_t* __restrict__ indptr, const float* __restrict__ data, int64_t m, int64_t n, int64_t nnz,
                                                  double* __restrict__ mean) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  int64_t p0 = indptr[0], p1 = indptr[m];
  p0 = p0 < 0 ? 0 : (p0 > nnz ? nnz : p0);
  p1 = p1 < p0 ? p0 : (p1 > nnz ? nnz : p1);
  const int64_t cnt = p1 - p0, c = (cnt + 255) / 256;
  const int64_t lo = t * c, hi = lo + c < cnt ? lo + c : cnt;
  double s = 0.0;
  if (data)
    for (int64_t p = lo; p < hi; ++p) s += (double)data[p0 + p];
  red[t] = s;
  __syncthreads();
  if (t == 0) {
    double tot = 0.0;
    for (int u = 0; u < 256; ++u) tot += red[u];
    if (!data) tot = (double)cnt;
    *mean = tot / ((double)m * (double)n);
  }
}

struct NmfSigma { double s[NMF_LD]; };   // the singular values, a kernel argument by value (entries k .. 15: 1)
__device__ __forceinline__ double nmf_pick(const NmfSigma& sg, int j) {   // s[j] without a dynamic index into the argument
  double v = 1.0;
#pragma unroll
  for (int c = 0; c < NMF_LD; ++c) v = c == j ? sg.s[c] : v;
  return v;
}

// part[g][0][j] / part[g][1][j] = the work-group's share of the squared norm of the positive / negative part of column j of src [rows][16]
// (each element divided by scale.s[j] first): work-group g takes the tiles g, g + G, .. of 64 rows; thread (s, j) adds
// the rows s, s + 16, s + 32, s + 48 of a tile in that order, and thread (0, j) adds the 16 sums s ascending.
__global__ __launch_bounds__(256) void k_nmf_norms(const double* __restrict__ src, int rows, int k, const NmfSigma scale, double* __restrict__ part) {
  __shared__ double red[2][16][16];
  const int t = threadIdx.x, s = t >> 4, j = t & 15;
  const double sc = nmf_pick(scale, j);
  const int tiles = (rows + NMF_GRAM_ROWS - 1) / NMF_GRAM_ROWS;
  double pos = 0.0, neg = 0.0;
  if (j < k) {
    for (int tl = blockIdx.x; tl < tiles; tl += gridDim.x) {
      for (int q = 0; q < 4; ++q) {
        const int64_t row = (int64_t)tl * NMF_GRAM_ROWS + s + 16 * q;
        if (row < rows) {
          const double x = src[(size_t)row * NMF_LD + j] / sc;
          if (x > 0.0) pos = fma(x, x, pos);
          else neg = fma(x, x, neg);
        }
      }
    }
  }
  red[0][s][j] = pos;
  red[1][s][j] = neg;
  __syncthreads();
  if (t < 32) {
    const int which = t >> 4;
    double tot = 0.0;
    for (int u = 0; u < 16; ++u) tot += red[which][u][j];
    part[(size_t)blockIdx.x * 32 + which * 16 + j] = tot;
  }
}

struct NmfInitArgs {
  const double* u;       // [m][16]: X V^T = U sigma (k_nmf_prod); divided by sigma on load
  const double* v;       // [n][16]: V^T
  NmfSigma sigma;
  const double* part_u;  // [parts_u][2][16] of u / sigma
  const double* part_v;  // [parts_v][2][16]
  const double* mean;
  int m, n, k, parts_u, parts_v;
  int blocks_w;          // work-groups [0, blocks_w) write W0, those behind them Ht0
  double* w0;            // [m][16]
  double* ht0;           // [n][16]
};

__global__ __launch_bounds__(256) void k_nmf_init(const NmfInitArgs a) {
  __shared__ double nrm[2][NMF_LD];   // the norm of the chosen part of u_j, v_j
  __shared__ double lbd[NMF_LD];
  __shared__ int mode[NMF_LD];        // 0: |x| (component 0), 1: the positive parts, 2: the negative parts
  const int t = threadIdx.x;
  if (t < NMF_LD) {
    double up = 0.0, un = 0.0, vp = 0.0, vn = 0.0;
    for (int p = 0; p < a.parts_u; ++p) { up += a.part_u[(size_t)p * 32 + t]; un += a.part_u[(size_t)p * 32 + 16 + t]; }   // block order
    for (int p = 0; p < a.parts_v; ++p) { vp += a.part_v[(size_t)p * 32 + t]; vn += a.part_v[(size_t)p * 32 + 16 + t]; }
    const double sg = t < a.k ? nmf_pick(a.sigma, t) : 0.0;
    if (t == 0) {
      mode[t] = 0; lbd[t] = sqrt(sg); nrm[0][t] = 1.0; nrm[1][t] = 1.0;
    } else {
      const double xp = sqrt(up), xn = sqrt(un), yp = sqrt(vp), yn = sqrt(vn);
      const double mp = xp * yp, mn = xn * yn;
      const bool positive = mp > mn;
      mode[t] = positive ? 1 : 2;
      nrm[0][t] = positive ? xp : xn;
      nrm[1][t] = positive ? yp : yn;
      lbd[t] = sqrt(sg * (positive ? mp : mn));
    }
  }
  __syncthreads();
  const bool is_w = (int)blockIdx.x < a.blocks_w;
  const int64_t row = (int64_t)(is_w ? blockIdx.x : blockIdx.x - a.blocks_w) * 256 + t;
  if (row >= (is_w ? a.m : a.n)) return;
  const double avg = *a.mean;
  const double2* src = reinterpret_cast<const double2*>(is_w ? a.u : a.v) + (size_t)row * 8;
  double2* dst = reinterpret_cast<double2*>(is_w ? a.w0 : a.ht0) + (size_t)row * 8;
  const int side = is_w ? 0 : 1;
#pragma unroll
  for (int c2 = 0; c2 < 8; ++c2) {
    const double2 x2 = src[c2];
    double o[2] = {x2.x, x2.y};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int c = 2 * c2 + h;
      double val = 0.0;
      if (c < a.k) {
        double x = is_w ? o[h] / a.sigma.s[c] : o[h];
        x = mode[c] == 0 ? fabs(x) : (mode[c] == 1 ? fmax(x, 0.0) : fabs(fmin(x, 0.0)));
        const double nr = nrm[side][c];
        val = nr > 0.0 ? lbd[c] * (x / nr) : 0.0;
        if (!(val >= NMF_INIT_EPS)) val = 0.0;   // (a NaN is a zero here too: nothing not finite leaves the start)
        if (val == 0.0) val = avg;
      }
      o[h] = val;
    }
    dst[c2] = make_double2(o[0], o[1]);
  }
}

struct NmfExpandArgs {
  const double* w;       // [m][16]
  const double* ht;      // [n][16]
  const int64_t* rows;   // [b] row ids (null: row0 .. row0 + b - 1)
  int64_t row0, m;
  int k, n, b;
  float* s;              // [b][n]
  unsigned* flag;        // the feed status word
};

// Block (x, y): columns 256 x .., row tiles y, y + gridDim.y, ..
__global__ __launch_bounds__(256) void k_nmf_expand(const NmfExpandArgs a) {
  __shared__ double tt[NMF_ROW_TILE][NMF_LD];
  const int t = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + t;
  const bool col_ok = j < a.n;
  double h[NMF_LD];
  {
    const double2* h2 = reinterpret_cast<const double2*>(a.ht) + (size_t)(col_ok ? j : 0) * 8;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const double2 v = col_ok ? h2[c] : make_double2(0.0, 0.0);
      h[2 * c] = 2 * c < a.k ? v.x : 0.0;
      h[2 * c + 1] = 2 * c + 1 < a.k ? v.y : 0.0;
    }
  }
  for (int64_t r0 = (int64_t)blockIdx.y * NMF_ROW_TILE; r0 < a.b; r0 += (int64_t)gridDim.y * NMF_ROW_TILE) {
    __syncthreads();   // the previous tile has been read
    {
      const int rr = t >> 4, c = t & 15;   // 256 threads: one element of the tile each
      const int64_t r = r0 + rr;
      double v = 0.0;
      if (r < a.b) {
        const int64_t src = a.rows ? a.rows[r] : a.row0 + r;
        if (src < 0 || src >= a.m) {
          if (c == 0 && blockIdx.x == 0) atomicOr(a.flag, (unsigned)FEED_BAD_ROW);
        } else if (c < a.k) {
          v = a.w[(size_t)src * NMF_LD + c];
        }
      }
      tt[rr][c] = v;
    }
    __syncthreads();
    if (col_ok) {
      for (int rr = 0; rr < NMF_ROW_TILE && r0 + rr < a.b; ++rr) {
        double s = 0.0;
#pragma unroll
        for (int c = 0; c < NMF_LD; ++c) s = fma(tt[rr][c], h[c], s);
        a.s[(size_t)(r0 + rr) * a.n + j] = (float)s;
      }
    }
  }
}

}  // namespace sdrm
