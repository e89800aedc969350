// Rank-k truncated SVD of a sparse matrix on the device, and the scores of its rank-k reconstruction (reference: svd_benchmark.py:17-70,
// `TruncatedSVD(n_components=20, n_iter=100)` + `inverse_transform(fit_transform(.))`; sklearn's randomized SVD is a subspace iteration).
// The scheme, on a panel of SVD_PW = 32 columns (float32 panels, float64 wherever a sum decides about orthogonality):
//   Q [n, 32] start panel (Philox normals, or the caller's)
//   n_iter times:  Y = A Q,  Y <- orth(Y),  Q = A^T Y,  Q <- orth(Q)
//   Y = A Q,  Y <- orth(Y),  Z = A^T Y            (Z^T = Y^T A = B [32, n]: the one read-back of the fit)
//   host, float64: eigh(B B^T) -> the top k directions rotated into V [k, n] and normalised; sigma = sqrt(eigenvalue)
// The kernels:
//   k_svd_spmm    Y[r, 0:32] = sum_p value_p Q[col_p, 0:32] over the entries of CSR row r in CSR ORDER, one fmaf chain per output element:
//                 no atomic, the same bits on every run.  A^T Y is the same kernel on the CSC arrays (the CSR of the transpose).  A row of 32
//                 floats is 8 float4 slices: 8 lanes own a row (one slice each, 32 rows per work-group), load 8 entries of it coalesced
//                 (one each), hand them round with 8-wide shuffles and issue the 8 16-byte loads of Q before the FMAs that consume
//                 them.  Row ids, indptr pairs (against nnz as well) and column indices are range-checked (csrc/csr_batch.h): an
//                 offender is skipped and raises the feed status word.
//   orth(Y)       CholeskyQR, applied twice:  k_svd_gram   G = Y^T Y in float64, per-work-group partials in a fixed order,
//                                             k_svd_chol   one work-group adds the partials in block order, factors G = L L^T in
//                                                          float64 and leaves R^-1 = L^-T (float64 [32, 32]),
//                                             k_svd_apply  Y <- Y R^-1 row by row (float64 sums, rounded once to float32), in place.
//   k_svd_start   the Philox start panel;  k_svd_vt  V [k, n] -> V^T [n, 32] zero-padded (the scores' gather operand);
//   k_svd_expand  S [b, n] = T [b, 32] V: the rank-k expansion, bound by writing b n floats.
//
// The breakdown threshold.  With d_j the j-th pivot of the factorisation (the squared distance of column j of Y from the span of the
// columns before it) and g = max_j G[j][j]: d_j >= sigma_min(Y)^2 and g <= sigma_max(Y)^2, so a panel with cond(Y) <= 2^18 keeps every
// d_j / g >= 2^-36.  A column that depends on the others in exact arithmetic arrives as a float32 product: a sum of r terms carries a
// relative rounding of about sqrt(r) 2^-24, so its pivot sits near r 2^-48 g (2^-45 g at the r = 16 of a 40 x 40 matrix of rank 5,
// measured; the float64 Gram sums add errors of order rows 2^-53 g, far below).  SVD_PIVOT_REL = 2^-40 lies 2^4 under the first figure
// and covers rows of up to 2^8 entries in the second.  A pivot that is not greater than 2^-40 g - non-positive and NaN included - is a
// breakdown: it raises bit 0 of the fit's status word and R^-1 becomes the ZERO matrix.  The panel is then all zeros, so is every later
// Gram matrix (g = 0 fails the same test), and nothing downstream meets a NaN or an infinity: the fit runs to its end inside its own
// buffers and the host refuses the result after the read-back.  (With longer rows a dependent column's pivot can pass the test: the
// column is then normalised rounding noise - finite, and orthogonal to the others after the second pass, so the leading directions
// are still found if the rank reaches k; what is promised for a matrix of rank < 32 is a refusal or finite output, never a NaN.)
// Plain HIP, vector / plain C++ stores only; no asm MFMA in here (tests/test_isa_lint.py has nothing to hold).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "philox.h"

namespace sdrm {

constexpr int SVD_PW = 32;              // panel width
constexpr int SVD_KMAX = SVD_PW - 10;   // most components: the reference's oversampling of 10 columns must fit the panel
constexpr int SVD_GRAM_ROWS = 64;       // rows of a Gram tile
constexpr int SVD_GRAM_PARTS = 256;     // most work-groups of k_svd_gram (one per CU)
constexpr int SVD_ROW_TILE = 16;        // rows of a tile of k_svd_expand
constexpr double SVD_PIVOT_REL = 0x1p-40;
constexpr uint32_t PURPOSE_SVD_START = 10;   // csrc/philox.h's list continued: normals 4 j .. 4 j + 3 of (row of Q, column quad j)
enum { SVD_BREAKDOWN = 1u };

struct SvdSpmmArgs {
  CsrBatch csr;      // the rows of the product (for A^T: the CSC arrays, n_rows = columns of A, n_items = rows of A)
  int64_t nnz;       // entries of csr.indices: an indptr pair that reaches behind them is an empty row
  const float* q;    // [csr.n_items][32]
  float* y;          // [csr.b][32]
};

__global__ __launch_bounds__(256) void k_svd_spmm(const SvdSpmmArgs a) {
  const int lane = threadIdx.x & 7;
  const int r = blockIdx.x * 32 + (threadIdx.x >> 3);
  if (r >= a.csr.b) return;   // (the 8 lanes of a row leave together: the shuffles below stay inside a row's lanes)
  CsrSpan s = csr_row_span(a.csr, r, lane);
  if (s.p1 > a.nnz) {
    if (lane == 0) atomicOr(a.csr.flag, (unsigned)FEED_BAD_PTR);
    s.p0 = s.p1 = 0;
  }
  const float4* __restrict__ q4 = reinterpret_cast<const float4*>(a.q);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
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
    float4 w[8];
    float vv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int cu = __shfl(col, u, 8);
      vv[u] = __shfl(val, u, 8);
      w[u] = cu >= 0 ? q4[(size_t)cu * 8 + lane] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      acc.x = fmaf(vv[u], w[u].x, acc.x);
      acc.y = fmaf(vv[u], w[u].y, acc.y);
      acc.z = fmaf(vv[u], w[u].z, acc.z);
      acc.w = fmaf(vv[u], w[u].w, acc.w);
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  reinterpret_cast<float4*>(a.y)[(size_t)r * 8 + lane] = acc;
}

// part[block][32][32] = the block's share of Y^T Y in float64: block k takes the tiles k, k + gridDim.x, .. of 64 rows in that order, a
// thread owns G[i][j0 .. j0 + 3] and adds the rows of a tile in row order.  Every block writes all of its 1024 partials.
__global__ __launch_bounds__(256) void k_svd_gram(const float* __restrict__ y, int rows, double* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[SVD_GRAM_ROWS][SVD_PW + 4];
  const int t = threadIdx.x, i = t >> 3, j0 = (t & 7) * 4;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  const int tiles = (rows + SVD_GRAM_ROWS - 1) / SVD_GRAM_ROWS;
  const float4* __restrict__ y4 = reinterpret_cast<const float4*>(y);
  for (int k = blockIdx.x; k < tiles; k += gridDim.x) {
    __syncthreads();   // the previous tile has been read
    for (int e = t; e < SVD_GRAM_ROWS * 8; e += 256) {
      const int rr = e >> 3, sl = e & 7;
      const int64_t row = (int64_t)k * SVD_GRAM_ROWS + rr;
      const float4 v = row < rows ? y4[(size_t)row * 8 + sl] : make_float4(0.f, 0.f, 0.f, 0.f);
      *reinterpret_cast<float4*>(&tile[rr][sl * 4]) = v;
    }
    __syncthreads();
    for (int rr = 0; rr < SVD_GRAM_ROWS; ++rr) {
      const double yi = (double)tile[rr][i];
#pragma unroll
      for (int c = 0; c < 4; ++c) acc[c] = fma(yi, (double)tile[rr][j0 + c], acc[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) part[(size_t)blockIdx.x * (SVD_PW * SVD_PW) + i * SVD_PW + j0 + c] = acc[c];
}

// One work-group: G = the partials added in block order, G = L L^T (right-looking, float64, in LDS), rinv [32][32] = L^-T (row i, column
// j: what column i of Y contributes to column j of Y R^-1; zero below the diagonal).  A breakdown (header comment) leaves rinv zero.
__global__ __launch_bounds__(256) void k_svd_chol(const double* __restrict__ part, int parts, double* __restrict__ rinv, unsigned* __restrict__ flag) {
  __shared__ double A[SVD_PW][SVD_PW + 1];
  __shared__ double Li[SVD_PW][SVD_PW + 1];
  const int t = threadIdx.x;
  for (int e = t; e < SVD_PW * SVD_PW; e += 256) {
    double s = 0.0;
    for (int k0 = 0; k0 < parts; k0 += 8) {   // block order, eight loads in flight
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = k0 + u < parts ? part[(size_t)(k0 + u) * (SVD_PW * SVD_PW) + e] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    A[e >> 5][e & 31] = s;
    Li[e >> 5][e & 31] = 0.0;
  }
  __syncthreads();
  double g = 0.0;
  for (int j = 0; j < SVD_PW; ++j) g = fmax(g, A[j][j]);   // (fmax drops a NaN: the pivot test below meets it)
  const double thr = SVD_PIVOT_REL * g;
  bool bad = !(g > 0.0) || !(g < 1e300);
  for (int j = 0; j < SVD_PW && !bad; ++j) {   // (every thread reads the same pivot: `bad` is uniform, and so are the barriers)
    const double d = A[j][j];
    if (!(d > thr)) { bad = true; break; }
    const double l = sqrt(d);
    __syncthreads();   // every thread has read the pivot
    if (t == j) A[j][j] = l;
    else if (t > j && t < SVD_PW) A[t][j] = A[t][j] / l;
    __syncthreads();
    for (int e = t; e < SVD_PW * SVD_PW; e += 256) {
      const int i = e >> 5, k = e & 31;
      if (k > j && i >= k) A[i][k] = fma(-A[i][j], A[k][j], A[i][k]);
    }
    __syncthreads();
  }
  if (!bad && t < SVD_PW) {   // column t of L^-1 by forward substitution, the column in registers: x_i = ((i == t) - sum_{k < i} L[i][k] x_k) / L[i][i]
    double x[SVD_PW];          // (the entries above the diagonal come out as exact zeros; L is read at the same address by all 32 threads)
#pragma unroll
    for (int i = 0; i < SVD_PW; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s = fma(A[i][k], x[k], s);
      x[i] = ((i == t ? 1.0 : 0.0) - s) / A[i][i];
    }
#pragma unroll
    for (int i = 0; i < SVD_PW; ++i) Li[i][t] = x[i];
  }
  __syncthreads();
  for (int e = t; e < SVD_PW * SVD_PW; e += 256) {
    const int i = e >> 5, j = e & 31;
    rinv[e] = (!bad && i <= j) ? Li[j][i] : 0.0;
  }
  if (bad && t == 0) atomicOr(flag, (unsigned)SVD_BREAKDOWN);
}

// Y <- Y R^-1 in place: a work-group takes 32 rows, 8 lanes a row, a lane the columns j0 .. j0 + 3; every sum runs over i = 0 .. j in
// that order in float64 and is rounded once.  A row is read into LDS by the lanes that write it, before any of them writes.
__global__ __launch_bounds__(256) void k_svd_apply(float* __restrict__ y, int rows, const double* __restrict__ rinv) {
  __shared__ double R[SVD_PW][SVD_PW];
  __shared__ __attribute__((aligned(16))) float tile[32][SVD_PW + 4];
  const int t = threadIdx.x, g = t >> 3, sl = t & 7, j0 = sl * 4;
  for (int e = t; e < SVD_PW * SVD_PW; e += 256) R[e >> 5][e & 31] = rinv[e];
  const int64_t row = (int64_t)blockIdx.x * 32 + g;
  float4* y4 = reinterpret_cast<float4*>(y);
  const float4 v = row < rows ? y4[(size_t)row * 8 + sl] : make_float4(0.f, 0.f, 0.f, 0.f);
  *reinterpret_cast<float4*>(&tile[g][j0]) = v;
  __syncthreads();
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < j0 + 4; ++i) {   // (R^-1 is zero below the diagonal: rows i > j add nothing)
    const double yi = (double)tile[g][i];
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] = fma(yi, R[i][j0 + c], acc[c]);
  }
  if (row < rows) y4[(size_t)row * 8 + sl] = make_float4((float)acc[0], (float)acc[1], (float)acc[2], (float)acc[3]);
}

// The start panel: Q[i][4 j .. 4 j + 3] = the two Box-Muller pairs of Philox4x32-10 with counter (i, j, PURPOSE_SVD_START, draw), key seed.
__global__ __launch_bounds__(256) void k_svd_start(float* __restrict__ q, int n, uint32_t k0, uint32_t k1, uint32_t draw) {
  const int64_t total = (int64_t)n * 8;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const U4 w = philox4x32_10((uint32_t)(idx >> 3), (uint32_t)(idx & 7), PURPOSE_SVD_START, draw, k0, k1);
    float4 o;
    box_muller(w.x, w.y, o.x, o.y);
    box_muller(w.z, w.w, o.z, o.w);
    reinterpret_cast<float4*>(q)[idx] = o;
  }
}

// vt [n][32] = v [k][n]^T, columns k .. 31 zero.
__global__ __launch_bounds__(256) void k_svd_vt(const float* __restrict__ v, int k, int n, float* __restrict__ vt) {
  const int64_t total = (int64_t)n * SVD_PW;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int c = (int)(idx & 31);
    const int64_t j = idx >> 5;
    vt[idx] = c < k ? v[(size_t)c * n + j] : 0.f;
  }
}

struct SvdExpandArgs {
  const float* t;   // [b][32]: the rows' coordinates A_rows V^T (columns k .. 31 are zero and are not read)
  const float* v;   // [k][n]
  int k, n, b;
  float* s;         // [b][n]
};

// s[r][j] = sum_{c < k} t[r][c] v[c][j], c ascending.  A thread holds column j of V in registers and writes that column of a tile of
// SVD_ROW_TILE rows: the stores of a work-group are 256 consecutive floats of one row.  Block (x, y): columns 256 x .., row tiles y, y + gridDim.y, ..
__global__ __launch_bounds__(256) void k_svd_expand(const SvdExpandArgs a) {
  __shared__ float tt[SVD_ROW_TILE][SVD_PW];
  const int t = threadIdx.x;
  const int64_t j = (int64_t)blockIdx.x * 256 + t;
  const bool col_ok = j < a.n;
  float v[SVD_KMAX];
#pragma unroll
  for (int c = 0; c < SVD_KMAX; ++c) v[c] = (col_ok && c < a.k) ? a.v[(size_t)c * a.n + j] : 0.f;
  for (int64_t r0 = (int64_t)blockIdx.y * SVD_ROW_TILE; r0 < a.b; r0 += (int64_t)gridDim.y * SVD_ROW_TILE) {
    __syncthreads();   // the previous tile has been read
    for (int e = t; e < SVD_ROW_TILE * SVD_PW; e += 256) {
      const int64_t row = r0 + (e >> 5);
      tt[e >> 5][e & 31] = row < a.b ? a.t[(size_t)row * SVD_PW + (e & 31)] : 0.f;
    }
    __syncthreads();
    if (col_ok) {
      for (int rr = 0; rr < SVD_ROW_TILE && r0 + rr < a.b; ++rr) {
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < SVD_KMAX; ++c) s = fmaf(tt[rr][c], v[c], s);
        a.s[(size_t)(r0 + rr) * a.n + j] = s;
      }
    }
  }
}

}  // namespace sdrm
