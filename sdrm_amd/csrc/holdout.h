// Per-user hold-out split of a device-resident CSR matrix, CSR in, two CSRs out (reference utilities.py:174-236,
// split_train_test_proportion_from_csr_matrix with ignore_zeros=False): of the n stored entries of a user with n >= 2,
// m = ceil(test_prop n) chosen uniformly without replacement go to the held-out matrix and the others to the train matrix, both
// binarised (no data array), columns in CSR order.  A user with fewer than two entries is an EMPTY ROW in both outputs (the
// reference drops the row): row numbers stay the input's, nothing is compacted over rows and nothing is read back.
// The reference's MT19937 stream is not reproduced.  The draw is defined by keys: entry p (0-based place inside feed row u) has
//   w_p     = word p & 3 of philox4x32_10(u, p >> 2, PURPOSE_HOLDOUT, draw, seed)
//   rank(p) = #{q : w_q < w_p or (w_q == w_p and q < p)},        held out iff rank(p) < m_u
//   m_u     = n_u < 2 ? 0 : min(n_u, (int64)ceil(test_prop (double)n_u))            (the product and the ceil in float64)
// The m smallest of iid keys are a uniform m-subset; the tie-break by place on equal 32-bit words is a bias of order n^2 2^-32.
// The split of row u is a function of (seed, draw, u, n_u) and the row's columns alone.
//   k_holdout_counts   a wave per row: checks the row (indptr pair ordered and inside [0, nnz], at most n_items entries, every
//                      column inside [0, n_items)); an offending row is recorded in the status word and counts as empty; leaves
//                      n_u (0 for an empty row) and m_u.
//   k_holdout_scan     work-group 0: exclusive scan of n_u - m_u -> train indptr; work-group 1: of m_u -> held indptr.
//   k_holdout_split    TPR threads own a row (TPR = 64, a wave, rows of at most HOLD_WAVE_MAX entries; TPR = 256, the work-group,
//                      longer rows; each launch skips the other's rows).  An owner holds four consecutive entries - one Philox call
//                      - and ranks them against every key of the row, which pass through an LDS tile of fixed size (the wave form's
//                      rows fit one tile), so a row of any length works; the ranking is quadratic in the row length.  The owners'
//                      held counts are scanned, and both outputs leave in CSR order with a carry from chunk to chunk.
// Every store is checked against nnz, every load address comes from a checked indptr pair.  Plain HIP, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "philox.h"

namespace sdrm {

constexpr int HOLD_WAVE_MAX = 256;    // longest row of the wave form: four entries per lane
constexpr int HOLD_TILE = 2048;       // keys of an LDS tile of the work-group form (16 KB)
constexpr int HOLD_SCAN_PER = 8;      // rows per thread and chunk of k_holdout_scan

struct HoldoutArgs {
  const int64_t* indptr; const int32_t* indices;   // CSR of the feed [n_rows, n_items], nnz entries
  int64_t n_rows, nnz; int n_items;
  double test_prop;
  uint32_t k0, k1, draw;      // the 64-bit seed, low and high word (the Philox key), and counter word 3
  uint32_t* cnt;              // [2][n_rows]: n_u (0: an empty row), m_u
  int64_t* train_indptr; int32_t* train_indices;
  int64_t* held_indptr; int32_t* held_indices;
  unsigned* flag;             // the handle's feed status word
};

__host__ __device__ inline int64_t holdout_m(double test_prop, int64_t n) {
  if (n < 2) return 0;
  const int64_t m = (int64_t)ceil(test_prop * (double)n);
  return m < n ? m : n;
}

// Sort key of entry p: the word above the place - no two entries of a row share one, and `<` on it is the rank's order.
__device__ __forceinline__ uint64_t holdout_key(uint32_t w, uint32_t p) { return ((uint64_t)w << 20) | (uint64_t)p; }

__global__ __launch_bounds__(256) void k_holdout_counts(const HoldoutArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); u < a.n_rows; u += nw) {   // (wave-uniform)
    const int64_t p0 = a.indptr[u], p1 = a.indptr[u + 1];
    int64_t n = p1 - p0;
    if (p0 < 0 || p1 < p0 || p1 > a.nnz || n > (int64_t)a.n_items) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_HOLD_PTR);
      n = 0;
    }
    bool bad = false;
    for (int64_t p = p0 + lane; p < p0 + n; p += 64) {
      const int32_t c = a.indices[p];
      bad |= (c < 0 || c >= a.n_items);
    }
    if (__any(bad)) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_HOLD_COL);
      n = 0;
    }
    if (n < 2) n = 0;
    if (lane == 0) {
      a.cnt[u] = (uint32_t)n;
      a.cnt[a.n_rows + u] = (uint32_t)holdout_m(a.test_prop, n);
    }
  }
}

// indptr[r] = sum of the counts of rows 0 .. r-1, indptr[n_rows] = their sum: one work-group per output walks chunks of 2048 rows
// with a carry (csrc/compact.h: k_csr_scan).  Integers only.
__global__ __launch_bounds__(256) void k_holdout_scan(const HoldoutArgs a) {
  __shared__ int64_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool held = blockIdx.x == 1;
  int64_t* out = held ? a.held_indptr : a.train_indptr;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < a.n_rows; c0 += 256 * HOLD_SCAN_PER) {
    const int64_t r0 = c0 + (int64_t)tid * HOLD_SCAN_PER;
    uint32_t c[HOLD_SCAN_PER];
    int64_t s = 0;
#pragma unroll
    for (int j = 0; j < HOLD_SCAN_PER; ++j) {
      c[j] = 0u;
      if (r0 + j < a.n_rows) {
        const uint32_t m = a.cnt[a.n_rows + r0 + j];
        c[j] = held ? m : a.cnt[r0 + j] - m;
      }
      s += c[j];
    }
    int64_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t run = carry + inc - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wave) run += wsum[i];
      carry += wsum[i];
    }
#pragma unroll
    for (int j = 0; j < HOLD_SCAN_PER; ++j) {
      if (r0 + j < a.n_rows) out[r0 + j] = run;
      run += c[j];
    }
    __syncthreads();
  }
  if (tid == 0) out[a.n_rows] = carry;
}

template <int TPR>
__device__ __forceinline__ void holdout_barrier() {
  if (TPR == 256) __syncthreads();
  else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
}

template <int TPR>
__global__ __launch_bounds__(256) void k_holdout_split(const HoldoutArgs a) {
  constexpr int RPB = 256 / TPR;                           // rows of a work-group at a time
  constexpr int TILE = TPR == 64 ? HOLD_WAVE_MAX : HOLD_TILE;
  constexpr int CHUNK = 4 * TPR;                           // entries the owners rank at a time
  __shared__ uint64_t keys[RPB][TILE];
  __shared__ int wsum[4];
  const int g = threadIdx.x / TPR, slot = threadIdx.x % TPR, lane = threadIdx.x & 63;
  const int64_t stride = (int64_t)gridDim.x * RPB;
  for (int64_t u = (int64_t)blockIdx.x * RPB + g; u < a.n_rows; u += stride) {   // (uniform over the row's owners)
    const int n = (int)a.cnt[u];
    if (n == 0 || (TPR == 64) != (n <= HOLD_WAVE_MAX)) continue;                 // empty, or the other form's
    const int m = (int)a.cnt[a.n_rows + u];
    const int64_t p0 = a.indptr[u];
    if (p0 < 0 || p0 + n > a.nnz) continue;                                      // (k_holdout_counts saw the same pair)
    int64_t to = a.train_indptr[u], ho = a.held_indptr[u];                       // the carry of both outputs
    for (int c0 = 0; c0 < n; c0 += CHUNK) {
      const int pb = c0 + 4 * slot;                        // this owner's entries pb .. pb + 3: one Philox call
      uint64_t mine[4];
      {
        const U4 w = philox4x32_10((uint32_t)u, (uint32_t)(pb >> 2), PURPOSE_HOLDOUT, a.draw, a.k0, a.k1);
        mine[0] = holdout_key(w.x, pb); mine[1] = holdout_key(w.y, pb + 1); mine[2] = holdout_key(w.z, pb + 2); mine[3] = holdout_key(w.w, pb + 3);
      }
      int rank[4] = {0, 0, 0, 0};
      for (int t0 = 0; t0 < n; t0 += TILE) {
        const int cnt = n - t0 < TILE ? n - t0 : TILE;
        holdout_barrier<TPR>();                            // the previous tile has been read
        for (int i = slot; 4 * i < cnt; i += TPR) {        // the tile's keys; places behind the row rank behind every entry
          const int q = t0 + 4 * i;
          const U4 w = philox4x32_10((uint32_t)u, (uint32_t)(q >> 2), PURPOSE_HOLDOUT, a.draw, a.k0, a.k1);
          keys[g][4 * i] = holdout_key(w.x, q);
          keys[g][4 * i + 1] = q + 1 < n ? holdout_key(w.y, q + 1) : ~0ull;
          keys[g][4 * i + 2] = q + 2 < n ? holdout_key(w.z, q + 2) : ~0ull;
          keys[g][4 * i + 3] = q + 3 < n ? holdout_key(w.w, q + 3) : ~0ull;
        }
        holdout_barrier<TPR>();
        if (pb < n) {
          for (int q = 0; q < cnt; q += 4) {               // (the same address in every lane: LDS broadcasts)
            uint64_t k[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) k[j] = keys[g][q + j];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
              for (int e = 0; e < 4; ++e) rank[e] += k[j] < mine[e];
            }
          }
        }
      }
      // this owner's entries, its held ones, and the held ones of the owners in front of it
      const int have = pb >= n ? 0 : (n - pb < 4 ? n - pb : 4);
      bool held[4];
      int h = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) { held[e] = e < have && rank[e] < m; h += held[e]; }
      int inc = h;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      int before = inc - h, total = __shfl(inc, 63);
      if (TPR == 256) {
        if (lane == 63) wsum[threadIdx.x >> 6] = inc;
        __syncthreads();                                   // (the tile loop's barriers stand between this read and the next chunk's write)
        const int w = threadIdx.x >> 6, s0 = wsum[0], s1 = wsum[1], s2 = wsum[2], s3 = wsum[3];
        before += (w > 0 ? s0 : 0) + (w > 1 ? s1 : 0) + (w > 2 ? s2 : 0);
        total = s0 + s1 + s2 + s3;
      }
      const int ahead = pb < n ? pb - c0 : n - c0;         // entries of the chunk in front of this owner
      int64_t hp = ho + before, tp = to + (ahead - before);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (e < have) {
          const int32_t c = a.indices[p0 + pb + e];
          if (held[e]) { if (hp < a.nnz) a.held_indices[hp] = c; ++hp; }
          else { if (tp < a.nnz) a.train_indices[tp] = c; ++tp; }
        }
      }
      const int in_chunk = n - c0 < CHUNK ? n - c0 : CHUNK;
      ho += total; to += in_chunk - total;
    }
  }
}

}  // namespace sdrm
