// Equal-sparsity output as CSR, built on the device from a bit mask (main.py:177-180 and, for the `<=` side, :259-262):
//     threshold = np.quantile(M.flatten(), q);  csr_matrix(M >= threshold)  |  csr_matrix(F <= threshold)
// The threshold is csrc/select.h's (SelectState, the three k_select_hist / k_select_pick passes, unchanged).  Behind it:
//   k_csr_mask   one sweep over x [n_rows, n_cols]: a bit mask of wpr = ceil(n_cols / 64) 64-bit words per row (bit c % 64 of word
//                c / 64 is the comparison of column c; the bits behind n_cols in a row's last word are 0 on both sides) and the row
//                counts (popcounts, integer atomics: one per row and wave, the same sum in any order).  4 B read + 1/8 B written
//                per element; the dense binarise moves 5.
//   k_csr_scan   exclusive scan of the row counts -> int64 indptr [n_rows + 1] (one work-group walks chunks of 2048 rows with a carry).
//   k_csr_fill   int32 indices [nnz] from the mask and the row offsets alone (x is not read again): within a row the word offsets are
//                a scan of the popcounts, inside a word the position is the popcount of the lower bits - columns ascend.
// No data array: the matrix is all ones.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrm {

constexpr int CSR_MASK_WORDS = 32;                   // mask words a wave of k_csr_mask makes (at most 64: lane k keeps word k)
constexpr int CSR_MASK_BATCH = 32;                   // loads a lane has in flight before the first comparison (divides CSR_MASK_WORDS)
constexpr int CSR_SCAN_PER = 8;                      // rows per thread and chunk of k_csr_scan
constexpr int CSR_SCAN_CHUNK = 256 * CSR_SCAN_PER;   // rows per chunk

// A work-group barrier that orders LDS traffic only: __syncthreads() also waits for every global load and store of the wave
// (k_csr_scan: the prefetched counts, the offsets just stored - a memory round trip per chunk), which no other wave reads.
__device__ __forceinline__ void csr_lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// A wave owns 32 consecutive words of the mask (the mask is [n_rows][wpr] words, flat: whatever the row length, every wave has
// the same work and stores 256 contiguous bytes).  Iteration k makes word g0 + k: the wave's 64 lanes compare 64 consecutive
// columns of that word's row, and the ballot IS the word, already in column order; lane k keeps it, so the words leave in ONE
// vector store of 32 lanes instead of 32 single-lane ones.  Rows are not 16-byte aligned in general (3125, 8582 columns): 4-byte
// loads, all 32 of a lane requested before the first comparison - a wave's life is then one memory round trip, which is what the
// sweep takes at the shapes whose waves all fit the chip at once (ML-1M: 8314 waves; 64 words per wave in batches of 8 or 16: 17 us).
// A lane without an element (behind n_cols, or behind the last word) loads column 0 of a row of the matrix and
// contributes a 0 bit whatever the side: a stale or zero value would satisfy `<=`.
template <int SIDE>   // 0: x >= threshold, 1: x <= threshold
__global__ __launch_bounds__(256) void k_csr_mask(const float* __restrict__ x, int n_cols, int wpr, uint32_t total_words,
                                                  const float* __restrict__ thr, uint64_t* __restrict__ mask,
                                                  uint32_t* __restrict__ counts) {
  const int lane = threadIdx.x & 63;
  const uint32_t g0 = (blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6))) * CSR_MASK_WORDS;   // wave-uniform
  if (g0 >= total_words) return;
  const float t = *thr;
  const int nw = (int)min((uint32_t)CSR_MASK_WORDS, total_words - g0);
  const uint32_t r0 = g0 / (uint32_t)wpr;
  int w = (int)(g0 - r0 * (uint32_t)wpr);           // word-in-row and row of iteration k (wave-uniform, carried; they stop at the
  const float* rowp = x + (int64_t)r0 * n_cols;     // wave's last word, so rowp never leaves the matrix)
  uint64_t keep = 0;
  for (int k0 = 0; k0 < nw; k0 += CSR_MASK_BATCH) {
    float v[CSR_MASK_BATCH];
    bool have[CSR_MASK_BATCH];
#pragma unroll
    for (int j = 0; j < CSR_MASK_BATCH; ++j) {
      const int c = w * 64 + lane;
      have[j] = (k0 + j < nw) && (c < n_cols);
      v[j] = rowp[have[j] ? c : 0];
      if (k0 + j + 1 < nw && ++w == wpr) { w = 0; rowp += n_cols; }
    }
#pragma unroll
    for (int j = 0; j < CSR_MASK_BATCH; ++j) {
      const bool p = SIDE ? v[j] <= t : v[j] >= t;
      const uint64_t b = __ballot(have[j] & p);
      if (lane == k0 + j) keep = b;
    }
  }
  if (lane < nw) mask[g0 + lane] = keep;
  // row counts: lane k holds word g0 + k of row rk; an inclusive scan of the popcounts over the lanes, and the last lane of every
  // row inside this wave adds (its prefix - the prefix in front of the row's first lane here) to that row's count
  const uint32_t gk = g0 + lane;
  const uint32_t rk = gk / (uint32_t)wpr;
  const int wk = (int)(gk - rk * (uint32_t)wpr);
  const int cnt = lane < nw ? __popcll(keep) : 0;
  int inc = cnt;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int up = __shfl_up(inc, d);
    if (lane >= d) inc += up;
  }
  const int head = max(0, lane - wk);                      // first lane of my row in this wave
  const int before = __shfl(inc, max(head - 1, 0));
  const int seg = inc - (head > 0 ? before : 0);
  const bool last = lane < nw && (wk == wpr - 1 || lane == nw - 1);
  if (last && seg) atomicAdd(&counts[rk], (uint32_t)seg);
}

// indptr[r] = sum of counts[0 .. r), indptr[n_rows] = nnz; written twice: `own` is the engine's copy that k_csr_fill reads (the
// caller's array may be anything by then), and nnz once more into `nnz_out` (host memory the device can write: the host reads it
// behind the stream synchronise, no copy command).  One work-group; a chunk is 8 consecutive rows per thread, scanned over the wave
// by shuffles and over the four waves through LDS; the carry runs from chunk to chunk, and the counts of the next chunk are
// requested before this one is scanned (the chain from chunk to chunk is then shuffles and two LDS-only barriers).  Integers only.
__global__ __launch_bounds__(256) void k_csr_scan(const uint32_t* __restrict__ counts, int64_t n_rows, int64_t* __restrict__ own,
                                                  int64_t* __restrict__ indptr, int64_t* __restrict__ nnz_out) {
  __shared__ int64_t wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  uint32_t nxt[CSR_SCAN_PER];
#pragma unroll
  for (int j = 0; j < CSR_SCAN_PER; ++j) {
    const int64_t r = (int64_t)tid * CSR_SCAN_PER + j;
    nxt[j] = (r < n_rows) ? counts[r] : 0u;
  }
  for (int64_t c0 = 0; c0 < n_rows; c0 += CSR_SCAN_CHUNK) {
    const int64_t r0 = c0 + (int64_t)tid * CSR_SCAN_PER;
    uint32_t c[CSR_SCAN_PER];
    int64_t s = 0;
#pragma unroll
    for (int j = 0; j < CSR_SCAN_PER; ++j) {
      c[j] = nxt[j];
      s += c[j];
      const int64_t r = r0 + CSR_SCAN_CHUNK + j;
      nxt[j] = (r < n_rows) ? counts[r] : 0u;
    }
    int64_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int64_t up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    csr_lds_barrier();
    int64_t run = carry + inc - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wave) run += wsum[i];
      carry += wsum[i];
    }
#pragma unroll
    for (int j = 0; j < CSR_SCAN_PER; ++j) {
      if (r0 + j < n_rows) { own[r0 + j] = run; indptr[r0 + j] = run; }
      run += c[j];
    }
    csr_lds_barrier();
  }
  if (tid == 0) { own[n_rows] = carry; indptr[n_rows] = carry; *nnz_out = carry; }
}

// G lanes own a row (G = 64: a wave; G = 16: four rows per wave, for rows of at most 32 words - 2048 columns - where a wave would
// idle three lanes in four).  Lane `sub` of the group takes the words sub, sub + G, ...: their popcounts are scanned over the group,
// the running position carries from round to round, and every lane writes the columns of its word's set bits, lowest first, at its
// own offset: ascending columns in [rowptr[r], rowptr[r + 1]).  An empty row costs its two offsets.  Every store is checked against
// nnz besides (the offsets and the mask come from the same sweep; the check costs nothing against a store).
template <int G>
__global__ __launch_bounds__(256) void k_csr_fill(const uint64_t* __restrict__ mask, const int64_t* __restrict__ rowptr, int64_t n_rows,
                                                  int wpr, int32_t* __restrict__ indices, int64_t nnz) {
  const int sub = threadIdx.x % G;
  const int64_t ngrp = (int64_t)gridDim.x * (256 / G);
  for (int64_t r = (int64_t)blockIdx.x * (256 / G) + threadIdx.x / G; r < n_rows; r += ngrp) {
    int64_t pos = rowptr[r];
    if (rowptr[r + 1] == pos) continue;   // (the same in every lane of the group)
    const uint64_t* row = mask + r * wpr;
    for (int w0 = 0; w0 < wpr; w0 += G) {
      const int w = w0 + sub;
      uint64_t m = (w < wpr) ? row[w] : 0ull;
      const int cnt = __popcll(m);
      int inc = cnt;
#pragma unroll
      for (int d = 1; d < G; d <<= 1) {
        const int up = __shfl_up(inc, d, G);
        if (sub >= d) inc += up;
      }
      int64_t o = pos + inc - cnt;
      const int col0 = w * 64;
      while (m) {
        const int b = __ffsll((unsigned long long)m) - 1;
        if (o < nnz) indices[o] = col0 + b;
        ++o;
        m &= m - 1;
      }
      pos += __shfl(inc, G - 1, G);
    }
  }
}

}  // namespace sdrm
