// The NeuMF evaluator's ranking problem on the device (neural_cf_benchmark_pt.py:294-326 as sdrm_amd/neumf.py's RankingProblem states it:
// the columns and the two CSR matrices its rankings select rows from), from the CSR parts sdrm_neumf_triples reads, the item bytes it
// wrote and the held-out triples.  The definition is include/sdrm_hip.h's at sdrm_neumf_rank_problem, restated in tests/neumf_rank_ref.py:
//   cols      the ids i with item_present[i] != 0, ascending; col_of[i] the place of i in cols, -1 for an absent item; C their number.
//   seen      CSR [n_rows, C], int64 indptr, int32 indices, no data, rows DENSE BY USER ID (row u is user u): row u is the ascending,
//             duplicate-free union, over every part p with user0_p <= u < user0_p + n_rows_p, of col_of[] of the present items of that part's
//             row u - user0_p.  A user no part covers has an empty row.  A part row is checked exactly as sdrm_neumf_triples checks it
//             (csrc/csr_batch.h's csr_row_span with FEED_STACK_PTR, held to the part's capacity and to n_items entries; csr_entry with
//             FEED_BAD_COL): an offending row contributes nothing.  A part row with an entry whose user is n_rows or above contributes
//             nothing and raises FEED_BAD_ROW.
//   relevant  the same form from the held-out triples (user, item, label): a triple whose user is outside [0, n_rows) is dropped, counted
//             and raises FEED_BAD_ROW; one whose item is outside [0, n_items) is dropped, counted and raises FEED_BAD_COL (either whatever
//             its label); of the others those with label > 0 and a present item set their bit, an absent item is dropped silently (a
//             held-out item that never occurs in training is no column), duplicates merge.
// The form: one bit table per matrix, [n_rows][wpr = ceil(n_items / 64)] 64-bit words over RAW item ids in csrc/compact.h's mask layout.
//   k_rank_cols        one work-group: item_present compacted into cols, col_of and C (chunks of 2048 bytes with a carry).
//   k_rank_mark_parts  a wave per part row: the checked span and a first pass over the columns (a bad one empties the row), then 64 entries
//                      per round: lanes whose bits fall into the same word OR them together across the wave (a row's columns ascend in the
//                      engine's own CSR, so a word's lanes are neighbours; any order is still correct, it only costs more atomics) and ONE
//                      64-bit integer atomic OR leaves per run of equal words - not one per entry.
//   k_rank_mark_held   a lane per held-out triple, one atomic OR; the dropped triples counted per wave, one integer atomic add.
//   k_rank_counts      a wave per table row: the popcounts of its words -> the row's length, for both tables.
//   k_csr_scan         csrc/compact.h's, as it is, once per matrix: lengths -> indptr (the engine's copy and the caller's) and nnz.
//   k_rank_fill        k_csr_fill's walk over both tables with the emitted column mapped through col_of (monotone: ascending ids give
//                      ascending columns); every store held to the caller's capacity.
//   k_rank_users       one work-group: a uint8 mask [n_rows] compacted into the ascending int32 user list and its length.
// Integer atomics only (OR into words the call cleared, one add): the same bytes on every run.  Vector stores, plain C++.
//   registers / LDS: every kernel here is a handful of integers per lane (VGPRs: cols 62, users 60, mark_parts 31, mark_held 8, counts 24,
//   fill 36, k_rank_metrics_rows 69 as the checked form; no spill); LDS is the compaction's 4 wave sums (16 bytes) and the ranking body's
//   1168 bytes beside the score row; scratch (SCR_RANK_WS, 8-byte words): 2 totals, 2 n_rows wpr table words, 2 (n_rows + 1) row offsets,
//   n_rows + 1 row lengths of both tables, n_items / 2 words of col_of.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "compact.h"
#include "csr_batch.h"
#include "csr_transpose.h"
#include "neumf_triples.h"
#include "rank.h"

namespace sdrm {

constexpr int64_t RANKP_MAX_DIM = (int64_t)1 << 22;          // n_rows, n_items, total part rows
constexpr int64_t RANKP_MAX_TABLE = (int64_t)1 << 31;        // bytes of one bit table
constexpr int64_t RANKP_MAX_HELD = (int64_t)1 << 30;         // held-out triples

struct RankProblemArgs {
  TriplePart part[CSR_STACK_MAX];
  int64_t first[CSR_STACK_MAX + 1];   // running row count in front of a part; first[n_parts] = part rows in all
  int n_parts, n_items;               // (stack_part_of and triple_row_span read these four as TripleArgs')
  unsigned* flag;                     // the handle's feed status word
  int64_t n_rows; int wpr;
  const uint8_t* present;             // [n_items]
  const int32_t* held; int64_t n_held;
  uint64_t* table[2];                 // seen, relevant: [n_rows][wpr]
  uint32_t* cnt[2];                   // [n_rows] row lengths
  const int64_t* own[2];              // the scan's result [n_rows + 1], the engine's copy
  int32_t* col_of;                    // [n_items]
  int32_t* cols;                      // the caller's, [>= n_items]
  int32_t* indices[2]; int64_t capacity[2];
  unsigned long long* counts;         // the caller's int64 [4]: C, seen nnz, relevant nnz, held-out triples dropped for a range defect
};

// A uint8 mask [n] compacted by ONE work-group of 256: ids[j] = the j-th i with mask[i] != 0, ascending; inverse[i] (when given) = that j, or
// -1; *count = their number.  Chunks of CSR_SCAN_CHUNK = 2048 bytes, 8 consecutive ones per thread, scanned over the wave by shuffles and
// over the four waves through LDS, the carry running from chunk to chunk.
__device__ __forceinline__ void rank_compact_mask(const uint8_t* __restrict__ mask, int64_t n, int32_t* __restrict__ ids,
                                                  int32_t* __restrict__ inverse, unsigned long long* __restrict__ count) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int64_t carry = 0;
  for (int64_t c0 = 0; c0 < n; c0 += CSR_SCAN_CHUNK) {   // (uniform over the work-group)
    const int64_t i0 = c0 + (int64_t)tid * CSR_SCAN_PER;
    bool on[CSR_SCAN_PER];
    int s = 0;
#pragma unroll
    for (int j = 0; j < CSR_SCAN_PER; ++j) {
      on[j] = (i0 + j < n) && mask[i0 + j] != 0;
      s += on[j];
    }
    int inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int64_t run = carry + inc - s;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wave) run += wsum[w];
      carry += wsum[w];
    }
#pragma unroll
    for (int j = 0; j < CSR_SCAN_PER; ++j) {
      if (i0 + j >= n) break;
      if (on[j]) ids[run] = (int32_t)(i0 + j);          // (run < the number of set bytes <= n)
      if (inverse) inverse[i0 + j] = on[j] ? (int32_t)run : -1;
      run += on[j];
    }
    __syncthreads();
  }
  if (tid == 0) *count = (unsigned long long)carry;
}

__global__ __launch_bounds__(256) void k_rank_cols(const RankProblemArgs a) {
  rank_compact_mask(a.present, a.n_items, a.cols, a.col_of, a.counts);
}

__global__ __launch_bounds__(256) void k_rank_users(const uint8_t* __restrict__ mask, int64_t n_rows, int32_t* __restrict__ users,
                                                    unsigned long long* __restrict__ count) {
  rank_compact_mask(mask, n_rows, users, nullptr, count);
}

__global__ __launch_bounds__(256) void k_rank_mark_parts(const RankProblemArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4, rows = a.first[a.n_parts];
  for (int64_t R = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); R < rows; R += nw) {   // (wave-uniform)
    int64_t r;
    const TriplePart& pt = a.part[stack_part_of(a, R, r)];
    const CsrBatch c = triple_batch(a, pt);
    const CsrSpan s = triple_row_span(a, pt, r, lane);
    if (s.p1 == s.p0) continue;
    bool bad = false;
    for (int64_t p = s.p0 + lane; p < s.p1; p += 64) {
      int32_t col;
      float v;
      csr_entry(c, p, bad, col, v);
    }
    if (__any(bad)) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_BAD_COL);
      continue;
    }
    const int64_t user = (int64_t)pt.user0 + r;
    if (user >= a.n_rows) {                               // (user0 >= 0: never below)
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_BAD_ROW);
      continue;
    }
    uint64_t* row = a.table[0] + (size_t)user * (size_t)a.wpr;
    for (int64_t p0 = s.p0; p0 < s.p1; p0 += 64) {
      const int64_t p = p0 + lane;
      int w = -1;
      unsigned long long bits = 0ull;
      if (p < s.p1) {
        const int32_t col = pt.indices[p];                // (the pass above found every column of the row inside [0, n_items))
        if (col >= 0 && col < a.n_items && a.present[col] != 0) { w = col >> 6; bits = 1ull << (col & 63); }
      }
      // a run of neighbouring lanes with one word: its last lane ends up with the bits of all of them (lanes further off with the same
      // word may add theirs too - the same word of the same row)
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long ub = __shfl_up(bits, d);
        const int uw = __shfl_up(w, d);
        if (lane >= d && uw == w) bits |= ub;
      }
      const int next = __shfl_down(w, 1);
      if (w >= 0 && (lane == 63 || next != w)) atomicOr(reinterpret_cast<unsigned long long*>(row + w), bits);
    }
  }
}

__global__ __launch_bounds__(256) void k_rank_mark_held(const RankProblemArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  unsigned raise = 0;
  if (j < a.n_held) {
    const int32_t user = a.held[3 * j], item = a.held[3 * j + 1], label = a.held[3 * j + 2];
    if (user < 0 || (int64_t)user >= a.n_rows) raise |= (unsigned)FEED_BAD_ROW;
    if (item < 0 || item >= a.n_items) raise |= (unsigned)FEED_BAD_COL;
    if (!raise && label > 0 && a.present[item] != 0)
      atomicOr(reinterpret_cast<unsigned long long*>(a.table[1] + (size_t)user * (size_t)a.wpr + (size_t)(item >> 6)), 1ull << (item & 63));
  }
  const unsigned long long dropped = (unsigned long long)__popcll(__ballot(raise != 0));
  if (dropped) {   // (wave-uniform)
    if (raise) atomicOr(a.flag, raise);
    if (lane == 0) atomicAdd(a.counts + 3, dropped);
  }
}

__global__ __launch_bounds__(256) void k_rank_counts(const RankProblemArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  for (int64_t R = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); R < 2 * a.n_rows; R += nw) {   // (wave-uniform)
    const int t = R >= a.n_rows;
    const int64_t u = R - (t ? a.n_rows : 0);
    const uint64_t* row = a.table[t] + (size_t)u * (size_t)a.wpr;
    int n = 0;
    for (int w = lane; w < a.wpr; w += 64) n += __popcll(row[w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) n += __shfl_down(n, d);
    if (lane == 0) a.cnt[t][u] = (uint32_t)n;
  }
}

// k_csr_fill<64>'s walk (csrc/compact.h) over the rows of both tables, blockIdx.y the table: lane `lane` takes the words lane, lane + 64, ..,
// their popcounts are scanned over the wave, and every lane writes col_of[] of its word's set bits, lowest first, at its own offset.
__global__ __launch_bounds__(256) void k_rank_fill(const RankProblemArgs a) {
  const int lane = threadIdx.x & 63, t = blockIdx.y;
  const int64_t nw = (int64_t)gridDim.x * 4, cap = a.capacity[t];
  const int64_t* rowptr = a.own[t];
  int32_t* out = a.indices[t];
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t total = rowptr[a.n_rows];
    a.counts[1 + t] = (unsigned long long)(total < cap ? total : cap);
    if (total > cap) atomicOr(a.flag, (unsigned)FEED_STACK_PTR);   // (part rows that share entries: the columns behind the capacity are dropped)
  }
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.n_rows; r += nw) {   // (wave-uniform)
    int64_t pos = rowptr[r];
    if (rowptr[r + 1] == pos) continue;
    const uint64_t* row = a.table[t] + (size_t)r * (size_t)a.wpr;
    for (int w0 = 0; w0 < a.wpr; w0 += 64) {
      const int w = w0 + lane;
      uint64_t m = (w < a.wpr) ? row[w] : 0ull;
      const int cnt = __popcll(m);
      int inc = cnt;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d);
        if (lane >= d) inc += up;
      }
      int64_t o = pos + inc - cnt;
      const int col0 = w * 64;
      while (m) {
        const int item = col0 + __ffsll((unsigned long long)m) - 1;
        if (o < cap && item < a.n_items) out[o] = a.col_of[item];   // (only present items inside [0, n_items) were marked)
        ++o;
        m &= m - 1;
      }
      pos += __shfl(inc, 63);
    }
  }
}

// The ranking body of csrc/rank.h with the row map and the NeuMF footing: sdrm_rank_metrics_rows.
__global__ __launch_bounds__(256) void k_rank_metrics_rows(const RankArgs a, const RankCheck ck, const RankRows rm) {
  rank_metrics_user<true, true, true>(a, ck, rm);
}

}  // namespace sdrm
