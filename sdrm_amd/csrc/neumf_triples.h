// The NeuMF evaluator's (user, item, label) triples from device-resident CSR parts (main.py:218-283 without pandas; the definition is
// include/sdrm_hip.h's at sdrm_neumf_triples, restated in tests/neumf_triples_ref.py): entry j of row r of part p becomes
// (user0_p + r, indices[j], label_p); parts in the order given, rows ascending, entries in their stored order, dense.
//   k_triple_counts  a wave per row: the checked row span (csrc/csr_batch.h's csr_row_span, held to the part's capacity and to n_items as
//                    sdrm_csr_vstack holds its rows) and the columns (csr_entry); the row's length, 0 for an offender.
//   k_csr_scan       csrc/compact.h's, as it is: lengths -> the rows' bases in the output, and the total.
//   k_triple_fill    a work-group per TRIPLE_ROWS consecutive rows.  Their triples are ONE contiguous stretch of the output, walked in
//                    chunks of TRIPLE_CHUNK triples by all 256 threads whatever the rows' lengths are: a thread finds the row of its
//                    triple among the group's bases in LDS, loads the column (consecutive threads: consecutive elements of a row) and
//                    parks the 12-byte record in LDS; the chunk then leaves as consecutive 4-byte words from consecutive lanes, 256 bytes
//                    per wave and store.  A 3000-entry row and sixteen 1-entry rows cost what their triples cost.  The same threads
//                    set the items' bytes of `item_present` and keep the label-1 count and the two maxima, reduced over the work-group
//                    in front of three integer atomics.
// Every load of a caller's index array goes through the checked span of BOTH passes; every store is held to capacity_out, n_items
// and the four counts.  Integer work, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "csr_transpose.h"

namespace sdrm {

constexpr int TRIPLE_ROWS = 16;                   // rows of a work-group of k_triple_fill
constexpr int TRIPLE_PER = 4;                     // triples per thread and chunk
constexpr int TRIPLE_CHUNK = 256 * TRIPLE_PER;    // triples per chunk: 12 KB of LDS
constexpr int64_t TRIPLE_MAX_OUT = (int64_t)1 << 30;   // sdrm_neumf_epoch_draw's bound on n

struct TriplePart { const int64_t* indptr; const int32_t* indices; int64_t n_rows, capacity; int32_t user0, label; };

struct TripleArgs {
  TriplePart part[CSR_STACK_MAX];
  int64_t first[CSR_STACK_MAX + 1];   // output row of a part's row 0; first[n_parts] = rows in all
  int n_parts, n_items;
  uint32_t* cnt;                      // [rows] checked lengths
  const int64_t* base;                // the scan's result [rows + 1]: triples in front of a row; base[rows] their sum
  int32_t* out; int64_t capacity_out;
  uint8_t* present;                   // null, or [n_items]
  unsigned long long* counts;         // the caller's int64 [4]: m, label-1 triples, max user + 1, max item + 1
  unsigned* flag;                     // the handle's feed status word
};

template <class A>   // TripleArgs, or csrc/neumf_rank.h's RankProblemArgs: n_items and flag
__device__ __forceinline__ CsrBatch triple_batch(const A& a, const TriplePart& pt) {
  return CsrBatch{pt.indptr, pt.indices, nullptr, nullptr, 0, pt.n_rows, 0, a.n_items, a.flag};
}

// Row r of a part, checked as sdrm_csr_vstack checks its rows: csr_row_span's pair, held to the part's capacity and to n_items entries.
// `owner` as in csr_row_span (0: this thread reports).
template <class A>
__device__ __forceinline__ CsrSpan triple_row_span(const A& a, const TriplePart& pt, int64_t r, int owner) {
  CsrSpan s = csr_row_span<FEED_STACK_PTR>(triple_batch(a, pt), (int)r, owner);
  if (s.p1 > pt.capacity || s.p1 - s.p0 > (int64_t)a.n_items) {
    if (owner == 0) atomicOr(a.flag, (unsigned)FEED_STACK_PTR);
    s.p0 = s.p1 = 0;
  }
  return s;
}

__global__ __launch_bounds__(256) void k_triple_counts(const TripleArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4, rows = a.first[a.n_parts];
  for (int64_t R = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); R < rows; R += nw) {   // (wave-uniform)
    int64_t r;
    const TriplePart& pt = a.part[stack_part_of(a, R, r)];
    const CsrBatch c = triple_batch(a, pt);
    const CsrSpan s = triple_row_span(a, pt, r, lane);
    int64_t len = s.p1 - s.p0;
    bool bad = false;
    for (int64_t p = s.p0 + lane; p < s.p1; p += 64) {
      int32_t col;
      float v;
      csr_entry(c, p, bad, col, v);
    }
    if (__any(bad)) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_BAD_COL);
      len = 0;
    }
    if (lane == 0) a.cnt[R] = (uint32_t)len;
  }
}

__global__ __launch_bounds__(256) void k_triple_fill(const TripleArgs a) {
  __shared__ int64_t sbase[TRIPLE_ROWS + 1];   // the group's bases; rows behind the last one repeat the total
  __shared__ int64_t ssrc[TRIPLE_ROWS];        // a row's first place in its part's indices; -1: nothing of it may be read
  __shared__ const int32_t* sidx[TRIPLE_ROWS];   // ... and that part's indices
  __shared__ int32_t suser[TRIPLE_ROWS], slabel[TRIPLE_ROWS];
  __shared__ int32_t stage[3 * TRIPLE_CHUNK];
  __shared__ unsigned long long red[4][3];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int64_t rows = a.first[a.n_parts], R0 = (int64_t)blockIdx.x * TRIPLE_ROWS;
  const int64_t total = a.base[rows];
  const int64_t m = total < a.capacity_out ? total : a.capacity_out;
  if (blockIdx.x == 0 && t == 0) {
    a.counts[0] = (unsigned long long)m;
    if (total > a.capacity_out) atomicOr(a.flag, (unsigned)FEED_STACK_PTR);   // (rows that share entries: the triples behind are dropped)
  }
  if (t <= TRIPLE_ROWS) {
    const int64_t R = R0 + t;
    sbase[t] = a.base[R < rows ? R : rows];
    if (t < TRIPLE_ROWS) {
      int64_t src = -1;
      int32_t user = 0, label = 0;
      const int32_t* idx = nullptr;
      if (R < rows) {
        int64_t r;
        const TriplePart& pt = a.part[stack_part_of(a, R, r)];
        const CsrSpan s = triple_row_span(a, pt, r, 1);   // (k_triple_counts has reported what this pass meets again)
        const int64_t len = a.base[R + 1] - a.base[R];
        if (len >= 0 && len <= s.p1 - s.p0) src = s.p0;
        user = (int32_t)((int64_t)pt.user0 + r);
        label = pt.label;
        idx = pt.indices;
      }
      ssrc[t] = src; sidx[t] = idx; suser[t] = user; slabel[t] = label;
    }
  }
  __syncthreads();
  const int64_t q_begin = sbase[0], q_end = sbase[TRIPLE_ROWS] < m ? sbase[TRIPLE_ROWS] : m;
  unsigned long long ones = 0, top_user = 0, top_item = 0;   // the maxima as id + 1
  for (int64_t q0 = q_begin; q0 < q_end; q0 += TRIPLE_CHUNK) {   // (uniform over the work-group)
    int32_t col[TRIPLE_PER], row_of[TRIPLE_PER];
#pragma unroll
    for (int u = 0; u < TRIPLE_PER; ++u) {
      const int64_t q = q0 + t + 256 * u;
      col[u] = 0; row_of[u] = -1;
      if (q < q_end) {
        int j = 0;
#pragma unroll
        for (int i = 1; i < TRIPLE_ROWS; ++i) j += sbase[i] <= q;   // (q < sbase[TRIPLE_ROWS]: j names a row with q inside)
        row_of[u] = j;
        if (ssrc[j] >= 0) col[u] = sidx[j][ssrc[j] + (q - sbase[j])];   // (inside the row's checked span: q - sbase[j] < its length)
      }
    }
#pragma unroll
    for (int u = 0; u < TRIPLE_PER; ++u) {
      const int j = row_of[u];
      if (j < 0) continue;
      const int e = t + 256 * u;
      const bool ok = ssrc[j] >= 0 && col[u] >= 0 && col[u] < a.n_items;   // (k_triple_counts emptied every row this would refuse)
      const int32_t item = ok ? col[u] : 0;
      stage[3 * e] = suser[j]; stage[3 * e + 1] = item; stage[3 * e + 2] = slabel[j];
      if (ok) {
        if (a.present) a.present[item] = 1;
        ones += (unsigned long long)(slabel[j] == 1);
        const unsigned long long un = (unsigned long long)(uint32_t)suser[j] + 1ull, in = (unsigned long long)item + 1ull;
        top_user = un > top_user ? un : top_user;
        top_item = in > top_item ? in : top_item;
      }
    }
    __syncthreads();
    const int64_t left = q_end - q0;
    const int words = 3 * (int)(left < TRIPLE_CHUNK ? left : TRIPLE_CHUNK);
    int32_t* dst = a.out + 3 * q0;   // (q0 + words / 3 <= q_end <= capacity_out)
#pragma unroll
    for (int k = 0; k < 3 * TRIPLE_PER; ++k) {
      const int w = t + 256 * k;
      if (w < words) dst[w] = stage[w];
    }
    __syncthreads();
  }
  // the work-group's three figures, then one atomic each (integers: the same result in any order)
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    ones += __shfl_down(ones, d);
    const unsigned long long ou = __shfl_down(top_user, d), oi = __shfl_down(top_item, d);
    top_user = ou > top_user ? ou : top_user;
    top_item = oi > top_item ? oi : top_item;
  }
  if (lane == 0) { red[wave][0] = ones; red[wave][1] = top_user; red[wave][2] = top_item; }
  __syncthreads();
  if (t == 0) {
    for (int w = 1; w < 4; ++w) {
      ones += red[w][0];
      top_user = red[w][1] > top_user ? red[w][1] : top_user;
      top_item = red[w][2] > top_item ? red[w][2] : top_item;
    }
    if (ones) atomicAdd(a.counts + 1, ones);
    if (top_user) atomicMax(a.counts + 2, top_user);
    if (top_item) atomicMax(a.counts + 3, top_item);
  }
}

}  // namespace sdrm
