// Two primitives on device-resident CSR matrices, integer kernels with a bit-exact reference (scipy):
//
// sdrm_csr_transpose   CSR [m, n] -> CSC (the CSR of the transpose): colptr from 0, row indices ascending within a column, the values
//                      along with them.  Columns within a row must be distinct and need not be sorted.  A row-blocked bit table, in the
//                      spirit of csrc/compact.h: rows are taken 64 at a time, and for row block B and column c the 64-bit word W[B][c] has
//                      bit j set when row 64 B + j holds column c.  Where an entry lands follows from the table alone, so the result does not
//                      depend on the order in which the passes meet the entries:
//   k_csrt_mark     a wave per row, one pass over the entries: every entry is checked (csrc/csr_batch.h) and ORs its row's bit into
//                   W[B][c] - a 64-bit integer atomic in global memory, the same word in any order - and the wave adds its checked
//                   entries to one integer count.  k_csrt_mark_lds makes the same table from column tiles of CSRT_TILE words in LDS, a
//                   work-group per row block and tile (LDS atomics, plain stores); the host takes it while a block's entries are read
//                   by at most CSRT_LDS_MAX_TILES work-groups (the measurement: profiles/svd_resident_bench.txt).
//   k_csrt_colscan  a thread per column walks the row blocks: off[B][c] is the exclusive running popcount, counts[c] the total; the
//                   loads of a wave are 64 consecutive words.
//   k_csr_scan      csrc/compact.h's, as it is: counts -> colptr (the caller's, and the engine's own copy that the fill reads).
//   k_csrt_fill     a wave per row, the same pass again: entry p of row r = 64 B + j with column c goes to
//                       q = colptr[c] + off[B][c] + popc(W[B][c] & ((1 << j) - 1)),      rowidx[q] = r,  cdata[q] = data[p].
//                   Every store is checked against the capacity.  One thread compares the scan's total with the count of checked
//                   entries: fewer bits than entries means that some row held a column twice (FEED_T_DUP: the output is not the
//                   transpose); a total above the capacity (rows that share entries) is reported as a bad indptr pair.
// A bad indptr pair (negative, out of order, or reaching behind the capacity) makes the row contribute nothing, a column outside
// [0, n_cols) is skipped; both raise the feed status word.  No float atomics; nothing is read back.
//
// sdrm_csr_vstack      up to CSR_STACK_MAX CSR matrices of one width, one under the other, rows checked the way sdrm_holdout_split
//                      checks them (the output feeds sdrm_rank_metrics, which trusts its column indices): a row with a bad indptr pair
//                      or with a column outside [0, n_cols) is EMPTY in the output and recorded in the status word.
//   k_stack_counts  a wave per output row: finds its part and checks it; leaves the row's length (0 for an offender).
//   k_csr_scan      the lengths -> indptr_out.  A part's true entry count never reaches the host: the parts' bases are this scan's.
//   k_stack_copy    a wave per output row copies its entries in their own order; a part without values contributes 1.0f.
// Plain HIP, vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"

namespace sdrm {

constexpr int64_t CSRT_MAX_DIM = (int64_t)1 << 22;     // most rows, and most columns
constexpr int64_t CSRT_MAX_WORDS = (int64_t)1 << 26;   // most words of the bit table, ceil(m / 64) n: 0.5 GB, and as many 4-byte offsets
constexpr int CSRT_TILE = 4096;                        // columns of an LDS tile of k_csrt_mark_lds: 32 KB
constexpr int CSRT_LDS_MAX_TILES = 9;                  // widest matrix, in tiles, whose mark pass runs on LDS tiles: every tile reads the block's entries,
                                                       // and 9 tiles (36864 columns, sdrm_rank_metrics' widest) is the widest measured - the faster form there
constexpr int CSR_STACK_MAX = 8;                       // most parts of one sdrm_csr_vstack

struct CsrTransposeArgs {
  CsrBatch csr;            // the matrix: rows 0 .. n_rows - 1, n_items = n_cols
  int64_t capacity;        // elements of csr.indices / csr.data and of rowidx / cdata
  uint64_t* table;         // W [blocks][n_cols]
  uint32_t* off;           // [blocks][n_cols]
  uint32_t* counts;        // [n_cols]
  const int64_t* colptr;   // the engine's copy of the scan's result [n_cols + 1]
  const int64_t* total;    // ... and its last element once more
  unsigned long long* checked;   // entries that passed k_csrt_mark's checks
  int blocks;              // ceil(n_rows / 64)
  int32_t* rowidx; float* cdata;
};

// Row r's stretch of the entry arrays, checked against the capacity as well; `owner` as in csr_row_span (0: this thread reports).
__device__ __forceinline__ CsrSpan csrt_row_span(const CsrTransposeArgs& a, int r, int owner) {
  CsrSpan s = csr_row_span(a.csr, r, owner);
  if (s.p1 > a.capacity) {
    if (owner == 0) atomicOr(a.csr.flag, (unsigned)FEED_BAD_PTR);
    s.p0 = s.p1 = 0;
  }
  return s;
}

__global__ __launch_bounds__(256) void k_csrt_mark(const CsrTransposeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const size_t n = (size_t)a.csr.n_items;
  unsigned long long seen = 0;   // (the same in every lane)
  bool bad = false;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.csr.n_rows; r += nw) {   // (wave-uniform)
    const CsrSpan s = csrt_row_span(a, (int)r, lane);
    uint64_t* row = a.table + (size_t)(r >> 6) * n;
    const unsigned long long bit = 1ull << (r & 63);
    for (int64_t p0 = s.p0; p0 < s.p1; p0 += 64) {
      const int64_t p = p0 + lane;
      bool ok = false;
      if (p < s.p1) {
        int32_t c;
        float v;
        ok = csr_entry(a.csr, p, bad, c, v);
        if (ok) atomicOr(reinterpret_cast<unsigned long long*>(row + c), bit);
      }
      seen += (unsigned long long)__popcll(__ballot(ok));
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  if (lane == 0 && seen) atomicAdd(a.checked, seen);
}

// The same table from column tiles in LDS: work-group (B, t) owns the words W[B][t CSRT_TILE ..] of ONE row block, ORs into them with
// LDS atomics while its four waves walk the block's 64 rows, and stores every word of its tile once, coalesced - no global atomic, and
// no clearing of the table in front of the launch.  Each of the ceil(n_cols / CSRT_TILE) tiles of a block reads all of the block's
// entries and counts those that fall into it; tile 0's work-group reports the block's bad indptr pairs.
__global__ __launch_bounds__(256) void k_csrt_mark_lds(const CsrTransposeArgs a) {
  __shared__ unsigned long long tile[CSRT_TILE];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c0 = (int)blockIdx.y * CSRT_TILE;
  const int width = a.csr.n_items - c0 < CSRT_TILE ? a.csr.n_items - c0 : CSRT_TILE;
  for (int i = threadIdx.x; i < width; i += 256) tile[i] = 0ull;
  __syncthreads();
  unsigned long long seen = 0;   // (the same in every lane)
  bool bad = false;
  for (int j = wave; j < 64; j += 4) {   // (wave-uniform)
    const int64_t r = (int64_t)blockIdx.x * 64 + j;
    if (r >= a.csr.n_rows) break;
    const CsrSpan s = csrt_row_span(a, (int)r, blockIdx.y == 0 ? lane : 1);
    for (int64_t p0 = s.p0; p0 < s.p1; p0 += 64) {
      const int64_t p = p0 + lane;
      bool ok = false;
      if (p < s.p1) {
        int32_t c;
        float v;
        if (csr_entry(a.csr, p, bad, c, v) && c >= c0 && c < c0 + width) {
          atomicOr(&tile[c - c0], 1ull << j);
          ok = true;
        }
      }
      seen += (unsigned long long)__popcll(__ballot(ok));
    }
  }
  if (bad && blockIdx.y == 0) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  if (lane == 0 && seen) atomicAdd(a.checked, seen);
  __syncthreads();
  uint64_t* row = a.table + (size_t)blockIdx.x * (size_t)a.csr.n_items + (size_t)c0;
  for (int i = threadIdx.x; i < width; i += 256) row[i] = tile[i];
}

__global__ __launch_bounds__(256) void k_csrt_colscan(const CsrTransposeArgs a) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= a.csr.n_items) return;
  const size_t n = (size_t)a.csr.n_items;
  uint32_t run = 0;
  for (int b = 0; b < a.blocks; ++b) {
    const size_t i = (size_t)b * n + (size_t)c;
    a.off[i] = run;
    run += (uint32_t)__popcll(a.table[i]);
  }
  a.counts[c] = run;
}

__global__ __launch_bounds__(256) void k_csrt_fill(const CsrTransposeArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4;
  const size_t n = (size_t)a.csr.n_items;
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const int64_t total = *a.total, checked = (int64_t)*a.checked;
    if (total != checked) atomicOr(a.csr.flag, (unsigned)FEED_T_DUP);
    if (total > a.capacity) atomicOr(a.csr.flag, (unsigned)FEED_BAD_PTR);
  }
  bool bad = false;   // (k_csrt_mark has reported what this pass meets again)
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.csr.n_rows; r += nw) {   // (wave-uniform)
    const CsrSpan s = csrt_row_span(a, (int)r, 1);
    const size_t base = (size_t)(r >> 6) * n;
    const uint64_t below = (1ull << (r & 63)) - 1ull;
    for (int64_t p = s.p0 + lane; p < s.p1; p += 64) {
      int32_t c;
      float v;
      if (!csr_entry(a.csr, p, bad, c, v)) continue;
      const int64_t q = a.colptr[c] + (int64_t)a.off[base + c] + (int64_t)__popcll(a.table[base + c] & below);
      if (q >= 0 && q < a.capacity) {
        a.rowidx[q] = (int32_t)r;
        if (a.cdata) a.cdata[q] = v;
      }
    }
  }
}

// ---- sdrm_csr_vstack ----
struct CsrStackPart { const int64_t* indptr; const int32_t* indices; const float* data; int64_t capacity; };

struct CsrStackArgs {
  CsrStackPart part[CSR_STACK_MAX];
  int64_t first[CSR_STACK_MAX + 1];   // output row of a part's row 0; first[n_parts] = rows of the output
  int n_parts, n_cols;
  uint32_t* cnt;             // [rows] checked lengths
  const int64_t* rowptr;     // the engine's copy of the scan's result [rows + 1]
  int32_t* indices_out; float* data_out; int64_t capacity_out;
  unsigned* flag;            // the handle's feed status word
};

// The part of output row R (wave-uniform) and the row's number inside it; A holds n_parts and first[] (csrc/neumf_triples.h's too).
template <class A>
__device__ __forceinline__ int stack_part_of(const A& a, int64_t R, int64_t& r) {
  int k = 0;
  while (k + 1 < a.n_parts && R >= a.first[k + 1]) ++k;
  r = R - a.first[k];
  return k;
}

__global__ __launch_bounds__(256) void k_stack_counts(const CsrStackArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4, rows = a.first[a.n_parts];
  for (int64_t R = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); R < rows; R += nw) {   // (wave-uniform)
    int64_t r;
    const CsrStackPart& pt = a.part[stack_part_of(a, R, r)];
    const int64_t p0 = pt.indptr[r], p1 = pt.indptr[r + 1];
    int64_t len = p1 - p0;
    if (p0 < 0 || p1 < p0 || p1 > pt.capacity || len > (int64_t)a.n_cols) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_STACK_PTR);
      len = 0;
    }
    bool bad = false;
    for (int64_t p = p0 + lane; p < p0 + len; p += 64) {
      const int32_t c = pt.indices[p];
      bad |= (c < 0 || c >= a.n_cols);
    }
    if (__any(bad)) {
      if (lane == 0) atomicOr(a.flag, (unsigned)FEED_STACK_COL);
      len = 0;
    }
    if (lane == 0) a.cnt[R] = (uint32_t)len;
  }
}

__global__ __launch_bounds__(256) void k_stack_copy(const CsrStackArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nw = (int64_t)gridDim.x * 4, rows = a.first[a.n_parts];
  for (int64_t R = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); R < rows; R += nw) {   // (wave-uniform)
    const int64_t o = a.rowptr[R], len = a.rowptr[R + 1] - o;
    if (len <= 0) continue;
    int64_t r;
    const CsrStackPart& pt = a.part[stack_part_of(a, R, r)];
    const int64_t p0 = pt.indptr[r];
    if (p0 < 0 || p0 + len > pt.capacity) continue;   // (k_stack_counts saw the same pair)
    for (int64_t i = lane; i < len; i += 64) {
      if (o + i >= a.capacity_out) break;
      a.indices_out[o + i] = pt.indices[p0 + i];
      if (a.data_out) a.data_out[o + i] = pt.data ? pt.data[p0 + i] : 1.f;
    }
  }
}

}  // namespace sdrm
