// What every kernel that reads a batch of rows of the device-resident CSR feed shares (csrc/feed.h, encode.h, nll.h, input_layer.h):
// the batch descriptor, the feed status word's bits and their messages, the checked row span and entry load, and the chunked gather
// of the row-owned kernels.  A caller's CSR is never trusted with an address: what fails a check is skipped and raises a status bit.
// Where one of those kernels still spells a piece out, the helper moved its register counts or its gather loop: the list, with the
// figures, is profiles/csr_feed_refactor.txt.  A new kernel starts from the helpers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sdrm {

struct CsrBatch {
  const int64_t* indptr; const int32_t* indices; const float* data;   // CSR of the whole feed [n_rows, n_items] (data null: all ones)
  const int64_t* rows;     // [b] row ids of this batch (null: rows row0 .. row0+b-1)
  int64_t row0, n_rows; int b, n_items;
  unsigned* flag;          // the handle's feed status word (read and cleared by sdrm_feed_status)
};

// The bits of the feed status word, and what sdrm_feed_status says for each.
enum { FEED_BAD_ROW = 1u, FEED_BAD_COL = 2u, FEED_BAD_PTR = 4u, FEED_HOLD_PTR = 8u, FEED_HOLD_COL = 16u, FEED_T_DUP = 32u, FEED_STACK_PTR = 64u,
       FEED_STACK_COL = 128u };
struct FeedStatusText { unsigned bit; const char* text; };
constexpr FeedStatusText FEED_STATUS_TEXT[] = {
    {FEED_BAD_ROW, " a row id outside [0, n_rows) (its output row is zero);"},
    {FEED_BAD_PTR, " an indptr pair that is negative or not ordered (its output row is zero);"},
    {FEED_BAD_COL, " a column index outside [0, n_items) (that entry was skipped; sdrm_neumf_triples: the row is empty in the output);"},
    {FEED_HOLD_PTR, " sdrm_holdout_split: an indptr pair that is out of order, reaches outside [0, nnz] or spans more than n_items entries (the row is empty in both outputs);"},
    {FEED_HOLD_COL, " sdrm_holdout_split: a column index outside [0, n_items) (the row is empty in both outputs);"},
    {FEED_T_DUP, " sdrm_csr_transpose: a row that holds a column more than once (the output is not the transpose);"},
    {FEED_STACK_PTR, " sdrm_csr_vstack: an indptr pair that is out of order, reaches outside its part's arrays or spans more than n_cols entries (the row is empty in the output; sdrm_neumf_triples reports its rows here too, and triples dropped behind capacity_out);"},
    {FEED_STACK_COL, " sdrm_csr_vstack: a column index outside [0, n_cols) (the row is empty in the output);"},
};

// Feed row `src` and CSR stretch [p0, p1) of batch row r, range-checked: a row id outside the matrix or an indptr pair out of order
// leaves the empty stretch, and the thread with `owner` == 0 among those that own the row raises the status word.  (The index, not
// the compare: a flag worked out by the caller is evaluated ahead of the loads and moves the register counts of k_nll_*.)
// PTR_BIT: the bit a bad indptr pair raises (sdrm_neumf_triples reports its rows under sdrm_csr_vstack's bit).
struct CsrSpan { int64_t src, p0, p1; };
template <unsigned PTR_BIT = FEED_BAD_PTR>
__device__ __forceinline__ CsrSpan csr_row_span(const CsrBatch& c, int r, int owner) {
  CsrSpan s{c.rows ? c.rows[r] : c.row0 + r, 0, 0};
  if (s.src < 0 || s.src >= c.n_rows) {
    if (owner == 0) atomicOr(c.flag, (unsigned)FEED_BAD_ROW);
    return s;
  }
  const int64_t q0 = c.indptr[s.src], q1 = c.indptr[s.src + 1];
  if (q0 < 0 || q1 < q0) {
    if (owner == 0) atomicOr(c.flag, PTR_BIT);
    return s;
  }
  s.p0 = q0; s.p1 = q1;
  return s;
}

// Entry p, range-checked: false and `bad` set for a column outside [0, n_items) (the caller raises FEED_BAD_COL once, at its end),
// else its column and its value (1 where the matrix stores none).
__device__ __forceinline__ bool csr_entry(const CsrBatch& c, int64_t p, bool& bad, int32_t& col, float& val) {
  col = c.indices[p];
  if (col < 0 || col >= c.n_items) { bad = true; return false; }
  val = c.data ? c.data[p] : 1.f;
  return true;
}

// ---- the chunked gather of the row-owned kernels (k_encode_csr, k_input_fwd, k_input_wgrad) ----
// TPR threads own a row (a wave, or the work-group of 256) and NV float4 slices each of a vector of q slices.  The row's (index,
// value) pairs are parked in LDS a chunk of TPR at a time, padded with (0, +0.0f) to a multiple of U; every owner then walks the chunk
// with same-address LDS reads.

// The chunk is written: every owner may read it.
template <int TPR>
__device__ __forceinline__ void chunk_barrier() {
  if (TPR == 256) __syncthreads();
  else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
}

// This thread's slices slot, slot + TPR, ..; one behind the vector reads the last slice again (never stored): the loads stay branch-free.
template <int TPR, int NV>
__device__ __forceinline__ void gather_slices(int slot, int q, int (&sl)[NV]) {
#pragma unroll
  for (int v = 0; v < NV; ++v) sl[v] = slot + v * TPR < q ? slot + v * TPR : q - 1;
}

// acc += value x row `index` of base [..][stride] for the entries j .. j + U - 1 of the chunk, in that order: the U x NV 16-byte loads
// are issued before the FMAs that consume them.  The entries' values come back in `val`.
template <int NV, int U>
__device__ __forceinline__ void gather_fma(const int2* ent, int j, const float4* __restrict__ base, size_t stride, const int (&sl)[NV],
                                           float4 (&acc)[NV], float (&val)[U]) {
  float4 w[U][NV];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int2 e2 = ent[j + u];
    val[u] = __int_as_float(e2.y);
    const float4* row = base + (size_t)e2.x * stride;
#pragma unroll
    for (int v = 0; v < NV; ++v) w[u][v] = row[sl[v]];
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      acc[v].x = fmaf(val[u], w[u][v].x, acc[v].x);
      acc[v].y = fmaf(val[u], w[u][v].y, acc[v].y);
      acc[v].z = fmaf(val[u], w[u][v].z, acc[v].z);
      acc[v].w = fmaf(val[u], w[u][v].w, acc[v].w);
    }
  }
}

}  // namespace sdrm
