// Recall@k / NDCG@k of a score matrix against held-out interactions, on the device (SURVEY.md §8f-3;
// utilities.py:116-171: mask_training_examples, recall_at_k_batch, NDCG_binary_at_k_batch).
//
// The reference partitions every row for its top-k (bn.argpartition) and then looks the held-out items up in it.
// Only the held-out items matter, and there are few of them per user, so no top-k is built here: one work-group
// per user keeps the user's score row in LDS (already-seen items set to -inf, utilities.py:118-119) and computes
// for every held-out item j its rank = #{i : s_i > s_j} + #{i < j : s_i == s_j} (ties towards the lower index;
// argpartition leaves them unspecified).  rank < k  <=>  the item is in the top-k, and its DCG discount is
// tp[rank].  One pass serves every k of the list.  HBM-bound: the score matrix is read once.
//
// Bit-exactness with numpy: hits are small integers (exact in float32 as the reference holds them); recall is
// hits / min(k, n_true) in float64; DCG is the row sum of a length-k float64 vector, summed exactly the way
// numpy's pairwise add-reduce does (8 strided accumulators), with the discount table tp and the ideal-DCG table
// computed by the caller with numpy and passed in.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"

namespace sdrm {

constexpr int RANK_MAX_K = 128;   // numpy's pairwise block: one level, no recursion
constexpr int RANK_MAX_NK = 8;

struct RankArgs {
  const float* scores; int U, I;
  const int64_t* held_indptr; const int32_t* held_indices;
  const int64_t* train_indptr; const int32_t* train_indices;   // may be null (no masking)
  int ks[RANK_MAX_NK]; int nk, kmax;
  const double* tp;     // [kmax]   1 / log2(r + 2)
  const double* idcg;   // [kmax+1] sum(tp[:m]) as numpy sums it
  double* recall;       // [nk][U]
  double* ndcg;         // [nk][U]
};

// numpy's pairwise_sum for n <= 128 (numpy/_core/src/umath/loops_utils.h.src)
__device__ inline double np_pairwise_sum(const double* a, int n) {
  if (n < 8) {
    double res = 0.;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  double r[8];
  for (int j = 0; j < 8; ++j) r[j] = a[j];
  int i = 8;
  for (; i < n - (n % 8); i += 8)
    for (int j = 0; j < 8; ++j) r[j] += a[i + j];
  double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
  for (; i < n; ++i) res += a[i];
  return res;
}

// What the CHECKED form (k_rank_metrics_checked, csrc/eval_half.h) knows beside RankArgs: the capacities of the two index arrays and
// the feed status word (csrc/csr_batch.h).  It trusts no offset and no column: an indptr pair that is out of order or reaches outside
// [0, nnz] is an empty row, an entry with a column outside [0, I) is skipped (a held one does not count as held), and either raises
// FEED_BAD_PTR / FEED_BAD_COL.  It writes the metrics whose pointer is not null.
struct RankCheck { int64_t held_nnz, train_nnz; unsigned* flag; };

// What the row-mapped form (k_rank_metrics_rows, csrc/neumf_rank.h) knows beside both: score row q ranks against CSR row rows[q] of both
// matrices [n_rows, I] (an id outside [0, n_rows) is an empty row and raises FEED_BAD_ROW), and whether the NDCG goes on the NeuMF footing.
struct RankRows { const int32_t* rows; int64_t n_rows; int full_idcg; };

// One work-group, one user.  CHECKED == false is k_rank_metrics as it always was: `ck` is not looked at.
// ROWMAP: the CSR row of score row q is rm.rows[q], not q.  FOOTING: with rm.full_idcg the NDCG is put on the footing of
// neural_cf_benchmark_pt.py's testing block (sdrm_amd/neumf.py: host_metrics), whose held-out matrix stores every pair of the cartesian
// product - the ideal DCG counts min(I, k) items for every user, and a user without a relevant item has NDCG 0 - by the three float64
// operations `rank_all_items` makes on the host, in its order: t = dcg / idcg[m]; t * idcg[m] / idcg[min(I, k)].  Recall is untouched.
template <bool CHECKED, bool ROWMAP = false, bool FOOTING = false>
__device__ __forceinline__ void rank_metrics_user(const RankArgs& a, const RankCheck& ck, const RankRows& rm = RankRows{}) {
  extern __shared__ float row[];            // [I] scores of this user, then the reduction scratch
  __shared__ int red[4];
  __shared__ double vec[RANK_MAX_K];        // hit * discount by rank
  __shared__ unsigned char hit[RANK_MAX_K];
  const int u = blockIdx.x, tid = threadIdx.x;
  const float* src = a.scores + (size_t)u * a.I;
  for (int i = tid; i < a.I; i += 256) row[i] = src[i];
  for (int r = tid; r < RANK_MAX_K; r += 256) hit[r] = 0;
  __syncthreads();
  unsigned bad = 0;
  int64_t cr = u;                           // the CSR row of both matrices; -1: none (an empty row)
  if (ROWMAP) {
    cr = rm.rows[u];
    if (cr < 0 || cr >= rm.n_rows) { bad |= (unsigned)FEED_BAD_ROW; cr = -1; }
  }
  if (a.train_indptr) {
    int64_t t0 = 0, t1 = 0;
    if (!ROWMAP || cr >= 0) { t0 = a.train_indptr[cr]; t1 = a.train_indptr[cr + 1]; }
    if (CHECKED && (t0 < 0 || t1 < t0 || t1 > ck.train_nnz)) { bad |= (unsigned)FEED_BAD_PTR; t0 = t1 = 0; }
    for (int64_t t = t0 + tid; t < t1; t += 256) {
      const int c = a.train_indices[t];
      if (CHECKED && (c < 0 || c >= a.I)) { bad |= (unsigned)FEED_BAD_COL; continue; }
      row[c] = -INFINITY;
    }
    __syncthreads();
  }
  int64_t h0 = 0, h1 = 0;
  if (!ROWMAP || cr >= 0) { h0 = a.held_indptr[cr]; h1 = a.held_indptr[cr + 1]; }
  if (CHECKED && (h0 < 0 || h1 < h0 || h1 > ck.held_nnz)) { bad |= (unsigned)FEED_BAD_PTR; h0 = h1 = 0; }
  int n_true = (int)(h1 - h0);
  for (int64_t h = h0; h < h1; ++h) {
    const int j = a.held_indices[h];
    if (CHECKED && (j < 0 || j >= a.I)) { bad |= (unsigned)FEED_BAD_COL; --n_true; continue; }   // (uniform over the work-group: every thread reads entry h)
    const float v = row[j];
    int c = 0;
    for (int i = tid; i < a.I; i += 256) {
      const float s = row[i];
      c += (s > v) || (s == v && i < j);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off, 64);
    if ((tid & 63) == 0) red[tid >> 6] = c;
    __syncthreads();
    if (tid == 0) {
      const int rank = red[0] + red[1] + red[2] + red[3];
      if (rank < a.kmax) hit[rank] = 1;
    }
    __syncthreads();
  }
  if (tid == 0) {
    for (int q = 0; q < a.nk; ++q) {
      const int k = a.ks[q];
      int hits = 0;
      for (int r = 0; r < k; ++r) {
        vec[r] = hit[r] ? a.tp[r] : 0.0;
        hits += hit[r];
      }
      const double dcg = np_pairwise_sum(vec, k);
      const int m = n_true < k ? n_true : k;
      if (!CHECKED || a.recall) a.recall[(size_t)q * a.U + u] = (double)hits / (double)m;          // 0/0 -> nan, like the reference
      double nd = dcg / a.idcg[m];                                                                 // idcg[0] = 0 -> nan
      if (FOOTING && rm.full_idcg) nd = n_true > 0 ? nd * a.idcg[m] / a.idcg[a.I < k ? a.I : k] : 0.0;
      if (!CHECKED || a.ndcg) a.ndcg[(size_t)q * a.U + u] = nd;
    }
  }
  if (CHECKED && bad) atomicOr(ck.flag, bad);
}

__global__ __launch_bounds__(256) void k_rank_metrics(const RankArgs a) { rank_metrics_user<false>(a, RankCheck{}); }

}  // namespace sdrm
