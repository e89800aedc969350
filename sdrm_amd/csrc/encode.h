// VAE encode on the engine: the frozen, eval-mode encode hook `VAE.encode` of the reference (train_SDRM.py:241-250 with is_training == 0
// and dropout off; encoder = Linear(n_items, hidden) -> Tanh -> Linear(hidden, 2 latent), :210-212):
//   z = mu = W2[:L] tanh(W1 x / max(|x|_2, 1e-12) + b1) + b2[:L],   kl = -0.5 mean_rows sum(1 + logvar - mu^2 - exp(logvar)).
// The second Linear is a launch of the MFMA GEMM of csrc/gemm.h.  The first one has two forms:
//   dense  x [n, n_items]: k_encode_norm_rows stages the L2-normalised, zero-padded rows and the GEMM does the rest;
//   CSR    k_encode_csr: W1 x is a sum of nnz columns of W1 (18 .. 550 of 1008 .. 8582 for the published configurations), gathered as
//          rows of the transposed copy W1^T [n_items][Hq] (Hq = hidden rounded up to 4), so that no dense batch ever exists.
// Plain HIP, vector / plain C++ stores only; no asm MFMA in here (tests/test_isa_lint.py has nothing to hold).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "gemm.h"

namespace sdrm {

// dst [n_items][Hq] = src [hidden][n_items]^T, columns hidden .. Hq-1 zero (32 x 32 tiles through LDS; block 32 x 8)
__global__ __launch_bounds__(256) void k_encode_w1t(const float* __restrict__ src, int hidden, int n_items, float* __restrict__ dst, int Hq) {
  __shared__ float tile[32][33];
  const int i0 = blockIdx.x * 32, h0 = blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int h = h0 + k, i = i0 + tx;
    tile[k][tx] = (h < hidden && i < n_items) ? src[(size_t)h * n_items + i] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int i = i0 + k, h = h0 + tx;
    if (i < n_items && h < Hq) dst[(size_t)i * Hq + h] = tile[tx][k];
  }
}

// sum over the 256 threads of a work-group in a fixed order (a tree over LDS), returned to every thread
template <class T>
__device__ __forceinline__ T encode_block_sum(T v, T* red) {
  const int t = threadIdx.x;
  __syncthreads();   // `red` may still be read from a previous call
  red[t] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s) red[t] += red[t + s];
    __syncthreads();
  }
  return red[0];
}

// Dense form, staging: dst [row][0 .. Ip) = x[row] / max(|x[row]|_2, 1e-12) (F.normalize, train_SDRM.py:242), columns n_items .. Ip-1 zero.
// One work-group per row; the row is read twice (the second time from L2).
__global__ __launch_bounds__(256) void k_encode_norm_rows(const float* __restrict__ x, int n_items, float* __restrict__ dst, int Ip) {
  __shared__ float red[256];
  const float* src = x + (size_t)blockIdx.x * n_items;
  float* out = dst + (size_t)blockIdx.x * Ip;
  float ss = 0.f;
  for (int c = threadIdx.x; c < n_items; c += 256) { const float v = src[c]; ss = fmaf(v, v, ss); }
  ss = encode_block_sum(ss, red);
  const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  for (int c = 4 * threadIdx.x; c < Ip; c += 1024) {
    float4 v;
    v.x = c < n_items ? src[c] * inv : 0.f;
    v.y = c + 1 < n_items ? src[c + 1] * inv : 0.f;
    v.z = c + 2 < n_items ? src[c + 2] * inv : 0.f;
    v.w = c + 3 < n_items ? src[c + 3] * inv : 0.f;
    *reinterpret_cast<float4*>(out + c) = v;
  }
}

struct EncodeCsrArgs {
  CsrBatch csr;
  const float* w1t;        // W1^T [n_items][Hq]
  const float* b1;         // [>= Hq], zero behind hidden
  int Hq, Hp;              // hidden rounded up to 4 / to the GEMM's 32
  float* hid;              // [>= b][Hp] hidden activations, the second-layer GEMM's operand
  int64_t nnz;             // entries of csr.indices; looked at by the CHECKED form alone (k_encode_csr_checked, csrc/eval_half.h)
};

// First Linear + normalise + tanh by gather.  TPR threads own one batch row (a work-group of 256: one row, or one row per wave for a narrow
// hidden layer); a thread owns the float4 slices slot, slot + TPR, .. of the hidden vector (NV of them) in registers.  The row's (column,
// value) pairs come in chunks of TPR, loaded coalesced, range-checked and parked in LDS; every thread then walks the chunk with same-address
// LDS reads, U entries at a time: the U x NV 16-byte loads of W1^T rows are issued before the FMAs that consume them.  Every thread adds the
// entries in CSR order, so a row's result is a function of that row alone (bit-reproducible, wherever the row sits in the batch).  An entry
// with a column outside [0, n_items) becomes (column 0, value 0): no stray load, and it adds +0.  sum(value^2) runs alongside in every thread.
// CHECKED == false is k_encode_csr as it always was: the upper end of an indptr pair is the caller's (the feed entry points are given
// no nnz).  CHECKED == true also holds it against a.nnz: a pair that reaches behind the index array is the empty row and raises FEED_BAD_PTR.
// ACT is what follows the sum: ENC_ACT_NORM_TANH is the encoder's tanh(sum / max(|x|_2, 1e-12) + b1); ENC_ACT_RELU is relu(sum + b1) with no
// scaling (the MLP evaluator's first layer from its folded rows, csrc/mlp_eval.h: sum(value^2) is then dead code).
enum : int { ENC_ACT_NORM_TANH = 0, ENC_ACT_RELU = 1 };
template <int TPR, int NV, int U, bool CHECKED, int ACT = ENC_ACT_NORM_TANH>
__device__ __forceinline__ void encode_csr_rows(const EncodeCsrArgs& a) {
  constexpr int RPW = 256 / TPR;   // rows per work-group
  __shared__ int2 ent[RPW][TPR];
  const int g = threadIdx.x / TPR, slot = threadIdx.x % TPR;
  const int r = blockIdx.x * RPW + g;
  const bool row_ok = r < a.csr.b;     // (uniform over the TPR threads of a row; with TPR == 256 over the work-group, so the barriers below are too)
  const int q = a.Hq >> 2;
  const CsrSpan s = row_ok ? csr_row_span(a.csr, r, slot) : CsrSpan{0, 0, 0};
  int64_t p0 = s.p0, p1 = s.p1;
  if (CHECKED && p1 > a.nnz) {
    if (slot == 0) atomicOr(a.csr.flag, (unsigned)FEED_BAD_PTR);
    p0 = p1 = 0;
  }
  float4 acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = make_float4(0.f, 0.f, 0.f, 0.f);
  float ss = 0.f;
  bool bad = false;
  const float4* __restrict__ wt = reinterpret_cast<const float4*>(a.w1t);
  int sl[NV];   // this thread's slices; one behind the hidden vector reads the last slice again (never stored): the loads stay branch-free
#pragma unroll
  for (int v = 0; v < NV; ++v) sl[v] = slot + v * TPR < q ? slot + v * TPR : q - 1;
  for (int64_t p = p0; p < p1; p += TPR) {
    const int cnt = (int)((p1 - p) < (int64_t)TPR ? (p1 - p) : (int64_t)TPR);
    if (TPR == 256) __syncthreads(); else __builtin_amdgcn_wave_barrier();   // the previous chunk has been read
    {
      int2 e2 = make_int2(0, 0);   // (column 0, value +0.0f): what pads the chunk to a multiple of U
      if (slot < cnt) {
        const int32_t c = a.csr.indices[p + slot];
        if (c < 0 || c >= a.csr.n_items) bad = true;
        else e2 = make_int2(c, __float_as_int(a.csr.data ? a.csr.data[p + slot] : 1.f));
      }
      ent[g][slot] = e2;
    }
    chunk_barrier<TPR>();
    for (int j = 0; j < cnt; j += U) {   // (TPR is a multiple of U: j + u stays inside the chunk's LDS row, padded with zero-valued entries)
      float val[U];
      gather_fma<NV, U>(ent[g], j, wt, (size_t)q, sl, acc, val);
#pragma unroll
      for (int u = 0; u < U; ++u) ss = fmaf(val[u], val[u], ss);
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  if (!row_ok) return;
  const float inv = 1.f / fmaxf(sqrtf(ss), 1e-12f);
  float4* out = reinterpret_cast<float4*>(a.hid + (size_t)r * a.Hp);
  const float4* b4 = reinterpret_cast<const float4*>(a.b1);
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int s = slot + v * TPR;
    if (s < q) {
      const float4 b = b4[s];
      if constexpr (ACT == ENC_ACT_RELU)
        out[s] = make_float4(fmaxf(acc[v].x + b.x, 0.f), fmaxf(acc[v].y + b.y, 0.f), fmaxf(acc[v].z + b.z, 0.f), fmaxf(acc[v].w + b.w, 0.f));
      else
        out[s] = make_float4(tanh_fast(fmaf(acc[v].x, inv, b.x)), tanh_fast(fmaf(acc[v].y, inv, b.y)), tanh_fast(fmaf(acc[v].z, inv, b.z)),
                             tanh_fast(fmaf(acc[v].w, inv, b.w)));
    }
  }
  for (int s = q + slot; s < (a.Hp >> 2); s += TPR) out[s] = make_float4(0.f, 0.f, 0.f, 0.f);   // the GEMM's K padding
}

template <int TPR, int NV, int U>
__global__ __launch_bounds__(256) void k_encode_csr(const EncodeCsrArgs a) { encode_csr_rows<TPR, NV, U, false>(a); }

// kl, first launch: block k takes rows k, k + gridDim.x, ..: copies mu = out2[row][0 .. L) to z[row] and leaves its share of
// sum(1 + logvar - mu^2 - exp(logvar)) in part[k] (float64; every thread in a fixed order, then the tree).  1 - exp(lv) is taken as
// -expm1(lv): the terms are O(lv^2) and the plain form cancels.
__global__ __launch_bounds__(256) void k_encode_kl_rows(const float* __restrict__ out2, int n, int L, float* __restrict__ z, double* __restrict__ part) {
  __shared__ double red[256];
  double s = 0.0;
  for (int r = blockIdx.x; r < n; r += gridDim.x) {
    const float* o = out2 + (size_t)r * 2 * L;
    for (int c = threadIdx.x; c < L; c += 256) {
      const float mu = o[c], lv = o[L + c];
      z[(size_t)r * L + c] = mu;
      s += (double)((lv - expm1f(lv)) - mu * mu);
    }
  }
  s = encode_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = s;
}

// kl, second launch (one work-group): the partials in block order, kl = -0.5 sum / n.  (A ticket in the last block of the first launch
// instead costs fences and a serial tail: csrc/elementwise.h measured that for the loss sums.)
__global__ __launch_bounds__(256) void k_encode_kl_sum(const double* __restrict__ part, int parts, int n, float* __restrict__ kl) {
  __shared__ double red[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < parts; k += 256) s += part[k];
  s = encode_block_sum(s, red);
  if (threadIdx.x == 0) *kl = (float)(-0.5 * s / (double)n);
}

}  // namespace sdrm
