// Loss head of the MultiVAE++ pre-stage on the engine: the multinomial negative log-likelihood of the decoder's logits against
// the batch's CSR rows and its gradient with respect to the logits (reference train_SDRM.py:141-142,
//   neg_ll = -torch.mean(torch.sum(F.log_softmax(out, dim=1) * X, dim=1))  and what autograd makes of it):
//   lse[r]  = log sum_i exp(o[r,i])
//   loss    = -(1/b) sum_r sum_{p in CSR row} x_p (o[r, col_p] - lse[r])
//   g[r,i]  = scale (exp(o[r,i] - lse[r]) s_r - x[r,i]) / b,   s_r = sum_p x_p.
// No dense X exists: the forward reads the logits once (and the row's nnz of them again, out of L2, for the terms), the gradient
// reads them once and writes g once; 12 B per element for the pair.  One work-group of 256 per batch row, rows streamed: a row
// never has to fit LDS.  Plain HIP, vector / plain C++ stores only, no floating-point atomic.
// A row's lse and gradient are functions of that row's logits, its CSR row, b and scale alone: the forward maps column c to
// thread c % 256 with scalar loads whatever the row's alignment is (a peeled head would move columns between threads with the
// row's place in the batch, and the sums with them); the gradient is elementwise, so it peels to 16-byte loads and stores.
// Non-finite logits are outside the contract (the running maximum starts at -FLT_MAX, and inf - inf is not handled).
#pragma once
#include <float.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode.h"

namespace sdrm {

struct NllArgs {
  const float* logits;     // [b, n_items], base 16-byte aligned
  CsrBatch csr;
};

// Forward.  Block k takes rows k, k + gridDim.x, ..  Per row: every thread keeps a running (max, sum of exp(o - max)) over its
// columns c = t, t + 256, .. (four loads in flight, one rescale per four), a fixed tree over LDS joins the 256 pairs, and
// lse = max + log(sum).  Then the row's CSR entries: x_p (o[col_p] - lse) in fp32, summed in float64 per thread in entry order.
// The block's float64 share of sum_r term_r goes to part[k] (the tree of csrc/encode.h); k_nll_sum adds the parts in block order.
__global__ __launch_bounds__(256) void k_nll_rows(const NllArgs a, float* __restrict__ lse, double* __restrict__ part) {
  __shared__ float red_m[256], red_s[256];
  __shared__ double red_d[256];
  const int t = threadIdx.x;
  double acc = 0.0;
  bool bad = false;
  for (int r = blockIdx.x; r < a.csr.b; r += gridDim.x) {
    const float* __restrict__ o = a.logits + (size_t)r * a.csr.n_items;
    float m = -FLT_MAX, s = 0.f;
    int c = t;
    for (; c + 768 < a.csr.n_items; c += 1024) {
      const float v0 = o[c], v1 = o[c + 256], v2 = o[c + 512], v3 = o[c + 768];
      const float mn = fmaxf(m, fmaxf(fmaxf(v0, v1), fmaxf(v2, v3)));
      s = s * expf(m - mn) + ((expf(v0 - mn) + expf(v1 - mn)) + (expf(v2 - mn) + expf(v3 - mn)));
      m = mn;
    }
    for (; c < a.csr.n_items; c += 256) {
      const float v = o[c];
      const float mn = fmaxf(m, v);
      s = s * expf(m - mn) + expf(v - mn);
      m = mn;
    }
    __syncthreads();   // the previous row's tree has been read
    red_m[t] = m; red_s[t] = s;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
      if (t < st) {   // a thread without a column holds (-FLT_MAX, 0): exp(-FLT_MAX - max) = 0, and 0 x exp(0) = 0 between two of them
        const float ma = red_m[t], mb = red_m[t + st];
        const float mn = fmaxf(ma, mb);
        red_s[t] = red_s[t] * expf(ma - mn) + red_s[t + st] * expf(mb - mn);
        red_m[t] = mn;
      }
      __syncthreads();
    }
    const float l = red_m[0] + logf(red_s[0]);
    if (t == 0) lse[r] = l;
    const CsrSpan sp = csr_row_span(a.csr, r, t);   // (uniform over the work-group: no barrier is skipped)
    const int64_t p0 = sp.p0, p1 = sp.p1;
    for (int64_t p = p0 + t; p < p1; p += 256) {
      const int32_t col = a.csr.indices[p];
      if (col < 0 || col >= a.csr.n_items) bad = true;
      else acc += (double)((a.csr.data ? a.csr.data[p] : 1.f) * (o[col] - l));
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
  acc = encode_block_sum(acc, red_d);
  if (t == 0) part[blockIdx.x] = acc;
}

// the parts in block order (one work-group): loss = -sum / b
__global__ __launch_bounds__(256) void k_nll_sum(const double* __restrict__ part, int parts, int b, float* __restrict__ loss) {
  __shared__ double red[256];
  double s = 0.0;
  for (int k = threadIdx.x; k < parts; k += 256) s += part[k];
  s = encode_block_sum(s, red);
  if (threadIdx.x == 0) *loss = (float)(-s / (double)b);
}

// one element of the softmax part of the gradient: k exp(o - lse) s_r with k = scale / b
__device__ __forceinline__ float nll_soft(float v, float l, float sr, float k) { return k * (expf(v - l) * sr); }

// Gradient.  Block k takes rows k, k + gridDim.x, ..  Per row: s_r over the row's valid entries (float64, the tree), then the
// full-width pass g[i] = k exp(o[i] - lse) s_r - every element is read by the thread that then writes it, so g may be the logits
// buffer itself - a barrier, and the row's entries take their k x_p off g[col_p].  The barrier orders those read-modify-writes
// behind the same work-group's full-width stores.  `g` and `logits` are not __restrict__: they may be one buffer.
__global__ __launch_bounds__(256) void k_nll_grad(const NllArgs a, const float* __restrict__ lse, const float* __restrict__ scale, float* g) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const float k = (scale ? *scale : 1.f) / (float)a.csr.b;
  bool bad = false;
  for (int r = blockIdx.x; r < a.csr.b; r += gridDim.x) {
    const CsrSpan sp = csr_row_span(a.csr, r, t);   // (uniform over the work-group: no barrier is skipped)
    const int64_t p0 = sp.p0, p1 = sp.p1;
    double sd = 0.0;
    for (int64_t p = p0 + t; p < p1; p += 256) {
      const int32_t col = a.csr.indices[p];
      if (col < 0 || col >= a.csr.n_items) bad = true;
      else sd += (double)(a.csr.data ? a.csr.data[p] : 1.f);
    }
    const float sr = (float)encode_block_sum(sd, red);
    const float l = lse[r];
    const float* o = a.logits + (size_t)r * a.csr.n_items;
    float* d = g + (size_t)r * a.csr.n_items;
    // both bases are 16-byte aligned, so the two rows share one misalignment: peel to a 16-byte boundary
    const int head = (int)(((16 - ((uintptr_t)d & 15)) & 15) >> 2);
    const int h = head < a.csr.n_items ? head : a.csr.n_items;
    if (t < h) d[t] = nll_soft(o[t], l, sr, k);
    const int nv = (a.csr.n_items - h) >> 2;
    const float4* o4 = reinterpret_cast<const float4*>(o + h);
    float4* d4 = reinterpret_cast<float4*>(d + h);
    for (int i = t; i < nv; i += 512) {   // two loads in flight (the compiler may not move a load over a store: the buffers may alias)
      const bool two = i + 256 < nv;
      const float4 v = o4[i];
      const float4 w = two ? o4[i + 256] : make_float4(0.f, 0.f, 0.f, 0.f);
      d4[i] = make_float4(nll_soft(v.x, l, sr, k), nll_soft(v.y, l, sr, k), nll_soft(v.z, l, sr, k), nll_soft(v.w, l, sr, k));
      if (two) d4[i + 256] = make_float4(nll_soft(w.x, l, sr, k), nll_soft(w.y, l, sr, k), nll_soft(w.z, l, sr, k), nll_soft(w.w, l, sr, k));
    }
    for (int i = h + 4 * nv + t; i < a.csr.n_items; i += 256) d[i] = nll_soft(o[i], l, sr, k);
    __syncthreads();   // the entries below land on this work-group's own stores above (same row)
    for (int64_t p = p0 + t; p < p1; p += 256) {
      const int32_t col = a.csr.indices[p];
      if (col >= 0 && col < a.csr.n_items) d[col] = d[col] - k * (a.csr.data ? a.csr.data[p] : 1.f);
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
}

}  // namespace sdrm
