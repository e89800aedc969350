// Adam over the VAE pre-stage's parameter tensors in ONE launch, with the L2 term of its loss, and the step's loss value into a slot
// of the epoch's buffer (gfx950).  Reference lines are into the reference's train_SDRM.py: :126 torch.optim.Adam(lr), :143-150
// `loss = neg_ll + anneal * kl + model.get_l2_reg()`, `optimizer.step()`, and :262-268 get_l2_reg.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "elementwise.h"

namespace sdrm {

constexpr int VADAM_MAX_TENSORS = 16;   // tensors of one launch (more go out as successive launches)
constexpr int VADAM_CHUNK = 4096;       // elements of one work-group: 256 threads x four 16-byte accesses

// One caller-owned tensor: p, m, v updated in place, g read only; float32, contiguous, n elements each.
struct VAdamTensor {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  float wd2;              // adam_math's wd: 2 x the coefficient c of c * sum(p^2) in the loss (the gradient of that term, folded in); 0: none
  unsigned first_chunk;   // chunks of the tensors in front of this one in the launch
  int vector_ok;          // all four pointers are 16-byte aligned (the host's test): 16-byte accesses; else dwords
};
struct VAdamTable { VAdamTensor t[VADAM_MAX_TENSORS]; int n; };   // by value in the kernel arguments (904 bytes)

struct VAdamArgs {
  float step_size, bc2_sqrt, b1, b2, eps;   // adam_scalars' two and the caller's three
  double* l2_partials;                      // [chunks of the whole step] or null: nothing is summed
  unsigned chunk0;                          // chunks of the launches in front of this one (the slots of this launch start there)
};

__device__ __forceinline__ void vadam_element(const VAdamTensor& t, const VAdamArgs& a, int64_t i, bool l2, double& sq) {
  const float w = t.p[i];
  float mm = t.m[i], vv = t.v[i];
  if (l2) sq += (double)w * (double)w;   // (exact product: the sum is the same fused or not)
  t.p[i] = adam_math(w, t.g[i], mm, vv, a.step_size, a.bc2_sqrt, a.b1, a.b2, a.eps, t.wd2);
  t.m[i] = mm; t.v[i] = vv;
}

// ... of one 16-byte quad whose four values are in registers already
__device__ __forceinline__ void vadam_quad(const VAdamTensor& t, const VAdamArgs& a, int64_t base, int q, float4 P, float4 G, float4 M, float4 V,
                                           bool l2, double& sq) {
  float w[4] = {P.x, P.y, P.z, P.w}, mm[4] = {M.x, M.y, M.z, M.w}, vv[4] = {V.x, V.y, V.z, V.w};
  const float g[4] = {G.x, G.y, G.z, G.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (l2) sq += (double)w[j] * (double)w[j];
    w[j] = adam_math(w[j], g[j], mm[j], vv[j], a.step_size, a.bc2_sqrt, a.b1, a.b2, a.eps, t.wd2);
  }
  reinterpret_cast<float4*>(t.p + base)[q] = make_float4(w[0], w[1], w[2], w[3]);
  reinterpret_cast<float4*>(t.m + base)[q] = make_float4(mm[0], mm[1], mm[2], mm[3]);
  reinterpret_cast<float4*>(t.v + base)[q] = make_float4(vv[0], vv[1], vv[2], vv[3]);
}

// Work is dealt by chunk: work-group c of the launch owns elements [4096 k, 4096 k + 4096) of the tensor whose chunk range holds c
// (linear search over at most 16 prefix entries) - a bias of a few hundred elements costs one work-group, not a grid row.  Every
// access is inside [ptr, ptr + n): the 16-byte accesses cover whole quads below n, the last partial quad and a tensor off the 16-byte
// grid go by dwords; no load is made through a selected address (a whole chunk takes the unpredicated body, a partial one a loop).  With l2_partials given, slot chunk0 + c receives sum(w^2) of the chunk's weights BEFORE the update in float64
// (0 for a tensor without an L2 coefficient): per thread in element order, down the wave, then the four waves in order - written,
// not added, so the buffer needs no zeroing and the value is the same bits on every call.
__global__ __launch_bounds__(256) void k_vae_adam(const VAdamTable tab, const VAdamArgs a) {
  __shared__ double sh[4];
  const unsigned chunk = blockIdx.x;
  int k = 0;
  for (int i = 1; i < tab.n; ++i)
    if (tab.t[i].first_chunk <= chunk) k = i;
  const VAdamTensor& t = tab.t[k];
  const int64_t base = (int64_t)(chunk - t.first_chunk) * VADAM_CHUNK;
  const int64_t left = t.n - base;
  const int cnt = left < (int64_t)VADAM_CHUNK ? (int)left : VADAM_CHUNK;   // >= 1: the host sized the grid by the chunk counts
  const bool l2 = a.l2_partials != nullptr && t.wd2 > 0.f;
  double sq = 0.0;
  if (t.vector_ok) {
    const float4* p4 = reinterpret_cast<const float4*>(t.p + base);
    const float4* g4 = reinterpret_cast<const float4*>(t.g + base);
    const float4* m4 = reinterpret_cast<const float4*>(t.m + base);
    const float4* v4 = reinterpret_cast<const float4*>(t.v + base);
    if (cnt == VADAM_CHUNK) {   // a whole chunk (uniform): sixteen independent 16-byte loads, one round trip
      float4 P[4], G[4], M[4], V[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int q = (int)threadIdx.x + 256 * u;
        P[u] = p4[q]; G[u] = g4[q]; M[u] = m4[q]; V[u] = v4[q];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) vadam_quad(t, a, base, (int)threadIdx.x + 256 * u, P[u], G[u], M[u], V[u], l2, sq);
    } else {                    // a tensor's last chunk: its whole quads, then its last partial quad (at most three elements) by dwords
      const int nq = cnt >> 2;
      for (int q = (int)threadIdx.x; q < nq; q += 256) vadam_quad(t, a, base, q, p4[q], g4[q], m4[q], v4[q], l2, sq);
      const int i = 4 * nq + (int)threadIdx.x;
      if (i < cnt) vadam_element(t, a, base + i, l2, sq);
    }
  } else {
#pragma unroll 4
    for (int u = 0; u < VADAM_CHUNK / 256; ++u) {
      const int i = (int)threadIdx.x + 256 * u;
      if (i < cnt) vadam_element(t, a, base + i, l2, sq);
    }
  }
  if (a.l2_partials != nullptr) {   // (uniform over the work-group: block_sum has barriers)
    const double s = block_sum(sq, sh);
    if (threadIdx.x == 0) a.l2_partials[(size_t)a.chunk0 + chunk] = s;
  }
}

// out = (neg_ll + anneal * kl) + (float)(weight_decay * sum of the partials): torch's parenthesisation of `neg_ll + anneal * kl + l2`
// on float32 scalars, contraction off.  Without partials the last term is +0.0f, what `torch.zeros(())` adds.
__device__ __forceinline__ float vae_loss_value(float neg_ll, float kl, float anneal, float weight_decay, double l2_sum) {
#pragma clang fp contract(off)
  const float akl = anneal * kl;
  const float base = neg_ll + akl;
  const float l2 = (float)((double)weight_decay * l2_sum);
  return base + l2;
}

// ONE work-group: the partials in chunk order per thread (i, i + 256, ..), then block_sum's tree - the same bits on every call.
__global__ __launch_bounds__(256) void k_vae_loss_slot(const float* __restrict__ neg_ll, const float* __restrict__ kl, float anneal,
                                                       const double* __restrict__ l2_partials, int64_t n_partials, float weight_decay,
                                                       float* __restrict__ out) {
  __shared__ double sh[4];
  double s = 0.0;
  if (l2_partials != nullptr) {
    double v = 0.0;
    for (int64_t i = threadIdx.x; i < n_partials; i += 256) v += l2_partials[i];
    s = block_sum(v, sh);
  }
  if (threadIdx.x == 0) *out = vae_loss_value(*neg_ll, *kl, anneal, weight_decay, s);
}

}  // namespace sdrm
