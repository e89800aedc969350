// The VAE decoder and the multinomial loss head in TRAIN mode, forward and backward (reference train_SDRM.py:252-254 `decode`,
// :141-142 the loss, and their share of :148), for the batch's interaction rows given as CSR rows of the device-resident feed:
//   h3 = tanh(z W3^T + b3)              logits = h3 W4^T + b4              lse[r] = log sum_i exp(logits[r, i])
//   loss = -(1/b) sum_r sum_p x_p (logits[r, col_p] - lse[r])
//   g = scale (exp(logits - lse) s_r - X) / b          s_r = sum_p x_p
//   dW4 = g^T h3    db4 = column sums of g    dpre3 = (g W4)(1 - h3^2)    dW3 = dpre3^T z    db3 = column sums of dpre3    dz = dpre3 W3
// The four Linears' products are launches of the MFMA GEMM of csrc/gemm.h on zero-padded operands, the forward's staging is k_pad2d
// (csrc/decode.h) and its loss is k_nll_rows / k_nll_sum (csrc/nll.h) on the caller's logits; what is here is the forward's copy of
// the padded h3 into the caller's tensor, the backward's staging (both weights transposed through LDS for the NT dgrads, h3 and z
// padded), the loss gradient on the padded row stride of the GEMMs' operand, and the unpadding of both weight gradients' slabs and
// bias sums.
// Launches: 6 forward (staging of z and the weights, GEMM + tanh, h3 unpadded, GEMM + bias, loss rows, loss sum), 7 backward
// (staging, loss gradient, weight-gradient GEMM of W4, dgrad GEMM through the tanh, weight-gradient GEMM of W3, dgrad GEMM to z,
// unpadding) - 6 when the caller wants no dz.  (A GEMM whose grid would leave the exact range of gemm.h's tile arithmetic goes out in
// bands, one launch each; no batch of the pre-stage comes near that.)
// PADDING IS WRITTEN, NEVER INHERITED: the scratch is grow-only and shared by calls of any batch size, so every operand of a reduction
// over the batch has its rows behind b and its columns behind the valid width written by a kernel of the same call - zeros stored by
// the kernels here, or products of those zeros computed by the dgrad GEMM (dpre3).
// Every kernel takes 16-byte accesses when the widths and the caller's pointers allow and a scalar path with the same arithmetic
// otherwise.  Plain HIP, vector / plain C++ stores only; no floating-point atomic: a result is a function of its inputs alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "encode.h"
#include "latent.h"
#include "nll.h"

namespace sdrm {

// ---- forward: h3p [MP][Hp], as the first GEMM's tanh epilogue left it, into the caller's h3 [b][H] ---------------------------------------
// (The forward's second GEMM reads h3p itself: its rows behind b hold tanh(b3) and reach only output rows that the bounds-checked
// epilogue drops.  The backward stages its own h3p from the caller's h3, zero behind b rows.)
struct DecH3Args { const float* h3p; float* h3; int b, H, Hp; };

__global__ __launch_bounds__(256) void k_dechead_h3(const DecH3Args a) {
  const int qpr = (a.H + 3) >> 2;
  const int64_t total = (int64_t)a.b * qpr;
  const bool vec = (a.H & 3) == 0 && latent_al16(a.h3);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / qpr), c = 4 * (int)(i - (int64_t)r * qpr);
    const float4 v = *reinterpret_cast<const float4*>(a.h3p + (size_t)r * a.Hp + c);   // (Hp is a multiple of 32: aligned, c + 3 < Hp)
    latent_store4(a.h3 + (size_t)r * a.H, c, a.H, vec, v);
  }
}

// ---- backward, staging: ONE launch ------------------------------------------------------------------------------------------------
// Work-groups [0, t4): 32 x 32 tiles of W4 [I][H] -> w4t [Hr][Ip]; [t4, t4 + t3): of W3 [H][L] -> w3t [Lr][Hp] (the NT dgrads' B
// operands, zero behind the source's rows / columns); the others copy h3 [b][H] -> h3p [MP][Hp] and z [b][L] -> zp [MP][Lp],
// zero-padded (the weight gradients' B operands, h3p also the dgrad epilogue's aux), and write the zero bias zb [Lr] of the last dgrad.
struct DecTranspose {
  const float* src; float* dst;   // src [R][C] -> dst [Cr][Rp], Cr and Rp multiples of 32
  int R, C, Rp;
  int tiles_r;                    // Rp / 32: tiles along the destination's columns
};
struct DecStageBwdArgs {
  DecTranspose t4, t3;
  int64_t tiles4, tiles;          // tiles of W4, tiles of both
  const float* h3; float* h3p; int b, H, MP, Hp;
  const float* z; float* zp; int L, Lp;
  float* zb; int Lr;
};

__device__ __forceinline__ void dec_transpose_tile(const DecTranspose& t, int64_t tile, float (&lds)[32][33]) {
  const int64_t tc = tile / t.tiles_r;
  const int c0 = (int)tc * 32, r0 = (int)(tile - tc * t.tiles_r) * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int r = r0 + k, c = c0 + tx;
    lds[k][tx] = (r < t.R && c < t.C) ? t.src[(size_t)r * t.C + c] : 0.f;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) t.dst[(size_t)(c0 + k) * t.Rp + r0 + tx] = lds[tx][k];   // (c0 + k < Cr, r0 + tx < Rp: whole tiles)
}

__global__ __launch_bounds__(256) void k_dechead_stage_bwd(const DecStageBwdArgs a) {
  __shared__ float lds[32][33];
  const int64_t blk = blockIdx.x;
  if (blk < a.tiles4) { dec_transpose_tile(a.t4, blk, lds); return; }
  if (blk < a.tiles) { dec_transpose_tile(a.t3, blk - a.tiles4, lds); return; }
  const int qh = a.Hp >> 2, ql = a.Lp >> 2;
  const int64_t nh = (int64_t)a.MP * qh, nz = (int64_t)a.MP * ql, total = nh + nz + (a.Lr >> 2);
  const bool vec_h = (a.H & 3) == 0 && latent_al16(a.h3), vec_z = (a.L & 3) == 0 && latent_al16(a.z);
  const int64_t nthreads = ((int64_t)gridDim.x - a.tiles) * blockDim.x;
  for (int64_t i = (blk - a.tiles) * blockDim.x + threadIdx.x; i < total; i += nthreads) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < nh) {
      const int r = (int)(i / qh), c = 4 * (int)(i - (int64_t)r * qh);
      if (r < a.b && c < a.H) v = latent_load4(a.h3 + (size_t)r * a.H, c, a.H, vec_h);
      *reinterpret_cast<float4*>(a.h3p + (size_t)r * a.Hp + c) = v;
    } else if (i < nh + nz) {
      const int64_t j = i - nh;
      const int r = (int)(j / ql), c = 4 * (int)(j - (int64_t)r * ql);
      if (r < a.b && c < a.L) v = latent_load4(a.z + (size_t)r * a.L, c, a.L, vec_z);
      *reinterpret_cast<float4*>(a.zp + (size_t)r * a.Lp + c) = v;
    } else {
      *reinterpret_cast<float4*>(a.zb + 4 * (i - nh - nz)) = v;
    }
  }
}

// ---- backward: the loss gradient g into the padded operand [MP][Ip] of the weight gradient and the dgrad ---------------------------
// Block k takes rows k, k + gridDim.x, .. of ALL MP rows: a row behind b is written as zeros.  Per batch row: s_r over the row's valid
// entries (float64, the tree; k_nll_grad's order), then one pass over the Ip / 4 column quads - g[i] = k exp(o[i] - lse) s_r for i < I
// (exactly I columns: the softmax never sees the stride), zero behind - a barrier, and the row's entries take their k x_p off
// g[col_p].  The logits' rows have the stride I (a 16-byte load where I is a multiple of four, four scalar loads otherwise); g's rows
// are 16-byte aligned whatever I is.  A row id out of range has the empty stretch: s_r = 0 and the row is all zeros.
struct DecGradArgs {
  const float* logits;     // [b][I], base 16-byte aligned
  const float* lse;        // [b]
  const float* scale;      // one device float or null (= 1)
  CsrBatch csr;
  float* g;                // [MP][Ip]
  int MP, Ip;
};

__global__ __launch_bounds__(256) void k_dechead_grad(const DecGradArgs a) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  const int I = a.csr.n_items, nq = a.Ip >> 2;
  const float k = (a.scale ? *a.scale : 1.f) / (float)a.csr.b;
  const bool vec = (I & 3) == 0;
  bool bad = false;
  for (int r = blockIdx.x; r < a.MP; r += gridDim.x) {
    float4* d4 = reinterpret_cast<float4*>(a.g + (size_t)r * a.Ip);   // (not __restrict__: the entries below read what it stored)
    if (r >= a.csr.b) {   // (uniform over the work-group)
      for (int q = t; q < nq; q += 256) d4[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const CsrSpan sp = csr_row_span(a.csr, r, t);   // (uniform over the work-group: no barrier is skipped)
    const int64_t p0 = sp.p0, p1 = sp.p1;
    double sd = 0.0;
    for (int64_t p = p0 + t; p < p1; p += 256) {
      int32_t col; float val;
      if (csr_entry(a.csr, p, bad, col, val)) sd += (double)val;
    }
    const float sr = (float)encode_block_sum(sd, red);
    const float l = a.lse[r];
    const float* __restrict__ o = a.logits + (size_t)r * I;
    for (int q = t; q < nq; q += 256) {
      const int c = 4 * q;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (c < I) {
        const float4 x = latent_load4(o, c, I, vec);
        v.x = nll_soft(x.x, l, sr, k);
        if (c + 1 < I) v.y = nll_soft(x.y, l, sr, k);
        if (c + 2 < I) v.z = nll_soft(x.z, l, sr, k);
        if (c + 3 < I) v.w = nll_soft(x.w, l, sr, k);
      }
      d4[q] = v;
    }
    __syncthreads();   // the entries below land on this work-group's own stores above (same row)
    float* d = a.g + (size_t)r * a.Ip;
    for (int64_t p = p0 + t; p < p1; p += 256) {
      int32_t col; float val;
      bool skip = false;
      if (csr_entry(a.csr, p, skip, col, val)) d[col] = d[col] - k * val;
    }
  }
  if (bad) atomicOr(a.csr.flag, (unsigned)FEED_BAD_COL);
}

// ---- backward: both weight gradients' slabs and bias sums into the caller's tensors, ONE launch, blockIdx.y = segment ------------------
//   0: slabs [S][Ip][Hp], bias sums [S][Ip] -> dw4 [I][H], db4 [I]        1: slabs [S][Hp][Lp], bias sums [S][Hp] -> dw3 [H][L], db3 [H]
// Slabs are added in slab order; every element is written exactly once.
struct DecUnpadSeg {
  const float* slab; const float* dbias; int S, N, K, Np, Kp;   // slab [S][Np][Kp] -> dw [N][K]
  float* dw; float* db;
};
struct DecUnpadArgs { DecUnpadSeg seg[2]; };

__global__ __launch_bounds__(256) void k_dechead_unpad(const DecUnpadArgs args) {
  const DecUnpadSeg& a = args.seg[blockIdx.y];
  const int qpr = (a.K + 3) >> 2;
  const int64_t nw = (int64_t)a.N * qpr, total = nw + a.N;
  const size_t slab_stride = (size_t)a.Np * a.Kp;
  const bool vec = (a.K & 3) == 0 && latent_al16(a.dw);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= nw) {
      const int n = (int)(i - nw);
      float s = a.dbias[n];
      for (int k = 1; k < a.S; ++k) s += a.dbias[(size_t)k * a.Np + n];
      a.db[n] = s;
      continue;
    }
    const int n = (int)(i / qpr), c = 4 * (int)(i - (int64_t)n * qpr);
    const float* __restrict__ p = a.slab + (size_t)n * a.Kp + c;   // (Kp is a multiple of 32: 16-byte aligned, and c + 3 < Kp)
    float4 s = *reinterpret_cast<const float4*>(p);
    for (int k = 1; k < a.S; ++k) {
      const float4 u = *reinterpret_cast<const float4*>(p + (size_t)k * slab_stride);
      s.x += u.x; s.y += u.y; s.z += u.z; s.w += u.w;
    }
    latent_store4(a.dw + (size_t)n * a.K, c, a.K, vec, s);
  }
}

}  // namespace sdrm
