// The VAE encoder behind its first pre-activation in TRAIN mode, forward and backward (reference train_SDRM.py:244-250 with
// is_training == 1 - Tanh, Linear(hidden, 2 latent), chunk, the KL, the reparameterisation - and their share of :148):
//   h1 = tanh(pre)                      out2 = h1 W2^T + b2 = [mu | lv]
//   eps[r, j] = normal j & 3 of philox4x32_10(R_r, j >> 2, PURPOSE_VAE_EPS, step; seed)   R_r the feed row of batch row r
//   z = mu + eps exp(0.5 lv)            kl = -0.5 / b sum (lv - mu^2 - expm1(lv))
//   dmu = gz + gkl mu / b               dlv = 0.5 gz eps exp(0.5 lv) + 0.5 gkl expm1(lv) / b
//   dW2 = dout2^T h1    db2 = column sums of dout2    dpre = (dout2 W2) (1 - h1^2)
// The two Linears and the weight gradient are launches of the MFMA GEMM of csrc/gemm.h on zero-padded operands; what is here stages
// those operands and does the elementwise work between them.  Every kernel takes 16-byte accesses when the widths and the caller's
// pointers allow (a row stride of a multiple of four floats on a 16-byte base) and a scalar path with the same arithmetic otherwise.
// Plain HIP, vector / plain C++ stores only; no floating-point atomic: a result is a function of its inputs alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "encode.h"
#include "philox.h"

namespace sdrm {

__device__ __forceinline__ bool latent_al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// The float4 of columns c .. c+3 of row `p` of a matrix `cols` wide, zero behind the row's end (vec: one 16-byte load).
__device__ __forceinline__ float4 latent_load4(const float* __restrict__ p, int c, int cols, bool vec) {
  if (vec) return *reinterpret_cast<const float4*>(p + c);
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  v.x = p[c];
  if (c + 1 < cols) v.y = p[c + 1];
  if (c + 2 < cols) v.z = p[c + 2];
  if (c + 3 < cols) v.w = p[c + 3];
  return v;
}
__device__ __forceinline__ void latent_store4(float* __restrict__ p, int c, int cols, bool vec, float4 v) {
  if (vec) { *reinterpret_cast<float4*>(p + c) = v; return; }
  p[c] = v.x;
  if (c + 1 < cols) p[c + 1] = v.y;
  if (c + 2 < cols) p[c + 2] = v.z;
  if (c + 3 < cols) p[c + 3] = v.w;
}

// ---- forward, staging: ONE launch, blockIdx.y = segment --------------------------------------------------------------------------
//   0: pre [b][H] -> h1 = tanh(pre) into the caller's h1 [b][H] AND the GEMM's A operand hp [MP][Hp] (zero behind b rows / H columns)
//   1: W2 [2L][H] -> w2p [L2r][Hp]        2: b2 [2L] -> b2p [L2r]                      (zero-padded: the GEMM loads without bounds)
struct LatentStageArgs {
  const float* pre; float* h1; float* hp; int b, H, MP, Hp;
  const float* w2; float* w2p; int L2, L2r;
  const float* b2; float* b2p;
};

__global__ __launch_bounds__(256) void k_latent_stage(const LatentStageArgs a) {
  const int seg = blockIdx.y;
  const float* __restrict__ src = seg == 0 ? a.pre : seg == 1 ? a.w2 : a.b2;
  float* __restrict__ dst = seg == 0 ? a.hp : seg == 1 ? a.w2p : a.b2p;
  const int rows = seg == 0 ? a.b : seg == 1 ? a.L2 : 1, cols = seg == 2 ? a.L2 : a.H;
  const int rowsP = seg == 0 ? a.MP : seg == 1 ? a.L2r : 1, colsP = seg == 2 ? a.L2r : a.Hp;
  const int qpr = colsP >> 2;
  const int64_t total = (int64_t)rowsP * qpr;
  const bool vec = (cols & 3) == 0 && latent_al16(src);
  const bool vec_h1 = (cols & 3) == 0 && latent_al16(a.h1);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / qpr), c = 4 * (int)(i - (int64_t)r * qpr);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows && c < cols) {
      v = latent_load4(src + (size_t)r * cols, c, cols, vec);
      if (seg == 0) {
        v = make_float4(tanh_fast(v.x), tanh_fast(v.y), tanh_fast(v.z), tanh_fast(v.w));   // (a lane behind the row's end: tanh(0) = 0)
        latent_store4(a.h1 + (size_t)r * cols, c, cols, vec_h1, v);
      }
    }
    *reinterpret_cast<float4*>(dst + (size_t)r * colsP + c) = v;
  }
}

// ---- forward: the draw, z and the KL partials ------------------------------------------------------------------------------------
struct LatentReparamArgs {
  const float* out2;       // [b][2L]: mu | lv
  const int64_t* rows;     // [b] feed rows (null: row0 .. row0+b-1): the Philox counter only, no feed is read
  int64_t row0;
  int b, L;
  uint32_t k0, k1, step;   // key = seed, counter word 3 = step
  int draw;                // != 0: eps is drawn and written; 0: eps is read
  float* eps;              // [b][L]
  float* z;                // [b][L]
  double* part;            // [gridDim.x] float64 partials of sum (lv - mu^2 - expm1(lv))
  unsigned* flag;          // the handle's feed status word: a feed row outside [0, 2^31) raises FEED_BAD_ROW (its counter is the id's low word)
};

// Block k takes rows k, k + gridDim.x, ..; a thread owns the column quads t, t + 256, .. of a row and draws each once (one Philox call,
// two Box-Muller pairs: the layout of oracle/philox_ref.py `_quad_normals`).  The KL terms are fp32, summed in float64: every thread
// in a fixed order, then the tree (encode_block_sum) - k_encode_kl_sum adds the partials in block order.
__global__ __launch_bounds__(256) void k_latent_reparam(const LatentReparamArgs a) {
  __shared__ double red[256];
  const int L = a.L, nq = (L + 3) >> 2;
  const bool vec = (L & 3) == 0 && latent_al16(a.out2) && latent_al16(a.eps) && latent_al16(a.z);
  double s = 0.0;
  for (int r = blockIdx.x; r < a.b; r += gridDim.x) {
    const int64_t R = a.rows ? a.rows[r] : a.row0 + r;
    if ((R < 0 || R >= ((int64_t)1 << 31)) && threadIdx.x == 0) atomicOr(a.flag, (unsigned)FEED_BAD_ROW);
    const float* __restrict__ mu_p = a.out2 + (size_t)r * 2 * L;
    const float* __restrict__ lv_p = mu_p + L;
    float* __restrict__ eps_p = a.eps + (size_t)r * L;
    float* __restrict__ z_p = a.z + (size_t)r * L;
    for (int q = threadIdx.x; q < nq; q += 256) {
      const int c = 4 * q;
      const float4 mu = latent_load4(mu_p, c, L, vec), lv = latent_load4(lv_p, c, L, vec);
      float4 e;
      if (a.draw) {
        const U4 w = philox4x32_10((uint32_t)R, (uint32_t)q, PURPOSE_VAE_EPS, a.step, a.k0, a.k1);
        box_muller(w.x, w.y, e.x, e.y);
        box_muller(w.z, w.w, e.z, e.w);
        latent_store4(eps_p, c, L, vec, e);
      } else {
        e = latent_load4(eps_p, c, L, vec);
      }
      float4 zz;
      zz.x = fmaf(e.x, expf(0.5f * lv.x), mu.x);
      zz.y = fmaf(e.y, expf(0.5f * lv.y), mu.y);
      zz.z = fmaf(e.z, expf(0.5f * lv.z), mu.z);
      zz.w = fmaf(e.w, expf(0.5f * lv.w), mu.w);
      latent_store4(z_p, c, L, vec, zz);
      // (columns behind L were loaded as mu = lv = 0: their term is exactly 0)
      s += (double)((lv.x - expm1f(lv.x)) - mu.x * mu.x);
      s += (double)((lv.y - expm1f(lv.y)) - mu.y * mu.y);
      s += (double)((lv.z - expm1f(lv.z)) - mu.z * mu.z);
      s += (double)((lv.w - expm1f(lv.w)) - mu.w * mu.w);
    }
  }
  s = encode_block_sum(s, red);
  if (threadIdx.x == 0) a.part[blockIdx.x] = s;
}

// ---- backward, staging: ONE launch ------------------------------------------------------------------------------------------------
// The first `tiles` work-groups transpose W2 [2L][H] into w2t [Hr][L2p] (the NT dgrad's B operand), 32 x 32 tiles through LDS, zero
// behind 2L columns / H rows; the others copy h1 [b][H] into hp [MP][Hp] (the weight gradient's B operand and the dgrad epilogue's
// aux), zero-padded.
struct LatentStageBwdArgs {
  const float* w2; float* w2t; int L2, H, L2p, Hr;
  const float* h1; float* hp; int b, MP, Hp;
  int tiles, tiles_l;      // tiles = (Hr / 32) * tiles_l, tiles_l = L2p / 32
};

__global__ __launch_bounds__(256) void k_latent_stage_bwd(const LatentStageBwdArgs a) {
  __shared__ float tile[32][33];
  if ((int)blockIdx.x < a.tiles) {
    const int th = blockIdx.x / a.tiles_l, tl = blockIdx.x - th * a.tiles_l;
    const int h0 = th * 32, l0 = tl * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8) {
      const int l = l0 + k, h = h0 + tx;
      tile[k][tx] = (l < a.L2 && h < a.H) ? a.w2[(size_t)l * a.H + h] : 0.f;
    }
    __syncthreads();
    for (int k = ty; k < 32; k += 8) a.w2t[(size_t)(h0 + k) * a.L2p + l0 + tx] = tile[tx][k];   // (h0 + k < Hr, l0 + tx < L2p: whole tiles)
    return;
  }
  const int qpr = a.Hp >> 2;
  const int64_t total = (int64_t)a.MP * qpr;
  const bool vec = (a.H & 3) == 0 && latent_al16(a.h1);
  const int64_t nthreads = (int64_t)(gridDim.x - a.tiles) * blockDim.x;
  for (int64_t i = (int64_t)(blockIdx.x - a.tiles) * blockDim.x + threadIdx.x; i < total; i += nthreads) {
    const int r = (int)(i / qpr), c = 4 * (int)(i - (int64_t)r * qpr);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < a.b && c < a.H) v = latent_load4(a.h1 + (size_t)r * a.H, c, a.H, vec);
    *reinterpret_cast<float4*>(a.hp + (size_t)r * a.Hp + c) = v;
  }
}

// ---- backward: the seed dout2 = [dmu | dlv] into the padded operand of both backward GEMMs ----------------------------------------
struct LatentSeedArgs {
  const float* out2; const float* eps;   // [b][2L], [b][L]
  const float* gz;                       // [b][L] or null (zero)
  const float* gkl;                      // device scalar or null (zero)
  int b, L, MP, L2p;
  float* dp;                             // [MP][L2p], zero behind b rows / 2L columns
};

__device__ __forceinline__ float latent_dmu(float mu, float gz, float gk) { return fmaf(gk, mu, gz); }
__device__ __forceinline__ float latent_dlv(float lv, float gz, float eps, float gk) {
  return fmaf(0.5f * gz * eps, expf(0.5f * lv), 0.5f * gk * expm1f(lv));
}

__global__ __launch_bounds__(256) void k_latent_seed(const LatentSeedArgs a) {
  const int L = a.L, qpr = a.L2p >> 2;
  const int64_t total = (int64_t)a.MP * qpr;
  const float gk = a.gkl ? *a.gkl / (float)a.b : 0.f;
  const bool vec = (L & 3) == 0 && latent_al16(a.out2) && latent_al16(a.eps) && (!a.gz || latent_al16(a.gz));
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(i / qpr), c = 4 * (int)(i - (int64_t)r * qpr);
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < a.b && c < 2 * L) {
      const float* __restrict__ o = a.out2 + (size_t)r * 2 * L;
      if (vec) {   // L a multiple of four: the quad lies on one side of the mu | lv boundary
        const float4 x = *reinterpret_cast<const float4*>(o + c);
        const int j = c < L ? c : c - L;
        const float4 g = a.gz ? *reinterpret_cast<const float4*>(a.gz + (size_t)r * L + j) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < L) {
          v = make_float4(latent_dmu(x.x, g.x, gk), latent_dmu(x.y, g.y, gk), latent_dmu(x.z, g.z, gk), latent_dmu(x.w, g.w, gk));
        } else {
          const float4 e = *reinterpret_cast<const float4*>(a.eps + (size_t)r * L + j);
          v = make_float4(latent_dlv(x.x, g.x, e.x, gk), latent_dlv(x.y, g.y, e.y, gk), latent_dlv(x.z, g.z, e.z, gk), latent_dlv(x.w, g.w, e.w, gk));
        }
      } else {
        float t[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int col = c + k;
          if (col >= 2 * L) continue;
          const int j = col < L ? col : col - L;
          const float g = a.gz ? a.gz[(size_t)r * L + j] : 0.f;
          t[k] = col < L ? latent_dmu(o[col], g, gk) : latent_dlv(o[col], g, a.eps[(size_t)r * L + j], gk);
        }
        v = make_float4(t[0], t[1], t[2], t[3]);
      }
    }
    *reinterpret_cast<float4*>(a.dp + (size_t)r * a.L2p + c) = v;
  }
}

// ---- backward: the weight gradient's slabs [S][L2p][Hp] and bias sums [S][L2p] into the caller's dw2 [2L][H] and db2 [2L] ----------
// Slabs are added in slab order (S = 1 but for batches of more than LATENT_WGRAD_KCHUNK rows); every element is written exactly once.
struct LatentUnpadArgs {
  const float* slab; const float* dbias; int S, L2, H, L2p, Hp;
  float* dw2; float* db2;
};

__global__ __launch_bounds__(256) void k_latent_unpad(const LatentUnpadArgs a) {
  const int qpr = (a.H + 3) >> 2;
  const int64_t nw = (int64_t)a.L2 * qpr, total = nw + a.L2;
  const size_t slab_stride = (size_t)a.L2p * a.Hp;
  const bool vec = (a.H & 3) == 0 && latent_al16(a.dw2);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    if (i >= nw) {
      const int n = (int)(i - nw);
      float s = a.dbias[n];
      for (int k = 1; k < a.S; ++k) s += a.dbias[(size_t)k * a.L2p + n];
      a.db2[n] = s;
      continue;
    }
    const int n = (int)(i / qpr), c = 4 * (int)(i - (int64_t)n * qpr);
    const float* __restrict__ p = a.slab + (size_t)n * a.Hp + c;   // (Hp is a multiple of 32: 16-byte aligned, and c + 3 < Hp)
    float4 s = *reinterpret_cast<const float4*>(p);
    for (int k = 1; k < a.S; ++k) {
      const float4 t = *reinterpret_cast<const float4*>(p + (size_t)k * slab_stride);
      s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
    }
    latent_store4(a.dw2 + (size_t)n * a.H, c, a.H, vec, s);
  }
}

}  // namespace sdrm
