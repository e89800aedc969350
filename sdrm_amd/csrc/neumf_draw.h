// An epoch's data preparation of the NeuMF evaluator on the device (reference: neural_cf_benchmark_pt.py:180-184 - the 80/20 split of the
// training triples, the label-0 rows of the 80 % drawn again with replacement, the shuffle), from triples T [n][3] int32 that stay resident.
// Everything is a function of (seed, epoch) and T, defined so that numpy restates it exactly (tests/neumf_draw_ref.py).
// The keyed permutation perm(n, seed, epoch, draw) of 0 .. n-1 (n >= 1) is a balanced Feistel network with cycle walking:
//   b = max(1, bit_length(n - 1)), h = (b + 1) / 2, mask = 2^h - 1 (the domain 4^h >= n);  for x: L = x >> h, R = x & mask, six rounds
//   r = 0 .. 5 of (L, R) <- (R, L ^ (W & mask)) with W = word 0 of philox4x32_10(R, r, PURPOSE_NEUMF_EPOCH | draw << 8, epoch; seed),
//   then x = L << h | R;  perm(i) starts at x = i and repeats that map until x < n.
// A bijection of [0, n) (the map is one of [0, 4^h), and walking a cycle of it back into [0, n) keeps that).  The loop here is bounded
// at DRAW_MAX_WALKS; a lane that reaches the bound raises DRAW_STATUS_WALK and reads row 0.
// The draw:  hold[j] = T[perm0(j)], j < n_hold;  part[q] = T[perm0(n_hold + q)], q < n_part = n - n_hold;  g_0 < g_1 < ... the places q
// with label 0 (n_neg of them), n_pos the places with label 1;  n_extra = n_neg ? n_pos : 0;  extra[k] = part[g_r], r = bounded(w, n_neg),
// w = word k & 3 of philox4x32_10(k >> 2, 0, PURPOSE_NEUMF_EPOCH | 1 << 8, epoch; seed);  m = n_part + n_extra;
// out[p] = (part ++ extra)[perm2(m)(p)], p < m.  Neither part nor extra exists in memory: only their source places in T do.
//   k_draw_split   a lane per place.  The first work-groups gather hold and mark `present`; the others store the source place of part[q]
//                  into part_src[q], the ballot of "label 0" of every wave as a mask word, and the work-group's label-0 / label-1 counts.
//   k_draw_scan    one work-group: exclusive scan of the label-0 counts with a carry (csrc/compact.h: k_csr_scan), the sum of the
//                  label-1 counts; leaves n_pos, n_neg, m in counts[3].
//   k_draw_neg     neg_src[0 .. n_neg) = part_src[g_0], part_src[g_1], ... from the mask words and the scanned offsets alone.
//   k_draw_out     over the capacity 2 n_part: lanes p >= m leave, the others gather T[part_src[j]] or T[neg_src[r]], j = perm2(m)(p).
// Integers only, no floating-point atomic, no unbounded loop; every load index is below n by construction, every store is held to its
// array.  The round words are Philox evaluations on the fly (a lane pays six per walk, 4^h / n <= 4 walks on average).  Vector stores only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "csr_batch.h"
#include "philox.h"

namespace sdrm {

constexpr int DRAW_MAX_WALKS = 1024;        // applications of the Feistel map a lane makes before it gives up
constexpr unsigned DRAW_STATUS_WALK = 1u;   // the call's status word: a lane met the bound
constexpr int DRAW_SCAN_PER = 8;            // work-group counts per thread and chunk of k_draw_scan

struct DrawTriple { int32_t user, item, label; };

struct DrawArgs {
  const DrawTriple* T;          // [n]
  uint32_t n, n_hold, n_part;   // n <= 2^30
  uint32_t k0, k1, epoch;       // the 64-bit seed, low and high word (the Philox key), and counter word 3
  DrawTriple* hold;             // [n_hold]
  DrawTriple* out;              // [2 n_part]
  uint8_t* present;             // [n_users], zeroed by the call, or null
  int n_users;
  uint32_t hold_blocks, part_blocks;   // work-groups of k_draw_split: ceil(n_hold / 256), then ceil(n_part / 256)
  int32_t* part_src;            // [n_part] the place in T of part[q]
  int32_t* neg_src;             // [n_part] the place in T of the j-th label-0 row of part (n_neg of them)
  uint64_t* mask0;              // [ceil(n_part / 64)] bit q & 63 of word q >> 6: part[q] has label 0
  uint32_t* cnt;                // [2][part_blocks] label-0 and label-1 rows of every work-group's 256 places
  uint32_t* off0;               // [part_blocks] label-0 rows in front of the work-group
  int64_t* counts;              // [3] n_pos, n_neg, m
  unsigned* status;             // DRAW_STATUS_*
  unsigned* flag;               // the handle's feed status word
};

struct DrawPerm { uint32_t n, h, mask, c2; };

__host__ __device__ inline DrawPerm draw_perm(uint32_t n, uint32_t draw) {
  uint32_t b = 0;
  for (uint32_t v = n - 1; v; v >>= 1) ++b;   // bit_length(n - 1), at most 32 steps
  if (b < 1) b = 1;
  const uint32_t h = (b + 1) >> 1;
  return DrawPerm{n, h, (1u << h) - 1u, PURPOSE_NEUMF_EPOCH | (draw << 8)};
}

__host__ __device__ inline uint32_t draw_feistel(const DrawPerm& p, uint32_t x, uint32_t epoch, uint32_t k0, uint32_t k1) {
  uint32_t L = x >> p.h, R = x & p.mask;
  for (uint32_t r = 0; r < 6; ++r) {
    const uint32_t w = philox4x32_10(R, r, p.c2, epoch, k0, k1).x;
    const uint32_t t = L ^ (w & p.mask);
    L = R;
    R = t;
  }
  return (L << p.h) | R;
}

// perm(i); `failed` is set (and 0 returned, a valid place) where the bound is met
__host__ __device__ inline uint32_t draw_perm_at(const DrawPerm& p, uint32_t i, uint32_t epoch, uint32_t k0, uint32_t k1, bool& failed) {
  uint32_t x = i;
  for (int w = 0; w < DRAW_MAX_WALKS; ++w) {
    x = draw_feistel(p, x, epoch, k0, k1);
    if (x < p.n) return x;
  }
  failed = true;
  return 0u;
}

__global__ __launch_bounds__(256) void k_draw_split(const DrawArgs a) {
  __shared__ uint32_t wcnt[2][4];
  const DrawPerm pm = draw_perm(a.n, 0u);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  bool failed = false;
  if (blockIdx.x < a.hold_blocks) {                        // (uniform over the work-group)
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < a.n_hold) {
      const uint32_t src = draw_perm_at(pm, j, a.epoch, a.k0, a.k1, failed);
      const DrawTriple t = a.T[src];
      a.hold[j] = t;
      if (a.present) {
        if (t.user >= 0 && t.user < a.n_users) a.present[t.user] = (uint8_t)1;
        else atomicOr(a.flag, (unsigned)FEED_BAD_ROW);
      }
    }
  } else {
    const uint32_t pb = blockIdx.x - a.hold_blocks;
    const uint32_t q = pb * 256u + threadIdx.x;
    bool zero = false, one = false;
    if (q < a.n_part) {
      const uint32_t src = draw_perm_at(pm, a.n_hold + q, a.epoch, a.k0, a.k1, failed);
      a.part_src[q] = (int32_t)src;
      const int32_t label = a.T[src].label;
      zero = label == 0;
      one = label == 1;
    }
    const uint64_t bz = __ballot(zero), bo = __ballot(one);
    if (lane == 0) {
      if (q < a.n_part) a.mask0[q >> 6] = bz;              // (lane 0 holds the wave's first place: behind n_part, the whole wave is)
      wcnt[0][wave] = (uint32_t)__popcll(bz);
      wcnt[1][wave] = (uint32_t)__popcll(bo);
    }
    __syncthreads();
    if (threadIdx.x == 0 && pb < a.part_blocks) {
      a.cnt[pb] = wcnt[0][0] + wcnt[0][1] + wcnt[0][2] + wcnt[0][3];
      a.cnt[a.part_blocks + pb] = wcnt[1][0] + wcnt[1][1] + wcnt[1][2] + wcnt[1][3];
    }
  }
  if (failed) atomicOr(a.status, DRAW_STATUS_WALK);
}

__global__ __launch_bounds__(256) void k_draw_scan(const DrawArgs a) {
  __shared__ uint32_t wsum[4];
  __shared__ uint32_t wone[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t nb = a.part_blocks;
  uint32_t carry = 0, ones = 0;
  for (uint32_t c0 = 0; c0 < nb; c0 += 256u * DRAW_SCAN_PER) {
    const uint32_t r0 = c0 + (uint32_t)tid * DRAW_SCAN_PER;
    uint32_t c[DRAW_SCAN_PER];
    uint32_t s = 0;
#pragma unroll
    for (int j = 0; j < DRAW_SCAN_PER; ++j) {
      c[j] = 0u;
      if (r0 + j < nb) { c[j] = a.cnt[r0 + j]; ones += a.cnt[nb + r0 + j]; }
      s += c[j];
    }
    uint32_t inc = s;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t up = __shfl_up(inc, d);
      if (lane >= d) inc += up;
    }
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t run = carry + inc - s;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < wave) run += wsum[i];
      carry += wsum[i];
    }
#pragma unroll
    for (int j = 0; j < DRAW_SCAN_PER; ++j) {
      if (r0 + j < nb) a.off0[r0 + j] = run;
      run += c[j];
    }
    __syncthreads();
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) ones += __shfl_xor(ones, d);
  if (lane == 0) wone[wave] = ones;
  __syncthreads();
  if (tid == 0) {
    const int64_t n_pos = (int64_t)wone[0] + wone[1] + wone[2] + wone[3], n_neg = (int64_t)carry;
    a.counts[0] = n_pos;
    a.counts[1] = n_neg;
    a.counts[2] = (int64_t)a.n_part + (n_neg > 0 ? n_pos : 0);
  }
}

__global__ __launch_bounds__(256) void k_draw_neg(const DrawArgs a) {
  const uint32_t q = blockIdx.x * 256u + threadIdx.x;
  if (q >= a.n_part) return;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint64_t mine = a.mask0[q >> 6];
  if (!((mine >> lane) & 1ull)) return;
  uint32_t pos = a.off0[blockIdx.x] + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
  for (int i = 0; i < wave; ++i) pos += (uint32_t)__popcll(a.mask0[blockIdx.x * 4u + i]);   // (the words of the waves in front exist: this one's does)
  if (pos < a.n_part) a.neg_src[pos] = a.part_src[q];
}

__global__ __launch_bounds__(256) void k_draw_out(const DrawArgs a) {
  const uint32_t p = blockIdx.x * 256u + threadIdx.x;
  const uint32_t m = (uint32_t)a.counts[2], n_neg = (uint32_t)a.counts[1];
  if (p >= m || m > 2u * a.n_part) return;
  const DrawPerm pm = draw_perm(m, 2u);
  bool failed = false;
  const uint32_t j = draw_perm_at(pm, p, a.epoch, a.k0, a.k1, failed);
  uint32_t src = 0u;
  if (j < a.n_part) {
    src = (uint32_t)a.part_src[j];
  } else if (n_neg > 0u && n_neg <= a.n_part) {
    const uint32_t k = j - a.n_part;
    const U4 w = philox4x32_10(k >> 2, 0u, PURPOSE_NEUMF_EPOCH | (1u << 8), a.epoch, a.k0, a.k1);
    const uint32_t word = (k & 3u) == 0u ? w.x : (k & 3u) == 1u ? w.y : (k & 3u) == 2u ? w.z : w.w;
    src = (uint32_t)a.neg_src[bounded(word, n_neg)];
  }
  if (src >= a.n) src = 0u;
  a.out[p] = a.T[src];
  if (failed) atomicOr(a.status, DRAW_STATUS_WALK);
}

}  // namespace sdrm
