// lgx_heads_row.h — the PPO loss head's per-row arithmetic (include/lgx_mlp.h: rsl_rl ppo.py:196-262
// with the Gaussian policy of actor_critic.py), shared by the kernels that run it: lgx_mlp.hip's
// lgx_loss_heads_fused / lgx_loss_heads_tail and lgx_s8.hip's forward epilogue (lgx_s8_heads_fwd).
// One copy of every expression: the kernels differ in where a row's inputs come from and which
// thread runs which piece, never in the arithmetic or in the order of a sum, so their outputs are
// equal bit for bit (both libraries build with -ffp-contract=off). Device code only.
#ifndef LGX_HEADS_ROW_H
#define LGX_HEADS_ROW_H
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/lgx_mlp.h"

namespace lgxh {

constexpr int HMAXA = 16;                 // max actions (a head->ws row is 3 + HMAXA floats)
constexpr int TR = LGX_HEADS_TAIL_ROWS;   // rows of one partial (ws row, column-sum partial)
constexpr float L2PI = 0.9189385332046727f;  // log(sqrt(2 pi))

__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
  const __bf16 x = (__bf16)a, y = (__bf16)b;
  return (unsigned)__builtin_bit_cast(unsigned short, x) | ((unsigned)__builtin_bit_cast(unsigned short, y) << 16);
}
// 8 fp32 -> one S8 group (32 B: the 8 bf16 hi values, then the 8 bf16 lo = bf16(x - hi))
__device__ __forceinline__ void store_s8_group(char* dst, const float (&v)[8]) {
  float lo[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) lo[e] = v[e] - (float)(__bf16)v[e];
  typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
  const u32x4_ H = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]), pack_bf16x2(v[6], v[7])};
  const u32x4_ L = {pack_bf16x2(lo[0], lo[1]), pack_bf16x2(lo[2], lo[3]), pack_bf16x2(lo[4], lo[5]),
                    pack_bf16x2(lo[6], lo[7])};
  reinterpret_cast<u32x4_*>(dst)[0] = H;
  reinterpret_cast<u32x4_*>(dst)[1] = L;
}

// One row's action-wide inputs, loaded up front at clamped columns (columns past A repeat the
// last one and are discarded by selects): no branch around a load, so all of a row's loads
// are in flight together (a guarded or late load is a round trip of its own, ~0.3 us).
template <int NA>
__device__ __forceinline__ void load_cols(const float* __restrict__ x, int i, int A, float (&v)[NA]) {
#pragma unroll
  for (int j = 0; j < NA; ++j) v[j] = x[(int64_t)i * A + min(j, A - 1)];
}

// ---- one action's terms of a row
// log-prob term of action j: the row's log-prob is their sum in action order (from 0.f)
__device__ __forceinline__ float lp_term(float act, float mu, float sd, float lsd) {
  const float d = act - mu;
  return -(d * d) / (2.f * sd * sd) - lsd - L2PI;
}
// KL term of action j (summed the same way)
__device__ __forceinline__ float kl_term(float om, float os, float mu, float sd) {
  const float dm = om - mu;
  return logf(sd / os + 1.0e-5f) + (os * os + dm * dm) / (2.f * (sd * sd)) - 0.5f;
}
// gradient of mu_j and the std-gradient term of action j from the row's dlogp
__device__ __forceinline__ void dmu_term(float dlogp, float act, float mu, float sd, float& dmu, float& dstd) {
  const float d = act - mu;
  const float var = sd * sd;
  dmu = dlogp * d / var;
  dstd = dlogp * (d * d / (var * sd) - 1.f / sd);
}

// ---- the row's scalar stages. The discrete decisions follow torch's gradient rules (max splits
// ties, clamp passes on [lo, hi]); `forced`: take them from the byte `din` instead
// (lgx_heads_s8_args.decisions_in). Each returns the row's OWN decision bits (decisions_out).
// The policy half (bits 0-2): surrogate value and dlogp from the row's log-prob.
__device__ __forceinline__ unsigned actor_row(float lp, float old_logp, float a, float clip, float gs, bool forced,
                                              unsigned din, float& surr, float& dlogp) {
  const float ratio = expf(lp - old_logp);
  const float lo = 1.f - clip, hi = 1.f + clip;
  const float s1 = -a * ratio, s2 = -a * fminf(fmaxf(ratio, lo), hi);
  float w1 = s1 > s2 ? 1.f : (s1 == s2 ? 0.5f : 0.f);
  float in = (ratio >= lo && ratio <= hi) ? 1.f : 0.f;
  const unsigned own = (unsigned)(2.f * w1) | ((unsigned)in << 2);
  if (forced) {
    w1 = 0.5f * (float)(din & 3u);
    in = (float)((din >> 2) & 1u);
  }
  // the forced branch's value (a tie: either)
  surr = !forced ? fmaxf(s1, s2) : (w1 > 0.75f ? s1 : (w1 < 0.25f ? s2 : fmaxf(s1, s2)));
  const float w2 = 1.f - w1;
  const float dratio = gs * (w1 * -a + w2 * -a * in);
  dlogp = dratio * ratio;
  return own;
}
// The value half (bits 3-5): value loss and dvalue. tv_in: the target value (read only with
// clipped_value).
__device__ __forceinline__ unsigned critic_row(float val, float R, float tv_in, float clip, bool clipped_value,
                                               float gv, bool forced, unsigned din, float& vloss, float& dv) {
  const float tv = clipped_value ? tv_in : val;
  const float vc = clipped_value ? tv + fminf(fmaxf(val - tv, -clip), clip) : 0.f;
  const float l1 = (val - R) * (val - R), l2 = (vc - R) * (vc - R);
  float u1 = l1 > l2 ? 1.f : (l1 == l2 ? 0.5f : 0.f);
  float inv = (val - tv >= -clip && val - tv <= clip) ? 1.f : 0.f;
  const unsigned own = ((unsigned)(2.f * u1) << 3) | ((unsigned)inv << 5);
  if (forced) {
    u1 = 0.5f * (float)((din >> 3) & 3u);
    inv = (float)((din >> 5) & 1u);
  }
  if (!forced) vloss = clipped_value ? fmaxf(l1, l2) : (R - val) * (R - val);
  else vloss = clipped_value ? (u1 > 0.75f ? l1 : (u1 < 0.25f ? l2 : fmaxf(l1, l2))) : (R - val) * (R - val);
  if (clipped_value) dv = gv * (u1 * 2.f * (val - R) + (1.f - u1) * 2.f * (vc - R) * inv);
  else dv = gv * 2.f * (val - R);
  return own;
}
// a decisions_in byte with bit 6 set leaves the row its own decisions (near-tie-only replays)
__device__ __forceinline__ bool decisions_forced(const lgx_heads_s8_args& s, int i, unsigned& din) {
  const bool forced = s.decisions_in != nullptr && !(s.decisions_in[i] & 0x40u);
  din = forced ? s.decisions_in[i] : 0u;
  return forced;
}

// ---- the last layers (fp32 FMAs, k in order)
// dot over k < n of two LDS rows (16-B aligned), k in order
__device__ __forceinline__ float lds_dot(const float* x, const float* w, int n) {
  float acc = 0.f;
#pragma unroll 8
  for (int k = 0; k < n; k += 4) {
    const float4 a = *reinterpret_cast<const float4*>(x + k);
    const float4 b = *reinterpret_cast<const float4*>(w + k);
    acc = fmaf(a.x, b.x, acc);
    acc = fmaf(a.y, b.y, acc);
    acc = fmaf(a.z, b.z, acc);
    acc = fmaf(a.w, b.w, acc);
  }
  return acc;
}
// 8 columns (one S8 group, at w[.. + 0..7]) of dmu W: a in order; rows of W past A are zero.
// dmu: the row's NA gradients; w: W's column group in LDS, row pitch pw floats.
template <int NA>
__device__ __forceinline__ void dmu_w8(const float* dmu, const float* w, int pw, float (&x)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = 0.f;
#pragma unroll
  for (int a = 0; a < NA; ++a) {
    const float d = dmu[a];
    const float4 w0 = *reinterpret_cast<const float4*>(w + a * pw);
    const float4 w1 = *reinterpret_cast<const float4*>(w + a * pw + 4);
    x[0] = fmaf(d, w0.x, x[0]); x[1] = fmaf(d, w0.y, x[1]); x[2] = fmaf(d, w0.z, x[2]);
    x[3] = fmaf(d, w0.w, x[3]); x[4] = fmaf(d, w1.x, x[4]); x[5] = fmaf(d, w1.y, x[5]);
    x[6] = fmaf(d, w1.z, x[6]); x[7] = fmaf(d, w1.w, x[7]);
  }
}
// 8 columns of dvalue W_c
__device__ __forceinline__ void dv_w8(float d, const float* w, float (&x)[8]) {
  const float4 w0 = *reinterpret_cast<const float4*>(w);
  const float4 w1 = *reinterpret_cast<const float4*>(w + 4);
  x[0] = d * w0.x; x[1] = d * w0.y; x[2] = d * w0.z; x[3] = d * w0.w;
  x[4] = d * w1.x; x[5] = d * w1.y; x[6] = d * w1.z; x[7] = d * w1.w;
}
// times ELU'(y) of the 8 LDS values at y (y: the ELU outputs), written back in place of y
__device__ __forceinline__ void delu8_inplace(const float (&x)[8], float* y, float (&d)[8]) {
  const float4 y0 = *reinterpret_cast<const float4*>(y);
  const float4 y1 = *reinterpret_cast<const float4*>(y + 4);
  const float yy[8] = {y0.x, y0.y, y0.z, y0.w, y1.x, y1.y, y1.z, y1.w};
#pragma unroll
  for (int e = 0; e < 8; ++e) d[e] = x[e] * (yy[e] > 0.f ? 1.f : yy[e] + 1.f);
  *reinterpret_cast<float4*>(y) = {d[0], d[1], d[2], d[3]};
  *reinterpret_cast<float4*>(y + 4) = {d[4], d[5], d[6], d[7]};
}
// column k's sum over the TR rows of one partial, rows in order (pitch p floats)
__device__ __forceinline__ float col_sum_rows(const float* y, int p) {
  float sum = 0.f;
#pragma unroll 8
  for (int r = 0; r < TR; ++r) sum += y[r * p];
  return sum;
}

// ---- one value k of partial bx (NV = 3 + 2 NA + 1 values: surrogate, value loss, KL | the
// std-gradient terms [NA] | the dmu column sums [NA] | the dvalue sum), summed over the partial's
// TR rows in row order and written where lgx_loss_heads_tail documents it: head->ws row bx =
// {surr / B, vloss / B, kl / B, dstd partial [A]} (partial 0's with the entropy term ge / std),
// s8->dmu_cs / dvalue_cs row bx. rowv [TR][4] (surrogate, value loss, KL, -), tvs [TR][NA],
// dmus [TR][NA], dvs [TR]: the rows' values; only the arrays that k reads are touched.
template <int NA>
__device__ __forceinline__ void partial_value(const lgx_ppo_head_args& p, const lgx_heads_s8_args& s, int k, int bx,
                                              const float* rowv, const float* tvs, const float* dmus,
                                              const float* dvs, const float* stdv, float ge) {
  float sum = 0.f;
  for (int q = 0; q < TR; ++q) {
    const float x = k < 3 ? rowv[q * 4 + k]
                          : (k < 3 + NA ? tvs[q * NA + k - 3]
                                        : (k < 3 + 2 * NA ? dmus[q * NA + k - 3 - NA] : dvs[q]));
    sum += x;
  }
  const float inv = 1.f / p.B;
  float* w = p.ws + (int64_t)bx * (3 + HMAXA);
  if (k < 3) w[k] = sum * inv;
  else if (k < 3 + NA) {
    const int j = k - 3;
    if (j < p.A) w[3 + j] = sum + (bx == 0 ? ge / stdv[j] : 0.f);
  } else if (k < 3 + 2 * NA) {
    const int j = k - 3 - NA;
    if (s.dmu_cs && j < p.A) s.dmu_cs[(int64_t)bx * p.A + j] = sum;
  } else if (s.dvalue_cs) {
    s.dvalue_cs[bx] = sum;
  }
}
// the entropy (a constant of std): partial 0 writes it into out[2]
__device__ __forceinline__ float entropy_of(const float* lstd, int A) {
  float ent = 0.f;
  for (int j = 0; j < A; ++j) ent += 0.5f + L2PI + lstd[j];
  return ent;
}

// ---------------------------------------------------------------- block sums (deterministic)
#ifndef LGX_HT
#define LGX_HT 256
#endif
constexpr int HT = LGX_HT;  // threads per block (rows per block and grid-stride pass)
// the loss heads' cross-wave scratch (red[4 * ...]) holds at most 4 waves
static_assert(HT % 64 == 0 && HT >= 64 && HT <= 256, "LGX_HT: 64..256 threads, whole waves");
// block-wide sum of NV values per thread into red[NV] (thread 0 holds the result)
template <int NV>
__device__ void block_sum(float (&v)[NV], float* red) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    float x = v[k];
    for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
    v[k] = x;
  }
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) red[wv * NV + k] = v[k];
  __syncthreads();
  if (threadIdx.x == 0)
#pragma unroll
    for (int k = 0; k < NV; ++k) {
      float t = red[k];
      for (int w = 1; w < (int)(blockDim.x >> 6); ++w) t += red[w * NV + k];  // waves in order
      v[k] = t;
    }
}

// The last block to finish reduces the per-block partials. Thread 0 wrote this block's
// partials: it alone releases them (agent scope) before the counter — an agent-scope fence
// by every thread of every block costs microseconds per block — and the last block's
// threads acquire before they read the other blocks' partials.
__device__ bool last_block(uint32_t* counter, unsigned nblk = 0) {
  __shared__ bool last;
  __syncthreads();
  if (threadIdx.x == 0) {
    __threadfence();
    last = atomicAdd(counter, 1u) == (nblk ? nblk : gridDim.x) - 1;
  }
  __syncthreads();
  if (last) __threadfence();
  return last;
}

// Sum of the NV-wide partial rows ws[b * stride + k] over b < nblk, by the whole block: a
// fixed assignment (thread t takes rows t, t + 256, ...) and the fixed block_sum tree, so
// the result is deterministic for a given grid. Thread 0 holds the totals.
template <int NV>
__device__ void final_sum(const float* ws, int stride, int nblk, float (&v)[NV], float* red) {
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.f;
  for (int b = threadIdx.x; b < nblk; b += blockDim.x)
#pragma unroll
    for (int k = 0; k < NV; ++k) v[k] += ws[b * stride + k];
  __syncthreads();  // red is reused
  block_sum<NV>(v, red);
}

// ---------------------------------------------------------------- ROA + estimator losses (the aux head)
// p rows i0 .. i0 + HT - 1, columns [j0, j0 + w) (w <= AUX_CW) staged into st[row][AUX_CW + 1]
// with coalesced loads: p is usually a column span of the actor-input buffer (row stride
// ld_p), where one row per thread would touch a separate cache line per lane and load.
constexpr int AUX_CW = 16;
constexpr int AUX_EU = 8;  // estimator columns per unrolled group
// Every load below is unconditional (row and column clamped into range, the extra values
// discarded by selects or by guarded stores): a load under a branch is a round trip of its
// own, and these kernels are a few dependent round trips long.
__device__ __forceinline__ void aux_stage_p(const lgx_aux_loss_args& p, int64_t ldp, int i0, int j0, int w,
                                            float* st) {
  __syncthreads();
  const int n = HT * w;
  // k / w through a float reciprocal (k < 4096, w <= 16: the product is within 1e-3 of the
  // quotient and 1/32 of the next integer, so floor is exact) — an integer division by a
  // run-time w is ~40 instructions, and one wave per SIMD pays every one of them
  const float rw = 1.f / (float)w;
  float x[AUX_CW];
#pragma unroll
  for (int u = 0; u < AUX_CW; ++u) {
    const int k = min((int)threadIdx.x + HT * u, n - 1);
    const int r = (int)(((float)k + 0.5f) * rw), j = k - r * w;
    x[u] = p.p[(int64_t)min(i0 + r, p.B - 1) * ldp + j0 + j];
  }
#pragma unroll
  for (int u = 0; u < AUX_CW; ++u) {
    const int k = (int)threadIdx.x + HT * u;
    const int r = (int)(((float)k + 0.5f) * rw), j = k - r * w;
    if (k < n) st[r * (AUX_CW + 1) + j] = x[u];
  }
  __syncthreads();
}

// sum_j (p[i, j] - a[i, j])^2 in column order for row i = i0 + threadIdx.x (block-uniform call;
// rows past B return a value of a clamped row, unused)
__device__ __forceinline__ float aux_row_sq(const lgx_aux_loss_args& p, int64_t ldp, int i0, float* st) {
  const int64_t ic = min(i0 + (int)threadIdx.x, p.B - 1);
  float s = 0.f;
  for (int j0 = 0; j0 < p.L; j0 += AUX_CW) {
    const int w = min(AUX_CW, p.L - j0);
    float a[AUX_CW];
#pragma unroll
    for (int j = 0; j < AUX_CW; ++j) a[j] = p.a[ic * p.L + j0 + min(j, w - 1)];
    aux_stage_p(p, ldp, i0, j0, w, st);
#pragma unroll
    for (int j = 0; j < AUX_CW; ++j) {
      const float d = st[threadIdx.x * (AUX_CW + 1) + j] - a[j];
      s = j < w ? s + d * d : s;
    }
  }
  return s;
}

// sum_j (e[i, j] - t[i, j])^2 in column order
__device__ __forceinline__ float aux_est_sq(const lgx_aux_loss_args& p, int64_t i) {
  float q = 0.f;
  for (int j0 = 0; j0 < p.E; j0 += AUX_EU) {
    float e[AUX_EU], t[AUX_EU];
#pragma unroll
    for (int u = 0; u < AUX_EU; ++u) {
      const int64_t c = i * p.E + min(j0 + u, p.E - 1);
      e[u] = p.e[c];
      t[u] = p.t[c];
    }
#pragma unroll
    for (int u = 0; u < AUX_EU; ++u) {
      const float d = e[u] - t[u];
      q = j0 + u < p.E ? q + d * d : q;
    }
  }
  return q;
}

// nblk: the blocks that take part (blockIdx.x < nblk; 0: the grid's)
// st: the row staging ([HT][AUX_CW + 1] floats of LDS)
__device__ __forceinline__ void aux_loss_fused_core(const lgx_aux_loss_args& p, const lgx_heads_s8_args& s,
                                                    unsigned nblk, float* st) {
  const unsigned nb = nblk ? nblk : gridDim.x;
  if (blockIdx.x >= nb) return;
  constexpr int NV = 2 + 8;  // forward sums | de column sums (E <= 8 on the S8 path)
  __shared__ float red[4 * NV];
  const int i0 = blockIdx.x * HT, i = i0 + threadIdx.x;
  const int64_t ic = min(i, p.B - 1);
  const float gr = p.g[0] / p.B, ge = p.g[1] / p.B;
  const int64_t ldp = p.ld_p > 0 ? p.ld_p : p.L;
  float v[NV];
#pragma unroll
  for (int k = 0; k < NV; ++k) v[k] = 0.f;
  const float n = sqrtf(aux_row_sq(p, ldp, i0, st));
  const float q = aux_est_sq(p, ic);
  if (i < p.B) {
    v[0] = n;
    const float nq = sqrtf(q);  // torch: norm(dim=1).pow(2)
    v[1] = nq * nq;
  }
  const float k = n > 0.f ? gr / n : 0.f;
  for (int j0 = 0; j0 < p.L; j0 += AUX_CW) {
    const int w = min(AUX_CW, p.L - j0);
    float a[AUX_CW];
#pragma unroll
    for (int j = 0; j < AUX_CW; ++j) a[j] = p.a[ic * p.L + j0 + min(j, w - 1)];
    aux_stage_p(p, ldp, i0, j0, w, st);
#pragma unroll
    for (int j = 0; j < AUX_CW; ++j)
      if (i < p.B && j < w) p.dp[ic * p.L + j0 + j] = k * (st[threadIdx.x * (AUX_CW + 1) + j] - a[j]);
  }
  float de[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const int64_t c = ic * p.E + min(u, p.E - 1);
    de[u] = u < p.E && i < p.B ? ge * 2.f * (p.e[c] - p.t[c]) : 0.f;
    v[2 + u] = de[u];
  }
  if (i < p.B) {
    if (p.de)
      for (int u = 0; u < p.E; ++u) p.de[ic * p.E + u] = de[u];
    if (s.de_s8) store_s8_group(static_cast<char*>(s.de_s8) + ic * s.ld_de * 4, de);
  }
  block_sum<NV>(v, red);
  if (threadIdx.x == 0) {
    p.ws[blockIdx.x * 2] = v[0];
    p.ws[blockIdx.x * 2 + 1] = v[1];
    if (s.de_cs)
      for (int u = 0; u < p.E; ++u) s.de_cs[(int64_t)blockIdx.x * p.E + u] = v[2 + u];
  }
  if (last_block(p.counter, nb)) {
    float t[2];
    final_sum<2>(p.ws, 2, nb, t, red);
    if (threadIdx.x == 0) {
      p.out[0] = t[0] / p.B;
      p.out[1] = t[1] / p.B;
      *p.counter = 0u;
    }
  }
}


// ---- a whole row by one thread (lgx_loss_heads_fused): the same pieces, a row's sums serial.
// A row's inputs of the PPO head besides mu and the value (columns past A repeat the last one)
template <int NA>
struct HeadIn {
  float act[NA], os[NA], om[NA];
  float old_logp, adv, tv, R;
  __device__ __forceinline__ void load(const lgx_ppo_head_args& p, int i) {
    load_cols(p.actions, i, p.A, act);
    load_cols(p.old_sigma, i, p.A, os);
    load_cols(p.old_mu, i, p.A, om);
    old_logp = p.old_logp[i];
    adv = p.adv[i];
    tv = p.clipped_value ? p.target_values[i] : 0.f;
    R = p.returns[i];
  }
};

// One row of the fused PPO head (forward sums into v, input gradients dmu / dv, the S8 / fp32
// gradient rows and the decisions): mu and the value come from the caller.
template <int NA>
__device__ __forceinline__ void head_fused_row(const lgx_ppo_head_args& p, const lgx_heads_s8_args& s, int i,
                                               const float* stdv, const float* lstd, const float (&mu)[NA], float val,
                                               const HeadIn<NA>& x, float gs, float gv, float (&v)[3 + 2 * NA + 1],
                                               float (&dmu)[NA], float& dv) {
  float lp = 0.f, kl = 0.f;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const float t = lp_term(x.act[j], mu[j], stdv[j], lstd[j]);
    lp = j < p.A ? lp + t : lp;
  }
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    const float t = kl_term(x.om[j], x.os[j], mu[j], stdv[j]);
    kl = j < p.A ? kl + t : kl;
  }
  unsigned din;
  const bool forced = decisions_forced(s, i, din);
  float surr, dlogp, vloss;
  const unsigned own = actor_row(lp, x.old_logp, x.adv, p.clip, gs, forced, din, surr, dlogp) |
                       critic_row(val, x.R, x.tv, p.clip, p.clipped_value != 0, gv, forced, din, vloss, dv);
  if (s.decisions_out) s.decisions_out[i] = (uint8_t)own;
  v[0] += surr;
  v[1] += vloss;
  v[2] += kl;
#pragma unroll
  for (int j = 0; j < NA; ++j) {
    float dm, ds;
    dmu_term(dlogp, x.act[j], mu[j], stdv[j], dm, ds);
    dmu[j] = j < p.A ? dm : 0.f;
    if (j < p.A) {
      if (p.dmu) p.dmu[(int64_t)i * p.A + j] = dmu[j];
      v[3 + j] += ds;
      v[3 + NA + j] += dmu[j];
    }
  }
  if (p.dvalue) p.dvalue[i] = dv;
  v[3 + 2 * NA] += dv;
  if (s.dmu_s8) {
#pragma unroll
    for (int g0 = 0; g0 < NA; g0 += 8) {
      if (g0 >= p.A) break;
      float q[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = g0 + e < NA ? dmu[g0 + e] : 0.f;
      store_s8_group(static_cast<char*>(s.dmu_s8) + ((int64_t)i * s.ld_dmu + g0) * 4, q);
    }
  }
  if (s.dvalue_s8) {
    const float q[8] = {dv, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    store_s8_group(static_cast<char*>(s.dvalue_s8) + (int64_t)i * s.ld_dvalue * 4, q);
  }
}

}  // namespace lgxh
#endif
