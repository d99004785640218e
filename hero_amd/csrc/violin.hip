// VIOLIN head (gfx950): the masked attention pool over the frames of each (video, statement) copy
// (HeroForViolin.get_modularized_video, model/violin.py:30-47) and the classifier tail behind the MLP's LayerNorm
// (linear_2 -> sigmoid -> binary_cross_entropy, model/violin.py:73-81, with eval_violin.py's loss / accuracy sums),
// forward and backward, one kernel each.
//
// Frame pool.  x[s, l, :], l < L, are the FRAME rows of sequence s of the temporal-transformer output [S, Lt, D], read
// where the encoder left them (the statement tokens behind them are never touched).  One workgroup (4 waves) owns one
// sequence - the softmax couples nothing else:
//   pass 1  one wave per row: the dot product with w (forward) / dpooled[s] (backward), 16-byte loads, DPP wave sum,
//           one float per row into an LDS table (<= 1 KB; it is written by lane 0 and read as a broadcast or one dword
//           per lane, so no bank is hit twice in a lane group)
//   pass 2  wave 0: the softmax over l, or its backward times d mask_logits / ds = mask
//   pass 3  one thread per 4 columns walks the L rows again (L2-resident, <= 256 rows of <= 4 KB): the weighted sum /
//           the row gradient and this sequence's share of dw
// dw leaves as one [D] share per sequence; the caller folds them in a fixed order (hero_colsum): no floating-point
// atomic, two runs give the same bits.
//
// Classifier tail.  h [S, K] is the LayerNorm output; z = <h, w> + b is one wave per row.  The loss is the stable
// min(softplus(-+z), 100): what binary_cross_entropy(sigmoid(z), t) computes wherever fp32 sigmoid has not saturated, with
// its clamp at 100 - and past saturation the gradient stays sigmoid(z) - t instead of the reference's 0.
// Forward is ONE workgroup (rows strided over its 4 waves, per-wave sums folded in wave order); backward is
// column-parallel threads that loop s.  Both fold over s in a fixed order.
#include "common.h"

namespace hero {
namespace {

constexpr int FP_MAX_L = 256, FP_MAX_LT = 512, FP_MAX_D = 1024, BCE_MAX_K = 2048;
constexpr float BCE_CLAMP = 100.f;                   // binary_cross_entropy clamps log() at -100

__device__ __forceinline__ float dot4(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
  acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}
__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

// table[l] = <x[l, :], v> for the L frame rows of one sequence, one wave per row
template <typename T>
__device__ __forceinline__ void row_dots(const T* x, const float* v, float* table, int L, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int l = wave; l < L; l += 4) {
    const T* row = x + (size_t)l * D;
    float s = 0.f;
    for (int d = lane * 4; d < D; d += 256) s += dot4(V4<T>::ld(row + d), ldf4(v + d));
    s = wave_sum(s);
    if (lane == 0) table[l] = s;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void frame_pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ mask,
                                                             const float* __restrict__ w, float* __restrict__ pooled,
                                                             float* __restrict__ att, int L, int Lt, int D) {
  __shared__ float t[FP_MAX_L];                      // scores, then attention
  const int s = blockIdx.x, lane = threadIdx.x & 63;
  x += (size_t)s * Lt * D;
  mask += (size_t)s * L;
  row_dots<T>(x, w, t, L, D);
  __syncthreads();
  if (threadIdx.x < 64) {                            // softmax over the frames; mask_logits, model/modeling_utils.py:42-43
    float mx = -3.0e38f;
    for (int l = lane; l < L; l += 64) {
      const float m = mask[l];
      const float sc = t[l] * m + (1.f - m) * -10000.f;
      t[l] = sc;
      mx = fmaxf(mx, sc);
    }
    mx = wave_max(mx);
    float sum = 0.f;
    for (int l = lane; l < L; l += 64) sum += expf(t[l] - mx);
    sum = wave_sum(sum);
    for (int l = lane; l < L; l += 64) {             // a fully masked sequence: L equal scores -> exactly 1 / L each
      const float p = expf(t[l] - mx) / sum;
      t[l] = p;
      att[(size_t)s * L + l] = p;
    }
  }
  __syncthreads();
  const int d = threadIdx.x * 4;                     // D <= 1024 -> at most one column quad per thread
  if (d >= D) return;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int l = 0; l < L; ++l) fma4(acc, t[l], V4<T>::ld(x + (size_t)l * D + d));
  stf4(pooled + (size_t)s * D + d, acc);
}

template <typename T>
__global__ __launch_bounds__(256) void frame_pool_bwd_kernel(const T* __restrict__ x, const float* __restrict__ mask,
                                                             const float* __restrict__ w, const float* __restrict__ att,
                                                             const float* __restrict__ dpooled, T* __restrict__ dx,
                                                             float* __restrict__ dw_part, int L, int Lt, int D) {
  __shared__ float t[FP_MAX_L];                      // d att, then d score
  __shared__ float p[FP_MAX_L];                      // attention
  const int s = blockIdx.x, lane = threadIdx.x & 63;
  x += (size_t)s * Lt * D;
  dx += (size_t)s * Lt * D;
  mask += (size_t)s * L;
  att += (size_t)s * L;
  dpooled += (size_t)s * D;
  row_dots<T>(x, dpooled, t, L, D);                  // d att[l] = <dpooled[s], x[l]>
  __syncthreads();
  if (threadIdx.x < 64) {                            // softmax backward over l, times d mask_logits / ds = mask
    float dot = 0.f;
    for (int l = lane; l < L; l += 64) {
      const float a = att[l];
      p[l] = a;
      dot += a * t[l];
    }
    dot = wave_sum(dot);
    for (int l = lane; l < L; l += 64) t[l] = p[l] * (t[l] - dot) * mask[l];
  }
  __syncthreads();
  const int d = threadIdx.x * 4;
  if (d < D) {
    const float4 wv = ldf4(w + d), g = ldf4(dpooled + d);
    float4 dw = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int l = 0; l < L; ++l) {
      const size_t off = (size_t)l * D + d;
      const float4 xv = V4<T>::ld(x + off);
      const float a = p[l], ds = t[l];
      V4<T>::st(dx + off, make_float4(a * g.x + ds * wv.x, a * g.y + ds * wv.y, a * g.z + ds * wv.z, a * g.w + ds * wv.w));
      fma4(dw, ds, xv);
    }
    stf4(dw_part + (size_t)s * D + d, dw);
  }
  // the statement-token rows behind the frames take no gradient from this head: written as zeros, the caller does no memset
  const int tail = (Lt - L) * D;                     // contiguous, a multiple of 4 elements, < 2^19
  T* q = dx + (size_t)L * D;
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x * 4; i < tail; i += 1024) V4<T>::st(q + i, z);
}

__device__ __forceinline__ float softplus(float z) { return fmaxf(z, 0.f) + log1pf(expf(-fabsf(z))); }
__device__ __forceinline__ float sigmoid(float z) {  // no overflow on either side, full relative precision in the tails
  const float e = expf(-fabsf(z));
  return (z >= 0.f ? 1.f : e) / (1.f + e);
}

template <typename T>
__global__ __launch_bounds__(256) void bce_head_fwd_kernel(const T* __restrict__ h, const float* __restrict__ w,
                                                           const float* __restrict__ b, const long long* __restrict__ targets,
                                                           float* __restrict__ logits, float* __restrict__ loss, float* acc,
                                                           int S, int K) {
  __shared__ float part[4][2];                       // per wave: sum of the loss terms, number of right predictions
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float bias = b[0];
  float sum = 0.f, hits = 0.f;                       // wave-uniform
  for (int s = wave; s < S; s += 4) {
    const T* row = h + (size_t)s * K;
    float z = 0.f;
    for (int k = lane * 4; k < K; k += 256) z += dot4(V4<T>::ld(row + k), ldf4(w + k));
    z = wave_sum(z) + bias;
    const bool one = targets[s] == 1;
    sum += fminf(softplus(one ? -z : z), BCE_CLAMP);
    hits += ((z > 0.f) == one) ? 1.f : 0.f;          // strict: z == 0 predicts 0, as sigmoid(z) > 0.5 does
    if (lane == 0) logits[s] = z;
  }
  if (lane == 0) {
    part[wave][0] = sum;
    part[wave][1] = hits;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float total = (part[0][0] + part[1][0]) + (part[2][0] + part[3][0]);
    const float right = (part[0][1] + part[1][1]) + (part[2][1] + part[3][1]);
    loss[0] = total / (float)S;
    if (acc) {                                       // stream-ordered accumulation: one writer, one launch at a time
      acc[0] += total;
      acc[1] += right;
      acc[2] += (float)S;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(64) void bce_head_bwd_kernel(const T* __restrict__ h, const float* __restrict__ w,
                                                          const float* __restrict__ logits, const long long* __restrict__ targets,
                                                          const float* __restrict__ dloss, T* __restrict__ dh,
                                                          float* __restrict__ dw, float* __restrict__ db, int S, int K) {
  const int k = (blockIdx.x * 64 + threadIdx.x) * 4;
  if (k >= K) return;
  const float scale = dloss[0] / (float)S;
  const float4 wv = ldf4(w + k);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  float sum = 0.f;
#pragma unroll 4
  for (int s = 0; s < S; ++s) {                      // dz is recomputed by every thread: S exps against a row of loads
    const float z = logits[s];
    const float dz = scale * (targets[s] == 1 ? -sigmoid(-z) : sigmoid(z));      // sigmoid(z) - t without cancellation
    const size_t off = (size_t)s * K + k;
    fma4(acc, dz, V4<T>::ld(h + off));
    V4<T>::st(dh + off, make_float4(dz * wv.x, dz * wv.y, dz * wv.z, dz * wv.w));
    sum += dz;
  }
  stf4(dw + k, acc);
  if (k == 0) db[0] = sum;
}

int pool_check(const char* what, int S, int L, int Lt, int D, int dtype) {
  HERO_REQUIRE(S >= 0 && L >= 1 && L <= FP_MAX_L && Lt >= L && Lt <= FP_MAX_LT && D >= 4 && D <= FP_MAX_D && D % 4 == 0,
               "%s: outside the envelope (S >= 0, 1 <= L <= %d, L <= Lt <= %d, D %% 4 == 0, 4 <= D <= %d): S=%d L=%d Lt=%d D=%d",
               what, FP_MAX_L, FP_MAX_LT, FP_MAX_D, S, L, Lt, D);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

int bce_check(const char* what, int S, int K, int dtype) {
  HERO_REQUIRE(S >= 1 && K >= 4 && K <= BCE_MAX_K && K % 4 == 0,
               "%s: outside the envelope (S >= 1, K %% 4 == 0, 4 <= K <= %d): S=%d K=%d", what, BCE_MAX_K, S, K);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_frame_pool_fwd(const void* x, const float* mask, const float* w, float* pooled, float* att,
                                   int S, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = pool_check("hero_frame_pool_fwd", S, L, Lt, D, dtype)) return rc;
  if (S == 0) return HERO_OK;
  HERO_REQUIRE(x && mask && w && pooled && att, "hero_frame_pool_fwd: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HERO_F32)
    hipLaunchKernelGGL((frame_pool_fwd_kernel<float>), dim3(S), dim3(256), 0, st, static_cast<const float*>(x), mask, w, pooled, att, L, Lt, D);
  else
    hipLaunchKernelGGL((frame_pool_fwd_kernel<bf16_t>), dim3(S), dim3(256), 0, st, static_cast<const bf16_t*>(x), mask, w, pooled, att, L, Lt, D);
  return check_launch("hero_frame_pool_fwd");
}

extern "C" int hero_frame_pool_bwd(const void* x, const float* mask, const float* w, const float* att, const float* dpooled,
                                   void* dx, float* dw_part, int S, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = pool_check("hero_frame_pool_bwd", S, L, Lt, D, dtype)) return rc;
  if (S == 0) return HERO_OK;
  HERO_REQUIRE(x && mask && w && att && dpooled && dx && dw_part, "hero_frame_pool_bwd: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HERO_F32)
    hipLaunchKernelGGL((frame_pool_bwd_kernel<float>), dim3(S), dim3(256), 0, st, static_cast<const float*>(x), mask, w, att, dpooled,
                       static_cast<float*>(dx), dw_part, L, Lt, D);
  else
    hipLaunchKernelGGL((frame_pool_bwd_kernel<bf16_t>), dim3(S), dim3(256), 0, st, static_cast<const bf16_t*>(x), mask, w, att, dpooled,
                       static_cast<bf16_t*>(dx), dw_part, L, Lt, D);
  return check_launch("hero_frame_pool_bwd");
}

extern "C" int hero_bce_head_fwd(const void* h, const float* w, const float* b, const long long* targets, float* logits, float* loss,
                                 float* acc, int S, int K, int dtype, hero_stream_t stream) {
  if (const int rc = bce_check("hero_bce_head_fwd", S, K, dtype)) return rc;
  HERO_REQUIRE(h && w && b && targets && logits && loss, "hero_bce_head_fwd: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HERO_F32)
    hipLaunchKernelGGL((bce_head_fwd_kernel<float>), dim3(1), dim3(256), 0, st, static_cast<const float*>(h), w, b, targets, logits, loss, acc, S, K);
  else
    hipLaunchKernelGGL((bce_head_fwd_kernel<bf16_t>), dim3(1), dim3(256), 0, st, static_cast<const bf16_t*>(h), w, b, targets, logits, loss, acc, S, K);
  return check_launch("hero_bce_head_fwd");
}

extern "C" int hero_bce_head_bwd(const void* h, const float* w, const float* logits, const long long* targets, const float* dloss,
                                 void* dh, float* dw, float* db, int S, int K, int dtype, hero_stream_t stream) {
  if (const int rc = bce_check("hero_bce_head_bwd", S, K, dtype)) return rc;
  HERO_REQUIRE(h && w && logits && targets && dloss && dh && dw && db, "hero_bce_head_bwd: null pointer");
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int blocks = (K / 4 + 63) / 64;
  if (dtype == HERO_F32)
    hipLaunchKernelGGL((bce_head_bwd_kernel<float>), dim3(blocks), dim3(64), 0, st, static_cast<const float*>(h), w, logits, targets, dloss,
                       static_cast<float*>(dh), dw, db, S, K);
  else
    hipLaunchKernelGGL((bce_head_bwd_kernel<bf16_t>), dim3(blocks), dim3(64), 0, st, static_cast<const bf16_t*>(h), w, logits, targets, dloss,
                       static_cast<bf16_t*>(dh), dw, db, S, K);
  return check_launch("hero_bce_head_bwd");
}
