// VIOLIN head (gfx950): the classifier tail behind the MLP's LayerNorm (linear_2 -> sigmoid -> binary_cross_entropy,
// model/violin.py:73-81, with eval_violin.py's loss / accuracy sums), forward and backward, one kernel each.  The head's
// other kernel, the masked attention pool over the frames (hero_frame_pool_*), is one of the pools of pool.hip.
//
// Classifier tail.  h [S, K] is the LayerNorm output; z = <h, w> + b is one wave per row.  The loss is the stable
// min(softplus(-+z), 100): what binary_cross_entropy(sigmoid(z), t) computes wherever fp32 sigmoid has not saturated, with
// its clamp at 100 - and past saturation the gradient stays sigmoid(z) - t instead of the reference's 0.
// Forward is ONE workgroup (rows strided over its 4 waves, per-wave sums folded in wave order); backward is
// column-parallel threads that loop s.  Both fold over s in a fixed order.
#include "common.h"

namespace hero {
namespace {

constexpr int BCE_MAX_K = 2048;
constexpr float BCE_CLAMP = 100.f;                   // binary_cross_entropy clamps log() at -100

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

int bce_check(const char* what, int S, int K, int dtype) {
  HERO_REQUIRE(S >= 1 && K >= 4 && K <= BCE_MAX_K && K % 4 == 0,
               "%s: outside the envelope (S >= 1, K %% 4 == 0, 4 <= K <= %d): S=%d K=%d", what, BCE_MAX_K, S, K);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_bce_head_fwd(const void* h, const float* w, const float* b, const long long* targets, float* logits, float* loss,
                                 float* acc, int S, int K, int dtype, hero_stream_t stream) {
  if (const int rc = bce_check("hero_bce_head_fwd", S, K, dtype)) return rc;
  HERO_REQUIRE(h && w && b && targets && logits && loss, "hero_bce_head_fwd: null pointer");
  return by_dtype(dtype, "hero_bce_head_fwd", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((bce_head_fwd_kernel<T>), dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const T*>(h), w, b,
                       targets, logits, loss, acc, S, K);
  });
}

extern "C" int hero_bce_head_bwd(const void* h, const float* w, const float* logits, const long long* targets, const float* dloss,
                                 void* dh, float* dw, float* db, int S, int K, int dtype, hero_stream_t stream) {
  if (const int rc = bce_check("hero_bce_head_bwd", S, K, dtype)) return rc;
  HERO_REQUIRE(h && w && logits && targets && dloss && dh && dw && db, "hero_bce_head_bwd: null pointer");
  return by_dtype(dtype, "hero_bce_head_bwd", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((bce_head_bwd_kernel<T>), dim3((K / 4 + 63) / 64), dim3(64), 0, static_cast<hipStream_t>(stream),
                       static_cast<const T*>(h), w, logits, targets, dloss, static_cast<T*>(dh), dw, db, S, K);
  });
}
