// Single-axis attention pools (gfx950), forward and backward, one kernel each for both users:
//   hero_query_pool_*  QueryFeatEncoder.get_modularized_queries (model/encoder.py:460-471): rows [B, L, D], any L <= 4096
//   hero_frame_pool_*  HeroForViolin.get_modularized_video (model/violin.py:30-47): x[s, l, :], l < L, are the FRAME rows
//                      of sequence s of the temporal-transformer output [S, Lt, D], read where the encoder left them (the
//                      statement tokens behind them are never touched; their gradient rows are written as zeros)
// The query pool is the frame pool with Lt = L.  One workgroup owns one sequence; the three passes are in pool_rows.h.
// dw leaves as one [D] share per sequence; the caller folds them in a fixed order (hero_colsum): no floating-point atomic,
// two runs give the same bits.
#include "pool_rows.h"

namespace hero {
namespace {

constexpr int FP_MAX_L = 256, FP_MAX_LT = 512, FP_MAX_D = 1024;

// VSM: pool_rows.h
template <typename T, bool VSM>
__global__ __launch_bounds__(256) void pool_fwd_kernel(const T* __restrict__ x, const float* __restrict__ mask,
                                                       const float* __restrict__ w, float* __restrict__ pooled,
                                                       float* __restrict__ att, int L, int Lt, int D) {
  extern __shared__ float t[];                       // [L] scores, then attention
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  x += (size_t)s * Lt * D;
  mask += (size_t)s * L;
  for (int l = wave; l < L; l += 4) {
    const float sc = row_dot<T>(x + (size_t)l * D, w, D);
    if (lane == 0) t[l] = sc;
  }
  __syncthreads();
  if (wave == 0) softmax_row<VSM>(t, mask, att + (size_t)s * L, L);
  __syncthreads();
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int l = 0; l < L; ++l) fma4(acc, t[l], V4<T>::ld(x + (size_t)l * D + d));
    stf4(pooled + (size_t)s * D + d, acc);
  }
}

template <typename T, bool VSM>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const T* __restrict__ x, const float* __restrict__ mask,
                                                       const float* __restrict__ w, const float* __restrict__ att,
                                                       const float* __restrict__ dpooled, T* __restrict__ dx,
                                                       float* __restrict__ dw_part, int L, int Lt, int D) {
  extern __shared__ float sm[];
  float* t = sm;                                     // [L] d att, then d score
  float* p = sm + L;                                 // [L] attention
  const int s = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  x += (size_t)s * Lt * D;
  dx += (size_t)s * Lt * D;
  mask += (size_t)s * L;
  att += (size_t)s * L;
  dpooled += (size_t)s * D;
  for (int l = wave; l < L; l += 4) {                // d att[l] = <dpooled[s], x[l]>
    const float da = row_dot<T>(x + (size_t)l * D, dpooled, D);
    if (lane == 0) t[l] = da;
  }
  __syncthreads();
  if (wave == 0) {
    for (int l = lane; l < L; l += 64) p[l] = att[l];
    softmax_bwd_row(t, p, mask, L);
  }
  __syncthreads();
  for (int d = threadIdx.x * 4; d < D; d += 1024) {
    const float4 wv = ldf4(w + d), g = ldf4(dpooled + d);
    float4 dw = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
    for (int l = 0; l < L; ++l) {
      const size_t off = (size_t)l * D + d;
      const float4 xv = V4<T>::ld(x + off);
      const float ds = t[l];
      V4<T>::st(dx + off, pool_drow<VSM>(p[l], g, ds, wv));
      fma4(dw, ds, xv);
    }
    if (dw_part) stf4(dw_part + (size_t)s * D + d, dw);
  }
  zero_rows(dx + (size_t)L * D, (Lt - L) * D);       // Lt - L < 512 rows of D <= 1024: < 2^19 elements
}

template <bool VSM>
int launch_fwd(const char* what, const void* x, const float* mask, const float* w, float* pooled, float* att, int S, int L, int Lt, int D,
               int dtype, hero_stream_t stream) {
  return by_dtype(dtype, what, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((pool_fwd_kernel<T, VSM>), dim3(S), dim3(256), L * sizeof(float), static_cast<hipStream_t>(stream),
                       static_cast<const T*>(x), mask, w, pooled, att, L, Lt, D);
  });
}
template <bool VSM>
int launch_bwd(const char* what, const void* x, const float* mask, const float* w, const float* att, const float* dpooled, void* dx,
               float* dw_part, int S, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  return by_dtype(dtype, what, [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL((pool_bwd_kernel<T, VSM>), dim3(S), dim3(256), 2 * L * sizeof(float), static_cast<hipStream_t>(stream),
                       static_cast<const T*>(x), mask, w, att, dpooled, static_cast<T*>(dx), dw_part, L, Lt, D);
  });
}

int frame_check(const char* what, int S, int L, int Lt, int D, int dtype) {
  HERO_REQUIRE(S >= 0 && L >= 1 && L <= FP_MAX_L && Lt >= L && Lt <= FP_MAX_LT && D >= 4 && D <= FP_MAX_D && D % 4 == 0,
               "%s: outside the envelope (S >= 0, 1 <= L <= %d, L <= Lt <= %d, D %% 4 == 0, 4 <= D <= %d): S=%d L=%d Lt=%d D=%d",
               what, FP_MAX_L, FP_MAX_LT, FP_MAX_D, S, L, Lt, D);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_query_pool_fwd(const HeroQueryPool* a, hero_stream_t stream) {
  HERO_REQUIRE(a && a->q && a->mask && a->w && a->pooled && a->att, "hero_query_pool_fwd: null pointer");
  HERO_REQUIRE(a->L > 0 && a->L <= 4096 && a->D > 0 && a->D % 4 == 0, "hero_query_pool_fwd: bad dims L=%d D=%d", a->L, a->D);
  if (a->B <= 0) return HERO_OK;
  return launch_fwd<true>("hero_query_pool_fwd", a->q, a->mask, a->w, a->pooled, a->att, a->B, a->L, a->L, a->D, a->dtype, stream);
}
extern "C" int hero_query_pool_bwd(const HeroQueryPool* a, hero_stream_t stream) {
  HERO_REQUIRE(a && a->q && a->mask && a->w && a->att && a->dpooled && a->dq, "hero_query_pool_bwd: null pointer");
  HERO_REQUIRE(a->L > 0 && a->L <= 4096 && a->D > 0 && a->D % 4 == 0, "hero_query_pool_bwd: bad dims L=%d D=%d", a->L, a->D);
  if (a->B <= 0) return HERO_OK;
  // dw: [B, D] partial sums, one row per query, or none
  return launch_bwd<true>("hero_query_pool_bwd", a->q, a->mask, a->w, a->att, a->dpooled, a->dq, a->dw, a->B, a->L, a->L, a->D, a->dtype,
                          stream);
}

extern "C" int hero_frame_pool_fwd(const void* x, const float* mask, const float* w, float* pooled, float* att,
                                   int S, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = frame_check("hero_frame_pool_fwd", S, L, Lt, D, dtype)) return rc;
  if (S == 0) return HERO_OK;
  HERO_REQUIRE(x && mask && w && pooled && att, "hero_frame_pool_fwd: null pointer");
  return launch_fwd<false>("hero_frame_pool_fwd", x, mask, w, pooled, att, S, L, Lt, D, dtype, stream);
}

extern "C" int hero_frame_pool_bwd(const void* x, const float* mask, const float* w, const float* att, const float* dpooled,
                                   void* dx, float* dw_part, int S, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = frame_check("hero_frame_pool_bwd", S, L, Lt, D, dtype)) return rc;
  if (S == 0) return HERO_OK;
  HERO_REQUIRE(x && mask && w && att && dpooled && dx && dw_part, "hero_frame_pool_bwd: null pointer");
  return launch_bwd<false>("hero_frame_pool_bwd", x, mask, w, att, dpooled, dx, dw_part, S, L, Lt, D, dtype, stream);
}
