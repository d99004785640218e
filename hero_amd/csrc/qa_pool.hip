// Video-QA head (gfx950): the two attention pools of HeroForVideoQA.get_modularized_video (model/videoQA.py:36-59),
// forward and backward, one kernel each.
//
// X[v, a, l, :] are the FRAME rows of the temporal-transformer output of answer copy a of video v, read where the
// encoder left them: sequence (v * A + a) of a [Nv * A, Lt, D] buffer whose rows l < L are frames (the QA tokens sit
// behind them and are never touched).  Two bias-free Linear(D, 1) score every row; one score table is soft-maxed
// over the frames of each copy (-> one pooled vector per answer), the other over the copies of each frame (-> one
// pooled vector per frame).  Written as tensor ops that is 2 matvecs, 2 mask_logits, 2 softmaxes and 2 einsums over
// a [Nv, A, L, D] slice copy - and their backward.
//
// One workgroup (4 waves) owns one video: the A * L rows of a video are all that either softmax couples.  The passes
// are those of pool_rows.h, with what two tables change:
//   pass 1  both dot products from ONE read of the row (forward: w_qa, w_se; backward: dqa[a], dse[l]) into two LDS
//           tables of A * L floats (<= 8 KB each)
//   pass 2  over l one wave per copy (pool_rows.h), over a one thread per frame (here)
//   pass 3  <= 8 * 256 rows of <= 4 KB: both weighted sums / the row gradient and both parameter-gradient shares, A
//           independent loads in flight per frame.  The A accumulators are a fully unrolled register array (A <= 8):
//           no scratch.
// Parameter gradients leave as one [D] share per video; the caller folds them in a fixed order (hero_colsum), so
// there is no floating-point atomic and two runs give the same bits.  The arithmetic is pool_rows.h's VSM = false.
#include "pool_rows.h"

namespace hero {
namespace {

constexpr int QA_MAX_A = 8, QA_MAX_L = 256, QA_MAX_LT = 512, QA_MAX_D = 1024;

struct QaPoolArgs {
  const void* x;            // [Nv * A, Lt, D] dtype
  const float* mask;        // [Nv * A, L] 0/1
  const float* w_qa;        // [D]
  const float* w_se;        // [D]
  float* qa_pooled;         // fwd out [Nv, A, D]
  float* se_pooled;         // fwd out [Nv, L, D]
  float* att_qa;            // fwd out / bwd in [Nv, A, L]  softmax over l
  float* att_se;            // fwd out / bwd in [Nv, A, L]  softmax over a
  const float* dqa;         // bwd in [Nv, A, D]
  const float* dse;         // bwd in [Nv, L, D]
  void* dx;                 // bwd out [Nv * A, Lt, D] dtype, rows >= L zero
  float* dw_qa;             // bwd out [Nv, D] per-video shares
  float* dw_se;             // bwd out [Nv, D]
  int A, L, Lt, D;
};

template <typename T>
__global__ __launch_bounds__(256) void qa_pool_fwd_kernel(QaPoolArgs a) {
  __shared__ float t_qa[QA_MAX_A * QA_MAX_L];        // scores, then attention, [a * L + l]
  __shared__ float t_se[QA_MAX_A * QA_MAX_L];
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A, L = a.L, D = a.D, rows = A * L;
  const size_t seq = (size_t)a.Lt * D;               // elements between two answer copies
  const T* x = static_cast<const T*>(a.x) + (size_t)v * A * seq;
  const float* mask = a.mask + (size_t)v * rows;

  for (int r = wave; r < rows; r += 4) {             // pass 1: r = ai * L + l
    const int ai = r / L, l = r - ai * L;
    const float* const w[2] = {a.w_qa, a.w_se};
    float s[2];
    row_dots<T, 2>(x + ai * seq + (size_t)l * D, w, D, s);
    if (lane == 0) {
      t_qa[r] = s[0];
      t_se[r] = s[1];
    }
  }
  __syncthreads();

  for (int ai = wave; ai < A; ai += 4)               // pass 2a: mask_logits and softmax over the frames of one copy
    softmax_row<false>(t_qa + ai * L, mask + ai * L, a.att_qa + (size_t)v * rows + ai * L, L);
  for (int l = threadIdx.x; l < L; l += 256) {       // pass 2b: the same over the copies of one frame, one thread each
    float mx = -3.0e38f;
    for (int ai = 0; ai < A; ++ai) {
      const float sc = mask_logits(t_se[ai * L + l], mask[ai * L + l]);
      t_se[ai * L + l] = sc;
      mx = fmaxf(mx, sc);
    }
    float sum = 0.f;
    for (int ai = 0; ai < A; ++ai) sum += expf(t_se[ai * L + l] - mx);
    for (int ai = 0; ai < A; ++ai) {                 // a masked frame: A equal scores -> exactly 1 / A each
      const float p = expf(t_se[ai * L + l] - mx) / sum;
      t_se[ai * L + l] = p;
      a.att_se[(size_t)v * rows + ai * L + l] = p;
    }
  }
  __syncthreads();

  const int d = threadIdx.x * 4;                     // pass 3: D <= 1024 -> at most one column quad per thread
  if (d >= D) return;
  float4 qa[QA_MAX_A];
#pragma unroll
  for (int ai = 0; ai < QA_MAX_A; ++ai) qa[ai] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int l = 0; l < L; ++l) {
    float4 se = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int ai = 0; ai < QA_MAX_A; ++ai) {
      if (ai < A) {
        const float4 xv = V4<T>::ld(x + ai * seq + (size_t)l * D + d);
        fma4(se, t_se[ai * L + l], xv);
        fma4(qa[ai], t_qa[ai * L + l], xv);
      }
    }
    stf4(a.se_pooled + ((size_t)v * L + l) * D + d, se);
  }
#pragma unroll
  for (int ai = 0; ai < QA_MAX_A; ++ai)
    if (ai < A) stf4(a.qa_pooled + ((size_t)v * A + ai) * D + d, qa[ai]);
}

template <typename T>
__global__ __launch_bounds__(256) void qa_pool_bwd_kernel(QaPoolArgs a) {
  __shared__ float t_qa[QA_MAX_A * QA_MAX_L];        // d att, then d score, [a * L + l]
  __shared__ float t_se[QA_MAX_A * QA_MAX_L];
  const int v = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int A = a.A, L = a.L, Lt = a.Lt, D = a.D, rows = A * L;
  const size_t seq = (size_t)Lt * D;
  const T* x = static_cast<const T*>(a.x) + (size_t)v * A * seq;
  T* dx = static_cast<T*>(a.dx) + (size_t)v * A * seq;
  const float* mask = a.mask + (size_t)v * rows;
  const float* att_qa = a.att_qa + (size_t)v * rows;
  const float* att_se = a.att_se + (size_t)v * rows;
  const float* dqa = a.dqa + (size_t)v * A * D;
  const float* dse = a.dse + (size_t)v * L * D;

  for (int r = wave; r < rows; r += 4) {             // pass 1: d att_qa[a,l] = <dqa[a], x>, d att_se[a,l] = <dse[l], x>
    const int ai = r / L, l = r - ai * L;
    const float* const g[2] = {dqa + (size_t)ai * D, dse + (size_t)l * D};
    float s[2];
    row_dots<T, 2>(x + ai * seq + (size_t)l * D, g, D, s);
    if (lane == 0) {
      t_qa[r] = s[0];
      t_se[r] = s[1];
    }
  }
  __syncthreads();

  for (int ai = wave; ai < A; ai += 4)               // pass 2a: softmax backward over l
    softmax_bwd_row(t_qa + ai * L, att_qa + ai * L, mask + ai * L, L);
  for (int l = threadIdx.x; l < L; l += 256) {       // pass 2b: softmax backward over a, one thread each
    float dot = 0.f;
    for (int ai = 0; ai < A; ++ai) dot += att_se[ai * L + l] * t_se[ai * L + l];
    for (int ai = 0; ai < A; ++ai) t_se[ai * L + l] = softmax_bwd(att_se[ai * L + l], t_se[ai * L + l], dot, mask[ai * L + l]);
  }
  __syncthreads();

  const int d = threadIdx.x * 4;                     // pass 3
  if (d < D) {
    const float4 wq = ldf4(a.w_qa + d), ws = ldf4(a.w_se + d);
    float4 gq[QA_MAX_A];
#pragma unroll
    for (int ai = 0; ai < QA_MAX_A; ++ai) gq[ai] = ai < A ? ldf4(dqa + (size_t)ai * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 dwq = make_float4(0.f, 0.f, 0.f, 0.f), dws = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int l = 0; l < L; ++l) {
      const float4 gs = ldf4(dse + (size_t)l * D + d);
#pragma unroll
      for (int ai = 0; ai < QA_MAX_A; ++ai) {
        if (ai < A) {
          const size_t off = ai * seq + (size_t)l * D + d;
          const float4 xv = V4<T>::ld(x + off);
          const float pq = att_qa[ai * L + l], ps = att_se[ai * L + l], sq = t_qa[ai * L + l], ss = t_se[ai * L + l];
          float4 g;
          g.x = (pq * gq[ai].x + ps * gs.x) + (sq * wq.x + ss * ws.x);
          g.y = (pq * gq[ai].y + ps * gs.y) + (sq * wq.y + ss * ws.y);
          g.z = (pq * gq[ai].z + ps * gs.z) + (sq * wq.z + ss * ws.z);
          g.w = (pq * gq[ai].w + ps * gs.w) + (sq * wq.w + ss * ws.w);
          V4<T>::st(dx + off, g);
          fma4(dwq, sq, xv);
          fma4(dws, ss, xv);
        }
      }
    }
    stf4(a.dw_qa + (size_t)v * D + d, dwq);
    stf4(a.dw_se + (size_t)v * D + d, dws);
  }
  // the QA-token rows behind the frames take no gradient from this head: written as zeros, the caller does no memset
  for (int ai = 0; ai < A; ++ai) zero_rows(dx + ai * seq + (size_t)L * D, (Lt - L) * D);   // contiguous per copy
}

int qa_check(const char* what, const void* x, int Nv, int A, int L, int Lt, int D) {
  HERO_REQUIRE(x != nullptr, "%s: null pointer", what);
  HERO_REQUIRE(Nv >= 0 && A >= 1 && A <= QA_MAX_A && L >= 1 && L <= QA_MAX_L && Lt >= L && Lt <= QA_MAX_LT && D >= 4 && D <= QA_MAX_D && D % 4 == 0,
               "%s: outside the envelope (1 <= A <= %d, 1 <= L <= %d, L <= Lt <= %d, D %% 4 == 0, D <= %d): Nv=%d A=%d L=%d Lt=%d D=%d",
               what, QA_MAX_A, QA_MAX_L, QA_MAX_LT, QA_MAX_D, Nv, A, L, Lt, D);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_qa_pool_fwd(const void* x, const float* mask, const float* w_qa, const float* w_se, float* qa_pooled, float* se_pooled,
                                float* att_qa, float* att_se, int Nv, int A, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = qa_check("hero_qa_pool_fwd", x, Nv, A, L, Lt, D)) return rc;
  HERO_REQUIRE(mask && w_qa && w_se && qa_pooled && se_pooled && att_qa && att_se, "hero_qa_pool_fwd: null pointer");
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "hero_qa_pool_fwd: bad dtype %d", dtype);
  if (Nv == 0) return HERO_OK;
  QaPoolArgs a = {};
  a.x = x; a.mask = mask; a.w_qa = w_qa; a.w_se = w_se;
  a.qa_pooled = qa_pooled; a.se_pooled = se_pooled; a.att_qa = att_qa; a.att_se = att_se;
  a.A = A; a.L = L; a.Lt = Lt; a.D = D;
  return by_dtype(dtype, "hero_qa_pool_fwd", [&](auto tag) {
    hipLaunchKernelGGL((qa_pool_fwd_kernel<typename decltype(tag)::type>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  });
}

extern "C" int hero_qa_pool_bwd(const void* x, const float* mask, const float* w_qa, const float* w_se, const float* att_qa, const float* att_se,
                                const float* dqa, const float* dse, void* dx, float* dw_qa, float* dw_se,
                                int Nv, int A, int L, int Lt, int D, int dtype, hero_stream_t stream) {
  if (const int rc = qa_check("hero_qa_pool_bwd", x, Nv, A, L, Lt, D)) return rc;
  HERO_REQUIRE(mask && w_qa && w_se && att_qa && att_se && dqa && dse && dx && dw_qa && dw_se, "hero_qa_pool_bwd: null pointer");
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "hero_qa_pool_bwd: bad dtype %d", dtype);
  if (Nv == 0) return HERO_OK;
  QaPoolArgs a = {};
  a.x = x; a.mask = mask; a.w_qa = w_qa; a.w_se = w_se;
  a.att_qa = const_cast<float*>(att_qa); a.att_se = const_cast<float*>(att_se);
  a.dqa = dqa; a.dse = dse; a.dx = dx; a.dw_qa = dw_qa; a.dw_se = dw_se;
  a.A = A; a.L = L; a.Lt = Lt; a.D = D;
  return by_dtype(dtype, "hero_qa_pool_bwd", [&](auto tag) {
    hipLaunchKernelGGL((qa_pool_bwd_kernel<typename decltype(tag)::type>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  });
}
