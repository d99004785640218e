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
// One workgroup (4 waves) owns one video: the A * L rows of a video are all that either softmax couples.
//   pass 1  one wave per row: both dot products from ONE read of the row (forward: w_qa, w_se; backward: dqa[a],
//           dse[l]), DPP butterfly sums, results into two LDS tables of A * L floats (<= 8 KB each)
//   pass 2  the two softmaxes (or their backward) in the LDS: over l one wave per copy, over a one thread per frame
//   pass 3  one thread per 4 columns walks the rows again (L2-resident: <= 8 * 256 rows of <= 4 KB): both weighted
//           sums / the row gradient and both parameter-gradient shares, 16-byte accesses, A independent loads in
//           flight per frame.  The A accumulators are a fully unrolled register array (A <= 8): no scratch.
// Parameter gradients leave as one [D] share per video; the caller folds them in a fixed order (hero_colsum), so
// there is no floating-point atomic and two runs give the same bits.
#include "common.h"

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

__device__ __forceinline__ float dot4(float4 a, float4 b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
__device__ __forceinline__ void fma4(float4& acc, float s, float4 v) {
  acc.x = fmaf(s, v.x, acc.x); acc.y = fmaf(s, v.y, acc.y); acc.z = fmaf(s, v.z, acc.z); acc.w = fmaf(s, v.w, acc.w);
}
__device__ __forceinline__ float4 ldf4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void stf4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

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
    const T* row = x + ai * seq + (size_t)l * D;
    float sq = 0.f, ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
      const float4 xv = V4<T>::ld(row + d);
      sq += dot4(xv, ldf4(a.w_qa + d));
      ss += dot4(xv, ldf4(a.w_se + d));
    }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if (lane == 0) {
      const float m = mask[r];
      t_qa[r] = sq * m + (1.f - m) * -10000.f;       // mask_logits, model/modeling_utils.py:42-43
      t_se[r] = ss * m + (1.f - m) * -10000.f;
    }
  }
  __syncthreads();

  for (int ai = wave; ai < A; ai += 4) {             // pass 2a: softmax over the frames of one copy
    float* s = t_qa + ai * L;
    float mx = -3.0e38f;
    for (int l = lane; l < L; l += 64) mx = fmaxf(mx, s[l]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int l = lane; l < L; l += 64) sum += expf(s[l] - mx);
    sum = wave_sum(sum);
    for (int l = lane; l < L; l += 64) {
      const float p = expf(s[l] - mx) / sum;
      s[l] = p;
      a.att_qa[(size_t)v * rows + ai * L + l] = p;
    }
  }
  for (int l = threadIdx.x; l < L; l += 256) {       // pass 2b: softmax over the copies of one frame
    float mx = -3.0e38f;
    for (int ai = 0; ai < A; ++ai) mx = fmaxf(mx, t_se[ai * L + l]);
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
    const T* row = x + ai * seq + (size_t)l * D;
    float sq = 0.f, ss = 0.f;
    for (int d = lane * 4; d < D; d += 256) {
      const float4 xv = V4<T>::ld(row + d);
      sq += dot4(xv, ldf4(dqa + (size_t)ai * D + d));
      ss += dot4(xv, ldf4(dse + (size_t)l * D + d));
    }
    sq = wave_sum(sq);
    ss = wave_sum(ss);
    if (lane == 0) {
      t_qa[r] = sq;
      t_se[r] = ss;
    }
  }
  __syncthreads();

  for (int ai = wave; ai < A; ai += 4) {             // pass 2a: softmax backward over l, times d mask_logits / ds = mask
    float dot = 0.f;
    for (int l = lane; l < L; l += 64) dot += att_qa[ai * L + l] * t_qa[ai * L + l];
    dot = wave_sum(dot);
    for (int l = lane; l < L; l += 64) t_qa[ai * L + l] = att_qa[ai * L + l] * (t_qa[ai * L + l] - dot) * mask[ai * L + l];
  }
  for (int l = threadIdx.x; l < L; l += 256) {       // pass 2b: softmax backward over a
    float dot = 0.f;
    for (int ai = 0; ai < A; ++ai) dot += att_se[ai * L + l] * t_se[ai * L + l];
    for (int ai = 0; ai < A; ++ai) t_se[ai * L + l] = att_se[ai * L + l] * (t_se[ai * L + l] - dot) * mask[ai * L + l];
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
  const int tail = (Lt - L) * D;                     // contiguous per copy, a multiple of 4 elements
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int ai = 0; ai < A; ++ai) {
    T* p = dx + ai * seq + (size_t)L * D;
    for (int i = threadIdx.x * 4; i < tail; i += 1024) V4<T>::st(p + i, z);
  }
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
  if (dtype == HERO_F32) hipLaunchKernelGGL((qa_pool_fwd_kernel<float>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL((qa_pool_fwd_kernel<bf16_t>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("hero_qa_pool_fwd");
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
  if (dtype == HERO_F32) hipLaunchKernelGGL((qa_pool_bwd_kernel<float>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  else hipLaunchKernelGGL((qa_pool_bwd_kernel<bf16_t>), dim3(Nv), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("hero_qa_pool_bwd");
}
