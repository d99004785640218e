// The passes of the masked attention pools (pool.hip: query pool and frame pool; qa_pool.hip: the two-axis video-QA pool).
// The operator: a score <x[l], w> per row, mask_logits, a softmax over one axis, the weighted row sum - and its backward.
// One workgroup of 256 threads (4 waves) owns everything one softmax couples:
//   pass 1  one wave per row: the dot products of the row with N vectors from ONE read of the row (forward: the score
//           weights; backward: the pooled gradients), 16-byte loads, DPP wave sums, one float per row and vector into an
//           LDS table (written by lane 0, read as a broadcast or one dword per lane: no bank is hit twice in a lane group)
//   pass 2  one wave per softmax row: mask_logits and the softmax over the table, or its backward times d mask_logits / ds = mask
//   pass 3  one thread per 4 columns walks the rows again (L2-resident): the weighted sums / the row gradient and the
//           workgroup's share of the parameter gradient (the caller folds the shares in a fixed order: no fp atomics)
// Device inline helpers only; the LDS tables come in by pointer, so static and dynamic LDS both work.
#pragma once
#include "common.h"

namespace hero {

// VSM: the ONE arithmetic switch of the pools.  The pools were written one task at a time and their arithmetic drifted:
//   true   (hero_query_pool_*)                     __expf, p = e * (1.f / sum), d row = fmaf(p, g, ds * w)
//   false  (hero_frame_pool_*, hero_qa_pool_*)     expf,   p = e / sum,         d row = p * g + ds * w
// It exists only so that folding the three copies into one body moved no result bit.  Nobody chose the difference; taking
// the switch out (one arithmetic for all) changes results and is a behaviour change for a pull request of its own.
template <bool VSM> __device__ __forceinline__ float pool_exp(float x) { return VSM ? __expf(x) : expf(x); }
template <bool VSM> __device__ __forceinline__ float4 pool_drow(float p, float4 g, float ds, float4 w) {
  if (VSM) return make_float4(fmaf(p, g.x, ds * w.x), fmaf(p, g.y, ds * w.y), fmaf(p, g.z, ds * w.z), fmaf(p, g.w, ds * w.w));
  return make_float4(p * g.x + ds * w.x, p * g.y + ds * w.y, p * g.z + ds * w.z, p * g.w + ds * w.w);
}

// mask_logits, model/modeling_utils.py:42-43
__device__ __forceinline__ float mask_logits(float s, float m) { return s * m + (1.f - m) * -10000.f; }

// pass 1: out[n] = <row, v[n]> for one row of D elements; the whole wave calls it, the results are wave-uniform
template <typename T, int N>
__device__ __forceinline__ void row_dots(const T* row, const float* const (&v)[N], int D, float (&out)[N]) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = 0.f;
  for (int d = lane * 4; d < D; d += 256) {
    const float4 xv = V4<T>::ld(row + d);
#pragma unroll
    for (int n = 0; n < N; ++n) out[n] += dot4(xv, ldf4(v[n] + d));
  }
#pragma unroll
  for (int n = 0; n < N; ++n) out[n] = wave_sum(out[n]);
}
template <typename T> __device__ __forceinline__ float row_dot(const T* row, const float* v, int D) {
  const float* const vs[1] = {v};
  float out[1];
  row_dots<T, 1>(row, vs, D, out);
  return out[0];
}

// pass 2, forward: one wave turns the L scores of t (LDS) into the softmax of their mask_logits, in place and into att (global).
// The mask is applied here, one coalesced read by the wave: read by lane 0 behind each row's wave sum in pass 1, it put one more
// memory round trip into every row of that pass.  A fully masked row holds L equal scores and comes out as exactly 1 / L each.
template <bool VSM> __device__ __forceinline__ void softmax_row(float* t, const float* mask, float* att, int L) {
  const int lane = threadIdx.x & 63;
  float mx = -3.0e38f;
  for (int l = lane; l < L; l += 64) {
    const float sc = mask_logits(t[l], mask[l]);
    t[l] = sc;
    mx = fmaxf(mx, sc);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int l = lane; l < L; l += 64) sum += pool_exp<VSM>(t[l] - mx);
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int l = lane; l < L; l += 64) {
    const float e = pool_exp<VSM>(t[l] - mx);
    const float p = VSM ? e * inv : e / sum;
    t[l] = p;
    att[l] = p;
  }
}

// pass 2, backward: d score from d att through the softmax (dot = <att, d att> over the softmax axis) and mask_logits
__device__ __forceinline__ float softmax_bwd(float att, float datt, float dot, float m) { return att * (datt - dot) * m; }
// ... for one wave and the L entries of t (LDS, d att in, d score out); att and mask may be LDS or global
__device__ __forceinline__ void softmax_bwd_row(float* t, const float* att, const float* mask, int L) {
  const int lane = threadIdx.x & 63;
  float dot = 0.f;
  for (int l = lane; l < L; l += 64) dot += att[l] * t[l];
  dot = wave_sum(dot);
  for (int l = lane; l < L; l += 64) t[l] = softmax_bwd(att[l], t[l], dot, mask[l]);
}

// The token rows behind the frames take no gradient from a pool: n contiguous elements (a multiple of 4) written as zeros
// by the whole workgroup, so the caller does no memset
template <typename T> __device__ __forceinline__ void zero_rows(T* p, int n) {
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = threadIdx.x * 4; i < n; i += 1024) V4<T>::st(p + i, z);
}

}  // namespace hero
