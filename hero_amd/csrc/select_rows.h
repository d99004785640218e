// What the two selection kernels of the captioning decode (beam.hip, sample.hip) do to a row of prediction scores in the same
// way: the row scan, the row's log-sum-exp, the 64-bit wave maximum and the step position.  Device inline helpers only; NT is
// the workgroup's thread count.
#pragma once
#include "common.h"

namespace hero {

// f(v, x) for the elements of the row that belong to this thread: 4 consecutive ones per load where the row allows it
template <typename T, int NT, class F>
__device__ __forceinline__ void for_row(const T* row, int V, bool vec, F f) {
  if (vec) {
    const int V4n = V >> 2;
    for (int g = threadIdx.x; g < V4n; g += NT) {
      const float4 x = V4<T>::ld(row + 4 * g);
      f(4 * g, x.x); f(4 * g + 1, x.y); f(4 * g + 2, x.z); f(4 * g + 3, x.w);
    }
    const int v = (V4n << 2) + threadIdx.x;
    if (v < V) f(v, ld1<T>(row + v));
  } else {
    for (int v = threadIdx.x; v < V; v += NT) f(v, ld1<T>(row + v));
  }
}

// host: every row of a [R, ld] matrix at `base` starts on a 4-element boundary, so for_row may load 4 elements at a time
inline int rows_vec4(const void* base, int ld, int dtype) {
  const size_t es = dtype == HERO_F32 ? 4 : 2;
  return (ld % 4 == 0 && (((uintptr_t)base) & (4 * es - 1)) == 0) ? 1 : 0;
}

struct RowLse {
  float max, lse;                // the row's maximum and max + log(sum exp(x - max))
};

// The log-sum-exp of a row: maximum and sum online per thread, folded over the wave on the DPP network and over the NT / 64
// waves in a fixed order through red_m / red_s (LDS, float[NT / 64] each).  All NT threads call it together; it holds one barrier.
template <typename T, int NT>
__device__ __forceinline__ RowLse row_lse(const T* row, int V, bool vec, float* red_m, float* red_s) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -3.0e38f, s = 0.f;
  for_row<T, NT>(row, V, vec, [&](int, float x) {
    if (x > m) {
      s = s * expf(m - x) + 1.f;
      m = x;
    } else {
      s += expf(x - m);
    }
  });
  const float wm = wave_max(m);
  const float ws = wave_sum(s * expf(m - wm));
  if (lane == 0) { red_m[wave] = wm; red_s[wave] = ws; }
  __syncthreads();
  float bm = red_m[0];
#pragma unroll
  for (int w = 1; w < NT / 64; ++w) bm = fmaxf(bm, red_m[w]);
  float bs = 0.f;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) bs += red_s[w] * expf(red_m[w] - bm);
  return {bm, bm + logf(bs)};
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long c) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long x = __shfl_xor(c, o, 64);
    c = x > c ? x : c;
  }
  return c;
}

// the position of this step: a device counter plus a host offset (a captured launch serves every step), or the host value
__device__ __forceinline__ int step_position(const int* pos_dev, int pos) { return pos_dev ? *pos_dev + pos : pos; }

}  // namespace hero
