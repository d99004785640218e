// LayerNorm forward / backward (HBM-bound) for gfx950.
//
// forward : one 64-lane wave per row, the whole row lives in registers (VPL float4 per lane),
//           exact two-pass statistics in fp32, optional gathered embedding-table rows added in
//           front (SubEmbeddings / ImageEmbeddings / FrameEmbeddings sums) and dropout behind.
// backward: dx with the same row-in-registers scheme; dgamma/dbeta and plain bias gradients by a
//           two-stage deterministic column reduction (partials in a caller workspace, no atomics).
//
// Every row body is written once and compiled in two forms (template parameter FULL):
//   general       any cols % 4 == 0: a chunk past the row end reads a clamped address and counts as 0 (forward) or is skipped
//                 (backward); ln_fwd_kernel, ln_bwd_dx_kernel, ln_bwd_fused_kernel
//   straight-line cols == VPL * 256, known at compile time: no per-chunk branches, so all loads of a row are in flight
//                 together; ln_fwd_full_kernel, ln_bwd_fused_full_kernel
// ln_fwd_row / ln_bwd_row are the rows, ln_bwd_fused the grid-stride walk with its column partials, colsum_chunk / colsum_fold
// the two stages of every column sum (colred_*: LayerNorm's dgamma / dbeta and hero_colsum; colsum_multi_*: many sums at once).
#include "common.h"

namespace hero {

__device__ __forceinline__ void add4(float4& s, const float4& v) { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
// v *= the dropout mask of the 4-element group at (row, c) of a [rows, cols] tensor
__device__ __forceinline__ void ln_mask4(float4& v, const DropCtx& drop, int row, int cols, int c) {
  const float4 m = drop.mask4(((uint64_t)row * (uint64_t)cols + (uint64_t)c) >> 2);
  v.x *= m.x; v.y *= m.y; v.z *= m.z; v.w *= m.w;
}

// gamma / beta of chunks i0 .. i0 + GRP - 1
template <int VPL, int GRP>
__device__ __forceinline__ void ln_fwd_gamma_beta(const HeroLnFwd& a, const int (&cc)[VPL], int i0, float4 (&g)[GRP], float4 (&b)[GRP]) {
#pragma unroll
  for (int u = 0; u < GRP; ++u)
    if (i0 + u < VPL) {
      g[u] = *reinterpret_cast<const float4*>(a.gamma + cc[i0 + u]);
      b[u] = *reinterpret_cast<const float4*>(a.beta + cc[i0 + u]);
    }
}

// One forward row.  Written in PHASES so that the loads of a phase are in flight together: per-chunk branches
// (`if (c < cols)`, `if (x)`, `if (t[k])`) make every chunk a basic block and the compiler waits vmcnt(0) right after each load
// (68 serial round trips for a 4352-wide row).  General form: optional x, up to three gathered table rows, a chunk past the
// row reads a clamped address and is multiplied by 0; gamma / beta are fetched GRP chunks at a time behind the statistics.
// Straight-line form (x given, no tables): gamma / beta are in flight together with the row.
template <typename TX, typename TY, int VPL, bool FULL>
__device__ __forceinline__ void ln_fwd_row(const HeroLnFwd& a, int row, int lane) {
  const int cols = FULL ? VPL * 256 : a.cols;
  int cc[VPL];
  float okf[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + 64 * i) * 4;
    cc[i] = FULL ? c : min(c, cols - 4);
    okf[i] = (FULL || c < cols) ? 1.f : 0.f;
  }
  float4 v[VPL];
  if (FULL || a.x) {                                  // uniform
    const TX* x = static_cast<const TX*>(a.x) + (size_t)row * cols;
#pragma unroll
    for (int i = 0; i < VPL; ++i) v[i] = V4<TX>::ld(x + cc[i]);
  } else {
#pragma unroll
    for (int i = 0; i < VPL; ++i) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  constexpr int GRP = FULL ? VPL : 4;                 // gamma / beta of GRP chunks are fetched together, then GRP stores
  float4 g[GRP], b[GRP];
  if constexpr (FULL) {
    ln_fwd_gamma_beta(a, cc, 0, g, b);
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k)
      if (a.tab[k]) {                                 // uniform
        const float* t = a.tab[k] + (size_t)(a.idx[k] ? a.idx[k][row] : 0) * cols;
        float4 w[VPL];
#pragma unroll
        for (int i = 0; i < VPL; ++i) w[i] = *reinterpret_cast<const float4*>(t + cc[i]);
#pragma unroll
        for (int i = 0; i < VPL; ++i) add4(v[i], w[i]);
      }
  }
  // ---- statistics: sum -> mean -> centred squares -> rstd
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    if constexpr (!FULL) { v[i].x *= okf[i]; v[i].y *= okf[i]; v[i].z *= okf[i]; v[i].w *= okf[i]; }
    s += (v[i].x + v[i].y) + (v[i].z + v[i].w);
  }
  const float mean = wave_sum(s) / (float)cols;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const float dx = v[i].x - mean, dy = v[i].y - mean, dz = v[i].z - mean, dw = v[i].w - mean;
    const float sq = (dx * dx + dy * dy) + (dz * dz + dw * dw);
    if constexpr (FULL) q += sq; else q += sq * okf[i];
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)cols + a.eps);
  if (lane == 0) {
    if (a.mean) a.mean[row] = mean;
    if (a.rstd) a.rstd[row] = rstd;
  }
  // ---- normalise, dropout, store
  DropCtx drop(a.dropout);
  TY* y = static_cast<TY*>(a.y) + (size_t)row * cols;
  TY* pre = a.pre ? static_cast<TY*>(a.pre) + (size_t)row * cols : nullptr;
#pragma unroll
  for (int i0 = 0; i0 < VPL; i0 += GRP) {
    if constexpr (!FULL) ln_fwd_gamma_beta(a, cc, i0, g, b);
    float4 o[GRP];
#pragma unroll
    for (int u = 0; u < GRP; ++u)
      if (i0 + u < VPL) {
        const int i = i0 + u;
        o[u].x = (v[i].x - mean) * rstd * g[u].x + b[u].x;
        o[u].y = (v[i].y - mean) * rstd * g[u].y + b[u].y;
        o[u].z = (v[i].z - mean) * rstd * g[u].z + b[u].z;
        o[u].w = (v[i].w - mean) * rstd * g[u].w + b[u].w;
      }
    if (drop.on()) {
#pragma unroll
      for (int u = 0; u < GRP; ++u)
        if (i0 + u < VPL) ln_mask4(o[u], drop, row, cols, cc[i0 + u]);
    }
    if (pre) {
#pragma unroll
      for (int u = 0; u < GRP; ++u)
        if (i0 + u < VPL && (FULL || okf[i0 + u] != 0.f)) V4<TY>::st(pre + cc[i0 + u], v[i0 + u]);
    }
#pragma unroll
    for (int u = 0; u < GRP; ++u)
      if (i0 + u < VPL && (FULL || okf[i0 + u] != 0.f)) V4<TY>::st(y + cc[i0 + u], o[u]);
  }
}

template <typename TX, typename TY, int VPL>
__global__ __launch_bounds__(256) void ln_fwd_kernel(HeroLnFwd a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row < a.rows) ln_fwd_row<TX, TY, VPL, false>(a, row, lane);
}
template <typename TX, typename TY, int VPL>
__global__ __launch_bounds__(256) void ln_fwd_full_kernel(HeroLnFwd a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row < a.rows) ln_fwd_row<TX, TY, VPL, true>(a, row, lane);
}

// One backward row: dx (and dx * mask_in); with ACC also this wave's column partials ag += dy*xhat (dgamma), ab += dy (dbeta),
// ai += dx*mask_in (dbias_in: the bias gradient of the linear layer that feeds this LayerNorm), dy being dy * mask_out.
// General form: a chunk past the row end is skipped, which makes every chunk a basic block of its own (the compiler waits
// vmcnt(0) after each chunk's loads).  Straight-line form: gamma comes in registers (gm, loaded once per kernel) and all loads
// of the row are issued before anything is used.  (The two DropCtx come by value: by reference the general fused kernels
// took 2 - 4 more VGPRs, one of them an occupancy step.)
template <typename TX, typename T, int VPL, bool FULL, bool ACC>
__device__ __forceinline__ void ln_bwd_row(const HeroLnBwd& a, int row, int lane, const DropCtx dout, const DropCtx din,
                                           const float4* gm, float4* ag, float4* ab, float4* ai) {
  const int cols = FULL ? VPL * 256 : a.cols;
  const float inv = 1.f / (float)cols;
  const TX* x = static_cast<const TX*>(a.x) + (size_t)row * cols;
  const T* dy = static_cast<const T*>(a.dy) + (size_t)row * cols;
  float4 xv[VPL], d[VPL];
  if constexpr (FULL) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      xv[i] = V4<TX>::ld(x + (lane + 64 * i) * 4);
      d[i] = V4<T>::ld(dy + (lane + 64 * i) * 4);
    }
  }
  const float mean = a.mean[row], rstd = a.rstd[row];
  if constexpr (FULL) {
    if (dout.on()) {
#pragma unroll
      for (int i = 0; i < VPL; ++i) ln_mask4(d[i], dout, row, cols, (lane + 64 * i) * 4);
    }
  }
  float4 xh[VPL], g[VPL];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + 64 * i) * 4;
    xh[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    g[i] = xh[i];
    if (FULL || c < cols) {
      if constexpr (!FULL) {
        xv[i] = V4<TX>::ld(x + c);
        d[i] = V4<T>::ld(dy + c);
        if (dout.on()) ln_mask4(d[i], dout, row, cols, c);
      }
      const float4 gv = FULL ? gm[i] : *reinterpret_cast<const float4*>(a.gamma + c);
      xh[i] = make_float4((xv[i].x - mean) * rstd, (xv[i].y - mean) * rstd, (xv[i].z - mean) * rstd, (xv[i].w - mean) * rstd);
      g[i] = make_float4(d[i].x * gv.x, d[i].y * gv.y, d[i].z * gv.z, d[i].w * gv.w);
      if constexpr (ACC) {
        ag[i].x += d[i].x * xh[i].x; ag[i].y += d[i].y * xh[i].y; ag[i].z += d[i].z * xh[i].z; ag[i].w += d[i].w * xh[i].w;
        add4(ab[i], d[i]);
      }
      s1 += (g[i].x + g[i].y) + (g[i].z + g[i].w);
      s2 += (g[i].x * xh[i].x + g[i].y * xh[i].y) + (g[i].z * xh[i].z + g[i].w * xh[i].w);
    }
  }
  s1 = wave_sum(s1) * inv;
  s2 = wave_sum(s2) * inv;
  T* dx = a.dx ? static_cast<T*>(a.dx) + (size_t)row * cols : nullptr;
  T* dxd = a.dx_dropped ? static_cast<T*>(a.dx_dropped) + (size_t)row * cols : nullptr;
  constexpr int GRP = FULL ? VPL : 1;                 // straight-line: the whole row goes through each step together
#pragma unroll
  for (int i0 = 0; i0 < VPL; i0 += GRP) {
    if (!FULL && (lane + 64 * i0) * 4 >= cols) continue;
    float4 o[GRP];
#pragma unroll
    for (int u = 0; u < GRP; ++u) {
      const int i = i0 + u;
      o[u].x = rstd * (g[i].x - s1 - xh[i].x * s2);
      o[u].y = rstd * (g[i].y - s1 - xh[i].y * s2);
      o[u].z = rstd * (g[i].z - s1 - xh[i].z * s2);
      o[u].w = rstd * (g[i].w - s1 - xh[i].w * s2);
    }
    if (dx) {
#pragma unroll
      for (int u = 0; u < GRP; ++u) V4<T>::st(dx + (lane + 64 * (i0 + u)) * 4, o[u]);
    }
    if (din.on()) {
#pragma unroll
      for (int u = 0; u < GRP; ++u) ln_mask4(o[u], din, row, cols, (lane + 64 * (i0 + u)) * 4);
    }
    if (dxd) {
#pragma unroll
      for (int u = 0; u < GRP; ++u) V4<T>::st(dxd + (lane + 64 * (i0 + u)) * 4, o[u]);
    }
    if constexpr (ACC) {
#pragma unroll
      for (int u = 0; u < GRP; ++u) add4(ai[i0 + u], o[u]);
    }
  }
}

template <typename TX, typename T, int VPL>
__global__ __launch_bounds__(256) void ln_bwd_dx_kernel(HeroLnBwd a) {
  const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  DropCtx dout(a.dropout_out), din(a.dropout_in);
  ln_bwd_row<TX, T, VPL, false, false>(a, row, lane, dout, din, nullptr, nullptr, nullptr, nullptr);
}

// Fused backward for rows <= 1024 wide: dx (and dx * mask_in) PLUS per-workgroup partial sums of dgamma, dbeta and dbias_in
// in the same pass over x and dy.  Each wave walks rows grid-stride and keeps the column partials in registers; one LDS
// reduction per workgroup writes partial[block][3][cols]; colred_final3_kernel folds the partials (deterministic, no atomics).
template <typename TX, typename T, int VPL, bool FULL>
__device__ __forceinline__ void ln_bwd_fused(const HeroLnBwd& a, float* partial) {
  extern __shared__ __attribute__((aligned(16))) float red[];       // [4 waves][3][cols]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int cols = FULL ? VPL * 256 : a.cols;
  DropCtx dout(a.dropout_out), din(a.dropout_in);
  float4 ag[VPL], ab[VPL], ai[VPL], gm[VPL];
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    ag[i] = ab[i] = ai[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (FULL) gm[i] = *reinterpret_cast<const float4*>(a.gamma + (lane + 64 * i) * 4);
  }
  for (int row = blockIdx.x * 4 + wave; row < a.rows; row += gridDim.x * 4)
    ln_bwd_row<TX, T, VPL, FULL, true>(a, row, lane, dout, din, gm, ag, ab, ai);
  // ---- workgroup reduction of the three column partials
#pragma unroll
  for (int i = 0; i < VPL; ++i) {
    const int c = (lane + 64 * i) * 4;
    if (FULL || c < cols) {
      *reinterpret_cast<float4*>(red + ((size_t)(wave * 3 + 0)) * cols + c) = ag[i];
      *reinterpret_cast<float4*>(red + ((size_t)(wave * 3 + 1)) * cols + c) = ab[i];
      *reinterpret_cast<float4*>(red + ((size_t)(wave * 3 + 2)) * cols + c) = ai[i];
    }
  }
  __syncthreads();
  const int n4 = 3 * (cols >> 2);
  for (int q = threadIdx.x; q < n4; q += 256) {
    const int k = q / (cols >> 2), c = (q - k * (cols >> 2)) * 4;
    float4 v = *reinterpret_cast<const float4*>(red + (size_t)k * cols + c);
#pragma unroll
    for (int w = 1; w < 4; ++w) add4(v, *reinterpret_cast<const float4*>(red + ((size_t)(w * 3 + k)) * cols + c));
    *reinterpret_cast<float4*>(partial + ((size_t)blockIdx.x * 3 + k) * cols + c) = v;
  }
}

template <typename TX, typename T, int VPL>
__global__ __launch_bounds__(256) void ln_bwd_fused_kernel(HeroLnBwd a, float* partial) {
  ln_bwd_fused<TX, T, VPL, false>(a, partial);
}
template <typename TX, typename T, int VPL>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 8))) void ln_bwd_fused_full_kernel(HeroLnBwd a, float* partial) {
  ln_bwd_fused<TX, T, VPL, true>(a, partial);
}

// out_k[c] = beta*out_k[c] + sum_b partial[b][k][c] for k = blockIdx.y (outputs may be NULL).
// 16 float4 column groups x 16 partial-lanes per workgroup; fixed summation order (the partials of a lane one after the other,
// not pairwise as in colsum_fold: the two loops are not one).
__global__ __launch_bounds__(256) void colred_final3_kernel(const float* partial, float* o0, float* o1, float* o2, int cols,
                                                            int nblocks, float beta) {
  const int k = blockIdx.y;
  float* out = k == 0 ? o0 : (k == 1 ? o1 : o2);
  if (!out) return;
  __shared__ float4 red[16][16];
  const int cg = threadIdx.x & 15, kl = threadIdx.x >> 4;
  const int c = (blockIdx.x * 16 + cg) * 4;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (c < cols) {
    int b = kl;
    // four partials per trip, loads issued together (one per trip = one 16-byte request in flight per thread: the
    // 8 trips of the 1024-block fold were 8 serial round trips, most of the kernel's 5 us)
    for (; b + 48 < nblocks; b += 64) {
      float4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const float4*>(partial + ((size_t)(b + 16 * u) * 3 + k) * cols + c);
#pragma unroll
      for (int u = 0; u < 4; ++u) add4(s, v[u]);
    }
    for (; b < nblocks; b += 16) add4(s, *reinterpret_cast<const float4*>(partial + ((size_t)b * 3 + k) * cols + c));
  }
  red[kl][cg] = s;
  __syncthreads();
  if (kl == 0 && c < cols) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);     // the destination is fetched while the LDS sum runs
    if (beta != 0.f) {
      o = *reinterpret_cast<const float4*>(out + c);
      o.x *= beta; o.y *= beta; o.z *= beta; o.w *= beta;
    }
#pragma unroll
    for (int j = 1; j < 16; ++j) add4(s, red[j][cg]);
    add4(o, s);
    *reinterpret_cast<float4*>(out + c) = o;
  }
}

// ---- column sums, stage 1: what one workgroup row-lane (ty of 4) adds up over the rows r0 + ty, r0 + ty + 4, ... < r1 of a
// chunk, 4 columns from c.  sb += d, and with x given sg += d * xhat, d being the dy row times its dropout mask (drop may be
// null).  Four rows per trip, their loads issued together (one load per trip left a single 8-byte request in flight per wave:
// 12 serial round trips per chunk).
template <typename TX, typename T>
__device__ __forceinline__ void colsum_chunk(const T* dy, int ld, int c, int r0, int r1, int ty, float4& sb, const TX* x,
                                             const float* mean, const float* rstd, int cols, const DropCtx* drop, float4& sg) {
  const bool masked = drop && drop->on();
  int r = r0 + ty;
  for (; r + 12 < r1; r += 16) {
    float4 d[4], xv[4];
    float mu[4], rs[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) d[u] = V4<T>::ld(dy + (size_t)(r + 4 * u) * ld + c);
    if (x) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        xv[u] = V4<TX>::ld(x + (size_t)(r + 4 * u) * cols + c);
        mu[u] = mean[r + 4 * u];
        rs[u] = rstd[r + 4 * u];
      }
    }
    if (masked) {
#pragma unroll
      for (int u = 0; u < 4; ++u) ln_mask4(d[u], *drop, r + 4 * u, cols, c);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) add4(sb, d[u]);
    if (x) {
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        sg.x += d[u].x * (xv[u].x - mu[u]) * rs[u]; sg.y += d[u].y * (xv[u].y - mu[u]) * rs[u];
        sg.z += d[u].z * (xv[u].z - mu[u]) * rs[u]; sg.w += d[u].w * (xv[u].w - mu[u]) * rs[u];
      }
    }
  }
  for (; r < r1; r += 4) {
    float4 d = V4<T>::ld(dy + (size_t)r * ld + c);
    if (masked) ln_mask4(d, *drop, r, cols, c);
    add4(sb, d);
    if (x) {
      const float4 xv = V4<TX>::ld(x + (size_t)r * cols + c);
      const float mu = mean[r], rs = rstd[r];
      sg.x += d.x * (xv.x - mu) * rs; sg.y += d.y * (xv.y - mu) * rs;
      sg.z += d.z * (xv.z - mu) * rs; sg.w += d.w * (xv.w - mu) * rs;
    }
  }
}

// ---- column sums, stage 2: the sum over part[nchunks][cols] of column c, fixed order: 16 columns x 16 chunk-lanes per
// workgroup, four chunks per trip (loads issued together), the lanes of a column combined with shuffles, the four waves
// through red.  part may be null (sum 0).  Every thread of the workgroup calls it; threads 0 .. 15 get the result.
__device__ __forceinline__ float colsum_fold(const float* part, int cols, int c, int nchunks, float (&red)[4][16]) {
  const int cl = threadIdx.x & 15;
  float s = 0.f;
  if (part && c < cols) {
    int k = threadIdx.x >> 4;
    for (; k + 48 < nchunks; k += 64) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = part[(size_t)(k + 16 * u) * cols + c];
      s += (v[0] + v[1]) + (v[2] + v[3]);
    }
    for (; k < nchunks; k += 16) s += part[(size_t)k * cols + c];
  }
#pragma unroll
  for (int o = 16; o < 64; o <<= 1) s += __shfl_xor(s, o, 64);
  if ((threadIdx.x & 63) < 16) red[threadIdx.x >> 6][cl] = s;
  __syncthreads();
  return (red[0][cl] + red[1][cl]) + (red[2][cl] + red[3][cl]);
}

// partial column sums over a chunk of rows.  pb[chunk][c] = sum dy_eff ; pg[chunk][c] = sum dy_eff*xhat
struct ColRed {
  const void* x;      // [rows, cols] TX or null
  const void* dy;     // [rows, ld]  T
  const float* mean;
  const float* rstd;
  float* pg;
  float* pb;
  int rows, cols, ld, rows_per_chunk;
  HeroDropout dropout;
};

template <typename TX, typename T>
__global__ __launch_bounds__(256) void colred_kernel(ColRed a) {
  __shared__ float4 red[2][4][64];
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = (blockIdx.x * 64 + tx) * 4;
  const int chunk = blockIdx.y;
  const int r0 = chunk * a.rows_per_chunk;
  const int r1 = min(a.rows, r0 + a.rows_per_chunk);
  float4 sg = make_float4(0.f, 0.f, 0.f, 0.f), sb = sg;
  if (c < a.cols) {
    DropCtx drop(a.dropout);
    colsum_chunk(static_cast<const T*>(a.dy), a.ld, c, r0, r1, ty, sb, static_cast<const TX*>(a.x), a.mean, a.rstd, a.cols, &drop, sg);
  }
  red[0][ty][tx] = sg;
  red[1][ty][tx] = sb;
  __syncthreads();
  if (ty == 0 && c < a.cols) {
#pragma unroll
    for (int k = 1; k < 4; ++k) { add4(sg, red[0][k][tx]); add4(sb, red[1][k][tx]); }
    if (a.pg) *reinterpret_cast<float4*>(a.pg + (size_t)chunk * a.cols + c) = sg;
    *reinterpret_cast<float4*>(a.pb + (size_t)chunk * a.cols + c) = sb;
  }
}

// out[c] = beta*out[c] + sum_k partial[k][c] (outputs may be NULL)
__global__ __launch_bounds__(256) void colred_final_kernel(const float* pg, const float* pb, float* og, float* ob, int cols,
                                                           int nchunks, float beta) {
  __shared__ float red[2][4][16];
  const int c = blockIdx.x * 16 + (threadIdx.x & 15);
  const float sg = colsum_fold(og ? pg : nullptr, cols, c, nchunks, red[0]);
  const float sb = colsum_fold(ob ? pb : nullptr, cols, c, nchunks, red[1]);
  if (threadIdx.x < 16 && c < cols) {
    if (og) og[c] = (beta != 0.f ? beta * og[c] : 0.f) + sg;
    if (ob) ob[c] = (beta != 0.f ? beta * ob[c] : 0.f) + sb;
  }
}

static inline int chunking(int rows, int* rpc) {
  int r = (rows + 255) / 256;
  if (r < 16) r = 16;
  *rpc = r;
  return (rows + r - 1) / r;
}

// Two launches, fixed order.  (fp32 atomics straight into the outputs instead of the fold were measured SLOWER, at 256-way and
// at 64-way contention; a fold cut into 8 z-slices that add their shares with atomics gives order-dependent sums, and one
// slice folds 256 partial rows in a few microseconds.)
template <typename TX, typename T>
static int run_colred(const void* x, const void* dy, const float* mean, const float* rstd, float* og, float* ob, int rows,
                      int cols, int ld, float beta, const HeroDropout& dr, void* ws, hipStream_t s) {
  ColRed a;
  a.x = x; a.dy = dy; a.mean = mean; a.rstd = rstd;
  a.rows = rows; a.cols = cols; a.ld = ld; a.dropout = dr;
  const int nchunks = chunking(rows, &a.rows_per_chunk);
  a.pb = static_cast<float*>(ws);
  a.pg = x ? a.pb + (size_t)nchunks * cols : nullptr;
  hipLaunchKernelGGL((colred_kernel<TX, T>), dim3((cols + 255) / 256, nchunks), dim3(256), 0, s, a);
  int rc = check_launch("colred");
  if (rc) return rc;
  hipLaunchKernelGGL(colred_final_kernel, dim3((cols + 15) / 16), dim3(256), 0, s, a.pg, a.pb, x ? og : nullptr, ob, cols,
                     nchunks, beta);
  return check_launch("colred_final");
}

// (x dtype, dy / y dtype) -> f(TX(), T()) for the three pairs the kernels are built for; `second` names the other tensor
template <typename F>
static int ln_dtypes(const char* who, const char* second, int xd, int d, F f) {
  if (xd == HERO_F32 && d == HERO_F32) return f(float(), float());
  if (xd == HERO_F32 && d == HERO_BF16) return f(float(), bf16_t());
  if (xd == HERO_BF16 && d == HERO_BF16) return f(bf16_t(), bf16_t());
  set_error("%s: unsupported dtypes x=%d %s=%d", who, xd, second, d);
  return HERO_ERR_UNSUPPORTED;
}

// CALL(VPL) with the float4 chunks per lane that a row of `cols` needs; rows up to 1024 wide (all that the fused backward and
// the straight-line kernels are built for) take HERO_VPL_SWITCH4
#define HERO_VPL_SWITCH4(cols, CALL)                                       \
  do {                                                                     \
    const int need4 = ((cols) + 255) / 256;                                \
    if (need4 <= 1) { CALL(1); }                                           \
    else if (need4 <= 2) { CALL(2); }                                      \
    else if (need4 <= 3) { CALL(3); }                                      \
    else { CALL(4); }                                                      \
  } while (0)
#define HERO_VPL_SWITCH(cols, CALL)                                        \
  do {                                                                     \
    const int need = ((cols) + 255) / 256;                                 \
    if (need <= 4) HERO_VPL_SWITCH4(cols, CALL);                           \
    else if (need <= 6) { CALL(6); }                                       \
    else if (need <= 8) { CALL(8); }                                       \
    else if (need <= 12) { CALL(12); }                                     \
    else if (need <= 17) { CALL(17); }                                     \
    else if (need <= 24) { CALL(24); }                                     \
    else { set_error("layernorm: cols %d too wide (max 6144)", (cols)); return HERO_ERR_UNSUPPORTED; } \
  } while (0)

}  // namespace hero

#define LN_BWD_MAX_BLOCKS 1024
using namespace hero;

extern "C" int hero_layernorm_fwd(const HeroLnFwd* a, hero_stream_t stream) {
  HERO_REQUIRE(a && a->y && a->gamma && a->beta, "hero_layernorm_fwd: null pointer");
  HERO_REQUIRE(a->x || a->tab[0] || a->tab[1] || a->tab[2], "hero_layernorm_fwd: no input");
  HERO_REQUIRE(a->cols > 0 && a->cols % 4 == 0, "hero_layernorm_fwd: cols (%d) must be a positive multiple of 4", a->cols);
  if (a->rows <= 0) return HERO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid((a->rows + 3) / 4), block(256);
  const int xd = a->x ? a->x_dtype : a->y_dtype, yd = a->y_dtype;
  int rc = HERO_OK;
#define LAUNCH(KERNEL, V)                                                                         \
  rc = ln_dtypes("hero_layernorm_fwd", "y", xd, yd, [&](auto tx, auto ty) {                       \
    hipLaunchKernelGGL((KERNEL<decltype(tx), decltype(ty), V>), grid, block, 0, s, *a);           \
    return HERO_OK;                                                                               \
  })
  if (a->x && !a->tab[0] && !a->tab[1] && !a->tab[2] && a->cols % 256 == 0 && a->cols <= 1024) {   // straight-line kernel
#define CALL(V) LAUNCH(ln_fwd_full_kernel, V)
    HERO_VPL_SWITCH4(a->cols, CALL);
#undef CALL
    return rc ? rc : check_launch("hero_layernorm_fwd(full)");
  }
#define CALL(V) LAUNCH(ln_fwd_kernel, V)
  HERO_VPL_SWITCH(a->cols, CALL);
#undef CALL
#undef LAUNCH
  return rc ? rc : check_launch("hero_layernorm_fwd");
}

extern "C" size_t hero_layernorm_bwd_workspace_bytes(int rows, int cols) {
  (void)rows;
  return (size_t)LN_BWD_MAX_BLOCKS * (size_t)cols * 3 * sizeof(float);
}
extern "C" size_t hero_colsum_workspace_bytes(int rows, int cols) {
  (void)rows;
  return (size_t)256 * (size_t)cols * sizeof(float);
}

extern "C" int hero_layernorm_bwd(const HeroLnBwd* a, hero_stream_t stream) {
  HERO_REQUIRE(a && a->x && a->dy && a->gamma && a->mean && a->rstd, "hero_layernorm_bwd: null pointer");
  HERO_REQUIRE(a->cols > 0 && a->cols % 4 == 0, "hero_layernorm_bwd: cols (%d) must be a positive multiple of 4", a->cols);
  if (a->rows <= 0) return HERO_OK;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int xd = a->x_dtype, d = a->dtype;
  const bool want_params = a->dgamma || a->dbeta || a->dbias_in;
  if (want_params) HERO_REQUIRE(a->workspace, "hero_layernorm_bwd: workspace required for parameter gradients");
  int rc = HERO_OK;
#define LAUNCH(KERNEL, V, LDS, ...)                                                                         \
  rc = ln_dtypes("hero_layernorm_bwd", "dy", xd, d, [&](auto tx, auto t) {                                  \
    hipLaunchKernelGGL((KERNEL<decltype(tx), decltype(t), V>), grid, block, LDS, s, __VA_ARGS__);          \
    return HERO_OK;                                                                                         \
  })
  // ---- fused single pass (rows up to 1024 wide)
  if (want_params && (a->dx || a->dx_dropped || a->dbias_in) && a->cols <= 1024) {
    int nblk = (a->rows + 3) / 4;
    if (nblk > LN_BWD_MAX_BLOCKS) nblk = LN_BWD_MAX_BLOCKS;   // 1024: 4 workgroups / CU (512: +0.06 ms/step, 2048: +0.03)
    float* partial = static_cast<float*>(a->workspace);
    const size_t lds = (size_t)4 * 3 * a->cols * sizeof(float);
    const dim3 grid(nblk), block(256);
    if (a->cols % 256 == 0) {                          // straight-line kernel
#define CALL(V) LAUNCH(ln_bwd_fused_full_kernel, V, lds, *a, partial)
      HERO_VPL_SWITCH4(a->cols, CALL);
#undef CALL
    } else {
#define CALL(V) LAUNCH(ln_bwd_fused_kernel, V, lds, *a, partial)
      HERO_VPL_SWITCH4(a->cols, CALL);
#undef CALL
    }
    if (rc) return rc;
    rc = check_launch("hero_layernorm_bwd(fused)");
    if (rc || a->defer_fold) return rc;
    // one fixed-order fold (see run_colred)
    hipLaunchKernelGGL(colred_final3_kernel, dim3((a->cols + 63) / 64, 3), dim3(256), 0, s, partial, a->dgamma, a->dbeta,
                       a->dbias_in, a->cols, nblk, a->grad_beta);
    return check_launch("hero_layernorm_bwd(final3)");
  }
  HERO_REQUIRE(!a->dbias_in, "hero_layernorm_bwd: dbias_in needs cols <= 1024");
  HERO_REQUIRE(!a->defer_fold, "hero_layernorm_bwd: defer_fold needs the fused path (cols <= 1024, dx or dbias_in wanted)");
  if (a->dx || a->dx_dropped) {
    const dim3 grid((a->rows + 3) / 4), block(256);
#define CALL(V) LAUNCH(ln_bwd_dx_kernel, V, 0, *a)
    HERO_VPL_SWITCH(a->cols, CALL);
#undef CALL
    if (rc) return rc;
    rc = check_launch("hero_layernorm_bwd(dx)");
    if (rc) return rc;
  }
#undef LAUNCH
  if (a->dgamma || a->dbeta)
    return ln_dtypes("hero_layernorm_bwd", "dy", xd, d, [&](auto tx, auto t) {
      return run_colred<decltype(tx), decltype(t)>(a->x, a->dy, a->mean, a->rstd, a->dgamma, a->dbeta, a->rows, a->cols, a->cols,
                                                   a->grad_beta, a->dropout_out, a->workspace, s);
    });
  return HERO_OK;
}

extern "C" int hero_layernorm_bwd_blocks(int rows) {
  int nblk = (rows + 3) / 4;
  return nblk > LN_BWD_MAX_BLOCKS ? LN_BWD_MAX_BLOCKS : nblk;
}

// ---- many column sums, two launches --------------------------------------------------------------------------------
// (passed by value: the whole struct must stay under the 4 KB kernel-argument limit - 64 x 48 + 772 bytes)
struct ColsumMulti {
  HeroColsum p[HERO_COLSUM_MULTI_MAX];
  int blk0[HERO_COLSUM_MULTI_MAX + 1];    // first workgroup of problem i (stage 1: col-blocks x chunks; stage 2: 16-column groups)
  int woff[HERO_COLSUM_MULTI_MAX];        // partial sums of problem i: workspace + woff[i], [nchunks][cols]
  int rpc[HERO_COLSUM_MULTI_MAX];         // rows per chunk
  int n;
};

__device__ __forceinline__ int colsum_find(const ColsumMulti& a, int b) {
  int lo = 0, hi = a.n - 1;                // uniform binary search over <= 64 prefix entries
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.blk0[mid] <= b) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void colsum_multi_part_kernel(ColsumMulti a, float* ws) {
  __shared__ float4 red[4][64];
  const int pi = colsum_find(a, blockIdx.x);
  const HeroColsum P = a.p[pi];
  const int ncb = (P.cols + 255) / 256;
  const int local = blockIdx.x - a.blk0[pi], cb = local % ncb, chunk = local / ncb;
  const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
  const int c = (cb * 64 + tx) * 4;
  const int r0 = chunk * a.rpc[pi], r1 = min(P.rows, r0 + a.rpc[pi]);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f), unused = s;
  const float* const none = nullptr;                  // plain sums: no x, no dropout
  if (c < P.cols) {
    if (P.dtype == HERO_BF16) colsum_chunk(static_cast<const bf16_t*>(P.src), P.ld, c, r0, r1, ty, s, none, none, none, 0, nullptr, unused);
    else colsum_chunk(static_cast<const float*>(P.src), P.ld, c, r0, r1, ty, s, none, none, none, 0, nullptr, unused);
  }
  red[ty][tx] = s;
  __syncthreads();
  if (ty == 0 && c < P.cols) {
#pragma unroll
    for (int k = 1; k < 4; ++k) add4(s, red[k][tx]);
    *reinterpret_cast<float4*>(ws + a.woff[pi] + (size_t)chunk * P.cols + c) = s;
  }
}

// dst[c] = beta*dst[c] + sum over the chunks
__global__ __launch_bounds__(256) void colsum_multi_fold_kernel(ColsumMulti a, const float* ws) {
  __shared__ float red[4][16];
  const int pi = colsum_find(a, blockIdx.x);
  const HeroColsum P = a.p[pi];
  const int nchunks = (P.rows + a.rpc[pi] - 1) / a.rpc[pi];
  const int c = (blockIdx.x - a.blk0[pi]) * 16 + (threadIdx.x & 15);
  const float s = colsum_fold(ws + a.woff[pi], P.cols, c, nchunks, red);
  if (threadIdx.x < 16 && c < P.cols) {
    if (P.dst_rows) {
      // indexed destination rows (periodic position ids): distinct rows receive exactly one value per launch, so the
      // atomic is order-free; only a clamped id that repeats inside one period (positions beyond 511) shares a row
      const int j = c / P.row_cols, r = P.dst_rows[j];
      if (r >= 0) atomicAdd(P.dst + (size_t)r * P.row_cols + (c - j * P.row_cols), s);
    } else {
      P.dst[c] = (P.beta != 0.f ? P.beta * P.dst[c] : 0.f) + s;
    }
  }
}

static_assert(sizeof(ColsumMulti) <= 4000, "kernel argument size");

static int colsum_multi_plan(const HeroColsum* p, int n, ColsumMulti* a, int* fold_blocks, size_t* ws_floats) {
  size_t off = 0;
  int b1 = 0;
  for (int i = 0; i < n; ++i) {
    int rpc;
    const int nchunks = chunking(p[i].rows, &rpc);
    if (a) { a->p[i] = p[i]; a->blk0[i] = b1; a->woff[i] = (int)off; a->rpc[i] = rpc; }
    b1 += ((p[i].cols + 255) / 256) * nchunks;
    off += (size_t)nchunks * p[i].cols;
  }
  if (a) { a->blk0[n] = b1; a->n = n; }
  if (fold_blocks) {
    int b2 = 0;
    for (int i = 0; i < n; ++i) b2 += (p[i].cols + 15) / 16;
    *fold_blocks = b2;
  }
  *ws_floats = off;
  return b1;
}

extern "C" size_t hero_colsum_multi_workspace_bytes(const HeroColsum* p, int n) {
  if (!p || n < 1 || n > HERO_COLSUM_MULTI_MAX) return 0;
  size_t fl = 0;
  colsum_multi_plan(p, n, nullptr, nullptr, &fl);
  return fl * sizeof(float);
}

extern "C" int hero_colsum_multi(const HeroColsum* p, int n, void* workspace, hero_stream_t stream) {
  HERO_REQUIRE(p && workspace && n >= 1 && n <= HERO_COLSUM_MULTI_MAX, "hero_colsum_multi: 1..%d problems and a workspace", HERO_COLSUM_MULTI_MAX);
  for (int i = 0; i < n; ++i) {
    HERO_REQUIRE(p[i].src && p[i].dst && p[i].rows > 0 && p[i].cols > 0 && p[i].cols % 4 == 0 && p[i].ld % 4 == 0 &&
                     (p[i].dtype == HERO_BF16 || p[i].dtype == HERO_F32) && ((uintptr_t)p[i].src & 7) == 0,
                 "hero_colsum_multi: bad problem %d", i);
    HERO_REQUIRE(!p[i].dst_rows || (p[i].beta == 1.f && p[i].row_cols > 0 && p[i].cols % p[i].row_cols == 0),
                 "hero_colsum_multi: problem %d: dst_rows needs beta = 1 and cols a multiple of row_cols", i);
  }
  ColsumMulti a, f;
  size_t fl = 0;
  int fold_blocks = 0;
  const int part_blocks = colsum_multi_plan(p, n, &a, &fold_blocks, &fl);
  HERO_REQUIRE(fl < 0x7fffffffull, "hero_colsum_multi: workspace too large");
  f = a;                                    // stage 2 walks 16-column groups instead
  int b2 = 0;
  for (int i = 0; i < n; ++i) { f.blk0[i] = b2; b2 += (p[i].cols + 15) / 16; }
  f.blk0[n] = b2;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(colsum_multi_part_kernel, dim3(part_blocks), dim3(256), 0, s, a, static_cast<float*>(workspace));
  int rc = check_launch("hero_colsum_multi(partials)");
  if (rc) return rc;
  hipLaunchKernelGGL(colsum_multi_fold_kernel, dim3(fold_blocks), dim3(256), 0, s, f, static_cast<const float*>(workspace));
  return check_launch("hero_colsum_multi(fold)");
}

extern "C" int hero_colsum(const void* x, float* out, int rows, int cols, int ld, int dtype, float beta, void* workspace,
                           hero_stream_t stream) {
  HERO_REQUIRE(x && out && workspace, "hero_colsum: null pointer");
  HERO_REQUIRE(cols > 0 && cols % 4 == 0 && ld % 4 == 0, "hero_colsum: cols/ld (%d, %d) must be multiples of 4", cols, ld);
  hipStream_t s = static_cast<hipStream_t>(stream);
  HeroDropout none = {nullptr, 0, 0, 1.f};
  if (rows <= 0) {
    if (beta == 0.f) hipLaunchKernelGGL(colred_final_kernel, dim3((cols + 15) / 16), dim3(256), 0, s, nullptr, nullptr, nullptr, out, cols, 0, 0.f);   // zeros (a kernel node, not a memset)
    return HERO_OK;
  }
  if (dtype == HERO_F32) return run_colred<float, float>(nullptr, x, nullptr, nullptr, nullptr, out, rows, cols, ld, beta, none, workspace, s);
  if (dtype == HERO_BF16) return run_colred<float, bf16_t>(nullptr, x, nullptr, nullptr, nullptr, out, rows, cols, ld, beta, none, workspace, s);
  set_error("hero_colsum: bad dtype %d", dtype);
  return HERO_ERR_ARG;
}
