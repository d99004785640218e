// Helpers shared by the matrix-core attention kernels (attention_mfma.hip: L <= 64, one or two waves per head;
// attention_mfma_long.hip: 64 < L <= 256, one workgroup per head).  bf16, head size 64.
#pragma once
#include "common.h"

namespace hero {
namespace attn {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

constexpr int RS = 72;   // LDS row stride (bf16 elements) of a [rows][64] head tile: 144 B, conflict-free b128 / tr reads

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// row fragment (MFMA A or B operand with the contraction along the row): 8 consecutive elements
__device__ __forceinline__ bf16x8_t gfrag(const bf16_t* __restrict__ base, int ld, int row, int L, int ks, int half) {
  return *reinterpret_cast<const bf16x8_t*>(base + (size_t)min(row, L - 1) * ld + 16 * ks + 8 * half);
}
__device__ __forceinline__ bf16x8_t lfrag(const bf16_t* tile, int row, int ks, int half) {
  return *reinterpret_cast<const bf16x8_t*>(tile + row * RS + 16 * ks + 8 * half);
}

// transposed fragment: the lane's 8 k-slots are rows (ra .. ra+3) and (rb .. rb+3) of an LDS tile,
// its m/n index is column cb*32 + (lane & 31).  `stride_b` = row stride in bytes.
__device__ __forceinline__ unsigned tr_addr(const void* tile, int stride_b, int row0, int cb, int lane) {
  const int p = lane & 15, gq = (lane >> 4) & 1;
  return (unsigned)(uintptr_t)tile + (row0 + (p >> 2)) * stride_b + (cb * 32 + gq * 16 + 4 * (p & 3)) * 2;
}
__device__ __forceinline__ bf16x8_t tr_frag(unsigned addr_a, unsigned addr_b) {
  uint2 r0, r1;
  asm volatile(
      "ds_read_b64_tr_b16 %0, %2\n\t"
      "ds_read_b64_tr_b16 %1, %3\n\t"
      "s_waitcnt lgkmcnt(0)"
      : "=&v"(r0), "=&v"(r1)
      : "v"(addr_a), "v"(addr_b)
      : "memory");
  const u32x4_t t = {r0.x, r0.y, r1.x, r1.y};
  return __builtin_bit_cast(bf16x8_t, t);
}

__device__ __forceinline__ bf16x8_t pack8(const float* v) {
  const u32x4_t t = {f2bf_pk(v[0], v[1]), f2bf_pk(v[2], v[3]), f2bf_pk(v[4], v[5]), f2bf_pk(v[6], v[7])};
  return __builtin_bit_cast(bf16x8_t, t);
}
__device__ __forceinline__ float xhalf(float v) { return __shfl_xor(v, 32, 64); }

// key (or, in the backward's LDS round trip, query) index of accumulator register r in a 32x32 tile
__device__ __forceinline__ int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// 8-byte store of 4 consecutive head dims
__device__ __forceinline__ void st_bf4(bf16_t* p, float a, float b, float c, float d) {
  uint2 u;
  u.x = f2bf_pk(a, b);
  u.y = f2bf_pk(c, d);
  *reinterpret_cast<uint2*>(p) = u;
}


// ---- per-tile bodies shared by the kernels.  NK = key tiles a query tile sees at compile time (1: one wave per pair, 2: two
// waves per pair).  Everything is lane <-> query row i, 16 keys per lane per key tile (acc_row); register arrays travel by
// reference to array and every loop is unrolled over compile-time bounds, so the bodies dissolve into their callers.

// transposed fragments f[dt][jt][ks] of NK 32-row tiles of an LDS head tile: k-slot e of step ks <-> row
// 32 jt + 16 ks + 4 half + (e & 3) + 8 (e >> 2), i.e. the keys this lane holds in accumulator registers 8 ks .. 8 ks + 7
// (V^T for ctx, K^T for dQ)
template <int NK>
__device__ __forceinline__ void tr_frags(const bf16_t* tile, bf16x8_t (&f)[2][NK][2], int half, int lane) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int jt = 0; jt < NK; ++jt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const int r0 = 32 * jt + 16 * ks + 4 * half;
        f[dt][jt][ks] = tr_frag(tr_addr(tile, RS * 2, r0, dt, lane), tr_addr(tile, RS * 2, r0 + 8, dt, lane));
      }
}

// out^T[dt] = sum over the keys of f[dt][jt][ks] x v[jt][8 ks .. 8 ks + 7], B straight from the registers
// (ctx^T = V^T P^T, dQ^T = K^T dS^T)
template <int NK>
__device__ __forceinline__ void tr_mfma(const bf16x8_t (&f)[2][NK][2], const float (&v)[NK][16], f32x16_t (&out)[2]) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int e = 0; e < 16; ++e) out[dt][e] = 0.f;
#pragma unroll
    for (int jt = 0; jt < NK; ++jt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks)
        out[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(f[dt][jt][ks], pack8(&v[jt][8 * ks]), out[dt], 0, 0, 0);
  }
}

// scores S^T of a query row -> p = exp(s * scale + mask - mx), mx = row maximum, inv = 1 / row sum
template <int NK>
__device__ __forceinline__ void softmax_rows(const f32x16_t (&sc)[NK], const float (&mk)[NK][16], float scale, int L, int half,
                                             float (&p)[NK][16], float& mx, float& inv) {
  mx = -3.0e38f;
#pragma unroll
  for (int jt = 0; jt < NK; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * jt + acc_row(r, half);
      const float v = j < L ? fmaf(sc[jt][r], scale, mk[jt][r]) : -3.0e38f;
      p[jt][r] = v;
      mx = fmaxf(mx, v);
    }
  mx = fmaxf(mx, xhalf(mx));
  float sum = 0.f;
#pragma unroll
  for (int jt = 0; jt < NK; ++jt)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int j = 32 * jt + acc_row(r, half);
      const float e = j < L ? __expf(p[jt][r] - mx) : 0.f;
      p[jt][r] = e;
      sum += e;
    }
  sum += xhalf(sum);
  inv = 1.f / sum;
}

// key tile jt of query row i: normalise, save the probabilities (prow: row i of the fp32 [Lm][Lm] matrix, or null), apply
// dropout (drow: first dropout index of the row).  Leaves the DROPPED probabilities in p.
__device__ __forceinline__ void emit_probs(float (&p)[16], float inv, float* prow, int i, int Lm, int L, int jt, int half,
                                           const DropCtx& drop, uint64_t drow) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j0 = 32 * jt + 8 * q + 4 * half;
    float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
    if (drop.on()) m = drop.mask4((drow + j0) >> 2);
    const float mm[4] = {m.x, m.y, m.z, m.w};
    float pr4[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      pr4[e] = p[4 * q + e] * inv;
      p[4 * q + e] = pr4[e] * mm[e];
    }
    if (prow && i < L) {
      if ((Lm & 3) == 0 && j0 + 3 < L) {
        *reinterpret_cast<float4*>(prow + j0) = make_float4(pr4[0], pr4[1], pr4[2], pr4[3]);   // one 16-byte store per run of 4 columns
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (j0 + e < L) prow[j0 + e] = pr4[e];
      }
    }
  }
}

// backward: the probabilities of query row i at this lane's keys, zero outside the sequence (rowok: 1.f if i < L, else 0.f).
// RC: no saved probabilities - rebuilt from S^T (the same MFMAs on the same operands as the forward's), then the same scale /
// mask / exp / normalise with the saved row maximum st.x and 1 / row sum st.y: bit-identical P.
// Else prow = row min(i, L - 1) of the saved fp32 [Lm][Lm] matrix.  The probabilities of this lane's 16 accumulator slots are 4
// runs of 4 consecutive columns: four 16-byte loads when the row stride allows it, issued UNCONDITIONALLY; the columns outside
// the sequence are then dropped by a SELECT on the loaded value, never by a multiplication: in a packed batch the forward
// writes only columns j < L of a row of stride Lm, the cells behind them hold whatever the allocator left there, and NaN * 0
// is NaN.  (The row factor stays a multiplication: row min(i, L - 1) is one the forward wrote.)  Written as
// `(i < L && j < L) ? prow[j] : 0` the compiler sank each of the 16 scalar loads into its own conditional block, each
// followed by s_waitcnt vmcnt(0): 16 serial round trips per 32-row block - a select per component of a float4 that is already
// loaded leaves the load where it is.
template <int NK, bool RC>
__device__ __forceinline__ void probs_row(const f32x16_t (&sc)[NK], const float (&mk)[NK][16], const float2& st, float scale,
                                          const float* __restrict__ prow, int Lm, int L, float rowok, int half, float (&pr)[NK][16]) {
  if constexpr (RC) {
#pragma unroll
    for (int jt = 0; jt < NK; ++jt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = 32 * jt + acc_row(r, half);
        const float v = j < L ? fmaf(sc[jt][r], scale, mk[jt][r]) : -3.0e38f;
        const float e = j < L ? __expf(v - st.x) : 0.f;
        pr[jt][r] = e * st.y * rowok;
      }
  } else if ((Lm & 3) == 0) {
#pragma unroll
    for (int jt = 0; jt < NK; ++jt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int j0 = 32 * jt + 8 * q + 4 * half;
        const float4 v = *reinterpret_cast<const float4*>(prow + min(j0, Lm - 4));
        pr[jt][4 * q + 0] = j0 + 0 < L ? v.x * rowok : 0.f;
        pr[jt][4 * q + 1] = j0 + 1 < L ? v.y * rowok : 0.f;
        pr[jt][4 * q + 2] = j0 + 2 < L ? v.z * rowok : 0.f;
        pr[jt][4 * q + 3] = j0 + 3 < L ? v.w * rowok : 0.f;
      }
  } else {
#pragma unroll
    for (int jt = 0; jt < NK; ++jt)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int j = 32 * jt + acc_row(r, half);
        pr[jt][r] = prow[min(j, L - 1)] * (j < L ? rowok : 0.f);
      }
  }
}

// backward: dS of a query row from dP^T (w.r.t. the DROPPED probabilities) and its probabilities: g = dP x dropout mask,
// delta = sum_j g P, dS = P (g - delta) scale.  The dropped probabilities (operand of dV) and dS go to rows Pl / Sl of the
// [query][key] bf16 LDS tiles.
template <int NK>
__device__ __forceinline__ void ds_row(const f32x16_t (&dp)[NK], const float (&pr)[NK][16], float scale, const DropCtx& drop,
                                       uint64_t drow, int half, bf16_t* Pl, bf16_t* Sl, float (&ds)[NK][16]) {
  float delta = 0.f;
#pragma unroll
  for (int jt = 0; jt < NK; ++jt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j0 = 32 * jt + 8 * q + 4 * half;
      float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
      if (drop.on()) m = drop.mask4((drow + j0) >> 2);
      const float mm[4] = {m.x, m.y, m.z, m.w};
      float pd[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float g = dp[jt][4 * q + e] * mm[e];       // dP w.r.t. the softmax output
        ds[jt][4 * q + e] = g;
        delta = fmaf(g, pr[jt][4 * q + e], delta);
        pd[e] = pr[jt][4 * q + e] * mm[e];
      }
      st_bf4(Pl + j0, pd[0], pd[1], pd[2], pd[3]);
    }
  delta += xhalf(delta);
#pragma unroll
  for (int jt = 0; jt < NK; ++jt) {
#pragma unroll
    for (int r = 0; r < 16; ++r) ds[jt][r] = pr[jt][r] * (ds[jt][r] - delta) * scale;
#pragma unroll
    for (int q = 0; q < 4; ++q)
      st_bf4(Sl + 32 * jt + 8 * q + 4 * half, ds[jt][4 * q], ds[jt][4 * q + 1], ds[jt][4 * q + 2], ds[jt][4 * q + 3]);
  }
}

// backward: dV^T = dO^T P_dropped, dK^T = Q^T dS for key tile jt, contracted over NQ query tiles: k-slot e of step ks <->
// query 32 it + 16 ks + 8 half + e for both operands (two transpose reads of 4 rows each).  Os / Qs: head tiles [query][RS],
// Pl / Sl: [query][key] tiles of row stride PS.
template <int NQ>
__device__ __forceinline__ void dkv_mfma(const bf16_t* Os, const bf16_t* Qs, const bf16_t* Pl, const bf16_t* Sl, int PS, int jt,
                                         f32x16_t (&gv)[2], f32x16_t (&gk)[2], int half, int lane) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int e = 0; e < 16; ++e) { gv[dt][e] = 0.f; gk[dt][e] = 0.f; }
#pragma unroll
  for (int it = 0; it < NQ; ++it)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int r0 = 32 * it + 16 * ks + 8 * half;
      bf16x8_t of[2], qf[2];
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        of[dt] = tr_frag(tr_addr(Os, RS * 2, r0, dt, lane), tr_addr(Os, RS * 2, r0 + 4, dt, lane));
        qf[dt] = tr_frag(tr_addr(Qs, RS * 2, r0, dt, lane), tr_addr(Qs, RS * 2, r0 + 4, dt, lane));
      }
      const bf16x8_t pf = tr_frag(tr_addr(Pl, PS * 2, r0, jt, lane), tr_addr(Pl, PS * 2, r0 + 4, jt, lane));
      const bf16x8_t sf = tr_frag(tr_addr(Sl, PS * 2, r0, jt, lane), tr_addr(Sl, PS * 2, r0 + 4, jt, lane));
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        gv[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(of[dt], pf, gv[dt], 0, 0, 0);
        gk[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[dt], sf, gk[dt], 0, 0, 0);
      }
    }
}

// NT threads copy rows [0, R) of a [L][64] bf16 head slice (row stride ld) to an LDS tile [R][RS], rows >= L zeroed
template <int NT>
__device__ __forceinline__ void stage_tile_wg(const bf16_t* __restrict__ src, int ld, int L, int R, bf16_t* dst) {
  for (int q = threadIdx.x; q < R * 8; q += NT) {
    const int r = q >> 3, c = (q & 7) * 8;
    uint4 t = *reinterpret_cast<const uint4*>(src + (size_t)min(r, L - 1) * ld + c);
    if (r >= L) t = make_uint4(0u, 0u, 0u, 0u);
    *reinterpret_cast<uint4*>(dst + r * RS + c) = t;
  }
}

// Output tiles leave through the LDS.  Straight from the accumulator layout (store_tileT below) one store instruction scatters
// 64 x 8 bytes over 32 rows of the [M, 3 D] tensor, 16 instructions per 32-row tile; staged, the same bytes leave as 4
// instructions of 16 bytes per lane, eight lanes per 128-byte head segment of a row - the map the operand loads use.
//
// stage_tileT: one 32-row tile of out^T[dt] (head dim x lane-owned row) -> 32 rows of an LDS head tile [row][RS] that the wave
// owns and no longer reads.  The conversion is st_bf4's (same rounding of the same values): the bits that reach memory are
// those of the direct store.
__device__ __forceinline__ void stage_tileT(bf16_t* rows, const f32x16_t& a0, const f32x16_t& a1, int lane) {
  bf16_t* p = rows + (lane & 31) * RS + 4 * (lane >> 5);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    st_bf4(p + 8 * q, a0[4 * q], a0[4 * q + 1], a0[4 * q + 2], a0[4 * q + 3]);
    st_bf4(p + 32 + 8 * q, a1[4 * q], a1[4 * q + 1], a1[4 * q + 2], a1[4 * q + 3]);
  }
}
// store_rows32: those 32 LDS rows (after a wave_sync_lds) -> out[row0 + r][0 .. 63], r < 32, only rows row0 + r < L.  Straight-line:
// four LDS reads, then four stores predicated per lane (no wave-uniform branch around the group).
__device__ __forceinline__ void store_rows32(bf16_t* __restrict__ dst, int ld, int L, int row0, const bf16_t* rows, int lane) {
  const int c = (lane & 7) * 8, r8 = lane >> 3;
  uint4 v[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) v[it] = *reinterpret_cast<const uint4*>(rows + (it * 8 + r8) * RS + c);
#pragma unroll
  for (int it = 0; it < 4; ++it) {
    const int r = row0 + it * 8 + r8;
    if (r < L) *reinterpret_cast<uint4*>(dst + (size_t)r * ld + c) = v[it];
  }
}

// one 32-row tile of out^T[dt] (head dim x lane-owned row) -> out[row][d], rows < L, straight from the accumulator layout: for
// the kernels whose waves own no LDS tile to stage through (attention_mfma_long.hip: forward and dQ pass)
__device__ __forceinline__ void store_tileT(bf16_t* __restrict__ dst, int ld, int L, int tile, const f32x16_t (&acc)[2], int lane) {
  const int half = lane >> 5, row = 32 * tile + (lane & 31);
  if (row < L) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
        st_bf4(dst + (size_t)row * ld + 32 * dt + 8 * q + 4 * half, acc[dt][4 * q], acc[dt][4 * q + 1], acc[dt][4 * q + 2],
               acc[dt][4 * q + 3]);
  }
}

}  // namespace attn
}  // namespace hero
