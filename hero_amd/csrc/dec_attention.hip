// Attention of the captioning decoder (gfx950): separate query and key/value sequences, optionally causal, head size 64,
// forward and backward, one kernel each (model/tvc.py:67-104 and the BertSelfAttention of its decoder layers under tri_mask).
//
//   scores[i, j] = <q_i, k_j> * scale + key_mask_add[n, j] + (causal && j > i ? -10000 : 0)
//   P = softmax_j(scores) (fp32),  ctx_i = sum_j dropout(P)[i, j] v_j
//
// The masks are ADDITIVE as in the reference, not -inf: a caption whose keys are all masked attends uniformly to all Lk
// keys and stays finite (data/tvc.py's get_st_ed_label yields an empty segment for a caption that starts at the video's end).
//
// The work is small (about 40 captions x 12 heads per step, Lq <= 60, Lk <= 100) and latency-bound: one workgroup of four
// waves owns one (caption, head) pair and keeps everything in LDS as fp32, whatever the storage dtype.
//   tiles    Q [Lq][68], K / V [round_up(Lk, 4)][68] (rows behind Lk zero), dO [Lq][68]; 68 = 64 + one 16-byte slot, so that
//            the 16 rows a ds_read_b128 lane group reads start on 16 different slots of the 256-byte bank row
//   scores   wave w owns the rows i = w + 4a, lane l the keys j = l, l + 64: a row's maximum and sum are two DPP wave
//            reductions on registers, the 16 x 2 accumulators of a lane take a broadcast Q read and two K reads per 4 dims
//   P        [Lq][round_up(Lk, 4) + 4] in LDS (dropout applied), read as float4 along j by  ctx = P V,  dQ = dS K  and, down
//            the columns, by  dV = P^T dO,  dK = dS^T Q
// The forward leaves stats [N, H, Lq, 2] = (row maximum, 1 / row sum).  The backward recomputes the scores with the SAME
// function and P = exp(s - max) * inv bit for bit, regenerates the dropout mask, and keeps no [N, H, Lq, Lk] tensor in
// memory.  dK / dV are summed over the queries inside the workgroup in a fixed order: no atomics, two runs give the same
// bits; every element of dq / dk / dv is written, the caller does no zero-fill.  In the backward dS takes V's place in LDS
// once dP = dO V^T is in registers.
//
// Incremental decoding has its own kernel further down (dec_attn_row_kernel: one query row per (caption, head), one wave each,
// keys straight from global memory or from a key/value cache that the kernel extends; inference only).
#include "common.h"

namespace hero {
namespace {

constexpr int DA_MAX_LQ = 64, DA_MAX_LK = 128, DA_LD = 68;
constexpr float DA_MASKED = -10000.f;

struct DecAttn {
  const void *q, *k, *v;
  const float* key_mask;   // [N, Lk] additive or NULL
  void* ctx;               // [N*Lq, H*64]
  float* stats;            // [N, H, Lq, 2]
  const void* dctx;        // [N*Lq, H*64]
  void *dq, *dk, *dv;      // ldq / ldkv as q / k, v
  int Lq, Lk, H, ldq, ldkv, causal;
  float scale;
  HeroDropout drop;
};

struct Tiles { int q, k, v, p, o, total; };          // offsets in floats, all multiples of 4
__host__ __device__ inline Tiles tiles(int Lq, int Lk, bool bwd) {
  const int Lk4 = (Lk + 3) & ~3, ps = Lk4 + 4;
  Tiles t;
  t.q = 0;
  t.k = t.q + Lq * DA_LD;
  t.v = t.k + Lk4 * DA_LD;
  int vsz = Lk4 * DA_LD;
  if (bwd && Lq * ps > vsz) vsz = Lq * ps;           // dS [Lq][ps] takes V's place
  t.p = t.v + vsz;
  t.o = t.p + Lq * ps;
  t.total = t.o + (bwd ? Lq * DA_LD : 0);
  return t;
}

// accumulating, one fma chain (common.h's two-argument dot4 is the pairwise sum of products)
__device__ __forceinline__ float dot4(float4 a, float4 b, float acc) {
  return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, fmaf(a.x, b.x, acc))));
}

// DropCtx::mask1 with the key chosen by arithmetic (its k0 / k1 select otherwise becomes an indexed load from a stack copy)
__device__ __forceinline__ float keep1(const DropCtx& dc, uint64_t elem) {
  const uint32_t key = dc.k0 ^ ((dc.k0 ^ dc.k1) & (0u - (uint32_t)((elem >> 1) & 1)));
  const uint32_t r = mix32(dc.fold(elem >> 2) ^ key);
  return (((r >> (16 * (uint32_t)(elem & 1))) & 0xffffu) >= dc.thr) ? dc.scale : 0.f;
}

// rows [0, rows) x 64 columns of a global matrix -> fp32 LDS tile; rows [rows, rows_pad) are zeroed
template <typename T>
__device__ __forceinline__ void load_tile(float* dst, const T* src, int rows, int rows_pad, size_t ld) {
  for (int e = threadIdx.x; e < rows_pad * 16; e += 256) {
    const int r = e >> 4, c = (e & 15) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < rows) v = V4<T>::ld(src + (size_t)r * ld + c);
    *reinterpret_cast<float4*>(dst + r * DA_LD + c) = v;
  }
}

// acc[a][b] = <A[w + 4a], B[l + 64b]> for the rows below Lq (wave-uniform test); keys at or past Lk read row Lk - 1
__device__ __forceinline__ void dots(const float* A, const float* B, int Lq, int Lk, float (&acc)[16][2]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* b0 = B + min(lane, Lk - 1) * DA_LD;
  const float* b1 = B + min(lane + 64, Lk - 1) * DA_LD;
  const bool two = Lk > 64;
#pragma unroll
  for (int a = 0; a < 16; ++a) acc[a][0] = acc[a][1] = 0.f;
  for (int d = 0; d < 64; d += 4) {
    const float4 k0 = ldf4(b0 + d);
    const float4 k1 = two ? ldf4(b1 + d) : k0;
#pragma unroll
    for (int a = 0; a < 16; ++a) {
      const int i = wave + 4 * a;
      if (i < Lq) {
        const float4 qv = ldf4(A + i * DA_LD + d);
        acc[a][0] = dot4(qv, k0, acc[a][0]);
        if (two) acc[a][1] = dot4(qv, k1, acc[a][1]);
      }
    }
  }
}

// the score of (i, j) from its dot product: one function for forward and backward, so that both see the same bits
__device__ __forceinline__ float score(float dot, int i, int j, const DecAttn& a, const float* km) {
  float s = dot * a.scale;
  if (km) s += km[j];
  if (a.causal && j > i) s += DA_MASKED;
  return s;
}

// out[i][d .. d+3] = sum_j P[i][j] B[j][d .. d+3], d = 4 (t % 16), i = t / 16 + 16a; j in a fixed ascending order
__device__ __forceinline__ void rows_times(const float* P, int ps, const float* B, int Lq, int Lk4, float4 (&acc)[4]) {
  const int d = (threadIdx.x & 15) * 4, i0 = threadIdx.x >> 4;
  const float* prow[4];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    acc[a] = make_float4(0.f, 0.f, 0.f, 0.f);
    prow[a] = P + min(i0 + 16 * a, Lq - 1) * ps;
  }
  for (int j = 0; j < Lk4; j += 4) {
    const float4 b0 = ldf4(B + (j + 0) * DA_LD + d), b1 = ldf4(B + (j + 1) * DA_LD + d);
    const float4 b2 = ldf4(B + (j + 2) * DA_LD + d), b3 = ldf4(B + (j + 3) * DA_LD + d);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      if (16 * a < Lq) {
        const float4 p = ldf4(prow[a] + j);
        fma4(acc[a], p.x, b0); fma4(acc[a], p.y, b1); fma4(acc[a], p.z, b2); fma4(acc[a], p.w, b3);
      }
    }
  }
}

template <typename T>
__device__ __forceinline__ void store_rows(T* dst, size_t ld, int Lq, const float4 (&acc)[4]) {
  const int d = (threadIdx.x & 15) * 4, i0 = threadIdx.x >> 4;
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int i = i0 + 16 * a;
    if (i < Lq) V4<T>::st(dst + (size_t)i * ld + d, acc[a]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void dec_attn_fwd_kernel(DecAttn a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = blockIdx.x / a.H, h = blockIdx.x % a.H, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Lq = a.Lq, Lk = a.Lk, Lk4 = (Lk + 3) & ~3, ps = Lk4 + 4;
  const Tiles t = tiles(Lq, Lk, false);
  float *Qs = lds + t.q, *Ks = lds + t.k, *Vs = lds + t.v, *Ps = lds + t.p;
  load_tile<T>(Qs, static_cast<const T*>(a.q) + (size_t)n * Lq * a.ldq + h * 64, Lq, Lq, a.ldq);
  load_tile<T>(Ks, static_cast<const T*>(a.k) + (size_t)n * Lk * a.ldkv + h * 64, Lk, Lk4, a.ldkv);
  load_tile<T>(Vs, static_cast<const T*>(a.v) + (size_t)n * Lk * a.ldkv + h * 64, Lk, Lk4, a.ldkv);
  __syncthreads();
  float acc[16][2];
  dots(Qs, Ks, Lq, Lk, acc);
  const float* km = a.key_mask ? a.key_mask + (size_t)n * Lk : nullptr;
  const DropCtx dc(a.drop);
  float* stats = a.stats + (size_t)blockIdx.x * Lq * 2;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = wave + 4 * r;
    if (i < Lq) {                                                   // wave-uniform: the reductions run with every lane on
      const int j0 = lane, j1 = lane + 64;
      const float s0 = j0 < Lk ? score(acc[r][0], i, j0, a, km) : -3.0e38f;
      const float s1 = j1 < Lk ? score(acc[r][1], i, j1, a, km) : -3.0e38f;
      const float m = wave_max(fmaxf(s0, s1));
      const float e0 = j0 < Lk ? expf(s0 - m) : 0.f, e1 = j1 < Lk ? expf(s1 - m) : 0.f;
      const float inv = 1.f / wave_sum(e0 + e1);
      float p0 = e0 * inv, p1 = e1 * inv;
      if (lane == 0) *reinterpret_cast<float2*>(stats + 2 * i) = make_float2(m, inv);
      if (dc.on()) {
        const uint64_t base = ((uint64_t)blockIdx.x * Lq + i) * (uint64_t)Lk4;
        p0 *= keep1(dc, base + j0);
        p1 *= keep1(dc, base + j1);
      }
      if (j0 < Lk4) Ps[i * ps + j0] = p0;                            // zero in the columns [Lk, Lk4)
      if (j1 < Lk4) Ps[i * ps + j1] = p1;
    }
  }
  __syncthreads();
  float4 out[4];
  rows_times(Ps, ps, Vs, Lq, Lk4, out);
  store_rows<T>(static_cast<T*>(a.ctx) + (size_t)n * Lq * (a.H * 64) + h * 64, (size_t)a.H * 64, Lq, out);
}

template <typename T>
__global__ __launch_bounds__(256) void dec_attn_bwd_kernel(DecAttn a) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int n = blockIdx.x / a.H, h = blockIdx.x % a.H, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Lq = a.Lq, Lk = a.Lk, Lk4 = (Lk + 3) & ~3, ps = Lk4 + 4;
  const Tiles t = tiles(Lq, Lk, true);
  float *Qs = lds + t.q, *Ks = lds + t.k, *Vs = lds + t.v, *Ps = lds + t.p, *Os = lds + t.o, *dSs = Vs;
  const size_t qoff = (size_t)n * Lq * a.ldq + h * 64, kvoff = (size_t)n * Lk * a.ldkv + h * 64;
  load_tile<T>(Qs, static_cast<const T*>(a.q) + qoff, Lq, Lq, a.ldq);
  load_tile<T>(Ks, static_cast<const T*>(a.k) + kvoff, Lk, Lk4, a.ldkv);
  load_tile<T>(Vs, static_cast<const T*>(a.v) + kvoff, Lk, Lk4, a.ldkv);
  load_tile<T>(Os, static_cast<const T*>(a.dctx) + (size_t)n * Lq * (a.H * 64) + h * 64, Lq, Lq, (size_t)a.H * 64);
  __syncthreads();
  float p[16][2], g[16][2];                                         // P, then dropout(P);  dO V^T, then dS
  dots(Qs, Ks, Lq, Lk, p);
  dots(Os, Vs, Lq, Lk, g);
  const float* km = a.key_mask ? a.key_mask + (size_t)n * Lk : nullptr;
  const DropCtx dc(a.drop);
  const float* stats = a.stats + (size_t)blockIdx.x * Lq * 2;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = wave + 4 * r;
    if (i < Lq) {
      const int j0 = lane, j1 = lane + 64;
      const float2 st = *reinterpret_cast<const float2*>(stats + 2 * i);
      const float p0 = j0 < Lk ? expf(score(p[r][0], i, j0, a, km) - st.x) * st.y : 0.f;
      const float p1 = j1 < Lk ? expf(score(p[r][1], i, j1, a, km) - st.x) * st.y : 0.f;
      float m0 = 1.f, m1 = 1.f;
      if (dc.on()) {
        const uint64_t base = ((uint64_t)blockIdx.x * Lq + i) * (uint64_t)Lk4;
        m0 = keep1(dc, base + j0);
        m1 = keep1(dc, base + j1);
      }
      const float dp0 = j0 < Lk ? g[r][0] * m0 : 0.f, dp1 = j1 < Lk ? g[r][1] * m1 : 0.f;
      const float rs = wave_sum(p0 * dp0 + p1 * dp1);
      p[r][0] = p0 * m0;
      p[r][1] = p1 * m1;
      g[r][0] = p0 * (dp0 - rs) * a.scale;                          // d scores, times d scores / d <q, k>
      g[r][1] = p1 * (dp1 - rs) * a.scale;
    }
  }
  __syncthreads();                                                  // every wave is done with V: dS takes its place
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int i = wave + 4 * r;
    if (i < Lq) {
      if (lane < Lk4) { Ps[i * ps + lane] = p[r][0]; dSs[i * ps + lane] = g[r][0]; }
      if (lane + 64 < Lk4) { Ps[i * ps + lane + 64] = p[r][1]; dSs[i * ps + lane + 64] = g[r][1]; }
    }
  }
  __syncthreads();
  {
    float4 out[4];
    rows_times(dSs, ps, Ks, Lq, Lk4, out);                          // dQ = dS K
    store_rows<T>(static_cast<T*>(a.dq) + qoff, (size_t)a.ldq, Lq, out);
  }
  // dK[j] = sum_i dS[i][j] Q[i], dV[j] = sum_i dropout(P)[i][j] dO[i]: thread = 4 columns x 2 groups of 4 keys, i ascending
  const int d = (threadIdx.x & 15) * 4, jt = threadIdx.x >> 4;
  float4 dk[2][4], dv[2][4];
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c) dk[b][c] = dv[b][c] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int i = 0; i < Lq; ++i) {
    const float4 qv = ldf4(Qs + i * DA_LD + d), ov = ldf4(Os + i * DA_LD + d);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = (jt + 16 * b) * 4;
      if (j < Lk4) {
        const float4 ds = ldf4(dSs + i * ps + j), pd = ldf4(Ps + i * ps + j);
        fma4(dk[b][0], ds.x, qv); fma4(dk[b][1], ds.y, qv); fma4(dk[b][2], ds.z, qv); fma4(dk[b][3], ds.w, qv);
        fma4(dv[b][0], pd.x, ov); fma4(dv[b][1], pd.y, ov); fma4(dv[b][2], pd.z, ov); fma4(dv[b][3], pd.w, ov);
      }
    }
  }
  T* dK = static_cast<T*>(a.dk) + kvoff;
  T* dV = static_cast<T*>(a.dv) + kvoff;
#pragma unroll
  for (int b = 0; b < 2; ++b)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int j = (jt + 16 * b) * 4 + c;
      if (j < Lk) {
        V4<T>::st(dK + (size_t)j * a.ldkv + d, dk[b][c]);
        V4<T>::st(dV + (size_t)j * a.ldkv + d, dv[b][c]);
      }
    }
}

// ---- one query row per (caption, head): the attentions of an incremental decode step ------------------------------------------
// One wavefront owns a (caption, head) pair, a workgroup holds four pairs; there is no K / V tile in LDS - a key row is read
// once, by one lane, straight from global memory.  Lane l owns the keys l and l + 64: 64 dims against q, which the wave keeps
// as 64 floats in LDS (a broadcast read), in the summation order of `dots` above.  Row maximum and sum are the two DPP wave
// reductions, P goes to a per-wave LDS row, and for P V the lanes regroup as (key residue lane >> 4, dims 4 (lane & 15)): 16
// lanes read one V row coalesced, each residue sums its keys in ascending order, and the four partial float4s are added in
// the order 0, 1, 2, 3.  No atomics; every element of ctx is written.
//   cross mode   keys [0, Lk) at rows n * Lk + j of k / v (leading dimension ldkv), the caption's additive key mask
//   step mode    keys [0, t) at rows n * Tcap + j of the cache [N, Tcap, 2 * H * 64], key t from this step's Q|K|V row; the
//                wave also copies that row's K|V columns of its head into cache row t (bits, not values) and never reads them
//                back.  t comes from the host or from a device int32; a device t outside [0, Tcap) writes nothing to the
//                cache and zeros to ctx.
//   grouped      cross mode with group > 1: row n reads the keys, values and key mask of block n / group - the rows of one
//                caption's beams share the caption's encoder K|V, which are not replicated.
//   beam         step mode with a table anc [N, Tcap]: key / value j < t of row n come from cache row anc[n * Tcap + j] (clamped
//                into [0, N)) at position j - a beam reads its ancestors' rows where they were written, nothing is copied.  Every
//                wave still writes ITS row's K|V to position t, and no wave reads position t of the cache, so the rows of one
//                launch do not race.  The lane that owns key j keeps the row index in a per-wave LDS table for the P V loop.
constexpr int DR_WAVES = 4, DR_Q = 64, DR_P = DA_MAX_LK, DR_RED = 4 * 64, DR_ANC = DA_MAX_LK;
constexpr int DR_LDS = DR_Q + DR_P + DR_RED + DR_ANC;                                                      // 4-byte words per wave

struct DecRow {
  const void* q;           // [N, ldq], the head's 64 columns at h * 64
  const void *k, *v;       // rows (n * rows_n + j) * ldkv, the head's columns at h * 64 (cache: k = cache, v = cache + H * 64)
  const void *kt, *vt;     // step mode: this step's K and V row [N, ldq] (inside the packed Q|K|V buffer); NULL in cross mode
  void* cache;             // step mode: [N, Tcap, 2 * H * 64], row t is written
  const float* key_mask;   // cross mode: [N, Lk] additive or NULL
  void* ctx;               // [N, H * 64]
  const int* pos_dev;
  int pos, N, rows_n, H, ldq, ldkv;   // rows_n = Lk (cross) | Tcap (step)
  float scale;
  const int* anc;          // step mode: [N, Tcap] cache row of every earlier position, or NULL = the row's own
  int group;               // cross mode: rows per key / value block (1 = a block per row)
};

// 64-dim dot product of a global row with the wave's q in LDS, d ascending in groups of 4 as in `dots`; 16-byte loads
template <typename T> __device__ __forceinline__ float dot_row(const T* row, const float* qs);
template <> __device__ __forceinline__ float dot_row<float>(const float* row, const float* qs) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < 64; d += 4) acc = dot4(ldf4(qs + d), ldf4(row + d), acc);
  return acc;
}
template <> __device__ __forceinline__ float dot_row<bf16_t>(const bf16_t* row, const float* qs) {
  float acc = 0.f;
#pragma unroll
  for (int d = 0; d < 64; d += 8) {
    const uint4 u = *reinterpret_cast<const uint4*>(row + d);
    const float4 lo = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u),
                                  __uint_as_float(u.y << 16), __uint_as_float(u.y & 0xffff0000u));
    const float4 hi = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xffff0000u),
                                  __uint_as_float(u.w << 16), __uint_as_float(u.w & 0xffff0000u));
    acc = dot4(ldf4(qs + d), lo, acc);
    acc = dot4(ldf4(qs + d + 4), hi, acc);
  }
  return acc;
}

template <typename T, bool STEP>
__global__ __launch_bounds__(256) void dec_attn_row_kernel(DecRow a) {
  __shared__ __attribute__((aligned(16))) float lds[DR_WAVES * DR_LDS];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = blockIdx.x * DR_WAVES + wave;
  const bool active = pair < a.N * a.H;                             // wave-uniform; idle waves only keep the barriers company
  const int n = active ? pair / a.H : 0, h = active ? pair % a.H : 0;
  float *qs = lds + wave * DR_LDS, *ps = qs + DR_Q, *red = ps + DR_P;
  int* as = reinterpret_cast<int*>(red + DR_RED);                   // beam: the cache row of key j
  const int D = a.H * 64;
  T* out = static_cast<T*>(a.ctx) + (size_t)n * D + h * 64;
  int Lm = a.rows_n;                                                // keys read from memory
  if (STEP) {
    const int t = a.pos_dev ? *a.pos_dev : a.pos;
    if (t < 0 || t >= a.rows_n) {                                   // uniform over the grid: no barrier is reached by anyone
      if (active && lane < 16) V4<T>::st(out + 4 * lane, make_float4(0.f, 0.f, 0.f, 0.f));
      return;
    }
    Lm = t;
  }
  const int Lall = Lm + (STEP ? 1 : 0);                             // <= 128
  const size_t row0 = (size_t)n * a.rows_n;                         // the row's own block: the cache row that is written
  const int* anc = STEP ? a.anc : nullptr;                          // uniform over the grid
  const int nb = STEP ? n : n / a.group;                            // the block the keys come from (beam: per key, below)
  const size_t rowk = anc ? 0 : (size_t)nb * a.rows_n;
  const T* K = static_cast<const T*>(a.k) + rowk * a.ldkv + h * 64;
  const T* V = static_cast<const T*>(a.v) + rowk * a.ldkv + h * 64;
  const T* Kt = STEP ? static_cast<const T*>(a.kt) + (size_t)n * a.ldq + h * 64 : nullptr;
  const T* Vt = STEP ? static_cast<const T*>(a.vt) + (size_t)n * a.ldq + h * 64 : nullptr;
  if (active && lane < 16)
    *reinterpret_cast<float4*>(qs + 4 * lane) = V4<T>::ld(static_cast<const T*>(a.q) + (size_t)n * a.ldq + h * 64 + 4 * lane);
  if (STEP && active && lane < 32) {                                // cache row t <- this step's K | V columns of the head, bit for bit
    const int c = 4 * (lane & 15);
    const T* src = (lane < 16 ? Kt : Vt) + c;
    T* dst = static_cast<T*>(a.cache) + (row0 + Lm) * a.ldkv + (lane < 16 ? 0 : D) + h * 64 + c;
    if (sizeof(T) == 4) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
    else *reinterpret_cast<uint2*>(dst) = *reinterpret_cast<const uint2*>(src);
  }
  __syncthreads();
  if (active) {
    const float* km = (!STEP && a.key_mask) ? a.key_mask + (size_t)nb * a.rows_n : nullptr;
    float s[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = lane + 64 * b;
      s[b] = -3.0e38f;
      if (j < Lall) {
        size_t jr = j;
        if (anc && j < Lm) {
          const int src = min(max(anc[row0 + j], 0), a.N - 1);
          as[j] = src;
          jr = (size_t)src * a.rows_n + j;
        }
        const T* row = (STEP && j == Lm) ? Kt : K + jr * a.ldkv;
        s[b] = dot_row<T>(row, qs) * a.scale;
        if (km) s[b] += km[j];
      }
    }
    const float m = wave_max(fmaxf(s[0], s[1]));
    const float e0 = lane < Lall ? expf(s[0] - m) : 0.f, e1 = lane + 64 < Lall ? expf(s[1] - m) : 0.f;
    const float inv = 1.f / wave_sum(e0 + e1);
    ps[lane] = e0 * inv;                                            // zero behind the last key
    ps[lane + 64] = e1 * inv;
  }
  __syncthreads();
  const int r = lane >> 4, d = 4 * (lane & 15);
  if (active) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int j = r; j < Lall; j += 4) {
      const size_t jr = (anc && j < Lm) ? (size_t)as[j] * a.rows_n + j : (size_t)j;
      const T* row = (STEP && j == Lm) ? Vt : V + jr * a.ldkv;
      fma4(acc, ps[j], V4<T>::ld(row + d));
    }
    *reinterpret_cast<float4*>(red + r * 64 + d) = acc;
  }
  __syncthreads();
  if (active && lane < 16) {
    float4 o = ldf4(red + d);
#pragma unroll
    for (int g = 1; g < 4; ++g) {
      const float4 x = ldf4(red + g * 64 + d);
      o.x += x.x; o.y += x.y; o.z += x.z; o.w += x.w;
    }
    V4<T>::st(out + d, o);
  }
}

bool aligned16(const void* p);

int launch_row(const char* what, const DecRow& a, bool step, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(a.ldq % 8 == 0 && a.ldkv % 8 == 0 && a.ldq >= a.H * 64 && a.ldkv >= a.H * 64,
               "%s: leading dimensions must be multiples of 8 and at least H * 64: ldq=%d ldkv=%d H=%d", what, a.ldq, a.ldkv, a.H);
  HERO_REQUIRE((long long)a.N * a.H < (1ll << 31), "%s: N * H too large", what);
  HERO_REQUIRE(a.q && a.k && a.v && a.ctx && (!step || (a.kt && a.vt && a.cache)), "%s: null pointer", what);
  HERO_REQUIRE(aligned16(a.q) && aligned16(a.k) && aligned16(a.v) && aligned16(a.ctx), "%s: operands must be 16-byte aligned", what);
  const dim3 grid((a.N * a.H + DR_WAVES - 1) / DR_WAVES), block(64 * DR_WAVES);
  hipStream_t st = static_cast<hipStream_t>(stream);
  return by_dtype(dtype, what, [&](auto tag) {
    using T = typename decltype(tag)::type;
    if (step) hipLaunchKernelGGL((dec_attn_row_kernel<T, true>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dec_attn_row_kernel<T, false>), grid, block, 0, st, a);
  });
}

bool row_in_envelope(int dtype, int Lk) { return (dtype == HERO_F32 || dtype == HERO_BF16) && Lk >= 1 && Lk <= DA_MAX_LK; }

bool in_envelope(int dtype, int Lq, int Lk) {
  return (dtype == HERO_F32 || dtype == HERO_BF16) && Lq >= 1 && Lq <= DA_MAX_LQ && Lk >= 1 && Lk <= DA_MAX_LK;
}

bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }

int check(const char* what, const DecAttn& a, int N, int dtype) {
  HERO_REQUIRE(in_envelope(dtype, a.Lq, a.Lk) && a.H >= 1 && N >= 0,
               "%s: outside the envelope (fp32 / bf16, 1 <= Lq <= %d, 1 <= Lk <= %d, H >= 1, N >= 0): dtype=%d N=%d Lq=%d Lk=%d H=%d",
               what, DA_MAX_LQ, DA_MAX_LK, dtype, N, a.Lq, a.Lk, a.H);
  HERO_REQUIRE(a.ldq >= a.H * 64 && a.ldkv >= a.H * 64 && a.ldq % 8 == 0 && a.ldkv % 8 == 0,
               "%s: leading dimensions must be multiples of 8 and at least H * 64: ldq=%d ldkv=%d H=%d", what, a.ldq, a.ldkv, a.H);
  HERO_REQUIRE((long long)N * a.H < (1ll << 31), "%s: N * H too large", what);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_dec_attention_in_envelope(int dtype, int Lq, int Lk) { return in_envelope(dtype, Lq, Lk) ? 1 : 0; }

extern "C" int hero_dec_attention_row_in_envelope(int dtype, int Lk) { return row_in_envelope(dtype, Lk) ? 1 : 0; }

extern "C" int hero_dec_attention_row(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx, int N, int Lk,
                                      int H, int ldq, int ldkv, float scale, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(row_in_envelope(dtype, Lk) && H >= 1 && N >= 1,
               "hero_dec_attention_row: outside the envelope (fp32 / bf16, 1 <= Lk <= %d, H >= 1, N >= 1): dtype=%d N=%d Lk=%d H=%d",
               DA_MAX_LK, dtype, N, Lk, H);
  const DecRow a = {q, k, v, nullptr, nullptr, nullptr, key_mask_add, ctx, nullptr, 0, N, Lk, H, ldq, ldkv, scale, nullptr, 1};
  return launch_row("hero_dec_attention_row", a, false, dtype, stream);
}

extern "C" int hero_dec_attention_row_grouped(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx, int N,
                                              int group, int Lk, int H, int ldq, int ldkv, float scale, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(row_in_envelope(dtype, Lk) && H >= 1 && N >= 1 && group >= 1,
               "hero_dec_attention_row_grouped: outside the envelope (fp32 / bf16, 1 <= Lk <= %d, H >= 1, N >= 1, group >= 1): dtype=%d "
               "N=%d group=%d Lk=%d H=%d", DA_MAX_LK, dtype, N, group, Lk, H);
  const DecRow a = {q, k, v, nullptr, nullptr, nullptr, key_mask_add, ctx, nullptr, 0, N, Lk, H, ldq, ldkv, scale, nullptr, group};
  return launch_row("hero_dec_attention_row_grouped", a, false, dtype, stream);
}

static int step(const char* what, const void* qkv, void* kv_cache, const int* anc, void* ctx, const int* pos_dev, int pos, int N, int Tcap,
                int H, float scale, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(row_in_envelope(dtype, Tcap) && H >= 1 && N >= 1,
               "%s: outside the envelope (fp32 / bf16, 1 <= Tcap <= %d, H >= 1, N >= 1): dtype=%d N=%d Tcap=%d H=%d", what, DA_MAX_LK,
               dtype, N, Tcap, H);
  HERO_REQUIRE(pos_dev || (pos >= 0 && pos < Tcap), "%s: position %d outside [0, Tcap = %d)", what, pos, Tcap);
  HERO_REQUIRE(H <= (1 << 20), "%s: H too large", what);
  const int D = H * 64;
  const size_t es = dtype == HERO_F32 ? 4 : 2;
  const char* row = static_cast<const char*>(qkv);
  const DecRow a = {qkv, kv_cache, kv_cache ? static_cast<const char*>(kv_cache) + D * es : nullptr, qkv ? row + D * es : nullptr,
                    qkv ? row + 2 * D * es : nullptr, kv_cache, nullptr, ctx, pos_dev, pos, N, Tcap, H, 3 * D, 2 * D, scale, anc, 1};
  return launch_row(what, a, true, dtype, stream);
}

extern "C" int hero_dec_attention_step(const void* qkv, void* kv_cache, void* ctx, const int* pos_dev, int pos, int N, int Tcap, int H,
                                       float scale, int dtype, hero_stream_t stream) {
  return step("hero_dec_attention_step", qkv, kv_cache, nullptr, ctx, pos_dev, pos, N, Tcap, H, scale, dtype, stream);
}

extern "C" int hero_dec_attention_step_beam(const void* qkv, void* kv_cache, const int* anc, void* ctx, const int* pos_dev, int pos, int N,
                                            int Tcap, int H, float scale, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(anc, "hero_dec_attention_step_beam: null pointer");
  return step("hero_dec_attention_step_beam", qkv, kv_cache, anc, ctx, pos_dev, pos, N, Tcap, H, scale, dtype, stream);
}

extern "C" int hero_dec_attention_fwd(const void* q, const void* k, const void* v, const float* key_mask_add, void* ctx, float* stats,
                                      int N, int Lq, int Lk, int H, int ldq, int ldkv, int causal, float scale, int dtype,
                                      const HeroDropout* dropout, hero_stream_t stream) {
  DecAttn a = {q, k, v, key_mask_add, ctx, stats, nullptr, nullptr, nullptr, nullptr, Lq, Lk, H, ldq, ldkv, causal ? 1 : 0, scale,
               dropout ? *dropout : HeroDropout{nullptr, 0, 0, 1.f}};
  if (const int rc = check("hero_dec_attention_fwd", a, N, dtype)) return rc;
  if (N == 0) return HERO_OK;
  HERO_REQUIRE(q && k && v && ctx && stats, "hero_dec_attention_fwd: null pointer");
  HERO_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(ctx) && aligned16(stats),
               "hero_dec_attention_fwd: q, k, v, ctx and stats must be 16-byte aligned");
  const int lds = tiles(Lq, Lk, false).total * 4;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HERO_F32) {
    HERO_ENSURE_LDS((&dec_attn_fwd_kernel<float>), tiles(DA_MAX_LQ, DA_MAX_LK, false).total * 4, "dec_attn_fwd_kernel");
    hipLaunchKernelGGL((dec_attn_fwd_kernel<float>), dim3(N * H), dim3(256), lds, st, a);
  } else {
    HERO_ENSURE_LDS((&dec_attn_fwd_kernel<bf16_t>), tiles(DA_MAX_LQ, DA_MAX_LK, false).total * 4, "dec_attn_fwd_kernel");
    hipLaunchKernelGGL((dec_attn_fwd_kernel<bf16_t>), dim3(N * H), dim3(256), lds, st, a);
  }
  return check_launch("hero_dec_attention_fwd");
}

extern "C" int hero_dec_attention_bwd(const void* q, const void* k, const void* v, const float* key_mask_add, const float* stats,
                                      const void* dctx, void* dq, void* dk, void* dv, int N, int Lq, int Lk, int H, int ldq, int ldkv,
                                      int causal, float scale, int dtype, const HeroDropout* dropout, hero_stream_t stream) {
  DecAttn a = {q, k, v, key_mask_add, nullptr, const_cast<float*>(stats), dctx, dq, dk, dv, Lq, Lk, H, ldq, ldkv, causal ? 1 : 0, scale,
               dropout ? *dropout : HeroDropout{nullptr, 0, 0, 1.f}};
  if (const int rc = check("hero_dec_attention_bwd", a, N, dtype)) return rc;
  if (N == 0) return HERO_OK;
  HERO_REQUIRE(q && k && v && stats && dctx && dq && dk && dv, "hero_dec_attention_bwd: null pointer");
  HERO_REQUIRE(aligned16(q) && aligned16(k) && aligned16(v) && aligned16(stats) && aligned16(dctx) && aligned16(dq) && aligned16(dk) && aligned16(dv),
               "hero_dec_attention_bwd: q, k, v, stats, dctx, dq, dk and dv must be 16-byte aligned");
  const int lds = tiles(Lq, Lk, true).total * 4;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (dtype == HERO_F32) {
    HERO_ENSURE_LDS((&dec_attn_bwd_kernel<float>), tiles(DA_MAX_LQ, DA_MAX_LK, true).total * 4, "dec_attn_bwd_kernel");
    hipLaunchKernelGGL((dec_attn_bwd_kernel<float>), dim3(N * H), dim3(256), lds, st, a);
  } else {
    HERO_ENSURE_LDS((&dec_attn_bwd_kernel<bf16_t>), tiles(DA_MAX_LQ, DA_MAX_LK, true).total * 4, "dec_attn_bwd_kernel");
    hipLaunchKernelGGL((dec_attn_bwd_kernel<bf16_t>), dim3(N * H), dim3(256), lds, st, a);
  }
  return check_launch("hero_dec_attention_bwd");
}
