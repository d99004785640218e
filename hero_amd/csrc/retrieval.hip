// Full-corpus moment retrieval (gfx950): per-row top-k, start / end probabilities of selected (query, video) pairs, and
// the top-n (video, start, end) moments of a query - the device side of eval_vcmr.py:232-323 (VR, SVMR, VCMR).
//
// The reference materialises start x end x video-score products for every (query, video, start, end), multiplies them by a
// band mask and sorts all of them to keep the first 200.  Here the products exist only in registers: a workgroup owns a
// query, recomputes the in-band products from the [K, L] probability rows on every pass and SELECTS instead of sorting.
//
// One selection routine (select_top) serves both hero_topk_rows and hero_moment_topk.  Every candidate has a 64-bit
// composite  (order-preserving bits of its fp32 score) << 32 | ~index : composites are unique, larger = better score, and
// among equal scores the lower index.  The top `n` composites are found by a most-significant-digit radix select - up to six
// histogram passes of 11 / 11 / 10 bits over the score and 11 / 11 / 10 over the index, in the LDS with INTEGER atomics; it stops
// at the first digit whose threshold bin holds exactly what is still missing, so the index digits are only walked when the
// n-th score is tied - then one pass collects the survivors and a bitonic sort of the <= 1024 composites orders them.
// Exact (the same multiset of scores as a full sort), deterministic (the collection order is arbitrary, the sort key is
// unique), no floating-point atomics.  LDS: 8 KB of histogram + 8 KB of survivors + 80 bytes, whatever K and L are - the
// probability rows are read through the L1 / L2 (80 KB per query at the TVR shape, 256 KB at the envelope corner: the
// latter does not fit the 160 KB LDS of a CU, so the rows are not staged at all).
#include "common.h"

namespace hero {
namespace {

constexpr int SEL_BINS = 2048;     // 11-bit digits
constexpr int SEL_CAP = 1024;      // survivors: top_n <= 1024

struct SelShared {
  uint32_t hist[SEL_BINS];
  unsigned long long buf[SEL_CAP];
  int wsum[16];
  int bin, above, cnt, count;
};

// inclusive scan over the NT threads of the workgroup (thread order); total = the sum over all of them
template <int NT>
__device__ __forceinline__ int block_incl_scan(int v, int* wsum, int& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  if (lane == 63) wsum[wave] = v;
  __syncthreads();
  int base = 0;
  total = 0;
#pragma unroll
  for (int w = 0; w < NT / 64; ++w) {
    const int s = wsum[w];
    if (w < wave) base += s;
    total += s;
  }
  __syncthreads();
  return v + base;
}

// The `top` best candidates of `src`, best first, to val / idx [top]; slots beyond the candidate count get val 0, idx -1.
// src.for_each(f) calls f(order_bits(score), index) once per candidate, in any order and any distribution over the threads,
// and gives the same candidates every time it is called.  alpha != 0: val = exp(alpha * score) (monotone: selected on score).
// All NT threads of the workgroup call it together; top <= SEL_CAP.
template <int NT, class Src>
__device__ void select_top(const Src& src, int top, SelShared& sh, float alpha, float* val, int* idx) {
  static_assert(SEL_BINS % NT == 0 && NT % 64 == 0 && NT <= 1024, "a thread owns SEL_BINS / NT bins");
  constexpr int BPT = SEL_BINS / NT;
  const int tid = threadIdx.x;
  unsigned long long prefix = 0ull, pmask = 0ull;
  int remaining = top, n_out = top;
  for (int p = 0; p < 6; ++p) {
    const int bits = (p % 3 == 2) ? 10 : 11;
    const int shift = p == 0 ? 53 : p == 1 ? 42 : p == 2 ? 32 : p == 3 ? 21 : p == 4 ? 10 : 0;
    const unsigned long long dmask = (1ull << bits) - 1ull;
    for (int i = tid; i < SEL_BINS; i += NT) sh.hist[i] = 0u;
    __syncthreads();
    src.for_each([&](uint32_t key, uint32_t id) {
      const unsigned long long comp = compose(key, id);
      if ((comp & pmask) == prefix) atomicAdd(&sh.hist[(int)((comp >> shift) & dmask)], 1u);
    });
    __syncthreads();
    int ts = 0;                                  // thread 0 owns the TOP bins: the scan runs from the best digit down
#pragma unroll
    for (int u = 0; u < BPT; ++u) ts += (int)sh.hist[SEL_BINS - 1 - (tid * BPT + u)];
    int total;
    const int incl = block_incl_scan<NT>(ts, sh.wsum, total);
    if (p == 0 && total <= top) {                // fewer candidates than slots: all of them
      n_out = total;
      break;
    }
    const int excl = incl - ts;
    if (excl < remaining && remaining <= incl) { // exactly one thread: the threshold bin is one of its bins
      int cum = excl;
      for (int u = 0; u < BPT; ++u) {
        const int b = SEL_BINS - 1 - (tid * BPT + u);
        const int h = (int)sh.hist[b];
        if (cum + h >= remaining) { sh.bin = b; sh.above = cum; sh.cnt = h; break; }
        cum += h;
      }
    }
    __syncthreads();
    remaining -= sh.above;
    prefix |= (unsigned long long)sh.bin << shift;
    pmask |= dmask << shift;
    if (sh.cnt == remaining) break;              // the whole threshold bin is in: no finer digit needed
  }
  if (tid == 0) sh.count = 0;
  __syncthreads();
  src.for_each([&](uint32_t key, uint32_t id) {
    const unsigned long long comp = compose(key, id);
    if ((comp & pmask) >= prefix) {
      const int pos = atomicAdd(&sh.count, 1);
      if (pos < SEL_CAP) sh.buf[pos] = comp;
    }
  });
  int P = 1;
  while (P < n_out) P <<= 1;
  __syncthreads();
  for (int i = n_out + tid; i < P; i += NT) sh.buf[i] = 0ull;      // below every real composite (an index is never 2^32 - 1)
  __syncthreads();
  for (int k = 2; k <= P; k <<= 1) {             // bitonic sort, descending
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < P; i += NT) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = sh.buf[i], b = sh.buf[l];
          const bool desc = (i & k) == 0;
          if (desc ? a < b : a > b) { sh.buf[i] = b; sh.buf[l] = a; }
        }
      }
      __syncthreads();
    }
  }
  for (int i = tid; i < top; i += NT) {
    float v = 0.f;
    int id = -1;
    if (i < n_out) {
      const unsigned long long comp = sh.buf[i];
      const float s = order_float((uint32_t)(comp >> 32));
      v = alpha != 0.f ? expf(alpha * s) : s;
      id = (int)~(uint32_t)comp;
    }
    val[i] = v;
    idx[i] = id;
  }
}

// ------------------------------------------------------------------------------------------------
// A. top-k of every row
// ------------------------------------------------------------------------------------------------
struct RowSrc {
  const float* s;
  int n;
  template <class F> __device__ __forceinline__ void for_each(F f) const {
    for (int c = threadIdx.x; c < n; c += blockDim.x) f(order_bits(s[c]), (uint32_t)c);
  }
};

constexpr int TOPK_NT = 256;
__global__ __launch_bounds__(TOPK_NT) void topk_rows_kernel(const float* scores, int N, int ld, int k, float alpha, float* val, int* idx) {
  __shared__ SelShared sh;
  const int row = blockIdx.x;
  RowSrc src;
  src.s = scores + (size_t)row * ld;
  src.n = N;
  select_top<TOPK_NT>(src, k, sh, alpha, val + (size_t)row * k, idx + (size_t)row * k);
}

// ------------------------------------------------------------------------------------------------
// B. start / end probabilities of the selected (query, video) pairs: one wave per pair, four pairs per workgroup
// ------------------------------------------------------------------------------------------------
constexpr int PROB_MAXK = 15;
constexpr int PROB_MAXL = 1024;

struct ProbArgs {
  const float* sim; const float* mask; const int* sel; const float* w_st; const float* w_ed;
  float* st_prob; float* ed_prob;
  long long ld_sim;
  int pairs, Nv, K, L, taps;
};

__global__ __launch_bounds__(256) void st_ed_probs_kernel(ProbArgs a) {
  extern __shared__ float sm[];                      // per wave: sim[L], lg[2][L]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int pair = blockIdx.x * 4 + wave;
  float* sim = sm + (size_t)wave * 3 * a.L;
  float* lg = sim + a.L;
  const bool live = pair < a.pairs;
  int v = -1;
  if (live) {
    v = a.sel[pair];
    if (v >= a.Nv) v = -1;
  }
  const int q = live ? pair / a.K : 0;
  if (v >= 0) {
    const float* row = a.sim + (size_t)q * a.ld_sim + (size_t)v * a.L;
    for (int l = lane; l < a.L; l += 64) sim[l] = row[l];
  }
  __syncthreads();
  if (v >= 0) {
    const int half = a.taps / 2;
    for (int i = lane; i < 2 * a.L; i += 64) {       // both convolutions over the whole row (zero padding taps / 2) + mask_logits
      const int which = i >= a.L, l = i - which * a.L;
      const float* w = which ? a.w_ed : a.w_st;
      float acc = 0.f;
      for (int k = 0; k < a.taps; ++k) {
        const int j = l + k - half;
        if (j >= 0 && j < a.L) acc = fmaf(w[k], sim[j], acc);
      }
      const float mk = a.mask[(size_t)v * a.L + l];
      lg[i] = acc * mk + (1.f - mk) * -10000.f;       // model/modeling_utils.py:42-43
    }
  }
  __syncthreads();
  if (!live) return;
  for (int which = 0; which < 2; ++which) {
    float* out = (which ? a.ed_prob : a.st_prob) + (size_t)pair * a.L;
    if (v < 0) {                                     // no video in this slot: a row of zeros
      for (int l = lane; l < a.L; l += 64) out[l] = 0.f;
      continue;
    }
    const float* x = lg + which * a.L;
    float mx = -3.0e38f;
    for (int l = lane; l < a.L; l += 64) mx = fmaxf(mx, x[l]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int l = lane; l < a.L; l += 64) sum += expf(x[l] - mx);
    sum = wave_sum(sum);
    for (int l = lane; l < a.L; l += 64) out[l] = expf(x[l] - mx) / sum;
  }
}

// ------------------------------------------------------------------------------------------------
// C. the top-n moments of a query: candidates (j, m, n) with min_l <= n - m < max_l, n < L (the ones of
//    generate_min_max_length_mask, utils/tvr_eval_utils.py:237-260), score st[j, m] * w[j] * ed[j, n], index (j L + m) L + n
// ------------------------------------------------------------------------------------------------
struct MomentSrc {
  const float* st; const float* ed; const float* w;
  int K, L, min_l, W;                                // W = max_l - min_l: band width
  // a group of 16 lanes walks a (video, start) row: its st * w factor is loaded once, the ends are consecutive floats
  template <class F> __device__ __forceinline__ void for_each(F f) const {
    const int g = threadIdx.x >> 4, d0 = threadIdx.x & 15, ng = blockDim.x >> 4;
    const int rows = K * L;
    for (int r = g; r < rows; r += ng) {
      const int j = r / L, m = r - j * L;
      const int n0 = m + min_l;
      const int cnt = min(W, L - n0);
      if (cnt <= 0) continue;
      const float sw = st[r] * w[j];
      const float* e = ed + (size_t)j * L + n0;
      for (int d = d0; d < cnt; d += 16) f(order_bits(sw * e[d]), (uint32_t)(r * L + n0 + d));
    }
  }
};

constexpr int MOMENT_NT = 1024;
__global__ __launch_bounds__(MOMENT_NT) void moment_topk_kernel(const float* st, const float* ed, const float* w, int K, int L, int min_l, int max_l,
                                                              int top_n, float* score, int* flat) {
  __shared__ SelShared sh;
  const int q = blockIdx.x;
  MomentSrc src;
  src.st = st + (size_t)q * K * L;
  src.ed = ed + (size_t)q * K * L;
  src.w = w + (size_t)q * K;
  src.K = K; src.L = L; src.min_l = min_l; src.W = max_l - min_l;
  select_top<MOMENT_NT>(src, top_n, sh, 0.f, score + (size_t)q * top_n, flat + (size_t)q * top_n);
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_topk_rows(const float* scores, int M, int N, int ld, int k, float alpha, float* val, int* idx, hero_stream_t stream) {
  HERO_REQUIRE(scores && val && idx, "hero_topk_rows: null pointer");
  HERO_REQUIRE(N >= 1 && N <= 65536 && ld >= N && k >= 1 && k <= 128, "hero_topk_rows: need 1 <= N <= 65536, ld >= N, 1 <= k <= 128 (N=%d ld=%d k=%d)",
               N, ld, k);
  if (M <= 0) return HERO_OK;
  hipLaunchKernelGGL(topk_rows_kernel, dim3(M), dim3(TOPK_NT), 0, static_cast<hipStream_t>(stream), scores, N, ld, k, alpha, val, idx);
  return check_launch("hero_topk_rows");
}

extern "C" int hero_st_ed_probs(const float* sim, long long ld_sim, const float* mask, const int* sel, const float* w_st, const float* w_ed, int Nq,
                                int Nv, int K, int L, int taps, float* st_prob, float* ed_prob, hero_stream_t stream) {
  HERO_REQUIRE(sim && mask && sel && w_st && w_ed && st_prob && ed_prob, "hero_st_ed_probs: null pointer");
  HERO_REQUIRE(L >= 1 && L <= PROB_MAXL && Nv >= 1 && K >= 1 && ld_sim >= (long long)Nv * L, "hero_st_ed_probs: bad dims Nv=%d K=%d L=%d ld_sim=%lld",
               Nv, K, L, ld_sim);
  HERO_REQUIRE(taps >= 1 && taps <= PROB_MAXK && (taps & 1), "hero_st_ed_probs: odd filters of at most %d taps (got %d)", PROB_MAXK, taps);
  if (Nq <= 0) return HERO_OK;
  HERO_REQUIRE((long long)Nq * K < (1ll << 31), "hero_st_ed_probs: Nq * K too large");
  ProbArgs a;
  a.sim = sim; a.mask = mask; a.sel = sel; a.w_st = w_st; a.w_ed = w_ed; a.st_prob = st_prob; a.ed_prob = ed_prob;
  a.ld_sim = ld_sim; a.pairs = Nq * K; a.Nv = Nv; a.K = K; a.L = L; a.taps = taps;
  hipLaunchKernelGGL(st_ed_probs_kernel, dim3((a.pairs + 3) / 4), dim3(256), (size_t)12 * L * sizeof(float), static_cast<hipStream_t>(stream), a);
  return check_launch("hero_st_ed_probs");
}

extern "C" int hero_moment_topk(const float* st_prob, const float* ed_prob, const float* w, int Nq, int K, int L, int min_l, int max_l, int top_n,
                                float* score, int* flat, hero_stream_t stream) {
  HERO_REQUIRE(st_prob && ed_prob && w && score && flat, "hero_moment_topk: null pointer");
  HERO_REQUIRE(L >= 1 && L <= 256 && K >= 1 && K <= 128 && top_n >= 1 && top_n <= SEL_CAP,
               "hero_moment_topk: need 1 <= L <= 256, 1 <= K <= 128, 1 <= top_n <= %d (L=%d K=%d top_n=%d)", SEL_CAP, L, K, top_n);
  HERO_REQUIRE(min_l >= 0 && max_l > min_l, "hero_moment_topk: need 0 <= min_l < max_l (min_l=%d max_l=%d)", min_l, max_l);
  if (Nq <= 0) return HERO_OK;
  hipLaunchKernelGGL(moment_topk_kernel, dim3(Nq), dim3(MOMENT_NT), 0, static_cast<hipStream_t>(stream), st_prob, ed_prob, w, K, L, min_l, max_l, top_n,
                     score, flat);
  return check_launch("hero_moment_topk");
}
