// Sampled decoding of the captioning decode (gfx950): one call per decode step draws the next token of R = N * S rows (row
// n * S + s = sample s of caption n) from the step's prediction scores [R, V] under temperature, top-k and top-p, and takes the
// tables of all rows to the next step, on the device, without a host read.
//
//   finished row   token = eos; cum, len unchanged; ids[r, t] = last[r] = eos; kept[r] = 0
//   live row       z_v = float(logit_v) * inv_temperature (one rounding).  Candidates are ordered by the composite of beam.hip /
//                  retrieval.hip, (order_bits(z_v) << 32) | ~v: larger z first, among equal z the lower token.
//     top-k        keep the first min(top_k, V) candidates in that order (0 = off)
//     top-p        masses exp(z_v - max z) over the survivors of top-k; keep the shortest prefix, in composite order, whose mass is
//                  >= top_p times the mass of all survivors, at least one candidate (>= 1 = off)
//     draw         Gumbel-max: the kept v that maximises z_v + g_v, ties by the same composite on the perturbed score, with
//                    base = splitmix64(seed ^ (site * 0xD6E8FEB86659FD93)),  site = (uint64)t * R + r
//                    h = mix32((uint32)v ^ (uint32)base) >> 9,  u = (2h + 1) * 2^-24,  g = -logf(-log1pf(-u))
//     update       cum[r] += logit_v - lse_r with lse_r the log-sum-exp of the RAW row (temperature 1, no filter: the model's own
//                  likelihood, what cum means in beam search); len[r] += 1; fin[r] = (v == eos); ids[r, t] = last[r] = v;
//                  kept[r] = the size of the kept set
// All arithmetic is fp32 whatever the storage dtype of the scores, except the masses of top-p: every mass is rounded ONCE to a
// 64-bit integer in units of 2^-40 and from there on only integers are added, so a sum does not depend on the order of its terms
// and its error is that of its terms (50 272 masses: below 5e-8 of the total, which is >= 1).
//
//   sample_rows_kernel  one workgroup of 256 threads per row.  Pass 1: the row's maximum and raw sum, online per thread, folded
//                       over the wave on the DPP network and over the four waves in a fixed order.  The kept set is the set of
//                       composites >= a threshold, found by a radix descent with 256-bin histograms (count, integer mass) in LDS:
//                       level 0 bins the distance to the maximum linearly (a monotone function of z that spreads a row over a
//                       hundred bins, where the exponent byte of z would pile it onto six), levels 1-4 the four bytes of
//                       order_bits(z) inside the chosen bin.  Counts serve top-k, masses serve top-p; with both filters the
//                       nucleus target needs the survivors' total first, so that case descends twice.  Only when the threshold
//                       value is shared by more candidates than are kept does a two-level descent on the token index find the
//                       last kept one.  The last pass is the Gumbel arg-max over the kept set.
// LDS integer atomics only, no floating-point atomics: two runs give the same bits.  The launch allocates nothing and reads
// nothing on the host; the seed is a device word and the step position a device int32 (a captured launch serves every seed and
// every step) or a host value.
#include "select_rows.h"

namespace hero {
namespace {

constexpr int SM_MAX_V = 65536, SM_MAX_T = 128, SM_NT = 256, SM_WAVES = SM_NT / 64, SM_BINS = 256;
constexpr float SM_FIX = 1099511627776.f;          // 2^40: the unit of an integer mass is 2^-40
constexpr float SM_BIN_SCALE = 4.f;                // level 0: bins of 1/4 in z below the maximum, the last one open-ended

typedef unsigned long long u64;

struct SampleSel {
  const void* logits;            // [R, ld]
  const u64* seed_dev;
  const int* pos_dev;
  float* cum;                    // [R]
  int *fin, *len, *ids, *last, *kept;   // [R], [R], [R, Tcap], [R], [R] | NULL
  int pos, N, S, V, ld, Tcap, eos, top_k, vec;
  float inv_t, top_p;
};

struct SampleLds {
  uint32_t cnt[SM_BINS];
  u64 mass[SM_BINS];
  uint32_t wave_c[SM_WAVES];
  u64 wave_m[SM_WAVES];
  int win_digit;
  uint32_t win_ca, win_cb;
  u64 win_ma, win_mb;
  float red_m[SM_WAVES], red_s[SM_WAVES];
  u64 red_c[SM_WAVES];
};

// what a descent found: the threshold key, count and mass of the candidates strictly above it and of those equal to it
struct Found {
  uint32_t key, cnt_above, cnt_eq;
  u64 mass_above, mass_eq, target;
};

__device__ __forceinline__ int bin0(float z, float zmax) {
  const float d = fminf(fmaxf((zmax - z) * SM_BIN_SCALE, 0.f), (float)(SM_BINS - 1));   // NaN -> 0
  return min(max((int)d, 0), SM_BINS - 1);
}
__device__ __forceinline__ u64 mass_of(float z, float zmax) { return __float2ull_rn(expf(z - zmax) * SM_FIX); }

// the smallest integer mass that is >= top_p * total (1 <= . <= total)
__device__ __forceinline__ u64 nucleus_target(float top_p, u64 total) {
  const u64 t = (u64)ceil((double)top_p * (double)total);
  return t < 1ull ? 1ull : (t > total ? total : t);
}

enum { SEL_COUNT = 0, SEL_MASS = 1, SEL_INDEX = 2 };

// Radix descent to the threshold: the key with  crit(above) false, crit(above + equal) true, candidates taken from the best.
//   SEL_COUNT  every element, crit = count >= target_cnt; the masses are added up only `with_mass` (a nucleus follows)
//   SEL_MASS   the elements above `floor_key` (all if !have_floor) plus `virt_cnt` virtual ones AT floor_key of total mass
//              virt_mass; crit = mass >= target_mass, which is the nucleus target of the total when passed as 0
//   SEL_INDEX  the elements whose key is floor_key, ordered by the token index ascending; crit = count >= target_cnt
template <typename T, int MODE>
__device__ Found descend(const SampleSel& a, const T* row, float zmax, SampleLds& sh, uint32_t floor_key, bool have_floor,
                         uint32_t virt_cnt, u64 virt_mass, uint32_t target_cnt, u64 target_mass, bool with_mass) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool vec = a.vec != 0;
  const int first = MODE == SEL_INDEX ? 1 : 0, last = MODE == SEL_INDEX ? 2 : 4;
  uint32_t prefix = 0, himask = 0, ca = 0, cb = 0;
  u64 ma = 0, mb = 0;
  int b0 = 0;
  for (int lvl = first; lvl <= last; ++lvl) {
    sh.cnt[tid] = 0;
    sh.mass[tid] = 0;
    __syncthreads();
    const int shift = 32 - 8 * lvl;
    auto add = [&](uint32_t key, float z, uint32_t c, u64 m_given, bool m_known) {
      int digit;
      if (lvl == 0) {
        digit = SM_BINS - 1 - bin0(z, zmax);
      } else {
        if (MODE != SEL_INDEX && bin0(z, zmax) != b0) return;
        if ((key ^ prefix) & himask) return;
        digit = (key >> shift) & 255u;
      }
      atomicAdd(&sh.cnt[digit], c);
      if (MODE != SEL_INDEX && with_mass) atomicAdd(&sh.mass[digit], m_known ? m_given : mass_of(z, zmax));
    };
    for_row<T, SM_NT>(row, a.V, vec, [&](int v, float x) {
      const float z = x * a.inv_t;
      const uint32_t key = order_bits(z);
      if (MODE == SEL_COUNT) {
        add(key, z, 1u, 0ull, false);
      } else if (MODE == SEL_MASS) {
        if (!have_floor || key > floor_key) add(key, z, 1u, 0ull, false);
      } else if (key == floor_key) {
        add((0xFFFFu - (uint32_t)v) << 16, 0.f, 1u, 0ull, true);
      }
    });
    if (MODE == SEL_MASS && tid == 0 && virt_cnt != 0) add(floor_key, order_float(floor_key), virt_cnt, virt_mass, true);
    __syncthreads();
    // thread i owns digit 255 - i: an inclusive scan over the threads adds the bins up from the best one down
    const int digit = SM_BINS - 1 - tid;
    const uint32_t c = sh.cnt[digit];
    const u64 m = sh.mass[digit];
    uint32_t ic = c;
    u64 im = m;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t tc = __shfl_up(ic, o, 64);
      const u64 tm = __shfl_up(im, o, 64);
      if (lane >= o) { ic += tc; im += tm; }
    }
    if (lane == 63) { sh.wave_c[wave] = ic; sh.wave_m[wave] = im; }
    __syncthreads();
    u64 tot_m = 0;
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) {
      if (w < wave) { ic += sh.wave_c[w]; im += sh.wave_m[w]; }
      tot_m += sh.wave_m[w];
    }
    if (MODE == SEL_MASS && target_mass == 0ull) target_mass = nucleus_target(a.top_p, ma + tot_m);   // level 0: the total
    const uint32_t c_in = ca + ic, c_ex = c_in - c;
    const u64 m_in = ma + im, m_ex = m_in - m;
    const bool before = MODE == SEL_MASS ? m_ex >= target_mass : c_ex >= target_cnt;
    const bool after = MODE == SEL_MASS ? m_in >= target_mass : c_in >= target_cnt;
    if (!before && (after || tid == SM_NT - 1)) {      // exactly one thread; the last bin takes what cannot happen
      sh.win_digit = digit;
      sh.win_ca = c_ex;
      sh.win_ma = m_ex;
      sh.win_cb = c;
      sh.win_mb = m;
    }
    __syncthreads();
    const int wd = sh.win_digit;
    ca = sh.win_ca; ma = sh.win_ma; cb = sh.win_cb; mb = sh.win_mb;
    if (lvl == 0) {
      b0 = SM_BINS - 1 - wd;
    } else {
      prefix |= (uint32_t)wd << shift;
      himask |= 255u << shift;
    }
  }
  return {prefix, ca, cb, ma, mb, target_mass};
}

template <typename T>
__global__ __launch_bounds__(SM_NT) void sample_rows_kernel(SampleSel a) {
  __shared__ SampleLds sh;
  const int t = step_position(a.pos_dev, a.pos);
  if (t < 0 || t >= a.Tcap) return;                                 // uniform over the grid: a device position cannot be refused on the host
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, V = a.V;
  if (a.fin[r] != 0) {                                              // uniform over the workgroup
    if (tid == 0) {
      a.ids[(size_t)r * a.Tcap + t] = a.eos;
      a.last[r] = a.eos;
      if (a.kept) a.kept[r] = 0;
    }
    return;
  }
  const T* row = static_cast<const T*>(a.logits) + (size_t)r * a.ld;
  const bool vec = a.vec != 0;
  const RowLse rl = row_lse<T, SM_NT>(row, V, vec, sh.red_m, sh.red_s);
  const float lse = rl.lse;
  const float zmax = rl.max * a.inv_t;                              // rounding is monotone: the maximum of z

  const uint32_t K = a.top_k > 0 ? (uint32_t)min(a.top_k, V) : (uint32_t)V;
  const bool have_k = K < (uint32_t)V, have_p = a.top_p < 1.f, all = !have_k && !have_p;
  uint32_t thr = 0, eq_take = 0, eq_real = 0, kept = (uint32_t)V;
  u64 floor_mass = 0, target = 0;
  if (have_k) {
    const Found f = descend<T, SEL_COUNT>(a, row, zmax, sh, 0u, false, 0u, 0ull, K, 0ull, have_p);
    thr = f.key;
    eq_real = f.cnt_eq;
    eq_take = min(max(K - f.cnt_above, 1u), max(f.cnt_eq, 1u));
    floor_mass = (f.mass_eq / max(f.cnt_eq, 1u)) * eq_take;         // equal z: equal integer masses
    target = nucleus_target(a.top_p, f.mass_above + floor_mass);
    kept = K;
  }
  if (have_p) {
    const Found f = descend<T, SEL_MASS>(a, row, zmax, sh, thr, have_k, eq_take, floor_mass, 0u, have_k ? target : 0ull, true);
    const uint32_t ce = max(f.cnt_eq, 1u);
    const u64 m1 = f.mass_eq / ce, need = f.target > f.mass_above ? f.target - f.mass_above : 1ull;
    const u64 e = m1 != 0ull ? (need + m1 - 1ull) / m1 : (u64)ce;
    if (!(have_k && f.key == thr)) eq_real = f.cnt_eq;              // at the top-k threshold the real elements were left out
    thr = f.key;
    eq_take = (uint32_t)(e < 1ull ? 1ull : (e > (u64)ce ? (u64)ce : e));
    kept = f.cnt_above + eq_take;
  }
  int v_cut = V;                                                    // among the candidates AT the threshold: tokens <= v_cut
  if (!all && eq_take < eq_real) {
    const Found f = descend<T, SEL_INDEX>(a, row, zmax, sh, thr, true, 0u, 0ull, eq_take, 0ull, false);
    v_cut = (int)(0xFFFFu - (f.key >> 16));
  }

  const u64 site = (u64)t * (u64)(a.N * a.S) + (u64)r;
  const uint32_t k32 = (uint32_t)splitmix64(*a.seed_dev ^ (site * 0xD6E8FEB86659FD93ull));
  u64 best = 0ull;
  for_row<T, SM_NT>(row, V, vec, [&](int v, float x) {
    const float z = x * a.inv_t;
    const uint32_t key = order_bits(z);
    if (all || key > thr || (key == thr && v <= v_cut)) {
      const uint32_t h = mix32((uint32_t)v ^ k32) >> 9;
      const float u = (float)(2u * h + 1u) * 5.9604644775390625e-8f;          // (2h + 1) * 2^-24: exact, in (0, 1)
      const float g = -logf(-log1pf(-u));
      const u64 c = compose(order_bits(z + g), (uint32_t)v);
      best = c > best ? c : best;
    }
  });
  best = wave_max_u64(best);
  if (lane == 0) sh.red_c[wave] = best;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 0; w < SM_WAVES; ++w) best = sh.red_c[w] > best ? sh.red_c[w] : best;
    const int v = min((int)(~(uint32_t)best & 0xFFFFu), V - 1);               // inside the row whatever happened above
    a.cum[r] = a.cum[r] + (ld1<T>(row + v) - lse);
    a.len[r] = a.len[r] + 1;
    a.fin[r] = v == a.eos ? 1 : 0;
    a.ids[(size_t)r * a.Tcap + t] = v;
    a.last[r] = v;
    if (a.kept) a.kept[r] = (int)kept;
  }
}

bool in_envelope(int dtype, int V, int Tcap) {
  return (dtype == HERO_F32 || dtype == HERO_BF16) && V >= 1 && V <= SM_MAX_V && Tcap >= 1 && Tcap <= SM_MAX_T;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_sample_in_envelope(int dtype, int V, int Tcap) { return in_envelope(dtype, V, Tcap) ? 1 : 0; }

extern "C" int hero_sample_select(const void* logits, float* cum, int* fin, int* len, int* ids, int* last, int* kept,
                                  const unsigned long long* seed_dev, const int* pos_dev, int pos, int N, int S, int V, int ld, int Tcap,
                                  int eos, float inv_temperature, int top_k, float top_p, int dtype, hero_stream_t stream) {
  HERO_REQUIRE(in_envelope(dtype, V, Tcap) && N >= 1 && S >= 1 && ld >= V && eos >= 0 && eos < V && (long long)N * S < (1ll << 24) &&
                   top_k >= 0 && top_p > 0.f && inv_temperature > 0.f && inv_temperature <= 3.0e38f,
               "hero_sample_select: outside the envelope (fp32 / bf16, N, S >= 1, 1 <= V <= %d, 1 <= Tcap <= %d, ld >= V, 0 <= eos < V, "
               "top_k >= 0, top_p > 0, inv_temperature finite and > 0): dtype=%d N=%d S=%d V=%d ld=%d Tcap=%d eos=%d top_k=%d top_p=%g "
               "inv_temperature=%g", SM_MAX_V, SM_MAX_T, dtype, N, S, V, ld, Tcap, eos, top_k, (double)top_p, (double)inv_temperature);
  HERO_REQUIRE(logits && cum && fin && len && ids && last && seed_dev, "hero_sample_select: null pointer");
  HERO_REQUIRE(pos_dev || (pos >= 0 && pos < Tcap), "hero_sample_select: position %d outside [0, Tcap = %d)", pos, Tcap);
  HERO_REQUIRE((((uintptr_t)seed_dev) & 7) == 0, "hero_sample_select: the seed word must be 8-byte aligned");
  const SampleSel a = {logits, seed_dev, pos_dev, cum, fin, len, ids, last, kept, pos, N, S, V, ld, Tcap, eos, top_k,
                       rows_vec4(logits, ld, dtype), inv_temperature, top_p};
  return by_dtype(dtype, "hero_sample_select", [&](auto tag) {
    hipLaunchKernelGGL((sample_rows_kernel<typename decltype(tag)::type>), dim3(N * S), dim3(SM_NT), 0, static_cast<hipStream_t>(stream), a);
  });
}
