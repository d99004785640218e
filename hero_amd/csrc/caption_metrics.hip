// Caption metrics on the device (gfx950): one launch scores M caption rows - the id rows the decoders leave - against the references
// of their clips: BLEU's integer statistics, ROUGE-L and CIDEr-D as eval/pycocoevalcap computes them on words (include/hero_hip.h
// "Caption metrics" has the definitions).  Token ids are below 65536, so the n-grams of order 1..4 pack into ONE signed 64-bit key
// exactly, key = ((t0 << 16 | t1) << 16 | t2) << 16 | t3: no hashing, no collisions.  A 4-gram whose first token is >= 32768 has a
// negative key; the reference tables come out of a signed sort, so every comparison in here is signed too.
//
// The reference side is one packed buffer built once by hero_amd.caption.CaptionRefs (8-byte aligned; the header's 64-bit words):
//   0 magic   1 C clips   2 R references   3 ld of the padded ids   4 log(C_idf) as double bits      byte offsets of
//   5 clip_ref [C + 1] i32 first reference of a clip   6 ref_len [R] i32   7 ref_norm [R, 4] f64   8 ref_ids [R, ld] i32   9 bytes
//   per order n = 1..4 at words 10 + 8 (n - 1) ..:
//     +0 cm_off [C + 1] i32, +1 cm_key i64, +2 cm_cnt i32   a clip's n-grams, sorted, with the LARGEST count among its references
//     +3 rw_off [R + 1] i32, +4 rw_key i64, +5 rw_cnt i32   a reference's n-grams, sorted, with their counts
//     +6 idf_key i64, +7 idf_val f64                        the idf corpus' n-grams, sorted, idf = log C - log df as float64
//   42 + (n - 1): the number of idf keys of order n.          An n-gram the idf corpus does not hold has df 0: idf = log C.
// All three lookups are binary searches.
//
// caption_score_kernel: one wavefront per row.  The row's caption is what stands before its first `eos` within Tcap; the tokens
// go to LDS.  Lanes 0 .. R-1 each take one reference: its length for BLEU's closest reference length, and its LCS with the
// caption by the bit-parallel recurrence V' = (V + (V & M)) | (V & ~M) on 128 bits (the LCS is the number of zero bits).  Per
// order the caption's keys go to LDS; lane i owns positions i and i + 64, counts its key among all positions and keeps it if no
// earlier position holds the same key - the deduplication.  A kept key is looked up in the clip's table (BLEU's clipped count;
// an n-gram that no reference of the clip has is not searched per reference), in the idf table, and, reference by reference, in
// the reference's table.  CIDEr's dot products and squared norms are float64, folded over the wave by xor shuffles in a fixed
// order.  No atomics, nothing allocated, nothing read on the host: two runs give the same bits, and the launch can be captured.
// A row whose clip index is outside [0, C) gets zeros.
#include "common.h"

namespace hero {
namespace {

constexpr int CP_MAX_T = 128, CP_MAX_V = 65536, CP_MAX_R = 32, CP_NT = 64, CP_STATS = 10;
constexpr long long CP_MAGIC = 0x4845524F43415031ll;

struct CapScore {
  const void* ids;               // [M, ld] int32 or int64
  const int* clip;               // [M]
  const unsigned char* refs;     // the packed reference tables
  int* stats;                    // [M, ld_stats]
  float *rouge, *cider;          // [M]
  int* lcs;                      // [M] or null
  int M, ld, ld_stats, Tcap, eos, i64;
};

__device__ __forceinline__ int cap_wave_sum(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int cap_wave_min(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ int cap_wave_max(int v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ double cap_wave_sum(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ double cap_wave_max(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m));
  return v;
}

// The index of `k` in the sorted keys[lo, hi), or -1.  Signed comparison: the order torch.sort gave the table.
__device__ __forceinline__ int find_key(const long long* keys, int lo, int hi, long long k) {
  const int end = hi;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return (lo < end && keys[lo] == k) ? lo : -1;
}

__global__ __launch_bounds__(CP_NT) void caption_score_kernel(CapScore a) {
  __shared__ int h[CP_MAX_T];
  __shared__ long long keys[CP_MAX_T];
  const int row = blockIdx.x, lane = threadIdx.x;
  const long long* hdr = reinterpret_cast<const long long*>(a.refs);
  const int C = (int)hdr[1], Lr = (int)hdr[3];
  const int c = a.clip[row];
  int* st = a.stats + (size_t)row * a.ld_stats;
  if (hdr[0] != CP_MAGIC || c < 0 || c >= C) {                       // uniform over the wave
    if (lane < CP_STATS) st[lane] = 0;
    if (lane == 0) {
      a.rouge[row] = 0.f;
      a.cider[row] = 0.f;
      if (a.lcs) a.lcs[row] = 0;
    }
    return;
  }
  const double logC = __longlong_as_double(hdr[4]);
  const int* clip_ref = reinterpret_cast<const int*>(a.refs + hdr[5]);
  const int* ref_len = reinterpret_cast<const int*>(a.refs + hdr[6]);
  const double* ref_norm = reinterpret_cast<const double*>(a.refs + hdr[7]);
  const int* ref_ids = reinterpret_cast<const int*>(a.refs + hdr[8]);

  // the caption: everything before the first eos within Tcap (what follows is junk: it reaches LDS and no count)
  int first = a.Tcap;
  for (int i = lane; i < a.Tcap; i += CP_NT) {
    const size_t e = (size_t)row * a.ld + i;
    const int v = a.i64 ? (int)static_cast<const long long*>(a.ids)[e] : static_cast<const int*>(a.ids)[e];
    h[i] = v;
    if (v == a.eos) first = min(first, i);
  }
  const int L = cap_wave_min(first);
  __syncthreads();

  const int r0 = clip_ref[c], R = min(clip_ref[c + 1] - r0, CP_MAX_R);
  // one reference per lane: the closest reference length (among equidistant ones the shorter) and the LCS
  int len_key = 0x7fffffff, my_lcs = 0, my_len = 1;
  if (lane < R) {
    my_len = ref_len[r0 + lane];
    len_key = abs(my_len - L) * 256 + my_len;
    const int* rt = ref_ids + (size_t)(r0 + lane) * Lr;
    unsigned long long v_lo = ~0ull, v_hi = ~0ull;
    const int l_lo = min(L, 64);
    for (int j = 0; j < my_len; ++j) {
      const int t = rt[j];
      unsigned long long m_lo = 0ull, m_hi = 0ull;
      for (int i = 0; i < l_lo; ++i) m_lo |= (unsigned long long)(h[i] == t) << i;
      for (int i = 64; i < L; ++i) m_hi |= (unsigned long long)(h[i] == t) << (i - 64);
      const unsigned long long u_lo = v_lo & m_lo, u_hi = v_hi & m_hi;
      const unsigned long long s_lo = v_lo + u_lo, s_hi = v_hi + u_hi + (s_lo < v_lo ? 1ull : 0ull);
      v_lo = s_lo | (v_lo & ~m_lo);
      v_hi = s_hi | (v_hi & ~m_hi);
    }
    const unsigned long long k_lo = L >= 64 ? ~0ull : ((1ull << L) - 1ull);
    const unsigned long long k_hi = L >= 128 ? ~0ull : (L > 64 ? ((1ull << (L - 64)) - 1ull) : 0ull);
    my_lcs = __popcll(~v_lo & k_lo) + __popcll(~v_hi & k_hi);
  }
  const int reflen = cap_wave_min(len_key) & 255;
  const int best_lcs = cap_wave_max(my_lcs);
  const double q = cap_wave_max(lane < R ? (double)my_lcs / (double)my_len : 0.0);
  const double p = (double)best_lcs / (double)max(L, 1);
  const double rouge = (p != 0.0 && q != 0.0) ? (1.0 + 1.44) * p * q / (q + 1.44 * p) : 0.0;

  int correct[4] = {0, 0, 0, 0};
  double score = 0.0;
  for (int n = 1; n <= 4; ++n) {
    const int P = L - n + 1;                                           // uniform
    if (P <= 0) break;
    const long long* w = hdr + 10 + 8 * (n - 1);
    const int* cm_off = reinterpret_cast<const int*>(a.refs + w[0]);
    const long long* cm_key = reinterpret_cast<const long long*>(a.refs + w[1]);
    const int* cm_cnt = reinterpret_cast<const int*>(a.refs + w[2]);
    const int* rw_off = reinterpret_cast<const int*>(a.refs + w[3]);
    const long long* rw_key = reinterpret_cast<const long long*>(a.refs + w[4]);
    const int* rw_cnt = reinterpret_cast<const int*>(a.refs + w[5]);
    const long long* idf_key = reinterpret_cast<const long long*>(a.refs + w[6]);
    const double* idf_val = reinterpret_cast<const double*>(a.refs + w[7]);
    const int n_idf = (int)hdr[42 + (n - 1)];
    __syncthreads();                                                   // the keys of the order before have been read
    for (int i = lane; i < P; i += CP_NT) {
      unsigned long long k = (unsigned long long)(h[i] & 0xffff);       // packed unsigned, compared signed
      for (int j = 1; j < n; ++j) k = (k << 16) | (unsigned long long)(h[i + j] & 0xffff);
      keys[i] = (long long)k;
    }
    __syncthreads();
    long long key[2] = {0, 0};
    double wh[2] = {0.0, 0.0}, idf[2] = {0.0, 0.0};
    bool in_clip[2] = {false, false};
    int hit = 0;
    double nh2 = 0.0;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const int i = lane + s * CP_NT;
      if (s * CP_NT >= P) break;                                       // uniform: the second slot only past 64 positions
      const long long k = i < P ? keys[i] : 0;
      int cnt = 0;
      bool firstocc = i < P;
      for (int j = 0; j < P; ++j) {
        const bool e = keys[j] == k;
        cnt += e ? 1 : 0;
        firstocc = firstocc && !(e && j < i);
      }
      if (firstocc) {
        const int at = find_key(cm_key, cm_off[c], cm_off[c + 1], k);
        if (at >= 0) hit += min(cnt, cm_cnt[at]);
        const int ai = find_key(idf_key, 0, n_idf, k);
        key[s] = k;
        idf[s] = ai >= 0 ? idf_val[ai] : logC;
        wh[s] = (double)cnt * idf[s];
        nh2 += wh[s] * wh[s];
        in_clip[s] = at >= 0;
      }
    }
    correct[n - 1] = cap_wave_sum(hit);
    const double nh = sqrt(cap_wave_sum(nh2));
    if (!__any(in_clip[0] || in_clip[1])) continue;                    // no n-gram of this order is in the clip: all dots are 0
    for (int r = 0; r < R; ++r) {
      const int g = r0 + r, lo = rw_off[g], hi = rw_off[g + 1];
      double dot = 0.0;
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (in_clip[s]) {
          const int at = find_key(rw_key, lo, hi, key[s]);
          if (at >= 0) {
            const double wr = (double)rw_cnt[at] * idf[s];
            dot += fmin(wh[s], wr) * wr;
          }
        }
      }
      double val = cap_wave_sum(dot);
      const double nr = ref_norm[(size_t)g * 4 + (n - 1)];
      if (nh != 0.0 && nr != 0.0) val /= nh * nr;
      const double delta = (double)(max(L - 1, 0) - max(ref_len[g] - 1, 0));    // the reference's "length" counts bigrams
      score += val * exp(-(delta * delta) / 72.0);
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int n = 0; n < 4; ++n) {
      st[n] = correct[n];
      st[4 + n] = max(0, L - n);
    }
    st[8] = L;
    st[9] = reflen;
    a.rouge[row] = (float)rouge;
    a.cider[row] = (float)(score / 4.0 / (double)max(R, 1) * 10.0);
    if (a.lcs) a.lcs[row] = best_lcs;
  }
}

bool in_envelope(int V, int Tcap) { return V >= 1 && V <= CP_MAX_V && Tcap >= 1 && Tcap <= CP_MAX_T; }

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_caption_in_envelope(int V, int Tcap) { return in_envelope(V, Tcap) ? 1 : 0; }

extern "C" int hero_caption_score(const void* ids, int ids_int64, const int* clip, const void* refs, int* stats, float* rouge,
                                  float* cider, int* lcs, int M, int ld, int ld_stats, int Tcap, int eos, int V, hero_stream_t stream) {
  HERO_REQUIRE(in_envelope(V, Tcap) && M >= 1 && ld >= Tcap && ld_stats >= CP_STATS && eos >= 0 && eos < V,
               "hero_caption_score: outside the envelope (1 <= V <= %d, 1 <= Tcap <= %d, ld >= Tcap, ld_stats >= %d, 0 <= eos < V, "
               "M >= 1): M=%d ld=%d ld_stats=%d Tcap=%d eos=%d V=%d", CP_MAX_V, CP_MAX_T, CP_STATS, M, ld, ld_stats, Tcap, eos, V);
  HERO_REQUIRE(ids && clip && refs && stats && rouge && cider, "hero_caption_score: null pointer");
  HERO_REQUIRE((((uintptr_t)refs) & 7) == 0, "hero_caption_score: the reference tables must be 8-byte aligned");
  const CapScore a = {ids, clip, static_cast<const unsigned char*>(refs), stats, rouge, cider, lcs, M, ld, ld_stats, Tcap, eos,
                      ids_int64 ? 1 : 0};
  hipLaunchKernelGGL(caption_score_kernel, dim3(M), dim3(CP_NT), 0, static_cast<hipStream_t>(stream), a);
  return check_launch("hero_caption_score");
}
