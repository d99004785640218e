// The random draws of the pre-training batches (MLM token masks, MFM frame masks, FOM frame shuffles) ON THE DEVICE.
//
// The reference draws them in the DataLoader workers with one random.random() per subtitle token / per frame
// (data/mlm.py:21-58 random_word, data/mfm.py:19-25 _get_img_mask, data/fom.py:96-115 random_reorder) and runs one
// dataset per task over the same videos.  Here ONE clean video batch, already on the device (DeviceCollate's length
// slots + f_sub_input_ids + c_v_feats), becomes the MLM, MFM and FOM batch by kernels; the seed is a device word, so a
// captured launch serves every seed (the pattern of hero_sample_select).
//
// THE DRAW (the one statement; tests/pretrain_mask_reference.py restates it in numpy integers):
//   base = splitmix64(seed ^ site * 0xD6E8FEB86659FD93),  k0 = low 32 bits, k1 = high 32 bits      (as DropCtx, common.h)
//   element e (its index in the PADDED layout, below)  ->  h = mix32(e ^ k0),  h2 = mix32(e ^ k1)
//   thr = floor(p * 2^32) as a 64-bit integer (p = 1 selects everything);  e is SELECTED iff h < thr
//   a bounded integer from a hash x:  lo + ((uint64)x * n >> 32)
//   MLM  e = r * max_sl + c for token (row r, column c), 1 <= c < sub_ntok[r] (column 0 is never drawn: it becomes
//        first_token).  selected: h < thr * 4 / 5 -> mask_id;  else h < thr * 9 / 10 -> v_lo + (h2 * (v_hi - v_lo) >> 32);
//        else the token stays.  A row with sub_ntok >= 2 and no selected token selects column 1 and writes mask_id
//        there (data/mlm.py:53-56); a row with sub_ntok <= 1 selects nothing.
//   MFM  e = b * NF + f for frame f < vid_nfrm[b].  A video with frames but none selected selects frame
//        (mix32(~b ^ k1) * vid_nfrm[b]) >> 32 (data/mfm.py:21-23).
//   FOM  e = b * NF + f for frame f < vid_nfrm[b]; no at-least-one rule (data/fom.py:96-115).  The selected positions
//        P[0] < P[1] < ... and the same positions S[0], S[1], ... ordered by (h2, position) - the reference's
//        target_pos_shuffled - give  shuffled_orders[b, P[i]] = S[i],  targets[b, S[i]] = P[i];  identity / -1 elsewhere.
// Compact outputs (txt_labels, txt_mask_rows, feat_targets) are in row-major order of their mask == torch.nonzero order,
// filled behind the count with -1 / -1 / zero rows; the counts are device words.  No atomics, no allocation, no host
// read: two runs give the same bits and every launch can be captured.
#include "common.h"

namespace hero {
namespace {

constexpr int DRAW_THREADS = 1024;        // the one workgroup of the MFM mask kernel: 16 waves, one video per wave at a time
constexpr int MLM_THREADS = 256;          // MLM: several workgroups of 4 waves, one row per wave at a time
constexpr int MLM_MAX_GROUPS = 64;
constexpr int DRAW_MAX_SEGMENTS = 4096;   // rows (MLM) / videos (MFM) whose counts a workgroup scans in LDS
constexpr int FOM_MAX_FRAMES = 2048;
constexpr int32_t FALLBACK_BIT = 1 << 30;

struct DrawKeys {
  uint32_t k0, k1;
  __device__ __forceinline__ DrawKeys(const unsigned long long* seed, unsigned long long site) {
    const uint64_t base = splitmix64((uint64_t)*seed ^ ((uint64_t)site * 0xD6E8FEB86659FD93ull));
    k0 = (uint32_t)base;
    k1 = (uint32_t)(base >> 32);
  }
  __device__ __forceinline__ uint32_t h(uint32_t e) const { return mix32(e ^ k0); }
  __device__ __forceinline__ uint32_t h2(uint32_t e) const { return mix32(e ^ k1); }
};

__device__ __forceinline__ int lanes_below(uint64_t ballot, int lane) { return __popcll(ballot & ((1ull << lane) - 1ull)); }

// cnt[0, n) (FALLBACK_BIT ignored) -> off[0, n) = exclusive prefix sums; returns the total.  Whole workgroup of THREADS
// threads, ends in a barrier.
template <int THREADS>
__device__ int block_exclusive_scan(const int32_t* cnt, int32_t* off, int n, int32_t* wsum) {
  constexpr int WAVES = THREADS / 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int per = (n + THREADS - 1) / THREADS, i0 = tid * per, i1 = min(i0 + per, n);
  int s = 0;
  for (int i = i0; i < i1; ++i) s += cnt[i] & ~FALLBACK_BIT;
  int x = s;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  if (lane == 63) wsum[wave] = x;
  __syncthreads();
  if (wave == 0) {
    int w = lane < WAVES ? wsum[lane] : 0;
    for (int d = 1; d < WAVES; d <<= 1) {
      const int y = __shfl_up(w, d);
      if (lane >= d) w += y;
    }
    if (lane < WAVES) wsum[lane] = w;
  }
  __syncthreads();
  int base = (wave ? wsum[wave - 1] : 0) + x - s;
  for (int i = i0; i < i1; ++i) {
    off[i] = base;
    base += cnt[i] & ~FALLBACK_BIT;
  }
  const int total = wsum[WAVES - 1];
  __syncthreads();
  return total;
}

// ---- MLM --------------------------------------------------------------------------------------------------------------
// One launch, several workgroups, no exchange between them: EVERY workgroup counts the selections of every row (one thread
// per row, hashes only - nothing but the two length arrays is read) and scans the counts in LDS, then writes the rows
// r = workgroup * 4 + wave (mod the grid), one row per wave at a time; workgroup 0 also writes the fill behind the count and
// the count.  A single workgroup would walk T / 16 rows per wave, each a chain of dependent global accesses.
__global__ __launch_bounds__(MLM_THREADS) void mlm_mask_kernel(
    const int64_t* __restrict__ ids_in, const int32_t* __restrict__ sub_nfrm, const int32_t* __restrict__ sub_ntok,
    const unsigned long long* __restrict__ seed, unsigned long long site, unsigned long long thr, unsigned long long thr80,
    unsigned long long thr90, int64_t mask_id, int64_t v_lo, uint32_t v_n, int64_t first_token, int64_t* __restrict__ ids_out,
    uint8_t* __restrict__ tgt, int64_t* __restrict__ labels, int32_t* __restrict__ rows, int32_t* __restrict__ count, int T, int max_sl,
    int Lf) {
  __shared__ int32_t cnt[DRAW_MAX_SEGMENTS], off[DRAW_MAX_SEGMENTS], wsum[MLM_THREADS / 64];
  const DrawKeys key(seed, site);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = threadIdx.x; r < T; r += MLM_THREADS) {
    const int nt = min(sub_ntok[r], max_sl), eff = max(sub_nfrm[r], 1), last = min(nt, Lf - eff);     // columns [1, last) can be drawn
    int n = 0;
    for (int c = 1; c < last; ++c) n += key.h((uint32_t)(r * max_sl + c)) < thr ? 1 : 0;
    cnt[r] = (n == 0 && last >= 2) ? (1 | FALLBACK_BIT) : n;     // data/mlm.py:53-56: at least one, the row's first token
  }
  __syncthreads();
  const int total = block_exclusive_scan<MLM_THREADS>(cnt, off, T, wsum);
  for (int r = blockIdx.x * (MLM_THREADS / 64) + wave; r < T; r += gridDim.x * (MLM_THREADS / 64)) {
    const int nt = min(sub_ntok[r], max_sl), eff = max(sub_nfrm[r], 1), last = min(nt, Lf - eff);
    const bool fallback = (cnt[r] & FALLBACK_BIT) != 0;
    int at = off[r];
    for (int c0 = 0; c0 < max_sl; c0 += 64) {
      const int c = c0 + lane;
      const uint32_t e = (uint32_t)(r * max_sl + c);
      const uint32_t hv = key.h(e);
      const bool drawn = c >= 1 && c < last && hv < thr, sel = fallback ? c == 1 : drawn;
      const int64_t was = c < max_sl ? ids_in[e] : 0;
      if (c < max_sl) {
        int64_t v = c == 0 ? first_token : was;
        if (drawn) v = hv < thr80 ? mask_id : (hv < thr90 ? v_lo + (int64_t)(((uint64_t)key.h2(e) * v_n) >> 32) : v);
        if (fallback && c == 1) v = mask_id;
        ids_out[e] = v;
      }
      const uint64_t b = __ballot(sel);                          // labels and flat target rows in row-major order == torch.nonzero order
      if (sel) {
        const int p = at + lanes_below(b, lane);
        labels[p] = was;
        rows[p] = r * Lf + eff + c;
      }
      at += __popcll(b);
    }
    for (int j = lane; j < Lf; j += 64) {
      const int c = j - eff;
      tgt[r * Lf + j] = (c >= 1 && c < last && (fallback ? c == 1 : key.h((uint32_t)(r * max_sl + c)) < thr)) ? 1 : 0;
    }
  }
  if (blockIdx.x == 0) {
    const int cap = T * (max_sl - 1);
    for (int i = total + threadIdx.x; i < cap; i += MLM_THREADS) {
      labels[i] = -1;
      rows[i] = -1;
    }
    if (threadIdx.x == 0) count[0] = total;
  }
}

// ---- MFM --------------------------------------------------------------------------------------------------------------
// src = [B * NF | T * max_vl | B * NF] int32: the row of c_v_feats behind every row of the masked clip copy, the masked
// subtitle copy and the compact targets; -1 = a row of zeros (masked, an empty slot, behind the count).
__global__ __launch_bounds__(DRAW_THREADS) void mfm_mask_kernel(
    const int32_t* __restrict__ vid_nfrm, const int32_t* __restrict__ vid_sub_off, const int32_t* __restrict__ sub_frm_off,
    const int32_t* __restrict__ sub_frm, const unsigned long long* __restrict__ seed, unsigned long long site, unsigned long long thr,
    uint8_t* __restrict__ c_mask, uint8_t* __restrict__ f_mask, int32_t* __restrict__ src, int32_t* __restrict__ count, int T, int max_vl,
    int B, int NF) {
  __shared__ int32_t cnt[DRAW_MAX_SEGMENTS], off[DRAW_MAX_SEGMENTS], forced[DRAW_MAX_SEGMENTS], wsum[DRAW_THREADS / 64];
  const DrawKeys key(seed, site);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = wave; b < B; b += DRAW_THREADS / 64) {
    const int nfv = min(max(vid_nfrm[b], 0), NF);
    int n = 0;
    for (int f0 = 0; f0 < nfv; f0 += 64) {
      const int f = f0 + lane;
      n += __popcll(__ballot(f < nfv && key.h((uint32_t)(b * NF + f)) < thr));
    }
    if (lane == 0) {
      const bool fallback = n == 0 && nfv > 0;                  // data/mfm.py:21-23: at least one, a random frame
      forced[b] = fallback ? (int32_t)(((uint64_t)key.h2(~(uint32_t)b) * (uint32_t)nfv) >> 32) : -1;
      cnt[b] = fallback ? 1 : n;
    }
  }
  __syncthreads();
  const int total = block_exclusive_scan<DRAW_THREADS>(cnt, off, B, wsum);
  int32_t* c_src = src;
  int32_t* f_src = src + B * NF;
  int32_t* t_src = f_src + T * max_vl;
  for (int b = wave; b < B; b += DRAW_THREADS / 64) {
    const int nfv = min(max(vid_nfrm[b], 0), NF), fb = forced[b];
    int at = off[b];
    for (int f0 = 0; f0 < NF; f0 += 64) {
      const int f = f0 + lane, e = b * NF + f;
      const bool sel = f < nfv && (key.h((uint32_t)e) < thr || f == fb);
      const uint64_t bal = __ballot(sel);
      if (f < NF) {
        c_mask[e] = sel ? 1 : 0;
        c_src[e] = sel ? -1 : e;
      }
      if (sel) t_src[at + lanes_below(bal, lane)] = e;
      at += __popcll(bal);
    }
  }
  for (int i = total + threadIdx.x; i < B * NF; i += DRAW_THREADS) t_src[i] = -1;
  // the subtitle copies: slot k of row r holds the k-th frame of the row's list that lies inside its video - the walk of
  // gather_feats_kernel (collate.hip) - and carries that frame's decision
  for (int q = threadIdx.x; q < T * max_vl; q += DRAW_THREADS) {
    const int r = q / max_vl, k = q - r * max_vl;
    int lo = 0, hi = B - 1;                                     // the video of row r: vid_sub_off[b] <= r < vid_sub_off[b + 1]
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (vid_sub_off[mid] <= r) lo = mid; else hi = mid - 1;
    }
    const int b = lo, nfv = vid_nfrm[b];
    int f = -1, seen = 0;
    for (int j = sub_frm_off[r]; j < sub_frm_off[r + 1]; ++j) {
      const int c = sub_frm[j];
      if (c >= 0 && c < nfv) {
        if (seen == k) { f = c; break; }
        ++seen;
      }
    }
    const bool have = f >= 0 && f < NF;
    const bool sel = have && (key.h((uint32_t)(b * NF + f)) < thr || f == forced[b]);
    f_mask[q] = sel ? 1 : 0;
    f_src[q] = (have && !sel) ? b * NF + f : -1;
  }
  if (threadIdx.x == 0) count[0] = total;
}

// The byte-heavy part: every destination row is a copy of one row of c_v_feats or a row of zeros.  One wave per row,
// 16-byte segments, four loads in flight per lane before the first store, 16 waves per CU (the shape that gathers whole
// rows at 5.5-5.8 TB/s); a masked row stores zeros and reads nothing.
__global__ __launch_bounds__(256) void mfm_copy_kernel(const float4* __restrict__ c_feats, float4* __restrict__ c_out, float4* __restrict__ f_out,
                                                       float4* __restrict__ t_out, const int32_t* __restrict__ src, int n_c, int n_f, int D4) {
  const int lane = threadIdx.x & 63, jobs = 2 * n_c + n_f;
  for (int job = blockIdx.x * 4 + (threadIdx.x >> 6); job < jobs; job += gridDim.x * 4) {
    const int s = __builtin_amdgcn_readfirstlane(src[job]);
    float4* dst = job < n_c ? c_out + (size_t)job * D4 : (job < n_c + n_f ? f_out + (size_t)(job - n_c) * D4 : t_out + (size_t)(job - n_c - n_f) * D4);
    if (s < 0 || s >= n_c) {
      const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c = lane; c < D4; c += 64) dst[c] = z;
      continue;
    }
    const float4* sp = c_feats + (size_t)s * D4;
    for (int c = lane; c < D4; c += 256) {
      // four named registers and in-bounds indices (a segment past the row re-reads segment c and is not stored): an array
      // of four went to LDS, a select between a load and a constant went through private memory
      const bool p1 = c + 64 < D4, p2 = c + 128 < D4, p3 = c + 192 < D4;
      const float4 v0 = sp[c];
      const float4 v1 = sp[p1 ? c + 64 : c];
      const float4 v2 = sp[p2 ? c + 128 : c];
      const float4 v3 = sp[p3 ? c + 192 : c];
      dst[c] = v0;
      if (p1) dst[c + 64] = v1;
      if (p2) dst[c + 128] = v2;
      if (p3) dst[c + 192] = v3;
    }
  }
}

// ---- FOM --------------------------------------------------------------------------------------------------------------
// one workgroup per video; the ranks by counting over the video's composites in LDS (at most NF keys)
__global__ __launch_bounds__(256) void fom_shuffle_kernel(const int32_t* __restrict__ vid_nfrm, const unsigned long long* __restrict__ seed,
                                                          unsigned long long site, unsigned long long thr, int64_t* __restrict__ orders,
                                                          int64_t* __restrict__ targets, int NF) {
  __shared__ uint64_t comp[FOM_MAX_FRAMES];            // (h2 << 32) | position of a selected frame, all ones otherwise
  __shared__ int16_t by_pos[FOM_MAX_FRAMES], by_key[FOM_MAX_FRAMES], rank_pos[FOM_MAX_FRAMES], rank_key[FOM_MAX_FRAMES];
  const DrawKeys key(seed, site);
  const int b = blockIdx.x, nfv = min(max(vid_nfrm[b], 0), NF);
  for (int f = threadIdx.x; f < nfv; f += blockDim.x) {
    const uint32_t e = (uint32_t)(b * NF + f);
    comp[f] = key.h(e) < thr ? (((uint64_t)key.h2(e) << 32) | (uint32_t)f) : ~0ull;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < nfv; f += blockDim.x) {
    const uint64_t mine = comp[f];
    if (mine == ~0ull) continue;
    int before = 0, smaller = 0;                       // f = P[before] = S[smaller]
    for (int g = 0; g < nfv; ++g) {
      const uint64_t other = comp[g];
      before += (other != ~0ull && g < f) ? 1 : 0;
      smaller += other < mine ? 1 : 0;
    }
    rank_pos[f] = (int16_t)before;
    rank_key[f] = (int16_t)smaller;
    by_pos[before] = (int16_t)f;
    by_key[smaller] = (int16_t)f;
  }
  __syncthreads();
  for (int f = threadIdx.x; f < NF; f += blockDim.x) {
    const bool sel = f < nfv && comp[f] != ~0ull;
    orders[b * NF + f] = sel ? by_key[rank_pos[f]] : f;
    targets[b * NF + f] = sel ? by_pos[rank_key[f]] : -1;
  }
}

// ---- fixed-capacity consumers: the stable partition of a mask and the NCE operand pack ------------------------------------
// order = the set indices in ascending order, then the unset ones in ascending order - the row order of the reference's
// cat([pos, neg]) in mfm_nce (masked frames in torch.nonzero order, then every unmasked frame, padding included); rank is its
// inverse.  One workgroup: a first pass counts the set elements, a second walks the mask in chunks of the workgroup size
// with a ballot per wave and a scan of the wave counts in LDS.
__global__ __launch_bounds__(DRAW_THREADS) void mask_partition_kernel(const uint8_t* __restrict__ mask, int n, int32_t* __restrict__ order,
                                                                      int32_t* __restrict__ rank, int32_t* __restrict__ count) {
  constexpr int WAVES = DRAW_THREADS / 64;
  __shared__ int32_t wsum[WAVES], total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int mine = 0;
  for (int i = tid; i < n; i += DRAW_THREADS) mine += mask[i] ? 1 : 0;
  for (int d = 32; d > 0; d >>= 1) mine += __shfl_xor(mine, d);
  if (lane == 0) wsum[wave] = mine;
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int w = 0; w < WAVES; ++w) m += wsum[w];
    total = m;
  }
  __syncthreads();
  const int m = total;
  int before = 0;                                               // set elements in front of the chunk
  for (int i0 = 0; i0 < n; i0 += DRAW_THREADS) {
    const int i = i0 + tid;
    const bool set = i < n && mask[i] != 0;
    const uint64_t b = __ballot(set);
    __syncthreads();                                            // the previous chunk's reads of wsum are over
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int ahead = 0, chunk = 0;
    for (int w = 0; w < WAVES; ++w) {
      const int c = wsum[w];
      ahead += w < wave ? c : 0;
      chunk += c;
    }
    if (i < n) {
      const int s = before + ahead + lanes_below(b, lane);      // set elements in front of i
      const int pos = set ? s : m + (i - s);
      order[pos] = i;
      rank[i] = pos;
    }
    before += chunk;
  }
  if (tid == 0) count[0] = m;
}

// cand[r] = targets[r] (r < m) | out[r] (m <= r < n) | 0 (n <= r < n8) and masked[r] = out[r] (r < cap), both converted to T:
// the two operands of the NCE logits GEMM from the regressed rows in partition order.  One wave per destination row,
// 16-byte source segments.
template <typename T>
__global__ __launch_bounds__(256) void nce_pack_fwd_kernel(const float* __restrict__ out, const float* __restrict__ targets,
                                                           const int32_t* __restrict__ count, T* __restrict__ cand, T* __restrict__ masked, int n,
                                                           int n8, int cap, int D) {
  const int lane = threadIdx.x & 63, jobs = n8 + cap, m = min(max(count[0], 0), n);
  for (int job = blockIdx.x * 4 + (threadIdx.x >> 6); job < jobs; job += gridDim.x * 4) {
    const int r = job < n8 ? job : job - n8;
    T* dst = job < n8 ? cand + (size_t)r * D : masked + (size_t)r * D;
    if (job < n8 && r >= n) {
      for (int c = lane * 4; c < D; c += 256) V4<T>::st(dst + c, make_float4(0.f, 0.f, 0.f, 0.f));
      continue;
    }
    const float* src = (job < n8 && r < m ? targets : out) + (size_t)r * D;
    for (int c = lane * 4; c < D; c += 256) V4<T>::st(dst + c, ldf4(src + c));
  }
}

// d_out[r] = (r < cap ? d_masked[r] : 0) + (r >= m ? d_cand[r] : 0) in fp32; the targets receive nothing
template <typename T>
__global__ __launch_bounds__(256) void nce_pack_bwd_kernel(const T* __restrict__ d_cand, const T* __restrict__ d_masked,
                                                           const int32_t* __restrict__ count, float* __restrict__ d_out, int n, int cap, int D) {
  const int lane = threadIdx.x & 63, m = min(max(count[0], 0), n);
  const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int r = blockIdx.x * 4 + (threadIdx.x >> 6); r < n; r += gridDim.x * 4) {
    const bool from_masked = d_masked && r < cap, from_cand = d_cand && r >= m;
    for (int c = lane * 4; c < D; c += 256) {
      const float4 a = from_masked ? V4<T>::ld(d_masked + (size_t)r * D + c) : z;
      const float4 b = from_cand ? V4<T>::ld(d_cand + (size_t)r * D + c) : z;
      stf4(d_out + (size_t)r * D + c, make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w));
    }
  }
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_mask_partition(const unsigned char* mask, int n, int32_t* order, int32_t* rank, int32_t* count, hero_stream_t stream) {
  HERO_REQUIRE(mask && order && rank && count, "hero_mask_partition: null pointer");
  HERO_REQUIRE(n >= 1 && n <= (1 << 20), "hero_mask_partition: 1 <= n <= 2^20, got %d", n);
  hipLaunchKernelGGL(mask_partition_kernel, dim3(1), dim3(DRAW_THREADS), 0, static_cast<hipStream_t>(stream), mask, n, order, rank, count);
  return check_launch("hero_mask_partition");
}

static int check_pack(const char* what, const int32_t* count, int n, int cap, int D, int dtype) {
  HERO_REQUIRE(count, "%s: count required", what);
  HERO_REQUIRE(n >= 1 && cap >= 1 && cap <= n && D >= 4 && D % 4 == 0 && (long long)(n + 8 + cap) * D < (1ll << 40),
               "%s: bad dims n=%d cap=%d D=%d (1 <= cap <= n, D a multiple of 4)", what, n, cap, D);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

extern "C" int hero_nce_pack_fwd(const float* out, const float* targets, const int32_t* count, void* cand, void* masked, int n, int cap,
                                 int D, int dtype, hero_stream_t stream) {
  if (const int rc = check_pack("hero_nce_pack_fwd", count, n, cap, D, dtype)) return rc;
  HERO_REQUIRE(out && targets && cand && masked, "hero_nce_pack_fwd: null pointer");
  HERO_REQUIRE(((uintptr_t)out | (uintptr_t)targets | (uintptr_t)cand | (uintptr_t)masked) % 16 == 0, "hero_nce_pack_fwd: buffers must be 16-byte aligned");
  const int n8 = (n + 7) / 8 * 8, jobs = n8 + cap;
  const int grid = (jobs + 3) / 4 < 1024 ? (jobs + 3) / 4 : 1024;
  return by_dtype(dtype, "hero_nce_pack_fwd", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nce_pack_fwd_kernel<T>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), out, targets, count,
                       static_cast<T*>(cand), static_cast<T*>(masked), n, n8, cap, D);
  });
}

extern "C" int hero_nce_pack_bwd(const void* d_cand, const void* d_masked, const int32_t* count, float* d_out, int n, int cap, int D,
                                 int dtype, hero_stream_t stream) {
  if (const int rc = check_pack("hero_nce_pack_bwd", count, n, cap, D, dtype)) return rc;
  HERO_REQUIRE(d_out, "hero_nce_pack_bwd: d_out required");
  HERO_REQUIRE(((uintptr_t)d_cand | (uintptr_t)d_masked | (uintptr_t)d_out) % 16 == 0, "hero_nce_pack_bwd: buffers must be 16-byte aligned");
  const int grid = (n + 3) / 4 < 1024 ? (n + 3) / 4 : 1024;
  return by_dtype(dtype, "hero_nce_pack_bwd", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(nce_pack_bwd_kernel<T>, dim3(grid), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const T*>(d_cand),
                       static_cast<const T*>(d_masked), count, d_out, n, cap, D);
  });
}

extern "C" int hero_mlm_mask(const int64_t* input_ids, const int32_t* sub_nfrm, const int32_t* sub_ntok, const unsigned long long* seed_dev,
                             unsigned long long site, unsigned long long threshold, long long mask_id, long long v_lo, long long v_hi,
                             long long first_token, int64_t* ids_out, unsigned char* txt_mask_tgt, int64_t* txt_labels,
                             int32_t* txt_mask_rows, int32_t* count, int T, int max_sl, int out_size, hero_stream_t stream) {
  HERO_REQUIRE(input_ids && sub_nfrm && sub_ntok && seed_dev && ids_out && txt_mask_tgt && txt_labels && txt_mask_rows && count,
               "hero_mlm_mask: null pointer");
  HERO_REQUIRE(input_ids != ids_out, "hero_mlm_mask: the masked ids need a buffer of their own (the clean batch stays clean)");
  HERO_REQUIRE(T >= 1 && T <= DRAW_MAX_SEGMENTS && max_sl >= 1 && out_size >= 1, "hero_mlm_mask: 1 <= T <= %d, max_sl, out_size >= 1", DRAW_MAX_SEGMENTS);
  HERO_REQUIRE((long long)T * max_sl < (1ll << 31) && (long long)T * out_size < (1ll << 31), "hero_mlm_mask: batch too large for 32-bit element indices");
  HERO_REQUIRE(threshold <= (1ull << 32), "hero_mlm_mask: threshold above 2^32");
  HERO_REQUIRE(v_hi > v_lo && v_hi - v_lo < (1ll << 32), "hero_mlm_mask: empty or too wide token range");
  const int groups = (T + 3) / 4 < MLM_MAX_GROUPS ? (T + 3) / 4 : MLM_MAX_GROUPS;
  hipLaunchKernelGGL(mlm_mask_kernel, dim3(groups), dim3(MLM_THREADS), 0, static_cast<hipStream_t>(stream), input_ids, sub_nfrm, sub_ntok, seed_dev,
                     site, threshold, threshold * 4ull / 5ull, threshold * 9ull / 10ull, (int64_t)mask_id, (int64_t)v_lo, (uint32_t)(v_hi - v_lo),
                     (int64_t)first_token, ids_out, txt_mask_tgt, txt_labels, txt_mask_rows, count, T, max_sl, out_size);
  return check_launch("hero_mlm_mask");
}

extern "C" int hero_mfm_mask(const float* c_v_feats, const int32_t* vid_nfrm, const int32_t* vid_sub_off, const int32_t* sub_frm_off,
                             const int32_t* sub_frm, const unsigned long long* seed_dev, unsigned long long site, unsigned long long threshold,
                             unsigned char* c_v_masks, unsigned char* f_v_masks, float* feat_targets, int32_t* count, float* c_v_feats_out,
                             float* f_v_feats_out, int32_t* row_src, int T, int max_vl, int B, int NF, int D, hero_stream_t stream) {
  HERO_REQUIRE(c_v_feats && vid_nfrm && vid_sub_off && sub_frm_off && sub_frm && seed_dev && c_v_masks && f_v_masks && feat_targets && count &&
               c_v_feats_out && f_v_feats_out && row_src, "hero_mfm_mask: null pointer");
  HERO_REQUIRE(c_v_feats != c_v_feats_out && c_v_feats != f_v_feats_out && c_v_feats != feat_targets,
               "hero_mfm_mask: the masked copies need buffers of their own (the clean batch stays clean)");
  HERO_REQUIRE(T >= 1 && max_vl >= 1 && B >= 1 && B <= DRAW_MAX_SEGMENTS && NF >= 1 && D >= 4 && D % 4 == 0,
               "hero_mfm_mask: bad dims (1 <= B <= %d, D a multiple of 4)", DRAW_MAX_SEGMENTS);
  HERO_REQUIRE(2ll * B * NF + (long long)T * max_vl < (1ll << 31), "hero_mfm_mask: batch too large for 32-bit row indices");
  HERO_REQUIRE(threshold <= (1ull << 32), "hero_mfm_mask: threshold above 2^32");
  HERO_REQUIRE(((uintptr_t)c_v_feats | (uintptr_t)c_v_feats_out | (uintptr_t)f_v_feats_out | (uintptr_t)feat_targets) % 16 == 0,
               "hero_mfm_mask: feature buffers must be 16-byte aligned");
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(mfm_mask_kernel, dim3(1), dim3(DRAW_THREADS), 0, s, vid_nfrm, vid_sub_off, sub_frm_off, sub_frm, seed_dev, site, threshold,
                     c_v_masks, f_v_masks, row_src, count, T, max_vl, B, NF);
  const int jobs = 2 * B * NF + T * max_vl;
  const int grid = (jobs + 3) / 4 < 1024 ? (jobs + 3) / 4 : 1024;            // 4 workgroups of 4 waves per CU: 16 rows in flight per CU
  hipLaunchKernelGGL(mfm_copy_kernel, dim3(grid), dim3(256), 0, s, reinterpret_cast<const float4*>(c_v_feats),
                     reinterpret_cast<float4*>(c_v_feats_out), reinterpret_cast<float4*>(f_v_feats_out), reinterpret_cast<float4*>(feat_targets),
                     row_src, B * NF, T * max_vl, D / 4);
  return check_launch("hero_mfm_mask");
}

extern "C" int hero_fom_shuffle(const int32_t* vid_nfrm, const unsigned long long* seed_dev, unsigned long long site,
                                unsigned long long threshold, int64_t* shuffled_orders, int64_t* targets, int B, int NF, hero_stream_t stream) {
  HERO_REQUIRE(vid_nfrm && seed_dev && shuffled_orders && targets, "hero_fom_shuffle: null pointer");
  HERO_REQUIRE(B >= 1 && NF >= 1 && NF <= FOM_MAX_FRAMES && (long long)B * NF < (1ll << 31), "hero_fom_shuffle: 1 <= NF <= %d, B >= 1", FOM_MAX_FRAMES);
  HERO_REQUIRE(threshold <= (1ull << 32), "hero_fom_shuffle: threshold above 2^32");
  hipLaunchKernelGGL(fom_shuffle_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), vid_nfrm, seed_dev, site, threshold,
                     shuffled_orders, targets, NF);
  return check_launch("hero_fom_shuffle");
}
