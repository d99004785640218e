// After the search (gfx950): greedy temporal NMS of the sorted candidate rows and the rank of the first correct prediction
// of every query - the device side of utils/tvr_eval_utils.py:35-92, 132-175, 214-234 (temporal_non_maximum_suppression,
// filter_vcmr_by_nms, post_processing_svmr_nms) and of utils/tvr_standalone_eval.py:86-257 (eval_by_task_type).
//
// hero_moment_nms: one wavefront owns a query.  Candidate i of the row sits in register slot i / 64 of lane i % 64 (at most
// 16 slots: N <= 1024), so a slot is 64 consecutive candidates in row = score order.  The sweep is sequential in the pivots
// and parallel in what a pivot does: the next pivot is the lowest set bit of a ballot over the slot's alive flags, its
// (video, start, end, kept-in-group) come from its lane by a lane broadcast, and every lane then updates its own later
// candidates of the pivot's video - one more kept in their group, dead if the IoU exceeds the threshold.  No LDS, no
// barrier, no atomics, no workspace; the result depends on the row alone.  The float64 division runs only for candidates
// of the pivot's video that overlap it.
//
// hero_first_hit / hero_first_hit_multi: one wavefront per query; the lanes stride over the predictions, each keeps the first
// position it saw per column, a butterfly minimum folds them.  One row scan serves both: one [st, ed] per query is the
// G = 1 instance of the several-annotator rule (DiDeMo).
#include "common.h"

namespace hero {
namespace {

constexpr int NMS_SLOTS = 16;      // x 64 lanes: N <= 1024
constexpr int HIT_MAX_T = 8;

__global__ __launch_bounds__(64) void moment_nms_kernel(const int* video, const int* st, const int* ed, int N, double thd, int cap, int max_after,
                                                       int* keep, int* count) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const int* vrow = video + (size_t)q * N;
  const int* srow = st + (size_t)q * N;
  const int* erow = ed + (size_t)q * N;
  int* krow = keep + (size_t)q * max_after;
  const int R = (N + 63) >> 6;
  int v[NMS_SLOTS], s[NMS_SLOTS], e[NMS_SLOTS], g[NMS_SLOTS];       // g: survivors so far among the EARLIER candidates of this one's video
  bool alive[NMS_SLOTS];
#pragma unroll
  for (int r = 0; r < NMS_SLOTS; ++r) {
    const int i = r * 64 + lane;
    const bool in = r < R && i < N;
    v[r] = in ? vrow[i] : -1;
    s[r] = in ? srow[i] : -1;
    e[r] = in ? erow[i] : -1;
    g[r] = 0;
    alive[r] = v[r] >= 0 && s[r] >= 0;                              // a vacant slot is never kept and suppresses nothing
  }
  int kept = 0;
#pragma unroll
  for (int r = 0; r < NMS_SLOTS; ++r) {
    if (r >= R || kept >= max_after) break;
    unsigned long long m = __ballot(alive[r]);
    while (m != 0ull && kept < max_after) {
      const int pl = __ffsll((long long)m) - 1;                     // the first candidate of the slot that is still alive
      const int pv = __builtin_amdgcn_readlane(v[r], pl), ps = __builtin_amdgcn_readlane(s[r], pl);       // wave-uniform: the branches
      const int pe = __builtin_amdgcn_readlane(e[r], pl), pg = __builtin_amdgcn_readlane(g[r], pl);       // below are scalar
      const unsigned long long later = pl == 63 ? 0ull : ~((2ull << pl) - 1ull);
      if (pg >= cap) {                                              // its video already has per_video_cap survivors: dropped, suppresses nothing
        m &= later;
        continue;
      }
      if (lane == 0) krow[kept] = r * 64 + pl;
      ++kept;
#pragma unroll
      for (int rr = r; rr < NMS_SLOTS; ++rr) {
        if (rr < R) {
          const bool after = rr > r || lane > pl;
          if (after && v[rr] == pv) {
            ++g[rr];
            if (alive[rr]) {
              const int inter = min(pe, e[rr]) + 1 - max(ps, s[rr]);       // half-open frame spans [st, ed + 1)
              const int uni = max(pe, e[rr]) + 1 - min(ps, s[rr]);         // "not the correct union": the hull, >= 1
              const double iou = inter > 0 ? (double)inter / (double)uni : 0.0;
              if (iou > thd) alive[rr] = false;
            }
          }
        }
      }
      m = __ballot(alive[r]) & later;
    }
  }
  for (int i = kept + lane; i < max_after; i += 64) krow[i] = -1;
  if (lane == 0) count[q] = kept;
}

// The row scan of both recall exports.  GCAP annotator timestamps of the query sit in registers; n of them are real (n is
// wave-uniform: q goes through readfirstlane, so the ground truth comes by scalar loads and `g < n` is a scalar branch).
// A prediction is correct at a threshold when at least `need` annotators reach it: 1, or the reference's least_n_overlap = 2
// from four annotators on (utils/tvr_standalone_eval.py:159-170).  gt_n == nullptr: one [st, ed] per query, GCAP = 1.
template <int GCAP>
__global__ __launch_bounds__(256) void first_hit_kernel(const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video,
                                                        const float* gt_ts, const int* gt_n, int G, float interval, const float* thds, int T,
                                                        int* first) {
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (q >= Nq) return;                                              // whole waves leave; no barrier below
  const int gv = gt_video[q];
  const bool timed = st != nullptr && T > 0;
  const int n = !timed ? 0 : gt_n == nullptr ? 1 : max(1, min(gt_n[q], min(G, GCAP)));       // never past the row's G slots
  const int need = n >= 4 ? 2 : 1;
  float g0[GCAP], g1[GCAP];
#pragma unroll
  for (int g = 0; g < GCAP; ++g) {                                  // slots >= n are padding: never read
    g0[g] = g < n ? gt_ts[((size_t)q * G + g) * 2] : 0.f;
    g1[g] = g < n ? gt_ts[((size_t)q * G + g) * 2 + 1] : 0.f;
  }
  float thd[HIT_MAX_T];
#pragma unroll
  for (int t = 0; t < HIT_MAX_T; ++t) thd[t] = t < T ? thds[t] : 0.f;
  int best[HIT_MAX_T + 1];
#pragma unroll
  for (int t = 0; t <= HIT_MAX_T; ++t) best[t] = P;
  for (int p = lane; p < P; p += 64) {
    const int pv = video[(size_t)q * ld + p];
    if (pv < 0 || pv != gv) continue;
    int ps = 0, pe = 0;
    if (st != nullptr) {
      ps = st[(size_t)q * ld + p];
      pe = ed[(size_t)q * ld + p];
      if (ps < 0) continue;                                         // vacant
    }
    best[0] = min(best[0], p);
    if (!timed) continue;
    const float p0 = (float)ps * interval, p1 = (float)(pe + 1) * interval;
    int reached[HIT_MAX_T];                                         // annotators with iou >= thd[t]
#pragma unroll
    for (int t = 0; t < HIT_MAX_T; ++t) reached[t] = 0;
#pragma unroll
    for (int g = 0; g < GCAP; ++g) {
      if (g < n) {
        const float inter = fmaxf(0.f, fminf(p1, g1[g]) - fmaxf(p0, g0[g]));
        const float uni = fmaxf(p1, g1[g]) - fminf(p0, g0[g]);
        const float iou = uni != 0.f ? inter / uni : 0.f;
#pragma unroll
        for (int t = 0; t < HIT_MAX_T; ++t) reached[t] += t < T && iou >= thd[t] ? 1 : 0;
      }
    }
#pragma unroll
    for (int t = 0; t < HIT_MAX_T; ++t)
      if (t < T && reached[t] >= need) best[1 + t] = min(best[1 + t], p);
  }
#pragma unroll
  for (int t = 0; t <= HIT_MAX_T; ++t) {
    if (t <= T) {
      int b = best[t];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) b = min(b, __shfl_xor(b, o, 64));
      if (lane == 0) first[(size_t)q * (T + 1) + t] = b;
    }
  }
}

constexpr int HIT_MAX_G = 16;

template <int GCAP>
int launch_first_hit(const char* what, const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video, const float* gt_ts,
                     const int* gt_n, int G, float interval, const float* thds, int T, int* first, hero_stream_t stream) {
  hipLaunchKernelGGL(first_hit_kernel<GCAP>, dim3((Nq + 3) / 4), dim3(256), 0, static_cast<hipStream_t>(stream), video, st, ed, Nq, P, ld, gt_video,
                     gt_ts, gt_n, G, interval, thds, T, first);
  return check_launch(what);
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_moment_nms(const int* video, const int* st, const int* ed, int Nq, int N, double thd, int per_video_cap, int max_after, int* keep,
                               int* count, hero_stream_t stream) {
  HERO_REQUIRE(video && st && ed && keep && count, "hero_moment_nms: null pointer");
  HERO_REQUIRE(N >= 1 && N <= NMS_SLOTS * 64 && max_after >= 1 && max_after <= N, "hero_moment_nms: need 1 <= N <= %d and 1 <= max_after <= N (N=%d max_after=%d)",
               NMS_SLOTS * 64, N, max_after);
  HERO_REQUIRE(per_video_cap >= 1 && thd == thd, "hero_moment_nms: need per_video_cap >= 1 and a threshold that is a number (per_video_cap=%d)", per_video_cap);
  if (Nq <= 0) return HERO_OK;
  hipLaunchKernelGGL(moment_nms_kernel, dim3(Nq), dim3(64), 0, static_cast<hipStream_t>(stream), video, st, ed, N, thd, per_video_cap, max_after, keep,
                     count);
  return check_launch("hero_moment_nms");
}

extern "C" int hero_first_hit(const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video, const float* gt_ts, float interval,
                              const float* thds, int T, int* first, hero_stream_t stream) {
  HERO_REQUIRE(video && gt_video && first, "hero_first_hit: null pointer");
  HERO_REQUIRE((st == nullptr) == (ed == nullptr), "hero_first_hit: st and ed are given together or not at all");
  HERO_REQUIRE(P >= 1 && ld >= P, "hero_first_hit: need 1 <= P <= ld (P=%d ld=%d)", P, ld);
  HERO_REQUIRE(T >= 0 && T <= HIT_MAX_T, "hero_first_hit: need 0 <= T <= %d (T=%d)", HIT_MAX_T, T);
  HERO_REQUIRE(T == 0 || (thds && gt_ts && st), "hero_first_hit: IoU thresholds need thds, gt_ts, st and ed");
  if (Nq <= 0) return HERO_OK;
  return launch_first_hit<1>("hero_first_hit", video, st, ed, Nq, P, ld, gt_video, gt_ts, nullptr, 1, interval, thds, T, first, stream);
}

extern "C" int hero_first_hit_multi(const int* video, const int* st, const int* ed, int Nq, int P, int ld, const int* gt_video, const float* gt_ts,
                                    const int* gt_n, int G, float interval, const float* thds, int T, int* first, hero_stream_t stream) {
  HERO_REQUIRE(video && gt_video && first, "hero_first_hit_multi: null pointer");
  HERO_REQUIRE((st == nullptr) == (ed == nullptr), "hero_first_hit_multi: st and ed are given together or not at all");
  HERO_REQUIRE(G >= 1 && G <= HIT_MAX_G, "hero_first_hit_multi: need 1 <= G <= %d (G=%d)", HIT_MAX_G, G);
  HERO_REQUIRE(P >= 1 && ld >= P, "hero_first_hit_multi: need 1 <= P <= ld (P=%d ld=%d)", P, ld);
  HERO_REQUIRE(T >= 0 && T <= HIT_MAX_T, "hero_first_hit_multi: need 0 <= T <= %d (T=%d)", HIT_MAX_T, T);
  HERO_REQUIRE(T == 0 || (thds && gt_ts && gt_n && st), "hero_first_hit_multi: IoU thresholds need thds, gt_ts, gt_n, st and ed");
  if (Nq <= 0) return HERO_OK;
  if (G == 1) return launch_first_hit<1>("hero_first_hit_multi", video, st, ed, Nq, P, ld, gt_video, gt_ts, gt_n, G, interval, thds, T, first, stream);
  if (G <= 4) return launch_first_hit<4>("hero_first_hit_multi", video, st, ed, Nq, P, ld, gt_video, gt_ts, gt_n, G, interval, thds, T, first, stream);
  return launch_first_hit<HIT_MAX_G>("hero_first_hit_multi", video, st, ed, Nq, P, ld, gt_video, gt_ts, gt_n, G, interval, thds, T, first, stream);
}
