// Which kernel a hero_gemm problem gets: ONE pure function (gemm_route) from (shape, layouts, dtype, epilogue, tuning state,
// compute units) to everything a launch needs.  Host-only plain C++17: no HIP runtime call, no global state, so the rules
// are testable without a GPU (hero_gemm_route, tests/test_cpu_gemm_route.py).  gemm.hip and gemm_ws.hip hold the two
// tables that map a route of their families onto the kernel instantiation; they decide nothing.
#pragma once
#include "../../include/hero_hip.h"

namespace hero {

// compile-time epilogue selection of the hot-path combinations (everything else is EK_GENERIC)
enum { EK_GENERIC = 0x100, EK_BIAS = 1, EK_GELU = 2, EK_RES = 4, EK_DROP = 8, EK_GELU_BWD = 16 };

// hero_prof_read slots (hero_hip.h).  0-7 = (dtype == HERO_BF16 ? 4 : 0) + a_layout * 2 + b_layout: the 4-wave kernels.
enum GemmProfSlot {
  PROF_F32_KK = 0, PROF_F32_KO = 1, PROF_F32_OK = 2, PROF_F32_OO = 3,
  PROF_F32_SKINNY = 3,          // shares the slot of the fp32 O,O launches
  PROF_BF16_KK = 4, PROF_BF16_KO = 5, PROF_BF16_OK = 6, PROF_BF16_OO = 7,
  PROF_WS_KK_192 = 8,           // wave-specialised 192 x 192 K,K
  PROF_WS_OO = 9,               // wave-specialised O,O (hero_gemm and hero_wgrad_group)
  PROF_WS_KK_SMALL = 10,        // wave-specialised 128 x 192 / 64 x 128 / 64 x 192 K,K
  PROF_SLOTS = 11
};

enum WsGeometry { WS_GEO_NONE = 0, WS_GEO_3x3, WS_GEO_2x3, WS_GEO_1x2, WS_GEO_1x3 };   // (64 TM) x (64 TN) tiles

// hero_gemm_force_config, decoded ONCE (decode_force); the integer encoding is the table in hero_hip.h.
struct GemmForce {
  bool heuristic = true;               // -1: nothing forced (only then fp32 GEMMs with M <= 32 take the skinny kernel)
  bool allow_ws = true;                // the wave-specialised family may take the problem
  int ws_geometry = WS_GEO_NONE;       // ... and must, with this geometry, where the shape is legal
  int tile4 = -1;                      // forced 4-wave geometry 0..3 (GEMM_TILE4), -1: by shape
  bool use_glds = true;                // direct-to-LDS staging where legal (false: register staging even for K,K operands)
  int group = 0;                       // M-tiles per L2 locality group of the 4-wave kernels, 0: by shape
};

inline GemmForce decode_force(int cfg) {
  GemmForce f;
  if (cfg < 0) return f;
  f.heuristic = false;
  if (cfg >= 8 && cfg <= 14 && cfg != 11 && cfg != 12) {     // wave-specialised kernels: 8 never, 9 / 10 always 192 x 192 / 128 x 192, 13 / 14 the 64 x 128 / 64 x 192 geometries (small-M, long-K GEMMs)
    f.allow_ws = cfg != 8;
    f.ws_geometry = cfg == 9 ? WS_GEO_3x3 : cfg == 10 ? WS_GEO_2x3 : cfg == 13 ? WS_GEO_1x2 : cfg == 14 ? WS_GEO_1x3 : WS_GEO_NONE;
    return f;
  }
  f.allow_ws = false;
  f.tile4 = cfg & 3;
  f.use_glds = !(cfg & 4);             // bit 2 set: register staging even for K,K operands
  f.group = cfg >> 8;                  // bits 8+: M-tiles per locality group (0 = heuristic)
  return f;
}

// 4-wave tile geometries: 0 128 x 128 (two workgroups / CU), 1 192 x 128 (20 % more FLOP per staged byte, 2 x 80 KB = the
// whole LDS of a CU), 2 256 x 256 (8 waves), 3 64 x 64 (problems that leave most CUs idle at 128 x 128)
struct Tile4 { int bm, bn, threads; };
constexpr Tile4 GEMM_TILE4[4] = {{128, 128, 256}, {192, 128, 256}, {256, 256, 512}, {64, 64, 256}};
constexpr int tile4_epi_bytes(Tile4 t) { return (t.bm < 128 ? t.bm : (t.bm % 128 == 0 ? 128 : t.bm / 2)) * t.bn * 4; }
constexpr int tile4_ring_lds(Tile4 t, int stages) {          // operand ring, reused by one fp32 epilogue pass
  return stages * (t.bm + t.bn) * 128 > tile4_epi_bytes(t) ? stages * (t.bm + t.bn) * 128 : tile4_epi_bytes(t);
}
constexpr int tile4_staged_lds(Tile4 t) { return tile4_ring_lds(t, 2); }
constexpr int tile4_glds_lds(Tile4 t) { return tile4_ring_lds(t, t.bm * t.bn <= 64 * 64 ? 4 : 2); }
constexpr int WS_LDS = 144 * 1024 + 16384, WS_THREADS = 512;   // every wave-specialised geometry: ring + column-sum fold

enum GemmFamily {
  GEMM_NONE = 0,          // nothing to launch (empty output) or no kernel (bad layout)
  GEMM_SKINNY_F32,        // gemm_skinny_f32_kernel
  GEMM_WS_KK,             // gemm_ws_kernel<TM, TN, false, EK>
  GEMM_WS_OO,             // gemm_ws_kernel<3, 3, true, 0>
  GEMM_GLDS_KK,           // gemm_glds_kernel<T, tile, EK>
  GEMM_GLDS_OO,           // gemm_glds_tr_kernel
  GEMM_STAGED             // gemm_kernel<T, a_layout, b_layout, tile>
};

struct GemmRoute {
  int family = GEMM_NONE;
  int tile_m = 0, tile_n = 0;
  int ek = 0;                          // compile-time epilogue mask of the instantiation
  int tiles_m = 0, tiles_n = 0;
  int grid = 0, threads = 0, lds = 0;  // workgroups, threads per workgroup, dynamic LDS bytes
  int splits = 1, k_per_split = 0;     // reduction ranges actually cut, and their length
  int group = 0;                       // M-tiles per L2 locality group
  bool prescale = false;               // C <- beta * C (gemm_scale_f32) in front: the fp32-atomic accumulate paths
  int slot = 0;                        // GemmProfSlot
  double flops = 0.0;
};

// Reduction splits a request for split_k gets: at most one per k-tile, rounded so that no split is empty (*per: k-tiles each).
inline int split_count(int K, int split_k, int bk, int* per) {
  const int ktiles = (K + bk - 1) / bk;
  int split = split_k < ktiles ? split_k : ktiles;
  if (split <= 1) return 1;
  *per = (ktiles + split - 1) / split;
  return (ktiles + *per - 1) / *per;
}

// ---- runtime epilogue flags -> compile-time EK, one function per family -------------------------------------------------
// Wave-specialised K,K: the six hot-path combinations, ReLU with the saved output on the GELU slot, and on the 64-row tiles
// (rows64) the LinearLayer form (frame_transform, model/layers.py:86-93 + model/model.py:211-212): relu(x W^T + b) + matched
// features.  -1: the family has no instantiation (no generic fallback); column sums exist in the gelu' epilogue only.
inline int ws_epilogue_kind(const HeroGemmEpilogue& e, bool rows64) {
  const bool b = e.bias != nullptr, r = e.residual != nullptr, d = e.dropout.threshold16 != 0;
  if (e.colsum != nullptr && e.act != HERO_ACT_GELU_BWD && e.act != HERO_ACT_MUL_AUX) return -1;
  if (e.act == HERO_ACT_NONE && b && !r && !d) return EK_BIAS;
  if (e.act == HERO_ACT_NONE && b && r) return EK_BIAS | EK_RES | EK_DROP;
  if ((e.act == HERO_ACT_GELU || e.act == HERO_ACT_GELU_DG) && b && !r && !d) return EK_BIAS | EK_GELU;
  if (e.act == HERO_ACT_RELU && b && !r && !d && e.aux) return EK_BIAS | EK_GELU;
  if (rows64 && e.act == HERO_ACT_RELU && b && r && !d && e.aux) return EK_BIAS | EK_GELU | EK_RES;
  if (e.act == HERO_ACT_NONE && !b && !r && !d) return 0;
  if (e.act == HERO_ACT_NONE && !b && r && !d) return EK_RES;
  if ((e.act == HERO_ACT_GELU_BWD || e.act == HERO_ACT_MUL_AUX) && !b && !r && !d) return EK_GELU_BWD;
  return -1;
}
// 4-wave direct-to-LDS K,K: the hot-path combinations of the bf16 training step get their own instantiation, everything
// else (and all of f32, fp32 outputs, reduction splits) the generic one.
inline int glds_epilogue_kind(const HeroGemmEpilogue& e, bool bf16, int splits) {
  const bool b = e.bias != nullptr, r = e.residual != nullptr, d = e.dropout.threshold16 != 0;
  if (!bf16 || e.out_f32 || splits > 1) return EK_GENERIC;
  if (e.act == HERO_ACT_NONE && b && !r && !d) return EK_BIAS;
  if (e.act == HERO_ACT_NONE && b && r) return EK_BIAS | EK_RES | EK_DROP;
  if ((e.act == HERO_ACT_GELU || e.act == HERO_ACT_GELU_DG) && b && !r && !d) return EK_BIAS | EK_GELU;
  if (e.act == HERO_ACT_NONE && !b && !r && !d) return 0;
  if (e.act == HERO_ACT_NONE && !b && r && !d) return EK_RES;
  if ((e.act == HERO_ACT_GELU_BWD || e.act == HERO_ACT_MUL_AUX) && !b && !r && !d) return EK_GELU_BWD;
  return EK_GENERIC;
}

// ---- 4-wave geometry (measured on MI355X, tools/gemm_bench.py): the 128x128 tile with two resident
// workgroups per CU is the best or within a few % of the best on every shape of the HERO step; the
// 256x256 tile wins ~5 % on the largest K-contiguous problems only.
inline int pick_tile4(int M, int N, int splits, bool k_contig, const GemmForce& force) {
  if (force.tile4 >= 0) return force.tile4;
  if (!k_contig || splits != 1) return 0;
  const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
  if (t128 <= 192) return 3;                                                // under one 128^2 tile per CU
  // a little over ONE round of the 512 resident slots (N = 768 at M = 12000: 564 tiles): 192x128 tiles
  // fit in a single round (378) - measured 12-18 % faster there, 5 % slower where 128^2 needs 3+ rounds
  if (t128 > 512 && t128 <= 700 && (long long)((M + 191) / 192) * ((N + 127) / 128) <= 512) return 1;
  // one 256x256 workgroup per CU: only worth it when the tiles fill whole rounds of the 256 CUs
  const long long tiles = (long long)((M + 255) / 256) * ((N + 255) / 256);
  const long long rounds = (tiles + 255) / 256;
  return (tiles >= 256 && tiles * 10 >= rounds * 256 * 9) ? 2 : 0;
}

// ---- the wave-specialised family.  Problems it takes: bf16, K,K operands with an epilogue it has an instantiation for, or
// the O,O wgrad accumulate; large enough to fill the chip with 192 x 192 (or, under one round, 128 x 192) tiles.  A forced
// geometry holds where the shape is legal.  (Round 4's deferred-epilogue variant - the finished tile parked in the loader
// waves' registers and drained during the next main loop, bit-exact and 1.0-1.3x SLOWER, profiles/r04_wsd_ab.txt - lives
// in tools/lab/gemm_wsd.hip.)  false: not this family's problem, *out untouched.
inline bool route_ws(GemmRoute* out, int M, int N, int K, int lda, int ldb, int ldc, bool kk, bool oo, const HeroGemmEpilogue& epi,
                     const GemmForce& force, int cus) {
  const int geo = force.ws_geometry;
  if (!force.allow_ws || (!kk && !oo)) return false;
  if (K < 64 || N % 8 != 0 || M < 8) return false;
  if ((geo == WS_GEO_2x3 || geo == WS_GEO_1x2 || geo == WS_GEO_1x3) && !kk) return false;
  GemmRoute r;
  r.threads = WS_THREADS; r.lds = WS_LDS; r.group = 8;
  const int tiles_n = (N + 191) / 192, ntile = ((M + 191) / 192) * tiles_n;
  auto done = [&](int tm, int tn, int ek, int slot) {
    r.tile_m = 64 * tm; r.tile_n = 64 * tn; r.ek = ek; r.slot = slot;
    r.tiles_m = (M + r.tile_m - 1) / r.tile_m; r.tiles_n = (N + r.tile_n - 1) / r.tile_n;
    const int nwork = r.tiles_m * r.tiles_n * r.splits;
    r.grid = nwork < cus ? nwork : cus;                                  // persistent workgroups, one per CU
    *out = r;
    return true;
  };
  if (kk) {
    if (K % 64 != 0 || epi.out_f32 || epi.split_k > 1) return false;
    // every per-lane offset of this family is relative to its tile (operand panels, residual / saved pre-activation reads,
    // stores); only the weight matrix B is addressed from its base
    if ((size_t)N * ldb * 2 >= 0x7fffffffull || (size_t)192 * lda * 2 >= 0x7fffffffull || (size_t)192 * ldc * 2 >= 0x7fffffffull) return false;
    r.family = GEMM_WS_KK; r.k_per_split = K;
    int tm = 3, tn = 3;
    // Geometry by rounds: the persistent workgroups walk ceil(tiles / CUs) tiles each, and a 128 x 192 tile (Geo<2, 3>)
    // costs ~0.75-0.8 of a 192 x 192 one (tools/lab/geo_ab.py: 11 vs 15 us per round at K = 768, 30 vs 40 at K = 3072).
    // The smaller tile wins where it does not need proportionally more rounds:
    //  * under one round (M = 1920, N = 3072: 240 instead of 160 tiles; N = 2304: 180 instead of 120);
    //  * just over a round boundary of the 192 x 192 grid - the usual case of a ragged batch: M = 14450 rows, N = 768
    //    = 304 tiles = 2 rounds at 59 % against 452 tiles of 128 x 192 = 2 rounds at 88 %: 32.4 -> 25.4 us (K = 768),
    //    80.7 -> 67.0 (K = 3072).  The bench batch sits ON the boundary (12000 rows x 768 = 252 tiles) and keeps 192 x 192.
    const int t23 = ((M + 127) / 128) * tiles_n;
    const int r33 = (ntile + cus - 1) / cus, r23 = (t23 + cus - 1) / cus;
    // Under half a round of 192 x 192 tiles - the Temporal Transformer's 1920 rows into N = 768: 40 tiles - the 64-row
    // geometries: 64 x 128 tiles (180 workgroups, 24 KB per step, a 6-deep ring so that as many bytes are in flight as the
    // large tiles keep with three stages).  The 4-wave 64 x 64 kernels put 360 workgroups of 16 KB steps on 256 CUs and are
    // bound by the busiest CU's L2 -> LDS fill (two tiles x 48 steps: 26 us at K = 3072, the vendor library 17.7,
    // profiles/r04_vs_library.txt); 18.2 us with this geometry, 6.7 vs 8.0 at K = 768 (tools/lab/smallm_ws.py).
    const int rows64 = (M + 63) / 64;
    const int t12 = rows64 * ((N + 127) / 128), t13 = rows64 * tiles_n;
    if (geo == WS_GEO_2x3 || (force.heuristic && r23 * 4 < r33 * 5 && t23 * 5 >= cus * 2)) {
      tm = 2;
    } else if (geo == WS_GEO_1x3 || (force.heuristic && ntile * 2 < cus && K >= 512 && t12 > cus && t13 <= cus)) {
      // 64 x 192 (four stages) where 64 x 128 tiles would spill into a second round: the ragged batch's ~3100 padded frame rows
      // (49 x 6 = 294 tiles against 49 x 4 = 196); per tile it is ~20 % behind 64 x 128, a partial second round costs more
      tm = 1;
    } else if (geo == WS_GEO_1x2 || (force.heuristic && ntile * 2 < cus && K >= 512 && t12 * 8 >= cus && t12 <= cus)) {
      tm = 1; tn = 2;                // down to the 480 query rows (48 tiles: 12.0 vs 13.7 us at K = 2304)
    } else if (geo != WS_GEO_3x3 && ntile * 2 < cus) {
      return false;                  // worth it from about half a round of tiles; below that the 4-wave 64 x 64 / 128 x 128 tiles fill the chip better
    }
    const int ek = ws_epilogue_kind(epi, tm == 1);
    return ek >= 0 && done(tm, tn, ek, tm == 3 ? PROF_WS_KK_192 : PROF_WS_KK_SMALL);
  }
  // O,O: fp32 accumulate, reduction split so that the items fill the CUs
  if (!epi.out_f32 || epi.act != HERO_ACT_NONE || epi.bias || epi.residual || epi.dropout.threshold16 != 0 || epi.colsum) return false;
  if (M % 8 != 0) return false;
  if ((size_t)K * lda * 2 >= 0xffffffffull || (size_t)K * ldb * 2 >= 0xffffffffull) return false;
  const int ksteps = (K + 63) / 64;
  // The fp32-atomic merge costs ~split x output bytes at ~1.2 TB/s (measured: 31 us for 4 x 9.4 MB) and is paid
  // after the last k-step by every item at once: worth it only where few splits fill the chip (>= 64 tiles of
  // 192 x 192, i.e. the 3072 x 768 weights: 77 vs 84 us); smaller outputs stay on the 128 x 128 kernel's finer
  // split.  (Tried and dropped: 96 x 96 tiles with the reduction split across the four compute waves of a
  // workgroup and no cross-workgroup merge - 104 vs 82 us: four times the LDS-DMA bytes per flop, and the
  // direct-to-LDS path of a CU saturates near 50 GB/s while MFMAs and fragment reads are running.)
  if (geo != WS_GEO_3x3 && (ksteps < 32 || ntile < 64)) return false;
  int split = cus / ntile;                               // at most one round of items
  if (split > ksteps / 4) split = ksteps / 4;
  if (split < 1) split = 1;
  const int per = (ksteps + split - 1) / split;
  r.family = GEMM_WS_OO;
  r.splits = (ksteps + per - 1) / per;
  r.k_per_split = per * 64;
  r.prescale = epi.beta != 1.f;
  return done(3, 3, 0, PROF_WS_OO);
}

// The single place that decides.  The epilogue's pointers are read only as null / non-null.
inline GemmRoute gemm_route(int M, int N, int K, int lda, int ldb, int ldc, int a_layout, int b_layout, int dtype,
                            const HeroGemmEpilogue& epi, const GemmForce& force, int cus) {
  GemmRoute r;
  const bool bf16 = dtype == HERO_BF16;
  const bool kk = a_layout == HERO_LAYOUT_K && b_layout == HERO_LAYOUT_K, oo = a_layout == HERO_LAYOUT_O && b_layout == HERO_LAYOUT_O;
  if (M <= 0 || N <= 0 || (unsigned)a_layout > 1u || (unsigned)b_layout > 1u) return r;
  const double flops = 2.0 * (double)M * (double)N * (double)K;
  if (!bf16 && kk && M <= 32 && K >= 256 && force.heuristic && epi.act == HERO_ACT_NONE && !epi.residual && !epi.colsum && !epi.out_f32 &&
      epi.split_k <= 1 && epi.dropout.threshold16 == 0) {               // the loss head's fp32 Linear layers on the 32 query vectors
    r.family = GEMM_SKINNY_F32; r.tile_m = 32; r.tile_n = 8; r.tiles_m = 1; r.tiles_n = (N + 7) / 8;
    r.grid = r.tiles_n; r.threads = 256;
    r.lds = 32 * (K < 1024 ? K : 1024) * 4 + 16;                        // + the dummy slot of the copy
    r.k_per_split = K; r.slot = PROF_F32_SKINNY; r.flops = flops;
    return r;
  }
  if (bf16 && route_ws(&r, M, N, K, lda, ldb, ldc, kk, oo, epi, force, cus)) {   // large problems: wave-specialised persistent tiles (gemm_ws.hip)
    r.flops = flops;
    return r;
  }
  // the 4-wave kernels: one workgroup per (tile, reduction split)
  const int bk = bf16 ? 64 : 32;
  int per = 0;
  r.splits = epi.split_k > 1 ? split_count(K, epi.split_k, bk, &per) : 1;
  r.k_per_split = r.splits > 1 ? per * bk : (K > 0 ? ((K + bk - 1) / bk) * bk : bk);
  r.prescale = r.splits > 1 && epi.split_stride == 0 && epi.beta != 1.f;   // atomics accumulate into beta * C (slabs are overwritten)
  // M-tiles per L2 locality group (tools/gemm_group_sweep.py): wide outputs like 16 (N = 3072: -4 %),
  // narrow ones 4 (N = 768: -2 %), 8 in between
  r.group = force.group ? force.group : (N >= 2560 ? 16 : (N <= 1024 ? 4 : 8));
  int tile = pick_tile4(M, N, r.splits, kk, force);
  r.ek = EK_GENERIC;
  if (oo && bf16 && force.use_glds && K > 0 && r.k_per_split % 64 == 0) {
    r.family = GEMM_GLDS_OO; tile = 0; r.lds = 65536; r.slot = PROF_BF16_OO;
  } else if (kk && force.use_glds && K > 0 && K % bk == 0 && r.k_per_split % bk == 0) {
    r.family = GEMM_GLDS_KK; r.lds = tile4_glds_lds(GEMM_TILE4[tile]); r.slot = bf16 ? PROF_BF16_KK : PROF_F32_KK;
    r.ek = glds_epilogue_kind(epi, bf16, r.splits);
  } else {
    r.family = GEMM_STAGED;
    tile = tile == 2 ? 2 : 0;          // register staging exists for 128 x 128 and 256 x 256 only
    r.lds = tile4_staged_lds(GEMM_TILE4[tile]); r.slot = (bf16 ? PROF_BF16_KK : PROF_F32_KK) + a_layout * 2 + b_layout;
  }
  const Tile4 t = GEMM_TILE4[tile];
  r.tile_m = t.bm; r.tile_n = t.bn; r.threads = t.threads;
  r.tiles_m = (M + t.bm - 1) / t.bm; r.tiles_n = (N + t.bn - 1) / t.bn;
  r.grid = r.tiles_m * r.tiles_n * r.splits;
  r.flops = flops;
  return r;
}

}  // namespace hero
