// Shared pieces of the wave-specialised persistent GEMM family (gemm_ws.hip): geometry and work-item order, the loader
// waves' DMA stream, the compute waves' fragment reader and main loop, the staging of an epilogue pass and the K,K
// epilogue.  The kernels of gemm_ws.hip differ in where the stream goes next (a panel source) and in what happens to a
// finished tile.  Roles, ring and LDS images are described at the top of gemm_ws.hip.
// (tools/lab/gemm_wsd.hip, a lab kernel outside the library, is built on this header too.)
#pragma once
#include <vector>

#include "gemm_args.h"

namespace hero {
namespace ws {

typedef __attribute__((ext_vector_type(8))) short bf16x8_t;
typedef __attribute__((ext_vector_type(4))) short bf16x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;

constexpr int NS = 3;                 // ring stages of the 192 x 192 / 128 x 192 geometries (Geo::NSG: per geometry)
constexpr int SPARE_OFF = 144 * 1024; // 16 KiB behind the largest ring: column-sum fold

// Cache policy of the epilogue stores (buffer-store aux bits; 2 = nt: streaming, no allocation priority in the L2).
// Measured on the bench step (same box): both K,K outputs nt 52.8 us per launch / 6.96 ms per step against 54.7 / 7.05
// with the default policy - the output of a tile is not read again by this kernel, and the panels the other CUs are
// re-reading stay in the L2.
#ifndef HERO_WS_STORE_AUX
#define HERO_WS_STORE_AUX 2          // the main output of a K,K tile
#endif
#ifndef HERO_WS_STORE_AUX2
#define HERO_WS_STORE_AUX2 2         // the saved pre-activation (read again only in the backward pass)
#endif
#ifndef HERO_WS_LOAD_AUX_A
#define HERO_WS_LOAD_AUX_A 0         // cache policy of the direct-to-LDS operand loads (lab)
#endif
#ifndef HERO_WS_LOAD_AUX_B
#define HERO_WS_LOAD_AUX_B 0
#endif
#ifndef HERO_WS_STORE_DW
#define HERO_WS_STORE_DW 0           // dW tiles of the batched wgrad (read again by the optimiser)
#endif
#define HERO_LDS_PTR(p) ((__attribute__((address_space(3))) void*)(p))
template <int N> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }
__device__ __forceinline__ void wait_lds() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Scheduling pattern of a region that holds NM MFMAs and ND LDS reads (ND <= 2 NM): MFMA, PER reads, MFMA, PER reads, ...
// (sched_group_barrier masks: 0x008 MFMA, 0x100 DS read).  HERO_WS_BLOCKED restores the round-2 order for A/B runs.
template <int NM, int ND, int PER>
__device__ __forceinline__ void ws_interleave() {
#ifndef HERO_WS_BLOCKED
  if constexpr (NM > 0) {
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    if constexpr (ND >= PER) __builtin_amdgcn_sched_group_barrier(0x100, PER, 0);
    else if constexpr (ND > 0) __builtin_amdgcn_sched_group_barrier(0x100, ND, 0);
    ws_interleave<NM - 1, (ND >= PER ? ND - PER : 0), PER>();
  }
#else
  __builtin_amdgcn_sched_group_barrier(0x100, ND, 0);
  __builtin_amdgcn_sched_group_barrier(0x008, NM, 0);
#endif
}
#define WS_INTERLEAVE(NM, ND) ws_interleave<(NM), (ND), ((ND) > (NM) ? 2 : 1)>()

#ifdef HERO_WS_TRACE
// timeline probe (tools/lab/trace_ws.py): s_memtime stamps of the first four items of workgroup 0, per wave
static __device__ unsigned long long g_ws_trace[4 * 16 * 8];   // one per translation unit
#define WS_T(item_no, ev, wave, lane)                                                                   \
  do {                                                                                                  \
    if (blockIdx.x == 0 && (lane) == 0 && (item_no) >= 0 && (item_no) < 4)                              \
      g_ws_trace[((item_no) * 16 + (ev)) * 8 + (wave)] = __builtin_readcyclecounter();                  \
  } while (0)
#else
#define WS_T(item_no, ev, wave, lane) do { } while (0)
#endif

struct WsArgs {
  const void* A;
  const void* B;
  void* C;
  int M, N, K, lda, ldb, ldc;       // output M x N, reduction K
  int tiles_m, tiles_n, group, nsplit, k_per_split, nwork;
  HeroGemmEpilogue epi;
};

template <int TM_, int TN_> struct Geo {
  static constexpr int TM = TM_, TN = TN_;
  static constexpr int BM = 64 * TM, BN = 64 * TN;
  static constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE = A_BYTES + B_BYTES;
  static constexpr int PA = BM / 32, PB = BN / 32, PW = PA + PB;      // 1-KiB pieces per loader wave per stage
  static constexpr int ROWB = BN * 4;                                   // fp32 staging row
  static constexpr int RPP = (STAGE / ROWB >= 64 && BM % 64 == 0) ? 64 : 32;   // rows per epilogue pass
  static constexpr int PASSES = BM / RPP;
  static constexpr int C8 = BN / 8, RPI = 512 / C8, ITERS = (RPP + RPI - 1) / RPI;
  // ring depth: what fits under the spare region, at most 6.  The 64-row geometries (small-M GEMMs) move 24-32 KB per step
  // and need the deeper ring to keep as many bytes in flight as the large tiles do with three stages.
  static constexpr int NSG = SPARE_OFF / STAGE > 6 ? 6 : SPARE_OFF / STAGE;
  static constexpr int LDS = SPARE_OFF + 16384;
  static_assert(NSG >= 3 && NSG * STAGE <= SPARE_OFF && RPP * ROWB <= STAGE && RPI * BN * 4 <= 16384 && (NSG - 2) * PW < 64, "LDS budget");
  static_assert(TM_ < 2 || NSG == NS, "the large geometries keep the three-stage ring");
};

struct Item { int m0, n0, kbeg, nk; };

template <typename G>
__device__ __forceinline__ Item item_coord(const WsArgs& g, int item) {
  const int ntile = g.tiles_m * g.tiles_n;
  const int split = item / ntile;
  const int tile = item - split * ntile;
  const int per_group = g.group * g.tiles_n;
  const int group = tile / per_group;
  const int first_m = group * g.group;
  const int gsz = min(g.tiles_m - first_m, g.group);
  const int in_group = tile - group * per_group;
  Item it;
  it.m0 = (first_m + in_group % gsz) * G::BM;
  it.n0 = (in_group / gsz) * G::BN;
  it.kbeg = split * g.k_per_split;
  it.nk = (min(g.K, it.kbeg + g.k_per_split) - it.kbeg + 63) >> 6;
  return it;
}

__device__ __forceinline__ int swz_k(int row) { return (row ^ (row >> 3)) & 7; }
// O,O image: chunk swizzle of reduction row k for a tile row of RB bytes
template <int RB> __device__ __forceinline__ int swz_o(int k) { return RB % 256 == 0 ? 4 * (k & 3) : 4 * ((k >> 1) & 1); }

// ------------------------------------------------------------------------------------------------
// loader waves
// ------------------------------------------------------------------------------------------------
// One stretch of the DMA stream: nk 64-k stages of the panels A (BM rows / columns at m0) and B (BN at n0) from
// reduction index k0 on.  K,K operands are [M, lda] / [N, ldb] (rows past M / N are clamped to the last one), O,O operands
// [K, lda] / [K, ldb] (stages past K are out of range for the descriptor and deliver zeros).
struct Panel {
  const bf16_t* A;
  const bf16_t* B;
  int lda, ldb, M, N, K;
  int m0, n0, k0, nk;
};

// A panel source tells the loader where the stream goes next: done() - the stream has ended; panel() - the stretch that
// starts now; advance() - that stretch has been issued; DMA - false drops the loads (lab ablation, timing only).
// This one walks the work items of a WsArgs launch (item_coord order), every nwg-th from `item` on.
template <typename G>
struct ItemSource {
  static constexpr bool DMA = true;
  const WsArgs& g;
  int item, nwg;
  __device__ __forceinline__ bool done() const { return item >= g.nwork; }
  __device__ __forceinline__ Panel panel() const {
    const Item ic = item_coord<G>(g, item);
    return Panel{static_cast<const bf16_t*>(g.A), static_cast<const bf16_t*>(g.B), g.lda, g.ldb, g.M, g.N, g.K, ic.m0, ic.n0, ic.kbeg, ic.nk};
  }
  __device__ __forceinline__ void advance() { item += nwg; }
};

template <typename G, bool TR, typename Src>
struct Loader {
  Src src;
  char* smem;
  int w, lane;
  int ik, nk;             // stage being issued next / stages of the current stretch
  unsigned fill;          // ring cursor
  unsigned goa[G::PA], gob[G::PB];
  const char* pa;         // stage base of the A / B panels (uniform)
  const char* pb;
  // O,O bounds: bytes from the stage base to the end of the operand (64-bit: 1.4 M rows x 3072 columns at config 5; the
  // descriptor base moves with the k-step, so offsets stay small and only the range is clamped to 32 bits)
  unsigned long long ra_left, rb_left;
  unsigned sa, sb;        // bytes the bases move per stage

  __device__ __forceinline__ Loader(const Src& src_, char* smem_, int w_, int lane_)
      : src(src_), smem(smem_), w(w_), lane(lane_), ik(0), nk(0), fill(0), pa(nullptr), pb(nullptr), ra_left(0), rb_left(0), sa(0), sb(0) {
    if (!src.done()) setup();
  }
  __device__ __forceinline__ void setup() {
    const Panel p = src.panel();
    nk = p.nk;
    if (!TR) {
#pragma unroll
      for (int i = 0; i < G::PA; ++i) {
        const int r = (w * G::PA + i) * 8 + (lane >> 3);
        goa[i] = (unsigned)(min(p.m0 + r, p.M - 1) - p.m0) * (unsigned)p.lda * 2u + (((lane & 7) ^ swz_k(r)) << 4);
      }
#pragma unroll
      for (int i = 0; i < G::PB; ++i) {
        const int r = (w * G::PB + i) * 8 + (lane >> 3);
        gob[i] = (unsigned)(min(p.n0 + r, p.N - 1) - p.n0) * (unsigned)p.ldb * 2u + (((lane & 7) ^ swz_k(r)) << 4);
      }
      pa = reinterpret_cast<const char*>(p.A + (size_t)p.m0 * p.lda + p.k0);
      pb = reinterpret_cast<const char*>(p.B + (size_t)p.n0 * p.ldb + p.k0);
      ra_left = rb_left = 0ull;                          // unused
      sa = sb = 128u;
    } else {
      constexpr int CA = G::BM / 8, CB = G::BN / 8;      // 16-B chunks per tile row
#pragma unroll
      for (int i = 0; i < G::PA; ++i) {
        const int id = (w * G::PA + i) * 64 + lane, row = id / CA, c = (id % CA) ^ swz_o<G::BM * 2>(row);
        goa[i] = (unsigned)row * (unsigned)p.lda * 2u + (c << 4);
      }
#pragma unroll
      for (int i = 0; i < G::PB; ++i) {
        const int id = (w * G::PB + i) * 64 + lane, row = id / CB, c = (id % CB) ^ swz_o<G::BN * 2>(row);
        gob[i] = (unsigned)row * (unsigned)p.ldb * 2u + (c << 4);
      }
      // A is [K, lda] with the tile's M columns at m0; B is [K, ldb] with the N columns at n0
      pa = reinterpret_cast<const char*>(p.A + (size_t)p.k0 * p.lda + p.m0);
      pb = reinterpret_cast<const char*>(p.B + (size_t)p.k0 * p.ldb + p.n0);
      // The operand ends behind column M - 1 (N - 1) of its LAST row, not a whole leading dimension behind that row's first
      // column: a tile that reaches past M reads, in the last row, columns that belong to nobody - with A a column slice of
      // a wider tensor (dY[:, col0:]) up to col0 elements behind the end of the allocation, whatever the allocator left there.
      // Those columns are never stored, but the selector MFMA of the bias-gradient ride spreads a NaN among them (0 x NaN)
      // over the sums of the wave's other column blocks.  Out of range reads as 0.
      // This closes the LAST row only.  In the rows before it a tile wider than M still loads what stands to the right of the
      // slice in the same tensor - the neighbouring slice, the pad columns of the leading dimension, the start of the next
      // row - and the selector multiplies it by 0: the ride REQUIRES every element of the rows [0, K) of the tensor that A
      // is a slice of, pad columns included, to be finite (a NaN or Inf there reaches the bias gradients of valid columns).
      ra_left = ((unsigned long long)(p.K - 1 - p.k0) * p.lda + (p.M - p.m0)) * 2;
      rb_left = ((unsigned long long)(p.K - 1 - p.k0) * p.ldb + (p.N - p.n0)) * 2;
      sa = 64u * (unsigned)p.lda * 2u;
      sb = 64u * (unsigned)p.ldb * 2u;
    }
  }
  // Descriptor range of a stage: K,K rows are clamped by setup(), nothing to bound.  O,O: clamped at 0xffffffff, so that every
  // count below 4 GB - all that gemm_ws_kernel / gemm_wsg_kernel are launched with - is the range itself, as with the 32-bit
  // counters these kernels had; above it (batched kernel, config 5; it used to clamp at 0xfffffff0) any value past the
  // < 2^31 bytes a stage touches does.
  __device__ __forceinline__ static unsigned range(unsigned long long left) {
    return !TR ? 0x7fffffffu : (unsigned)(left < 0xffffffffull ? left : 0xffffffffull);
  }
  // issue the next stage of the stream (false: the stream has ended)
  __device__ __forceinline__ bool issue() {
    if (src.done()) return false;
    stage();
    return true;
  }
  __device__ __forceinline__ void stage() {
    char* buf = smem + fill;
    const __amdgpu_buffer_rsrc_t ra = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pa), 0, range(ra_left), 0x00020000);
    const __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<char*>(pb), 0, range(rb_left), 0x00020000);
    if constexpr (Src::DMA) {
#pragma unroll
      for (int i = 0; i < G::PA; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(ra, HERO_LDS_PTR(buf + (w * G::PA + i) * 1024), 16, goa[i], 0, 0, HERO_WS_LOAD_AUX_A);
#pragma unroll
      for (int i = 0; i < G::PB; ++i)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rb, HERO_LDS_PTR(buf + G::A_BYTES + (w * G::PB + i) * 1024), 16, gob[i], 0, 0, HERO_WS_LOAD_AUX_B);
    }
    fill += G::STAGE;
    if (fill == G::NSG * G::STAGE) fill = 0;
    if (++ik == nk) {
      ik = 0;
      src.advance();
      if (!src.done()) setup();
    } else {
      pa += sa; pb += sb;
      if (TR) {
        ra_left = ra_left > sa ? ra_left - sa : 0ull;
        rb_left = rb_left > sb ? rb_left - sb : 0ull;
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------
// compute waves
// ------------------------------------------------------------------------------------------------
// Fragment reader of compute wave (wm, wn): per-lane LDS offsets inside a stage (slice 0) and the reads of one 16-k slice.
// TR = false: K,K image, one ds_read_b128 per fragment; TR = true: O,O image, two transposing 64-bit reads.
// Read order a[0], b[0..], a[1..]: the MFMAs of the NEXT slice run (i outer, j inner), the reads are spread over the
// MFMAs of the current slice in this order, so every fragment is requested >= 7 MFMAs (224 cycles) before its first
// use (a[0..], b[0..] order: 5 MFMAs for b[0] - less than the LDS latency beside the DMA writes).
template <typename G, bool TR>
struct Frags {
  static constexpr int TM = G::TM, TN = G::TN;
  static constexpr int NRD = TR ? 2 * (TM + TN) : TM + TN;            // LDS reads per slice
  unsigned ao[TM], bo[TN];
  __device__ __forceinline__ Frags(int wm, int wn, int lane) {
    const int arow0 = wm * TM * 32, brow0 = wn * TN * 32;
    if (!TR) {
      const int r = lane & 31, kg = lane >> 5;
#pragma unroll
      for (int i = 0; i < TM; ++i) { const int ra = arow0 + i * 32 + r; ao[i] = ra * 128 + ((kg ^ swz_k(ra)) << 4); }
#pragma unroll
      for (int j = 0; j < TN; ++j) { const int rb = brow0 + j * 32 + r; bo[j] = G::A_BYTES + rb * 128 + ((kg ^ swz_k(rb)) << 4); }
    } else {
      const int p = lane & 15, gq = (lane >> 4) & 1, kg = lane >> 5;
      const int krow = kg * 8 + (p >> 2);
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int col = arow0 + i * 32 + gq * 16 + 4 * (p & 3);
        ao[i] = krow * (G::BM * 2) + ((((col >> 3) ^ swz_o<G::BM * 2>(krow)) << 4) | ((col & 7) * 2));
      }
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        const int col = brow0 + j * 32 + gq * 16 + 4 * (p & 3);
        bo[j] = G::A_BYTES + krow * (G::BN * 2) + ((((col >> 3) ^ swz_o<G::BN * 2>(krow)) << 4) | ((col & 7) * 2));
      }
    }
  }
  template <int RB>                                                   // RB: bytes of a reduction row of the O,O image
  __device__ __forceinline__ static bf16x8_t read(const char* st, unsigned off, int ks) {
    if (!TR) {
      return *reinterpret_cast<const bf16x8_t*>(st + (off ^ (ks << 5)));
    } else {
      typedef __attribute__((address_space(3))) bf16x4_t* lp_t;
      const char* q = st + off + ks * 16 * RB;
      const bf16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(q));
      const bf16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp_t)(q + 4 * RB));
      return bf16x8_t{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    }
  }
  __device__ __forceinline__ void load(bf16x8_t (&a)[TM], bf16x8_t (&b)[TN], const char* st, int ks) const {
    a[0] = read<G::BM * 2>(st, ao[0], ks);
#pragma unroll
    for (int j = 0; j < TN; ++j) b[j] = read<G::BN * 2>(st, bo[j], ks);
#pragma unroll
    for (int i = 1; i < TM; ++i) a[i] = read<G::BM * 2>(st, ao[i], ks);
  }
};

// lab ablations of the main loop (timing only, results are garbage): no fragment reads / no MFMAs / no step barrier
enum { LAB_NOLDF = 1, LAB_NOMFMA = 2, LAB_NOBAR = 4 };

// Main loop of a compute wave: two fragment register sets, the accumulators and the ring cursor.
// SWAP: the MFMA operands are swapped (D^T = B A^T: lane <-> output row, a lane holds 4 consecutive columns of a row), which
// is what stage_pass wants; unswapped, a half-wave holds 32 consecutive columns (atomic_tile).
template <typename G, bool TR, bool SWAP, int LAB = 0>
struct MainLoop {
  static constexpr int TM = G::TM, TN = G::TN;
  Frags<G, TR> fr;
  const char* smem;
  bf16x8_t a0[TM], b0[TN], a1[TM], b1[TN];
  f32x16_t acc[TM][TN];
  // The ride (batched wgrad, bias gradient = column sums of the dY panel, the operand a[i]: lane <-> dW row): one more MFMA
  // per row block against a constant SELECTOR - sel_i[mm][k] = 1 for the eight output rows mm = 8 i .. 8 i + 7, else 0 - so
  // that rows 8 i .. 8 i + 7 of ONE extra accumulator collect block i's sums: accumulator register 4 i of lane l < 32 = the
  // sum of column arow0 + 32 i + l of the tile.  3 MFMAs on top of 9 per 16-k slice on a loop whose matrix pipe is about half
  // idle, no LDS traffic, 16 more registers.
  f32x16_t accb;
  unsigned selw[TM];
  unsigned curo, last;      // ring cursor: the stage read next / the stage read last (the epilogue's staging slot)

  __device__ __forceinline__ MainLoop(const char* smem_, int wm, int wn, int lane) : fr(wm, wn, lane), smem(smem_), curo(0), last(0) {
#pragma unroll
    for (int i = 0; i < TM; ++i) selw[i] = ((lane & 31) >> 3) == i ? 0x3f803f80u : 0u;       // two bf16 ones
  }
  __device__ __forceinline__ void ldf(bf16x8_t (&a)[TM], bf16x8_t (&b)[TN], const char* st, int ks) {
    if constexpr (!(LAB & LAB_NOLDF)) fr.load(a, b, st, ks);
  }
  // Slice 0 of the stage at the cursor (start of the stream, and again behind an epilogue that used the ring).  The empty asm
  // pins the reads to the call site: without it the compiler merges the two sites of a kernel into the top of the item loop,
  // behind the item's coordinate arithmetic, and their latency is no longer covered by it (64 x 128 tiles, two items per
  // workgroup: +1 - 2 %).
  __device__ __forceinline__ void read_first() {
    ldf(a0, b0, smem + curo, 0);
    asm volatile("");
  }
  template <bool RIDE>
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    if constexpr (RIDE) {
#pragma unroll
      for (int e = 0; e < 16; ++e) accb[e] = 0.f;
    }
    last = curo;
  }
  template <bool RIDE>
  __device__ __forceinline__ void mma(const bf16x8_t (&a)[TM], const bf16x8_t (&b)[TN]) {
    if constexpr (LAB & LAB_NOMFMA) {
      asm volatile("" ::"v"(a[0]), "v"(b[0]), "v"(a[TM - 1]), "v"(b[TN - 1]));
    } else {
#pragma unroll
      for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          if (SWAP) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(b[j], a[i], acc[i][j], 0, 0, 0);
          else acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
        }
        if constexpr (RIDE) {
          const u32x4_t w4 = {selw[i], selw[i], selw[i], selw[i]};
          accb = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, w4), a[i], accb, 0, 0, 0);
        }
      }
    }
  }
  // nk 64-k steps.  One scheduling region per 16-k slice: the fragment reads of the NEXT slice are spread between the MFMAs
  // of the current one (MFMA, 1-2 reads, MFMA, ...).  Issued as a block in front of the MFMAs (round 2) the reads cost ~140
  // cycles of MFMA-idle issue time per slice: 0.89 us per 64-k step with the DMA switched off against 0.58 us of MFMA issue
  // (tools/lab/wsb_sweep.py, noloads).  RIDE is a template argument: a branch inside the loop would split its regions.
  template <bool RIDE>
  __device__ __forceinline__ void run(int nk) {
    constexpr int NM = TM * TN + (RIDE ? TM : 0), NRD = Frags<G, TR>::NRD;
    for (int t = 0; t < nk; ++t) {
      const char* cur = smem + curo;
      last = curo;
      curo += G::STAGE;
      if (curo == G::NSG * G::STAGE) curo = 0;
      const char* nxt = smem + curo;
      ldf(a1, b1, cur, 1);
      mma<RIDE>(a0, b0);
      WS_INTERLEAVE(NM, NRD);
      __builtin_amdgcn_sched_barrier(0);
      ldf(a0, b0, cur, 2);
      mma<RIDE>(a1, b1);
      WS_INTERLEAVE(NM, NRD);
      __builtin_amdgcn_sched_barrier(0);
      ldf(a1, b1, cur, 3);
      mma<RIDE>(a0, b0);
      WS_INTERLEAVE(NM, NRD);
      __builtin_amdgcn_sched_barrier(0);
      wait_lds();
      if constexpr (!(LAB & LAB_NOBAR)) __builtin_amdgcn_s_barrier();   // B(u): done reading `cur`, stage u+1 landed
      __builtin_amdgcn_sched_barrier(0);
      // unconditional (a branch around it doubles the MFMA code and spills): behind the last step of a stretch this reads the
      // landed first stage of the next one - read again behind an epilogue that used the ring - or stale LDS, never used
      ldf(a0, b0, nxt, 0);
      mma<RIDE>(a1, b1);
      WS_INTERLEAVE(NM, NRD);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
};

// fp32 atomics straight from the UNSWAPPED accumulator layout of a wave whose fragments start at (m0, n0): 32 consecutive
// columns per half-wave, two rows per instruction
template <int TM, int TN>
__device__ __forceinline__ void atomic_tile(float* C, int ldc, int M, int N, int m0, int n0, const f32x16_t (*acc)[TN], int lane) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int gn = n0 + j * 32 + (lane & 31);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int gm = m0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (gm < M && gn < N) atomicAdd(C + (size_t)gm * ldc + gn, acc[i][j][r]);
      }
    }
}

// ------------------------------------------------------------------------------------------------
// epilogues through LDS (swapped accumulators): the thread's place in a pass and the staging of a pass
// ------------------------------------------------------------------------------------------------
// A pass stages RPP rows of the tile as fp32 in a ring slot (16-byte chunks XOR-swizzled by row); all 8 waves then work on
// full rows, thread (r0 + it * RPI, c8) on 8 columns.
// Everything derived from the thread index is recomputed per tile from an opaque copy: hoisted out of the item loop these
// values stay live across the main loop, where 144 accumulators + 48 fragment registers leave no room, and get spilled to
// scratch (a reload = one memory round trip at the start of every epilogue).
template <typename G>
struct PassLane {
  static constexpr int TM = G::TM, TN = G::TN, RPP = G::RPP;
  // With three passes over a 192-row tile the two 32-row blocks of a pass are taken from the two wave rows (block p of
  // each), so that all four compute waves stage 12 fragments per pass instead of two waves staging 24 (the staging of a
  // pass was 2100 cycles of a 5300-cycle pass, tools/lab/trace_ws.py).
  static constexpr bool SPLIT = (RPP == 64 && G::PASSES == TM);
  int tid, lane, wave, c8, r0;
  __device__ __forceinline__ PassLane() {
    tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    lane = tid & 63;
    wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    c8 = tid % G::C8;
    r0 = tid / G::C8;
  }
  // row of the tile that row `row` of pass p holds
  __device__ __forceinline__ static int tile_row(int p, int row) { return SPLIT ? (row >> 5) * (TM * 32) + p * 32 + (row & 31) : p * RPP + row; }
  // compute waves: this wave's share of pass p, accumulators -> the pass image at st (ds_write_b128)
  __device__ __forceinline__ void stage_pass(char* st, int p, const f32x16_t (*acc)[TN]) const {
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, half = lane >> 5;
#pragma unroll
    for (int b = 0; b < RPP / 32; ++b) {
      const int blk = SPLIT ? b * TM + p : p * (RPP / 32) + b;   // 32-row block of the tile
      if (wm == blk / TM) {
        const int i = blk % TM;                     // compile-time after unrolling
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int chunk = (wn * TN * 32 + j * 32 + 8 * q + 4 * half) >> 2;
            const f32x4_t v = {acc[i][j][4 * q], acc[i][j][4 * q + 1], acc[i][j][4 * q + 2], acc[i][j][4 * q + 3]};
            *reinterpret_cast<f32x4_t*>(st + (32 * b + l31) * G::ROWB + ((chunk ^ (l31 & 7)) << 4)) = v;
          }
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------
// K,K epilogue: run by all 8 waves; the compute waves additionally stage their accumulators
// ------------------------------------------------------------------------------------------------
template <typename G, int EK, bool COMPUTE>
__device__ __forceinline__ void epilogue_rows(const WsArgs& g, const Item& ic, char* smem, unsigned slot, f32x16_t (*acc)[G::TN], int wave,
                                              int lane, int trace_item = -1) {
  constexpr int BN = G::BN, RPP = G::RPP, RPI = G::RPI, ITERS = G::ITERS;
  const HeroGemmEpilogue& e = g.epi;
  char* st = smem + slot;
  const PassLane<G> pl;                               // opaque copy of the thread index: see PassLane
  const int tid = pl.tid, c8 = pl.c8, r0 = pl.r0;
  lane = pl.lane;
  wave = pl.wave;
  const bool active = r0 < RPI;
  const int gn = ic.n0 + c8 * 8;
  const bool col_ok = active && gn < g.N;
  const int gnc = min(gn, g.N - 8);
  bf16_t* Cb = static_cast<bf16_t*>(g.C);
  const bf16_t* R = (EK & EK_RES) ? static_cast<const bf16_t*>(e.residual) : nullptr;
  bf16_t* X = static_cast<bf16_t*>(e.aux);
  // tile-relative store descriptors (offsets inside a tile stay far below 2^31 bytes whatever the size of C)
  const size_t torg = (size_t)ic.m0 * g.ldc + ic.n0;
  const __amdgpu_buffer_rsrc_t rsc = __builtin_amdgcn_make_buffer_rsrc(Cb + torg, 0, 0x7fffffff, 0x00020000);
  const __amdgpu_buffer_rsrc_t rsx = __builtin_amdgcn_make_buffer_rsrc((EK & EK_GELU) ? X + torg : Cb + torg, 0, 0x7fffffff, 0x00020000);
  DropCtx drop(e.dropout);
  const bool use_drop = (EK & EK_DROP) && drop.on();
  float bias[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (EK & EK_BIAS) {
    const float4 b0 = *reinterpret_cast<const float4*>(e.bias + gnc);
    const float4 b1 = *reinterpret_cast<const float4*>(e.bias + gnc + 4);
    bias[0] = b0.x; bias[1] = b0.y; bias[2] = b0.z; bias[3] = b0.w;
    bias[4] = b1.x; bias[5] = b1.y; bias[6] = b1.z; bias[7] = b1.w;
  }
  const bool do_csum = (EK & EK_GELU_BWD) && e.colsum != nullptr;
  const bool save_dg = (EK & EK_GELU) && e.act == HERO_ACT_GELU_DG, mul_aux = (EK & EK_GELU_BWD) && e.act == HERO_ACT_MUL_AUX;
  const bool relu = (EK & EK_GELU) && e.act == HERO_ACT_RELU;      // uniform: the activation-with-saved-value instantiations serve ReLU too
  float cs[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  auto tile_row = [](int p, int row) { return PassLane<G>::tile_row(p, row); };

#pragma unroll
  for (int p = 0; p < G::PASSES; ++p) {
    // residual / saved pre-activation of this pass: fetched before the accumulators are staged
    uint4 pre[ITERS];
    unsigned off[ITERS];
    bool ok[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = r0 + it * RPI;
      const int gm = ic.m0 + tile_row(p, row);
      ok[it] = col_ok && row < RPP && gm < g.M;
      // tile-relative (like the stores): the matrix itself may hold more than 2^32 elements (config 5: 1.5 M rows x 3072)
      off[it] = (unsigned)(min(gm, g.M - 1) - ic.m0) * (unsigned)g.ldc + (unsigned)(gnc - ic.n0);
      if (EK & EK_RES) pre[it] = *reinterpret_cast<const uint4*>(R + torg + off[it]);
      if (EK & EK_GELU_BWD) pre[it] = *reinterpret_cast<const uint4*>(X + torg + off[it]);
    }
    WS_T(trace_item, 2 + 4 * p, wave, lane);
    if constexpr (COMPUTE) pl.stage_pass(st, p, acc);
    wait_lds();
    WS_T(trace_item, 3 + 4 * p, wave, lane);
    __builtin_amdgcn_s_barrier();                    // E1: the pass is staged
    WS_T(trace_item, 4 + 4 * p, wave, lane);
    // All iterations are computed first (branch-free: inactive threads and rows past the pass read a clamped row and
    // store nothing), THEN the stores are issued back to back.  With a store inside each iteration the compiler put
    // an s_waitcnt vmcnt(0) in front of the next iteration's arithmetic (its registers were the store's data), i.e.
    // every iteration waited for the previous store's round trip to HBM: 4 serialised round trips per pass.
    uint4 outv[ITERS], auxv[(EK & EK_GELU) ? ITERS : 1];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const int row = min(r0 + it * RPI, RPP - 1);
      {
        const int x = row & 7;
        const f32x4_t v0 = *reinterpret_cast<const f32x4_t*>(st + row * G::ROWB + (((2 * c8) ^ x) << 4));
        const f32x4_t v1 = *reinterpret_cast<const f32x4_t*>(st + row * G::ROWB + (((2 * c8 + 1) ^ x) << 4));
        float v[8] = {v0[0], v0[1], v0[2], v0[3], v1[0], v1[1], v1[2], v1[3]};
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] += bias[k];
        if (EK & EK_GELU) {
          uint4 u;
          if (save_dg) {                                // uniform (HERO_ACT_GELU_DG): the derivative is saved, not the pre-activation
            float dg[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) gelu_both<bf16_t>(v[k], v[k], dg[k]);
            u.x = f2bf_pk(dg[0], dg[1]); u.y = f2bf_pk(dg[2], dg[3]); u.z = f2bf_pk(dg[4], dg[5]); u.w = f2bf_pk(dg[6], dg[7]);
          } else if (relu) {                            // HERO_ACT_RELU: aux <- relu(acc + bias), the value before the residual
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = fmaxf(v[k], 0.f);
            u.x = f2bf_pk(v[0], v[1]); u.y = f2bf_pk(v[2], v[3]); u.z = f2bf_pk(v[4], v[5]); u.w = f2bf_pk(v[6], v[7]);
          } else {
            u.x = f2bf_pk(v[0], v[1]); u.y = f2bf_pk(v[2], v[3]); u.z = f2bf_pk(v[4], v[5]); u.w = f2bf_pk(v[6], v[7]);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = gelu_fwd<bf16_t>(v[k]);
          }
          auxv[(EK & EK_GELU) ? it : 0] = u;
        }
        float pv[8];                                  // residual / saved pre-activation as fp32
        if (EK & (EK_RES | EK_GELU_BWD)) {
          const uint32_t w4[4] = {pre[it].x, pre[it].y, pre[it].z, pre[it].w};
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            pv[2 * k] = __uint_as_float(w4[k] << 16);
            pv[2 * k + 1] = __uint_as_float(w4[k] & 0xffff0000u);
          }
        }
        if (EK & EK_GELU_BWD) {
          if (mul_aux) {                                // uniform (HERO_ACT_MUL_AUX): aux already holds gelu'
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= pv[k];
          } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] *= gelu_grad<bf16_t>(pv[k]);
          }
        }
        if (use_drop) {
          const int gm = ic.m0 + tile_row(p, row);
          const uint64_t grp = ((uint64_t)gm * (uint64_t)g.N + (uint64_t)gn) >> 2;
          const float4 m0 = drop.mask4(grp), m1 = drop.mask4(grp + 1);
          v[0] *= m0.x; v[1] *= m0.y; v[2] *= m0.z; v[3] *= m0.w;
          v[4] *= m1.x; v[5] *= m1.y; v[6] *= m1.z; v[7] *= m1.w;
        }
        if (EK & EK_RES) {
#pragma unroll
          for (int k = 0; k < 8; ++k) v[k] += pv[k];
        }
        if (do_csum && ok[it]) {
#pragma unroll
          for (int k = 0; k < 8; ++k) cs[k] += v[k];
        }
        uint4 o;
        o.x = f2bf_pk(v[0], v[1]); o.y = f2bf_pk(v[2], v[3]); o.z = f2bf_pk(v[4], v[5]); o.w = f2bf_pk(v[6], v[7]);
        outv[it] = o;
      }
    }
    // Branch-free stores: a masked-off lane gets an offset past the descriptor's range and the hardware drops it.
    // (Behind `if (ok)` every store sat in its own basic block, and each block re-waited vmcnt(0) for the bias /
    // residual loads of the tile start - which by then also meant the previous block's store.)
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
      const unsigned vo = ok[it] ? (unsigned)(tile_row(p, r0 + it * RPI) * g.ldc + c8 * 8) * 2u : 0xffffffffu;
      if (EK & EK_GELU) {
        const uint4 u = auxv[(EK & EK_GELU) ? it : 0];
        __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{u.x, u.y, u.z, u.w}, rsx, vo, 0, HERO_WS_STORE_AUX2);
      }
      __builtin_amdgcn_raw_buffer_store_b128(u32x4_t{outv[it].x, outv[it].y, outv[it].z, outv[it].w}, rsc, vo, 0, HERO_WS_STORE_AUX);
    }
    wait_lds();
    WS_T(trace_item, 5 + 4 * p, wave, lane);
    __builtin_amdgcn_s_barrier();                    // E2: the slot may be restaged / refilled
  }
  WS_T(trace_item, 14, wave, lane);
  if (EK & EK_GELU_BWD) {                            // uniform across the workgroup (kernel argument)
    if (e.colsum != nullptr) {
      float* sp = reinterpret_cast<float*>(smem + SPARE_OFF);
      if (active) {
        *reinterpret_cast<f32x4_t*>(sp + r0 * BN + c8 * 8) = f32x4_t{cs[0], cs[1], cs[2], cs[3]};
        *reinterpret_cast<f32x4_t*>(sp + r0 * BN + c8 * 8 + 4) = f32x4_t{cs[4], cs[5], cs[6], cs[7]};
      }
      wait_lds();
      __builtin_amdgcn_s_barrier();                  // E3
      if (tid < BN && ic.n0 + tid < g.N) {
        float t = 0.f;
#pragma unroll 4
        for (int k = 0; k < RPI; ++k) t += sp[k * BN + tid];
        if (e.colsum_partial) {
          // deterministic: this tile's sums go to row (m0 / 64) of the [ceil(M / 64), N] partial table, zeros to the rows of
          // the tile's other 64-row blocks - whatever the tile height, the table's column sums are the result
          float* pr = e.colsum + (size_t)(ic.m0 >> 6) * g.N + ic.n0 + tid;
          const int nb = min(G::BM >> 6, ((g.M + 63) >> 6) - (ic.m0 >> 6));
          pr[0] = t;
          for (int b = 1; b < nb; ++b) pr[(size_t)b * g.N] = 0.f;
        } else {
          atomicAdd(e.colsum + ic.n0 + tid, t);
        }
      }
      // the next writer of the spare region is the next tile's fold, >= one step barrier away
    }
  }
}


}  // namespace ws
}  // namespace hero
