// Types shared by the GEMM translation units (gemm.hip: 4-wave tiles, gemm_ws.hip: wave-specialised
// persistent tiles).  Which kernel a problem gets is decided in gemm_route.h alone.
#pragma once
#include "common.h"
#include "gemm_route.h"

namespace hero {

// per-launch timing with HIP events on the launch stream (bench.py roofline leg; gemm.hip owns the slots: GemmProfSlot)
void* gemm_prof_begin(int slot, hipStream_t s);
void gemm_prof_end(void* token, double flops, hipStream_t s);

// C <- beta * C over an [M, N] fp32 matrix (pre-pass of the fp32-atomic accumulate paths; gemm.hip)
int gemm_scale_f32(float* C, int M, int N, int ldc, float beta, hipStream_t s);

int num_cus();                // compute units of the current device, 256 where there is none (gemm_ws.hip)

// Logical workgroup index of block `bid` of an nwg-block grid.  The hardware deals consecutive block ids round-robin to the
// 8 XCDs; in the logical order every XCD owns one contiguous chunk, so neighbouring tiles share their panels in its L2.
__device__ __forceinline__ int xcd_order(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

const GemmForce& gemm_force();     // the decoded hero_gemm_force_config state (gemm.hip)

// gemm_ws.hip: launches a route of the wave-specialised families (GEMM_WS_KK / GEMM_WS_OO).  C[M,N] (+)= op(A) op(B).
int gemm_ws_launch(const GemmRoute& r, const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                   const HeroGemmEpilogue& epi, hipStream_t s);

}  // namespace hero
