// Beam-search selection of the captioning decode (gfx950): one call per decode step takes the step's prediction scores
// [R = N * B, V] and the beam tables of all N captions to the next step, on the device, without a host read.
//
//   live beam b      candidates (b, v), v in [0, V):  score = cum[b] + (logit[b, v] - lse_b),  lse_b = max + log(sum exp(x - max))
//   finished beam b  exactly one candidate (b, eos) with score cum[b], unchanged
//   choice           the B best candidates of a caption by score, among equal scores the lower flat index b * V + v; new beam i
//                    is the i-th best.  With parent p and token v:  cum'[i] = score, fin'[i] = fin[p] | (v == eos),
//                    len'[i] = len[p] + (fin[p] ? 0 : 1), ids'[i, :t] = ids[p, :t], ids'[i, t] = v, anc'[i, :t] = anc[p, :t],
//                    anc'[i, t] = n * B + p, last[i] = v.
// All arithmetic is fp32 whatever the storage dtype of the scores.
//
// Every candidate is the 64-bit composite of retrieval.hip, (order_bits(score) << 32) | ~flat index: composites are unique,
// larger = better, so the tie rule is an integer comparison and nothing depends on the order in which candidates are met.
//   beam_rows_kernel   one workgroup per row.  Pass 1: the row's maximum and sum, online per thread, folded over the wave on the
//                      DPP network and over the four waves in a fixed order.  Pass 2 (the row comes from the L2 now): every
//                      element's composite; a thread keeps the 8 best of its elements sorted in registers, and B rounds of a
//                      workgroup-wide maximum pop the row's B best - no more than B of a caption's best B can come from one beam.
//                      Writes cand [R, B]; a finished row writes its one candidate and B - 1 empty slots (composite 0 is below
//                      every real one: an index is never 2^32 - 1).
//   beam_merge_kernel  one workgroup per caption.  Ranks the B * B composites by counting, stages the caption's OLD tables in
//                      LDS, and only behind a barrier writes the new ones: beams mix only within a caption, so the in-place
//                      update is safe for any parent assignment, cycles included.
// No floating-point atomics, no atomics at all: two runs give the same bits.  The launches allocate nothing and read nothing
// on the host; the step position comes from a device int32 (a captured launch serves every step) or from the host.
#include "select_rows.h"

namespace hero {
namespace {

constexpr int BM_MAX_B = 8, BM_MAX_V = 65536, BM_MAX_T = 128, BM_NT = 256, BM_WAVES = BM_NT / 64;

struct BeamSel {
  const void* logits;            // [R, ld]
  const int* pos_dev;
  float* cum;                    // [R]
  int *fin, *len, *ids, *anc, *last;   // [R], [R], [R, Tcap], [R, Tcap], [R]
  unsigned long long* cand;      // workspace [R, B]
  int pos, N, B, V, ld, Tcap, eos, vec;
};

template <typename T>
__global__ __launch_bounds__(BM_NT) void beam_rows_kernel(BeamSel a) {
  __shared__ float red_m[BM_WAVES], red_s[BM_WAVES];
  __shared__ unsigned long long red_c[2][BM_WAVES];
  const int r = blockIdx.x, b = r % a.B, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  unsigned long long* out = a.cand + (size_t)r * a.B;
  const float cum = a.cum[r];
  if (a.fin[r] != 0) {                                              // uniform over the workgroup
    if (tid < a.B) out[tid] = tid == 0 ? compose(order_bits(cum), (uint32_t)(b * a.V + a.eos)) : 0ull;
    return;
  }
  const T* row = static_cast<const T*>(a.logits) + (size_t)r * a.ld;
  const bool vec = a.vec != 0;
  const float lse = row_lse<T, BM_NT>(row, a.V, vec, red_m, red_s).lse;

  unsigned long long top[BM_MAX_B];
#pragma unroll
  for (int k = 0; k < BM_MAX_B; ++k) top[k] = 0ull;
  const int flat0 = b * a.V;
  for_row<T, BM_NT>(row, a.V, vec, [&](int v, float x) {
    const unsigned long long c = compose(order_bits(cum + (x - lse)), (uint32_t)(flat0 + v));
    if (c > top[BM_MAX_B - 1]) {
      top[BM_MAX_B - 1] = c;
#pragma unroll
      for (int k = BM_MAX_B - 1; k > 0; --k) {
        const unsigned long long hi = top[k - 1], lo = top[k];
        top[k - 1] = lo > hi ? lo : hi;
        top[k] = lo > hi ? hi : lo;
      }
    }
  });
  for (int i = 0; i < a.B; ++i) {                                   // the buffers alternate: one barrier per round
    const unsigned long long w = wave_max_u64(top[0]);
    if (lane == 0) red_c[i & 1][wave] = w;
    __syncthreads();
    unsigned long long best = red_c[i & 1][0];
#pragma unroll
    for (int k = 1; k < BM_WAVES; ++k) best = red_c[i & 1][k] > best ? red_c[i & 1][k] : best;
    if (best != 0ull && top[0] == best) {                           // composites are unique: one thread pops
#pragma unroll
      for (int k = 0; k + 1 < BM_MAX_B; ++k) top[k] = top[k + 1];
      top[BM_MAX_B - 1] = 0ull;
    }
    if (tid == 0) out[i] = best;
  }
}

__global__ __launch_bounds__(BM_NT) void beam_merge_kernel(BeamSel a) {
  __shared__ unsigned long long cs[BM_MAX_B * BM_MAX_B];
  __shared__ int par[BM_MAX_B], tok[BM_MAX_B], o_fin[BM_MAX_B], o_len[BM_MAX_B];
  __shared__ float sc[BM_MAX_B];
  __shared__ int o_ids[BM_MAX_B * BM_MAX_T], o_anc[BM_MAX_B * BM_MAX_T];
  const int t = step_position(a.pos_dev, a.pos);
  if (t < 0 || t >= a.Tcap) return;                                 // uniform over the grid: a device position cannot be refused on the host
  const int tid = threadIdx.x, B = a.B, Tcap = a.Tcap, row0 = blockIdx.x * B, nc = B * B;
  if (tid < nc) cs[tid] = a.cand[(size_t)row0 * B + tid];
  if (tid < B) {
    o_fin[tid] = a.fin[row0 + tid];
    o_len[tid] = a.len[row0 + tid];
    par[tid] = tid;                                                 // what a row keeps if the candidates were fewer than B (they are not)
    tok[tid] = a.eos;
    sc[tid] = a.cum[row0 + tid];
  }
  for (int e = tid; e < B * Tcap; e += BM_NT) {
    if (e % Tcap < t) {
      o_ids[e] = a.ids[(size_t)row0 * Tcap + e];
      o_anc[e] = a.anc[(size_t)row0 * Tcap + e];
    }
  }
  __syncthreads();
  if (tid < nc) {
    const unsigned long long c = cs[tid];
    int rank = 0;
    for (int k = 0; k < nc; ++k) rank += cs[k] > c ? 1 : 0;
    if (c != 0ull && rank < B) {
      const int flat = (int)~(uint32_t)c;
      par[rank] = min(flat / a.V, B - 1);
      tok[rank] = flat % a.V;
      sc[rank] = order_float((uint32_t)(c >> 32));
    }
  }
  __syncthreads();                                                  // every read of the old tables is behind us
  if (tid < B) {
    const int p = par[tid], v = tok[tid], r = row0 + tid;
    a.cum[r] = sc[tid];
    a.fin[r] = (o_fin[p] != 0 || v == a.eos) ? 1 : 0;
    a.len[r] = o_len[p] + (o_fin[p] != 0 ? 0 : 1);
    a.last[r] = v;
    a.ids[(size_t)r * Tcap + t] = v;
    a.anc[(size_t)r * Tcap + t] = row0 + p;
  }
  for (int e = tid; e < B * Tcap; e += BM_NT) {
    const int i = e / Tcap, j = e % Tcap;
    if (j < t) {
      a.ids[(size_t)row0 * Tcap + e] = o_ids[par[i] * Tcap + j];
      a.anc[(size_t)row0 * Tcap + e] = o_anc[par[i] * Tcap + j];
    }
  }
}

bool in_envelope(int dtype, int V, int B, int Tcap) {
  return (dtype == HERO_F32 || dtype == HERO_BF16) && B >= 1 && B <= BM_MAX_B && V >= B && V <= BM_MAX_V && Tcap >= 1 && Tcap <= BM_MAX_T;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_beam_in_envelope(int dtype, int V, int B, int Tcap) { return in_envelope(dtype, V, B, Tcap) ? 1 : 0; }

extern "C" int hero_beam_select(const void* logits, float* cum, int* fin, int* len, int* ids, int* anc, int* last, void* workspace,
                                const int* pos_dev, int pos, int N, int B, int V, int ld, int Tcap, int eos, int dtype,
                                hero_stream_t stream) {
  HERO_REQUIRE(in_envelope(dtype, V, B, Tcap) && N >= 1 && ld >= V && eos >= 0 && eos < V && (long long)N * B < (1ll << 24),
               "hero_beam_select: outside the envelope (fp32 / bf16, 1 <= B <= %d, B <= V <= %d, 1 <= Tcap <= %d, ld >= V, 0 <= eos < V, "
               "N >= 1): dtype=%d N=%d B=%d V=%d ld=%d Tcap=%d eos=%d", BM_MAX_B, BM_MAX_V, BM_MAX_T, dtype, N, B, V, ld, Tcap, eos);
  HERO_REQUIRE(logits && cum && fin && len && ids && anc && last && workspace, "hero_beam_select: null pointer");
  HERO_REQUIRE(pos_dev || (pos >= 0 && pos < Tcap), "hero_beam_select: position %d outside [0, Tcap = %d)", pos, Tcap);
  HERO_REQUIRE((((uintptr_t)workspace) & 7) == 0, "hero_beam_select: the workspace must be 8-byte aligned");
  const BeamSel a = {logits, pos_dev, cum, fin, len, ids, anc, last, static_cast<unsigned long long*>(workspace),
                     pos, N, B, V, ld, Tcap, eos, rows_vec4(logits, ld, dtype)};
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int rc = by_dtype(dtype, "hero_beam_select", [&](auto tag) {
    hipLaunchKernelGGL((beam_rows_kernel<typename decltype(tag)::type>), dim3(N * B), dim3(BM_NT), 0, st, a);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(beam_merge_kernel, dim3(N), dim3(BM_NT), 0, st, a);
  return check_launch("hero_beam_select");
}
