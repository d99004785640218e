// Row-wise softmax cross-entropy over wide logit rows, forward and backward (gfx950).
//
// Replaces F.cross_entropy at the pre-training heads (BASELINE configs[3]):
//   MLM     model/encoder.py:355-389 + model/layers.py:330-354: [n_masked, 50272] logits of the tied-weight
//           vocabulary GEMM (the last `pad` columns are vocabulary padding, model/encoder.py:232-233: excluded)
//   MFM-NCE model/model.py:271-291: [n_masked, n_masked + n_neg] logits / temperature
//   FOM     model/model.py:293-336: [B * L, max_clip_len] logits, ignore_index -1
// HBM-bound: forward reads the logits once (online max / sum per thread, one block per row), backward reads
// them once more and writes the gradient in the logits' dtype (may alias the logits):
//   loss_r = lse_r - x[r, y_r],   dx[r, c] = (exp(x[r, c] - lse_r) - [c == y_r]) * g_r * inv_temp
// with x = logits * inv_temp; rows whose label equals ignore_index give loss 0 and a zero gradient row.
//
// Four families live here - the plain loss, the same with the live row count on the device, the label-smoothed captioning
// loss, the validation counters - and all of them are built from ONE copy each of
//   label_live   which labels take part
//   row_walk     a 256-thread workgroup over one row: 16-byte groups of 8 columns where the rows are aligned, single columns behind
//   row_lse      the online soft-max scan: lse of the row on thread 0, in the FAST (x * t, __expf, __logf) or the accurate
//                (expf, logf) arithmetic, with the caller's hooks on the stored values (sum of x; arg-max)
//   grad_row     the gradient row of an element functor (column, x) -> dx, padding columns zero, dx may alias x
//   fold_tree    K sums over a workgroup's 256 partials in a fixed order, in the caller's accumulator type
#include <math.h>
#include "common.h"

namespace hero {
namespace {

template <typename T> __device__ __forceinline__ void ld8(const T* p, float (&v)[8]);
template <> __device__ __forceinline__ void ld8<bf16_t>(const bf16_t* p, float (&v)[8]) {
  const uint4 u = *reinterpret_cast<const uint4*>(p);
  const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) { v[2 * k] = __uint_as_float(w[k] << 16); v[2 * k + 1] = __uint_as_float(w[k] & 0xffff0000u); }
}
template <> __device__ __forceinline__ void ld8<float>(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
template <typename T> __device__ __forceinline__ void st8(T* p, const float (&v)[8]);
template <> __device__ __forceinline__ void st8<bf16_t>(bf16_t* p, const float (&v)[8]) {
  uint4 u;
  u.x = f2bf_pk(v[0], v[1]); u.y = f2bf_pk(v[2], v[3]); u.z = f2bf_pk(v[4], v[5]); u.w = f2bf_pk(v[6], v[7]);
  *reinterpret_cast<uint4*>(p) = u;
}
template <> __device__ __forceinline__ void st8<float>(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}

// ---- the shared pieces ----------------------------------------------------------------------------------------------
__device__ __forceinline__ bool label_live(long long y, long long ignore_index, int cols) { return !(y == ignore_index || y < 0 || y >= cols); }

// One row, the whole 256-thread workgroup: f8(c) for every group of 8 columns below cols when the leading dimension(s), OR-ed
// into `align`, allow 16-byte loads, then f1(c) for the single columns from there to `end` (cols, or ld to reach the padding).
// A thread meets its columns in ascending order.
__device__ __forceinline__ int row_vec_end(int align, int cols) { return ((align & 7) == 0) ? (cols & ~7) : 0; }
template <class F8, class F1>
__device__ __forceinline__ void row_walk(int align, int cols, int end, F8 f8, F1 f1) {
  const int vec_end = row_vec_end(align, cols);
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) f8(c);
  for (int c = vec_end + threadIdx.x; c < end; c += 256) f1(c);
}

// The two arithmetics of the soft-max: FAST for the pre-training heads (scaled by inv_temp), accurate for the smoothed loss,
// which is judged at a few 2^-24 (no scale: it has no temperature)
template <bool FAST> __device__ __forceinline__ float sm_exp(float x) { return FAST ? __expf(x) : expf(x); }
template <bool FAST> __device__ __forceinline__ float sm_log(float x) { return FAST ? __logf(x) : logf(x); }
template <bool FAST> __device__ __forceinline__ float sm_scale(float v, float t) { return FAST ? v * t : v; }
// (max, sum exp(x - max)) pairs combine associatively
template <bool FAST> __device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = s * sm_exp<FAST>(m - mx) + s2 * sm_exp<FAST>(m2 - mx);
  m = mx;
}
struct NoHook { template <class... A> __device__ __forceinline__ void operator()(A&&...) const {} };

// The online soft-max scan of one row: every thread's (max, sum exp) over its columns, folded over the wave (DPP) and the four
// waves; returns lse = log sum_c exp(x_c * t) on thread 0 (0 elsewhere).  The ONE statement of this arithmetic: the plain, counted
// and validation losses all call it, so their bits agree by construction.  h8(c, v[8]) / h1(c, v) see the stored values of the
// columns the thread meets.  park(lane, wave) is called once by EVERY thread behind the walk and before the one __syncthreads:
// there the caller folds what its hooks gathered over the wave (wave intrinsics are fine: no thread has left) and parks it
// in LDS of its own, to read it on thread 0 after row_lse returns.
template <bool FAST, typename T, class H8, class H1, class Park>
__device__ __forceinline__ float row_lse(const T* x, int cols, int ld, float t, H8 h8, H1 h1, Park park) {
  __shared__ float sm[4], ss[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -3.0e38f, s = 0.f;
  row_walk(
      ld, cols, cols,
      [&](int c) {
        float v[8];
        ld8<T>(x + c, v);
        float mx = sm_scale<FAST>(v[0], t);
#pragma unroll
        for (int k = 1; k < 8; ++k) mx = fmaxf(mx, sm_scale<FAST>(v[k], t));
        float e = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) e += sm_exp<FAST>(sm_scale<FAST>(v[k], t) - mx);
        ms_merge<FAST>(m, s, mx, e);
        h8(c, v);
      },
      [&](int c) {
        const float v = ld1<T>(x + c);
        ms_merge<FAST>(m, s, sm_scale<FAST>(v, t), 1.f);
        h1(c, v);
      });
  const float wm = wave_max(m);
  s = wave_sum(s * sm_exp<FAST>(m - wm));
  if (lane == 0) { sm[wave] = wm; ss[wave] = s; }
  park(lane, wave);
  __syncthreads();
  float lse = 0.f;
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) ms_merge<FAST>(M, S, sm[w], ss[w]);
    lse = M + sm_log<FAST>(S);
  }
  return lse;
}

// One gradient row dx[c] = f(c, x[c]) for c < cols and +0 in the padding; dx may alias x: a thread reads its columns before it
// writes them
template <typename T, class F>
__device__ __forceinline__ void grad_row(const T* x, T* dx, int cols, int ld, F f) {
  row_walk(
      ld, cols, ld,
      [&](int c) {
        float v[8];
        ld8<T>(x + c, v);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = f(c + k, v[k]);
        st8<T>(dx + c, v);
      },
      [&](int c) {
        float v = 0.f;
        if (c < cols) v = f(c, ld1<T>(x + c));
        st1<T>(dx + c, v);                                             // padding columns get a zero gradient
      });
}

// K sums over one 256-thread workgroup in a fixed order: thread i brings the partial sums v of its rows i, i + 256, ... (added
// in order), a halving tree adds the 256 partials; afterwards ps[k][0] is sum k, visible to every thread
template <typename A, int K>
__device__ __forceinline__ void fold_tree(A (&ps)[K][256], const A (&v)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) ps[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < K; ++k) ps[k][threadIdx.x] += ps[k][threadIdx.x + w];
    }
    __syncthreads();
  }
}

// ---- the plain loss ---------------------------------------------------------------------------------------------------
// thread 0 writes lse and the loss of one row
template <typename T>
__device__ __forceinline__ void ce_row_fwd(const T* x, long long y, int cols, int ld, float t, long long ignore_index, float* lse_out,
                                           float* loss_out) {
  const float lse = row_lse<true, T>(x, cols, ld, t, NoHook(), NoHook(), NoHook());
  if (threadIdx.x == 0) {
    *lse_out = lse;
    *loss_out = label_live(y, ignore_index, cols) ? lse - ld1<T>(x + y) * t : 0.f;
  }
}

// one gradient row with upstream g (already times inv_temp)
template <typename T>
__device__ __forceinline__ void ce_row_bwd(const T* x, T* dx, long long y, int cols, int ld, float t, float lse, float g) {
  grad_row<T>(x, dx, cols, ld, [=](int c, float v) { return (sm_exp<true>(v * t - lse) - ((long long)c == y ? 1.f : 0.f)) * g; });
}

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(HeroCrossEntropy a) {
  const int row = blockIdx.x;
  ce_row_fwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, a.labels[row], a.cols, a.ld, a.inv_temp, a.ignore_index, a.lse + row,
                a.loss + row);
}

// a dead row is multiplied by g = 0, not skipped: -0 under a label inside [0, cols) that equals ignore_index, NaN from a
// non-finite logit (ce_counted_bwd_kernel writes +0 and reads nothing)
template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(HeroCrossEntropy a) {
  const int row = blockIdx.x;
  const long long y = a.labels[row];
  const float t = a.inv_temp;
  ce_row_bwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, static_cast<T*>(a.dlogits) + (size_t)row * a.ld, y, a.cols, a.ld, t,
                a.lse[row], label_live(y, a.ignore_index, a.cols) ? a.dloss[row] * t : 0.f);
}

// ---- the same loss with the LIVE ROW COUNT ON THE DEVICE (fixed-capacity pre-training heads under graph replay) ------
// Row r is live when r < min(*count, rows) (count == nullptr: rows) and its label is valid.  Rows at or behind the count give
// loss = lse = 0 and a row of +0 gradients and their logits are never read (whatever they hold - the zero rows of a
// fixed-capacity gather, NaN - stays out); a row below the count with an ignored label computes lse and has loss 0, as above.
// One workgroup then folds the live rows' losses in float64 in a fixed order: mean_cnt = (mean over the live rows, their
// number); the backward divides the device scalar dloss[0] by that number on the device.  No atomics, no host read.
struct CeCounted {
  const void* logits;
  const long long* labels;
  const int32_t* count;
  float *loss, *lse, *mean_cnt;
  const float* dloss;
  void* dlogits;
  int rows, cols, ld;
  float inv_temp;
  long long ignore_index;
};

__device__ __forceinline__ int ce_live_rows(const CeCounted& a) { return a.count ? min(max(*a.count, 0), a.rows) : a.rows; }

template <typename T>
__global__ __launch_bounds__(256) void ce_counted_fwd_kernel(CeCounted a) {
  const int row = blockIdx.x;
  if (row >= ce_live_rows(a)) {                                       // uniform over the workgroup
    if (threadIdx.x == 0) { a.loss[row] = 0.f; a.lse[row] = 0.f; }
    return;
  }
  ce_row_fwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, a.labels[row], a.cols, a.ld, a.inv_temp, a.ignore_index, a.lse + row,
                a.loss + row);
}

// rows == 0 gives (0, 0)
__global__ __launch_bounds__(256) void ce_counted_fold_kernel(CeCounted a) {
  __shared__ double ps[2][256];
  const int n = ce_live_rows(a);
  double v[2] = {0.0, 0.0};
  for (int r = threadIdx.x; r < n; r += 256)
    if (label_live(a.labels[r], a.ignore_index, a.cols)) { v[0] += (double)a.loss[r]; v[1] += 1.0; }
  fold_tree(ps, v);
  if (threadIdx.x == 0) {
    const double live = ps[1][0];
    a.mean_cnt[0] = (float)(ps[0][0] / (live > 1.0 ? live : 1.0));
    a.mean_cnt[1] = (float)live;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_counted_bwd_kernel(CeCounted a) {
  const int row = blockIdx.x;
  T* dx = static_cast<T*>(a.dlogits) + (size_t)row * a.ld;
  bool live = row < ce_live_rows(a);
  long long y = -1;
  if (live) {
    y = a.labels[row];
    live = label_live(y, a.ignore_index, a.cols);
  }
  if (!live) {                                                        // +0 over all ld columns, nothing read
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    row_walk(a.ld, a.ld, a.ld, [&](int c) { st8<T>(dx + c, z); }, [&](int c) { st1<T>(dx + c, 0.f); });
    return;
  }
  const float t = a.inv_temp, g = a.dloss[0] / fmaxf(a.mean_cnt[1], 1.f);
  ce_row_bwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, dx, y, a.cols, a.ld, t, a.lse[row], g * t);
}

// ---- label-smoothed loss of the captioning decoder (model/tvc.py:19-64) -------------------------
// KL(smoothed one-hot || softmax(x)) of a row with label t, C = cols, s = eps / (C - 1), conf = 1 - eps, in closed form:
//   loss = H0 - (conf - s) (x_t - lse) - s (sum_c x_c - C lse),   H0 = conf ln conf + (C - 1) s ln s   (0 ln 0 = 0)
//   dx_c = (softmax(x)_c - s - (conf - s) [c == t]) * upstream
// so no [rows, C] target matrix exists.  Forward: one pass over the row (row_lse in the accurate arithmetic, its hook adding
// sum_c x_c in fp32), then ONE workgroup folds the row losses and counts the valid rows in a fixed order into a device pair.
// Backward: upstream is a device scalar (times an optional per-row factor); in mean mode it is divided by the valid count
// read from that pair - no host synchronisation.  Zero valid rows: loss 0, zero gradients.
struct SmoothCe {
  const void* logits;
  const long long* labels;
  float *loss, *lse, *sum_cnt;
  const float *dloss, *dloss_rows, *mean_cnt;
  void* dlogits;
  int rows, cols, ld;
  long long ignore_index;
  double cms, s, h0;                                  // conf - s, s, H0
};

__device__ __forceinline__ float sum8(const float (&v)[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

template <typename T>
__global__ __launch_bounds__(256) void smooth_ce_fwd_kernel(SmoothCe a) {
  __shared__ float sx[4];
  const int row = blockIdx.x;
  const T* x = static_cast<const T*>(a.logits) + (size_t)row * a.ld;
  float tot = 0.f;
  const float lse = row_lse<false, T>(
      x, a.cols, a.ld, 1.f, [&](int, const float (&v)[8]) { tot += sum8(v); }, [&](int, float v) { tot += v; },
      [&](int lane, int wave) {
        tot = wave_sum(tot);
        if (lane == 0) sx[wave] = tot;
      });
  if (threadIdx.x == 0) {
    const long long y = a.labels[row];
    a.lse[row] = lse;
    float loss = 0.f;
    if (label_live(y, a.ignore_index, a.cols)) {
      const double all = ((double)sx[0] + (double)sx[1]) + ((double)sx[2] + (double)sx[3]) - (double)a.cols * (double)lse;
      loss = (float)(a.h0 - a.cms * ((double)ld1<T>(x + y) - (double)lse) - a.s * all);
    }
    a.loss[row] = loss;
  }
}

// sum_cnt = (sum of the row losses, number of valid rows), in fp32
__global__ __launch_bounds__(256) void smooth_ce_fold_kernel(SmoothCe a) {
  __shared__ float ps[2][256];
  float v[2] = {0.f, 0.f};
  for (int r = threadIdx.x; r < a.rows; r += 256)
    if (label_live(a.labels[r], a.ignore_index, a.cols)) { v[0] += a.loss[r]; v[1] += 1.f; }
  fold_tree(ps, v);
  if (threadIdx.x == 0) { a.sum_cnt[0] = ps[0][0]; a.sum_cnt[1] = ps[1][0]; }
}

template <typename T>
__global__ __launch_bounds__(256) void smooth_ce_bwd_kernel(SmoothCe a) {
  const int row = blockIdx.x;
  const long long y = a.labels[row];
  const bool live = label_live(y, a.ignore_index, a.cols);
  const float lse = a.lse[row];
  float g = 0.f;
  if (live) {
    g = a.dloss[0];
    if (a.dloss_rows) g *= a.dloss_rows[row];
    if (a.mean_cnt) g /= fmaxf(a.mean_cnt[1], 1.f);
  }
  const float s = (float)a.s, cms = (float)a.cms;
  grad_row<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, static_cast<T*>(a.dlogits) + (size_t)row * a.ld, a.cols, a.ld,
              [=](int c, float v) { return live ? ((sm_exp<false>(v - lse) - s) - ((long long)c == y ? cms : 0.f)) * g : 0.f; });
}

// ---- validation counters of the pre-training heads (pretrain.py:462-608) --------------------------------------------
// One pass over the raw logits gives what validate_mlm / validate_mfm_nce / validate_fom take from F.cross_entropy(sum) and
// scores.max(-1): the row loss (row_lse in the FAST arithmetic, the call ce_fwd_kernel makes) and, from its hooks, the arg-max
// of the STORED values, lowest column first among equal maxima.  Row results go to a workspace; one workgroup folds them into
// float64 counters in a fixed order (no atomics: two runs give the same bits).
template <typename T>
__global__ __launch_bounds__(256) void ce_eval_kernel(const T* logits, const long long* labels, int cols, int ld, float t, long long ignore_index,
                                                      float* row_loss, float* row_hit, float* row_valid, int32_t* pred) {
  __shared__ unsigned long long sb[4];
  const int row = blockIdx.x;
  const T* x = logits + (size_t)row * ld;
  float bv = -INFINITY;                                               // a thread meets its columns in ascending order, so a
  int bi = 0x7fffffff;                                                // strict > keeps the first of equal values
  const float lse = row_lse<true, T>(
      x, cols, ld, t,
      [&](int c, const float (&v)[8]) {
        float b = bv;                                                 // local copies: updating bv through the reference eight times
        int i = bi;                                                   // made the compiler carry a second copy of it round the loop
#pragma unroll
        for (int k = 0; k < 8; ++k)
          if (v[k] > b) { b = v[k]; i = c + k; }
        bv = b;
        bi = i;
      },
      [&](int c, float v) {
        if (v > bv) { bv = v; bi = c; }
      },
      [&](int lane, int wave) {
        if (bi == 0x7fffffff) {                                       // nothing above -inf: the thread's first column, if it has one
          const int vec_end = row_vec_end(ld, cols);
          const int first = ((int)threadIdx.x * 8 < vec_end) ? (int)threadIdx.x * 8 : vec_end + (int)threadIdx.x;
          if (first < cols) bi = first;
        }
        // larger composite = larger value, then lower column (-0 and +0 tie): the maximum over the row is the prediction
        unsigned long long best = compose(order_bits(bv), (uint32_t)bi);
#pragma unroll
        for (int w = 32; w > 0; w >>= 1) {
          const unsigned long long o = __shfl_xor(best, w, 64);
          best = o > best ? o : best;
        }
        if (lane == 0) sb[wave] = best;
      });
  if (threadIdx.x == 0) {
    unsigned long long B = sb[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) B = sb[w] > B ? sb[w] : B;
    const int p = (int)~(uint32_t)B;
    const long long y = labels[row];
    const bool live = label_live(y, ignore_index, cols);
    row_loss[row] = live ? lse - ld1<T>(x + y) * t : 0.f;
    row_hit[row] = (live && (long long)p == y) ? 1.f : 0.f;
    row_valid[row] = live ? 1.f : 0.f;
    if (pred) pred[row] = p;
  }
}

// Per row of [rows, ld] predictions and targets: l2 = |p - t|, cos = p.t / (max(|p|, eps) max(|t|, eps)), eps = 1e-8
// (F.cosine_similarity), sums in fp32: each thread adds its columns in ascending order, then the 256 partial sums are
// added pairwise (lanes 2i and 2i+1, then pairs of pairs, ..., then the four waves the same way).
template <typename T>
__global__ __launch_bounds__(256) void feat_eval_kernel(const T* pred, const T* target, int cols, int ld_p, int ld_t, float* row_l2, float* row_cos) {
  __shared__ float sq[4][4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* p = pred + (size_t)row * ld_p;
  const T* g = target + (size_t)row * ld_t;
  float dd = 0.f, pg = 0.f, pp = 0.f, gg = 0.f;
  const auto add = [&](float a, float b) {
    const float d = a - b;
    dd += d * d; pg += a * b; pp += a * a; gg += b * b;
  };
  row_walk(
      ld_p | ld_t, cols, cols,
      [&](int c) {
        float a[8], b[8];
        ld8<T>(p + c, a);
        ld8<T>(g + c, b);
#pragma unroll
        for (int k = 0; k < 8; ++k) add(a[k], b[k]);
      },
      [&](int c) { add(ld1<T>(p + c), ld1<T>(g + c)); });
  dd = wave_sum(dd); pg = wave_sum(pg); pp = wave_sum(pp); gg = wave_sum(gg);
  if (lane == 0) { sq[0][wave] = dd; sq[1][wave] = pg; sq[2][wave] = pp; sq[3][wave] = gg; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float q[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = (sq[k][0] + sq[k][1]) + (sq[k][2] + sq[k][3]);
    row_l2[row] = sqrtf(q[0]);
    row_cos[row] = q[1] / (fmaxf(sqrtf(q[2]), 1e-8f) * fmaxf(sqrtf(q[3]), 1e-8f));
  }
}

// acc[0..2] += (sum a, sum b, sum c) in float64 (c == nullptr: the row count)
__global__ __launch_bounds__(256) void eval_fold_kernel(const float* a, const float* b, const float* c, int rows, double* acc) {
  __shared__ double ps[3][256];
  double v[3] = {0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < rows; r += 256) {
    v[0] += (double)a[r];
    v[1] += (double)b[r];
    v[2] += c ? (double)c[r] : 1.0;
  }
  fold_tree(ps, v);
  if (threadIdx.x < 3) acc[threadIdx.x] += ps[threadIdx.x][0];
}

// the dims check, then the dtype check: adjacent and in this order in six entries; min_cols is 2 for the smoothed pair, else 1
static int check_shape(const char* what, int rows, int cols, int ld, int min_cols, int dtype) {
  HERO_REQUIRE(rows >= 0 && cols >= min_cols && ld >= cols, "%s: bad dims rows=%d cols=%d ld=%d", what, rows, cols, ld);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
  return HERO_OK;
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_ce_eval(const void* logits, const long long* labels, int rows, int cols, int ld, int dtype, float inv_temp,
                            long long ignore_index, double* acc, int32_t* pred, void* workspace, hero_stream_t stream) {
  if (const int rc = check_shape("hero_ce_eval", rows, cols, ld, 1, dtype)) return rc;
  HERO_REQUIRE(inv_temp > 0.f, "hero_ce_eval: inv_temp must be positive, got %g", (double)inv_temp);
  if (rows == 0) return HERO_OK;
  HERO_REQUIRE(logits && labels && acc && workspace, "hero_ce_eval: null pointer");
  HERO_REQUIRE((((uintptr_t)logits) & 15) == 0, "hero_ce_eval: logits must be 16-byte aligned");
  HERO_REQUIRE((((uintptr_t)acc) & 7) == 0 && (((uintptr_t)workspace) & 3) == 0 && (((uintptr_t)pred) & 3) == 0,
               "hero_ce_eval: acc / workspace / pred misaligned");
  float* ws = static_cast<float*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = by_dtype(dtype, "hero_ce_eval", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(ce_eval_kernel<T>, dim3(rows), dim3(256), 0, s, static_cast<const T*>(logits), labels, cols, ld, inv_temp, ignore_index,
                       ws, ws + rows, ws + 2 * (size_t)rows, pred);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, s, ws, ws + rows, ws + 2 * (size_t)rows, rows, acc);
  return check_launch("hero_ce_eval");
}

extern "C" int hero_feat_eval(const void* pred, const void* target, int rows, int cols, int ld_p, int ld_t, int dtype, double* acc,
                              void* workspace, hero_stream_t stream) {
  HERO_REQUIRE(rows >= 0 && cols > 0 && ld_p >= cols && ld_t >= cols, "hero_feat_eval: bad dims rows=%d cols=%d ld_p=%d ld_t=%d", rows, cols, ld_p,
               ld_t);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "hero_feat_eval: bad dtype %d", dtype);
  if (rows == 0) return HERO_OK;
  HERO_REQUIRE(pred && target && acc && workspace, "hero_feat_eval: null pointer");
  HERO_REQUIRE(((((uintptr_t)pred) | ((uintptr_t)target)) & 15) == 0, "hero_feat_eval: pred / target must be 16-byte aligned");
  HERO_REQUIRE((((uintptr_t)acc) & 7) == 0 && (((uintptr_t)workspace) & 3) == 0, "hero_feat_eval: acc / workspace misaligned");
  float* ws = static_cast<float*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = by_dtype(dtype, "hero_feat_eval", [&](auto tag) {
    using T = typename decltype(tag)::type;
    hipLaunchKernelGGL(feat_eval_kernel<T>, dim3(rows), dim3(256), 0, s, static_cast<const T*>(pred), static_cast<const T*>(target), cols, ld_p,
                       ld_t, ws, ws + rows);
  });
  if (rc) return rc;
  hipLaunchKernelGGL(eval_fold_kernel, dim3(1), dim3(256), 0, s, ws, ws + rows, static_cast<const float*>(nullptr), rows, acc);
  return check_launch("hero_feat_eval");
}

static int check_ce(const HeroCrossEntropy* a, bool bwd) {
  HERO_REQUIRE(a && a->logits && a->labels && a->lse, "hero_cross_entropy: null pointer");
  if (const int rc = check_shape("hero_cross_entropy", a->rows, a->cols, a->ld, 1, a->dtype)) return rc;
  HERO_REQUIRE((((uintptr_t)a->logits) & 15) == 0, "hero_cross_entropy: logits must be 16-byte aligned");
  if (bwd) HERO_REQUIRE(a->dloss && a->dlogits && (((uintptr_t)a->dlogits) & 15) == 0, "hero_cross_entropy_bwd: dloss / dlogits required (16-byte aligned)");
  else HERO_REQUIRE(a->loss, "hero_cross_entropy_fwd: loss required");
  return HERO_OK;
}

extern "C" int hero_cross_entropy_fwd(const HeroCrossEntropy* a, hero_stream_t stream) {
  int rc = check_ce(a, false);
  if (rc) return rc;
  if (a->rows == 0) return HERO_OK;
  return by_dtype(a->dtype, "hero_cross_entropy_fwd", [&](auto tag) {
    hipLaunchKernelGGL(ce_fwd_kernel<typename decltype(tag)::type>, dim3(a->rows), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  });
}

extern "C" int hero_cross_entropy_bwd(const HeroCrossEntropy* a, hero_stream_t stream) {
  int rc = check_ce(a, true);
  if (rc) return rc;
  if (a->rows == 0) return HERO_OK;
  return by_dtype(a->dtype, "hero_cross_entropy_bwd", [&](auto tag) {
    hipLaunchKernelGGL(ce_bwd_kernel<typename decltype(tag)::type>, dim3(a->rows), dim3(256), 0, static_cast<hipStream_t>(stream), *a);
  });
}

static int check_counted(const char* what, const void* logits, const long long* labels, const float* lse, const float* mean_cnt, int rows,
                         int cols, int ld, int dtype, float inv_temp) {
  if (const int rc = check_shape(what, rows, cols, ld, 1, dtype)) return rc;
  HERO_REQUIRE(inv_temp > 0.f, "%s: inv_temp must be positive, got %g", what, (double)inv_temp);
  HERO_REQUIRE(mean_cnt && (((uintptr_t)mean_cnt) & 3) == 0, "%s: mean_cnt required (4-byte aligned)", what);
  if (rows == 0) return HERO_OK;
  HERO_REQUIRE(logits && labels && lse, "%s: null pointer", what);
  HERO_REQUIRE((((uintptr_t)logits) & 15) == 0, "%s: logits must be 16-byte aligned", what);
  return HERO_OK;
}

extern "C" int hero_ce_counted_fwd(const void* logits, const long long* labels, const int32_t* count, float* loss, float* lse, float* mean_cnt,
                                   int rows, int cols, int ld, int dtype, float inv_temp, long long ignore_index, hero_stream_t stream) {
  if (const int rc = check_counted("hero_ce_counted_fwd", logits, labels, lse, mean_cnt, rows, cols, ld, dtype, inv_temp)) return rc;
  HERO_REQUIRE(rows == 0 || loss, "hero_ce_counted_fwd: loss required");
  const CeCounted a = {logits, labels, count, loss, lse, mean_cnt, nullptr, nullptr, rows, cols, ld, inv_temp, ignore_index};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows > 0) with_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(ce_counted_fwd_kernel<typename decltype(tag)::type>, dim3(rows), dim3(256), 0, s, a); });
  hipLaunchKernelGGL(ce_counted_fold_kernel, dim3(1), dim3(256), 0, s, a);    // rows == 0: the pair is (0, 0)
  return check_launch("hero_ce_counted_fwd");
}

extern "C" int hero_ce_counted_bwd(const void* logits, const long long* labels, const int32_t* count, const float* lse, const float* dloss,
                                   const float* mean_cnt, void* dlogits, int rows, int cols, int ld, int dtype, float inv_temp,
                                   long long ignore_index, hero_stream_t stream) {
  if (const int rc = check_counted("hero_ce_counted_bwd", logits, labels, lse, mean_cnt, rows, cols, ld, dtype, inv_temp)) return rc;
  if (rows == 0) return HERO_OK;
  HERO_REQUIRE(dloss && dlogits && (((uintptr_t)dlogits) & 15) == 0, "hero_ce_counted_bwd: dloss / dlogits required (16-byte aligned)");
  const CeCounted a = {logits, labels, count, nullptr, const_cast<float*>(lse), const_cast<float*>(mean_cnt), dloss, dlogits, rows, cols, ld,
                       inv_temp, ignore_index};
  return by_dtype(dtype, "hero_ce_counted_bwd", [&](auto tag) {
    hipLaunchKernelGGL(ce_counted_bwd_kernel<typename decltype(tag)::type>, dim3(rows), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  });
}

static int check_smooth(const char* what, const void* logits, const long long* labels, const float* lse, int rows, int cols, int ld, int dtype,
                        double eps) {
  HERO_REQUIRE(logits && labels && lse, "%s: null pointer", what);
  if (const int rc = check_shape(what, rows, cols, ld, 2, dtype)) return rc;
  HERO_REQUIRE(eps > 0.0 && eps <= 1.0, "%s: smoothing must be in (0, 1], got %g", what, eps);
  HERO_REQUIRE((((uintptr_t)logits) & 15) == 0, "%s: logits must be 16-byte aligned", what);
  return HERO_OK;
}

static void smooth_consts(SmoothCe& a, double eps) {
  const double C = a.cols, e = eps, s = e / (C - 1.0), conf = 1.0 - e;
  a.s = s;
  a.cms = conf - s;
  a.h0 = (conf > 0.0 ? conf * log(conf) : 0.0) + (C - 1.0) * s * log(s);
}

extern "C" int hero_smooth_ce_fwd(const void* logits, const long long* labels, float* loss, float* lse, float* sum_cnt, int rows, int cols,
                                  int ld, int dtype, double eps, long long ignore_index, hero_stream_t stream) {
  if (const int rc = check_smooth("hero_smooth_ce_fwd", logits, labels, lse, rows, cols, ld, dtype, eps)) return rc;
  HERO_REQUIRE(loss && sum_cnt, "hero_smooth_ce_fwd: loss and sum_cnt required");
  SmoothCe a = {logits, labels, loss, lse, sum_cnt, nullptr, nullptr, nullptr, nullptr, rows, cols, ld, ignore_index, 0.0, 0.0, 0.0};
  smooth_consts(a, eps);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (rows > 0) with_dtype(dtype, [&](auto tag) { hipLaunchKernelGGL(smooth_ce_fwd_kernel<typename decltype(tag)::type>, dim3(rows), dim3(256), 0, s, a); });
  hipLaunchKernelGGL(smooth_ce_fold_kernel, dim3(1), dim3(256), 0, s, a);     // rows == 0: the pair is (0, 0)
  return check_launch("hero_smooth_ce_fwd");
}

extern "C" int hero_smooth_ce_bwd(const void* logits, const long long* labels, const float* lse, const float* dloss, const float* dloss_rows,
                                  const float* mean_cnt, void* dlogits, int rows, int cols, int ld, int dtype, double eps,
                                  long long ignore_index, hero_stream_t stream) {
  if (const int rc = check_smooth("hero_smooth_ce_bwd", logits, labels, lse, rows, cols, ld, dtype, eps)) return rc;
  HERO_REQUIRE(dloss && dlogits && (((uintptr_t)dlogits) & 15) == 0, "hero_smooth_ce_bwd: dloss / dlogits required (16-byte aligned)");
  if (rows == 0) return HERO_OK;
  SmoothCe a = {logits, labels, nullptr, const_cast<float*>(lse), nullptr, dloss, dloss_rows, mean_cnt, dlogits, rows, cols, ld, ignore_index,
                0.0, 0.0, 0.0};
  smooth_consts(a, eps);
  return by_dtype(dtype, "hero_smooth_ce_bwd", [&](auto tag) {
    hipLaunchKernelGGL(smooth_ce_bwd_kernel<typename decltype(tag)::type>, dim3(rows), dim3(256), 0, static_cast<hipStream_t>(stream), a);
  });
}
