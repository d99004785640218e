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

// (max, sum exp(x - max)) pairs combine associatively
__device__ __forceinline__ void ms_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = s * __expf(m - mx) + s2 * __expf(m2 - mx);
  m = mx;
}

// One row, the whole 256-thread workgroup: thread 0 writes lse and the loss.  The one statement of the row arithmetic -
// ce_fwd_kernel and ce_counted_fwd_kernel both call it, so their bits agree by construction.
template <typename T>
__device__ __forceinline__ void ce_row_fwd(const T* x, long long y, int cols, int ld, float t, long long ignore_index, float* lse_out,
                                           float* loss_out, float (&sm)[4], float (&ss)[4]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float m = -3.0e38f, s = 0.f;
  const int vec_end = ((ld & 7) == 0) ? (cols & ~7) : 0;              // 16-byte loads need aligned rows
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float v[8];
    ld8<T>(x + c, v);
    float mx = v[0] * t;
#pragma unroll
    for (int k = 1; k < 8; ++k) mx = fmaxf(mx, v[k] * t);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) e += __expf(v[k] * t - mx);
    ms_merge(m, s, mx, e);
  }
  for (int c = vec_end + threadIdx.x; c < cols; c += 256) ms_merge(m, s, ld1<T>(x + c) * t, 1.f);
  // wave, then block
  const float wm = wave_max(m);
  s = wave_sum(s * __expf(m - wm));
  if (lane == 0) { sm[wave] = wm; ss[wave] = s; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) ms_merge(M, S, sm[w], ss[w]);
    const float lse = M + __logf(S);
    *lse_out = lse;
    *loss_out = (y == ignore_index || y < 0 || y >= cols) ? 0.f : lse - ld1<T>(x + y) * t;
  }
}

// One gradient row with upstream g (already times inv_temp); dx may alias x: a thread reads its columns before it writes them
template <typename T>
__device__ __forceinline__ void ce_row_bwd(const T* x, T* dx, long long y, int cols, int ld, float t, float lse, float g) {
  const int vec_end = ((ld & 7) == 0) ? (cols & ~7) : 0;
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float v[8];
    ld8<T>(x + c, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = (__expf(v[k] * t - lse) - ((long long)(c + k) == y ? 1.f : 0.f)) * g;
    st8<T>(dx + c, v);
  }
  for (int c = vec_end + threadIdx.x; c < ld; c += 256) {
    float v = 0.f;
    if (c < cols) v = (__expf(ld1<T>(x + c) * t - lse) - ((long long)c == y ? 1.f : 0.f)) * g;
    st1<T>(dx + c, v);                                               // padding columns get a zero gradient
  }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_kernel(HeroCrossEntropy a) {
  __shared__ float sm[4], ss[4];
  const int row = blockIdx.x;
  ce_row_fwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, a.labels[row], a.cols, a.ld, a.inv_temp, a.ignore_index, a.lse + row,
                a.loss + row, sm, ss);
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_kernel(HeroCrossEntropy a) {
  const int row = blockIdx.x;
  const long long y = a.labels[row];
  const bool live = !(y == a.ignore_index || y < 0 || y >= a.cols);
  const float t = a.inv_temp;
  ce_row_bwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, static_cast<T*>(a.dlogits) + (size_t)row * a.ld, y, a.cols, a.ld, t,
                a.lse[row], live ? a.dloss[row] * t : 0.f);
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
  __shared__ float sm[4], ss[4];
  const int row = blockIdx.x;
  if (row >= ce_live_rows(a)) {                                       // uniform over the workgroup
    if (threadIdx.x == 0) { a.loss[row] = 0.f; a.lse[row] = 0.f; }
    return;
  }
  ce_row_fwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, a.labels[row], a.cols, a.ld, a.inv_temp, a.ignore_index, a.lse + row,
                a.loss + row, sm, ss);
}

// thread i adds rows i, i + 256, ... in order, then a fixed tree (eval_fold_kernel's pattern); rows == 0 gives (0, 0)
__global__ __launch_bounds__(256) void ce_counted_fold_kernel(CeCounted a) {
  __shared__ double ps[2][256];
  const int n = ce_live_rows(a);
  double s = 0.0, c = 0.0;
  for (int r = threadIdx.x; r < n; r += 256) {
    const long long y = a.labels[r];
    if (!(y == a.ignore_index || y < 0 || y >= a.cols)) { s += (double)a.loss[r]; c += 1.0; }
  }
  ps[0][threadIdx.x] = s;
  ps[1][threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { ps[0][threadIdx.x] += ps[0][threadIdx.x + w]; ps[1][threadIdx.x] += ps[1][threadIdx.x + w]; }
    __syncthreads();
  }
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
    live = !(y == a.ignore_index || y < 0 || y >= a.cols);
  }
  if (!live) {                                                        // +0 over all ld columns, nothing read
    const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int vec_end = ((a.ld & 7) == 0) ? a.ld : 0;
    for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) st8<T>(dx + c, z);
    for (int c = vec_end + threadIdx.x; c < a.ld; c += 256) st1<T>(dx + c, 0.f);
    return;
  }
  const float t = a.inv_temp, g = a.dloss[0] / fmaxf(a.mean_cnt[1], 1.f);
  ce_row_bwd<T>(static_cast<const T*>(a.logits) + (size_t)row * a.ld, dx, y, a.cols, a.ld, t, a.lse[row], g * t);
}

// ---- label-smoothed loss of the captioning decoder (model/tvc.py:19-64) -------------------------
// KL(smoothed one-hot || softmax(x)) of a row with label t, C = cols, s = eps / (C - 1), conf = 1 - eps, in closed form:
//   loss = H0 - (conf - s) (x_t - lse) - s (sum_c x_c - C lse),   H0 = conf ln conf + (C - 1) s ln s   (0 ln 0 = 0)
//   dx_c = (softmax(x)_c - s - (conf - s) [c == t]) * upstream
// so no [rows, C] target matrix exists.  Forward: one pass over the row (online max / sum of exponentials as above, plus
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

// ms_merge with the accurate exponential: the loss is judged at a few 2^-24
__device__ __forceinline__ void ms_merge_acc(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  s = s * expf(m - mx) + s2 * expf(m2 - mx);
  m = mx;
}
__device__ __forceinline__ float sum8(const float (&v)[8]) { return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7])); }

template <typename T>
__global__ __launch_bounds__(256) void smooth_ce_fwd_kernel(SmoothCe a) {
  __shared__ float sm[4], ss[4], sx[4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* x = static_cast<const T*>(a.logits) + (size_t)row * a.ld;
  float m = -3.0e38f, s = 0.f, tot = 0.f;
  const int vec_end = ((a.ld & 7) == 0) ? (a.cols & ~7) : 0;
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float v[8];
    ld8<T>(x + c, v);
    float mx = v[0];
#pragma unroll
    for (int k = 1; k < 8; ++k) mx = fmaxf(mx, v[k]);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) e += expf(v[k] - mx);
    ms_merge_acc(m, s, mx, e);
    tot += sum8(v);
  }
  for (int c = vec_end + threadIdx.x; c < a.cols; c += 256) {
    const float v = ld1<T>(x + c);
    ms_merge_acc(m, s, v, 1.f);
    tot += v;
  }
  const float wm = wave_max(m);
  s = wave_sum(s * expf(m - wm));
  tot = wave_sum(tot);
  if (lane == 0) { sm[wave] = wm; ss[wave] = s; sx[wave] = tot; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) ms_merge_acc(M, S, sm[w], ss[w]);
    const float lse = M + logf(S);
    const long long y = a.labels[row];
    a.lse[row] = lse;
    float loss = 0.f;
    if (!(y == a.ignore_index || y < 0 || y >= a.cols)) {
      const double all = ((double)sx[0] + (double)sx[1]) + ((double)sx[2] + (double)sx[3]) - (double)a.cols * (double)lse;
      loss = (float)(a.h0 - a.cms * ((double)ld1<T>(x + y) - (double)lse) - a.s * all);
    }
    a.loss[row] = loss;
  }
}

// sum_cnt = (sum of the row losses, number of valid rows): one workgroup, strided partial sums, a fixed tree
__global__ __launch_bounds__(256) void smooth_ce_fold_kernel(SmoothCe a) {
  __shared__ float ps[256], pc[256];
  float s = 0.f, c = 0.f;
  for (int r = threadIdx.x; r < a.rows; r += 256) {
    const long long y = a.labels[r];
    if (!(y == a.ignore_index || y < 0 || y >= a.cols)) { s += a.loss[r]; c += 1.f; }
  }
  ps[threadIdx.x] = s;
  pc[threadIdx.x] = c;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) { ps[threadIdx.x] += ps[threadIdx.x + w]; pc[threadIdx.x] += pc[threadIdx.x + w]; }
    __syncthreads();
  }
  if (threadIdx.x == 0) { a.sum_cnt[0] = ps[0]; a.sum_cnt[1] = pc[0]; }
}

template <typename T>
__global__ __launch_bounds__(256) void smooth_ce_bwd_kernel(SmoothCe a) {
  const int row = blockIdx.x;
  const T* x = static_cast<const T*>(a.logits) + (size_t)row * a.ld;
  T* dx = static_cast<T*>(a.dlogits) + (size_t)row * a.ld;
  const long long y = a.labels[row];
  const bool live = !(y == a.ignore_index || y < 0 || y >= a.cols);
  const float lse = a.lse[row];
  float g = 0.f;
  if (live) {
    g = a.dloss[0];
    if (a.dloss_rows) g *= a.dloss_rows[row];
    if (a.mean_cnt) g /= fmaxf(a.mean_cnt[1], 1.f);
  }
  const float s = (float)a.s, cms = (float)a.cms;
  const int vec_end = ((a.ld & 7) == 0) ? (a.cols & ~7) : 0;
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float v[8];
    ld8<T>(x + c, v);
#pragma unroll
    for (int k = 0; k < 8; ++k) v[k] = live ? ((expf(v[k] - lse) - s) - ((long long)(c + k) == y ? cms : 0.f)) * g : 0.f;
    st8<T>(dx + c, v);
  }
  for (int c = vec_end + threadIdx.x; c < a.ld; c += 256) {
    float v = 0.f;
    if (live && c < a.cols) v = ((expf(ld1<T>(x + c) - lse) - s) - ((long long)c == y ? cms : 0.f)) * g;
    st1<T>(dx + c, v);                                               // padding columns get a zero gradient
  }
}

// ---- validation counters of the pre-training heads (pretrain.py:462-608) --------------------------------------------
// One pass over the raw logits gives what validate_mlm / validate_mfm_nce / validate_fom take from F.cross_entropy(sum) and
// scores.max(-1): the row loss (the arithmetic of ce_fwd_kernel, statement for statement) and the arg-max of the STORED
// values, lowest column first among equal maxima.  Row results go to a workspace; one workgroup folds them into float64
// counters in a fixed order (no atomics: two runs give the same bits).
template <typename T>
__global__ __launch_bounds__(256) void ce_eval_kernel(const T* logits, const long long* labels, int cols, int ld, float t, long long ignore_index,
                                                      float* row_loss, float* row_hit, float* row_valid, int32_t* pred) {
  __shared__ float sm[4], ss[4];
  __shared__ unsigned long long sb[4];
  const int row = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const T* x = logits + (size_t)row * ld;
  float m = -3.0e38f, s = 0.f;
  float bv = -INFINITY;                                               // a thread meets its columns in ascending order, so a
  int bi = 0x7fffffff;                                                // strict > keeps the first of equal values
  const int vec_end = ((ld & 7) == 0) ? (cols & ~7) : 0;
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float v[8];
    ld8<T>(x + c, v);
    float mx = v[0] * t;
#pragma unroll
    for (int k = 1; k < 8; ++k) mx = fmaxf(mx, v[k] * t);
    float e = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) e += __expf(v[k] * t - mx);
    ms_merge(m, s, mx, e);
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (v[k] > bv) { bv = v[k]; bi = c + k; }
  }
  for (int c = vec_end + threadIdx.x; c < cols; c += 256) {
    const float v = ld1<T>(x + c);
    ms_merge(m, s, v * t, 1.f);
    if (v > bv) { bv = v; bi = c; }
  }
  if (bi == 0x7fffffff) {                                             // nothing above -inf: the thread's first column, if it has one
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
  const float wm = wave_max(m);
  s = wave_sum(s * __expf(m - wm));
  if (lane == 0) { sm[wave] = wm; ss[wave] = s; sb[wave] = best; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float M = sm[0], S = ss[0];
    unsigned long long B = sb[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      ms_merge(M, S, sm[w], ss[w]);
      B = sb[w] > B ? sb[w] : B;
    }
    const float lse = M + __logf(S);
    const int p = (int)~(uint32_t)B;
    const long long y = labels[row];
    const bool live = !(y == ignore_index || y < 0 || y >= cols);
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
  const int vec_end = (((ld_p | ld_t) & 7) == 0) ? (cols & ~7) : 0;
  for (int c = threadIdx.x * 8; c < vec_end; c += 256 * 8) {
    float a[8], b[8];
    ld8<T>(p + c, a);
    ld8<T>(g + c, b);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float d = a[k] - b[k];
      dd += d * d; pg += a[k] * b[k]; pp += a[k] * a[k]; gg += b[k] * b[k];
    }
  }
  for (int c = vec_end + threadIdx.x; c < cols; c += 256) {
    const float a = ld1<T>(p + c), b = ld1<T>(g + c), d = a - b;
    dd += d * d; pg += a * b; pp += a * a; gg += b * b;
  }
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

// acc[0..2] += (sum a, sum b, sum c) in float64 (c == nullptr: the row count): one workgroup, thread i adds rows i, i + 256,
// ... in order, then a fixed tree
__global__ __launch_bounds__(256) void eval_fold_kernel(const float* a, const float* b, const float* c, int rows, double* acc) {
  __shared__ double ps[3][256];
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) {
    s0 += (double)a[r];
    s1 += (double)b[r];
    s2 += c ? (double)c[r] : 1.0;
  }
  ps[0][threadIdx.x] = s0; ps[1][threadIdx.x] = s1; ps[2][threadIdx.x] = s2;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) {
#pragma unroll
      for (int k = 0; k < 3; ++k) ps[k][threadIdx.x] += ps[k][threadIdx.x + w];
    }
    __syncthreads();
  }
  if (threadIdx.x < 3) acc[threadIdx.x] += ps[threadIdx.x][0];
}

}  // namespace
}  // namespace hero

using namespace hero;

extern "C" int hero_ce_eval(const void* logits, const long long* labels, int rows, int cols, int ld, int dtype, float inv_temp,
                            long long ignore_index, double* acc, int32_t* pred, void* workspace, hero_stream_t stream) {
  HERO_REQUIRE(rows >= 0 && cols > 0 && ld >= cols, "hero_ce_eval: bad dims rows=%d cols=%d ld=%d", rows, cols, ld);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "hero_ce_eval: bad dtype %d", dtype);
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
  HERO_REQUIRE(a->rows >= 0 && a->cols > 0 && a->ld >= a->cols, "hero_cross_entropy: bad dims rows=%d cols=%d ld=%d", a->rows, a->cols, a->ld);
  HERO_REQUIRE(a->dtype == HERO_F32 || a->dtype == HERO_BF16, "hero_cross_entropy: bad dtype %d", a->dtype);
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
  HERO_REQUIRE(rows >= 0 && cols > 0 && ld >= cols, "%s: bad dims rows=%d cols=%d ld=%d", what, rows, cols, ld);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
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
  if (rows > 0) {
    if (dtype == HERO_BF16) hipLaunchKernelGGL(ce_counted_fwd_kernel<bf16_t>, dim3(rows), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(ce_counted_fwd_kernel<float>, dim3(rows), dim3(256), 0, s, a);
  }
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
  HERO_REQUIRE(rows >= 0 && cols >= 2 && ld >= cols, "%s: bad dims rows=%d cols=%d ld=%d", what, rows, cols, ld);
  HERO_REQUIRE(dtype == HERO_F32 || dtype == HERO_BF16, "%s: bad dtype %d", what, dtype);
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
  if (rows > 0) {
    if (dtype == HERO_BF16) hipLaunchKernelGGL(smooth_ce_fwd_kernel<bf16_t>, dim3(rows), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(smooth_ce_fwd_kernel<float>, dim3(rows), dim3(256), 0, s, a);
  }
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
