// Fused softmax cross-entropy (mean reduction, ignore_index, label smoothing), bf16 logits, fp32 math.
// One wavefront per row: lane-strided max / sum-exp with 64-lane butterflies, no LDS; one THREAD per row for few classes and
// many rows.  The mean is the two-stage fp64 fold of loss_common.h.
#include "loss_common.h"
#include <stdlib.h>
#include <math.h>

namespace {

__global__ __launch_bounds__(256) void ce_fwd_kernel(const bf16* __restrict__ logits,
                                                     const int64_t* __restrict__ target, int rows,
                                                     int classes, int ld, int64_t ignore_index, float smooth,
                                                     float* __restrict__ lse, float* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16* z = logits + (size_t)row * ld;
  float mx = -INFINITY;
  for (int c = lane; c < classes; c += 64) mx = fmaxf(mx, bf2f(z[c]));
  mx = wave_max(mx);
  float s = 0.f, zs = 0.f;
  for (int c = lane; c < classes; c += 64) { const float v = bf2f(z[c]); s += expf(v - mx); zs += v; }
  s = wave_sum(s);
  const float l = mx + logf(s);
  if (smooth != 0.f) zs = wave_sum(zs);   // label smoothing: + smooth * mean_c(-log p_c) = smooth * (lse - mean_c z_c)
  if (lane == 0) {
    lse[row] = l;
    const int64_t t = target[row];
    float rl = 0.f;
    if (ce_row_valid(t, ignore_index, classes)) {
      rl = l - bf2f(z[t]);
      if (smooth != 0.f) rl = (1.f - smooth) * rl + smooth * (l - zs / (float)classes);
    }
    row_loss[row] = rl;
  }
}

// Few classes, many rows (segmentation logits: 4 M pixel rows x 19 classes): one THREAD per row, the row in
// registers through 16-byte loads (ld <= 64); a wavefront per row would leave most of its lanes idle.
__global__ __launch_bounds__(256) void ce_fwd_small_kernel(const bf16* __restrict__ logits,
                                                           const int64_t* __restrict__ target, int rows, int classes,
                                                           int ld, int64_t ignore_index, float smooth,
                                                           float* __restrict__ lse, float* __restrict__ row_loss) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const bf16* z = logits + (size_t)row * ld;
  const int nv = ld >> 3;
  float v[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < nv) {
      const bf16x8 q = ldg16(z + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i * 8 + e] = (i * 8 + e < classes) ? bf2f(q[e]) : -INFINITY;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[i * 8 + e] = -INFINITY;
    }
  }
  float mx = -INFINITY;
#pragma unroll
  for (int c = 0; c < 64; ++c) mx = fmaxf(mx, v[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 64; ++c) s += (c < classes) ? expf(v[c] - mx) : 0.f;
  const float l = mx + logf(s);
  lse[row] = l;
  const int64_t t = target[row];
  float rl = 0.f;
  if (ce_row_valid(t, ignore_index, classes)) {
    rl = l - bf2f(z[t]);
    if (smooth != 0.f) {
      float zs = 0.f;
#pragma unroll
      for (int c = 0; c < 64; ++c) zs += (c < classes) ? v[c] : 0.f;
      rl = (1.f - smooth) * rl + smooth * (l - zs / (float)classes);
    }
  }
  row_loss[row] = rl;
}

__global__ __launch_bounds__(256) void ce_bwd_small_kernel(const bf16* __restrict__ logits,
                                                           const int64_t* __restrict__ target,
                                                           const float* __restrict__ lse, const float* __restrict__ loss,
                                                           const float* __restrict__ gscale, int rows, int classes, int ld,
                                                           int64_t ignore_index, float smooth, bf16* __restrict__ dlogits) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int64_t t = target[row];
  const bool valid = ce_row_valid(t, ignore_index, classes);
  const float g = valid ? (gscale ? gscale[0] : 1.f) / loss[1] : 0.f;
  const float l = lse[row];
  const bf16* z = logits + (size_t)row * ld;
  bf16* d = dlogits + (size_t)row * ld;
  const int nv = ld >> 3;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    if (i < nv) {
      const bf16x8 q = ldg16(z + i * 8);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = i * 8 + e;
        float w = 0.f;
        if (valid && c < classes) w = (expf(bf2f(q[e]) - l) - (c == t ? 1.f - smooth : 0.f) - smooth / (float)classes) * g;
        o[e] = f2bf(w);
      }
      stg16(d + i * 8, o);
    }
  }
}

__global__ __launch_bounds__(256) void ce_bwd_kernel(const bf16* __restrict__ logits,
                                                     const int64_t* __restrict__ target,
                                                     const float* __restrict__ lse,
                                                     const float* __restrict__ loss,
                                                     const float* __restrict__ gscale, int rows, int classes,
                                                     int ld, int64_t ignore_index, float smooth,
                                                     bf16* __restrict__ dlogits) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t t = target[row];
  const bool valid = ce_row_valid(t, ignore_index, classes);
  const float g = valid ? (gscale ? gscale[0] : 1.f) / loss[1] : 0.f;
  const float l = lse[row];
  const bf16* z = logits + (size_t)row * ld;
  bf16* d = dlogits + (size_t)row * ld;
  for (int c = lane; c < ld; c += 64) {
    float v = 0.f;
    if (valid && c < classes) v = (expf(bf2f(z[c]) - l) - (c == t ? 1.f - smooth : 0.f) - smooth / (float)classes) * g;
    d[c] = f2bf(v);
  }
}

// thread-per-row kernels: rows of at most 64 bf16 in whole 16-byte vectors, enough rows to fill the chip
inline bool ce_small(const void* logits, int rows, int ld) {
  return ld <= 64 && (ld & 7) == 0 && rows >= 16384 && (reinterpret_cast<uintptr_t>(logits) & 15) == 0;
}

}  // namespace

extern "C" int tok_softmax_ce_smooth_fwd(const void* logits, const int64_t* target, int rows, int classes, int ld,
                                         int64_t ignore_index, float label_smoothing, float* lse, float* row_loss,
                                         float* loss, void* stream) {
  TOK_CHECK_ARG(logits && target && lse && row_loss && loss, "tok_softmax_ce_fwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && classes > 0 && ld >= classes, "tok_softmax_ce_fwd: bad sizes");
  TOK_CHECK_ARG(label_smoothing >= 0.f && label_smoothing <= 1.f, "tok_softmax_ce_fwd: label_smoothing outside [0, 1]");
  hipStream_t st = tok_stream(stream);
  if (ce_small(logits, rows, ld))
    hipLaunchKernelGGL(ce_fwd_small_kernel, dim3((rows + 255) / 256), dim3(256), 0, st, (const bf16*)logits, target, rows,
                       classes, ld, ignore_index, label_smoothing, lse, row_loss);
  else
    hipLaunchKernelGGL(ce_fwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, st, (const bf16*)logits, target, rows,
                       classes, ld, ignore_index, label_smoothing, lse, row_loss);
  TOK_CHECK_LAUNCH("tok_softmax_ce_fwd");
  return ce_mean_launch("tok_softmax_ce_fwd", row_loss, target, rows, ignore_index, classes, loss, st);
}

extern "C" int tok_softmax_ce_fwd(const void* logits, const int64_t* target, int rows, int classes, int ld,
                                  int64_t ignore_index, float* lse, float* row_loss, float* loss, void* stream) {
  return tok_softmax_ce_smooth_fwd(logits, target, rows, classes, ld, ignore_index, 0.f, lse, row_loss, loss, stream);
}

extern "C" int tok_softmax_ce_smooth_bwd(const void* logits, const int64_t* target, const float* lse,
                                         const float* loss, const float* gscale, int rows, int classes, int ld,
                                         int64_t ignore_index, float label_smoothing, void* dlogits, void* stream) {
  TOK_CHECK_ARG(logits && target && lse && loss && dlogits, "tok_softmax_ce_bwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && classes > 0 && ld >= classes, "tok_softmax_ce_bwd: bad sizes");
  if (ce_small(logits, rows, ld) && (reinterpret_cast<uintptr_t>(dlogits) & 15) == 0)
    hipLaunchKernelGGL(ce_bwd_small_kernel, dim3((rows + 255) / 256), dim3(256), 0, tok_stream(stream),
                       (const bf16*)logits, target, lse, loss, gscale, rows, classes, ld, ignore_index, label_smoothing,
                       (bf16*)dlogits);
  else
    hipLaunchKernelGGL(ce_bwd_kernel, dim3((rows + 3) / 4), dim3(256), 0, tok_stream(stream),
                       (const bf16*)logits, target, lse, loss, gscale, rows, classes, ld, ignore_index, label_smoothing,
                       (bf16*)dlogits);
  TOK_CHECK_LAUNCH("tok_softmax_ce_bwd");
  return TOK_OK;
}

extern "C" int tok_softmax_ce_bwd(const void* logits, const int64_t* target, const float* lse,
                                  const float* loss, const float* gscale, int rows, int classes, int ld,
                                  int64_t ignore_index, void* dlogits, void* stream) {
  return tok_softmax_ce_smooth_bwd(logits, target, lse, loss, gscale, rows, classes, ld, ignore_index, 0.f, dlogits, stream);
}
