// Element-wise losses on bf16 predictions and fp32 targets, fp32 math, mean or sum through a two-stage fp64 fold in the order
// loss_common.h describes (8192 elements per part): BCE-with-logits with an ignore value, and the L1 / MSE / smooth-L1 / Huber
// family.  Stage 1: one contiguous chunk of the element range per block -> (sum, count) doubles; stage 2 folds them in fixed order.
#include "loss_common.h"
#include <stdlib.h>
#include <math.h>

namespace {
// BCEWithLogitsLoss with an ignore value (losses/classification/binary_cross_entropy.py:50-59): elements whose target
// equals `ignore` are dropped, the rest take  (1 - t) x - log_sigmoid(x)  in fp32 (ATen's formula), mean or sum.
// Element e lives at logits[(e / classes) * ld + e % classes].
__device__ __forceinline__ float bce_elem(float x, float t) {
  const float ls = fminf(x, 0.f) - log1pf(expf(-fabsf(x)));   // log_sigmoid(x)
  return (1.f - t) * x - ls;
}

__global__ __launch_bounds__(256) void bce_partial_kernel(const bf16* __restrict__ logits, const float* __restrict__ target,
                                                          int64_t n, int classes, int ld, float ignore, int64_t chunk,
                                                          double* __restrict__ part) {
  const int64_t e0 = (int64_t)blockIdx.x * chunk;
  const int64_t e1 = e0 + chunk < n ? e0 + chunk : n;
  double s = 0.0, cnt = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) {
    const float t = target[e];
    if (t != ignore) {
      const int64_t r = e / classes;
      const int c = (int)(e - r * classes);
      s += (double)bce_elem(bf2f(logits[r * ld + c]), t);
      cnt += 1.0;
    }
  }
  block_reduce2(s, cnt);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = cnt; }
}

// stage 2 of both families
__global__ __launch_bounds__(256) void bce_final_kernel(const double* __restrict__ part, int nparts, int mean, float* loss) {
  double s = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) { s += part[2 * i]; cnt += part[2 * i + 1]; }
  block_reduce2(s, cnt);
  if (threadIdx.x == 0) {
    // nothing selected: the reference returns a zero (binary_cross_entropy.py:58-59), not 0/0
    loss[0] = cnt > 0.0 ? (float)(mean ? s / cnt : s) : 0.f;
    loss[1] = (float)cnt;
  }
}

// d loss / d x = (sigmoid(x) - t) * gscale / (mean ? n_valid : 1) on the selected elements, 0 elsewhere and in the pad
__global__ __launch_bounds__(256) void bce_bwd_kernel(const bf16* __restrict__ logits, const float* __restrict__ target,
                                                      const float* __restrict__ loss, const float* __restrict__ gscale,
                                                      int64_t rows, int classes, int ld, float ignore, int mean,
                                                      bf16* __restrict__ dlogits) {
  const float nv = loss[1];
  const float g = gscale[0] * (mean ? (nv > 0.f ? 1.f / nv : 0.f) : 1.f);
  const int64_t total = rows * ld;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t r = i / ld;
    const int c = (int)(i - r * ld);
    float d = 0.f;
    if (c < classes) {
      const float t = target[r * classes + c];
      if (t != ignore) {
        const float x = bf2f(logits[i]);
        d = (1.f / (1.f + expf(-x)) - t) * g;
      }
    }
    dlogits[i] = f2bf(d);
  }
}

// torch.nn.L1Loss / MSELoss / SmoothL1Loss(beta) / HuberLoss(delta) (registered at losses/__init__.py:13-25) on a flat bf16
// prediction and fp32 target: kind 0 |d|, 1 d^2, 2 smooth-L1, 3 Huber; d = x - t.
__device__ __forceinline__ float reg_elem(int kind, float d, float k) {
  const float a = fabsf(d);
  if (kind == 0) return a;
  if (kind == 1) return d * d;
  if (kind == 2) return a < k ? 0.5f * d * d / k : a - 0.5f * k;
  return a <= k ? 0.5f * d * d : k * (a - 0.5f * k);
}
__device__ __forceinline__ float reg_grad(int kind, float d, float k) {
  const float a = fabsf(d), sg = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  if (kind == 0) return sg;
  if (kind == 1) return 2.f * d;
  if (kind == 2) return a < k ? d / k : sg;
  return a <= k ? d : k * sg;
}

__global__ __launch_bounds__(256) void reg_partial_kernel(const bf16* __restrict__ x, const float* __restrict__ t, int64_t n,
                                                          int kind, float k, int64_t chunk, double* __restrict__ part) {
  const int64_t e0 = (int64_t)blockIdx.x * chunk;
  const int64_t e1 = e0 + chunk < n ? e0 + chunk : n;
  double s = 0.0, cnt = 0.0;
  for (int64_t e = e0 + threadIdx.x; e < e1; e += 256) { s += (double)reg_elem(kind, bf2f(x[e]) - t[e], k); cnt += 1.0; }
  block_reduce2(s, cnt);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = cnt; }
}

__global__ __launch_bounds__(256) void reg_bwd_kernel(const bf16* __restrict__ x, const float* __restrict__ t,
                                                      const float* __restrict__ gscale, int64_t n, int kind, float k,
                                                      float scale, bf16* __restrict__ dx) {
  const float g = gscale[0] * scale;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    dx[i] = f2bf(reg_grad(kind, bf2f(x[i]) - t[i], k) * g);
}
}  // namespace

extern "C" int tok_bce_logits_fwd(const void* logits, const float* target, int64_t rows, int classes, int ld,
                                  float ignore_value, int mean, float* loss, void* stream) {
  TOK_CHECK_ARG(logits && target && loss, "tok_bce_logits_fwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && classes > 0 && ld >= classes, "tok_bce_logits_fwd: bad sizes");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(loss) & 7) == 0, "tok_bce_logits_fwd: loss must be 8-byte aligned");
  hipStream_t st = tok_stream(stream);
  double* part = reinterpret_cast<double*>(loss + 2);   // loss holds TOK_CE_LOSS_FLOATS floats
  const int64_t n = rows * classes;
  const int nparts = fold_parts(n, 8192);
  const int64_t chunk = (n + nparts - 1) / nparts;
  hipLaunchKernelGGL(bce_partial_kernel, dim3(nparts), dim3(256), 0, st, (const bf16*)logits, target, n, classes, ld,
                     ignore_value, chunk, part);
  TOK_CHECK_LAUNCH("tok_bce_logits_fwd(partial)");
  hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, st, part, nparts, mean, loss);
  TOK_CHECK_LAUNCH("tok_bce_logits_fwd(final)");
  return TOK_OK;
}

extern "C" int tok_bce_logits_bwd(const void* logits, const float* target, const float* loss, const float* gscale,
                                  int64_t rows, int classes, int ld, float ignore_value, int mean, void* dlogits,
                                  void* stream) {
  TOK_CHECK_ARG(logits && target && loss && gscale && dlogits, "tok_bce_logits_bwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && classes > 0 && ld >= classes, "tok_bce_logits_bwd: bad sizes");
  const int64_t total = rows * ld;
  const int blocks = (int)(tok_cdiv(total, (int64_t)256) < 4096 ? tok_cdiv(total, (int64_t)256) : 4096);
  hipLaunchKernelGGL(bce_bwd_kernel, dim3(blocks), dim3(256), 0, tok_stream(stream), (const bf16*)logits, target, loss,
                     gscale, rows, classes, ld, ignore_value, mean, (bf16*)dlogits);
  TOK_CHECK_LAUNCH("tok_bce_logits_bwd");
  return TOK_OK;
}

extern "C" int tok_regression_loss_fwd(const void* x, const float* target, int64_t n, int kind, float knee, int mean,
                                       float* loss, void* stream) {
  TOK_CHECK_ARG(x && target && loss && n > 0 && kind >= 0 && kind <= 3, "tok_regression_loss_fwd: bad args");
  TOK_CHECK_ARG(kind < 2 || knee > 0.f, "tok_regression_loss_fwd: beta / delta must be positive");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(loss) & 7) == 0, "tok_regression_loss_fwd: loss must be 8-byte aligned");
  hipStream_t st = tok_stream(stream);
  double* part = reinterpret_cast<double*>(loss + 2);   // loss holds TOK_CE_LOSS_FLOATS floats
  const int nparts = fold_parts(n, 8192);
  const int64_t chunk = (n + nparts - 1) / nparts;
  hipLaunchKernelGGL(reg_partial_kernel, dim3(nparts), dim3(256), 0, st, (const bf16*)x, target, n, kind, knee, chunk, part);
  TOK_CHECK_LAUNCH("tok_regression_loss_fwd(partial)");
  hipLaunchKernelGGL(bce_final_kernel, dim3(1), dim3(256), 0, st, part, nparts, mean, loss);
  TOK_CHECK_LAUNCH("tok_regression_loss_fwd(final)");
  return TOK_OK;
}

extern "C" int tok_regression_loss_bwd(const void* x, const float* target, const float* gscale, int64_t n, int kind,
                                       float knee, int mean, void* dx, void* stream) {
  TOK_CHECK_ARG(x && target && gscale && dx && n > 0 && kind >= 0 && kind <= 3, "tok_regression_loss_bwd: bad args");
  const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(reg_bwd_kernel, dim3(blocks), dim3(256), 0, tok_stream(stream), (const bf16*)x, target, gscale, n,
                     kind, knee, mean ? 1.f / (float)n : 1.f, (bf16*)dx);
  TOK_CHECK_LAUNCH("tok_regression_loss_bwd");
  return TOK_OK;
}
