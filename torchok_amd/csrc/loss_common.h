// Shared pieces of the loss kernels (loss_ce.hip, loss_upsample_ce.hip, loss_pointwise.hip): the row validity predicate of the
// cross entropies, the block fold of a (sum, count) pair and the deterministic two-stage fp64 mean over the valid rows.
//
// The fold's SUMMATION ORDER is a contract (the loss scalar's bits follow from it), here and in loss_pointwise.hip: up to
// CE_PARTS blocks each take one contiguous chunk [e0, e1); element e goes to thread (e - e0) % 256, which adds its elements in
// stride order; the 256 threads go through the 128 ... 1 tree of block_reduce2 into the (sum, count) double pair of the part,
// kept in the caller's loss buffer behind the two result floats; then ONE block gives part i to thread i % 256 and folds
// through the same tree.
#pragma once
#include "tok_common.h"

namespace {

// ONE validity predicate for forward, mean denominator and backward: a row counts iff its label is a class index and is not
// `ignore_index`.  (torch raises on labels outside [0, classes) that are not ignore_index; a device-side raise would need a
// host sync per step, so such rows are dropped — consistently: zero loss, not counted in the mean, zero gradient.  The
// Python wrapper validates the labels on the host under TOK_CHECK_TARGETS=1.)
__device__ __forceinline__ bool ce_row_valid(int64_t t, int64_t ignore_index, int classes) {
  return t != ignore_index && t >= 0 && t < (int64_t)classes;
}

constexpr int CE_PARTS = (TOK_CE_LOSS_FLOATS - 2) / 4;   // (sum, count) doubles

__device__ __forceinline__ void block_reduce2(double& s, double& c) {
  __shared__ double rs[256];
  __shared__ double rc[256];
  rs[threadIdx.x] = s;
  rc[threadIdx.x] = c;
  __syncthreads();
  for (int k = 128; k > 0; k >>= 1) {
    if (threadIdx.x < k) { rs[threadIdx.x] += rs[threadIdx.x + k]; rc[threadIdx.x] += rc[threadIdx.x + k]; }
    __syncthreads();
  }
  s = rs[0];
  c = rc[0];
}

// parts of a two-stage fold over n elements, `per_part` elements each, at most CE_PARTS
inline int fold_parts(int64_t n, int per_part) {
  const int64_t want = (n + per_part - 1) / per_part;
  return (int)(want < CE_PARTS ? want : CE_PARTS);
}

__global__ __launch_bounds__(256) void ce_partial_kernel(const float* __restrict__ row_loss,
                                                         const int64_t* __restrict__ target, int rows,
                                                         int64_t ignore_index, int classes, int chunk,
                                                         double* __restrict__ part) {
  const int r0 = blockIdx.x * chunk;
  const int r1 = min(rows, r0 + chunk);
  double s = 0.0, cnt = 0.0;
  for (int r = r0 + threadIdx.x; r < r1; r += 256) {
    if (ce_row_valid(target[r], ignore_index, classes)) { s += (double)row_loss[r]; cnt += 1.0; }
  }
  block_reduce2(s, cnt);
  if (threadIdx.x == 0) { part[2 * blockIdx.x] = s; part[2 * blockIdx.x + 1] = cnt; }
}

__global__ __launch_bounds__(256) void ce_mean_kernel(const double* __restrict__ part, int nparts, float* loss) {
  double s = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < nparts; i += 256) { s += part[2 * i]; cnt += part[2 * i + 1]; }
  block_reduce2(s, cnt);
  if (threadIdx.x == 0) {
    loss[0] = (float)(s / cnt);  // 0/0 = nan, as torch
    loss[1] = (float)cnt;
  }
}

// loss[0] = mean of row_loss over the valid rows, loss[1] = their count; 4096 rows per part, the parts in loss[2 ...]
// (loss holds TOK_CE_LOSS_FLOATS floats, 8-byte aligned).  The tail of tok_softmax_ce_fwd and tok_upsample_ce_fwd (`who`).
inline int ce_mean_launch(const char* who, const float* row_loss, const int64_t* target, int rows, int64_t ignore_index, int classes,
                          float* loss, hipStream_t st) {
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(loss) & 7) == 0, "%s: loss must be 8-byte aligned", who);
  double* part = reinterpret_cast<double*>(loss + 2);
  const int nparts = fold_parts(rows, 4096);
  hipLaunchKernelGGL(ce_partial_kernel, dim3(nparts), dim3(256), 0, st, row_loss, target, rows, ignore_index, classes,
                     tok_cdiv(rows, nparts), part);
  TOK_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(ce_mean_kernel, dim3(1), dim3(256), 0, st, part, nparts, loss);
  TOK_CHECK_LAUNCH(who);
  return TOK_OK;
}

}  // namespace
