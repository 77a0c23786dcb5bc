// The per-channel row-streaming skeleton (bn.hip, layer_scale.hip, se.hip, relu_mask_reduce in unit3.hip, bilinear_sum_stats in
// neck_resample.hip): a [rows][ld] bf16 matrix, CGE = min(C/8, 256) channel groups across the 256-thread block, RPB = 256 / CGE
// rows per block iteration; a lane keeps ONE 8-channel group (16 bytes of bf16) for a whole pass over its rows, so its
// per-channel coefficients live in registers.  A kernel is a `setup` lambda: setup(cg) loads the lane's coefficients of channel
// group cg and returns the per-row body (TOK_ROW_INLINE behind both parameter lists).  Everything is force-inlined: no call
// and no dispatch inside the row loop.
#pragma once
#include "tok_common.h"

struct Geo {
  int cg_total, cge, rpb;
};
inline Geo make_geo(int c) {
  Geo g;
  g.cg_total = c / 8;
  g.cge = g.cg_total < 256 ? g.cg_total : 256;
  g.rpb = 256 / g.cge;
  return g;
}
// blocks of a pass over m rows: one block iteration each, at most `cap`
inline int row_blocks(int64_t m, const Geo& g, int cap) {
  int64_t b = (m + g.rpb - 1) / g.rpb;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}
// Block caps of the BatchNorm passes (bn.hip, bn_droppath.hip).  Map passes: TOK_BN_BLOCKS overrides; 1024 = 4 per CU = half the
// wave slots: the weight-gradient kernels of the side stream run beside them (2048 measured 1.7 % slower end to end)
inline int row_stream_cap() {
  static const int v = tok_env_int("TOK_BN_BLOCKS", 1024);
  return v;
}
constexpr int kRowReduceCap = 1024;   // partial rows of the reducing kernels (tok_bn_bwd_rows)
// The completion event armed by tok_next_launch_event for the calling thread's next apply launch, disarmed by the read (bn.hip)
hipEvent_t tok_take_launch_event();

// the lane's 8 per-channel fp32 coefficients
__device__ __forceinline__ void load8f(const float* p, float (&v)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  const float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// The rows a block walks: row lane rl takes first + rl, first + rl + step, ... below end.
struct RowSpan {
  int64_t first, end, step;
};
// the whole matrix, grid-strided: what every kernel but se_sum_kernel walks
__device__ __forceinline__ RowSpan grid_rows(int64_t M, int rpb) {
  return {(int64_t)blockIdx.x * rpb, M, (int64_t)gridDim.x * rpb};
}

// Map pass: row(m, off) for every row m of the span and every channel group of the lane, off = m * ld + cg * 8.
template <class Setup>
__device__ __forceinline__ void rows_map(RowSpan rows, int C, int ld, int cge, int rpb, Setup&& setup) {
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  if (rl >= rpb) return;
  const int cg_total = C >> 3;
  for (int cg = cgl; cg < cg_total; cg += cge) {
    auto row = setup(cg);
    for (int64_t m = rows.first + rl; m < rows.end; m += rows.step) row(m, (size_t)m * ld + cg * 8);
  }
}

// Reduce pass: row(m, off, s) accumulates the lane's NS sums of 8 channels, then the block folds them into
// partial[k][prow][C], k < NS, the buffer holding `prows` rows per sum.  Fold order, which every consumer's bits depend on: a
// lane adds its rows in stride order, then row lane 0 adds the row lanes r = 1 .. rpb-1 in order.  No atomics.
// The barriers sit inside the channel-group loop, so its trip count is block-uniform (cg_end) and a lane past the last group
// idles through it (`live`): any C % 8 == 0 is well defined, also C > 2048 with a ragged last pass.
// partial == nullptr skips the fold (block-uniform): a map pass that reduces only on request.
template <int NS, class Setup>
__device__ __forceinline__ void rows_reduce(RowSpan rows, int C, int ld, int cge, int rpb, float* __restrict__ partial,
                                            size_t prow, size_t prows, Setup&& setup) {
  __shared__ float red[NS][256][8];
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  const int cg_total = C >> 3;
  const int cg_end = (cg_total + cge - 1) / cge * cge;
  for (int cg = cgl; cg < cg_end; cg += cge) {
    const bool live = cg < cg_total;
    float s[NS][8];
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) s[k][e] = 0.f;
    if (rl < rpb && live) {
      auto row = setup(cg);
      for (int64_t m = rows.first + rl; m < rows.end; m += rows.step) row(m, (size_t)m * ld + cg * 8, s);
    }
    if (partial == nullptr) continue;
#pragma unroll
    for (int k = 0; k < NS; ++k)
#pragma unroll
      for (int e = 0; e < 8; ++e) red[k][tid][e] = s[k][e];
    __syncthreads();
    if (rl == 0 && live) {
      for (int r = 1; r < rpb; ++r)
#pragma unroll
        for (int k = 0; k < NS; ++k)
#pragma unroll
          for (int e = 0; e < 8; ++e) s[k][e] += red[k][r * cge + cgl][e];
#pragma unroll
      for (int k = 0; k < NS; ++k)
#pragma unroll
        for (int e = 0; e < 8; ++e) partial[((size_t)k * prows + prow) * C + cg * 8 + e] = s[k][e];
    }
    __syncthreads();
  }
}
