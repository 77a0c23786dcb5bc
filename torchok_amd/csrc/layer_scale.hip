// LayerScale residual of BEiT ([timm 0.6.13] beit.Block): x + drop_path(gamma * f(x)) on bf16 token rows [rows][d], fp32 arithmetic.
//   forward : out = bf16(x + (s_b * gamma[c]) * a)        s_b = row_scale[row / rows_per_sample] (1 without drop-path scales)
//   backward: da (=|+=) bf16((s_b * gamma[c]) * dout);  partial[block][c] = sum over the block's rows of s_b * dout * a, folded
//             by tok_colsum_f32 into dgamma (the tok_bn_bwd_reduce -> finalize pattern); dx = dout is the caller's (no pass).
// Geometry: make_geo (tok_common.h), min(d/8, 256) channel groups across the block, 8 channels (16 bytes) per lane, grid-stride over
// rows.  Fixed summation order, no atomics: two runs give the same bits.
#include "tok_common.h"

namespace {

constexpr int LS_BLOCKS = 512;     // block cap of both passes = partial rows of the backward

inline int blocks_for_rows(int64_t rows, int d) {
  const Geo g = make_geo(d);
  const int64_t b = (rows + g.rpb - 1) / g.rpb;
  return (int)(b < LS_BLOCKS ? b : LS_BLOCKS);
}

__global__ __launch_bounds__(256) void layer_scale_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ a,
                                                              const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                              int rps, bf16* __restrict__ out, int64_t M, int D, int cge, int rpb) {
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  if (rl >= rpb) return;
  const int cg_total = D >> 3;
  for (int cg = cgl; cg < cg_total; cg += cge) {
    float gm[8];
    load8f(gamma + cg * 8, gm);
    for (int64_t m = (int64_t)blockIdx.x * rpb + rl; m < M; m += (int64_t)gridDim.x * rpb) {
      const size_t off = (size_t)m * D + cg * 8;
      const float s = row_scale ? row_scale[m / rps] : 1.f;
      const bf16x8 xv = ldg16(x + off), av = ldg16(a + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(s * gm[e], bf2f(av[e]), bf2f(xv[e])));
      stg16(out + off, o);
    }
  }
}

__global__ __launch_bounds__(256) void layer_scale_bwd_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ a,
                                                              const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                              int rps, bf16* __restrict__ da, int da_acc,
                                                              float* __restrict__ partial, int64_t M, int D, int cge, int rpb) {
  __shared__ float red[256][8];
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  const int cg_total = D >> 3;
  for (int cg0 = 0; cg0 < cg_total; cg0 += cge) {      // block-uniform trip count: every lane reaches both barriers
    const int cg = cg0 + cgl;
    float s1[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] = 0.f;
    if (rl < rpb && cg < cg_total) {
      float gm[8];
      load8f(gamma + cg * 8, gm);
      for (int64_t m = (int64_t)blockIdx.x * rpb + rl; m < M; m += (int64_t)gridDim.x * rpb) {
        const size_t off = (size_t)m * D + cg * 8;
        const float s = row_scale ? row_scale[m / rps] : 1.f;
        const bf16x8 g = ldg16(dout + off);
        if (partial) {
          const bf16x8 av = ldg16(a + off);
#pragma unroll
          for (int e = 0; e < 8; ++e) s1[e] = fmaf(s * bf2f(g[e]), bf2f(av[e]), s1[e]);
        }
        if (da) {
          bf16x8 o;
          if (da_acc) {
            const bf16x8 cur = ldg16(da + off);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(s * gm[e], bf2f(g[e]), bf2f(cur[e])));
          } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = f2bf((s * gm[e]) * bf2f(g[e]));
          }
          stg16(da + off, o);
        }
      }
    }
    if (!partial) continue;                             // block-uniform
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid][e] = s1[e];
    __syncthreads();
    if (rl == 0 && cg < cg_total) {
      for (int r = 1; r < rpb; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) s1[e] += red[r * cge + cgl][e];
#pragma unroll
      for (int e = 0; e < 8; ++e) partial[(size_t)blockIdx.x * D + cg * 8 + e] = s1[e];
    }
    __syncthreads();
  }
}

}  // namespace

extern "C" int tok_layer_scale_bwd_rows(int64_t rows, int d) {
  if (rows <= 0 || d <= 0 || d % 8) return 0;
  return blocks_for_rows(rows, d);
}

extern "C" int tok_layer_scale_fwd(const void* x, const void* a, const float* gamma, const float* row_scale,
                                   int rows_per_sample, void* out, int64_t rows, int d, void* stream) {
  TOK_CHECK_ARG(x && a && gamma && out, "tok_layer_scale_fwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && d > 0 && d % 8 == 0 && (!row_scale || rows_per_sample > 0), "tok_layer_scale_fwd: bad sizes");
  const Geo g = make_geo(d);
  hipLaunchKernelGGL(layer_scale_fwd_kernel, dim3(blocks_for_rows(rows, d)), dim3(256), 0, tok_stream(stream), (const bf16*)x,
                     (const bf16*)a, gamma, row_scale, row_scale ? rows_per_sample : 1, (bf16*)out, rows, d, g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_layer_scale_fwd");
  return TOK_OK;
}

extern "C" int tok_layer_scale_bwd(const void* dout, const void* a, const float* gamma, const float* row_scale,
                                   int rows_per_sample, void* da, int da_accumulate, float* dgamma, int dgamma_accumulate,
                                   float* partial, int64_t rows, int d, void* stream) {
  TOK_CHECK_ARG(dout && gamma && (da || dgamma) && (!dgamma || (a && partial)), "tok_layer_scale_bwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && d > 0 && d % 8 == 0 && (!row_scale || rows_per_sample > 0), "tok_layer_scale_bwd: bad sizes");
  const Geo g = make_geo(d);
  const int blocks = blocks_for_rows(rows, d);
  hipLaunchKernelGGL(layer_scale_bwd_kernel, dim3(blocks), dim3(256), 0, tok_stream(stream), (const bf16*)dout, (const bf16*)a,
                     gamma, row_scale, row_scale ? rows_per_sample : 1, (bf16*)da, da_accumulate ? 1 : 0,
                     dgamma ? partial : (float*)nullptr, rows, d, g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_layer_scale_bwd");
  if (!dgamma) return TOK_OK;
  return tok_colsum_f32(partial, blocks, d, dgamma, dgamma_accumulate, stream);
}
