// LayerScale residual of BEiT ([timm 0.6.13] beit.Block): x + drop_path(gamma * f(x)) on bf16 token rows [rows][d], fp32 arithmetic.
//   forward : out = bf16(x + (s_b * gamma[c]) * a)        s_b = row_scale[row / rows_per_sample] (1 without drop-path scales)
//   backward: da (=|+=) bf16((s_b * gamma[c]) * dout);  partial[block][c] = sum over the block's rows of s_b * dout * a, folded
//             by tok_colsum_f32 into dgamma (the tok_bn_bwd_reduce -> finalize pattern); dx = dout is the caller's (no pass).
// Geometry: the row skeleton of row_stream.h, min(d/8, 256) channel groups across the block, 8 channels (16 bytes) per lane,
// grid-stride over rows.  Fixed summation order, no atomics: two runs give the same bits.
#include "row_stream.h"

namespace {

constexpr int LS_BLOCKS = 512;     // block cap of both passes = partial rows of the backward

__global__ __launch_bounds__(256) void layer_scale_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ a,
                                                              const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                              int rps, bf16* __restrict__ out, int64_t M, int D, int cge, int rpb) {
  rows_map(grid_rows(M, rpb), D, D, cge, rpb, [&](int cg) TOK_ROW_INLINE {
    float gm[8];
    load8f(gamma + cg * 8, gm);
    return [=](int64_t m, size_t off) TOK_ROW_INLINE {
      const float s = row_scale ? row_scale[m / rps] : 1.f;
      const bf16x8 xv = ldg16(x + off), av = ldg16(a + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(s * gm[e], bf2f(av[e]), bf2f(xv[e])));
      stg16(out + off, o);
    };
  });
}

// partial == nullptr (no dgamma asked for): da only
__global__ __launch_bounds__(256) void layer_scale_bwd_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ a,
                                                              const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                              int rps, bf16* __restrict__ da, int da_acc,
                                                              float* __restrict__ partial, int64_t M, int D, int cge, int rpb) {
  rows_reduce<1>(grid_rows(M, rpb), D, D, cge, rpb, partial, blockIdx.x, gridDim.x, [&](int cg) TOK_ROW_INLINE {
    float gm[8];
    load8f(gamma + cg * 8, gm);
    return [=](int64_t m, size_t off, float (&s1)[1][8]) TOK_ROW_INLINE {
      const float s = row_scale ? row_scale[m / rps] : 1.f;
      const bf16x8 g = ldg16(dout + off);
      if (partial) {
        const bf16x8 av = ldg16(a + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) s1[0][e] = fmaf(s * bf2f(g[e]), bf2f(av[e]), s1[0][e]);
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
    };
  });
}

}  // namespace

extern "C" int tok_layer_scale_bwd_rows(int64_t rows, int d) {
  if (rows <= 0 || d <= 0 || d % 8) return 0;
  return row_blocks(rows, make_geo(d), LS_BLOCKS);
}

extern "C" int tok_layer_scale_fwd(const void* x, const void* a, const float* gamma, const float* row_scale,
                                   int rows_per_sample, void* out, int64_t rows, int d, void* stream) {
  TOK_CHECK_ARG(x && a && gamma && out, "tok_layer_scale_fwd: null pointer");
  TOK_CHECK_ARG(rows > 0 && d > 0 && d % 8 == 0 && (!row_scale || rows_per_sample > 0), "tok_layer_scale_fwd: bad sizes");
  const Geo g = make_geo(d);
  hipLaunchKernelGGL(layer_scale_fwd_kernel, dim3(row_blocks(rows, g, LS_BLOCKS)), dim3(256), 0, tok_stream(stream), (const bf16*)x,
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
  const int blocks = row_blocks(rows, g, LS_BLOCKS);
  hipLaunchKernelGGL(layer_scale_bwd_kernel, dim3(blocks), dim3(256), 0, tok_stream(stream), (const bf16*)dout, (const bf16*)a,
                     gamma, row_scale, row_scale ? rows_per_sample : 1, (bf16*)da, da_accumulate ? 1 : 0,
                     dgamma ? partial : (float*)nullptr, rows, d, g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_layer_scale_bwd");
  if (!dgamma) return TOK_OK;
  return tok_colsum_f32(partial, blocks, d, dgamma, dgamma_accumulate, stream);
}
