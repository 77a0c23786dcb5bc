// BatchNorm + hard-swish (MobileNetV3), NHWC bf16, fp32 arithmetic: the mask-less activation path.
//   z = y*scale + shift        out = hswish(z) = z * min(max(z + 3, 0), 6) / 6
//   dz = dout * hswish'(z)     hswish'(z) = 0 (z < -3), z/3 + 0.5 (-3 <= z <= 3), 1 (z > 3)      dy = c1*dz + c2*y + c3
// Nothing is kept between the passes but y: forward, reduce and apply each recompute z = fmaf(y, scale, shift) from the stored
// bf16 y (the expression bn_act_fwd_kernel evaluates), so all three see the same z and the same branch of the derivative.
// Geometry: make_geo (tok_common.h), min(C/8, 256) channel groups across the block, 8 channels (16 bytes) per lane, grid-stride
// over rows; a lane keeps its channel group's coefficients in registers.  The reduce leaves partial[2][rows][C] in the row
// layout of tok_bn_bwd_reduce (rows = tok_bn_bwd_rows): tok_bn_bwd_finalize folds it with dzy_form = 0.  Fixed summation
// order, no atomics: two runs give the same bits.
#include "tok_common.h"

namespace {

__device__ __forceinline__ float hswish_f(float z) {
  return z * __builtin_amdgcn_fmed3f(z + 3.f, 0.f, 6.f) * (1.f / 6.f);
}
// what torch.nn.functional.hardswish differentiates to (the kinks belong to the middle branch)
__device__ __forceinline__ float hswish_d(float z) {
  const float mid = fmaf(z, 1.f / 3.f, 0.5f);
  return z < -3.f ? 0.f : (z <= 3.f ? mid : 1.f);
}

__global__ __launch_bounds__(256) void bn_hswish_fwd_kernel(const bf16* __restrict__ y, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, bf16* __restrict__ out,
                                                            int64_t M, int C, int cge, int rpb) {
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  if (rl >= rpb) return;
  const int cg_total = C >> 3;
  for (int cg = cgl; cg < cg_total; cg += cge) {
    float sc[8], sh[8];
    load8f(scale + cg * 8, sc);
    load8f(shift + cg * 8, sh);
    for (int64_t m = (int64_t)blockIdx.x * rpb + rl; m < M; m += (int64_t)gridDim.x * rpb) {
      const size_t off = (size_t)m * C + cg * 8;
      const bf16x8 v = ldg16(y + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(hswish_f(fmaf(bf2f(v[e]), sc[e], sh[e])));
      stg16(out + off, o);
    }
  }
}

// partial[2][gridDim.x][C] = (sum dz, sum dz * xhat)
__global__ __launch_bounds__(256) void bn_hswish_bwd_reduce_kernel(
    const bf16* __restrict__ dout, const bf16* __restrict__ y, const float* __restrict__ scale,
    const float* __restrict__ shift, const float* __restrict__ mean, const float* __restrict__ rstd, int64_t M, int C, int cge,
    int rpb, float* __restrict__ partial) {
  __shared__ float red[2][256][8];
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  const int cg_total = C >> 3;
  for (int cg0 = 0; cg0 < cg_total; cg0 += cge) {     // block-uniform trip count: every lane reaches both barriers
    const int cg = cg0 + cgl;
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
    if (rl < rpb && cg < cg_total) {
      float sc[8], sh[8], mu[8], rs[8];
      load8f(scale + cg * 8, sc);
      load8f(shift + cg * 8, sh);
      load8f(mean + cg * 8, mu);
      load8f(rstd + cg * 8, rs);
      for (int64_t m = (int64_t)blockIdx.x * rpb + rl; m < M; m += (int64_t)gridDim.x * rpb) {
        const size_t off = (size_t)m * C + cg * 8;
        const bf16x8 g = ldg16(dout + off);
        const bf16x8 v = ldg16(y + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float yf = bf2f(v[e]);
          const float dz = bf2f(g[e]) * hswish_d(fmaf(yf, sc[e], sh[e]));
          s1[e] += dz;
          s2[e] = fmaf(dz, (yf - mu[e]) * rs[e], s2[e]);
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) { red[0][tid][e] = s1[e]; red[1][tid][e] = s2[e]; }
    __syncthreads();
    if (rl == 0 && cg < cg_total) {
      for (int r = 1; r < rpb; ++r)
#pragma unroll
        for (int e = 0; e < 8; ++e) { s1[e] += red[0][r * cge + cgl][e]; s2[e] += red[1][r * cge + cgl][e]; }
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        partial[((size_t)0 * gridDim.x + blockIdx.x) * C + cg * 8 + e] = s1[e];
        partial[((size_t)1 * gridDim.x + blockIdx.x) * C + cg * 8 + e] = s2[e];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void bn_hswish_bwd_apply_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ y,
                                                                  const float* __restrict__ scale,
                                                                  const float* __restrict__ shift,
                                                                  const float* __restrict__ coef, bf16* __restrict__ dy,
                                                                  int64_t M, int C, int cge, int rpb) {
  const int tid = threadIdx.x;
  const int cgl = tid % cge, rl = tid / cge;
  if (rl >= rpb) return;
  const int cg_total = C >> 3;
  for (int cg = cgl; cg < cg_total; cg += cge) {
    float sc[8], sh[8], c1[8], c2[8], c3[8];
    load8f(scale + cg * 8, sc);
    load8f(shift + cg * 8, sh);
    load8f(coef + cg * 8, c1);
    load8f(coef + C + cg * 8, c2);
    load8f(coef + 2 * C + cg * 8, c3);
    for (int64_t m = (int64_t)blockIdx.x * rpb + rl; m < M; m += (int64_t)gridDim.x * rpb) {
      const size_t off = (size_t)m * C + cg * 8;
      const bf16x8 g = ldg16(dout + off);
      const bf16x8 v = ldg16(y + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float yf = bf2f(v[e]);
        const float dz = bf2f(g[e]) * hswish_d(fmaf(yf, sc[e], sh[e]));
        o[e] = f2bf(fmaf(c1[e], dz, fmaf(c2[e], yf, c3[e])));
      }
      stg16(dy + off, o);
    }
  }
}

}  // namespace

// Grid sizes come from the exported row counts of bn.hip, so the block cap of the elementwise passes (TOK_BN_BLOCKS) and the
// partial-row layout of the reduce are those of the ReLU path by construction.
extern "C" int tok_bn_hswish_fwd(const void* y, const float* scale, const float* shift, void* out, int64_t m, int c,
                                 void* stream) {
  TOK_CHECK_ARG(y && scale && shift && out && m > 0 && c > 0 && c % 8 == 0, "tok_bn_hswish_fwd: bad args");
  if (tok_dbg_skip(8)) return TOK_OK;
  const Geo g = make_geo(c);
  hipLaunchKernelGGL(bn_hswish_fwd_kernel, dim3(tok_bn_act_fwd_colsum_rows(m, c)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)y, scale, shift, (bf16*)out, m, c, g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_bn_hswish_fwd");
  return TOK_OK;
}

extern "C" int tok_bn_hswish_bwd_reduce(const void* dout, const void* y, const float* scale, const float* shift,
                                        const float* mean, const float* rstd, int64_t m, int c, float* partial, void* stream) {
  TOK_CHECK_ARG(dout && y && scale && shift && mean && rstd && partial, "tok_bn_hswish_bwd_reduce: null pointer");
  TOK_CHECK_ARG(m > 0 && c > 0 && c % 8 == 0, "tok_bn_hswish_bwd_reduce: bad sizes");
  const Geo g = make_geo(c);
  hipLaunchKernelGGL(bn_hswish_bwd_reduce_kernel, dim3(tok_bn_bwd_rows(m, c)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)dout, (const bf16*)y, scale, shift, mean, rstd, m, c, g.cge, g.rpb, partial);
  TOK_CHECK_LAUNCH("tok_bn_hswish_bwd_reduce");
  return TOK_OK;
}

extern "C" int tok_bn_hswish_bwd_apply(const void* dout, const void* y, const float* scale, const float* shift,
                                       const float* coef, void* dy, int64_t m, int c, void* stream) {
  TOK_CHECK_ARG(dout && y && scale && shift && coef && dy, "tok_bn_hswish_bwd_apply: null pointer");
  TOK_CHECK_ARG(m > 0 && c > 0 && c % 8 == 0, "tok_bn_hswish_bwd_apply: bad sizes");
  if (tok_dbg_skip(8)) return TOK_OK;
  const Geo g = make_geo(c);
  hipLaunchKernelGGL(bn_hswish_bwd_apply_kernel, dim3(tok_bn_act_fwd_colsum_rows(m, c)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)dout, (const bf16*)y, scale, shift, coef, (bf16*)dy, m, c, g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_bn_hswish_bwd_apply");
  return TOK_OK;
}
