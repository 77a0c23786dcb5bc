// Token-embedding helpers of the Vision Transformer family: patch gather, class token + position embedding and its gradient,
// and the selection of a range of token rows.
#include "tok_common.h"

namespace {

// img NHWC bf16 [n][h][w][4] -> rows [n * (h/p) * (w/p)][p * p * 4]: one thread per pixel (8 bytes)
__global__ __launch_bounds__(256) void patch_gather_kernel(const uint2* __restrict__ img, int n, int h, int w, int p,
                                                           uint2* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * h * w) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h), b = (int)(t / h);
  const int gh = h / p, gw = w / p;
  const int64_t row = ((int64_t)b * gh + y / p) * gw + x / p;
  rows[row * p * p + (y % p) * p + (x % p)] = img[i];
}

// out[b][t] = (t < prefix ? cls (+ pos[0]) : patch[b][t - prefix] + pos[no_embed_class ? t - prefix : t]), rounded once
__global__ __launch_bounds__(256) void vit_embed_fwd_kernel(const bf16* __restrict__ patch, const float* __restrict__ pos,
                                                            const float* __restrict__ cls, int B, int P, int D, int prefix,
                                                            int no_embed_class, bf16* __restrict__ out) {
  const int T = P + prefix, dg = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * T * dg) return;
  const int d0 = (int)(i % dg) * 8;
  const int64_t row = i / dg;
  const int t = (int)(row % T), b = (int)(row / T);
  float v[8];
  if (t < prefix) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = cls[d0 + j] + (no_embed_class ? 0.f : pos[d0 + j]);
  } else {
    const bf16x8 x = ldg16(patch + ((int64_t)b * P + (t - prefix)) * D + d0);
    const float* pr = pos + (size_t)(no_embed_class ? t - prefix : t) * D + d0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(x[j]) + pr[j];
  }
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bf(v[j]);
  stg16(out + row * D + d0, r);
}

// d(pos)[j][d] = sum_b dout[b][j + off][d] for j < L; d(cls)[d] = sum_b dout[b][0][d] (row L of the launch); image order
__global__ __launch_bounds__(256) void vit_embed_bwd_kernel(const bf16* __restrict__ dout, int B, int T, int D, int L, int off,
                                                            float* __restrict__ dpos, int pos_acc, float* __restrict__ dcls,
                                                            int cls_acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)(L + 1) * D) return;
  const int d = (int)(i % D), j = (int)(i / D);
  float* dst;
  int acc, row;
  if (j < L) {
    if (!dpos) return;
    dst = dpos + (size_t)j * D + d;
    acc = pos_acc;
    row = j + off;
  } else {
    if (!dcls) return;
    dst = dcls + d;
    acc = cls_acc;
    row = 0;
  }
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += bf2f(dout[((int64_t)b * T + row) * D + d]);
  *dst = acc ? *dst + s : s;
}

// rows [first, first + count) of every image's T rows: forward gather (dir 0) or its transpose (dir 1: dsrc (+)= scatter, the
// other rows 0 / unchanged)
__global__ __launch_bounds__(256) void rows_select_kernel(const bf16* __restrict__ src, int B, int T, int first, int count, int D,
                                                          bf16* __restrict__ dst, int dir, int accumulate) {
  const int dg = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (dir == 0) {
    if (i >= (int64_t)B * count * dg) return;
    const int d0 = (int)(i % dg) * 8;
    const int64_t r = i / dg;
    const int b = (int)(r / count), t = (int)(r % count) + first;
    stg16(dst + r * D + d0, ldg16(src + ((int64_t)b * T + t) * D + d0));
    return;
  }
  if (i >= (int64_t)B * T * dg) return;
  const int d0 = (int)(i % dg) * 8;
  const int64_t r = i / dg;
  const int b = (int)(r / T), t = (int)(r % T);
  bf16* o = dst + r * D + d0;
  if (t < first || t >= first + count) {
    if (!accumulate) stg16(o, zero8());
    return;
  }
  const bf16x8 gsel = ldg16(src + ((int64_t)b * count + (t - first)) * D + d0);
  if (!accumulate) {
    stg16(o, gsel);
    return;
  }
  const bf16x8 cur = ldg16(o);
  bf16x8 r8;
#pragma unroll
  for (int j = 0; j < 8; ++j) r8[j] = f2bf(bf2f(cur[j]) + bf2f(gsel[j]));
  stg16(o, r8);
}

}  // namespace

extern "C" int tok_patch_gather(const void* img, int n, int h, int w, int p, void* rows, void* stream) {
  TOK_CHECK_ARG(img && rows && n > 0 && p > 0 && h >= p && w >= p && h % p == 0 && w % p == 0,
                "tok_patch_gather: %dx%d image, patch %d (sides must be multiples of the patch)", h, w, p);
  TOK_CHECK_ARG(tok_aligned(img, 8) && tok_aligned(rows, 8), "tok_patch_gather: img / rows must be 8-byte aligned");
  const int64_t px = (int64_t)n * h * w;
  hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks_of(px)), dim3(256), 0, tok_stream(stream), (const uint2*)img, n, h, w, p,
                     (uint2*)rows);
  TOK_CHECK_LAUNCH("tok_patch_gather");
  return TOK_OK;
}

extern "C" int tok_vit_embed_fwd(const void* patch, const float* pos, const float* cls, int batch, int patches, int d,
                                 int no_embed_class, void* out, void* stream) {
  TOK_CHECK_ARG(patch && pos && out && batch > 0 && patches > 0 && d > 0 && d % 8 == 0, "tok_vit_embed_fwd: bad args");
  TOK_CHECK_ARG(tok_aligned(patch, 16) && tok_aligned(out, 16), "tok_vit_embed_fwd: patch / out must be 16-byte aligned");
  const int prefix = cls ? 1 : 0;
  hipLaunchKernelGGL(vit_embed_fwd_kernel, dim3(blocks_of((int64_t)batch * (patches + prefix) * (d / 8))), dim3(256), 0,
                     tok_stream(stream), (const bf16*)patch, pos, cls, batch, patches, d, prefix, no_embed_class ? 1 : 0,
                     (bf16*)out);
  TOK_CHECK_LAUNCH("tok_vit_embed_fwd");
  return TOK_OK;
}

extern "C" int tok_vit_embed_bwd(const void* dout, int batch, int patches, int d, int has_cls, int no_embed_class, float* dpos,
                                 int pos_acc, float* dcls, int cls_acc, void* stream) {
  TOK_CHECK_ARG(dout && batch > 0 && patches > 0 && d > 0 && d % 8 == 0 && (!dcls || has_cls), "tok_vit_embed_bwd: bad args");
  if (!dpos && !dcls) return TOK_OK;
  const int prefix = has_cls ? 1 : 0, T = patches + prefix;
  const int L = no_embed_class ? patches : T, off = no_embed_class ? prefix : 0;
  hipLaunchKernelGGL(vit_embed_bwd_kernel, dim3(blocks_of((int64_t)(L + 1) * d)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)dout, batch, T, d, L, off, dpos, pos_acc, dcls, cls_acc);
  TOK_CHECK_LAUNCH("tok_vit_embed_bwd");
  return TOK_OK;
}

extern "C" int tok_rows_select(const void* src, int batch, int t, int first, int count, int d, void* dst, int dir,
                               int accumulate, void* stream) {
  TOK_CHECK_ARG(src && dst && batch > 0 && t > 0 && first >= 0 && count > 0 && first + count <= t && d > 0 && d % 8 == 0 &&
                (dir == 0 || dir == 1), "tok_rows_select: bad args");
  TOK_CHECK_ARG(tok_aligned(src, 16) && tok_aligned(dst, 16), "tok_rows_select: src / dst must be 16-byte aligned");
  const int64_t work = (int64_t)batch * (dir == 0 ? count : t) * (d / 8);
  hipLaunchKernelGGL(rows_select_kernel, dim3(blocks_of(work)), dim3(256), 0, tok_stream(stream), (const bf16*)src, batch, t,
                     first, count, d, (bf16*)dst, dir, accumulate ? 1 : 0);
  TOK_CHECK_LAUNCH("tok_rows_select");
  return TOK_OK;
}
