// Pixel-wise cross entropy on bilinearly upsampled logits, without the upsampled tensor.
// SegmentationHead.forward (heads/segmentation/base.py:31-41) ends in
// F.interpolate(segm_logits, size=input.shape[2:], mode='bilinear') and the recipe's loss is CrossEntropyLoss on the result
// (examples/configs/segmentation_*.yaml): at HRNet-W48 / 512x1024 / batch 24 the (B, 19 -> 24, 512, 1024) bf16 tensor is
// 604 MB, written by tok_bilinear_fwd, read by the loss, and its gradient written and read once more by tok_bilinear_bwd.
// Here every full-resolution pixel evaluates its 2x2 footprint of the LOW-resolution logits on the fly (resample.h's
// src_index and the same bf16 rounding of the interpolated value as tok_bilinear_fwd: the loss is the unfused one),
// and the backward is the adjoint in gather form (tok_bilinear_bwd's adjoint_walk): a low-resolution pixel visits the
// full-resolution pixels whose footprint contains it, recomputes their softmax from the saved log-sum-exp and sums
// weight * bf16(d logits) — deterministic, no atomics, nothing full-resolution in HBM except lse / row_loss (4 bytes per pixel each).
#include "loss_common.h"
#include "resample.h"
#include <stdlib.h>
#include <math.h>
#include <type_traits>

namespace {

struct UpArgs {
  int n, hs, ws, classes, ld, hd, wd;
  float sh, sw;     // in / out
};

// interpolated, bf16-rounded logits of full-resolution pixel (b, y, x): v[0 .. 8 NV)
template <int NV>
__device__ __forceinline__ void up_logits(const bf16* __restrict__ low, const UpArgs& a, int b, int y, int x, float* v) {
  int y0, y1, x0, x1;
  float ly, lx;
  src_index(a.sh, y, a.hs, y0, y1, ly);
  src_index(a.sw, x, a.ws, x0, x1, lx);
  const float hy = 1.f - ly, hx = 1.f - lx;
  const bf16* base = low + (size_t)b * a.hs * a.ws * a.ld;
  const bf16* p00 = base + ((size_t)y0 * a.ws + x0) * a.ld;
  const bf16* p01 = base + ((size_t)y0 * a.ws + x1) * a.ld;
  const bf16* p10 = base + ((size_t)y1 * a.ws + x0) * a.ld;
  const bf16* p11 = base + ((size_t)y1 * a.ws + x1) * a.ld;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const bf16x8 v00 = ldg16(p00 + i * 8), v01 = ldg16(p01 + i * 8), v10 = ldg16(p10 + i * 8), v11 = ldg16(p11 + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e)
      v[i * 8 + e] = bf2f(f2bf(hy * (hx * bf2f(v00[e]) + lx * bf2f(v01[e])) + ly * (hx * bf2f(v10[e]) + lx * bf2f(v11[e]))));
  }
}

template <int NV>
__global__ __launch_bounds__(256) void upce_fwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target, UpArgs a,
                                                       int64_t ignore_index, float* __restrict__ lse,
                                                       float* __restrict__ row_loss) {
  const size_t total = (size_t)a.n * a.hd * a.wd;
  for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < total; pix += (size_t)gridDim.x * 256) {
    int x, y, b;
    split_pixel(pix, a.wd, a.hd, x, y, b);
    float v[8 * NV];
    up_logits<NV>(low, a, b, y, x, v);
    float mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < 8 * NV; ++c) mx = fmaxf(mx, c < a.classes ? v[c] : -INFINITY);
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 8 * NV; ++c) s += (c < a.classes) ? __expf(v[c] - mx) : 0.f;
    const float l = mx + __logf(s);
    lse[pix] = l;
    const int64_t t = target[pix];
    float rl = 0.f;
    if (ce_row_valid(t, ignore_index, a.classes)) {
      float zt = 0.f;
#pragma unroll
      for (int c = 0; c < 8 * NV; ++c) zt = (c == (int)t) ? v[c] : zt;
      rl = l - zt;
    }
    row_loss[pix] = rl;
  }
}

template <int NV>
__global__ __launch_bounds__(256) void upce_bwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target, UpArgs a,
                                                       int64_t ignore_index, const float* __restrict__ lse,
                                                       const float* __restrict__ loss, const float* __restrict__ gscale,
                                                       bf16* dlow, int accumulate) {
  const size_t total = (size_t)a.n * a.hs * a.ws;
  const float g = (gscale ? gscale[0] : 1.f) / loss[1];
  for (size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x; pix < total; pix += (size_t)gridDim.x * 256) {
    int xs, ys, b;
    split_pixel(pix, a.ws, a.hs, xs, ys, b);
    float acc[NV][8];
#pragma unroll
    for (int c = 0; c < 8 * NV; ++c) acc[c >> 3][c & 7] = 0.f;
    adjoint_walk(a.sh, a.sw, a.hs, a.ws, a.hd, a.wd, ys, xs, [&](int yd, int xd, float wgt) TOK_ROW_INLINE {
      const size_t dp = ((size_t)b * a.hd + yd) * a.wd + xd;
      const int64_t t = target[dp];
      if (!ce_row_valid(t, ignore_index, a.classes)) return;
      float v[8 * NV];
      up_logits<NV>(low, a, b, yd, xd, v);
      const float l = lse[dp];
#pragma unroll
      for (int c = 0; c < 8 * NV; ++c) {
        // d(upsampled logits), rounded to bf16 as the unfused tok_softmax_ce_bwd stores it
        const float w = c < a.classes ? bf2f(f2bf((__expf(v[c] - l) - (c == (int)t ? 1.f : 0.f)) * g)) : 0.f;
        acc[c >> 3][c & 7] = fmaf(wgt, w, acc[c >> 3][c & 7]);
      }
    });
#pragma unroll
    for (int i = 0; i < NV; ++i) store_acc<8>(dlow + pix * a.ld + i * 8, acc[i], accumulate);
  }
}

// The same adjoint with every full-resolution pixel evaluated ONCE per block instead of once per low-resolution pixel it
// touches (4x for a scale of 4: the gather kernel above spends its time in 19 expf per visit): a block owns UT x UT
// low-resolution pixels, stages bf16(d upsampled logits) of the full-resolution window that can touch them in LDS (phase 1),
// then every (low-resolution pixel, 8-channel group) walks its footprint with tok_bilinear_bwd's exact index / weight
// arithmetic, reading LDS (phase 2).  Window = the union of the per-pixel windows of the gather kernel, at most UWIN x UWIN.
constexpr int UT = 8, UWIN = 40, UPP = 12;     // tile edge, window edge, window of ONE source pixel (2 r + 4 at r <= 4)

template <int NV>
__global__ __launch_bounds__(256) void upce_bwd_tiled_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                             UpArgs a, int64_t ignore_index, const float* __restrict__ lse,
                                                             const float* __restrict__ loss, const float* __restrict__ gscale,
                                                             bf16* dlow, int accumulate, int tiles_y, int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) char up_smem[];
  bf16* win = reinterpret_cast<bf16*>(up_smem);                 // [wh][ww][8 NV]
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x;
  const int t2 = tile / tiles_x;
  const int ty = t2 % tiles_y;
  const int b = t2 / tiles_y;
  const int ys0 = ty * UT, xs0 = tx * UT;
  const int ys1 = min(a.hs, ys0 + UT) - 1, xs1 = min(a.ws, xs0 + UT) - 1;
  const float rh = 1.f / a.sh, rw = 1.f / a.sw;
  int wy0, wy1, wx0, wx1, tmp0, tmp1;
  adj_window(rh, ys0, a.hd, wy0, tmp1);
  adj_window(rh, ys1, a.hd, tmp0, wy1);
  adj_window(rw, xs0, a.wd, wx0, tmp1);
  adj_window(rw, xs1, a.wd, tmp0, wx1);
  const int wh = wy1 - wy0 + 1, ww = wx1 - wx0 + 1;             // <= UWIN (checked by the launcher for the scale)
  const float g = (gscale ? gscale[0] : 1.f) / loss[1];
  // ---- phase 1: bf16(d upsampled logits) of the window ----------------------------------------------------------------------
  for (int i = threadIdx.x; i < wh * ww; i += 256) {
    const int yd = wy0 + i / ww, xd = wx0 + i % ww;
    const size_t dp = ((size_t)b * a.hd + yd) * a.wd + xd;
    const int64_t t = target[dp];
    bf16* o = win + (size_t)i * (8 * NV);
    if (!ce_row_valid(t, ignore_index, a.classes)) {
#pragma unroll
      for (int v8 = 0; v8 < NV; ++v8) *reinterpret_cast<bf16x8*>(o + v8 * 8) = zero8();
      continue;
    }
    float v[8 * NV];
    up_logits<NV>(low, a, b, yd, xd, v);
    const float l = lse[dp];
#pragma unroll
    for (int v8 = 0; v8 < NV; ++v8) {
      bf16x8 q;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = v8 * 8 + e;
        q[e] = f2bf(c < a.classes ? (__expf(v[c] - l) - (c == (int)t ? 1.f : 0.f)) * g : 0.f);
      }
      *reinterpret_cast<bf16x8*>(o + v8 * 8) = q;
    }
  }
  __syncthreads();
  // ---- phase 2: the adjoint of the interpolation, one (low-resolution pixel, 8-channel group) per thread ------------------------
  for (int i = threadIdx.x; i < UT * UT * NV; i += 256) {
    const int v8 = i % NV;
    const int p = i / NV;
    const int ys = ys0 + p / UT, xs = xs0 + p % UT;
    if (ys > ys1 || xs > xs1) continue;
    int yd0, yd1, xd0, xd1;
    adj_window(rh, ys, a.hd, yd0, yd1);
    adj_window(rw, xs, a.wd, xd0, xd1);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    // the column weights of this pixel once (the window of one source pixel is at most UPP wide at the scales the tiled
    // kernel serves), then rows x columns of LDS reads
    float wxs[UPP];
#pragma unroll
    for (int j = 0; j < UPP; ++j) {
      const int xd = xd0 + j;
      const float wx = adj_weight(a.sw, xd <= xd1 ? xd : xd1, a.ws, xs);
      wxs[j] = xd <= xd1 ? wx : 0.f;
    }
    for (int yd = yd0; yd <= yd1; ++yd) {
      const float wy = adj_weight(a.sh, yd, a.hs, ys);
      if (wy == 0.f) continue;
      const bf16* rowp = win + ((size_t)(yd - wy0) * ww + (xd0 - wx0)) * (8 * NV) + v8 * 8;
#pragma unroll
      for (int j = 0; j < UPP; ++j) {
        if (wxs[j] == 0.f) continue;
        const bf16x8 q = *reinterpret_cast<const bf16x8*>(rowp + (size_t)j * (8 * NV));
        const float wgt = wy * wxs[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, bf2f(q[e]), acc[e]);
      }
    }
    store_acc<8>(dlow + (((size_t)b * a.hs + ys) * a.ws + xs) * a.ld + v8 * 8, acc, accumulate);
  }
}

// window of UT source pixels at destination/source ratio r: (UT - 1) r between first and last pixel + (2 r + 4) per pixel
bool up_tiled_ok(const UpArgs& a) {
  const float r = fmaxf(1.f / a.sh, 1.f / a.sw);
  return (int)ceilf((UT + 1) * r) + 4 <= UWIN;
}

bool fill_up(UpArgs& a, int n, int hs, int ws, int classes, int ld, int hd, int wd) {
  if (n <= 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0 || classes <= 0 || ld < classes || (ld & 7) || ld > 32) return false;
  if ((long long)n * hd * wd >= (1ll << 31)) return false;
  a.n = n; a.hs = hs; a.ws = ws; a.classes = classes; a.ld = ld; a.hd = hd; a.wd = wd;
  a.sh = (float)hs / (float)hd; a.sw = (float)ws / (float)wd;
  return true;
}

// f(NV as a compile-time constant) for a row of nv = ld / 8 = 1 .. 4 16-byte vectors: the kernels keep the row in registers
template <class F>
void with_nv(int nv, F&& f) {
  switch (nv) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}
}  // namespace

extern "C" int tok_upsample_ce_serves(int classes, int ld) { return classes > 0 && ld >= classes && (ld & 7) == 0 && ld <= 32; }

extern "C" int tok_upsample_ce_fwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                   const int64_t* target, int64_t ignore_index, float* lse, float* row_loss, float* loss,
                                   void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && row_loss && loss && fill_up(a, n, hs, ws, classes, ld, hd, wd),
                "tok_upsample_ce_fwd: bad args (row pitch a multiple of 8 up to 32 channels, n*hd*wd < 2^31)");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(low) & 15) == 0 && (reinterpret_cast<uintptr_t>(loss) & 7) == 0,
                "tok_upsample_ce_fwd: low must be 16-byte, loss 8-byte aligned");
  hipStream_t st = tok_stream(stream);
  const int rows = n * hd * wd;
  with_nv(ld >> 3, [&](auto nv) {
    hipLaunchKernelGGL(upce_fwd_kernel<decltype(nv)::value>, dim3(grid_for((size_t)rows)), dim3(256), 0, st, (const bf16*)low,
                       target, a, ignore_index, lse, row_loss);
  });
  TOK_CHECK_LAUNCH("tok_upsample_ce_fwd");
  return ce_mean_launch("tok_upsample_ce_fwd", row_loss, target, rows, ignore_index, classes, loss, st);
}

extern "C" int tok_upsample_ce_bwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                   const int64_t* target, int64_t ignore_index, const float* lse, const float* loss,
                                   const float* gscale, void* dlow, int accumulate, void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && loss && dlow && fill_up(a, n, hs, ws, classes, ld, hd, wd), "tok_upsample_ce_bwd: bad args");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(low) & 15) == 0 && (reinterpret_cast<uintptr_t>(dlow) & 15) == 0,
                "tok_upsample_ce_bwd: low / dlow must be 16-byte aligned");
  hipStream_t st = tok_stream(stream);
  if (up_tiled_ok(a)) {
    const int tiles_y = tok_cdiv(hs, UT), tiles_x = tok_cdiv(ws, UT);
    with_nv(ld >> 3, [&](auto nv) {
      constexpr int NV = decltype(nv)::value;
      tok_launch_lds<&upce_bwd_tiled_kernel<NV>>(UWIN * UWIN * NV * 16, dim3(n * tiles_y * tiles_x), dim3(256), UWIN * UWIN * ld * 2,
                                                 st, (const bf16*)low, target, a, ignore_index, lse, loss, gscale, (bf16*)dlow,
                                                 accumulate, tiles_y, tiles_x);
    });
    TOK_CHECK_LAUNCH("tok_upsample_ce_bwd(tiled)");
    return TOK_OK;
  }
  with_nv(ld >> 3, [&](auto nv) {
    hipLaunchKernelGGL(upce_bwd_kernel<decltype(nv)::value>, dim3(grid_for((size_t)n * hs * ws)), dim3(256), 0, st,
                       (const bf16*)low, target, a, ignore_index, lse, loss, gscale, (bf16*)dlow, accumulate);
  });
  TOK_CHECK_LAUNCH("tok_upsample_ce_bwd");
  return TOK_OK;
}
