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
#include "loss_upsample.h"
#include <stdlib.h>

namespace {

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

// The gather backward of channels [c0, c0 + 8 NV) (the narrow kernel: the whole row, c0 = 0, no weights; the wide one: one chunk
// per blockIdx.y).  d(upsampled logits) of a pixel with label t carries w[t] under class weights (ce_row_scale).
template <int NV>
__device__ __forceinline__ void upce_bwd_gather(const bf16* __restrict__ low, const int64_t* __restrict__ target, const UpArgs& a,
                                                int64_t ignore_index, const float* __restrict__ weight,
                                                const float* __restrict__ lse, const float* __restrict__ loss,
                                                const float* __restrict__ gscale, bf16* dlow, int accumulate, int c0) {
  const size_t total = (size_t)a.n * a.hs * a.ws;
  const float g0 = (gscale ? gscale[0] : 1.f) / loss[1];
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
      up_logits<NV>(low + c0, a, b, yd, xd, v);
      const float l = lse[dp];
      const float g = ce_row_scale(g0, weight, t);
#pragma unroll
      for (int c = 0; c < 8 * NV; ++c) {
        // d(upsampled logits), rounded to bf16 as the unfused tok_softmax_ce_bwd stores it
        const float w = c0 + c < a.classes ? bf2f(f2bf((__expf(v[c] - l) - (c0 + c == (int)t ? 1.f : 0.f)) * g)) : 0.f;
        acc[c >> 3][c & 7] = fmaf(wgt, w, acc[c >> 3][c & 7]);
      }
    });
#pragma unroll
    for (int i = 0; i < NV; ++i) store_acc<8>(dlow + pix * a.ld + c0 + i * 8, acc[i], accumulate);
  }
}

template <int NV>
__global__ __launch_bounds__(256) void upce_bwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target, UpArgs a,
                                                       int64_t ignore_index, const float* __restrict__ lse,
                                                       const float* __restrict__ loss, const float* __restrict__ gscale,
                                                       bf16* dlow, int accumulate) {
  upce_bwd_gather<NV>(low, target, a, ignore_index, nullptr, lse, loss, gscale, dlow, accumulate, 0);
}

// The same adjoint with every full-resolution pixel evaluated ONCE per block instead of once per low-resolution pixel it
// touches (4x for a scale of 4: the gather kernel above spends its time in 19 expf per visit): a block owns UT x UT
// low-resolution pixels, stages bf16(d upsampled logits) of the full-resolution window that can touch them in LDS (phase 1),
// then every (low-resolution pixel, 8-channel group) walks its footprint with tok_bilinear_bwd's exact index / weight
// arithmetic, reading LDS (phase 2).  Window = the union of the per-pixel windows of the gather kernel, at most UWIN x UWIN.
// (channels [c0, c0 + 8 NV) and the class weights as in upce_bwd_gather)
template <int NV>
__device__ __forceinline__ void upce_bwd_tiled(const bf16* __restrict__ low, const int64_t* __restrict__ target, const UpArgs& a,
                                               int64_t ignore_index, const float* __restrict__ weight,
                                               const float* __restrict__ lse, const float* __restrict__ loss,
                                               const float* __restrict__ gscale, bf16* dlow, int accumulate, int tiles_y,
                                               int tiles_x, int c0) {
  extern __shared__ __attribute__((aligned(16))) char up_smem[];
  bf16* win = reinterpret_cast<bf16*>(up_smem);                 // [wh][ww][8 NV]
  const UpTile tl = up_tile<UT>(a, tiles_y, tiles_x);
  const int b = tl.b, wy0 = tl.wy0, wx0 = tl.wx0, wh = tl.wh, ww = tl.ww;             // wh, ww <= UWIN
  const float g0 = (gscale ? gscale[0] : 1.f) / loss[1];
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
    up_logits<NV>(low + c0, a, b, yd, xd, v);
    const float l = lse[dp];
    const float g = ce_row_scale(g0, weight, t);
#pragma unroll
    for (int v8 = 0; v8 < NV; ++v8) {
      bf16x8 q;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int c = v8 * 8 + e;
        q[e] = f2bf(c0 + c < a.classes ? (__expf(v[c] - l) - (c0 + c == (int)t ? 1.f : 0.f)) * g : 0.f);
      }
      *reinterpret_cast<bf16x8*>(o + v8 * 8) = q;
    }
  }
  __syncthreads();
  // ---- phase 2: the adjoint of the interpolation, one (low-resolution pixel, 8-channel group) per thread ------------------------
  up_adjoint_tile<UT>(win, a, tl, NV, dlow, accumulate, c0);
}

template <int NV>
__global__ __launch_bounds__(256) void upce_bwd_tiled_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                             UpArgs a, int64_t ignore_index, const float* __restrict__ lse,
                                                             const float* __restrict__ loss, const float* __restrict__ gscale,
                                                             bf16* dlow, int accumulate, int tiles_y, int tiles_x) {
  upce_bwd_tiled<NV>(low, target, a, ignore_index, nullptr, lse, loss, gscale, dlow, accumulate, tiles_y, tiles_x, 0);
}

// ---- rows of up to 256 classes (tok_upsample_ce_wide_*) ---------------------------------------------------------------------------
// A row of 33 .. 256 classes does not fit one thread's registers, so the forward lays the classes ACROSS lanes: a group of G lanes
// (G = the power of two >= ld / 8, at most 32) owns one full-resolution pixel, lane j holds the 16-byte vector of classes
// [8 j, 8 j + 8); maximum, sum of exponentials and the target's logit are folded over the group with shuffles, and a wavefront
// works on 64 / G pixels at once.  A block owns a WT x WT tile of destination pixels and stages the tile's low-resolution
// footprint in LDS with 16-byte loads (STAGE; at scale 4 about 7 x 7 source pixels, 25 KB at ld = 256), so the four taps of every
// pixel are LDS reads instead of four global gathers.  Where the footprint does not fit (downsampling, identity at wide rows) the
// taps come from global memory.  Blend, rounding, __expf / __logf and the validity rule are the narrow kernel's; so is the order of
// the sum inside every block of 32 classes (group_sum), which makes unweighted results at ld <= 32 the narrow kernel's bits.
constexpr int WIDE_LDS = 64 * 1024;

template <int G, bool STAGE>
__global__ __launch_bounds__(256) void upce_wide_fwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                            UpArgs a, int64_t ignore_index, const float* __restrict__ weight,
                                                            float* __restrict__ lse, float* __restrict__ row_loss, int tiles_y,
                                                            int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) char up_smem[];
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x;
  const int t2 = tile / tiles_x;
  const int ty = t2 % tiles_y;
  const int b = t2 / tiles_y;
  const int yt0 = ty * WT, xt0 = tx * WT;
  const int yt1 = min(a.hd, yt0 + WT) - 1, xt1 = min(a.wd, xt0 + WT) - 1;
  // taps are read at src[((y - sy0) * fw + (x - sx0)) * ld]: the image in global memory, or the footprint [fh][fw][ld] in LDS
  const bf16* src = low + (size_t)b * a.hs * a.ws * a.ld;
  int sy0 = 0, sx0 = 0, fw = a.ws;
  if constexpr (STAGE) {
    bf16* win = reinterpret_cast<bf16*>(up_smem);
    up_stage_footprint(src, a, yt0, yt1, xt0, xt1, win, sy0, sx0, fw);
    __syncthreads();
    src = win;
  }
  const int j = threadIdx.x & (G - 1);
  const bool lane_on = j * 8 < a.ld;                             // (idle lanes of a group: ld / 8 is no power of two)
  for (int p = threadIdx.x / G; p < WT * WT; p += 256 / G) {
    // every lane of a group stays in the loop for the shuffles: a pixel outside a partial tile is computed at the tile's
    // edge and not stored
    const int yy = yt0 + p / WT, xx = xt0 + p % WT;
    const int y = min(yy, yt1), x = min(xx, xt1);
    float v[8] = {};
    if (lane_on) {
      int y0, y1, x0, x1;
      float ly, lx;
      src_index(a.sh, y, a.hs, y0, y1, ly);
      src_index(a.sw, x, a.ws, x0, x1, lx);
      const bf16* r0 = src + (size_t)(y0 - sy0) * fw * a.ld + j * 8;
      const bf16* r1 = src + (size_t)(y1 - sy0) * fw * a.ld + j * 8;
      const int o0 = (x0 - sx0) * a.ld, o1 = (x1 - sx0) * a.ld;
      up_blend8(1.f - ly, ly, 1.f - lx, lx, ldg16(r0 + o0), ldg16(r0 + o1), ldg16(r1 + o0), ldg16(r1 + o1), v);
    }
    // classes beyond the row (the tail of the last vector, idle lanes) are -inf: never a maximum, exponential 0
    float mx = -INFINITY;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      v[e] = (lane_on && j * 8 + e < a.classes) ? v[e] : -INFINITY;
      mx = fmaxf(mx, v[e]);
    }
#pragma unroll
    for (int off = 1; off < G; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, G));
    float ex[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) ex[e] = (j * 8 + e < a.classes) ? __expf(v[e] - mx) : 0.f;
    const float l = mx + __logf(group_sum<G>(ex, j));
    const size_t pix = ((size_t)b * a.hd + y) * a.wd + x;
    const int64_t t = target[pix];
    const bool valid = ce_row_valid(t, ignore_index, a.classes);
    // the target's logit sits in lane t / 8
    float mine = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) mine = (e == ((int)t & 7)) ? v[e] : mine;
    const float zt = __shfl(mine, valid ? (int)t >> 3 : 0, G);
    if (j == 0 && yy <= yt1 && xx <= xt1) {
      lse[pix] = l;
      float rl = 0.f;
      if (valid) {
        rl = l - zt;
        if (weight) rl *= weight[t];
      }
      row_loss[pix] = rl;
    }
  }
}

// The backward needs no fold over the classes (softmax = exp(v - lse) of the saved lse), so it separates by channel: the narrow
// kernels' window-and-walk bodies on a grid of (tile or pixel block) x (chunk of 8 NV channels), blockIdx.y the chunk behind `c_base`.
template <int NV>
__global__ __launch_bounds__(256) void upce_wide_bwd_tiled_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                                  UpArgs a, int64_t ignore_index, const float* __restrict__ weight,
                                                                  const float* __restrict__ lse, const float* __restrict__ loss,
                                                                  const float* __restrict__ gscale, bf16* dlow, int accumulate,
                                                                  int tiles_y, int tiles_x, int c_base) {
  upce_bwd_tiled<NV>(low, target, a, ignore_index, weight, lse, loss, gscale, dlow, accumulate, tiles_y, tiles_x,
                     c_base + blockIdx.y * 8 * NV);
}

template <int NV>
__global__ __launch_bounds__(256) void upce_wide_bwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                            UpArgs a, int64_t ignore_index, const float* __restrict__ weight,
                                                            const float* __restrict__ lse, const float* __restrict__ loss,
                                                            const float* __restrict__ gscale, bf16* dlow, int accumulate,
                                                            int c_base) {
  upce_bwd_gather<NV>(low, target, a, ignore_index, weight, lse, loss, gscale, dlow, accumulate, c_base + blockIdx.y * 8 * NV);
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

constexpr int WIDE_NV = 2;     // channel chunk of the wide backward: 16 channels, a UWIN x UWIN window of 51 KB
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

extern "C" int tok_upsample_ce_wide_serves(int classes, int ld) { return classes > 0 && ld >= classes && (ld & 7) == 0 && ld <= 256; }

extern "C" int tok_upsample_ce_wide_fwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                        const int64_t* target, int64_t ignore_index, const float* weight, float* lse,
                                        float* row_loss, float* loss, void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && row_loss && loss && fill_up(a, n, hs, ws, classes, ld, hd, wd, 256),
                "tok_upsample_ce_wide_fwd: bad args (row pitch a multiple of 8 up to 256 channels, n*hd*wd < 2^31)");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(low) & 15) == 0 && (reinterpret_cast<uintptr_t>(loss) & 7) == 0,
                "tok_upsample_ce_wide_fwd: low must be 16-byte, loss 8-byte aligned");
  hipStream_t st = tok_stream(stream);
  const int tiles_y = tok_cdiv(hd, WT), tiles_x = tok_cdiv(wd, WT);
  const size_t bytes = (size_t)wide_footprint(a.sh, hs) * wide_footprint(a.sw, ws) * ld * 2;
  with_group(ld >> 3, [&](auto g) {
    constexpr int G = decltype(g)::value;
    if (bytes <= (size_t)WIDE_LDS)
      tok_launch_lds<&upce_wide_fwd_kernel<G, true>>(WIDE_LDS, dim3(n * tiles_y * tiles_x), dim3(256), bytes, st, (const bf16*)low,
                                                     target, a, ignore_index, weight, lse, row_loss, tiles_y, tiles_x);
    else
      hipLaunchKernelGGL((upce_wide_fwd_kernel<G, false>), dim3(n * tiles_y * tiles_x), dim3(256), 0, st, (const bf16*)low,
                         target, a, ignore_index, weight, lse, row_loss, tiles_y, tiles_x);
  });
  TOK_CHECK_LAUNCH("tok_upsample_ce_wide_fwd");
  return ce_mean_launch("tok_upsample_ce_wide_fwd", row_loss, target, n * hd * wd, ignore_index, classes, loss, st, weight);
}

extern "C" int tok_upsample_ce_wide_bwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                        const int64_t* target, int64_t ignore_index, const float* weight, const float* lse,
                                        const float* loss, const float* gscale, void* dlow, int accumulate, void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && loss && dlow && fill_up(a, n, hs, ws, classes, ld, hd, wd, 256),
                "tok_upsample_ce_wide_bwd: bad args");
  TOK_CHECK_ARG((reinterpret_cast<uintptr_t>(low) & 15) == 0 && (reinterpret_cast<uintptr_t>(dlow) & 15) == 0,
                "tok_upsample_ce_wide_bwd: low / dlow must be 16-byte aligned");
  hipStream_t st = tok_stream(stream);
  const bool tiled = up_tiled_ok(a);
  const int tiles_y = tok_cdiv(hs, UT), tiles_x = tok_cdiv(ws, UT);
  const unsigned blocks = tiled ? n * tiles_y * tiles_x : grid_for((size_t)n * hs * ws);
  // chunks of WIDE_NV vectors, then the rest of the row (ld / 8 odd) as one chunk of its own; rows of up to 32 channels whole
  auto launch = [&](auto nv, int chunks, int c_base) {
    constexpr int NV = decltype(nv)::value;
    if (tiled)
      tok_launch_lds<&upce_wide_bwd_tiled_kernel<NV>>(UWIN * UWIN * NV * 16, dim3(blocks, chunks), dim3(256), UWIN * UWIN * NV * 16,
                                                      st, (const bf16*)low, target, a, ignore_index, weight, lse, loss, gscale,
                                                      (bf16*)dlow, accumulate, tiles_y, tiles_x, c_base);
    else
      hipLaunchKernelGGL(upce_wide_bwd_kernel<NV>, dim3(blocks, chunks), dim3(256), 0, st, (const bf16*)low, target, a,
                         ignore_index, weight, lse, loss, gscale, (bf16*)dlow, accumulate, c_base);
  };
  const int nvec = ld >> 3, full = nvec / WIDE_NV;
  if (nvec <= 4) {
    // a row the narrow kernels hold in registers: one chunk, their instantiation of the body
    with_nv(nvec, [&](auto nv) { launch(nv, 1, 0); });
  } else {
    launch(std::integral_constant<int, WIDE_NV>(), full, 0);
    if (nvec % WIDE_NV) launch(std::integral_constant<int, 1>(), 1, full * WIDE_NV * 8);
  }
  TOK_CHECK_LAUNCH("tok_upsample_ce_wide_bwd");
  return TOK_OK;
}
