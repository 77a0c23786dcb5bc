// Multiclass Dice loss on bilinearly upsampled logits, without the upsampled tensor: the Dice half of the segmentation recipes'
// CrossEntropyLoss + DiceLoss pair (examples/configs/segmentation_*.yaml), next to loss_upsample_ce.hip.  Unfused, DiceLoss on a
// SegmentationHead output costs tok_bilinear_fwd (writes [n][hd][wd][ld]), tok_dice_fwd and tok_dice_bwd (read it twice, write its
// gradient) and tok_bilinear_bwd (reads the gradient); here the only full-resolution tensor is the fp32 log-sum-exp, 4 bytes a pixel.
//
// Forward.  A block walks WT x WT tiles of destination pixels; per tile it stages the low-resolution footprint in LDS (where it fits
// DICE_FWD_LDS, else the taps come from global memory).  The classes of a pixel lie across a group of G lanes, lane j holding
// classes [8 j, 8 j + 8): the interpolated logits are up_blend8's (tok_bilinear_fwd's stored bf16 values), maximum and sum of
// exponentials are folded over the group with shuffles, and every lane keeps I = sum p y, P = sum p, Y = sum y of its eight
// classes in registers over all the pixels it visits.  Lanes fold to waves by a butterfly, waves to the block through LDS, in a
// fixed order: one partial row [3][classes] per block, folded by loss_dice.hip's finalize into the loss and the coefficients
// coef[2][classes] of d loss / d p = coef[0][c] y + coef[1][c].
//
// Backward.  d(upsampled logit c) = bf16(p_c (dp_c - sum_k p_k dp_k) g) with p = exp(v - lse) of the saved lse: tok_dice_bwd's
// value, evaluated with the same lane group (the dot product is a butterfly over the group).  The adjoint of the interpolation
// takes the two forms of the cross entropy: tiled (a block owns TE x TE low-resolution pixels, stages the d logits of the window
// that can touch them in LDS once, up_adjoint_tile walks it) at destination / source ratios up to 4, gather (adjoint_walk per
// low-resolution pixel) beyond.  No atomics, every sum in a fixed order.
#include "loss_dice.h"
#include "loss_upsample.h"
#include <stdlib.h>

namespace {

constexpr int DICE_FWD_LDS = 16 * 1024;     // footprint of a tile: 7 x 7 pixels at scale 4, 18 x 18 at identity up to ld = 24
constexpr int DICE_ROWS = 1024;             // blocks of the forward = partial rows the one-block finalize folds

// tile edge of the tiled backward: the window of (TE + 1) 4 + 4 pixels squared holds ld channels in at most 100 KB
constexpr int dice_te(int G) { return G <= 4 ? UT : UT / 2; }
constexpr int dice_win(int G) { return (dice_te(G) + 1) * 4 + 4; }

template <int G, bool STAGE>
__global__ __launch_bounds__(256) void updice_fwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target, UpArgs a,
                                                         float* __restrict__ lse, float* __restrict__ partial, int tiles_y,
                                                         int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) char up_smem[];
  __shared__ float red[4][3][64];
  const int j = threadIdx.x & (G - 1);
  const bool lane_on = j * 8 < a.ld;                             // (idle lanes of a group: ld / 8 is no power of two)
  float si[8] = {}, sp[8] = {}, sy[8] = {};
  const int tiles = a.n * tiles_y * tiles_x;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
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
      if (tile != (int)blockIdx.x) __syncthreads();              // the previous tile's taps are read
      up_stage_footprint(src, a, yt0, yt1, xt0, xt1, win, sy0, sx0, fw);
      __syncthreads();
      src = win;
    }
    for (int p = threadIdx.x / G; p < WT * WT; p += 256 / G) {
      // every lane of a group stays in the loop for the shuffles: a pixel outside a partial tile is computed at the tile's
      // edge and neither stored nor counted
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
        v[e] = j * 8 + e < a.classes ? v[e] : -INFINITY;
        mx = fmaxf(mx, v[e]);
      }
#pragma unroll
      for (int off = 1; off < G; off <<= 1) mx = fmaxf(mx, __shfl_xor(mx, off, G));
      float ex[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) ex[e] = j * 8 + e < a.classes ? __expf(v[e] - mx) : 0.f;
      const float s = group_sum<G>(ex, j);
      if (yy > yt1 || xx > xt1) continue;
      const size_t pix = ((size_t)b * a.hd + y) * a.wd + x;
      if (j == 0) lse[pix] = mx + __logf(s);
      // y = (target == class): a label outside [0, classes) matches no lane and contributes to P only, as in dice_fwd_kernel
      const int64_t t = target[pix];
      const float inv = 1.f / s;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float pr = ex[e] * inv, yv = t == (int64_t)(j * 8 + e) ? 1.f : 0.f;
        si[e] = fmaf(pr, yv, si[e]);
        sp[e] += pr;
        sy[e] += yv;
      }
    }
  }
  // lanes of the same class group -> wave (butterfly over the 64 / G groups), waves -> block through LDS in wave order
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
#pragma unroll
    for (int off = G; off < 64; off <<= 1) {
      si[e] += __shfl_xor(si[e], off, 64);
      sp[e] += __shfl_xor(sp[e], off, 64);
      sy[e] += __shfl_xor(sy[e], off, 64);
    }
    if (lane < G) { red[wv][0][lane * 8 + e] = si[e]; red[wv][1][lane * 8 + e] = sp[e]; red[wv][2][lane * 8 + e] = sy[e]; }
  }
  __syncthreads();
  if (threadIdx.x < 3 * 64) {
    const int which = threadIdx.x / 64, c = threadIdx.x & 63;
    if (c < a.classes)
      partial[((size_t)blockIdx.x * 3 + which) * a.classes + c] = red[0][which][c] + red[1][which][c] + red[2][which][c] + red[3][which][c];
  }
}

// The lane's two coefficient vectors (0 beyond the classes)
__device__ __forceinline__ void updice_coef(const float* __restrict__ coef, int classes, int j, float (&ca)[8], float (&cb)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = j * 8 + e;
    ca[e] = c < classes ? coef[c] : 0.f;
    cb[e] = c < classes ? coef[classes + c] : 0.f;
  }
}

// d(upsampled logits) of full-resolution pixel (b, yd, xd) for the lane's classes [8 j, 8 j + 8), rounded to bf16 as tok_dice_bwd
// stores it.  Every lane of the group calls it together (the dot product is folded over the group).
template <int G>
__device__ __forceinline__ void updice_dlogits(const bf16* __restrict__ low, const int64_t* __restrict__ target, const UpArgs& a,
                                               const float* __restrict__ lse, const float (&ca)[8], const float (&cb)[8], float g,
                                               int b, int yd, int xd, int j, bool lane_on, float* d) {
  const size_t dp = ((size_t)b * a.hd + yd) * a.wd + xd;
  const int64_t t = target[dp];
  const float l = lse[dp];
  float v[8] = {};
  if (lane_on) up_logits<1>(low + j * 8, a, b, yd, xd, v);
  float pr[8], dpv[8], dot = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = j * 8 + e;
    pr[e] = c < a.classes ? __expf(v[e] - l) : 0.f;
    dpv[e] = (t == (int64_t)c ? ca[e] : 0.f) + cb[e];
    dot = fmaf(pr[e], dpv[e], dot);
  }
#pragma unroll
  for (int off = 1; off < G; off <<= 1) dot += __shfl_xor(dot, off, G);
#pragma unroll
  for (int e = 0; e < 8; ++e) d[e] = bf2f(f2bf(pr[e] * (dpv[e] - dot) * g));     // (p = 0 beyond the classes: 0)
}

template <int G>
__global__ __launch_bounds__(256) void updice_bwd_tiled_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target,
                                                               UpArgs a, const float* __restrict__ lse,
                                                               const float* __restrict__ coef, const float* __restrict__ gscale,
                                                               bf16* dlow, int accumulate, int tiles_y, int tiles_x) {
  extern __shared__ __attribute__((aligned(16))) char up_smem[];
  bf16* win = reinterpret_cast<bf16*>(up_smem);                 // [wh][ww][ld]
  const UpTile tl = up_tile<dice_te(G)>(a, tiles_y, tiles_x);   // wh, ww <= dice_win(G)
  const int j = threadIdx.x & (G - 1);
  const bool lane_on = j * 8 < a.ld;
  const float g = gscale ? gscale[0] : 1.f;
  float ca[8], cb[8];
  updice_coef(coef, a.classes, j, ca, cb);
  // ---- phase 1: bf16(d upsampled logits) of the window, a lane group per pixel (the last pass repeats the last pixel) -----------
  const int npix = tl.wh * tl.ww;
  for (int i0 = 0; i0 < npix; i0 += 256 / G) {
    const int i = i0 + threadIdx.x / G, ii = min(i, npix - 1);
    float d[8];
    updice_dlogits<G>(low, target, a, lse, ca, cb, g, tl.b, tl.wy0 + ii / tl.ww, tl.wx0 + ii % tl.ww, j, lane_on, d);
    if (i < npix && lane_on) {
      bf16x8 q;
#pragma unroll
      for (int e = 0; e < 8; ++e) q[e] = f2bf(d[e]);
      *reinterpret_cast<bf16x8*>(win + (size_t)i * a.ld + j * 8) = q;
    }
  }
  __syncthreads();
  // ---- phase 2: the adjoint of the interpolation, one (low-resolution pixel, 8-channel group) per thread ------------------------
  up_adjoint_tile<dice_te(G)>(win, a, tl, a.ld >> 3, dlow, accumulate, 0);
}

// The gather form: a lane group per low-resolution pixel walks the full-resolution pixels whose footprint contains it.  The lanes
// of a group share every branch of the walk, so the group's shuffles find all their lanes.
template <int G>
__global__ __launch_bounds__(256) void updice_bwd_kernel(const bf16* __restrict__ low, const int64_t* __restrict__ target, UpArgs a,
                                                         const float* __restrict__ lse, const float* __restrict__ coef,
                                                         const float* __restrict__ gscale, bf16* dlow, int accumulate) {
  const size_t total = (size_t)a.n * a.hs * a.ws;
  const int j = threadIdx.x & (G - 1);
  const bool lane_on = j * 8 < a.ld;
  const float g = gscale ? gscale[0] : 1.f;
  float ca[8], cb[8];
  updice_coef(coef, a.classes, j, ca, cb);
  for (size_t p0 = (size_t)blockIdx.x * (256 / G); p0 < total; p0 += (size_t)gridDim.x * (256 / G)) {
    const size_t pix = p0 + threadIdx.x / G;
    const bool live = pix < total;
    int xs, ys, b;
    split_pixel(live ? pix : total - 1, a.ws, a.hs, xs, ys, b);
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.f;
    adjoint_walk(a.sh, a.sw, a.hs, a.ws, a.hd, a.wd, ys, xs, [&](int yd, int xd, float wgt) TOK_ROW_INLINE {
      float d[8];
      updice_dlogits<G>(low, target, a, lse, ca, cb, g, b, yd, xd, j, lane_on, d);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, d[e], acc[e]);
    });
    if (live && lane_on) store_acc<8>(dlow + pix * a.ld + j * 8, acc, accumulate);
  }
}

}  // namespace

extern "C" int tok_upsample_dice_serves(int classes, int ld) { return classes > 0 && ld >= classes && (ld & 7) == 0 && ld <= 64; }

extern "C" int tok_upsample_dice_rows(int n, int hd, int wd) {
  TOK_CHECK_ARG(n > 0 && hd > 0 && wd > 0, "tok_upsample_dice_rows: bad args");
  const long long tiles = (long long)n * tok_cdiv(hd, WT) * tok_cdiv(wd, WT);
  return (int)(tiles < DICE_ROWS ? tiles : DICE_ROWS);
}

extern "C" int tok_upsample_dice_fwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                     const int64_t* target, float smooth, float eps, int log_loss, const int64_t* class_sel,
                                     int n_sel, float* lse, float* partial, float* loss, float* coef, void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && partial && loss && coef && fill_up(a, n, hs, ws, classes, ld, hd, wd, 64),
                "tok_upsample_dice_fwd: bad args (row pitch a multiple of 8 up to 64 channels, n*hd*wd < 2^31)");
  TOK_CHECK_ARG(tok_aligned(low, 16), "tok_upsample_dice_fwd: low must be 16-byte aligned");
  TOK_CHECK_ARG(!class_sel || n_sel > 0, "tok_upsample_dice_fwd: empty class selection");
  hipStream_t st = tok_stream(stream);
  const int tiles_y = tok_cdiv(hd, WT), tiles_x = tok_cdiv(wd, WT);
  const int rows = tok_upsample_dice_rows(n, hd, wd);
  const size_t bytes = (size_t)wide_footprint(a.sh, hs) * wide_footprint(a.sw, ws) * ld * 2;
  with_group(ld >> 3, [&](auto gr) {
    constexpr int G = decltype(gr)::value < 8 ? decltype(gr)::value : 8;
    if (bytes <= (size_t)DICE_FWD_LDS)
      hipLaunchKernelGGL((updice_fwd_kernel<G, true>), dim3(rows), dim3(256), bytes, st, (const bf16*)low, target, a, lse, partial,
                         tiles_y, tiles_x);
    else
      hipLaunchKernelGGL((updice_fwd_kernel<G, false>), dim3(rows), dim3(256), 0, st, (const bf16*)low, target, a, lse, partial,
                         tiles_y, tiles_x);
  });
  TOK_CHECK_LAUNCH("tok_upsample_dice_fwd");
  return dice_finalize_launch("tok_upsample_dice_fwd", partial, rows, classes, smooth, eps, log_loss, class_sel, n_sel, loss, coef, st);
}

extern "C" int tok_upsample_dice_bwd(const void* low, int n, int hs, int ws, int classes, int ld, int hd, int wd,
                                     const int64_t* target, const float* lse, const float* coef, const float* gscale, void* dlow,
                                     int accumulate, void* stream) {
  UpArgs a;
  TOK_CHECK_ARG(low && target && lse && coef && dlow && fill_up(a, n, hs, ws, classes, ld, hd, wd, 64), "tok_upsample_dice_bwd: bad args");
  TOK_CHECK_ARG(tok_aligned(low, 16) && tok_aligned(dlow, 16), "tok_upsample_dice_bwd: low / dlow must be 16-byte aligned");
  hipStream_t st = tok_stream(stream);
  const bool tiled = up_tiled_ok(a);     // ratio <= 4, whatever the tile edge: the window is (TE + 1) r + 4 wide
  with_group(ld >> 3, [&](auto gr) {
    constexpr int G = decltype(gr)::value < 8 ? decltype(gr)::value : 8;
    if (tiled) {
      constexpr int TE = dice_te(G), LDS = dice_win(G) * dice_win(G) * G * 16;
      const int tiles_y = tok_cdiv(hs, TE), tiles_x = tok_cdiv(ws, TE);
      tok_launch_lds<&updice_bwd_tiled_kernel<G>>(LDS, dim3(n * tiles_y * tiles_x), dim3(256), (size_t)dice_win(G) * dice_win(G) * ld * 2,
                                                  st, (const bf16*)low, target, a, lse, coef, gscale, (bf16*)dlow, accumulate, tiles_y,
                                                  tiles_x);
    } else {
      hipLaunchKernelGGL(updice_bwd_kernel<G>, dim3(grid_for((size_t)n * hs * ws * G)), dim3(256), 0, st, (const bf16*)low, target, a,
                         lse, coef, gscale, (bf16*)dlow, accumulate);
    }
  });
  TOK_CHECK_LAUNCH("tok_upsample_dice_bwd");
  return TOK_OK;
}
