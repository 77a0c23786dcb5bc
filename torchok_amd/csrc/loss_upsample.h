// What the losses on bilinearly upsampled logits share (loss_upsample_ce.hip, loss_upsample_dice.hip): the argument block, the
// blend that gives tok_bilinear_fwd's bits, the lane-group sum of the forward kernels, the tile and window geometry of the tiled
// adjoint and its phase 2 (the walk over a window of bf16(d upsampled logits) staged in LDS).  The index and weight rules are
// resample.h's.
#pragma once
#include "resample.h"
#include <math.h>
#include <type_traits>

namespace {

struct UpArgs {
  int n, hs, ws, classes, ld, hd, wd;
  float sh, sw;     // in / out
};

// eight interpolated logits from the four corners' vectors, rounded to bf16 as tok_bilinear_fwd stores them: the ONE text of
// the blend hy (hx a + lx b) + ly (hx c + lx d) for the narrow and the wide kernels, with every rounding written out.  Left to
// the compiler, the contraction into fused multiply-adds differs from kernel to kernel (the packed form of the wide forward
// fused the other product of some elements), and at dyadic weights the bf16 rounding behind it sits on ties: the wide entries
// would not give the narrow entries' bits.  The form below is the one hipcc chose for the narrow kernels.
__device__ __forceinline__ void up_blend8(float hy, float ly, float hx, float lx, bf16x8 v00, bf16x8 v01, bf16x8 v10, bf16x8 v11,
                                          float* v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float u = fmaf(lx, bf2f(v01[e]), hx * bf2f(v00[e])), w = fmaf(lx, bf2f(v11[e]), hx * bf2f(v10[e]));
    v[e] = bf2f(f2bf(fmaf(hy, u, ly * w)));
  }
}

// interpolated, bf16-rounded logits of full-resolution pixel (b, y, x): v[0 .. 8 NV), from channel 0 of `low` on (a chunk of the
// wide backward hands in low + its first channel)
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
    up_blend8(hy, ly, hx, lx, ldg16(p00 + i * 8), ldg16(p01 + i * 8), ldg16(p10 + i * 8), ldg16(p11 + i * 8), v + i * 8);
  }
}

// ---- the tiled adjoint: a block owns TE x TE low-resolution pixels and stages bf16(d upsampled logits) of the full-resolution
// window that can touch them in LDS; window = the union of the per-pixel windows of the gather form -----------------------------
constexpr int UT = 8, UWIN = 40, UPP = 12;     // tile edge, window edge, window of ONE source pixel (2 r + 4 at r <= 4)

// window of UT source pixels at destination/source ratio r: (UT - 1) r between first and last pixel + (2 r + 4) per pixel
inline bool up_tiled_ok(const UpArgs& a) {
  const float r = fmaxf(1.f / a.sh, 1.f / a.sw);
  return (int)ceilf((UT + 1) * r) + 4 <= UWIN;
}

struct UpTile {
  int b, ys0, xs0, ys1, xs1;     // image, first and last low-resolution pixel of the tile
  int wy0, wx0, wh, ww;          // the window: origin and extent in full-resolution pixels
  float rh, rw;                  // out / in
};

// tile blockIdx.x of a grid of n x tiles_y x tiles_x tiles of edge TE
template <int TE>
__device__ __forceinline__ UpTile up_tile(const UpArgs& a, int tiles_y, int tiles_x) {
  UpTile t;
  const int tile = blockIdx.x;
  const int tx = tile % tiles_x;
  const int t2 = tile / tiles_x;
  const int ty = t2 % tiles_y;
  t.b = t2 / tiles_y;
  t.ys0 = ty * TE, t.xs0 = tx * TE;
  t.ys1 = min(a.hs, t.ys0 + TE) - 1, t.xs1 = min(a.ws, t.xs0 + TE) - 1;
  t.rh = 1.f / a.sh, t.rw = 1.f / a.sw;
  int wy1, wx1, tmp0, tmp1;
  adj_window(t.rh, t.ys0, a.hd, t.wy0, tmp1);
  adj_window(t.rh, t.ys1, a.hd, tmp0, wy1);
  adj_window(t.rw, t.xs0, a.wd, t.wx0, tmp1);
  adj_window(t.rw, t.xs1, a.wd, tmp0, wx1);
  t.wh = wy1 - t.wy0 + 1, t.ww = wx1 - t.wx0 + 1;     // <= (TE + 1) r + 4 (checked by the launcher for the scale)
  return t;
}

// phase 2: the adjoint of the interpolation from the window win[wh][ww][8 nv], one (low-resolution pixel, 8-channel group) per
// thread, tok_bilinear_bwd's exact index / weight arithmetic; dlow channels [c0, c0 + 8 nv)
template <int TE>
__device__ __forceinline__ void up_adjoint_tile(const bf16* win, const UpArgs& a, const UpTile& t, int nv, bf16* dlow, int accumulate,
                                                int c0) {
  for (int i = threadIdx.x; i < TE * TE * nv; i += 256) {
    const int v8 = i % nv;
    const int p = i / nv;
    const int ys = t.ys0 + p / TE, xs = t.xs0 + p % TE;
    if (ys > t.ys1 || xs > t.xs1) continue;
    int yd0, yd1, xd0, xd1;
    adj_window(t.rh, ys, a.hd, yd0, yd1);
    adj_window(t.rw, xs, a.wd, xd0, xd1);
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
      const bf16* rowp = win + ((size_t)(yd - t.wy0) * t.ww + (xd0 - t.wx0)) * (8 * nv) + v8 * 8;
#pragma unroll
      for (int j = 0; j < UPP; ++j) {
        if (wxs[j] == 0.f) continue;
        const bf16x8 q = *reinterpret_cast<const bf16x8*>(rowp + (size_t)j * (8 * nv));
        const float wgt = wy * wxs[j];
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf(wgt, bf2f(q[e]), acc[e]);
      }
    }
    store_acc<8>(dlow + (((size_t)t.b * a.hs + ys) * a.ws + xs) * a.ld + c0 + v8 * 8, acc, accumulate);
  }
}

// ---- the forward with the classes ACROSS lanes: a group of G lanes (the power of two >= ld / 8) owns one full-resolution pixel,
// lane j holds the 16-byte vector of classes [8 j, 8 j + 8); a block owns a WT x WT tile of destination pixels ---------------------
constexpr int WT = 16;

// Sum of the group's exponentials.  Inside a block of 32 classes the four lanes hand a running sum on, lane 0 first, each adding
// its eight values in class order: the narrow kernel's sequential sum.  The blocks of 32 are folded by a butterfly.
template <int G>
__device__ __forceinline__ float group_sum(const float (&ex)[8], int j) {
  constexpr int Q = G < 4 ? G : 4;
  float run = 0.f;
#pragma unroll
  for (int step = 0; step < Q; ++step) {
    const float prev = step ? __shfl_up(run, 1, Q) : 0.f;
    if ((j & (Q - 1)) == step) {
      float s = prev;
#pragma unroll
      for (int e = 0; e < 8; ++e) s += ex[e];
      run = s;
    }
  }
  float s = __shfl(run, Q - 1, Q);
#pragma unroll
  for (int off = Q; off < G; off <<= 1) s += __shfl_xor(s, off, G);
  return s;
}

// The low-resolution footprint [fh][fw][ld] of destination pixels [yt0, yt1] x [xt0, xt1] of image `src` into LDS with 16-byte
// loads; origin and width of the footprint come back.  src_index is monotone in the destination index: the footprint runs from
// the first pixel's i0 to the last pixel's i1.  (The caller's barrier follows.)
__device__ __forceinline__ void up_stage_footprint(const bf16* __restrict__ src, const UpArgs& a, int yt0, int yt1, int xt0, int xt1,
                                                   bf16* win, int& sy0, int& sx0, int& fw) {
  int sy1, sx1, tmp;
  float l;
  src_index(a.sh, yt0, a.hs, sy0, tmp, l);
  src_index(a.sh, yt1, a.hs, tmp, sy1, l);
  src_index(a.sw, xt0, a.ws, sx0, tmp, l);
  src_index(a.sw, xt1, a.ws, tmp, sx1, l);
  fw = sx1 - sx0 + 1;
  const int nv = a.ld >> 3;
  for (int i = threadIdx.x; i < (sy1 - sy0 + 1) * fw * nv; i += 256) {
    const int p = i / nv, v8 = i - p * nv;
    const int fy = p / fw, fx = p - fy * fw;
    *reinterpret_cast<bf16x8*>(win + (size_t)p * a.ld + v8 * 8) = ldg16(src + ((size_t)(sy0 + fy) * a.ws + sx0 + fx) * a.ld + v8 * 8);
  }
}

// Source pixels along one axis that WT destination pixels can touch, scale = in / out: floor(s) moves by at most
// ceil((WT - 1) scale) + 1 between the first and the last pixel (the +1: fp32 rounding of the coordinate), one more for the last
// pixel's i1, one for the count.
inline int wide_footprint(float scale, int n_src) {
  const int f = (int)ceilf((WT - 1) * scale) + 3;
  return f < n_src ? f : n_src;
}

inline bool fill_up(UpArgs& a, int n, int hs, int ws, int classes, int ld, int hd, int wd, int max_ld = 32) {
  if (n <= 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0 || classes <= 0 || ld < classes || (ld & 7) || ld > max_ld) return false;
  if ((long long)n * hd * wd >= (1ll << 31)) return false;
  a.n = n; a.hs = hs; a.ws = ws; a.classes = classes; a.ld = ld; a.hd = hd; a.wd = wd;
  a.sh = (float)hs / (float)hd; a.sw = (float)ws / (float)wd;
  return true;
}

// f(G as a compile-time constant): the lane group of a row of nv = ld / 8 = 1 .. 32 vectors, the power of two >= nv
template <class F>
void with_group(int nv, F&& f) {
  if (nv <= 1) f(std::integral_constant<int, 1>());
  else if (nv <= 2) f(std::integral_constant<int, 2>());
  else if (nv <= 4) f(std::integral_constant<int, 4>());
  else if (nv <= 8) f(std::integral_constant<int, 8>());
  else if (nv <= 16) f(std::integral_constant<int, 16>());
  else f(std::integral_constant<int, 32>());
}

}  // namespace
