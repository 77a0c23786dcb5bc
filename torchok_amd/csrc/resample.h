// The rules of the resampling kernels, written once (resample.hip, neck_resample.hip, fuse_sum.hip, loss_upsample_ce.hip): the
// align_corners=False source index, the adjoint's destination window, weight and walk, the accumulate-and-store epilogue and the
// argument block of the gather entries.  The fused upsample cross-entropy promises tok_bilinear_fwd's bits and the backward
// passes promise to be exact transposes of their forwards: both rest on every kernel going through THESE functions.
// Everything is force-inlined; taps are lambdas (TOK_ROW_INLINE behind the parameter list), as in row_stream.h.
#pragma once
#include "tok_common.h"

// ATen area_pixel_compute_source_index(scale, dst, align_corners=false, cubic=false)
__device__ __forceinline__ void src_index(float scale, int dst, int in_size, int& i0, int& i1, float& l1) {
  float s = scale * ((float)dst + 0.5f) - 0.5f;
  s = s < 0.f ? 0.f : s;
  i0 = (int)s;
  i0 = i0 > in_size - 1 ? in_size - 1 : i0;
  i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
  l1 = s - (float)i0;
}

// Destination indices [d0, d1] that can read source index s, r = out / in: those with source coordinate in (s - 1, s + 1),
// widened by one for rounding; source index 0 also owns the clamp.
__device__ __forceinline__ void adj_window(float r, int s, int n_dst, int& d0, int& d1) {
  d0 = s == 0 ? 0 : (int)floorf(((float)s - 0.5f) * r - 0.5f) - 1;
  d1 = (int)ceilf(((float)s + 1.5f) * r - 0.5f) + 1;
  d0 = d0 < 0 ? 0 : d0;
  d1 = d1 > n_dst - 1 ? n_dst - 1 : d1;
}

// Weight of source index s in destination index d: the forward's own index and weight (same src_index), so forward and
// backward are transposes bit for bit.
__device__ __forceinline__ float adj_weight(float scale, int d, int in_size, int s) {
  int i0, i1;
  float l;
  src_index(scale, d, in_size, i0, i1, l);
  return (i0 == s ? 1.f - l : 0.f) + (i1 == s ? l : 0.f);
}

// The adjoint as a gather: source pixel (ys, xs) visits the destination pixels of its window, rows outside then columns inside,
// skipping zero weights: tap(yd, xd, wy * wx).  Deterministic, no atomics.
template <class Tap>
__device__ __forceinline__ void adjoint_walk(float sh, float sw, int hs, int ws, int hd, int wd, int ys, int xs, Tap&& tap) {
  int yd0, yd1, xd0, xd1;
  adj_window(1.f / sh, ys, hd, yd0, yd1);
  adj_window(1.f / sw, xs, wd, xd0, xd1);
  for (int yd = yd0; yd <= yd1; ++yd) {
    const float wy = adj_weight(sh, yd, hs, ys);
    if (wy == 0.f) continue;
    for (int xd = xd0; xd <= xd1; ++xd) {
      const float wx = adj_weight(sw, xd, ws, xs);
      if (wx == 0.f) continue;
      tap(yd, xd, wy * wx);
    }
  }
}

// pixel index of an [n][h][w] map -> (b, y, x)
__device__ __forceinline__ void split_pixel(size_t pix, int w, int h, int& x, int& y, int& b) {
  x = (int)(pix % w);
  const size_t t2 = pix / w;
  y = (int)(t2 % h);
  b = (int)(t2 / h);
}

// V = 8: one lane moves 16 bytes; V = 1: one element (channel counts, pitches or offsets that are no multiple of 8, such as the
// 18 + 36 + 72 + 144 = 270 concat channels of HRNet-W18)
template <int V>
using bf16v = __bf16 __attribute__((ext_vector_type(V)));
template <int V>
__device__ __forceinline__ bf16v<V> ldv(const bf16* p) {
  // (V = 1 as a scalar load: behind a one-element vector load hipcc contracted the scalar forward's blend differently)
  if constexpr (V == 1) { bf16v<1> r; r[0] = *p; return r; }
  else return *reinterpret_cast<const bf16v<V>*>(p);
}
template <int V>
__device__ __forceinline__ void stv(bf16* p, bf16v<V> v) { *reinterpret_cast<bf16v<V>*>(p) = v; }

// *d = bf16(acc (+ *d if accumulate)): the fp32 sum takes the previous value LAST and is rounded once
template <int V>
__device__ __forceinline__ void store_acc(bf16* d, const float (&acc)[V], int accumulate) {
  bf16v<V> o;
  if (accumulate) {
    const bf16v<V> prev = ldv<V>(d);
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = f2bf(acc[e] + bf2f(prev[e]));
  } else {
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = f2bf(acc[e]);
  }
  stv<V>(d, o);
}

// ---- host side of the gather entries (bilinear and nearest, forward and backward) -----------------------------------------------
struct ResampleArgs {
  int n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off;
  float sh, sw;   // in / out
};

inline bool fill_resample(ResampleArgs& a, int n, int hs, int ws, int c, int ld_src, int hd, int wd, int ld_dst, int ch_off) {
  if (n <= 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0 || c <= 0 || ch_off < 0 || ld_src < c || ld_dst < ch_off + c)
    return false;
  a.n = n; a.hs = hs; a.ws = ws; a.c = c; a.ld_src = ld_src; a.hd = hd; a.wd = wd; a.ld_dst = ld_dst; a.ch_off = ch_off;
  a.sh = (float)hs / (float)hd;
  a.sw = (float)ws / (float)wd;
  return true;
}

inline bool vec_ok(const ResampleArgs& a) { return !((a.c | a.ld_src | a.ld_dst | a.ch_off) & 7); }

// blocks of a grid-strided pass of 256-thread blocks over `total` items
inline int grid_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}
