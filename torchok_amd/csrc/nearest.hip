// Nearest-neighbour resample into a channel slice, NHWC bf16 (the U-Net decoder, necks/segmentation/unet.py:
//   x = F.interpolate(x, scale_factor=2, mode='nearest'); skip = F.interpolate(skip, size=x.shape[2:]) when the heights
//   differ; x = torch.cat([x, skip], dim=1)): every source is written straight into its slice of the concat buffer.
// The forward is a copy (bit for bit the source values), the backward its exact transpose in gather form (deterministic, no
// atomics).  Both are HBM streaming kernels of the resample.hip kind: one lane per (pixel, 8-channel group), 16 bytes per
// lane, or one lane per element when a channel count, pitch or slice offset is no multiple of 8.  Offsets are 64-bit.
#include "tok_common.h"

namespace {

struct NearArgs {
  int n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off;
  float sh, sw;   // in / out
};

// ATen nearest_neighbor_compute_source_index(scale, dst, in_size): min(floor(dst * scale), in_size - 1)
__device__ __forceinline__ int near_index(float scale, int dst, int in_size) {
  const int i = (int)floorf((float)dst * scale);
  return i < in_size - 1 ? i : in_size - 1;
}

// First destination index whose source index is >= s (out_size when there is none).  near_index is monotone in dst, so the
// preimage of s is [near_first(s), near_first(s + 1)).  The estimate ceil(s / scale) is off by a rounding step at most; the
// two walks settle it against near_index itself, so forward and backward agree bit for bit.
__device__ __forceinline__ int near_first(float scale, float rscale, int s, int in_size, int out_size) {
  if (s <= 0) return 0;
  if (s >= in_size) return out_size;
  // the decoder's two cases need no search: at scale 1 and 0.5 near_index is d and d >> 1 exactly (while fp32 holds d)
  if (out_size <= (1 << 24) && out_size == in_size) return s;
  if (out_size <= (1 << 24) && out_size == 2 * in_size) return 2 * s;
  int g = (int)ceilf((float)s * rscale);
  g = g < 0 ? 0 : (g > out_size ? out_size : g);
  while (g > 0 && near_index(scale, g - 1, in_size) >= s) --g;
  while (g < out_size && near_index(scale, g, in_size) < s) ++g;
  return g;
}

// V = 8: one lane moves 16 bytes; V = 1: one element (same index math)
template <int V>
__global__ __launch_bounds__(256) void nearest_fwd_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, NearArgs a) {
  const int cgs = a.c / V;
  const size_t total = (size_t)a.n * a.hd * a.wd * cgs;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    const int x = (int)(pix % a.wd);
    const size_t t2 = pix / a.wd;
    const int y = (int)(t2 % a.hd);
    const int b = (int)(t2 / a.hd);
    const int ys = near_index(a.sh, y, a.hs), xs = near_index(a.sw, x, a.ws);
    const bf16* s = src + (((size_t)b * a.hs + ys) * a.ws + xs) * a.ld_src + cg * V;
    bf16* d = dst + pix * a.ld_dst + a.ch_off + cg * V;
    if constexpr (V == 8) stg16(d, ldg16(s));
    else *d = *s;
  }
}

// d src[b][ys][xs][:] (+)= sum of d dst over the preimage rectangle, in row-major order of dst, fp32, rounded once
template <int V>
__global__ __launch_bounds__(256) void nearest_bwd_kernel(const bf16* __restrict__ ddst, bf16* dsrc, NearArgs a, int accumulate) {
  const int cgs = a.c / V;
  const size_t total = (size_t)a.n * a.hs * a.ws * cgs;
  const float rh = 1.f / a.sh, rw = 1.f / a.sw;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    const int xs = (int)(pix % a.ws);
    const size_t t2 = pix / a.ws;
    const int ys = (int)(t2 % a.hs);
    const int b = (int)(t2 / a.hs);
    const int yd0 = near_first(a.sh, rh, ys, a.hs, a.hd), yd1 = near_first(a.sh, rh, ys + 1, a.hs, a.hd);
    const int xd0 = near_first(a.sw, rw, xs, a.ws, a.wd), xd1 = near_first(a.sw, rw, xs + 1, a.ws, a.wd);
    bf16* d = dsrc + pix * a.ld_src + cg * V;
    float acc[V];
    if constexpr (V == 8) {
      if (accumulate) {
        const bf16x8 prev = ldg16(d);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = bf2f(prev[e]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = 0.f;
      }
    } else {
      acc[0] = accumulate ? bf2f(*d) : 0.f;
    }
    for (int yd = yd0; yd < yd1; ++yd) {
      const bf16* g = ddst + (((size_t)b * a.hd + yd) * a.wd + xd0) * a.ld_dst + a.ch_off + cg * V;
      for (int xd = xd0; xd < xd1; ++xd, g += a.ld_dst) {
        if constexpr (V == 8) {
          const bf16x8 v = ldg16(g);
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[e] += bf2f(v[e]);
        } else {
          acc[0] += bf2f(*g);
        }
      }
    }
    if constexpr (V == 8) {
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[e]);
      stg16(d, o);
    } else {
      *d = f2bf(acc[0]);
    }
  }
}

inline int blocks_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

bool fill_near(NearArgs& a, int n, int hs, int ws, int c, int ld_src, int hd, int wd, int ld_dst, int ch_off) {
  if (n <= 0 || hs <= 0 || ws <= 0 || hd <= 0 || wd <= 0 || c <= 0 || ch_off < 0 || ld_src < c || ld_dst < ch_off + c)
    return false;
  a.n = n; a.hs = hs; a.ws = ws; a.c = c; a.ld_src = ld_src; a.hd = hd; a.wd = wd; a.ld_dst = ld_dst; a.ch_off = ch_off;
  a.sh = (float)hs / (float)hd;
  a.sw = (float)ws / (float)wd;
  return true;
}

inline bool vec_ok(const NearArgs& a) { return !((a.c | a.ld_src | a.ld_dst | a.ch_off) & 7); }

}  // namespace

extern "C" int tok_nearest_fwd(const void* src, int n, int hs, int ws, int c, int ld_src, void* dst, int hd, int wd,
                               int ld_dst, int ch_off, void* stream) {
  NearArgs a;
  TOK_CHECK_ARG(src && dst && fill_near(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_nearest_fwd: bad args");
  if (vec_ok(a))
    hipLaunchKernelGGL(nearest_fwd_kernel<8>, dim3(blocks_for((size_t)n * hd * wd * (c >> 3))), dim3(256), 0,
                       tok_stream(stream), (const bf16*)src, (bf16*)dst, a);
  else
    hipLaunchKernelGGL(nearest_fwd_kernel<1>, dim3(blocks_for((size_t)n * hd * wd * c)), dim3(256), 0,
                       tok_stream(stream), (const bf16*)src, (bf16*)dst, a);
  TOK_CHECK_LAUNCH("tok_nearest_fwd");
  return TOK_OK;
}

extern "C" int tok_nearest_bwd(const void* ddst, int n, int hd, int wd, int ld_dst, int ch_off, void* dsrc, int hs,
                               int ws, int c, int ld_src, int accumulate, void* stream) {
  NearArgs a;
  TOK_CHECK_ARG(ddst && dsrc && fill_near(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_nearest_bwd: bad args");
  if (vec_ok(a))
    hipLaunchKernelGGL(nearest_bwd_kernel<8>, dim3(blocks_for((size_t)n * hs * ws * (c >> 3))), dim3(256), 0,
                       tok_stream(stream), (const bf16*)ddst, (bf16*)dsrc, a, accumulate);
  else
    hipLaunchKernelGGL(nearest_bwd_kernel<1>, dim3(blocks_for((size_t)n * hs * ws * c)), dim3(256), 0,
                       tok_stream(stream), (const bf16*)ddst, (bf16*)dsrc, a, accumulate);
  TOK_CHECK_LAUNCH("tok_nearest_bwd");
  return TOK_OK;
}
