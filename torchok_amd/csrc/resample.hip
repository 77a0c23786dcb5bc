// Resampling into a channel slice, NHWC bf16: one lane per (pixel, 8-channel group) and 16 bytes per lane, or one lane per
// element when a channel count, pitch or slice offset is no multiple of 8 (same index math).  Offsets are 64-bit.
//   bilinear fwd/bwd   F.interpolate(mode='bilinear', align_corners=False): HRNetSegmentationNeck
//                      (necks/segmentation/hrnet.py:36-39, written straight into its slice of the concat buffer, :41)
//                      and SegmentationHead (heads/segmentation/base.py:37)
//   nearest fwd/bwd    the U-Net decoder (necks/segmentation/unet.py: x = F.interpolate(x, scale_factor=2, mode='nearest');
//                      skip = F.interpolate(skip, size=x.shape[2:]) when the heights differ; x = torch.cat([x, skip], dim=1)):
//                      every source is written straight into its slice of the concat buffer
// All four are HBM streaming kernels; the backward passes are gathers (deterministic, no atomics), exact transposes of their
// forwards.  The bilinear rules live in resample.h.
#include "resample.h"

namespace {

template <int V>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst,
                                                           ResampleArgs a) {
  const int cgs = V == 8 ? a.c >> 3 : a.c;
  const size_t total = (size_t)a.n * a.hd * a.wd * cgs;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    int x, y, b, y0, y1, x0, x1;
    float ly, lx;
    split_pixel(pix, a.wd, a.hd, x, y, b);
    src_index(a.sh, y, a.hs, y0, y1, ly);
    src_index(a.sw, x, a.ws, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const bf16* base = src + (size_t)b * a.hs * a.ws * a.ld_src + cg * V;
    const bf16v<V> v00 = ldv<V>(base + ((size_t)y0 * a.ws + x0) * a.ld_src);
    const bf16v<V> v01 = ldv<V>(base + ((size_t)y0 * a.ws + x1) * a.ld_src);
    const bf16v<V> v10 = ldv<V>(base + ((size_t)y1 * a.ws + x0) * a.ld_src);
    const bf16v<V> v11 = ldv<V>(base + ((size_t)y1 * a.ws + x1) * a.ld_src);
    bf16v<V> o;
#pragma unroll
    for (int e = 0; e < V; ++e)
      o[e] = f2bf(hy * (hx * bf2f(v00[e]) + lx * bf2f(v01[e])) + ly * (hx * bf2f(v10[e]) + lx * bf2f(v11[e])));
    stv<V>(dst + pix * a.ld_dst + a.ch_off + cg * V, o);
  }
}

template <int V>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const bf16* __restrict__ ddst, bf16* dsrc, ResampleArgs a,
                                                           int accumulate) {
  const int cgs = V == 8 ? a.c >> 3 : a.c;
  const size_t total = (size_t)a.n * a.hs * a.ws * cgs;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    int xs, ys, b;
    split_pixel(pix, a.ws, a.hs, xs, ys, b);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    adjoint_walk(a.sh, a.sw, a.hs, a.ws, a.hd, a.wd, ys, xs, [&](int yd, int xd, float wgt) TOK_ROW_INLINE {
      const bf16v<V> g = ldv<V>(ddst + (((size_t)b * a.hd + yd) * a.wd + xd) * a.ld_dst + a.ch_off + cg * V);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = fmaf(wgt, bf2f(g[e]), acc[e]);
    });
    store_acc<V>(dsrc + pix * a.ld_src + cg * V, acc, accumulate);
  }
}

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

// a copy: bit for bit the source values
template <int V>
__global__ __launch_bounds__(256) void nearest_fwd_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, ResampleArgs a) {
  const int cgs = a.c / V;
  const size_t total = (size_t)a.n * a.hd * a.wd * cgs;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    int x, y, b;
    split_pixel(pix, a.wd, a.hd, x, y, b);
    const int ys = near_index(a.sh, y, a.hs), xs = near_index(a.sw, x, a.ws);
    const bf16* s = src + (((size_t)b * a.hs + ys) * a.ws + xs) * a.ld_src + cg * V;
    bf16* d = dst + pix * a.ld_dst + a.ch_off + cg * V;
    stv<V>(d, ldv<V>(s));
  }
}

// d src[b][ys][xs][:] (+)= sum of d dst over the preimage rectangle, in row-major order of dst, fp32, rounded once.  The sum
// STARTS from the previous value (store_acc adds it last: another rounding order), so this kernel keeps its own epilogue.
template <int V>
__global__ __launch_bounds__(256) void nearest_bwd_kernel(const bf16* __restrict__ ddst, bf16* dsrc, ResampleArgs a, int accumulate) {
  const int cgs = a.c / V;
  const size_t total = (size_t)a.n * a.hs * a.ws * cgs;
  const float rh = 1.f / a.sh, rw = 1.f / a.sw;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    int xs, ys, b;
    split_pixel(pix, a.ws, a.hs, xs, ys, b);
    const int yd0 = near_first(a.sh, rh, ys, a.hs, a.hd), yd1 = near_first(a.sh, rh, ys + 1, a.hs, a.hd);
    const int xd0 = near_first(a.sw, rw, xs, a.ws, a.wd), xd1 = near_first(a.sw, rw, xs + 1, a.ws, a.wd);
    bf16* d = dsrc + pix * a.ld_src + cg * V;
    float acc[V];
    if (accumulate) {
      const bf16v<V> prev = ldv<V>(d);
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = bf2f(prev[e]);
    } else {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = 0.f;
    }
    for (int yd = yd0; yd < yd1; ++yd) {
      const bf16* g = ddst + (((size_t)b * a.hd + yd) * a.wd + xd0) * a.ld_dst + a.ch_off + cg * V;
      for (int xd = xd0; xd < xd1; ++xd, g += a.ld_dst) {
        const bf16v<V> v = ldv<V>(g);
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e] += bf2f(v[e]);
      }
    }
    bf16v<V> o;
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = f2bf(acc[e]);
    stv<V>(d, o);
  }
}

// 16 bytes per lane where every channel count, pitch and offset allows it, else one element per lane
template <class... KArgs, class... Args>
int launch_gather(const char* who, void (*k8)(KArgs...), void (*k1)(KArgs...), const ResampleArgs& a, size_t pixels, void* stream,
                  Args... args) {
  const bool v = vec_ok(a);
  hipLaunchKernelGGL(v ? k8 : k1, dim3(grid_for(pixels * (v ? a.c >> 3 : a.c))), dim3(256), 0, tok_stream(stream), args...);
  TOK_CHECK_LAUNCH(who);
  return TOK_OK;
}

}  // namespace

extern "C" int tok_bilinear_fwd(const void* src, int n, int hs, int ws, int c, int ld_src, void* dst, int hd, int wd,
                                int ld_dst, int ch_off, void* stream) {
  ResampleArgs a;
  TOK_CHECK_ARG(src && dst && fill_resample(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_bilinear_fwd: bad args");
  return launch_gather("tok_bilinear_fwd", bilinear_fwd_kernel<8>, bilinear_fwd_kernel<1>, a, (size_t)n * hd * wd, stream,
                       (const bf16*)src, (bf16*)dst, a);
}

extern "C" int tok_bilinear_bwd(const void* ddst, int n, int hd, int wd, int ld_dst, int ch_off, void* dsrc, int hs,
                                int ws, int c, int ld_src, int accumulate, void* stream) {
  ResampleArgs a;
  TOK_CHECK_ARG(ddst && dsrc && fill_resample(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_bilinear_bwd: bad args");
  return launch_gather("tok_bilinear_bwd", bilinear_bwd_kernel<8>, bilinear_bwd_kernel<1>, a, (size_t)n * hs * ws, stream,
                       (const bf16*)ddst, (bf16*)dsrc, a, accumulate);
}

extern "C" int tok_nearest_fwd(const void* src, int n, int hs, int ws, int c, int ld_src, void* dst, int hd, int wd,
                               int ld_dst, int ch_off, void* stream) {
  ResampleArgs a;
  TOK_CHECK_ARG(src && dst && fill_resample(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_nearest_fwd: bad args");
  return launch_gather("tok_nearest_fwd", nearest_fwd_kernel<8>, nearest_fwd_kernel<1>, a, (size_t)n * hd * wd, stream,
                       (const bf16*)src, (bf16*)dst, a);
}

extern "C" int tok_nearest_bwd(const void* ddst, int n, int hd, int wd, int ld_dst, int ch_off, void* dsrc, int hs,
                               int ws, int c, int ld_src, int accumulate, void* stream) {
  ResampleArgs a;
  TOK_CHECK_ARG(ddst && dsrc && fill_resample(a, n, hs, ws, c, ld_src, hd, wd, ld_dst, ch_off), "tok_nearest_bwd: bad args");
  return launch_gather("tok_nearest_bwd", nearest_bwd_kernel<8>, nearest_bwd_kernel<1>, a, (size_t)n * hs * ws, stream,
                       (const bf16*)ddst, (bf16*)dsrc, a, accumulate);
}
