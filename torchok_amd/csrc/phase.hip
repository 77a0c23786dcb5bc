// Phase split / merge (space-to-batch by d), NHWC bf16: the permutation that lets a dilated ResNet stage run on the plain
// kernels.  A 3x3 / stride-1 convolution with dilation d and padding d is the plain 3x3 / padding-1 convolution on each of the
// d x d phase images x[:, a::d, b::d, :]; everything else in such a stage (1x1 convolutions, BatchNorm, ReLU, the residual add)
// does not care which pixel is where.
//   merged  [n][h][w][ld]                 pixel (i, Y, X)
//   phased  [n][d][d][h/d][w/d][ld]       pixel (i, a, b, y, x) = merged (i, y*d + a, x*d + b): n*d*d images of h/d x w/d
// One lane per (destination pixel, 8-channel group), 16 bytes per lane, grid-strided, 64-bit element offsets (the addressing
// of resample.hip).  Without `accumulate` a lane moves its 16 bytes as they are (NaN payloads, infinities, -0); with it the
// destination becomes bf16(float(old) + float(v)), rounded once: the backward form, the gradient of a split being a merge.
// No LDS, no atomics, nothing data-dependent; channels [c, ld) are neither read into a result nor written.
#include "resample.h"

namespace {

struct PhaseArgs {
  int n, h, w, c, ld, ds;   // ds = log2(d)
};

// SPLIT: the destination is the phased tensor; else the merged one.  `pix` walks the DESTINATION, so stores are contiguous.
template <bool SPLIT>
__global__ __launch_bounds__(256) void phase_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, PhaseArgs a,
                                                    int accumulate) {
  const int cgs = a.c >> 3;
  const int d = 1 << a.ds, dm = d - 1;
  const int hq = a.h >> a.ds, wq = a.w >> a.ds;
  const size_t total = (size_t)a.n * a.h * a.w * cgs;
  for (size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (size_t)gridDim.x * 256) {
    const int cg = (int)(idx % cgs);
    const size_t pix = idx / cgs;
    size_t other;
    if (SPLIT) {
      int x, y, img;                                    // img = (i * d + pa) * d + pb
      split_pixel(pix, wq, hq, x, y, img);
      const int pb = img & dm, pa = (img >> a.ds) & dm, i = img >> (2 * a.ds);
      other = ((size_t)i * a.h + ((y << a.ds) + pa)) * a.w + ((x << a.ds) + pb);
    } else {
      int X, Y, i;
      split_pixel(pix, a.w, a.h, X, Y, i);
      const int img = (((i << a.ds) + (Y & dm)) << a.ds) + (X & dm);
      other = ((size_t)img * hq + (Y >> a.ds)) * wq + (X >> a.ds);
    }
    const bf16* s = src + other * a.ld + cg * 8;
    bf16* t = dst + pix * a.ld + cg * 8;
    if (accumulate) {
      const bf16v<8> v = ldv<8>(s), old = ldv<8>(t);
      bf16v<8> o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(bf2f(old[e]) + bf2f(v[e]));
      stv<8>(t, o);
    } else {
      *reinterpret_cast<uint4*>(t) = *reinterpret_cast<const uint4*>(s);
    }
  }
}

template <bool SPLIT>
int phase_launch(const char* who, const void* src, int n, int h, int w, int c, int ld, int d, void* dst, int accumulate,
                 void* stream) {
  TOK_CHECK_ARG(src && dst && src != dst && !(((uintptr_t)src | (uintptr_t)dst) & 15), "%s: NULL, aliased or unaligned pointer", who);
  TOK_CHECK_ARG((d == 2 || d == 4) && n >= 1 && h >= d && w >= d && h % d == 0 && w % d == 0, "%s: d in {2, 4}, h and w multiples of d", who);
  TOK_CHECK_ARG(c >= 8 && c % 8 == 0 && ld >= c && ld % 8 == 0, "%s: c and ld multiples of 8, ld >= c", who);
  TOK_CHECK_ARG((int64_t)n * h * w < ((int64_t)1 << 31), "%s: 2^31 pixels or more", who);
  PhaseArgs a{n, h, w, c, ld, d == 2 ? 1 : 2};
  const size_t total = (size_t)n * h * w * (c >> 3);
  hipLaunchKernelGGL(phase_kernel<SPLIT>, dim3(grid_for(total)), dim3(256), 0, tok_stream(stream), (const bf16*)src, (bf16*)dst,
                     a, accumulate != 0);
  TOK_CHECK_LAUNCH(who);
  return TOK_OK;
}

}  // namespace

extern "C" int tok_phase_split(const void* x, int n, int h, int w, int c, int ld, int d, void* out, int accumulate, void* stream) {
  return phase_launch<true>("tok_phase_split", x, n, h, w, c, ld, d, out, accumulate, stream);
}

extern "C" int tok_phase_merge(const void* xs, int n, int h, int w, int c, int ld, int d, void* out, int accumulate, void* stream) {
  return phase_launch<false>("tok_phase_merge", xs, n, h, w, c, ld, d, out, accumulate, stream);
}
