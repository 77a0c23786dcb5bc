// Grouped 3x3 convolution (padding 1, stride in {1, 2}, no bias, no dilation) of the ResNeXt bottleneck ([timm] Bottleneck.conv2 with
// groups = cardinality), cin / groups == cout / groups == cg in {4, 8, 16, 32, 64}, and its data and weight gradients.
//
// Layout: x / out / dout / dx bf16 NHWC with row pitch ld (c % 8 == 0, ld % 8 == 0); the weight is the fp32 master (K, cg, 3, 3),
// [k][cg][3][3] or [k][3][3][cg] in memory (w_krsc).  Products are bf16 x bf16-rounded weight, accumulation is fp32.
//
// The arithmetic does not grow with the number of groups: every MFMA multiplies a tile of 16 channels against the IC = max(cg, 16)
// channels of the group(s) that tile belongs to, never against the whole channel axis.
//   cg = 64 / 32   a tile is a quarter / half of one group; K = 32 is (half) a tap of that group's channels
//   cg = 16        a tile is one group; K = 32 is two taps
//   cg = 8 / 4     a tile is two / four groups; K = 32 is two taps of the tile's own 16 channels, and the weight fragment is
//                  block diagonal: the zeros between the groups are put there when the fragment is built, once per wave
//
// Forward and data gradient are one kernel (v_mfma_f32_16x16x32_bf16, A = weights [16 channels][K], B = pixels [K][16 pixels]):
// a wave owns one 16-channel tile, builds its (9 * IC / 32, rounded up) weight fragments from the fp32 master once, keeps them in
// registers and walks a contiguous run of the map's 16-pixel tiles.  The B fragment of a lane is 8 channels of the source pixel
// its tap points at (zero outside the map, and for a tap whose stride-2 parity does not reach the pixel).  In the MFMA's lane
// order neighbouring lanes are neighbouring PIXELS, a whole row pitch apart in memory, so the fragments are not loaded from
// global memory directly (that form ran the 56^2 x 128 layer at 1.3 TB/s, profiles/resnext_kernel_times.txt): the four waves of a block own the four tiles of a
// 64-channel span and stage the nine shifted copies of the 16 pixels x 64 channels together, 8 lanes per pixel, through LDS.
//   forward       dst[oh][ow][k] = sum_{r,s,c} src[oh*S - 1 + r][ow*S - 1 + s][c] w[k][c][r][s]
//   data gradient dst[ih][iw][c] = sum_{r,s,k: (ih+1-r) % S == 0, (iw+1-s) % S == 0} src[(ih+1-r)/S][(iw+1-s)/S][k] w[k][c][r][s]
// (the data gradient is the same kernel on per-group-transposed weights with the gather running backwards, which is what a
// tap flip amounts to).  The result tile has the pixel on the lane and four consecutive channels in the registers: 8-byte stores.
// The forward optionally leaves the per-channel (sum, sum of squares) of the ROUNDED output, partial[2][rows][c] as
// tok_bn_finalize reads it: a lane sums its pixels in walk order, the 16 pixel lanes of a channel quad are folded in lane order.
//
// Weight gradient: a wave owns a tile of 16 output channels and pairs it with each 16-channel input tile of the same IC span
// (IC / 16 pairs, 9 accumulator tiles each, one per tap).  A block walks a contiguous run of 32-pixel chunks: dout and the nine
// shifted copies of x, 64 channels wide, are staged once for its four waves ([pixel][channel] LDS images, 136-byte rows) and
// come back channel-major as the A = dout^T [16][32] and B = x [32][16] fragments.
// The accumulators go to ws[row][pair][tap][16][16]; a second launch folds the rows in order and writes the in-group entries.
// No float atomics anywhere: results are bit-reproducible run to run.
#include "tok_common.h"

namespace {

constexpr int kFwdBlocks = 1024;   // workgroups of a forward / data-gradient launch (each walks several tiles beyond)
constexpr int kWgWaves = 2048;     // waves of a weight-gradient launch
constexpr int kIp = 72;            // bf16 per LDS row of the forward's [tap][pixel][64 channels] images (144 bytes: the 16 pixel
                                   // lanes of a 16-byte fragment read start 36 banks apart, meant to avoid bank conflicts; not profiled)
constexpr int kWp = 68;            // bf16 per LDS row of the weight gradient's [pixel][64 channels] images (136 bytes: the four
                                   // 8-pixel groups of a channel-major read start 16 banks apart, meant to avoid conflicts; not profiled)

__device__ __forceinline__ bf16x4 zero4() {
  bf16x4 z;
#pragma unroll
  for (int e = 0; e < 4; ++e) z[e] = f2bf(0.f);
  return z;
}

__device__ __forceinline__ size_t w_index(int k, int ci, int tap, int cg, int w_krsc) {
  return w_krsc ? ((size_t)k * 9 + tap) * cg + ci : ((size_t)k * cg + ci) * 9 + tap;
}

template <int IC, int S, bool DG>
__global__ __launch_bounds__(256) void gconv_kernel(const bf16* __restrict__ src, const float* __restrict__ w,
                                                    bf16* __restrict__ dst, int N, int SH, int SW, int DH, int DW, int C, int ld,
                                                    int cg, int w_krsc, int accumulate, float* __restrict__ stats, int ctiles,
                                                    int ptiles) {
  constexpr int NM = (9 * IC + 31) / 32;
  __shared__ float red[2][256][4];
  __shared__ __attribute__((aligned(16))) bf16 img[2][9 * 16][kIp];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
  const int ct = blockIdx.x * 4 + wave;
  const bool live = ct < ctiles;
  const int c0 = ct * 16;
  const int icb = IC == 16 ? c0 : (c0 / IC) * IC;   // first channel of the span this tile multiplies against
  // A: row l15 is channel cm of the result, element e of k-slot (mf, kg) is channel ck of the source under tap `tap`
  bf16x8 wf[NM];
  {
    const int cm = c0 + l15;
#pragma unroll
    for (int mf = 0; mf < NM; ++mf) {
      const int kk = (mf * 4 + kg) * 8, tap = kk / IC, cio = kk % IC;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int ck = icb + cio + e;
        float v = 0.f;
        if (live && tap < 9 && cm < C && ck < C && cm / cg == ck / cg)
          v = DG ? w[w_index(ck, cm % cg, tap, cg, w_krsc)] : w[w_index(cm, ck % cg, tap, cg, w_krsc)];
        wf[mf][e] = f2bf(v);
      }
    }
  }
  float s1[4], s2[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) { s1[i] = 0.f; s2[i] = 0.f; }
  const int M = N * DH * DW;                         // (pixel indices are 32-bit, the host checks; element offsets are not)
  const int ch = c0 + 4 * kg;                        // D: column l15 is the pixel, rows 4 kg + i are the channels
  // a block row walks a contiguous run of tiles: the intent is that the rows of the map its taps reach are still cached for the
  // next tile (hit rates not measured).
  // The block's four waves share the pixels: together they stage the nine shifted copies of the tile's 16 pixels x 64 channels
  // with coalesced 16-byte loads (8 lanes per pixel) into LDS (two images: one barrier per tile), and every wave reads its
  // fragments back in the MFMA's lane order.
  const int per = (ptiles + (int)gridDim.y - 1) / (int)gridDim.y;
  const int pt1 = min(((int)blockIdx.y + 1) * per, ptiles);
  const int cb = blockIdx.x * 64;
  const int sch = (tid & 7) * 8, spx = (tid >> 3) & 15, stap0 = tid >> 7;   // staging: channel chunk, pixel, first tap (then + 2)
  int buf = 0;
  for (int pt = blockIdx.y * per; pt < pt1; ++pt, buf ^= 1) {               // (uniform over the block: the barrier below)
    {
      const int pix = pt * 16 + spx;
      const bool pv = pix < M && cb + sch < C;
      const int ow = pix % DW;
      const int rowid = pix / DW;
      const int oh = rowid % DH;
      const int srow = (rowid / DH) * SH;
      bf16x8 v[5];
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int tap = stap0 + 2 * i;
        const int r = tap / 3, s = tap % 3;
        bool ok = pv && tap < 9;
        int sh, sw;
        if (DG) {
          const int eh = oh + 1 - r, ew = ow + 1 - s;
          ok = ok && eh >= 0 && ew >= 0 && eh % S == 0 && ew % S == 0;
          sh = eh / S;
          sw = ew / S;
          ok = ok && sh < SH && sw < SW;
        } else {
          sh = oh * S - 1 + r;
          sw = ow * S - 1 + s;
          ok = ok && sh >= 0 && sh < SH && sw >= 0 && sw < SW;
        }
        v[i] = ok ? ldg16(src + (size_t)((srow + sh) * SW + sw) * ld + cb + sch) : zero8();
      }
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        const int tap = stap0 + 2 * i;
        if (tap < 9) *reinterpret_cast<bf16x8*>(&img[buf][tap * 16 + spx][sch]) = v[i];
      }
    }
    __syncthreads();
    const int pix = pt * 16 + l15;
    const bool pv = live && pix < M;
    bf16x8 b[NM];
#pragma unroll
    for (int mf = 0; mf < NM; ++mf) {
      const int kk = (mf * 4 + kg) * 8, tap = kk / IC, cio = kk % IC;
      b[mf] = tap < 9 ? *reinterpret_cast<const bf16x8*>(&img[buf][tap * 16 + l15][icb - cb + cio]) : zero8();
    }
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int mf = 0; mf < NM; ++mf) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[mf], b[mf], acc, 0, 0, 0);
    if (pv && ch < C) {
      bf16* p = dst + (size_t)pix * ld + ch;
      const bf16x4 old = accumulate ? *reinterpret_cast<const bf16x4*>(p) : zero4();
      bf16x4 o;
#pragma unroll
      for (int i = 0; i < 4; ++i) o[i] = f2bf(acc[i] + bf2f(old[i]));
      *reinterpret_cast<bf16x4*>(p) = o;
      if (stats != nullptr) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float f = bf2f(o[i]);
          s1[i] += f;
          s2[i] = fmaf(f, f, s2[i]);
        }
      }
    }
  }
  if (stats == nullptr) return;       // (uniform: a launch argument)
#pragma unroll
  for (int i = 0; i < 4; ++i) { red[0][tid][i] = s1[i]; red[1][tid][i] = s2[i]; }
  __syncthreads();
  if (l15 == 0 && live && ch < C) {
    for (int p = 1; p < 16; ++p)
#pragma unroll
      for (int i = 0; i < 4; ++i) { s1[i] += red[0][tid + p][i]; s2[i] += red[1][tid + p][i]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      stats[(size_t)blockIdx.y * C + ch + i] = s1[i];
      stats[((size_t)gridDim.y + blockIdx.y) * C + ch + i] = s2[i];
    }
  }
}

// ws[blockIdx.y][pair][tap][16 output channels][16 input channels]: this wave's sums over the block row's chunks, for each of
// the PPW = IC / 16 input tiles its output tile pairs with
template <int S, int PPW>
__global__ __launch_bounds__(256) void gconv_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dout, int N, int H,
                                                          int W, int P, int Q, int C, int ld, int ctiles, int npairs,
                                                          int nchunks, float* __restrict__ ws) {
  constexpr int IC = 16 * PPW;
  __shared__ __attribute__((aligned(16))) bf16 img[10][32][kWp];   // [0] dout, [1 + tap] x under the tap: 32 pixels x 64 channels
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l15 = lane & 15, kg = lane >> 4;
  const int cb = blockIdx.x * 64;
  const int ct = blockIdx.x * 4 + wave;                 // output-channel tile
  const bool live = ct < ctiles;
  const int c0 = ct * 16;
  const int xo = (IC == 16 ? c0 : (c0 / IC) * IC) - cb; // first channel, inside the block's span, of the input tiles it pairs with
  const int sch = (tid & 7) * 8, spx = tid >> 3;        // staging: channel chunk of the span, pixel of the chunk
  const int M = N * P * Q;
  f32x4 acc[PPW][9];
#pragma unroll
  for (int j = 0; j < PPW; ++j)
#pragma unroll
    for (int t = 0; t < 9; ++t) acc[j][t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int per = (nchunks + (int)gridDim.y - 1) / (int)gridDim.y;       // a contiguous run of chunks per workspace row
  const int chn1 = min(((int)blockIdx.y + 1) * per, nchunks);
  for (int chn = blockIdx.y * per; chn < chn1; ++chn) {                  // (uniform over the block: the barriers below)
    const int pix = chn * 32 + spx;
    const bool pv = pix < M && cb + sch < C;
    const int ow = pix % Q;
    const int rowid = pix / Q;
    const int oh = rowid % P;
    const int xrow = (rowid / P) * H;
    u32x4 v[10];
    v[0] = __builtin_bit_cast(u32x4, pv ? ldg16(dout + (size_t)pix * ld + cb + sch) : zero8());
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int ih = oh * S - 1 + t / 3, iw = ow * S - 1 + t % 3;
      const bool ok = pv && ih >= 0 && ih < H && iw >= 0 && iw < W;
      v[1 + t] = __builtin_bit_cast(u32x4, ok ? ldg16(x + (size_t)((xrow + ih) * W + iw) * ld + cb + sch) : zero8());
    }
    __syncthreads();                                   // the previous chunk's fragments have been read
#pragma unroll
    for (int t = 0; t < 10; ++t) {
      u32x2* q = reinterpret_cast<u32x2*>(&img[t][spx][sch]);
      q[0] = u32x2{v[t][0], v[t][1]};
      q[1] = u32x2{v[t][2], v[t][3]};
    }
    __syncthreads();
    bf16x8 a;
#pragma unroll
    for (int i = 0; i < 8; ++i) a[i] = img[0][8 * kg + i][wave * 16 + l15];
#pragma unroll
    for (int j = 0; j < PPW; ++j)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        bf16x8 b;
#pragma unroll
        for (int i = 0; i < 8; ++i) b[i] = img[1 + t][8 * kg + i][xo + 16 * j + l15];
        acc[j][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc[j][t], 0, 0, 0);
      }
  }
  if (!live) return;
#pragma unroll
  for (int j = 0; j < PPW; ++j) {
    float* o = ws + ((size_t)blockIdx.y * npairs + ct * PPW + j) * (9 * 256);
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) o[t * 256 + (4 * kg + i) * 16 + l15] = acc[j][t][i];
  }
}

// dw[k][ci][tap] (+)= sum over the workspace rows, in row order; one thread per element of the (K, cg, 3, 3) gradient
__global__ __launch_bounds__(256) void gconv_wgrad_fold_kernel(const float* __restrict__ ws, int rows, int npairs, int C, int cg,
                                                               int IC, int w_krsc, float* __restrict__ dw, int accumulate) {
  const int total = C * cg * 9;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    const int tap = i % 9, ci = (i / 9) % cg, k = i / (9 * cg);
    const int ca = (k / cg) * cg + ci;                  // the input channel on the activation's channel axis
    const int c0 = (k >> 4) << 4, icb = (c0 / IC) * IC;
    const int pr = (k >> 4) * (IC >> 4) + ((ca - icb) >> 4);
    const float* p = ws + ((size_t)pr * 9 + tap) * 256 + (k & 15) * 16 + ((ca - icb) & 15);
    float a = 0.f;
    for (int y = 0; y < rows; ++y) a += p[(size_t)y * npairs * (9 * 256)];
    const size_t o = w_index(k, ci, tap, cg, w_krsc);
    dw[o] = accumulate ? dw[o] + a : a;
  }
}

struct GGeo {
  int cg, ic, ctiles, gx, rows, ptiles;        // forward / data gradient: grid (gx, rows)
  int npairs, wgx, wrows, nchunks;             // weight gradient: grid (wgx, wrows)
};

inline int out_dim(int h, int stride) { return (h - 1) / stride + 1; }

// out_rows x out_w: the map the forward / data-gradient launch writes; wg_rows x wg_w: the forward's output (weight gradient)
GGeo g_geo(long long pixels, long long wg_pixels, int c, int groups) {
  GGeo g;
  g.cg = c / groups;
  g.ic = g.cg < 16 ? 16 : g.cg;
  g.ctiles = (c + 15) / 16;
  g.gx = (g.ctiles + 3) / 4;
  g.ptiles = (int)((pixels + 15) / 16);
  long long cap = kFwdBlocks / g.gx;
  if (cap < 1) cap = 1;
  g.rows = (int)(g.ptiles < cap ? g.ptiles : cap);
  g.npairs = g.ctiles * (g.ic / 16);
  g.wgx = g.gx;
  g.nchunks = (int)((wg_pixels + 31) / 32);
  cap = kWgWaves / g.npairs;
  if (cap < 1) cap = 1;
  g.wrows = (int)(g.nchunks < cap ? g.nchunks : cap);
  return g;
}

bool g_args_ok(int n, int h, int wd, int c, int ld, int groups, int stride) {
  if (!(n > 0 && h > 0 && wd > 0 && c > 0 && c % 8 == 0 && ld >= c && ld % 8 == 0 && (stride == 1 || stride == 2))) return false;
  if ((long long)n * h * wd > 0x7fffffffLL - 64) return false;      // pixel indices are 32-bit in the kernels
  if (groups < 2 || c % groups != 0) return false;
  const int cg = c / groups;
  return cg == 4 || cg == 8 || cg == 16 || cg == 32 || cg == 64;
}

#define TOK_GCONV_SERVED                                                                                                    \
  "served: c %% 8 == 0, ld %% 8 == 0, ld >= c, groups >= 2 dividing c, c / groups in {4, 8, 16, 32, 64}, stride in {1, 2}, " \
  "n * h * w < 2^31 - 64 (groups == 1 is the dense route)"

template <bool DG>
bool launch_g(const GGeo& g, int stride, hipStream_t st, const bf16* src, const float* w, bf16* dst, int n, int sh, int sw, int dh,
              int dwid, int c, int ld, int w_krsc, int acc, float* stats) {
  const dim3 grid(g.gx, g.rows);
#define TOK_G_CASE(IC_, S_)                                                                                                   \
  if (g.ic == IC_ && stride == S_) {                                                                                          \
    hipLaunchKernelGGL((gconv_kernel<IC_, S_, DG>), grid, dim3(256), 0, st, src, w, dst, n, sh, sw, dh, dwid, c, ld, g.cg, w_krsc, \
                       acc, stats, g.ctiles, g.ptiles);                                                                       \
    return true;                                                                                                              \
  }
  TOK_G_CASE(16, 1) TOK_G_CASE(16, 2) TOK_G_CASE(32, 1) TOK_G_CASE(32, 2) TOK_G_CASE(64, 1) TOK_G_CASE(64, 2)
#undef TOK_G_CASE
  return false;      // a width g_args_ok admits and this list does not: nothing was launched
}

}  // namespace

extern "C" int tok_gconv_rows(int n, int h, int wd, int c, int groups, int stride) {
  if (!g_args_ok(n, h, wd, c, c, groups, stride)) return TOK_ERR_INVALID;
  const long long m = (long long)n * out_dim(h, stride) * out_dim(wd, stride);
  return g_geo(m, m, c, groups).rows;
}

extern "C" int tok_gconv_fwd(const void* x, const float* w, int w_krsc, int n, int h, int wd, int c, int ld, int groups, int stride,
                             void* out, float* stats, void* stream) {
  TOK_CHECK_ARG(x && w && out, "tok_gconv_fwd: null pointer");
  TOK_CHECK_ARG(g_args_ok(n, h, wd, c, ld, groups, stride), "tok_gconv_fwd: bad sizes; " TOK_GCONV_SERVED);
  const int p = out_dim(h, stride), q = out_dim(wd, stride);
  const long long m = (long long)n * p * q;
  const GGeo g = g_geo(m, m, c, groups);
  TOK_CHECK_ARG(launch_g<false>(g, stride, tok_stream(stream), (const bf16*)x, w, (bf16*)out, n, h, wd, p, q, c, ld, w_krsc != 0, 0,
                                stats), "tok_gconv_fwd: no kernel for group width %d", g.cg);
  TOK_CHECK_LAUNCH("tok_gconv_fwd");
  return TOK_OK;
}

extern "C" int tok_gconv_dgrad(const void* dout, const float* w, int w_krsc, int n, int h, int wd, int c, int ld, int groups,
                               int stride, void* dx, int accumulate, void* stream) {
  TOK_CHECK_ARG(dout && w && dx, "tok_gconv_dgrad: null pointer");
  TOK_CHECK_ARG(g_args_ok(n, h, wd, c, ld, groups, stride), "tok_gconv_dgrad: bad sizes; " TOK_GCONV_SERVED);
  const int p = out_dim(h, stride), q = out_dim(wd, stride);
  const GGeo g = g_geo((long long)n * h * wd, (long long)n * p * q, c, groups);
  TOK_CHECK_ARG(launch_g<true>(g, stride, tok_stream(stream), (const bf16*)dout, w, (bf16*)dx, n, p, q, h, wd, c, ld, w_krsc != 0,
                               accumulate, nullptr), "tok_gconv_dgrad: no kernel for group width %d", g.cg);
  TOK_CHECK_LAUNCH("tok_gconv_dgrad");
  return TOK_OK;
}

extern "C" size_t tok_gconv_wgrad_ws_bytes(int n, int h, int wd, int c, int groups, int stride) {
  if (!g_args_ok(n, h, wd, c, c, groups, stride)) return 0;
  const long long m = (long long)n * out_dim(h, stride) * out_dim(wd, stride);
  const GGeo g = g_geo(m, m, c, groups);
  return (size_t)g.wrows * g.npairs * 9 * 256 * sizeof(float);
}

extern "C" int tok_gconv_wgrad(const void* x, const void* dout, int n, int h, int wd, int c, int ld, int groups, int stride,
                               float* dw, int w_krsc, int accumulate, float* ws, size_t ws_bytes, void* stream) {
  TOK_CHECK_ARG(x && dout && dw && ws, "tok_gconv_wgrad: null pointer");
  TOK_CHECK_ARG(g_args_ok(n, h, wd, c, ld, groups, stride), "tok_gconv_wgrad: bad sizes; " TOK_GCONV_SERVED);
  TOK_CHECK_ARG(ws_bytes >= tok_gconv_wgrad_ws_bytes(n, h, wd, c, groups, stride), "tok_gconv_wgrad: workspace too small");
  const int p = out_dim(h, stride), q = out_dim(wd, stride);
  const long long m = (long long)n * p * q;
  const GGeo g = g_geo(m, m, c, groups);
  const dim3 grid(g.wgx, g.wrows);
  hipStream_t st = tok_stream(stream);
  bool launched = false;
#define TOK_GW_CASE(IC_, S_)                                                                                                  \
  if (g.ic == IC_ && stride == S_) {                                                                                          \
    hipLaunchKernelGGL((gconv_wgrad_kernel<S_, IC_ / 16>), grid, dim3(256), 0, st, (const bf16*)x, (const bf16*)dout, n, h, wd, p, \
                       q, c, ld, g.ctiles, g.npairs, g.nchunks, ws);                                                          \
    launched = true;                                                                                                          \
  }
  TOK_GW_CASE(16, 1) TOK_GW_CASE(16, 2) TOK_GW_CASE(32, 1) TOK_GW_CASE(32, 2) TOK_GW_CASE(64, 1) TOK_GW_CASE(64, 2)
#undef TOK_GW_CASE
  TOK_CHECK_ARG(launched, "tok_gconv_wgrad: no kernel for group width %d", g.cg);
  const int total = c * g.cg * 9;
  int blocks = (total + 255) / 256;
  if (blocks > 1024) blocks = 1024;
  hipLaunchKernelGGL(gconv_wgrad_fold_kernel, dim3(blocks), dim3(256), 0, st, ws, g.wrows, g.npairs, c, g.cg, g.ic, w_krsc != 0, dw,
                     accumulate);
  TOK_CHECK_LAUNCH("tok_gconv_wgrad");
  return TOK_OK;
}
