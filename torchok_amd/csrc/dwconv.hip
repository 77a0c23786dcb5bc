// Depthwise k x k convolution (k in {3, 5}, stride in {1, 2}, padding k / 2) of the MnasNet blocks ([timm] create_conv2d with
// depthwise=True inside DepthwiseSeparableConv / InvertedResidual), and its data and weight gradients.
//
// Layout: x / out / dout / dx bf16 NHWC with row pitch ld (c % 8 == 0, ld % 8 == 0); the weight is the fp32 master [c][k][k]
// (a (C,1,k,k) tensor is [c][k][k] in memory in either memory format).  Accumulation is fp32.
//
// One kernel serves the forward and the data gradient: a block owns a tile of CG channel groups (8 channels, one 16-byte vector
// each) and 256 / CG pixel lanes; a lane produces strips of T = 4 consecutive output columns.  For every filter row it loads the
// source columns the strip needs once ((T-1)*S + k for the forward) and applies all k taps of that row to the T outputs: per
// output, k * ((T-1)*S + k) / T vector loads instead of k * k.  The tile's filter sits in LDS ([tap][channel]).
//   forward       dst[oh][oq] = sum_{r,s} src[oh*S - p + r][oq*S - p + s] w[r][s]
//   data gradient dst[ih][iw] = sum_{r,s: (ih + p - r) % S == 0, (iw + p - s) % S == 0} src[(ih + p - r)/S][(iw + p - s)/S] w[r][s]
// (stride 2 is the transposed correlation: each output parity gets its own taps, no flipped filter).
// The forward optionally leaves the per-channel (sum, sum of squares) of the ROUNDED output, partial[2][rows][c] as
// tok_bn_finalize reads it: a BatchNorm after the depthwise unit needs no statistics pass of its own.
//
// Weight gradient: the same tiles, one block row per filter row r (gridDim.z = k); a lane keeps the k * 8 sums of its row of taps
// over its strips, the block folds its lanes in a fixed order into partial[blockIdx.y][c][k*k], and a second launch folds the
// block rows in order.  No float atomics anywhere: results are bit-reproducible run to run.
#include "tok_common.h"

namespace {

constexpr int kT = 4;            // output columns per strip
constexpr int kGridCap = 2048;   // workgroups of a launch (grid-stride beyond)

__host__ __device__ constexpr int floordiv_c(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// channel groups per block: the largest divisor of c / 8 that is <= 8 (a tile never straddles the channel count)
inline int tile_groups(int c) {
  const int g = c >> 3;
  for (int d = 8; d > 1; --d)
    if (g % d == 0) return d;
  return 1;
}

inline int grid_rows(long long strips, int lanes, int tiles, int z) {
  const long long want = (strips + lanes - 1) / lanes;
  long long cap = kGridCap / ((long long)tiles * z);
  if (cap < 1) cap = 1;
  return (int)(want < cap ? want : cap);
}

template <int K, int S, bool DG>
__global__ __launch_bounds__(256) void dwconv_kernel(const bf16* __restrict__ src, const float* __restrict__ w,
                                                     bf16* __restrict__ dst, int N, int SH, int SW, int DH, int DW, int C,
                                                     int ld, int CG, int accumulate, float* __restrict__ stats) {
  constexpr int PAD = K / 2, KK = K * K;
  constexpr int DMIN = floordiv_c(PAD - (K - 1), S), DMAX = floordiv_c(kT - 1 + PAD, S);
  constexpr int NC = DG ? DMAX - DMIN + 1 : (kT - 1) * S + K;   // source columns per strip and filter row
  __shared__ float wl[KK][64];
  __shared__ float red[2][256][8];
  const int tid = threadIdx.x;
  const int cgl = tid % CG, pl = tid / CG, PL = 256 / CG;
  const int c0 = blockIdx.x * CG * 8;
  for (int i = tid; i < KK * CG * 8; i += 256) {
    const int tap = i / (CG * 8), cc = i % (CG * 8);
    wl[tap][cc] = w[(size_t)(c0 + cc) * KK + tap];
  }
  __syncthreads();
  const int c = c0 + cgl * 8;
  const bool live = pl < PL;
  float s1[8], s2[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { s1[e] = 0.f; s2[e] = 0.f; }
  const int strips_w = (DW + kT - 1) / kT;
  const long long total = (long long)N * DH * strips_w;
  for (long long st = (long long)blockIdx.y * PL + pl; live && st < total; st += (long long)gridDim.y * PL) {
    const int sw = (int)(st % strips_w);
    const long long rowid = st / strips_w;
    const int oh = (int)(rowid % DH);
    const int img = (int)(rowid / DH);
    const int d0 = sw * kT;
    float acc[kT][8];
#pragma unroll
    for (int t = 0; t < kT; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[t][e] = 0.f;
#pragma unroll
    for (int r = 0; r < K; ++r) {
      int sh;
      bool valid;
      if (DG) {
        const int e = oh + PAD - r;
        valid = e >= 0 && e % S == 0 && e / S < SH;
        sh = e / S;
      } else {
        sh = oh * S - PAD + r;
        valid = sh >= 0 && sh < SH;
      }
      if (!valid) continue;
      const int col0 = DG ? d0 / S + DMIN : d0 * S - PAD;
      const bf16* row = src + ((size_t)img * SH + sh) * SW * ld + c;
      bf16x8 v[NC];
#pragma unroll
      for (int j = 0; j < NC; ++j) {
        const int col = col0 + j;
        v[j] = (col >= 0 && col < SW) ? ldg16(row + (size_t)col * ld) : zero8();
      }
#pragma unroll
      for (int s = 0; s < K; ++s) {
        float wv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) wv[e] = wl[r * K + s][cgl * 8 + e];
#pragma unroll
        for (int t = 0; t < kT; ++t) {
          int j;
          if (DG) {
            const int e = t + PAD - s;
            if (e % S != 0) continue;
            j = e / S - DMIN;
          } else {
            j = t * S + s;
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[t][e] = fmaf(bf2f(v[j][e]), wv[e], acc[t][e]);
        }
      }
    }
    bf16* orow = dst + ((size_t)img * DH + oh) * DW * ld + c;
#pragma unroll
    for (int t = 0; t < kT; ++t) {
      if (d0 + t >= DW) break;
      bf16* p = orow + (size_t)(d0 + t) * ld;
      const bf16x8 old = accumulate ? ldg16(p) : zero8();
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(acc[t][e] + bf2f(old[e]));
      stg16(p, o);
      if (stats != nullptr) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = bf2f(o[e]);
          s1[e] += f;
          s2[e] = fmaf(f, f, s2[e]);
        }
      }
    }
  }
  if (stats == nullptr) return;       // (uniform: a launch argument)
#pragma unroll
  for (int e = 0; e < 8; ++e) { red[0][tid][e] = s1[e]; red[1][tid][e] = s2[e]; }
  __syncthreads();
  if (pl == 0) {
    for (int p = 1; p < PL; ++p)
#pragma unroll
      for (int e = 0; e < 8; ++e) { s1[e] += red[0][p * CG + cgl][e]; s2[e] += red[1][p * CG + cgl][e]; }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      stats[(size_t)blockIdx.y * C + c + e] = s1[e];
      stats[((size_t)gridDim.y + blockIdx.y) * C + c + e] = s2[e];
    }
  }
}

// partial[blockIdx.y][c][K*K]: this block's sums for filter row r = blockIdx.z
template <int K, int S>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const bf16* __restrict__ x, const bf16* __restrict__ dout, int N,
                                                           int H, int W, int P, int Q, int C, int ld, int CG,
                                                           float* __restrict__ partial) {
  constexpr int PAD = K / 2, KK = K * K;
  constexpr int NC = (kT - 1) * S + K;
  __shared__ float red[256][8];
  const int tid = threadIdx.x;
  const int cgl = tid % CG, pl = tid / CG, PL = 256 / CG;
  const int c = (blockIdx.x * CG + cgl) * 8;
  const int r = blockIdx.z;
  float acc[K][8];
#pragma unroll
  for (int s = 0; s < K; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[s][e] = 0.f;
  const int strips_w = (Q + kT - 1) / kT;
  const long long total = (long long)N * P * strips_w;
  for (long long st = (long long)blockIdx.y * PL + pl; pl < PL && st < total; st += (long long)gridDim.y * PL) {
    const int sw = (int)(st % strips_w);
    const long long rowid = st / strips_w;
    const int oh = (int)(rowid % P);
    const int img = (int)(rowid / P);
    const int ih = oh * S - PAD + r;
    if (ih < 0 || ih >= H) continue;
    const int q0 = sw * kT;
    bf16x8 g[kT];
    const bf16* grow = dout + ((size_t)img * P + oh) * Q * ld + c;
#pragma unroll
    for (int t = 0; t < kT; ++t) g[t] = (q0 + t < Q) ? ldg16(grow + (size_t)(q0 + t) * ld) : zero8();
    const bf16* xrow = x + ((size_t)img * H + ih) * W * ld + c;
    const int col0 = q0 * S - PAD;
    bf16x8 v[NC];
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const int col = col0 + j;
      v[j] = (col >= 0 && col < W) ? ldg16(xrow + (size_t)col * ld) : zero8();
    }
#pragma unroll
    for (int s = 0; s < K; ++s)
#pragma unroll
      for (int t = 0; t < kT; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[s][e] = fmaf(bf2f(g[t][e]), bf2f(v[t * S + s][e]), acc[s][e]);
  }
  // fold the pixel lanes of every channel group in lane order, one tap at a time
#pragma unroll
  for (int s = 0; s < K; ++s) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[tid][e] = acc[s][e];
    __syncthreads();
    if (pl == 0) {
      float a[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] = acc[s][e];
      for (int p = 1; p < PL; ++p)
#pragma unroll
        for (int e = 0; e < 8; ++e) a[e] += red[p * CG + cgl][e];
#pragma unroll
      for (int e = 0; e < 8; ++e) partial[((size_t)blockIdx.y * C + c + e) * KK + r * K + s] = a[e];
    }
    __syncthreads();
  }
}

// dw[i] (+)= sum over the partial rows, in row order; i over c * k * k
__global__ __launch_bounds__(256) void dwconv_wgrad_fold_kernel(const float* __restrict__ partial, int rows, int n,
                                                                float* __restrict__ dw, int accumulate) {
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    float a = 0.f;
    for (int y = 0; y < rows; ++y) a += partial[(size_t)y * n + i];
    dw[i] = accumulate ? dw[i] + a : a;
  }
}

struct DwGeo {
  int cg, lanes, tiles, rows;
};

DwGeo dw_geo(long long out_rows, int out_w, int c, int z) {
  DwGeo g;
  g.cg = tile_groups(c);
  g.lanes = 256 / g.cg;
  g.tiles = (c >> 3) / g.cg;
  g.rows = grid_rows(out_rows * ((out_w + kT - 1) / kT), g.lanes, g.tiles, z);
  return g;
}

inline int out_dim(int h, int k, int stride) { return (h + 2 * (k / 2) - k) / stride + 1; }

bool dw_args_ok(int n, int h, int wd, int c, int ld, int k, int stride) {
  return n > 0 && h > 0 && wd > 0 && c > 0 && c % 8 == 0 && ld >= c && ld % 8 == 0 && (k == 3 || k == 5) &&
         (stride == 1 || stride == 2);
}

template <bool DG>
void launch_dw(int k, int stride, dim3 grid, hipStream_t st, const bf16* src, const float* w, bf16* dst, int n, int sh, int sw,
               int dh, int dwid, int c, int ld, int cg, int acc, float* stats) {
#define TOK_DW_CASE(K_, S_)                                                                                               \
  if (k == K_ && stride == S_) {                                                                                          \
    hipLaunchKernelGGL((dwconv_kernel<K_, S_, DG>), grid, dim3(256), 0, st, src, w, dst, n, sh, sw, dh, dwid, c, ld, cg, \
                       acc, stats);                                                                                       \
    return;                                                                                                               \
  }
  TOK_DW_CASE(3, 1) TOK_DW_CASE(3, 2) TOK_DW_CASE(5, 1) TOK_DW_CASE(5, 2)
#undef TOK_DW_CASE
}

}  // namespace

extern "C" int tok_dwconv_rows(int n, int h, int wd, int c, int k, int stride) {
  if (!dw_args_ok(n, h, wd, c, c, k, stride)) return TOK_ERR_INVALID;
  return dw_geo((long long)n * out_dim(h, k, stride), out_dim(wd, k, stride), c, 1).rows;
}

extern "C" int tok_dwconv_fwd(const void* x, const float* w, int n, int h, int wd, int c, int ld, int k, int stride, void* out,
                              float* stats, void* stream) {
  TOK_CHECK_ARG(x && w && out, "tok_dwconv_fwd: null pointer");
  TOK_CHECK_ARG(dw_args_ok(n, h, wd, c, ld, k, stride), "tok_dwconv_fwd: bad sizes (c %% 8 == 0, k in {3,5}, stride in {1,2})");
  const int p = out_dim(h, k, stride), q = out_dim(wd, k, stride);
  const DwGeo g = dw_geo((long long)n * p, q, c, 1);
  launch_dw<false>(k, stride, dim3(g.tiles, g.rows), tok_stream(stream), (const bf16*)x, w, (bf16*)out, n, h, wd, p, q, c, ld,
                   g.cg, 0, stats);
  TOK_CHECK_LAUNCH("tok_dwconv_fwd");
  return TOK_OK;
}

extern "C" int tok_dwconv_dgrad(const void* dout, const float* w, int n, int h, int wd, int c, int ld, int k, int stride,
                                void* dx, int accumulate, void* stream) {
  TOK_CHECK_ARG(dout && w && dx, "tok_dwconv_dgrad: null pointer");
  TOK_CHECK_ARG(dw_args_ok(n, h, wd, c, ld, k, stride), "tok_dwconv_dgrad: bad sizes (c %% 8 == 0, k in {3,5}, stride in {1,2})");
  const int p = out_dim(h, k, stride), q = out_dim(wd, k, stride);
  const DwGeo g = dw_geo((long long)n * h, wd, c, 1);
  launch_dw<true>(k, stride, dim3(g.tiles, g.rows), tok_stream(stream), (const bf16*)dout, w, (bf16*)dx, n, p, q, h, wd, c, ld,
                  g.cg, accumulate, nullptr);
  TOK_CHECK_LAUNCH("tok_dwconv_dgrad");
  return TOK_OK;
}

extern "C" size_t tok_dwconv_wgrad_ws_bytes(int n, int h, int wd, int c, int k, int stride) {
  if (!dw_args_ok(n, h, wd, c, c, k, stride)) return 0;
  const DwGeo g = dw_geo((long long)n * out_dim(h, k, stride), out_dim(wd, k, stride), c, k);
  return (size_t)g.rows * c * k * k * sizeof(float);
}

extern "C" int tok_dwconv_wgrad(const void* x, const void* dout, int n, int h, int wd, int c, int ld, int k, int stride,
                                float* dw, int accumulate, float* ws, size_t ws_bytes, void* stream) {
  TOK_CHECK_ARG(x && dout && dw && ws, "tok_dwconv_wgrad: null pointer");
  TOK_CHECK_ARG(dw_args_ok(n, h, wd, c, ld, k, stride), "tok_dwconv_wgrad: bad sizes (c %% 8 == 0, k in {3,5}, stride in {1,2})");
  TOK_CHECK_ARG(ws_bytes >= tok_dwconv_wgrad_ws_bytes(n, h, wd, c, k, stride), "tok_dwconv_wgrad: workspace too small");
  const int p = out_dim(h, k, stride), q = out_dim(wd, k, stride);
  const DwGeo g = dw_geo((long long)n * p, q, c, k);
  const dim3 grid(g.tiles, g.rows, k);
  hipStream_t st = tok_stream(stream);
#define TOK_DWW_CASE(K_, S_)                                                                                                 \
  if (k == K_ && stride == S_)                                                                                              \
    hipLaunchKernelGGL((dwconv_wgrad_kernel<K_, S_>), grid, dim3(256), 0, st, (const bf16*)x, (const bf16*)dout, n, h, wd, p, \
                       q, c, ld, g.cg, ws);
  TOK_DWW_CASE(3, 1) TOK_DWW_CASE(3, 2) TOK_DWW_CASE(5, 1) TOK_DWW_CASE(5, 2)
#undef TOK_DWW_CASE
  const int total = c * k * k;
  int blocks = (total + 255) / 256;
  if (blocks > kGridCap) blocks = kGridCap;
  hipLaunchKernelGGL(dwconv_wgrad_fold_kernel, dim3(blocks), dim3(256), 0, st, ws, g.rows, total, dw, accumulate);
  TOK_CHECK_LAUNCH("tok_dwconv_wgrad");
  return TOK_OK;
}
