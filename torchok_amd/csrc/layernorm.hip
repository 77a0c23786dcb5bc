// Row-wise and element-wise kernels of the token-major [rows][C] bf16 matrices (SwinV2 / ViT / BEiT blocks).
//   layernorm fwd/bwd       res-post-norm  x = shortcut + drop_path(LN(y))  (per-sample scale = stochastic depth), fp32 statistics
//   colsum_f32 (+ _pair)    fixed-order reduction of fp32 partial rows (dgamma/dbeta, dbias, dlogit_scale), fp64 accumulation
//   act fwd/bwd             GELU (erf) of the MLP, ReLU of the cpb_mlp
// Deterministic: no atomics.  (Window attention: window_attn.hip; position-bias gathers and patch merge: transformer.hip.)
#include "tok_common.h"
#include <type_traits>

namespace {

// sum over the LPR (16 / 32 / 64) consecutive lanes that hold one LayerNorm row
template <int LPR>
__device__ __forceinline__ float lpr_sum(float v) {
  v = row16_sum(v);
  if constexpr (LPR > 16) v += __shfl_xor(v, 16, 64);
  if constexpr (LPR > 32) v += __shfl_xor(v, 32, 64);
  return v;
}

// ---------------------------------------------------------------------------------------------------------------
// LayerNorm.  16-byte vector lanes: a row of c channels is covered by LPR lanes (16 / 32 / 64) holding VPL vectors
// of 8 channels each, so a wave normalises 64 / LPR rows at once and every global access is a full 16-byte lane
// (c % 8 == 0, c <= 1024).  Other widths (HRNet never, SwinV2 never) use the scalar one-wave-per-row kernels.
template <int LPR, int VPL>
__global__ __launch_bounds__(256) void ln_fwd_vec_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shortcut,
                                                         const float* __restrict__ row_scale, int rows_per_sample,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         bf16* __restrict__ out, float* __restrict__ mean,
                                                         float* __restrict__ rstd, int64_t rows, int c, float eps) {
  constexpr int RPW = 64 / LPR;                 // rows per wave
  const int lane = threadIdx.x & 63, sub = lane % LPR;
  const int64_t row = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * RPW + lane / LPR;
  const bool live = row < rows;
  const int cg = c >> 3;
  float v[VPL][8];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int g = sub + u * LPR;
    if (live && g < cg) {
      const bf16x8 t = ldg16(x + row * c + g * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) { v[u][e] = bf2f(t[e]); s += v[u][e]; }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[u][e] = 0.f;
    }
  }
  s = lpr_sum<LPR>(s);
  const float mu = s / (float)c;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u)
    if (sub + u * LPR < cg)
#pragma unroll
      for (int e = 0; e < 8; ++e) { const float d = v[u][e] - mu; q = fmaf(d, d, q); }
  q = lpr_sum<LPR>(q);
  const float rs = rsqrtf(q / (float)c + eps);
  if (!live) return;
  if (sub == 0) { mean[row] = mu; rstd[row] = rs; }
  const float sc = row_scale ? row_scale[row / rows_per_sample] : 1.f;
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int g = sub + u * LPR;
    if (g >= cg) continue;
    float ga[8], be[8];
    *reinterpret_cast<f32x4*>(ga) = *reinterpret_cast<const f32x4*>(gamma + g * 8);
    *reinterpret_cast<f32x4*>(ga + 4) = *reinterpret_cast<const f32x4*>(gamma + g * 8 + 4);
    *reinterpret_cast<f32x4*>(be) = *reinterpret_cast<const f32x4*>(beta + g * 8);
    *reinterpret_cast<f32x4*>(be + 4) = *reinterpret_cast<const f32x4*>(beta + g * 8 + 4);
    bf16x8 o;
    if (shortcut != nullptr) {
      const bf16x8 sh = ldg16(shortcut + row * c + g * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(((v[u][e] - mu) * rs * ga[e] + be[e]) * sc + bf2f(sh[e]));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(((v[u][e] - mu) * rs * ga[e] + be[e]) * sc);
    }
    stg16(out + row * c + g * 8, o);
  }
}

// backward: dx = rstd * (g - mean(g) - xhat * mean(g * xhat)), g = dout * scale * gamma; each lane keeps the dgamma /
// dbeta contributions of ITS 8*VPL columns in registers across all the rows it visits, then the lanes that own the
// same columns are folded through LDS -> one partial row per block (fixed order: deterministic)
template <int LPR, int VPL>
__global__ __launch_bounds__(256) void ln_bwd_vec_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ x,
                                                         const float* __restrict__ mean, const float* __restrict__ rstd,
                                                         const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                         int rows_per_sample, bf16* dx, int accumulate,
                                                         float* __restrict__ partial, int64_t rows, int c) {
  constexpr int RPW = 64 / LPR, RPB = 4 * RPW;  // rows per wave / per block pass
  extern __shared__ float sm[];                 // [RPB][2][c]
  const int lane = threadIdx.x & 63, sub = lane % LPR;
  const int rl = (threadIdx.x >> 6) * RPW + lane / LPR;     // row slot inside the block pass
  const int cg = c >> 3;
  float ga[VPL][8], pg[VPL][8], pb[VPL][8];
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int g = sub + u * LPR;
#pragma unroll
    for (int e = 0; e < 8; ++e) { ga[u][e] = g < cg ? gamma[g * 8 + e] : 0.f; pg[u][e] = 0.f; pb[u][e] = 0.f; }
  }
  // two row slots per iteration: all loads of both rows are requested before the first is consumed (one row per iteration
  // left a wave with two 16-byte loads in flight: 2.7 TB/s at 1024 blocks)
  constexpr int UNR = 2;
  for (int64_t row0 = (int64_t)blockIdx.x * RPB; row0 < rows; row0 += (int64_t)gridDim.x * RPB * UNR) {
    int64_t rowv[UNR];
    bool livev[UNR];
    bf16x8 xv[UNR][VPL], gv[UNR][VPL], pv[UNR][VPL];
    float muv[UNR], rsv[UNR], scv[UNR];
#pragma unroll
    for (int r = 0; r < UNR; ++r) {
      rowv[r] = row0 + (int64_t)r * gridDim.x * RPB + rl;
      livev[r] = rowv[r] < rows;
#pragma unroll
      for (int u = 0; u < VPL; ++u) {
        const int g = sub + u * LPR;
        const bool ok = livev[r] && g < cg;
        xv[r][u] = ok ? ldg16(x + rowv[r] * c + g * 8) : zero8();
        gv[r][u] = ok ? ldg16(dout + rowv[r] * c + g * 8) : zero8();
        pv[r][u] = (ok && accumulate) ? ldg16(dx + rowv[r] * c + g * 8) : zero8();
      }
      muv[r] = livev[r] ? mean[rowv[r]] : 0.f;
      rsv[r] = livev[r] ? rstd[rowv[r]] : 0.f;
      scv[r] = (livev[r] && row_scale) ? row_scale[rowv[r] / rows_per_sample] : 1.f;
    }
#pragma unroll
    for (int r = 0; r < UNR; ++r) {
      const int64_t row = rowv[r];
      const bool live = livev[r];
      const float mu = muv[r], rs = rsv[r], sc = scv[r];
      float xh[VPL][8], gg[VPL][8];
      float s1 = 0.f, s2 = 0.f;
#pragma unroll
      for (int u = 0; u < VPL; ++u) {
        const int g = sub + u * LPR;
        if (live && g < cg) {
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            xh[u][e] = (bf2f(xv[r][u][e]) - mu) * rs;
            const float go = bf2f(gv[r][u][e]) * sc;
            gg[u][e] = go * ga[u][e];
            s1 += gg[u][e];
            s2 = fmaf(gg[u][e], xh[u][e], s2);
            pg[u][e] = fmaf(go, xh[u][e], pg[u][e]);
            pb[u][e] += go;
          }
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) { xh[u][e] = 0.f; gg[u][e] = 0.f; }
        }
      }
      s1 = lpr_sum<LPR>(s1);
      s2 = lpr_sum<LPR>(s2);
      const float m1 = s1 / (float)c, m2 = s2 / (float)c;
      if (live)
#pragma unroll
        for (int u = 0; u < VPL; ++u) {
          const int g = sub + u * LPR;
          if (g >= cg) continue;
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = f2bf(rs * (gg[u][e] - m1 - xh[u][e] * m2) + bf2f(pv[r][u][e]));
          stg16(dx + row * c + g * 8, o);
        }
    }
  }
#pragma unroll
  for (int u = 0; u < VPL; ++u) {
    const int g = sub + u * LPR;
    if (g < cg)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        sm[((size_t)rl * 2 + 0) * c + g * 8 + e] = pg[u][e];
        sm[((size_t)rl * 2 + 1) * c + g * 8 + e] = pb[u][e];
      }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 2 * c; i += 256) {
    const int which = i / c, col = i - which * c;
    float t = 0.f;
    for (int r = 0; r < RPB; ++r) t += sm[((size_t)r * 2 + which) * c + col];
    partial[((size_t)which * gridDim.x + blockIdx.x) * c + col] = t;
  }
}

// scalar fallback: one wave per row.
__global__ __launch_bounds__(256) void ln_fwd_kernel(const bf16* __restrict__ x, const bf16* __restrict__ shortcut,
                                                     const float* __restrict__ row_scale, int rows_per_sample,
                                                     const float* __restrict__ gamma, const float* __restrict__ beta,
                                                     bf16* __restrict__ out, float* __restrict__ mean,
                                                     float* __restrict__ rstd, int64_t rows, int c, int ld, float eps) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const bf16* xr = x + row * ld;
  float s = 0.f;
  for (int i = lane; i < c; i += 64) s += bf2f(xr[i]);
  const float mu = wave_sum(s) / (float)c;
  float v = 0.f;
  for (int i = lane; i < c; i += 64) { const float d = bf2f(xr[i]) - mu; v = fmaf(d, d, v); }
  const float rs = rsqrtf(wave_sum(v) / (float)c + eps);
  if (lane == 0) { mean[row] = mu; rstd[row] = rs; }
  const float sc = row_scale ? row_scale[row / rows_per_sample] : 1.f;
  bf16* orow = out + row * ld;
  const bf16* srow = shortcut ? shortcut + row * ld : nullptr;
  for (int i = lane; i < ld; i += 64) {
    float o = 0.f;
    if (i < c) {
      o = ((bf2f(xr[i]) - mu) * rs * gamma[i] + beta[i]) * sc;
      if (srow) o += bf2f(srow[i]);
    }
    orow[i] = f2bf(o);
  }
}

// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dout * scale * gamma;  partial dgamma/dbeta per block
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ x,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, const float* __restrict__ row_scale,
                                                     int rows_per_sample, bf16* dx, int accumulate,
                                                     float* __restrict__ partial, int64_t rows, int c, int ld) {
  extern __shared__ float sm[];   // [4 waves][2][c]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  float* pg = sm + (size_t)wv * 2 * c;
  float* pb = pg + c;
  for (int i = lane; i < c; i += 64) { pg[i] = 0.f; pb[i] = 0.f; }
  for (int64_t row = (int64_t)blockIdx.x * 4 + wv; row < rows; row += (int64_t)gridDim.x * 4) {
    const bf16* xr = x + row * ld;
    const bf16* gr = dout + row * ld;
    const float mu = mean[row], rs = rstd[row];
    const float sc = row_scale ? row_scale[row / rows_per_sample] : 1.f;
    float s1 = 0.f, s2 = 0.f;
    for (int i = lane; i < c; i += 64) {
      const float xh = (bf2f(xr[i]) - mu) * rs;
      const float go = bf2f(gr[i]) * sc;
      const float g = go * gamma[i];
      s1 += g;
      s2 = fmaf(g, xh, s2);
      pg[i] = fmaf(go, xh, pg[i]);   // each lane owns its columns: no conflicts inside a wave
      pb[i] += go;
    }
    const float m1 = wave_sum(s1) / (float)c, m2 = wave_sum(s2) / (float)c;
    bf16* dr = dx + row * ld;
    for (int i = lane; i < ld; i += 64) {
      float o = 0.f;
      if (i < c) {
        const float xh = (bf2f(xr[i]) - mu) * rs;
        o = rs * (bf2f(gr[i]) * sc * gamma[i] - m1 - xh * m2);
        if (accumulate) o += bf2f(dr[i]);
      }
      dr[i] = f2bf(o);
    }
  }
  __syncthreads();
  // partial [2][gridDim.x][c]: dgamma rows, then dbeta rows
  for (int i = threadIdx.x; i < 2 * c; i += 256) {
    const float v = sm[i] + sm[2 * c + i] + sm[4 * c + i] + sm[6 * c + i];
    if (i < c) partial[(size_t)blockIdx.x * c + i] = v;
    else partial[((size_t)gridDim.x + blockIdx.x) * c + (i - c)] = v;
  }
}

// dst[col] (+)= sum_r src[r][col], fixed order, fp64 accumulation.  blockIdx.y = 1: the second (src, dst, accumulate) of a pair
// launch (LayerNorm's d(gamma) and d(beta) rows in one launch: 48 small launches less per SwinV2-T step)
template <int U>
__device__ __forceinline__ void colsum_rows(const float* __restrict__ s0, int64_t rows, int cols, int rl, double& a) {
  for (int64_t r = rl; r < rows; r += 16 * U) {
    float v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r + 16 * u;
      v[u] = s0[(ru < rows ? ru : rows - 1) * cols];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) a += r + 16 * u < rows ? (double)v[u] : 0.0;
  }
}

__global__ __launch_bounds__(256) void colsum_f32_kernel(const float* __restrict__ src, int64_t rows, int cols,
                                                         float* dst, int accumulate, const float* __restrict__ src1,
                                                         float* dst1, int accumulate1) {
  __shared__ double red[256];
  if (blockIdx.y == 1) { src = src1; dst = dst1; accumulate = accumulate1; }
  const int cl = threadIdx.x & 15, rl = threadIdx.x >> 4;
  const int col = blockIdx.x * 16 + cl;
  double a = 0.0;
  if (col < cols) {
    const float* s0 = src + col;
    // as many loads in flight per lane as it has rows, up to 32; additions in row order (round 5: with 8 in flight the 1024
    // partial rows of an activation pass were eight dependent L2-miss rounds, 6 us on the forward chain of every fused
    // residual unit; the loads are unconditional, so short folds keep the 8-wide form)
    if (rows > 128) colsum_rows<32>(s0, rows, cols, rl, a);
    else colsum_rows<8>(s0, rows, cols, rl, a);
  }
  red[threadIdx.x] = a;
  __syncthreads();
  for (int s = 8; s > 0; s >>= 1) {
    if (rl < s) red[threadIdx.x] += red[threadIdx.x + s * 16];
    __syncthreads();
  }
  if (rl == 0 && col < cols) dst[col] = (float)red[threadIdx.x] + (accumulate ? dst[col] : 0.f);
}

// The same fold for WIDE matrices (window attention's d(bias) partials: 64 ... 1024 rows of 7 203 ... 57 624 columns, 15-30 MB
// per launch, twelve launches per SwinV2-T step).  colsum_f32_kernel gives a block 16 columns: a wave instruction touches four
// rows x 64 bytes, and the fold ran at ~160 GB/s (up to 360 us per launch, 1.2 ms of a step on the position-bias stream).
// Here a block owns 256 columns and a wave instruction reads 256 contiguous bytes of ONE row (lane l: columns l, l + 64,
// l + 128, l + 192 — no alignment condition: 49 x 49 x heads is odd for three heads); the block's sixteen waves take the rows
// round-robin, sixteen loads in flight per lane, and are folded through LDS in wave order; fp64 accumulation in row order per
// wave like the narrow kernel (deterministic; the order of additions differs from the narrow kernel's, which no caller mixes
// on one tensor).
__global__ __launch_bounds__(1024) void colsum_f32_wide_kernel(const float* __restrict__ src, int64_t rows, int cols,
                                                               float* dst, int accumulate) {
  __shared__ double red[16][4][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int col0 = blockIdx.x * 256 + lane;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  constexpr int U = 4;
  for (int64_t r = wv; r < rows; r += 16 * U) {
    float v[U][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ru = r + 16 * u;
      const float* s0 = src + (ru < rows ? ru : rows - 1) * cols;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int c = col0 + 64 * e;
        v[u][e] = s0[c < cols ? c : cols - 1];
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (r + 16 * u < rows)
#pragma unroll
        for (int e = 0; e < 4; ++e) a[e] += (double)v[u][e];
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[wv][e][lane] = a[e];
  __syncthreads();
  if (wv < 4) {                      // wave e folds column slot e
    const int c = col0 + 64 * wv;
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w][wv][lane];
    if (c < cols) dst[c] = (float)t + (accumulate ? dst[c] : 0.f);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// activations (kind 0 = ReLU, 1 = GELU erf)
// gelu_f / gelu_d: tok_common.h (shared with the GEMM epilogues of conv_igemm.hip)

__global__ __launch_bounds__(256) void act_fwd_kernel(int kind, const bf16* __restrict__ x, bf16* __restrict__ out,
                                                      size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const bf16x8 v = ldg16(x + i * 8);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = bf2f(v[e]);
      o[e] = f2bf(kind == 0 ? fmaxf(f, 0.f) : gelu_f(f));
    }
    stg16(out + i * 8, o);
  }
}

__global__ __launch_bounds__(256) void act_bwd_kernel(int kind, const bf16* __restrict__ dout,
                                                      const bf16* __restrict__ x, bf16* dx, int accumulate, size_t n8) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (size_t)gridDim.x * 256) {
    const bf16x8 v = ldg16(x + i * 8), g = ldg16(dout + i * 8);
    bf16x8 o;
    bf16x8 prev = accumulate ? ldg16(dx + i * 8) : zero8();
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = bf2f(v[e]);
      const float d = kind == 0 ? (f > 0.f ? 1.f : 0.f) : (kind == 1 ? gelu_d(f) : 1.f);
      o[e] = f2bf(bf2f(g[e]) * d + bf2f(prev[e]));
    }
    stg16(dx + i * 8, o);
  }
}

inline int blocks_for(size_t total) {     // grid of the grid-stride activation kernels (as in transformer.hip)
  const size_t b = (total + 255) / 256;
  return (int)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

// the vector kernels serve dense rows of whole 16-byte lanes up to 1024 channels; everything else takes the one-wave-per-row pair
inline bool ln_vec_serves(int c, int ld) { return c == ld && c % 8 == 0 && c <= 1024; }

// (LPR, VPL) of the vector kernels for a row of c channels: f(integral_constant<LPR>, integral_constant<VPL>)
template <class F>
void ln_with_lanes(int c, F&& f) {
  using std::integral_constant;
  const int cg = c >> 3;
  if (cg <= 16) f(integral_constant<int, 16>{}, integral_constant<int, 1>{});
  else if (cg <= 32) f(integral_constant<int, 32>{}, integral_constant<int, 1>{});
  else if (cg <= 64) f(integral_constant<int, 64>{}, integral_constant<int, 1>{});
  else f(integral_constant<int, 64>{}, integral_constant<int, 2>{});
}

}  // namespace

extern "C" int tok_layernorm_fwd(const void* x, const void* shortcut, const float* row_scale, int rows_per_sample,
                                 const float* gamma, const float* beta, void* out, float* mean, float* rstd,
                                 int64_t rows, int c, int ld, float eps, void* stream) {
  TOK_CHECK_ARG(x && gamma && beta && out && mean && rstd && rows > 0 && c > 0 && ld >= c, "tok_layernorm_fwd: bad args");
  TOK_CHECK_ARG(!row_scale || rows_per_sample > 0, "tok_layernorm_fwd: rows_per_sample");
  hipStream_t st = tok_stream(stream);
  if (ln_vec_serves(c, ld)) {
    ln_with_lanes(c, [&](auto lpr, auto vpl) {
      constexpr int LPR = decltype(lpr)::value, VPL = decltype(vpl)::value;
      hipLaunchKernelGGL((ln_fwd_vec_kernel<LPR, VPL>), dim3((unsigned)tok_cdiv(rows, 4 * (64 / LPR))), dim3(256), 0, st,
                         (const bf16*)x, (const bf16*)shortcut, row_scale, rows_per_sample, gamma, beta, (bf16*)out, mean,
                         rstd, rows, c, eps);
    });
  } else {
    hipLaunchKernelGGL(ln_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, st, (const bf16*)x,
                       (const bf16*)shortcut, row_scale, rows_per_sample, gamma, beta, (bf16*)out, mean, rstd, rows, c, ld,
                       eps);
  }
  TOK_CHECK_LAUNCH("tok_layernorm_fwd");
  return TOK_OK;
}

extern "C" int tok_layernorm_bwd_rows(int64_t rows, int c) {
  const int64_t b = (rows + 3) / 4;
  (void)c;
  // four blocks per CU = what is resident at 102 registers; the partial d(gamma) / d(beta) rows the fold reads scale with the
  // grid (SwinV2-T B=256, ms/step: 512 20.42, 1024 20.37, 2048 20.43, 4096 20.59, 8192 20.97)
  constexpr int cap = 1024;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

extern "C" int tok_layernorm_bwd(const void* dout, const void* x, const float* mean, const float* rstd,
                                 const float* gamma, const float* row_scale, int rows_per_sample, void* dx,
                                 int accumulate, float* partial, int64_t rows, int c, int ld, void* stream) {
  TOK_CHECK_ARG(dout && x && mean && rstd && gamma && dx && partial && rows > 0 && c > 0 && ld >= c,
                "tok_layernorm_bwd: bad args");
  const int g = tok_layernorm_bwd_rows(rows, c);
  hipStream_t st = tok_stream(stream);
  if (ln_vec_serves(c, ld)) {
    ln_with_lanes(c, [&](auto lpr, auto vpl) {
      constexpr int LPR = decltype(lpr)::value, VPL = decltype(vpl)::value;
      const size_t smem = (size_t)(4 * (64 / LPR)) * 2 * c * sizeof(float);
      hipLaunchKernelGGL((ln_bwd_vec_kernel<LPR, VPL>), dim3(g), dim3(256), smem, st, (const bf16*)dout, (const bf16*)x, mean,
                         rstd, gamma, row_scale, rows_per_sample, (bf16*)dx, accumulate, partial, rows, c);
    });
  } else {
    TOK_CHECK_ARG((size_t)c * 8 * sizeof(float) <= 64 * 1024, "tok_layernorm_bwd: c too large (%d)", c);
    hipLaunchKernelGGL(ln_bwd_kernel, dim3(g), dim3(256), (size_t)c * 8 * sizeof(float), st, (const bf16*)dout,
                       (const bf16*)x, mean, rstd, gamma, row_scale, rows_per_sample, (bf16*)dx, accumulate, partial,
                       rows, c, ld);
  }
  TOK_CHECK_LAUNCH("tok_layernorm_bwd");
  return TOK_OK;
}

extern "C" int tok_colsum_f32(const float* src, int64_t rows, int cols, float* dst, int accumulate, void* stream) {
  TOK_CHECK_ARG(src && dst && rows > 0 && cols > 0, "tok_colsum_f32: bad args");
  if (tok_dbg_skip(4)) return TOK_OK;
  if (cols >= 2048) {
    hipLaunchKernelGGL(colsum_f32_wide_kernel, dim3((cols + 255) / 256), dim3(1024), 0, tok_stream(stream), src, rows, cols, dst,
                       accumulate);
    TOK_CHECK_LAUNCH("tok_colsum_f32(wide)");
    return TOK_OK;
  }
  hipLaunchKernelGGL(colsum_f32_kernel, dim3((cols + 15) / 16), dim3(256), 0, tok_stream(stream), src, rows, cols, dst,
                     accumulate, (const float*)nullptr, (float*)nullptr, 0);
  TOK_CHECK_LAUNCH("tok_colsum_f32");
  return TOK_OK;
}

extern "C" int tok_colsum_f32_pair(const float* src0, const float* src1, int64_t rows, int cols, float* dst0, int accumulate0,
                                   float* dst1, int accumulate1, void* stream) {
  TOK_CHECK_ARG(src0 && src1 && dst0 && dst1 && rows > 0 && cols > 0, "tok_colsum_f32_pair: bad args");
  hipLaunchKernelGGL(colsum_f32_kernel, dim3((cols + 15) / 16, 2), dim3(256), 0, tok_stream(stream), src0, rows, cols, dst0,
                     accumulate0, src1, dst1, accumulate1);
  TOK_CHECK_LAUNCH("tok_colsum_f32_pair");
  return TOK_OK;
}

extern "C" int tok_act_fwd(int kind, const void* x, void* out, size_t count, void* stream) {
  TOK_CHECK_ARG(x && out && count > 0 && count % 8 == 0 && (kind == 0 || kind == 1), "tok_act_fwd: bad args");
  TOK_CHECK_ARG(tok_aligned(x, 16) && tok_aligned(out, 16), "tok_act_fwd: x / out must be 16-byte aligned");
  hipLaunchKernelGGL(act_fwd_kernel, dim3(blocks_for(count / 8)), dim3(256), 0, tok_stream(stream), kind, (const bf16*)x,
                     (bf16*)out, count / 8);
  TOK_CHECK_LAUNCH("tok_act_fwd");
  return TOK_OK;
}

extern "C" int tok_act_bwd(int kind, const void* dout, const void* x, void* dx, int accumulate, size_t count,
                           void* stream) {
  TOK_CHECK_ARG(dout && x && dx && count > 0 && count % 8 == 0 && kind >= 0 && kind <= 2, "tok_act_bwd: bad args");
  TOK_CHECK_ARG(tok_aligned(dout, 16) && tok_aligned(x, 16) && tok_aligned(dx, 16), "tok_act_bwd: dout / x / dx must be 16-byte aligned");
  hipLaunchKernelGGL(act_bwd_kernel, dim3(blocks_for(count / 8)), dim3(256), 0, tok_stream(stream), kind,
                     (const bf16*)dout, (const bf16*)x, (bf16*)dx, accumulate, count / 8);
  TOK_CHECK_LAUNCH("tok_act_bwd");
  return TOK_OK;
}
