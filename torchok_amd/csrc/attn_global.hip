// Global (whole-image) multi-head self-attention of the Vision Transformer and its token-embedding helpers.
//
// [timm 0.6.13] vision_transformer.Attention.forward between qkv and proj:
//   q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4);  O = softmax(q k^T * 64^-0.5) v;  O.transpose(1, 2).reshape(B, N, C)
// qkv rows bf16 [B*N][ldq] with columns (3, heads, 64); O rows bf16 [B*N][ldo] at column h*64 + d; lse fp32 [B][H][N] (natural log).
//
// Forward : one workgroup per (image, head, 64-query tile), one wave per 16 queries.  K / V tiles of 64 keys are staged in LDS (V
//           transposed), S = Q K^T and O += P V on mfma_f32_16x16x32_bf16, online fp32 softmax in exp2 units, key tail masked.
// Backward: delta = rowsum(dO o O) (pre-pass); dK / dV per (image, head, 64-key tile), dQ per (image, head, 64-query tile), each
//           recomputing P from Q, K and the LSE.  Every output element is written by exactly one lane and every sum runs in a fixed
//           order: no float atomics, bit-reproducible run to run.
// Bias    : BEiT's relative-position bias ([timm 0.6.13] beit.Attention) is one more template argument of the same kernels:
//           softmax(q k^T * 64^-0.5 + bias[h]); its gradient is a reduction over the images (gattn_dbias_kernel).
// Pieces  : the four MFMA kernels (fwd, dkv, dq, dbias) are written on load_rows16 (16 token rows as an A operand), frag_x_tile
//           (operand x row-major LDS tile), rows_x_tile_t (staged rows x transposed LDS tile), load_row_stats (LSE and delta of a
//           lane's four queries), prob and ds_tile (P and dS = P (dP - delta), shared by dq and dbias).  What these pieces
//           multiply and add is written as fmaf where it is fused and as mul_rn / sub_rn where it is not, so that hipcc's
//           contraction cannot differ between the callers; the three forms of the bias term are listed at prob.
//           On the host one launcher serves both forward entry points and one routine both backward ones (bias == nullptr picks
//           the un-biased kernels).
#include "tok_common.h"

namespace {

constexpr int HD = 64;         // head_dim served
constexpr int TL = 64;         // tokens per tile (queries of a workgroup, keys per staged tile)
constexpr int PT = 72;         // LDS row pitch in bf16 (144 B: 16-B aligned rows)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr float SCALE = 0.125f;  // 64^-0.5

__device__ __forceinline__ bf16x8 lds8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// rows [r0, r0 + 64) of the 64-wide column block `col` of a token matrix -> LDS row-major [row][PT] and/or transposed [d][PT];
// rows past n are zero
__device__ __forceinline__ void stage_tile(const bf16* __restrict__ base, int ld, int col, int r0, int n, bf16* rm, bf16* tr) {
  for (int c = threadIdx.x; c < TL * (HD / 8); c += 256) {
    const int row = c >> 3, d0 = (c & 7) * 8, gr = r0 + row;
    const bf16x8 v = gr < n ? ldg16(base + (size_t)gr * ld + col + d0) : zero8();
    if (rm) *reinterpret_cast<bf16x8*>(rm + row * PT + d0) = v;
    if (tr) {
#pragma unroll
      for (int j = 0; j < 8; ++j) tr[(d0 + j) * PT + row] = v[j];
    }
  }
}

__device__ __forceinline__ float max16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ float sum16(float v) {
#pragma unroll
  for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- the pieces the four MFMA kernels are written on ---------------------------------------------------------------------------
// A lane is (l15, g) = (lane & 15, lane >> 4) of its wave.  Element (j, r) of a product, j the f32x4 of four and r its component,
// is row 4 g + r of the A operand's 16 rows against row 16 j + l15 of the 64-row LDS tile.  Every accumulator takes t = 0, then
// t = 1 (the two halves of the 64-wide reduction): the bits of every output depend on that order.

// a * b and a - b rounded on their own.  hipcc contracts a * b + c wherever both operations allow it, and the __fmul_rn / __fsub_rn
// of this toolchain are the plain operators, which fuse like any other: what must stay unfused is written under contract(off),
// what is fused is written fmaf.
__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float sub_rn(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// token rows [r0, r0 + 16) of the 64-wide column block `col` as an A operand (the lane: row r0 + l15, columns 32 t + 8 g ... + 7);
// rows past n are zero
__device__ __forceinline__ void load_rows16(const bf16* __restrict__ base, int ld, int col, int r0, int n, int l15, int g,
                                            bf16x8 (&f)[2]) {
  const int row = r0 + l15;
#pragma unroll
  for (int t = 0; t < 2; ++t) f[t] = row < n ? ldg16(base + (size_t)row * ld + col + 32 * t + 8 * g) : zero8();
}

// acc = a x tile^T, tile a row-major LDS tile [64][PT]
__device__ __forceinline__ void frag_x_tile(const bf16x8 (&a)[2], const bf16* tile, int l15, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 2; ++t)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], lds8(tile + (j * 16 + l15) * PT + 32 * t + 8 * g), acc[j], 0, 0, 0);
  }
}

// acc += rows x tile_t^T: the [16][PT] rows a wave staged in LDS (P, dS or their transposes) times a transposed LDS tile [d][PT]
__device__ __forceinline__ void rows_x_tile_t(const bf16* rows, const bf16* tile_t, int l15, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bf16x8 a = lds8(rows + l15 * PT + 32 * t + 8 * g);
#pragma unroll
    for (int j = 0; j < 4; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, lds8(tile_t + (j * 16 + l15) * PT + 32 * t + 8 * g), acc[j], 0, 0, 0);
  }
}

// log-sum-exp in log2 units (INFINITY past n: P = 0) and delta (0 past n) of the query rows q ... q + 3
__device__ __forceinline__ void load_row_stats(const float* __restrict__ lrow, const float* __restrict__ drow, int q, int n,
                                               float (&lr)[4], float (&dr)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = q + r < n ? mul_rn(lrow[q + r], LOG2E) : INFINITY;
    dr[r] = q + r < n ? drow[q + r] : 0.f;
  }
}

// P = exp2(s * 64^-0.5 * log2e - lb) in one fused multiply-subtract; lb is the query's log-sum-exp less the bias term, both in
// log2 units.
// The bias term enters in three forms, each pinned to what its kernel has always computed, so the caller forms it:
//   forward          bl = bias * log2e rounded, then fma(s, sc, bl)
//   dK/dV and dQ     lb = fma(-bias, log2e, lse): one rounding
//   d(bias)          lb = lse - bl with bl = bias * log2e rounded: two roundings (bl is loaded once per tile, outside the image loop)
// so the P of the backward is not the same float in d(bias) as in dQ.  Making them one form changes output bits.
__device__ __forceinline__ float prob(float s, float lb) { return exp2f(fmaf(s, SCALE * LOG2E, -lb)); }

// dS = P (dP - delta) of the wave's 16 queries against the 64 keys from k0: sink(kj, r, p, d) takes the two factors of element
// (kj, r), dS = p * d, with p = 0 for a key past n.  lb(kj, r, live) is the caller's log-sum-exp less bias term (see prob).
// gattn_dq_kernel rounds the product to bf16, gattn_dbias_kernel fuses it into its sum over the images.
template <class Lb, class Sink>
__device__ __forceinline__ void ds_tile(const f32x4 (&s)[4], const f32x4 (&dp)[4], const float (&dr)[4], int k0, int n, int l15,
                                        Lb&& lb, Sink&& sink) {
#pragma unroll
  for (int kj = 0; kj < 4; ++kj) {
    const bool live = k0 + kj * 16 + l15 < n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = prob(s[kj][r], lb(kj, r, live));
      sink(kj, r, live ? p : 0.f, dp[kj][r] - dr[r]);
    }
  }
}

// BIAS: logits get + bias[h][query][key] (fp32, row pitch ldb, shared by every image); columns >= N of a bias row and rows of
// queries >= N are never loaded.  Without it the kernel is the one the un-biased entry point has always launched.
template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_fwd_kernel(const bf16* __restrict__ qkv, int ldq, int N, int H,
                                                        bf16* __restrict__ out, int ldo, float* __restrict__ lse,
                                                        const float* __restrict__ bias, int ldb) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PT];        // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vt[HD * PT];        // V^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 ps[4][16 * PT];     // per wave: P [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / H, h = blockIdx.y % H, C = H * HD;
  const int q0 = blockIdx.x * TL + wv * 16;
  const bf16* base = qkv + (size_t)b * N * ldq;
  bf16x8 qf[2];
  load_rows16(base, ldq, h * HD, q0, N, l15, g, qf);
  float m[4], l[4];
  f32x4 o[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
    o[r] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float sc = SCALE * LOG2E;
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();                                    // the previous tile has been consumed by every wave
    stage_tile(base, ldq, C + h * HD, k0, N, ks, nullptr);
    stage_tile(base, ldq, 2 * C + h * HD, k0, N, nullptr, vt);
    __syncthreads();
    f32x4 s[4];
    frag_x_tile(qf, ks, l15, g, s);
    // element (kj, r): query 4g + r of the wave's 16, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[4], mx = -INFINITY;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        if constexpr (BIAS) {
          const int q = q0 + 4 * g + r;
          const float bl = (key < N && q < N) ? mul_rn(bias[((size_t)h * N + q) * ldb + key], LOG2E) : 0.f;
          v[kj] = (key < N) ? fmaf(s[kj][r], sc, bl) : -INFINITY;
        } else {
          v[kj] = (key < N) ? s[kj][r] * sc : -INFINITY;
        }
        mx = fmaxf(mx, v[kj]);
      }
      const float mn = fmaxf(m[r], max16(mx));           // finite: key k0 < N is in every tile
      const float alpha = exp2f(m[r] - mn);
      float ls = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float p = exp2f(v[kj] - mn);
        ls += p;
        ps[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(p);
      }
      l[r] = l[r] * alpha + sum16(ls);
      m[r] = mn;
#pragma unroll
      for (int dj = 0; dj < 4; ++dj) o[dj][r] *= alpha;
    }
    __syncthreads();
    rows_x_tile_t(ps[wv], vt, l15, g, o);
  }
  // o[dj][r]: query q0 + 4g + r, dim 16 dj + l15
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    const float inv = 1.f / l[r];
    bf16* orow = out + ((size_t)b * N + q) * ldo + h * HD;
#pragma unroll
    for (int dj = 0; dj < 4; ++dj) orow[dj * 16 + l15] = f2bf(o[dj][r] * inv);
    if (l15 == 0) lse[((size_t)b * H + h) * N + q] = (m[r] + log2f(l[r])) * LN2;
  }
}

// delta[b][h][q] = sum_d dO[q][h*64+d] * O[q][h*64+d]   (one thread per (token, head), fixed order over d)
__global__ __launch_bounds__(256) void gattn_delta_kernel(const bf16* __restrict__ out, const bf16* __restrict__ dout, int ldo,
                                                          int B, int N, int H, float* __restrict__ delta) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * N * H) return;
  const int h = (int)(i % H);
  const int64_t row = i / H;
  const int b = (int)(row / N), q = (int)(row % N);
  const bf16* po = out + row * ldo + h * HD;
  const bf16* pd = dout + row * ldo + h * HD;
  float acc = 0.f;
#pragma unroll
  for (int c = 0; c < HD; c += 8) {
    const bf16x8 a = ldg16(po + c), d = ldg16(pd + c);
#pragma unroll
    for (int j = 0; j < 8; ++j) acc = fmaf(bf2f(a[j]), bf2f(d[j]), acc);
  }
  delta[((size_t)b * H + h) * N + q] = acc;
}

// dK, dV of 64 keys: a wave owns 16 keys and walks every query tile
template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_dkv_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                        int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                        int N, int H, bf16* __restrict__ dqkv, int ldd,
                                                        const float* __restrict__ bias, int ldb) {
  __shared__ __attribute__((aligned(16))) bf16 qs[TL * PT];       // Q [query][d]
  __shared__ __attribute__((aligned(16))) bf16 qt[HD * PT];       // Q^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 dos[TL * PT];      // dO [query][d]
  __shared__ __attribute__((aligned(16))) bf16 dot[HD * PT];      // dO^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: P^T, then dS^T [key][query]
  __shared__ float lsl[TL], dl[TL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / H, h = blockIdx.y % H, C = H * HD;
  const int k0 = blockIdx.x * TL + wv * 16;
  const bf16* base = qkv + (size_t)b * N * ldq;
  const bf16* dbase = dout + (size_t)b * N * ldo;
  const float* lrow = lse + ((size_t)b * H + h) * N;
  const float* drow = delta + ((size_t)b * H + h) * N;
  bf16x8 kf[2], vf[2];
  load_rows16(base, ldq, C + h * HD, k0, N, l15, g, kf);
  load_rows16(base, ldq, 2 * C + h * HD, k0, N, l15, g, vf);
  f32x4 dk[4], dv[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dk[j] = dv[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TL) {
    __syncthreads();
    stage_tile(base, ldq, h * HD, q0, N, qs, qt);
    stage_tile(dbase, ldo, h * HD, q0, N, dos, dot);
    if (threadIdx.x < TL) {
      const int q = q0 + threadIdx.x;
      lsl[threadIdx.x] = q < N ? lrow[q] * LOG2E : INFINITY;      // queries past N: P = 0
      dl[threadIdx.x] = q < N ? drow[q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
    frag_x_tile(kf, qs, l15, g, st);
    frag_x_tile(vf, dos, l15, g, dpt);
    // S^T and dP^T leave the accumulator file here, in one go: without it hipcc schedules a v_accvgpr_read of the next element
    // onto the data register of a ds_write_b16 of P^T still in flight (tools/isa_lint.py; the note at the delta reduction of
    // attn_bwd_mfma_kernel in window_attn.hip)
    asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(dpt[0]), "+v"(dpt[1]), "+v"(dpt[2]), "+v"(dpt[3]));
    // element (qj, r): key k0 + 4g + r, query q0 + 16 qj + l15
    float dsv[4][4];
#pragma unroll
    for (int qj = 0; qj < 4; ++qj) {
      const int ql = qj * 16 + l15;
      const float lq = lsl[ql], dq = dl[ql];
      float lqb[4] = {lq, lq, lq, lq};
      if constexpr (BIAS) {
        // keys k0 + 4g ... + 3 of query row q0 + ql: one aligned 16-byte load (ldb % 4 == 0 keeps it inside the row)
        const int q = q0 + ql, kb = k0 + 4 * g;
        if (q < N && kb < N) {
          const float4 b4 = *reinterpret_cast<const float4*>(bias + ((size_t)h * N + q) * ldb + kb);
          const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) lqb[r] = kb + r < N ? fmaf(-bv[r], LOG2E, lq) : lq;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = prob(st[qj][r], lqb[r]);
        ws[wv][(4 * g + r) * PT + ql] = f2bf(p);
        dsv[qj][r] = p * (dpt[qj][r] - dq);
      }
    }
    __syncthreads();
    rows_x_tile_t(ws[wv], dot, l15, g, dv);
    __syncthreads();
#pragma unroll
    for (int qj = 0; qj < 4; ++qj)
#pragma unroll
      for (int r = 0; r < 4; ++r) ws[wv][(4 * g + r) * PT + qj * 16 + l15] = f2bf(dsv[qj][r]);
    __syncthreads();
    rows_x_tile_t(ws[wv], qt, l15, g, dk);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + 4 * g + r;
    if (k >= N) continue;
    bf16* row = dqkv + ((size_t)b * N + k) * ldd + h * HD;
#pragma unroll
    for (int dj = 0; dj < 4; ++dj) {
      row[C + dj * 16 + l15] = f2bf(dk[dj][r] * SCALE);
      row[2 * C + dj * 16 + l15] = f2bf(dv[dj][r]);
    }
  }
}

// dQ of 64 queries: a wave owns 16 queries and walks every key tile
template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_dq_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                       int N, int H, bf16* __restrict__ dqkv, int ldd,
                                                       const float* __restrict__ bias, int ldb) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PT];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kt[HD * PT];       // K^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PT];       // V [key][d]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: dS [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / H, h = blockIdx.y % H, C = H * HD;
  const int q0 = blockIdx.x * TL + wv * 16;
  const bf16* base = qkv + (size_t)b * N * ldq;
  bf16x8 qf[2], df[2];
  load_rows16(base, ldq, h * HD, q0, N, l15, g, qf);
  load_rows16(dout + (size_t)b * N * ldo, ldo, h * HD, q0, N, l15, g, df);
  float lr[4], dr[4];
  load_row_stats(lse + ((size_t)b * H + h) * N, delta + ((size_t)b * H + h) * N, q0 + 4 * g, N, lr, dr);
  f32x4 dq[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile(base, ldq, C + h * HD, k0, N, ks, kt);
    stage_tile(base, ldq, 2 * C + h * HD, k0, N, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile(qf, ks, l15, g, s);
    frag_x_tile(df, vs, l15, g, dp);
    // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
    ds_tile(s, dp, dr, k0, N, l15,
            [&](int kj, int r, bool live) {
              if constexpr (BIAS) {
                const int q = q0 + 4 * g + r;
                if (live && q < N) return fmaf(-bias[((size_t)h * N + q) * ldb + k0 + kj * 16 + l15], LOG2E, lr[r]);
              }
              return lr[r];
            },
            [&](int kj, int r, float p, float d) { ws[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(p * d); });
    __syncthreads();
    rows_x_tile_t(ws[wv], kt, l15, g, dq);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    bf16* row = dqkv + ((size_t)b * N + q) * ldd + h * HD;
#pragma unroll
    for (int dj = 0; dj < 4; ++dj) row[dj * 16 + l15] = f2bf(dq[dj][r] * SCALE);
  }
}

// d(bias)[h][i][j] = sum over images of dS_b[i][j] = P_b (dP_b - delta_b): one workgroup per (64-query x 64-key tile, head, chunk
// of images), a wave owns 16 queries.  The workgroup walks the images of its chunk in image order, recomputes S and dP of its tile
// (16 MFMA per wave and image) and keeps the fp32 sum in registers; the bias values of the tile are loaded once.  Partials
// [chunk][h][N][ldb] are folded in chunk order by gattn_dbias_fold_kernel: no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void gattn_dbias_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                          int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const float* __restrict__ bias, int ldb, int B, int N, int H,
                                                          int per_chunk, float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PT];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PT];       // V [key][d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int nt = (N + TL - 1) / TL;
  const int h = blockIdx.y, C = H * HD;
  const int q0 = (blockIdx.x / nt) * TL + wv * 16, k0 = (blockIdx.x % nt) * TL;
  const int b_lo = blockIdx.z * per_chunk, b_hi = min(B, b_lo + per_chunk);
  float bl[4][4];
#pragma unroll
  for (int kj = 0; kj < 4; ++kj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r, key = k0 + kj * 16 + l15;
      bl[kj][r] = (q < N && key < N) ? mul_rn(bias[((size_t)h * N + q) * ldb + key], LOG2E) : 0.f;
    }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int b = b_lo; b < b_hi; ++b) {
    const bf16* base = qkv + (size_t)b * N * ldq;
    __syncthreads();                                    // the previous image's tiles have been consumed by every wave
    stage_tile(base, ldq, C + h * HD, k0, N, ks, nullptr);
    stage_tile(base, ldq, 2 * C + h * HD, k0, N, vs, nullptr);
    bf16x8 qf[2], df[2];
    load_rows16(base, ldq, h * HD, q0, N, l15, g, qf);
    load_rows16(dout + (size_t)b * N * ldo, ldo, h * HD, q0, N, l15, g, df);
    float lr[4], dr[4];
    load_row_stats(lse + ((size_t)b * H + h) * N, delta + ((size_t)b * H + h) * N, q0 + 4 * g, N, lr, dr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile(qf, ks, l15, g, s);
    frag_x_tile(df, vs, l15, g, dp);
    ds_tile(s, dp, dr, k0, N, l15, [&](int kj, int r, bool) { return sub_rn(lr[r], bl[kj][r]); },
            [&](int kj, int r, float p, float d) { acc[kj][r] = fmaf(p, d, acc[kj][r]); });
  }
  float* dst = part + (size_t)blockIdx.z * H * N * ldb;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const int key = k0 + kj * 16 + l15;
      if (key < N) dst[((size_t)h * N + q) * ldb + key] = acc[kj][r];
    }
  }
}

// dbias[h][i][j] (=|+=) sum_chunk part[chunk][h][i][j], chunk order; columns >= N of a row are not touched
__global__ __launch_bounds__(256) void gattn_dbias_fold_kernel(const float* __restrict__ part, int chunks, int H, int N, int ldb,
                                                               float* __restrict__ dbias, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * N * N) return;
  const int j = (int)(i % N);
  const int64_t row = i / N;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[((size_t)c * H * N + row) * ldb + j];
  float* o = dbias + row * ldb + j;
  *o = accumulate ? *o + s : s;
}

// ---- embedding helpers ------------------------------------------------------------------------------------------------------
// img NHWC bf16 [n][h][w][4] -> rows [n * (h/p) * (w/p)][p * p * 4]: one thread per pixel (8 bytes)
__global__ __launch_bounds__(256) void patch_gather_kernel(const uint2* __restrict__ img, int n, int h, int w, int p,
                                                           uint2* __restrict__ rows) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)n * h * w) return;
  const int x = (int)(i % w);
  const int64_t t = i / w;
  const int y = (int)(t % h), b = (int)(t / h);
  const int gh = h / p, gw = w / p;
  const int64_t row = ((int64_t)b * gh + y / p) * gw + x / p;
  rows[row * p * p + (y % p) * p + (x % p)] = img[i];
}

// out[b][t] = (t < prefix ? cls (+ pos[0]) : patch[b][t - prefix] + pos[no_embed_class ? t - prefix : t]), rounded once
__global__ __launch_bounds__(256) void vit_embed_fwd_kernel(const bf16* __restrict__ patch, const float* __restrict__ pos,
                                                            const float* __restrict__ cls, int B, int P, int D, int prefix,
                                                            int no_embed_class, bf16* __restrict__ out) {
  const int T = P + prefix, dg = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)B * T * dg) return;
  const int d0 = (int)(i % dg) * 8;
  const int64_t row = i / dg;
  const int t = (int)(row % T), b = (int)(row / T);
  float v[8];
  if (t < prefix) {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = cls[d0 + j] + (no_embed_class ? 0.f : pos[d0 + j]);
  } else {
    const bf16x8 x = ldg16(patch + ((int64_t)b * P + (t - prefix)) * D + d0);
    const float* pr = pos + (size_t)(no_embed_class ? t - prefix : t) * D + d0;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = bf2f(x[j]) + pr[j];
  }
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = f2bf(v[j]);
  stg16(out + row * D + d0, r);
}

// d(pos)[j][d] = sum_b dout[b][j + off][d] for j < L; d(cls)[d] = sum_b dout[b][0][d] (row L of the launch); image order
__global__ __launch_bounds__(256) void vit_embed_bwd_kernel(const bf16* __restrict__ dout, int B, int T, int D, int L, int off,
                                                            float* __restrict__ dpos, int pos_acc, float* __restrict__ dcls,
                                                            int cls_acc) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)(L + 1) * D) return;
  const int d = (int)(i % D), j = (int)(i / D);
  float* dst;
  int acc, row;
  if (j < L) {
    if (!dpos) return;
    dst = dpos + (size_t)j * D + d;
    acc = pos_acc;
    row = j + off;
  } else {
    if (!dcls) return;
    dst = dcls + d;
    acc = cls_acc;
    row = 0;
  }
  float s = 0.f;
  for (int b = 0; b < B; ++b) s += bf2f(dout[((int64_t)b * T + row) * D + d]);
  *dst = acc ? *dst + s : s;
}

// rows [first, first + count) of every image's T rows: forward gather (dir 0) or its transpose (dir 1: dsrc (+)= scatter, the
// other rows 0 / unchanged)
__global__ __launch_bounds__(256) void rows_select_kernel(const bf16* __restrict__ src, int B, int T, int first, int count, int D,
                                                          bf16* __restrict__ dst, int dir, int accumulate) {
  const int dg = D / 8;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (dir == 0) {
    if (i >= (int64_t)B * count * dg) return;
    const int d0 = (int)(i % dg) * 8;
    const int64_t r = i / dg;
    const int b = (int)(r / count), t = (int)(r % count) + first;
    stg16(dst + r * D + d0, ldg16(src + ((int64_t)b * T + t) * D + d0));
    return;
  }
  if (i >= (int64_t)B * T * dg) return;
  const int d0 = (int)(i % dg) * 8;
  const int64_t r = i / dg;
  const int b = (int)(r / T), t = (int)(r % T);
  bf16* o = dst + r * D + d0;
  if (t < first || t >= first + count) {
    if (!accumulate) stg16(o, zero8());
    return;
  }
  const bf16x8 gsel = ldg16(src + ((int64_t)b * count + (t - first)) * D + d0);
  if (!accumulate) {
    stg16(o, gsel);
    return;
  }
  const bf16x8 cur = ldg16(o);
  bf16x8 r8;
#pragma unroll
  for (int j = 0; j < 8; ++j) r8[j] = f2bf(bf2f(cur[j]) + bf2f(gsel[j]));
  stg16(o, r8);
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// the geometry every attention entry point serves; `who` opens each refusal
int check_geo(const char* who, int ldq, int batch, int n, int heads, int head_dim, int ldo) {
  TOK_CHECK_ARG(head_dim == HD, "%s: head_dim %d is not served (64 only)", who, head_dim);
  TOK_CHECK_ARG(batch > 0 && heads > 0 && n >= 1 && n <= TOK_GLOBAL_ATTN_MAX_TOKENS, "%s: %d tokens (1 ... %d served)", who, n,
                TOK_GLOBAL_ATTN_MAX_TOKENS);
  TOK_CHECK_ARG(ldq >= 3 * heads * HD && ldq % 8 == 0 && ldo >= heads * HD && ldo % 8 == 0,
                "%s: row pitches ldq %d / ldo %d (>= 3C / C, multiples of 8)", who, ldq, ldo);
  TOK_CHECK_ARG((size_t)batch * heads <= 65535u, "%s: batch * heads %d > 65535", who, batch * heads);
  return TOK_OK;
}

int check_bias(const char* who, const float* bias, int ldb, int n) {
  TOK_CHECK_ARG(bias && ldb >= n && ldb % 4 == 0 && ((uintptr_t)bias & 15) == 0,
                "%s: bias pointer / row pitch ldb %d (16-byte aligned, >= n, a multiple of 4)", who, ldb);
  return TOK_OK;
}

// TOK_CHECK_LAUNCH for the launch "<who><stage>"
int launched(const char* who, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TOK_OK;
  tok_set_error("%s%s: launch failed: %s", who, stage, hipGetErrorString(e));
  return TOK_ERR_LAUNCH;
}

// bias == nullptr: the un-biased kernel
int launch_fwd(const char* who, const void* qkv, int ldq, const float* bias, int ldb, int batch, int n, int heads, void* out,
               int ldo, float* lse, void* stream) {
  hipLaunchKernelGGL(bias ? gattn_fwd_kernel<true> : gattn_fwd_kernel<false>, dim3(tok_cdiv(n, TL), batch * heads), dim3(256), 0,
                     tok_stream(stream), (const bf16*)qkv, ldq, n, heads, (bf16*)out, ldo, lse, bias, ldb);
  return launched(who, "");
}

}  // namespace

extern "C" int tok_global_attn_fwd(const void* qkv, int ldq, int batch, int n, int heads, int head_dim, void* out, int ldo,
                                   float* lse, void* stream) {
  const char* who = "tok_global_attn_fwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && lse, "%s: null pointer", who);
  return launch_fwd(who, qkv, ldq, nullptr, 0, batch, n, heads, out, ldo, lse, stream);
}

extern "C" int tok_global_attn_bias_fwd(const void* qkv, int ldq, const float* bias, int ldb, int batch, int n, int heads,
                                        int head_dim, void* out, int ldo, float* lse, void* stream) {
  const char* who = "tok_global_attn_bias_fwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && lse, "%s: null pointer", who);
  if (int rc = check_bias(who, bias, ldb, n)) return rc;
  return launch_fwd(who, qkv, ldq, bias, ldb, batch, n, heads, out, ldo, lse, stream);
}

extern "C" size_t tok_global_attn_bwd_ws_bytes(int batch, int n, int heads) {
  if (batch <= 0 || n <= 0 || heads <= 0) return 0;
  return ((size_t)batch * heads * n * sizeof(float) + 255) / 256 * 256;
}

// images per d(bias) chunk: enough (tile, head, chunk) workgroups for eight per CU of the 256 where the batch allows it
// (heads x tiles^2 is 192 at base / 224), at most 64 chunks to fold
static int dbias_per_chunk(int batch, int n, int heads) {
  const long long tiles = (long long)tok_cdiv(n, TL) * tok_cdiv(n, TL) * heads;
  long long chunks = (2048 + tiles - 1) / tiles;
  if (chunks > 64) chunks = 64;
  if (chunks > batch) chunks = batch;
  return tok_cdiv(batch, chunks);
}

extern "C" int tok_global_attn_bias_bwd_chunks(int batch, int n, int heads) {
  if (batch <= 0 || n <= 0 || heads <= 0) return 0;
  return tok_cdiv(batch, dbias_per_chunk(batch, n, heads));
}

extern "C" size_t tok_global_attn_bias_bwd_ws_bytes(int batch, int n, int heads, int ldb) {
  if (batch <= 0 || n <= 0 || heads <= 0 || ldb < n) return 0;
  return tok_global_attn_bwd_ws_bytes(batch, n, heads) +
         (size_t)tok_global_attn_bias_bwd_chunks(batch, n, heads) * heads * n * ldb * sizeof(float);
}

// delta, dK / dV, dQ, then with dbias the chunk partials and their fold.  bias == nullptr: the un-biased kernels (dbias is null
// then).  The workspace is [delta | partials].
static int launch_bwd(const char* who, const void* qkv, int ldq, const void* out, const void* dout, int ldo, const float* lse,
                      const float* bias, int ldb, int batch, int n, int heads, void* dqkv, int ldd, float* dbias, int accumulate,
                      void* ws, size_t ws_bytes, void* stream) {
  // without dbias only delta lives in the workspace: a frozen table pays for no chunk partials
  const size_t ws_need = dbias ? tok_global_attn_bias_bwd_ws_bytes(batch, n, heads, ldb) : tok_global_attn_bwd_ws_bytes(batch, n, heads);
  if (ws_bytes < ws_need) {
    tok_set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, ws_need);
    return TOK_ERR_WORKSPACE;
  }
  hipStream_t st = tok_stream(stream);
  const float* delta = (const float*)ws;
  const dim3 tiles(tok_cdiv(n, TL), batch * heads);
  hipLaunchKernelGGL(gattn_delta_kernel, dim3(blocks_of((int64_t)batch * n * heads)), dim3(256), 0, st, (const bf16*)out,
                     (const bf16*)dout, ldo, batch, n, heads, (float*)ws);
  if (int rc = launched(who, "(delta)")) return rc;
  hipLaunchKernelGGL(bias ? gattn_dkv_kernel<true> : gattn_dkv_kernel<false>, tiles, dim3(256), 0, st, (const bf16*)qkv, ldq,
                     (const bf16*)dout, ldo, lse, delta, n, heads, (bf16*)dqkv, ldd, bias, ldb);
  if (int rc = launched(who, "(dkv)")) return rc;
  hipLaunchKernelGGL(bias ? gattn_dq_kernel<true> : gattn_dq_kernel<false>, tiles, dim3(256), 0, st, (const bf16*)qkv, ldq,
                     (const bf16*)dout, ldo, lse, delta, n, heads, (bf16*)dqkv, ldd, bias, ldb);
  if (int rc = launched(who, "(dq)")) return rc;
  if (!dbias) return TOK_OK;
  float* part = (float*)((char*)ws + tok_global_attn_bwd_ws_bytes(batch, n, heads));
  const int per = dbias_per_chunk(batch, n, heads), chunks = tok_cdiv(batch, per), nt = tok_cdiv(n, TL);
  hipLaunchKernelGGL(gattn_dbias_kernel, dim3(nt * nt, heads, chunks), dim3(256), 0, st, (const bf16*)qkv, ldq, (const bf16*)dout,
                     ldo, lse, delta, bias, ldb, batch, n, heads, per, part);
  if (int rc = launched(who, "(dbias)")) return rc;
  hipLaunchKernelGGL(gattn_dbias_fold_kernel, dim3(blocks_of((int64_t)heads * n * n)), dim3(256), 0, st, (const float*)part,
                     chunks, heads, n, ldb, dbias, accumulate ? 1 : 0);
  return launched(who, "(fold)");
}

extern "C" int tok_global_attn_bwd(const void* qkv, int ldq, const void* out, const void* dout, int ldo, const float* lse,
                                   int batch, int n, int heads, int head_dim, void* dqkv, int ldd, void* ws, size_t ws_bytes,
                                   void* stream) {
  const char* who = "tok_global_attn_bwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && dout && lse && dqkv && ws, "%s: null pointer", who);
  TOK_CHECK_ARG(ldd >= 3 * heads * HD && ldd % 8 == 0, "%s: ldd %d", who, ldd);
  return launch_bwd(who, qkv, ldq, out, dout, ldo, lse, nullptr, 0, batch, n, heads, dqkv, ldd, nullptr, 0, ws, ws_bytes, stream);
}

extern "C" int tok_global_attn_bias_bwd(const void* qkv, int ldq, const void* out, const void* dout, int ldo, const float* lse,
                                        const float* bias, int ldb, int batch, int n, int heads, int head_dim, void* dqkv,
                                        int ldd, float* dbias, int dbias_accumulate, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tok_global_attn_bias_bwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && dout && lse && dqkv && ws, "%s: null pointer", who);
  if (int rc = check_bias(who, bias, ldb, n)) return rc;
  TOK_CHECK_ARG(ldd >= 3 * heads * HD && ldd % 8 == 0, "%s: ldd %d", who, ldd);
  return launch_bwd(who, qkv, ldq, out, dout, ldo, lse, bias, ldb, batch, n, heads, dqkv, ldd, dbias, dbias_accumulate, ws, ws_bytes,
                    stream);
}

extern "C" int tok_patch_gather(const void* img, int n, int h, int w, int p, void* rows, void* stream) {
  TOK_CHECK_ARG(img && rows && n > 0 && p > 0 && h >= p && w >= p && h % p == 0 && w % p == 0,
                "tok_patch_gather: %dx%d image, patch %d (sides must be multiples of the patch)", h, w, p);
  const int64_t px = (int64_t)n * h * w;
  hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks_of(px)), dim3(256), 0, tok_stream(stream), (const uint2*)img, n, h, w, p,
                     (uint2*)rows);
  TOK_CHECK_LAUNCH("tok_patch_gather");
  return TOK_OK;
}

extern "C" int tok_vit_embed_fwd(const void* patch, const float* pos, const float* cls, int batch, int patches, int d,
                                 int no_embed_class, void* out, void* stream) {
  TOK_CHECK_ARG(patch && pos && out && batch > 0 && patches > 0 && d > 0 && d % 8 == 0, "tok_vit_embed_fwd: bad args");
  const int prefix = cls ? 1 : 0;
  hipLaunchKernelGGL(vit_embed_fwd_kernel, dim3(blocks_of((int64_t)batch * (patches + prefix) * (d / 8))), dim3(256), 0,
                     tok_stream(stream), (const bf16*)patch, pos, cls, batch, patches, d, prefix, no_embed_class ? 1 : 0,
                     (bf16*)out);
  TOK_CHECK_LAUNCH("tok_vit_embed_fwd");
  return TOK_OK;
}

extern "C" int tok_vit_embed_bwd(const void* dout, int batch, int patches, int d, int has_cls, int no_embed_class, float* dpos,
                                 int pos_acc, float* dcls, int cls_acc, void* stream) {
  TOK_CHECK_ARG(dout && batch > 0 && patches > 0 && d > 0 && d % 8 == 0 && (!dcls || has_cls), "tok_vit_embed_bwd: bad args");
  if (!dpos && !dcls) return TOK_OK;
  const int prefix = has_cls ? 1 : 0, T = patches + prefix;
  const int L = no_embed_class ? patches : T, off = no_embed_class ? prefix : 0;
  hipLaunchKernelGGL(vit_embed_bwd_kernel, dim3(blocks_of((int64_t)(L + 1) * d)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)dout, batch, T, d, L, off, dpos, pos_acc, dcls, cls_acc);
  TOK_CHECK_LAUNCH("tok_vit_embed_bwd");
  return TOK_OK;
}

extern "C" int tok_rows_select(const void* src, int batch, int t, int first, int count, int d, void* dst, int dir,
                               int accumulate, void* stream) {
  TOK_CHECK_ARG(src && dst && batch > 0 && t > 0 && first >= 0 && count > 0 && first + count <= t && d > 0 && d % 8 == 0 &&
                (dir == 0 || dir == 1), "tok_rows_select: bad args");
  const int64_t work = (int64_t)batch * (dir == 0 ? count : t) * (d / 8);
  hipLaunchKernelGGL(rows_select_kernel, dim3(blocks_of(work)), dim3(256), 0, tok_stream(stream), (const bf16*)src, batch, t,
                     first, count, d, (bf16*)dst, dir, accumulate ? 1 : 0);
  TOK_CHECK_LAUNCH("tok_rows_select");
  return TOK_OK;
}
