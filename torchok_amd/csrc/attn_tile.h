// Softmax attention on 64-token tiles, the part written once for the two families that use it: whole-image attention of ViT /
// BEiT (attn_global.hip, head_dim 64, dense rows) and the window attention of GCViT (gc_attn.hip, head_dim 32, window-relative
// rows, optionally a query shared by the windows of an image).
//
// Forward : one workgroup per (unit, 64-query tile), unit = (image or window, head), one wave per 16 queries.  K / V tiles of 64
//           keys are staged in LDS (V transposed), S = Q K^T and O += P V on mfma_f32_16x16x32_bf16, online fp32 softmax in exp2
//           units, key tail masked (attn_fwd).
// Backward: dK / dV per (unit, 64-key tile) (attn_dkv); the d(bias) chunk partials are folded in chunk order
//           (attn_dbias_fold_kernel).  delta, dQ and d(bias) are kernels of the two .hip files on the pieces below: delta and
//           the bias term of d(bias) differ in arithmetic, and GCViT's dQ / d(bias) in this text were measurably slower than
//           their own (profiles/attn_family_ab.txt).  Each recomputes P from Q, K, the bias and the LSE.  Every output element
//           is written by exactly one lane and every sum runs in a fixed order: no float atomics, bit-reproducible.
// Pieces  : the kernels are written on stage_tile (64 token rows -> LDS), load_rows16 (16 token rows as an A operand),
//           frag_x_tile (operand x row-major LDS tile), rows_x_tile_t (staged rows x transposed LDS tile), load_row_stats (LSE and
//           delta of a lane's four queries), prob and ds_tile (P and dS, shared by dq and dbias).  What these pieces multiply and
//           add is written as fmaf where it is fused and as mul_rn / sub_rn where it is not, so that hipcc's contraction cannot
//           differ between the callers; the three forms of the bias term are listed at prob.
//
// A kernel body takes its problem P by value; the .hip file wraps it in a __global__ function.  P states what differs:
//   P::HD                      head_dim, 64 or 32: the A operand is bf16x8[HD / 32], a product across the head has HD / 16
//                              accumulators, a row-major LDS tile has the pitch HD + 8, stage_tile moves HD / 32 pieces per thread
//   P::BIAS                    logits get + bias[h][query][key] (fp32, shared by every unit)
//   P::Reduce                  the 16-lane max / sum of the forward (Butterfly16 or DppRow16: the addition order differs)
//   P::unit(), P::tile()       which block index counts the units (u * heads + h) and which the 64-token tiles
//   n(), heads()               tokens per unit, heads
//   q(u, h), k(u, h), v(u, h)  the rows of an operand: at(t) is the HD contiguous bf16 of token t, row(t) its row in the matrix
//   tokens(p, ld, u, h)        the same for a [tokens][heads * HD] matrix in the order of the output (dO)
//   token(u, t)                row of token t of unit u in that order
//   kcol(h)                    column of k of head h in qkv and d(qkv); v is heads * HD further
//   bias_row(h, q)             row q of head h's bias
#pragma once
#include "tok_common.h"

namespace {

constexpr int TL = 64;         // tokens per tile (queries of a workgroup, keys per staged tile)
constexpr int PT = 72;         // LDS row pitch of a [.][64 tokens] tile in bf16 (144 B: 16-B aligned rows)
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

template <int HD>
struct HeadDim {
  static_assert(HD == 64 || HD == 32, "head_dim 64 and 32 are served");
  static constexpr int ND = HD / 16;   // accumulators of a product across the head
  static constexpr int PR = HD + 8;    // LDS row pitch of a row-major [token][HD] tile in bf16 (16-B aligned rows)
  static constexpr float SCALE = HD == 64 ? 0.125f : 0.17677669529663687f;   // HD^-0.5
};

// base + (b*N + t) * ld + col: the tokens of image b, contiguous in the matrix (ViT, BEiT).  `base` is the address of token 0.
struct DenseRows {
  const bf16* base;
  int ld;
  int64_t first;      // b * N
  __device__ __forceinline__ int64_t row(int t) const { return first + t; }
  __device__ __forceinline__ const bf16* at(int t) const { return base + (size_t)t * ld; }
};
__device__ __forceinline__ DenseRows dense_rows(const bf16* p, int ld, int col, int64_t first) {
  return DenseRows{p + first * ld + col, ld, first};
}

__device__ __forceinline__ bf16x8 lds8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// tokens [r0, r0 + 64) of `src` -> LDS row-major [token][PR] and/or transposed [d][PT]; tokens past n are zero.  256 threads, 16
// bytes a piece: two trips at head_dim 64, one at 32.
template <int HD, class Rows>
__device__ __forceinline__ void stage_tile(const Rows& src, int r0, int n, bf16* rm, bf16* tr) {
  constexpr int PR = HeadDim<HD>::PR, SH = HD == 64 ? 3 : 2, PIECES = TL * (HD / 8);
  auto piece = [&](int c) {
    const int row = c >> SH, d0 = (c & (HD / 8 - 1)) * 8, t = r0 + row;
    const bf16x8 v = t < n ? ldg16(src.at(t) + d0) : zero8();
    if (rm) *reinterpret_cast<bf16x8*>(rm + row * PR + d0) = v;
    if (tr) {
#pragma unroll
      for (int j = 0; j < 8; ++j) tr[(d0 + j) * PT + row] = v[j];
    }
  };
  // each family keeps the form it had: hipcc does not fold the loop's bound check away for one trip
  if constexpr (PIECES == 256) {
    piece(threadIdx.x);
  } else {
    for (int c = threadIdx.x; c < PIECES; c += 256) piece(c);
  }
}

// The 16-lane reductions of the forward.  The two families have always used different ones and the addition order differs
// (tok_common.h at row16_sum), so each keeps its own.
struct Butterfly16 {
  static __device__ __forceinline__ float max(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
  }
  static __device__ __forceinline__ float sum(float v) {
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) v += __shfl_xor(v, o, 64);
    return v;
  }
};
struct DppRow16 {
  static __device__ __forceinline__ float max(float v) { return row16_max(v); }
  static __device__ __forceinline__ float sum(float v) { return row16_sum(v); }
};

// ---- the pieces the MFMA kernels are written on --------------------------------------------------------------------------------
// A lane is (l15, g) = (lane & 15, lane >> 4) of its wave.  Element (j, r) of a product, j the f32x4 and r its component, is row
// 4 g + r of the A operand's 16 rows against row 16 j + l15 of the 64-row LDS tile.  Every accumulator takes t = 0, then t = 1
// (the two halves of a 64-wide reduction): the bits of every output depend on that order.

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

// tokens [r0, r0 + 16) as an A operand (the lane: token r0 + l15, dims 32 t + 8 g ... + 7); tokens past n are zero
template <int HD, class Rows>
__device__ __forceinline__ void load_rows16(const Rows& src, int r0, int n, int l15, int g, bf16x8 (&f)[HD / 32]) {
  const int row = r0 + l15;
#pragma unroll
  for (int t = 0; t < HD / 32; ++t) f[t] = row < n ? ldg16(src.at(row) + 32 * t + 8 * g) : zero8();
}

// acc = a x tile^T, tile a row-major LDS tile [64][PR]
template <int HD>
__device__ __forceinline__ void frag_x_tile(const bf16x8 (&a)[HD / 32], const bf16* tile, int l15, int g, f32x4 (&acc)[4]) {
  constexpr int PR = HeadDim<HD>::PR;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < HD / 32; ++t)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[t], lds8(tile + (j * 16 + l15) * PR + 32 * t + 8 * g), acc[j], 0, 0, 0);
  }
}

// acc += rows x tile_t^T: the [16][PT] rows a wave staged in LDS (P, dS or their transposes) times a transposed LDS tile [HD][PT]
template <int HD>
__device__ __forceinline__ void rows_x_tile_t(const bf16* rows, const bf16* tile_t, int l15, int g, f32x4 (&acc)[HD / 16]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bf16x8 a = lds8(rows + l15 * PT + 32 * t + 8 * g);
#pragma unroll
    for (int j = 0; j < HD / 16; ++j)
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

// P = exp2(s * HD^-0.5 * log2e - lb) in one fused multiply-subtract; lb is the query's log-sum-exp less the bias term, both in
// log2 units.
// The bias term enters in three forms, each pinned to what its kernel has always computed, so the caller forms it:
//   forward                          bl = bias * log2e rounded, then fma(s, sc, bl)
//   dK/dV, dQ, delta and d(bias) of the windowed family
//                                    lb = fma(-bias, log2e, lse): one rounding (lse_less_bias, or written out)
//   d(bias) of the dense family      lb = lse - bl with bl = bias * log2e rounded: two roundings (bl is loaded once per tile,
//                                    outside the image loop: gattn_dbias_kernel)
// so the P of the dense backward is not the same float in d(bias) as in dQ.  Making them one form changes output bits.
template <int HD>
__device__ __forceinline__ float prob(float s, float lb) { return exp2f(fmaf(s, HeadDim<HD>::SCALE * LOG2E, -lb)); }

// lb of query q against `key` where both are tokens (`live`: key < n), the bare log-sum-exp elsewhere and without a bias
template <class P>
__device__ __forceinline__ float lse_less_bias(const P& p, int h, int q, int key, bool live, float lse2) {
  if constexpr (P::BIAS) return (live && q < p.n()) ? fmaf(-p.bias_row(h, q)[key], LOG2E, lse2) : lse2;
  return lse2;
}

// dS = P (dP - delta) of the wave's 16 queries against the 64 keys from k0: sink(kj, r, p, d) takes the two factors of element
// (kj, r), dS = p * d, with p = 0 for a key past n.  lb(kj, r, live) is the caller's log-sum-exp less bias term (see prob).
// The dq kernels round the product to bf16, the dbias kernels fuse it into their sum over the units.
template <int HD, class Lb, class Sink>
__device__ __forceinline__ void ds_tile(const f32x4 (&s)[4], const f32x4 (&dp)[4], const float (&dr)[4], int k0, int n, int l15,
                                        Lb&& lb, Sink&& sink) {
#pragma unroll
  for (int kj = 0; kj < 4; ++kj) {
    const bool live = k0 + kj * 16 + l15 < n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = prob<HD>(s[kj][r], lb(kj, r, live));
      sink(kj, r, live ? p : 0.f, dp[kj][r] - dr[r]);
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
// out rows bf16 [tokens][ldo] at column h * HD; lse fp32 [units][N] (natural log).  Columns >= N of a bias row and rows of queries
// >= N are never loaded.
template <class P>
__device__ __forceinline__ void attn_fwd(const P p, bf16* __restrict__ out, int ldo, float* __restrict__ lse) {
  constexpr int HD = P::HD, PR = HeadDim<HD>::PR, ND = HeadDim<HD>::ND;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];        // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vt[HD * PT];        // V^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 ps[4][16 * PT];     // per wave: P [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const unsigned unit = P::unit();                    // unsigned, as the block index is: no sign fix-up in the division
  const int u = unit / p.heads(), h = unit % p.heads(), N = p.n();
  const int q0 = P::tile() * TL + wv * 16;
  const auto krows = p.k(u, h), vrows = p.v(u, h);
  bf16x8 qf[HD / 32];
  load_rows16<HD>(p.q(u, h), q0, N, l15, g, qf);
  float m[4], l[4];
  f32x4 o[ND];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
#pragma unroll
  for (int dj = 0; dj < ND; ++dj) o[dj] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float sc = HeadDim<HD>::SCALE * LOG2E;
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();                                    // the previous tile has been consumed by every wave
    stage_tile<HD>(krows, k0, N, ks, nullptr);
    stage_tile<HD>(vrows, k0, N, nullptr, vt);
    __syncthreads();
    f32x4 s[4];
    frag_x_tile<HD>(qf, ks, l15, g, s);
    // element (kj, r): query 4g + r of the wave's 16, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[4], mx = -INFINITY;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        if constexpr (P::BIAS) {
          const int q = q0 + 4 * g + r;
          const float bl = (key < N && q < N) ? mul_rn(p.bias_row(h, q)[key], LOG2E) : 0.f;
          v[kj] = (key < N) ? fmaf(s[kj][r], sc, bl) : -INFINITY;
        } else {
          v[kj] = (key < N) ? s[kj][r] * sc : -INFINITY;
        }
        mx = fmaxf(mx, v[kj]);
      }
      const float mn = fmaxf(m[r], P::Reduce::max(mx));  // finite: key k0 < N is in every tile
      const float alpha = exp2f(m[r] - mn);
      float ls = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float pr = exp2f(v[kj] - mn);
        ls += pr;
        ps[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(pr);
      }
      l[r] = l[r] * alpha + P::Reduce::sum(ls);
      m[r] = mn;
#pragma unroll
      for (int dj = 0; dj < ND; ++dj) o[dj][r] *= alpha;
    }
    __syncthreads();
    rows_x_tile_t<HD>(ps[wv], vt, l15, g, o);
  }
  // o[dj][r]: query q0 + 4g + r, dim 16 dj + l15
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    const float inv = 1.f / l[r];
    bf16* orow = out + p.token(u, q) * ldo + h * HD;
#pragma unroll
    for (int dj = 0; dj < ND; ++dj) orow[dj * 16 + l15] = f2bf(o[dj][r] * inv);
    if (l15 == 0) lse[(size_t)unit * N + q] = (m[r] + log2f(l[r])) * LN2;
  }
}

// ---- dK, dV of 64 keys: a wave owns 16 keys and walks every query tile ---------------------------------------------------------
template <class P>
__device__ __forceinline__ void attn_dkv(const P p, const bf16* __restrict__ dout, int ldo, const float* __restrict__ lse,
                                         const float* __restrict__ delta, bf16* __restrict__ dqkv, int ldd) {
  constexpr int HD = P::HD, PR = HeadDim<HD>::PR, ND = HeadDim<HD>::ND;
  __shared__ __attribute__((aligned(16))) bf16 qs[TL * PR];       // Q [query][d]
  __shared__ __attribute__((aligned(16))) bf16 qt[HD * PT];       // Q^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 dos[TL * PR];      // dO [query][d]
  __shared__ __attribute__((aligned(16))) bf16 dot[HD * PT];      // dO^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: P^T, then dS^T [key][query]
  __shared__ float lsl[TL], dl[TL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const unsigned unit = P::unit();
  const int u = unit / p.heads(), h = unit % p.heads(), N = p.n(), C = p.heads() * HD;
  const int k0 = P::tile() * TL + wv * 16;
  const auto qrows = p.q(u, h);
  const auto drows = p.tokens(dout, ldo, u, h);
  const float* lrow = lse + (size_t)unit * N;
  const float* drow = delta + (size_t)unit * N;
  bf16x8 kf[HD / 32], vf[HD / 32];
  load_rows16<HD>(p.k(u, h), k0, N, l15, g, kf);
  load_rows16<HD>(p.v(u, h), k0, N, l15, g, vf);
  f32x4 dk[ND], dv[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) dk[j] = dv[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TL) {
    __syncthreads();
    stage_tile<HD>(qrows, q0, N, qs, qt);
    stage_tile<HD>(drows, q0, N, dos, dot);
    if (threadIdx.x < TL) {
      const int q = q0 + threadIdx.x;
      lsl[threadIdx.x] = q < N ? mul_rn(lrow[q], LOG2E) : INFINITY;      // queries past N: P = 0
      dl[threadIdx.x] = q < N ? drow[q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
    frag_x_tile<HD>(kf, qs, l15, g, st);
    frag_x_tile<HD>(vf, dos, l15, g, dpt);
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
      if constexpr (P::BIAS) {
        // keys k0 + 4g ... + 3 of query row q0 + ql: one aligned 16-byte load (ldb % 4 == 0 keeps it inside the row)
        const int q = q0 + ql, kb = k0 + 4 * g;
        if (q < N && kb < N) {
          const float4 b4 = *reinterpret_cast<const float4*>(p.bias_row(h, q) + kb);
          const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) lqb[r] = kb + r < N ? fmaf(-bv[r], LOG2E, lq) : lq;
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = prob<HD>(st[qj][r], lqb[r]);
        ws[wv][(4 * g + r) * PT + ql] = f2bf(pr);
        dsv[qj][r] = pr * (dpt[qj][r] - dq);
      }
    }
    __syncthreads();
    rows_x_tile_t<HD>(ws[wv], dot, l15, g, dv);
    __syncthreads();
#pragma unroll
    for (int qj = 0; qj < 4; ++qj)
#pragma unroll
      for (int r = 0; r < 4; ++r) ws[wv][(4 * g + r) * PT + qj * 16 + l15] = f2bf(dsv[qj][r]);
    __syncthreads();
    rows_x_tile_t<HD>(ws[wv], qt, l15, g, dk);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int k = k0 + 4 * g + r;
    if (k >= N) continue;
    bf16* row = dqkv + p.token(u, k) * ldd + p.kcol(h);
#pragma unroll
    for (int dj = 0; dj < ND; ++dj) {
      row[dj * 16 + l15] = f2bf(dk[dj][r] * HeadDim<HD>::SCALE);
      row[C + dj * 16 + l15] = f2bf(dv[dj][r]);
    }
  }
}

// ---- d(bias) fold ---------------------------------------------------------------------------------------------------------------
// dbias[h][i][j] (=|+=) sum_chunk part[chunk][h][i][j], chunk order; part rows have the pitch np, dbias rows ldb; columns >= N of
// a row are not touched
__global__ __launch_bounds__(256) void attn_dbias_fold_kernel(const float* __restrict__ part, int chunks, int H, int N, int np,
                                                              float* __restrict__ dbias, int ldb, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)H * N * N) return;
  const int j = (int)(i % N);
  const int64_t row = i / N;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[((size_t)c * H * N + row) * np + j];
  float* o = dbias + row * ldb + j;
  *o = accumulate ? *o + s : s;
}

// images or windows per d(bias) chunk: enough (tile, head, chunk) workgroups for eight per CU of the 256 where the units allow
// it (heads x tiles^2 is 192 at ViT-base / 224), at most max_chunks partial tables to fold — the partials do not grow with the
// number of units
inline int dbias_per_chunk(long long units, int n, int heads, int max_chunks) {
  const long long tiles = (long long)tok_cdiv(n, TL) * tok_cdiv(n, TL) * heads;
  long long chunks = (2048 + tiles - 1) / tiles;
  if (chunks > max_chunks) chunks = max_chunks;
  if (chunks > units) chunks = units;
  return tok_cdiv(units, chunks);
}

}  // namespace
