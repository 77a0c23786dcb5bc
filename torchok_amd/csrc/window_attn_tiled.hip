// SwinV2 window attention on 64-token tiles, for the windows the scalar pair of window_attn.hip cannot hold in LDS (18 x 18 tokens
// and up: the 24 x 24 windows of the 384-px variants, N = 576).  The arithmetic is that of the MFMA pair for windows of up to 64
// tokens but for one rounding point, so the contract paragraph of include/tok.h holds with room to spare:
//   qn = q / max(|q|, 1e-12) as a bf16 pair (bf16(qn) and the bf16 of what that rounding dropped), kn likewise, the norm in fp32
//   from the bf16 inputs.  The cosine qn . kn takes both parts (three MFMAs per block, cos_tile of attn_tile.h); every other
//   product takes bf16(qn) / bf16(kn) alone.  Why: with one bf16 per operand the logit is off by scale 2^-8 sum |qn||kn|, which at
//   the clamped scale of 100 is e^0.4 in P.  The contract's forward bounds carry that term, its 3e-2 row gates on dq / dk / dv do
//   not: an exact kernel with single-bf16 operands (emulate_device of tests/window_attn_ref.py) sits at 2.2e-2 / 7.6e-2 / 9.9e-2
//   on the clamped head of tests/test_window_attn_tiled_contract_gpu.py at 324 keys, and at 2e-3 ... 4e-3 with exact cosines.
//   logit = (qn . kn) exp(min(logit_scale[h], ln 100)) + bias[h][i][j] + mask[win][i][j];  softmax in fp32;  P to bf16 for P V;
//   lse fp32 [B*nW*heads][N], natural log;  token_row (window_attn.h) is roll(-shift) + window_partition, nothing is permuted.
// The kernels are written on the pieces of attn_tile.h at head_dim 32 (stage_tile, load_rows16, frag_x_tile, rows_x_tile_t) and
// its unit-length forms (stage_tile_unit, load_rows16_unit: q and k are normalised while they are loaded, by two shuffles among
// the four lanes that hold a row; no prologue pass over HBM and no workspace in the forward).
//
// Forward : one workgroup per (image, window, head, 64-query tile), one wave per 16 queries; kn and V tiles of 64 keys through LDS
//           (V transposed), S and P V on mfma_f32_16x16x32_bf16, online softmax in exp2 units, key tail masked.
// Backward: five launches, each recomputing P from qn, kn, bias, mask and the forward's lse:
//   delta     delta_i = sum_j P_ij dP_ij per (unit, query tile) into the workspace, from the same P and dP that dS is formed from,
//             as the N <= 64 path and gc_attn.hip's gc_delta_kernel do.  NOT rowsum(dO o O) of the stored bf16 O, so the backward
//             does not take `out`: that sum is off by 2^-9 |dO| |O| per term while dP - delta cancels, which is what
//             gc_delta_kernel records as having dominated dS behind a LayerNorm.  (The CPU emulation of tests/window_attn_ref.py
//             does not tell the two forms apart at the shapes of tests/test_window_attn_tiled_contract_gpu.py; the choice
//             rests on that earlier finding, not on a measurement of this family.)
//   dkv       per (unit, 64-key tile): a wave owns 16 keys and walks the query tiles; dV = P^T dO, dkn = (dS scale)^T qn, then
//             F.normalize's backward of the row and 16-byte stores.
//   dq        per (unit, 64-query tile): dqn = (dS scale) kn, the same epilogue; and the tile's partial of sum dS_ij cos_ij,
//             times the scale, zero for a clamped head.
//   fold      the d(logit_scale) partials in tile order, then image order, into dscale_part[row][head].
//   dlogits   per (scratch row, head, 64 x 64 tile): walks the images of the row in order, keeps the fp32 sum of dS in registers
//             (16 per lane) and stores it once into ds_scratch[row][head][i][j].
// Scratch row r of window win holds the images [r ipr, min(B, (r + 1) ipr)), ipr = ceil(B / SCRATCH_ROWS).
// Every output element is written by exactly one lane and every sum runs in a fixed order: no atomics, reruns are bit-identical.
// Nothing here assumes N >= 311: which windows come here is attn_tiled (window_attn.h) alone.
#include "attn_tile.h"
#include "window_attn.h"

namespace {

constexpr int HD = WIN_HEAD_DIM, PR = HeadDim<HD>::PR;
constexpr float LN100 = 4.605170185988092f;
// Image groups per window in ds_scratch.  One row is heads * N * N floats per window: 85 MB per group at stage 1 of
// swinv2_base_window12to24_192to384 (96 x 96, 4 heads, 16 windows), so the batch * nW rows of the scalar pair are out of reach.
// Two rows keep the d(logits) grid at 2 * nW * heads * tiles^2 workgroups (2592 at the 24 x 24 / 16-head stage, ten per CU) and
// the fold that follows at two rows per column.  Timings: profiles/swin_tiled_times.txt.
constexpr int SCRATCH_ROWS = 2;
constexpr int EP = 36;         // fp32 row pitch of the epilogue tile [16 tokens][32 dims]

// the rows of one operand of one (image, window, head): token t -> 32 contiguous bf16
struct WinRows {
  const bf16* base;   // column of the head already added
  int ld, b, win;
  AttnArgs a;         // by value (see Rows of gc_attn.hip)
  __device__ __forceinline__ int64_t row(int t) const { return token_row(a, b, win, t); }
  __device__ __forceinline__ const bf16* at(int t) const { return base + row(t) * ld; }
};

struct Unit { int b, win, h; };

// the operands every kernel of the family reads
struct Tiled {
  AttnArgs a;
  const bf16* qkv;
  const float *logit_scale, *bias, *mask;
  __device__ __forceinline__ Unit unit(unsigned u) const {
    const unsigned bw = u / a.heads;
    return Unit{(int)(bw / a.nW), (int)(bw % a.nW), (int)(u % a.heads)};
  }
  __device__ __forceinline__ size_t index(const Unit& u) const { return ((size_t)u.b * a.nW + u.win) * a.heads + u.h; }
  __device__ __forceinline__ WinRows q(const Unit& u) const { return WinRows{qkv + u.h * HD, a.ld, u.b, u.win, a}; }
  __device__ __forceinline__ WinRows k(const Unit& u) const { return WinRows{qkv + a.C + u.h * HD, a.ld, u.b, u.win, a}; }
  __device__ __forceinline__ WinRows v(const Unit& u) const { return WinRows{qkv + 2 * a.C + u.h * HD, a.ld, u.b, u.win, a}; }
  __device__ __forceinline__ WinRows tokens(const bf16* p, int ld, const Unit& u) const {
    return WinRows{p + u.h * HD, ld, u.b, u.win, a};
  }
  __device__ __forceinline__ float raw_scale(int h) const { return logit_scale[h]; }
  __device__ __forceinline__ float scale(int h) const { return expf(fminf(logit_scale[h], LN100)); }   // clamp(max = ln 100).exp()
};

// position bias + shift mask of (query, key) of one (head, window), in log2 units
struct AddTerm {
  const float *bh, *mw;
  int N;
  __device__ __forceinline__ AddTerm(const Tiled& p, const Unit& u)
      : bh(p.bias + (size_t)u.h * p.a.N * p.a.N), mw(p.mask ? p.mask + (size_t)u.win * p.a.N * p.a.N : nullptr), N(p.a.N) {}
  __device__ __forceinline__ float operator()(int q, int key) const {
    const size_t i = (size_t)q * N + key;
    return mul_rn(bh[i] + (mw ? mw[i] : 0.f), LOG2E);
  }
};

// P and d(logits) of the wave's 16 queries against 64 keys: element (kj, r) is query q0 + 4g + r, key k0 + 16 kj + l15, with
// S = qn kn^T in s and dP = dO V^T in dp.  sink(kj, r, p, d) takes P (0 past N) and dP - delta: dS = p * d.  lr: the log-sum-exp
// of the lane's four queries in log2 units, dr their delta.
template <class Sink>
__device__ __forceinline__ void p_ds_tile(const AddTerm& add, const f32x4 (&s)[4], const f32x4 (&dp)[4], const float (&lr)[4],
                                          const float (&dr)[4], int q0, int k0, int N, int l15, int g, float sc2, Sink&& sink) {
#pragma unroll
  for (int kj = 0; kj < 4; ++kj) {
    const int key = k0 + kj * 16 + l15;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r;
      const bool live = key < N && q < N;
      const float p = live ? exp2f(fmaf(s[kj][r], sc2, add(q, key)) - lr[r]) : 0.f;
      sink(kj, r, p, dp[kj][r] - dr[r]);
    }
  }
}

// log-sum-exp in log2 units and delta of queries q ... q + 3 (0 past N, where p_ds_tile gives P = 0 by itself)
__device__ __forceinline__ void row_stats(const float* __restrict__ lrow, const float* __restrict__ drow, int q, int N,
                                          float (&lr)[4], float (&dr)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = q + r < N ? mul_rn(lrow[q + r], LOG2E) : 0.f;
    dr[r] = (drow && q + r < N) ? drow[q + r] : 0.f;
  }
}

// F.normalize's backward of the wave's 16 token rows, d = (dn - n <n, dn>) * inv, from the accumulators of a product across the
// head (element (dj, r): token 4g + r, dim 16 dj + l15) through the wave's fp32 tile to the layout of load_rows16 (the lane: token
// l15, dims 8g ... + 7, whose unit row it still holds in n8), then one 16-byte store per lane.  `unit` false: the plain row (dV).
// Called by every wave of the workgroup at the same place (two barriers).
__device__ __forceinline__ void store_rows16(float* ep, const f32x4 (&acc)[2], bool unit, const bf16x8& n8, float inv, bf16* dst,
                                             bool live, int l15, int g) {
  __syncthreads();                                      // the tile's previous readers are done
#pragma unroll
  for (int dj = 0; dj < 2; ++dj)
#pragma unroll
    for (int r = 0; r < 4; ++r) ep[(4 * g + r) * EP + dj * 16 + l15] = acc[dj][r];
  __syncthreads();
  float x[8], dot = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    x[e] = ep[l15 * EP + 8 * g + e];
    dot = fmaf(bf2f(n8[e]), x[e], dot);
  }
  dot += __shfl_xor(dot, 16, 64);
  dot += __shfl_xor(dot, 32, 64);
  bf16x8 o8;
#pragma unroll
  for (int e = 0; e < 8; ++e) o8[e] = f2bf(unit ? (x[e] - bf2f(n8[e]) * dot) * inv : x[e]);
  if (live) stg16(dst, o8);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void wt_fwd_kernel(Tiled p, bf16* __restrict__ out, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];        // kn [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kl[TL * PR];        // its low part
  __shared__ __attribute__((aligned(16))) bf16 vt[HD * PT];        // V^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 ps[4][16 * PT];     // per wave: P [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const Unit u = p.unit(blockIdx.x);
  const int N = p.a.N, q0 = blockIdx.y * TL + wv * 16;
  const WinRows krows = p.k(u), vrows = p.v(u);
  const AddTerm add(p, u);
  bf16x8 qf[1], ql[1];
  load_rows16_unit(p.q(u), q0, N, l15, g, qf, ql);
  const float sc2 = p.scale(u.h) * LOG2E;               // logits in log2 units: exp(x) = exp2(x log2 e)
  float m[4], l[4];
  f32x4 o[2];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  o[0] = o[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();                                    // the previous tile has been consumed by every wave
    stage_tile_unit(krows, k0, N, ks, kl, nullptr);
    stage_tile<HD>(vrows, k0, N, nullptr, vt);
    __syncthreads();
    f32x4 s[4];
    cos_tile(qf, ql, ks, kl, l15, g, s);
    // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r;
      float v[4], mx = -INFINITY;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        const float al = (key < N && q < N) ? add(q, key) : 0.f;
        v[kj] = key < N ? fmaf(s[kj][r], sc2, al) : -INFINITY;
        mx = fmaxf(mx, v[kj]);
      }
      const float mn = fmaxf(m[r], row16_max(mx));      // finite: key k0 < N is in every tile and the mask is -100, not -inf
      const float alpha = exp2f(m[r] - mn);
      float ls = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float pr = exp2f(v[kj] - mn);
        ls += pr;
        ps[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(pr);
      }
      l[r] = l[r] * alpha + row16_sum(ls);
      m[r] = mn;
      o[0][r] *= alpha;
      o[1][r] *= alpha;
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
    bf16* orow = out + token_row(p.a, u.b, u.win, q) * p.a.C + u.h * HD;
    orow[l15] = f2bf(o[0][r] * inv);
    orow[16 + l15] = f2bf(o[1][r] * inv);
    if (l15 == 0) lse[(size_t)blockIdx.x * N + q] = (m[r] + log2f(l[r])) * LN2;
  }
}

// ---- delta[unit][q] = sum_j P[q][j] dP[q][j]: grid (units, query tiles), a wave owns 16 queries and walks the key tiles ----------
__global__ __launch_bounds__(256) void wt_delta_kernel(Tiled p, const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                       float* __restrict__ delta) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];        // kn [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kl[TL * PR];        // its low part
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];        // V [key][d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const Unit u = p.unit(blockIdx.x);
  const int N = p.a.N, q0 = blockIdx.y * TL + wv * 16;
  const WinRows krows = p.k(u), vrows = p.v(u);
  const AddTerm add(p, u);
  bf16x8 qf[1], ql[1], df[1];
  load_rows16_unit(p.q(u), q0, N, l15, g, qf, ql);
  load_rows16<HD>(p.tokens(dout, p.a.C, u), q0, N, l15, g, df);
  const float sc2 = p.scale(u.h) * LOG2E;
  float lr[4], zero[4], acc[4] = {0.f, 0.f, 0.f, 0.f};
  row_stats(lse + (size_t)blockIdx.x * N, nullptr, q0 + 4 * g, N, lr, zero);
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile_unit(krows, k0, N, ks, kl, nullptr);
    stage_tile<HD>(vrows, k0, N, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    cos_tile(qf, ql, ks, kl, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    float part[4] = {0.f, 0.f, 0.f, 0.f};
    p_ds_tile(add, s, dp, lr, zero, q0, k0, N, l15, g, sc2, [&](int, int r, float pr, float d) { part[r] = fmaf(pr, d, part[r]); });
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] += row16_sum(part[r]);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q < N && l15 == 0) delta[(size_t)blockIdx.x * N + q] = acc[r];
  }
}

// ---- dK, dV of 64 keys: grid (units, key tiles), a wave owns 16 keys and walks every query tile -------------------------------------
__global__ __launch_bounds__(256) void wt_dkv_kernel(Tiled p, const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                     const float* __restrict__ delta, bf16* __restrict__ dqkv) {
  __shared__ __attribute__((aligned(16))) bf16 qs[TL * PR];       // qn [query][d]
  __shared__ __attribute__((aligned(16))) bf16 qls[TL * PR];      // its low part
  __shared__ __attribute__((aligned(16))) bf16 qt[HD * PT];       // qn^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 dos[TL * PR];      // dO [query][d]
  __shared__ __attribute__((aligned(16))) bf16 dot[HD * PT];      // dO^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: P^T, then (dS scale)^T [key][query]
  __shared__ float ep[4][16 * EP];                                // per wave: the epilogue tile
  __shared__ float lsl[TL], dl[TL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const Unit u = p.unit(blockIdx.x);
  const int N = p.a.N, C = p.a.C, k0 = blockIdx.y * TL + wv * 16;
  const WinRows qrows = p.q(u), drows = p.tokens(dout, C, u);
  const AddTerm add(p, u);
  const float* lrow = lse + (size_t)blockIdx.x * N;
  const float* drow = delta + (size_t)blockIdx.x * N;
  bf16x8 kf[1], kfl[1], vf[1];
  const float kinv = load_rows16_unit(p.k(u), k0, N, l15, g, kf, kfl);
  load_rows16<HD>(p.v(u), k0, N, l15, g, vf);
  const float scale = p.scale(u.h), sc2 = scale * LOG2E;
  f32x4 dk[2], dv[2];
  dk[0] = dk[1] = dv[0] = dv[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TL) {
    __syncthreads();
    stage_tile_unit(qrows, q0, N, qs, qls, qt);
    stage_tile<HD>(drows, q0, N, dos, dot);
    if (threadIdx.x < TL) {
      const int q = q0 + threadIdx.x;
      lsl[threadIdx.x] = q < N ? mul_rn(lrow[q], LOG2E) : 0.f;
      dl[threadIdx.x] = q < N ? drow[q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
    cos_tile(kf, kfl, qs, qls, l15, g, st);
    frag_x_tile<HD>(vf, dos, l15, g, dpt);
    // S^T and dP^T leave the accumulator file in one go, as in attn_dkv of attn_tile.h (tools/isa_lint.py)
    asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(dpt[0]), "+v"(dpt[1]), "+v"(dpt[2]), "+v"(dpt[3]));
    // element (qj, r): key k0 + 4g + r, query q0 + 16 qj + l15
    float dsv[4][4];
#pragma unroll
    for (int qj = 0; qj < 4; ++qj) {
      const int ql = qj * 16 + l15, q = q0 + ql;
      const float lq = lsl[ql], dq = dl[ql];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = k0 + 4 * g + r;
        const float pr = (q < N && key < N) ? exp2f(fmaf(st[qj][r], sc2, add(q, key)) - lq) : 0.f;
        ws[wv][(4 * g + r) * PT + ql] = f2bf(pr);
        dsv[qj][r] = pr * (dpt[qj][r] - dq) * scale;     // d(qn kn^T) = d(logits) * scale
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
  const int key = k0 + l15;
  bf16* row = dqkv + token_row(p.a, u.b, u.win, key < N ? key : 0) * p.a.ld + C + u.h * HD + 8 * g;
  store_rows16(ep[wv], dk, true, kf[0], kinv, row, key < N, l15, g);
  store_rows16(ep[wv], dv, false, kf[0], 1.f, row + C, key < N, l15, g);
}

// ---- dQ of 64 queries and the tile's d(logit_scale) partial: grid (units, query tiles) -----------------------------------------------
__global__ __launch_bounds__(256) void wt_dq_kernel(Tiled p, const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                    const float* __restrict__ delta, bf16* __restrict__ dqkv,
                                                    float* __restrict__ dsc_tiles) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // kn [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kl[TL * PR];       // its low part
  __shared__ __attribute__((aligned(16))) bf16 kt[HD * PT];       // kn^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: dS scale [query][key]
  __shared__ float ep[4][16 * EP];
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const Unit u = p.unit(blockIdx.x);
  const int N = p.a.N, q0 = blockIdx.y * TL + wv * 16;
  const WinRows krows = p.k(u), vrows = p.v(u);
  const AddTerm add(p, u);
  bf16x8 qf[1], ql[1], df[1];
  const float qinv = load_rows16_unit(p.q(u), q0, N, l15, g, qf, ql);
  load_rows16<HD>(p.tokens(dout, p.a.C, u), q0, N, l15, g, df);
  const float raw = p.raw_scale(u.h), scale = p.scale(u.h), sc2 = scale * LOG2E;
  float lr[4], dr[4], dsc = 0.f;
  row_stats(lse + (size_t)blockIdx.x * N, delta + (size_t)blockIdx.x * N, q0 + 4 * g, N, lr, dr);
  f32x4 dq[2];
  dq[0] = dq[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile_unit(krows, k0, N, ks, kl, kt);
    stage_tile<HD>(vrows, k0, N, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    cos_tile(qf, ql, ks, kl, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    asm volatile("" : "+v"(s[0]), "+v"(s[1]), "+v"(s[2]), "+v"(s[3]), "+v"(dp[0]), "+v"(dp[1]), "+v"(dp[2]), "+v"(dp[3]));
    p_ds_tile(add, s, dp, lr, dr, q0, k0, N, l15, g, sc2, [&](int kj, int r, float pr, float d) {
      const float ds = pr * d;
      dsc = fmaf(ds, s[kj][r], dsc);                     // d(scale) = sum dS cos
      ws[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(ds * scale);
    });
    __syncthreads();
    rows_x_tile_t<HD>(ws[wv], kt, l15, g, dq);
  }
  const int q = q0 + l15;
  bf16* row = dqkv + token_row(p.a, u.b, u.win, q < N ? q : 0) * p.a.ld + u.h * HD + 8 * g;
  store_rows16(ep[wv], dq, true, qf[0], qinv, row, q < N, l15, g);
  // d(logit_scale) = d(scale) * scale, zero where the clamp is active: lanes by the butterfly, then the four waves in order
  dsc = wave_sum(dsc);
  if (lane == 0) wsum[wv] = dsc;
  __syncthreads();
  if (threadIdx.x == 0)
    dsc_tiles[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = raw < LN100 ? (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * scale : 0.f;
}

// dscale_part[row][head] = the tile partials of the row's images: tiles in order, then images in order
__global__ __launch_bounds__(256) void wt_dscale_fold_kernel(AttnArgs a, const float* __restrict__ dsc_tiles, int nt, int ipr,
                                                             int rows, float* __restrict__ dscale_part) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= rows * a.heads) return;
  const int h = i % a.heads, row = i / a.heads, win = row % a.nW, rg = row / a.nW;
  const int b_hi = min(a.B, (rg + 1) * ipr);
  float s = 0.f;
  for (int b = rg * ipr; b < b_hi; ++b) {
    const float* t = dsc_tiles + (((size_t)b * a.nW + win) * a.heads + h) * nt;
    float si = 0.f;
    for (int j = 0; j < nt; ++j) si += t[j];
    s += si;
  }
  dscale_part[i] = s;
}

// ---- d(logits) scratch: grid ((scratch row, head), 64 x 64 tiles); a wave owns 16 queries of the tile -------------------------------
__global__ __launch_bounds__(256) void wt_dlogits_kernel(Tiled p, const bf16* __restrict__ dout, const float* __restrict__ lse,
                                                         const float* __restrict__ delta, int ipr, float* __restrict__ ds_scratch) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // kn [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kl[TL * PR];       // its low part
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int N = p.a.N, nt = (N + TL - 1) / TL;
  const int h = blockIdx.x % p.a.heads, row = blockIdx.x / p.a.heads, win = row % p.a.nW, rg = row / p.a.nW;
  const int q0 = (blockIdx.y / nt) * TL + wv * 16, k0 = (blockIdx.y % nt) * TL;
  const int b_hi = min(p.a.B, (rg + 1) * ipr);
  const float sc2 = p.scale(h) * LOG2E;
  float acc[4][4];
#pragma unroll
  for (int kj = 0; kj < 4; ++kj)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[kj][r] = 0.f;
  for (int b = rg * ipr; b < b_hi; ++b) {
    const Unit u{b, win, h};
    const AddTerm add(p, u);
    const size_t unit = p.index(u);
    __syncthreads();                                    // the previous image's tiles have been consumed by every wave
    stage_tile_unit(p.k(u), k0, N, ks, kl, nullptr);
    stage_tile<HD>(p.v(u), k0, N, vs, nullptr);
    bf16x8 qf[1], ql[1], df[1];
    load_rows16_unit(p.q(u), q0, N, l15, g, qf, ql);
    load_rows16<HD>(p.tokens(dout, p.a.C, u), q0, N, l15, g, df);
    float lr[4], dr[4];
    row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    __syncthreads();
    f32x4 s[4], dp[4];
    cos_tile(qf, ql, ks, kl, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    p_ds_tile(add, s, dp, lr, dr, q0, k0, N, l15, g, sc2,
              [&](int kj, int r, float pr, float d) { acc[kj][r] = fmaf(pr, d, acc[kj][r]); });
  }
  float* dst = ds_scratch + (size_t)blockIdx.x * N * N;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const int key = k0 + kj * 16 + l15;
      if (key < N) dst[(size_t)q * N + key] = acc[kj][r];
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int images_per_row(int batch) { return tok_cdiv(batch, SCRATCH_ROWS); }
size_t delta_bytes(long long units, int n) { return ((size_t)units * n * sizeof(float) + 255) / 256 * 256; }

// what the forward and the backward check alike; `who` opens each refusal
int check_common(const char* who, AttnArgs& a, const void* qkv, int batch, int h, int w, int c, int heads, int ws, int shift, int ld,
                 const float* logit_scale, const float* bias, const float* mask) {
  const char* why = fill_attn(a, batch, h, w, c, heads, ws, shift, ld);
  TOK_CHECK_ARG(why == nullptr, "%s: bad args: %s", who, why);
  TOK_CHECK_ARG(attn_tiled(a), "%s: ws %d: windows of %d tokens are served by tok_window_attn_fwd / _bwd", who, ws, a.N);
  TOK_CHECK_ARG(logit_scale && bias, "%s: logit_scale / bias are null: the plain mode covers unshifted windows of up to 64 tokens",
                who);
  TOK_CHECK_ARG(qkv, "%s: qkv is null", who);
  TOK_CHECK_ARG(tok_aligned(qkv, 16), "%s: qkv must be 16-byte aligned", who);
  TOK_CHECK_ARG(tok_aligned(logit_scale, 4) && tok_aligned(bias, 4) && tok_aligned(mask, 4),
                "%s: logit_scale / bias / mask must be 4-byte aligned", who);
  const long long units = (long long)batch * a.nW * heads, nt = tok_cdiv(a.N, TL);
  TOK_CHECK_ARG(units * nt < (1ll << 31) && (long long)batch * h * w < (1ll << 31) && nt * nt <= 65535,
                "%s: batch %d x %d windows x %d heads of %d tokens: index range past 2^31", who, batch, a.nW, heads, a.N);
  return TOK_OK;
}

}  // namespace

extern "C" int tok_window_attn_tiled_fwd(const void* qkv, int batch, int h, int w, int c, int heads, int ws, int shift, int ld,
                                         const float* logit_scale, const float* bias, const float* mask, void* out, float* lse,
                                         void* stream) {
  const char* who = "tok_window_attn_tiled_fwd";
  AttnArgs a;
  if (int rc = check_common(who, a, qkv, batch, h, w, c, heads, ws, shift, ld, logit_scale, bias, mask)) return rc;
  TOK_CHECK_ARG(out, "%s: out is null", who);
  TOK_CHECK_ARG(lse, "%s: lse is null", who);
  TOK_CHECK_ARG(tok_aligned(out, 16) && tok_aligned(lse, 4), "%s: out must be 16-byte aligned (lse 4-byte)", who);
  const Tiled p{a, (const bf16*)qkv, logit_scale, bias, mask};
  hipLaunchKernelGGL(wt_fwd_kernel, dim3(batch * a.nW * heads, tok_cdiv(a.N, TL)), dim3(256), 0, tok_stream(stream), p, (bf16*)out,
                     lse);
  return launched(who, "");
}

extern "C" int tok_window_attn_tiled_bwd_rows(int batch, int h, int w, int heads, int ws) {
  AttnArgs a;
  if (fill_attn(a, batch, h, w, heads * HD, heads, ws, 0, 3 * heads * HD) != nullptr || !attn_tiled(a)) return TOK_ERR_INVALID;
  return tok_cdiv(batch, images_per_row(batch)) * a.nW;       // min(batch, SCRATCH_ROWS) * nW
}

extern "C" size_t tok_window_attn_tiled_ws_bytes(int batch, int h, int w, int heads, int ws) {
  AttnArgs a;
  if (fill_attn(a, batch, h, w, heads * HD, heads, ws, 0, 3 * heads * HD) != nullptr || !attn_tiled(a)) return 0;
  const long long units = (long long)batch * a.nW * heads;
  return delta_bytes(units, a.N) + (size_t)units * tok_cdiv(a.N, TL) * sizeof(float);
}

extern "C" int tok_window_attn_tiled_bwd(const void* qkv, const void* dout, int batch, int h, int w, int c, int heads, int ws,
                                         int shift, int ld, const float* logit_scale, const float* bias, const float* mask,
                                         const float* lse, void* dqkv, float* ds_scratch, float* dscale_part, void* ws_buf,
                                         size_t ws_bytes, void* stream) {
  const char* who = "tok_window_attn_tiled_bwd";
  AttnArgs a;
  if (int rc = check_common(who, a, qkv, batch, h, w, c, heads, ws, shift, ld, logit_scale, bias, mask)) return rc;
  TOK_CHECK_ARG(dout, "%s: dout is null", who);
  TOK_CHECK_ARG(lse, "%s: lse is null", who);
  TOK_CHECK_ARG(dqkv, "%s: dqkv is null", who);
  TOK_CHECK_ARG(ds_scratch && dscale_part, "%s: ds_scratch / dscale_part are null", who);
  TOK_CHECK_ARG(ws_buf, "%s: ws_buf is null", who);
  TOK_CHECK_ARG(tok_aligned(dout, 16) && tok_aligned(dqkv, 16) && tok_aligned(ws_buf, 16),
                "%s: dout / dqkv / ws_buf must be 16-byte aligned", who);
  TOK_CHECK_ARG(tok_aligned(lse, 4) && tok_aligned(ds_scratch, 4) && tok_aligned(dscale_part, 4),
                "%s: lse / ds_scratch / dscale_part must be 4-byte aligned", who);
  const size_t need = tok_window_attn_tiled_ws_bytes(batch, h, w, heads, ws);
  if (ws_bytes < need) {
    tok_set_error("%s: ws_bytes %zu < %zu bytes (tok_window_attn_tiled_ws_bytes)", who, ws_bytes, need);
    return TOK_ERR_WORKSPACE;
  }
  hipStream_t st = tok_stream(stream);
  const int units = batch * a.nW * heads, nt = tok_cdiv(a.N, TL), ipr = images_per_row(batch);
  const int rows = tok_cdiv(batch, ipr) * a.nW;
  const Tiled p{a, (const bf16*)qkv, logit_scale, bias, mask};
  const bf16* pd = (const bf16*)dout;
  float* delta = (float*)ws_buf;
  float* dsc_tiles = (float*)((char*)ws_buf + delta_bytes(units, a.N));
  hipLaunchKernelGGL(wt_delta_kernel, dim3(units, nt), dim3(256), 0, st, p, pd, lse, delta);
  if (int rc = launched(who, "(delta)")) return rc;
  hipLaunchKernelGGL(wt_dkv_kernel, dim3(units, nt), dim3(256), 0, st, p, pd, lse, (const float*)delta, (bf16*)dqkv);
  if (int rc = launched(who, "(dkv)")) return rc;
  hipLaunchKernelGGL(wt_dq_kernel, dim3(units, nt), dim3(256), 0, st, p, pd, lse, (const float*)delta, (bf16*)dqkv, dsc_tiles);
  if (int rc = launched(who, "(dq)")) return rc;
  hipLaunchKernelGGL(wt_dscale_fold_kernel, dim3(blocks_of((int64_t)rows * heads)), dim3(256), 0, st, a, (const float*)dsc_tiles, nt,
                     ipr, rows, dscale_part);
  if (int rc = launched(who, "(dscale fold)")) return rc;
  hipLaunchKernelGGL(wt_dlogits_kernel, dim3(rows * heads, nt * nt), dim3(256), 0, st, p, pd, lse, (const float*)delta, ipr,
                     ds_scratch);
  return launched(who, "(dlogits)");
}
