// Window attention of the Global Context ViT ([timm 0.6.13] gcvit.WindowAttentionGlobal.forward between qkv and proj):
//   local  : q, k, v = qkv.reshape(Bw, N, 3, heads, 32).permute(2, 0, 3, 1, 4)
//   global : k, v    = qkv.reshape(Bw, N, 2, heads, 32).permute(2, 0, 3, 1, 4);  q = q_global.repeat(Bw // B, 1, 1, 1)...
//   O = softmax(q k^T * 32^-0.5 + bias[h]) v;  O.transpose(1, 2).reshape(Bw, N, C)
// over the N = ws x ws tokens of a window.  window_partition / window_reverse are index arithmetic on the token grid
// (token_row): qkv rows bf16 [B*H*W][ld] and out rows bf16 [B*H*W][ldo] stay in token order, nothing is permuted in memory.
// Windows are numbered image-major, u = img * nW + wy * nWx + wx; q_global rows are bf16 [B*N][ldg], columns (heads, 32).  In
// global mode window u takes the query of image u mod B (the reference's `repeat` tiles image-minor): query_image is the one
// place that says so.  bias fp32 [heads][N][ldb]; lse fp32 [B*nW][heads][N] (natural log).
//
// Forward : one workgroup per (window, head, 64-query tile), one wave per 16 queries; K / V tiles of 64 keys are staged in LDS
//           (V transposed), S = Q K^T and O += P V on mfma_f32_16x16x32_bf16 (K = head_dim = 32: one instruction per 16 x 16
//           tile of S), online fp32 softmax in exp2 units, key tail masked.  The two modes differ in where the query rows are
//           loaded from and in the column of k and v, nothing else.
// Backward: delta = rowsum(dO o O) as rowsum(P o dP) (pre-pass, see gc_delta_kernel); dK / dV per (window, head, 64-key tile);
//           dQ per 64-query tile of a (window, head) in local mode, of an (image, head) in global mode, where the workgroup walks the windows u = img, img + B, ... in
//           ascending u and keeps the fp32 sum in its accumulators; d(bias) per (64 x 64 tile, head, chunk of windows), walked in
//           ascending u, chunk partials folded in chunk order.  Each recomputes P from q, k, bias and the LSE.  Every output
//           element is written by exactly one lane and every sum runs in a fixed order: no float atomics, bit-reproducible.
#include "tok_common.h"

namespace {

constexpr int HD = 32;         // head_dim served
constexpr int TL = 64;         // tokens per tile (queries of a workgroup, keys per staged tile)
constexpr int PR = 40;         // LDS row pitch of a row-major [token][32] tile in bf16 (80 B: 16-B aligned rows)
constexpr int PT = 72;         // LDS row pitch of a [.][64 tokens] tile in bf16 (144 B)
constexpr int MAXN = 256;      // tokens per window served
constexpr int MAX_CHUNKS = 128;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;
constexpr float SCALE = 0.17677669529663687f;  // 32^-0.5

struct Geo {
  int B, H, W, heads, ws, nwx, nW, N;
};

// the image whose q_global rows window u reads: `repeat` tiles image-minor, so u mod B and not u div nW
__device__ __forceinline__ int query_image(int u, int B) { return u % B; }

// row of token t of window u in the [B*H*W] token order
__device__ __forceinline__ int64_t token_row(const Geo& g, int u, int t) {
  const int img = u / g.nW, wi = u % g.nW;
  const int wy = wi / g.nwx, wx = wi % g.nwx;
  return ((int64_t)img * g.H + wy * g.ws + t / g.ws) * g.W + wx * g.ws + t % g.ws;
}

// the rows of one operand of one (window, head): token t -> 32 contiguous bf16
struct Rows {
  const bf16* base;   // column of the head already added
  int ld;
  int u;              // window (windowed) or first row / N (dense: q_global)
  bool windowed;
  __device__ __forceinline__ const bf16* at(const Geo& g, int t) const {
    return base + (windowed ? token_row(g, u, t) : (int64_t)u * g.N + t) * ld;
  }
};

__device__ __forceinline__ Rows window_rows(const bf16* p, int ld, int col, int u) { return Rows{p + col, ld, u, true}; }
// the query rows of window u: its own tokens, or q_global of image query_image(u)
__device__ __forceinline__ Rows query_rows(const bf16* qkv, int ld, const bf16* qg, int ldg, int col, int u, int B) {
  return qg ? Rows{qg + col, ldg, query_image(u, B), false} : window_rows(qkv, ld, col, u);
}

__device__ __forceinline__ bf16x8 lds8(const bf16* p) { return *reinterpret_cast<const bf16x8*>(p); }

// tokens [r0, r0 + 64) -> LDS row-major [token][PR] and/or transposed [d][PT]; tokens past N are zero.  256 threads: one
// 16-byte piece each.
__device__ __forceinline__ void stage_tile(const Geo& g, const Rows& src, int r0, bf16* rm, bf16* tr) {
  const int row = threadIdx.x >> 2, d0 = (threadIdx.x & 3) * 8, t = r0 + row;
  const bf16x8 v = t < g.N ? ldg16(src.at(g, t) + d0) : zero8();
  if (rm) *reinterpret_cast<bf16x8*>(rm + row * PR + d0) = v;
  if (tr) {
#pragma unroll
    for (int j = 0; j < 8; ++j) tr[(d0 + j) * PT + row] = v[j];
  }
}

// A lane is (l15, g) = (lane & 15, lane >> 4).  Element (j, r) of a product is row 4 g + r of the A operand's 16 rows against
// row 16 j + l15 of the 64-row LDS tile.

// tokens [r0, r0 + 16) as an A operand (the lane: token r0 + l15, dims 8 g ... + 7); tokens past N are zero
__device__ __forceinline__ bf16x8 load_rows16(const Geo& geo, const Rows& src, int r0, int l15, int g) {
  const int t = r0 + l15;
  return t < geo.N ? ldg16(src.at(geo, t) + 8 * g) : zero8();
}

// acc = a x tile^T, tile a row-major LDS tile [64][PR]
__device__ __forceinline__ void frag_x_tile(const bf16x8 a, const bf16* tile, int l15, int g, f32x4 (&acc)[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j)
    acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, lds8(tile + (j * 16 + l15) * PR + 8 * g), (f32x4){0.f, 0.f, 0.f, 0.f}, 0, 0,
                                                     0);
}

// acc += rows x tile_t^T: the [16][PT] rows a wave staged in LDS (P, dS or their transposes) times a transposed tile [32][PT]
__device__ __forceinline__ void rows_x_tile_t(const bf16* rows, const bf16* tile_t, int l15, int g, f32x4 (&acc)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    const bf16x8 a = lds8(rows + l15 * PT + 32 * t + 8 * g);
#pragma unroll
    for (int j = 0; j < 2; ++j)
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, lds8(tile_t + (j * 16 + l15) * PT + 32 * t + 8 * g), acc[j], 0, 0, 0);
  }
}

__device__ __forceinline__ float mul_rn(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// P = exp2(s * 32^-0.5 * log2e - lb), lb = lse * log2e - bias * log2e formed by the caller as fma(-bias, log2e, lse2): every
// backward kernel uses this one form
__device__ __forceinline__ float prob(float s, float lb) { return exp2f(fmaf(s, SCALE * LOG2E, -lb)); }

// log-sum-exp in log2 units (INFINITY past N: P = 0) and delta (0 past N) of the query rows q ... q + 3
__device__ __forceinline__ void load_row_stats(const float* __restrict__ lrow, const float* __restrict__ drow, int q, int n,
                                               float (&lr)[4], float (&dr)[4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = q + r < n ? mul_rn(lrow[q + r], LOG2E) : INFINITY;
    dr[r] = q + r < n ? drow[q + r] : 0.f;
  }
}

// grid (B * nW * heads, query tiles): unit = u * heads + h, so the heads of a window are neighbours
__global__ __launch_bounds__(256) void gc_fwd_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                     const float* __restrict__ bias, int ldb, Geo geo, bf16* __restrict__ out,
                                                     int ldo, float* __restrict__ lse) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];        // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vt[HD * PT];        // V^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 ps[4][16 * PT];     // per wave: P [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int u = blockIdx.x / geo.heads, h = blockIdx.x % geo.heads, C = geo.heads * HD, N = geo.N;
  const int q0 = blockIdx.y * TL + wv * 16;
  const int kcol = (qg ? 0 : C) + h * HD;
  const Rows krows = window_rows(qkv, ld, kcol, u), vrows = window_rows(qkv, ld, kcol + C, u);
  const bf16x8 qf = load_rows16(geo, query_rows(qkv, ld, qg, ldg, h * HD, u, geo.B), q0, l15, g);
  float m[4], l[4];
  f32x4 o[2];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    m[r] = -INFINITY;
    l[r] = 0.f;
  }
  o[0] = o[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const float sc = SCALE * LOG2E;
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();                                    // the previous tile has been consumed by every wave
    stage_tile(geo, krows, k0, ks, nullptr);
    stage_tile(geo, vrows, k0, nullptr, vt);
    __syncthreads();
    f32x4 s[4];
    frag_x_tile(qf, ks, l15, g, s);
    // element (kj, r): query 4g + r of the wave's 16, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float v[4], mx = -INFINITY;
      const int q = q0 + 4 * g + r;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        const float bl = (key < N && q < N) ? mul_rn(bias[((size_t)h * N + q) * ldb + key], LOG2E) : 0.f;
        v[kj] = (key < N) ? fmaf(s[kj][r], sc, bl) : -INFINITY;
        mx = fmaxf(mx, v[kj]);
      }
      const float mn = fmaxf(m[r], row16_max(mx));       // finite: key k0 < N is in every tile
      const float alpha = exp2f(m[r] - mn);
      float ls = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float p = exp2f(v[kj] - mn);
        ls += p;
        ps[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(p);
      }
      l[r] = l[r] * alpha + row16_sum(ls);
      m[r] = mn;
      o[0][r] *= alpha;
      o[1][r] *= alpha;
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
    bf16* orow = out + token_row(geo, u, q) * ldo + h * HD;
    orow[l15] = f2bf(o[0][r] * inv);
    orow[16 + l15] = f2bf(o[1][r] * inv);
    if (l15 == 0) lse[((size_t)blockIdx.x) * N + q] = (m[r] + log2f(l[r])) * LN2;
  }
}

// delta[u][h][q] = sum_j P[q][j] dP[q][j] with dP = dO V^T: rowsum(dO o O) of the UNROUNDED O, formed from the same P and dP that dS
// is formed from, so that the rows of dS = P (dP - delta) sum to zero as far as fp32 goes.  rowsum(dO o O) of the bf16 O the
// forward stored is off by 2^-9 |dO| |O| per term, and dP - delta cancels: where the values of a window lie close together (the
// tokens behind a LayerNorm) that error came to dominate dS — d(q_global) was 2x further from fp64 than a bf16-autocast run.
// grid (units, query tiles) as the forward; a wave owns 16 queries and walks the key tiles in order.
__global__ __launch_bounds__(256) void gc_delta_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                       const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, Geo geo, float* __restrict__ delta) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int u = blockIdx.x / geo.heads, h = blockIdx.x % geo.heads, C = geo.heads * HD, N = geo.N;
  const int q0 = blockIdx.y * TL + wv * 16;
  const int kcol = (qg ? 0 : C) + h * HD;
  const Rows krows = window_rows(qkv, ld, kcol, u), vrows = window_rows(qkv, ld, kcol + C, u);
  const bf16x8 qf = load_rows16(geo, query_rows(qkv, ld, qg, ldg, h * HD, u, geo.B), q0, l15, g);
  const bf16x8 df = load_rows16(geo, window_rows(dout, ldo, h * HD, u), q0, l15, g);
  const float* bias_h = bias + (size_t)h * N * ldb;
  const float* lrow = lse + (size_t)blockIdx.x * N;
  float lr[4], acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = q0 + 4 * g + r < N ? mul_rn(lrow[q0 + 4 * g + r], LOG2E) : INFINITY;
    acc[r] = 0.f;
  }
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile(geo, krows, k0, ks, nullptr);
    stage_tile(geo, vrows, k0, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile(qf, ks, l15, g, s);
    frag_x_tile(df, vs, l15, g, dp);
    // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r;
      float part = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        const bool live = key < N;
        const float lb = (live && q < N) ? fmaf(-bias_h[(size_t)q * ldb + key], LOG2E, lr[r]) : lr[r];
        part = fmaf(live ? prob(s[kj][r], lb) : 0.f, dp[kj][r], part);
      }
      acc[r] += row16_sum(part);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q < N && l15 == 0) delta[(size_t)blockIdx.x * N + q] = acc[r];
  }
}

// dK, dV of 64 keys of a (window, head): a wave owns 16 keys and walks every query tile.  grid (units, key tiles)
__global__ __launch_bounds__(256) void gc_dkv_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                     const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                     int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                     Geo geo, bf16* __restrict__ dqkv, int ldd) {
  __shared__ __attribute__((aligned(16))) bf16 qs[TL * PR];       // Q [query][d]
  __shared__ __attribute__((aligned(16))) bf16 qt[HD * PT];       // Q^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 dos[TL * PR];      // dO [query][d]
  __shared__ __attribute__((aligned(16))) bf16 dot[HD * PT];      // dO^T [d][query]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: P^T, then dS^T [key][query]
  __shared__ float lsl[TL], dl[TL];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int u = blockIdx.x / geo.heads, h = blockIdx.x % geo.heads, C = geo.heads * HD, N = geo.N;
  const int k0 = blockIdx.y * TL + wv * 16;
  const int kcol = (qg ? 0 : C) + h * HD;
  const Rows qrows = query_rows(qkv, ld, qg, ldg, h * HD, u, geo.B), drows = window_rows(dout, ldo, h * HD, u);
  const float* lrow = lse + (size_t)blockIdx.x * N;
  const float* drow = delta + (size_t)blockIdx.x * N;
  const bf16x8 kf = load_rows16(geo, window_rows(qkv, ld, kcol, u), k0, l15, g);
  const bf16x8 vf = load_rows16(geo, window_rows(qkv, ld, kcol + C, u), k0, l15, g);
  f32x4 dk[2], dv[2];
  dk[0] = dk[1] = dv[0] = dv[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int q0 = 0; q0 < N; q0 += TL) {
    __syncthreads();
    stage_tile(geo, qrows, q0, qs, qt);
    stage_tile(geo, drows, q0, dos, dot);
    if (threadIdx.x < TL) {
      const int q = q0 + threadIdx.x;
      lsl[threadIdx.x] = q < N ? mul_rn(lrow[q], LOG2E) : INFINITY;      // queries past N: P = 0
      dl[threadIdx.x] = q < N ? drow[q] : 0.f;
    }
    __syncthreads();
    f32x4 st[4], dpt[4];
    frag_x_tile(kf, qs, l15, g, st);
    frag_x_tile(vf, dos, l15, g, dpt);
    // S^T and dP^T leave the accumulator file here, in one go (the note at the same place in attn_global.hip: without it hipcc
    // may schedule a v_accvgpr_read onto the data register of a ds_write_b16 still in flight; tools/isa_lint.py)
    asm volatile("" : "+v"(st[0]), "+v"(st[1]), "+v"(st[2]), "+v"(st[3]), "+v"(dpt[0]), "+v"(dpt[1]), "+v"(dpt[2]), "+v"(dpt[3]));
    // element (qj, r): key k0 + 4g + r, query q0 + 16 qj + l15
    float dsv[4][4];
#pragma unroll
    for (int qj = 0; qj < 4; ++qj) {
      const int ql = qj * 16 + l15;
      const float lq = lsl[ql], dq = dl[ql];
      float lqb[4] = {lq, lq, lq, lq};
      // keys k0 + 4g ... + 3 of query row q0 + ql: one aligned 16-byte load (ldb % 4 == 0 keeps it inside the row)
      const int q = q0 + ql, kb = k0 + 4 * g;
      if (q < N && kb < N) {
        const float4 b4 = *reinterpret_cast<const float4*>(bias + ((size_t)h * N + q) * ldb + kb);
        const float bv[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int r = 0; r < 4; ++r) lqb[r] = kb + r < N ? fmaf(-bv[r], LOG2E, lq) : lq;
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
    bf16* row = dqkv + token_row(geo, u, k) * ldd + kcol;
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
      row[dj * 16 + l15] = f2bf(dk[dj][r] * SCALE);
      row[C + dj * 16 + l15] = f2bf(dv[dj][r]);
    }
  }
}

// dS = P (dP - delta) of the wave's 16 queries against the 64 keys from k0: sink(kj, r, p, d) takes the two factors of element
// (kj, r), with p = 0 for a key past N
template <class Sink>
__device__ __forceinline__ void ds_tile(const f32x4 (&s)[4], const f32x4 (&dp)[4], const float (&lr)[4], const float (&dr)[4],
                                        const float* __restrict__ bias_h, int ldb, int q0, int k0, int n, int l15, int g,
                                        Sink&& sink) {
#pragma unroll
  for (int kj = 0; kj < 4; ++kj) {
    const int key = k0 + kj * 16 + l15;
    const bool live = key < n;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r;
      const float lb = (live && q < n) ? fmaf(-bias_h[(size_t)q * ldb + key], LOG2E, lr[r]) : lr[r];
      const float p = prob(s[kj][r], lb);
      sink(kj, r, live ? p : 0.f, dp[kj][r] - dr[r]);
    }
  }
}

// dQ of 64 queries.  Local mode (qg == NULL): grid.x = (window, head), the workgroup serves its window and writes d(qkv).
// Global mode: grid.x = (image, head), the workgroup walks the windows u = img, img + B, ... (the windows whose query_image is
// img) in ascending u, its accumulators carry the sum, and it writes d(q_global) of that image.
__global__ __launch_bounds__(256) void gc_dq_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                    const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                    int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                    Geo geo, bf16* __restrict__ dq_out, int lddq) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kt[HD * PT];       // K^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: dS [query][key]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int first = blockIdx.x / geo.heads, h = blockIdx.x % geo.heads, C = geo.heads * HD, N = geo.N;
  const int q0 = blockIdx.y * TL + wv * 16;
  const int kcol = (qg ? 0 : C) + h * HD;
  const int walk = qg ? geo.nW : 1, step = qg ? geo.B : 0;        // query_image(first + j * B) == first
  const bf16x8 qf = load_rows16(geo, query_rows(qkv, ld, qg, ldg, h * HD, first, geo.B), q0, l15, g);
  const float* bias_h = bias + (size_t)h * N * ldb;
  f32x4 dq[2];
  dq[0] = dq[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < walk; ++j) {
    const int u = first + j * step;
    const size_t unit = (size_t)u * geo.heads + h;
    const bf16x8 df = load_rows16(geo, window_rows(dout, ldo, h * HD, u), q0, l15, g);
    float lr[4], dr[4];
    load_row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    const Rows krows = window_rows(qkv, ld, kcol, u), vrows = window_rows(qkv, ld, kcol + C, u);
    for (int k0 = 0; k0 < N; k0 += TL) {
      __syncthreads();
      stage_tile(geo, krows, k0, ks, kt);
      stage_tile(geo, vrows, k0, vs, nullptr);
      __syncthreads();
      f32x4 s[4], dp[4];
      frag_x_tile(qf, ks, l15, g, s);
      frag_x_tile(df, vs, l15, g, dp);
      // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
      ds_tile(s, dp, lr, dr, bias_h, ldb, q0, k0, N, l15, g,
              [&](int kj, int r, float p, float d) { ws[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(p * d); });
      __syncthreads();
      rows_x_tile_t(ws[wv], kt, l15, g, dq);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    bf16* row = qg ? dq_out + ((int64_t)first * N + q) * lddq + h * HD : dq_out + token_row(geo, first, q) * lddq + h * HD;
    row[l15] = f2bf(dq[0][r] * SCALE);
    row[16 + l15] = f2bf(dq[1][r] * SCALE);
  }
}

// d(bias)[h][i][j] = sum over the windows of dS_u[i][j]: one workgroup per (64-query x 64-key tile, head, chunk of windows), a
// wave owns 16 queries.  The workgroup walks the windows of its chunk in ascending u, recomputes S and dP of its tile and keeps
// the fp32 sum in registers.  Partials [chunk][h][N][np] are folded in chunk order by gc_dbias_fold_kernel.
__global__ __launch_bounds__(256) void gc_dbias_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                       const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                       Geo geo, int per_chunk, float* __restrict__ part, int np) {
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int N = geo.N, nt = (N + TL - 1) / TL;
  const int h = blockIdx.y, C = geo.heads * HD;
  const int q0 = (blockIdx.x / nt) * TL + wv * 16, k0 = (blockIdx.x % nt) * TL;
  const int kcol = (qg ? 0 : C) + h * HD;
  const int windows = geo.B * geo.nW;
  const int u_lo = blockIdx.z * per_chunk, u_hi = min(windows, u_lo + per_chunk);
  const float* bias_h = bias + (size_t)h * N * ldb;
  float acc[4][4];
#pragma unroll
  for (int kj = 0; kj < 4; ++kj)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[kj][r] = 0.f;
  for (int u = u_lo; u < u_hi; ++u) {
    const size_t unit = (size_t)u * geo.heads + h;
    __syncthreads();                                    // the previous window's tiles have been consumed by every wave
    stage_tile(geo, window_rows(qkv, ld, kcol, u), k0, ks, nullptr);
    stage_tile(geo, window_rows(qkv, ld, kcol + C, u), k0, vs, nullptr);
    const bf16x8 qf = load_rows16(geo, query_rows(qkv, ld, qg, ldg, h * HD, u, geo.B), q0, l15, g);
    const bf16x8 df = load_rows16(geo, window_rows(dout, ldo, h * HD, u), q0, l15, g);
    float lr[4], dr[4];
    load_row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile(qf, ks, l15, g, s);
    frag_x_tile(df, vs, l15, g, dp);
    ds_tile(s, dp, lr, dr, bias_h, ldb, q0, k0, N, l15, g,
            [&](int kj, int r, float p, float d) { acc[kj][r] = fmaf(p, d, acc[kj][r]); });
  }
  float* dst = part + (size_t)blockIdx.z * geo.heads * N * np;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const int key = k0 + kj * 16 + l15;
      if (key < N) dst[((size_t)h * N + q) * np + key] = acc[kj][r];
    }
  }
}

// dbias[h][i][j] (=|+=) sum_chunk part[chunk][h][i][j], chunk order; columns >= N of a row are not touched
__global__ __launch_bounds__(256) void gc_dbias_fold_kernel(const float* __restrict__ part, int chunks, int heads, int N, int np,
                                                            float* __restrict__ dbias, int ldb, int accumulate) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)heads * N * N) return;
  const int j = (int)(i % N);
  const int64_t row = i / N;
  float s = 0.f;
  for (int c = 0; c < chunks; ++c) s += part[((size_t)c * heads * N + row) * np + j];
  float* o = dbias + row * ldb + j;
  *o = accumulate ? *o + s : s;
}

unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

// the geometry both entry points serve; `who` opens each refusal
int check_geo(const char* who, int ld, int global, int ldg, const float* bias, int ldb, int batch, int h, int w, int c, int heads,
              int ws, int ldo, Geo* g) {
  TOK_CHECK_ARG(batch > 0 && h > 0 && w > 0 && heads > 0 && ws > 0, "%s: batch %d, map %dx%d, %d heads, window %d", who, batch, h, w,
                heads, ws);
  TOK_CHECK_ARG(c == heads * HD, "%s: width %d with %d heads: head_dim %d is not served (32 only)", who, c, heads,
                heads > 0 ? c / heads : 0);
  TOK_CHECK_ARG(h % ws == 0 && w % ws == 0, "%s: a %dx%d token map is not a multiple of the window %d", who, h, w, ws);
  TOK_CHECK_ARG((long long)ws * ws <= MAXN, "%s: %d tokens per window (at most %d served)", who, ws * ws, MAXN);
  const int cols = global ? 2 * c : 3 * c;
  TOK_CHECK_ARG(ld >= cols && ld % 8 == 0 && ldo >= c && ldo % 8 == 0 && (!global || (ldg >= c && ldg % 8 == 0)),
                "%s: row pitches ld %d / ldg %d / ldo %d (>= %d / C / C, multiples of 8)", who, ld, ldg, ldo, cols);
  TOK_CHECK_ARG(bias && ldb >= ws * ws && ldb % 4 == 0 && ((uintptr_t)bias & 15) == 0,
                "%s: bias pointer / row pitch ldb %d (16-byte aligned, >= N, a multiple of 4)", who, ldb);
  const long long nw = (long long)(h / ws) * (w / ws);
  TOK_CHECK_ARG((long long)batch * nw * heads < (1ll << 31) && (long long)batch * h * w < (1ll << 31), "%s: problem too large", who);
  *g = Geo{batch, h, w, heads, ws, w / ws, (int)nw, ws * ws};
  return TOK_OK;
}

int launched(const char* who, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TOK_OK;
  tok_set_error("%s%s: launch failed: %s", who, stage, hipGetErrorString(e));
  return TOK_ERR_LAUNCH;
}

size_t delta_bytes(long long units, int n) { return ((size_t)units * n * sizeof(float) + 255) / 256 * 256; }

// windows per d(bias) chunk: enough (tile, head, chunk) workgroups for eight per CU of the 256 where the windows allow it, at
// most MAX_CHUNKS partial tables to fold — the partials do not grow with batch * nW
int dbias_per_chunk(long long windows, int n, int heads) {
  const long long tiles = (long long)tok_cdiv(n, TL) * tok_cdiv(n, TL) * heads;
  long long chunks = (2048 + tiles - 1) / tiles;
  if (chunks > MAX_CHUNKS) chunks = MAX_CHUNKS;
  if (chunks > windows) chunks = windows;
  return tok_cdiv(windows, chunks);
}

}  // namespace

extern "C" int tok_gc_attn_fwd(const void* qkv, int ld, const void* q_global, int ldg, const float* bias, int ldb, int batch, int h,
                               int w, int c, int heads, int ws, void* out, int ldo, float* lse, void* stream) {
  const char* who = "tok_gc_attn_fwd";
  Geo g;
  if (int rc = check_geo(who, ld, q_global != nullptr, ldg, bias, ldb, batch, h, w, c, heads, ws, ldo, &g)) return rc;
  TOK_CHECK_ARG(qkv && out && lse, "%s: null pointer", who);
  hipLaunchKernelGGL(gc_fwd_kernel, dim3(g.B * g.nW * g.heads, tok_cdiv(g.N, TL)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)qkv, ld, (const bf16*)q_global, ldg, bias, ldb, g, (bf16*)out, ldo, lse);
  return launched(who, "");
}

extern "C" size_t tok_gc_attn_bwd_ws_bytes(int batch, int h, int w, int heads, int ws, int global, int want_dbias) {
  (void)global;
  if (batch <= 0 || h <= 0 || w <= 0 || heads <= 0 || ws <= 0 || h % ws || w % ws || (long long)ws * ws > MAXN) return 0;
  const long long windows = (long long)batch * (h / ws) * (w / ws);
  const int n = ws * ws, np = (n + 3) / 4 * 4;
  size_t bytes = delta_bytes(windows * heads, n);
  if (want_dbias) bytes += (size_t)tok_cdiv(windows, dbias_per_chunk(windows, n, heads)) * heads * n * np * sizeof(float);
  return bytes;
}

extern "C" int tok_gc_attn_bwd(const void* qkv, int ld, const void* q_global, int ldg, const float* bias, int ldb, const void* out,
                               const void* dout, int ldo, const float* lse, int batch, int h, int w, int c, int heads, int ws,
                               void* dqkv, int ldd, void* dq_global, int lddg, float* dbias, int dbias_accumulate, void* ws_buf,
                               size_t ws_bytes, void* stream) {
  const char* who = "tok_gc_attn_bwd";
  Geo g;
  const int global = q_global != nullptr;
  if (int rc = check_geo(who, ld, global, ldg, bias, ldb, batch, h, w, c, heads, ws, ldo, &g)) return rc;
  TOK_CHECK_ARG(qkv && out && dout && lse && dqkv && ws_buf && (!global || dq_global), "%s: null pointer", who);
  TOK_CHECK_ARG(ldd >= (global ? 2 : 3) * c && ldd % 8 == 0 && (!global || (lddg >= c && lddg % 8 == 0)),
                "%s: gradient row pitches ldd %d / lddg %d", who, ldd, lddg);
  const size_t need = tok_gc_attn_bwd_ws_bytes(batch, h, w, heads, ws, global, dbias != nullptr);
  if (ws_bytes < need) {
    tok_set_error("%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    return TOK_ERR_WORKSPACE;
  }
  hipStream_t st = tok_stream(stream);
  const long long windows = (long long)g.B * g.nW;
  const int units = (int)(windows * g.heads), nt = tok_cdiv(g.N, TL);
  float* delta = (float*)ws_buf;
  const bf16 *pq = (const bf16*)qkv, *pg = (const bf16*)q_global, *pd = (const bf16*)dout;
  hipLaunchKernelGGL(gc_delta_kernel, dim3(units, nt), dim3(256), 0, st, pq, ld, pg, ldg, bias, ldb, pd, ldo, lse, g, delta);
  if (int rc = launched(who, "(delta)")) return rc;
  hipLaunchKernelGGL(gc_dkv_kernel, dim3(units, nt), dim3(256), 0, st, pq, ld, pg, ldg, bias, ldb, pd, ldo, lse, delta, g,
                     (bf16*)dqkv, ldd);
  if (int rc = launched(who, "(dkv)")) return rc;
  hipLaunchKernelGGL(gc_dq_kernel, dim3(global ? g.B * g.heads : units, nt), dim3(256), 0, st, pq, ld, pg, ldg, bias, ldb, pd, ldo,
                     lse, delta, g, (bf16*)(global ? dq_global : dqkv), global ? lddg : ldd);
  if (int rc = launched(who, "(dq)")) return rc;
  if (!dbias) return TOK_OK;
  float* part = (float*)((char*)ws_buf + delta_bytes(units, g.N));
  const int per = dbias_per_chunk(windows, g.N, g.heads), chunks = tok_cdiv(windows, per), np = (g.N + 3) / 4 * 4;
  hipLaunchKernelGGL(gc_dbias_kernel, dim3(nt * nt, g.heads, chunks), dim3(256), 0, st, pq, ld, pg, ldg, bias, ldb, pd, ldo, lse,
                     delta, g, per, part, np);
  if (int rc = launched(who, "(dbias)")) return rc;
  hipLaunchKernelGGL(gc_dbias_fold_kernel, dim3(blocks_of((int64_t)g.heads * g.N * g.N)), dim3(256), 0, st, (const float*)part,
                     chunks, g.heads, g.N, np, dbias, ldb, dbias_accumulate ? 1 : 0);
  return launched(who, "(fold)");
}
