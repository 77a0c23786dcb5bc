// Global (whole-image) multi-head self-attention of the Vision Transformer.
//
// [timm 0.6.13] vision_transformer.Attention.forward between qkv and proj:
//   q, k, v = qkv.reshape(B, N, 3, H, 64).permute(2, 0, 3, 1, 4);  O = softmax(q k^T * 64^-0.5) v;  O.transpose(1, 2).reshape(B, N, C)
// qkv rows bf16 [B*N][ldq] with columns (3, heads, 64); O rows bf16 [B*N][ldo] at column h*64 + d; lse fp32 [B][H][N] (natural log).
//
// The kernels are the ones of attn_tile.h at head_dim 64 on dense rows: one workgroup per (image, head, 64-token tile), the
// tiles in grid.x.  delta = rowsum(dO o O) is a pre-pass of its own (gattn_delta_kernel).
// Bias    : BEiT's relative-position bias ([timm 0.6.13] beit.Attention) is one more template argument of the same kernels:
//           softmax(q k^T * 64^-0.5 + bias[h]); its gradient is a reduction over the images (gattn_dbias_kernel).
//           On the host one launcher serves both forward entry points and one routine both backward ones (bias == nullptr picks
//           the un-biased kernels).
#include "attn_tile.h"

namespace {

constexpr int HEAD_DIM = 64;   // head_dim served

// BIAS: logits get + bias[h][query][key] (fp32, row pitch ldb, shared by every image).  Without it the kernels are the ones the
// un-biased entry points have always launched.
template <bool BIAS_>
struct Dense {
  static constexpr int HD = HEAD_DIM;
  static constexpr bool BIAS = BIAS_;
  using Reduce = Butterfly16;                   // pinned: the __shfl_xor order of additions
  const bf16* qkv;
  int ld, N, H;
  const float* bias;
  int ldb;
  static __device__ __forceinline__ unsigned unit() { return blockIdx.y; }
  static __device__ __forceinline__ unsigned tile() { return blockIdx.x; }
  __device__ __forceinline__ int n() const { return N; }
  __device__ __forceinline__ int heads() const { return H; }
  __device__ __forceinline__ int kcol(int h) const { return (H + h) * HD; }
  __device__ __forceinline__ DenseRows q(int b, int h) const { return dense_rows(qkv, ld, h * HD, token(b, 0)); }
  __device__ __forceinline__ DenseRows k(int b, int h) const { return dense_rows(qkv, ld, kcol(h), token(b, 0)); }
  __device__ __forceinline__ DenseRows v(int b, int h) const { return dense_rows(qkv, ld, kcol(h) + H * HD, token(b, 0)); }
  __device__ __forceinline__ DenseRows tokens(const bf16* p, int ldp, int b, int h) const {
    return dense_rows(p, ldp, h * HD, token(b, 0));
  }
  __device__ __forceinline__ int64_t token(int b, int t) const { return (int64_t)b * N + t; }
  __device__ __forceinline__ const float* bias_row(int h, int q) const { return bias + ((size_t)h * N + q) * ldb; }
};

template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_fwd_kernel(const bf16* __restrict__ qkv, int ldq, int N, int H,
                                                        bf16* __restrict__ out, int ldo, float* __restrict__ lse,
                                                        const float* __restrict__ bias, int ldb) {
  attn_fwd(Dense<BIAS>{qkv, ldq, N, H, bias, ldb}, out, ldo, lse);
}

// delta[b][h][q] = sum_d dO[q][h*64+d] * O[q][h*64+d]   (one thread per (token, head), fixed order over d).  Pinned: the bf16 O
// the forward stored, where gc_delta_kernel takes the unrounded one.
__global__ __launch_bounds__(256) void gattn_delta_kernel(const bf16* __restrict__ out, const bf16* __restrict__ dout, int ldo,
                                                          int B, int N, int H, float* __restrict__ delta) {
  constexpr int HD = HEAD_DIM;
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

template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_dkv_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                        int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                        int N, int H, bf16* __restrict__ dqkv, int ldd,
                                                        const float* __restrict__ bias, int ldb) {
  attn_dkv(Dense<BIAS>{qkv, ldq, N, H, bias, ldb}, dout, ldo, lse, delta, dqkv, ldd);
}

// dQ of 64 queries: a wave owns 16 queries and walks every key tile
template <bool BIAS>
__global__ __launch_bounds__(256) void gattn_dq_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                       int N, int H, bf16* __restrict__ dqkv, int ldd,
                                                       const float* __restrict__ bias, int ldb) {
  constexpr int HD = HEAD_DIM, PR = HeadDim<HD>::PR, ND = HeadDim<HD>::ND;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kt[HD * PT];       // K^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: dS [query][key]
  const Dense<BIAS> p{qkv, ldq, N, H, bias, ldb};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int b = blockIdx.y / H, h = blockIdx.y % H;
  const int q0 = blockIdx.x * TL + wv * 16;
  bf16x8 qf[HD / 32], df[HD / 32];
  load_rows16<HD>(p.q(b, h), q0, N, l15, g, qf);
  load_rows16<HD>(p.tokens(dout, ldo, b, h), q0, N, l15, g, df);
  float lr[4], dr[4];
  load_row_stats(lse + (size_t)blockIdx.y * N, delta + (size_t)blockIdx.y * N, q0 + 4 * g, N, lr, dr);
  const DenseRows krows = p.k(b, h), vrows = p.v(b, h);
  f32x4 dq[ND];
#pragma unroll
  for (int j = 0; j < ND; ++j) dq[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile<HD>(krows, k0, N, ks, kt);
    stage_tile<HD>(vrows, k0, N, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile<HD>(qf, ks, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
    ds_tile<HD>(s, dp, dr, k0, N, l15,
                [&](int kj, int r, bool live) { return lse_less_bias(p, h, q0 + 4 * g + r, k0 + kj * 16 + l15, live, lr[r]); },
                [&](int kj, int r, float pr, float d) { ws[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(pr * d); });
    __syncthreads();
    rows_x_tile_t<HD>(ws[wv], kt, l15, g, dq);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    bf16* row = dqkv + p.token(b, q) * ldd + h * HD;
#pragma unroll
    for (int dj = 0; dj < ND; ++dj) row[dj * 16 + l15] = f2bf(dq[dj][r] * HeadDim<HD>::SCALE);
  }
}

// d(bias)[h][i][j] = sum over images of dS_b[i][j] = P_b (dP_b - delta_b): one workgroup per (64-query x 64-key tile, head, chunk
// of images), a wave owns 16 queries.  The workgroup walks the images of its chunk in image order, recomputes S and dP of its tile
// (16 MFMA per wave and image) and keeps the fp32 sum in registers; the bias values of the tile are loaded once.  Partials
// [chunk][h][N][ldb] are folded in chunk order by attn_dbias_fold_kernel: no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void gattn_dbias_kernel(const bf16* __restrict__ qkv, int ldq, const bf16* __restrict__ dout,
                                                          int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                          const float* __restrict__ bias, int ldb, int B, int N, int H,
                                                          int per_chunk, float* __restrict__ part) {
  constexpr int HD = HEAD_DIM, PR = HeadDim<HD>::PR;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const Dense<true> p{qkv, ldq, N, H, bias, ldb};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int nt = (N + TL - 1) / TL;
  const int h = blockIdx.y;
  const int q0 = (blockIdx.x / nt) * TL + wv * 16, k0 = (blockIdx.x % nt) * TL;
  const int b_lo = blockIdx.z * per_chunk, b_hi = min(B, b_lo + per_chunk);
  // pinned: bl = bias * log2e rounded and loaded once, outside the image loop, then lb = lse - bl: two roundings where dkv, dq
  // and gc_dbias_kernel form fma(-bias, log2e, lse) (see prob in attn_tile.h)
  float bl[4][4];
#pragma unroll
  for (int kj = 0; kj < 4; ++kj)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int q = q0 + 4 * g + r, key = k0 + kj * 16 + l15;
      bl[kj][r] = (q < N && key < N) ? mul_rn(p.bias_row(h, q)[key], LOG2E) : 0.f;
    }
  f32x4 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int b = b_lo; b < b_hi; ++b) {
    const size_t unit = (size_t)b * H + h;
    __syncthreads();                                    // the previous image's tiles have been consumed by every wave
    stage_tile<HD>(p.k(b, h), k0, N, ks, nullptr);
    stage_tile<HD>(p.v(b, h), k0, N, vs, nullptr);
    bf16x8 qf[HD / 32], df[HD / 32];
    load_rows16<HD>(p.q(b, h), q0, N, l15, g, qf);
    load_rows16<HD>(p.tokens(dout, ldo, b, h), q0, N, l15, g, df);
    float lr[4], dr[4];
    load_row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile<HD>(qf, ks, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    ds_tile<HD>(s, dp, dr, k0, N, l15, [&](int kj, int r, bool) { return sub_rn(lr[r], bl[kj][r]); },
                [&](int kj, int r, float pr, float d) { acc[kj][r] = fmaf(pr, d, acc[kj][r]); });
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

constexpr int MAX_CHUNKS = 64;   // d(bias) partial tables to fold, at most

// the geometry every attention entry point serves; `who` opens each refusal
int check_geo(const char* who, int ldq, int batch, int n, int heads, int head_dim, int ldo) {
  constexpr int HD = HEAD_DIM;
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

extern "C" int tok_global_attn_bias_bwd_chunks(int batch, int n, int heads) {
  if (batch <= 0 || n <= 0 || heads <= 0) return 0;
  return tok_cdiv(batch, dbias_per_chunk(batch, n, heads, MAX_CHUNKS));
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
  const int per = dbias_per_chunk(batch, n, heads, MAX_CHUNKS), chunks = tok_cdiv(batch, per), nt = tok_cdiv(n, TL);
  hipLaunchKernelGGL(gattn_dbias_kernel, dim3(nt * nt, heads, chunks), dim3(256), 0, st, (const bf16*)qkv, ldq, (const bf16*)dout,
                     ldo, lse, delta, bias, ldb, batch, n, heads, per, part);
  if (int rc = launched(who, "(dbias)")) return rc;
  hipLaunchKernelGGL(attn_dbias_fold_kernel, dim3(blocks_of((int64_t)heads * n * n)), dim3(256), 0, st, (const float*)part,
                     chunks, heads, n, ldb, dbias, ldb, accumulate ? 1 : 0);
  return launched(who, "(fold)");
}

extern "C" int tok_global_attn_bwd(const void* qkv, int ldq, const void* out, const void* dout, int ldo, const float* lse,
                                   int batch, int n, int heads, int head_dim, void* dqkv, int ldd, void* ws, size_t ws_bytes,
                                   void* stream) {
  const char* who = "tok_global_attn_bwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && dout && lse && dqkv && ws, "%s: null pointer", who);
  TOK_CHECK_ARG(ldd >= 3 * heads * HEAD_DIM && ldd % 8 == 0, "%s: ldd %d", who, ldd);
  return launch_bwd(who, qkv, ldq, out, dout, ldo, lse, nullptr, 0, batch, n, heads, dqkv, ldd, nullptr, 0, ws, ws_bytes, stream);
}

extern "C" int tok_global_attn_bias_bwd(const void* qkv, int ldq, const void* out, const void* dout, int ldo, const float* lse,
                                        const float* bias, int ldb, int batch, int n, int heads, int head_dim, void* dqkv,
                                        int ldd, float* dbias, int dbias_accumulate, void* ws, size_t ws_bytes, void* stream) {
  const char* who = "tok_global_attn_bias_bwd";
  if (int rc = check_geo(who, ldq, batch, n, heads, head_dim, ldo)) return rc;
  TOK_CHECK_ARG(qkv && out && dout && lse && dqkv && ws, "%s: null pointer", who);
  if (int rc = check_bias(who, bias, ldb, n)) return rc;
  TOK_CHECK_ARG(ldd >= 3 * heads * HEAD_DIM && ldd % 8 == 0, "%s: ldd %d", who, ldd);
  return launch_bwd(who, qkv, ldq, out, dout, ldo, lse, bias, ldb, batch, n, heads, dqkv, ldd, dbias, dbias_accumulate, ws, ws_bytes,
                    stream);
}
