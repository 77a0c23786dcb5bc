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
// The kernels are the ones of attn_tile.h at head_dim 32 (one MFMA per 16 x 16 tile of S) on window-relative rows: one
// workgroup per (window, head, 64-token tile), grid (B * nW * heads, tiles) with unit = u * heads + h, so the heads of a window
// are neighbours.  The two modes differ in where the query rows are loaded from and in the column of k and v, nothing else.
// Backward: delta = rowsum(dO o O) as rowsum(P o dP) (pre-pass, see gc_delta_kernel); dK / dV per (window, head, 64-key tile);
//           dQ per 64-query tile of a (window, head) in local mode, of an (image, head) in global mode, where the workgroup walks
//           the windows u = img, img + B, ... in ascending u and keeps the fp32 sum in its accumulators and writes d(q_global) of
//           that image; d(bias) per (64 x 64 tile, head, chunk of windows), walked in ascending u, chunk partials folded in
//           chunk order.
#include "attn_tile.h"

namespace {

constexpr int HEAD_DIM = 32;   // head_dim served
constexpr int MAXN = 256;      // tokens per window served
constexpr int MAX_CHUNKS = 128;

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
  Geo g;              // by value: a stored reference to the kernel's Geo cost up to 9 % of the backward (hipcc kept it in memory early on)
  __device__ __forceinline__ int64_t row(int t) const { return windowed ? token_row(g, u, t) : (int64_t)u * g.N + t; }
  __device__ __forceinline__ const bf16* at(int t) const { return base + row(t) * ld; }
};

__device__ __forceinline__ Rows window_rows(const Geo& g, const bf16* p, int ld, int col, int u) {
  return Rows{p + col, ld, u, true, g};
}
// the query rows of window u: its own tokens, or q_global of image query_image(u)
__device__ __forceinline__ Rows query_rows(const Geo& g, const bf16* qkv, int ld, const bf16* qg, int ldg, int col, int u) {
  return qg ? Rows{qg + col, ldg, query_image(u, g.B), false, g} : window_rows(g, qkv, ld, col, u);
}

// GCViT is always biased.  qg == NULL: local mode, qkv has the columns (3, heads, 32); else (2, heads, 32) and the query is
// q_global's.
struct Windowed {
  static constexpr int HD = HEAD_DIM;
  static constexpr bool BIAS = true;
  using Reduce = DppRow16;                      // pinned: the DPP rotate order of additions
  const bf16* qkv;
  int ld;
  const bf16* qg;
  int ldg;
  const float* bias;
  int ldb;
  Geo geo;
  static __device__ __forceinline__ unsigned unit() { return blockIdx.x; }
  static __device__ __forceinline__ unsigned tile() { return blockIdx.y; }
  __device__ __forceinline__ int n() const { return geo.N; }
  __device__ __forceinline__ int heads() const { return geo.heads; }
  __device__ __forceinline__ int kcol(int h) const { return (qg ? 0 : geo.heads * HD) + h * HD; }
  __device__ __forceinline__ Rows q(int u, int h) const { return query_rows(geo, qkv, ld, qg, ldg, h * HD, u); }
  __device__ __forceinline__ Rows k(int u, int h) const { return window_rows(geo, qkv, ld, kcol(h), u); }
  __device__ __forceinline__ Rows v(int u, int h) const { return window_rows(geo, qkv, ld, kcol(h) + geo.heads * HD, u); }
  __device__ __forceinline__ Rows tokens(const bf16* p, int ldp, int u, int h) const { return window_rows(geo, p, ldp, h * HD, u); }
  __device__ __forceinline__ int64_t token(int u, int t) const { return token_row(geo, u, t); }
  __device__ __forceinline__ const float* bias_row(int h, int q) const { return bias + (size_t)h * geo.N * ldb + (size_t)q * ldb; }
};

__global__ __launch_bounds__(256) void gc_fwd_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                     const float* __restrict__ bias, int ldb, Geo geo, bf16* __restrict__ out,
                                                     int ldo, float* __restrict__ lse) {
  attn_fwd(Windowed{qkv, ld, qg, ldg, bias, ldb, geo}, out, ldo, lse);
}

// delta[u][h][q] = sum_j P[q][j] dP[q][j] with dP = dO V^T: rowsum(dO o O) of the UNROUNDED O, formed from the same P and dP that dS
// is formed from, so that the rows of dS = P (dP - delta) sum to zero as far as fp32 goes.  rowsum(dO o O) of the bf16 O the
// forward stored is off by 2^-9 |dO| |O| per term, and dP - delta cancels: where the values of a window lie close together (the
// tokens behind a LayerNorm) that error came to dominate dS — d(q_global) was 2x further from fp64 than a bf16-autocast run.
// grid (units, query tiles) as the forward; a wave owns 16 queries and walks the key tiles in order.
__global__ __launch_bounds__(256) void gc_delta_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                       const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, Geo geo, float* __restrict__ delta) {
  constexpr int HD = HEAD_DIM, PR = HeadDim<HD>::PR;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const Windowed p{qkv, ld, qg, ldg, bias, ldb, geo};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const unsigned unit = Windowed::unit();
  const int u = unit / geo.heads, h = unit % geo.heads, N = geo.N;
  const int q0 = Windowed::tile() * TL + wv * 16;
  const Rows krows = p.k(u, h), vrows = p.v(u, h);
  bf16x8 qf[1], df[1];
  load_rows16<HD>(p.q(u, h), q0, N, l15, g, qf);
  load_rows16<HD>(p.tokens(dout, ldo, u, h), q0, N, l15, g, df);
  const float* lrow = lse + (size_t)unit * N;
  float lr[4], acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    lr[r] = q0 + 4 * g + r < N ? mul_rn(lrow[q0 + 4 * g + r], LOG2E) : INFINITY;
    acc[r] = 0.f;
  }
  for (int k0 = 0; k0 < N; k0 += TL) {
    __syncthreads();
    stage_tile<HD>(krows, k0, N, ks, nullptr);
    stage_tile<HD>(vrows, k0, N, vs, nullptr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile<HD>(qf, ks, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    // element (kj, r): query q0 + 4g + r, key k0 + 16 kj + l15
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      float part = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int key = k0 + kj * 16 + l15;
        const bool live = key < N;
        const float lb = lse_less_bias(p, h, q0 + 4 * g + r, key, live, lr[r]);
        part = fmaf(live ? prob<HD>(s[kj][r], lb) : 0.f, dp[kj][r], part);
      }
      acc[r] += row16_sum(part);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q < N && l15 == 0) delta[(size_t)unit * N + q] = acc[r];
  }
}

__global__ __launch_bounds__(256) void gc_dkv_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                     const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                     int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                     Geo geo, bf16* __restrict__ dqkv, int ldd) {
  attn_dkv(Windowed{qkv, ld, qg, ldg, bias, ldb, geo}, dout, ldo, lse, delta, dqkv, ldd);
}

// dQ of 64 queries.  Local mode (qg == NULL): grid.x = (window, head), the workgroup serves its window and writes d(qkv).
// Global mode: grid.x = (image, head), the workgroup walks the windows u = img, img + B, ... (the windows whose query_image is
// img) in ascending u, its accumulators carry the sum, and it writes d(q_global) of that image.
// A kernel of its own on the shared pieces, with gc_dbias_kernel: as instantiations of one body with the dense family's both were
// slower than this text (profiles/attn_family_ab.txt), although every output bit was the same.
__global__ __launch_bounds__(256) void gc_dq_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                    const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                    int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                    Geo geo, bf16* __restrict__ dq_out, int lddq) {
  constexpr int HD = HEAD_DIM, PR = HeadDim<HD>::PR;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 kt[HD * PT];       // K^T [d][key]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  __shared__ __attribute__((aligned(16))) bf16 ws[4][16 * PT];    // per wave: dS [query][key]
  const Windowed p{qkv, ld, qg, ldg, bias, ldb, geo};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int first = blockIdx.x / geo.heads, h = blockIdx.x % geo.heads, N = geo.N;
  const int q0 = blockIdx.y * TL + wv * 16;
  const int walk = qg ? geo.nW : 1, step = qg ? geo.B : 0;        // query_image(first + j * B) == first
  bf16x8 qf[1];
  load_rows16<HD>(p.q(first, h), q0, N, l15, g, qf);
  const float* bias_h = bias + (size_t)h * N * ldb;
  f32x4 dq[2];
  dq[0] = dq[1] = (f32x4){0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < walk; ++j) {
    const int u = first + j * step;
    const size_t unit = (size_t)u * geo.heads + h;
    bf16x8 df[1];
    load_rows16<HD>(p.tokens(dout, ldo, u, h), q0, N, l15, g, df);
    float lr[4], dr[4];
    load_row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    const Rows krows = p.k(u, h), vrows = p.v(u, h);
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
                  [&](int kj, int r, bool live) {
                    const int q = q0 + 4 * g + r, key = k0 + kj * 16 + l15;
                    return (live && q < N) ? fmaf(-bias_h[(size_t)q * ldb + key], LOG2E, lr[r]) : lr[r];
                  },
                  [&](int kj, int r, float pr, float d) { ws[wv][(4 * g + r) * PT + kj * 16 + l15] = f2bf(pr * d); });
      __syncthreads();
      rows_x_tile_t<HD>(ws[wv], kt, l15, g, dq);
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int q = q0 + 4 * g + r;
    if (q >= N) continue;
    bf16* row = qg ? dq_out + ((int64_t)first * N + q) * lddq + h * HD : dq_out + token_row(geo, first, q) * lddq + h * HD;
    row[l15] = f2bf(dq[0][r] * HeadDim<HD>::SCALE);
    row[16 + l15] = f2bf(dq[1][r] * HeadDim<HD>::SCALE);
  }
}

// d(bias)[h][i][j] = sum over the windows of dS_u[i][j]: one workgroup per (64-query x 64-key tile, head, chunk of windows), a
// wave owns 16 queries.  The workgroup walks the windows of its chunk in ascending u, recomputes S and dP of its tile and keeps
// the fp32 sum in registers.  Partials [chunk][h][N][np], np = N rounded up to 4, are folded in chunk order by
// attn_dbias_fold_kernel.
__global__ __launch_bounds__(256) void gc_dbias_kernel(const bf16* __restrict__ qkv, int ld, const bf16* __restrict__ qg, int ldg,
                                                       const float* __restrict__ bias, int ldb, const bf16* __restrict__ dout,
                                                       int ldo, const float* __restrict__ lse, const float* __restrict__ delta,
                                                       Geo geo, int per_chunk, float* __restrict__ part, int np) {
  constexpr int HD = HEAD_DIM, PR = HeadDim<HD>::PR;
  __shared__ __attribute__((aligned(16))) bf16 ks[TL * PR];       // K [key][d]
  __shared__ __attribute__((aligned(16))) bf16 vs[TL * PR];       // V [key][d]
  const Windowed p{qkv, ld, qg, ldg, bias, ldb, geo};
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int N = geo.N, nt = (N + TL - 1) / TL;
  const int h = blockIdx.y;
  const int q0 = (blockIdx.x / nt) * TL + wv * 16, k0 = (blockIdx.x % nt) * TL;
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
    stage_tile<HD>(p.k(u, h), k0, N, ks, nullptr);
    stage_tile<HD>(p.v(u, h), k0, N, vs, nullptr);
    bf16x8 qf[1], df[1];
    load_rows16<HD>(p.q(u, h), q0, N, l15, g, qf);
    load_rows16<HD>(p.tokens(dout, ldo, u, h), q0, N, l15, g, df);
    float lr[4], dr[4];
    load_row_stats(lse + unit * N, delta + unit * N, q0 + 4 * g, N, lr, dr);
    __syncthreads();
    f32x4 s[4], dp[4];
    frag_x_tile<HD>(qf, ks, l15, g, s);
    frag_x_tile<HD>(df, vs, l15, g, dp);
    ds_tile<HD>(s, dp, dr, k0, N, l15,
                [&](int kj, int r, bool live) {
                  const int q = q0 + 4 * g + r, key = k0 + kj * 16 + l15;
                  return (live && q < N) ? fmaf(-bias_h[(size_t)q * ldb + key], LOG2E, lr[r]) : lr[r];
                },
                [&](int kj, int r, float pr, float d) { acc[kj][r] = fmaf(pr, d, acc[kj][r]); });
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

// the geometry both entry points serve; `who` opens each refusal
int check_geo(const char* who, int ld, int global, int ldg, const float* bias, int ldb, int batch, int h, int w, int c, int heads,
              int ws, int ldo, Geo* g) {
  TOK_CHECK_ARG(batch > 0 && h > 0 && w > 0 && heads > 0 && ws > 0, "%s: batch %d, map %dx%d, %d heads, window %d", who, batch, h, w,
                heads, ws);
  TOK_CHECK_ARG(c == heads * HEAD_DIM, "%s: width %d with %d heads: head_dim %d is not served (32 only)", who, c, heads,
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

size_t delta_bytes(long long units, int n) { return ((size_t)units * n * sizeof(float) + 255) / 256 * 256; }

}  // namespace

extern "C" int tok_gc_attn_fwd(const void* qkv, int ld, const void* q_global, int ldg, const float* bias, int ldb, int batch, int h,
                               int w, int c, int heads, int ws, void* out, int ldo, float* lse, void* stream) {
  const char* who = "tok_gc_attn_fwd";
  Geo g;              // by value: a stored reference to the kernel's Geo cost up to 9 % of the backward (hipcc kept it in memory early on)
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
  if (want_dbias) bytes += (size_t)tok_cdiv(windows, dbias_per_chunk(windows, n, heads, MAX_CHUNKS)) * heads * n * np * sizeof(float);
  return bytes;
}

extern "C" int tok_gc_attn_bwd(const void* qkv, int ld, const void* q_global, int ldg, const float* bias, int ldb, const void* out,
                               const void* dout, int ldo, const float* lse, int batch, int h, int w, int c, int heads, int ws,
                               void* dqkv, int ldd, void* dq_global, int lddg, float* dbias, int dbias_accumulate, void* ws_buf,
                               size_t ws_bytes, void* stream) {
  const char* who = "tok_gc_attn_bwd";
  Geo g;              // by value: a stored reference to the kernel's Geo cost up to 9 % of the backward (hipcc kept it in memory early on)
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
  const int per = dbias_per_chunk(windows, g.N, g.heads, MAX_CHUNKS), chunks = tok_cdiv(windows, per), np = (g.N + 3) / 4 * 4;
  hipLaunchKernelGGL(gc_dbias_kernel, dim3(nt * nt, g.heads, chunks), dim3(256), 0, st, pq, ld, pg, ldg, bias, ldb, pd, ldo, lse,
                     delta, g, per, part, np);
  if (int rc = launched(who, "(dbias)")) return rc;
  hipLaunchKernelGGL(attn_dbias_fold_kernel, dim3(blocks_of((int64_t)g.heads * g.N * g.N)), dim3(256), 0, st, (const float*)part,
                     chunks, g.heads, g.N, np, dbias, ldb, dbias_accumulate ? 1 : 0);
  return launched(who, "(fold)");
}
