// Window attention of the SwinV2 row: swin.py:71-256 over [timm 0.6.13] swin_transformer_v2.WindowAttention
// (SURVEY.md App. A.3), and the plain windowed softmax(q k^T / sqrt(head_dim)) v of DaViT.
//   cosine attention with learned logit scale, continuous relative position bias and the shifted-window mask; roll /
//   window_partition / window_reverse are index arithmetic on the token grid (exact), nothing is permuted in HBM.
//   windows of up to 64 tokens: attn_fwd_mfma_kernel / attn_bwd_mfma_kernel, written on one toolkit of __forceinline__ pieces;
//   larger windows: the scalar pair attn_fwd_kernel / attn_bwd_kernel, one wave per (image, window, head), lane = query row.
// Tokens are rows of a [B*H*W][C] bf16 matrix, head_dim = 32; softmax in fp32.  Deterministic: no atomics.
// (LayerNorm, column folds, activations: layernorm.hip; the position-bias tables: transformer.hip.)
#include "tok_common.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------------------
// window attention.  One wave per (image, window, head); lane = query row (rows loop for N > 64).
struct AttnArgs {
  int B, H, W, C, heads, ws, shift, nWx, nW, N, ld;   // ld: row pitch of qkv (>= 3C); head_dim = 32
  int plain;   // 1: softmax(q k^T / sqrt(head_dim)) v — no cosine normalisation, logit scale, bias (DaViT, davit.py:168-207)
};

constexpr int HD = 32;

__device__ __forceinline__ int64_t token_row(const AttnArgs& a, int b, int win, int t) {
  const int wy = win / a.nWx, wx = win - wy * a.nWx;
  const int iy = t / a.ws, ix = t - iy * a.ws;
  int oy = wy * a.ws + iy + a.shift, ox = wx * a.ws + ix + a.shift;   // roll(-shift): rolled[i] = x[(i + shift) % H]
  oy = oy >= a.H ? oy - a.H : oy;
  ox = ox >= a.W ? ox - a.W : ox;
  return ((int64_t)b * a.H + oy) * a.W + ox;
}

// loads q, k, v of one (b, window, head) into LDS as fp32, q and k L2-normalised (F.normalize eps 1e-12)
__device__ __forceinline__ void load_qkv(const AttnArgs& a, const bf16* __restrict__ qkv, int b, int win, int h,
                                         float* qn, float* kn, float* v, float* qinv, float* kinv) {
  const int lane = threadIdx.x;
  for (int t = lane; t < a.N; t += 64) {
    const bf16* r = qkv + token_row(a, b, win, t) * a.ld + h * HD;
    float sq = 0.f, sk = 0.f;
#pragma unroll
    for (int d = 0; d < HD; d += 8) {
      const bf16x8 q8 = ldg16(r + d), k8 = ldg16(r + a.C + d), v8 = ldg16(r + 2 * a.C + d);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float qf = bf2f(q8[e]), kf = bf2f(k8[e]);
        qn[t * HD + d + e] = qf;
        kn[t * HD + d + e] = kf;
        v[t * HD + d + e] = bf2f(v8[e]);
        sq = fmaf(qf, qf, sq);
        sk = fmaf(kf, kf, sk);
      }
    }
    const float qi = 1.f / fmaxf(sqrtf(sq), 1e-12f), ki = 1.f / fmaxf(sqrtf(sk), 1e-12f);
    if (qinv) { qinv[t] = qi; kinv[t] = ki; }
    for (int d = 0; d < HD; ++d) { qn[t * HD + d] *= qi; kn[t * HD + d] *= ki; }
  }
}

// logit (i, j) of the scalar kernels in natural-log units: idx = i * N + j
__device__ __forceinline__ float scalar_logit(float s, float scale, const float* __restrict__ bh, const float* __restrict__ mw,
                                              int idx) {
  return s * scale + bh[idx] + (mw ? mw[idx] : 0.f);
}

// F.normalize backward of one token row held by a lane, d = (dn - n <n, dn>) / |x|, and its 16-byte stores
__device__ __forceinline__ void store_normalize_bwd(bf16* dst, const float (&dn)[HD], const float (&n)[HD], float inv) {
  float dot = 0.f;
#pragma unroll
  for (int d = 0; d < HD; ++d) dot = fmaf(n[d], dn[d], dot);
#pragma unroll
  for (int d = 0; d < HD; d += 8) {
    bf16x8 o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = f2bf((dn[d + e] - n[d + e] * dot) * inv);
    stg16(dst + d, o8);
  }
}

__global__ __launch_bounds__(64) void attn_fwd_kernel(AttnArgs a, const bf16* __restrict__ qkv,
                                                      const float* __restrict__ logit_scale,
                                                      const float* __restrict__ bias, const float* __restrict__ mask,
                                                      bf16* __restrict__ out, float* __restrict__ lse) {
  extern __shared__ float sm[];
  float* qn = sm;
  float* kn = qn + a.N * HD;
  float* v = kn + a.N * HD;
  const int h = blockIdx.x % a.heads;
  const int win = (blockIdx.x / a.heads) % a.nW;
  const int b = blockIdx.x / (a.heads * a.nW);
  load_qkv(a, qkv, b, win, h, qn, kn, v, nullptr, nullptr);
  __syncthreads();
  const float scale = expf(fminf(logit_scale[h], 4.605170185988092f));   // clamp(max = ln 100).exp()
  const float* bh = bias + (size_t)h * a.N * a.N;
  const float* mw = mask ? mask + (size_t)win * a.N * a.N : nullptr;
  for (int i = threadIdx.x; i < a.N; i += 64) {
    float q[HD], o[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { q[d] = qn[i * HD + d]; o[d] = 0.f; }
    float mx = -INFINITY, den = 0.f;
    for (int j = 0; j < a.N; ++j) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) s = fmaf(q[d], kn[j * HD + d], s);
      s = scalar_logit(s, scale, bh, mw, i * a.N + j);
      const float nm = fmaxf(mx, s);
      const float corr = expf(mx - nm), p = expf(s - nm);
      den = den * corr + p;
#pragma unroll
      for (int d = 0; d < HD; ++d) o[d] = fmaf(o[d], corr, p * v[j * HD + d]);
      mx = nm;
    }
    const float inv = 1.f / den;
    bf16* orow = out + token_row(a, b, win, i) * a.C + h * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 8) {
      bf16x8 o8;
#pragma unroll
      for (int e = 0; e < 8; ++e) o8[e] = f2bf(o[d + e] * inv);
      stg16(orow + d, o8);
    }
    lse[((size_t)blockIdx.x) * a.N + i] = mx + logf(den);
  }
}

// ---- MFMA kernels for windows of up to 64 tokens (7x7, 8x8): one 4-wave workgroup per (image, window, head) ------
// S = Qn Kn^T as 16x16 tiles of mfma_f32_16x16x32_bf16 (K = head_dim = 32: one instruction per tile), fp32 softmax on
// the accumulator layout (row = 4*(lane>>4)+reg, col = lane&15), P through LDS (bf16) into the A operand of
// O = P V (V kept transposed in LDS so a lane's 8 k-slots are 8 consecutive keys).  Wave w owns query tile w; the
// four waves stage q / k / v (/ dO) in parallel.  (One wave per unit left < 1 wave per SIMD resident: LDS-bound
// occupancy, every latency exposed.)
// Both kernels are written on the pieces below: unit_coords, load_add_tile, request_rows / stage_rows, qk_tiles, stage_kq.  The
// softmax of the forward and the P / dS arithmetic of the backward stay in their kernels: they share no expression.
constexpr int QPITCH = 40;    // bf16 elements per Q/K row in LDS (32 + 8: spreads 16 rows over the banks)
constexpr int PPITCH = 72;    // P rows / transposed rows: 64 + 8
constexpr int ROWMAJ = 64 * QPITCH;                  // one row-major [token][QPITCH] tile; q, k, v (, dO) lie one after another
constexpr int MFMA_FWD_LDS = (3 * ROWMAJ + 64 * PPITCH) * 2;   // bytes per workgroup: q, k, v row-major + P^T
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

typedef __attribute__((address_space(3))) bf16x4 attn_lds_bf16x4;
__device__ __forceinline__ bf16x4 attn_tr4(const bf16* p) { return __builtin_amdgcn_ds_read_tr16_b64_v4bf16((attn_lds_bf16x4*)(p)); }
// fragment of a row-major [token][pitch] tile whose k-slots are tokens 32 ks .. and whose MFMA row / column index is the
// tile column c0 + l15
__device__ __forceinline__ bf16x8 attn_tr_frag(const bf16* tile, int pitch, int ks, int c0, int g, int l15) {
  const bf16* p = tile + (32 * ks + 4 * g + (l15 >> 2)) * pitch + c0 + (l15 & 3) * 4;
  const bf16x4 lo = attn_tr4(p), hi = attn_tr4(p + 16 * pitch);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = lo[e]; r[4 + e] = hi[e]; }
  return r;
}
// the same k-slot order read along a ROW of a [row][pitch] tile: tokens 32 ks + 4g .. +3 and 32 ks + 16 + 4g .. +3
__device__ __forceinline__ bf16x8 attn_row_frag(const bf16* tile, int pitch, int row, int ks, int g) {
  const bf16* p = tile + row * pitch + 32 * ks + 4 * g;
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(p), hi = *reinterpret_cast<const bf16x4*>(p + 16);
  bf16x8 r;
#pragma unroll
  for (int e = 0; e < 4; ++e) { r[e] = lo[e]; r[4 + e] = hi[e]; }
  return r;
}

// Workgroup -> unit.  A 32-wide head slice of a token row is 64 bytes: the heads of a window share 128-byte lines (and a row's
// q / k / v parts are contiguous), so when consecutive workgroups — which the dispatcher deals round-robin to the eight XCDs,
// each with its own L2 — take consecutive heads, every line is fetched by two L2s: PMC read traffic of the round-3 kernels was
// 2.0x the q, k, v, dO bytes (4.43 GB against 2.2 for the SwinV2-T forward launches of a step).  Unit u = (xcd, slot) with
// xcd = blockIdx % 8 instead: each XCD walks a contiguous range of units, so the heads of one window are neighbours in time on
// ONE L2.  The grid is 8 * ceil(units / 8) workgroups; the surplus ones leave at once.  (Speed only: nothing depends on where
// a workgroup really runs.)
__device__ __forceinline__ int attn_unit(int units) {
  const int per = (units + 7) >> 3;
  return (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
}
// the unit of this workgroup and its (head, window, image group); false: a surplus workgroup, which leaves
struct AttnUnit { int id, h, win, bg; };
__device__ __forceinline__ bool unit_coords(int units, const AttnArgs& a, AttnUnit& u) {
  u.id = attn_unit(units);
  if (u.id >= units) return false;
  u.h = u.id % a.heads;
  u.win = (u.id / a.heads) % a.nW;
  u.bg = u.id / (a.heads * a.nW);
  return true;
}

// Additive logit terms of query tile qi (position bias + shift mask; -inf on padding), in log2 units (P = exp2(..)): loaded once
// per workgroup, reused for every image it walks.  element (reg, kj): query i = qi*16 + 4g + reg, key j = kj*16 + l15.
// Straight-line loads on clamped indices + selects: a branch per element puts an s_waitcnt (one exposed L2 round trip) in front
// of each load.
__device__ __forceinline__ void load_add_tile(const float* __restrict__ bias, const float* __restrict__ mask, int h, int win,
                                              int N, int qi, int g, int l15, float (&addt)[4][4]) {
  const float* bh = bias ? bias + (size_t)h * N * N : nullptr;
  const float* mw = mask ? mask + (size_t)win * N * N : nullptr;
  const bool any_add = bh != nullptr || mw != nullptr;
  const float bsel = bh ? 1.f : 0.f, msel = mw ? 1.f : 0.f;
  const float* bp = bh ? bh : mw;
  const float* mp = mw ? mw : bp;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) {
      const int i = qi * 16 + 4 * g + reg, j = kj * 16 + l15;
      const int idx = (i < N ? i : N - 1) * N + (j < N ? j : N - 1);
      float v = 0.f;
      if (any_add) v = (bsel * bp[idx] + msel * mp[idx]) * LOG2E;
      addt[reg][kj] = (i < N && j < N) ? v : -INFINITY;
    }
}

// The image-ahead pipeline.  A lane's token row is loaded in two halves, so that the NEXT image's rows can be in flight while the
// current one is computed: request_rows asks for the 32-wide head slice of token row `row` (wave 0: q, 1: k, 2: v; wave 3: dO
// in the backward, nothing in the forward), stage_rows L2-normalises q and k (F.normalize, eps 1e-12) and puts the row into the
// wave's row-major tile at tiles + wave * ROWMAJ; the backward keeps 1/|q| and 1/|k| in inv_qk[2][64].
template <bool BWD>
__device__ __forceinline__ void request_rows(const AttnArgs& a, const bf16* __restrict__ qkv, const bf16* __restrict__ dout,
                                             int64_t row, int h, int wv, bool valid, bf16x8 (&rnext)[4]) {
  if (!BWD && wv >= 3) return;
  const bf16* src = (!BWD || wv < 3) ? qkv + row * a.ld + h * HD + wv * a.C : dout + row * a.C + h * HD;
#pragma unroll
  for (int d = 0; d < 4; ++d) rnext[d] = valid ? ldg16(src + d * 8) : zero8();
}
__device__ __forceinline__ float finish_head_row(bool normalise, bf16x8 (&o)[4]) {
  if (!normalise) return 1.f;
  float f[HD], ss = 0.f;
#pragma unroll
  for (int d = 0; d < HD; d += 8)
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[d + e] = bf2f(o[d >> 3][e]); ss = fmaf(f[d + e], f[d + e], ss); }
  // F.normalize: 1 / max(|x|, 1e-12) = min(rsqrt(|x|^2), 1e12) — one v_rsq_f32 (the forward and the backward's recomputation
  // use the same expression: the recomputed probabilities are normalised by the forward's log-sum-exp)
  const float inv = fminf(__builtin_amdgcn_rsqf(ss), 1e12f);
#pragma unroll
  for (int d = 0; d < HD; d += 8)
#pragma unroll
    for (int e = 0; e < 8; ++e) o[d >> 3][e] = f2bf(f[d + e] * inv);
  return inv;
}
template <bool BWD>
__device__ __forceinline__ void stage_rows(const AttnArgs& a, bf16* tiles, float* inv_qk, int wv, int t,
                                           const bf16x8 (&rnext)[4]) {
  if (!BWD && wv >= 3) return;
  bf16x8 r8[4];
#pragma unroll
  for (int d = 0; d < 4; ++d) r8[d] = rnext[d];
  const float inv = finish_head_row(wv < 2 && !a.plain, r8);
  bf16* rowmaj = tiles + wv * ROWMAJ;
#pragma unroll
  for (int d = 0; d < HD; d += 8) *reinterpret_cast<bf16x8*>(rowmaj + t * QPITCH + d) = r8[d >> 3];
  if (BWD && wv < 2) inv_qk[wv * 64 + t] = inv;
}

// acc[kj] = rows 16 qi .. + 15 of `rows_tile` against rows 16 kj .. + 15 of `key_tile` (both row-major [token][QPITCH], K = 32):
// S = Qn Kn^T of one query tile against the 64 keys, and the backward's dP = dO V^T
__device__ __forceinline__ void qk_tiles(const bf16* rows_tile, const bf16* key_tile, int qi, int g, int l15, f32x4 (&acc)[4]) {
  const bf16x8 qf = *reinterpret_cast<const bf16x8*>(rows_tile + (qi * 16 + l15) * QPITCH + g * 8);
#pragma unroll
  for (int kj = 0; kj < 4; ++kj) {
    const bf16x8 kf = *reinterpret_cast<const bf16x8*>(key_tile + (kj * 16 + l15) * QPITCH + g * 8);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    acc[kj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qf, kf, z, 0, 0, 0);
  }
}

// [key][query] staging of an accumulator-layout matrix: this lane holds queries qi*16 + 4g .. +3 of key kj*16 + l15 -> one
// 8-byte store per key tile (sixteen 2-byte stores in the [query][key] layout of round 2)
__device__ __forceinline__ void stage_kq(bf16* tile, int kj, int qi, int g, int l15, const f32x4& vals) {
  bf16x4 v4;
#pragma unroll
  for (int reg = 0; reg < 4; ++reg) v4[reg] = f2bf(vals[reg]);
  *reinterpret_cast<bf16x4*>(tile + (kj * 16 + l15) * PPITCH + qi * 16 + 4 * g) = v4;
}

__global__ __launch_bounds__(256) void attn_fwd_mfma_kernel(AttnArgs a, const bf16* __restrict__ qkv,
                                                            const float* __restrict__ logit_scale,
                                                            const float* __restrict__ bias, const float* __restrict__ mask,
                                                            bf16* __restrict__ out, float* __restrict__ lse, int bpw,
                                                            int units) {
  extern __shared__ char smraw[];
  bf16* qs = reinterpret_cast<bf16*>(smraw);   // q, k, v row-major [token][QPITCH]
  bf16* ks = qs + ROWMAJ;
  bf16* vs = ks + ROWMAJ;
  bf16* pt = vs + ROWMAJ;               // P^T [64 keys][PPITCH queries]: a wave owns the 16 columns of its query tile
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  AttnUnit u;
  if (!unit_coords(units, a, u)) return;
  const int h = u.h, win = u.win, bg = u.bg;
  const int N = a.N;
  const int l15 = lane & 15, g = lane >> 4, qi = wv;
  // logits in log2 units: exp(x) = exp2(x log2 e) on v_exp_f32 (one instruction; libm's expf is ~20)
  const float scale = (a.plain ? 0.17677669529663687f : expf(fminf(logit_scale[h], 4.605170185988092f))) * LOG2E;
  float addt[4][4];
  load_add_tile(bias, mask, h, win, N, qi, g, l15, addt);
  // rows of the image being staged (wave 0: q, 1: k, 2: v) are requested one image ahead, as in the backward
  const int64_t tok_sp = token_row(a, 0, win, lane < N ? lane : 0);
  const int64_t img_rows = (int64_t)a.H * a.W;
  bf16x8 rnext[4];
  auto request = [&](int b) { request_rows<false>(a, qkv, nullptr, tok_sp + (int64_t)b * img_rows, h, wv, lane < N, rnext); };
  if (bg * bpw < a.B) request(bg * bpw);
  for (int bb = 0; bb < bpw; ++bb) {
    const int b = bg * bpw + bb;
    if (b >= a.B) break;                 // uniform for the workgroup
    const size_t unit = ((size_t)b * a.nW + win) * a.heads + h;
    stage_rows<false>(a, qs, nullptr, wv, lane, rnext);
    if (bb + 1 < bpw && b + 1 < a.B) request(b + 1);
    __syncthreads();
    f32x4 sc[4];
    qk_tiles(qs, ks, qi, g, l15, sc);
    // the logits leave the accumulator file here, in one go: no v_accvgpr_read among the LDS traffic of the softmax below
    // (see the note at the delta reduction of attn_bwd_mfma_kernel; tools/isa_lint.py)
    asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(sc[2]), "+v"(sc[3]));
    float rsum[4], rmax[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = qi * 16 + 4 * g + reg;
      float mx = -INFINITY;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float v = fmaf(sc[kj][reg], scale, addt[reg][kj]);
        sc[kj][reg] = v;
        mx = fmaxf(mx, v);
      }
      mx = row16_max(mx);
      float sum = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float p = (i < N) ? __builtin_amdgcn_exp2f(sc[kj][reg] - mx) : 0.f;
        sc[kj][reg] = p;
        sum += p;
      }
      sum = row16_sum(sum);
      rsum[reg] = sum;
      rmax[reg] = mx;
      // normalised probabilities (v_rcp_f32 once per query row; what the backward recomputes from the log-sum-exp)
      const float rinv = (i < N) ? __builtin_amdgcn_rcpf(sum) : 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) sc[kj][reg] *= rinv;
    }
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) stage_kq(pt, kj, qi, g, l15, sc[kj]);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_wave_barrier();      // the P^T columns of this query tile are produced and consumed by the same wave
    // ---- O^T[dim][query] = V^T P^T: both operands by transpose reads from the row-major tiles (k-slots = keys), and the
    // accumulator puts four consecutive dims of ONE query in a lane: 8-byte global stores, no staging of the output tile ----
    {
      bf16x8 pb[2];
#pragma unroll
      for (int kt = 0; kt < 2; ++kt) pb[kt] = attn_tr_frag(pt, PPITCH, kt, qi * 16, g, l15);
      const int t = qi * 16 + l15;
      bf16* orow = out + token_row(a, b, win, t < N ? t : 0) * a.C + h * HD + 4 * g;
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kt = 0; kt < 2; ++kt)
          o = __builtin_amdgcn_mfma_f32_16x16x32_bf16(attn_tr_frag(vs, QPITCH, kt, dj * 16, g, l15), pb[kt], o, 0, 0, 0);
        bf16x4 o4;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) o4[reg] = f2bf(o[reg]);
        if (t < N) *reinterpret_cast<bf16x4*>(orow + dj * 16) = o4;
      }
    }
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = qi * 16 + 4 * g + reg;
      if (i < N && l15 == 0) lse[unit * N + i] = (rmax[reg] + __builtin_amdgcn_logf(rsum[reg])) * LN2;   // natural-log units
    }
    __syncthreads();                     // before the next image overwrites q / k / v
  }
}

// (Occupancy: 228 registers = two workgroups per CU.  Forcing three or four with __launch_bounds__ spills: 3.85 vs 2.44 ms per
// SwinV2-T step in isolation, tools/ubench/attn_time.py; the forward at six instead of five: no change.)
// Backward: recomputes P from (Qn, Kn, lse); dP = dO V^T on the same accumulator layout, dS = P (dP - delta) in registers.
// Round 3: the three products whose reduction index is a token — dV^T = dO^T P, dKn^T = Qn^T dS, dQn^T = Kn^T dS^T — take
// their operands with ds_read_b64_tr_b16 from the ROW-MAJOR tiles (conv_wgrad.hip's recipe: k-slot (g, e) <-> token
// 32s + (e < 4 ? 4g + e : 16 + 4g + e - 4) for both operands): no transposed copies of Qn / Kn / dO (96 scalar LDS stores per
// image), P and dS staged once as [key][query] with 8-byte stores (the accumulator layout holds four consecutive queries of a
// key), and the TRANSPOSED results put four consecutive dims of one token in a lane: 8-byte global stores straight from the
// accumulators, F.normalize's backward with two cross-lane steps.  A workgroup walks `bpw` images of its (window, head) and
// sums d(logits) into ONE [N][N] scratch tile, so the d(bias) scratch is bpw times smaller.
constexpr int BW_ST = 64 * PPITCH;                    // dS^T staging: [key][PPITCH queries]
constexpr int BW_PT = 64 * PPITCH;                    // P^T staging:  [key][PPITCH queries]
constexpr int MFMA_BWD_LDS = (4 * ROWMAJ + BW_ST + BW_PT) * 2 + (2 * 64 + 4) * 4;   // + qinv, kinv, 4 partial sums

__global__ __launch_bounds__(256) void attn_bwd_mfma_kernel(AttnArgs a, const bf16* __restrict__ qkv,
                                                            const bf16* __restrict__ dout,
                                                            const float* __restrict__ logit_scale,
                                                            const float* __restrict__ bias, const float* __restrict__ mask,
                                                            const float* __restrict__ lse, bf16* __restrict__ dqkv,
                                                            float* __restrict__ ds_scratch, float* __restrict__ dscale_part,
                                                            int bpw, int units) {
  extern __shared__ char smraw[];
  bf16* qs = reinterpret_cast<bf16*>(smraw);   // qn, kn, v, dO row-major [token][QPITCH]
  bf16* ks = qs + ROWMAJ;
  bf16* vs = ks + ROWMAJ;
  bf16* gs = vs + ROWMAJ;
  bf16* dst = gs + ROWMAJ;               // dS^T * scale [key][query]
  bf16* pt = dst + BW_ST;                // P^T [key][query]
  float* qinv = reinterpret_cast<float*>(pt + BW_PT);
  float* kinv = qinv + 64;
  float* wsum = kinv + 64;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l15 = lane & 15, g = lane >> 4;
  const int N = a.N;
  AttnUnit u;
  if (!unit_coords(units, a, u)) return;
  const int h = u.h, win = u.win, bg = u.bg;
  const float raw_ls = a.plain ? 0.f : logit_scale[h];
  const float scale = a.plain ? 0.17677669529663687f : expf(fminf(raw_ls, 4.605170185988092f));
  float* dS = ds_scratch ? ds_scratch + (size_t)u.id * N * N : nullptr;
  float dsc = 0.f;
  float dsa[4][4];         // d(logits) of this wave's query tile summed over the images the workgroup walks (-> d(bias))
#pragma unroll
  for (int reg = 0; reg < 4; ++reg)
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) dsa[reg][kj] = 0.f;
  float addt[4][4];
  load_add_tile(bias, mask, h, win, N, wv, g, l15, addt);
  const float scale2 = scale * LOG2E;
  // this lane's row of the image being staged (wave 0: q, 1: k, 2: v, 3: dO) and the log-sum-exp of its four queries are
  // requested one image AHEAD: global latency (and the mid-kernel lse round trip) sit under the previous image's arithmetic
  const int64_t tok_sp = token_row(a, 0, win, lane < N ? lane : 0);        // row inside image 0; + b * H * W per image
  const int64_t img_rows = (int64_t)a.H * a.W;
  bf16x8 rnext[4];
  float lse_next[4];
  auto request = [&](int b) {
    request_rows<true>(a, qkv, dout, tok_sp + (int64_t)b * img_rows, h, wv, lane < N, rnext);
    const size_t ub = ((size_t)b * a.nW + win) * a.heads + h;
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int i = wv * 16 + 4 * g + reg;
      lse_next[reg] = lse[ub * N + (i < N ? i : 0)];
    }
  };
  if (bg * bpw < a.B) request(bg * bpw);
  for (int bb = 0; bb < bpw; ++bb) {
    const int b = bg * bpw + bb;
    if (b >= a.B) break;                 // uniform for the workgroup
    float lsev[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) lsev[reg] = lse_next[reg] * LOG2E;
    stage_rows<true>(a, qs, qinv, wv, lane, rnext);
    if (bb + 1 < bpw && b + 1 < a.B) request(b + 1);
    __syncthreads();
    const int qi = wv;
    f32x4 sc[4], dp[4];
    qk_tiles(qs, ks, qi, g, l15, sc);
    qk_tiles(gs, vs, qi, g, l15, dp);
    // logits and dP leave the accumulator file in one go (no v_accvgpr_read among the ds_bpermute / ds_write below)
    asm volatile("" : "+v"(sc[0]), "+v"(sc[1]), "+v"(sc[2]), "+v"(sc[3]), "+v"(dp[0]), "+v"(dp[1]), "+v"(dp[2]), "+v"(dp[3]));
    // ---- P, dP, dS on the accumulator layout: query i = qi*16 + 4g + reg, key j = kj*16 + l15 ----
    f32x4 pv[4], dsv[4];                 // [kj][reg]
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const float li = lsev[reg];
      float dl = 0.f;
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        // (padding: addt is -inf there and the staged rows / the clamped log-sum-exp are finite, so exp2 gives exactly 0)
        pv[kj][reg] = __builtin_amdgcn_exp2f(fmaf(sc[kj][reg], scale2, addt[reg][kj]) - li);
        dl = fmaf(pv[kj][reg], dp[kj][reg], dl);
      }
      dl = row16_sum(dl);
      // Value barrier (kept with the DPP reduction; it was found with the __shfl_xor butterfly that stood here): the reduced
      // delta is materialised in a register of its own before its consumers.  Without it hipcc (ROCm 7.2) paired the
      // butterfly's last steps with the d(logits) arithmetic and overwrote the address register of two ds_bpermute in flight
      // with a v_accvgpr_read of the next accumulator ("ds_bpermute v152, v20, v144; ds_bpermute v153, v20, v145;
      // v_accvgpr_read_b32 v20, a6"): under load the last quarter-wave (lanes 48-63) of the second permute then read a stale
      // index and rows 12..15 of a query tile got delta = 0 for one key tile — a few hundred wrong d(q) / d(k) elements per
      // launch, different ones every run (found by tests/test_fullsize_properties_gpu.py's bit-reproducibility check;
      // tests/test_kernels_gpu.py::test_window_attention_is_bit_reproducible pins it at the kernel level).
      asm volatile("" : "+v"(dl));
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const float ds = pv[kj][reg] * (dp[kj][reg] - dl);
        dsa[reg][kj] += ds;
        dsc = fmaf(ds, sc[kj][reg], dsc);
        dsv[kj][reg] = ds * scale;       // d(qn kn^T) = d(logits) * scale
      }
    }
#pragma unroll
    for (int kj = 0; kj < 4; ++kj) { stage_kq(pt, kj, qi, g, l15, pv[kj]); stage_kq(dst, kj, qi, g, l15, dsv[kj]); }
    __syncthreads();
    // ---- wave mt: dV^T, dKn^T of key tile mt (= dO^T P, Qn^T dS) and dQn^T of query tile mt (= Kn^T dS^T) ----
    {
      const int mt = wv;
      const int t = mt * 16 + l15;        // the token (key for dv / dk, query for dq) of this lane's accumulator column
      f32x4 dv[2], dk[2], dq[2];
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) dv[dj] = dk[dj] = dq[dj] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const bf16x8 pb = attn_row_frag(pt, PPITCH, t, kk, g);                    // P[q][key t], q in k-slot order
        const bf16x8 db = attn_row_frag(dst, PPITCH, t, kk, g);                   // dS[q][key t] * scale
        const bf16x8 dtb = attn_tr_frag(dst, PPITCH, kk, mt * 16, g, l15);        // dS^T[key][query t] * scale, keys in k-slot order
#pragma unroll
        for (int dj = 0; dj < 2; ++dj) {
          const bf16x8 gta = attn_tr_frag(gs, QPITCH, kk, dj * 16, g, l15);       // dO^T[dim][q]
          const bf16x8 qta = attn_tr_frag(qs, QPITCH, kk, dj * 16, g, l15);       // Qn^T[dim][q]
          const bf16x8 kta = attn_tr_frag(ks, QPITCH, kk, dj * 16, g, l15);       // Kn^T[dim][key]
          dv[dj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(gta, pb, dv[dj], 0, 0, 0);
          dk[dj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qta, db, dk[dj], 0, 0, 0);
          dq[dj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kta, dtb, dq[dj], 0, 0, 0);
        }
      }
      // accumulator element (dj, reg): dim dj*16 + 4g + reg of token t.  F.normalize backward: d = (dn - n <n, dn>) / |x|
      // (written out here: four dims of a token per lane and 8-byte stores, where the scalar kernels' store_normalize_bwd has a
      // whole row per lane)
      float qn[2][4], kn[2][4], dotq = 0.f, dotk = 0.f;
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const bf16x4 q4 = *reinterpret_cast<const bf16x4*>(qs + t * QPITCH + dj * 16 + 4 * g);
        const bf16x4 k4 = *reinterpret_cast<const bf16x4*>(ks + t * QPITCH + dj * 16 + 4 * g);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
          qn[dj][reg] = bf2f(q4[reg]);
          kn[dj][reg] = bf2f(k4[reg]);
          dotq = fmaf(qn[dj][reg], dq[dj][reg], dotq);
          dotk = fmaf(kn[dj][reg], dk[dj][reg], dotk);
        }
      }
      dotq += __shfl_xor(dotq, 16, 64); dotq += __shfl_xor(dotq, 32, 64);
      dotk += __shfl_xor(dotk, 16, 64); dotk += __shfl_xor(dotk, 32, 64);
      if (t < N) {
        const float qi_ = qinv[t], ki_ = kinv[t];
        bf16* dr = dqkv + token_row(a, b, win, t) * a.ld + h * HD + 4 * g;
#pragma unroll
        for (int dj = 0; dj < 2; ++dj) {
          bf16x4 oq, ok, ov;
#pragma unroll
          for (int reg = 0; reg < 4; ++reg) {
            oq[reg] = f2bf(a.plain ? dq[dj][reg] : (dq[dj][reg] - qn[dj][reg] * dotq) * qi_);
            ok[reg] = f2bf(a.plain ? dk[dj][reg] : (dk[dj][reg] - kn[dj][reg] * dotk) * ki_);
            ov[reg] = f2bf(dv[dj][reg]);
          }
          *reinterpret_cast<bf16x4*>(dr + dj * 16) = oq;
          *reinterpret_cast<bf16x4*>(dr + a.C + dj * 16) = ok;
          *reinterpret_cast<bf16x4*>(dr + 2 * a.C + dj * 16) = ov;
        }
      }
    }
    __syncthreads();                     // before the next image overwrites the tiles / the staging
  }
  if (dS != nullptr) {
#pragma unroll
    for (int reg = 0; reg < 4; ++reg)
#pragma unroll
      for (int kj = 0; kj < 4; ++kj) {
        const int i = wv * 16 + 4 * g + reg, j = kj * 16 + l15;
        if (i < N && j < N) dS[(size_t)i * N + j] = dsa[reg][kj];
      }
  }
  dsc = wave_sum(dsc);
  if (lane == 0) wsum[wv] = dsc;
  __syncthreads();
  if (threadIdx.x == 0 && dscale_part != nullptr)
    dscale_part[u.id] = raw_ls < 4.605170185988092f ? (wsum[0] + wsum[1] + wsum[2] + wsum[3]) * scale : 0.f;
}

// backward, phase A (lane = query i): dS row -> scratch dS[(b,w)][h][i][j] (fp32), dq; partial dscale
// phase B (lane = key j): dv_j, dk_j from the columns of P and dS
__global__ __launch_bounds__(64) void attn_bwd_kernel(AttnArgs a, const bf16* __restrict__ qkv,
                                                      const bf16* __restrict__ dout, const float* __restrict__ logit_scale,
                                                      const float* __restrict__ bias, const float* __restrict__ mask,
                                                      const float* __restrict__ lse, bf16* __restrict__ dqkv,
                                                      float* __restrict__ dST, float* __restrict__ dscale_part) {
  extern __shared__ float sm[];
  const int N = a.N;
  float* qn = sm;
  float* kn = qn + N * HD;
  float* v = kn + N * HD;
  float* dO = v + N * HD;
  float* qinv = dO + N * HD;
  float* kinv = qinv + N;
  float* delta = kinv + N;
  float* lrow = delta + N;
  const int h = blockIdx.x % a.heads;
  const int win = (blockIdx.x / a.heads) % a.nW;
  const int b = blockIdx.x / (a.heads * a.nW);
  load_qkv(a, qkv, b, win, h, qn, kn, v, qinv, kinv);
  const float raw = logit_scale[h];
  const float scale = expf(fminf(raw, 4.605170185988092f));
  const float* bh = bias + (size_t)h * N * N;
  const float* mw = mask ? mask + (size_t)win * N * N : nullptr;
  float* dS = dST + (size_t)blockIdx.x * N * N;
  for (int t = threadIdx.x; t < N; t += 64) {
    const bf16* g = dout + token_row(a, b, win, t) * a.C + h * HD;
#pragma unroll
    for (int d = 0; d < HD; d += 8) {
      const bf16x8 g8 = ldg16(g + d);
#pragma unroll
      for (int e = 0; e < 8; ++e) dO[t * HD + d + e] = bf2f(g8[e]);
    }
    lrow[t] = lse[(size_t)blockIdx.x * N + t];
  }
  __syncthreads();
  float dsc = 0.f;
  // ---- phase A ----
  for (int i = threadIdx.x; i < N; i += 64) {
    float q[HD], go[HD], dq[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { q[d] = qn[i * HD + d]; go[d] = dO[i * HD + d]; dq[d] = 0.f; }
    const float li = lrow[i];
    // delta_i = sum_j p_ij dP_ij  (= dO_i . O_i)
    float dl = 0.f;
    for (int j = 0; j < N; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { s = fmaf(q[d], kn[j * HD + d], s); dp = fmaf(go[d], v[j * HD + d], dp); }
      const float p = expf(scalar_logit(s, scale, bh, mw, i * N + j) - li);
      dl = fmaf(p, dp, dl);
    }
    delta[i] = dl;
    for (int j = 0; j < N; ++j) {
      float s = 0.f, dp = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) { s = fmaf(q[d], kn[j * HD + d], s); dp = fmaf(go[d], v[j * HD + d], dp); }
      const float p = expf(scalar_logit(s, scale, bh, mw, i * N + j) - li);
      const float ds = p * (dp - dl);
      dS[(size_t)i * N + j] = ds;
      dsc = fmaf(ds, s, dsc);
#pragma unroll
      for (int d = 0; d < HD; ++d) dq[d] = fmaf(ds * scale, kn[j * HD + d], dq[d]);
    }
    // through F.normalize: dq_raw = (dqn - qn (qn . dqn)) / |q|
    store_normalize_bwd(dqkv + token_row(a, b, win, i) * a.ld + h * HD, dq, q, qinv[i]);
  }
  dsc = wave_sum(dsc);
  // d logit_scale = d scale * scale (zero where the clamp is active)
  if (threadIdx.x == 0) dscale_part[blockIdx.x] = raw < 4.605170185988092f ? dsc * scale : 0.f;
  __syncthreads();
  // ---- phase B ----
  for (int j = threadIdx.x; j < N; j += 64) {
    float k[HD], dk[HD], dv[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) { k[d] = kn[j * HD + d]; dk[d] = 0.f; dv[d] = 0.f; }
    for (int i = 0; i < N; ++i) {
      float s = 0.f;
#pragma unroll
      for (int d = 0; d < HD; ++d) s = fmaf(qn[i * HD + d], k[d], s);
      const float p = expf(scalar_logit(s, scale, bh, mw, i * N + j) - lrow[i]);
      const float ds = dS[(size_t)i * N + j] * scale;
#pragma unroll
      for (int d = 0; d < HD; ++d) {
        dv[d] = fmaf(p, dO[i * HD + d], dv[d]);
        dk[d] = fmaf(ds, qn[i * HD + d], dk[d]);
      }
    }
    bf16* dr = dqkv + token_row(a, b, win, j) * a.ld + h * HD;
    store_normalize_bwd(dr + a.C, dk, k, kinv[j]);
#pragma unroll
    for (int d = 0; d < HD; d += 8) {
      bf16x8 v8;
#pragma unroll
      for (int e = 0; e < 8; ++e) v8[e] = f2bf(dv[d + e]);
      stg16(dr + 2 * a.C + d, v8);
    }
  }
}

// nullptr when the geometry is accepted, otherwise the reason of the refusal (what tok_last_error() reports)
const char* fill_attn(AttnArgs& a, int B, int H, int W, int C, int heads, int ws, int shift, int ld) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws <= 0) return "batch, h, w, heads and ws must be positive";
  if (C != heads * HD) return "c must be heads * 32 (head_dim 32)";
  if (H % ws || W % ws) return "h and w must be multiples of the window";
  if (shift < 0 || shift >= ws) return "shift must be in [0, ws)";
  if (ld < 3 * C) return "ld must be at least 3c";
  if (ld & 7) return "ld must be a multiple of 8";
  a.B = B; a.H = H; a.W = W; a.C = C; a.heads = heads; a.ws = ws; a.shift = shift;
  a.nWx = W / ws; a.nW = (H / ws) * a.nWx; a.N = ws * ws; a.ld = ld; a.plain = 0;
  return nullptr;
}

int attn_bpw(const AttnArgs& a) {     // images per wave on the MFMA path
  const long long units = (long long)a.B * a.nW * a.heads;
  // images a workgroup walks: about 1536 workgroups per launch (three rounds of the backward's 512 resident ones), at most 16
  // images each — the per-workgroup prologue (sixteen bias / mask loads per lane) and the first image's exposed load are paid
  // once per workgroup.  Measured per SwinV2-T step in isolation (tools/ubench/attn_time.py): units / 4096 capped at 8 (rounds
  // 2-3) 1.00 / 2.36 ms forward / backward, / 1536 capped at 16: 0.95 / 1.99 ms; / 1024 cap 8: 0.96 / 2.06; / 8192: 1.15 / 2.84.
  // (constants: tok_window_attn_bwd_rows and the launch agree on this number by construction)
  constexpr int div = 1536, cap = 16;
  long long bpw = units / div;
  bpw = bpw < 1 ? 1 : (bpw > cap ? cap : bpw);
  return (int)(bpw > a.B ? a.B : bpw);
}

}  // namespace

extern "C" int tok_window_attn_fwd(const void* qkv, int batch, int h, int w, int c, int heads, int ws, int shift, int ld,
                                   const float* logit_scale, const float* bias, const float* mask, void* out,
                                   float* lse, void* stream) {
  AttnArgs a;
  TOK_CHECK_ARG(qkv && out && lse, "tok_window_attn_fwd: bad args (null qkv / out / lse)");
  const char* why = fill_attn(a, batch, h, w, c, heads, ws, shift, ld);
  TOK_CHECK_ARG(why == nullptr, "tok_window_attn_fwd: bad args: %s", why);
  TOK_CHECK_ARG((logit_scale == nullptr) == (bias == nullptr), "tok_window_attn_fwd: logit_scale and bias go together");
  a.plain = logit_scale == nullptr;
  TOK_CHECK_ARG(!a.plain || (a.N <= 64 && !mask && shift == 0),
                "tok_window_attn_fwd: the plain mode covers unshifted windows of up to 64 tokens");
  if (a.N <= 64) {
    const int bpw = attn_bpw(a);
    const int groups = tok_cdiv(batch, bpw) * a.nW * heads;
    hipLaunchKernelGGL(attn_fwd_mfma_kernel, dim3(8 * tok_cdiv(groups, 8)), dim3(256), MFMA_FWD_LDS, tok_stream(stream), a,
                       (const bf16*)qkv, logit_scale, bias, mask, (bf16*)out, lse, bpw, groups);
    TOK_CHECK_LAUNCH("tok_window_attn_fwd(mfma)");
    return TOK_OK;
  }
  const size_t smem = (size_t)a.N * HD * 3 * sizeof(float);
  TOK_CHECK_ARG(smem <= 160 * 1024, "tok_window_attn_fwd: window %d too large", ws);
  tok_launch_lds<&attn_fwd_kernel>(160 * 1024, dim3(batch * a.nW * heads), dim3(64), smem, tok_stream(stream), a,
                                   (const bf16*)qkv, logit_scale, bias, mask, (bf16*)out, lse);
  TOK_CHECK_LAUNCH("tok_window_attn_fwd");
  return TOK_OK;
}

extern "C" int tok_window_attn_bwd_rows(int batch, int h, int w, int heads, int ws) {
  AttnArgs a;
  if (fill_attn(a, batch, h, w, heads * HD, heads, ws, 0, 3 * heads * HD) != nullptr) return TOK_ERR_INVALID;
  if (a.N <= 64) return tok_cdiv(batch, attn_bpw(a)) * a.nW;
  return batch * a.nW;
}

extern "C" int tok_window_attn_bwd(const void* qkv, const void* dout, int batch, int h, int w, int c, int heads, int ws,
                                   int shift, int ld, const float* logit_scale, const float* bias, const float* mask,
                                   const float* lse, void* dqkv, float* ds_scratch, float* dscale_part, void* stream) {
  AttnArgs a;
  TOK_CHECK_ARG(qkv && dout && lse && dqkv, "tok_window_attn_bwd: bad args (null qkv / dout / lse / dqkv)");
  const char* why = fill_attn(a, batch, h, w, c, heads, ws, shift, ld);
  TOK_CHECK_ARG(why == nullptr, "tok_window_attn_bwd: bad args: %s", why);
  a.plain = logit_scale == nullptr;
  TOK_CHECK_ARG(a.plain || bias, "tok_window_attn_bwd: logit_scale and bias go together");
  TOK_CHECK_ARG(a.plain || (ds_scratch && dscale_part), "tok_window_attn_bwd: SwinV2 mode needs ds_scratch and dscale_part");
  TOK_CHECK_ARG(!a.plain || (!bias && !mask && shift == 0 && a.N <= 64),
                "tok_window_attn_bwd: the plain mode covers unshifted windows of up to 64 tokens (no bias / mask)");
  if (a.N <= 64) {
    const int bpw = attn_bpw(a);
    const int waves = tok_cdiv(batch, bpw) * a.nW * heads;
    tok_launch_lds<&attn_bwd_mfma_kernel>(160 * 1024, dim3(8 * tok_cdiv(waves, 8)), dim3(256), MFMA_BWD_LDS, tok_stream(stream), a,
                                          (const bf16*)qkv, (const bf16*)dout, logit_scale, bias, mask, lse, (bf16*)dqkv, ds_scratch,
                                          dscale_part, bpw, waves);
    TOK_CHECK_LAUNCH("tok_window_attn_bwd(mfma)");
    return TOK_OK;
  }
  const size_t smem = ((size_t)a.N * HD * 4 + (size_t)a.N * 4) * sizeof(float);
  TOK_CHECK_ARG(smem <= 160 * 1024, "tok_window_attn_bwd: window %d too large", ws);
  tok_launch_lds<&attn_bwd_kernel>(160 * 1024, dim3(batch * a.nW * heads), dim3(64), smem, tok_stream(stream), a,
                                   (const bf16*)qkv, (const bf16*)dout, logit_scale, bias, mask, lse, (bf16*)dqkv, ds_scratch,
                                   dscale_part);
  TOK_CHECK_LAUNCH("tok_window_attn_bwd");
  return TOK_OK;
}
