// What the two window-attention files of the SwinV2 row share (window_attn.hip: windows of up to 64 tokens on MFMA and the scalar
// pair above; window_attn_tiled.hip: the 64-token-tile family for the windows the scalar pair cannot hold): the geometry of a
// call, the one index rule of roll(-shift) + window_partition, and the rule that routes a window to the tiled family.
#pragma once
#include "tok_common.h"

namespace {

struct AttnArgs {
  int B, H, W, C, heads, ws, shift, nWx, nW, N, ld;   // ld: row pitch of qkv (>= 3C); head_dim = 32
  int plain;   // 1: softmax(q k^T / sqrt(head_dim)) v — no cosine normalisation, logit scale, bias (DaViT, davit.py:168-207)
};

constexpr int WIN_HEAD_DIM = 32;

__device__ __forceinline__ int64_t token_row(const AttnArgs& a, int b, int win, int t) {
  const int wy = win / a.nWx, wx = win - wy * a.nWx;
  const int iy = t / a.ws, ix = t - iy * a.ws;
  int oy = wy * a.ws + iy + a.shift, ox = wx * a.ws + ix + a.shift;   // roll(-shift): rolled[i] = x[(i + shift) % H]
  oy = oy >= a.H ? oy - a.H : oy;
  ox = ox >= a.W ? ox - a.W : ox;
  return ((int64_t)b * a.H + oy) * a.W + ox;
}

// nullptr when the geometry is accepted, otherwise the reason of the refusal (what tok_last_error() reports)
inline const char* fill_attn(AttnArgs& a, int B, int H, int W, int C, int heads, int ws, int shift, int ld) {
  if (B <= 0 || H <= 0 || W <= 0 || heads <= 0 || ws <= 0) return "batch, h, w, heads and ws must be positive";
  if (C != heads * WIN_HEAD_DIM) return "c must be heads * 32 (head_dim 32)";
  if (H % ws || W % ws) return "h and w must be multiples of the window";
  if (shift < 0 || shift >= ws) return "shift must be in [0, ws)";
  if (ld < 3 * C) return "ld must be at least 3c";
  if (ld & 7) return "ld must be a multiple of 8";
  a.B = B; a.H = H; a.W = W; a.C = C; a.heads = heads; a.ws = ws; a.shift = shift;
  a.nWx = W / ws; a.nW = (H / ws) * a.nWx; a.N = ws * ws; a.ld = ld; a.plain = 0;
  return nullptr;
}

// LDS bytes of the scalar backward (attn_bwd_kernel: q, k, v, dO rows and four per-token floats, all fp32) and the windows it
// cannot hold, which the tiled family serves forward and backward: ws >= 18
inline size_t attn_scalar_bwd_lds(const AttnArgs& a) { return ((size_t)a.N * WIN_HEAD_DIM * 4 + (size_t)a.N * 4) * sizeof(float); }
inline bool attn_tiled(const AttnArgs& a) { return attn_scalar_bwd_lds(a) > 160 * 1024; }

}  // namespace
