// Squeeze-excite of the MnasNet-A1 and MobileNetV3 blocks ([timm] efficientnet_blocks.SqueezeExcite with ReLU and a sigmoid
// or hard-sigmoid gate):
//   s[n][c] = gate(b2 + W2 relu(b1 + W1 mean_hw(x[n])))      out = x * s   (the product: tok_channel_scale)
//   gate 0: sigmoid(a), s' = s (1 - s);  gate 1: hard sigmoid min(max(a + 3, 0), 6) / 6, s' = 1/6 where 0 < s < 1, else 0
// The gate is a compile-time parameter of the two per-image kernels: the sigmoid instantiation is the MnasNet code.
// So are the activation between the two layers (ReLU, or erf-GELU for [timm 0.6.13] SEModule as GCViT's MbConvBlock builds it) and
// "the layers have biases": tok_se_act_fwd / _bwd reach the new instantiations, the four older entry points launch the
// <gate, ReLU, biases> ones, whose instruction streams are what they were (profiles/gcvit_se_isa.txt).
// x / dout / dx bf16 [n][hw][ld] (c % 8 == 0), W1 fp32 [rd][c] (conv_reduce), W2 fp32 [c][rd] (conv_expand), 1 <= rd <= 256.
//
// Forward : per-(image, chunk) channel sums -> one block per image folds them in chunk order and runs the two 1x1 layers.
// Backward: per-(image, chunk) sums of dout * x (= d(out)/ds) -> one block per image: ds, d(hidden), d(mean) -> the four
//           parameter gradients summed over the images in image order -> dx (=|+=) dout * s + d(mean) / hw in one pass.
// Every sum folds in a fixed order (no float atomics): bit-reproducible run to run.
#include "row_stream.h"

namespace {

constexpr int kCap = 2048;        // workgroups of the streaming launches
constexpr int kMaxC = 2048;       // channels one image block keeps in LDS
constexpr int kMaxRd = 256;

struct SeGeo {
  int cge, rpb, chunks;
};

SeGeo se_geo(int n, int hw, int c) {
  const Geo rg = make_geo(c);
  SeGeo g;
  g.cge = rg.cge;
  g.rpb = rg.rpb;
  int want = (hw + 4 * g.rpb - 1) / (4 * g.rpb);        // at least 4 rows per lane
  const int cap = (kCap + n - 1) / n;
  if (want > cap) want = cap;
  g.chunks = want < 1 ? 1 : want;
  return g;
}

// part[img][chunk][c] = sum over the chunk's pixels of a (* b when b != NULL): a block walks the pixel range of its chunk of
// one image instead of grid-striding over the whole matrix
__global__ __launch_bounds__(256) void se_sum_kernel(const bf16* __restrict__ a, const bf16* __restrict__ b, int hw, int C,
                                                     int ld, int cge, int rpb, float* __restrict__ part) {
  const int img = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int len = (hw + chunks - 1) / chunks;
  const int p0 = chunk * len, p1 = p0 + len < hw ? p0 + len : hw;
  const RowSpan rows = {(int64_t)img * hw + p0, (int64_t)img * hw + p1, rpb};
  rows_reduce<1>(rows, C, ld, cge, rpb, part, (size_t)img * chunks + chunk, 0, [&](int) TOK_ROW_INLINE {
    return [=](int64_t, size_t off, float (&s)[1][8]) TOK_ROW_INLINE {
      const bf16x8 va = ldg16(a + off);
      if (b != nullptr) {
        const bf16x8 vb = ldg16(b + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0][e] = fmaf(bf2f(va[e]), bf2f(vb[e]), s[0][e]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0][e] += bf2f(va[e]);
      }
    };
  });
}

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + __expf(-v)); }
__device__ __forceinline__ float hard_sigmoid_f(float v) { return fminf(fmaxf(v + 3.f, 0.f), 6.f) / 6.f; }

// one block per image: mean, hidden = act(W1 mean + b1), gate = GATE(W2 hidden + b2).  ACT 0: ReLU, `hid` keeps the hidden
// activation.  ACT 1: erf-GELU (gelu_f), `hid` keeps the PRE-activation, which is what the backward differentiates at.
// BIAS false: b1 and b2 are not read (the layers have none).  <GATE, 0, true> is the code the kernel had before ACT and BIAS.
template <int GATE, int ACT, bool BIAS>
__global__ __launch_bounds__(256) void se_fwd_image_kernel(const float* __restrict__ part, int chunks, int hw, int C, int rd,
                                                           const float* __restrict__ w1, const float* __restrict__ b1,
                                                           const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ mean, float* __restrict__ hid,
                                                           float* __restrict__ gate) {
  __shared__ float m[kMaxC];
  __shared__ float h[kMaxRd];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float inv = 1.f / (float)hw;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int k = 0; k < chunks; ++k) a += part[((size_t)img * chunks + k) * C + c];
    m[c] = a * inv;
    mean[(size_t)img * C + c] = a * inv;
  }
  __syncthreads();
  for (int j = wave; j < rd; j += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = fmaf(w1[(size_t)j * C + c], m[c], a);
    a = wave_sum(a);
    if (lane == 0) {
      if constexpr (ACT == 0) {
        const float v = fmaxf(BIAS ? a + b1[j] : a, 0.f);
        h[j] = v;
        hid[(size_t)img * rd + j] = v;
      } else {
        const float pre = BIAS ? a + b1[j] : a;
        h[j] = gelu_f(pre);
        hid[(size_t)img * rd + j] = pre;
      }
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = BIAS ? b2[c] : 0.f;
    for (int j = 0; j < rd; ++j) a = fmaf(w2[(size_t)c * rd + j], h[j], a);
    gate[(size_t)img * C + c] = GATE == 0 ? sigmoid_f(a) : hard_sigmoid_f(a);
  }
}

// one block per image: ds = g s' (s' from the stored gate, see the top), dh = act'(hidden) W2^T ds, dmean = W1^T dh.
// ACT 1: `hid` holds the pre-activation (see the forward), dh = gelu_d(pre) W2^T ds, and the hidden activation gelu_f(pre) that
// the parameter gradients multiply with is written behind dh_out ([2][images][rd]: dh, then the activation).
template <int GATE, int ACT>
__global__ __launch_bounds__(256) void se_bwd_image_kernel(const float* __restrict__ part, int chunks, int C, int rd,
                                                           const float* __restrict__ w1, const float* __restrict__ w2,
                                                           const float* __restrict__ hid, const float* __restrict__ gate,
                                                           float* __restrict__ ds_out, float* __restrict__ dh_out,
                                                           float* __restrict__ dmean) {
  __shared__ float ds[kMaxC];
  __shared__ float dh[kMaxRd];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int k = 0; k < chunks; ++k) a += part[((size_t)img * chunks + k) * C + c];
    const float s = gate[(size_t)img * C + c];
    const float d = GATE == 0 ? a * s * (1.f - s) : ((s > 0.f && s < 1.f) ? a * (1.f / 6.f) : 0.f);
    ds[c] = d;
    ds_out[(size_t)img * C + c] = d;
  }
  __syncthreads();
  for (int j = wave; j < rd; j += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) a = fmaf(w2[(size_t)c * rd + j], ds[c], a);
    a = wave_sum(a);
    if (lane == 0) {
      float v;
      if constexpr (ACT == 0) {
        v = hid[(size_t)img * rd + j] > 0.f ? a : 0.f;
      } else {
        const float pre = hid[(size_t)img * rd + j];
        v = a * gelu_d(pre);
        dh_out[((size_t)gridDim.x + img) * rd + j] = gelu_f(pre);
      }
      dh[j] = v;
      dh_out[(size_t)img * rd + j] = v;
    }
  }
  __syncthreads();
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int j = 0; j < rd; ++j) a = fmaf(w1[(size_t)j * C + c], dh[j], a);
    dmean[(size_t)img * C + c] = a;
  }
}

// the four parameter gradients, each element summed over the images in image order:
//   dw2[c][j] = sum_n ds[n][c] hid[n][j]   db2[c] = sum_n ds[n][c]   dw1[j][c] = sum_n dh[n][j] mean[n][c]   db1[j] = sum_n dh[n][j]
__global__ __launch_bounds__(256) void se_param_grad_kernel(const float* __restrict__ ds, const float* __restrict__ dh,
                                                            const float* __restrict__ hid, const float* __restrict__ mean,
                                                            int N, int C, int rd, float* dw1, float* db1, float* dw2, float* db2,
                                                            int acc) {
  const int n_w = C * rd;
  const int total = 2 * n_w + C + rd;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
    float a = 0.f;
    float* dst;
    int bit;
    if (i < n_w) {                        // dw2 [c][j]
      const int c = i / rd, j = i % rd;
      for (int n = 0; n < N; ++n) a = fmaf(ds[(size_t)n * C + c], hid[(size_t)n * rd + j], a);
      dst = dw2 ? dw2 + i : nullptr;
      bit = 4;
    } else if (i < 2 * n_w) {             // dw1 [j][c]
      const int k = i - n_w, j = k / C, c = k % C;
      for (int n = 0; n < N; ++n) a = fmaf(dh[(size_t)n * rd + j], mean[(size_t)n * C + c], a);
      dst = dw1 ? dw1 + k : nullptr;
      bit = 1;
    } else if (i < 2 * n_w + C) {         // db2 [c]
      const int c = i - 2 * n_w;
      for (int n = 0; n < N; ++n) a += ds[(size_t)n * C + c];
      dst = db2 ? db2 + c : nullptr;
      bit = 8;
    } else {                              // db1 [j]
      const int j = i - 2 * n_w - C;
      for (int n = 0; n < N; ++n) a += dh[(size_t)n * rd + j];
      dst = db1 ? db1 + j : nullptr;
      bit = 2;
    }
    if (dst != nullptr) *dst = (acc & bit) ? *dst + a : a;
  }
}

// dx (=|+=) dout * s[n][c] + dmean[n][c] / hw
__global__ __launch_bounds__(256) void se_dx_kernel(const bf16* __restrict__ dout, const float* __restrict__ gate,
                                                    const float* __restrict__ dmean, int N, int hw, int C, int ld, bf16* dx,
                                                    int accumulate) {
  const int cgs = C >> 3;
  const size_t total = (size_t)N * hw * cgs;
  const float inv = 1.f / (float)hw;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int cg = (int)(i % cgs);
    const size_t row = i / cgs;
    const int img = (int)(row / hw);
    const size_t off = row * ld + cg * 8;
    const bf16x8 g = ldg16(dout + off);
    const bf16x8 old = accumulate ? ldg16(dx + off) : zero8();
    const float* sv = gate + (size_t)img * C + cg * 8;
    const float* mv = dmean + (size_t)img * C + cg * 8;
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(bf2f(g[e]), sv[e], fmaf(mv[e], inv, bf2f(old[e]))));
    stg16(dx + off, o);
  }
}

bool se_args_ok(int n, int hw, int c, int ld, int rd) {
  return n > 0 && n <= 65535 && hw > 0 && c > 0 && c % 8 == 0 && c <= kMaxC && ld >= c && ld % 8 == 0 && rd >= 1 &&
         rd <= kMaxRd;
}

int blocks_for(size_t work) {
  size_t b = (work + 255) / 256;
  return (int)(b < (size_t)kCap ? (b < 1 ? 1 : b) : kCap);
}

}  // namespace

extern "C" size_t tok_se_ws_floats(int n, int hw, int c, int rd) {
  if (!se_args_ok(n, hw, c, c, rd)) return 0;
  const SeGeo g = se_geo(n, hw, c);
  return (size_t)n * g.chunks * c + 2 * (size_t)n * c + (size_t)n * rd;
}

namespace {

template <int ACT, bool BIAS>
int se_fwd_launch(const char* name, int gate_kind, const void* x, int n, int hw, int c, int ld, int rd, const float* w1,
                  const float* b1, const float* w2, const float* b2, float* mean, float* hid, float* gate, float* ws,
                  void* stream) {
  const SeGeo g = se_geo(n, hw, c);
  hipStream_t st = tok_stream(stream);
  hipLaunchKernelGGL(se_sum_kernel, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)x, (const bf16*)nullptr, hw, c, ld, g.cge,
                     g.rpb, ws);
  if (gate_kind == 0)
    hipLaunchKernelGGL((se_fwd_image_kernel<0, ACT, BIAS>), dim3(n), dim3(256), 0, st, ws, g.chunks, hw, c, rd, w1, b1, w2, b2, mean, hid,
                       gate);
  else
    hipLaunchKernelGGL((se_fwd_image_kernel<1, ACT, BIAS>), dim3(n), dim3(256), 0, st, ws, g.chunks, hw, c, rd, w1, b1, w2, b2, mean, hid,
                       gate);
  TOK_CHECK_LAUNCH(name);
  return TOK_OK;
}

template <int ACT>
int se_bwd_launch(const char* name, int gate_kind, const void* dout, const void* x, int n, int hw, int c, int ld, int rd,
                  const float* w1, const float* w2, const float* mean, const float* hid, const float* gate, float* dw1,
                  float* db1, float* dw2, float* db2, int param_accumulate, void* dx, int dx_accumulate, float* ws,
                  void* stream) {
  const SeGeo g = se_geo(n, hw, c);
  hipStream_t st = tok_stream(stream);
  float* part = ws;
  float* ds = part + (size_t)n * g.chunks * c;
  float* dmean = ds + (size_t)n * c;
  float* dh = dmean + (size_t)n * c;
  hipLaunchKernelGGL(se_sum_kernel, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)dout, (const bf16*)x, hw, c, ld, g.cge,
                     g.rpb, part);
  if (gate_kind == 0)
    hipLaunchKernelGGL((se_bwd_image_kernel<0, ACT>), dim3(n), dim3(256), 0, st, part, g.chunks, c, rd, w1, w2, hid, gate, ds, dh,
                       dmean);
  else
    hipLaunchKernelGGL((se_bwd_image_kernel<1, ACT>), dim3(n), dim3(256), 0, st, part, g.chunks, c, rd, w1, w2, hid, gate, ds, dh,
                       dmean);
  if (dw1 || db1 || dw2 || db2)
    hipLaunchKernelGGL(se_param_grad_kernel, dim3(blocks_for(2 * (size_t)c * rd + c + rd)), dim3(256), 0, st, ds, dh,
                       ACT == 0 ? hid : dh + (size_t)n * rd, mean, n, c, rd, dw1, db1, dw2, db2, param_accumulate);
  if (dx != nullptr)
    hipLaunchKernelGGL(se_dx_kernel, dim3(blocks_for((size_t)n * hw * (c >> 3))), dim3(256), 0, st, (const bf16*)dout, gate,
                       dmean, n, hw, c, ld, (bf16*)dx, dx_accumulate);
  TOK_CHECK_LAUNCH(name);
  return TOK_OK;
}

}  // namespace

extern "C" int tok_se_fwd(const void* x, int n, int hw, int c, int ld, int rd, const float* w1, const float* b1, const float* w2,
                          const float* b2, float* mean, float* hid, float* gate, float* ws, void* stream) {
  TOK_CHECK_ARG(x && w1 && b1 && w2 && b2 && mean && hid && gate && ws, "tok_se_fwd: null pointer");
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "tok_se_fwd: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)");
  return se_fwd_launch<0, true>("tok_se_fwd", 0, x, n, hw, c, ld, rd, w1, b1, w2, b2, mean, hid, gate, ws, stream);
}

extern "C" int tok_se_bwd(const void* dout, const void* x, int n, int hw, int c, int ld, int rd, const float* w1,
                          const float* w2, const float* mean, const float* hid, const float* gate, float* dw1, float* db1,
                          float* dw2, float* db2, int param_accumulate, void* dx, int dx_accumulate, float* ws, void* stream) {
  TOK_CHECK_ARG(dout && x && w1 && w2 && mean && hid && gate && ws, "tok_se_bwd: null pointer");
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "tok_se_bwd: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)");
  return se_bwd_launch<0>("tok_se_bwd", 0, dout, x, n, hw, c, ld, rd, w1, w2, mean, hid, gate, dw1, db1, dw2, db2,
                       param_accumulate, dx, dx_accumulate, ws, stream);
}

extern "C" int tok_se_gate_fwd(const void* x, int n, int hw, int c, int ld, int rd, int gate_kind, const float* w1,
                               const float* b1, const float* w2, const float* b2, float* mean, float* hid, float* gate,
                               float* ws, void* stream) {
  TOK_CHECK_ARG(x && w1 && b1 && w2 && b2 && mean && hid && gate && ws, "tok_se_gate_fwd: null pointer");
  TOK_CHECK_ARG(gate_kind == 0 || gate_kind == 1, "tok_se_gate_fwd: gate 0 (sigmoid) or 1 (hard sigmoid)");
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "tok_se_gate_fwd: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)");
  return se_fwd_launch<0, true>("tok_se_gate_fwd", gate_kind, x, n, hw, c, ld, rd, w1, b1, w2, b2, mean, hid, gate, ws, stream);
}

extern "C" int tok_se_gate_bwd(const void* dout, const void* x, int n, int hw, int c, int ld, int rd, int gate_kind,
                               const float* w1, const float* w2, const float* mean, const float* hid, const float* gate,
                               float* dw1, float* db1, float* dw2, float* db2, int param_accumulate, void* dx,
                               int dx_accumulate, float* ws, void* stream) {
  TOK_CHECK_ARG(dout && x && w1 && w2 && mean && hid && gate && ws, "tok_se_gate_bwd: null pointer");
  TOK_CHECK_ARG(gate_kind == 0 || gate_kind == 1, "tok_se_gate_bwd: gate 0 (sigmoid) or 1 (hard sigmoid)");
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "tok_se_gate_bwd: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)");
  return se_bwd_launch<0>("tok_se_gate_bwd", gate_kind, dout, x, n, hw, c, ld, rd, w1, w2, mean, hid, gate, dw1, db1, dw2, db2,
                       param_accumulate, dx, dx_accumulate, ws, stream);
}

// The inner activation and the biases as arguments (GCViT's SEModule: GELU between two bias-free 1x1 layers).
extern "C" size_t tok_se_act_ws_floats(int n, int hw, int c, int rd) {
  const size_t base = tok_se_ws_floats(n, hw, c, rd);
  return base ? base + (size_t)n * rd : 0;
}

extern "C" int tok_se_act_fwd(const void* x, int n, int hw, int c, int ld, int rd, int gate_kind, int act_kind, const float* w1,
                              const float* b1, const float* w2, const float* b2, float* mean, float* hid, float* gate, float* ws,
                              void* stream) {
  const char* who = "tok_se_act_fwd";
  TOK_CHECK_ARG(x && w1 && w2 && mean && hid && gate && ws, "%s: null pointer", who);
  TOK_CHECK_ARG((b1 == nullptr) == (b2 == nullptr), "%s: b1 and b2 are both given or both NULL", who);
  TOK_CHECK_ARG(gate_kind == 0 || gate_kind == 1, "%s: gate 0 (sigmoid) or 1 (hard sigmoid)", who);
  TOK_CHECK_ARG(act_kind == 0 || act_kind == 1, "%s: activation 0 (ReLU) or 1 (GELU)", who);
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "%s: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)", who);
#define TOK_SE_FWD(A, B) se_fwd_launch<A, B>(who, gate_kind, x, n, hw, c, ld, rd, w1, b1, w2, b2, mean, hid, gate, ws, stream)
  if (act_kind == 0) return b1 ? TOK_SE_FWD(0, true) : TOK_SE_FWD(0, false);
  return b1 ? TOK_SE_FWD(1, true) : TOK_SE_FWD(1, false);
#undef TOK_SE_FWD
}

extern "C" int tok_se_act_bwd(const void* dout, const void* x, int n, int hw, int c, int ld, int rd, int gate_kind, int act_kind,
                              const float* w1, const float* w2, const float* mean, const float* hid, const float* gate, float* dw1,
                              float* db1, float* dw2, float* db2, int param_accumulate, void* dx, int dx_accumulate, float* ws,
                              void* stream) {
  const char* who = "tok_se_act_bwd";
  TOK_CHECK_ARG(dout && x && w1 && w2 && mean && hid && gate && ws, "%s: null pointer", who);
  TOK_CHECK_ARG(gate_kind == 0 || gate_kind == 1, "%s: gate 0 (sigmoid) or 1 (hard sigmoid)", who);
  TOK_CHECK_ARG(act_kind == 0 || act_kind == 1, "%s: activation 0 (ReLU) or 1 (GELU)", who);
  TOK_CHECK_ARG(se_args_ok(n, hw, c, ld, rd), "%s: bad sizes (c %% 8 == 0, c <= 2048, 1 <= rd <= 256)", who);
  if (act_kind == 0)
    return se_bwd_launch<0>(who, gate_kind, dout, x, n, hw, c, ld, rd, w1, w2, mean, hid, gate, dw1, db1, dw2, db2,
                            param_accumulate, dx, dx_accumulate, ws, stream);
  return se_bwd_launch<1>(who, gate_kind, dout, x, n, hw, c, ld, rd, w1, w2, mean, hid, gate, dw1, db1, dw2, db2, param_accumulate,
                          dx, dx_accumulate, ws, stream);
}
