// Efficient channel attention and the residual that follows it ([timm 0.6.13] EcaModule as the `se` of a ResNet block):
//   m[n][c] = mean_hw z[n]      a[n][c] = sum_{j<k} w[j] m[n][c + j - k/2]  (zero outside 0..C-1)      g = sigmoid(a)
//   out = relu(z * g + shortcut)
// z / shortcut / out / dout / dz / dshort bf16 [n][hw][ld] (c % 8 == 0, c <= 2048), w fp32 [k] (odd k <= 15), mean / gate fp32 [n][c].
//
// Forward : per-(image, chunk) channel sums of z -> one block per image folds them in chunk order, keeps mean[c] in LDS and reads
//           the k-tap window from there -> out in one pass, the lane's eight gates in registers.
// Backward: dm = dout where the STORED out > 0.  Per-(image, chunk) sums of dm * z (= d(out)/dg) -> one block per image:
//           da = dg g (1 - g) in LDS, dmean[c] = sum_j w[j] da[c - j + k/2], and the image's share of dw[j] = sum_c da[c] m[c + j - k/2]
//           (a lane adds its channels in order, then the wave's butterfly) -> dw[j] folds the images in image order ->
//           dz (=|+=) dm * g + dmean / hw and dshort (=|+=) dm in one pass.
// Every sum folds in a fixed order (no float atomics): bit-reproducible run to run.
#include "row_stream.h"

namespace {

constexpr int kCap = 2048;        // workgroups of the streaming launches
constexpr int kMaxC = 2048;       // channels one image block keeps in LDS
constexpr int kMaxK = 15;         // taps
constexpr int kTapRow = 16;       // floats per image of the dw partials

struct EcaGeo {
  int cge, rpb, chunks;
};

EcaGeo eca_geo(int n, int hw, int c) {
  const Geo rg = make_geo(c);
  EcaGeo g;
  g.cge = rg.cge;
  g.rpb = rg.rpb;
  int want = (hw + 4 * g.rpb - 1) / (4 * g.rpb);        // at least 4 rows per lane
  const int cap = (kCap + n - 1) / n;
  if (want > cap) want = cap;
  g.chunks = want < 1 ? 1 : want;
  return g;
}

// the rows of chunk blockIdx.x of image blockIdx.y
__device__ __forceinline__ RowSpan chunk_rows(int hw, int rpb) {
  const int img = blockIdx.y, chunk = blockIdx.x, chunks = gridDim.x;
  const int len = (hw + chunks - 1) / chunks;
  const int p0 = chunk * len < hw ? chunk * len : hw, p1 = p0 + len < hw ? p0 + len : hw;
  return {(int64_t)img * hw + p0, (int64_t)img * hw + p1, rpb};
}

// part[img][chunk][c] = sum over the chunk's pixels of z (forward), of dm * z (BWD)
template <bool BWD>
__global__ __launch_bounds__(256) void eca_sum_kernel(const bf16* __restrict__ z, const bf16* __restrict__ dout,
                                                      const bf16* __restrict__ out, int hw, int C, int ld, int cge, int rpb,
                                                      float* __restrict__ part) {
  const RowSpan rows = chunk_rows(hw, rpb);
  rows_reduce<1>(rows, C, ld, cge, rpb, part, (size_t)blockIdx.y * gridDim.x + blockIdx.x, 0, [&](int) TOK_ROW_INLINE {
    return [=](int64_t, size_t off, float (&s)[1][8]) TOK_ROW_INLINE {
      const bf16x8 vz = ldg16(z + off);
      if constexpr (BWD) {
        const bf16x8 vg = ldg16(dout + off);
        const bf16x8 vo = ldg16(out + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0][e] = fmaf(bf2f(vo[e]) > 0.f ? bf2f(vg[e]) : 0.f, bf2f(vz[e]), s[0][e]);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) s[0][e] += bf2f(vz[e]);
      }
    };
  });
}

__device__ __forceinline__ float sigmoid_f(float v) { return 1.f / (1.f + __expf(-v)); }

// one block per image: mean (chunks folded in order), gate = sigmoid(the k-tap window of the mean, taps in order)
__global__ __launch_bounds__(256) void eca_fwd_image_kernel(const float* __restrict__ part, int chunks, int hw, int C,
                                                            const float* __restrict__ w, int k, float* __restrict__ mean,
                                                            float* __restrict__ gate) {
  __shared__ float m[kMaxC];
  const int img = blockIdx.x, tid = threadIdx.x;
  const float inv = 1.f / (float)hw;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int q = 0; q < chunks; ++q) a += part[((size_t)img * chunks + q) * C + c];
    m[c] = a * inv;
    mean[(size_t)img * C + c] = a * inv;
  }
  __syncthreads();
  const int half = k >> 1;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int j = 0; j < k; ++j) {
      const int i = c + j - half;
      if (i >= 0 && i < C) a = fmaf(w[j], m[i], a);
    }
    gate[(size_t)img * C + c] = sigmoid_f(a);
  }
}

// out = relu(z * g + shortcut)
__global__ __launch_bounds__(256) void eca_out_kernel(const bf16* __restrict__ z, const bf16* __restrict__ sc,
                                                      const float* __restrict__ gate, int hw, int C, int ld, int cge, int rpb,
                                                      bf16* __restrict__ out) {
  const RowSpan rows = chunk_rows(hw, rpb);
  const float* g_img = gate + (size_t)blockIdx.y * C;
  rows_map(rows, C, ld, cge, rpb, [&](int cg) TOK_ROW_INLINE {
    float g[8];
    load8f(g_img + cg * 8, g);
    return [=](int64_t, size_t off) TOK_ROW_INLINE {
      const bf16x8 vz = ldg16(z + off);
      const bf16x8 vs = ldg16(sc + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaxf(fmaf(bf2f(vz[e]), g[e], bf2f(vs[e])), 0.f));
      stg16(out + off, o);
    };
  });
}

// one block per image: da = dg g (1 - g), dmean = the transposed window of da, dwp[img][j] = sum_c da[c] mean[c + j - k/2]
// (dwp == nullptr: not computed)
__global__ __launch_bounds__(256) void eca_bwd_image_kernel(const float* __restrict__ part, int chunks, int C,
                                                            const float* __restrict__ w, int k, const float* __restrict__ mean,
                                                            const float* __restrict__ gate, float* __restrict__ dmean,
                                                            float* __restrict__ dwp) {
  __shared__ float da[kMaxC];
  __shared__ float m[kMaxC];
  const int img = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int q = 0; q < chunks; ++q) a += part[((size_t)img * chunks + q) * C + c];
    const float g = gate[(size_t)img * C + c];
    da[c] = a * g * (1.f - g);
    m[c] = mean[(size_t)img * C + c];
  }
  __syncthreads();
  const int half = k >> 1;
  for (int c = tid; c < C; c += 256) {
    float a = 0.f;
    for (int j = 0; j < k; ++j) {
      const int i = c - j + half;
      if (i >= 0 && i < C) a = fmaf(w[j], da[i], a);
    }
    dmean[(size_t)img * C + c] = a;
  }
  if (dwp == nullptr) return;
  for (int j = wave; j < k; j += 4) {
    float a = 0.f;
    for (int c = lane; c < C; c += 64) {
      const int i = c + j - half;
      if (i >= 0 && i < C) a = fmaf(da[c], m[i], a);
    }
    a = wave_sum(a);
    if (lane == 0) dwp[(size_t)img * kTapRow + j] = a;
  }
}

// dw[j] (=|+=) sum over the images, in image order: the block stages 256 images' rows in LDS with coalesced loads, then thread j
// adds them in order (a serial walk over global memory pays one load latency per image: 39 us at 256 images)
__global__ __launch_bounds__(256) void eca_dw_fold_kernel(const float* __restrict__ dwp, int N, int k, float* dw, int acc) {
  __shared__ float t[256 * kTapRow];
  const int tid = threadIdx.x;
  float a = 0.f;
  for (int n0 = 0; n0 < N; n0 += 256) {
    const int cnt = N - n0 < 256 ? N - n0 : 256;
    for (int i = tid; i < cnt * kTapRow; i += 256) t[i] = dwp[(size_t)n0 * kTapRow + i];
    __syncthreads();
    if (tid < k)
      for (int i = 0; i < cnt; ++i) a += t[i * kTapRow + tid];
    __syncthreads();
  }
  if (tid < k) dw[tid] = acc ? dw[tid] + a : a;
}

// dz (=|+=) dm * g + dmean / hw,  dshort (=|+=) dm;  either may be NULL (block-uniform)
__global__ __launch_bounds__(256) void eca_dx_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ out,
                                                     const float* __restrict__ gate, const float* __restrict__ dmean, int hw,
                                                     int C, int ld, int cge, int rpb, bf16* dz, int dz_acc, bf16* dshort,
                                                     int dshort_acc) {
  const RowSpan rows = chunk_rows(hw, rpb);
  const float* g_img = gate + (size_t)blockIdx.y * C;
  const float* d_img = dmean + (size_t)blockIdx.y * C;
  const float inv = 1.f / (float)hw;
  rows_map(rows, C, ld, cge, rpb, [&](int cg) TOK_ROW_INLINE {
    float g[8], dm_c[8];
    if (dz != nullptr) {
      load8f(g_img + cg * 8, g);
      load8f(d_img + cg * 8, dm_c);
#pragma unroll
      for (int e = 0; e < 8; ++e) dm_c[e] *= inv;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] = dm_c[e] = 0.f;
    }
    return [=](int64_t, size_t off) TOK_ROW_INLINE {
      const bf16x8 vg = ldg16(dout + off);
      const bf16x8 vo = ldg16(out + off);
      float dm[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) dm[e] = bf2f(vo[e]) > 0.f ? bf2f(vg[e]) : 0.f;
      if (dz != nullptr) {
        const bf16x8 old = dz_acc ? ldg16(dz + off) : zero8();
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(dm[e], g[e], dm_c[e] + bf2f(old[e])));
        stg16(dz + off, o);
      }
      if (dshort != nullptr) {
        const bf16x8 old = dshort_acc ? ldg16(dshort + off) : zero8();
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = f2bf(dm[e] + bf2f(old[e]));
        stg16(dshort + off, o);
      }
    };
  });
}

bool eca_c_ok(int c) { return c > 0 && c % 8 == 0 && c <= kMaxC; }

}  // namespace

extern "C" size_t tok_eca_ws_floats(int n, int hw, int c) {
  if (n <= 0 || n > 65535 || hw <= 0 || !eca_c_ok(c)) return 0;
  const EcaGeo g = eca_geo(n, hw, c);
  return (size_t)n * g.chunks * c + (size_t)n * c + (size_t)n * kTapRow;
}

#define TOK_ECA_CHECK_SIZES(who)                                                                       \
  TOK_CHECK_ARG(n > 0 && n <= 65535 && hw > 0, "%s: bad sizes (1 <= n <= 65535, hw >= 1)", who);       \
  TOK_CHECK_ARG(eca_c_ok(c), "%s: bad channels (c %% 8 == 0, c <= 2048)", who);                        \
  TOK_CHECK_ARG(ld >= c && ld % 8 == 0, "%s: bad pitch (ld >= c, ld %% 8 == 0)", who);                 \
  TOK_CHECK_ARG(k >= 1 && k <= kMaxK && (k & 1), "%s: bad window (k odd, 1 <= k <= 15)", who)

extern "C" int tok_eca_fwd(const void* z, const void* shortcut, int n, int hw, int c, int ld, const float* w, int k, float* mean,
                           float* gate, void* out, float* ws, void* stream) {
  const char* who = "tok_eca_fwd";
  TOK_CHECK_ARG(z && shortcut && w && mean && gate && out && ws, "%s: null pointer", who);
  TOK_ECA_CHECK_SIZES(who);
  const EcaGeo g = eca_geo(n, hw, c);
  hipStream_t st = tok_stream(stream);
  hipLaunchKernelGGL(eca_sum_kernel<false>, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)z, (const bf16*)nullptr,
                     (const bf16*)nullptr, hw, c, ld, g.cge, g.rpb, ws);
  hipLaunchKernelGGL(eca_fwd_image_kernel, dim3(n), dim3(256), 0, st, ws, g.chunks, hw, c, w, k, mean, gate);
  hipLaunchKernelGGL(eca_out_kernel, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)z, (const bf16*)shortcut, gate, hw, c, ld,
                     g.cge, g.rpb, (bf16*)out);
  TOK_CHECK_LAUNCH(who);
  return TOK_OK;
}

extern "C" int tok_eca_bwd(const void* dout, const void* out, const void* z, int n, int hw, int c, int ld, const float* w, int k,
                           const float* mean, const float* gate, float* dw, int dw_accumulate, void* dz, int dz_accumulate,
                           void* dshort, int dshort_accumulate, float* ws, void* stream) {
  const char* who = "tok_eca_bwd";
  TOK_CHECK_ARG(dout && out && z && w && mean && gate && ws, "%s: null pointer", who);
  TOK_ECA_CHECK_SIZES(who);
  const EcaGeo g = eca_geo(n, hw, c);
  hipStream_t st = tok_stream(stream);
  float* part = ws;
  float* dmean = part + (size_t)n * g.chunks * c;
  float* dwp = dmean + (size_t)n * c;
  if (dw != nullptr || dz != nullptr) {      // (dshort alone needs neither the sums nor the per-image math)
    hipLaunchKernelGGL(eca_sum_kernel<true>, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)z, (const bf16*)dout,
                       (const bf16*)out, hw, c, ld, g.cge, g.rpb, part);
    hipLaunchKernelGGL(eca_bwd_image_kernel, dim3(n), dim3(256), 0, st, part, g.chunks, c, w, k, mean, gate, dmean,
                       dw != nullptr ? dwp : (float*)nullptr);
    if (dw != nullptr) hipLaunchKernelGGL(eca_dw_fold_kernel, dim3(1), dim3(256), 0, st, dwp, n, k, dw, dw_accumulate);
  }
  if (dz != nullptr || dshort != nullptr)
    hipLaunchKernelGGL(eca_dx_kernel, dim3(g.chunks, n), dim3(256), 0, st, (const bf16*)dout, (const bf16*)out, gate, dmean, hw,
                       c, ld, g.cge, g.rpb, (bf16*)dz, dz_accumulate, (bf16*)dshort, dshort_accumulate);
  TOK_CHECK_LAUNCH(who);
  return TOK_OK;
}
