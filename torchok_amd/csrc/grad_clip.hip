// Gradient clipping over the flat gradient arenas of one optimizer (torch.nn.utils.clip_grad_norm_ / clip_grad_value_,
// the calls Lightning's `clip_gradients` makes between the gradient exchange and optimizer.step()).
//
// Every launch walks a SPAN TABLE (tok_grad_span, include/tok.h): one entry per parameter that has a gradient in this
// step, across all arenas of the optimizer.  Only [0, numel) of each span is read or written: the arena padding between
// parameters and the slots of parameters whose .grad is None (which still hold an older step's values) are never
// touched.  The spans are laid end to end into one element space of `total` elements; block b of a launch takes the
// fixed slice [b * chunk, (b + 1) * chunk) of that space and finds its first span by binary search over the prefix sums.
// The grid depends on `total` alone (grad_clip_grid), so the fp64 partial of every block, and the fixed-order fold of the
// partials in tok_grad_clip_coef, give bit-identical norms from run to run: no float atomics anywhere.
//
// Inside a span, 16-B vectors start at the span's first element (slots start on 256-B boundaries): a block's slice can
// begin or end inside a 4-element group, and those at most 3 + 3 elements per span are handled as scalars, so no vector
// straddles two spans and nothing outside a span is addressed.
#include "tok_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int64_t kMinPerBlock = 8192;       // elements (32 KB) per block before the grid grows
enum { OP_SQNORM = 0, OP_SCALE = 1, OP_CLAMP = 2 };
// the span pointers come out of a table in memory: without the global address space hipcc emits flat loads / stores
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gf32x4;

// 1 .. TOK_GRAD_CLIP_MAX_PARTIALS blocks: enough to fill 256 CUs at four blocks each once the gradients are large
inline int grad_clip_grid(int64_t total) {
  const int64_t b = (total + kMinPerBlock - 1) / kMinPerBlock;
  return (int)(b < 1 ? 1 : (b > TOK_GRAD_CLIP_MAX_PARTIALS ? TOK_GRAD_CLIP_MAX_PARTIALS : b));
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// fixed-order block sum (lanes by xor butterfly, then waves 0..3 in order); the result is valid in thread 0
__device__ __forceinline__ double block_sum_f64(double v) {
  __shared__ double wsum[kThreads / TOK_WAVE];
  v = wave_sum_f64(v);
  if ((threadIdx.x & (TOK_WAVE - 1)) == 0) wsum[threadIdx.x / TOK_WAVE] = v;
  __syncthreads();
  double s = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < kThreads / TOK_WAVE; ++w) s += wsum[w];
  return s;
}

// torch.clamp_(g, -v, v): max with -v, then min with v (v < 0 gives v everywhere, as torch); NaN stays NaN (both compares
// are false), which fminf / fmaxf would not preserve
__device__ __forceinline__ float clamp_nan(float x, float v) {
  x = x < -v ? -v : x;
  return x > v ? v : x;
}

template <int OP>
__device__ __forceinline__ void visit(gfloat* g, double& acc, float f) {
  const float x = *g;
  if (OP == OP_SQNORM) acc = fma((double)x, (double)x, acc);
  else if (OP == OP_SCALE) *g = x * f;
  else *g = clamp_nan(x, f);
}

template <int OP>
__device__ __forceinline__ void visit4(gf32x4* g, double& acc, f32x4 x, float f) {
  if (OP == OP_SQNORM) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = fma((double)x[j], (double)x[j], acc);
  } else if (OP == OP_SCALE) {
    *g = x * f;
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) x[j] = clamp_nan(x[j], f);
    *g = x;
  }
}

// OP_SQNORM: partials[blockIdx.x] = sum of squares of the block's slice (every block writes, an empty slice 0).
// OP_SCALE: g *= *coef, nothing at all when *coef == 1 (the same bits as multiplying by one).  OP_CLAMP: g = clamp(g, -v, v).
template <int OP>
__global__ __launch_bounds__(kThreads) void grad_span_kernel(const tok_grad_span* __restrict__ spans, int n_spans,
                                                             int64_t total, int64_t chunk, double* __restrict__ partials,
                                                             const float* __restrict__ coef, float v) {
  float f = v;
  if (OP == OP_SCALE) {
    f = *coef;
    if (f == 1.0f) return;
  }
  const int t = threadIdx.x;
  const int64_t lo = (int64_t)blockIdx.x * chunk;
  const int64_t hi = lo + chunk < total ? lo + chunk : total;
  double acc = 0.0;
  if (lo < hi) {
    int a = 0, b = n_spans - 1;                 // last span with start <= lo (starts strictly increase: numel >= 1)
    while (a < b) {
      const int m = (a + b + 1) >> 1;
      if (spans[m].start <= lo) a = m;
      else b = m - 1;
    }
    for (int s = a; s < n_spans; ++s) {
      const int64_t st = spans[s].start;
      if (st >= hi) break;
      const int64_t n = spans[s].numel;
      gfloat* __restrict__ g = (gfloat*)spans[s].grad;
      const int64_t i0 = (lo > st ? lo : st) - st;
      const int64_t i1 = (hi < st + n ? hi : st + n) - st;
      int64_t v0 = (i0 + 3) & ~(int64_t)3, v1 = i1 & ~(int64_t)3;
      if (v0 > v1) v0 = v1 = i1;               // the whole piece lies inside one 4-element group: scalars only
      if (i0 + t < v0) visit<OP>(g + i0 + t, acc, f);
      gf32x4* g4 = (gf32x4*)g;
      int64_t k = v0 / 4 + t;
      const int64_t k1 = v1 / 4;
      for (; k + kThreads < k1; k += 2 * kThreads) {   // two 16-B loads in flight per lane
        const f32x4 x0 = g4[k], x1 = g4[k + kThreads];
        visit4<OP>(g4 + k, acc, x0, f);
        visit4<OP>(g4 + k + kThreads, acc, x1, f);
      }
      if (k < k1) visit4<OP>(g4 + k, acc, g4[k], f);
      if (v1 + t < i1) visit<OP>(g + v1 + t, acc, f);
    }
  }
  if (OP == OP_SQNORM) {
    const double sum = block_sum_f64(acc);
    if (t == 0) partials[blockIdx.x] = sum;
  }
}

// one block: fold the partials in a fixed order; total = ||g||_2 and coef = clamp(max_norm / (total + 1e-6), max=1) in fp32,
// as torch.nn.utils.clip_grad_norm_ forms them (NaN propagates through the clamp: NaN > 1 is false)
__global__ __launch_bounds__(kThreads) void grad_clip_coef_kernel(const double* __restrict__ partials, int n_partials,
                                                                  float max_norm, float* __restrict__ total_norm,
                                                                  float* __restrict__ coef) {
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partials; i += kThreads) acc += partials[i];
  const double sum = block_sum_f64(acc);
  if (threadIdx.x == 0) {
    const float tot = (float)sqrt(sum);
    const float c = max_norm / (tot + 1e-6f);
    *total_norm = tot;
    *coef = c > 1.f ? 1.f : c;
  }
}

inline int64_t chunk_of(int64_t total) {
  const int g = grad_clip_grid(total);
  return (total + g - 1) / g;
}

}  // namespace

extern "C" int tok_grad_sqnorm_partial(const tok_grad_span* spans, int n_spans, int64_t total, double* partials,
                                       void* stream) {
  TOK_CHECK_ARG(spans && partials && n_spans > 0 && total > 0, "tok_grad_sqnorm_partial: bad args");
  hipLaunchKernelGGL(grad_span_kernel<OP_SQNORM>, dim3(grad_clip_grid(total)), dim3(kThreads), 0, tok_stream(stream), spans,
                     n_spans, total, chunk_of(total), partials, (const float*)nullptr, 0.f);
  TOK_CHECK_LAUNCH("tok_grad_sqnorm_partial");
  return TOK_OK;
}

extern "C" int tok_grad_clip_coef(const double* partials, int64_t total, float max_norm, float* total_norm, float* coef,
                                  void* stream) {
  TOK_CHECK_ARG(partials && total_norm && coef && total > 0, "tok_grad_clip_coef: bad args");
  hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(kThreads), 0, tok_stream(stream), partials, grad_clip_grid(total),
                     max_norm, total_norm, coef);
  TOK_CHECK_LAUNCH("tok_grad_clip_coef");
  return TOK_OK;
}

extern "C" int tok_grad_scale(const tok_grad_span* spans, int n_spans, int64_t total, const float* coef, void* stream) {
  TOK_CHECK_ARG(spans && coef && n_spans > 0 && total > 0, "tok_grad_scale: bad args");
  hipLaunchKernelGGL(grad_span_kernel<OP_SCALE>, dim3(grad_clip_grid(total)), dim3(kThreads), 0, tok_stream(stream), spans,
                     n_spans, total, chunk_of(total), (double*)nullptr, coef, 0.f);
  TOK_CHECK_LAUNCH("tok_grad_scale");
  return TOK_OK;
}

extern "C" int tok_grad_clamp(const tok_grad_span* spans, int n_spans, int64_t total, float clip_value, void* stream) {
  TOK_CHECK_ARG(spans && n_spans > 0 && total > 0, "tok_grad_clamp: bad args");
  hipLaunchKernelGGL(grad_span_kernel<OP_CLAMP>, dim3(grad_clip_grid(total)), dim3(kThreads), 0, tok_stream(stream), spans,
                     n_spans, total, chunk_of(total), (double*)nullptr, (const float*)nullptr, clip_value);
  TOK_CHECK_LAUNCH("tok_grad_clamp");
  return TOK_OK;
}
