// Shared device/host helpers for libtok_gfx950.so (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdio.h>
#include <stdarg.h>
#include <math.h>
#include "../../include/tok.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

#define TOK_WAVE 64

// ---- host-side error plumbing -------------------------------------------------------------
void tok_set_error(const char* fmt, ...);

#define TOK_CHECK_ARG(cond, ...)                 \
  do {                                           \
    if (!(cond)) {                               \
      tok_set_error(__VA_ARGS__);                \
      return TOK_ERR_INVALID;                    \
    }                                            \
  } while (0)

#define TOK_CHECK_LAUNCH(name)                                                   \
  do {                                                                           \
    hipError_t e__ = hipGetLastError();                                          \
    if (e__ != hipSuccess) {                                                     \
      tok_set_error("%s: launch failed: %s", name, hipGetErrorString(e__));      \
      return TOK_ERR_LAUNCH;                                                     \
    }                                                                            \
  } while (0)

// TOK_CHECK_LAUNCH for the launch "<who><stage>" of an entry point that issues several: returns the code instead of leaving
static inline int launched(const char* who, const char* stage) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return TOK_OK;
  tok_set_error("%s%s: launch failed: %s", who, stage, hipGetErrorString(e));
  return TOK_ERR_LAUNCH;
}

// the vector loads and stores (ldg16 / stg16, 16-byte buffer accesses, 8-byte pixels) need a base aligned to the access size as well
// as a pitch that is a multiple of it
static inline bool tok_aligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// workgroups of 256 threads for n work items
static inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

static inline hipStream_t tok_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

// TOK_DBG_SKIP=<bitmask>: ablation probe for step-time budgeting (tools/ubench/runs/*): the named launches are NOT issued, results are
// garbage, only the step time means something (an upper bound on what removing / folding that launch class can buy).
//   1 BatchNorm finalizes (forward + backward)   2 wgrad_reduce_flat   4 fused-unit helpers (Gram finalize, prepare rows, Wb) + colsum_f32
//   8 BatchNorm apply passes (bn_act_fwd, bn_bwd_apply)   16 every weight-gradient launch
//   32 BatchNorm apply passes of units without activation (bn.hip)
#include <stdlib.h>
// A process that runs with it set says so once on stderr: the launches it names return TOK_OK without running.
inline int tok_dbg_skip(int bit) {   // (inline, not static: ONE instance and one warning per process)
  static const int v = [] {
    const char* e = getenv("TOK_DBG_SKIP");
    const int m = (int)(e ? atoi(e) : 0);
    if (m != 0)
      fprintf(stderr, "libtok_gfx950: TOK_DBG_SKIP=%d — ablation mode, the named launch classes are NOT issued and every result of "
                      "this process is garbage (timing probe only; unset it for real runs)\n", m);
    return m;
  }();
  return v & bit;
}
static inline int tok_cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
// integer knob from the environment; callers keep it in a function-local static, so it is read once per process
static inline int tok_env_int(const char* name, int dflt) { const char* e = getenv(name); return (int)(e ? atoi(e) : dflt); }

// Launch of a kernel that may need more than 64 KB of dynamic LDS.  Above 64 KB a kernel has to opt in through
// hipFuncAttributeMaxDynamicSharedMemorySize: every instantiation does so at its first launch, once per process (thread-safe
// function-local static).  `max_bytes` is the limit asked for, `bytes` what this launch uses (the same number at most sites).
template <auto Kernel, typename... Args>
void tok_launch_lds(int max_bytes, dim3 grid, dim3 block, size_t bytes, hipStream_t st, const Args&... args) {
  static const bool armed = [&] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, max_bytes);
    return true;
  }();
  (void)armed;
  hipLaunchKernelGGL(Kernel, grid, block, bytes, st, args...);
}

// ---- device helpers -----------------------------------------------------------------------
// behind the parameter list of a lambda handed to a force-inlined skeleton (row_stream.h, resample.h)
#define TOK_ROW_INLINE __attribute__((always_inline))

__device__ __forceinline__ float bf2f(bf16 v) { return (float)v; }
__device__ __forceinline__ bf16 f2bf(float v) { return (bf16)v; }  // RNE (v_cvt_pk_bf16_f32)

__device__ __forceinline__ bf16x8 ldg16(const bf16* p) {
  return *reinterpret_cast<const bf16x8*>(p);
}
__device__ __forceinline__ void stg16(bf16* p, bf16x8 v) { *reinterpret_cast<bf16x8*>(p) = v; }

// erf-GELU and its derivative: one definition for tok_act_fwd/_bwd, the fused GEMM epilogues and the fused MLP, so that all
// paths give the same bits.  GELU(x) = x Phi(x) with the lower tail Phi(-a) = 0.5 erfc(a / sqrt 2) = exp2(P5(a)), a = min(|x|, 5.6):
// a degree-5 polynomial of log2 Phi(-a) (weighted minimax fit, |error in Phi| <= 3e-7 over the whole range; beyond 5.6 the tail is
// < 2e-8) and ONE v_exp_f32, then GELU(x) = max(x, 0) - a Phi(-a) for either sign.  8 VALU + 1 transcendental per element (the
// Abramowitz-Stegun 7.1.26 form of round 3a cost 12 + 2, libm's erff + expf ~55): in the GEMM epilogues and in the fused MLP the
// activation's VALU time is what competes with the MFMA pipe.  All of it is fma / med3, so the two-wide form (v_pk_fma_f32)
// rounds identically.  A NaN input is dropped (med3 / max): a quiet NaN, the only kind arithmetic produces, gives 0; a signalling
// one is clamped to 5.6 by v_med3_f32 and gives what every x < -5.6 gives, -5.6 Phi(-5.6) ~ -5e-8.  The residual stream next to
// every GELU here keeps the NaN.
typedef __attribute__((ext_vector_type(2))) float f32x2;
#define TOK_GELU_C0 (-1.0000008344650269f)
#define TOK_GELU_C1 (-1.1510831117630005f)
#define TOK_GELU_C2 (-0.45927679538726807f)
#define TOK_GELU_C3 (-0.05253789573907852f)
#define TOK_GELU_C4 (0.007387148682028055f)
#define TOK_GELU_C5 (-0.0005188509239815176f)
#define TOK_GELU_AMAX 5.6f
__device__ __forceinline__ float tok_gelu_tail(float a) {   // Phi(-a), 0 <= a <= 5.6
  float q = fmaf(a, TOK_GELU_C5, TOK_GELU_C4);
  q = fmaf(q, a, TOK_GELU_C3);
  q = fmaf(q, a, TOK_GELU_C2);
  q = fmaf(q, a, TOK_GELU_C1);
  q = fmaf(q, a, TOK_GELU_C0);
  return __builtin_amdgcn_exp2f(q);
}
__device__ __forceinline__ float gelu_f(float x) {
  const float a = __builtin_amdgcn_fmed3f(fabsf(x), 0.f, TOK_GELU_AMAX);
  const float m = __builtin_amdgcn_fmed3f(x, 0.f, __builtin_inff());
  return fmaf(-a, tok_gelu_tail(a), m);
}
__device__ __forceinline__ float gelu_d(float x) {           // Phi(x) + x phi(x)
  const float a = __builtin_amdgcn_fmed3f(fabsf(x), 0.f, TOK_GELU_AMAX);
  const float t = tok_gelu_tail(a);
  const float cdf = x >= 0.f ? 1.f - t : t;
  const float pdf = __builtin_amdgcn_exp2f(fmaf(x * x, -0.72134752044448170f, -1.3257480647361593f));
  return fmaf(x, pdf, cdf);
}
// two elements per instruction where the ISA has a packed form
__device__ __forceinline__ f32x2 tok_gelu_tail2(f32x2 a) {
  f32x2 q = __builtin_elementwise_fma(a, (f32x2)(TOK_GELU_C5), (f32x2)(TOK_GELU_C4));
  q = __builtin_elementwise_fma(q, a, (f32x2)(TOK_GELU_C3));
  q = __builtin_elementwise_fma(q, a, (f32x2)(TOK_GELU_C2));
  q = __builtin_elementwise_fma(q, a, (f32x2)(TOK_GELU_C1));
  q = __builtin_elementwise_fma(q, a, (f32x2)(TOK_GELU_C0));
  f32x2 e;
  e.x = __builtin_amdgcn_exp2f(q.x);
  e.y = __builtin_amdgcn_exp2f(q.y);
  return e;
}
__device__ __forceinline__ f32x2 gelu_f2(f32x2 x) {
  f32x2 a, m;
  a.x = __builtin_amdgcn_fmed3f(fabsf(x.x), 0.f, TOK_GELU_AMAX);
  a.y = __builtin_amdgcn_fmed3f(fabsf(x.y), 0.f, TOK_GELU_AMAX);
  m.x = __builtin_amdgcn_fmed3f(x.x, 0.f, __builtin_inff());
  m.y = __builtin_amdgcn_fmed3f(x.y, 0.f, __builtin_inff());
  return __builtin_elementwise_fma(-a, tok_gelu_tail2(a), m);
}

__device__ __forceinline__ f32x2 gelu_d2(f32x2 x) {          // the two-wide gelu_d: same operations, same bits
  f32x2 a;
  a.x = __builtin_amdgcn_fmed3f(fabsf(x.x), 0.f, TOK_GELU_AMAX);
  a.y = __builtin_amdgcn_fmed3f(fabsf(x.y), 0.f, TOK_GELU_AMAX);
  const f32x2 t = tok_gelu_tail2(a);
  f32x2 cdf;
  cdf.x = x.x >= 0.f ? 1.f - t.x : t.x;
  cdf.y = x.y >= 0.f ? 1.f - t.y : t.y;
  const f32x2 e = __builtin_elementwise_fma(x * x, (f32x2)(-0.72134752044448170f), (f32x2)(-1.3257480647361593f));
  f32x2 pdf;
  pdf.x = __builtin_amdgcn_exp2f(e.x);
  pdf.y = __builtin_amdgcn_exp2f(e.y);
  return __builtin_elementwise_fma(x, pdf, cdf);
}

__device__ __forceinline__ bf16x8 zero8() {
  bf16x8 z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = (bf16)0.0f;
  return z;
}

// XCD-aware bijective block remap (guide T1): block b runs on XCD b % 8; give each XCD a
// contiguous range of logical tile ids so neighbouring tiles share that XCD's L2.
__device__ __forceinline__ int tok_xcd_remap(int b, int nwg) {
  const int xcd = b & 7, slot = b >> 3;
  const int q = nwg >> 3, r = nwg & 7;
  const int base = (xcd < r) ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return base + slot;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// Reductions over the 16 lanes of a DPP row (the lanes that share lane >> 4: the 16 keys of an accumulator column block, or 16
// lanes of a LayerNorm row), every lane gets the result: four rotate-and-combine steps on the VALU (row_ror 8 / 4 / 2 / 1).  A
// __shfl_xor butterfly costs five VALU instructions + a ds_bpermute round trip per step, all on the unit's dependent chain.
// (layernorm.hip and window_attn.hip; the order of additions differs from a butterfly's.)
__device__ __forceinline__ float row16_ror(float v, int sel) {
  switch (sel) {
    case 8: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x128, 0xF, 0xF, false));
    case 4: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x124, 0xF, 0xF, false));
    case 2: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x122, 0xF, 0xF, false));
    default: return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x121, 0xF, 0xF, false));
  }
}
__device__ __forceinline__ float row16_sum(float v) {
  v += row16_ror(v, 8); v += row16_ror(v, 4); v += row16_ror(v, 2); v += row16_ror(v, 1);
  return v;
}
__device__ __forceinline__ float row16_max(float v) {
  v = fmaxf(v, row16_ror(v, 8)); v = fmaxf(v, row16_ror(v, 4)); v = fmaxf(v, row16_ror(v, 2)); v = fmaxf(v, row16_ror(v, 1));
  return v;
}
