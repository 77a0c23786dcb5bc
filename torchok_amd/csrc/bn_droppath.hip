// Stochastic depth on the last BatchNorm of a residual block ([timm 0.6.13] DropPath in front of the residual add), NHWC bf16:
//   z = y*scale + shift          (the statistics come from the un-dropped y: BatchNorm itself is unchanged)
//   out = relu(s[i] * z + shortcut),   s[i] = row_scale[row / rows_per_sample]: 0 (sample i dropped) or 1 / keep
// Backward:  dt = dout * relu_mask ;  dshortcut = dt ;  dz = s[i] * dt ;  partial = (sum dz, sum dz * xhat) -> tok_bn_bwd_finalize
//            dy = c1*dz + c2*y + c3: a DROPPED sample still receives c2*y + c3, the batch-statistics terms.
// The three kernels are bn.hip's bn_act_fwd / bn_bwd_reduce / bn_bwd_apply on the row skeleton of row_stream.h with one more
// factor per row: same geometry, block caps, partial-row layout and fold order, so with s == 1 they give the same bits.
// The sample of a row is walked, not divided: a lane's rows are a stride apart (SampleWalk).
#include "row_stream.h"
#include <hip/hip_ext.h>

namespace {

// row / rows_per_sample of the lane's current row, advanced with the row stride: no division inside the row loop
struct SampleWalk {
  int64_t n, r, dn, dr, rps;
  __device__ __forceinline__ SampleWalk(int64_t m0, int64_t step, int64_t rps_) : rps(rps_) {
    n = m0 / rps; r = m0 % rps;
    dn = step / rps; dr = step % rps;
  }
  __device__ __forceinline__ void next() {
    r += dr;
    n += dn;
    if (r >= rps) { r -= rps; ++n; }
  }
};

// dt = dout where the forward's mask bit says out > 0, else 0
__device__ __forceinline__ void masked_dt(const uint8_t* __restrict__ mask, int64_t m, int cg, int cg_total, const bf16x8& g,
                                          float (&dt)[8]) {
  const unsigned bits = mask[(size_t)m * cg_total + cg];
#pragma unroll
  for (int e = 0; e < 8; ++e) dt[e] = ((bits >> e) & 1u) ? bf2f(g[e]) : 0.f;
}

__global__ __launch_bounds__(256) void bn_droppath_fwd_kernel(const bf16* __restrict__ y, const float* __restrict__ scale,
                                                              const float* __restrict__ shift,
                                                              const bf16* __restrict__ shortcut,
                                                              const float* __restrict__ row_scale, int64_t rps,
                                                              bf16* __restrict__ out, uint8_t* __restrict__ mask, int64_t M,
                                                              int C, int cge, int rpb) {
  const int cg_total = C >> 3;
  const RowSpan rows = grid_rows(M, rpb);
  rows_map(rows, C, C, cge, rpb, [&](int cg) TOK_ROW_INLINE {
    float sc[8], sh[8];
    load8f(scale + cg * 8, sc);
    load8f(shift + cg * 8, sh);
    SampleWalk smp(rows.first + threadIdx.x / cge, rows.step, rps);
    return [=](int64_t m, size_t off) TOK_ROW_INLINE mutable {
      const float rs = row_scale[smp.n];
      smp.next();
      const bf16x8 v = ldg16(y + off);
      const bf16x8 s = ldg16(shortcut + off);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaxf(fmaf(rs, fmaf(bf2f(v[e]), sc[e], sh[e]), bf2f(s[e])), 0.f));
      stg16(out + off, o);
      if (mask != nullptr) {   // bit e = (out[e] > 0), the layout of tok_bn_act_fwd
        unsigned bits = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) bits |= (bf2f(o[e]) > 0.f ? 1u : 0u) << e;
        mask[(size_t)m * cg_total + cg] = (uint8_t)bits;
      }
    };
  });
}

// partial[2][gridDim.x][C] = (sum dz, sum dz * xhat), dz = s * dt
__global__ __launch_bounds__(256) void bn_droppath_bwd_reduce_kernel(const bf16* __restrict__ dout, const bf16* __restrict__ y,
                                                                     const uint8_t* __restrict__ mask,
                                                                     const float* __restrict__ row_scale, int64_t rps,
                                                                     const float* __restrict__ mean,
                                                                     const float* __restrict__ rstd, int64_t M, int C, int cge,
                                                                     int rpb, float* __restrict__ partial) {
  const int cg_total = C >> 3;
  const RowSpan rows = grid_rows(M, rpb);
  rows_reduce<2>(rows, C, C, cge, rpb, partial, blockIdx.x, gridDim.x, [&](int cg) TOK_ROW_INLINE {
    float mu[8], rs[8];
    load8f(mean + cg * 8, mu);
    load8f(rstd + cg * 8, rs);
    SampleWalk smp(rows.first + threadIdx.x / cge, rows.step, rps);
    return [=](int64_t m, size_t off, float (&s)[2][8]) TOK_ROW_INLINE mutable {
      const float scl = row_scale[smp.n];
      smp.next();
      const bf16x8 g = ldg16(dout + off);
      const bf16x8 v = ldg16(y + off);
      float dt[8];
      masked_dt(mask, m, cg, cg_total, g, dt);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float dz = __fmul_rn(scl, dt[e]);     // rounded on its own: both sums and the apply pass see the same dz
        s[0][e] += dz;
        s[1][e] = fmaf(dz, (bf2f(v[e]) - mu[e]) * rs[e], s[1][e]);
      }
    };
  });
}

// dy = c1*dz + c2*y + c3 for EVERY row (dz = 0 in a dropped sample); dshortcut (= | +=) dt.
// dout / dshortcut may alias (in-place masking of the incoming gradient): no restrict on them; a lane reads its 16 bytes first.
__global__ __launch_bounds__(256) void bn_droppath_bwd_apply_kernel(const bf16* dout, const bf16* __restrict__ y,
                                                                    const uint8_t* __restrict__ mask,
                                                                    const float* __restrict__ row_scale, int64_t rps,
                                                                    const float* __restrict__ coef, bf16* __restrict__ dy,
                                                                    bf16* dshortcut, int ds_acc, int64_t M, int C, int cge,
                                                                    int rpb) {
  const int cg_total = C >> 3;
  const RowSpan rows = grid_rows(M, rpb);
  rows_map(rows, C, C, cge, rpb, [&](int cg) TOK_ROW_INLINE {
    float c1[8], c2[8], c3[8];
    load8f(coef + cg * 8, c1);
    load8f(coef + C + cg * 8, c2);
    load8f(coef + 2 * C + cg * 8, c3);
    SampleWalk smp(rows.first + threadIdx.x / cge, rows.step, rps);
    return [=](int64_t m, size_t off) TOK_ROW_INLINE mutable {
      const float scl = row_scale[smp.n];
      smp.next();
      const bf16x8 g = ldg16(dout + off);
      const bf16x8 v = ldg16(y + off);
      float dt[8];
      masked_dt(mask, m, cg, cg_total, g, dt);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f2bf(fmaf(c1[e], __fmul_rn(scl, dt[e]), fmaf(c2[e], bf2f(v[e]), c3[e])));
      stg16(dy + off, o);
      if (dshortcut != nullptr) {
        bf16x8 d;
        if (ds_acc) {
          const bf16x8 old = ldg16(dshortcut + off);
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = f2bf(dt[e] + bf2f(old[e]));
        } else {
#pragma unroll
          for (int e = 0; e < 8; ++e) d[e] = f2bf(dt[e]);
        }
        stg16(dshortcut + off, d);
      }
    };
  });
}

}  // namespace

// the sizes every call of the trio refuses
#define DROPPATH_CHECK_SIZES(name)                                                                                            \
  TOK_CHECK_ARG(m > 0 && c > 0 && c % 8 == 0, "%s: m > 0 and c a positive multiple of 8 (m = %lld, c = %d)", name, (long long)m, c); \
  TOK_CHECK_ARG(rows_per_sample > 0 && m % rows_per_sample == 0,                                                              \
                "%s: rows_per_sample = %lld must be positive and divide m = %lld", name, (long long)rows_per_sample, (long long)m)

extern "C" int tok_bn_droppath_fwd(const void* y, const float* scale, const float* shift, const void* shortcut,
                                   const float* row_scale, int64_t rows_per_sample, void* out, uint8_t* mask, int64_t m, int c,
                                   void* stream) {
  TOK_CHECK_ARG(y && scale && shift && shortcut && row_scale && out, "tok_bn_droppath_fwd: null pointer");
  DROPPATH_CHECK_SIZES("tok_bn_droppath_fwd");
  if (tok_dbg_skip(8)) return TOK_OK;
  const Geo g = make_geo(c);
  hipLaunchKernelGGL(bn_droppath_fwd_kernel, dim3(row_blocks(m, g, row_stream_cap())), dim3(256), 0, tok_stream(stream),
                     (const bf16*)y, scale, shift, (const bf16*)shortcut, row_scale, rows_per_sample, (bf16*)out, mask, m, c,
                     g.cge, g.rpb);
  TOK_CHECK_LAUNCH("tok_bn_droppath_fwd");
  return TOK_OK;
}

extern "C" int tok_bn_droppath_bwd_reduce(const void* dout, const void* y, const uint8_t* mask, const float* row_scale,
                                          int64_t rows_per_sample, const float* mean, const float* rstd, int64_t m, int c,
                                          float* partial, void* stream) {
  TOK_CHECK_ARG(dout && y && mask && row_scale && mean && rstd && partial, "tok_bn_droppath_bwd_reduce: null pointer");
  DROPPATH_CHECK_SIZES("tok_bn_droppath_bwd_reduce");
  const Geo g = make_geo(c);
  hipLaunchKernelGGL(bn_droppath_bwd_reduce_kernel, dim3(row_blocks(m, g, kRowReduceCap)), dim3(256), 0, tok_stream(stream),
                     (const bf16*)dout, (const bf16*)y, mask, row_scale, rows_per_sample, mean, rstd, m, c, g.cge, g.rpb,
                     partial);
  TOK_CHECK_LAUNCH("tok_bn_droppath_bwd_reduce");
  return TOK_OK;
}

extern "C" int tok_bn_droppath_bwd_apply(const void* dout, const void* y, const uint8_t* mask, const float* row_scale,
                                         int64_t rows_per_sample, const float* coef, void* dy, void* dshortcut,
                                         int dshortcut_accumulate, int64_t m, int c, void* stream) {
  // an armed completion event belongs to THIS call whatever becomes of it: never left for an unrelated later launch
  hipEvent_t ev = tok_take_launch_event();
  TOK_CHECK_ARG(dout && y && mask && row_scale && coef && dy, "tok_bn_droppath_bwd_apply: null pointer");
  DROPPATH_CHECK_SIZES("tok_bn_droppath_bwd_apply");
  if (tok_dbg_skip(8)) return TOK_OK;
  const Geo g = make_geo(c);
  const dim3 grid(row_blocks(m, g, row_stream_cap()));
  if (ev != nullptr) {
    // the launch carries the event as tok_bn_bwd_apply's does (hipExtLaunchKernelGGL stop event)
    hipExtLaunchKernelGGL(bn_droppath_bwd_apply_kernel, grid, dim3(256), 0, tok_stream(stream), nullptr, ev, 0,
                          (const bf16*)dout, (const bf16*)y, mask, row_scale, rows_per_sample, coef, (bf16*)dy,
                          (bf16*)dshortcut, dshortcut_accumulate, m, c, g.cge, g.rpb);
  } else {
    hipLaunchKernelGGL(bn_droppath_bwd_apply_kernel, grid, dim3(256), 0, tok_stream(stream), (const bf16*)dout, (const bf16*)y,
                       mask, row_scale, rows_per_sample, coef, (bf16*)dy, (bf16*)dshortcut, dshortcut_accumulate, m, c, g.cge,
                       g.rpb);
  }
  TOK_CHECK_LAUNCH("tok_bn_droppath_bwd_apply");
  return TOK_OK;
}
