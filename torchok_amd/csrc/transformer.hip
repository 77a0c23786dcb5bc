// Exact index kernels of the transformer rows: gathers and permutations, no arithmetic on the tokens.
//   relpos bias             BEiT: bias[h][i][j] = table[relative_position_index[i][j]][h] and its ordered transpose
//   cpb bias                SwinV2: 16 * sigmoid(table)[relative_position_index]  (exact gather) and its transpose
//   patch merge             the 2x2 strided gather of PatchMerging (exact permutation) and its inverse
// Deterministic: no atomics.  (LayerNorm, column folds, activations: layernorm.hip; window attention: window_attn.hip.)
#include "tok_common.h"
#include <math.h>

namespace {

// ---------------------------------------------------------------------------------------------------------------
// relative position bias of BEiT ([timm 0.6.13] beit.Attention): bias[h][i][j] = table[index[i][j]][h], table fp32 [T][heads]
__global__ __launch_bounds__(256) void relpos_bias_fwd_kernel(const float* __restrict__ table, const int64_t* __restrict__ index,
                                                              int heads, int n, float* __restrict__ bias, int ldb) {
  const int64_t nn = (int64_t)n * n, total = heads * nn;
  // grid-stride: blocks_for() caps the grid, and 16 heads x 1025^2 (large / 512) is more than the cap covers in one trip
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int h = (int)(i / nn);
    const int64_t ij = i - h * nn;
    bias[((size_t)h * n + ij / n) * ldb + ij % n] = table[index[ij] * heads + h];
  }
}

// dtable[t][h] (=|+=) sum_{(i,j): index == t} dbias[h][i][j]: the ordered transpose of cpb_bias_bwd_kernel with one block per table
// row serving every head, so the index is scanned once per row.  Thread x takes the positions p = x (mod 256) in ascending order
// and keeps one running sum per head in LDS; a wave then folds the 256 sums of a head in a fixed order.
__global__ __launch_bounds__(256) void relpos_bias_bwd_kernel(const float* __restrict__ dbias, int ldb,
                                                              const int64_t* __restrict__ index, int heads, int n,
                                                              float* __restrict__ dtable, int accumulate) {
  extern __shared__ float rp_acc[];      // [heads][256]
  const int t = blockIdx.x, nn = n * n, tid = threadIdx.x;
  for (int h = 0; h < heads; ++h) rp_acc[h * 256 + tid] = 0.f;
  // eight index loads per thread in flight, all unconditional, before any is compared (the one-at-a-time form is a chain of
  // dependent L2 round trips, see cpb_bias_bwd_kernel); only the rare matches read d(bias).  Ascending p per thread as before.
  for (int p0 = tid; p0 < nn; p0 += 256 * 8) {
    int64_t idx[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int p = p0 + 256 * u;
      idx[u] = index[p < nn ? p : nn - 1];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int p = p0 + 256 * u;
      if (p >= nn || idx[u] != t) continue;
      const size_t off = (size_t)(p / n) * ldb + p % n;
      for (int h = 0; h < heads; ++h) rp_acc[h * 256 + tid] += dbias[(size_t)h * n * ldb + off];
    }
  }
  __syncthreads();
  const int lane = tid & 63, wv = tid >> 6;
  for (int h = wv; h < heads; h += 4) {
    const float* a = rp_acc + h * 256;
    const float v = wave_sum((a[lane] + a[lane + 64]) + (a[lane + 128] + a[lane + 192]));
    if (lane == 0) {
      float* o = dtable + (size_t)t * heads + h;
      *o = accumulate ? *o + v : v;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------
// continuous position bias: bias[h][i][j] = 16 * sigmoid(table[index[i][j]][h])
__global__ __launch_bounds__(256) void cpb_bias_fwd_kernel(const bf16* __restrict__ table, int ld,
                                                           const int64_t* __restrict__ index, int heads, int nn,
                                                           float* __restrict__ bias) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= heads * nn) return;
  const int h = i / nn, ij = i - h * nn;
  const float t = bf2f(table[index[ij] * ld + h]);
  bias[i] = 16.f / (1.f + expf(-t));
}

// dtable[t][h] = sum_{(i,j): index == t} dbias[h][i][j] * 16 s (1 - s)     (gather over the index: exact, ordered)
__global__ __launch_bounds__(64) void cpb_bias_bwd_kernel(const float* __restrict__ dbias, const bf16* __restrict__ table,
                                                          int ld, const int64_t* __restrict__ index, int heads, int n,
                                                          int transposed, bf16* __restrict__ dtable) {
  const int t = blockIdx.x;
  const int h = blockIdx.y;
  const int nn = n * n;
  if (h >= heads) {   // padding columns of the cpb_mlp output row: defined zeros for the GEMMs downstream
    if (threadIdx.x == 0) dtable[(size_t)t * ld + h] = f2bf(0.f);
    return;
  }
  // eight positions per lane and iteration, every load unconditional (select afterwards): the branchy one-at-a-time form was a
  // chain of 38 dependent L2 round trips per block (68 us per launch on the SwinV2-T step's main queue); the summation order per
  // lane is unchanged (ascending p), so the result keeps its bits
  float acc = 0.f;
  for (int p0 = threadIdx.x; p0 < nn; p0 += 64 * 8) {
    int64_t idx[8];
    float dv[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int p = p0 + 64 * u;
      const int pc = p < nn ? p : nn - 1;
      // transposed: dbias is stored [h][j][i] (what tok_window_attn_bwd's scratch reduces to)
      const int ij = transposed ? (pc % n) * n + pc / n : pc;
      idx[u] = index[ij];
      dv[u] = dbias[(size_t)h * nn + pc];
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) acc += (p0 + 64 * u < nn && idx[u] == t) ? dv[u] : 0.f;
  }
  acc = wave_sum(acc);
  if (threadIdx.x == 0) {
    const float s = 1.f / (1.f + expf(-bf2f(table[(size_t)t * ld + h])));
    dtable[(size_t)t * ld + h] = f2bf(acc * 16.f * s * (1.f - s));
  }
}

// ---------------------------------------------------------------------------------------------------------------
// PatchMerging gather: out[b][y][x][q*C + c] = in[b][2y + (q & 1)][2x + (q >> 1)][c]   (x0, x1, x2, x3 order)
__global__ __launch_bounds__(256) void patch_merge_kernel(const bf16* __restrict__ src, bf16* __restrict__ dst, int B,
                                                          int H, int W, int C, int inverse) {
  const int cg = C >> 3, H2 = H >> 1, W2 = W >> 1;
  const size_t total = (size_t)B * H2 * W2 * 4 * cg;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int g = (int)(i % cg);
    size_t r = i / cg;
    const int q = (int)(r & 3);
    r >>= 2;
    const int x = (int)(r % W2);
    r /= W2;
    const int y = (int)(r % H2);
    const int b = (int)(r / H2);
    const size_t merged = ((((size_t)b * H2 + y) * W2 + x) * 4 + q) * C + g * 8;
    const size_t plain = (((size_t)b * H + 2 * y + (q & 1)) * W + 2 * x + (q >> 1)) * C + g * 8;
    if (inverse) stg16(dst + plain, ldg16(src + merged));
    else stg16(dst + merged, ldg16(src + plain));
  }
}

inline int blocks_for(size_t total) {
  const size_t b = (total + 255) / 256;
  return (int)(b > 65536 ? 65536 : (b < 1 ? 1 : b));
}

}  // namespace

extern "C" int tok_cpb_bias_fwd(const void* table, int ld, const int64_t* index, int heads, int n_tokens, float* bias,
                                void* stream) {
  TOK_CHECK_ARG(table && index && bias && heads > 0 && n_tokens > 0 && ld >= heads, "tok_cpb_bias_fwd: bad args");
  const int nn = n_tokens * n_tokens;
  hipLaunchKernelGGL(cpb_bias_fwd_kernel, dim3((heads * nn + 255) / 256), dim3(256), 0, tok_stream(stream),
                     (const bf16*)table, ld, index, heads, nn, bias);
  TOK_CHECK_LAUNCH("tok_cpb_bias_fwd");
  return TOK_OK;
}

extern "C" int tok_cpb_bias_bwd(const float* dbias, int transposed, const void* table, int ld, const int64_t* index,
                                int heads, int n_tokens, int table_rows, void* dtable, void* stream) {
  TOK_CHECK_ARG(dbias && table && index && dtable && heads > 0 && n_tokens > 0 && table_rows > 0 && ld >= heads,
                "tok_cpb_bias_bwd: bad args");
  hipLaunchKernelGGL(cpb_bias_bwd_kernel, dim3(table_rows, ld), dim3(64), 0, tok_stream(stream), dbias,
                     (const bf16*)table, ld, index, heads, n_tokens, transposed, (bf16*)dtable);
  TOK_CHECK_LAUNCH("tok_cpb_bias_bwd");
  return TOK_OK;
}

extern "C" int tok_relpos_bias_fwd(const float* table, const int64_t* index, int heads, int n_tokens, float* bias, int ldb,
                                   void* stream) {
  TOK_CHECK_ARG(table && index && bias && heads > 0 && n_tokens > 0 && ldb >= n_tokens, "tok_relpos_bias_fwd: bad args");
  hipLaunchKernelGGL(relpos_bias_fwd_kernel, dim3(blocks_for((size_t)heads * n_tokens * n_tokens)), dim3(256), 0,
                     tok_stream(stream), table, index, heads, n_tokens, bias, ldb);
  TOK_CHECK_LAUNCH("tok_relpos_bias_fwd");
  return TOK_OK;
}

extern "C" int tok_relpos_bias_bwd(const float* dbias, int ldb, const int64_t* index, int heads, int n_tokens, int table_rows,
                                   float* dtable, int accumulate, void* stream) {
  TOK_CHECK_ARG(dbias && index && dtable && heads > 0 && heads <= TOK_RELPOS_MAX_HEADS && n_tokens > 0 && table_rows > 0 &&
                ldb >= n_tokens, "tok_relpos_bias_bwd: bad args (1 ... %d heads)", TOK_RELPOS_MAX_HEADS);
  hipLaunchKernelGGL(relpos_bias_bwd_kernel, dim3(table_rows), dim3(256), (size_t)heads * 256 * sizeof(float),
                     tok_stream(stream), dbias, ldb, index, heads, n_tokens, dtable, accumulate ? 1 : 0);
  TOK_CHECK_LAUNCH("tok_relpos_bias_bwd");
  return TOK_OK;
}

extern "C" int tok_patch_merge(const void* src, void* dst, int batch, int h, int w, int c, int inverse, void* stream) {
  TOK_CHECK_ARG(src && dst && batch > 0 && h > 0 && w > 0 && h % 2 == 0 && w % 2 == 0 && c > 0 && c % 8 == 0,
                "tok_patch_merge: bad args");
  TOK_CHECK_ARG(tok_aligned(src, 16) && tok_aligned(dst, 16), "tok_patch_merge: src / dst must be 16-byte aligned");
  hipLaunchKernelGGL(patch_merge_kernel, dim3(blocks_for((size_t)batch * h * w * (c >> 3))), dim3(256), 0,
                     tok_stream(stream), (const bf16*)src, (bf16*)dst, batch, h, w, c, inverse);
  TOK_CHECK_LAUNCH("tok_patch_merge");
  return TOK_OK;
}
