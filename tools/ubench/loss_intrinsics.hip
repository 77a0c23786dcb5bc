// Accuracy of the device math functions the loss kernels (torchok_amd/csrc/loss_*.hip) call, against fp64 on the host, over the
// argument ranges those kernels feed them: expf / __expf on v - max in [-104, 0], logf / __logf on a sum of exponentials in
// [1, 1024], log1pf on exp(-|x|) in (0, 1]; expf also on [0, 88], the arguments of the sigmoids 1 / (1 + expf(-z)), and on
// [-1.2e9, -104], where the online softmax of NT-Xent (csrc/metric.hip: un-normalised embeddings, the -1e9 diagonal) sends it.
// Prints one JSON line; tests/loss_ref.py carries the maxima with a 2x margin.
//   hipcc --offload-arch=gfx950 -O3 tools/ubench/loss_intrinsics.hip -o tools/ubench/bin/loss_intrinsics
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

__global__ void eval_kernel(const float* __restrict__ ex, const float* __restrict__ lg, const float* __restrict__ l1,
                            const float* __restrict__ ep, const float* __restrict__ en, int n,
                            float* __restrict__ o_exp, float* __restrict__ o_fexp, float* __restrict__ o_log,
                            float* __restrict__ o_flog, float* __restrict__ o_l1p, float* __restrict__ o_pexp,
                            float* __restrict__ o_nexp) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  o_exp[i] = expf(ex[i]);
  o_fexp[i] = __expf(ex[i]);
  o_log[i] = logf(lg[i]);
  o_flog[i] = __logf(lg[i]);
  o_l1p[i] = log1pf(l1[i]);
  o_pexp[i] = expf(ep[i]);
  o_nexp[i] = expf(en[i]);
}

int main() {
  const int n = 1 << 22;
  const double U32 = ldexp(1.0, -24), FLT_MIN_D = ldexp(1.0, -126);
  std::vector<float> ex(n), lg(n), l1(n), ep(n), en(n);
  for (int i = 0; i < n; ++i) {
    const double f = (double)i / (double)(n - 1);
    // half of the points uniform over the range, half crowded towards the end where the result is largest / the log smallest
    ex[i] = (float)(i & 1 ? -104.0 * f : -8.0 * f * f);
    lg[i] = (float)(i & 1 ? 1.0 + 1023.0 * f : 1.0 + 3.0 * f * f * f);
    l1[i] = (float)exp(i & 1 ? -104.0 * f : -4.0 * f);
    ep[i] = (float)(i & 1 ? 88.0 * f : 8.0 * f * f);
    en[i] = (float)(i & 1 ? -104.0 - 296.0 * f : -104.0 * exp(16.26 * f));      // to -400 evenly, to -1.2e9 geometrically
  }
  float* d[12];
  for (int k = 0; k < 12; ++k) CK(hipMalloc(&d[k], n * sizeof(float)));
  CK(hipMemcpy(d[0], ex.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(d[1], lg.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(d[2], l1.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(d[8], ep.data(), n * sizeof(float), hipMemcpyHostToDevice));
  CK(hipMemcpy(d[10], en.data(), n * sizeof(float), hipMemcpyHostToDevice));
  hipLaunchKernelGGL(eval_kernel, dim3((n + 255) / 256), dim3(256), 0, 0, d[0], d[1], d[2], d[8], d[10], n, d[3], d[4], d[5], d[6], d[7], d[9],
                     d[11]);
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  std::vector<float> o[7];
  for (int k = 0; k < 7; ++k) { o[k].resize(n); CK(hipMemcpy(o[k].data(), d[k < 5 ? 3 + k : k == 5 ? 9 : 11], n * sizeof(float), hipMemcpyDeviceToHost)); }
  // exp: relative error in units of 2^-24 where the result is a normal number, absolute error / 2^-126 below
  // log: |error| / (2^-24 max(1, |log|));  log1p: relative error in units of 2^-24 where the argument is a normal number
  double e_rel[2] = {0, 0}, e_tail[2] = {0, 0}, l_abs[2] = {0, 0}, p_rel = 0, p_tail = 0, e_pos = 0, e_far = 0;
  for (int i = 0; i < n; ++i) {
    const double r = exp((double)ex[i]);
    for (int k = 0; k < 2; ++k) {
      const double err = fabs((double)o[k][i] - r);
      if (r >= FLT_MIN_D) e_rel[k] = fmax(e_rel[k], err / (U32 * r));
      else e_tail[k] = fmax(e_tail[k], err / FLT_MIN_D);
    }
    e_far = fmax(e_far, fabs((double)o[6][i] - exp((double)en[i])) / FLT_MIN_D);      // every true value is below 2^-149
    const double rq = exp((double)ep[i]);
    e_pos = fmax(e_pos, fabs((double)o[5][i] - rq) / (U32 * rq));
    const double rl = log((double)lg[i]);
    for (int k = 0; k < 2; ++k) l_abs[k] = fmax(l_abs[k], fabs((double)o[2 + k][i] - rl) / (U32 * fmax(1.0, rl)));
    const double rp = log1p((double)l1[i]), errp = fabs((double)o[4][i] - rp);
    if ((double)l1[i] >= FLT_MIN_D) p_rel = fmax(p_rel, errp / (U32 * rp));
    else p_tail = fmax(p_tail, errp / FLT_MIN_D);
  }
  printf("{\"points\": %d, \"unit\": \"2^-24\", \"expf_rel\": %.4f, \"expf_tail_over_fltmin\": %.4f, \"fast_expf_rel\": %.4f, "
         "\"fast_expf_tail_over_fltmin\": %.4f, \"logf_abs_over_max1\": %.4f, \"fast_logf_abs_over_max1\": %.4f, "
         "\"log1pf_rel\": %.4f, \"log1pf_tail_over_fltmin\": %.4f, \"expf_positive_rel\": %.4f, "
         "\"expf_far_tail_over_fltmin\": %.4f}\n",
         n, e_rel[0], e_tail[0], e_rel[1], e_tail[1], l_abs[0], l_abs[1], p_rel, p_tail, e_pos, e_far);
  return 0;
}
