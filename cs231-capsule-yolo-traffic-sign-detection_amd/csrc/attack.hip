// The signed-gradient step of FGSM / PGD and the saliency map of an image gradient (include/capsyolo_hip.h: cy_attack_step,
// cy_grad_saliency_u8).  Both are elementwise passes whose every operation is one named fp32 rounding, so that a numpy restatement
// gives the same bits (tests/attack_ref.py); the roundings are spelled with the _rn intrinsics, which the compiler does not contract.
#include <float.h>

#include "common.h"

namespace {

__global__ __launch_bounds__(256) void attack_step_kernel(float* __restrict__ x, const float* __restrict__ x0, const float* __restrict__ g,
                                                          float alpha, float eps, float lo, float hi, long long n) {
  const long long stride = (long long)gridDim.x * blockDim.x;
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const float gv = g[i];
    const float s = (gv > 0.f ? 1.f : 0.f) - (gv < 0.f ? 1.f : 0.f);          // 0 for g == 0 and for NaN
    float t = __fadd_rn(x[i], alpha * s);                                      // alpha * s is exact
    const float c = x0[i];
    t = fminf(fmaxf(t, __fsub_rn(c, eps)), __fadd_rn(c, eps));
    x[i] = fminf(fmaxf(t, lo), hi);
  }
}

constexpr int SAL_T = 256;

// max_c |g| of one pixel: NaN counts as 0, infinity as the largest finite float (the scaling below then stays finite)
__device__ __forceinline__ float sal_pixel(const float* __restrict__ g, long long plane, long long p) {
  float m = 0.f;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a = fabsf(g[c * plane + p]);
    a = a != a ? 0.f : fminf(a, FLT_MAX);
    m = fmaxf(m, a);
  }
  return m;
}

__global__ __launch_bounds__(SAL_T) void grad_saliency_kernel(const float* __restrict__ g, unsigned char* __restrict__ out, long long plane) {
  __shared__ float red[SAL_T / 64];
  const float* const gi = g + (long long)blockIdx.x * 3 * plane;
  unsigned char* const oi = out + (long long)blockIdx.x * plane;
  float mx = 0.f;
  for (long long p = threadIdx.x; p < plane; p += SAL_T) mx = fmaxf(mx, sal_pixel(gi, plane, p));
  mx = wave_allmax(mx);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < SAL_T / 64; ++w) mx = fmaxf(mx, red[w]);
  for (long long p = threadIdx.x; p < plane; p += SAL_T) {
    float q = 0.f;
    if (mx > 0.f) q = __fmul_rn(__fdiv_rn(sal_pixel(gi, plane, p), mx), 255.f);
    oi[p] = (unsigned char)(int)floorf(__fadd_rn(q, 0.5f));                  // q in [0, 255]: to nearest, halves up
  }
}

}  // namespace

extern "C" int cy_attack_step(float* x, const float* x0, const float* g, float alpha, float eps, float lo, float hi, long long n,
                              void* stream) {
  CY_REQUIRE(x && x0 && g && n >= 0, "cy_attack_step: bad arguments");
  CY_REQUIRE(alpha >= 0.f && eps >= 0.f && lo <= hi, "cy_attack_step: alpha=%g eps=%g lo=%g hi=%g (alpha, eps >= 0 and lo <= hi)",
             (double)alpha, (double)eps, (double)lo, (double)hi);
  if (n == 0) return 0;
  long long blocks = cy_ceil_div(n, 256);
  if (blocks > 4096) blocks = 4096;
  attack_step_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, x0, g, alpha, eps, lo, hi, n);
  CY_LAUNCH_CHECK("cy_attack_step");
  return 0;
}

extern "C" int cy_grad_saliency_u8(const float* g, unsigned char* out, int B, int H, int W, void* stream) {
  CY_REQUIRE(g && out && B >= 1 && H >= 1 && W >= 1, "cy_grad_saliency_u8: bad arguments (B=%d H=%d W=%d)", B, H, W);
  grad_saliency_kernel<<<(unsigned)B, SAL_T, 0, (hipStream_t)stream>>>(g, out, (long long)H * W);
  CY_LAUNCH_CHECK("cy_grad_saliency_u8");
  return 0;
}
