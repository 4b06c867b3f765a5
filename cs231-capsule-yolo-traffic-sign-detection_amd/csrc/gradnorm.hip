// Global gradient norm for optim.Adam's clipping and non-finite guard (gfx950): a deterministic two-stage reduction over every
// gradient of a step that leaves its verdict in device memory, where the Adam launch reads it (csrc/adam.hip, cy_adam_step's record).
//   stage 1  cy_grad_sumsq_multi: one workgroup per entry of Adam's own block map, partial[b] = sum of g^2 over that chunk
//   stage 2  cy_grad_clip_finish: one workgroup adds the partials and writes record = {total_norm, coef, go, 0}
// The squares are formed and summed in double from the fp32 values: no overflow (an fp32 square is below 2^256), so the sum is
// non-finite exactly when some gradient element is.  Every sum has a fixed order (strided per-thread sums, then a tree through
// LDS) and there are no atomics: two runs on the same gradients give the same bits.  HBM-bound: one read of 4 B per element.
#include "common.h"
#include "multi_tensor.h"

namespace {

// sum over the 256 threads of the workgroup in a fixed tree; the result is valid in thread 0
__device__ __forceinline__ double block_sum_256(double acc, double* red) {
  red[threadIdx.x] = acc;
  __syncthreads();
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}

// Gradients that are views into dp.GradBucket's flat buffer start at any 4-byte offset: 4-byte loads only (a wave reads 256
// contiguous bytes per instruction either way).  Four running sums per thread keep four loads in flight.
__global__ __launch_bounds__(256) void grad_sumsq_multi_kernel(const AdamEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                               int chunk, double* __restrict__ partial) {
  __shared__ double red[256];
  const int2 bm = blockmap[blockIdx.x];
  const AdamEntry e = table[bm.x];
  long long begin, end;
  chunk_range(bm, chunk, e.n, begin, end);
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  long long i = begin + threadIdx.x;
  for (; i + 768 < end; i += 1024) {
    const double g0 = e.g[i], g1 = e.g[i + 256], g2 = e.g[i + 512], g3 = e.g[i + 768];
    a0 += g0 * g0;
    a1 += g1 * g1;
    a2 += g2 * g2;
    a3 += g3 * g3;
  }
  for (; i < end; i += 256) {
    const double g0 = e.g[i];
    a0 += g0 * g0;
  }
  const double total = block_sum_256((a0 + a1) + (a2 + a3), red);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void grad_clip_finish_kernel(const double* __restrict__ partial, int n_partial, float max_norm,
                                                               int guard, float* __restrict__ record,
                                                               long long* __restrict__ skipped) {
  __shared__ double red[256];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n_partial; i += 256) acc += partial[i];
  const double sumsq = block_sum_256(acc, red);
  if (threadIdx.x != 0) return;
  const double total = sqrt(sumsq);
  const bool finite = isfinite(total);
  double coef = 1.0;
  if (max_norm > 0.f) {
    coef = (double)max_norm / (total + 1e-6);        // 1e-6: the constant of torch.nn.utils.clip_grad_norm_
    if (coef > 1.0) coef = 1.0;                      // a NaN stays a NaN, as torch's clamp keeps it (guard off: the formula is followed)
  }
  const bool go = !(guard && !finite);
  record[0] = (float)total;
  record[1] = (float)coef;
  record[2] = go ? 1.f : 0.f;
  record[3] = 0.f;
  if (!go) skipped[0] = skipped[0] + 1;              // one thread of one workgroup, launches ordered by the stream
}

}  // namespace

extern "C" int cy_grad_sumsq_multi(const void* table, const void* blockmap, int n_blocks, int chunk, double* partial, void* stream) {
  CY_REQUIRE(table && blockmap && partial && n_blocks > 0 && chunk > 0, "cy_grad_sumsq_multi: bad arguments");
  grad_sumsq_multi_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (const int2*)blockmap, chunk, partial);
  CY_LAUNCH_CHECK("cy_grad_sumsq_multi");
  return 0;
}

extern "C" int cy_grad_clip_finish(const double* partial, int n_partial, float max_norm, int guard, float* record,
                                   long long* skipped, void* stream) {
  CY_REQUIRE(partial && record && skipped && n_partial > 0, "cy_grad_clip_finish: bad arguments");
  CY_REQUIRE(!(max_norm != max_norm), "cy_grad_clip_finish: max_norm is NaN");
  grad_clip_finish_kernel<<<1, 256, 0, (hipStream_t)stream>>>(partial, n_partial, max_norm, guard, record, skipped);
  CY_LAUNCH_CHECK("cy_grad_clip_finish");
  return 0;
}
