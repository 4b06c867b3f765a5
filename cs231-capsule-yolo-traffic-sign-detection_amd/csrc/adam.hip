// torch.optim.Adam step (main.py:72,280) for a whole list of tensors in one launch (gfx950): cy_adam_step, whose rule stands in
// include/capsyolo_hip.h.  table[k] = {param*, grad*, exp_avg*, exp_avg_sq*, numel}; blockmap[b] = {tensor, chunk}.
// Same update order as torch's single-tensor path: m, v, denom = sqrt(v)/sqrt(bc2) + eps,
// p -= (lr/bc1) * m / denom.  HBM-bound: 4 reads + 3 writes of 4 B per element, one more of each with the moving average.
#include "common.h"
#include "multi_tensor.h"

namespace {

// The update of one block-map entry.  CLIP: the gradient is scaled by the clipping coefficient of csrc/gradnorm.hip on its way in
// (p.grad itself stays as it is).  EMA: the moving average of the parameter moves in the same pass, with the p this step has just
// stored (still in a register).  The instantiations without EMA never look at ema_table and compute p with the same expression:
// parameters, exp_avg and exp_avg_sq have the same bits with and without the average.
template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_chunk(const AdamEntry* __restrict__ table, float* const* __restrict__ ema_table,
                                           const int2* __restrict__ blockmap, int chunk, float step_size, float beta1, float beta2,
                                           float eps, float inv_bc2_sqrt, float coef, float one_minus_decay) {
  const int2 bm = blockmap[blockIdx.x];
  const AdamEntry e = table[bm.x];
  float* ema = nullptr;
  if (EMA) ema = ema_table[bm.x];
  long long begin, end;
  chunk_range(bm, chunk, e.n, begin, end);
  for (long long i = begin + threadIdx.x; i < end; i += 256) {
    const float g = CLIP ? coef * e.g[i] : e.g[i];
    const float m = beta1 * e.m[i] + (1.f - beta1) * g;
    const float v = beta2 * e.v[i] + (1.f - beta2) * g * g;
    e.m[i] = m;
    e.v[i] = v;
    const float denom = sqrtf(v) * inv_bc2_sqrt + eps;
    if (EMA) {
      const float p = e.p[i] - step_size * (m / denom);
      e.p[i] = p;
      const float a = ema[i];
      ema[i] = a + one_minus_decay * (p - a);
    } else {
      e.p[i] -= step_size * (m / denom);
    }
  }
}

// DEV: the scalars come from device memory (a captured HIP graph freezes kernel arguments; the step count and a scheduler's learning
// rate change from step to step, so the host refreshes hyper with one small copy in front of every replay, graph_step.py); the
// scalar arguments are then not read.  CLIP: record is one value for the whole launch, so every workgroup takes the same way.
// An instantiation reads only the pointers its template arguments name.
// The scalars are plain kernel arguments on purpose.  `beta1 * m + (1 - beta1) * g` has two products and hipcc contracts ONE of them
// into the FMA; which one it takes follows the form of the surrounding code (as built: beta1 * m without CLIP, (1 - beta1) * g with
// it).  With the scalars in a by-value struct the two host-scalar CLIP instantiations took the other product and exp_avg moved by an
// ulp against the library before this kernel was one template; with plain arguments all eight have the instruction sequence they had.
template <bool DEV, bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void adam_step_kernel(const AdamEntry* __restrict__ table, float* const* __restrict__ ema_table,
                                                        const int2* __restrict__ blockmap, int chunk,
                                                        const float* __restrict__ hyper, const float* __restrict__ record,
                                                        float step_size, float beta1, float beta2, float eps, float inv_bc2_sqrt,
                                                        float one_minus_decay) {
  float coef = 1.f;
  if (CLIP) {
    if (record[2] == 0.f) return;
    coef = record[1];
  }
  if (DEV) {
    beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3];
    step_size = hyper[0] / hyper[4], inv_bc2_sqrt = 1.f / sqrtf(hyper[5]);
    if (EMA) one_minus_decay = hyper[6];
  }
  adam_chunk<CLIP, EMA>(table, ema_table, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, coef, one_minus_decay);
}

// flat[offset_k + i] = scale * tensor_k[i] (pack) or tensor_k[i] = scale * flat[offset_k + i] (unpack) for a whole list
// of tensors in one launch: table[k] = {tensor*, offset into flat, numel}, blockmap as above
__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                         int chunk, float* __restrict__ flat, int unpack, float scale) {
  const int2 bm = blockmap[blockIdx.x];
  const CopyEntry e = table[bm.x];
  long long begin, end;
  chunk_range(bm, chunk, e.n, begin, end);
  for (long long i = begin + threadIdx.x; i < end; i += 256) {
    if (unpack) e.t[i] = scale * flat[e.off + i];
    else flat[e.off + i] = scale * e.t[i];
  }
}

}  // namespace

extern "C" int cy_multi_copy(const void* table, const void* blockmap, int n_blocks, int chunk, float* flat, int unpack,
                             float scale, void* stream) {
  CY_REQUIRE(table && blockmap && flat && n_blocks > 0 && chunk > 0, "cy_multi_copy: bad arguments");
  multi_copy_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const CopyEntry*)table, (const int2*)blockmap, chunk, flat,
                                                               unpack, scale);
  CY_LAUNCH_CHECK("cy_multi_copy");
  return 0;
}

extern "C" int cy_adam_step(const cy_adam_step_t* a, void* stream) {
  CY_REQUIRE(a, "cy_adam_step: the descriptor is null");
  CY_REQUIRE(a->table, "cy_adam_step: table is null");
  CY_REQUIRE(a->blockmap, "cy_adam_step: blockmap is null");
  CY_REQUIRE(a->n_blocks > 0, "cy_adam_step: n_blocks must be positive");
  CY_REQUIRE(a->chunk > 0, "cy_adam_step: chunk must be positive");
  float step_size = 0.f, inv_bc2_sqrt = 0.f;
  if (!a->hyper) {
    // (scalars in device memory cannot be checked here: optim.Adam.step_scalars is their only source)
    CY_REQUIRE(a->bias_corr1 > 0.f, "cy_adam_step: bias_corr1 must be positive");
    CY_REQUIRE(a->bias_corr2 > 0.f, "cy_adam_step: bias_corr2 must be positive");
    // 0 would freeze the average and a value above 1 would make it jump past the parameter
    CY_REQUIRE(!a->ema_table || (a->one_minus_decay > 0.f && a->one_minus_decay <= 1.f),
               "cy_adam_step: one_minus_decay must be in (0, 1]");
    step_size = a->lr / a->bias_corr1;
    inv_bc2_sqrt = 1.f / sqrtf(a->bias_corr2);
  }
  // the three pointers select the instantiation: [hyper][record][ema_table]
  using Kernel = void (*)(const AdamEntry*, float* const*, const int2*, int, const float*, const float*, float, float, float, float,
                          float, float);
  static const Kernel kernels[8] = {
      adam_step_kernel<false, false, false>, adam_step_kernel<false, false, true>, adam_step_kernel<false, true, false>,
      adam_step_kernel<false, true, true>,   adam_step_kernel<true, false, false>, adam_step_kernel<true, false, true>,
      adam_step_kernel<true, true, false>,   adam_step_kernel<true, true, true>};
  const Kernel kernel = kernels[(a->hyper ? 4 : 0) | (a->record ? 2 : 0) | (a->ema_table ? 1 : 0)];
  kernel<<<a->n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)a->table, (float* const*)a->ema_table,
                                                       (const int2*)a->blockmap, a->chunk, a->hyper, a->record, step_size, a->beta1,
                                                       a->beta2, a->eps, inv_bc2_sqrt, a->one_minus_decay);
  CY_LAUNCH_CHECK("cy_adam_step");
  return 0;
}
