// torch.optim.Adam step (main.py:72,280) for a whole list of tensors in one launch (gfx950).
// table[k] = {param*, grad*, exp_avg*, exp_avg_sq*, numel}; blockmap[b] = {tensor, chunk}.
// Same update order as torch's single-tensor path: m, v, denom = sqrt(v)/sqrt(bc2) + eps,
// p -= (lr/bc1) * m / denom.  HBM-bound: 4 reads + 3 writes of 4 B per element.
#include "common.h"

namespace {

struct AdamEntry {
  float* p; const float* g; float* m; float* v; long long n;
};

// The update of one block-map entry.  CLIP: the gradient is scaled by the clipping coefficient of csrc/gradnorm.hip on its way in
// (p.grad itself stays as it is); the instantiation without it is the step as it always was.
// EMA: the exponential moving average of the parameter moves in the same pass, ema += one_minus_decay * (p - ema) with the p this
// step has just stored (still in a register: one more read and one more write of 4 B per element, 36 B against 28 B).  The averages
// come in a table of their own, ema_table[k] = the float* that belongs to table[k]; one_minus_decay = 1 - decay is formed in double on
// the host and rounded once (never 1.f - decay here: 1.f - 0.999f is 1.3e-5 below 0.001).  The instantiations without EMA never
// look at ema_table and compute p with the same expression: they keep their bits.
template <bool CLIP, bool EMA>
__device__ __forceinline__ void adam_chunk(const AdamEntry* __restrict__ table, float* const* __restrict__ ema_table,
                                           const int2* __restrict__ blockmap, int chunk, float step_size, float beta1, float beta2,
                                           float eps, float inv_bc2_sqrt, float coef, float one_minus_decay) {
  const int2 bm = blockmap[blockIdx.x];
  const AdamEntry e = table[bm.x];
  float* ema = nullptr;
  if (EMA) ema = ema_table[bm.x];
  const long long begin = (long long)bm.y * chunk;
  long long end = begin + chunk;
  if (end > e.n) end = e.n;
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

__global__ __launch_bounds__(256) void adam_multi_kernel(const AdamEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                         int chunk, float step_size, float beta1, float beta2, float eps,
                                                         float inv_bc2_sqrt) {
  adam_chunk<false, false>(table, nullptr, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, 1.f, 0.f);
}

// The same step with its scalars read from DEVICE memory: hyper = {lr, beta1, beta2, eps, bias_corr1, bias_corr2}.  A captured HIP
// graph freezes kernel arguments; the step count (bias corrections) and a scheduler's learning rate change from step to step, so
// the host refreshes the six floats with one small copy in front of every replay (graph_step.py).
__global__ __launch_bounds__(256) void adam_multi_dev_kernel(const AdamEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                             int chunk, const float* __restrict__ hyper) {
  const float beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3];
  const float step_size = hyper[0] / hyper[4], inv_bc2_sqrt = 1.f / sqrtf(hyper[5]);
  adam_chunk<false, false>(table, nullptr, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, 1.f, 0.f);
}

// The two steps behind the verdict of cy_grad_clip_finish: record = {total_norm, coef, go, 0} in device memory.  go == 0 (a
// non-finite gradient under the guard) returns before anything is read or written: the record is one value for the whole launch,
// so every workgroup takes the same way.
__global__ __launch_bounds__(256) void adam_multi_clip_kernel(const AdamEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                              int chunk, float step_size, float beta1, float beta2, float eps,
                                                              float inv_bc2_sqrt, const float* __restrict__ record) {
  if (record[2] == 0.f) return;
  adam_chunk<true, false>(table, nullptr, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, record[1], 0.f);
}

__global__ __launch_bounds__(256) void adam_multi_dev_clip_kernel(const AdamEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                                  int chunk, const float* __restrict__ hyper,
                                                                  const float* __restrict__ record) {
  if (record[2] == 0.f) return;
  const float beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3];
  const float step_size = hyper[0] / hyper[4], inv_bc2_sqrt = 1.f / sqrtf(hyper[5]);
  adam_chunk<true, false>(table, nullptr, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, record[1], 0.f);
}

// The four steps with the parameters' moving average (adam_chunk<., true>): the same launches with the table of EMA pointers and
// one_minus_decay next to the other scalars; the _dev ones read it from hyper[6] (hyper has 8 floats here, hyper[7] is 0).  The clip
// variants return on record[2] == 0 before anything is read or written: a skipped step changes no bit of an average either.
__global__ __launch_bounds__(256) void adam_multi_ema_kernel(const AdamEntry* __restrict__ table, float* const* __restrict__ ema_table,
                                                             const int2* __restrict__ blockmap, int chunk, float step_size, float beta1,
                                                             float beta2, float eps, float inv_bc2_sqrt, float one_minus_decay) {
  adam_chunk<false, true>(table, ema_table, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, 1.f, one_minus_decay);
}

__global__ __launch_bounds__(256) void adam_multi_dev_ema_kernel(const AdamEntry* __restrict__ table, float* const* __restrict__ ema_table,
                                                                 const int2* __restrict__ blockmap, int chunk,
                                                                 const float* __restrict__ hyper) {
  const float beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3];
  const float step_size = hyper[0] / hyper[4], inv_bc2_sqrt = 1.f / sqrtf(hyper[5]);
  adam_chunk<false, true>(table, ema_table, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, 1.f, hyper[6]);
}

__global__ __launch_bounds__(256) void adam_multi_clip_ema_kernel(const AdamEntry* __restrict__ table,
                                                                  float* const* __restrict__ ema_table,
                                                                  const int2* __restrict__ blockmap, int chunk, float step_size,
                                                                  float beta1, float beta2, float eps, float inv_bc2_sqrt,
                                                                  float one_minus_decay, const float* __restrict__ record) {
  if (record[2] == 0.f) return;
  adam_chunk<true, true>(table, ema_table, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, record[1], one_minus_decay);
}

__global__ __launch_bounds__(256) void adam_multi_dev_clip_ema_kernel(const AdamEntry* __restrict__ table,
                                                                      float* const* __restrict__ ema_table,
                                                                      const int2* __restrict__ blockmap, int chunk,
                                                                      const float* __restrict__ hyper,
                                                                      const float* __restrict__ record) {
  if (record[2] == 0.f) return;
  const float beta1 = hyper[1], beta2 = hyper[2], eps = hyper[3];
  const float step_size = hyper[0] / hyper[4], inv_bc2_sqrt = 1.f / sqrtf(hyper[5]);
  adam_chunk<true, true>(table, ema_table, blockmap, chunk, step_size, beta1, beta2, eps, inv_bc2_sqrt, record[1], hyper[6]);
}

// flat[offset_k + i] = scale * tensor_k[i] (pack) or tensor_k[i] = scale * flat[offset_k + i] (unpack) for a whole list
// of tensors in one launch: table[k] = {tensor*, offset into flat, numel}, blockmap as above
struct CopyEntry { float* t; long long off; long long n; };
__global__ __launch_bounds__(256) void multi_copy_kernel(const CopyEntry* __restrict__ table, const int2* __restrict__ blockmap,
                                                         int chunk, float* __restrict__ flat, int unpack, float scale) {
  const int2 bm = blockmap[blockIdx.x];
  const CopyEntry e = table[bm.x];
  const long long begin = (long long)bm.y * chunk;
  long long end = begin + chunk;
  if (end > e.n) end = e.n;
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

extern "C" int cy_adam_multi(const void* table, const void* blockmap, int n_blocks, int chunk, float lr, float beta1,
                             float beta2, float eps, float bias_corr1, float bias_corr2, void* stream) {
  CY_REQUIRE(table && blockmap && n_blocks > 0 && chunk > 0, "cy_adam_multi: bad arguments");
  CY_REQUIRE(bias_corr1 > 0.f && bias_corr2 > 0.f, "cy_adam_multi: bias corrections must be positive");
  adam_multi_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (const int2*)blockmap, chunk,
                                                               lr / bias_corr1, beta1, beta2, eps,
                                                               1.f / sqrtf(bias_corr2));
  CY_LAUNCH_CHECK("cy_adam_multi");
  return 0;
}

extern "C" int cy_adam_multi_dev(const void* table, const void* blockmap, int n_blocks, int chunk, const float* hyper, void* stream) {
  CY_REQUIRE(table && blockmap && hyper && n_blocks > 0 && chunk > 0, "cy_adam_multi_dev: bad arguments");
  adam_multi_dev_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (const int2*)blockmap, chunk, hyper);
  CY_LAUNCH_CHECK("cy_adam_multi_dev");
  return 0;
}

extern "C" int cy_adam_multi_clip(const void* table, const void* blockmap, int n_blocks, int chunk, float lr, float beta1,
                                  float beta2, float eps, float bias_corr1, float bias_corr2, const float* record, void* stream) {
  CY_REQUIRE(table && blockmap && record && n_blocks > 0 && chunk > 0, "cy_adam_multi_clip: bad arguments");
  CY_REQUIRE(bias_corr1 > 0.f && bias_corr2 > 0.f, "cy_adam_multi_clip: bias corrections must be positive");
  adam_multi_clip_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (const int2*)blockmap, chunk,
                                                                    lr / bias_corr1, beta1, beta2, eps,
                                                                    1.f / sqrtf(bias_corr2), record);
  CY_LAUNCH_CHECK("cy_adam_multi_clip");
  return 0;
}

extern "C" int cy_adam_multi_dev_clip(const void* table, const void* blockmap, int n_blocks, int chunk, const float* hyper,
                                      const float* record, void* stream) {
  CY_REQUIRE(table && blockmap && hyper && record && n_blocks > 0 && chunk > 0, "cy_adam_multi_dev_clip: bad arguments");
  adam_multi_dev_clip_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (const int2*)blockmap, chunk, hyper,
                                                                        record);
  CY_LAUNCH_CHECK("cy_adam_multi_dev_clip");
  return 0;
}

// one_minus_decay = 1 - decay of a decay in (0, 1), formed in double and rounded once to fp32 by the caller: 0 would freeze the
// average and a value above 1 would make it jump past the parameter.  (The _dev variants read it from device memory and
// cannot check it here: optim.Adam.step_scalars is their only source.)
#define CY_EMA_REQUIRE(name) \
  CY_REQUIRE(ema_table, name ": ema_table is null"); \
  CY_REQUIRE(one_minus_decay > 0.f && one_minus_decay <= 1.f, name ": one_minus_decay must be in (0, 1]")

extern "C" int cy_adam_multi_ema(const void* table, const void* ema_table, const void* blockmap, int n_blocks, int chunk, float lr,
                                 float beta1, float beta2, float eps, float bias_corr1, float bias_corr2, float one_minus_decay,
                                 void* stream) {
  CY_REQUIRE(table && blockmap && n_blocks > 0 && chunk > 0, "cy_adam_multi_ema: bad arguments");
  CY_REQUIRE(bias_corr1 > 0.f && bias_corr2 > 0.f, "cy_adam_multi_ema: bias corrections must be positive");
  CY_EMA_REQUIRE("cy_adam_multi_ema");
  adam_multi_ema_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (float* const*)ema_table,
                                                                   (const int2*)blockmap, chunk, lr / bias_corr1, beta1, beta2, eps,
                                                                   1.f / sqrtf(bias_corr2), one_minus_decay);
  CY_LAUNCH_CHECK("cy_adam_multi_ema");
  return 0;
}

extern "C" int cy_adam_multi_dev_ema(const void* table, const void* ema_table, const void* blockmap, int n_blocks, int chunk,
                                     const float* hyper, void* stream) {
  CY_REQUIRE(table && ema_table && blockmap && hyper && n_blocks > 0 && chunk > 0, "cy_adam_multi_dev_ema: bad arguments");
  adam_multi_dev_ema_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (float* const*)ema_table,
                                                                       (const int2*)blockmap, chunk, hyper);
  CY_LAUNCH_CHECK("cy_adam_multi_dev_ema");
  return 0;
}

extern "C" int cy_adam_multi_clip_ema(const void* table, const void* ema_table, const void* blockmap, int n_blocks, int chunk, float lr,
                                      float beta1, float beta2, float eps, float bias_corr1, float bias_corr2, float one_minus_decay,
                                      const float* record, void* stream) {
  CY_REQUIRE(table && blockmap && record && n_blocks > 0 && chunk > 0, "cy_adam_multi_clip_ema: bad arguments");
  CY_REQUIRE(bias_corr1 > 0.f && bias_corr2 > 0.f, "cy_adam_multi_clip_ema: bias corrections must be positive");
  CY_EMA_REQUIRE("cy_adam_multi_clip_ema");
  adam_multi_clip_ema_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (float* const*)ema_table,
                                                                        (const int2*)blockmap, chunk, lr / bias_corr1, beta1, beta2,
                                                                        eps, 1.f / sqrtf(bias_corr2), one_minus_decay, record);
  CY_LAUNCH_CHECK("cy_adam_multi_clip_ema");
  return 0;
}

extern "C" int cy_adam_multi_dev_clip_ema(const void* table, const void* ema_table, const void* blockmap, int n_blocks, int chunk,
                                          const float* hyper, const float* record, void* stream) {
  CY_REQUIRE(table && ema_table && blockmap && hyper && record && n_blocks > 0 && chunk > 0,
             "cy_adam_multi_dev_clip_ema: bad arguments");
  adam_multi_dev_clip_ema_kernel<<<n_blocks, 256, 0, (hipStream_t)stream>>>((const AdamEntry*)table, (float* const*)ema_table,
                                                                            (const int2*)blockmap, chunk, hyper, record);
  CY_LAUNCH_CHECK("cy_adam_multi_dev_clip_ema");
  return 0;
}
