// Shared declarations for the gfx950 kernels behind include/capsyolo_hip.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "capsyolo_hip.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

int cy_set_error(int code, const char* fmt, ...);

#define CY_REQUIRE(cond, ...)                                      \
  do {                                                             \
    if (!(cond)) return cy_set_error(CY_EINVAL, __VA_ARGS__);      \
  } while (0)

#define CY_LAUNCH_CHECK(name)                                                          \
  do {                                                                                 \
    hipError_t e__ = hipGetLastError();                                                \
    if (e__ != hipSuccess) return cy_set_error((int)e__, "%s: %s", name, hipGetErrorString(e__)); \
  } while (0)

static inline long long cy_ceil_div(long long a, long long b) { return (a + b - 1) / b; }

// opt a kernel in to more than the default dynamic-LDS limit (gfx950 has 160 KiB per CU)
template <typename K>
static inline int cy_allow_lds(K kernel, size_t bytes) {
  if (bytes <= 48 * 1024) return 0;
  if (bytes > 160 * 1024) return cy_set_error(CY_EINVAL, "kernel needs %zu bytes of LDS (> 160 KiB)", bytes);
  hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e != hipSuccess) return cy_set_error((int)e, "hipFuncSetAttribute(LDS=%zu): %s", bytes, hipGetErrorString(e));
  return 0;
}

// CU count of the current device, or 0 when it cannot be had (no device, no driver: the workspace-size queries run there too).
// What 0 means is the caller's policy: an error, an assumed 256, or no split.  err (optional): the failing call's code.
static inline int cyi_cu_count(hipError_t* err = nullptr) {
  int dev = 0, ncu = 0;
  hipError_t he = hipGetDevice(&dev);
  if (he == hipSuccess) he = hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev);
  if (err) *err = he;
  return he == hipSuccess && ncu > 0 ? ncu : 0;
}
// persistent grid: one block per CU, at most one per tile
static inline int cyi_persistent_blocks(const char* who, long long tiles, long long* blocks) {
  hipError_t he;
  const int ncu = cyi_cu_count(&he);
  if (ncu == 0) return cy_set_error((int)he, "%s: cannot query the CU count: %s", who, hipGetErrorString(he));
  *blocks = tiles < ncu ? tiles : ncu;
  return 0;
}
#ifdef __HIPCC__
// opts the kernel it is about to launch (and no other instantiation) in to `lds` bytes of dynamic LDS, launches it, returns the code
template <typename... P, typename... A>
static inline int cyi_launch_lds(const char* who, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s, const A&... args) {
  if (int rc = cy_allow_lds(kernel, lds)) return rc;
  kernel<<<grid, block, lds, s>>>(args...);
  CY_LAUNCH_CHECK(who);
  return 0;
}
#endif

// A developer knob whose nonzero value compiles kernels that compute wrong results (timing experiments) must not reach a production
// library through a plain -D: each such knob's definition site invokes this, and only a build that says -DCY_DEV_BUILD may set it.
#ifdef CY_DEV_BUILD
#define CY_WRONG_RESULT_KNOB(knob) static_assert(true, "")
#else
#define CY_WRONG_RESULT_KNOB(knob) \
  static_assert((knob) == 0, #knob " is set: its kernels compute wrong results; a build that wants that says -DCY_DEV_BUILD")
#endif

// ---- internal interface of routing_rows.hip (the row-stationary routing pass for C > 1), used by routing.hip
typedef struct {
  const float* u; const float* Wp;                       // Wp: W repacked by cyi_rows_pack_w (the LDS image layout)
  const float* V; const float* ds; float* slab;          // one pass of a phased plan: V_t (null for t = 0), ds^t, partial sums
  float* s_hist; float* v_out;                           // fused forward (s_hist is read by the fused backward)
  const float* dv; float* ds_all; float* V_all;          // fused backward
  float* cdb;                                            // fused backward, optional: c^t and db^t of every (t >= 1, row, i, j) for routing_caps.hip
  int R, N, C, n_iter, it, ic, g, B, fused;
} cyi_rows_args_t;
typedef struct { int slots, nj, wps, waves, rows_per_block, row_blocks, nch, ic, phased; } cyi_rows_plan_t;
void cyi_rows_plan(int R, int N, int C, int Dout, int mode, cyi_rows_plan_t* p);
int cyi_rows_launch(int mode, const cyi_rows_args_t* a, const cyi_rows_plan_t* p, int Dout, hipStream_t s);
long long cyi_rows_wp_floats(int N, int C, int Dout);                  // floats of the packed W image
int cyi_rows_pack_w(const float* W, float* Wp, int N, int C, int Dout, hipStream_t s);

// ---- routing_mfma.hip: the forward pass with u_hat = u W on v_mfma_f32_16x16x4_f32 (row tiles of 16; C <= 48, Dout 16 / 21)
bool cyi_mfma_ok(int C, int Dout);
long long cyi_mfma_wp_floats(int N, int C, int Dout);                  // floats of its packed W image
int cyi_mfma_pack_w(const float* W, float* Wp, int N, int C, int Dout, hipStream_t s);
int cyi_mfma_launch(const cyi_rows_args_t* a, int nch, int Dout, hipStream_t s);   // a->fused: all iterations; else one phased iteration over nch chunks of a->ic

int cyi_caps_bwd_launch(const cy_routing_bwd_t* a, const float* cdb, hipStream_t s);   // routing_caps.hip: du and dW (cdb: saved couplings or NULL)

// ---- the routing plan: everything the host decides about one routing call (routing.hip cyi_routing_plan, pure host arithmetic).
// The launchers of routing.hip and routing_general.hip take their launch numbers and every workspace pointer from it, the
// _ws_floats queries return its `total`, cy_routing_plan exports it.  DESIGN section 4 has the region tables per path.
enum { CYI_ROUTE_C1, CYI_ROUTE_ROWS_FUSED, CYI_ROUTE_ROWS_PHASED, CYI_ROUTE_GENERAL, CYI_ROUTE_MFMA_FUSED, CYI_ROUTE_MFMA_PHASED };
enum { CYI_WS_DS_ALL, CYI_WS_V, CYI_WS_SA, CYI_WS_SLABS, CYI_WS_TAIL, CYI_WS_W, CYI_WS_CDB, CYI_WS_DUH, CYI_WS_DWS, CYI_WS_N };
enum { CYI_RG_MAX_DIN = 16, CYI_RG_MAX_DOUT = 64, CYI_RG_MAX_C = 256 };     // the envelope of the general kernels
typedef struct cyi_routing_plan_t {
  int path;                    // CYI_ROUTE_*
  cyi_rows_plan_t rows;        // rows / mfma paths: the plan of routing_rows.hip
  struct cyi_rg_plan_t {       // general path: the plan of routing_general.hip (filled by cyi_general_plan)
    int DP, CW, Cp, nrb;
    int nch, ic;               // forward / dV passes: chunks of input capsules
    int ich, nich, ipb;        // du_hat pass: input capsules per staged chunk, number of chunks, per block
    int rs, rps;               // dW contraction: row splits, rows per split
    long long plane, wp;       // R*C*DP, floats of the packed W
  } rg;
  int row_blocks, nch, ic;     // what the pass launches use: blocks along the rows (c1: persistent blocks), chunks of input capsules, capsules per chunk
  int cdb;                     // fused rows backward: the row part saves c^t, db^t for routing_caps.hip
  // workspace regions in floats, in the order they lie in (len 0: the call has no such region).  V is the forward's running sum or
  // the backward's V_all; TAIL: the 4 floats routing_caps.hip may read past ds_all / V_all (it reads whole 16-byte pieces).
  int nreg, order[CYI_WS_N];
  long long off[CYI_WS_N], len[CYI_WS_N], total;
} cyi_routing_plan_t;
// appends a region at the end of the workspace (align: on a 16-byte boundary)
static inline void cyi_ws_add(cyi_routing_plan_t* p, int id, long long len, int align) {
  p->off[id] = align ? (p->total + 3) & ~3ll : p->total;
  p->len[id] = len;
  p->order[p->nreg++] = id;
  p->total = p->off[id] + len;
}
static inline float* cyi_ws_at(float* ws, const cyi_routing_plan_t* p, int id) { return p->len[id] ? ws + p->off[id] : nullptr; }
// 0, or CY_EINVAL with the message (prefixed by fn) for a shape no path takes.  force_general: the general kernels also where the specialised ones apply.
int cyi_routing_plan(const char* fn, int R, int N, int C, int Din, int Dout, int n_iter, int g, int B, int backward, int force_general,
                     cyi_routing_plan_t* p);
void cyi_general_plan(int R, int N, int C, int Din, int Dout, int n_iter, int backward, cyi_routing_plan_t* p);   // routing_general.hip: p->rg, launch numbers, regions
int cyi_general_fwd(const cy_routing_fwd_t* a, const cyi_routing_plan_t* p, hipStream_t s);
int cyi_general_bwd(const cy_routing_bwd_t* a, const cyi_routing_plan_t* p, hipStream_t s);

#ifdef __HIPCC__
// offset (in floats) of the 8-vector of input capsule i of capsule row `row`: contiguous rows [R][N][8], or (g != 0)
// the DarkCapsuleNet cell gather (models.py:393-398) read in place from the NHWC feature map [B][4g][4g][256]
__device__ __forceinline__ long long u_offset_g(int row, int i, int N, int g, int B) {
  if (g == 0) return ((long long)row * N + i) * 8;
  const int k = row / B, b = row - k * B;
  const int pos = i >> 5, chg = i & 31;
  const long long pix = (long long)b * 16 * g * g + (long long)(pos >> 2) * 4 * g * g + 4 * k + (pos & 3);
  return pix * 256 + chg * 8;
}
#endif

// wave64 reductions on the DPP cross-lane network (no LDS round trips; __shfl_xor lowers to ds_bpermute_b32,
// ~100 cycles each and serialised by its s_waitcnt): quad swaps, half-row / row mirrors, then row broadcasts
// 15 and 31 leave the total in lane 63, which v_readlane returns to every lane as a scalar.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_get(float fallback, float src) {
  return __int_as_float(
      __builtin_amdgcn_update_dpp(__float_as_int(fallback), __float_as_int(src), CTRL, ROW_MASK, 0xF, false));
}
__device__ __forceinline__ float wave_sum(float v) {
  v += dpp_get<0xB1, 0xF>(0.f, v);     // quad_perm [1,0,3,2]
  v += dpp_get<0x4E, 0xF>(0.f, v);     // quad_perm [2,3,0,1]
  v += dpp_get<0x141, 0xF>(0.f, v);    // row_half_mirror
  v += dpp_get<0x140, 0xF>(0.f, v);    // row_mirror          -> every lane: sum of its 16-lane row
  v += dpp_get<0x142, 0xA>(0.f, v);    // row_bcast:15 into rows 1 and 3
  v += dpp_get<0x143, 0xC>(0.f, v);    // row_bcast:31 into rows 2 and 3 -> lane 63: total
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
// sum over each 16-lane row only (4 DPP steps); every lane of a row ends with its row's sum
__device__ __forceinline__ float row16_sum(float v) {
  v += dpp_get<0xB1, 0xF>(0.f, v);
  v += dpp_get<0x4E, 0xF>(0.f, v);
  v += dpp_get<0x141, 0xF>(0.f, v);
  v += dpp_get<0x140, 0xF>(0.f, v);
  return v;
}
#ifdef __HIPCC__
// all-reduce over the wave with every lane holding the result: 4 DPP steps inside the 16-lane rows, then the two gfx950
// row / half swaps (v_permlane16_swap, v_permlane32_swap) -- no v_readlane, so no VALU -> SALU -> VALU round trip
__device__ __forceinline__ float swap_add16(float v) {
  typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
  const u32x2_ r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float swap_add32(float v) {
  typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
  const u32x2_ r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(r[0]) + __uint_as_float(r[1]);
}
__device__ __forceinline__ float wave_allsum(float v) { return swap_add32(swap_add16(row16_sum(v))); }
__device__ __forceinline__ float wave_allmax(float v) {
  typedef unsigned u32x2_ __attribute__((ext_vector_type(2)));
  v = fmaxf(v, dpp_get<0xB1, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x4E, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x141, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x140, 0xF>(v, v));
  u32x2_ r = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
  r = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
}
#endif
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_get<0xB1, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x4E, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x141, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x140, 0xF>(v, v));
  v = fmaxf(v, dpp_get<0x142, 0xA>(v, v));
  v = fmaxf(v, dpp_get<0x143, 0xC>(v, v));
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
