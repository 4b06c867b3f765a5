// Capsule dynamic routing for any shape of the envelope Din 1..16, Dout 1..64, C 1..256 (any R, N, n_iter), forward and
// backward (gfx950).  routing.hip sends here every shape its specialised kernels do not take; cy_routing_general_* also
// reach these kernels directly (A/B runs, cross-checks).  Same maths, s_hist layout and determinism as routing.hip:
//   u_hat_ij = u_i W_ij ;  b^t_ij = u_hat_ij . V_t[j],  V_t = sum_{tau<t} v^tau ;  c^t = softmax_j(b^t) ;
//   s^t_j = sum_i c^t_ij u_hat_ij ;  v^t = squash(s^t) ;  s_hist[t] = s^t.
// Neither the logits nor u_hat are stored; u_hat is recomputed from (u, W) wherever it is needed.
//
// Layout: Dout is zero-padded to DP in {4, 8, 16, 24, 32, 48, 64} (a zero component changes neither u_hat . V nor |s|),
// C is padded to Cp = 64 * CW lanes with CW = 1, 2 or 4 waves per row (the padded lanes take no part in the softmax:
// their logit is -inf).  A block of 4 waves holds 4 / CW rows; lane <-> output capsule j, the DP components of s, V and
// u_hat of that (row, j) live in registers.  W is repacked once per call into Wp[i][d][DP/4][Cp][4] so that one f32x4
// load of a wave reads 1 KiB contiguous, shared through L1 by the rows of the block.  The softmax is a wave all-reduce
// (DPP / permlane) plus, for CW > 1, one exchange of (max, sum) pairs through LDS.
//
// Every sum that crosses blocks is a fixed-order split sum, no atomics:
//  * forward, per iteration: pass over (row blocks) x (chunks of i) writing per-chunk partial sums, then a finish
//    launch (sum over chunks in order, s_hist, squash, V += v);
//  * backward: prep (V_t of every t, ds^{T-1}), then for t = T-1..1 a pass producing dV_t = sum_i db^t_ij u_hat_ij per
//    chunk and a finish (SA += dV_t, ds^{t-1} = squash'(s^{t-1}) SA); then, per chunk of input capsules, one pass
//    writes du and du_hat = sum_t c^t ds^t + db^t V_t to a staging buffer, and a row-split contraction
//    dW_i = sum_rows u_i (x) du_hat_i (plus a fixed-order sum over the row splits) finishes dW.
// Nothing is allocated and nothing synchronises the host: the workspace is sized by the _ws_floats queries.
#include "common.h"
#include <math.h>

namespace {

constexpr int RG_THREADS = 256;
constexpr long long RG_DUH_BUDGET = 64ll << 20;     // floats of the du_hat staging buffer per chunk of input capsules
constexpr int RG_MAX_DIN = CYI_RG_MAX_DIN;

inline int rg_cw(int C) { return C <= 64 ? 1 : C <= 128 ? 2 : 4; }
inline int rg_dp(int Dout) {
  return Dout <= 4 ? 4 : Dout <= 8 ? 8 : Dout <= 16 ? 16 : Dout <= 24 ? 24 : Dout <= 32 ? 32 : Dout <= 48 ? 48 : 64;
}
inline long long rg_align4(long long n) { return (n + 3) & ~3ll; }

// offset (in floats) of the Din-vector of input capsule i of row `row` (g != 0: the DarkCapsuleNet cell gather, Din = 8)
__device__ __forceinline__ long long rg_u_offset(int row, int i, int N, int Din, int g, int B) {
  if (g == 0) return ((long long)row * N + i) * Din;
  const int k = row / B, b = row - k * B;
  const int pos = i >> 5, chg = i & 31;
  const long long pix = (long long)b * 16 * g * g + (long long)(pos >> 2) * 4 * g * g + 4 * k + (pos & 3);
  return pix * 256 + chg * 8;
}
__device__ __forceinline__ long long rg_out_row(int row, int g, int B) {
  if (g == 0) return row;
  const int k = row / B, b = row - k * B;
  return (long long)b * g * g + k;
}

template <int D>
__device__ __forceinline__ void rg_squash(const float* s, float* v) {
  float n2 = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) n2 += s[o] * s[o];
  const float f = (n2 / (1.f + n2)) / sqrtf(n2);          // no epsilon: 0 -> NaN like the reference
#pragma unroll
  for (int o = 0; o < D; ++o) v[o] = f * s[o];
}
template <int D>
__device__ __forceinline__ void rg_squash_bwd(const float* s, const float* dv, float* ds) {
  float n2 = 0.f, sd = 0.f;
#pragma unroll
  for (int o = 0; o < D; ++o) { n2 += s[o] * s[o]; sd += s[o] * dv[o]; }
  const float n = sqrtf(n2);
  const float h = n / (1.f + n2);
  const float hp = (1.f - n2) / ((1.f + n2) * (1.f + n2));
  const float k = sd * hp / n;
#pragma unroll
  for (int o = 0; o < D; ++o) ds[o] = h * dv[o] + k * s[o];
}
template <int DP>
__device__ __forceinline__ void rg_load(float* x, const float* p) {
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    const f32x4 v = *(const f32x4*)(p + 4 * q);
    x[4 * q] = v[0]; x[4 * q + 1] = v[1]; x[4 * q + 2] = v[2]; x[4 * q + 3] = v[3];
  }
}
template <int DP>
__device__ __forceinline__ void rg_store(float* p, const float* x) {
#pragma unroll
  for (int q = 0; q < DP / 4; ++q) {
    f32x4 v;
    v[0] = x[4 * q]; v[1] = x[4 * q + 1]; v[2] = x[4 * q + 2]; v[3] = x[4 * q + 3];
    *(f32x4*)(p + 4 * q) = v;
  }
}
template <int DP>
__device__ __forceinline__ float rg_dot(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int o = 0; o < DP; ++o) s += a[o] * b[o];
  return s;
}

// Reductions over the CW waves of one row group.  Each call writes one parity of its LDS table and passes one block barrier;
// the next call on the same table uses the other parity, so a table is never rewritten before every wave has read it.
struct rg_group {
  int CW, grp, w, lane;
  float (*red)[4][2];        // [parity][wave][max, sum]
  float (*redv)[4][RG_MAX_DIN];
  int par, parv;

  // softmax over the row's capsules of this lane's logit b (-inf on padded lanes, which then get 0)
  __device__ __forceinline__ float softmax(float b) {
    const float m = wave_allmax(b);
    const float e = b == -INFINITY ? 0.f : expf(b - m);
    const float S = wave_allsum(e);
    if (CW == 1) return e / S;
    if (lane == 0) { red[par][w][0] = m; red[par][w][1] = S; }
    __syncthreads();
    float M = -INFINITY;
    for (int k = 0; k < CW; ++k) M = fmaxf(M, red[par][grp * CW + k][0]);
    float T = 0.f;
    for (int k = 0; k < CW; ++k) {
      const float mk = red[par][grp * CW + k][0], sk = red[par][grp * CW + k][1];
      T += sk == 0.f ? 0.f : sk * expf(mk - M);
    }
    par ^= 1;
    return b == -INFINITY ? 0.f : expf(b - M) / T;
  }
  __device__ __forceinline__ float sum(float x) {
    const float s = wave_allsum(x);
    if (CW == 1) return s;
    if (lane == 0) red[par][w][1] = s;
    __syncthreads();
    float T = 0.f;
    for (int k = 0; k < CW; ++k) T += red[par][grp * CW + k][1];
    par ^= 1;
    return T;
  }
  // p[0..Din) summed over the row's capsules, every lane of the group gets the totals
  __device__ __forceinline__ void sum_vec(float* p, int Din) {
#pragma unroll
    for (int d = 0; d < RG_MAX_DIN; ++d)
      if (d < Din) p[d] = wave_allsum(p[d]);
    if (CW == 1) return;
    if (lane == 0) {
#pragma unroll
      for (int d = 0; d < RG_MAX_DIN; ++d)
        if (d < Din) redv[parv][w][d] = p[d];
    }
    __syncthreads();
#pragma unroll
    for (int d = 0; d < RG_MAX_DIN; ++d) {
      if (d < Din) {
        float T = 0.f;
        for (int k = 0; k < CW; ++k) T += redv[parv][grp * CW + k][d];
        p[d] = T;
      }
    }
    parv ^= 1;
  }
};

struct rg_args {
  const float* u; const float* Wp;
  int R, N, C, Din, Dout, Cp, CW, g, B;
  int i0, ic, i1;            // block y covers input capsules [i0 + y*ic, min(i0 + (y+1)*ic, i1))
  const float* V;            // [R][C][DP] (forward: NULL in iteration 0)
  const float* ds;           // [R][C][DP] (dV pass)
  float* slab;               // [gridDim.y][R][C][DP] partial sums
  long long plane;           // R*C*DP
  int T; const float* V_all; const float* ds_all; float* duh; float* du; int ich;   // du_hat pass
};

enum { RG_FWD = 0, RG_DV = 1, RG_DUH = 2 };

// u_hat of (row, i) for this lane's capsule j: Din x DP/4 coalesced f32x4 loads of the packed W
template <int DP>
__device__ __forceinline__ void rg_uhat(const rg_args& a, int row, int i, int j, float* uh) {
  constexpr int DQ = DP / 4;
#pragma unroll
  for (int o = 0; o < DP; ++o) uh[o] = 0.f;
  const long long uo = rg_u_offset(row, i, a.N, a.Din, a.g, a.B);
  const f32x4* wp = (const f32x4*)a.Wp + (long long)i * a.Din * DQ * a.Cp + j;
  for (int d = 0; d < a.Din; ++d) {
    const float x = a.u[uo + d];
#pragma unroll
    for (int q = 0; q < DQ; ++q) {
      const f32x4 w4 = wp[(long long)(d * DQ + q) * a.Cp];
      uh[4 * q] += x * w4[0]; uh[4 * q + 1] += x * w4[1]; uh[4 * q + 2] += x * w4[2]; uh[4 * q + 3] += x * w4[3];
    }
  }
}

template <int DP, int MODE>
__global__ __launch_bounds__(RG_THREADS) void rg_pass_kernel(rg_args a) {
  __shared__ float red[2][4][2];
  __shared__ float redv[2][4][RG_MAX_DIN];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  rg_group G{a.CW, w / a.CW, w, lane, red, redv, 0, 0};
  const int wj = w - G.grp * a.CW;
  const int j = wj * 64 + lane;
  const bool jv = j < a.C;
  const int row0 = blockIdx.x * (4 / a.CW) + G.grp;
  const bool rv = row0 < a.R;
  const int row = rv ? row0 : a.R - 1;    // a group past the last row recomputes row R-1 (it takes part in the barriers), stores nothing
  const int ib = a.i0 + blockIdx.y * a.ic;
  const int ie = min(ib + a.ic, a.i1);
  const long long rj = ((long long)row * a.C + (jv ? j : 0)) * DP;
  const float inv_c = 1.f / (float)a.C;
  float uh[DP], acc[DP];
#pragma unroll
  for (int o = 0; o < DP; ++o) acc[o] = 0.f;

  if constexpr (MODE == RG_FWD || MODE == RG_DV) {
    float Vr[DP], dsr[DP];
    const bool hasV = a.V != nullptr;
    if (hasV) rg_load<DP>(Vr, a.V + rj);
    else {
#pragma unroll
      for (int o = 0; o < DP; ++o) Vr[o] = 0.f;
    }
    if constexpr (MODE == RG_DV) rg_load<DP>(dsr, a.ds + rj);
    for (int i = ib; i < ie; ++i) {
      rg_uhat<DP>(a, row, i, j, uh);
      float c = jv ? inv_c : 0.f;       // iteration 0: softmax of zero logits
      if (hasV) c = G.softmax(jv ? rg_dot<DP>(uh, Vr) : -INFINITY);
      if constexpr (MODE == RG_FWD) {
#pragma unroll
        for (int o = 0; o < DP; ++o) acc[o] += c * uh[o];
      } else {
        const float dc = rg_dot<DP>(dsr, uh);
        const float cd = G.sum(c * dc);
        const float db = c * (dc - cd);
#pragma unroll
        for (int o = 0; o < DP; ++o) acc[o] += db * uh[o];
      }
    }
    if (rv && jv) rg_store<DP>(a.slab + (long long)blockIdx.y * a.plane + rj, acc);
  } else {
    constexpr int DQ = DP / 4;
    for (int i = ib; i < ie; ++i) {
      rg_uhat<DP>(a, row, i, j, uh);
#pragma unroll
      for (int o = 0; o < DP; ++o) acc[o] = 0.f;               // du_hat of (row, i, j)
      for (int tt = 0; tt < a.T; ++tt) {
        float dsr[DP];
        rg_load<DP>(dsr, a.ds_all + (long long)tt * a.plane + rj);
        if (tt == 0) {
          const float c = jv ? inv_c : 0.f;
#pragma unroll
          for (int o = 0; o < DP; ++o) acc[o] += c * dsr[o];
        } else {
          float Vt[DP];
          rg_load<DP>(Vt, a.V_all + (long long)tt * a.plane + rj);
          const float c = G.softmax(jv ? rg_dot<DP>(uh, Vt) : -INFINITY);
          const float dc = rg_dot<DP>(dsr, uh);
          const float cd = G.sum(c * dc);
          const float db = c * (dc - cd);
#pragma unroll
          for (int o = 0; o < DP; ++o) acc[o] += c * dsr[o] + db * Vt[o];
        }
      }
      if (rv && jv) rg_store<DP>(a.duh + (((long long)row * a.ich + (i - a.i0)) * a.C + j) * DP, acc);
      // du_i = sum_j W_ij du_hat_ij
      float p[RG_MAX_DIN];
      const f32x4* wp = (const f32x4*)a.Wp + (long long)i * a.Din * DQ * a.Cp + j;
#pragma unroll
      for (int d = 0; d < RG_MAX_DIN; ++d) {
        p[d] = 0.f;
        if (d < a.Din) {
#pragma unroll
          for (int q = 0; q < DQ; ++q) {
            const f32x4 w4 = wp[(long long)(d * DQ + q) * a.Cp];
            p[d] += w4[0] * acc[4 * q] + w4[1] * acc[4 * q + 1] + w4[2] * acc[4 * q + 2] + w4[3] * acc[4 * q + 3];
          }
        }
      }
      G.sum_vec(p, a.Din);
      if (rv && wj == 0) {
        const long long uo = rg_u_offset(row, i, a.N, a.Din, a.g, a.B);
#pragma unroll
        for (int d = 0; d < RG_MAX_DIN; ++d)
          if (d < a.Din && lane == d) a.du[uo + d] = p[d];
      }
    }
  }
}

// Wp[i][d][q][jp][4] = W[i][jp][d][4q + c] (0 for jp >= C or 4q + c >= Dout)
__global__ void rg_pack_kernel(const float* __restrict__ W, float* __restrict__ Wp, int N, int C, int Din, int Dout, int DP,
                               int Cp) {
  const long long n = (long long)N * Din * DP * Cp;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int c4 = (int)(e & 3);
  long long r = e >> 2;
  const int jp = (int)(r % Cp); r /= Cp;
  const int q = (int)(r % (DP / 4)); r /= DP / 4;
  const int d = (int)(r % Din);
  const long long i = r / Din;
  const int o = 4 * q + c4;
  Wp[e] = (jp < C && o < Dout) ? W[((i * C + jp) * Din + d) * Dout + o] : 0.f;
}

// forward finish of iteration `it`, one thread per (row, j): s = sum of the chunks in order, s_hist, v = squash(s), V (+)= v
template <int DP>
__global__ __launch_bounds__(128) void rg_fwd_fin_kernel(const float* __restrict__ slab, int nch, long long plane, int R, int C, int Dout,
                                  float* __restrict__ s_hist_it, float* __restrict__ V, float* __restrict__ v_out, int it,
                                  int last, int g, int B) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)R * C) return;
  float s[DP], x[DP], v[DP];
#pragma unroll
  for (int o = 0; o < DP; ++o) s[o] = 0.f;
  for (int k = 0; k < nch; ++k) {
    rg_load<DP>(x, slab + k * plane + idx * DP);
#pragma unroll
    for (int o = 0; o < DP; ++o) s[o] += x[o];
  }
#pragma unroll
  for (int o = 0; o < DP; ++o)
    if (o < Dout) s_hist_it[idx * Dout + o] = s[o];
  rg_squash<DP>(s, v);
  if (it > 0) {
    rg_load<DP>(x, V + idx * DP);
#pragma unroll
    for (int o = 0; o < DP; ++o) x[o] += v[o];
    rg_store<DP>(V + idx * DP, x);
  } else {
    rg_store<DP>(V + idx * DP, v);
  }
  if (last) {
    const int row = (int)(idx / C), j = (int)(idx - (long long)row * C);
    float* dst = v_out + (rg_out_row(row, g, B) * C + j) * Dout;
#pragma unroll
    for (int o = 0; o < DP; ++o)
      if (o < Dout) dst[o] = v[o];
  }
}

// backward preparation, one thread per (row, j): V_all[t] = sum_{tau<t} squash(s^tau), ds_all[T-1] = squash'(s^{T-1}) dv,
// SA = 0.  C == 1: every iteration has the same sums (the coupling is 1), and the specialised C == 1 forward keeps only the
// last one, so s^{T-1} stands for all of them.
template <int DP>
__global__ __launch_bounds__(128) void rg_bwd_prep_kernel(const float* __restrict__ s_hist, const float* __restrict__ dv, float* __restrict__ V_all,
                                   float* __restrict__ ds_all, float* __restrict__ SA, int R, int C, int Dout, int T, int g,
                                   int B) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)R * C) return;
  const long long plane = (long long)R * C * DP, uplane = (long long)R * C * Dout;
  float Vt[DP], st[DP], x[DP];
#pragma unroll
  for (int o = 0; o < DP; ++o) Vt[o] = 0.f;
  for (int t = 0; t < T; ++t) {
    const float* sp = s_hist + (long long)(C == 1 ? T - 1 : t) * uplane + idx * Dout;
#pragma unroll
    for (int o = 0; o < DP; ++o) st[o] = o < Dout ? sp[o] : 0.f;
    rg_store<DP>(V_all + t * plane + idx * DP, Vt);
    if (t == T - 1) {
      const int row = (int)(idx / C), j = (int)(idx - (long long)row * C);
      const float* dp = dv + (rg_out_row(row, g, B) * C + j) * Dout;
      float d[DP];
#pragma unroll
      for (int o = 0; o < DP; ++o) d[o] = o < Dout ? dp[o] : 0.f;
      rg_squash_bwd<DP>(st, d, x);
      rg_store<DP>(ds_all + t * plane + idx * DP, x);
#pragma unroll
      for (int o = 0; o < DP; ++o) x[o] = 0.f;
      rg_store<DP>(SA + idx * DP, x);
    } else {
      rg_squash<DP>(st, x);
#pragma unroll
      for (int o = 0; o < DP; ++o) Vt[o] += x[o];
    }
  }
}

// backward finish of step t: A_t = sum of the chunks in order, SA += A_t, ds^{t-1} = squash'(s^{t-1}) SA
template <int DP>
__global__ __launch_bounds__(128) void rg_bwd_fin_kernel(const float* __restrict__ slab, int nch, long long plane, int R, int C, int Dout,
                                  const float* __restrict__ s_prev, float* __restrict__ SA, float* __restrict__ ds_prev) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (long long)R * C) return;
  float s[DP], x[DP], st[DP];
  rg_load<DP>(s, SA + idx * DP);
  for (int k = 0; k < nch; ++k) {
    rg_load<DP>(x, slab + k * plane + idx * DP);
#pragma unroll
    for (int o = 0; o < DP; ++o) s[o] += x[o];
  }
  rg_store<DP>(SA + idx * DP, s);
#pragma unroll
  for (int o = 0; o < DP; ++o) st[o] = o < Dout ? s_prev[idx * Dout + o] : 0.f;
  rg_squash_bwd<DP>(st, s, x);
  rg_store<DP>(ds_prev + idx * DP, x);
}

// dW of a chunk of input capsules [i0, i0 + ich) over the rows of split blockIdx.y: out[split][il][j][d][o] =
// sum_rows u[row, i0 + il, d] du_hat[row][il][j][o], one thread per (il, j, o)
__global__ __launch_bounds__(RG_THREADS) void rg_dw_kernel(const float* __restrict__ u, const float* __restrict__ duh,
                                                          float* __restrict__ out, int R, int N, int C, int Din, int Dout,
                                                          int DP, int i0, int nic, int ich, int rps, int g, int B) {
  const long long n = (long long)nic * C * Dout;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  const int o = (int)(e % Dout);
  const long long ij = e / Dout;
  const int j = (int)(ij % C), il = (int)(ij / C);
  const int r0 = blockIdx.y * rps, r1 = min(R, r0 + rps);
  float acc[RG_MAX_DIN];
#pragma unroll
  for (int d = 0; d < RG_MAX_DIN; ++d) acc[d] = 0.f;
  for (int r = r0; r < r1; ++r) {
    const float x = duh[(((long long)r * ich + il) * C + j) * DP + o];
    const long long uo = rg_u_offset(r, i0 + il, N, Din, g, B);
#pragma unroll
    for (int d = 0; d < RG_MAX_DIN; ++d)
      if (d < Din) acc[d] += u[uo + d] * x;
  }
  float* dst = out + (long long)blockIdx.y * ich * C * Din * Dout + (ij * Din) * Dout + o;
#pragma unroll
  for (int d = 0; d < RG_MAX_DIN; ++d)
    if (d < Din) dst[(long long)d * Dout] = acc[d];
}

// out[e] = sum_k slabs[k * stride + e], k in order
__global__ void rg_split_sum_kernel(const float* __restrict__ slabs, float* __restrict__ out, int nslabs, long long stride,
                                    long long n) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  float s = 0.f;
  for (int k = 0; k < nslabs; ++k) s += slabs[k * stride + e];
  out[e] = s;
}

// ------------------------------------------------------------------------------------------------ host plan
typedef cyi_routing_plan_t::cyi_rg_plan_t rg_plan;

rg_args base_args(const float* u, const float* Wp, int R, int N, int C, int Din, int Dout, int g, int B, const rg_plan& p) {
  rg_args r{};
  r.u = u; r.Wp = Wp; r.R = R; r.N = N; r.C = C; r.Din = Din; r.Dout = Dout; r.Cp = p.Cp; r.CW = p.CW; r.g = g; r.B = B;
  r.plane = p.plane;
  return r;
}

int pack(const float* W, float* Wp, int N, int C, int Din, int Dout, const rg_plan& p, hipStream_t s) {
  rg_pack_kernel<<<(unsigned)cy_ceil_div(p.wp, 256), 256, 0, s>>>(W, Wp, N, C, Din, Dout, p.DP, p.Cp);
  CY_LAUNCH_CHECK("routing general: pack W");
  return 0;
}

template <int DP>
int fwd_dp(const cy_routing_fwd_t* a, const cyi_routing_plan_t& P, hipStream_t s) {
  const rg_plan& p = P.rg;
  float* Wp = cyi_ws_at(a->ws, &P, CYI_WS_W);
  float* V = cyi_ws_at(a->ws, &P, CYI_WS_V);
  float* slab = cyi_ws_at(a->ws, &P, CYI_WS_SLABS);
  int rc = pack(a->W, Wp, a->N, a->C, a->Din, a->Dout, p, s);
  if (rc) return rc;
  rg_args r = base_args(a->u, Wp, a->R, a->N, a->C, a->Din, a->Dout, a->gather_g, a->gather_B, p);
  r.i0 = 0; r.ic = p.ic; r.i1 = a->N; r.slab = slab;
  const unsigned fb = (unsigned)cy_ceil_div((long long)a->R * a->C, 128);
  const long long uplane = (long long)a->R * a->C * a->Dout;
  for (int it = 0; it < a->n_iter; ++it) {
    r.V = it > 0 ? V : nullptr;
    rg_pass_kernel<DP, RG_FWD><<<dim3(p.nrb, p.nch), RG_THREADS, 0, s>>>(r);
    CY_LAUNCH_CHECK("cy_routing_general_fwd: pass");
    rg_fwd_fin_kernel<DP><<<fb, 128, 0, s>>>(slab, p.nch, p.plane, a->R, a->C, a->Dout, a->s_hist + it * uplane, V, a->v_out, it,
                                             it == a->n_iter - 1, a->gather_g, a->gather_B);
    CY_LAUNCH_CHECK("cy_routing_general_fwd: finish");
  }
  return 0;
}

template <int DP>
int bwd_dp(const cy_routing_bwd_t* a, const cyi_routing_plan_t& P, hipStream_t s) {
  const rg_plan& p = P.rg;
  const int T = a->n_iter, R = a->R, C = a->C;
  float* Wp = cyi_ws_at(a->ws, &P, CYI_WS_W);
  float* V_all = cyi_ws_at(a->ws, &P, CYI_WS_V);
  float* ds_all = cyi_ws_at(a->ws, &P, CYI_WS_DS_ALL);
  float* SA = cyi_ws_at(a->ws, &P, CYI_WS_SA);
  float* slab = cyi_ws_at(a->ws, &P, CYI_WS_SLABS);
  float* duh = cyi_ws_at(a->ws, &P, CYI_WS_DUH);
  float* dws = cyi_ws_at(a->ws, &P, CYI_WS_DWS);          // NULL without row splits (p.rs == 1)
  int rc = pack(a->W, Wp, a->N, C, a->Din, a->Dout, p, s);
  if (rc) return rc;
  const unsigned fb = (unsigned)cy_ceil_div((long long)R * C, 128);
  rg_bwd_prep_kernel<DP><<<fb, 128, 0, s>>>(a->s_hist, a->dv, V_all, ds_all, SA, R, C, a->Dout, T, a->gather_g, a->gather_B);
  CY_LAUNCH_CHECK("cy_routing_general_bwd: prep");
  rg_args r = base_args(a->u, Wp, R, a->N, C, a->Din, a->Dout, a->gather_g, a->gather_B, p);
  const long long uplane = (long long)R * C * a->Dout;
  for (int t = T - 1; t >= 1; --t) {
    r.i0 = 0; r.ic = p.ic; r.i1 = a->N; r.slab = slab;
    r.V = V_all + t * p.plane; r.ds = ds_all + t * p.plane;
    rg_pass_kernel<DP, RG_DV><<<dim3(p.nrb, p.nch), RG_THREADS, 0, s>>>(r);
    CY_LAUNCH_CHECK("cy_routing_general_bwd: dV pass");
    rg_bwd_fin_kernel<DP><<<fb, 128, 0, s>>>(slab, p.nch, p.plane, R, C, a->Dout, a->s_hist + (C == 1 ? T - 1 : t - 1) * uplane,
                                             SA, ds_all + (t - 1) * p.plane);
    CY_LAUNCH_CHECK("cy_routing_general_bwd: finish");
  }
  r.T = T; r.V_all = V_all; r.ds_all = ds_all; r.duh = duh; r.du = a->du; r.ich = p.ich; r.V = nullptr; r.ds = nullptr;
  const long long wi = (long long)C * a->Din * a->Dout;    // dW floats per input capsule
  for (int c = 0; c < p.nich; ++c) {
    const int i0 = c * p.ich, n = min(p.ich, a->N - i0);
    r.i0 = i0; r.ic = p.ipb; r.i1 = i0 + n;
    rg_pass_kernel<DP, RG_DUH><<<dim3(p.nrb, (unsigned)cy_ceil_div(n, p.ipb)), RG_THREADS, 0, s>>>(r);
    CY_LAUNCH_CHECK("cy_routing_general_bwd: du pass");
    const unsigned xb = (unsigned)cy_ceil_div((long long)n * C * a->Dout, RG_THREADS);
    float* dWc = a->dW + i0 * wi;
    rg_dw_kernel<<<dim3(xb, p.rs), RG_THREADS, 0, s>>>(a->u, duh, p.rs > 1 ? dws : dWc, R, a->N, C, a->Din, a->Dout, DP, i0, n,
                                                      p.ich, p.rps, a->gather_g, a->gather_B);
    CY_LAUNCH_CHECK("cy_routing_general_bwd: dW");
    if (p.rs > 1) {      // the splits are p.ich input capsules apart; a short last chunk fills the first n of each
      const long long m = (long long)n * wi;
      rg_split_sum_kernel<<<(unsigned)cy_ceil_div(m, 256), 256, 0, s>>>(dws, dWc, p.rs, (long long)p.ich * wi, m);
      CY_LAUNCH_CHECK("cy_routing_general_bwd: dW splits");
    }
  }
  return 0;
}

}  // namespace

// the general kernels' part of the routing plan: launch numbers and workspace regions (tables: DESIGN section 4g)
void cyi_general_plan(int R, int N, int C, int Din, int Dout, int n_iter, int backward, cyi_routing_plan_t* P) {
  rg_plan& p = P->rg;
  p.DP = rg_dp(Dout);
  p.CW = rg_cw(C);
  p.Cp = 64 * p.CW;
  p.nrb = (int)cy_ceil_div(R, 4 / p.CW);
  p.plane = (long long)R * C * p.DP;
  p.wp = (long long)N * Din * p.DP * p.Cp;
  // about 4 blocks per CU, chunks of at least 4 input capsules
  long long n = cy_ceil_div(1024, p.nrb);
  const long long nmax = cy_ceil_div(N, 4);
  if (n > nmax) n = nmax;
  if (n < 1) n = 1;
  p.ic = (int)cy_ceil_div(N, n);
  p.nch = (int)cy_ceil_div(N, p.ic);
  long long ich = RG_DUH_BUDGET / p.plane;
  if (ich > N) ich = N;
  if (ich < 1) ich = 1;
  p.ich = (int)ich;
  p.nich = (int)cy_ceil_div(N, p.ich);
  long long ipb = cy_ceil_div((long long)p.nrb * p.ich, 1024);
  if (ipb > p.ich) ipb = p.ich;
  p.ipb = (int)ipb;
  const long long xb = cy_ceil_div((long long)p.ich * C * Dout, RG_THREADS);
  long long rs = cy_ceil_div(2048, xb);
  const long long rsmax = cy_ceil_div(R, 8);
  if (rs > rsmax) rs = rsmax;
  if (rs < 1) rs = 1;
  p.rps = (int)cy_ceil_div(R, rs);
  p.rs = (int)cy_ceil_div(R, p.rps);
  P->row_blocks = p.nrb; P->nch = p.nch; P->ic = p.ic;
  cyi_ws_add(P, CYI_WS_W, p.wp, 1);
  cyi_ws_add(P, CYI_WS_V, (backward ? n_iter : 1) * p.plane, 1);
  if (backward) {
    cyi_ws_add(P, CYI_WS_DS_ALL, n_iter * p.plane, 1);
    cyi_ws_add(P, CYI_WS_SA, p.plane, 1);
  }
  cyi_ws_add(P, CYI_WS_SLABS, p.nch * p.plane, 1);
  if (backward) {
    cyi_ws_add(P, CYI_WS_DUH, (long long)R * p.ich * C * p.DP, 1);
    if (p.rs > 1) cyi_ws_add(P, CYI_WS_DWS, (long long)p.rs * p.ich * C * Din * Dout, 1);
  }
}

#define RG_DISPATCH(fn, a, p, s)                \
  switch ((p)->rg.DP) {                         \
    case 4: return fn<4>(a, *(p), s);           \
    case 8: return fn<8>(a, *(p), s);           \
    case 16: return fn<16>(a, *(p), s);         \
    case 24: return fn<24>(a, *(p), s);         \
    case 32: return fn<32>(a, *(p), s);         \
    case 48: return fn<48>(a, *(p), s);         \
    default: return fn<64>(a, *(p), s);         \
  }
int cyi_general_fwd(const cy_routing_fwd_t* a, const cyi_routing_plan_t* p, hipStream_t s) {
  CY_REQUIRE(a->ws, "cy_routing_general_fwd: needs the workspace (ws) of cy_routing_general_fwd_ws_floats()");
  RG_DISPATCH(fwd_dp, a, p, s)
}
int cyi_general_bwd(const cy_routing_bwd_t* a, const cyi_routing_plan_t* p, hipStream_t s) { RG_DISPATCH(bwd_dp, a, p, s) }

#define RG_PLAN_OF(fn, a, backward, p) \
  cyi_routing_plan(fn, (a)->R, (a)->N, (a)->C, (a)->Din, (a)->Dout, (a)->n_iter, (a)->gather_g, (a)->gather_B, backward, 1, p)

extern "C" long long cy_routing_general_fwd_ws_floats(const cy_routing_fwd_t* a) {
  cyi_routing_plan_t p;
  return a && RG_PLAN_OF("cy_routing_general_fwd_ws_floats", a, 0, &p) == 0 ? p.total : -1;
}
extern "C" long long cy_routing_general_bwd_ws_floats(const cy_routing_bwd_t* a) {
  cyi_routing_plan_t p;
  return a && RG_PLAN_OF("cy_routing_general_bwd_ws_floats", a, 1, &p) == 0 ? p.total : -1;
}

extern "C" int cy_routing_general_fwd(const cy_routing_fwd_t* a, void* stream) {
  CY_REQUIRE(a && a->u && a->W && a->v_out && a->s_hist, "cy_routing_general_fwd: null pointer");
  cyi_routing_plan_t p;
  const int rc = RG_PLAN_OF("cy_routing_general_fwd", a, 0, &p);
  return rc ? rc : cyi_general_fwd(a, &p, (hipStream_t)stream);
}
extern "C" int cy_routing_general_bwd(const cy_routing_bwd_t* a, void* stream) {
  CY_REQUIRE(a && a->u && a->W && a->s_hist && a->dv && a->du && a->dW && a->ws, "cy_routing_general_bwd: null pointer");
  cyi_routing_plan_t p;
  const int rc = RG_PLAN_OF("cy_routing_general_bwd", a, 1, &p);
  return rc ? rc : cyi_general_bwd(a, &p, (hipStream_t)stream);
}
