// Linear layers with a long reduction and few rows, and the softmax cross-entropy (gfx950).
// Replaces the nn.Linear pair of models.py:22-43 (ConvNet: Linear(128*16*16 -> 128) -> ReLU -> Linear(128 -> C)) with its
// autograd, and loss_fns.py:6-8 (cnn_loss).  Everything is fp32 and row-major; W[N][K] lies as nn.Linear stores it.
//
// All three products run on v_mfma_f32_16x16x4_f32 (the compiler-tracked builtin: no hand-counted waits), operands straight from
// global memory -- every operand element is used by one wave only, so there is nothing LDS could share:
//   forward   Y[m][n]  = sum_k X[m][k] W[n][k]     both operands are contiguous along the reduction: a lane loads 16 bytes of a row of
//                                                  X and of W (k = k0 + 4 (lane / 16) + j) and issues one MFMA per j -- the order of the
//                                                  reduction inside a tile is free as long as both operands use the same one;
//   dgrad     dX[m][k] = sum_n dY[m][n] W[n][k]    } one kernel, C[r][k] = sum_q A(r, q) B[q][k]: the long axis k is the COLUMN axis;
//   wgrad     dW[n][k] = sum_m dY[m][n] X[m][k]    } a lane loads 16 bytes of a row of B (columns k0 + 4 (lane % 16) + j: tile j of
//                                                  four column tiles) and ends with 4 consecutive k of a row: 16-byte stores.
// The forward's reduction is long (K = 32768) and its output tiny (2 tiles at M = 16, N = 128): K is split over the chip in shares,
// every share writes its partial tile to ws[share][M][N], and a second kernel adds the shares in a fixed order (+ bias, ReLU).
// No atomics anywhere: every kernel of this file repeats bit for bit.
#include "common.h"
#include "prims.h"

namespace {

using cyk::mfma16;

constexpr int LIN_MAX_M = 4096, LIN_MAX_N = 1024, LIN_MAX_C = 1024, LIN_MAX_K = 1 << 20;
constexpr int LIN_SLICE_UNIT = 64;    // a share's slice of K is a multiple of this (one unrolled trip of the forward's loop)
constexpr int LIN_SLICE_MIN = 128;    // K up to this: one share
constexpr int LIN_MAX_SHARES = 256;

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ f32x4 ld4_if(const float* p, bool ok) { return ok ? ld4(p) : f32x4{0.f, 0.f, 0.f, 0.f}; }

// ---- forward.  Block: 4 waves, wave w owns the 16 rows of W at n = 64 blockIdx.x + 16 w and all MT row tiles of X at
// m = 16 MT blockIdx.y; blockIdx.z is the share.  Rows past M / N are clamped for the loads (a row of A only reaches the same row of
// the tile, a column of B the same column) and dropped at the store.
template <int MT>
__global__ __launch_bounds__(256) void linear_fwd_kernel(const float* __restrict__ X, const float* __restrict__ W,
                                                         const float* __restrict__ bias, float* __restrict__ out, int M, int N, int K,
                                                         int slice, int act, int direct) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 64 + wave * 16, m0 = blockIdx.y * 16 * MT;
  if (n0 >= N) return;                                       // (no barrier in this kernel)
  const int k_begin = blockIdx.z * slice;
  const int k_end = k_begin + slice < K ? k_begin + slice : K;
  const float* wp = W + (long long)(n0 + c < N ? n0 + c : N - 1) * K + 4 * g;
  const float* xp[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = m0 + 16 * t + c;
    xp[t] = X + (long long)(m < M ? m : M - 1) * K + 4 * g;
  }
  f32x4 acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};

  int kb = k_begin;
  for (; kb + 64 <= k_end; kb += 64) {                       // 4 x 16 k per trip, every load inside the slice
    f32x4 w[4], x[4][MT];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      w[u] = ld4(wp + kb + 16 * u);
#pragma unroll
      for (int t = 0; t < MT; ++t) x[u][t] = ld4(xp[t] + kb + 16 * u);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t] = mfma16(x[u][t][j], w[u][j], acc[t]);
  }
  for (; kb < k_end; kb += 16) {                             // the ragged end of K (a multiple of 4): whole 16-byte pieces in or out
    const bool ok = kb + 4 * g < k_end;
    const f32x4 w = ld4_if(wp + kb, ok);
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const f32x4 x = ld4_if(xp[t] + kb, ok);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[t] = mfma16(x[j], w[j], acc[t]);
    }
  }

  const int n = n0 + c;
  if (n >= N) return;
  const float b = (direct && bias) ? bias[n] : 0.f;
  float* dst = direct ? out : out + (long long)blockIdx.z * M * N;
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = m0 + 16 * t + 4 * g + i;
      if (m >= M) continue;
      float v = acc[t][i] + b;
      if (direct && act == 1) v = v > 0.f ? v : 0.f;
      dst[(long long)m * N + n] = v;
    }
}

// Y = act(sum over the shares + bias) in a fixed order: 64 outputs per block, 16 threads per output; thread p adds the shares
// p, p + 16, ... in ascending order (at M = 16 there are 2048 outputs and 256 shares: one thread per output would walk 256 dependent
// loads on 8 blocks), thread 0 of the output then adds the 16 sums in ascending p.
constexpr int RED_PARTS = 16;
__global__ __launch_bounds__(64 * RED_PARTS) void linear_reduce_kernel(const float* __restrict__ P, const float* __restrict__ bias,
                                                                       float* __restrict__ Y, int MN, int N, int S, int act) {
  __shared__ float part[RED_PARTS][64];
  const int o = threadIdx.x & 63, p = threadIdx.x >> 6;
  const int idx = blockIdx.x * 64 + o;
  float s = 0.f;
  if (idx < MN)
    for (int z = p; z < S; z += RED_PARTS) s += P[(long long)z * MN + idx];
  part[p][o] = s;
  __syncthreads();
  if (p != 0 || idx >= MN) return;
  float t = part[0][o];
#pragma unroll
  for (int q = 1; q < RED_PARTS; ++q) t += part[q][o];
  if (bias) t += bias[idx % N];
  if (act == 1) t = t > 0.f ? t : 0.f;
  Y[idx] = t;
}

// ---- C[r][k] = sum_q A[r a_sr + q a_sq] B[q][k], r < R, q < Q (short), k < K (long); optional mask[R][K]: C = 0 where mask <= 0.
// Block: one wave, 16 RT rows x 64 columns (4 column tiles: tile j holds the columns k0 + 4 c + j, so that lane (c, g) ends with
// C[4 g + i][k0 + 4 c .. + 3] of every row tile).
template <int RT>
__global__ __launch_bounds__(64) void linear_out_kernel(const float* __restrict__ A, long long a_sr, long long a_sq,
                                                        const float* __restrict__ B, float* __restrict__ Cout,
                                                        const float* __restrict__ mask, int R, int Q, int K) {
  const int lane = threadIdx.x, c = lane & 15, g = lane >> 4;
  const int k = blockIdx.x * 64 + 4 * c;
  const int r0 = blockIdx.y * 16 * RT;
  const bool kok = k < K;                                    // K is a multiple of 4: the lane's 4 columns are all in or all out
  f32x4 acc[RT][4];
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[t][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const float* ap[RT];
  bool rok[RT];
#pragma unroll
  for (int t = 0; t < RT; ++t) {
    const int r = r0 + 16 * t + c;
    rok[t] = r < R;
    ap[t] = A + (long long)(rok[t] ? r : 0) * a_sr;
  }
  // A trip is 4 steps of 4 along q.  Its operands are loaded one trip ahead into the other of two register sets (one wave per SIMD at
  // the large shapes: nothing else hides the loads), from addresses clamped into the arrays: no branch around a load.  Only q past Q
  // needs a zero, and B gets it where it is used: a row of A past R or a column of B past K reaches only rows / columns that are not
  // stored, and A at a clamped q is an element of the same row r.
  const float* bp = B + (kok ? k : 0);
  f32x4 b0[4], b1[4];
  float a0[4][RT], a1[4][RT];
  auto fetch = [&](int q0, f32x4 (&fb)[4], float (&fa)[4][RT]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = q0 + 4 * u + g;
      const long long qc = q < Q ? q : Q - 1;
      fb[u] = ld4(bp + qc * K);
#pragma unroll
      for (int t = 0; t < RT; ++t) fa[u][t] = ap[t][qc * a_sq];
    }
  };
  auto multiply = [&](int q0, const f32x4 (&fb)[4], const float (&fa)[4][RT]) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      if (q0 + 4 * u >= Q) break;                            // (the same for the whole wave)
      const f32x4 bz = q0 + 4 * u + g < Q ? fb[u] : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int t = 0; t < RT; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[t][j] = mfma16(fa[u][t], bz[j], acc[t][j]);
    }
  };
  fetch(0, b0, a0);
  for (int q0 = 0; q0 < Q; q0 += 32) {                       // (a fetch past Q re-reads row Q - 1 and is not used: a fetch under a
    fetch(q0 + 16, b1, a1);                                  // condition would make the compiler wait for it where the paths join)
    multiply(q0, b0, a0);
    fetch(q0 + 32, b0, a0);
    multiply(q0 + 16, b1, a1);
  }
  if (!kok) return;
#pragma unroll
  for (int t = 0; t < RT; ++t)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = r0 + 16 * t + 4 * g + i;
      if (r >= R) continue;
      f32x4 v = {acc[t][0][i], acc[t][1][i], acc[t][2][i], acc[t][3][i]};
      if (mask) {
        const f32x4 x = ld4(mask + (long long)r * K + k);
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = x[j] > 0.f ? v[j] : 0.f;
      }
      *reinterpret_cast<f32x4*>(Cout + (long long)r * K + k) = v;
    }
}

// db[n] = sum_m dY[m][n], rows in ascending order
__global__ __launch_bounds__(256) void linear_db_kernel(const float* __restrict__ dY, float* __restrict__ db, int M, int N) {
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
  for (int m = 0; m < M; ++m) s += dY[(long long)m * N + n];
  db[n] = s;
}

template <int RT>
int launch_out(const char* who, const float* A, long long a_sr, long long a_sq, const float* B, float* Cout, const float* mask, int R,
               int Q, int K, hipStream_t s) {
  linear_out_kernel<RT><<<dim3((unsigned)cy_ceil_div(K, 64), (unsigned)cy_ceil_div(R, 16 * RT)), 64, 0, s>>>(A, a_sr, a_sq, B, Cout,
                                                                                                             mask, R, Q, K);
  CY_LAUNCH_CHECK(who);
  return 0;
}
// Row tiles per wave: as many as the rows need, up to 4; 8 when the reduction is short (Q <= 64) and the rows are many -- the kernel is
// then bound by the stream of B and C, and 8 row tiles (the 128 rows of dW in ConvNet's first linear layer) read B once.
int out_product(const char* who, const float* A, long long a_sr, long long a_sq, const float* B, float* Cout, const float* mask, int R,
                int Q, int K, hipStream_t s) {
  if (R <= 16) return launch_out<1>(who, A, a_sr, a_sq, B, Cout, mask, R, Q, K, s);
  if (R <= 32) return launch_out<2>(who, A, a_sr, a_sq, B, Cout, mask, R, Q, K, s);
  if (R <= 64 || Q > 64) return launch_out<4>(who, A, a_sr, a_sq, B, Cout, mask, R, Q, K, s);
  return launch_out<8>(who, A, a_sr, a_sq, B, Cout, mask, R, Q, K, s);
}

bool lin_shape_ok(int M, int N, int K) {
  return M >= 1 && M <= LIN_MAX_M && N >= 1 && N <= LIN_MAX_N && K >= 4 && K <= LIN_MAX_K && K % 4 == 0;
}
int lin_rows_per_block(int M) { return M <= 16 ? 16 : M <= 32 ? 32 : 64; }
bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The shares of the forward's reduction (host arithmetic, see include/capsyolo_hip.h).
void lin_fwd_plan(int M, int N, int K, int* shares, int* slice) {
  int ncu = cyi_cu_count();
  if (ncu == 0) ncu = 256;
  const long long tiles = cy_ceil_div(N, 64) * cy_ceil_div(M, lin_rows_per_block(M));
  long long S = cy_ceil_div(2ll * ncu, tiles);               // two blocks of four waves per CU
  const long long by_bytes = K / (4ll * M), by_len = cy_ceil_div(K, LIN_SLICE_MIN);
  if (S > by_bytes) S = by_bytes;                            // partials [S][M][N] at most a quarter of W[N][K]
  if (S > by_len) S = by_len;
  if (S > LIN_MAX_SHARES) S = LIN_MAX_SHARES;
  if (S < 1) S = 1;
  const long long sl = cy_ceil_div(cy_ceil_div(K, S), LIN_SLICE_UNIT) * LIN_SLICE_UNIT;
  *slice = (int)sl;
  *shares = (int)cy_ceil_div(K, sl);
}

// ---- softmax cross-entropy: one block, wave w takes the rows w, w + 16, ...; a row's maximum and sum are wave reductions (fixed
// order), a wave adds its rows in ascending order, thread 0 the 16 waves in ascending order.
constexpr int XT = 1024;
__global__ __launch_bounds__(XT) void softmax_xent_kernel(const float* __restrict__ scores, const long long* __restrict__ y,
                                                          float* loss_out, float* __restrict__ dscores, int M, int C) {
  __shared__ float red[XT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float invM = 1.f / (float)M;
  float local = 0.f;
  for (int m = wave; m < M; m += XT / 64) {
    const float* s = scores + (long long)m * C;
    float* d = dscores + (long long)m * C;
    const long long lab = y[m];
    float mx = -INFINITY;
    for (int j = lane; j < C; j += 64) mx = fmaxf(mx, s[j]);
    mx = wave_allmax(mx);
    float sum = 0.f, tgt = 0.f;
    for (int j = lane; j < C; j += 64) {
      const float v = s[j] - mx;
      sum += expf(v);
      if ((long long)j == lab) tgt = v;                      // a label outside 0 .. C-1 reads nothing and adds no target term
    }
    sum = wave_allsum(sum);
    tgt = wave_allsum(tgt);
    local += logf(sum) - tgt;
    const float inv = 1.f / sum;
    for (int j = lane; j < C; j += 64) d[j] = (expf(s[j] - mx) * inv - ((long long)j == lab ? 1.f : 0.f)) * invM;
  }
  if (lane == 0) red[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) {
    float t = 0.f;
    for (int w = 0; w < XT / 64; ++w) t += red[w];
    *loss_out = t * invM;
  }
}

}  // namespace

extern "C" int cy_linear_fwd_shares(int M, int N, int K) {
  if (!lin_shape_ok(M, N, K)) return -1;
  int S, sl;
  lin_fwd_plan(M, N, K, &S, &sl);
  return S;
}

extern "C" int cy_linear_fwd_slice(int M, int N, int K) {
  if (!lin_shape_ok(M, N, K)) return -1;
  int S, sl;
  lin_fwd_plan(M, N, K, &S, &sl);
  return sl;
}

extern "C" long long cy_linear_fwd_ws_floats(int M, int N, int K) {
  if (!lin_shape_ok(M, N, K)) return -1;
  int S, sl;
  lin_fwd_plan(M, N, K, &S, &sl);
  return S > 1 ? (long long)S * M * N : 0;
}

extern "C" int cy_linear_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, int act, float* ws,
                             void* stream) {
  CY_REQUIRE(lin_shape_ok(M, N, K), "cy_linear_fwd: M=%d N=%d K=%d outside M 1..%d, N 1..%d, K a multiple of 4 up to %d", M, N, K,
             LIN_MAX_M, LIN_MAX_N, LIN_MAX_K);
  CY_REQUIRE(X && W && Y && (act == 0 || act == 1), "cy_linear_fwd: bad arguments");
  CY_REQUIRE(aligned16(X) && aligned16(W), "cy_linear_fwd: X and W must be 16-byte aligned");
  int S, slice;
  lin_fwd_plan(M, N, K, &S, &slice);
  CY_REQUIRE(S == 1 || ws, "cy_linear_fwd: %d shares need the workspace of cy_linear_fwd_ws_floats", S);
  hipStream_t s = (hipStream_t)stream;
  const int rows = lin_rows_per_block(M);
  const dim3 grid((unsigned)cy_ceil_div(N, 64), (unsigned)cy_ceil_div(M, rows), (unsigned)S);
  const int direct = S == 1;
  float* out = direct ? Y : ws;
  if (rows == 16) linear_fwd_kernel<1><<<grid, 256, 0, s>>>(X, W, bias, out, M, N, K, slice, act, direct);
  else if (rows == 32) linear_fwd_kernel<2><<<grid, 256, 0, s>>>(X, W, bias, out, M, N, K, slice, act, direct);
  else linear_fwd_kernel<4><<<grid, 256, 0, s>>>(X, W, bias, out, M, N, K, slice, act, direct);
  CY_LAUNCH_CHECK("cy_linear_fwd");
  if (!direct) {
    linear_reduce_kernel<<<(unsigned)cy_ceil_div((long long)M * N, 64), 64 * RED_PARTS, 0, s>>>(ws, bias, Y, M * N, N, S, act);
    CY_LAUNCH_CHECK("cy_linear_fwd (reduce)");
  }
  return 0;
}

extern "C" int cy_linear_dgrad(const float* dY, const float* W, float* dX, const float* X, int M, int N, int K, void* stream) {
  CY_REQUIRE(lin_shape_ok(M, N, K), "cy_linear_dgrad: M=%d N=%d K=%d outside M 1..%d, N 1..%d, K a multiple of 4 up to %d", M, N, K,
             LIN_MAX_M, LIN_MAX_N, LIN_MAX_K);
  CY_REQUIRE(dY && W && dX, "cy_linear_dgrad: bad arguments");
  CY_REQUIRE(aligned16(W) && aligned16(dX) && aligned16(X), "cy_linear_dgrad: W, dX and X must be 16-byte aligned");
  return out_product("cy_linear_dgrad", dY, N, 1, W, dX, X, M, N, K, (hipStream_t)stream);
}

extern "C" int cy_linear_wgrad(const float* dY, const float* X, float* dW, float* db, int M, int N, int K, void* stream) {
  CY_REQUIRE(lin_shape_ok(M, N, K), "cy_linear_wgrad: M=%d N=%d K=%d outside M 1..%d, N 1..%d, K a multiple of 4 up to %d", M, N, K,
             LIN_MAX_M, LIN_MAX_N, LIN_MAX_K);
  CY_REQUIRE(dY && X && dW, "cy_linear_wgrad: bad arguments");
  CY_REQUIRE(aligned16(X) && aligned16(dW), "cy_linear_wgrad: X and dW must be 16-byte aligned");
  if (int rc = out_product("cy_linear_wgrad", dY, 1, N, X, dW, nullptr, N, M, K, (hipStream_t)stream)) return rc;
  if (db) {
    linear_db_kernel<<<(unsigned)cy_ceil_div(N, 256), 256, 0, (hipStream_t)stream>>>(dY, db, M, N);
    CY_LAUNCH_CHECK("cy_linear_wgrad (db)");
  }
  return 0;
}

extern "C" int cy_softmax_xent(const float* scores, const long long* y, float* loss, float* dscores, int M, int C, void* stream) {
  CY_REQUIRE(M >= 1 && M <= LIN_MAX_M && C >= 1 && C <= LIN_MAX_C, "cy_softmax_xent: M=%d C=%d outside M 1..%d, C 1..%d", M, C,
             LIN_MAX_M, LIN_MAX_C);
  CY_REQUIRE(scores && y && loss && dscores, "cy_softmax_xent: bad arguments");
  softmax_xent_kernel<<<1, XT, 0, (hipStream_t)stream>>>(scores, y, loss, dscores, M, C);
  CY_LAUNCH_CHECK("cy_softmax_xent");
  return 0;
}
