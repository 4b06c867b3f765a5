// The CapsuleNet decoder forward (models.py:96-111) in ONE launch, for capsule interpretation (capsule_interpret.py:54-68) and
// reconstruction outside the training loss: Linear(16,256) ReLU UnFlatten(16,4,4), three times nearest Upsample x2 + 3x3 conv + ReLU
// (16->4 at 8^2, 4->8 at 16^2, 8->16 at 32^2), 3x3 conv 16->3 at 32^2, tanh.  3.4 MFLOP and 6 831 parameters per vector: every
// intermediate of one vector and all weights stay in the LDS of one CU.  The training decoder
// (models.Decoder.forward, per-layer launches with a backward) is not touched.
#include "common.h"

namespace {

constexpr int DEC_THREADS = 1024;     // 16 waves, 4 per SIMD; one workgroup per CU (104 KB of LDS)

// LDS carve in floats; every offset is a multiple of 4 (16-byte pieces are read from the weight images).
// Weights are transposed while they are staged: the linear layer to [16 j][256 k] (lane k reads bank k), a convolution from OIHW to
// [ci][tap][co padded to 4] (the co of one tap are one or more 16-byte pieces at a wave-uniform address: a broadcast read).
constexpr int L_WL = 0;                    // Linear weight  [16][256]
constexpr int L_BL = L_WL + 16 * 256;      // Linear bias    [256]
constexpr int L_W1 = L_BL + 256;           // decoder.4   [16*9][4]
constexpr int L_B1 = L_W1 + 16 * 9 * 4;
constexpr int L_W2 = L_B1 + 4;             // decoder.7   [4*9][8]
constexpr int L_B2 = L_W2 + 4 * 9 * 8;
constexpr int L_W3 = L_B2 + 8;             // decoder.10  [8*9][16]
constexpr int L_B3 = L_W3 + 8 * 9 * 16;
constexpr int L_W4 = L_B3 + 16;            // decoder.12  [16*9][3 -> 4]
constexpr int L_B4 = L_W4 + 16 * 9 * 4;
constexpr int L_T = L_B4 + 4;              // the capsule vector [16]
constexpr int L_H0 = L_T + 16;             // maps, CHW: [16][4][4]
constexpr int L_H1 = L_H0 + 256;           // [4][8][8]
constexpr int L_H2 = L_H1 + 256;           // [8][16][16]
constexpr int L_H3 = L_H2 + 2048;          // [16][32][32]
constexpr int L_RED = L_H3 + 16384;        // per-wave partial sums of sqerr [16]
constexpr int L_END = L_RED + DEC_THREADS / 64;
constexpr size_t DEC_LDS_BYTES = (size_t)L_END * sizeof(float);
static_assert(DEC_LDS_BYTES <= 160 * 1024, "the decoder's LDS image must fit one CU");
static_assert(L_BL % 4 == 0 && L_W1 % 4 == 0 && L_W2 % 4 == 0 && L_W3 % 4 == 0 && L_W4 % 4 == 0 && L_H0 % 4 == 0, "16-byte carve");

// OIHW [CO][CI][3][3] in global memory -> [CI*9][COP] in LDS (columns CO .. COP-1 zero), bias -> [COP]
template <int CI, int CO>
__device__ __forceinline__ void stage_conv(const float* __restrict__ w, const float* __restrict__ b, float* lw, float* lb) {
  constexpr int COP = (CO + 3) & ~3;
  for (int i = threadIdx.x; i < CI * 9 * COP; i += DEC_THREADS) {
    const int co = i % COP, rem = i / COP;
    lw[i] = co < CO ? w[co * CI * 9 + rem] : 0.f;
  }
  for (int i = threadIdx.x; i < COP; i += DEC_THREADS) lb[i] = i < CO ? b[i] : 0.f;
}

// 3x3 convolution, zero padding 1, of a CHW map in LDS, S x S outputs.  UP: the input map is (S/2) x (S/2) and stands for its nearest
// x2 up-sampling, read as source pixel (y >> 1, x >> 1).  One work item = ROWS vertically adjacent output pixels x COT output channels
// (the ROWS + 2 input rows and every weight are read once per item); lanes run along x.  epi(y, x, co, value with bias).
template <int CI, int CO, int S, bool UP, int COT, int ROWS, typename Epi>
__device__ __forceinline__ void conv3x3(const float* in, const float* w, const float* bias, Epi epi) {
  constexpr int SI = UP ? S / 2 : S;
  constexpr int COP = (CO + 3) & ~3;
  constexpr int NG = CO / COT;
  constexpr int YR = S / ROWS;
  static_assert(CO % COT == 0 && S % ROWS == 0 && (COT % 4 == 0 || NG == 1 || COT == 1), "conv3x3: item shape");
  for (int it = threadIdx.x; it < S * YR * NG; it += DEC_THREADS) {
    const int x = it % S, y0 = (it / S) % YR * ROWS, co0 = it / (S * YR) * COT;
    float acc[ROWS][COT];
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < COT; ++c) acc[r][c] = bias[co0 + c];
    int xs[3], ys[ROWS + 2];
    bool xv[3], yv[ROWS + 2];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
      const int xx = x + d - 1;
      xv[d] = xx >= 0 && xx < S;
      xs[d] = min(max(xx, 0), S - 1) >> (UP ? 1 : 0);
    }
#pragma unroll
    for (int r = 0; r < ROWS + 2; ++r) {
      const int yy = y0 + r - 1;
      yv[r] = yy >= 0 && yy < S;
      ys[r] = (min(max(yy, 0), S - 1) >> (UP ? 1 : 0)) * SI;
    }
#pragma unroll 2
    for (int ci = 0; ci < CI; ++ci) {
      float v[ROWS + 2][3];
#pragma unroll
      for (int r = 0; r < ROWS + 2; ++r)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
          const float ld = in[ci * SI * SI + ys[r] + xs[d]];
          v[r][d] = (yv[r] && xv[d]) ? ld : 0.f;
        }
#pragma unroll
      for (int tap = 0; tap < 9; ++tap) {
        const float* wp = w + (ci * 9 + tap) * COP + co0;
        float wv[COT];
        if constexpr (COT == 3) {
          const f32x4 q = *reinterpret_cast<const f32x4*>(wp);
          wv[0] = q[0]; wv[1] = q[1]; wv[2] = q[2];
        } else if constexpr (COT % 4 == 0) {
#pragma unroll
          for (int c = 0; c < COT; c += 4) {
            const f32x4 q = *reinterpret_cast<const f32x4*>(wp + c);
            wv[c] = q[0]; wv[c + 1] = q[1]; wv[c + 2] = q[2]; wv[c + 3] = q[3];
          }
        } else {
#pragma unroll
          for (int c = 0; c < COT; ++c) wv[c] = wp[c];
        }
#pragma unroll
        for (int r = 0; r < ROWS; ++r)
#pragma unroll
          for (int c = 0; c < COT; ++c) acc[r][c] += v[r + tap / 3][tap % 3] * wv[c];
      }
    }
#pragma unroll
    for (int r = 0; r < ROWS; ++r)
#pragma unroll
      for (int c = 0; c < COT; ++c) epi(y0 + r, x, co0 + c, acc[r][c]);
  }
}

__global__ __launch_bounds__(DEC_THREADS) void decoder_fwd_kernel(cy_decoder_t a, int rows) {
  extern __shared__ __attribute__((aligned(16))) float s[];
  const int tid = threadIdx.x;
  // ---- the weights, once per block
  for (int i = tid; i < 16 * 256; i += DEC_THREADS) s[L_WL + (i & 15) * 256 + (i >> 4)] = a.lin_w[i];      // [256 k][16 j] -> [j][k]
  for (int i = tid; i < 256; i += DEC_THREADS) s[L_BL + i] = a.lin_b[i];
  stage_conv<16, 4>(a.w4, a.b4, s + L_W1, s + L_B1);
  stage_conv<4, 8>(a.w7, a.b7, s + L_W2, s + L_B2);
  stage_conv<8, 16>(a.w10, a.b10, s + L_W3, s + L_B3);
  stage_conv<16, 3>(a.w12, a.b12, s + L_W4, s + L_B4);

  const int per = a.deltas ? 16 * a.n_delta : 1;            // launch rows per source vector
  for (int row = blockIdx.x; row < rows; row += gridDim.x) {
    // ---- row = (sample b, swept component comp, offset index di): caps[b][label[b]][:] with deltas[di] added to component comp
    const int b = row / per, rem = row - b * per;
    long long src = b;
    if (a.labels) {
      const long long lab = a.labels[b];
      if (lab < 0 || lab >= a.C) {                          // block-uniform: no barrier is skipped by part of the block
        if (tid == 0) atomicAdd(a.err, 1);
        continue;
      }
      src = (long long)b * a.C + lab;
    }
    if (tid < 16) {
      float t = a.caps[src * 16 + tid];
      if (a.deltas && tid == rem / a.n_delta) t += a.deltas[rem % a.n_delta];
      s[L_T + tid] = t;
    }
    // the previous vector's last reads of h0 .. h3 and of the sqerr partials lie before its later barriers; this one also publishes
    // the weights on the first trip
    __syncthreads();
    if (tid < 256) {                                        // Linear + ReLU; element k is (channel k / 16, row k % 16 / 4, column k % 4)
      float acc = s[L_BL + tid];
#pragma unroll
      for (int j = 0; j < 16; ++j) acc += s[L_T + j] * s[L_WL + j * 256 + tid];
      s[L_H0 + tid] = fmaxf(acc, 0.f);
    }
    __syncthreads();
    conv3x3<16, 4, 8, true, 1, 1>(s + L_H0, s + L_W1, s + L_B1,
                                  [&](int y, int x, int co, float v) { s[L_H1 + co * 64 + y * 8 + x] = fmaxf(v, 0.f); });
    __syncthreads();
    conv3x3<4, 8, 16, true, 4, 1>(s + L_H1, s + L_W2, s + L_B2,
                                  [&](int y, int x, int co, float v) { s[L_H2 + co * 256 + y * 16 + x] = fmaxf(v, 0.f); });
    __syncthreads();
    conv3x3<8, 16, 32, true, 8, 2>(s + L_H2, s + L_W3, s + L_B3,
                                   [&](int y, int x, int co, float v) { s[L_H3 + co * 1024 + y * 32 + x] = fmaxf(v, 0.f); });
    __syncthreads();
    float se = 0.f;
    const float* img = a.x ? a.x + (long long)b * 3072 : nullptr;
    conv3x3<16, 3, 32, false, 3, 2>(s + L_H3, s + L_W4, s + L_B4, [&](int y, int x, int co, float v) {
      const float o = tanhf(v);
      if (a.out_f32) a.out_f32[((long long)row * 3 + co) * 1024 + y * 32 + x] = o;
      if (a.out_u8) {
        const float q = fminf(fmaxf(rintf(o * 128.f + 128.f), 0.f), 255.f);
        a.out_u8[((long long)row * 1024 + y * 32 + x) * 3 + co] = (unsigned char)(int)q;
      }
      if (a.sqerr) {
        const float d = img[co * 1024 + y * 32 + x] - o;
        se += d * d;
      }
    });
    if (a.sqerr) {        // fixed order: 6 terms per thread, the DPP tree of a wave, the 16 waves in turn
      const float ws = wave_sum(se);
      if ((tid & 63) == 0) s[L_RED + (tid >> 6)] = ws;
      __syncthreads();
      if (tid == 0) {
        float tot = 0.f;
        for (int k = 0; k < DEC_THREADS / 64; ++k) tot += s[L_RED + k];
        a.sqerr[row] = tot;
      }
    }
  }
}

}  // namespace

extern "C" int cy_decoder_fwd(const cy_decoder_t* a, void* stream) {
  CY_REQUIRE(a, "cy_decoder_fwd: null argument");
  CY_REQUIRE(a->caps && a->lin_w && a->lin_b && a->w4 && a->b4 && a->w7 && a->b7 && a->w10 && a->b10 && a->w12 && a->b12,
             "cy_decoder_fwd: null capsule or parameter pointer");
  CY_REQUIRE(a->n >= 1 && a->C >= 1, "cy_decoder_fwd: n = %d vectors of C = %d classes", a->n, a->C);
  CY_REQUIRE(a->D == 16, "cy_decoder_fwd: capsule vectors of %d floats (the decoder takes 16)", a->D);
  CY_REQUIRE(a->labels ? a->err != nullptr : a->C == 1, "cy_decoder_fwd: labels need the error word; dense rows are C = 1");
  CY_REQUIRE(a->deltas ? a->n_delta >= 1 : a->n_delta == 0, "cy_decoder_fwd: %d deltas", a->n_delta);
  CY_REQUIRE(a->out_f32 || a->out_u8 || a->sqerr, "cy_decoder_fwd: no output");
  CY_REQUIRE(!a->sqerr || a->x, "cy_decoder_fwd: sqerr needs the input images x");
  const long long rows = (long long)a->n * (a->deltas ? 16ll * a->n_delta : 1ll);
  CY_REQUIRE(rows < (1ll << 31), "cy_decoder_fwd: %lld rows are too many for one launch", rows);
  long long blocks;
  if (int rc = cyi_persistent_blocks("cy_decoder_fwd", rows, &blocks)) return rc;
  return cyi_launch_lds("cy_decoder_fwd", decoder_fwd_kernel, dim3((unsigned)blocks), dim3(DEC_THREADS), DEC_LDS_BYTES,
                        (hipStream_t)stream, *a, (int)rows);
}
