// Gradient with respect to the NCHW image of a first layer (include/capsyolo_hip.h: cy_conv_image_grad).
//
//   dz[p,co]     = dy[p,co] * (act ? (act[p,co] > 0 ? 1 : slope) : 1) * (scale ? scale[co] : 1)
//   dx[b,c,y,x]  = sum_co sum_kh sum_kw dz[b, y+pad-kh, x+pad-kw, co] * W[co,c,kh,kw]           (terms off the map are absent)
//
// Form: one block of 128 threads owns a 16 x 32 tile of image pixels of one image; a thread owns 4 neighbouring pixels of one row
// and their 3 channels (12 fp32 accumulators).  The reduction over Cout runs in chunks of IG_CK channels: the chunk's dz patch
// ((16 + k - 1) x (32 + k - 1) pixels, activation derivative and BatchNorm scale applied on the load, zero off the map and past Cout)
// goes to LDS channel-major.  Per (channel, kh) a thread then reads k + 3 neighbouring dz values (16-byte LDS reads) and the wave reads
// that row's 3k weights with scalar loads (one address for every lane: SGPR operands, no LDS traffic) for 12k FMAs, issued as 6k packed
// FMAs over pairs of neighbouring pixels with the weight broadcast.  Every output element is summed by one thread in one order (co
// ascending, kh ascending, kw ascending): no atomics, no workspace, the same bits in every run.
// Edges: patch loads and the stores are predicated; nothing is read or written outside dy, act, W, scale, dx.
#include "common.h"

namespace {

constexpr int IG_TX = 32, IG_TY = 16, IG_PX = 4;          // tile of image pixels, pixels per thread along x
constexpr int IG_THREADS = (IG_TX / IG_PX) * IG_TY;       // 128
constexpr int IG_CK = 8;                                   // channels of dz per staged chunk
constexpr int IG_MAX_K = 9, IG_MAX_COUT = 1024;

template <int K> struct ig_geom {
  static constexpr int NV4 = (K + 3 + 3) / 4;              // 16-byte reads that cover the K + 3 values a thread needs of one patch row
  static constexpr int PW = IG_TX - 4 + NV4 * 4;           // patch row length (>= IG_TX + K - 1, a multiple of 4)
  static constexpr int PH = IG_TY + K - 1;
  static constexpr int PLANE = PH * PW + 4;                // + 4: neighbouring channel planes start 4 banks apart, rows stay 16-byte aligned
  static constexpr int WCH = 3 * K * K;                    // weights per output channel
  static constexpr int LDS_FLOATS = IG_CK * PLANE;
};

template <int K>
__global__ __launch_bounds__(IG_THREADS) void image_grad_kernel(const float* __restrict__ dy, const float* __restrict__ act,
                                                                const float* __restrict__ scale, const float* __restrict__ Wt,
                                                                float* __restrict__ dx, int H, int W, int Ho, int Wo, int Cout, int pad,
                                                                float slope, int tiles_x, int tiles_y) {
  typedef ig_geom<K> G;
  __shared__ __attribute__((aligned(16))) float lds[G::LDS_FLOATS];
  float* const patch = lds;

  int t = blockIdx.x;
  const int tx_tile = t % tiles_x;
  t /= tiles_x;
  const int ty_tile = t % tiles_y;
  const int b = t / tiles_y;
  const int x0 = tx_tile * IG_TX, y0 = ty_tile * IG_TY;
  const int tid = threadIdx.x;
  const int tx4 = tid % (IG_TX / IG_PX), ty = tid / (IG_TX / IG_PX);
  // patch pixel (py, px) is dz pixel (y0 + pad - (K - 1) + py, x0 + pad - (K - 1) + px)
  const int oy0 = y0 + pad - (K - 1), ox0 = x0 + pad - (K - 1);
  constexpr int PWU = IG_TX + K - 1;                       // patch columns that are used
  const long long img = (long long)b * Ho * Wo;

  // accumulators as pairs of neighbouring pixels: one packed FMA (v_pk_fma_f32) per pair, the weight broadcast to both halves
  f32x2 acc[3][IG_PX / 2];
#pragma unroll
  for (int ch = 0; ch < 3; ++ch)
#pragma unroll
    for (int p = 0; p < IG_PX / 2; ++p) acc[ch][p] = f32x2{0.f, 0.f};

  for (int c0 = 0; c0 < Cout; c0 += IG_CK) {
    __syncthreads();                                       // the previous chunk has been consumed
    // ---- the chunk's dz patch: lanes run over the channels of a pixel first (contiguous in dy), then over pixels
    for (int e = tid; e < G::PH * PWU * IG_CK; e += IG_THREADS) {
      const int c = e % IG_CK, p = e / IG_CK;
      const int py = p / PWU, px = p - py * PWU;
      const int oy = oy0 + py, ox = ox0 + px, co = c0 + c;
      float v = 0.f;
      if (oy >= 0 && oy < Ho && ox >= 0 && ox < Wo && co < Cout) {
        const long long o = (img + (long long)oy * Wo + ox) * Cout + co;
        v = dy[o];
        if (act) v *= act[o] > 0.f ? 1.f : slope;
        if (scale) v *= scale[co];
      }
      patch[c * G::PLANE + py * G::PW + px] = v;
    }
    __syncthreads();
    // ---- the chunk's weights W[co][3][K][K] come straight from memory: their address is the same for every lane, so they are
    // scalar loads into SGPRs (the constant cache holds the 3 k^2 Cout floats), not LDS traffic
    const int nc = Cout - c0 < IG_CK ? Cout - c0 : IG_CK;
#pragma unroll 1
    for (int c = 0; c < nc; ++c) {
      const float* const pc = patch + c * G::PLANE;
      const float* const wc = Wt + (long long)(c0 + c) * G::WCH;
#pragma unroll 1                                            // (one kh at a time: its 3 K weights fit the SGPRs; unrolled, all 3 K K spill)
      for (int kh = 0; kh < K; ++kh) {
        // output row ty takes dz row ty + pad - kh, patch row ty + (K - 1) - kh
        const f32x4* const row = reinterpret_cast<const f32x4*>(pc + (ty + (K - 1) - kh) * G::PW + tx4 * IG_PX);
        // the row's values as pairs at even offsets (de) and at odd offsets (dd): every pair a packed FMA reads is one of them
        f32x2 de[G::NV4 * 2], dd[G::NV4 * 2 - 1];
#pragma unroll
        for (int j = 0; j < G::NV4; ++j) {
          const f32x4 q = row[j];
          de[2 * j] = f32x2{q[0], q[1]}, de[2 * j + 1] = f32x2{q[2], q[3]};
        }
#pragma unroll
        for (int j = 0; j < G::NV4 * 2 - 1; ++j) dd[j] = f32x2{de[j][1], de[j + 1][0]};
#pragma unroll
        for (int kw = 0; kw < K; ++kw) {
          const float w[3] = {wc[kh * K + kw], wc[K * K + kh * K + kw], wc[2 * K * K + kh * K + kw]};
          const int o = (K - 1) - kw;                      // output column x takes dz column x + pad - kw: pixel i reads d[i + o]
#pragma unroll
          for (int p = 0; p < IG_PX / 2; ++p) {
            const f32x2 dv = (o & 1) ? dd[p + o / 2] : de[p + o / 2];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) acc[ch][p] = __builtin_elementwise_fma(dv, f32x2{w[ch], w[ch]}, acc[ch][p]);
          }
        }
      }
    }
  }
  const int y = y0 + ty;
  if (y < H) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float* const o = dx + (((long long)b * 3 + ch) * H + y) * W;
#pragma unroll
      for (int i = 0; i < IG_PX; ++i) {
        const int x = x0 + tx4 * IG_PX + i;
        if (x < W) o[x] = acc[ch][i / 2][i % 2];
      }
    }
  }
}

bool ig_shape_ok(int B, int H, int W, int Cout, int k, int pad) {
  if (B < 1 || H < 1 || W < 1 || Cout < 1 || Cout > IG_MAX_COUT) return false;
  if (k < 1 || k > IG_MAX_K || k % 2 == 0 || pad < 0 || pad > k / 2) return false;
  if (H + 2 * pad < k || W + 2 * pad < k) return false;                 // the forward has at least one output pixel
  const long long blocks = (long long)B * cy_ceil_div(H, IG_TY) * cy_ceil_div(W, IG_TX);
  return blocks < (1ll << 31) && (long long)B * 3 * H * W < (1ll << 40);
}

template <int K>
int ig_launch(const float* dy, const float* act, const float* scale, const float* Wt, float* dx, int B, int H, int W, int Cout, int pad,
              float slope, hipStream_t s) {
  const int tiles_x = (int)cy_ceil_div(W, IG_TX), tiles_y = (int)cy_ceil_div(H, IG_TY);
  const int Ho = H + 2 * pad - K + 1, Wo = W + 2 * pad - K + 1;
  image_grad_kernel<K><<<(unsigned)((long long)B * tiles_x * tiles_y), IG_THREADS, 0, s>>>(dy, act, scale, Wt, dx, H, W, Ho, Wo, Cout, pad,
                                                                                             slope, tiles_x, tiles_y);
  CY_LAUNCH_CHECK("cy_conv_image_grad");
  return 0;
}

}  // namespace

extern "C" int cy_conv_image_grad_ok(int B, int H, int W, int Cout, int k, int pad) { return ig_shape_ok(B, H, W, Cout, k, pad) ? 1 : 0; }

extern "C" int cy_conv_image_grad(const float* dy, const float* act, const float* scale, const float* Wt, float* dx, int B, int H, int W,
                                  int Cin, int Cout, int k, int pad, float slope, void* stream) {
  CY_REQUIRE(Cin == 3, "cy_conv_image_grad: Cin=%d, the image gradient is built for 3 input channels", Cin);
  CY_REQUIRE(ig_shape_ok(B, H, W, Cout, k, pad),
             "cy_conv_image_grad: B=%d H=%d W=%d Cout=%d k=%d pad=%d outside Cout 1..%d, k odd in 1..%d, pad 0..k/2, H and W >= k - 2 pad", B,
             H, W, Cout, k, pad, IG_MAX_COUT, IG_MAX_K);
  CY_REQUIRE(dy && Wt && dx, "cy_conv_image_grad: bad arguments");
  CY_REQUIRE(!act || (slope >= 0.f && slope <= 1.f), "cy_conv_image_grad: slope %g outside [0, 1] (the sign of act is the sign of z only there)",
             (double)slope);
  hipStream_t s = (hipStream_t)stream;
  switch (k) {
    case 1: return ig_launch<1>(dy, act, scale, Wt, dx, B, H, W, Cout, pad, slope, s);
    case 3: return ig_launch<3>(dy, act, scale, Wt, dx, B, H, W, Cout, pad, slope, s);
    case 5: return ig_launch<5>(dy, act, scale, Wt, dx, B, H, W, Cout, pad, slope, s);
    case 7: return ig_launch<7>(dy, act, scale, Wt, dx, B, H, W, Cout, pad, slope, s);
    default: return ig_launch<9>(dy, act, scale, Wt, dx, B, H, W, Cout, pad, slope, s);
  }
}
