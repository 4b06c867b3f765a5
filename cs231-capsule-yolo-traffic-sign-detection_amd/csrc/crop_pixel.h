// The per-pixel body of crop + bilinear resize + affine, shared by crop_resize_kernel (predict.hip, rectangles from the host)
// and boxes_crop_resize_kernel (serve.hip, rectangles computed on the device), each for packed RGB and for NV12 images: one copy of
// the interpolation, so all four give the same bits on the same pixel values.
#pragma once
#include "common.h"

// the arithmetic below (and the double arithmetic of the units that include this) restates numpy / cv2 expressions operation by
// operation: no fused multiply-add
#pragma clang fp contract(off)

struct __attribute__((packed, aligned(4))) cyi_float3s { float x, y, z; };

// ---- where a tap comes from.  A fetch policy hands cyi_crop_pixel the three channel values of the four taps (rows ya / yb, columns
// xa / xb of ONE image, frame coordinates) as exact floats 0..255; everything behind that is the one interpolation body below.

// packed HWC uint8, W pixels wide
struct cyi_fetch_rgb {
  const unsigned char* __restrict__ base;
  int W;
  __device__ __forceinline__ void taps(int ya, int yb, int xa, int xb, float t[4][3]) const {
    const unsigned char* paa = base + ((long long)ya * W + xa) * 3;
    const unsigned char* pab = base + ((long long)ya * W + xb) * 3;
    const unsigned char* pba = base + ((long long)yb * W + xa) * 3;
    const unsigned char* pbb = base + ((long long)yb * W + xb) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { t[0][c] = (float)paa[c]; t[1][c] = (float)pab[c]; t[2][c] = (float)pba[c]; t[3][c] = (float)pbb[c]; }
  }
};

// the colour rule of include/capsyolo_hip.h (NV12 section): one (Y, U, V) triple to the rounded, clamped RGB bytes, all in int32;
// >> on a negative int is the arithmetic shift (floor)
__device__ __forceinline__ void cyi_yuv_to_rgb(const cy_yuv_coef_t& k, int Y, int U, int V, int rgb[3]) {
  const int y = max(Y - k.y_off, 0) * k.cy, u = U - 128, v = V - 128;
  rgb[0] = min(max((y + k.cvr * v + (1 << 19)) >> 20, 0), 255);
  rgb[1] = min(max((y - k.cug * u - k.cvg * v + (1 << 19)) >> 20, 0), 255);
  rgb[2] = min(max((y + k.cub * u + (1 << 19)) >> 20, 0), 255);
}

// host side: a coefficient row whose every value before the shift stays inside int32 for all (Y, U, V) bytes
static inline bool cyi_yuv_coef_ok(const cy_yuv_coef_t& k) {
  const auto mag = [](int v) { return v < 0 ? -(long long)v : (long long)v; };
  const long long c = mag(k.cvr) > mag(k.cub) ? mag(k.cvr) : mag(k.cub), g = mag(k.cug) + mag(k.cvg);
  return k.y_off >= 0 && k.y_off <= 255 && 255 * mag(k.cy) + 128 * (c > g ? c : g) + (1 << 19) <= 0x7fffffffll;
}
#define CYI_YUV_COEF_MSG "coefficients (%d, %d, %d, %d, %d, %d): y_off must be in 0..255 and 255 |cy| + 128 max(|cvr|, |cug| + |cvg|, |cub|) + 2^19 inside int32"
#define CYI_YUV_COEF_ARGS(k) (k).y_off, (k).cy, (k).cvr, (k).cug, (k).cvg, (k).cub

// NV12: a Y plane and an interleaved half-resolution UV plane of one row pitch.  Byte loads only: no alignment is assumed.  The
// chroma pair of a tap is indexed by the tap's FRAME coordinate (y >> 1, x >> 1); the two columns of a tap pair, and the two rows,
// fall into one 2 x 2 block about every other time, and then the pair is not loaded again.
struct cyi_fetch_nv12 {
  const unsigned char* __restrict__ luma;      // Y sample (0, 0)
  const unsigned char* __restrict__ chroma;    // U of block (0, 0)
  int pitch;
  cy_yuv_coef_t k;
  __device__ __forceinline__ void taps(int ya, int yb, int xa, int xb, float t[4][3]) const {
    const long long la = (long long)ya * pitch, lb = (long long)yb * pitch;
    const int Y[4] = {luma[la + xa], luma[la + xb], luma[lb + xa], luma[lb + xb]};
    const long long ca = (long long)(ya >> 1) * pitch, cb = (long long)(yb >> 1) * pitch;
    const int xa2 = 2 * (xa >> 1), xb2 = 2 * (xb >> 1);
    const bool same_col = xa2 == xb2, same_row = ca == cb;
    int U[4], V[4];
    U[0] = chroma[ca + xa2]; V[0] = chroma[ca + xa2 + 1];
    if (same_col) { U[1] = U[0]; V[1] = V[0]; } else { U[1] = chroma[ca + xb2]; V[1] = chroma[ca + xb2 + 1]; }
    if (same_row) { U[2] = U[0]; V[2] = V[0]; U[3] = U[1]; V[3] = V[1]; }
    else {
      U[2] = chroma[cb + xa2]; V[2] = chroma[cb + xa2 + 1];
      if (same_col) { U[3] = U[2]; V[3] = V[2]; } else { U[3] = chroma[cb + xb2]; V[3] = chroma[cb + xb2 + 1]; }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      int rgb[3];
      cyi_yuv_to_rgb(k, Y[i], U[i], V[i], rgb);
      t[i][0] = (float)rgb[0]; t[i][1] = (float)rgb[1]; t[i][2] = (float)rgb[2];
    }
  }
};

// ---- where an image comes from: the packed buffer's tables.  image(k, H, W, f) reads image k's size, builds its fetch policy and
// says whether the image is well formed and lies inside the buffer (a caller reads no byte of one that does not).  k is in range.
struct cyi_images_rgb {
  typedef cyi_fetch_rgb fetch_t;
  const unsigned char* __restrict__ imgs;
  const long long* __restrict__ img_off;
  const int* __restrict__ img_hw;             // [n][2] = (H, W)
  long long imgs_bytes;
  __device__ __forceinline__ bool image(int k, int& H, int& W, fetch_t& f) const {
    H = img_hw[2 * k]; W = img_hw[2 * k + 1];
    const long long off = img_off[k];
    f.base = imgs + off; f.W = W;
    return H > 0 && W > 0 && off >= 0 && off + (long long)H * W * 3 <= imgs_bytes;
  }
};

struct cyi_images_nv12 {
  typedef cyi_fetch_nv12 fetch_t;
  const unsigned char* __restrict__ imgs;
  const long long* __restrict__ img_off;
  const int* __restrict__ img_geom;           // [n][4] = (H, W, pitch, uv_off)
  long long imgs_bytes;
  cy_yuv_coef_t k;
  __device__ __forceinline__ bool image(int i, int& H, int& W, fetch_t& f) const {
    H = img_geom[4 * i]; W = img_geom[4 * i + 1];
    const int pitch = img_geom[4 * i + 2], uv_off = img_geom[4 * i + 3];
    const long long off = img_off[i];
    f.luma = imgs + off; f.chroma = imgs + off + uv_off; f.pitch = pitch; f.k = k;
    return H > 0 && W > 0 && (long long)pitch >= 2 * (((long long)W + 1) >> 1) && (long long)uv_off >= (long long)H * pitch && off >= 0 &&
           off + uv_off + (((long long)H + 1) >> 1) * pitch <= imgs_bytes;
  }
};

// Output pixel (oy, ox) of the half-open rectangle (y0, y1, x0, x1) of the image behind `f`, resized as a
// stand-alone image to OH x OW with the half-pixel convention of cv2's INTER_LINEAR: source coordinate
// s = (o + 0.5) * n_in / n_out - 0.5, rows floor(s) and floor(s) + 1 clamped into the crop.  The coordinate is kept as the exact
// fraction ((2 o + 1) n_in - n_out) / (2 n_out), so the only rounding of the weight is the final division; the interpolation
// itself is fp32 (cv2's 11-bit fixed-point weights are not reproduced).  v[c] = (value + shift) * scale.  The caller has checked
// that the rectangle is not empty and lies inside the image.
template <class Fetch>
__device__ __forceinline__ void cyi_crop_pixel(const Fetch& f, int y0, int y1, int x0, int x1, int oy, int ox,
                                               int OH, int OW, float shift, float scale, float v[3]) {
  const int ch = y1 - y0, cw = x1 - x0;
  const long long ny = (long long)(2 * oy + 1) * ch - OH, nx = (long long)(2 * ox + 1) * cw - OW;
  // floor division (the numerator is negative for the first outputs of an upscale)
  long long ry = ny / (2 * OH), rx = nx / (2 * OW);
  if (ny < 0 && ry * 2 * OH != ny) --ry;
  if (nx < 0 && rx * 2 * OW != nx) --rx;
  const float fy = (float)(ny - ry * 2 * OH) / (float)(2 * OH), fx = (float)(nx - rx * 2 * OW) / (float)(2 * OW);
  const int ra = (int)min(max(ry, 0ll), (long long)ch - 1), rb = (int)min(max(ry + 1, 0ll), (long long)ch - 1);
  const int ca = (int)min(max(rx, 0ll), (long long)cw - 1), cb = (int)min(max(rx + 1, 0ll), (long long)cw - 1);
  float t[4][3];
  f.taps(y0 + ra, y0 + rb, x0 + ca, x0 + cb, t);
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float aa = t[0][c], ab = t[1][c], ba = t[2][c], bb = t[3][c];
    const float top = aa + fx * (ab - aa), bot = ba + fx * (bb - ba);
    v[c] = (top + fy * (bot - top) + shift) * scale;
  }
}

// pixel i = (b, oy, ox) of out[n][OH][OW][3] (one 12-byte store), or of [n][3][OH][OW] with to_nchw
__device__ __forceinline__ void cyi_store_pixel(float* __restrict__ out, long long i, long long b, int oy, int ox, int OH, int OW, int to_nchw,
                                                float r, float g, float bl) {
  if (to_nchw) {
    const long long plane = (long long)OH * OW, o = b * 3 * plane + (long long)oy * OW + ox;
    out[o] = r; out[o + plane] = g; out[o + 2 * plane] = bl;
  } else {
    cyi_float3s px; px.x = r; px.y = g; px.z = bl;
    *(cyi_float3s*)(out + 3 * i) = px;
  }
}
