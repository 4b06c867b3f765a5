// The per-pixel body of crop + bilinear resize + affine, shared by crop_resize_u8_kernel (predict.hip, rectangles from the host)
// and boxes_crop_resize_u8_kernel (serve.hip, rectangles computed on the device): one copy, so both give the same bits.
#pragma once
#include "common.h"

// the arithmetic below (and the double arithmetic of the units that include this) restates numpy / cv2 expressions operation by
// operation: no fused multiply-add
#pragma clang fp contract(off)

struct __attribute__((packed, aligned(4))) cyi_float3s { float x, y, z; };

// Output pixel (oy, ox) of the half-open rectangle (y0, y1, x0, x1) of the HWC uint8 image at `base` (W pixels wide), resized as a
// stand-alone image to OH x OW with the half-pixel convention of cv2's INTER_LINEAR: source coordinate
// s = (o + 0.5) * n_in / n_out - 0.5, rows floor(s) and floor(s) + 1 clamped into the crop.  The coordinate is kept as the exact
// fraction ((2 o + 1) n_in - n_out) / (2 n_out), so the only rounding of the weight is the final division; the interpolation
// itself is fp32 (cv2's 11-bit fixed-point weights are not reproduced).  v[c] = (value + shift) * scale.  The caller has checked
// that the rectangle is not empty and lies inside the image.
__device__ __forceinline__ void cyi_crop_pixel(const unsigned char* __restrict__ base, int W, int y0, int y1, int x0, int x1, int oy, int ox,
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
  const unsigned char* paa = base + ((long long)(y0 + ra) * W + (x0 + ca)) * 3;
  const unsigned char* pab = base + ((long long)(y0 + ra) * W + (x0 + cb)) * 3;
  const unsigned char* pba = base + ((long long)(y0 + rb) * W + (x0 + ca)) * 3;
  const unsigned char* pbb = base + ((long long)(y0 + rb) * W + (x0 + cb)) * 3;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float aa = (float)paa[c], ab = (float)pab[c], ba = (float)pba[c], bb = (float)pbb[c];
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
