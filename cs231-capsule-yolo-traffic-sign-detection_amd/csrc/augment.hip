// Sign-paste augmentation and the data-set resize on the device (gfx950): build_data.py:80 (cv2.resize of a frame), 28-29 + 44
// (ROI crop of a GTSRB sign, resized) and 171-288 (gtsdb_aug_: signs pasted over a frame, then the frame resized) as ONE kernel
// that never forms the composited frame.  DESIGN section 6h.
//   paste_resize_u8_kernel   output sample = resize(source rectangle of (background with the sample's pastes applied in order))
// The classifiers' augmentation (utils.py:126-143: shift with zero fill, lightness increase) as one gather kernel.  DESIGN section 6i.
//   gather_jitter_u8_kernel  output sample = centre(brighten(shift(resident image index[b]))), NHWC bytes -> NCHW floats
#include "common.h"

namespace {

enum { MAX_PASTES = 64, PASTE_INTS = 9, MAX_SIDE = 1 << 24 };

// One staged paste: the sign's ROI (origin, size, row pitch, byte offset in the sign buffer) and the destination rectangle.
struct Paste { long long off; int sy0, sx0, sh, sw, W, dy0, dy1, dx0, dx1; };

// One axis of the half-pixel sampling rule in integers: source coordinate ((2 o + 1) n_in - n_out) / (2 n_out) = r + w / (2 n_out)
// with r = floor(..) and 0 <= w < 2 n_out; the taps r and r + 1 are clamped into [0, n_in).
struct Axis { int lo, hi; long long w; };
__device__ __forceinline__ Axis axis_taps(int o, int n_out, int n_in) {
  const long long num = (2ll * o + 1) * n_in - n_out, den = 2ll * n_out;
  long long r = num / den;
  if (num < 0 && r * den != num) --r;                                // floor: the numerator is negative for the first outputs of an upscale
  Axis a;
  a.w = num - r * den;
  a.lo = (int)min(max(r, 0ll), (long long)n_in - 1);
  a.hi = (int)min(max(r + 1, 0ll), (long long)n_in - 1);
  return a;
}
// round-half-up of the exact bilinear value: all operands below 2^24, so every product stays below 2^58
__device__ __forceinline__ int blend(const Axis& y, const Axis& x, int oh, int ow, int aa, int ab, int ba, int bb) {
  const long long a = y.w, b = x.w, na = 2ll * oh - a, nb = 2ll * ow - b;
  return (int)((nb * na * aa + b * na * ab + nb * a * ba + b * a * bb + 2ll * ow * oh) / (4ll * ow * oh));
}

// Pixel (y, x) of the composited frame: the last paste whose destination holds it, resized there as a stand-alone image
// (a byte), else the background.
__device__ __forceinline__ void frame_tap(const unsigned char* __restrict__ bg, int W, int y, int x, const Paste* sp, int cnt,
                                          const unsigned char* __restrict__ signs, int v[3]) {
  for (int k = cnt - 1; k >= 0; --k) {
    const Paste& p = sp[k];
    if (y < p.dy0 || y >= p.dy1 || x < p.dx0 || x >= p.dx1) continue;
    const int dh = p.dy1 - p.dy0, dw = p.dx1 - p.dx0;
    const Axis ay = axis_taps(y - p.dy0, dh, p.sh), ax = axis_taps(x - p.dx0, dw, p.sw);
    const unsigned char* base = signs + p.off;
    const unsigned char* paa = base + ((long long)(p.sy0 + ay.lo) * p.W + (p.sx0 + ax.lo)) * 3;
    const unsigned char* pab = base + ((long long)(p.sy0 + ay.lo) * p.W + (p.sx0 + ax.hi)) * 3;
    const unsigned char* pba = base + ((long long)(p.sy0 + ay.hi) * p.W + (p.sx0 + ax.lo)) * 3;
    const unsigned char* pbb = base + ((long long)(p.sy0 + ay.hi) * p.W + (p.sx0 + ax.hi)) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend(ay, ax, dh, dw, paa[c], pab[c], pba[c], pbb[c]);
    return;
  }
  const unsigned char* q = bg + ((long long)y * W + x) * 3;
  v[0] = q[0]; v[1] = q[1]; v[2] = q[2];
}

struct __attribute__((packed, aligned(4))) float3s { float x, y, z; };

// Grid (pixel tiles, samples): the sample and its paste slice are uniform per block.  The first threads check and stage one
// paste each in LDS; a sample with anything out of range is zero-filled and counted once (by its first tile).
__global__ __launch_bounds__(256) void paste_resize_u8_kernel(
    const unsigned char* __restrict__ imgs, const long long* __restrict__ img_off, const int* __restrict__ img_hw, int n_images,
    long long imgs_bytes, const unsigned char* __restrict__ signs, const long long* __restrict__ sign_off,
    const int* __restrict__ sign_hw, int n_signs, long long signs_bytes, const int* __restrict__ sample_img,
    const int* __restrict__ sample_rect, const int* __restrict__ begin, const int* __restrict__ pastes, int n_pastes, int OH, int OW,
    int mode, void* __restrict__ out, int* err) {
  __shared__ Paste sp[MAX_PASTES];
  __shared__ int bad_s;
  const int t = threadIdx.x, s = blockIdx.y;
  if (t == 0) bad_s = 0;
  __syncthreads();
  const int img = sample_img[s];
  const int b0 = begin[s], b1 = begin[s + 1];
  bool ok = img >= 0 && img < n_images && b0 >= 0 && b0 <= b1 && b1 <= n_pastes && b1 - b0 <= MAX_PASTES;
  int H = 0, W = 0, y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  long long off = 0;
  if (ok) {
    H = img_hw[2 * img];
    W = img_hw[2 * img + 1];
    off = img_off[img];
    y0 = sample_rect[4 * s]; y1 = sample_rect[4 * s + 1]; x0 = sample_rect[4 * s + 2]; x1 = sample_rect[4 * s + 3];
    ok = H >= 1 && W >= 1 && H < MAX_SIDE && W < MAX_SIDE && off >= 0 && off + (long long)H * W * 3 <= imgs_bytes &&
         y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W;
  }
  const int cnt = ok ? b1 - b0 : 0;
  if (t < cnt) {
    const int* row = pastes + (long long)(b0 + t) * PASTE_INTS;
    const int sg = row[0];
    bool pok = sg >= 0 && sg < n_signs;
    Paste p = {};
    if (pok) {
      const int SH = sign_hw[2 * sg], SW = sign_hw[2 * sg + 1];
      p.off = sign_off[sg];
      p.W = SW;
      p.sy0 = row[1]; p.sx0 = row[3];
      p.dy0 = row[5]; p.dy1 = row[6]; p.dx0 = row[7]; p.dx1 = row[8];
      pok = SH >= 1 && SW >= 1 && SH < MAX_SIDE && SW < MAX_SIDE && p.off >= 0 && p.off + (long long)SH * SW * 3 <= signs_bytes &&
            row[1] >= 0 && row[1] < row[2] && row[2] <= SH && row[3] >= 0 && row[3] < row[4] && row[4] <= SW &&
            p.dy0 >= 0 && p.dy0 < p.dy1 && p.dy1 <= H && p.dx0 >= 0 && p.dx0 < p.dx1 && p.dx1 <= W;
      if (pok) { p.sh = row[2] - row[1]; p.sw = row[4] - row[3]; }
    }
    if (pok) sp[t] = p;
    else bad_s = 1;                                                  // every writer stores the same value
  }
  __syncthreads();
  if (bad_s) ok = false;
  if (!ok && blockIdx.x == 0 && t == 0) atomicAdd(err, 1);           // one count per bad sample

  const long long plane = (long long)OH * OW, i = (long long)blockIdx.x * 256 + t;
  if (i >= plane) return;
  const int oy = (int)(i / OW), ox = (int)(i - (long long)oy * OW);
  int v[3] = {0, 0, 0};
  if (ok) {
    const Axis ay = axis_taps(oy, OH, y1 - y0), ax = axis_taps(ox, OW, x1 - x0);
    const unsigned char* bg = imgs + off;
    int aa[3], ab[3], ba[3], bb[3];
    frame_tap(bg, W, y0 + ay.lo, x0 + ax.lo, sp, cnt, signs, aa);
    frame_tap(bg, W, y0 + ay.lo, x0 + ax.hi, sp, cnt, signs, ab);
    frame_tap(bg, W, y0 + ay.hi, x0 + ax.lo, sp, cnt, signs, ba);
    frame_tap(bg, W, y0 + ay.hi, x0 + ax.hi, sp, cnt, signs, bb);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = blend(ay, ax, OH, OW, aa[c], ab[c], ba[c], bb[c]);
  }
  if (mode == CY_PASTE_OUT_U8) {
    unsigned char* o = (unsigned char*)out + ((long long)s * plane + i) * 3;
    o[0] = (unsigned char)v[0]; o[1] = (unsigned char)v[1]; o[2] = (unsigned char)v[2];
    return;
  }
  // (byte - 128) / 128 is exact in fp32; a bad sample is zero-filled, not centred
  float f[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) f[c] = ok ? (float)(v[c] - 128) * 0.0078125f : 0.f;
  if (mode == CY_PASTE_OUT_F32_NCHW) {
    float* o = (float*)out + (long long)s * 3 * plane + i;
    o[0] = f[0]; o[plane] = f[1]; o[2 * plane] = f[2];
  } else {
    float3s px; px.x = f[0]; px.y = f[1]; px.z = f[2];
    *(float3s*)((float*)out + ((long long)s * plane + i) * 3) = px;  // one 12-byte store
  }
}

// Grid (pixel tiles, batch): the sample number, its shift and its lightness are uniform per block (scalar loads), a thread owns one
// output pixel: three byte loads of its source pixel, three stores that are contiguous across the wave in each colour plane.
// A sample number outside the set reads nothing: zeros, label -1, one count in *err (by the first thread of its first tile).
__global__ __launch_bounds__(256) void gather_jitter_u8_kernel(
    const unsigned char* __restrict__ set, const long long* __restrict__ labels, int n_set, int H, int W,
    const int* __restrict__ shift, const float* __restrict__ light, const int* __restrict__ index, float* __restrict__ x_out,
    long long* __restrict__ y_out, int* err) {
  const int t = threadIdx.x, b = blockIdx.y, s = index[b];
  const bool ok = s >= 0 && s < n_set;
  if (blockIdx.x == 0 && t == 0) {
    y_out[b] = ok ? labels[s] : -1ll;
    if (!ok) atomicAdd(err, 1);
  }
  const int plane = H * W, i = (int)blockIdx.x * 256 + t;
  if (i >= plane) return;
  float f[3] = {0.f, 0.f, 0.f};                                      // off the image: grey on the centred scale, not brightened
  if (ok) {
    const int y = i / W, x = i - y * W;
    const long long sy = (long long)y - (shift ? shift[2 * s] : 0), sx = (long long)x - (shift ? shift[2 * s + 1] : 0);
    if (sy >= 0 && sy < H && sx >= 0 && sx < W) {
      const unsigned char* q = set + ((long long)s * plane + sy * W + sx) * 3;
      float k[3] = {(float)q[0], (float)q[1], (float)q[2]};
      // hsv_to_rgb(rgb_to_hsv(k / 256) + (0, 0, d)): V = max(k) grows by d, hue and saturation stay, so every channel is scaled by
      // (v + 256 d) / v; a black pixel has saturation 0 and becomes the grey 256 d.  d = 0: the gain is exactly 1.
      const float add = light ? 256.f * light[s] : 0.f, v = fmaxf(k[0], fmaxf(k[1], k[2]));
      const float g = (v + add) / v;
#pragma unroll
      for (int c = 0; c < 3; ++c) f[c] = ((v > 0.f ? k[c] * g : add) - 128.f) * 0.0078125f;
    }
  }
  float* o = x_out + (long long)b * 3 * plane + i;
  o[0] = f[0]; o[plane] = f[1]; o[2 * (long long)plane] = f[2];
}

}  // namespace

extern "C" int cy_paste_resize_max_pastes(void) { return MAX_PASTES; }

extern "C" int cy_paste_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                                  const unsigned char* signs, const long long* sign_off, const int* sign_hw, int n_signs,
                                  long long signs_bytes, const int* sample_img, const int* sample_rect, const int* begin, int n,
                                  const int* pastes, int n_pastes, int OH, int OW, int mode, void* out, int* err, void* stream) {
  CY_REQUIRE(n >= 0, "cy_paste_resize_u8: n = %d samples", n);
  if (n == 0) return 0;
  CY_REQUIRE(imgs && img_off && img_hw && sample_img && sample_rect && begin && out && err, "cy_paste_resize_u8: null argument");
  CY_REQUIRE(n_pastes >= 0 && (n_pastes == 0 || (signs && sign_off && sign_hw && pastes && n_signs > 0 && signs_bytes > 0)),
             "cy_paste_resize_u8: %d pastes need the sign set and the paste table", n_pastes);
  CY_REQUIRE(n_images > 0 && imgs_bytes > 0 && OH > 0 && OW > 0 && OH < (1 << 20) && OW < (1 << 20), "cy_paste_resize_u8: bad sizes");
  CY_REQUIRE(mode == CY_PASTE_OUT_U8 || mode == CY_PASTE_OUT_F32_NHWC || mode == CY_PASTE_OUT_F32_NCHW,
             "cy_paste_resize_u8: output mode %d", mode);
  CY_REQUIRE(n <= 65535, "cy_paste_resize_u8: %d samples are too many for one launch (65535)", n);
  const long long tiles = cy_ceil_div((long long)OH * OW, 256);
  CY_REQUIRE(tiles < (1ll << 31), "cy_paste_resize_u8: %d x %d output pixels are too many for one launch", OH, OW);
  paste_resize_u8_kernel<<<dim3((unsigned)tiles, (unsigned)n), 256, 0, (hipStream_t)stream>>>(
      imgs, img_off, img_hw, n_images, imgs_bytes, signs, sign_off, sign_hw, n_pastes ? n_signs : 0, signs_bytes, sample_img,
      sample_rect, begin, pastes, n_pastes, OH, OW, mode, out, err);
  CY_LAUNCH_CHECK("cy_paste_resize_u8");
  return 0;
}

extern "C" int cy_gather_jitter_u8(const unsigned char* set, const long long* labels, int n_set, int H, int W, const int* shift,
                                   const float* light, const int* index, int B, float* x_out, long long* y_out, int* err,
                                   void* stream) {
  CY_REQUIRE(B >= 0, "cy_gather_jitter_u8: B = %d samples", B);
  if (B == 0) return 0;
  CY_REQUIRE(set && labels && index && x_out && y_out && err, "cy_gather_jitter_u8: null argument");
  CY_REQUIRE(n_set > 0 && H > 0 && W > 0, "cy_gather_jitter_u8: a set of %d images of %d x %d", n_set, H, W);
  CY_REQUIRE((long long)H * W <= (1ll << 30), "cy_gather_jitter_u8: %d x %d pixels are too many for one image", H, W);
  CY_REQUIRE(B <= 65535, "cy_gather_jitter_u8: %d samples are too many for one launch (65535)", B);
  const long long tiles = cy_ceil_div((long long)H * W, 256);
  gather_jitter_u8_kernel<<<dim3((unsigned)tiles, (unsigned)B), 256, 0, (hipStream_t)stream>>>(set, labels, n_set, H, W, shift, light,
                                                                                                  index, x_out, y_out, err);
  CY_LAUNCH_CHECK("cy_gather_jitter_u8");
  return 0;
}
