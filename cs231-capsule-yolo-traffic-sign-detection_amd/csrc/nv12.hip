// NV12 images converted whole to packed HWC RGB uint8 by the colour rule of include/capsyolo_hip.h: for drawing, for debugging, and
// the device-side counterpart of the tests.  The streaming detector does not come through here: its two crop launches
// (cy_crop_resize_nv12 in predict.hip, cy_boxes_crop_resize_nv12 in serve.hip) convert in their tap fetch (crop_pixel.h).
#include "common.h"
#include "crop_pixel.h"

namespace {

// blockIdx.z = image; the blocks walk the image's rows with a stride of gridDim.y and a row's columns with a stride of gridDim.x * 256
// (the sizes are device data, so the launch cannot be cut to them; no division per pixel).  An image that is not well formed, or
// whose source or destination leaves its buffer, is not touched and counted once.
__global__ __launch_bounds__(256) void nv12_to_rgb_kernel(const cyi_images_nv12 src, unsigned char* __restrict__ out,
                                                          const long long* __restrict__ out_off, long long out_bytes, int* err) {
  const int img = blockIdx.z;
  int H, W;
  cyi_fetch_nv12 f;
  bool ok = src.image(img, H, W, f);
  const long long o = out_off[img];
  ok = ok && o >= 0 && o + (long long)H * W * 3 <= out_bytes;
  if (!ok) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) atomicAdd(err, 1);
    return;
  }
  for (int y = blockIdx.y; y < H; y += gridDim.y) {
    const unsigned char* __restrict__ lrow = f.luma + (long long)y * f.pitch;
    const unsigned char* __restrict__ crow = f.chroma + (long long)(y >> 1) * f.pitch;
    unsigned char* __restrict__ drow = out + o + (long long)y * W * 3;
    for (int x = blockIdx.x * 256 + threadIdx.x; x < W; x += gridDim.x * 256) {
      const int c = 2 * (x >> 1);
      int rgb[3];
      cyi_yuv_to_rgb(f.k, lrow[x], crow[c], crow[c + 1], rgb);
      unsigned char* d = drow + 3 * (long long)x;      // (byte stores: out_off promises no alignment)
      d[0] = (unsigned char)rgb[0]; d[1] = (unsigned char)rgb[1]; d[2] = (unsigned char)rgb[2];
    }
  }
}

}  // namespace

extern "C" int cy_nv12_to_rgb_u8(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images,
                                 long long imgs_bytes, cy_yuv_coef_t coef, unsigned char* out, const long long* out_off,
                                 long long out_bytes, int* err, void* stream) {
  CY_REQUIRE(imgs && img_off && img_geom && out && out_off && err, "cy_nv12_to_rgb_u8: null argument");
  CY_REQUIRE(n_images > 0 && n_images <= 65535 && imgs_bytes > 0 && out_bytes > 0, "cy_nv12_to_rgb_u8: %d images (1..65535) in %lld bytes to %lld bytes",
             n_images, imgs_bytes, out_bytes);
  CY_REQUIRE(cyi_yuv_coef_ok(coef), "cy_nv12_to_rgb_u8: " CYI_YUV_COEF_MSG, CYI_YUV_COEF_ARGS(coef));
  const cyi_images_nv12 src = {imgs, img_off, img_geom, imgs_bytes, coef};
  nv12_to_rgb_kernel<<<dim3(4, 64, (unsigned)n_images), 256, 0, (hipStream_t)stream>>>(src, out, out_off, out_bytes, err);
  CY_LAUNCH_CHECK("cy_nv12_to_rgb_u8");
  return 0;
}
