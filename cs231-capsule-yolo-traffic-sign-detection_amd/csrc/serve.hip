// The device-side glue of the streaming detector (serve.py, SignDetector): what predict_fns._detect_and_crop does on the host between
// the detector and the classifier, and what follows the classifier, as two fixed-shape launches that read the box count from device
// memory -- so the chain frame -> detector -> crops -> classifier -> labelled boxes has no host hop and captures into a HIP graph.
//   boxes_crop_resize_kernel      utils.crop_rectangles (the rectangle rule) fused with cy_crop_resize_u8, for K slots
//   pack_detections_kernel        np.argmax of the class scores + gather of every slot into one record buffer
#include "common.h"
#include "crop_pixel.h"

// the double arithmetic below restates numpy expressions operation by operation: no fused multiply-add
#pragma clang fp contract(off)

namespace {

// np.clip(np.trunc(v), 0, hi) of a finite v, as an int (hi is an image side)
__device__ __forceinline__ int trunc_clip(double v, int hi) {
  const double t = trunc(v);
  return (int)fmin(fmax(t, 0.0), (double)hi);
}

// One thread per output pixel of every slot; the launch does not depend on *count.  Every thread of a slot computes the slot's
// rectangle again (four doubles), the slot's first thread writes it and counts a bad slot.  Images: cyi_images_rgb or cyi_images_nv12
// (crop_pixel.h); the slot rule below is the one copy for both.
template <class Images>
__global__ __launch_bounds__(256) void boxes_crop_resize_kernel(const Images src, int n_images, const int* __restrict__ count,
                                                                const int* __restrict__ box_img, const double* __restrict__ box_xy,
                                                                long long total, int K, int OH, int OW, float shift, float scale,
                                                                int to_nchw, float* __restrict__ out, int* __restrict__ rect_out, int* err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % OW);
  const long long q = i / OW;
  const int oy = (int)(q % OH);
  const int s = (int)(q / OH);
  const int n = *count;
  const bool live = s < (n < K ? n : K);
  float v[3] = {0.f, 0.f, 0.f};
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  bool ok = false;
  if (live) {
    const int img = box_img[s];
    const double bx0 = box_xy[4 * s], by0 = box_xy[4 * s + 1], bx1 = box_xy[4 * s + 2], by1 = box_xy[4 * s + 3];
    ok = img >= 0 && img < n_images && isfinite(bx0) && isfinite(by0) && isfinite(bx1) && isfinite(by1);
    if (ok) {
      int H, W;
      typename Images::fetch_t f;
      // (an image that does not lie inside the buffer is never read: its slots are bad)
      const bool inside = src.image(img, H, W, f);
      x0 = trunc_clip(bx0, W); x1 = trunc_clip(bx1, W);
      y0 = trunc_clip(by0, H); y1 = trunc_clip(by1, H);
      ok = y0 < y1 && x0 < x1 && inside;
      if (ok) cyi_crop_pixel(f, y0, y1, x0, x1, oy, ox, OH, OW, shift, scale, v);
      else y0 = y1 = x0 = x1 = 0;
    }
  }
  if (ox == 0 && oy == 0) {
    rect_out[4 * s] = y0; rect_out[4 * s + 1] = y1; rect_out[4 * s + 2] = x0; rect_out[4 * s + 3] = x1;
    if (live && !ok) atomicAdd(err, 1);              // one count per bad slot; its output is zero-filled
  }
  cyi_store_pixel(out, i, s, oy, ox, OH, OW, to_nchw, v[0], v[1], v[2]);
}

// One thread per slot: np.argmax over the slot's C scores (the first maximum wins; a NaN counts as the maximum, so the first NaN
// wins), then the slot's record.  Thread 0 writes the header.  The slots behind `kept` hold zeros and class -1, whatever the box
// arrays still hold there from an earlier frame, so a record depends on its own frame alone.
__global__ __launch_bounds__(64) void pack_detections_kernel(const float* __restrict__ scores, int C, const int* __restrict__ count,
                                                             const int* __restrict__ box_img, const double* __restrict__ box_xy,
                                                             const float* __restrict__ conf, const int* __restrict__ rect,
                                                             const int* __restrict__ crop_err, const int* __restrict__ resize_err, int K,
                                                             cy_detections_header_t* __restrict__ head, cy_detection_t* __restrict__ rec) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  const int n = *count;
  const int kept = n < 0 ? 0 : (n < K ? n : K);
  if (s == 0) {
    head->total = n; head->kept = kept;
    head->crop_err = crop_err ? *crop_err : 0;
    head->resize_err = resize_err ? *resize_err : 0;
  }
  if (s >= K) return;
  cy_detection_t d;
  d.xy[0] = d.xy[1] = d.xy[2] = d.xy[3] = 0.0;
  d.image = 0; d.cls = -1; d.conf = 0.f; d.score = 0.f;
  if (s < kept) {
    d.xy[0] = box_xy[4 * s]; d.xy[1] = box_xy[4 * s + 1]; d.xy[2] = box_xy[4 * s + 2]; d.xy[3] = box_xy[4 * s + 3];
    d.image = box_img[s];
    d.conf = conf[s];
    if (rect[4 * s] | rect[4 * s + 1] | rect[4 * s + 2] | rect[4 * s + 3]) {        // a good slot: its rectangle is not (0,0,0,0)
      const float* row = scores + (long long)s * C;
      int best = 0; float bv = row[0];
      for (int c = 1; c < C; ++c) {
        const float x = row[c];
        if (bv == bv && (x > bv || x != x)) { bv = x; best = c; }
      }
      d.cls = best; d.score = bv;
    }
  }
  rec[s] = d;
}

}  // namespace

#define CY_S ((hipStream_t)stream)

// the checks and the launch of both image formats; `who` names the entry point in the messages
template <class Images>
static int boxes_crop_resize(const char* who, const Images& src, bool tables, int n_images, long long imgs_bytes, const int* count,
                             const int* box_img, const double* box_xy, int K, int OH, int OW, float shift, float scale, int to_nchw,
                             float* out, int* rect_out, int* err, void* stream) {
  CY_REQUIRE(count && out && rect_out && err, "%s: null argument (count, out, rect_out, err)", who);
  CY_REQUIRE(K >= 0, "%s: K=%d slots", who, K);
  CY_REQUIRE(OH >= 1 && OW >= 1 && OH < (1 << 20) && OW < (1 << 20), "%s: output size %d x %d", who, OH, OW);
  if (K == 0) return 0;
  CY_REQUIRE(tables && box_img && box_xy, "%s: null argument (images or boxes)", who);
  CY_REQUIRE(n_images > 0 && imgs_bytes > 0, "%s: %d images in %lld bytes", who, n_images, imgs_bytes);
  const long long total = (long long)K * OH * OW;
  CY_REQUIRE(cy_ceil_div(total, 256) < (1ll << 31), "%s: %lld output pixels are too many for one launch", who, total);
  boxes_crop_resize_kernel<<<(unsigned)cy_ceil_div(total, 256), 256, 0, CY_S>>>(src, n_images, count, box_img, box_xy, total, K, OH, OW, shift,
                                                                                scale, to_nchw, out, rect_out, err);
  CY_LAUNCH_CHECK(who);
  return 0;
}

extern "C" int cy_boxes_crop_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images,
                                       long long imgs_bytes, const int* count, const int* box_img, const double* box_xy, int K, int OH,
                                       int OW, float shift, float scale, int to_nchw, float* out, int* rect_out, int* err, void* stream) {
  const cyi_images_rgb src = {imgs, img_off, img_hw, imgs_bytes};
  return boxes_crop_resize("cy_boxes_crop_resize_u8", src, imgs && img_off && img_hw, n_images, imgs_bytes, count, box_img, box_xy, K, OH, OW,
                           shift, scale, to_nchw, out, rect_out, err, stream);
}

extern "C" int cy_boxes_crop_resize_nv12(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images,
                                         long long imgs_bytes, cy_yuv_coef_t coef, const int* count, const int* box_img,
                                         const double* box_xy, int K, int OH, int OW, float shift, float scale, int to_nchw, float* out,
                                         int* rect_out, int* err, void* stream) {
  CY_REQUIRE(cyi_yuv_coef_ok(coef), "cy_boxes_crop_resize_nv12: " CYI_YUV_COEF_MSG, CYI_YUV_COEF_ARGS(coef));
  const cyi_images_nv12 src = {imgs, img_off, img_geom, imgs_bytes, coef};
  return boxes_crop_resize("cy_boxes_crop_resize_nv12", src, imgs && img_off && img_geom, n_images, imgs_bytes, count, box_img, box_xy, K, OH,
                           OW, shift, scale, to_nchw, out, rect_out, err, stream);
}

extern "C" int cy_pack_detections(const float* scores, int C, const int* count, const int* box_img, const double* box_xy,
                                  const float* conf, const int* rect, const int* crop_err, const int* resize_err, int K, void* record,
                                  void* stream) {
  CY_REQUIRE(count && record, "cy_pack_detections: null argument (count, record)");
  CY_REQUIRE(K >= 0, "cy_pack_detections: K=%d slots", K);
  CY_REQUIRE(K == 0 || (scores && box_img && box_xy && conf && rect), "cy_pack_detections: null argument (scores or boxes)");
  CY_REQUIRE(K == 0 || C >= 1, "cy_pack_detections: C=%d class scores per slot", C);
  CY_REQUIRE(((uintptr_t)record & 7) == 0, "cy_pack_detections: the record buffer must be 8-byte aligned");
  cy_detections_header_t* head = (cy_detections_header_t*)record;
  pack_detections_kernel<<<K > 0 ? (unsigned)cy_ceil_div(K, 64) : 1u, 64, 0, CY_S>>>(scores, C, count, box_img, box_xy, conf, rect, crop_err,
                                                                                      resize_err, K, head, (cy_detection_t*)(head + 1));
  CY_LAUNCH_CHECK("cy_pack_detections");
  return 0;
}
