// Two-stage prediction on the device (gfx950): the glue between the detector and the classifier of
// predict_fns.dark_class_pred (predict_fns.py:75-82) and the threshold sweep of metrics.detect_and_recog_mAP
// (metrics.py:284-339).
//   crop_resize_u8_kernel     cv2.resize of whole images (predict_fns.py:38) and of box crops (plot.py:22, predict_fns.py:57)
//   combine_*_kernel          utils.combine_y_hat (utils.py:336-351)
//   yolo_decode_conf_kernel   utils.y_to_boxes_vec (utils.py:288-334) that also returns each box's confidence
//   confusion_sweep_kernel    metrics.single_img_confusion for every (group, confidence threshold, IoU threshold) at once
#include "common.h"
#include "box_iou.h"
#include "crop_pixel.h"

// the double arithmetic below restates numpy expressions operation by operation: no fused multiply-add
#pragma clang fp contract(off)

namespace {

// One thread per output pixel; the pixel itself is cyi_crop_pixel (crop_pixel.h, shared with serve.hip).  Images: where the
// images lie and how a tap is fetched (cyi_images_rgb: packed HWC; cyi_images_nv12: NV12 converted in the tap fetch).
template <class Images>
__global__ __launch_bounds__(256) void crop_resize_kernel(const Images src, const int* __restrict__ box_img, const int* __restrict__ rect,
                                                          long long total, int n_images, int OH, int OW, float shift, float scale,
                                                          int to_nchw, float* __restrict__ out, int* err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ox = (int)(i % OW);
  const long long q = i / OW;
  const int oy = (int)(q % OH);
  const long long b = q / OH;
  const int img = box_img[b];
  float v[3] = {0.f, 0.f, 0.f};
  bool ok = img >= 0 && img < n_images;
  int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
  typename Images::fetch_t f;
  if (ok) {
    int H, W;
    const bool inside = src.image(img, H, W, f);
    y0 = rect[4 * b]; y1 = rect[4 * b + 1]; x0 = rect[4 * b + 2]; x1 = rect[4 * b + 3];
    ok = y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W && inside;
  }
  if (!ok) {
    if (ox == 0 && oy == 0) atomicAdd(err, 1);       // one count per bad box; its output is zero-filled
  } else {
    cyi_crop_pixel(f, y0, y1, x0, x1, oy, ox, OH, OW, shift, scale, v);
  }
  cyi_store_pixel(out, i, b, oy, ox, OH, OW, to_nchw, v[0], v[1], v[2]);
}

// combine_y_hat, step 1: the cell of every box, in the reference's order of operations (resize_box_xy -> xy_to_cwh ->
// normalize_box_cwh, utils.py:198-230) in double; the highest box index of a cell is kept (the reference's loop lets the
// last box overwrite the earlier ones).  winner[] holds box index + 1, 0 = no box.
__global__ void combine_cells_kernel(const int* __restrict__ box_img, const double* __restrict__ box_xy, const long long* __restrict__ image_hw,
                                     double side, int B, int g, int n, int* winner, int* err) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const int img = box_img[i];
  if (img < 0 || img >= B) { atomicAdd(err, 1); return; }
  const double orig_h = (double)image_hw[2 * img], orig_w = (double)image_hw[2 * img + 1];
  const double w_ratio = 1. * side / orig_w, h_ratio = 1. * side / orig_h;
  const double rx1 = box_xy[4 * i] * w_ratio, rx2 = box_xy[4 * i + 2] * w_ratio;
  const double ry1 = box_xy[4 * i + 1] * h_ratio, ry2 = box_xy[4 * i + 3] * h_ratio;
  const double xc = (rx1 + rx2) / 2, yc = (ry1 + ry2) / 2;
  const double grid_w = 1. * side / g, grid_h = 1. * side / g;
  const double fc = trunc(xc / grid_w), fr = trunc(yc / grid_h);      // int(): towards zero
  if (!(fc >= 0 && fc < g && fr >= 0 && fr < g)) { atomicAdd(err, 1); return; }   // also NaN
  atomicMax(winner + ((long long)img * g + (int)fr) * g + (int)fc, i + 1);
}
// step 2: y_hat[cell] = [detector output (D) | class scores of the cell's winning box, or zeros (C)]
__global__ void combine_copy_kernel(const float* __restrict__ dark, const float* __restrict__ scores, const int* __restrict__ winner,
                                    long long cells, int D, int C, float* __restrict__ y_hat) {
  const long long total = cells * (D + C);
  for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
    const long long cell = i / (D + C);
    const int k = (int)(i - cell * (D + C));
    float v;
    if (k < D) v = dark[cell * D + k];
    else { const int w = winner[cell]; v = w > 0 ? scores[(long long)(w - 1) * C + (k - D)] : 0.f; }
    y_hat[i] = v;
  }
}

// yolo_decode_kernel of misc.hip with one more output, the stored confidence of every box (same order; the same arithmetic,
// here without fused multiply-adds like the rest of this file).
__global__ __launch_bounds__(1024) void yolo_decode_conf_kernel(const float* __restrict__ y, const long long* __restrict__ image_hw,
                                                                double img_h, double img_w, int B, int g, int nb, int C, float conf_th,
                                                                int* count, int* image_idx, double* xy, int* cls, float* conf, int max_boxes) {
  __shared__ int wave_cnt[16];
  __shared__ int base_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D = 5 * nb + C;
  const long long total = (long long)B * g * g * nb;
  if (t == 0) base_s = 0;
  __syncthreads();
  for (long long c0 = 0; c0 < total; c0 += 1024) {
    const long long i = c0 + t;
    bool hit = false;
    int bi = 0, row = 0, col = 0, k = 0;
    float cf = 0.f;
    if (i < total) {
      long long r = i;
      k = (int)(r % nb); r /= nb;
      col = (int)(r % g); r /= g;
      row = (int)(r % g); bi = (int)(r / g);
      cf = y[(((long long)bi * g + row) * g + col) * D + 5 * k];
      hit = cf > conf_th;
    }
    const unsigned long long m = __ballot(hit);
    if (lane == 0) wave_cnt[wave] = __popcll(m);
    __syncthreads();
    int before = 0, chunk_total = 0;
    for (int w = 0; w < 16; ++w) { const int cnt = wave_cnt[w]; if (w < wave) before += cnt; chunk_total += cnt; }
    const int base = base_s;
    if (hit) {
      const int o = base + before + __popcll(m & ((1ull << lane) - 1ull));
      if (o < max_boxes) {
        const float* cell = y + (((long long)bi * g + row) * g + col) * D;
        const double ih = image_hw ? (double)image_hw[2 * bi] : img_h, iw = image_hw ? (double)image_hw[2 * bi + 1] : img_w;
        const double gw = 1.0 * iw / g, gh = 1.0 * ih / g;
        double xc = (double)cell[5 * k + 1] * gw, yc = (double)cell[5 * k + 2] * gh;
        const double w_ = (double)cell[5 * k + 3] * iw, h_ = (double)cell[5 * k + 4] * ih;
        xc += col * gw; yc += row * gh;
        image_idx[o] = bi;
        conf[o] = cf;
        xy[4 * o + 0] = xc - w_ / 2; xy[4 * o + 1] = yc - h_ / 2;
        xy[4 * o + 2] = xc + w_ / 2; xy[4 * o + 3] = yc + h_ / 2;
        if (C > 0) {
          int best = 0; float bv = cell[5 * nb];
          for (int c = 1; c < C; ++c) { const float v = cell[5 * nb + c]; if (v > bv) { bv = v; best = c; } }
          cls[o] = best;
        }
      }
    }
    __syncthreads();
    if (t == 0) base_s = base + chunk_total;
    __syncthreads();
  }
  if (t == 0) *count = base_s;
}

__device__ __forceinline__ int lower_bound_key(const int* __restrict__ key, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// The whole threshold sweep of detect_and_recog_mAP / detect_AP in one launch.  The reference decodes both arrays again for
// every confidence threshold and matches the survivors; but a pair's IoU does not depend on that threshold, and a box
// survives threshold th iff its confidence exceeds it.  So with best[i][t] = the highest confidence among the partners of box
// i at IoU threshold t, box i is "hit" at (th, t) iff min(conf_i, best[i][t]) > th.  One block per group (the boxes of one
// image, or of one image and class; keys ascending): boxes in LDS, one thread per box builds best[][], then one thread per
// (k, t) counts and adds (gt hit, predictions - predictions hit, gt - gt hit) to out[k][group % C][t][0..2].
__global__ __launch_bounds__(256) void confusion_sweep_kernel(const int* __restrict__ gt_key, const double* __restrict__ gt_xy,
                                                              const float* __restrict__ gt_conf, int n_gt,
                                                              const int* __restrict__ pr_key, const double* __restrict__ pr_xy,
                                                              const float* __restrict__ pr_conf, int n_pr, int C,
                                                              const double* __restrict__ conf_ths, int K,
                                                              const double* __restrict__ iou_ths, int T, int M, int* out, int* err) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* gxy = sm;                               // [M][4]
  double* pxy = gxy + (size_t)M * 4;              // [M][4]
  double* ths = pxy + (size_t)M * 4;              // [K] confidence thresholds
  double* ious = ths + K;                         // [T] IoU thresholds
  float* gcf = (float*)(ious + T);                // [M]
  float* pcf = gcf + M;                           // [M]
  float* gbest = pcf + M;                         // [M][T]
  float* pbest = gbest + (size_t)M * T;           // [M][T]
  const int grp = blockIdx.x, t = threadIdx.x;
  const int g0 = lower_bound_key(gt_key, n_gt, grp), g1 = lower_bound_key(gt_key, n_gt, grp + 1);
  const int p0 = lower_bound_key(pr_key, n_pr, grp), p1 = lower_bound_key(pr_key, n_pr, grp + 1);
  const int n1 = g1 - g0, n2 = p1 - p0;
  if (n1 == 0 && n2 == 0) return;                 // adds nothing to any count
  if (n1 > M || n2 > M) { if (t == 0) atomicAdd(err, 1 << 20); return; }
  for (int i = t; i < n1 * 4; i += 256) gxy[i] = gt_xy[(size_t)g0 * 4 + i];
  for (int i = t; i < n2 * 4; i += 256) pxy[i] = pr_xy[(size_t)p0 * 4 + i];
  for (int i = t; i < n1; i += 256) gcf[i] = gt_conf[g0 + i];
  for (int i = t; i < n2; i += 256) pcf[i] = pr_conf[p0 + i];
  for (int i = t; i < K; i += 256) ths[i] = conf_ths[i];
  for (int i = t; i < T; i += 256) ious[i] = iou_ths[i];
  __syncthreads();
  int bad = 0;
  for (int b = t; b < n1 + n2; b += 256) {
    const bool is_gt = b < n1;
    const int i = is_gt ? b : b - n1;
    const double* mine = (is_gt ? gxy : pxy) + 4 * i;
    bad += (mine[0] > mine[2]) || (mine[1] > mine[3]);
    float* best = (is_gt ? gbest : pbest) + (size_t)i * T;
    for (int q = 0; q < T; ++q) best[q] = -INFINITY;
    const int nj = is_gt ? n2 : n1;
    const double* theirs = is_gt ? pxy : gxy;
    const float* their_cf = is_gt ? pcf : gcf;
    for (int j = 0; j < nj; ++j) {
      const double iou = is_gt ? box_iou(mine, theirs + 4 * j) : box_iou(theirs + 4 * j, mine);
      const float cf = their_cf[j];
      for (int q = 0; q < T; ++q) if (iou > ious[q]) best[q] = fmaxf(best[q], cf);
    }
  }
  if (bad) atomicAdd(err, bad);
  __syncthreads();
  const int cls = grp % C;
  for (int pair = t; pair < K * T; pair += 256) {
    const int k = pair / T, q = pair - k * T;
    const double th = ths[k];
    int c1 = 0, c2 = 0, gh = 0, ph = 0;
    for (int i = 0; i < n1; ++i) {
      const float cf = gcf[i];
      c1 += (double)cf > th;
      gh += (double)fminf(cf, gbest[(size_t)i * T + q]) > th;
    }
    for (int j = 0; j < n2; ++j) {
      const float cf = pcf[j];
      c2 += (double)cf > th;
      ph += (double)fminf(cf, pbest[(size_t)j * T + q]) > th;
    }
    int* o = out + (((size_t)k * C + cls) * T + q) * 3;
    if (gh) atomicAdd(o + 0, gh);
    if (c2 - ph) atomicAdd(o + 1, c2 - ph);
    if (c1 - gh) atomicAdd(o + 2, c1 - gh);
  }
}

}  // namespace

#define CY_S ((hipStream_t)stream)

extern "C" int cy_crop_resize_u8(const unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                                 const int* box_img, const int* rect, int n, int OH, int OW, float shift, float scale, int to_nchw,
                                 float* out, int* err, void* stream) {
  CY_REQUIRE(imgs && img_off && img_hw && box_img && rect && out && err, "cy_crop_resize_u8: null argument");
  CY_REQUIRE(n_images > 0 && imgs_bytes > 0 && n > 0 && OH > 0 && OW > 0 && OH < (1 << 20) && OW < (1 << 20), "cy_crop_resize_u8: bad sizes");
  const long long total = (long long)n * OH * OW;
  CY_REQUIRE(cy_ceil_div(total, 256) < (1ll << 31), "cy_crop_resize_u8: %lld output pixels are too many for one launch", total);
  const cyi_images_rgb src = {imgs, img_off, img_hw, imgs_bytes};
  crop_resize_kernel<<<(unsigned)cy_ceil_div(total, 256), 256, 0, CY_S>>>(src, box_img, rect, total, n_images, OH, OW, shift, scale, to_nchw,
                                                                          out, err);
  CY_LAUNCH_CHECK("cy_crop_resize_u8");
  return 0;
}

extern "C" int cy_crop_resize_nv12(const unsigned char* imgs, const long long* img_off, const int* img_geom, int n_images,
                                   long long imgs_bytes, cy_yuv_coef_t coef, const int* box_img, const int* rect, int n, int OH, int OW,
                                   float shift, float scale, int to_nchw, float* out, int* err, void* stream) {
  CY_REQUIRE(imgs && img_off && img_geom && box_img && rect && out && err, "cy_crop_resize_nv12: null argument");
  CY_REQUIRE(n_images > 0 && imgs_bytes > 0 && n > 0 && OH > 0 && OW > 0 && OH < (1 << 20) && OW < (1 << 20), "cy_crop_resize_nv12: bad sizes");
  CY_REQUIRE(cyi_yuv_coef_ok(coef), "cy_crop_resize_nv12: " CYI_YUV_COEF_MSG, CYI_YUV_COEF_ARGS(coef));
  const long long total = (long long)n * OH * OW;
  CY_REQUIRE(cy_ceil_div(total, 256) < (1ll << 31), "cy_crop_resize_nv12: %lld output pixels are too many for one launch", total);
  const cyi_images_nv12 src = {imgs, img_off, img_geom, imgs_bytes, coef};
  crop_resize_kernel<<<(unsigned)cy_ceil_div(total, 256), 256, 0, CY_S>>>(src, box_img, rect, total, n_images, OH, OW, shift, scale, to_nchw,
                                                                          out, err);
  CY_LAUNCH_CHECK("cy_crop_resize_nv12");
  return 0;
}

extern "C" int cy_combine_scores(const float* dark, const float* scores, const int* box_img, const double* box_xy, int n,
                                 const long long* image_hw, double side, int B, int g, int D, int C, int* winner, float* y_hat, int* err,
                                 void* stream) {
  CY_REQUIRE(dark && image_hw && winner && y_hat && err && B > 0 && g > 0 && D > 0 && C > 0 && n >= 0 && side > 0,
             "cy_combine_scores: bad arguments");
  CY_REQUIRE(n == 0 || (scores && box_img && box_xy), "cy_combine_scores: null box arrays");
  if (n > 0) {
    combine_cells_kernel<<<(unsigned)cy_ceil_div(n, 256), 256, 0, CY_S>>>(box_img, box_xy, image_hw, side, B, g, n, winner, err);
    CY_LAUNCH_CHECK("cy_combine_scores (cells)");
  }
  const long long cells = (long long)B * g * g;
  long long blocks = cy_ceil_div(cells * (D + C), 256);
  if (blocks > 8192) blocks = 8192;
  combine_copy_kernel<<<(unsigned)blocks, 256, 0, CY_S>>>(dark, scores, winner, cells, D, C, y_hat);
  CY_LAUNCH_CHECK("cy_combine_scores (copy)");
  return 0;
}

extern "C" int cy_yolo_decode_boxes_conf(const float* y, const long long* image_hw, double img_h, double img_w, int B, int g, int nb,
                                         int C, float conf_th, int* count, int* image_idx, double* xy, int* cls, float* conf,
                                         int max_boxes, void* stream) {
  CY_REQUIRE(y && count && image_idx && xy && conf && B > 0 && g > 0 && nb > 0 && C >= 0 && max_boxes > 0,
             "cy_yolo_decode_boxes_conf: bad arguments");
  CY_REQUIRE(C == 0 || cls, "cy_yolo_decode_boxes_conf: cls must be given when C > 0");
  yolo_decode_conf_kernel<<<1, 1024, 0, CY_S>>>(y, image_hw, img_h, img_w, B, g, nb, C, conf_th, count, image_idx, xy, cls, conf, max_boxes);
  CY_LAUNCH_CHECK("cy_yolo_decode_boxes_conf");
  return 0;
}

extern "C" int cy_confusion_sweep(const int* gt_key, const double* gt_xy, const float* gt_conf, int n_gt, const int* pr_key,
                                  const double* pr_xy, const float* pr_conf, int n_pr, int n_groups, int C, const double* conf_ths, int K,
                                  const double* iou_ths, int T, int max_per_group, int* out, int* err, void* stream) {
  CY_REQUIRE(out && err && conf_ths && iou_ths && n_groups > 0 && C > 0 && K > 0 && T > 0 && n_gt >= 0 && n_pr >= 0 && max_per_group > 0,
             "cy_confusion_sweep: bad arguments");
  CY_REQUIRE((n_gt == 0 || (gt_key && gt_xy && gt_conf)) && (n_pr == 0 || (pr_key && pr_xy && pr_conf)), "cy_confusion_sweep: null box arrays");
  const size_t M = (size_t)max_per_group;
  const size_t lds = (2 * M * 4 + (size_t)K + (size_t)T) * sizeof(double) + (2 * M + 2 * M * (size_t)T) * sizeof(float);
  CY_REQUIRE(lds <= 160 * 1024, "cy_confusion_sweep: max_per_group=%d with %d confidence and %d IoU thresholds needs %zu bytes of LDS (limit 160 KiB)",
             max_per_group, K, T, lds);
  if (int rc = cy_allow_lds(confusion_sweep_kernel, lds)) return rc;
  confusion_sweep_kernel<<<n_groups, 256, lds, CY_S>>>(gt_key, gt_xy, gt_conf, n_gt, pr_key, pr_xy, pr_conf, n_pr, C, conf_ths, K, iou_ths, T,
                                                       max_per_group, out, err);
  CY_LAUNCH_CHECK("cy_confusion_sweep");
  return 0;
}
