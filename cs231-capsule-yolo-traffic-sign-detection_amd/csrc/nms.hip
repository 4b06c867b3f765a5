// Non-maximum suppression of a decoded box list on the device (gfx950): the step between the decode kernel and everything that
// reads boxes (the crops of serve.SignDetector, the drawn boxes and metric sweeps behind utils.nms_y_hat_device).  The reference
// has no such step; the rule is restated in numpy in tests/nms_ref.py.
//   nms_sweep_kernel    one block per image: rank by confidence, greedy sweep in LDS, keep[] = visit ordinal of every survivor
//   nms_gather_kernel   one block per image: survivors copied to the output slots behind those of the earlier images
// Both launches have shapes that depend on n_images alone and read the list length from device memory.
#include "common.h"
#include "box_iou.h"

// the double arithmetic below restates numpy expressions operation by operation: no fused multiply-add
#pragma clang fp contract(off)

namespace {

enum { NMS_ALIVE = 1, NMS_MALFORMED = 2 };
constexpr size_t NMS_LDS_PER_BOX = 4 * sizeof(double) + sizeof(float) + 3 * sizeof(int);     // sxy, cf, ssrc, scls, state

// first index of the sorted key[0..n) that is not below v
__device__ __forceinline__ int nms_lower_bound(const int* __restrict__ key, int n, int v) {
  int lo = 0, hi = n;
  while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] < v) lo = mid + 1; else hi = mid; }
  return lo;
}

// the live length of the list and the entries [g0, g1) of image `img` in it
__device__ __forceinline__ void nms_range(const int* __restrict__ count_in, const int* __restrict__ box_img, int n_cap, int img, int* n,
                                          int* g0, int* g1) {
  const int c = *count_in;
  *n = c < 0 ? 0 : (c < n_cap ? c : n_cap);
  *g0 = nms_lower_bound(box_img, *n, img);
  *g1 = nms_lower_bound(box_img, *n, img + 1);
}

// does entry j (confidence cj) come before entry i (ci) in the visit order?  Confidence descending, ties to the lower index; a NaN
// confidence comes behind every number (np.argsort(-conf, kind='stable'))
__device__ __forceinline__ bool nms_before(float cj, int j, float ci, int i) {
  if (ci != ci) return cj == cj || j < i;
  return cj == cj && (cj > ci || (cj == ci && j < i));
}

// Greedy suppression of one image's boxes.  LDS, M = max_per_image: the boxes in visit order (sxy, scls), the visit position's
// entry (ssrc), its state (NMS_ALIVE: not suppressed so far; NMS_MALFORMED: takes no part) and the confidences in list order (cf).
// The sweep walks the positions in order; every thread reads the same states, so all agree on the next kept box without talking.
// A kept box kills the later boxes it overlaps, one thread per 256 positions, and only then a barrier is needed: the scan for the
// next kept box reads positions at or below it, the next round writes positions above it.
// keep[i] = 0 for a suppressed entry, its 1-based ordinal among the image's survivors otherwise; ws[img] = the survivors.
__global__ __launch_bounds__(256) void nms_sweep_kernel(const int* __restrict__ count_in, const int* __restrict__ box_img,
                                                        const double* __restrict__ box_xy, const float* __restrict__ conf,
                                                        const int* __restrict__ cls, int n_cap, int n_images, double iou_th, int class_aware,
                                                        int per_image, int M, int* __restrict__ keep, int* __restrict__ ws, int* err) {
  extern __shared__ __attribute__((aligned(16))) double sm[];
  double* sxy = sm;                               // [M][4]
  float* cf = (float*)(sxy + (size_t)M * 4);      // [M]
  int* ssrc = (int*)(cf + M);                     // [M]
  int* scls = ssrc + M;                           // [M]
  int* state = scls + M;                          // [M]
  const int img = blockIdx.x, t = threadIdx.x;
  int n, g0, g1;
  nms_range(count_in, box_img, n_cap, img, &n, &g0, &g1);
  // entries of no image (an index outside 0..n_images-1, or past the live length) are not kept
  if (img == 0) for (int i = t; i < g0; i += 256) keep[i] = 0;
  if (img == n_images - 1) for (int i = g1 + t; i < n_cap; i += 256) keep[i] = 0;
  const int ni = g1 - g0;
  if (ni > M) {
    for (int i = g0 + t; i < g1; i += 256) keep[i] = 0;
    if (t == 0) { atomicAdd(err, 1 << 20); ws[img] = 0; }
    return;
  }
  if (ni == 0) { if (t == 0) ws[img] = 0; return; }
  for (int i = t; i < ni; i += 256) cf[i] = conf[g0 + i];
  __syncthreads();
  for (int i = t; i < ni; i += 256) {
    const float ci = cf[i];
    int r = 0;
    for (int j = 0; j < ni; ++j) r += nms_before(cf[j], j, ci, i);
    const double x1 = box_xy[(size_t)(g0 + i) * 4], y1 = box_xy[(size_t)(g0 + i) * 4 + 1];
    const double x2 = box_xy[(size_t)(g0 + i) * 4 + 2], y2 = box_xy[(size_t)(g0 + i) * 4 + 3];
    sxy[4 * r] = x1; sxy[4 * r + 1] = y1; sxy[4 * r + 2] = x2; sxy[4 * r + 3] = y2;
    ssrc[r] = i;
    scls[r] = class_aware ? cls[g0 + i] : 0;
    const bool good = isfinite(x1) && isfinite(y1) && isfinite(x2) && isfinite(y2) && x1 <= x2 && y1 <= y2;
    state[r] = good ? NMS_ALIVE : (NMS_ALIVE | NMS_MALFORMED);
  }
  __syncthreads();
  int kept = 0, p = 0;
  while (p < ni) {
    const int s = state[p];
    if (!(s & NMS_ALIVE)) { ++p; continue; }
    if (t == 0) keep[g0 + ssrc[p]] = kept + 1;
    ++kept;
    if (per_image > 0 && kept == per_image) { ++p; break; }
    if (!(s & NMS_MALFORMED)) {
      const double b[4] = {sxy[4 * p], sxy[4 * p + 1], sxy[4 * p + 2], sxy[4 * p + 3]};
      const int c = scls[p];
      for (int q = p + 1 + t; q < ni; q += 256) {
        if (state[q] == NMS_ALIVE && scls[q] == c && box_iou(b, sxy + 4 * q) > iou_th) {        // (a NaN IoU suppresses nothing)
          state[q] = 0;
          keep[g0 + ssrc[q]] = 0;
        }
      }
      __syncthreads();
    }
    ++p;
  }
  for (int q = p + t; q < ni; q += 256)           // what the per_image cap cut off
    if (state[q] & NMS_ALIVE) keep[g0 + ssrc[q]] = 0;
  if (t == 0) ws[img] = kept;
}

// Survivor number k of image `img` goes to slot (survivors of the images before it) + k - 1, a copy of its list entry; keep[] becomes
// 1 / 0.  The slots behind the last survivor are zero-filled by all blocks together, block 0 writes the count.
__global__ __launch_bounds__(256) void nms_gather_kernel(const int* __restrict__ count_in, const int* __restrict__ box_img,
                                                         const double* __restrict__ box_xy, const float* __restrict__ conf,
                                                         const int* __restrict__ cls, int n_cap, int n_images, const int* __restrict__ ws, int K,
                                                         int* __restrict__ keep, int* __restrict__ out_img, double* __restrict__ out_xy,
                                                         float* __restrict__ out_conf, int* __restrict__ out_cls, int* __restrict__ out_src,
                                                         int* __restrict__ count_out) {
  __shared__ int sums[2];                         // survivors of the images before this one, and of all images
  const int img = blockIdx.x, t = threadIdx.x;
  if (t < 2) sums[t] = 0;
  __syncthreads();
  int before = 0, all = 0;
  for (int i = t; i < n_images; i += 256) { const int c = ws[i]; all += c; if (i < img) before += c; }
  if (before) atomicAdd(&sums[0], before);
  if (all) atomicAdd(&sums[1], all);
  __syncthreads();
  const int base = sums[0], total = sums[1];
  int n, g0, g1;
  nms_range(count_in, box_img, n_cap, img, &n, &g0, &g1);
  for (int i = g0 + t; i < g1; i += 256) {
    const int k = keep[i];
    if (k <= 0) continue;
    keep[i] = 1;
    const int s = base + k - 1;
    if (s >= K) continue;
    out_img[s] = box_img[i];
    out_xy[4 * (size_t)s] = box_xy[4 * (size_t)i]; out_xy[4 * (size_t)s + 1] = box_xy[4 * (size_t)i + 1];
    out_xy[4 * (size_t)s + 2] = box_xy[4 * (size_t)i + 2]; out_xy[4 * (size_t)s + 3] = box_xy[4 * (size_t)i + 3];
    out_conf[s] = conf[i];
    if (cls) out_cls[s] = cls[i];
    out_src[s] = i;
  }
  for (long long s = (long long)(total < K ? total : K) + (long long)img * 256 + t; s < K; s += (long long)n_images * 256) {
    out_img[s] = 0;
    out_xy[4 * s] = 0.0; out_xy[4 * s + 1] = 0.0; out_xy[4 * s + 2] = 0.0; out_xy[4 * s + 3] = 0.0;
    out_conf[s] = 0.f;
    if (cls) out_cls[s] = 0;
    out_src[s] = 0;
  }
  if (img == 0 && t == 0) *count_out = total;
}

}  // namespace

#define CY_S ((hipStream_t)stream)

extern "C" int cy_nms_max_per_image(void) { return (int)((160 * 1024) / NMS_LDS_PER_BOX); }

extern "C" int cy_nms_boxes(const int* count_in, const int* box_img, const double* box_xy, const float* conf, const int* cls, int n_cap,
                            int n_images, double iou_th, int class_aware, int per_image, int max_per_image, int* keep, int K,
                            int* out_img, double* out_xy, float* out_conf, int* out_cls, int* out_src, int* count_out, int* ws, int* err,
                            void* stream) {
  CY_REQUIRE(count_in && keep && count_out && ws && err, "cy_nms_boxes: null argument (count_in, keep, count_out, ws, err)");
  CY_REQUIRE(K >= 0, "cy_nms_boxes: K=%d slots", K);
  CY_REQUIRE(n_cap >= 0, "cy_nms_boxes: n_cap=%d list entries", n_cap);
  CY_REQUIRE(n_images >= 1, "cy_nms_boxes: n_images=%d", n_images);
  CY_REQUIRE(iou_th >= 0.0 && iou_th <= 1.0, "cy_nms_boxes: iou_th=%g is not in [0, 1]", iou_th);       // also NaN
  CY_REQUIRE(per_image >= 0, "cy_nms_boxes: per_image=%d", per_image);
  CY_REQUIRE(!class_aware || cls, "cy_nms_boxes: class_aware=%d needs cls", class_aware);
  CY_REQUIRE(max_per_image >= 1, "cy_nms_boxes: max_per_image=%d", max_per_image);
  const size_t lds = (size_t)max_per_image * NMS_LDS_PER_BOX;
  CY_REQUIRE(lds <= 160 * 1024, "cy_nms_boxes: max_per_image=%d needs %zu bytes of LDS (limit 160 KiB: at most %d boxes per image)",
             max_per_image, lds, cy_nms_max_per_image());
  if (K == 0 || n_cap == 0) return 0;
  CY_REQUIRE(box_img && box_xy && conf && out_img && out_xy && out_conf && out_src, "cy_nms_boxes: null argument (boxes or output slots)");
  CY_REQUIRE(!cls || out_cls, "cy_nms_boxes: null argument (out_cls, with cls given)");
  if (int rc = cyi_launch_lds("cy_nms_boxes (sweep)", nms_sweep_kernel, dim3(n_images), dim3(256), lds, CY_S, count_in, box_img, box_xy, conf,
                              cls, n_cap, n_images, iou_th, class_aware, per_image, max_per_image, keep, ws, err))
    return rc;
  nms_gather_kernel<<<n_images, 256, 0, CY_S>>>(count_in, box_img, box_xy, conf, cls, n_cap, n_images, ws, K, keep, out_img, out_xy, out_conf,
                                                out_cls, out_src, count_out);
  CY_LAUNCH_CHECK("cy_nms_boxes (gather)");
  return 0;
}
