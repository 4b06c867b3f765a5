// Tiled detection on the device (gfx950): the step that puts the detector's outputs for overlapping windows of a frame back into
// that frame (capsyolo_amd/tiles.py, serve.SignDetector(tiles=), predict_fns.dark_pred_tiled).
//   yolo_decode_tiles_kernel   yolo_decode_conf_kernel (predict.hip) for a batch whose images are tiles: the same decode with the
//                              tile as the image, the border rule, the shift into frame pixels, the frame as the image index
// The reference has no such step; tests/tiles_ref.py restates the rule in numpy.
#include "common.h"

// the double arithmetic below restates numpy expressions operation by operation: no fused multiply-add
#pragma clang fp contract(off)

namespace {

// One workgroup; 1024 cells (tile, row, column, box) per pass in list order.  A cell is KEPT iff its confidence is over the threshold,
// its tile is valid and the border rule lets it through; the kept cells of a pass are compacted with one ballot and a count per wave,
// and the running base is carried from pass to pass: the list order is (tile, row, column, box) with no atomic on it.  The boxes the
// border rule drops are counted the same way.
__global__ __launch_bounds__(1024) void yolo_decode_tiles_kernel(const float* __restrict__ y, const int* __restrict__ tile_frame,
                                                                 const int* __restrict__ tile_rect, const int* __restrict__ frame_hw,
                                                                 int n_frames, double margin, int Bt, int g, int nb, int C, float conf_th,
                                                                 int* count, int* dropped, int* image_idx, double* xy, int* cls, float* conf,
                                                                 int* out_tile, int max_boxes, int* err) {
  __shared__ int wave_cnt[16];
  __shared__ int wave_drop[16];
  __shared__ int base_s;
  __shared__ int drop_s;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int D = 5 * nb + C;
  const long long total = (long long)Bt * g * g * nb;
  if (t == 0) { base_s = 0; drop_s = 0; }
  __syncthreads();
  for (long long c0 = 0; c0 < total; c0 += 1024) {
    const long long i = c0 + t;
    bool keep = false, drop = false;
    int bi = 0, row = 0, col = 0, k = 0, frame = 0, x0 = 0, y0 = 0;
    float cf = 0.f;
    double bx1 = 0, by1 = 0, bx2 = 0, by2 = 0;
    if (i < total) {
      long long r = i;
      k = (int)(r % nb); r /= nb;
      col = (int)(r % g); r /= g;
      row = (int)(r % g); bi = (int)(r / g);
      frame = tile_frame[bi];
      bool ok = frame >= 0 && frame < n_frames;
      int y1 = 0, x1 = 0, H = 0, W = 0;
      if (ok) {
        H = frame_hw[2 * frame]; W = frame_hw[2 * frame + 1];
        y0 = tile_rect[4 * bi]; y1 = tile_rect[4 * bi + 1]; x0 = tile_rect[4 * bi + 2]; x1 = tile_rect[4 * bi + 3];
        ok = y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W;
      }
      if (!ok) {
        if (row == 0 && col == 0 && k == 0) atomicAdd(err, 1);       // one count per bad tile; it contributes no box
      } else {
        const float* cell = y + (((long long)bi * g + row) * g + col) * D;
        cf = cell[5 * k];
        if (cf > conf_th) {
          // the tile is the image: yolo_decode_conf_kernel's operations in its order
          const double ih = (double)(y1 - y0), iw = (double)(x1 - x0);
          const double gw = 1.0 * iw / g, gh = 1.0 * ih / g;
          double xc = (double)cell[5 * k + 1] * gw, yc = (double)cell[5 * k + 2] * gh;
          const double w_ = (double)cell[5 * k + 3] * iw, h_ = (double)cell[5 * k + 4] * ih;
          xc += col * gw; yc += row * gh;
          bx1 = xc - w_ / 2; by1 = yc - h_ / 2;
          bx2 = xc + w_ / 2; by2 = yc + h_ / 2;
          // a box that a window edge inside the frame may have cut is left to the neighbouring window (a NaN corner drops nothing)
          drop = margin >= 0 && ((x0 > 0 && bx1 < margin) || (x1 < W && bx2 > iw - margin) ||
                                 (y0 > 0 && by1 < margin) || (y1 < H && by2 > ih - margin));
          keep = !drop;
        }
      }
    }
    const unsigned long long m = __ballot(keep);
    const unsigned long long md = __ballot(drop);
    if (lane == 0) { wave_cnt[wave] = __popcll(m); wave_drop[wave] = __popcll(md); }
    __syncthreads();
    int before = 0, chunk_total = 0, chunk_drop = 0;
    for (int w = 0; w < 16; ++w) { const int cnt = wave_cnt[w]; if (w < wave) before += cnt; chunk_total += cnt; chunk_drop += wave_drop[w]; }
    const int base = base_s;
    if (keep) {
      const int o = base + before + __popcll(m & ((1ull << lane) - 1ull));
      if (o < max_boxes) {
        const float* cell = y + (((long long)bi * g + row) * g + col) * D;
        image_idx[o] = frame;
        conf[o] = cf;
        xy[4 * o + 0] = bx1 + (double)x0; xy[4 * o + 1] = by1 + (double)y0;
        xy[4 * o + 2] = bx2 + (double)x0; xy[4 * o + 3] = by2 + (double)y0;
        if (C > 0) {
          int best = 0; float bv = cell[5 * nb];
          for (int c = 1; c < C; ++c) { const float v = cell[5 * nb + c]; if (v > bv) { bv = v; best = c; } }
          cls[o] = best;
        }
        if (out_tile) out_tile[o] = bi;
      }
    }
    __syncthreads();
    if (t == 0) { base_s = base + chunk_total; drop_s += chunk_drop; }
    __syncthreads();
  }
  if (t == 0) { *count = base_s; *dropped += drop_s; }
}

}  // namespace

#define CY_S ((hipStream_t)stream)

extern "C" int cy_yolo_decode_tiles_conf(const float* y, const int* tile_frame, const int* tile_rect, const int* frame_hw, int n_frames,
                                         double margin, int Bt, int g, int nb, int C, float conf_th, int* count, int* dropped,
                                         int* image_idx, double* xy, int* cls, float* conf, int* out_tile, int max_boxes, int* err,
                                         void* stream) {
  CY_REQUIRE(Bt >= 0, "cy_yolo_decode_tiles_conf: Bt=%d tiles", Bt);
  CY_REQUIRE(g >= 1, "cy_yolo_decode_tiles_conf: g=%d", g);
  CY_REQUIRE(nb >= 1, "cy_yolo_decode_tiles_conf: nb=%d", nb);
  CY_REQUIRE(C >= 0, "cy_yolo_decode_tiles_conf: C=%d", C);
  CY_REQUIRE(n_frames >= 1, "cy_yolo_decode_tiles_conf: n_frames=%d", n_frames);
  CY_REQUIRE(max_boxes >= 0, "cy_yolo_decode_tiles_conf: max_boxes=%d", max_boxes);
  CY_REQUIRE(margin == margin, "cy_yolo_decode_tiles_conf: margin=%g (a negative margin switches the border rule off)", margin);
  if (Bt == 0 || max_boxes == 0) return 0;
  CY_REQUIRE(y, "cy_yolo_decode_tiles_conf: null argument (y)");
  CY_REQUIRE(tile_frame && tile_rect && frame_hw, "cy_yolo_decode_tiles_conf: null argument (tile_frame, tile_rect, frame_hw)");
  CY_REQUIRE(count && dropped && err, "cy_yolo_decode_tiles_conf: null argument (count, dropped, err)");
  CY_REQUIRE(image_idx && xy && conf, "cy_yolo_decode_tiles_conf: null argument (image_idx, xy, conf)");
  CY_REQUIRE(C == 0 || cls, "cy_yolo_decode_tiles_conf: cls must be given when C=%d", C);
  yolo_decode_tiles_kernel<<<1, 1024, 0, CY_S>>>(y, tile_frame, tile_rect, frame_hw, n_frames, margin, Bt, g, nb, C, conf_th, count, dropped,
                                                 image_idx, xy, cls, conf, out_tile, max_boxes, err);
  CY_LAUNCH_CHECK("cy_yolo_decode_tiles_conf");
  return 0;
}
