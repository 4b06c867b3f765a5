// Box drawing on the device (gfx950): plot.draw_boxes (plot.py:24-33) for every box of a chunk of images in one launch, into
// the packed uint8 buffer that crop_resize_u8_kernel (predict.hip) reads.  DESIGN section 6g.
//   draw_boxes_u8_kernel   cv2.rectangle(img, (x1, y1), (x2, y2), color, 1) and the class index in a 5 x 7 digit font
#include "common.h"

namespace {

enum { GLYPH_W = 5, GLYPH_H = 7, GLYPH_PITCH = GLYPH_W + 1, LABEL_W = 3 * GLYPH_PITCH - 1, LABEL_CELLS = LABEL_W * GLYPH_H };

// floor((a + b) / 2): Python's (a + b) // 2 (an arithmetic shift rounds towards minus infinity)
__device__ __forceinline__ long long floor_mid(int a, int b) { return ((long long)a + (long long)b) >> 1; }

// Is (x, y) a cell of the label block of a box that the digits of `lab` (0..999) set?  The block's bottom-left corner is
// (xc, yc): glyph rows yc-6 .. yc, glyph k columns xc + 6 k .. xc + 6 k + 4, most significant digit first.
__device__ __forceinline__ bool label_sets(long long xc, long long yc, int lab, long long x, long long y,
                                           const unsigned char* __restrict__ glyphs) {
  const long long r = y - (yc - (GLYPH_H - 1)), c = x - xc;
  const int nd = lab < 10 ? 1 : (lab < 100 ? 2 : 3);
  if (r < 0 || r >= GLYPH_H || c < 0 || c >= nd * GLYPH_PITCH - 1) return false;
  const int k = (int)c / GLYPH_PITCH, col = (int)c - k * GLYPH_PITCH;
  if (col >= GLYPH_W) return false;                                  // the empty column between two digits
  const int left = nd - 1 - k;                                       // decimal places to the right of digit k
  const int digit = (left == 2 ? lab / 100 : (left == 1 ? lab / 10 : lab)) % 10;
  return (glyphs[digit * GLYPH_H + (int)r] >> (GLYPH_W - 1 - col)) & 1;
}

// Does box (x1, y1, x2, y2, lab) set pixel (x, y)?  The outline rule of the header, then the label.
__device__ __forceinline__ bool box_sets(int x1, int y1, int x2, int y2, int lab, int x, int y,
                                         const unsigned char* __restrict__ glyphs) {
  const int xlo = min(x1, x2), xhi = max(x1, x2), ylo = min(y1, y2), yhi = max(y1, y2);
  if ((y == y1 || y == y2) && x >= xlo && x <= xhi) return true;
  if ((x == x1 || x == x2) && y >= ylo && y <= yhi) return true;
  return lab >= 0 && label_sets(floor_mid(x1, x2), floor_mid(y1, y2), lab, x, y, glyphs);
}

// One thread per (box, item).  The items of a box are the pixels of its outline that lie inside the image -- cw for the row
// y1, cw for the row y2, ch for the column x1, ch for the column x2, with cw / ch the number of image columns / rows the box
// spans -- followed, for a labelled box, by the 17 x 7 cells of the label block.  An item that names a pixel the box sets is
// stored unless a LATER box of the same image sets that pixel too (the boxes of an image are contiguous, image index
// ascending): then that box's thread stores it.  So every pixel has one owner, the highest box index that sets it, which is
// what drawing the boxes one after the other leaves behind, and no two threads ever store different bytes to one address.
// (Two items of ONE box may name the same pixel, a corner or a glyph cell on the outline: both store the same colour.)
__global__ __launch_bounds__(256) void draw_boxes_u8_kernel(unsigned char* __restrict__ imgs, const long long* __restrict__ img_off,
                                                            const int* __restrict__ img_hw, int n_images, long long imgs_bytes,
                                                            const int* __restrict__ box_img, const int* __restrict__ box_xy,
                                                            const unsigned char* __restrict__ box_color, const int* __restrict__ box_label,
                                                            int n, int max_items, long long total,
                                                            const unsigned char* __restrict__ glyphs, int* err) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int b = (int)(i / max_items), it = (int)(i - (long long)b * max_items);
  const int img = box_img[b];
  const int lab = box_label ? box_label[b] : -1;
  bool ok = img >= 0 && img < n_images && lab >= -1 && lab <= 999 && (b == 0 || box_img[b - 1] <= img);
  int H = 0, W = 0;
  long long off = 0;
  if (ok) {
    H = img_hw[2 * img];
    W = img_hw[2 * img + 1];
    off = img_off[img];
    ok = H >= 1 && W >= 1 && off >= 0 && off + (long long)H * W * 3 <= imgs_bytes;
  }
  const int x1 = box_xy[4 * b], y1 = box_xy[4 * b + 1], x2 = box_xy[4 * b + 2], y2 = box_xy[4 * b + 3];
  int cx0 = 0, cy0 = 0, cw = 0, ch = 0;
  long long items = 0;
  if (ok) {
    cx0 = max(min(x1, x2), 0);
    cy0 = max(min(y1, y2), 0);
    const int cx1 = min(max(x1, x2), W - 1), cy1 = min(max(y1, y2), H - 1);
    cw = cx1 >= cx0 ? cx1 - cx0 + 1 : 0;                             // cx0 >= 0 and cx1 <= W - 1: no overflow
    ch = cy1 >= cy0 ? cy1 - cy0 + 1 : 0;
    items = 2ll * cw + 2ll * ch + (lab >= 0 ? LABEL_CELLS : 0);
    ok = items <= max_items;
  }
  if (!ok) {
    if (it == 0) atomicAdd(err, 1);                                  // one count per bad box; it draws nothing
    return;
  }
  if (it >= items) return;
  int x, y;
  bool sets;
  if (it < 2 * cw) {                                                 // the rows y1 and y2
    const bool second = it >= cw;
    x = cx0 + (second ? it - cw : it);
    y = second ? y2 : y1;
    sets = y >= 0 && y < H;
  } else if (it < 2 * cw + 2 * ch) {                                 // the columns x1 and x2
    const int k = it - 2 * cw;
    const bool second = k >= ch;
    y = cy0 + (second ? k - ch : k);
    x = second ? x2 : x1;
    sets = x >= 0 && x < W;
  } else {                                                           // the label block
    const int cell = it - 2 * cw - 2 * ch;
    const int r = cell / LABEL_W, c = cell - r * LABEL_W;
    const long long xc = floor_mid(x1, x2), yc = floor_mid(y1, y2);
    const long long lx = xc + c, ly = yc - (GLYPH_H - 1) + r;
    sets = lx >= 0 && lx < W && ly >= 0 && ly < H && label_sets(xc, yc, lab, lx, ly, glyphs);
    x = (int)lx;
    y = (int)ly;
  }
  if (!sets) return;
  for (int j = b + 1; j < n && box_img[j] == img; ++j) {
    const int lj = box_label ? box_label[j] : -1;
    if (lj < -1 || lj > 999) continue;                               // a refused box draws nothing, so it hides nothing
    if (box_sets(box_xy[4 * j], box_xy[4 * j + 1], box_xy[4 * j + 2], box_xy[4 * j + 3], lj, x, y, glyphs)) return;
  }
  // 0 <= x < W and 0 <= y < H, and the image lies inside [0, imgs_bytes): three byte stores at a 64-bit offset
  unsigned char* p = imgs + off + ((long long)y * W + x) * 3;
  p[0] = box_color[3 * b];
  p[1] = box_color[3 * b + 1];
  p[2] = box_color[3 * b + 2];
}

}  // namespace

extern "C" int cy_draw_boxes_u8(unsigned char* imgs, const long long* img_off, const int* img_hw, int n_images, long long imgs_bytes,
                                const int* box_img, const int* box_xy, const unsigned char* box_color, const int* box_label, int n,
                                int max_items, const unsigned char* glyphs, int* err, void* stream) {
  CY_REQUIRE(n >= 0, "cy_draw_boxes_u8: n = %d boxes", n);
  if (n == 0) return 0;
  CY_REQUIRE(imgs && img_off && img_hw && box_img && box_xy && box_color && err, "cy_draw_boxes_u8: null argument");
  CY_REQUIRE(!box_label || glyphs, "cy_draw_boxes_u8: labels need the glyph table");
  CY_REQUIRE(n_images > 0 && imgs_bytes > 0 && max_items > 0, "cy_draw_boxes_u8: bad sizes");
  const long long total = (long long)n * max_items;
  CY_REQUIRE(cy_ceil_div(total, 256) < (1ll << 31), "cy_draw_boxes_u8: %lld items are too many for one launch", total);
  draw_boxes_u8_kernel<<<(unsigned)cy_ceil_div(total, 256), 256, 0, (hipStream_t)stream>>>(
      imgs, img_off, img_hw, n_images, imgs_bytes, box_img, box_xy, box_color, box_label, n, max_items, total, glyphs, err);
  CY_LAUNCH_CHECK("cy_draw_boxes_u8");
  return 0;
}
