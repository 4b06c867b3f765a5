// The IoU of two boxes, shared by confusion_sweep_kernel (predict.hip) and nms_sweep_kernel (nms.hip): one copy, so a pair has
// the same IoU, bit for bit, in the metric sweeps and in the suppression step.
#pragma once
#include "common.h"

// the double arithmetic below restates numpy expressions operation by operation: no fused multiply-add
#pragma clang fp contract(off)

// IoU of metrics.calc_iou_individual (metrics.py:121-133) with its early-out; a = ground truth, p = prediction
__device__ __forceinline__ double box_iou(const double* a, const double* p) {
  const double x1t = a[0], y1t = a[1], x2t = a[2], y2t = a[3];
  const double x1p = p[0], y1p = p[1], x2p = p[2], y2p = p[3];
  if (x2t < x1p || x2p < x1t || y2t < y1p || y2p < y1t) return 0.0;
  const double inter = (fmin(x2t, x2p) - fmax(x1t, x1p)) * (fmin(y2t, y2p) - fmax(y1t, y1p));
  return inter / ((x2t - x1t) * (y2t - y1t) + (x2p - x1p) * (y2p - y1p) - inter);
}
