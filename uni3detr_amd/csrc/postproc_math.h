// The arithmetic of the test-time post-processing, one definition for the per-scene routines (postproc.hip: u3d_soft_nms,
// u3d_box_merge) and the batched tail (det_tail.hip: U3D_DET_TAIL_SOFT_NMS / _MERGE), whose results must agree bit for bit.
#pragma once
#include "box_iou.h"

// One Gaussian soft-NMS step: the score v of a box that overlaps the selected one by iou.  A multiply, a divide, expf and a multiply:
// nothing an inlining caller could contract into a fused multiply-add.
__device__ __forceinline__ float pp_soft_decay(float v, float iou, float sigma) { return v * expf(-iou * iou / sigma); }

// Box merging.  The reference hands its LiDAR boxes (x, y, z, dx, dy, dz, yaw) to a routine written for (x3d, y3d, z3d, l, h, w, yaw)
// camera boxes, so the polygon lives in the (x, z) plane with extents (dx, dz), rotated by -yaw, and the "height" interval is
// [y - dy, y]: reproduced as is.  Callers only compare the result with a threshold.
__device__ static float pp_merge_overlap(const float* p, const float* q) {
  Q2 a[4], b[4];
  pp_rect(0.f, 0.f, p[3], p[5], -p[6], a);
  pp_rect(q[0] - p[0], q[2] - p[2], q[3], q[5], -q[6], b);
  float ax0 = a[0].x, ax1 = a[0].x, az0 = a[0].y, az1 = a[0].y, bx0 = b[0].x, bx1 = b[0].x, bz0 = b[0].y, bz1 = b[0].y;
  for (int i = 1; i < 4; ++i) {
    ax0 = fminf(ax0, a[i].x); ax1 = fmaxf(ax1, a[i].x); az0 = fminf(az0, a[i].y); az1 = fmaxf(az1, a[i].y);
    bx0 = fminf(bx0, b[i].x); bx1 = fmaxf(bx1, b[i].x); bz0 = fminf(bz0, b[i].y); bz1 = fmaxf(bz1, b[i].y);
  }
  const float ay1 = fmaxf(p[1], p[1] - p[4]), ay0 = fminf(p[1], p[1] - p[4]);
  const float by1 = fmaxf(q[1], q[1] - q[4]), by0 = fminf(q[1], q[1] - q[4]);
  if (ax1 < bx0 || ax0 > bx1 || az1 < bz0 || az0 > bz1 || ay1 < by0 || ay0 > by1) return 0.f;
  const float area1 = fabsf(p[3] * p[5]), area2 = fabsf(q[3] * q[5]);
  // clip in whichever orientation the corner lists have (negative extents flip it): use absolute areas
  Q2 bb[4] = {b[0], b[1], b[2], b[3]};
  float cross = (b[1].x - b[0].x) * (b[2].y - b[1].y) - (b[1].y - b[0].y) * (b[2].x - b[1].x);
  if (cross < 0.f) { bb[1] = b[3]; bb[3] = b[1]; }
  const float shared = pp_inter_area(a, bb);
  const float shared_y = fminf(by1, ay1) - fmaxf(by0, ay0);
  const float inter = shared_y * shared;
  const float uni = (by1 - by0) * area2 + (ay1 - ay0) * area1;
  return inter / (uni - inter);
}

// numpy's median of m values from the element of rank (m - 1) / 2 (lo) and the one of rank m / 2 (hi): the mean of the two middle
// values for an even count.  An add and a multiply by a half: no contraction possible.
__device__ __forceinline__ float pp_median_of(float lo, float hi, int m) { return (m & 1) ? lo : 0.5f * (lo + hi); }
