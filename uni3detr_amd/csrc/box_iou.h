// Rotated-box IoU device helpers shared by postproc.hip (soft-NMS, box merging) and eval.hip (indoor detection evaluation).
// pp_iou3d is the arithmetic of mmdet3d's bbox_overlaps_3d / DepthInstance3DBoxes.overlaps (oracle/boxes.py::bbox_overlaps_3d).
#pragma once
#include <hip/hip_runtime.h>

struct Q2 { float x, y; };

__device__ static int pp_clip(const Q2* in, int n, Q2 a, Q2 b, Q2* out) {
  int m = 0;
  for (int i = 0; i < n; ++i) {
    Q2 p = in[i], q = in[(i + 1 == n) ? 0 : i + 1];
    float sp = (b.x - a.x) * (p.y - a.y) - (b.y - a.y) * (p.x - a.x);
    float sq = (b.x - a.x) * (q.y - a.y) - (b.y - a.y) * (q.x - a.x);
    if (sp >= 0.f) out[m++] = p;
    if ((sp >= 0.f) != (sq >= 0.f)) {
      float t = sp / (sp - sq);
      out[m++] = Q2{p.x + t * (q.x - p.x), p.y + t * (q.y - p.y)};
    }
  }
  return m;
}
__device__ static void pp_rect(float cx, float cy, float w, float h, float ang, Q2* c) {
  float cs = cosf(ang), sn = sinf(ang);
  const float sx[4] = {-0.5f, 0.5f, 0.5f, -0.5f}, sy[4] = {-0.5f, -0.5f, 0.5f, 0.5f};
  for (int i = 0; i < 4; ++i) {
    float x = sx[i] * w, y = sy[i] * h;
    c[i] = Q2{cx + x * cs - y * sn, cy + x * sn + y * cs};
  }
}
// intersection area of two rectangles given as counter-clockwise corner lists (the second one relative to the first's frame)
__device__ static float pp_inter_area(const Q2* a, const Q2* b) {
  Q2 poly[12], tmp[12];
  for (int i = 0; i < 4; ++i) poly[i] = a[i];
  int m = 4;
  for (int e = 0; e < 4 && m > 0; ++e) {
    m = pp_clip(poly, m, b[e], b[(e + 1) & 3], tmp);
    for (int t = 0; t < m; ++t) poly[t] = tmp[t];
  }
  float inter = 0.f;
  if (m >= 3) {
    for (int t = 0; t < m; ++t) {
      Q2 u = poly[t], v = poly[(t + 1 == m) ? 0 : t + 1];
      inter += u.x * v.y - v.x * u.y;
    }
    inter = fabsf(inter) * 0.5f;
  }
  return inter;
}
// rotated 3-D IoU of bottom-centre LiDAR boxes (x, y, z_bottom, dx, dy, dz, yaw): the arithmetic of k_iou3d_rotated_aligned (query.hip)
__device__ static float pp_iou3d(const float* p, const float* q) {
  float w1 = fmaxf(p[3], 1e-4f), h1 = fmaxf(p[4], 1e-4f), w2 = fmaxf(q[3], 1e-4f), h2 = fmaxf(q[4], 1e-4f);
  float a1 = w1 * h1, a2 = w2 * h2, iou2d = 0.f;
  if (a1 >= 1e-14f && a2 >= 1e-14f) {
    Q2 ra[4], rb[4];
    pp_rect(0.f, 0.f, w1, h1, p[6], ra);
    pp_rect(q[0] - p[0], q[1] - p[1], w2, h2, q[6], rb);
    float inter = pp_inter_area(ra, rb);
    iou2d = inter / (a1 + a2 - inter);
  }
  float ov_bev = iou2d * (a1 + a2) / (1.f + iou2d);
  float top = fminf(p[2] + p[5], q[2] + q[5]), bot = fmaxf(p[2], q[2]);
  float ov = ov_bev * fmaxf(top - bot, 0.f);
  float v1 = p[3] * p[4] * p[5], v2 = q[3] * q[4] * q[5];
  return ov / fmaxf(v1 + v2 - ov, 1e-8f);
}
