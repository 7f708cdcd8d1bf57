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
// rotated BEV IoU of (cx, cy, w, h, angle) rows: the arithmetic of bev_iou_rot (query.hip, class-aware NMS) on 5-column rows
// (tta.hip: the box merge of test-time augmentation)
__device__ static float pp_iou_bev(const float* p, const float* q) {
  float a1 = p[2] * p[3], a2 = q[2] * q[3];
  if (a1 <= 0.f || a2 <= 0.f) return 0.f;
  Q2 ra[4], rb[4];
  pp_rect(0.f, 0.f, p[2], p[3], p[4], ra);
  pp_rect(q[0] - p[0], q[1] - p[1], q[2], q[3], q[4], rb);
  float inter = pp_inter_area(ra, rb);
  return inter / fmaxf(a1 + a2 - inter, 1e-8f);
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

// ---- rectangle corners and the upstream BEV collision test (GT-paste / ObjectNoise, objaug.hip) ----
// Corner order of mmdet3d's box2d_to_corner_jit (recalled): (-.5,-.5), (-.5,.5), (.5,.5), (.5,-.5) times (dx, dy), rotated
// counter-clockwise by yaw, plus the centre - a clockwise list for dx, dy > 0.
__device__ static void bx_corners(float cx, float cy, float dx, float dy, float yaw, Q2* c) {
  const float cs = cosf(yaw), sn = sinf(yaw);
  const float sx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, sy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
  for (int i = 0; i < 4; ++i) {
    const float x = sx[i] * dx, y = sy[i] * dy;
    c[i] = Q2{x * cs - y * sn + cx, x * sn + y * cs + cy};
  }
}
// mmdet3d data_augment_utils.box_collision_test (recalled, clockwise=True) for one pair: the standup boxes overlap and either two
// edges cross or one rectangle holds all four corners of the other.
__device__ static bool bx_collide(const Q2* a, const Q2* b) {
  float ax0 = a[0].x, ax1 = a[0].x, ay0 = a[0].y, ay1 = a[0].y, bx0 = b[0].x, bx1 = b[0].x, by0 = b[0].y, by1 = b[0].y;
  for (int i = 1; i < 4; ++i) {
    ax0 = fminf(ax0, a[i].x); ax1 = fmaxf(ax1, a[i].x); ay0 = fminf(ay0, a[i].y); ay1 = fmaxf(ay1, a[i].y);
    bx0 = fminf(bx0, b[i].x); bx1 = fmaxf(bx1, b[i].x); by0 = fminf(by0, b[i].y); by1 = fmaxf(by1, b[i].y);
  }
  if (!(fminf(ax1, bx1) - fmaxf(ax0, bx0) > 0.f) || !(fminf(ay1, by1) - fmaxf(ay0, by0) > 0.f)) return false;
  for (int k = 0; k < 4; ++k) {
    const Q2 A = a[k], B = a[(k + 1) & 3];
    for (int l = 0; l < 4; ++l) {
      const Q2 C = b[l], D = b[(l + 1) & 3];
      const bool acd = (D.y - A.y) * (C.x - A.x) > (C.y - A.y) * (D.x - A.x);
      const bool bcd = (D.y - B.y) * (C.x - B.x) > (C.y - B.y) * (D.x - B.x);
      if (acd != bcd) {
        const bool abc = (C.y - A.y) * (B.x - A.x) > (B.y - A.y) * (C.x - A.x);
        const bool abd = (D.y - A.y) * (B.x - A.x) > (B.y - A.y) * (D.x - A.x);
        if (abc != abd) return true;
      }
    }
  }
  for (int pass = 0; pass < 2; ++pass) {           // pass 0: a holds every corner of b; pass 1: the other way round
    const Q2* o = pass ? b : a;
    const Q2* q = pass ? a : b;
    bool holds = true;
    for (int l = 0; l < 4 && holds; ++l)
      for (int k = 0; k < 4; ++k) {
        const float vx = o[(k + 1) & 3].x - o[k].x, vy = o[(k + 1) & 3].y - o[k].y;
        if (vy * (o[k].x - q[l].x) - vx * (o[k].y - q[l].y) >= 0.f) { holds = false; break; }
      }
    if (holds) return true;
  }
  return false;
}
