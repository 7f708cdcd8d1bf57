// Per-box flip -> rotate -> scale -> translate of the on-device data path, shared by datapath.hip (u3d_boxes_augment) and tta.hip
// (the test-time-augmentation map-back, which must be bit-identical to a u3d_boxes_augment call with the inverse parameters).
// Parameters: f32 [U3D_AUG_NPARAM] = (flip_horizontal, flip_vertical, sin(angle), cos(angle), angle, scale, tx, ty, tz).
#pragma once
#include <hip/hip_runtime.h>

// coord: 0 = Depth (SUN RGB-D / ScanNet boxes), 1 = LiDAR (KITTI / nuScenes).  Flip axes follow mmdet3d v1.0 (recalled):
//   Depth : horizontal x -> -x (yaw -> pi - yaw), vertical y -> -y (yaw -> -yaw)
//   LiDAR : horizontal y -> -y (yaw -> -yaw),     vertical x -> -x (yaw -> pi - yaw)
__device__ __forceinline__ void dp_flip_xy(int coord, bool fh, bool fv, float& x, float& y) {
  if (coord == 0) { if (fh) x = -x; if (fv) y = -y; }
  else { if (fh) y = -y; if (fv) x = -x; }
}

// in [dim] -> out [dim] (dim 7 or 9; in may alias out): (x, y, z, dx, dy, dz, yaw [, vx, vy]) under the parameter row p
__device__ __forceinline__ void dp_box_augment(const float* in, float* out, int dim, const float* p, int coord) {
  const bool fh = p[0] != 0.f, fv = p[1] != 0.f;
  float x = in[0], y = in[1], z = in[2], yaw = in[6];
  const float dx = in[3], dy = in[4], dz = in[5];
  dp_flip_xy(coord, fh, fv, x, y);
  const float PI = 3.14159265358979323846f;
  if (coord == 0) { if (fh) yaw = -yaw + PI; if (fv) yaw = -yaw; }
  else { if (fh) yaw = -yaw; if (fv) yaw = -yaw + PI; }
  const float s = p[2], c = p[3], sc = p[5];
  float vx = 0.f, vy = 0.f;
  if (dim >= 9) { vx = in[7]; vy = in[8]; }
  out[0] = (x * c - y * s) * sc + p[6];
  out[1] = (x * s + y * c) * sc + p[7];
  out[2] = z * sc + p[8];
  out[3] = dx * sc; out[4] = dy * sc; out[5] = dz * sc;
  out[6] = yaw + p[4];
  if (dim >= 9) {      // velocities flip and rotate with the frame and SCALE with it (mmdet3d BaseInstance3DBoxes.scale: tensor[:, 7:] *= s, recalled)
    dp_flip_xy(coord, fh, fv, vx, vy);
    out[7] = (vx * c - vy * s) * sc;
    out[8] = (vx * s + vy * c) * sc;
  }
}
