// Point-in-box test shared by the GT-paste kernels (objaug.hip) and the object-database crop (gtdb.hip), so that what GT-paste removes
// and what the database holds are decided by one piece of arithmetic.  Boxes are bottom-centre (x, y, z, dx, dy, dz, yaw [, vx, vy]);
// a point is inside when it is strictly inside all six faces (mmdet3d points_in_rbbox with origin (0.5, 0.5, 0), recalled).
#pragma once
#include "common.h"

// a box row staged as 8 floats: centre x, y, bottom z, half dx (-1 when the box is switched off: it then holds nothing), half dy, dz,
// cos(yaw), sin(yaw)
__device__ __forceinline__ void pb_stage(float* b, const float* r, bool on) {
  b[0] = r[0]; b[1] = r[1]; b[2] = r[2];
  b[3] = on ? 0.5f * r[3] : -1.f;
  b[4] = 0.5f * r[4]; b[5] = r[5]; b[6] = cosf(r[6]); b[7] = sinf(r[6]);
}

__device__ __forceinline__ bool pb_inside(float px, float py, float pz, const float* b) {
  const float dx = px - b[0], dy = py - b[1];
  const float lx = dx * b[6] + dy * b[7], ly = -dx * b[7] + dy * b[6];
  return fabsf(lx) < b[3] && fabsf(ly) < b[4] && pz > b[2] && pz < b[2] + b[5];
}

// exclusive scan of one int per thread over a 256-thread workgroup (sh: 4 ints of LDS); every thread must call it
__device__ __forceinline__ int pb_scan256(int v, int* sh, int& total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int x = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  if (lane == 63) sh[w] = x;
  __syncthreads();
  int base = 0;
  for (int i = 0; i < w; ++i) base += sh[i];
  total = sh[0] + sh[1] + sh[2] + sh[3];
  __syncthreads();
  return base + x - v;
}
