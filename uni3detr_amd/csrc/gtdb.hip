// The GT-paste object database (mmdet3d create_groundtruth_database / the plugin's create_unified_gt_database, recalled) cropped on the
// device: every box of every scene becomes one object holding the scene's points strictly inside it, in scene order, columns 0-2
// relative to the box's (x, y, z_bottom).  A point inside two boxes goes to both.  It is a stable segmented compaction straight from
// the packed points and boxes - no point x box bit matrix, no atomics, so the output is the same bytes on every run:
//   k_gtdb_pass<false>  one workgroup per (scene, 256-point tile): per box of the scene the tile's inside count (ballot + popcount per
//                       wave) -> tile_ws[box row][tile]
//   k_gtdb_tile_scan    one workgroup per box row: exclusive scan over the tiles in place (count -> base), the sum -> num_points
//   k_gtdb_obj_scan     one wave: exclusive scan of num_points -> obj_off, the total as int64 (the caller's one host read)
//   k_gtdb_pass<true>   the same traversal; a point inside box j goes to row obj_off[j] + tile base + rank within the tile
// The scene's boxes are staged through LDS GD_BLK at a time (point_box.h: the inside test GT-paste uses); a thread keeps its point's
// columns in registers and one bit per staged box.
#include "common.h"
#include "point_box.h"

#define GD_T 256
#define GD_BLK 64           // boxes per LDS block: one bit of a 64-bit register mask each
#define GD_MAXF 8
#define GD_MAX_BOXES 1024   // per scene (the GT-paste kernels' OA_CAP)

template <bool WRITE>
__global__ void __launch_bounds__(GD_T) k_gtdb_pass(const float* __restrict__ pts, long long n_rows, const int32_t* __restrict__ scene_off,
                                                    const int32_t* __restrict__ n_live, int feat, int tiles,
                                                    const float* __restrict__ boxes, int n_boxes, const int32_t* __restrict__ box_off,
                                                    const int32_t* __restrict__ box_valid, int dim, int32_t* __restrict__ tile_ws,
                                                    const int32_t* __restrict__ obj_off, long long out_rows, float* __restrict__ out) {
  __shared__ float bs[GD_BLK][8];
  __shared__ int wc[GD_BLK][GD_T / 64];
  const int b = blockIdx.y, t = blockIdx.x, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int live = n_live ? n_live[b] : scene_off[b + 1] - scene_off[b];
  const int q0 = box_off[b], nq = min(box_off[b + 1] - q0, n_boxes - q0);
  if (q0 < 0 || nq <= 0) return;
  if ((long long)t * GD_T >= live) {                       // no live point in this tile: every box counts 0 here
    if (!WRITE)
      for (int j = threadIdx.x; j < nq; j += GD_T) tile_ws[(long long)(q0 + j) * tiles + t] = 0;
    return;
  }
  const int i = t * GD_T + threadIdx.x;
  const long long row = (long long)scene_off[b] + i;
  const bool valid = i < live && row >= 0 && row < n_rows;
  float v[GD_MAXF];
#pragma unroll
  for (int f = 0; f < GD_MAXF; ++f) v[f] = (valid && (f < 3 || (WRITE && f < feat))) ? pts[row * feat + f] : 0.f;
  for (int c0 = 0; c0 < nq; c0 += GD_BLK) {
    const int nc = min(GD_BLK, nq - c0);
    __syncthreads();
    if (threadIdx.x < nc) {
      const int r = q0 + c0 + threadIdx.x;
      pb_stage(bs[threadIdx.x], boxes + (long long)r * dim, !box_valid || box_valid[r] != 0);
    }
    __syncthreads();
    unsigned long long mine = 0;
    for (int j = 0; j < nc; ++j) {
      const bool in = valid && pb_inside(v[0], v[1], v[2], bs[j]);
      const unsigned long long m = __ballot(in);
      if (lane == 0) wc[j][wv] = __popcll(m);
      mine |= (unsigned long long)in << j;
    }
    __syncthreads();
    if (!WRITE) {
      if (threadIdx.x < nc)
        tile_ws[(long long)(q0 + c0 + threadIdx.x) * tiles + t] = wc[threadIdx.x][0] + wc[threadIdx.x][1] + wc[threadIdx.x][2] + wc[threadIdx.x][3];
      continue;
    }
    for (int j = 0; j < nc; ++j) {
      const bool in = (mine >> j) & 1ull;
      const unsigned long long m = __ballot(in);
      if (!in) continue;
      int before = 0;
      for (int w = 0; w < wv; ++w) before += wc[j][w];
      const int r = q0 + c0 + j;
      const long long o = (long long)obj_off[r] + tile_ws[(long long)r * tiles + t] + before + __popcll(m & ((1ull << lane) - 1ull));
      if (o < 0 || o >= out_rows) continue;                // never taken when obj_off / tile_ws come from the count pass of the same input
      float* dst = out + o * feat;
      dst[0] = v[0] - bs[j][0];
      dst[1] = v[1] - bs[j][1];
      dst[2] = v[2] - bs[j][2];
#pragma unroll
      for (int f = 3; f < GD_MAXF; ++f)
        if (f < feat) dst[f] = v[f];
    }
  }
}

__global__ void __launch_bounds__(GD_T) k_gtdb_tile_scan(int32_t* __restrict__ tile_ws, int tiles, int32_t* __restrict__ num_points) {
  __shared__ int sh[4];
  int32_t* w = tile_ws + (long long)blockIdx.x * tiles;
  int carry = 0;                                           // at most the scene's points: fits
  for (int k0 = 0; k0 < tiles; k0 += GD_T) {
    const int k = k0 + threadIdx.x;
    int tot;
    const int ex = pb_scan256(k < tiles ? w[k] : 0, sh, tot);
    if (k < tiles) w[k] = carry + ex;
    carry += tot;
  }
  if (threadIdx.x == 0) num_points[blockIdx.x] = carry;
}

// obj_off wraps when the total passes int32; the total itself is exact, and u3d_gtdb_crop refuses such a total
__global__ void __launch_bounds__(64) k_gtdb_obj_scan(const int32_t* __restrict__ num_points, int n_boxes, int32_t* __restrict__ obj_off,
                                                      long long* __restrict__ total) {
  const int lane = threadIdx.x;
  long long carry = 0;
  for (int k0 = 0; k0 < n_boxes; k0 += 64) {
    const int k = k0 + lane;
    const long long val = k < n_boxes ? num_points[k] : 0;
    long long x = val;
    for (int d = 1; d < 64; d <<= 1) {
      const long long y = __shfl_up(x, d, 64);
      if (lane >= d) x += y;
    }
    if (k < n_boxes) obj_off[k] = (int32_t)(carry + x - val);
    carry += __shfl(x, 63, 64);
  }
  if (lane == 0) {
    obj_off[n_boxes] = (int32_t)carry;
    total[0] = carry;
  }
}

static int32_t gd_check(const float* points, int64_t n_rows, const int32_t* scene_off, int32_t batch, int32_t feat, int32_t tiles,
                        const float* boxes, int32_t n_boxes, const int32_t* box_off, int32_t box_dim, int32_t max_boxes,
                        const int32_t* tile_ws) {
  U3D_REQUIRE(scene_off && box_off && batch > 0 && batch <= 65535 && feat >= 3 && feat <= GD_MAXF && tiles >= 0 && n_boxes >= 0 &&
                  n_rows >= 0 && max_boxes >= 0 && (box_dim == 7 || box_dim == 9),
              U3D_ERR_ARG);
  U3D_REQUIRE(max_boxes <= GD_MAX_BOXES, U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE((int64_t)n_boxes * tiles <= INT32_MAX, U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE(tiles == 0 || n_boxes == 0 || (points && boxes && tile_ws), U3D_ERR_ARG);
  return U3D_OK;
}

extern "C" int32_t u3d_gtdb_count(const float* points, int64_t n_rows, const int32_t* scene_off, const int32_t* n_live, int32_t batch,
                                  int32_t feat, int32_t tiles, const float* boxes, int32_t n_boxes, const int32_t* box_off,
                                  const int32_t* box_valid, int32_t box_dim, int32_t max_boxes, int32_t* tile_ws, u3d_stream s) {
  const int32_t rc = gd_check(points, n_rows, scene_off, batch, feat, tiles, boxes, n_boxes, box_off, box_dim, max_boxes, tile_ws);
  if (rc != U3D_OK) return rc;
  if (tiles == 0 || n_boxes == 0) return U3D_OK;
  k_gtdb_pass<false><<<dim3(tiles, batch), GD_T, 0, (hipStream_t)s>>>(points, (long long)n_rows, scene_off, n_live, feat, tiles, boxes,
                                                                     n_boxes, box_off, box_valid, box_dim, tile_ws, nullptr, 0, nullptr);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_gtdb_scan(int32_t* tile_ws, int32_t n_boxes, int32_t tiles, int32_t* num_points, int32_t* obj_off, int64_t* total,
                                 u3d_stream s) {
  U3D_REQUIRE(obj_off && total && n_boxes >= 0 && tiles >= 0 && (n_boxes == 0 || num_points) && (n_boxes == 0 || tiles == 0 || tile_ws),
              U3D_ERR_ARG);
  U3D_REQUIRE((int64_t)n_boxes * tiles <= INT32_MAX, U3D_ERR_UNSUPPORTED);
  if (n_boxes > 0) {
    k_gtdb_tile_scan<<<n_boxes, GD_T, 0, (hipStream_t)s>>>(tile_ws, tiles, num_points);
    U3D_CHECK_LAUNCH();
  }
  k_gtdb_obj_scan<<<1, 64, 0, (hipStream_t)s>>>(num_points, n_boxes, obj_off, (long long*)total);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_gtdb_crop(const float* points, int64_t n_rows, const int32_t* scene_off, const int32_t* n_live, int32_t batch,
                                 int32_t feat, int32_t tiles, const float* boxes, int32_t n_boxes, const int32_t* box_off,
                                 const int32_t* box_valid, int32_t box_dim, int32_t max_boxes, const int32_t* tile_ws,
                                 const int32_t* obj_off, int64_t total, float* out, u3d_stream s) {
  const int32_t rc = gd_check(points, n_rows, scene_off, batch, feat, tiles, boxes, n_boxes, box_off, box_dim, max_boxes, tile_ws);
  if (rc != U3D_OK) return rc;
  U3D_REQUIRE(total >= 0, U3D_ERR_ARG);
  U3D_REQUIRE(total <= INT32_MAX, U3D_ERR_UNSUPPORTED);    // the int32 object offsets of this chunk have wrapped: crop fewer scenes at once
  if (tiles == 0 || n_boxes == 0 || total == 0) return U3D_OK;
  U3D_REQUIRE(obj_off && out, U3D_ERR_ARG);
  k_gtdb_pass<true><<<dim3(tiles, batch), GD_T, 0, (hipStream_t)s>>>(points, (long long)n_rows, scene_off, n_live, feat, tiles, boxes,
                                                                    n_boxes, box_off, box_valid, box_dim, (int32_t*)tile_ws, obj_off,
                                                                    (long long)total, out);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
