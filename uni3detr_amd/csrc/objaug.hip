// GT-paste (mmdet3d ObjectSample / the plugin's UnifiedObjectSample) and ObjectNoise on a packed batch in HBM.
//
// The random draws stay on the host (uni3detr_amd/datapath.py, as upstream draws them per sample); everything that depends on the
// scene's geometry runs here:
//   ObjectSample : BEV collision of the drawn candidates against the scene's GT and each other (k_oa_collide), the greedy accept of
//                  UnifiedDataBaseSampler.sample_class_v2 (ref: projects/mmdet3d_plugin/datasets/pipelines/dbsampler.py, k_oa_greedy),
//                  removal of the scene points inside an accepted box (k_oa_mask), and the paste into an exactly packed output
//                  (k_oa_layout, k_oa_scatter_kept, k_oa_paste, k_oa_boxes_out).
//   ObjectNoise  : mmdet3d noise_per_object_v3_ with global_rot_range = 0 (recalled): per box, the lowest collision-free try
//                  (k_oa_noise_search), then every point moves with the lowest-index original box that holds it (k_oa_point_move).
// Boxes are bottom-centre (x, y, z, dx, dy, dz, yaw [, vx, vy]); a point is inside a box when it is strictly inside all six faces
// (mmdet3d points_in_rbbox with origin (0.5, 0.5, 0), recalled).  Everything is deterministic and order-preserving.
#include "common.h"
#include "box_iou.h"
#include "point_box.h"

#define OA_T 256            // threads per workgroup of every kernel except k_oa_greedy (one wave)
#define OA_CAP 1024         // boxes staged in LDS per scene (collision, noise search)
#define OA_CHUNK 256        // boxes staged per round by the point kernels

__device__ __forceinline__ int oa_live(const int32_t* live, const int32_t* off, int b) {
  return live ? live[b] : off[b + 1] - off[b];
}

// stats = [n_live[B] | g_live[B] | hist[B][C]]: live points, live GT rows, GT rows per class label in [0, C)
__global__ void __launch_bounds__(OA_T) k_oa_stats(const int32_t* scene_off, const int32_t* count, const int32_t* gt_off,
                                                   const int32_t* gt_count, const int32_t* labels, int batch, int ncls, int32_t* stats) {
  __shared__ int h[64];
  const int b = blockIdx.x;
  if (threadIdx.x < 64) h[threadIdx.x] = 0;
  __syncthreads();
  const int g = oa_live(gt_count, gt_off, b);
  for (int i = threadIdx.x; i < g; i += OA_T) {
    const int l = labels[gt_off[b] + i];
    if (l >= 0 && l < ncls) atomicAdd(&h[l], 1);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    stats[b] = oa_live(count, scene_off, b);
    stats[batch + b] = g;
  }
  if (threadIdx.x < ncls) stats[2 * batch + b * ncls + threadIdx.x] = h[threadIdx.x];
}

// candidate k (scene b, local index kl): hit[k] = collides with a live GT box of the scene; cc[k][w] bit j = collides with the
// scene's candidate 32w + j (j != kl).  Host guarantees cand_off[b+1] - cand_off[b] <= min(32 * words, OA_CAP).
__global__ void __launch_bounds__(OA_T) k_oa_collide(const float* gt, const int32_t* gt_off, const int32_t* g_live, int dim,
                                                     const float* db_boxes, const int32_t* cand_ids, const int32_t* cand_off, int words,
                                                     int32_t* hit, uint32_t* cc) {
  __shared__ Q2 cs[OA_CAP][4];
  __shared__ Q2 gs[OA_CHUNK][4];
  __shared__ int hs[OA_CAP];
  const int b = blockIdx.x, k0 = cand_off[b], nk = cand_off[b + 1] - k0;
  if (nk <= 0 || nk > OA_CAP || nk > 32 * words) return;
  for (int k = threadIdx.x; k < nk; k += OA_T) {
    const float* r = db_boxes + (long long)cand_ids[k0 + k] * dim;
    bx_corners(r[0], r[1], r[3], r[4], r[6], cs[k]);
    hs[k] = 0;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < nk * words; it += OA_T) {
    const int k = it / words, w = it - k * words;
    uint32_t m = 0;
    for (int j = 0; j < 32; ++j) {
      const int q = 32 * w + j;
      if (q < nk && q != k && bx_collide(cs[k], cs[q])) m |= 1u << j;
    }
    cc[(long long)(k0 + k) * words + w] = m;
  }
  const int g0 = gt_off[b], ng = g_live[b];
  for (int c0 = 0; c0 < ng; c0 += OA_CHUNK) {
    const int nc = min(OA_CHUNK, ng - c0);
    __syncthreads();
    for (int j = threadIdx.x; j < nc; j += OA_T) {
      const float* r = gt + (long long)(g0 + c0 + j) * dim;
      bx_corners(r[0], r[1], r[3], r[4], r[6], gs[j]);
    }
    __syncthreads();
    for (int it = threadIdx.x; it < nk * nc; it += OA_T) {
      const int k = it / nc, j = it - k * nc;
      if (bx_collide(cs[k], gs[j])) hs[k] = 1;
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < nk; k += OA_T) hit[k0 + k] = hs[k];
}

// sample_class_v2's greedy rule, one wave per scene, lane w holding bit word w: in scene order, candidate i is rejected when it
// collides with a GT box, with an accepted candidate, or with any LATER candidate of its own class (accepted or not); a rejected
// candidate's row and column are cleared, which is why only accepted ones are remembered.
__global__ void __launch_bounds__(64) k_oa_greedy(const int32_t* hit, const uint32_t* cc, const int32_t* cand_off, const int32_t* cand_grp,
                                                  int words, int32_t* acc) {
  const int b = blockIdx.x, lane = threadIdx.x, k0 = cand_off[b], nk = cand_off[b + 1] - k0;
  if (nk > OA_CAP || nk > 32 * words) {          // the host never sends this: reject everything rather than read past the matrix
    for (int i = lane; i < nk; i += 64) acc[k0 + i] = 0;
    return;
  }
  uint32_t accm = 0;
  int grp_end = 0;
  for (int i = 0; i < nk; ++i) {
    if (i >= grp_end) {            // first candidate of a class: find where its class ends (classes arrive contiguous)
      grp_end = i + 1;
      while (grp_end < nk && cand_grp[k0 + grp_end] == cand_grp[k0 + i]) ++grp_end;
    }
    uint32_t later = 0;            // bits (i, grp_end) of word `lane`
    const int lo = max(i + 1, 32 * lane), hi = min(grp_end, 32 * lane + 32);
    if (lane < words && hi > lo) {
      const int n = hi - lo;
      later = (n == 32 ? 0xffffffffu : ((1u << n) - 1u)) << (lo - 32 * lane);
    }
    const uint32_t row = lane < words ? cc[(long long)(k0 + i) * words + lane] : 0u;
    const bool bad = __any((row & (accm | later)) != 0u) || hit[k0 + i] != 0;
    if (!bad && lane == (i >> 5)) accm |= 1u << (i & 31);
    if (lane == 0) acc[k0 + i] = bad ? 0 : 1;
  }
}

// points vs boxes of their own scene, OA_CHUNK boxes at a time in LDS: first[row] = local index of the lowest (active) box that
// holds the point, -1 for none; bits (nullable) [row][words]: bit per (point, box); tile_free (nullable) [B][tiles]: points of the
// 256-point tile inside no box.  box_active (nullable) int32 per box row.
__global__ void __launch_bounds__(OA_T) k_oa_mask(const float* pts, const int32_t* scene_off, const int32_t* n_live, int feat, int tiles,
                                                  const float* boxes, const int32_t* box_off, const int32_t* box_live, const int32_t* box_active,
                                                  int dim, int words, int32_t* first, uint32_t* bits, int32_t* tile_free) {
  __shared__ float bs[OA_CHUNK][8];
  __shared__ int sh[4];
  const int b = blockIdx.y, t = blockIdx.x;
  const int i = t * OA_T + threadIdx.x;
  const bool valid = i < oa_live(n_live, scene_off, b);
  const long long row = (long long)scene_off[b] + i;
  float px = 0.f, py = 0.f, pz = 0.f;
  if (valid) { px = pts[row * feat]; py = pts[row * feat + 1]; pz = pts[row * feat + 2]; }
  const int q0 = box_off[b], nq = oa_live(box_live, box_off, b);
  int fst = -1;
  for (int c0 = 0; c0 < nq; c0 += OA_CHUNK) {
    const int nc = min(OA_CHUNK, nq - c0);
    __syncthreads();
    for (int j = threadIdx.x; j < nc; j += OA_T) {
      const float* r = boxes + (long long)(q0 + c0 + j) * dim;
      const bool on = !box_active || box_active[q0 + c0 + j];
      pb_stage(bs[j], r, on);
    }
    __syncthreads();
    if (!valid) continue;
    for (int w0 = 0; w0 < nc; w0 += 32) {
      uint32_t m = 0;
      for (int j = w0; j < min(nc, w0 + 32); ++j) {
        if (pb_inside(px, py, pz, bs[j])) m |= 1u << (j - w0);
      }
      if (m && fst < 0) fst = c0 + w0 + __builtin_ctz(m);
      if (bits) bits[row * words + ((c0 + w0) >> 5)] = m;
    }
  }
  if (valid) first[row] = fst;
  if (tile_free) {
    int tot;
    pb_scan256(valid && fst < 0 ? 1 : 0, sh, tot);
    if (threadIdx.x == 0) tile_free[b * tiles + t] = tot;
  }
}

// one workgroup: the output layout.  Per scene the sampled points of the accepted candidates (candidate order) and the kept scene
// points (scene order) follow each other, sampled first when sampled_first; then the live GT rows and the accepted candidates' boxes.
__global__ void __launch_bounds__(OA_T) k_oa_layout(int batch, int tiles, const int32_t* tile_free, const int32_t* g_live,
                                                    const int32_t* cand_off, const int32_t* cand_ids, const int32_t* db_obj_off,
                                                    const int32_t* acc, int sampled_first, int32_t* tile_base, int32_t* cand_base,
                                                    int32_t* cand_row, int32_t* out_scene_off, int32_t* out_gt_off) {
  __shared__ int sh[4];
  int pbase = 0, gbase = 0;
  for (int b = 0; b < batch; ++b) {
    const int k0 = cand_off ? cand_off[b] : 0, nk = cand_off ? cand_off[b + 1] - k0 : 0;
    int kept = 0, paste = 0, nacc = 0, tot;
    for (int c = 0; c < tiles; c += OA_T) {
      const int t = c + threadIdx.x;
      pb_scan256(t < tiles ? tile_free[b * tiles + t] : 0, sh, tot);
      kept += tot;
    }
    for (int c = 0; c < nk; c += OA_T) {
      const int k = c + threadIdx.x;
      const bool a = k < nk && acc[k0 + k];
      const int id = a ? cand_ids[k0 + k] : 0;
      pb_scan256(a ? db_obj_off[id + 1] - db_obj_off[id] : 0, sh, tot);
      paste += tot;
    }
    const int kbase = pbase + (sampled_first ? paste : 0), sbase = pbase + (sampled_first ? 0 : kept);
    int run = 0;
    for (int c = 0; c < tiles; c += OA_T) {
      const int t = c + threadIdx.x;
      const int e = pb_scan256(t < tiles ? tile_free[b * tiles + t] : 0, sh, tot);
      if (t < tiles) tile_base[b * tiles + t] = kbase + run + e;
      run += tot;
    }
    const int gl = g_live[b];
    run = 0;
    int arun = 0;
    for (int c = 0; c < nk; c += OA_T) {
      const int k = c + threadIdx.x;
      const bool a = k < nk && acc[k0 + k];
      const int id = a ? cand_ids[k0 + k] : 0;
      const int e = pb_scan256(a ? db_obj_off[id + 1] - db_obj_off[id] : 0, sh, tot);
      int atot;
      const int ae = pb_scan256(a ? 1 : 0, sh, atot);
      if (k < nk) {
        cand_base[k0 + k] = a ? sbase + run + e : -1;
        cand_row[k0 + k] = a ? gbase + gl + arun + ae : -1;
      }
      run += tot;
      arun += atot;
    }
    nacc = arun;
    if (threadIdx.x == 0) { out_scene_off[b] = pbase; out_gt_off[b] = gbase; }
    pbase += kept + paste;
    gbase += gl + nacc;
  }
  if (threadIdx.x == 0) { out_scene_off[batch] = pbase; out_gt_off[batch] = gbase; }
}

__global__ void __launch_bounds__(OA_T) k_oa_scatter_kept(const float* pts, const int32_t* scene_off, const int32_t* n_live, int feat,
                                                          int tiles, const int32_t* first, const int32_t* tile_base, float* out) {
  __shared__ int sh[4];
  const int b = blockIdx.y, t = blockIdx.x, i = t * OA_T + threadIdx.x;
  const long long row = (long long)scene_off[b] + i;
  const bool keep = i < n_live[b] && first[row] < 0;
  int tot;
  const int r = pb_scan256(keep ? 1 : 0, sh, tot);
  if (!keep) return;
  const long long o = (long long)tile_base[b * tiles + t] + r;
  for (int f = 0; f < feat; ++f) out[o * feat + f] = pts[row * feat + f];
}

// accepted candidate k = blockIdx.y: its database points, translated by the box's (x, y, z_bottom) (create_groundtruth_database stores
// them relative to it)
__global__ void __launch_bounds__(OA_T) k_oa_paste(const float* db_pts, const int32_t* db_obj_off, const float* db_boxes, int dim, int feat,
                                                   const int32_t* cand_ids, const int32_t* cand_base, float* out) {
  const int k = blockIdx.y;
  const long long o0 = cand_base[k];
  if (o0 < 0) return;
  const int id = cand_ids[k], s0 = db_obj_off[id], n = db_obj_off[id + 1] - s0;
  const int i = blockIdx.x * OA_T + threadIdx.x;
  if (i >= n) return;
  const float* src = db_pts + (long long)(s0 + i) * feat;
  float* dst = out + (o0 + i) * feat;
  const float* bx = db_boxes + (long long)id * dim;
  for (int f = 0; f < feat; ++f) dst[f] = src[f] + (f < 3 ? bx[f] : 0.f);
}

__global__ void __launch_bounds__(OA_T) k_oa_boxes_out(const float* gt, const int32_t* labels, const int32_t* gt_off, const int32_t* g_live,
                                                       int dim, const float* db_boxes, const int32_t* db_labels, const int32_t* cand_ids,
                                                       const int32_t* cand_off, const int32_t* cand_row, const int32_t* out_gt_off,
                                                       float* out_boxes, int32_t* out_labels) {
  const int b = blockIdx.x, g0 = gt_off[b], o0 = out_gt_off[b];
  for (int r = threadIdx.x; r < g_live[b]; r += OA_T) {
    for (int d = 0; d < dim; ++d) out_boxes[(long long)(o0 + r) * dim + d] = gt[(long long)(g0 + r) * dim + d];
    out_labels[o0 + r] = labels[g0 + r];
  }
  if (!cand_off) return;
  for (int k = cand_off[b] + threadIdx.x; k < cand_off[b + 1]; k += OA_T) {
    const int o = cand_row[k];
    if (o < 0) continue;
    const int id = cand_ids[k];
    for (int d = 0; d < dim; ++d) out_boxes[(long long)o * dim + d] = db_boxes[(long long)id * dim + d];
    out_labels[o] = db_labels[id];
  }
}

// try tj of a box: its corners rotated by rot[tj] about (cx, cy), then shifted by loc[tj][0:2] (_rotation_box2d_jit_, recalled)
__device__ __forceinline__ void oa_try_corners(const Q2* c0, float cx, float cy, const float* rot, const float* loc, long long tj, Q2* out) {
  const float a = rot[tj], c = cosf(a), s = sinf(a), lx = loc[tj * 3], ly = loc[tj * 3 + 1];
  Q2 cur[4];
  for (int q = 0; q < 4; ++q) {
    const float x = c0[q].x - cx, y = c0[q].y - cy;
    cur[q] = Q2{x * c - y * s + (cx + lx), x * s + y * c + (cy + ly)};
  }
  for (int q = 0; q < 4; ++q) out[q] = cur[q];
}

// noise_per_box (recalled): boxes of the scene in index order; for box i every try j (rotation rot[i][j] about its centre, then the
// BEV shift loc[i][j][0:2]) is tested against the CURRENT corners of every other box, the lowest free try wins and box i's corners
// become the moved ones.  sel[row] = (x, y, z of the original centre, loc x, y, z, rot, 0) of the chosen try; the box is updated in
// place.  Host guarantees g_live[b] <= OA_CAP.
__global__ void __launch_bounds__(OA_T) k_oa_noise_search(float* boxes, const int32_t* gt_off, const int32_t* g_live, int dim, int num_try,
                                                          const float* loc, const float* rot, int32_t* chosen, float* sel) {
  __shared__ Q2 cs[OA_CAP][4];
  __shared__ Q2 tc[OA_T][4];
  __shared__ int best;
  const int b = blockIdx.x, g0 = gt_off[b], ng = g_live[b];
  if (ng > OA_CAP) return;
  for (int i = threadIdx.x; i < ng; i += OA_T) {
    const float* r = boxes + (long long)(g0 + i) * dim;
    bx_corners(r[0], r[1], r[3], r[4], r[6], cs[i]);
  }
  __syncthreads();
  for (int i = 0; i < ng; ++i) {
    if (threadIdx.x == 0) best = num_try;
    const float* r = boxes + (long long)(g0 + i) * dim;
    const float cx = r[0], cy = r[1];
    __syncthreads();
    for (int j = threadIdx.x; j < num_try; j += OA_T) {
      Q2* cur = tc[threadIdx.x];           // in LDS: bx_collide picks its operands by pointer
      oa_try_corners(cs[i], cx, cy, rot, loc, (long long)(g0 + i) * num_try + j, cur);
      bool free = true;
      for (int o = 0; o < ng && free; ++o)
        if (o != i && bx_collide(cur, cs[o])) free = false;
      if (free) { atomicMin(&best, j); break; }
    }
    __syncthreads();
    const int j = best;
    if (j < num_try && threadIdx.x == 0) oa_try_corners(cs[i], cx, cy, rot, loc, (long long)(g0 + i) * num_try + j, cs[i]);
    if (threadIdx.x == 0) {
      float* w = boxes + (long long)(g0 + i) * dim;
      float* sl = sel + (long long)(g0 + i) * 8;
      sl[0] = w[0]; sl[1] = w[1]; sl[2] = w[2];
      if (j < num_try) {
        const long long tj = (long long)(g0 + i) * num_try + j;
        sl[3] = loc[tj * 3]; sl[4] = loc[tj * 3 + 1]; sl[5] = loc[tj * 3 + 2]; sl[6] = rot[tj];
        w[0] += sl[3]; w[1] += sl[4]; w[2] += sl[5]; w[6] += sl[6];
      } else {
        sl[3] = sl[4] = sl[5] = sl[6] = 0.f;
      }
      sl[7] = 0.f;
      chosen[g0 + i] = j < num_try ? j : -1;
    }
    __syncthreads();
  }
}

// points_transform_ (recalled): a point held by (original) box i - the lowest index among those holding it - is rotated about the
// box's original centre and shifted with it; points of a box without a free try stay where they are
__global__ void __launch_bounds__(OA_T) k_oa_point_move(float* pts, const int32_t* scene_off, const int32_t* n_live, int feat,
                                                        const int32_t* first, const int32_t* gt_off, const int32_t* chosen, const float* sel) {
  const int b = blockIdx.y, i = blockIdx.x * OA_T + threadIdx.x;
  if (i >= oa_live(n_live, scene_off, b)) return;
  const long long row = (long long)scene_off[b] + i;
  const int q = first[row];
  if (q < 0 || chosen[gt_off[b] + q] < 0) return;
  const float* s = sel + (long long)(gt_off[b] + q) * 8;
  const float c = cosf(s[6]), sn = sinf(s[6]);
  float* p = pts + row * feat;
  const float x = p[0] - s[0], y = p[1] - s[1], z = p[2] - s[2];
  p[0] = (x * c - y * sn) + s[0] + s[3];
  p[1] = (x * sn + y * c) + s[1] + s[4];
  p[2] = z + s[2] + s[5];
}

// ------------------------------------------------------------------------------------------------ C ABI (include/u3d_hip.h)

extern "C" int32_t u3d_objaug_stats(const int32_t* scene_off, const int32_t* count, const int32_t* gt_off, const int32_t* gt_count,
                                    const int32_t* labels, int32_t batch, int32_t ncls, int32_t* stats, u3d_stream s) {
  U3D_REQUIRE(scene_off && gt_off && labels && stats && batch > 0 && ncls > 0 && ncls <= 64, U3D_ERR_ARG);
  k_oa_stats<<<batch, OA_T, 0, (hipStream_t)s>>>(scene_off, count, gt_off, gt_count, labels, batch, ncls, stats);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_objaug_accept(const float* gt, const int32_t* gt_off, const int32_t* g_live, int32_t box_dim, const float* db_boxes,
                                     const int32_t* cand_ids, const int32_t* cand_off, const int32_t* cand_grp, int32_t batch, int32_t words,
                                     int32_t* hit_ws, uint32_t* cc_ws, int32_t* acc, u3d_stream s) {
  U3D_REQUIRE(gt && gt_off && g_live && db_boxes && cand_ids && cand_off && cand_grp && hit_ws && cc_ws && acc && batch > 0 &&
              (box_dim == 7 || box_dim == 9) && words >= 1 && words * 32 <= OA_CAP, U3D_ERR_ARG);
  k_oa_collide<<<batch, OA_T, 0, (hipStream_t)s>>>(gt, gt_off, g_live, box_dim, db_boxes, cand_ids, cand_off, words, hit_ws, cc_ws);
  U3D_CHECK_LAUNCH();
  k_oa_greedy<<<batch, 64, 0, (hipStream_t)s>>>(hit_ws, cc_ws, cand_off, cand_grp, words, acc);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_points_in_boxes(const float* points, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat,
                                       int32_t tiles, const float* boxes, const int32_t* box_off, const int32_t* box_live,
                                       const int32_t* box_active, int32_t box_dim, int32_t words, int32_t* first, uint32_t* bits,
                                       int32_t* tile_free, u3d_stream s) {
  U3D_REQUIRE(points && scene_off && box_off && first && batch > 0 && feat >= 3 && tiles >= 0 && (box_dim == 7 || box_dim == 9) &&
              (!bits || words >= 1), U3D_ERR_ARG);
  if (tiles == 0) return U3D_OK;
  U3D_REQUIRE(boxes || !box_live, U3D_ERR_ARG);
  k_oa_mask<<<dim3(tiles, batch), OA_T, 0, (hipStream_t)s>>>(points, scene_off, n_live, feat, tiles, boxes, box_off, box_live, box_active,
                                                             box_dim, words, first, bits, tile_free);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_objaug_paste(const float* points, const int32_t* scene_off, const int32_t* n_live, int32_t feat, const int32_t* first,
                                    const int32_t* tile_free, int32_t tiles, const float* gt, const int32_t* labels, const int32_t* gt_off,
                                    const int32_t* g_live, int32_t box_dim, const float* db_points, const int32_t* db_obj_off,
                                    const float* db_boxes, const int32_t* db_labels, const int32_t* cand_ids, const int32_t* cand_off,
                                    const int32_t* acc, int32_t n_cand, int32_t max_obj_points, int32_t batch, int32_t sampled_first,
                                    int32_t* tile_base_ws, int32_t* cand_base_ws, int32_t* cand_row_ws, float* out_points,
                                    int32_t* out_scene_off, float* out_boxes, int32_t* out_labels, int32_t* out_gt_off, u3d_stream s) {
  U3D_REQUIRE(points && scene_off && n_live && first && tile_free && gt_off && g_live && out_points && out_scene_off && out_gt_off &&
              batch > 0 && feat >= 3 && tiles >= 1 && (box_dim == 7 || box_dim == 9) && n_cand >= 0 && max_obj_points >= 0 &&
              tile_base_ws, U3D_ERR_ARG);
  U3D_REQUIRE(n_cand == 0 || (db_points && db_obj_off && db_boxes && db_labels && cand_ids && cand_off && acc && cand_base_ws &&
                              cand_row_ws), U3D_ERR_ARG);
  const hipStream_t st = (hipStream_t)s;
  const int32_t* co = n_cand ? cand_off : nullptr;
  k_oa_layout<<<1, OA_T, 0, st>>>(batch, tiles, tile_free, g_live, co, cand_ids, db_obj_off, acc, sampled_first, tile_base_ws,
                                  cand_base_ws, cand_row_ws, out_scene_off, out_gt_off);
  U3D_CHECK_LAUNCH();
  k_oa_scatter_kept<<<dim3(tiles, batch), OA_T, 0, st>>>(points, scene_off, n_live, feat, tiles, first, tile_base_ws, out_points);
  U3D_CHECK_LAUNCH();
  if (n_cand > 0 && max_obj_points > 0) {
    k_oa_paste<<<dim3(u3d_cdiv(max_obj_points, OA_T), n_cand), OA_T, 0, st>>>(db_points, db_obj_off, db_boxes, box_dim, feat, cand_ids,
                                                                              cand_base_ws, out_points);
    U3D_CHECK_LAUNCH();
  }
  if (out_boxes) {
    U3D_REQUIRE(gt && labels && out_labels, U3D_ERR_ARG);
    k_oa_boxes_out<<<batch, OA_T, 0, st>>>(gt, labels, gt_off, g_live, box_dim, db_boxes, db_labels, cand_ids, co, cand_row_ws,
                                           out_gt_off, out_boxes, out_labels);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}

extern "C" int32_t u3d_object_noise(float* points, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat, int32_t tiles,
                                    float* boxes, const int32_t* gt_off, const int32_t* g_live, int32_t box_dim, int32_t num_try,
                                    const float* loc, const float* rot, int32_t* first_ws, float* sel_ws, int32_t* chosen, u3d_stream s) {
  U3D_REQUIRE(points && scene_off && boxes && gt_off && g_live && loc && rot && first_ws && sel_ws && chosen && batch > 0 && feat >= 3 &&
              tiles >= 0 && (box_dim == 7 || box_dim == 9) && num_try >= 1, U3D_ERR_ARG);
  const hipStream_t st = (hipStream_t)s;
  if (tiles > 0) {      // the mask holds the ORIGINAL boxes: before the search moves them
    k_oa_mask<<<dim3(tiles, batch), OA_T, 0, st>>>(points, scene_off, n_live, feat, tiles, boxes, gt_off, g_live, nullptr, box_dim, 1,
                                                   first_ws, nullptr, nullptr);
    U3D_CHECK_LAUNCH();
  }
  k_oa_noise_search<<<batch, OA_T, 0, st>>>(boxes, gt_off, g_live, box_dim, num_try, loc, rot, chosen, sel_ws);
  U3D_CHECK_LAUNCH();
  if (tiles > 0) {
    k_oa_point_move<<<dim3(tiles, batch), OA_T, 0, st>>>(points, scene_off, n_live, feat, first_ws, gt_off, chosen, sel_ws);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}
