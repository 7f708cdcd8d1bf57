// KITTI 3-D detection evaluation on the device: the semantics of mmdet3d's kitti_eval (the numba port of the KITTI devkit:
// clean_data, compute_statistics, get_thresholds, eval_class), restated in uni3detr_amd/kitti_eval.py.  Parity is unpinned: no upstream
// source is vendored here, the contract is the module docstring.
//
// Records (float32, KE_REC per row): 0-6 camera box (x, y, z = bottom centre, l, h, w, ry), 7-10 2-D box (x1, y1, x2, y2), 11 alpha,
// 12 score (detections) / ignore bits of the three difficulties (GT, computed on the host in float64), 13 class code (KE_*).
//   u3d_kitti_convert     per LiDAR detection: camera box, projected and clipped 2-D box, alpha, validity (image and point-cloud range)
//   (the caller scans the validity flags and keeps the valid rows with u3d_compact_rows, csrc/compact.hip)
//   u3d_kitti_overlaps    one workgroup per scene, the scene's GT in LDS: bbox / bev / 3d overlap matrices [dt][gt], flat, scene-offset
//   u3d_kitti_flags       GT and detection flags per (class, difficulty), num_valid_gt, DontCare IoF per detection
//   u3d_kitti_pass1       one wave per (group, scene): compute_statistics(compute_fp = False); the detection argmax is a wave reduction
//   (the caller sorts each group's TP scores descending)
//   u3d_kitti_thresholds  one thread per group: get_thresholds (at most 41)
//   u3d_kitti_pass2       one wave per (group, scene), lane t = threshold t: compute_statistics(compute_fp = True), overlaps in LDS
//   u3d_kitti_reduce      per group: fixed-order sums over scenes, precision / aos, suffix max, AP11 / AP40 in float64
// No float atomics: the only atomics are integer counts, whose result does not depend on arrival order.
#include "common.h"
#include "box_iou.h"

#define KE_REC 16
#define KE_NT 41
#define KE_THREADS 256
#define KE_GT_LDS 256               // GT records staged per scene in the overlap kernel; the rest of a larger scene is read from global
#define KE_MAX_DT 4096              // detections per scene (pass 1 keeps its assigned flags in one 64-bit mask per lane)
#define KE_NO_DET -10000000.0f
#define KE_CAR 0
#define KE_PED 1
#define KE_CYC 2
#define KE_VAN 3
#define KE_PSIT 4
#define KE_DONTCARE 5

__constant__ float ke_min_height[3] = {40.f, 25.f, 25.f};

// ---------------------------------------------------------------------------------------------------------------------------
// LiDAR -> KITTI camera-frame detections.  calib [n_scene][32] = T = R0_rect @ Tr_velo_to_cam (4x4, row-major), then P2 (4x4);
// img [n_scene][2] = (H, W); lim [6] = pcd_limit_range; label_code [n_label] = class code of class_names[label].
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KE_THREADS) void k_kitti_convert(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                              const int* __restrict__ labels, const int* __restrict__ off, int n_scene, int n,
                                                              const float* __restrict__ calib, const float* __restrict__ img,
                                                              const int* __restrict__ label_code, int n_label, const float* __restrict__ lim,
                                                              float* __restrict__ rec, int* __restrict__ valid) {
  const int d = blockIdx.x * KE_THREADS + threadIdx.x;
  if (d >= n) return;
  const int s = u3d_segment_of(off, n_scene, d);
  const float* T = calib + (long long)s * 32;
  const float* P = T + 16;
  const float* b = boxes + (long long)d * 7;
  const float x = b[0], y = b[1], z = b[2];
  float c[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = T[4 * k] * x + T[4 * k + 1] * y + T[4 * k + 2] * z + T[4 * k + 3];
  const float l = b[3], w = b[4], h = b[5];
  const float ry = -b[6] - 1.5707963267948966f;
  const float cs = cosf(ry), sn = sinf(ry);
  float x1 = INFINITY, y1 = INFINITY, x2 = -INFINITY, y2 = -INFINITY;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float lx = (k & 1) ? 0.5f * l : -0.5f * l;
    const float ly = (k & 2) ? -h : 0.f;
    const float lz = (k & 4) ? 0.5f * w : -0.5f * w;
    const float X = cs * lx + sn * lz + c[0], Y = ly + c[1], Z = -sn * lx + cs * lz + c[2];
    const float u = P[0] * X + P[1] * Y + P[2] * Z + P[3];
    const float v = P[4] * X + P[5] * Y + P[6] * Z + P[7];
    const float q = P[8] * X + P[9] * Y + P[10] * Z + P[11];
    x1 = fminf(x1, u / q); x2 = fmaxf(x2, u / q);
    y1 = fminf(y1, v / q); y2 = fmaxf(y2, v / q);
  }
  const float H = img[2 * s], W = img[2 * s + 1];
  const bool in_img = x1 < W && y1 < H && x2 > 0.f && y2 > 0.f;
  const bool in_pcd = x > lim[0] && y > lim[1] && z > lim[2] && x < lim[3] && y < lim[4] && z < lim[5];
  const int lab = labels[d];
  float* r = rec + (long long)d * KE_REC;
  r[0] = c[0]; r[1] = c[1]; r[2] = c[2]; r[3] = l; r[4] = h; r[5] = w; r[6] = ry;
  r[7] = fmaxf(x1, 0.f); r[8] = fmaxf(y1, 0.f); r[9] = fminf(x2, W); r[10] = fminf(y2, H);
  r[11] = -atan2f(-y, x) + ry;
  r[12] = scores[d];
  r[13] = (float)((lab >= 0 && lab < n_label) ? label_code[lab] : -1);
  r[14] = 0.f; r[15] = 0.f;
  valid[d] = (in_img && in_pcd) ? 1 : 0;
}

extern "C" int32_t u3d_kitti_convert(const float* boxes, const float* scores, const int32_t* labels, const int32_t* off, int32_t n_scene,
                                     int32_t n, const float* calib, const float* img, const int32_t* label_code, int32_t n_label,
                                     const float* lim, float* rec, int32_t* valid, u3d_stream s) {
  U3D_REQUIRE(n >= 0 && n_scene >= 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(boxes && scores && labels && off && n_scene > 0 && calib && img && label_code && n_label > 0 && lim && rec && valid,
              U3D_ERR_ARG);
  hipLaunchKernelGGL(k_kitti_convert, dim3(u3d_cdiv(n, KE_THREADS)), dim3(KE_THREADS), 0, s, boxes, scores, labels, off, n_scene, n, calib,
                     img, label_code, n_label, lim, rec, valid);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// overlaps, one workgroup per scene: ov [3][P] with P = ov_off[n_scene]; metric m, scene s, pair (d, i) at m * P + ov_off[s] + d * ng + i.
//   bbox: 2-D IoU without +1; bev: rotated IoU of (x, z, l, w, ry); 3d: bev intersection x height overlap (camera y points down).
// The rotation R_y(ry) acts on (x, z) as x' = c x + s z, z' = -s x + c z, i.e. pp_rect's counter-clockwise turn by -ry.
// ---------------------------------------------------------------------------------------------------------------------------
__device__ static void ke_pair(const float* a, const float* b, float* out3) {
  // a: detection record (11 floats used), b: GT record
  const float iw = fminf(a[9], b[9]) - fmaxf(a[7], b[7]);
  float iou2 = 0.f;
  if (iw > 0.f) {
    const float ih = fminf(a[10], b[10]) - fmaxf(a[8], b[8]);
    if (ih > 0.f) {
      const float ua = (a[9] - a[7]) * (a[10] - a[8]) + (b[9] - b[7]) * (b[10] - b[8]) - iw * ih;
      iou2 = iw * ih / ua;
    }
  }
  // a box with a non-positive l, h or w (KITTI's DontCare rows) has no BEV / 3-D overlap
  const bool ok = a[3] > 0.f && a[4] > 0.f && a[5] > 0.f && b[3] > 0.f && b[4] > 0.f && b[5] > 0.f;
  float inter = 0.f;
  if (ok) {
    Q2 ra[4], rb[4];
    pp_rect(0.f, 0.f, a[3], a[5], -a[6], ra);
    pp_rect(b[0] - a[0], b[2] - a[2], b[3], b[5], -b[6], rb);
    inter = pp_inter_area(ra, rb);
  }
  const float den_bev = a[3] * a[5] + b[3] * b[5] - inter;
  const float dy = fminf(a[1], b[1]) - fmaxf(a[1] - a[4], b[1] - b[4]);
  const float inter3 = inter * fmaxf(dy, 0.f);
  const float den3 = a[3] * a[4] * a[5] + b[3] * b[4] * b[5] - inter3;
  out3[0] = iou2;
  out3[1] = (ok && den_bev > 0.f) ? inter / den_bev : 0.f;
  out3[2] = (ok && den3 > 0.f) ? inter3 / den3 : 0.f;
}

__global__ __launch_bounds__(KE_THREADS) void k_kitti_overlaps(const float* __restrict__ dt, const int* __restrict__ dt_off,
                                                               const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                               const long long* __restrict__ ov_off, long long P, float* __restrict__ ov) {
  __shared__ float gsh[KE_GT_LDS * 11];
  const int s = blockIdx.x;
  const int d0 = dt_off[s], nd = dt_off[s + 1] - d0, g0 = gt_off[s], ng = gt_off[s + 1] - g0;
  if (nd == 0 || ng == 0) return;
  const int nst = min(ng, KE_GT_LDS);
  for (int k = threadIdx.x; k < nst * 11; k += KE_THREADS) gsh[k] = gt[(long long)(g0 + k / 11) * KE_REC + k % 11];
  __syncthreads();
  const long long base = ov_off[s];
  for (int p = threadIdx.x; p < nd * ng; p += KE_THREADS) {
    const int d = p / ng, i = p - d * ng;
    float a[11], b[11];
#pragma unroll
    for (int c = 0; c < 11; ++c) a[c] = dt[(long long)(d0 + d) * KE_REC + c];
    if (i < KE_GT_LDS) {
#pragma unroll
      for (int c = 0; c < 11; ++c) b[c] = gsh[i * 11 + c];
    } else {
#pragma unroll
      for (int c = 0; c < 11; ++c) b[c] = gt[(long long)(g0 + i) * KE_REC + c];
    }
    float o[3];
    ke_pair(a, b, o);
    ov[base + p] = o[0];
    ov[P + base + p] = o[1];
    ov[2 * P + base + p] = o[2];
  }
}

extern "C" int32_t u3d_kitti_overlaps(const float* dt, const int32_t* dt_off, const float* gt, const int32_t* gt_off, const int64_t* ov_off,
                                      int32_t n_scene, int64_t n_pairs, float* ov, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_pairs >= 0, U3D_ERR_ARG);
  if (n_pairs == 0 || n_scene == 0) return U3D_OK;
  U3D_REQUIRE(dt && dt_off && gt && gt_off && ov_off && ov, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_kitti_overlaps, dim3(n_scene), dim3(KE_THREADS), 0, s, dt, dt_off, gt, gt_off, (const long long*)ov_off,
                     (long long)n_pairs, ov);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// clean_data.  cls [K] = class codes of current_classes; flag index f = ci * 3 + difficulty.
//   gt_flag int8 [3K][n_gt], nvalid int32 [3K] (zeroed here), dt_flag int8 [3K][n_dt], dc_iof f32 [n_dt] = max over the scene's
//   DontCare boxes of intersection / detection area (0 without one).
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(KE_THREADS) void k_kitti_gt_flags(const float* __restrict__ gt, int n_gt, const int* __restrict__ cls, int K,
                                                               signed char* __restrict__ gt_flag, int* __restrict__ nvalid) {
  const int i = blockIdx.x * KE_THREADS + threadIdx.x;
  const bool live = i < n_gt;
  const int code = live ? (int)gt[(long long)i * KE_REC + 13] : -1;
  const int ign = live ? (int)gt[(long long)i * KE_REC + 12] : 0;
  for (int ci = 0; ci < K; ++ci) {
    const int cc = cls[ci];
    const int vc = code == cc ? 1 : ((cc == KE_PED && code == KE_PSIT) || (cc == KE_CAR && code == KE_VAN)) ? 0 : -1;
    for (int df = 0; df < 3; ++df) {
      const bool ignore = (ign >> df) & 1;
      const int f = (vc == 1 && !ignore) ? 0 : (vc == 0 || (ignore && vc == 1)) ? 1 : -1;
      if (live) gt_flag[(long long)(ci * 3 + df) * n_gt + i] = (signed char)f;
      const unsigned long long m = __ballot(live && f == 0);
      if ((threadIdx.x & 63) == 0 && m) atomicAdd(nvalid + ci * 3 + df, __popcll(m));
    }
  }
}

__global__ __launch_bounds__(KE_THREADS) void k_kitti_dt_flags(const float* __restrict__ dt, const int* __restrict__ dt_off, int n_scene,
                                                               int n_dt, const float* __restrict__ gt, const int* __restrict__ gt_off,
                                                               const int* __restrict__ cls, int K, signed char* __restrict__ dt_flag,
                                                               float* __restrict__ dc_iof) {
  const int j = blockIdx.x * KE_THREADS + threadIdx.x;
  if (j >= n_dt) return;
  const float* a = dt + (long long)j * KE_REC;
  const int code = (int)a[13];
  const double height = fabs((double)a[10] - (double)a[8]);
  for (int ci = 0; ci < K; ++ci)
    for (int df = 0; df < 3; ++df)
      dt_flag[(long long)(ci * 3 + df) * n_dt + j] = (signed char)(height < (double)ke_min_height[df] ? 1 : code == cls[ci] ? 0 : -1);
  const int s = u3d_segment_of(dt_off, n_scene, j);
  const float area = (a[9] - a[7]) * (a[10] - a[8]);
  float best = 0.f;
  for (int i = gt_off[s]; i < gt_off[s + 1]; ++i) {
    const float* b = gt + (long long)i * KE_REC;
    if ((int)b[13] != KE_DONTCARE) continue;
    const float iw = fminf(a[9], b[9]) - fmaxf(a[7], b[7]);
    if (!(iw > 0.f)) continue;
    const float ih = fminf(a[10], b[10]) - fmaxf(a[8], b[8]);
    if (!(ih > 0.f)) continue;
    best = fmaxf(best, iw * ih / area);
  }
  dc_iof[j] = best;
}

extern "C" int32_t u3d_kitti_flags(const float* dt, const int32_t* dt_off, int32_t n_scene, int32_t n_dt, const float* gt,
                                   const int32_t* gt_off, int32_t n_gt, const int32_t* cls, int32_t K, int8_t* gt_flag, int32_t* nvalid,
                                   int8_t* dt_flag, float* dc_iof, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_dt >= 0 && n_gt >= 0 && K > 0 && K <= 3 && cls && nvalid, U3D_ERR_ARG);
  if (hipMemsetAsync(nvalid, 0, sizeof(int32_t) * 3 * K, s) != hipSuccess) return U3D_ERR_LAUNCH;
  if (n_gt > 0) {
    U3D_REQUIRE(gt && gt_flag, U3D_ERR_ARG);
    hipLaunchKernelGGL(k_kitti_gt_flags, dim3(u3d_cdiv(n_gt, KE_THREADS)), dim3(KE_THREADS), 0, s, gt, n_gt, cls, K, (signed char*)gt_flag,
                       nvalid);
    U3D_CHECK_LAUNCH();
  }
  if (n_dt > 0) {
    U3D_REQUIRE(dt && dt_off && gt_off && n_scene > 0 && dt_flag && dc_iof && (gt || n_gt == 0), U3D_ERR_ARG);
    hipLaunchKernelGGL(k_kitti_dt_flags, dim3(u3d_cdiv(n_dt, KE_THREADS)), dim3(KE_THREADS), 0, s, dt, dt_off, n_scene, n_dt, gt, gt_off,
                       cls, K, (signed char*)dt_flag, dc_iof);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// groups: g -> (flag index gfid[g], metric gmet[g] in {0 bbox, 1 bev, 2 3d}, min overlap gmin[g]).  Block b = g * n_scene + s.
// pass 1: the GT loop runs in index order; per GT the eligible detection with the highest score (lowest index on ties) is found by a
// wave reduction; a TP writes its score to tp_sc[g][gt_off[s] + k] (k-th TP of the scene); the scene's other slots get -inf.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_kitti_pass1(const float* __restrict__ dt, const int* __restrict__ dt_off, int n_dt,
                                                    const int* __restrict__ gt_off, int n_gt, int n_scene, const long long* __restrict__ ov_off,
                                                    long long P, const float* __restrict__ ov, const signed char* __restrict__ gt_flag,
                                                    const signed char* __restrict__ dt_flag, const int* __restrict__ gfid,
                                                    const int* __restrict__ gmet, const float* __restrict__ gmin, float* __restrict__ tp_sc) {
  const int g = blockIdx.x / n_scene, s = blockIdx.x - g * n_scene;
  const int lane = threadIdx.x;
  const int d0 = dt_off[s], nd = dt_off[s + 1] - d0, g0 = gt_off[s], ng = gt_off[s + 1] - g0;
  const float mino = gmin[g];
  const float* o = ov + (long long)gmet[g] * P + ov_off[s];
  const signed char* gf = gt_flag + (long long)gfid[g] * n_gt + g0;
  const signed char* df = dt_flag + (long long)gfid[g] * n_dt + d0;
  float* out = tp_sc + (long long)g * n_gt + g0;
  unsigned long long asg = 0ull;            // bit k: detection lane + 64 k is assigned
  int ntp = 0;
  for (int i = 0; i < ng; ++i) {
    const int gfi = gf[i];
    if (gfi == -1) continue;
    float best = KE_NO_DET;
    int bj = -1;
    for (int j = lane, k = 0; j < nd; j += 64, ++k) {
      if ((asg >> k) & 1ull) continue;
      if (df[j] == -1) continue;
      const float sc = dt[(long long)(d0 + j) * KE_REC + 12];
      if (o[(long long)j * ng + i] > mino && sc > best) { best = sc; bj = j; }
    }
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      const float ob = __shfl_xor(best, m, 64);
      const int oj = __shfl_xor(bj, m, 64);
      if (oj >= 0 && (bj < 0 || ob > best || (ob == best && oj < bj))) { best = ob; bj = oj; }
    }
    if (bj < 0) continue;
    if (!(gfi == 1 || df[bj] == 1)) {
      if (lane == 0) out[ntp] = best;
      ++ntp;
    }
    if ((bj & 63) == lane) asg |= 1ull << (bj >> 6);
  }
  for (int k = ntp + lane; k < ng; k += 64) out[k] = -INFINITY;
}

extern "C" int32_t u3d_kitti_pass1(const float* dt, const int32_t* dt_off, int32_t n_dt, const int32_t* gt_off, int32_t n_gt, int32_t n_scene,
                                   const int64_t* ov_off, int64_t n_pairs, const float* ov, const int8_t* gt_flag, const int8_t* dt_flag,
                                   const int32_t* gfid, const int32_t* gmet, const float* gmin, int32_t n_group, int32_t max_dt,
                                   float* tp_sc, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_group >= 0 && n_dt >= 0 && n_gt >= 0 && max_dt >= 0, U3D_ERR_ARG);
  U3D_REQUIRE(max_dt <= KE_MAX_DT, U3D_ERR_UNSUPPORTED);
  if (n_scene == 0 || n_group == 0 || n_gt == 0) return U3D_OK;
  U3D_REQUIRE(dt_off && gt_off && ov_off && gt_flag && gfid && gmet && gmin && tp_sc, U3D_ERR_ARG);
  U3D_REQUIRE(n_dt == 0 || (dt && ov && dt_flag), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_kitti_pass1, dim3(n_group * n_scene), dim3(64), 0, s, dt, dt_off, n_dt, gt_off, n_gt, n_scene,
                     (const long long*)ov_off, (long long)n_pairs, ov, (const signed char*)gt_flag, (const signed char*)dt_flag, gfid, gmet,
                     gmin, tp_sc);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// get_thresholds over each group's TP scores sorted descending (-inf padding after the last one): thr [n_group][41], nthr [n_group]
__global__ __launch_bounds__(64) void k_kitti_thresholds(const float* __restrict__ sorted, int n_gt, int n_group, const int* __restrict__ gfid,
                                                         const int* __restrict__ nvalid, float* __restrict__ thr, int* __restrict__ nthr) {
  const int g = blockIdx.x * 64 + threadIdx.x;
  if (g >= n_group) return;
  const float* sc = sorted + (long long)g * n_gt;
  const int nv = nvalid[gfid[g]];
  int nt = 0;
  if (nv > 0) {
    double cur = 0.0;
    const double dn = (double)nv;
    for (int i = 0; i < n_gt; ++i) {
      const float v = sc[i];
      if (v == -INFINITY) break;
      const bool last = i + 1 >= n_gt || sc[i + 1] == -INFINITY;
      const double lr = (double)(i + 1) / dn;
      const double rr = last ? lr : (double)(i + 2) / dn;
      if ((rr - cur) < (cur - lr) && !last) continue;
      if (nt < KE_NT) thr[(long long)g * KE_NT + nt] = v;
      ++nt;
      cur += 1.0 / 40.0;
    }
  }
  nthr[g] = min(nt, KE_NT);
}

extern "C" int32_t u3d_kitti_thresholds(const float* sorted, int32_t n_gt, int32_t n_group, const int32_t* gfid, const int32_t* nvalid,
                                        float* thr, int32_t* nthr, u3d_stream s) {
  U3D_REQUIRE(n_gt >= 0 && n_group >= 0, U3D_ERR_ARG);
  if (n_group == 0) return U3D_OK;
  U3D_REQUIRE(gfid && nvalid && thr && nthr && (sorted || n_gt == 0), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_kitti_thresholds, dim3(u3d_cdiv(n_group, 64)), dim3(64), 0, s, sorted, n_gt, n_group, gfid, nvalid, thr, nthr);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// pass 2: lane t runs compute_statistics(compute_fp = True, thresh = thr[g][t]) over the scene.  LDS (dynamic, sized by the host
// with u3d_kitti_pass2_lds for the largest scene): per-lane assigned bits [ceil(nd/32)][64] u32 | overlaps [nd][ng] f32 |
// scores [nd] f32 | detection flags [nd] i8 | DontCare hits [nd] i8 | GT flags [ng] i8.  The overlap, flag and score reads are
// wave-uniform (broadcast); only the assigned bits and the threshold test differ between lanes.
// st_tp / st_fp / st_fn int32 and st_sim f64: [n_group][n_scene][41] (slots t >= nthr[g] are not written).
// ---------------------------------------------------------------------------------------------------------------------------
__host__ __device__ static inline long long ke_pass2_lds(long long nd, long long ng) {
  const long long words = (nd + 31) / 32;
  return words * 64 * 4 + nd * ng * 4 + nd * 4 + nd * 2 + ng;
}

extern "C" int64_t u3d_kitti_pass2_lds(int32_t nd, int32_t ng) { return ke_pass2_lds(nd, ng); }

__global__ __launch_bounds__(64) void k_kitti_pass2(const float* __restrict__ dt, const int* __restrict__ dt_off, int n_dt,
                                                    const float* __restrict__ gt, const int* __restrict__ gt_off, int n_gt, int n_scene,
                                                    const long long* __restrict__ ov_off, long long P, const float* __restrict__ ov,
                                                    const signed char* __restrict__ gt_flag, const signed char* __restrict__ dt_flag,
                                                    const float* __restrict__ dc_iof, const int* __restrict__ gfid,
                                                    const int* __restrict__ gmet, const float* __restrict__ gmin, const float* __restrict__ thr,
                                                    const int* __restrict__ nthr, int aos, int* __restrict__ st_tp, int* __restrict__ st_fp,
                                                    int* __restrict__ st_fn, double* __restrict__ st_sim) {
  extern __shared__ unsigned int ke_lds[];
  const int g = blockIdx.x / n_scene, s = blockIdx.x - g * n_scene;
  const int lane = threadIdx.x;
  const int nt = nthr[g];
  if (nt == 0) return;
  const int d0 = dt_off[s], nd = dt_off[s + 1] - d0, g0 = gt_off[s], ng = gt_off[s + 1] - g0;
  const int met = gmet[g];
  const float mino = gmin[g];
  const bool bbox = met == 0, do_aos = aos && bbox;
  const int words = (nd + 31) >> 5;
  unsigned int* bits = ke_lds;
  float* ovs = (float*)(bits + words * 64);
  float* scs = ovs + nd * ng;
  signed char* dfs = (signed char*)(scs + nd);
  signed char* dcs = dfs + nd;
  signed char* gfs = dcs + nd;
  const float* o = ov + (long long)met * P + ov_off[s];
  const signed char* gf = gt_flag + (long long)gfid[g] * n_gt + g0;
  const signed char* df = dt_flag + (long long)gfid[g] * n_dt + d0;
  for (int k = lane; k < words * 64; k += 64) bits[k] = 0u;
  for (int k = lane; k < nd * ng; k += 64) ovs[k] = o[k];
  for (int k = lane; k < nd; k += 64) {
    scs[k] = dt[(long long)(d0 + k) * KE_REC + 12];
    dfs[k] = df[k];
    dcs[k] = (bbox && dc_iof[d0 + k] > mino) ? 1 : 0;
  }
  for (int k = lane; k < ng; k += 64) gfs[k] = gf[k];
  __syncthreads();
  const float th = lane < nt ? thr[(long long)g * KE_NT + lane] : INFINITY;
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  for (int i = 0; i < ng; ++i) {
    const int gfi = gfs[i];
    if (gfi == -1) continue;
    int det = -1;
    float maxov = 0.f;
    bool aig = false;
    for (int j = 0; j < nd; ++j) {
      const float ovl = ovs[j * ng + i];
      if (!(ovl > mino)) continue;
      const int f = dfs[j];
      if (f == -1) continue;
      if ((bits[(j >> 5) * 64 + lane] >> (j & 31)) & 1u) continue;
      if (scs[j] < th) continue;
      if (f == 0 && (ovl > maxov || aig)) { maxov = ovl; det = j; aig = false; }
      else if (f == 1 && det < 0) { det = j; aig = true; }
    }
    if (det < 0) {
      if (gfi == 0) ++fn;
    } else {
      if (!(gfi == 1 || dfs[det] == 1)) {
        ++tp;
        if (do_aos) {
          const double delta = (double)gt[(long long)(g0 + i) * KE_REC + 11] - (double)dt[(long long)(d0 + det) * KE_REC + 11];
          sim += (1.0 + cos(delta)) / 2.0;
        }
      }
      bits[(det >> 5) * 64 + lane] |= 1u << (det & 31);
    }
  }
  int nstuff = 0;
  for (int j = 0; j < nd; ++j) {
    if (dfs[j] != 0 || scs[j] < th || ((bits[(j >> 5) * 64 + lane] >> (j & 31)) & 1u)) continue;
    ++fp;
    if (dcs[j]) ++nstuff;
  }
  fp -= nstuff;
  if (lane < nt) {
    const long long k = ((long long)g * n_scene + s) * KE_NT + lane;
    st_tp[k] = tp;
    st_fp[k] = fp;
    st_fn[k] = fn;
    st_sim[k] = do_aos ? ((tp > 0 || fp > 0) ? sim : -1.0) : 0.0;
  }
}

extern "C" int32_t u3d_kitti_pass2(const float* dt, const int32_t* dt_off, int32_t n_dt, const float* gt, const int32_t* gt_off, int32_t n_gt,
                                   int32_t n_scene, const int64_t* ov_off, int64_t n_pairs, const float* ov, const int8_t* gt_flag,
                                   const int8_t* dt_flag, const float* dc_iof, const int32_t* gfid, const int32_t* gmet, const float* gmin,
                                   const float* thr, const int32_t* nthr, int32_t n_group, int32_t aos, int64_t lds_bytes, int32_t* st_tp,
                                   int32_t* st_fp, int32_t* st_fn, double* st_sim, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_group >= 0 && n_dt >= 0 && n_gt >= 0 && lds_bytes >= 0, U3D_ERR_ARG);
  U3D_REQUIRE(lds_bytes <= 160 * 1024, U3D_ERR_UNSUPPORTED);
  if (n_scene == 0 || n_group == 0) return U3D_OK;
  U3D_REQUIRE(dt_off && gt_off && ov_off && gfid && gmet && gmin && thr && nthr && st_tp && st_fp && st_fn && st_sim, U3D_ERR_ARG);
  U3D_REQUIRE(n_gt == 0 || (gt && gt_flag), U3D_ERR_ARG);
  U3D_REQUIRE(n_dt == 0 || (dt && dt_flag && dc_iof), U3D_ERR_ARG);
  U3D_REQUIRE(n_pairs == 0 || ov, U3D_ERR_ARG);
  const int bytes = (int)((lds_bytes + 15) / 16 * 16);
  if (bytes > 64 * 1024) U3D_ALLOW_LDS(k_kitti_pass2, bytes);
  hipLaunchKernelGGL(k_kitti_pass2, dim3(n_group * n_scene), dim3(64), bytes, s, dt, dt_off, n_dt, gt, gt_off, n_gt, n_scene,
                     (const long long*)ov_off, (long long)n_pairs, ov, (const signed char*)gt_flag, (const signed char*)dt_flag, dc_iof, gfid,
                     gmet, gmin, thr, nthr, aos, st_tp, st_fp, st_fn, st_sim);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// reduction, one workgroup per group: thread (part p, lane t) sums scenes [p S / 4, (p+1) S / 4) in order, the 4 partial sums are
// added in part order.  Then precision = tp / (tp + fp), aos = sim / (tp + fp) (float64, NaN-propagating suffix max as np.max),
// AP11 = sum prec[0:41:4] / 11 * 100, AP40 = sum prec[1:41] / 40 * 100.
// tot int32 [n_group][3][41] (tp, fp, fn; zero past nthr), sim f64 [n_group][41], ap f64 [n_group][4] = (AP11, AP40, AOS11, AOS40).
// ---------------------------------------------------------------------------------------------------------------------------
#define KE_PARTS 4
__device__ static inline double ke_max_nan(double a, double b) { return (a != a || b != b) ? __longlong_as_double(0x7ff8000000000000ll) : fmax(a, b); }

__global__ __launch_bounds__(KE_PARTS * 64) void k_kitti_reduce(const int* __restrict__ st_tp, const int* __restrict__ st_fp,
                                                                const int* __restrict__ st_fn, const double* __restrict__ st_sim,
                                                                int n_scene, const int* __restrict__ nthr, int* __restrict__ tot,
                                                                double* __restrict__ sim_tot, double* __restrict__ ap) {
  __shared__ int ptp[KE_PARTS][64], pfp[KE_PARTS][64], pfn[KE_PARTS][64];
  __shared__ double psim[KE_PARTS][64];
  __shared__ double prec[KE_NT], aosv[KE_NT];
  const int g = blockIdx.x;
  const int t = threadIdx.x & 63, p = threadIdx.x >> 6;
  const int nt = nthr[g];
  const int s0 = (int)((long long)n_scene * p / KE_PARTS), s1 = (int)((long long)n_scene * (p + 1) / KE_PARTS);
  int tp = 0, fp = 0, fn = 0;
  double sim = 0.0;
  if (t < nt) {
    for (int s = s0; s < s1; ++s) {
      const long long k = ((long long)g * n_scene + s) * KE_NT + t;
      tp += st_tp[k];
      fp += st_fp[k];
      fn += st_fn[k];
      const double v = st_sim[k];
      if (v != -1.0) sim += v;
    }
  }
  ptp[p][t] = tp; pfp[p][t] = fp; pfn[p][t] = fn; psim[p][t] = sim;
  __syncthreads();
  if (threadIdx.x < KE_NT) {
    int a = 0, b = 0, c = 0;
    double m = 0.0;
    for (int q = 0; q < KE_PARTS; ++q) { a += ptp[q][t]; b += pfp[q][t]; c += pfn[q][t]; m += psim[q][t]; }
    tot[((long long)g * 3 + 0) * KE_NT + t] = a;
    tot[((long long)g * 3 + 1) * KE_NT + t] = b;
    tot[((long long)g * 3 + 2) * KE_NT + t] = c;
    sim_tot[(long long)g * KE_NT + t] = m;
    prec[t] = t < nt ? (double)a / (double)(a + b) : 0.0;
    aosv[t] = t < nt ? m / (double)(a + b) : 0.0;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double mp = prec[KE_NT - 1], ma = aosv[KE_NT - 1];
#pragma unroll 1
    for (int i = KE_NT - 1; i >= 0; --i) {
      mp = ke_max_nan(mp, prec[i]);
      ma = ke_max_nan(ma, aosv[i]);
      if (i < nt) { prec[i] = mp; aosv[i] = ma; }
    }
    double s11 = 0.0, s40 = 0.0, a11 = 0.0, a40 = 0.0;
#pragma unroll 1
    for (int i = 0; i < KE_NT; i += 4) { s11 += prec[i]; a11 += aosv[i]; }
#pragma unroll 1
    for (int i = 1; i < KE_NT; ++i) { s40 += prec[i]; a40 += aosv[i]; }
    ap[g * 4 + 0] = s11 / 11.0 * 100.0;
    ap[g * 4 + 1] = s40 / 40.0 * 100.0;
    ap[g * 4 + 2] = a11 / 11.0 * 100.0;
    ap[g * 4 + 3] = a40 / 40.0 * 100.0;
  }
}

extern "C" int32_t u3d_kitti_reduce(const int32_t* st_tp, const int32_t* st_fp, const int32_t* st_fn, const double* st_sim, int32_t n_scene,
                                    const int32_t* nthr, int32_t n_group, int32_t* tot, double* sim_tot, double* ap, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_group >= 0, U3D_ERR_ARG);
  if (n_group == 0) return U3D_OK;
  U3D_REQUIRE(nthr && tot && sim_tot && ap && (n_scene == 0 || (st_tp && st_fp && st_fn && st_sim)), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_kitti_reduce, dim3(n_group), dim3(KE_PARTS * 64), 0, s, st_tp, st_fp, st_fn, st_sim, n_scene, nthr, tot, sim_tot, ap);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
