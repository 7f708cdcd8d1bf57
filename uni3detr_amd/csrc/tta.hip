// Test-time augmentation: the multi-view box merge (ref: projects/mmdet3d_plugin/core/merge_all_augs.py:9-98 with
// core/bbox/util.py:82-102 bbox3d_mapping_back), for all scenes of a batch in one call.  The reference merges one sample with a host
// loop (one .item() sync for the class count, one nms_bev call per class); here:
//   k_tta_inverse / k_tta_prep  per view its inverse (fh, fv, -angle, 1/scale, no translation), per candidate that table applied with
//                 dp_box_augment - the arithmetic of u3d_boxes_augment on the same parameters, bit for bit - and the BEV row (cx, cy, w, h, yaw) after the f32 round trip of
//                 xywhr2xyxyr + mmcv nms_bev;
//   k_tta_rank    per candidate: its position in the scene's (label asc, score desc, index asc) order among the valid candidates
//                 (finite score, label in [0, num_classes)): a stable counting sort, no host sort; per (scene, class) segment start / size;
//   k_tta_nms_lds one workgroup per (scene, class) segment of at most TTA_LDS_CAP candidates: greedy rotated-BEV NMS with the segment's
//                 BEV rows in LDS (a candidate is suppressed iff a kept, higher-ranked one has IoU > thr);
//   k_tta_mask / k_tta_sweep  the same for larger segments through global memory: 64-bit suppression words per (row, word) as in
//                 k_nms_mask / k_nms_sweep (query.hip), segmented, one sweeping wave per segment;
//   k_tta_select  per kept candidate: its rank in the class-major kept list stably sorted by descending score; the first max_num of
//                 every scene are written out, count[s] = min(kept, max_num).
// Layout: boxes [n, box_dim] f32 bottom-centre, box_dim 7 or 9, scores [n] f32, labels [n] int32; det_off int32 [batch*views + 1]:
// view v = rows det_off[v] .. det_off[v+1]), scene s = views s*views .. s*views + views - 1 (scene-major, view-minor); params f32
// [batch*views][U3D_AUG_NPARAM], the FORWARD parameters of every view (rotation / scale, then flip: the inner test pipeline's order).
// u3d_tta_merge_padded runs the same kernels on the padded layout of the batched detection tail (boxes [batch*views][K][box_dim], a
// device count per view): candidate i of the concatenated order lives at memory row v*K + (i - det_off[v]), det_off being the scan of
// the clamped counts that k_tta_scan leaves in the workspace.  Only k_tta_prep touches the caller's rows - it is the one kernel
// templated on the layout, and for the padded one it also leaves the candidate's score and label at index i - so everything behind
// it is literally the ragged entry's code on the ragged entry's indices.  Every grid is sized by batch*views*K; threads past
// det_off[batch*views] leave at once.  k_tta_zero_tail / k_tta_scan finish the DetBatch (zero rows past the count, out_off).
#include "common.h"
#include "box_aug.h"
#include "box_iou.h"

#define TTA_NP U3D_AUG_NPARAM
#define TTA_LDS_CAP U3D_TTA_LDS_CAP
#define TTA_LDS_THREADS 256

__device__ __forceinline__ bool tta_valid(float score, int label, int ncls) {
  return isfinite(score) && label >= 0 && label < ncls;
}

// the inverse of every view, "rotate by angle, scale by s, then flip": flip, rotate by -angle, scale by 1/s (rotation and scale
// commute), as a parameter table in memory - the map-back then runs dp_box_augment on exactly what u3d_boxes_augment would read
__global__ void k_tta_inverse(const float* __restrict__ params, int nviews, float* __restrict__ inv) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= nviews) return;
  const float* p = params + (long long)v * TTA_NP;
  float* q = inv + (long long)v * TTA_NP;
  q[0] = p[0]; q[1] = p[1]; q[2] = -p[2]; q[3] = p[3]; q[4] = -p[4]; q[5] = 1.f / p[5]; q[6] = 0.f; q[7] = 0.f; q[8] = 0.f;
}

template <bool PADDED>
__global__ void k_tta_prep(const float* __restrict__ boxes, const float* __restrict__ scores, const int* __restrict__ labels,
                           const int* __restrict__ det_off, const float* __restrict__ inv, int nviews, int n, int dim, int coord, int K,
                           float* __restrict__ mapped, float* __restrict__ bev, float* __restrict__ cscores, int* __restrict__ clabels) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n || i >= det_off[nviews]) return;
  const int v = u3d_segment_of(det_off, nviews, i);
  // the candidate's memory row: the concatenated index itself, or its place in view v's block of K rows (rows at or past the view's
  // count are never addressed: i - det_off[v] < det_off[v + 1] - det_off[v])
  const long long row = PADDED ? (long long)v * K + (i - det_off[v]) : (long long)i;
  if (PADDED) {
    cscores[i] = scores[row];
    clabels[i] = labels[row];
  }
  float* o = mapped + (long long)i * dim;
  for (int k = 0; k < dim; ++k) o[k] = boxes[row * dim + k];
  dp_box_augment(o, o, dim, inv + (long long)v * TTA_NP, coord);      // in place, as k_boxes_augment
  // mmdet3d xywhr2xyxyr on .bev = (x, y, dx, dy, yaw), then nms_bev's way back to (cx, cy, w, h, yaw), in f32
  const float hw = o[3] / 2.f, hh = o[4] / 2.f;
  const float x1 = o[0] - hw, y1 = o[1] - hh, x2 = o[0] + hw, y2 = o[1] + hh;
  float* b = bev + (long long)i * 5;
  b[0] = (x1 + x2) / 2.f; b[1] = (y1 + y2) / 2.f; b[2] = x2 - x1; b[3] = y2 - y1; b[4] = o[6];
}

// seg [batch][ncls][2] = (first sorted position relative to the scene's base, size); nvalid [batch]; ord [n]: scene s's valid candidates
// at ord[base_s + 0 .. nvalid[s]) in (label, score desc, index) order.  seg / nvalid are zeroed by the host before the launch; every
// candidate of a scene writes the same values.
__global__ void k_tta_rank(const float* __restrict__ scores, const int* __restrict__ labels, const int* __restrict__ det_off, int batch,
                           int nviews_per_scene, int n, int ncls, int* __restrict__ ord, int* __restrict__ seg, int* __restrict__ nvalid) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int V = nviews_per_scene;
  if (i >= n || i >= det_off[batch * V]) return;
  const int s = u3d_segment_of(det_off, batch, i, V);
  const int base = det_off[s * V], end = det_off[(s + 1) * V];
  const float sc = scores[i];
  const int lab = labels[i];
  const bool ok = tta_valid(sc, lab, ncls);
  int cnt = 0, before = 0, same = 0, rank = 0;
  for (int j = base; j < end; ++j) {
    const float sj = scores[j];
    const int lj = labels[j];
    if (!tta_valid(sj, lj, ncls)) continue;
    ++cnt;
    if (!ok) continue;
    if (lj < lab) ++before;
    else if (lj == lab) {
      ++same;
      if (sj > sc || (sj == sc && j < i)) ++rank;
    }
  }
  nvalid[s] = cnt;
  if (!ok) return;
  ord[base + before + rank] = i;
  seg[((long long)s * ncls + lab) * 2 + 0] = before;
  seg[((long long)s * ncls + lab) * 2 + 1] = same;
}

__global__ __launch_bounds__(TTA_LDS_THREADS) void k_tta_nms_lds(const float* __restrict__ bev, const int* __restrict__ det_off,
                                                                int nviews_per_scene, const int* __restrict__ ord,
                                                                const int* __restrict__ seg, int ncls, float thr,
                                                                unsigned char* __restrict__ keep) {
  __shared__ float sb[TTA_LDS_CAP * 5];
  __shared__ unsigned char removed[TTA_LDS_CAP];
  const int c = blockIdx.x, s = blockIdx.y, t = threadIdx.x;
  const int start = seg[((long long)s * ncls + c) * 2], cnt = seg[((long long)s * ncls + c) * 2 + 1];
  if (cnt == 0 || cnt > TTA_LDS_CAP) return;                  // empty class: skipped; large segment: the global path
  const int base = det_off[s * nviews_per_scene] + start;
  for (int r = t; r < cnt; r += TTA_LDS_THREADS) {
    const float* b = bev + (long long)ord[base + r] * 5;
    for (int k = 0; k < 5; ++k) sb[r * 5 + k] = b[k];
    removed[r] = 0;
  }
  for (int i = 0; i < cnt; ++i) {
    __syncthreads();                                           // removed[i] is final: only rows < i write it
    if (removed[i]) continue;
    const float* bi = sb + i * 5;
    for (int j = i + 1 + t; j < cnt; j += TTA_LDS_THREADS)
      if (!removed[j] && pp_iou_bev(bi, sb + j * 5) > thr) removed[j] = 1;
  }
  __syncthreads();
  for (int r = t; r < cnt; r += TTA_LDS_THREADS) keep[base + r] = removed[r] ? 0 : 1;
}

// mask [batch][max_rows][nw]: bit j of word w of row r set iff j > r in the same segment and iou(r, j) > thr (rows / j are sorted
// positions relative to the scene's base).  Only rows of segments larger than TTA_LDS_CAP are computed; only words the segment covers
// are written (and read by the sweep).
__global__ void k_tta_mask(const float* __restrict__ bev, const int* __restrict__ labels, const int* __restrict__ det_off,
                           int nviews_per_scene, const int* __restrict__ ord, const int* __restrict__ seg, const int* __restrict__ nvalid,
                           int ncls, float thr, int max_rows, int nw, unsigned long long* __restrict__ mask) {
  const int r = blockIdx.x, w = blockIdx.y, s = blockIdx.z, lane = threadIdx.x;
  if (r >= nvalid[s] || r >= max_rows) return;
  const int base = det_off[s * nviews_per_scene];
  const int ir = ord[base + r];
  const long long sg = ((long long)s * ncls + labels[ir]) * 2;
  const int start = seg[sg], cnt = seg[sg + 1];
  const int end = min(start + cnt, max_rows);
  if (cnt <= TTA_LDS_CAP || w < (start >> 6) || w > ((end - 1) >> 6)) return;
  const int j = w * 64 + lane;
  bool sup = false;
  if (j > r && j < end) sup = pp_iou_bev(bev + (long long)ir * 5, bev + (long long)ord[base + j] * 5) > thr;
  const unsigned long long bits = __ballot(sup);
  if (lane == 0) mask[((long long)s * max_rows + r) * nw + w] = bits;
}

// one wave per large segment (64 threads in lock step: every lane reads removed[i] before any lane ORs a row into it)
__global__ __launch_bounds__(64) void k_tta_sweep(const unsigned long long* __restrict__ mask, const int* __restrict__ det_off,
                                                 int nviews_per_scene, const int* __restrict__ seg, int ncls, int max_rows, int nw,
                                                 unsigned char* __restrict__ keep) {
  extern __shared__ unsigned long long removed_w[];
  const int c = blockIdx.x, s = blockIdx.y, lane = threadIdx.x;
  const int start = seg[((long long)s * ncls + c) * 2], cnt = seg[((long long)s * ncls + c) * 2 + 1];
  if (cnt <= TTA_LDS_CAP) return;
  const int end = min(start + cnt, max_rows);
  const int w0 = start >> 6, w1 = (end - 1) >> 6;
  for (int w = w0 + lane; w <= w1; w += 64) removed_w[w] = 0ull;
  __syncthreads();
  const int base = det_off[s * nviews_per_scene];
  for (int i = start; i < end; ++i) {
    const bool k = !((removed_w[i >> 6] >> (i & 63)) & 1ull);
    if (lane == 0) keep[base + i] = k ? 1 : 0;
    if (k) {
      const unsigned long long* row = mask + ((long long)s * max_rows + i) * nw;
      for (int w = (i >> 6) + lane; w <= w1; w += 64) removed_w[w] |= row[w];
    }
    __syncthreads();
  }
}

// per sorted position g of a kept candidate: rank among the scene's kept ones by (score desc, sorted position asc) - the class-major
// list stably sorted by descending score - and the first max_num written out
__global__ void k_tta_select(const float* __restrict__ mapped, const float* __restrict__ scores, const int* __restrict__ labels,
                             const int* __restrict__ det_off, int batch, int nviews_per_scene, int n, int dim,
                             const int* __restrict__ ord, const int* __restrict__ nvalid, const unsigned char* __restrict__ keep,
                             int max_num, float* __restrict__ out_boxes, float* __restrict__ out_scores, int* __restrict__ out_labels,
                             int* __restrict__ out_count) {
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  const int V = nviews_per_scene;
  if (g >= n || g >= det_off[batch * V]) return;
  const int s = u3d_segment_of(det_off, batch, g, V);
  const int base = det_off[s * V], r = g - base, nv = nvalid[s];
  if (r >= nv || !keep[g]) return;
  const int i = ord[g];
  const float sc = scores[i];
  int total = 0, rank = 0;
  for (int q = 0; q < nv; ++q) {
    if (!keep[base + q]) continue;
    ++total;
    const float sq = scores[ord[base + q]];
    if (sq > sc || (sq == sc && q < r)) ++rank;
  }
  if (rank < max_num) {
    const long long o = (long long)s * max_num + rank;
    for (int k = 0; k < dim; ++k) out_boxes[o * dim + k] = mapped[(long long)i * dim + k];
    out_scores[o] = sc;
    out_labels[o] = labels[i];
  }
  if (rank == 0) out_count[s] = min(total, max_num);
}

// out[0 .. n] = exclusive scan of in[i] clamped to [0, hi]: ONE workgroup, every thread a contiguous chunk
__global__ __launch_bounds__(256) void k_tta_scan(const int* __restrict__ in, int n, int hi, int* __restrict__ out) {
  __shared__ int part[256];
  const int t = threadIdx.x, per = (n + 255) / 256;
  const int lo = min(t * per, n), end = min(lo + per, n);
  int sum = 0;
  for (int i = lo; i < end; ++i) sum += min(max(in[i], 0), hi);
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += add;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int i = lo; i < end; ++i) {
    out[i] = run;
    run += min(max(in[i], 0), hi);
  }
  if (t == 255) out[n] = part[255];
}

// seg, nvalid and out_count <- 0 for the entry that may be captured.  A kernel, not hipMemsetAsync: the memset NODE of a captured graph
// does not leave zeros on replay on this stack (geometry.hip, query.hip fps_launch), and a (scene, class) without candidates keeps
// what the clear left in seg.
__global__ void k_tta_clear(int* __restrict__ seg, int nseg, int* __restrict__ nvalid, int* __restrict__ out_count, int batch) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < nseg) seg[i] = 0;
  if (i < batch) {
    nvalid[i] = 0;
    out_count[i] = 0;
  }
}

// DetBatch's contract: rows at or past out_count[b] are zero (a replay's static outputs still hold the previous replay's rows)
__global__ void k_tta_zero_tail(const int* __restrict__ out_count, int batch, int max_num, int dim, float* __restrict__ out_boxes,
                                float* __restrict__ out_scores, int* __restrict__ out_labels) {
  const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= (long long)batch * max_num) return;
  if ((int)(g % max_num) < out_count[g / max_num]) return;
  for (int k = 0; k < dim; ++k) out_boxes[g * dim + k] = 0.f;
  out_scores[g] = 0.f;
  out_labels[g] = 0;
}

static inline size_t tta_align(size_t b) { return (b + 255) & ~(size_t)255; }

extern "C" int64_t u3d_tta_merge_workspace(int32_t n, int32_t box_dim, int32_t batch, int32_t views, int32_t num_classes,
                                           int32_t max_per_scene) {
  if (n < 0 || batch <= 0 || views <= 0 || num_classes <= 0) return -1;
  size_t b = tta_align((size_t)batch * views * TTA_NP * 4) + tta_align((size_t)n * box_dim * 4) + tta_align((size_t)n * 5 * 4) + tta_align((size_t)n * 4) + tta_align((size_t)n) +
             tta_align((size_t)batch * num_classes * 2 * 4) + tta_align((size_t)batch * 4);
  if (max_per_scene > TTA_LDS_CAP) {
    const size_t nw = ((size_t)max_per_scene + 63) / 64;
    b += tta_align((size_t)batch * max_per_scene * nw * 8);
  }
  return (int64_t)b;
}

// the suppression words of one mask row must fit the sweep's LDS and the mask grid's y dimension
static inline bool tta_global_ok(int max_per_scene) {
  const int nw = (max_per_scene + 63) / 64;
  return max_per_scene <= TTA_LDS_CAP || ((size_t)nw * 8 <= 64 * 1024 && nw <= 65535);
}

// The merge behind both entries.  n bounds the candidates (the grids); the real total is det_off[batch * views], read on the device.
// PADDED: boxes / scores / labels are [batch*views][K] blocks and cscores / clabels receive the candidates' scores and labels in
// concatenated order; otherwise the caller's arrays already are in that order and K, cscores, clabels are unused.
template <bool PADDED>
static int32_t tta_run(const float* boxes, const float* scores, const int32_t* labels, int32_t n, int32_t box_dim, const int32_t* det_off,
                       const float* params, int32_t batch, int32_t views, int32_t coord, int32_t num_classes, float nms_thr,
                       int32_t max_num, int32_t max_per_scene, int32_t K, float* cscores, int32_t* clabels, void* workspace,
                       float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_count, u3d_stream s) {
  const bool global_path = max_per_scene > TTA_LDS_CAP;
  const int nw = (max_per_scene + 63) / 64;
  char* w = (char*)workspace;
  float* inv = (float*)w; w += tta_align((size_t)batch * views * TTA_NP * 4);
  float* mapped = (float*)w; w += tta_align((size_t)n * box_dim * 4);
  float* bev = (float*)w; w += tta_align((size_t)n * 5 * 4);
  int* ord = (int*)w; w += tta_align((size_t)n * 4);
  unsigned char* keep = (unsigned char*)w; w += tta_align((size_t)n);
  int* seg = (int*)w; w += tta_align((size_t)batch * num_classes * 2 * 4);
  int* nvalid = (int*)w; w += tta_align((size_t)batch * 4);
  unsigned long long* mask = global_path ? (unsigned long long*)w : nullptr;
  const float* sc = PADDED ? cscores : scores;              // what every kernel behind k_tta_prep reads, by concatenated index
  const int32_t* lb = PADDED ? clabels : labels;
  if (PADDED) {
    const int nseg = batch * num_classes * 2;
    hipLaunchKernelGGL(k_tta_clear, dim3(u3d_cdiv(nseg, 256)), dim3(256), 0, s, seg, nseg, nvalid, out_count, batch);
  } else {                                                  // (the ragged entry: its out_count is cleared by the caller)
    U3D_REQUIRE(hipMemsetAsync(seg, 0, (size_t)batch * num_classes * 2 * 4, s) == hipSuccess, U3D_ERR_LAUNCH);
    U3D_REQUIRE(hipMemsetAsync(nvalid, 0, (size_t)batch * 4, s) == hipSuccess, U3D_ERR_LAUNCH);
  }
  const int nviews = batch * views;
  hipLaunchKernelGGL(k_tta_inverse, dim3(u3d_cdiv(nviews, 64)), dim3(64), 0, s, params, nviews, inv);
  hipLaunchKernelGGL(k_tta_prep<PADDED>, dim3(u3d_cdiv(n, 256)), dim3(256), 0, s, boxes, scores, labels, det_off, inv, nviews, n, box_dim,
                     coord, K, mapped, bev, cscores, clabels);
  hipLaunchKernelGGL(k_tta_rank, dim3(u3d_cdiv(n, 256)), dim3(256), 0, s, sc, lb, det_off, batch, views, n, num_classes, ord, seg, nvalid);
  hipLaunchKernelGGL(k_tta_nms_lds, dim3(num_classes, batch), dim3(TTA_LDS_THREADS), 0, s, bev, det_off, views, ord, seg, num_classes,
                     nms_thr, keep);
  if (global_path) {
    // (the padded entry: a grid of views * K rows whatever the counts are; blocks past nvalid[s] or of a small segment leave at once.
    //  Measured at 4 x 900 rows, 500 live: 0.10 ms per call for the grid that does nothing - profiles/tta_step_ab.txt)
    hipLaunchKernelGGL(k_tta_mask, dim3(max_per_scene, nw, batch), dim3(64), 0, s, bev, lb, det_off, views, ord, seg, nvalid,
                       num_classes, nms_thr, max_per_scene, nw, mask);
    hipLaunchKernelGGL(k_tta_sweep, dim3(num_classes, batch), dim3(64), (size_t)nw * 8, s, mask, det_off, views, seg, num_classes,
                       max_per_scene, nw, keep);
  }
  hipLaunchKernelGGL(k_tta_select, dim3(u3d_cdiv(n, 256)), dim3(256), 0, s, mapped, sc, lb, det_off, batch, views, n, box_dim, ord,
                     nvalid, keep, max_num, out_boxes, out_scores, out_labels, out_count);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_tta_merge(const float* boxes, const float* scores, const int32_t* labels, int32_t n, int32_t box_dim,
                                 const int32_t* det_off, const float* params, int32_t batch, int32_t views, int32_t coord,
                                 int32_t num_classes, float nms_thr, int32_t max_num, int32_t max_per_scene, void* workspace,
                                 int64_t workspace_bytes, float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_count,
                                 u3d_stream s) {
  U3D_REQUIRE(det_off && params && out_count && batch > 0 && views > 0 && (box_dim == 7 || box_dim == 9) && (coord == 0 || coord == 1) &&
              num_classes > 0 && max_num > 0 && n >= 0 && max_per_scene >= 0, U3D_ERR_ARG);
  U3D_REQUIRE(hipMemsetAsync(out_count, 0, (size_t)batch * 4, s) == hipSuccess, U3D_ERR_LAUNCH);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(boxes && scores && labels && workspace && out_boxes && out_scores && out_labels, U3D_ERR_ARG);
  U3D_REQUIRE(workspace_bytes >= u3d_tta_merge_workspace(n, box_dim, batch, views, num_classes, max_per_scene), U3D_ERR_WORKSPACE);
  U3D_REQUIRE(tta_global_ok(max_per_scene), U3D_ERR_UNSUPPORTED);
  return tta_run<false>(boxes, scores, labels, n, box_dim, det_off, params, batch, views, coord, num_classes, nms_thr, max_num,
                        max_per_scene, 0, nullptr, nullptr, workspace, out_boxes, out_scores, out_labels, out_count, s);
}

// ---- the padded layout of the batched detection tail ------------------------------------------------------------------------------
static inline bool tta_padded_shape_ok(int batch, int views, int K, int box_dim, int num_classes) {
  return batch > 0 && views > 0 && K > 0 && (box_dim == 7 || box_dim == 9) && num_classes > 0;
}

// batch*views*K candidates at most, a scene views*K: what the grids, the workspace and the choice of the NMS path depend on
static inline bool tta_padded_supported(int batch, int views, int K, int num_classes) {
  return batch <= 65535 && K <= U3D_DET_TAIL_MAX_K && (long long)views * K < (1ll << 31) && (long long)batch * views * K < (1ll << 31) &&
         (long long)batch * num_classes * 2 < (1ll << 31) && tta_global_ok(views * K);
}

extern "C" int64_t u3d_tta_merge_padded_workspace(int32_t batch, int32_t views, int32_t max_det, int32_t box_dim, int32_t num_classes) {
  if (!tta_padded_shape_ok(batch, views, max_det, box_dim, num_classes) || !tta_padded_supported(batch, views, max_det, num_classes)) return -1;
  const int n = batch * views * max_det;
  return (int64_t)(tta_align(((size_t)batch * views + 1) * 4) + 2 * tta_align((size_t)n * 4)) +
         u3d_tta_merge_workspace(n, box_dim, batch, views, num_classes, views * max_det);
}

extern "C" int32_t u3d_tta_merge_padded(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int32_t batch,
                                        int32_t views, int32_t max_det, int32_t box_dim, const float* params, int32_t coord,
                                        int32_t num_classes, float nms_thr, int32_t max_num, void* workspace, int64_t workspace_bytes,
                                        float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_count, int32_t* out_off,
                                        u3d_stream s) {
  U3D_REQUIRE(boxes && scores && labels && count && params && workspace && out_boxes && out_scores && out_labels && out_count && out_off,
              U3D_ERR_ARG);
  U3D_REQUIRE(tta_padded_shape_ok(batch, views, max_det, box_dim, num_classes) && (coord == 0 || coord == 1) && max_num > 0, U3D_ERR_ARG);
  U3D_REQUIRE(tta_padded_supported(batch, views, max_det, num_classes) && max_num <= U3D_DET_TAIL_MAX_K, U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE(workspace_bytes >= u3d_tta_merge_padded_workspace(batch, views, max_det, box_dim, num_classes), U3D_ERR_WORKSPACE);
  const int nviews = batch * views, n = nviews * max_det;
  char* w = (char*)workspace;
  int* det_off = (int*)w; w += tta_align(((size_t)nviews + 1) * 4);
  float* cscores = (float*)w; w += tta_align((size_t)n * 4);
  int* clabels = (int*)w; w += tta_align((size_t)n * 4);
  hipLaunchKernelGGL(k_tta_scan, dim3(1), dim3(256), 0, s, count, nviews, max_det, det_off);      // (out_count: cleared in tta_run)
  const int32_t rc = tta_run<true>(boxes, scores, labels, n, box_dim, det_off, params, batch, views, coord, num_classes, nms_thr, max_num,
                                   views * max_det, max_det, cscores, clabels, w, out_boxes, out_scores, out_labels, out_count, s);
  if (rc != U3D_OK) return rc;
  hipLaunchKernelGGL(k_tta_zero_tail, dim3(u3d_cdiv((long long)batch * max_num, 256)), dim3(256), 0, s, out_count, batch, max_num, box_dim,
                     out_boxes, out_scores, out_labels);
  hipLaunchKernelGGL(k_tta_scan, dim3(1), dim3(256), 0, s, out_count, batch, max_num, out_off);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
