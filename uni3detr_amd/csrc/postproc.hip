// Test-time post-processing on the device:
//   u3d_soft_nms   class-wise Gaussian soft-NMS with the rotated 3-D IoU (ref: models/dense_heads/uni3detr_head.py:796-823, called
//                  per class from get_bboxes :849-880) - the reference is a host loop with two .item() syncs per kept box
//   u3d_box_merge  KITTI "box_merging": score-sorted greedy merge, each kept box replaced by the per-coordinate MEDIAN of itself and
//                  the same-class boxes it absorbs (ref: core/bbox/bbox_merging.py:112-158 bboxes_nms_merge_only with
//                  overlapped_boxes_3d_fast_poly :67-92, called from uni3detr_head.py:881-891 with overlapped_thres 0.1) - the
//                  reference is numpy + shapely on the CPU
#include "common.h"
#include "box_iou.h"
#include "postproc_math.h"

// ---------------------------------------------------------------------------------------------------------------------------
// soft-NMS: one workgroup per class.  out_idx / out_score: [num_classes][n] (selection order), out_cnt [num_classes].
// ---------------------------------------------------------------------------------------------------------------------------
#define SNMS_THREADS 256
__global__ __launch_bounds__(SNMS_THREADS) void k_soft_nms(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                           const int* __restrict__ labels, int n, float sigma, float prune,
                                                           int* __restrict__ out_idx, float* __restrict__ out_score, int* __restrict__ out_cnt) {
  extern __shared__ unsigned char smem[];
  float* sc = (float*)smem;                 // [n] current score of member k (dead: -1)
  int* mem = (int*)(sc + n);                // [n] original index of member k
  __shared__ float red_v[SNMS_THREADS];
  __shared__ int red_i[SNMS_THREADS];
  __shared__ int m_sh, top_sh;
  __shared__ float topbox[7];
  const int cls = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int m = 0;
    for (int i = 0; i < n; ++i)
      if (labels[i] == cls) { mem[m] = i; sc[m] = scores[i]; ++m; }
    m_sh = m;
  }
  __syncthreads();
  const int m = m_sh;
  int cnt = 0;
  while (true) {
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int k = tid; k < m; k += SNMS_THREADS) {
      const float v = sc[k];
      if (v >= 0.f && (v > bv || (v == bv && k < bi))) { bv = v; bi = k; }
    }
    red_v[tid] = bv; red_i[tid] = bi;
    __syncthreads();
    for (int s = SNMS_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const float v2 = red_v[tid + s];
        const int i2 = red_i[tid + s];
        if (v2 > red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) { red_v[tid] = v2; red_i[tid] = i2; }
      }
      __syncthreads();
    }
    if (red_i[0] == 0x7fffffff) break;              // nothing alive
    if (tid == 0) {
      const int k = red_i[0];
      top_sh = k;
      out_idx[(long long)cls * n + cnt] = mem[k];
      out_score[(long long)cls * n + cnt] = red_v[0];
      for (int j = 0; j < 7; ++j) topbox[j] = boxes[(long long)mem[k] * 7 + j];
    }
    __syncthreads();
    const int top = top_sh;
    for (int k = tid; k < m; k += SNMS_THREADS) {
      float v = sc[k];
      if (v < 0.f) continue;
      const float iou = pp_iou3d(topbox, boxes + (long long)mem[k] * 7);
      v = pp_soft_decay(v, iou, sigma);
      sc[k] = (k != top && v > prune) ? v : -1.f;
    }
    ++cnt;
    __syncthreads();
  }
  if (tid == 0) out_cnt[cls] = cnt;
}

extern "C" int32_t u3d_soft_nms(const float* boxes, const float* scores, const int32_t* labels, int32_t n, int32_t num_classes, float sigma,
                                float prune, int32_t* out_idx, float* out_score, int32_t* out_cnt, u3d_stream s) {
  U3D_REQUIRE(boxes && scores && labels && out_idx && out_score && out_cnt && num_classes > 0 && sigma > 0.f, U3D_ERR_ARG);
  if (n <= 0) {
    (void)hipMemsetAsync(out_cnt, 0, sizeof(int32_t) * num_classes, s);
    return U3D_OK;
  }
  const size_t lds = (size_t)n * 8;
  U3D_REQUIRE(lds <= 60 * 1024, U3D_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(k_soft_nms, dim3(num_classes), dim3(SNMS_THREADS), lds, s, boxes, scores, labels, n, sigma, prune, out_idx, out_score,
                     out_cnt);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// box merging.  Input boxes are ALREADY sorted by descending score.  The overlap is pp_merge_overlap (postproc_math.h), which keeps
// the reference's camera-axis reading of the LiDAR columns.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ void k_merge_mask(const float* __restrict__ boxes, const int* __restrict__ labels, int n, float thr,
                             unsigned long long* __restrict__ mask, int nw) {
  const int i = blockIdx.x, j = blockIdx.y * 64 + threadIdx.x;
  bool hit = false;
  if (j < n && j > i && labels[i] == labels[j]) hit = pp_merge_overlap(boxes + (long long)i * 7, boxes + (long long)j * 7) > thr;
  const unsigned long long b = __ballot(hit);
  if (threadIdx.x == 0) mask[(long long)i * nw + blockIdx.y] = b;
}
// one wavefront: keep[i] and, for kept i, its members (row & still-alive) written back into its mask row
__global__ void k_merge_sweep(unsigned long long* __restrict__ mask, int n, int nw, unsigned char* __restrict__ keep) {
  extern __shared__ unsigned long long removed[];
  for (int w = threadIdx.x; w < nw; w += 64) removed[w] = 0ull;
  __syncthreads();
  for (int i = 0; i < n; ++i) {
    const bool alive = !((removed[i >> 6] >> (i & 63)) & 1ull);
    if (threadIdx.x == 0) keep[i] = alive ? 1 : 0;
    if (alive) {
      for (int w = threadIdx.x; w < nw; w += 64) {
        const unsigned long long r = mask[(long long)i * nw + w] & ~removed[w];
        mask[(long long)i * nw + w] = r;
        removed[w] |= r;
      }
    }
    __syncthreads();
  }
}
// one workgroup per box: kept boxes become the per-column median over {members, self}; others are copied
#define MERGE_THREADS 256
__global__ __launch_bounds__(MERGE_THREADS) void k_merge_median(const float* __restrict__ boxes, const unsigned long long* __restrict__ mask,
                                                                const unsigned char* __restrict__ keep, int n, int nw, float* __restrict__ out) {
  extern __shared__ int members[];           // [n]
  __shared__ int m_sh;
  const int i = blockIdx.x, tid = threadIdx.x;
  if (!keep[i]) {
    if (tid < 7) out[(long long)i * 7 + tid] = boxes[(long long)i * 7 + tid];
    return;
  }
  if (tid == 0) {
    int m = 0;
    for (int w = 0; w < nw; ++w) {
      unsigned long long b = mask[(long long)i * nw + w];
      while (b) {
        const int t = __ffsll((long long)b) - 1;
        members[m++] = w * 64 + t;
        b &= b - 1ull;
      }
    }
    members[m++] = i;
    m_sh = m;
  }
  __syncthreads();
  const int m = m_sh;
  __shared__ float lo[7], hi[7];
  for (int col = 0; col < 7; ++col) {
    // rank selection: the element whose rank (ties by position) is (m-1)/2 and the one of rank m/2
    for (int a = tid; a < m; a += MERGE_THREADS) {
      const float va = boxes[(long long)members[a] * 7 + col];
      int rank = 0;
      for (int b = 0; b < m; ++b) {
        const float vb = boxes[(long long)members[b] * 7 + col];
        rank += (vb < va || (vb == va && b < a)) ? 1 : 0;
      }
      if (rank == (m - 1) / 2) lo[col] = va;
      if (rank == m / 2) hi[col] = va;
    }
  }
  __syncthreads();
  if (tid < 7) out[(long long)i * 7 + tid] = pp_median_of(lo[tid], hi[tid], m);
}

extern "C" int64_t u3d_box_merge_workspace(int32_t n) { return (int64_t)n * ((n + 63) / 64) * 8; }

extern "C" int32_t u3d_box_merge(const float* boxes, const int32_t* labels, int32_t n, float thr, float* merged, uint8_t* keep,
                                 void* workspace, int64_t workspace_bytes, u3d_stream s) {
  U3D_REQUIRE(boxes && labels && merged && keep && workspace, U3D_ERR_ARG);
  if (n <= 0) return U3D_OK;
  const int nw = (n + 63) / 64;
  U3D_REQUIRE(workspace_bytes >= u3d_box_merge_workspace(n), U3D_ERR_WORKSPACE);
  U3D_REQUIRE((size_t)nw * 8 <= 48 * 1024 && (size_t)n * 4 <= 60 * 1024, U3D_ERR_UNSUPPORTED);
  unsigned long long* mask = (unsigned long long*)workspace;
  hipLaunchKernelGGL(k_merge_mask, dim3(n, nw), dim3(64), 0, s, boxes, labels, n, thr, mask, nw);
  hipLaunchKernelGGL(k_merge_sweep, dim3(1), dim3(64), (size_t)nw * 8, s, mask, n, nw, keep);
  hipLaunchKernelGGL(k_merge_median, dim3(n), dim3(MERGE_THREADS), (size_t)n * 4, s, boxes, (const unsigned long long*)mask, keep, n, nw, merged);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
