// Batch ingest (u3d_batch_ingest): a DevicePipeline batch -> the static input buffers of a capacity-mode TrainStep
// (uni3detr_amd/trainer.py), without a host read.  The pipeline's batch is packed [n_src, F] with per-scene segments scene_off and,
// after a range filter, a live prefix count[b] per segment; its boxes are bottom-centre [g_src, 7|9] with gt_off / gt_count.  The step
// reads `cat` [B*P, F] exactly packed (scene b = rows dst_off[b] .. dst_off[b+1], live rows only, order kept; rows past dst_off[B]
// are spare capacity nothing reads) and the GT layout Uni3DETRHead._pack_gts makes (gravity centre z + dz/2, gt_dim = 7 | 9 columns,
// labels int32, gt_off).  P / G are per-scene capacities: a scene above one of them is cut to it and reported - `flag` (one float,
// ADDED to) feeds the step's HOLD flag, so a cut batch never updates the weights; `overflow` counts the calls by kind.
//
// Two launches whatever B is:
//   k_ingest_scan  one workgroup: live counts clamped to segment and capacity, exclusive scan -> dst_off / gt_off_out, flag, counters
//   k_ingest_rows  one thread per 16-byte (F % 4 == 0) or 4-byte unit of a live destination row; the row finds its scene by a
//                  binary search over the B + 1 destination offsets held in LDS; behind the point blocks, one thread per GT row
// Bandwidth-trivial (nuScenes: ~1.4 M rows x 20 B): nothing here is tuned beyond "no scratch, no spills".
#include "common.h"

#define INGEST_THREADS 256
#define INGEST_MAX_BATCH 4096      /* B + 1 offsets in LDS: 16 KiB */

__device__ __forceinline__ int ingest_live(const int* __restrict__ off, const int* __restrict__ cnt, int b) {
  const int seg = off[b + 1] - off[b];
  int live = cnt ? cnt[b] : seg;
  live = live > seg ? seg : live;
  return live < 0 ? 0 : live;
}

__device__ __forceinline__ int ingest_wave_scan(int v, int lane) {      // inclusive, 64 lanes
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

__global__ __launch_bounds__(INGEST_THREADS) void k_ingest_scan(const int* __restrict__ scene_off, const int* __restrict__ count, int B, int P,
                                                                const int* __restrict__ gt_off, const int* __restrict__ gt_count, int G,
                                                                int* __restrict__ dst_off, int* __restrict__ gt_off_out,
                                                                float* __restrict__ flag, int* __restrict__ overflow) {
  constexpr int NW = INGEST_THREADS / 64;
  __shared__ int s_wp[NW], s_wg[NW], s_carry[2], s_over[2];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if (tid < 2) { s_carry[tid] = 0; s_over[tid] = 0; }
  __syncthreads();
  for (int base = 0; base < B; base += INGEST_THREADS) {
    const int b = base + tid;
    int n = 0, g = 0;
    if (b < B) {
      const int live = ingest_live(scene_off, count, b);
      n = live > P ? P : live;
      if (live > P) atomicOr(&s_over[0], 1);
      if (gt_off) {
        const int glive = ingest_live(gt_off, gt_count, b);
        g = glive > G ? G : glive;
        if (glive > G) atomicOr(&s_over[1], 1);
      }
    }
    const int ip = ingest_wave_scan(n, lane), ig = ingest_wave_scan(g, lane);
    if (lane == 63) { s_wp[wid] = ip; s_wg[wid] = ig; }
    __syncthreads();
    int wp = s_carry[0], wg = s_carry[1], tp = 0, tg = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
      if (w < wid) { wp += s_wp[w]; wg += s_wg[w]; }
      tp += s_wp[w]; tg += s_wg[w];
    }
    if (b < B) {
      dst_off[b] = wp + ip - n;
      if (gt_off_out) gt_off_out[b] = wg + ig - g;
    }
    __syncthreads();
    if (tid == 0) { s_carry[0] += tp; s_carry[1] += tg; }
    __syncthreads();
  }
  if (tid == 0) {
    dst_off[B] = s_carry[0];
    if (gt_off_out) gt_off_out[B] = s_carry[1];
    if (s_over[0] | s_over[1]) *flag += 1.f;
    if (overflow) { overflow[0] += s_over[0]; overflow[1] += s_over[1]; }
  }
}

template <int W>
__global__ __launch_bounds__(INGEST_THREADS) void k_ingest_rows(const float* __restrict__ points, int n_src, int F,
                                                                const int* __restrict__ scene_off, const int* __restrict__ dst_off, int B,
                                                                float* __restrict__ cat, int point_blocks, const float* __restrict__ gt,
                                                                int g_src, int sd, const int* __restrict__ gt_labels,
                                                                const int* __restrict__ gt_off, const int* __restrict__ gt_off_out, int gd,
                                                                float* __restrict__ gt_out, int* __restrict__ labels_out) {
  extern __shared__ int s_off[];        // B + 1 destination offsets (points or boxes: uniform per workgroup)
  const bool pts = (int)blockIdx.x < point_blocks;
  const int* off = pts ? dst_off : gt_off_out;
  for (int i = threadIdx.x; i <= B; i += INGEST_THREADS) s_off[i] = off[i];
  __syncthreads();
  if (pts) {
    const int upr = F / W;              // units per row
    const long long u = (long long)blockIdx.x * INGEST_THREADS + threadIdx.x;
    const long long row = u / upr;
    if (row >= s_off[B]) return;
    const int q = (int)(u - row * upr), b = u3d_segment_of(s_off, B, (int)row);
    const long long src = (long long)scene_off[b] + (row - s_off[b]);
    if (src >= n_src) return;           // (offsets that point past the source: nothing is read there)
    if (W == 4) ((float4*)cat)[row * upr + q] = ((const float4*)points)[src * upr + q];
    else cat[row * F + q] = points[src * F + q];
    return;
  }
  const long long j = (long long)(blockIdx.x - point_blocks) * INGEST_THREADS + threadIdx.x;
  if (j >= s_off[B]) return;
  const int b = u3d_segment_of(s_off, B, (int)j);
  const long long src = (long long)gt_off[b] + (j - s_off[b]);
  if (src >= g_src) return;
  const float* r = gt + src * sd;
  float* o = gt_out + j * gd;
  o[0] = r[0]; o[1] = r[1];
  o[2] = __fadd_rn(r[2], __fmul_rn(r[5], 0.5f));      // bottom centre -> gravity centre (Boxes3D.gravity_center)
  o[3] = r[3]; o[4] = r[4]; o[5] = r[5]; o[6] = r[6];
  if (gd == 9) { o[7] = sd == 9 ? r[7] : 0.f; o[8] = sd == 9 ? r[8] : 0.f; }
  labels_out[j] = gt_labels[src];
}

extern "C" int32_t u3d_batch_ingest(const float* points, int32_t n_src, int32_t feat, const int32_t* scene_off, const int32_t* count,
                                    int32_t batch, int32_t point_cap, const float* gt, int32_t g_src, int32_t box_dim,
                                    const int32_t* gt_labels, const int32_t* gt_off, const int32_t* gt_count, int32_t gt_cap, int32_t gt_dim,
                                    float* cat, int32_t* dst_off, float* gt_out, int32_t* labels_out, int32_t* gt_off_out, float* flag,
                                    int32_t* overflow, u3d_stream s) {
  U3D_REQUIRE(scene_off && cat && dst_off && flag && batch > 0 && batch <= INGEST_MAX_BATCH && n_src >= 0 && (points || n_src == 0) &&
                  feat >= 1 && point_cap > 0 && (long long)batch * point_cap < 0x7fffffffll, U3D_ERR_ARG);
  const bool has_gt = gt != nullptr && g_src > 0;
  if (has_gt || gt_out)
    U3D_REQUIRE(gt_out && labels_out && gt_off_out && gt_cap > 0 && (gt_dim == 7 || gt_dim == 9) &&
                    (long long)batch * gt_cap < 0x7fffffffll, U3D_ERR_ARG);
  if (has_gt) U3D_REQUIRE(gt_labels && gt_off && (box_dim == 7 || box_dim == 9) && g_src >= 0, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_ingest_scan, dim3(1), dim3(INGEST_THREADS), 0, (hipStream_t)s, scene_off, count, batch, point_cap,
                     has_gt ? gt_off : (const int32_t*)nullptr, gt_count, gt_cap, dst_off, gt_off_out, flag, overflow);
  const long long cap_rows = (long long)batch * point_cap, cap_g = (long long)batch * gt_cap;
  const long long rows = n_src < cap_rows ? n_src : cap_rows;
  const long long grow = has_gt ? (g_src < cap_g ? g_src : cap_g) : 0;
  const bool vec = feat % 4 == 0 && (((uintptr_t)points | (uintptr_t)cat) & 15) == 0;
  const int upr = vec ? feat / 4 : feat;
  const long long pb = (rows * upr + INGEST_THREADS - 1) / INGEST_THREADS, gb = (grow + INGEST_THREADS - 1) / INGEST_THREADS;
  U3D_REQUIRE(pb + gb < 0x7fffffffll, U3D_ERR_ARG);
  if (pb + gb > 0) {
    const size_t lds = (size_t)(batch + 1) * sizeof(int);
    if (vec)
      hipLaunchKernelGGL(k_ingest_rows<4>, dim3((unsigned)(pb + gb)), dim3(INGEST_THREADS), lds, (hipStream_t)s, points, n_src, feat, scene_off,
                         (const int32_t*)dst_off, batch, cat, (int)pb, gt, g_src, box_dim, gt_labels, gt_off, (const int32_t*)gt_off_out, gt_dim,
                         gt_out, labels_out);
    else
      hipLaunchKernelGGL(k_ingest_rows<1>, dim3((unsigned)(pb + gb)), dim3(INGEST_THREADS), lds, (hipStream_t)s, points, n_src, feat, scene_off,
                         (const int32_t*)dst_off, batch, cat, (int)pb, gt, g_src, box_dim, gt_labels, gt_off, (const int32_t*)gt_off_out, gt_dim,
                         gt_out, labels_out);
  }
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
