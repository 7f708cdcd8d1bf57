// Indoor 3-D detection evaluation on the device: per-class AP (area under the enveloped precision / recall curve) and recall at a set
// of 3-D IoU thresholds, the semantics of mmdet3d's indoor_eval (ref: projects/mmdet3d_plugin/core/indoor_eval.py eval_det_cls :58-140,
// average_precision :7-55).  The reference walks every detection in Python; here:
//   u3d_eval_iou_argmax  per detection: best same-class, same-scene GT (iou_max, jmax) with the reference's strict '>' from -inf, and
//                        the 64-bit sort key (class, descending score)
//   (the caller sorts the keys with a STABLE device sort: ties keep (scene, position in the scene), the project's tie rule)
//   u3d_eval_segments    per class: the [lo, hi) range of its detections in the sorted order, and its GT count npos
//   u3d_eval_first_hit   per threshold and GT: the rank of the earliest eligible (iou_max > t) detection whose jmax is that GT
//   u3d_eval_tp          per threshold and rank: TP iff eligible and first[t][jmax] == rank (== the reference's greedy loop)
//   u3d_eval_ap          per (class, threshold): TP count -> precision at each TP, reverse running max, AP sum in float64
// Every step is deterministic: the only atomics are integer atomicMin, whose result does not depend on arrival order.
#include "common.h"
#include "box_iou.h"

#define EVAL_THREADS 256
#define EVAL_GT_LDS 1024            // GT boxes staged per workgroup (32 B each); the rest of a very large scene is read from global
#define EVAL_AP_THREADS 1024

// descending-orderable score bits: a larger score gives a smaller key; -0.0 is +0.0
__device__ static unsigned int eval_desc_bits(float s) {
  if (s == 0.f) s = 0.f;
  const unsigned int u = __float_as_uint(s);
  const unsigned int asc = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ~asc;
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_iou_argmax(const float* __restrict__ det_boxes, const float* __restrict__ det_scores,
                                                                  const int* __restrict__ det_labels, const int* __restrict__ det_off,
                                                                  const float* __restrict__ gt_boxes, const int* __restrict__ gt_labels,
                                                                  const int* __restrict__ gt_off, int n_scene, int n_det,
                                                                  float* __restrict__ iou_max, int* __restrict__ jmax,
                                                                  long long* __restrict__ sort_key) {
  __shared__ float gsh[EVAL_GT_LDS * 8];      // box (7) + label bits
  __shared__ int range_sh[2];
  const int d0 = blockIdx.x * EVAL_THREADS;
  const int d = d0 + threadIdx.x;
  if (threadIdx.x == 0) {
    const int s0 = u3d_segment_of(det_off, n_scene, d0);
    const int s1 = u3d_segment_of(det_off, n_scene, min(d0 + EVAL_THREADS, n_det) - 1);
    range_sh[0] = gt_off[s0];
    range_sh[1] = gt_off[s1 + 1];
  }
  __syncthreads();
  const int g0 = range_sh[0];
  const int nst = min(range_sh[1] - g0, EVAL_GT_LDS);
  for (int k = threadIdx.x; k < nst * 8; k += EVAL_THREADS) {
    const int j = g0 + (k >> 3), c = k & 7;
    gsh[k] = c < 7 ? gt_boxes[(long long)j * 7 + c] : __int_as_float(gt_labels[j]);
  }
  __syncthreads();
  if (d >= n_det) return;
  const int s = u3d_segment_of(det_off, n_scene, d);
  const int cls = det_labels[d];
  float p[7];
#pragma unroll
  for (int c = 0; c < 7; ++c) p[c] = det_boxes[(long long)d * 7 + c];
  float best = -INFINITY;
  int bj = -1;
  const int ge = gt_off[s + 1];
  for (int j = gt_off[s]; j < ge; ++j) {
    float q[7];
    int gl;
    const int k = j - g0;
    if (k < EVAL_GT_LDS) {
      gl = __float_as_int(gsh[k * 8 + 7]);
      if (gl != cls) continue;
#pragma unroll
      for (int c = 0; c < 7; ++c) q[c] = gsh[k * 8 + c];
    } else {
      gl = gt_labels[j];
      if (gl != cls) continue;
#pragma unroll
      for (int c = 0; c < 7; ++c) q[c] = gt_boxes[(long long)j * 7 + c];
    }
    const float iou = pp_iou3d(p, q);             // pred vs GT, the reference's overlaps(pred, gt) orientation
    if (iou > best) { best = iou; bj = j; }       // strict: the first maximal GT wins, a NaN never does
  }
  iou_max[d] = best;
  jmax[d] = bj;
  sort_key[d] = (long long)(((unsigned long long)(unsigned int)cls << 32) | eval_desc_bits(det_scores[d]));
}

extern "C" int32_t u3d_eval_iou_argmax(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const int32_t* det_off,
                                       const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_off, int32_t n_scene, int32_t n_det,
                                       float* iou_max, int32_t* jmax, int64_t* sort_key, u3d_stream s) {
  U3D_REQUIRE(n_scene >= 0 && n_det >= 0, U3D_ERR_ARG);
  if (n_det == 0) return U3D_OK;              // includes n_scene == 0
  U3D_REQUIRE(det_off && gt_off && n_scene > 0 && det_boxes && det_scores && det_labels && iou_max && jmax && sort_key, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_eval_iou_argmax, dim3(u3d_cdiv(n_det, EVAL_THREADS)), dim3(EVAL_THREADS), 0, s, det_boxes, det_scores, det_labels,
                     det_off, gt_boxes, gt_labels, gt_off, n_scene, n_det, iou_max, jmax, (long long*)sort_key);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// one workgroup per class: seg[2c], seg[2c+1] = [lo, hi) of the class in the sorted keys; npos[c] = number of GT with label c
// ---------------------------------------------------------------------------------------------------------------------------
__device__ static int eval_lower_bound(const long long* __restrict__ key, int n, long long v) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (key[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_segments(const long long* __restrict__ sorted_key, int n_det,
                                                                const int* __restrict__ gt_labels, int n_gt, int* __restrict__ seg,
                                                                int* __restrict__ npos) {
  __shared__ int part[EVAL_THREADS / U3D_WAVE];
  const int c = blockIdx.x;
  int cnt = 0;
  for (int j = threadIdx.x; j < n_gt; j += EVAL_THREADS) cnt += gt_labels[j] == c ? 1 : 0;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int t = 0;
    for (int w = 0; w < EVAL_THREADS / U3D_WAVE; ++w) t += part[w];
    npos[c] = t;
    seg[2 * c] = eval_lower_bound(sorted_key, n_det, (long long)c << 32);
    seg[2 * c + 1] = eval_lower_bound(sorted_key, n_det, (long long)(c + 1) << 32);
  }
}

extern "C" int32_t u3d_eval_segments(const int64_t* sorted_key, int32_t n_det, const int32_t* gt_labels, int32_t n_gt, int32_t num_classes,
                                     int32_t* seg, int32_t* npos, u3d_stream s) {
  U3D_REQUIRE(seg && npos && num_classes > 0 && n_det >= 0 && n_gt >= 0, U3D_ERR_ARG);
  U3D_REQUIRE((sorted_key || n_det == 0) && (gt_labels || n_gt == 0), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_eval_segments, dim3(num_classes), dim3(EVAL_THREADS), 0, s, (const long long*)sorted_key, n_det, gt_labels, n_gt,
                     seg, npos);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// greedy matching as a first-hit rule.  The reference's loop (in score order: TP iff iou_max > t and jmax not yet taken; only TPs take
// a GT) makes a detection a TP iff it is the earliest-ranked eligible detection with its jmax.  first: int32 [n_thr][n_gt].
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_THREADS) void k_eval_first_hit(const long long* __restrict__ perm, int n_det, const float* __restrict__ iou_max,
                                                                 const int* __restrict__ jmax, const float* __restrict__ thr, int n_thr,
                                                                 int n_gt, int* __restrict__ first) {
  const int r = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (r >= n_det) return;
  const int d = (int)perm[r];
  const float v = iou_max[d];
  const int j = jmax[d];
  if (j < 0 || j >= n_gt) return;
  for (int t = 0; t < n_thr; ++t)
    if (v > thr[t]) atomicMin(first + (long long)t * n_gt + j, r);
}

__global__ __launch_bounds__(EVAL_THREADS) void k_eval_tp(const long long* __restrict__ perm, int n_det, const float* __restrict__ iou_max,
                                                          const int* __restrict__ jmax, const float* __restrict__ thr, int n_thr, int n_gt,
                                                          const int* __restrict__ first, unsigned char* __restrict__ tp) {
  const int r = blockIdx.x * EVAL_THREADS + threadIdx.x;
  if (r >= n_det) return;
  const int d = (int)perm[r];
  const float v = iou_max[d];
  const int j = jmax[d];
  const bool ok = j >= 0 && j < n_gt;
  for (int t = 0; t < n_thr; ++t)
    tp[(long long)t * n_det + r] = (ok && v > thr[t] && first[(long long)t * n_gt + j] == r) ? 1 : 0;
}

extern "C" int32_t u3d_eval_first_hit(const int64_t* perm, int32_t n_det, const float* iou_max, const int32_t* jmax, const float* thr,
                                      int32_t n_thr, int32_t n_gt, int32_t* first, u3d_stream s) {
  U3D_REQUIRE(thr && n_thr > 0 && n_det >= 0 && n_gt >= 0, U3D_ERR_ARG);
  if (n_gt == 0) return U3D_OK;
  U3D_REQUIRE(first, U3D_ERR_ARG);
  if (hipMemsetAsync(first, 0x7f, sizeof(int32_t) * (size_t)n_thr * n_gt, s) != hipSuccess) return U3D_ERR_LAUNCH;   // 0x7f7f7f7f > any rank
  if (n_det == 0) return U3D_OK;
  U3D_REQUIRE(perm && iou_max && jmax, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_eval_first_hit, dim3(u3d_cdiv(n_det, EVAL_THREADS)), dim3(EVAL_THREADS), 0, s, (const long long*)perm, n_det, iou_max,
                     jmax, thr, n_thr, n_gt, first);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_eval_tp(const int64_t* perm, int32_t n_det, const float* iou_max, const int32_t* jmax, const float* thr, int32_t n_thr,
                               int32_t n_gt, const int32_t* first, uint8_t* tp, u3d_stream s) {
  U3D_REQUIRE(thr && n_thr > 0 && n_det >= 0 && n_gt >= 0, U3D_ERR_ARG);
  if (n_det == 0) return U3D_OK;
  U3D_REQUIRE(perm && iou_max && jmax && tp && (first || n_gt == 0), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_eval_tp, dim3(u3d_cdiv(n_det, EVAL_THREADS)), dim3(EVAL_THREADS), 0, s, (const long long*)perm, n_det, iou_max, jmax,
                     thr, n_thr, n_gt, first, tp);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// AP, one workgroup per (class, threshold).  With i TPs among the first k+1 ranks of the class, recall = i / npos and precision =
// i / (k+1) in float64 (the reference's cumsum arrays).  The recall only changes at a TP, and the reverse running max of precision at a
// TP equals the max over the TPs at or after it (precision falls between TPs), so 'area' AP = sum over TPs of
// (i/npos - (i-1)/npos) * max_{i' >= i} prec_i'.  Sweep 1 counts TPs in rank order (ballot + popcount) and writes prec_i into a
// compact float64 list (at most npos entries: each TP takes a distinct GT); sweep 2 runs the list backwards with a suffix max and a
// fixed-order sum.  AP is rounded to float32 as the reference stores it; recall stays float64.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_AP_THREADS) void k_eval_ap(const unsigned char* __restrict__ tp, int n_det, const int* __restrict__ seg,
                                                             const int* __restrict__ npos_c, int num_classes, int n_gt,
                                                             double* __restrict__ prec, float* __restrict__ ap, double* __restrict__ rec) {
  constexpr int NW = EVAL_AP_THREADS / U3D_WAVE;
  __shared__ int wcnt[NW];
  __shared__ double wval[NW];
  __shared__ double wsum[NW];
  const int c = blockIdx.x % num_classes, t = blockIdx.x / num_classes;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lo = seg[2 * c], hi = seg[2 * c + 1];
  const int np = npos_c[c];
  int goff = 0;
  for (int k = 0; k < c; ++k) goff += npos_c[k];
  double* pl = prec + (long long)t * n_gt + goff;
  const unsigned char* tpt = tp + (long long)t * n_det;
  // sweep 1: TP ranks -> compact precision list
  int carry = 0;
  for (int base = lo; base < hi; base += EVAL_AP_THREADS) {
    const int pos = base + tid;
    const bool f = pos < hi && tpt[pos] != 0;
    const unsigned long long m = __ballot(f);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    int before = carry, total = 0;
    for (int k = 0; k < NW; ++k) {
      total += wcnt[k];
      if (k < w) before += wcnt[k];
    }
    const int i = before + below + 1;
    if (f && i <= np) pl[i - 1] = (double)i / (double)(pos - lo + 1);
    carry += total;
    __syncthreads();
  }
  const int K = min(carry, np);
  if (np == 0) {
    if (tid == 0) {
      // no GT of this class anywhere: the reference divides by npos = 0 -> NaN recall and NaN AP (the class is only reported if
      // predicted); a class with neither GT nor predictions gets no key and its slot is never read
      ap[t * num_classes + c] = hi > lo ? __int_as_float(0x7fc00000) : 0.f;
      rec[t * num_classes + c] = hi > lo ? __longlong_as_double(0x7ff8000000000000ll) : 0.0;
    }
    return;
  }
  // sweep 2: backwards over the K precisions, suffix max carried from the end, terms summed in a fixed order
  const double dn = (double)np;
  double env_carry = 0.0, acc = 0.0;
  for (int end = K; end > 0; end -= EVAL_AP_THREADS) {
    const int idx = end - EVAL_AP_THREADS + tid;
    const bool valid = idx >= 0;
    double v = valid ? pl[idx] : 0.0;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double u = __shfl_down(v, o, 64);
      if (lane + o < 64) v = fmax(v, u);
    }
    if (lane == 0) wval[w] = v;
    __syncthreads();
    double after = env_carry, all = env_carry;
    for (int k = 0; k < NW; ++k) {
      all = fmax(all, wval[k]);
      if (k > w) after = fmax(after, wval[k]);
    }
    const double env = fmax(v, after);
    const double term = valid ? ((double)(idx + 1) / dn - (double)idx / dn) * env : 0.0;
    const double ws = u3d_wave_sum_d(term);
    if (lane == 0) wsum[w] = ws;
    __syncthreads();
    if (tid == 0)
      for (int k = 0; k < NW; ++k) acc += wsum[k];
    env_carry = all;
    __syncthreads();
  }
  if (tid == 0) {
    ap[t * num_classes + c] = (float)acc;
    rec[t * num_classes + c] = (double)K / dn;
  }
}

extern "C" int32_t u3d_eval_ap(const uint8_t* tp, int32_t n_det, const int32_t* seg, const int32_t* npos, int32_t num_classes, int32_t n_thr,
                               int32_t n_gt, double* prec_ws, float* ap, double* rec, u3d_stream s) {
  U3D_REQUIRE(seg && npos && ap && rec && num_classes > 0 && n_thr > 0 && n_det >= 0 && n_gt >= 0, U3D_ERR_ARG);
  U3D_REQUIRE((tp || n_det == 0) && (prec_ws || n_gt == 0), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_eval_ap, dim3(num_classes * n_thr), dim3(EVAL_AP_THREADS), 0, s, tp, n_det, seg, npos, num_classes, n_gt, prec_ws, ap,
                     rec);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
