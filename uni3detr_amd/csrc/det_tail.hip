// The inference tail after the head's forward, for every scene of a batch in one call (u3d_det_tail): the selection of
// NMSFreeCoder.decode_single (ref: core/bbox/coders/nms_free_coder.py:42-100) and the post-processing of Uni3DETRHead.get_bboxes (ref:
// models/dense_heads/uni3detr_head.py:827-918) for post_processing None / 'nms', bit for bit what the per-scene host loop gives.  The
// transcendental part (layer mean, sigmoid, denormalize_bbox, score fusion) stays in torch, batched; the kernels here only select,
// compare, move and run the rotated IoU:
//   k_dt_select  one workgroup per scene.  Key of a (query, class) entry = monotone-uint32(prob) in the high word (inverted), flat index
//                in the low word.  The k-th largest 32-bit score key by four 8-bit histogram passes (LDS counters), the winners - every key
//                above it and the first ties by ascending flat index - compacted with ballot + popcount, then a bitonic sort of the K
//                64-bit keys in LDS: descending score, ascending (query, class) index, the pinned order of decode_single.  The keep mask
//                (centre within center_range, prob > score_threshold) compacts that list stably -> the coder's output order.
//                NMS mode: the kept candidates are sorted once more by (label asc, fused score desc, compacted position asc) - the order
//                nms3d_classwise emits - their BEV rows (cx, cy, dx, dy, yaw) and the (scene, class) segments go to the workspace.
//   k_dt_nms     one workgroup per (scene, class) segment: greedy rotated-BEV NMS in that order with pp_iou_bev, the arithmetic of
//                bev_iou_rot (u3d_nms3d).  Suppression never crosses labels, so the greedy pass per segment equals the pass over the
//                whole score-sorted scene.  Segments of at most DT_LDS_CAP = 2048 candidates hold their BEV rows in LDS (40 KiB); larger
//                ones run the same loop on the rows in the workspace (no mask matrix: K <= 8192 rows stay in L2).
//   k_dt_emit    one workgroup per scene: survivors with fused score > score_thr[label], stably compacted; with num_thr > 0 sorted by
//                (fused score desc, position asc) and cut - the per-scene path's torch.argsort(-scores) leaves ties open there, this is the
//                pin -; boxes gathered (z -= dz * 0.5 in two rounded f32 steps unless the caller asks for the coder's gravity centres),
//                rows past the count zeroed, count written.
//   k_dt_offsets out_off = exclusive scan of out_count (the det_off layout of u3d_eval_* / u3d_tta_merge).
// No atomics on global memory (LDS counters are integers: any order gives the same sum), so two runs give the same bytes.
// Limits: K = min(max_num, nq * num_classes) <= 8192, box_dim 7 or 9, nq * num_classes < 2^31, num_classes <= 65536.
// Non-finite scores are outside the contract (torch orders NaN above everything; here a NaN orders by its bit pattern).
#include "common.h"
#include "box_iou.h"

#define DT_THREADS 1024
#define DT_WAVES (DT_THREADS / 64)
#define DT_MAX_K U3D_DET_TAIL_MAX_K
#define DT_LDS_CAP U3D_DET_TAIL_LDS_CAP
#define DT_NMS_THREADS 256
#define DT_POS_BITS 13                 /* a position < DT_MAX_K = 2^13 */
#define DT_PAD 0xffffffffffffffffull

typedef unsigned long long dt_u64;

// larger float <-> larger key; -0 counts as +0, as in a float comparison
__device__ __forceinline__ unsigned dt_mono(float v) {
  if (v == 0.f) v = 0.f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// rank of this thread's flag among the set flags of the workgroup in thread order; *total = how many are set.  Called by ALL threads.
__device__ __forceinline__ int dt_scan(bool f, int* wsum, int* total) {
  const dt_u64 b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();                                             // the previous call's reads of wsum are over
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int before = 0, tot = 0;
  for (int k = 0; k < DT_WAVES; ++k) {
    const int v = wsum[k];
    if (k < w) before += v;
    tot += v;
  }
  *total = tot;
  return before + in_wave;
}

// ascending bitonic sort of a[0 .. p), p a power of two, in LDS; ends with a barrier
__device__ void dt_bitonic(dt_u64* a, int p) {
  for (int k = 2; k <= p; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int t = threadIdx.x; t < (p >> 1); t += DT_THREADS) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
        const bool up = (i & k) == 0;
        const dt_u64 x = a[i], y = a[l];
        if ((x > y) == up) { a[i] = y; a[l] = x; }
      }
    }
  __syncthreads();
}

// cand0 [B][K]: flat index by compacted position (NMS mode); cand [B][K]: flat index by final position of this kernel; ncand [B];
// seg [B][C][2] = (first, one past last) position of the class; bev [B][K][5]
__global__ __launch_bounds__(DT_THREADS) void k_dt_select(const float* __restrict__ prob, const float* __restrict__ fused,
                                                          const float* __restrict__ boxes, int nq, int ncls, int dim, int K, int P,
                                                          const float* __restrict__ range, float score_threshold, int nms,
                                                          int* __restrict__ cand0, int* __restrict__ cand, int* __restrict__ ncand,
                                                          int* __restrict__ seg, float* __restrict__ bev) {
  extern __shared__ dt_u64 keys[];                             // [P]
  __shared__ int hist[256];
  __shared__ int wsum[DT_WAVES];
  __shared__ unsigned sel_prefix;
  __shared__ int sel_remaining;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = nq * ncls;
  const float* pr = prob + (long long)b * N;
  const float* fu = fused + (long long)b * N;
  const float* bx = boxes + (long long)b * nq * dim;
  cand0 += (long long)b * K; cand += (long long)b * K; bev += (long long)b * K * 5; seg += (long long)b * ncls * 2;

  // ---- the K-th largest score key: 8 bits per pass, most significant first ----
  if (tid == 0) { sel_prefix = 0u; sel_remaining = K; }
  unsigned mask = 0u;
  for (int shift = 24; shift >= 0; shift -= 8) {
    for (int i = tid; i < 256; i += DT_THREADS) hist[i] = 0;
    __syncthreads();
    const unsigned prefix = sel_prefix;
    for (long long i = tid; i < N; i += DT_THREADS) {        // 64-bit: N may lie within DT_THREADS of 2^31
      const unsigned k = dt_mono(pr[i]);
      if ((k & mask) == prefix) atomicAdd(&hist[(k >> shift) & 255u], 1);
    }
    __syncthreads();
    if (tid == 0) {
      int rem = sel_remaining, bin = 255;
      while (bin > 0 && hist[bin] < rem) rem -= hist[bin--];  // the matching keys number >= rem, so the walk ends inside the table
      sel_prefix = prefix | ((unsigned)bin << shift);
      sel_remaining = rem;
    }
    __syncthreads();
    mask |= 255u << shift;
  }
  const unsigned kth = sel_prefix;
  const int need = sel_remaining;                              // how many entries that tie with the k-th are taken, lowest index first

  // ---- winners -> keys[0 .. K) ----
  int eq_seen = 0, w_seen = 0;
  for (long long base = 0; base < N; base += DT_THREADS) {   // 64-bit, as above; a valid i fits the key's low word
    const long long i = base + tid;
    const bool valid = i < N;
    const unsigned k = valid ? dt_mono(pr[i]) : 0u;
    const bool eq = valid && k == kth;
    int tot;
    const int r = dt_scan(eq, wsum, &tot);
    const bool win = valid && (k > kth || (eq && eq_seen + r < need));
    eq_seen += tot;
    const int s = dt_scan(win, wsum, &tot);
    if (win && w_seen + s < K) keys[w_seen + s] = ((dt_u64)(~k) << 32) | (unsigned)i;      // exactly K win; the bound is a guard
    w_seen += tot;
  }
  for (int i = K + tid; i < P; i += DT_THREADS) keys[i] = DT_PAD;
  dt_bitonic(keys, P);                                         // descending score, ascending flat index

  // ---- keep mask, stable compaction.  In NMS mode the new key of compacted position j overwrites keys[j]: j <= the position read,
  //      and every read of a tile happens before the barriers inside dt_scan, every write after them ----
  float lo[3], hi[3];
  for (int a = 0; a < 3; ++a) { lo[a] = range[a]; hi[a] = range[3 + a]; }
  int n = 0;
  for (int base = 0; base < K; base += DT_THREADS) {
    const int p = base + tid;
    const bool valid = p < K;
    const int idx = valid ? (int)(unsigned)keys[p] : 0;
    bool keep = valid;
    if (valid) {
      const float* c = bx + (long long)(idx / ncls) * dim;
      for (int a = 0; a < 3; ++a) keep = keep && c[a] >= lo[a] && c[a] <= hi[a];
      if (score_threshold > 0.f) keep = keep && pr[idx] > score_threshold;
    }
    int tot;
    const int j = n + dt_scan(keep, wsum, &tot);
    if (keep) {
      if (nms) {
        cand0[j] = idx;
        keys[j] = ((dt_u64)(unsigned)(idx % ncls) << (32 + DT_POS_BITS)) | ((dt_u64)(~dt_mono(fu[idx])) << DT_POS_BITS) | (unsigned)j;
      } else {
        cand[j] = idx;
      }
    }
    n += tot;
  }
  if (tid == 0) ncand[b] = n;
  if (!nms) return;

  // ---- NMS order: label ascending, fused score descending, compacted position ascending ----
  for (int c = tid; c < 2 * ncls; c += DT_THREADS) seg[c] = 0;
  __syncthreads();
  for (int i = n + tid; i < P; i += DT_THREADS) keys[i] = DT_PAD;
  dt_bitonic(keys, P);
  for (int r = tid; r < n; r += DT_THREADS) {
    const dt_u64 k = keys[r];
    const int idx = cand0[(int)(k & ((1u << DT_POS_BITS) - 1u))];
    const int lab = (int)(k >> (32 + DT_POS_BITS));
    cand[r] = idx;
    const float* c = bx + (long long)(idx / ncls) * dim;
    float* o = bev + (long long)r * 5;
    o[0] = c[0]; o[1] = c[1]; o[2] = c[3]; o[3] = c[4]; o[4] = c[6];
    if (r == 0 || (int)(keys[r - 1] >> (32 + DT_POS_BITS)) != lab) seg[2 * lab] = r;
    if (r == n - 1 || (int)(keys[r + 1] >> (32 + DT_POS_BITS)) != lab) seg[2 * lab + 1] = r + 1;
  }
}

// greedy pass over rows[0 .. cnt) (5 floats each, best first); removed[] in LDS
__device__ __forceinline__ void dt_greedy(const float* rows, int cnt, float thr, unsigned char* removed) {
  const int t = threadIdx.x;
  for (int i = 0; i < cnt; ++i) {
    __syncthreads();                                           // removed[i] is final: only rows < i write it
    if (removed[i]) continue;
    const float* bi = rows + i * 5;
    for (int j = i + 1 + t; j < cnt; j += DT_NMS_THREADS)
      if (!removed[j] && pp_iou_bev(bi, rows + j * 5) > thr) removed[j] = 1;
  }
  __syncthreads();
}

__global__ __launch_bounds__(DT_NMS_THREADS) void k_dt_nms(const float* __restrict__ bev, const int* __restrict__ seg, int ncls, int K,
                                                           float thr, unsigned char* __restrict__ keep) {
  __shared__ float sb[DT_LDS_CAP * 5];
  __shared__ unsigned char removed[DT_MAX_K];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int start = seg[((long long)b * ncls + c) * 2], end = seg[((long long)b * ncls + c) * 2 + 1];
  const int cnt = end - start;
  if (cnt <= 0) return;
  const float* rows = bev + ((long long)b * K + start) * 5;
  for (int r = t; r < cnt; r += DT_NMS_THREADS) removed[r] = 0;
  if (cnt <= DT_LDS_CAP) {
    for (int r = t; r < cnt * 5; r += DT_NMS_THREADS) sb[r] = rows[r];
    dt_greedy(sb, cnt, thr, removed);
  } else {
    dt_greedy(rows, cnt, thr, removed);
  }
  for (int r = t; r < cnt; r += DT_NMS_THREADS) keep[(long long)b * K + start + r] = removed[r] ? 0 : 1;
}

// the two steps of get_bboxes' `boxes[:, 2] - boxes[:, 5] * 0.5`, each rounded to f32 (no contraction into one fused multiply-add)
__device__ __forceinline__ float dt_bottom_z(float z, float dz) {
#pragma clang fp contract(off)
  const float half = dz * 0.5f;
  return z - half;
}

__device__ __forceinline__ void dt_write(const float* __restrict__ bx, const float* __restrict__ fu, int idx, int ncls, int dim,
                                         int bottom, long long o, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                         int* __restrict__ out_labels) {
  const float* c = bx + (long long)(idx / ncls) * dim;
  float* ob = out_boxes + o * dim;
  for (int k = 0; k < dim; ++k) ob[k] = (k == 2 && bottom) ? dt_bottom_z(c[2], c[5]) : c[k];
  out_scores[o] = fu[idx];
  out_labels[o] = idx % ncls;
}

__global__ __launch_bounds__(DT_THREADS) void k_dt_emit(const float* __restrict__ fused, const float* __restrict__ boxes, int nq, int ncls,
                                                        int dim, int K, int P, const int* __restrict__ cand,
                                                        const int* __restrict__ ncand, const unsigned char* __restrict__ keep,
                                                        const float* __restrict__ score_thr, int num_thr, int bottom,
                                                        float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                        int* __restrict__ out_labels, int* __restrict__ out_count) {
  extern __shared__ dt_u64 keys[];                             // [P] when num_thr > 0
  __shared__ int wsum[DT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = nq * ncls;
  const float* fu = fused + (long long)b * N;
  const float* bx = boxes + (long long)b * nq * dim;
  cand += (long long)b * K;
  const int n = ncand[b];
  int m = 0;
  for (int base = 0; base < n; base += DT_THREADS) {
    const int r = base + tid;
    bool ok = r < n;
    int idx = 0;
    if (ok) {
      idx = cand[r];
      if (keep) ok = keep[(long long)b * K + r] != 0;
      if (ok && score_thr) ok = fu[idx] > score_thr[idx % ncls];
    }
    int tot;
    const int pos = m + dt_scan(ok, wsum, &tot);
    if (ok) {
      if (num_thr > 0) keys[pos] = ((dt_u64)(~dt_mono(fu[idx])) << 32) | (unsigned)r;
      else dt_write(bx, fu, idx, ncls, dim, bottom, (long long)b * K + pos, out_boxes, out_scores, out_labels);
    }
    m += tot;
  }
  int count = m;
  if (num_thr > 0) {
    __syncthreads();
    for (int i = m + tid; i < P; i += DT_THREADS) keys[i] = DT_PAD;
    dt_bitonic(keys, P);                                       // descending fused score, ties by the order above
    count = min(m, num_thr);
    for (int pos = tid; pos < count; pos += DT_THREADS)
      dt_write(bx, fu, cand[(int)(unsigned)keys[pos]], ncls, dim, bottom, (long long)b * K + pos, out_boxes, out_scores, out_labels);
  }
  for (int pos = count + tid; pos < K; pos += DT_THREADS) {
    const long long o = (long long)b * K + pos;
    for (int k = 0; k < dim; ++k) out_boxes[o * dim + k] = 0.f;
    out_scores[o] = 0.f;
    out_labels[o] = 0;
  }
  if (tid == 0) out_count[b] = count;
}

// one wave: off[i] = count[0] + ... + count[i-1], off[batch] = the total
__global__ __launch_bounds__(64) void k_dt_offsets(const int* __restrict__ count, int batch, int* __restrict__ off) {
  const int lane = threadIdx.x;
  int carry = 0;
  for (int base = 0; base < batch; base += 64) {
    const int i = base + lane;
    const int v = i < batch ? count[i] : 0;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (i < batch) off[i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) off[batch] = carry;
}

static inline size_t dt_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int dt_k(int nq, int ncls, int max_num) {
  const long long n = (long long)nq * ncls;
  return (int)(n < max_num ? n : max_num);
}

extern "C" int64_t u3d_det_tail_workspace(int32_t batch, int32_t nq, int32_t num_classes, int32_t max_num, int32_t box_dim) {
  if (batch <= 0 || nq <= 0 || num_classes <= 0 || max_num <= 0 || (box_dim != 7 && box_dim != 9)) return -1;
  const size_t K = (size_t)dt_k(nq, num_classes, max_num), B = (size_t)batch;
  return (int64_t)(2 * dt_align(B * K * 4) + dt_align(B * 4) + dt_align(B * num_classes * 2 * 4) + dt_align(B * K * 5 * 4) +
                   dt_align(B * K));
}

extern "C" int32_t u3d_det_tail(const float* prob, const float* fused, const float* boxes, int32_t batch, int32_t nq, int32_t num_classes,
                                int32_t box_dim, int32_t max_num, const float* center_range, float score_threshold, int32_t mode,
                                float nms_thr, const float* score_thr, int32_t num_thr, float* out_boxes, float* out_scores,
                                int32_t* out_labels, int32_t* out_count, int32_t* out_off, void* workspace, int64_t workspace_bytes,
                                u3d_stream s) {
  U3D_REQUIRE(prob && fused && boxes && center_range && out_boxes && out_scores && out_labels && out_count && out_off && workspace &&
              batch > 0 && nq > 0 && num_classes > 0 && max_num > 0 && (box_dim == 7 || box_dim == 9) &&
              (mode == U3D_DET_TAIL_NONE || mode == U3D_DET_TAIL_NMS || mode == U3D_DET_TAIL_DECODE), U3D_ERR_ARG);
  U3D_REQUIRE((long long)nq * num_classes < (1ll << 31) && num_classes <= 65536 && batch <= 65535, U3D_ERR_UNSUPPORTED);
  const int K = dt_k(nq, num_classes, max_num);
  U3D_REQUIRE(K <= DT_MAX_K, U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE(workspace_bytes >= u3d_det_tail_workspace(batch, nq, num_classes, max_num, box_dim), U3D_ERR_WORKSPACE);
  int P = 1;
  while (P < K) P <<= 1;
  const size_t B = (size_t)batch;
  char* w = (char*)workspace;
  int* cand0 = (int*)w; w += dt_align(B * K * 4);
  int* cand = (int*)w; w += dt_align(B * K * 4);
  int* ncand = (int*)w; w += dt_align(B * 4);
  int* seg = (int*)w; w += dt_align(B * num_classes * 2 * 4);
  float* bev = (float*)w; w += dt_align(B * K * 5 * 4);
  unsigned char* keep = (unsigned char*)w;
  const int nms = mode == U3D_DET_TAIL_NMS;
  U3D_ALLOW_LDS(k_dt_select, DT_MAX_K * 8);
  U3D_ALLOW_LDS(k_dt_emit, DT_MAX_K * 8);
  hipLaunchKernelGGL(k_dt_select, dim3(batch), dim3(DT_THREADS), (size_t)P * 8, s, prob, fused, boxes, nq, num_classes, box_dim, K, P,
                     center_range, score_threshold, nms, cand0, cand, ncand, seg, bev);
  if (nms)
    hipLaunchKernelGGL(k_dt_nms, dim3(num_classes, batch), dim3(DT_NMS_THREADS), 0, s, bev, seg, num_classes, K, nms_thr, keep);
  hipLaunchKernelGGL(k_dt_emit, dim3(batch), dim3(DT_THREADS), num_thr > 0 ? (size_t)P * 8 : 0, s, fused, boxes, nq, num_classes, box_dim,
                     K, P, cand, ncand, nms ? keep : (const unsigned char*)nullptr, score_thr, num_thr, mode != U3D_DET_TAIL_DECODE ? 1 : 0,
                     out_boxes, out_scores, out_labels, out_count);
  hipLaunchKernelGGL(k_dt_offsets, dim3(1), dim3(64), 0, s, out_count, batch, out_off);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
