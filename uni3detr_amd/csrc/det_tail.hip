// The inference tail after the head's forward, for every scene of a batch in one call (u3d_det_tail / u3d_det_tail_pp): the selection of
// NMSFreeCoder.decode_single (ref: core/bbox/coders/nms_free_coder.py:42-100) and the post-processing of Uni3DETRHead.get_bboxes (ref:
// models/dense_heads/uni3detr_head.py:827-918) for post_processing None / 'nms' / 'soft_nms' / 'box_merging', bit for bit what the
// per-scene host loop gives.  The
// transcendental part (layer mean, sigmoid, denormalize_bbox, score fusion) stays in torch, batched; the kernels here only select,
// compare, move and run the rotated IoU:
//   k_dt_select  one workgroup per scene.  Key of a (query, class) entry = monotone-uint32(prob) in the high word (inverted), flat index
//                in the low word.  The k-th largest 32-bit score key by four 8-bit histogram passes (LDS counters), the winners - every key
//                above it and the first ties by ascending flat index - compacted with ballot + popcount, then a bitonic sort of the K
//                64-bit keys in LDS: descending score, ascending (query, class) index, the pinned order of decode_single.  The keep mask
//                (centre within center_range, prob > score_threshold) compacts that list stably -> the coder's output order.
//                NMS mode: the kept candidates are sorted once more by (label asc, fused score desc, compacted position asc) - the order
//                nms3d_classwise emits - their BEV rows (cx, cy, dx, dy, yaw) and the (scene, class) segments go to the workspace.
//                MERGE mode: the same order with 7-column bottom-centre rows, plus the compacted position of every row.  SOFT_NMS mode:
//                (label asc, compacted position asc) - u3d_soft_nms's member order, which its tie rule reads - and 7-column rows.
//   k_dt_nms     one workgroup per (scene, class) segment: greedy rotated-BEV NMS in that order with pp_iou_bev, the arithmetic of
//                bev_iou_rot (u3d_nms3d).  Suppression never crosses labels, so the greedy pass per segment equals the pass over the
//                whole score-sorted scene.  Segments of at most DT_LDS_CAP = 2048 candidates hold their BEV rows in LDS (40 KiB); larger
//                ones run the same loop on the rows in the workspace (no mask matrix: K <= 8192 rows stay in L2).
//   k_dt_soft    one workgroup per (scene, class) segment: the Gaussian soft-NMS loop of k_soft_nms (postproc.hip) with pp_iou3d and
//                pp_soft_decay; the current scores of up to 8192 members live in LDS (32 KiB), the rows too up to DT_LDS_CAP (56 KiB),
//                above that they are read from the workspace.  Selected members go, in selection order, to the front of the segment
//                (flat index, decayed score, keep = 1); the emit then reads them class-major.
//   k_dt_merge   one workgroup per (scene, class) segment: the greedy sweep of u3d_box_merge with pp_merge_overlap on the un-merged
//                rows.  Absorption never crosses labels and a segment is in scene-wide (score, position) order, so the sweep per
//                segment equals the sweep over the score-sorted scene.  A live row i marks every later live row it overlaps (the
//                reference's mask row & ~removed, without the mask matrix: kept rows x cnt overlap evaluations instead of cnt^2 / 2);
//                they are compacted in ascending order, i itself goes last - the member order of k_merge_median - and each of the
//                first 7 columns becomes the median by rank selection (ties by that position).  Flags, member list and one column of
//                values live in LDS for any segment size (8 + 16 + 32 KiB), the rows as in k_dt_soft.
//   k_dt_emit    one workgroup per scene: survivors with score > score_thr[label], stably compacted (the score is the fused one, in
//                SOFT_NMS mode the decayed one k_dt_soft left); MERGE mode sorts them by (fused score desc, compacted position asc),
//                the scene-wide order of the per-scene path, and takes columns 0-6 from the merged rows; with num_thr > 0 sorted by
//                (fused score desc, position asc) and cut - the per-scene path's torch.argsort(-scores) leaves ties open there, this is the
//                pin -; boxes gathered (z -= dz * 0.5 in two rounded f32 steps unless the caller asks for the coder's gravity centres),
//                rows past the count zeroed, count written.
//   k_dt_offsets out_off = exclusive scan of out_count (the det_off layout of u3d_eval_* / u3d_tta_merge).
//   k_dt_gate    u3d_det_gate, for a captured inference step: empties the scenes of a finished DetBatch that must not be read (a raised
//                validity flag, or a padded scene at or past *n_live) and writes the flag as an int32; k_dt_offsets then rewrites off.
// No atomics on global memory (LDS counters are integers: any order gives the same sum), so two runs give the same bytes.
// Limits: K = min(max_num, nq * num_classes) <= 8192, box_dim 7 or 9, nq * num_classes < 2^31, num_classes <= 65536, in every mode.
// Non-finite scores are outside the contract (torch orders NaN above everything; here a NaN orders by its bit pattern).
#include "common.h"
#include "box_iou.h"
#include "postproc_math.h"

#define DT_THREADS 1024
#define DT_WAVES (DT_THREADS / 64)
#define DT_MAX_K U3D_DET_TAIL_MAX_K
#define DT_LDS_CAP U3D_DET_TAIL_LDS_CAP
#define DT_NMS_THREADS 256
#define DT_PP_THREADS 256                  /* k_dt_soft, k_dt_merge */
#define DT_GATE_THREADS 256
#define DT_ORDER_SCORE 1                /* k_dt_select: label, fused score descending, compacted position */
#define DT_ORDER_POS 2                  /* label, compacted position */
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
template <int WAVES>
__device__ __forceinline__ int dt_scan_w(bool f, int* wsum, int* total) {
  const dt_u64 b = __ballot(f);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int in_wave = __popcll(b & ((1ull << lane) - 1ull));
  __syncthreads();                                             // the previous call's reads of wsum are over
  if (lane == 0) wsum[w] = __popcll(b);
  __syncthreads();
  int before = 0, tot = 0;
  for (int k = 0; k < WAVES; ++k) {
    const int v = wsum[k];
    if (k < w) before += v;
    tot += v;
  }
  *total = tot;
  return before + in_wave;
}
__device__ __forceinline__ int dt_scan(bool f, int* wsum, int* total) { return dt_scan_w<DT_WAVES>(f, wsum, total); }

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

// the two steps of get_bboxes' `boxes[:, 2] - boxes[:, 5] * 0.5`, each rounded to f32 (no contraction into one fused multiply-add)
__device__ __forceinline__ float dt_bottom_z(float z, float dz) {
#pragma clang fp contract(off)
  const float half = dz * 0.5f;
  return z - half;
}

// cand0 [B][K]: flat index by compacted position (NMS mode); cand [B][K]: flat index by final position of this kernel; ncand [B];
// seg [B][C][2] = (first, one past last) position of the class; rows [B][K][rowdim]: rowdim 5 = BEV (cx, cy, dx, dy, yaw), 7 = the
// bottom-centre box; cpos [B][K] (or null): compacted position by final position.  order: 0, DT_ORDER_SCORE or DT_ORDER_POS
__global__ __launch_bounds__(DT_THREADS) void k_dt_select(const float* __restrict__ prob, const float* __restrict__ fused,
                                                          const float* __restrict__ boxes, int nq, int ncls, int dim, int K, int P,
                                                          const float* __restrict__ range, float score_threshold, int order,
                                                          int rowdim, int* __restrict__ cand0, int* __restrict__ cand,
                                                          int* __restrict__ ncand, int* __restrict__ seg, float* __restrict__ rows,
                                                          int* __restrict__ cpos) {
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
  cand0 += (long long)b * K; cand += (long long)b * K; rows += (long long)b * K * rowdim; seg += (long long)b * ncls * 2;
  if (cpos) cpos += (long long)b * K;

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

  // ---- keep mask, stable compaction.  In the ordered modes the new key of compacted position j overwrites keys[j]: j <= the position read,
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
      if (order) {
        cand0[j] = idx;
        const dt_u64 sk = order == DT_ORDER_SCORE ? (dt_u64)(~dt_mono(fu[idx])) << DT_POS_BITS : 0ull;
        keys[j] = ((dt_u64)(unsigned)(idx % ncls) << (32 + DT_POS_BITS)) | sk | (unsigned)j;
      } else {
        cand[j] = idx;
      }
    }
    n += tot;
  }
  if (tid == 0) ncand[b] = n;
  if (!order) return;

  // ---- label ascending, then (DT_ORDER_SCORE) fused score descending, then compacted position ascending ----
  for (int c = tid; c < 2 * ncls; c += DT_THREADS) seg[c] = 0;
  __syncthreads();
  for (int i = n + tid; i < P; i += DT_THREADS) keys[i] = DT_PAD;
  dt_bitonic(keys, P);
  for (int r = tid; r < n; r += DT_THREADS) {
    const dt_u64 k = keys[r];
    const int j = (int)(k & ((1u << DT_POS_BITS) - 1u));
    const int idx = cand0[j];
    const int lab = (int)(k >> (32 + DT_POS_BITS));
    cand[r] = idx;
    if (cpos) cpos[r] = j;
    const float* c = bx + (long long)(idx / ncls) * dim;
    float* o = rows + (long long)r * rowdim;
    if (rowdim == 5) {
      o[0] = c[0]; o[1] = c[1]; o[2] = c[3]; o[3] = c[4]; o[4] = c[6];
    } else {
      o[0] = c[0]; o[1] = c[1]; o[2] = dt_bottom_z(c[2], c[5]); o[3] = c[3]; o[4] = c[4]; o[5] = c[5]; o[6] = c[6];
    }
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

// ---- SOFT_NMS: the loop of k_soft_nms over rows[0 .. cnt) (7 floats each, member k = compacted order), sc[] current scores in LDS ----
__device__ __forceinline__ int dt_soft_loop(const float* rows, int cnt, float sigma, float prune, float* sc, float* red_v, int* red_i,
                                            float* topbox, const int* __restrict__ cand, int* __restrict__ sel,
                                            float* __restrict__ sel_score) {
  const int tid = threadIdx.x;
  int n_sel = 0;
  while (true) {
    float bv = -1.f;
    int bi = 0x7fffffff;
    for (int k = tid; k < cnt; k += DT_PP_THREADS) {
      const float v = sc[k];
      if (v >= 0.f && (v > bv || (v == bv && k < bi))) { bv = v; bi = k; }
    }
    red_v[tid] = bv; red_i[tid] = bi;
    __syncthreads();
    for (int s = DT_PP_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const float v2 = red_v[tid + s];
        const int i2 = red_i[tid + s];
        if (v2 > red_v[tid] || (v2 == red_v[tid] && i2 < red_i[tid])) { red_v[tid] = v2; red_i[tid] = i2; }
      }
      __syncthreads();
    }
    const int top = red_i[0];
    if (top == 0x7fffffff) break;                              // nothing alive
    if (tid == 0) { sel[n_sel] = cand[top]; sel_score[n_sel] = red_v[0]; }
    if (tid < 7) topbox[tid] = rows[top * 7 + tid];
    __syncthreads();                                           // topbox is there; red_v[0] / red_i[0] are read
    for (int k = tid; k < cnt; k += DT_PP_THREADS) {
      float v = sc[k];
      if (v < 0.f) continue;
      v = pp_soft_decay(v, pp_iou3d(topbox, rows + k * 7), sigma);
      sc[k] = (k != top && v > prune) ? v : -1.f;
    }
    ++n_sel;
    __syncthreads();
  }
  return n_sel;
}

// sel [B][K] / sel_score [B][K]: the selected members of a segment, in selection order, at the segment's first positions;
// keep [B][K] = 1 there, 0 on the rest of the segment
__global__ __launch_bounds__(DT_PP_THREADS) void k_dt_soft(const float* __restrict__ rows7, const float* __restrict__ fused,
                                                           const int* __restrict__ cand, const int* __restrict__ seg, int nq, int ncls,
                                                           int K, float sigma, float prune, int* __restrict__ sel,
                                                           float* __restrict__ sel_score, unsigned char* __restrict__ keep) {
  __shared__ float sb[DT_LDS_CAP * 7];
  __shared__ float sc[DT_MAX_K];
  __shared__ float red_v[DT_PP_THREADS];
  __shared__ int red_i[DT_PP_THREADS];
  __shared__ float topbox[7];
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int start = seg[((long long)b * ncls + c) * 2], end = seg[((long long)b * ncls + c) * 2 + 1];
  const int cnt = end - start;
  if (cnt <= 0) return;
  const long long base = (long long)b * K + start;
  const float* rows = rows7 + base * 7;
  const float* fu = fused + (long long)b * nq * ncls;
  for (int r = t; r < cnt; r += DT_PP_THREADS) sc[r] = fu[cand[base + r]];
  int n_sel;
  if (cnt <= DT_LDS_CAP) {
    for (int r = t; r < cnt * 7; r += DT_PP_THREADS) sb[r] = rows[r];
    __syncthreads();
    n_sel = dt_soft_loop(sb, cnt, sigma, prune, sc, red_v, red_i, topbox, cand + base, sel + base, sel_score + base);
  } else {
    __syncthreads();
    n_sel = dt_soft_loop(rows, cnt, sigma, prune, sc, red_v, red_i, topbox, cand + base, sel + base, sel_score + base);
  }
  for (int r = t; r < cnt; r += DT_PP_THREADS) keep[base + r] = r < n_sel ? 1 : 0;
}

// ---- MERGE: greedy sweep over rows[0 .. cnt) (7 floats each, best first) with the medians; flag 0 live, 1 absorbed, 2 absorbed in
//      the running step.  merged: the segment's [cnt][7] output (rows of absorbed boxes are left unwritten: the emit skips them) ----
__device__ __forceinline__ void dt_merge_sweep(const float* rows, int cnt, float thr, unsigned char* flag, unsigned short* members,
                                               float* vals, float* med, int* wsum, int* lasthit, float* __restrict__ merged) {
  const int t = threadIdx.x;
  for (int i = 0; i < cnt; ++i) {
    __syncthreads();                                           // flag[i] is final; the previous step's reads of members / med are over
    if (flag[i]) continue;
    const float* bi = rows + i * 7;
    bool mine = false;
    for (int j = i + 1 + t; j < cnt; j += DT_PP_THREADS)
      if (!flag[j] && pp_merge_overlap(bi, rows + j * 7) > thr) { flag[j] = 2; mine = true; }
    if (mine) *lasthit = i;                                    // any writer writes the same value
    __syncthreads();
    if (*lasthit != i) {                                       // nothing absorbed: the median of one value
      if (t < 7) merged[i * 7 + t] = bi[t];
      continue;
    }
    int m = 0;
    for (int base = i + 1; base < cnt; base += DT_PP_THREADS) {   // the absorbed rows in ascending order
      const int j = base + t;
      const bool hit = j < cnt && flag[j] == 2;
      int tot;
      const int pos = m + dt_scan_w<DT_PP_THREADS / 64>(hit, wsum, &tot);
      if (hit) { flag[j] = 1; members[pos] = (unsigned short)j; }
      m += tot;
    }
    if (t == 0) members[m] = (unsigned short)i;                // itself last, as k_merge_median lists it
    ++m;
    for (int col = 0; col < 7; ++col) {
      __syncthreads();                                         // members are there; the previous column's reads of vals are over
      for (int a = t; a < m; a += DT_PP_THREADS) vals[a] = rows[(int)members[a] * 7 + col];
      __syncthreads();
      // rank selection: the element whose rank (ties by position) is (m-1)/2 and the one of rank m/2
      for (int a = t; a < m; a += DT_PP_THREADS) {
        const float va = vals[a];
        int rank = 0;
        for (int q = 0; q < m; ++q) {
          const float vq = vals[q];
          rank += (vq < va || (vq == va && q < a)) ? 1 : 0;
        }
        if (rank == (m - 1) / 2) med[col] = va;
        if (rank == m / 2) med[7 + col] = va;
      }
    }
    __syncthreads();
    if (t < 7) merged[i * 7 + t] = pp_median_of(med[t], med[7 + t], m);
  }
  __syncthreads();
}

__global__ __launch_bounds__(DT_PP_THREADS) void k_dt_merge(const float* __restrict__ rows7, const int* __restrict__ seg, int ncls, int K,
                                                            float thr, float* __restrict__ merged, unsigned char* __restrict__ keep) {
  __shared__ float sb[DT_LDS_CAP * 7];
  __shared__ float vals[DT_MAX_K];
  __shared__ unsigned short members[DT_MAX_K];
  __shared__ unsigned char flag[DT_MAX_K];
  __shared__ float med[14];
  __shared__ int wsum[DT_PP_THREADS / 64];
  __shared__ int lasthit;
  const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
  const int start = seg[((long long)b * ncls + c) * 2], end = seg[((long long)b * ncls + c) * 2 + 1];
  const int cnt = end - start;
  if (cnt <= 0) return;
  const long long base = (long long)b * K + start;
  const float* rows = rows7 + base * 7;
  for (int r = t; r < cnt; r += DT_PP_THREADS) flag[r] = 0;
  if (t == 0) lasthit = -1;
  if (cnt <= DT_LDS_CAP) {
    for (int r = t; r < cnt * 7; r += DT_PP_THREADS) sb[r] = rows[r];
    dt_merge_sweep(sb, cnt, thr, flag, members, vals, med, wsum, &lasthit, merged + base * 7);
  } else {
    dt_merge_sweep(rows, cnt, thr, flag, members, vals, med, wsum, &lasthit, merged + base * 7);
  }
  for (int r = t; r < cnt; r += DT_PP_THREADS) keep[base + r] = flag[r] ? 0 : 1;
}

// row: the first 7 columns from elsewhere (MERGE), or null
__device__ __forceinline__ void dt_write(const float* __restrict__ bx, float score, const float* __restrict__ row, int idx, int ncls,
                                         int dim, int bottom, long long o, float* __restrict__ out_boxes,
                                         float* __restrict__ out_scores, int* __restrict__ out_labels) {
  const float* c = bx + (long long)(idx / ncls) * dim;
  float* ob = out_boxes + o * dim;
  for (int k = 0; k < dim; ++k) ob[k] = (row && k < 7) ? row[k] : (k == 2 && bottom) ? dt_bottom_z(c[2], c[5]) : c[k];
  out_scores[o] = score;
  out_labels[o] = idx % ncls;
}

// score_over [B][K] (or null): the score of position r instead of fused[cand[r]]; row_over [B][K][7] (or null): its first 7 columns;
// tie [B][K] (or null): what orders equal scores before the position does; sort_all: sort even without num_thr

__global__ __launch_bounds__(DT_THREADS) void k_dt_emit(const float* __restrict__ fused, const float* __restrict__ boxes, int nq, int ncls,
                                                        int dim, int K, int P, const int* __restrict__ cand,
                                                        const int* __restrict__ ncand, const unsigned char* __restrict__ keep,
                                                        const float* __restrict__ score_thr, int num_thr, int bottom,
                                                        const float* __restrict__ score_over, const float* __restrict__ row_over,
                                                        const int* __restrict__ tie, int sort_all, float* __restrict__ out_boxes, float* __restrict__ out_scores,
                                                        int* __restrict__ out_labels, int* __restrict__ out_count) {
  extern __shared__ dt_u64 keys[];                             // [P] when sorting
  __shared__ int wsum[DT_WAVES];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int N = nq * ncls;
  const float* fu = fused + (long long)b * N;
  const float* bx = boxes + (long long)b * nq * dim;
  cand += (long long)b * K;
  const int n = ncand[b];
  const long long bk = (long long)b * K;
  const bool sorting = num_thr > 0 || sort_all;
  const unsigned rmask = (1u << DT_POS_BITS) - 1u;
  int m = 0;
  for (int base = 0; base < n; base += DT_THREADS) {
    const int r = base + tid;
    bool ok = r < n;
    int idx = 0;
    float sc = 0.f;
    if (ok) {
      idx = cand[r];
      if (keep) ok = keep[bk + r] != 0;
      if (ok) sc = score_over ? score_over[bk + r] : fu[idx];
      if (ok && score_thr) ok = sc > score_thr[idx % ncls];
    }
    int tot;
    const int pos = m + dt_scan(ok, wsum, &tot);
    if (ok) {
      if (sorting) keys[pos] = ((dt_u64)(~dt_mono(sc)) << 32) | ((unsigned)(tie ? tie[bk + r] : 0) << DT_POS_BITS) | (unsigned)r;
      else dt_write(bx, sc, row_over ? row_over + (bk + r) * 7 : nullptr, idx, ncls, dim, bottom, bk + pos, out_boxes, out_scores, out_labels);
    }
    m += tot;
  }
  int count = m;
  if (sorting) {
    __syncthreads();
    for (int i = m + tid; i < P; i += DT_THREADS) keys[i] = DT_PAD;
    dt_bitonic(keys, P);                                       // descending score, ties by `tie`, then by the order above
    if (num_thr > 0) count = min(m, num_thr);
    for (int pos = tid; pos < count; pos += DT_THREADS) {
      const int r = (int)((unsigned)keys[pos] & rmask);
      const int idx = cand[r];
      dt_write(bx, score_over ? score_over[bk + r] : fu[idx], row_over ? row_over + (bk + r) * 7 : nullptr, idx, ncls, dim, bottom,
               bk + pos, out_boxes, out_scores, out_labels);
    }
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

// u3d_det_gate, one workgroup per scene: a scene is dead when the flag is raised (any non-zero value, a NaN too) or it lies at or past
// *n_live.  A dead scene's rows [0, count[b]) are zeroed - the rows behind them are zero already (k_dt_emit) - and its count becomes 0,
// so a gated DetBatch keeps "rows past count[b] are zero".  Every thread reads count[b] before thread 0 rewrites it (the barrier).
__global__ __launch_bounds__(DT_GATE_THREADS) void k_dt_gate(const float* __restrict__ flag, const int* __restrict__ n_live, int K, int dim,
                                                             float* __restrict__ boxes, float* __restrict__ scores,
                                                             int* __restrict__ labels, int* __restrict__ count, int* __restrict__ valid) {
  const int b = blockIdx.x, tid = threadIdx.x;
  const bool ok = flag[0] == 0.f;
  if (b == 0 && tid == 0) valid[0] = ok ? 1 : 0;
  if (ok && b < n_live[0]) return;                             // uniform over the workgroup
  const int c = min(max(count[b], 0), K);
  __syncthreads();
  const long long bk = (long long)b * K;
  for (int i = tid; i < c * dim; i += DT_GATE_THREADS) boxes[bk * dim + i] = 0.f;
  for (int i = tid; i < c; i += DT_GATE_THREADS) {
    scores[bk + i] = 0.f;
    labels[bk + i] = 0;
  }
  if (tid == 0) count[b] = 0;
}

extern "C" int32_t u3d_det_gate(const float* flag, const int32_t* n_live, float* boxes, float* scores, int32_t* labels, int32_t* count,
                                int32_t* off, int32_t batch, int32_t max_num, int32_t box_dim, int32_t* valid, u3d_stream s) {
  U3D_REQUIRE(flag && n_live && boxes && scores && labels && count && off && valid && batch > 0 && max_num > 0 &&
              (box_dim == 7 || box_dim == 9), U3D_ERR_ARG);
  U3D_REQUIRE(batch <= 65535 && max_num <= DT_MAX_K, U3D_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(k_dt_gate, dim3(batch), dim3(DT_GATE_THREADS), 0, s, flag, n_live, max_num, box_dim, boxes, scores, labels, count, valid);
  hipLaunchKernelGGL(k_dt_offsets, dim3(1), dim3(64), 0, s, count, batch, off);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

static inline size_t dt_align(size_t b) { return (b + 255) & ~(size_t)255; }
static inline int dt_k(int nq, int ncls, int max_num) {
  const long long n = (long long)nq * ncls;
  return (int)(n < max_num ? n : max_num);
}

// the workspace, in order: cand0 | cand | ncand | seg | rows | keep, then SOFT_NMS: decayed scores; MERGE: merged rows | compacted positions
struct dt_ws { size_t cand0, cand, ncand, seg, rows, keep, f_aux, i_aux, total; };
static inline dt_ws dt_layout(size_t B, size_t K, size_t C, int mode) {
  const bool pp = mode == U3D_DET_TAIL_SOFT_NMS || mode == U3D_DET_TAIL_MERGE;
  dt_ws w;
  size_t o = 0;
  w.cand0 = o; o += dt_align(B * K * 4);
  w.cand = o; o += dt_align(B * K * 4);
  w.ncand = o; o += dt_align(B * 4);
  w.seg = o; o += dt_align(B * C * 2 * 4);
  w.rows = o; o += dt_align(B * K * (pp ? 7 : 5) * 4);
  w.keep = o; o += dt_align(B * K);
  w.f_aux = o;
  if (mode == U3D_DET_TAIL_SOFT_NMS) o += dt_align(B * K * 4);
  if (mode == U3D_DET_TAIL_MERGE) o += dt_align(B * K * 7 * 4);
  w.i_aux = o;
  if (mode == U3D_DET_TAIL_MERGE) o += dt_align(B * K * 4);
  w.total = o;
  return w;
}

extern "C" int64_t u3d_det_tail_pp_workspace(int32_t batch, int32_t nq, int32_t num_classes, int32_t max_num, int32_t box_dim, int32_t mode) {
  if (batch <= 0 || nq <= 0 || num_classes <= 0 || max_num <= 0 || (box_dim != 7 && box_dim != 9) || mode < U3D_DET_TAIL_NONE ||
      mode > U3D_DET_TAIL_MERGE)
    return -1;
  return (int64_t)dt_layout((size_t)batch, (size_t)dt_k(nq, num_classes, max_num), (size_t)num_classes, mode).total;
}

extern "C" int64_t u3d_det_tail_workspace(int32_t batch, int32_t nq, int32_t num_classes, int32_t max_num, int32_t box_dim) {
  return u3d_det_tail_pp_workspace(batch, nq, num_classes, max_num, box_dim, U3D_DET_TAIL_NMS);
}

extern "C" int32_t u3d_det_tail_pp(const float* prob, const float* fused, const float* boxes, int32_t batch, int32_t nq, int32_t num_classes,
                                   int32_t box_dim, int32_t max_num, const float* center_range, float score_threshold, int32_t mode,
                                   float nms_thr, const float* score_thr, int32_t num_thr, float soft_sigma, float soft_prune,
                                   float* out_boxes, float* out_scores, int32_t* out_labels, int32_t* out_count, int32_t* out_off,
                                   void* workspace, int64_t workspace_bytes, u3d_stream s) {
  U3D_REQUIRE(prob && fused && boxes && center_range && out_boxes && out_scores && out_labels && out_count && out_off && workspace &&
              batch > 0 && nq > 0 && num_classes > 0 && max_num > 0 && (box_dim == 7 || box_dim == 9) && mode >= U3D_DET_TAIL_NONE &&
              mode <= U3D_DET_TAIL_MERGE && (mode != U3D_DET_TAIL_SOFT_NMS || soft_sigma > 0.f), U3D_ERR_ARG);
  U3D_REQUIRE((long long)nq * num_classes < (1ll << 31) && num_classes <= 65536 && batch <= 65535, U3D_ERR_UNSUPPORTED);
  const int K = dt_k(nq, num_classes, max_num);
  U3D_REQUIRE(K <= DT_MAX_K, U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE(workspace_bytes >= u3d_det_tail_pp_workspace(batch, nq, num_classes, max_num, box_dim, mode), U3D_ERR_WORKSPACE);
  int P = 1;
  while (P < K) P <<= 1;
  const dt_ws l = dt_layout((size_t)batch, (size_t)K, (size_t)num_classes, mode);
  char* w = (char*)workspace;
  int* cand0 = (int*)(w + l.cand0);
  int* cand = (int*)(w + l.cand);
  int* ncand = (int*)(w + l.ncand);
  int* seg = (int*)(w + l.seg);
  float* rows = (float*)(w + l.rows);
  unsigned char* keep = (unsigned char*)(w + l.keep);
  float* f_aux = (float*)(w + l.f_aux);
  int* i_aux = (int*)(w + l.i_aux);
  const bool nms = mode == U3D_DET_TAIL_NMS, soft = mode == U3D_DET_TAIL_SOFT_NMS, merge = mode == U3D_DET_TAIL_MERGE;
  const int order = soft ? DT_ORDER_POS : (nms || merge) ? DT_ORDER_SCORE : 0;
  const bool sorting = num_thr > 0 || merge;
  U3D_ALLOW_LDS(k_dt_select, DT_MAX_K * 8);
  U3D_ALLOW_LDS(k_dt_emit, DT_MAX_K * 8);
  hipLaunchKernelGGL(k_dt_select, dim3(batch), dim3(DT_THREADS), (size_t)P * 8, s, prob, fused, boxes, nq, num_classes, box_dim, K, P,
                     center_range, score_threshold, order, (soft || merge) ? 7 : 5, cand0, cand, ncand, seg, rows,
                     merge ? i_aux : (int*)nullptr);
  if (nms)
    hipLaunchKernelGGL(k_dt_nms, dim3(num_classes, batch), dim3(DT_NMS_THREADS), 0, s, rows, seg, num_classes, K, nms_thr, keep);
  // SOFT_NMS: cand0 (the flat index by compacted position) has served k_dt_select; it now takes the selected members
  if (soft)
    hipLaunchKernelGGL(k_dt_soft, dim3(num_classes, batch), dim3(DT_PP_THREADS), 0, s, rows, fused, cand, seg, nq, num_classes, K,
                       soft_sigma, soft_prune, cand0, f_aux, keep);
  if (merge)
    hipLaunchKernelGGL(k_dt_merge, dim3(num_classes, batch), dim3(DT_PP_THREADS), 0, s, rows, seg, num_classes, K, nms_thr, f_aux, keep);
  hipLaunchKernelGGL(k_dt_emit, dim3(batch), dim3(DT_THREADS), sorting ? (size_t)P * 8 : 0, s, fused, boxes, nq, num_classes, box_dim, K, P,
                     soft ? cand0 : cand, ncand, order ? keep : (const unsigned char*)nullptr, score_thr, num_thr,
                     mode != U3D_DET_TAIL_DECODE ? 1 : 0, soft ? f_aux : (const float*)nullptr, merge ? f_aux : (const float*)nullptr,
                     merge ? i_aux : (const int*)nullptr, merge ? 1 : 0, out_boxes, out_scores, out_labels, out_count);
  hipLaunchKernelGGL(k_dt_offsets, dim3(1), dim3(64), 0, s, out_count, batch, out_off);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

extern "C" int32_t u3d_det_tail(const float* prob, const float* fused, const float* boxes, int32_t batch, int32_t nq, int32_t num_classes,
                                int32_t box_dim, int32_t max_num, const float* center_range, float score_threshold, int32_t mode,
                                float nms_thr, const float* score_thr, int32_t num_thr, float* out_boxes, float* out_scores,
                                int32_t* out_labels, int32_t* out_count, int32_t* out_off, void* workspace, int64_t workspace_bytes,
                                u3d_stream s) {
  U3D_REQUIRE(mode == U3D_DET_TAIL_NONE || mode == U3D_DET_TAIL_NMS || mode == U3D_DET_TAIL_DECODE, U3D_ERR_ARG);
  return u3d_det_tail_pp(prob, fused, boxes, batch, nq, num_classes, box_dim, max_num, center_range, score_threshold, mode, nms_thr,
                         score_thr, num_thr, 1.f, 0.f, out_boxes, out_scores, out_labels, out_count, out_off, workspace, workspace_bytes, s);
}
