// A device-resident store for the detections of a whole dataset (u3d_det_store_append / _pack / _merge; include/u3d_hip.h states the
// semantics).  A finished DetBatch - the padded outputs of u3d_det_tail_pp behind u3d_det_gate - is appended stream-ordered, with no
// host read; the store keeps the scenes in dataset order and is packed once into the flat layout the evaluators consume.
//
// The store is caller-owned memory: rows (boxes [R, D], scores [R], labels [R]), table [S, 2] = (first row, count) per scene, cursor [4]
// = (scenes recorded, rows used, invalid calls, refused calls), invalid [M, 2] = (first scene, scenes) per invalid call.
//
//   k_ds_copy    append, launch 1.  grid (B, DS_SPLIT_MAX at most), one scene per blockIdx.x.  Every workgroup derives the plan of the call
//                from count / n_live / valid / scene_ids and the cursor (ds_plan: the clamped counts before its scene, their total, the
//                refusal) - O(B) reads of a few hundred bytes, B being a batch size - and copies its share of the scene's live rows as
//                flat runs of dwords, one dword per lane per step (a 7-column row is 28 bytes: no wider aligned unit exists).  It only
//                READS the cursor.
//   k_ds_commit  append, launch 2.  One wave.  The same plan again, then the table entries (an exclusive scan of the counts, 64 scenes per
//                step), the invalid record and the cursor.  It is the only writer of table / invalid / cursor, and stream order puts it
//                behind every read of k_ds_copy: no atomics, no scratch memory, and a refused call has written nothing.
//   k_ds_offsets pack, launch 1.  One wave: out_off = exclusive scan of the table's counts, bad[] zeroed.
//   k_ds_gather  pack, launch 2.  One workgroup per scene: its run of rows to out_off[scene], flat dword copies as above; a non-finite
//                score or a label outside [0, num_classes) stores 1 to bad[0] / bad[1] (every writer stores the same value).
//   k_dm_plan    merge, launch 1.  ONE workgroup: n_scenes is a dataset size, so the plan is made once and kept in the workspace - the
//                refusal (heads, map entries, cursor, capacities) and, 256 scenes per step, the exclusive scan of the mapped counts
//                (64-lane scans, the four wave totals through LDS).  It is the only reader of the cursor's first two entries.
//   k_dm_copy    merge, launch 2.  One workgroup per scene: its run of shard rows to the planned place, flat dword copies as above, and
//                its table entry; workgroup 0 writes the cursor (or counts the refusal).  The only writer of table / cursor.
// Nothing here reads a store row at or past the used rows, so the bytes written depend on the inputs alone.
#include "common.h"

#define DS_THREADS 256
#define DS_WAVES (DS_THREADS / 64)
#define DS_SPLIT_FLOATS 2048            /* k_ds_copy: one more workgroup per scene for every 2048 floats of K * D ... */
#define DS_SPLIT_MAX 32                 /* ... up to 32 */

struct ds_plan_t {
  int nl;            // scenes this call carries: n_live clamped to [0, B]
  int ok;            // valid[0] != 0 (or no valid)
  int before;        // rows of the scenes in front of scene b
  int total;         // rows of all nl scenes
  int refuse;        // the call writes nothing
  int cur_s, cur_r;  // cursor[0], cursor[1] as read
};

__device__ __forceinline__ int ds_clamp(int c, int K) { return min(max(c, 0), K); }

// Called by ALL threads of a workgroup of `waves` waves (red: 3 * waves ints of LDS).  b: the scene whose `before` is wanted.
template <int WAVES>
__device__ __forceinline__ ds_plan_t ds_plan(const int* __restrict__ count, int B, int K, const int* __restrict__ n_live,
                                             const int* __restrict__ valid, const int* __restrict__ scene_ids,
                                             const int* __restrict__ cursor, int R, int S, int b, int* red) {
  ds_plan_t p;
  p.nl = n_live ? min(max(n_live[0], 0), B) : B;
  p.ok = valid ? (valid[0] != 0) : 1;
  p.cur_s = cursor[0];
  p.cur_r = cursor[1];
  int before = 0, total = 0, bad_id = 0;
  for (int i = threadIdx.x; i < p.nl; i += WAVES * 64) {
    const int c = p.ok ? ds_clamp(count[i], K) : 0;
    total += c;
    if (i < b) before += c;
    if (scene_ids) {
      const int id = scene_ids[i];
      bad_id |= (id < 0 || id >= p.cur_s) ? 1 : 0;
    }
  }
  for (int d = 32; d > 0; d >>= 1) {
    before += __shfl_down(before, d, 64);
    total += __shfl_down(total, d, 64);
    bad_id |= __shfl_down(bad_id, d, 64);
  }
  if (WAVES > 1) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if (lane == 0) { red[w * 3] = before; red[w * 3 + 1] = total; red[w * 3 + 2] = bad_id; }
    __syncthreads();
    before = total = bad_id = 0;
    for (int k = 0; k < WAVES; ++k) { before += red[k * 3]; total += red[k * 3 + 1]; bad_id |= red[k * 3 + 2]; }
  } else {
    before = __shfl(before, 0, 64);
    total = __shfl(total, 0, 64);
    bad_id = __shfl(bad_id, 0, 64);
  }
  p.before = before;
  p.total = total;
  // a cursor outside the store (never produced here; the memory is the caller's) refuses as well: no index below is taken on trust
  const bool rows_over = p.cur_r < 0 || p.cur_s < 0 || p.cur_s > S || (long long)p.cur_r + total > (long long)R;
  if (scene_ids) p.refuse = (bad_id || rows_over || !p.ok) ? 1 : 0;          // a repair is never itself invalid
  else p.refuse = (rows_over || (long long)p.cur_s + p.nl > (long long)S) ? 1 : 0;
  return p;
}

__global__ __launch_bounds__(DS_THREADS) void k_ds_copy(const float* __restrict__ boxes, const float* __restrict__ scores,
                                                        const int* __restrict__ labels, const int* __restrict__ count, int B, int K, int D,
                                                        const int* __restrict__ n_live, const int* __restrict__ valid,
                                                        const int* __restrict__ scene_ids, const int* __restrict__ cursor, int R, int S,
                                                        float* __restrict__ st_boxes, float* __restrict__ st_scores,
                                                        int* __restrict__ st_labels) {
  __shared__ int red[3 * DS_WAVES];
  const int b = blockIdx.x;
  const ds_plan_t p = ds_plan<DS_WAVES>(count, B, K, n_live, valid, scene_ids, cursor, R, S, b, red);
  if (p.refuse || b >= p.nl || !p.ok) return;                        // uniform over the workgroup
  const int c = ds_clamp(count[b], K);
  const long long first = (long long)p.cur_r + p.before;             // first + c <= cur_r + total <= R: checked by the plan
  const long long src = (long long)b * K;
  const int step = gridDim.y * DS_THREADS, t0 = blockIdx.y * DS_THREADS + threadIdx.x;
  const float* sb = boxes + src * D;
  float* db = st_boxes + first * D;
  for (int i = t0; i < c * D; i += step) db[i] = sb[i];
  for (int i = t0; i < c; i += step) {
    st_scores[first + i] = scores[src + i];
    st_labels[first + i] = labels[src + i];
  }
}

__global__ __launch_bounds__(64) void k_ds_commit(const int* __restrict__ count, int B, int K, const int* __restrict__ n_live,
                                                  const int* __restrict__ valid, const int* __restrict__ scene_ids, int R, int S, int M,
                                                  int* __restrict__ table, int* __restrict__ cursor, int* __restrict__ invalid) {
  const int lane = threadIdx.x;
  const int n_inv = cursor[2], n_ref = cursor[3];
  const ds_plan_t p = ds_plan<1>(count, B, K, n_live, valid, scene_ids, cursor, R, S, 0, nullptr);
  if (p.refuse) {
    if (lane == 0) cursor[3] = n_ref + 1;
    return;
  }
  int carry = p.cur_r;
  for (int base = 0; base < p.nl; base += 64) {
    const int i = base + lane;
    const bool live = i < p.nl;
    const int v = (live && p.ok) ? ds_clamp(count[i], K) : 0;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    int scene = p.cur_s + i;
    bool write = live;
    if (scene_ids) {
      // a scene id named twice in one call: the last one wins - inside these 64 by the test below, across steps by program order
      const int id = live ? scene_ids[i] : -1;
      bool later = false;
      for (int j = 0; j < 64; ++j) {
        const int other = __shfl(id, j, 64);
        later |= (j > lane) && (base + j < p.nl) && (other == id);
      }
      scene = id;
      write = live && !later;
    }
    if (write) {
      table[2 * (long long)scene] = carry + incl - v;
      table[2 * (long long)scene + 1] = v;
    }
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) {
    if (!scene_ids) cursor[0] = p.cur_s + p.nl;
    cursor[1] = carry;
    if (!scene_ids && !p.ok && p.nl > 0) {
      if (n_inv < M) {
        invalid[2 * n_inv] = p.cur_s;
        invalid[2 * n_inv + 1] = p.nl;
      }
      cursor[2] = n_inv + 1;
    }
  }
}

extern "C" int32_t u3d_det_store_append(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int32_t batch,
                                        int32_t max_num, int32_t box_dim, const int32_t* n_live, const int32_t* valid,
                                        const int32_t* scene_ids, float* st_boxes, float* st_scores, int32_t* st_labels, int32_t* table,
                                        int32_t* cursor, int32_t* invalid, int32_t row_capacity, int32_t scene_capacity,
                                        int32_t invalid_capacity, u3d_stream s) {
  U3D_REQUIRE(boxes && scores && labels && count && st_boxes && st_scores && st_labels && table && cursor && batch > 0 && max_num > 0 &&
              (box_dim == 7 || box_dim == 9) && row_capacity > 0 && scene_capacity > 0 && invalid_capacity >= 0 &&
              (invalid || invalid_capacity == 0), U3D_ERR_ARG);
  U3D_REQUIRE(batch <= 65535 && max_num <= U3D_DET_TAIL_MAX_K && (long long)row_capacity * box_dim < (1ll << 31), U3D_ERR_UNSUPPORTED);
  const int split = min(DS_SPLIT_MAX, u3d_cdiv((long long)max_num * box_dim, DS_SPLIT_FLOATS));
  hipLaunchKernelGGL(k_ds_copy, dim3(batch, split), dim3(DS_THREADS), 0, s, boxes, scores, labels, count, batch, max_num, box_dim, n_live,
                     valid, scene_ids, cursor, row_capacity, scene_capacity, st_boxes, st_scores, st_labels);
  hipLaunchKernelGGL(k_ds_commit, dim3(1), dim3(64), 0, s, count, batch, max_num, n_live, valid, scene_ids, row_capacity, scene_capacity,
                     invalid_capacity, table, cursor, invalid);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// a table entry as the pack reads it: a run inside the store's rows, whatever the entry holds
__device__ __forceinline__ void ds_entry(const int* __restrict__ table, int scene, int R, int* first, int* cnt) {
  const int f = min(max(table[2 * (long long)scene], 0), R);
  *first = f;
  *cnt = min(max(table[2 * (long long)scene + 1], 0), R - f);
}

__global__ __launch_bounds__(64) void k_ds_offsets(const int* __restrict__ table, int n, int R, int* __restrict__ off, int* __restrict__ bad) {
  const int lane = threadIdx.x;
  if (lane < 2) bad[lane] = 0;
  int carry = 0;
  for (int base = 0; base < n; base += 64) {
    const int i = base + lane;
    int f, v = 0;
    if (i < n) ds_entry(table, i, R, &f, &v);
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (i < n) off[i] = carry + incl - v;
    carry += __shfl(incl, 63, 64);
  }
  if (lane == 0) off[n] = carry;
}

// rows whose place lies at or past out_rows are not written: the caller sees out_off[n_scenes] > out_rows
__global__ __launch_bounds__(DS_THREADS) void k_ds_gather(const float* __restrict__ st_boxes, const float* __restrict__ st_scores,
                                                          const int* __restrict__ st_labels, const int* __restrict__ table, int R, int D,
                                                          int ncls, const int* __restrict__ off, int out_rows, float* __restrict__ out_boxes,
                                                          float* __restrict__ out_scores, int* __restrict__ out_labels,
                                                          int* __restrict__ bad) {
  const int scene = blockIdx.x, tid = threadIdx.x;
  int first, c;
  ds_entry(table, scene, R, &first, &c);
  const int dst = off[scene];
  c = dst < 0 ? 0 : min(c, max(out_rows - dst, 0));
  const float* sb = st_boxes + (long long)first * D;
  float* ob = out_boxes + (long long)dst * D;
  for (int i = tid; i < c * D; i += DS_THREADS) ob[i] = sb[i];
  bool bad_score = false, bad_label = false;
  for (int i = tid; i < c; i += DS_THREADS) {
    const float sc = st_scores[first + i];
    const int lb = st_labels[first + i];
    out_scores[dst + i] = sc;
    out_labels[dst + i] = lb;
    bad_score |= (__float_as_uint(sc) & 0x7f800000u) == 0x7f800000u;          // Inf or NaN
    bad_label |= ncls > 0 && (lb < 0 || lb >= ncls);
  }
  if (bad_score) bad[0] = 1;
  if (bad_label) bad[1] = 1;
}

extern "C" int32_t u3d_det_store_pack(const float* st_boxes, const float* st_scores, const int32_t* st_labels, const int32_t* table,
                                      int32_t n_scenes, int32_t row_capacity, int32_t box_dim, int32_t num_classes, float* out_boxes,
                                      float* out_scores, int32_t* out_labels, int32_t out_rows, int32_t* out_off, int32_t* bad,
                                      u3d_stream s) {
  U3D_REQUIRE(st_boxes && st_scores && st_labels && table && out_boxes && out_scores && out_labels && out_off && bad && n_scenes >= 0 &&
              row_capacity > 0 && out_rows >= 0 && (box_dim == 7 || box_dim == 9), U3D_ERR_ARG);
  U3D_REQUIRE((long long)row_capacity * box_dim < (1ll << 31) && (long long)out_rows * box_dim < (1ll << 31), U3D_ERR_UNSUPPORTED);
  hipLaunchKernelGGL(k_ds_offsets, dim3(1), dim3(64), 0, s, table, n_scenes, row_capacity, out_off, bad);
  if (n_scenes > 0)
    hipLaunchKernelGGL(k_ds_gather, dim3(n_scenes), dim3(DS_THREADS), 0, s, st_boxes, st_scores, st_labels, table, row_capacity, box_dim,
                       num_classes, out_off, out_rows, out_boxes, out_scores, out_labels, bad);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---- merge: the shards of several ranks into one store ----------------------------------------------------------------------------
// workspace, int32: [0] refuse, [1] cursor[0] as read, [2] cursor[1] as read, [3] rows used after the call; then per mapped scene
// (first row in the store, count, first row in the flattened shards [W * Nmax])
#define DM_HEAD 4
#define DM_REC 3

__global__ __launch_bounds__(DS_THREADS) void k_dm_plan(const int* __restrict__ sh_off, const int* __restrict__ sh_head, int W, int Nmax,
                                                        int Smax, const int* __restrict__ map, int n, const int* __restrict__ cursor, int R,
                                                        int S, int* __restrict__ ws) {
  __shared__ long long wave_sum[DS_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cur_s = cursor[0], cur_r = cursor[1];
  int bad = 0;
  for (int w = tid; w < W; w += DS_THREADS) {
    const int hs = sh_head[2 * w], hr = sh_head[2 * w + 1];
    bad |= (hs < 0 || hs > Smax || hr < 0 || hr > Nmax) ? 1 : 0;
  }
  long long carry = cur_r;
  for (int base = 0; base < n; base += DS_THREADS) {                   // (uniform trip count: the barriers below are reached by all)
    const int i = base + tid;
    int cnt = 0, src = 0;
    if (i < n) {
      const int w = map[2 * (long long)i], l = map[2 * (long long)i + 1];
      bool ok = false;
      if (w >= 0 && w < W) {
        const int hs = sh_head[2 * w], hr = sh_head[2 * w + 1];
        if (hs >= 0 && hs <= Smax && hr >= 0 && hr <= Nmax && l >= 0 && l < hs) {      // no index below is taken on trust
          const int* off = sh_off + (long long)w * (Smax + 1) + l;
          const int a = min(max(off[0], 0), hr), b = min(max(off[1], 0), hr);
          cnt = max(b - a, 0);
          src = w * Nmax + a;                                          // + cnt <= (w + 1) * Nmax: inside shard w
          ok = true;
        }
      }
      bad |= ok ? 0 : 1;
    }
    long long incl = cnt;
    for (int d = 1; d < 64; d <<= 1) {
      const long long u = __shfl_up(incl, d, 64);
      if (lane >= d) incl += u;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    long long pre = 0, tot = 0;
    for (int k = 0; k < DS_WAVES; ++k) {
      const long long v = wave_sum[k];
      if (k < wave) pre += v;
      tot += v;
    }
    if (i < n) {
      int* rec = ws + DM_HEAD + DM_REC * (long long)i;
      rec[0] = (int)(carry + pre + incl - cnt);                        // meaningful when the call is not refused: then <= R
      rec[1] = cnt;
      rec[2] = src;
    }
    carry += tot;
    __syncthreads();
  }
  const int any_bad = __syncthreads_or(bad);
  if (tid == 0) {
    const bool outside = cur_s < 0 || cur_s > S || cur_r < 0;
    ws[0] = (any_bad || outside || (long long)cur_s + n > (long long)S || carry > (long long)R) ? 1 : 0;
    ws[1] = cur_s;
    ws[2] = cur_r;
    ws[3] = (int)carry;
  }
}

__global__ __launch_bounds__(DS_THREADS) void k_dm_copy(const float* __restrict__ sh_boxes, const float* __restrict__ sh_scores,
                                                        const int* __restrict__ sh_labels, int D, int n, const int* __restrict__ ws,
                                                        float* __restrict__ st_boxes, float* __restrict__ st_scores,
                                                        int* __restrict__ st_labels, int* __restrict__ table, int* __restrict__ cursor) {
  const int scene = blockIdx.x, tid = threadIdx.x;
  if (ws[0]) {                                                         // uniform over the grid
    if (scene == 0 && tid == 0) cursor[3] = cursor[3] + 1;
    return;
  }
  const int cur_s = ws[1];
  if (scene < n) {                                                     // (n == 0 still launches workgroup 0, for the cursor)
    const int* rec = ws + DM_HEAD + DM_REC * (long long)scene;
    const int dst = rec[0], c = rec[1], src = rec[2];                  // dst + c <= R, src + c inside its shard: checked by the plan
    const float* sb = sh_boxes + (long long)src * D;
    float* db = st_boxes + (long long)dst * D;
    for (int i = tid; i < c * D; i += DS_THREADS) db[i] = sb[i];
    for (int i = tid; i < c; i += DS_THREADS) {
      st_scores[dst + i] = sh_scores[src + i];
      st_labels[dst + i] = sh_labels[src + i];
    }
    if (tid == 0) {
      table[2 * ((long long)cur_s + scene)] = dst;                     // cur_s + n <= S: checked by the plan
      table[2 * ((long long)cur_s + scene) + 1] = c;
    }
  }
  if (scene == 0 && tid == 0) {
    cursor[0] = cur_s + n;
    cursor[1] = ws[3];
  }
}

extern "C" int64_t u3d_det_store_merge_workspace(int32_t n_scenes) {
  return 4ll * (DM_HEAD + DM_REC * (long long)max(n_scenes, 0));
}

extern "C" int32_t u3d_det_store_merge(const float* sh_boxes, const float* sh_scores, const int32_t* sh_labels, const int32_t* sh_off,
                                       const int32_t* sh_head, int32_t n_shards, int32_t shard_rows, int32_t shard_scenes, int32_t box_dim,
                                       const int32_t* scene_map, int32_t n_scenes, float* st_boxes, float* st_scores, int32_t* st_labels,
                                       int32_t* table, int32_t* cursor, int32_t* invalid, int32_t row_capacity, int32_t scene_capacity,
                                       int32_t invalid_capacity, void* workspace, int64_t workspace_bytes, u3d_stream s) {
  U3D_REQUIRE(sh_boxes && sh_scores && sh_labels && sh_off && sh_head && scene_map && st_boxes && st_scores && st_labels && table &&
              cursor && workspace && n_shards > 0 && shard_rows > 0 && shard_scenes >= 0 && n_scenes >= 0 && row_capacity > 0 &&
              scene_capacity > 0 && invalid_capacity >= 0 && (invalid || invalid_capacity == 0) && (box_dim == 7 || box_dim == 9),
              U3D_ERR_ARG);
  U3D_REQUIRE((long long)row_capacity * box_dim < (1ll << 31) && (long long)n_shards * shard_rows * box_dim < (1ll << 31),
              U3D_ERR_UNSUPPORTED);
  U3D_REQUIRE(workspace_bytes >= u3d_det_store_merge_workspace(n_scenes), U3D_ERR_WORKSPACE);
  int* ws = (int*)workspace;
  hipLaunchKernelGGL(k_dm_plan, dim3(1), dim3(DS_THREADS), 0, s, sh_off, sh_head, n_shards, shard_rows, shard_scenes, scene_map, n_scenes,
                     cursor, row_capacity, scene_capacity, ws);
  hipLaunchKernelGGL(k_dm_copy, dim3(max(n_scenes, 1)), dim3(DS_THREADS), 0, s, sh_boxes, sh_scores, sh_labels, box_dim, n_scenes, ws,
                     st_boxes, st_scores, st_labels, table, cursor);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
