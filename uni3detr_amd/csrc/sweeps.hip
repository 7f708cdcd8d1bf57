// LoadPointsFromMultiSweeps on the device (mmdet3d v1.0.0rc5, recalled; the contract is INTEGRATION.md section H): the key frame of
// every scene, then the chosen LiDAR sweeps (remove-close filtered, transformed into the key frame, time lag in column 4) or the
// padding copies of the key frame, packed scene after scene into one exactly packed output, then the use_dim column gather.
//
// The host reads the sweep files and makes the choice draw (uni3detr_amd/datapath.py read_sweeps); it builds one table of SEGMENTS
// (key frame, one sweep or one pad copy), scene-major, in output order, and uploads it with the raw rows.  Every segment is cut into
// chunks of U3D_SWEEPS_CHUNK rows, numbered globally in the same order (seg_chunk0: the first chunk of every segment):
//   k_sweeps_count  one workgroup per chunk: kept rows (ballot + popcount per wave)
//   k_sweeps_scan   one workgroup: exclusive scan of the chunk counts -> chunk bases, and scene_off from the scenes' first chunks
//   k_sweeps_write  one workgroup per chunk: the kept rows, transformed, at chunk base + rank within the chunk
// So the output offsets are computed on the device and nothing is read back.
//
// Arithmetic: upstream computes `xyz @ R.T` in float64 from the float32 rows and rounds once to float32, then `xyz += t` in float64,
// rounded again; the lag ts - sweep_ts is a float64 the host computes.  Restated with a fixed summation order (r0*x + r1*y) + r2*z and
// no contraction into fused multiply-adds, so the result is reproducible bit for bit by the NumPy restatement.
#include "common.h"

#pragma clang fp contract(off)

#define SW_CHUNK U3D_SWEEPS_CHUNK
#define SW_MAXF 8
#define SW_NPARAM U3D_SWEEPS_NPARAM
#define SW_SCAN_THREADS 1024

static_assert(SW_CHUNK == 256, "one row per thread of a 256-thread workgroup");

struct SwUseDim {
  int d[SW_MAXF];
};

// The row this thread handles in chunk c, its segment and whether it is kept.  Rows are read only when valid.
struct SwRow {
  int seg, kind, row;
  bool valid;
  const float* src;
};

__device__ __forceinline__ SwRow sw_row(const float* __restrict__ key, long long n_key, const float* __restrict__ raw, long long n_raw,
                                        int load_dim, const int* __restrict__ seg_tab, const int* __restrict__ seg_chunk0, int n_seg, int c,
                                        int t) {
  SwRow r;
  r.seg = u3d_segment_of(seg_chunk0, n_seg, c);
  const int* e = seg_tab + r.seg * U3D_SWEEPS_SEG_FIELDS;
  r.kind = e[0];
  const long long src0 = e[1];
  const int rows = e[2];
  r.row = (c - seg_chunk0[r.seg]) * SW_CHUNK + t;
  const long long g = src0 + r.row;
  const bool from_raw = r.kind == U3D_SWEEP_SEG_SWEEP;
  r.valid = r.row < rows && g < (from_raw ? n_raw : n_key);
  r.src = (from_raw ? raw : key) + g * load_dim;
  return r;
}

__device__ __forceinline__ bool sw_keep(const SwRow& r, int remove_close) {
  if (!r.valid) return false;
  if (r.kind == U3D_SWEEP_SEG_KEY || !remove_close) return true;
  // _remove_close(radius=1.0): drop |x| < 1 and |y| < 1, strict, on the raw coordinates
  return !(fabsf(r.src[0]) < 1.f && fabsf(r.src[1]) < 1.f);
}

__global__ __launch_bounds__(SW_CHUNK) void k_sweeps_count(const float* __restrict__ key, long long n_key, const float* __restrict__ raw,
                                                          long long n_raw, int load_dim, const int* __restrict__ seg_tab,
                                                          const int* __restrict__ seg_chunk0, int n_seg, int remove_close,
                                                          int* __restrict__ chunk_count) {
  __shared__ int wsum[SW_CHUNK / 64];
  const int c = blockIdx.x, t = threadIdx.x;
  const SwRow r = sw_row(key, n_key, raw, n_raw, load_dim, seg_tab, seg_chunk0, n_seg, c, t);
  const unsigned long long m = __ballot(sw_keep(r, remove_close));
  if ((t & 63) == 0) wsum[t >> 6] = __popcll(m);
  __syncthreads();
  if (t == 0) {
    int s = 0;
    for (int w = 0; w < SW_CHUNK / 64; ++w) s += wsum[w];
    chunk_count[c] = s;
  }
}

// Exclusive scan of n_chunks counts, 1024 at a time (wave scans by shuffles, then the 16 wave totals); the bases of the current tile
// stay in LDS so that every scene whose first chunk lies in it takes its offset from there (scene_chunk0[b] == n_chunks: the total).
__global__ __launch_bounds__(SW_SCAN_THREADS) void k_sweeps_scan(const int* __restrict__ chunk_count, int n_chunks,
                                                                const int* __restrict__ scene_chunk0, int batch, int* __restrict__ chunk_base,
                                                                int* __restrict__ scene_off) {
  __shared__ int wsum[SW_SCAN_THREADS / 64];
  __shared__ int tile_base[SW_SCAN_THREADS];
  __shared__ int carry_s;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  if (t == 0) carry_s = 0;
  __syncthreads();
  for (int k0 = 0; k0 < n_chunks; k0 += SW_SCAN_THREADS) {
    const int k = k0 + t;
    const int v = k < n_chunks ? chunk_count[k] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const int u = __shfl_up(inc, d, 64);
      if (lane >= d) inc += u;
    }
    if (lane == 63) wsum[wv] = inc;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < SW_SCAN_THREADS / 64; ++w) { const int s = wsum[w]; if (w < wv) before += s; total += s; }
    const int base = carry_s + before + inc - v;
    tile_base[t] = base;
    if (k < n_chunks) chunk_base[k] = base;
    __syncthreads();
    for (int b = t; b <= batch; b += SW_SCAN_THREADS) {
      const int c = scene_chunk0[b];
      if (c >= k0 && c < k0 + SW_SCAN_THREADS && c < n_chunks) scene_off[b] = tile_base[c - k0];
    }
    __syncthreads();
    if (t == 0) carry_s += total;
    __syncthreads();
  }
  for (int b = t; b <= batch; b += SW_SCAN_THREADS)
    if (scene_chunk0[b] >= n_chunks) scene_off[b] = carry_s;
}

__global__ __launch_bounds__(SW_CHUNK) void k_sweeps_write(const float* __restrict__ key, long long n_key, const float* __restrict__ raw,
                                                          long long n_raw, int load_dim, const int* __restrict__ seg_tab,
                                                          const double* __restrict__ seg_param, const int* __restrict__ seg_chunk0, int n_seg,
                                                          int remove_close, SwUseDim use, int n_use, const int* __restrict__ chunk_base,
                                                          long long out_cap, float* __restrict__ out) {
  __shared__ int wsum[SW_CHUNK / 64];
  const int c = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const SwRow r = sw_row(key, n_key, raw, n_raw, load_dim, seg_tab, seg_chunk0, n_seg, c, t);
  const bool keep = sw_keep(r, remove_close);
  const unsigned long long m = __ballot(keep);
  if (lane == 0) wsum[wv] = __popcll(m);
  __syncthreads();
  if (!keep) return;
  int before = 0;
  for (int w = 0; w < wv; ++w) before += wsum[w];
  const long long o = (long long)chunk_base[c] + before + __popcll(m & ((1ull << lane) - 1ull));
  if (o >= out_cap) return;
  float v[SW_MAXF];
#pragma unroll
  for (int f = 0; f < SW_MAXF; ++f) v[f] = f < load_dim ? r.src[f] : 0.f;
  if (r.kind == U3D_SWEEP_SEG_SWEEP) {
    const double* P = seg_param + (long long)r.seg * SW_NPARAM;     // R row-major [9], t [3], ts - sweep_ts
    const double x = v[0], y = v[1], z = v[2];
    const float rx = (float)((P[0] * x + P[1] * y) + P[2] * z);
    const float ry = (float)((P[3] * x + P[4] * y) + P[5] * z);
    const float rz = (float)((P[6] * x + P[7] * y) + P[8] * z);
    v[0] = (float)((double)rx + P[9]);
    v[1] = (float)((double)ry + P[10]);
    v[2] = (float)((double)rz + P[11]);
    v[4] = (float)P[12];
  } else {
    v[4] = 0.f;                                                      // the key frame's time column, pad copies included
  }
  float* dst = out + o * n_use;
#pragma unroll
  for (int k = 0; k < SW_MAXF; ++k) {
    if (k < n_use) {
      float x = 0.f;
#pragma unroll
      for (int f = 0; f < SW_MAXF; ++f) x = use.d[k] == f ? v[f] : x;  // a select chain, not a dynamically indexed register array
      dst[k] = x;
    }
  }
}

extern "C" int64_t u3d_sweeps_merge_workspace(int32_t n_chunks) {
  if (n_chunks < 0) return -1;
  return (int64_t)2 * ((((int64_t)n_chunks * 4) + 255) / 256 * 256) + 256;
}

extern "C" int32_t u3d_sweeps_merge(const float* key_points, int64_t n_key_rows, const float* raw, int64_t n_raw_rows, int32_t load_dim,
                                    const int32_t* seg_tab, const double* seg_param, int32_t n_seg, const int32_t* seg_chunk0,
                                    const int32_t* scene_chunk0, int32_t batch, int32_t n_chunks, const int32_t* use_dim, int32_t n_use,
                                    int32_t remove_close, void* workspace, int64_t workspace_bytes, float* out, int64_t out_rows,
                                    int32_t* out_scene_off, u3d_stream s) {
  U3D_REQUIRE(seg_tab && seg_param && seg_chunk0 && scene_chunk0 && use_dim && out_scene_off && batch > 0 && n_seg >= batch &&
                  n_chunks >= 0 && load_dim >= 5 && load_dim <= SW_MAXF && n_use >= 1 && n_use <= SW_MAXF && n_key_rows >= 0 &&
                  n_raw_rows >= 0 && out_rows >= 0,
              U3D_ERR_ARG);
  U3D_REQUIRE(n_chunks == 0 || (out && workspace && (key_points || n_key_rows == 0) && (raw || n_raw_rows == 0)), U3D_ERR_ARG);
  if (workspace_bytes < u3d_sweeps_merge_workspace(n_chunks)) return U3D_ERR_WORKSPACE;
  SwUseDim use;
  for (int k = 0; k < SW_MAXF; ++k) use.d[k] = -1;
  for (int k = 0; k < n_use; ++k) {
    U3D_REQUIRE(use_dim[k] >= 0 && use_dim[k] < load_dim, U3D_ERR_ARG);
    use.d[k] = use_dim[k];
  }
  char* ws = (char*)workspace;
  int* chunk_count = (int*)ws;
  int* chunk_base = (int*)(ws + ((((int64_t)n_chunks * 4) + 255) / 256 * 256));
  if (n_chunks > 0) {
    hipLaunchKernelGGL(k_sweeps_count, dim3(n_chunks), dim3(SW_CHUNK), 0, s, key_points, (long long)n_key_rows, raw, (long long)n_raw_rows,
                       load_dim, seg_tab, seg_chunk0, n_seg, remove_close, chunk_count);
    U3D_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(k_sweeps_scan, dim3(1), dim3(SW_SCAN_THREADS), 0, s, chunk_count, n_chunks, scene_chunk0, batch, chunk_base,
                     out_scene_off);
  U3D_CHECK_LAUNCH();
  if (n_chunks > 0) {
    hipLaunchKernelGGL(k_sweeps_write, dim3(n_chunks), dim3(SW_CHUNK), 0, s, key_points, (long long)n_key_rows, raw, (long long)n_raw_rows,
                       load_dim, seg_tab, seg_param, seg_chunk0, n_seg, remove_close, use, n_use, chunk_base, (long long)out_rows, out);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}
