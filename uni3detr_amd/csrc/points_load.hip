// LoadPointsFromFile and NormalizePointsColor on the device (mmdet3d v1.0.0rc5, RECALLED from its published behaviour: that version is
// not in the reference tree, parity with it is unpinned; the contract is INTEGRATION.md section P).  The host reads the files and
// uploads the raw rows [R, load_dim] of all scenes in one copy (uni3detr_amd/datapath.py read_points / pack_batch(raw=...)); here:
//   k_points_floor   shift_height: one workgroup per scene, the exact order statistics a = z_(i), b = z_(min(i + 1, n - 1)) of the
//                    scene's float32 z column by a radix select over order-preserving uint32 keys, then NumPy's `linear` percentile
//                    in float64 from the (i, g) the host computed, rounded once to float32
//   k_points_gather  one pass over the rows: the use_dim gather, height = z - floor32 inserted after the third selected column
//   k_points_color   (c - mean) / 255 in place over three colour columns
//
// The select: keys are the float bits made monotonic (sign flipped for positives, all bits for negatives; -0.0 is keyed as +0.0), so
// unsigned key order is float order and the selected key decodes to the selected value exactly.  Pass 0 reads the strided z column,
// flags NaN and stores the keys contiguously in the workspace; four 8-bit digit passes, high digit first, histogram the keys that share
// the prefix found so far in LDS (integer atomics only: the counts, and therefore every result, do not depend on arrival order).  The
// high digit of a room's z values is nearly constant, so equal digits are aggregated within the wave before the LDS atomic: the
// first active lane's digit is broadcast, its holders are counted by a ballot and leave with ONE add; after PL_LEADERS rounds the rest
// (digits that really are spread) add one by one.  The second statistic needs no second selection: one more pass counts the keys <= a
// and takes the smallest key > a; b = a when rank i + 1 still lies within the keys <= a (or i is the last rank), else that minimum.
//
// A NaN anywhere in a scene's z makes its floor NaN (np.percentile does the same) and with it every height of the scene.
#include "common.h"

#pragma clang fp contract(off)

#define PL_THREADS 1024
#define PL_WAVES (PL_THREADS / 64)
#define PL_BINS 256
#define PL_LEADERS 4
#define PL_UNROLL 4
#define PL_MAXF 8
#define PL_ROWS 256

struct PlUseDim {
  int d[PL_MAXF];
};

__device__ __forceinline__ unsigned pl_key(float z) {
  unsigned u = z == 0.f ? 0u : __float_as_uint(z);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float pl_value(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// hist[digit] += 1 for every lane with part set; the trip count is wave-uniform (ballots only)
__device__ __forceinline__ void pl_hist_add(unsigned* hist, bool part, unsigned digit, int lane) {
  unsigned long long rem = __ballot(part);
#pragma unroll 1
  for (int r = 0; r < PL_LEADERS && rem; ++r) {
    const int leader = __ffsll((long long)rem) - 1;
    const unsigned d = (unsigned)__builtin_amdgcn_readlane((int)digit, leader);       // leader is wave-uniform: no LDS round trip
    const unsigned long long m = __ballot(part && digit == d) & rem;
    if (lane == leader) atomicAdd(&hist[d], (unsigned)__popcll(m));
    rem &= ~m;
  }
  if ((rem >> lane) & 1ull) atomicAdd(&hist[digit], 1u);
}

__global__ __launch_bounds__(PL_THREADS) void k_points_floor(const float* __restrict__ raw, long long n_rows, int load_dim, int z_col,
                                                            const int* __restrict__ scene_off, const double* __restrict__ table,
                                                            unsigned* __restrict__ keys, float* __restrict__ floor_out) {
  __shared__ unsigned hist[PL_BINS];
  __shared__ unsigned wsum[PL_BINS / 64];
  __shared__ unsigned s_prefix, s_rank, s_nan, s_cle, s_min;
  const int b = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  long long r0 = scene_off[b], r1 = scene_off[b + 1];
  r0 = r0 < 0 ? 0 : r0;
  r1 = r1 > n_rows ? n_rows : r1;
  const long long n = r1 - r0;
  if (n <= 0) {                                     // an empty scene has no percentile (the host refuses it): NaN, nothing read
    if (t == 0) floor_out[b] = __uint_as_float(0x7fc00000u);
    return;
  }
  long long i = (long long)table[2 * b];
  i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
  const double g = table[2 * b + 1];
  unsigned* __restrict__ key = keys + r0;
  if (t < PL_BINS) hist[t] = 0u;
  if (t == 0) { s_prefix = 0u; s_rank = (unsigned)i; s_nan = 0u; s_cle = 0u; s_min = 0xffffffffu; }
  __syncthreads();

  for (int pass = 0; pass < 4; ++pass) {
    const int shift = 24 - 8 * pass;
    const unsigned prefix = s_prefix;
    bool nan = false;
    for (long long k0 = 0; k0 < n; k0 += PL_THREADS * PL_UNROLL) {
      unsigned kk[PL_UNROLL];
      bool valid[PL_UNROLL];
#pragma unroll
      for (int u = 0; u < PL_UNROLL; ++u) {           // the loads of one round are independent: issued together
        const long long k = k0 + u * PL_THREADS + t;
        valid[u] = k < n;
        kk[u] = 0u;
        if (valid[u]) {
          if (pass == 0) {
            const float z = raw[(r0 + k) * load_dim + z_col];
            nan |= z != z;
            kk[u] = pl_key(z);
            key[k] = kk[u];
          } else {
            kk[u] = key[k];
          }
        }
      }
#pragma unroll
      for (int u = 0; u < PL_UNROLL; ++u) {
        const bool part = valid[u] && (pass == 0 || (kk[u] >> (shift + 8)) == prefix);
        pl_hist_add(hist, part, (kk[u] >> shift) & 0xffu, lane);
      }
    }
    if (pass == 0 && __ballot(nan) != 0ull && lane == 0) atomicOr(&s_nan, 1u);
    __syncthreads();
    // exclusive scan of the 256 bins by the first four waves; the one bin that holds the rank becomes the next digit
    unsigned v = 0u, inc = 0u;
    const unsigned rank = s_rank;                   // read before the barrier below: the owner of the rank's bin rewrites it after
    if (t < PL_BINS) {
      v = hist[t];
      inc = v;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const unsigned u = (unsigned)__shfl_up((int)inc, d, 64);
        if (lane >= d) inc += u;
      }
      if (lane == 63) wsum[wv] = inc;
    }
    __syncthreads();
    if (t < PL_BINS) {
      unsigned before = 0u;
      for (int w = 0; w < wv; ++w) before += wsum[w];
      const unsigned excl = before + inc - v;
      hist[t] = 0u;
      if (v != 0u && excl <= rank && rank < excl + v) {       // exactly one thread: the bins partition the candidates
        s_prefix = (prefix << 8) | (unsigned)t;
        s_rank = rank - excl;
      }
    }
    __syncthreads();
  }

  const unsigned a_key = s_prefix;
  unsigned cle = 0u, mn = 0xffffffffu;
#pragma unroll 4
  for (long long k = t; k < n; k += PL_THREADS) {
    const unsigned kk = key[k];
    if (kk <= a_key) ++cle;
    else mn = kk < mn ? kk : mn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cle += (unsigned)__shfl_xor((int)cle, o, 64);
    const unsigned m2 = (unsigned)__shfl_xor((int)mn, o, 64);
    mn = m2 < mn ? m2 : mn;
  }
  if (lane == 0) {
    atomicAdd(&s_cle, cle);
    atomicMin(&s_min, mn);
  }
  __syncthreads();
  if (t == 0) {
    const bool same = i + 1 > n - 1 || (unsigned long long)(i + 1) < (unsigned long long)s_cle;
    const double a = (double)pl_value(a_key), bb = (double)pl_value(same ? a_key : s_min);
    const double d = bb - a;
    const double fl = g < 0.5 ? a + d * g : bb - d * (1.0 - g);
    floor_out[b] = s_nan ? __uint_as_float(0x7fc00000u) : (float)fl;
  }
}

__global__ __launch_bounds__(PL_ROWS) void k_points_gather(const float* __restrict__ raw, long long n_rows, int load_dim,
                                                          const int* __restrict__ scene_off, int batch, PlUseDim use, int n_use,
                                                          const float* __restrict__ floor_h, float* __restrict__ out) {
  const long long r = (long long)blockIdx.x * PL_ROWS + threadIdx.x;
  if (r >= n_rows) return;
  const float* __restrict__ src = raw + r * load_dim;
  float v[PL_MAXF];
#pragma unroll
  for (int f = 0; f < PL_MAXF; ++f) v[f] = f < load_dim ? src[f] : 0.f;
  const int feat = n_use + (floor_h ? 1 : 0);
  float* __restrict__ dst = out + r * feat;
  float z = 0.f;
#pragma unroll
  for (int k = 0; k < PL_MAXF; ++k) {
    if (k < n_use) {
      float x = 0.f;
#pragma unroll
      for (int f = 0; f < PL_MAXF; ++f) x = use.d[k] == f ? v[f] : x;      // a select chain, not a dynamically indexed register array
      if (k == 2) z = x;
      dst[floor_h && k >= 3 ? k + 1 : k] = x;
    }
  }
  if (floor_h) dst[3] = z - floor_h[u3d_segment_of(scene_off, batch, r)];
}

__global__ __launch_bounds__(PL_ROWS) void k_points_color(float* __restrict__ points, long long n_rows, int feat, int col0, float m0, float m1,
                                                         float m2) {
  const long long r = (long long)blockIdx.x * PL_ROWS + threadIdx.x;
  if (r >= n_rows) return;
  float* __restrict__ c = points + r * feat + col0;
  c[0] = (c[0] - m0) / 255.0f;
  c[1] = (c[1] - m1) / 255.0f;
  c[2] = (c[2] - m2) / 255.0f;
}

extern "C" int64_t u3d_points_load_workspace(int64_t n_rows, int32_t shift_height) {
  if (n_rows < 0) return -1;
  return shift_height ? (n_rows * 4 + 255) / 256 * 256 + 256 : 0;
}

extern "C" int32_t u3d_points_load(const float* raw, int64_t n_rows, int32_t load_dim, const int32_t* scene_off, int32_t batch,
                                   const double* load_table, const int32_t* use_dim, int32_t n_use, int32_t shift_height, void* workspace,
                                   int64_t workspace_bytes, float* out, float* floor_height, u3d_stream s) {
  U3D_REQUIRE(scene_off && use_dim && batch > 0 && n_rows >= 0 && n_rows < (1ll << 31) && load_dim >= 3 && load_dim <= PL_MAXF &&
                  n_use >= 1 && n_use + (shift_height ? 1 : 0) <= PL_MAXF,
              U3D_ERR_ARG);
  U3D_REQUIRE(!shift_height || (n_use >= 3 && load_table && floor_height), U3D_ERR_ARG);
  U3D_REQUIRE(n_rows == 0 || (raw && out && (!shift_height || workspace)), U3D_ERR_ARG);
  PlUseDim use;
  for (int k = 0; k < PL_MAXF; ++k) use.d[k] = -1;
  for (int k = 0; k < n_use; ++k) {
    U3D_REQUIRE(use_dim[k] >= 0 && use_dim[k] < load_dim, U3D_ERR_ARG);
    use.d[k] = use_dim[k];
  }
  if (workspace_bytes < u3d_points_load_workspace(n_rows, shift_height)) return U3D_ERR_WORKSPACE;
  if (shift_height) {
    hipLaunchKernelGGL(k_points_floor, dim3(batch), dim3(PL_THREADS), 0, s, raw, (long long)n_rows, load_dim, use.d[2], scene_off, load_table,
                       (unsigned*)workspace, floor_height);
    U3D_CHECK_LAUNCH();
  }
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_points_gather, dim3(u3d_cdiv(n_rows, PL_ROWS)), dim3(PL_ROWS), 0, s, raw, (long long)n_rows, load_dim, scene_off,
                       batch, use, n_use, shift_height ? floor_height : (const float*)nullptr, out);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}

extern "C" int32_t u3d_points_color_norm(float* points, int64_t n_rows, int32_t feat, int32_t col0, float mean0, float mean1, float mean2,
                                         u3d_stream s) {
  U3D_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && feat >= 3 && feat <= PL_MAXF && col0 >= 0 && col0 + 3 <= feat, U3D_ERR_ARG);
  U3D_REQUIRE(n_rows == 0 || points, U3D_ERR_ARG);
  if (n_rows > 0) {
    hipLaunchKernelGGL(k_points_color, dim3(u3d_cdiv(n_rows, PL_ROWS)), dim3(PL_ROWS), 0, s, points, (long long)n_rows, feat, col0, mean0, mean1,
                       mean2);
    U3D_CHECK_LAUNCH();
  }
  return U3D_OK;
}
