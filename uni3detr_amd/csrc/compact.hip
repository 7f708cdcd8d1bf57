// Stable compaction of fixed-size rows: out[pos[d]] = rec[d] where valid[d], with pos the exclusive scan of valid (the caller scans
// the flags).  Rows are row_bytes wide, a positive multiple of 4, and move as 32-bit words: one thread per word, so the KITTI records
// (16 x f32) and the nuScenes records (12 x f64) go through the same kernel bit for bit.
#include "common.h"

#define CR_THREADS 256

__global__ __launch_bounds__(CR_THREADS) void k_compact_rows(const unsigned int* __restrict__ rec, const int* __restrict__ valid,
                                                             const int* __restrict__ pos, int n, int row_words,
                                                             unsigned int* __restrict__ out) {
  const long long k = (long long)blockIdx.x * CR_THREADS + threadIdx.x;
  if (k >= (long long)n * row_words) return;
  const int d = (int)(k / row_words), c = (int)(k % row_words);
  if (valid[d]) out[(long long)pos[d] * row_words + c] = rec[k];
}

extern "C" int32_t u3d_compact_rows(const void* rec, const int32_t* valid, const int32_t* pos, int32_t n, int32_t row_bytes, void* out,
                                    u3d_stream s) {
  U3D_REQUIRE(n >= 0 && row_bytes > 0 && row_bytes % 4 == 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(rec && valid && pos && out, U3D_ERR_ARG);
  const int row_words = row_bytes / 4;
  hipLaunchKernelGGL(k_compact_rows, dim3(u3d_cdiv((long long)n * row_words, CR_THREADS)), dim3(CR_THREADS), 0, s,
                     (const unsigned int*)rec, valid, pos, n, row_words, (unsigned int*)out);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
