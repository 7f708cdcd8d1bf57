// Operand preparation and gradient sum of the split-bf16 convolutions (u3d_igemm_fwd_split_bf16, igemm_bf16.hip): an f32 tensor x is
// held as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi), and x.w ~ hi.wh + hi.wl + lo.wh.
#include "igemm_common.h"

// hi / lo bf16 planes of an f32 row matrix: dst[r] = bf16(x[r]), dst[n_cap + r] = bf16(x[r] - dst[r]) (round to nearest even both)
__global__ __launch_bounds__(256) void k_split_rows_f32(const float* __restrict__ x, const int* __restrict__ n_dev, int n_cap, int c,
                                                        u16* __restrict__ dst) {
  // rows past the device-side count (capacity padding of a captured step) become ZERO rows of both planes: a table entry can then
  // never pick up a stale NaN pattern, whatever it names
  const long long n = (long long)min(*n_dev, n_cap) * c / 4, plane = (long long)n_cap * c, ncap = plane / 4;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < ncap; i += (long long)gridDim.x * 256) {
    const f32x4 v = i < n ? *(const f32x4*)(x + i * 4) : (f32x4){0.f, 0.f, 0.f, 0.f};
    const bf16x4 h = __builtin_convertvector(v, bf16x4);
    const bf16x4 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x4), bf16x4);
    *(bf16x4*)(dst + i * 4) = h;
    *(bf16x4*)(dst + plane + i * 4) = l;
  }
}
extern "C" int32_t u3d_split_rows_f32(const float* x, const int32_t* n_dev, int32_t n_cap, int32_t c, void* dst, u3d_stream s) {
  U3D_REQUIRE(x && n_dev && dst && c > 0 && c % 4 == 0, U3D_ERR_ARG);
  if (n_cap <= 0) return U3D_OK;
  const long long n4 = (long long)n_cap * c / 4;
  const int blocks = (int)(n4 / 256 + 1 < 4096 ? n4 / 256 + 1 : 4096);
  hipLaunchKernelGGL(k_split_rows_f32, dim3(blocks), dim3(256), 0, s, x, n_dev, n_cap, c, (u16*)dst);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// the weight side of a split-bf16 product: dst bf16 [3][K][A][B] = (hi, lo, hi) of src[k * sk + a * sa + b * sb] (f32, any layout:
// the checkpoint layouts [kD,kH,kW,Cin,Cout] / [Cout,Cin,kD,kH,kW] are read in place, no re-laid-out f32 copy in between)
__global__ __launch_bounds__(256) void k_split3_weights(const float* __restrict__ src, long long sk, long long sa, long long sb, int K, int A,
                                                        int B, u16* __restrict__ dst) {
  const long long n = (long long)K * A * B;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const int b = (int)(i % B), a = (int)((i / B) % A), k = (int)(i / ((long long)A * B));
    const float v = src[k * sk + a * sa + b * sb];
    const u16 h = f2bf(v);
    const u16 l = f2bf(v - __uint_as_float((unsigned)h << 16));
    dst[i] = h; dst[n + i] = l; dst[2 * n + i] = h;
  }
}
extern "C" int32_t u3d_split3_weights(const float* src, int64_t sk, int64_t sa, int64_t sb, int32_t k, int32_t a, int32_t b, void* dst,
                                      u3d_stream s) {
  U3D_REQUIRE(src && dst && k > 0 && a > 0 && b > 0, U3D_ERR_ARG);
  const long long n = (long long)k * a * b;
  const int blocks = (int)(n / 256 + 1 < 2048 ? n / 256 + 1 : 2048);
  hipLaunchKernelGGL(k_split3_weights, dim3(blocks), dim3(256), 0, s, src, (long long)sk, (long long)sa, (long long)sb, k, a, b, (u16*)dst);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// All weight splits of a step in ONE launch (a `parity` step made 88 launches of k_split3_weights, ~6.6 us each whatever the size):
// jobs[j] (u3d_split3_job, include/u3d_hip.h) describes one (parameter, layout) pair, blocks [first_block[j], first_block[j + 1]) of the grid work on it.
#define SPLIT3_EPB 2048          /* elements per block */
__global__ __launch_bounds__(256) void k_split3_weights_batch(const u3d_split3_job* __restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs;                               // the job this block belongs to: last j with first_block[j] <= blockIdx.x
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const u3d_split3_job jb = jobs[lo];
  const long long n = (long long)jb.K * jb.A * jb.B;
  const long long i0 = (long long)((int)blockIdx.x - jb.first_block) * SPLIT3_EPB;
  for (long long i = i0 + threadIdx.x; i < i0 + SPLIT3_EPB && i < n; i += 256) {
    const int b = (int)(i % jb.B), a = (int)((i / jb.B) % jb.A), k = (int)(i / ((long long)jb.A * jb.B));
    const float v = jb.src[k * jb.sk + a * jb.sa + b * jb.sb];
    const u16 h = f2bf(v);
    const u16 l = f2bf(v - __uint_as_float((unsigned)h << 16));
    jb.dst[i] = h; jb.dst[n + i] = l; jb.dst[2 * n + i] = h;
  }
}
// hi / lo planes of up to 32 (possibly strided) f32 row matrices in ONE launch (the decoder's parameter-gradient operands in `parity`
// mode: ~30 tensors of 7 200 rows per layer, each of which was a copy + a u3d_split_rows_f32 launch of ~6 us).  The job list travels
// BY VALUE in the kernel arguments: the sources are slots of per-step workspaces, so nothing about it can be uploaded ahead of time.
// (U3dSplitRowsJobs: include/u3d_hip.h - row r of job j starts at src[j] + r * ld[j]; dst[j] bf16 [2 * rows[j]][cols[j]], hi plane then lo
//  plane; blocks [first_block[j], first_block[j + 1]) work on job j, 1024 elements per block)
__global__ __launch_bounds__(256) void k_split_rows_batch(const U3dSplitRowsJobs jb) {
  int j = 0;
  while (j + 1 < jb.njobs && jb.first_block[j + 1] <= (int)blockIdx.x) ++j;
  const int cols = jb.cols[j], c4 = cols >> 2;
  const long long n4 = (long long)jb.rows[j] * c4, plane = (long long)jb.rows[j] * cols;
  const long long i = (long long)((int)blockIdx.x - jb.first_block[j]) * 256 + threadIdx.x;
  if (i >= n4) return;
  const int r = (int)(i / c4), c = (int)(i % c4) * 4;
  const f32x4 v = *(const f32x4*)(jb.src[j] + (long long)r * jb.ld[j] + c);
  const bf16x4 h = __builtin_convertvector(v, bf16x4);
  const bf16x4 l = __builtin_convertvector(v - __builtin_convertvector(h, f32x4), bf16x4);
  u16* d = (u16*)jb.dst[j] + (long long)r * cols + c;
  *(bf16x4*)d = h;
  *(bf16x4*)(d + plane) = l;
}
// jobs->first_block is filled here (cols % 4 == 0, 16-byte aligned rows); njobs <= 32
extern "C" int32_t u3d_split_rows_batch(const U3dSplitRowsJobs* jobs, u3d_stream s) {
  U3D_REQUIRE(jobs && jobs->njobs > 0 && jobs->njobs <= 32, U3D_ERR_ARG);
  U3dSplitRowsJobs jb = *jobs;
  int fb = 0;
  for (int j = 0; j < jb.njobs; ++j) {
    U3D_REQUIRE(jb.src[j] && jb.dst[j] && jb.cols[j] > 0 && jb.cols[j] % 4 == 0 && jb.ld[j] % 4 == 0 && jb.rows[j] >= 0, U3D_ERR_ARG);
    jb.first_block[j] = fb;
    fb += (int)(((long long)jb.rows[j] * (jb.cols[j] / 4) + 255) / 256);
  }
  jb.first_block[jb.njobs] = fb;
  if (fb == 0) return U3D_OK;
  hipLaunchKernelGGL(k_split_rows_batch, dim3(fb), dim3(256), 0, s, jb);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
// dW of a split-bf16 product = the sum of its three bf16 products' f32 weight gradients (x^T dy ~ xh^T dyh + xl^T dyh + xh^T dyl):
// one pass instead of two element-wise additions
__global__ __launch_bounds__(256) void k_sum3_f32(const float* __restrict__ a, const float* __restrict__ b, const float* __restrict__ c,
                                                  float* __restrict__ out, long long n4) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256)
    *(f32x4*)(out + i * 4) = (*(const f32x4*)(a + i * 4) + *(const f32x4*)(b + i * 4)) + *(const f32x4*)(c + i * 4);
}
extern "C" int32_t u3d_sum3_f32(const float* a, const float* b, const float* c, float* out, int64_t n, u3d_stream s) {
  U3D_REQUIRE(a && b && c && out && n >= 0 && n % 4 == 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  const long long n4 = n / 4;
  hipLaunchKernelGGL(k_sum3_f32, dim3((int)(n4 / 256 + 1 < 2048 ? n4 / 256 + 1 : 2048)), dim3(256), 0, s, a, b, c, out, n4);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
extern "C" int64_t u3d_split3_job_bytes(void) { return (int64_t)sizeof(u3d_split3_job); }
extern "C" int32_t u3d_split3_job_blocks(int32_t k, int32_t a, int32_t b) {
  const long long n = (long long)k * a * b;
  return (int32_t)((n + SPLIT3_EPB - 1) / SPLIT3_EPB);
}
// jobs: DEVICE array of njobs u3d_split3_job records, first_block ascending from 0; total_blocks = sum of u3d_split3_job_blocks over the jobs
extern "C" int32_t u3d_split3_weights_batch(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s) {
  U3D_REQUIRE(jobs && njobs > 0 && total_blocks > 0, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_split3_weights_batch, dim3(total_blocks), dim3(256), 0, s, (const u3d_split3_job*)jobs, njobs);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
