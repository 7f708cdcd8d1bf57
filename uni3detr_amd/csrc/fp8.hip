// FP8 (OCP e4m3fn) inference of the wide dense convolutions: everything but the convolution itself (igemm_fp8.hip).
//
//   u3d_quant_rows_e4m3      bf16 rows -> e4m3 codes under one power-of-two scale (the activation pass in front of a convolution)
//   u3d_absmax_rows          running max |x| of bf16 rows into one f32 slot (calibration; no host sync)
//   u3d_bn_fold_fp8_batched  conv weight x eval-mode BatchNorm scale -> e4m3 codes + one exponent per output channel + the f32 shift
//
// All scales are powers of two: x * 2^-e is exact in f32 until it leaves the normal range, a code times its scale is an exact bf16
// number, and a floating-point format loses no relative precision to such a scale (only the subnormal floor moves).  The quantiser
// is fp8_quant.h: saturating, round to nearest even, NaN stays NaN.  Nothing here allocates or synchronises.
#include "common.h"
#include "fp8_quant.h"

typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// bf16 rows -> e4m3 rows.  Memory bound: 16-byte loads (8 bf16), 8-byte stores.  Rows at or past *n_dev are not written.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_quant_rows_e4m3(const u32x4* __restrict__ x, u32x2* __restrict__ q, const int* __restrict__ n_dev,
                                                         int n_cap, int c8, const int* __restrict__ e_dev) {
  const long long nvec = (long long)min(max(*n_dev, 0), n_cap) * c8;
  const int e = -*e_dev;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const u32x4 v = x[i];
    u32x2 o;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      unsigned w = 0;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned pair = v[h * 2 + (j >> 1)];
        const float f = __uint_as_float((j & 1) ? (pair & 0xffff0000u) : (pair << 16));
        w |= u3d_e4m3_from_f32(ldexpf(f, e)) << (8 * j);
      }
      o[h] = w;
    }
    q[i] = o;
  }
}

extern "C" int32_t u3d_quant_rows_e4m3(const void* x, void* q, const int32_t* n_dev, int32_t n_cap, int32_t c, const int32_t* e_dev,
                                       u3d_stream s) {
  U3D_REQUIRE(x && q && n_dev && e_dev && c > 0, U3D_ERR_ARG);
  if (c % 8 != 0) return U3D_ERR_UNSUPPORTED;
  if (n_cap <= 0) return U3D_OK;
  const long long nvec = (long long)n_cap * (c / 8);
  const int blocks = nvec < 256LL * 4096 ? u3d_cdiv(nvec, 256) : 4096;
  hipLaunchKernelGGL(k_quant_rows_e4m3, dim3(blocks), dim3(256), 0, (hipStream_t)s, (const u32x4*)x, (u32x2*)q, n_dev, n_cap, c / 8, e_dev);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------
// slot = max(slot, max |x|) over the first *n_dev rows.  |x| of a bf16 is its low 15 bits, and non-negative floats order as their
// bit patterns do: the maximum is an unsigned integer atomicMax on the f32 pattern - exact and independent of the order in which the
// workgroups arrive.  A NaN or Inf input leaves +Inf.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_absmax_rows(const u32x4* __restrict__ x, const int* __restrict__ n_dev, int n_cap, int c8,
                                                     unsigned* __restrict__ slot) {
  __shared__ unsigned red[4];
  const long long nvec = (long long)min(max(*n_dev, 0), n_cap) * c8;
  unsigned m = 0;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (long long)gridDim.x * 256) {
    const u32x4 v = x[i];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      m = max(m, v[j] & 0x7fffu);
      m = max(m, (v[j] >> 16) & 0x7fffu);
    }
  }
  m = min(m, 0x7f80u);                                    // NaN patterns lie above Inf's
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
    m = max(max(red[0], red[1]), max(red[2], red[3]));
    if (m) atomicMax(slot, m << 16);
  }
}

extern "C" int32_t u3d_absmax_rows(const void* x, const int32_t* n_dev, int32_t n_cap, int32_t c, float* slot, u3d_stream s) {
  U3D_REQUIRE(x && n_dev && slot && c > 0, U3D_ERR_ARG);
  if (c % 8 != 0) return U3D_ERR_UNSUPPORTED;
  if (n_cap <= 0) return U3D_OK;
  const long long nvec = (long long)n_cap * (c / 8);
  const int blocks = nvec < 256LL * 2048 ? u3d_cdiv(nvec, 256) : 2048;
  hipLaunchKernelGGL(k_absmax_rows, dim3(blocks), dim3(256), 0, (hipStream_t)s, (const u32x4*)x, n_dev, n_cap, c / 8, (unsigned*)slot);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------
// Weight fold.  One workgroup per (pair, output channel): the channel's exponent needs max |w * scale| over all offsets and input
// channels first, so the workgroup walks its kvol * cin elements twice (the second time out of L2).  The f32 product is
// u3d_bn_fold_batched's, and the code is rounded from it once - not from the bf16 copy.
// ---------------------------------------------------------------------------------------------
// (the job record: u3d_bn_fold_fp8_job, include/u3d_hip.h)

__global__ __launch_bounds__(256) void k_bn_fold_fp8_batched(const u3d_bn_fold_fp8_job* __restrict__ jobs, int njobs) {
  __shared__ unsigned red[4];
  int lo = 0, hi = njobs;                               // the job of this block: last j with first_block[j] <= blockIdx.x
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const u3d_bn_fold_fp8_job jb = jobs[lo];
  const int co = (int)blockIdx.x - jb.first_block;
  if (co >= jb.cout) return;
  const float scale = jb.gamma[co] / sqrtf(jb.var[co] + jb.eps);
  const float* src = jb.w + co * jb.sa;
  const int n = jb.kvol * jb.cin;
  unsigned m = 0;                                       // max |w * scale| as a bit pattern
  for (int i = threadIdx.x; i < n; i += 256) {
    const int k = i / jb.cin, ci = i - k * jb.cin;
    m = max(m, __float_as_uint(src[k * jb.sk + ci * jb.sb] * scale) & 0x7fffffffu);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
  __syncthreads();
  m = max(max(red[0], red[1]), max(red[2], red[3]));
  int e = 0;
  if (m != 0 && m < 0x7f800000u) {                      // max = mant * 2^x, mant in [0.5, 1); 448 = 0.875 * 2^9
    int x;
    const float mant = frexpf(__uint_as_float(m), &x);
    e = mant <= 0.875f ? x - 9 : x - 8;
  }
  if (threadIdx.x == 0) {
    jb.e_w[co] = e;
    jb.shift[co] = jb.beta[co] - jb.mean[co] * scale;
  }
  unsigned char* dst = jb.qw + (long long)co * jb.cin;
  for (int i = threadIdx.x; i < n; i += 256) {
    const int k = i / jb.cin, ci = i - k * jb.cin;
    const float v = src[k * jb.sk + ci * jb.sb] * scale;
    dst[(long long)k * jb.cout * jb.cin + ci] = (unsigned char)u3d_e4m3_from_f32(ldexpf(v, -e));
  }
}

extern "C" int64_t u3d_bn_fold_fp8_job_bytes(void) { return (int64_t)sizeof(u3d_bn_fold_fp8_job); }
// jobs: DEVICE array of njobs u3d_bn_fold_fp8_job records, first_block ascending from 0; total_blocks = the sum of cout over all jobs.
extern "C" int32_t u3d_bn_fold_fp8_batched(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s) {
  U3D_REQUIRE(jobs && njobs > 0 && total_blocks > 0, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_bn_fold_fp8_batched, dim3(total_blocks), dim3(256), 0, (hipStream_t)s, (const u3d_bn_fold_fp8_job*)jobs, njobs);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
