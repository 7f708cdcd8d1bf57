// Eval-mode BatchNorm folded into the convolution in front of it (inference only).
//
// In eval mode BatchNorm is the per-channel affine map y = x * scale + shift with scale = gamma / sqrt(running_var + eps) and
// shift = beta - running_mean * scale.  The scale goes into the weights, the shift into the per-column f32 bias that the epilogue of
// the LDS-DMA implicit-GEMM kernels already adds (glds_epilogue.inc, u3d_igemm_fwd_affine_bf16): conv -> BatchNorm -> ReLU becomes one
// launch and one trip over the activation tensor.
//
// One launch folds every conv + BatchNorm pair of a model: the job table lives on the device (as u3d_split3_job does for the split-bf16
// weights, split_bf16.hip), blocks [first_block[j], first_block[j + 1]) of the grid work on job j.  The f32 master weight is read in
// place through element strides, so both checkpoint layouts ([kD,kH,kW,Cin,Cout] and [Cout,Cin,kD,kH,kW]) need no re-laid-out copy.
// Nothing here allocates or synchronises.
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

#define BNFOLD_EPB 2048          /* elements per block: 256 threads x 4 consecutive input channels x 2 */

__global__ __launch_bounds__(256) void k_bn_fold_batched(const u3d_bn_fold_job* __restrict__ jobs, int njobs) {
  int lo = 0, hi = njobs;                               // the job of this block: last j with first_block[j] <= blockIdx.x
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (jobs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const u3d_bn_fold_job jb = jobs[lo];
  const int blk = (int)blockIdx.x - jb.first_block;
  if (blk == 0 && !jb.scale_only)                       // the job's first block also leaves the shift
    for (int c = threadIdx.x; c < jb.cout; c += 256) {
      const float scale = jb.gamma[c] / sqrtf(jb.var[c] + jb.eps);
      jb.shift[c] = jb.beta[c] - jb.mean[c] * scale;
    }
  const long long n = (long long)jb.kvol * jb.cout * jb.cin;          // cin % 4 == 0: a group of 4 shares its output channel
  // 16-byte loads where the input channels are contiguous in the master weight (1x1x1 convolutions stored [Cout,Cin,1,1,1])
  const bool vec = jb.sb == 1 && (jb.sa & 3) == 0 && (jb.kvol == 1 || (jb.sk & 3) == 0) && ((unsigned long long)jb.w & 15) == 0;
  const long long i0 = (long long)blk * BNFOLD_EPB;
  for (long long i = i0 + (long long)threadIdx.x * 4; i < i0 + BNFOLD_EPB && i < n; i += 1024) {
    const int ci = (int)(i % jb.cin), co = (int)((i / jb.cin) % jb.cout), k = (int)(i / ((long long)jb.cin * jb.cout));
    const float scale = jb.gamma[co] / sqrtf(jb.var[co] + jb.eps);
    const float* src = jb.w + k * jb.sk + co * jb.sa + ci * jb.sb;
    f32x4 v;
    if (vec) v = *(const f32x4*)src;
    else { v[0] = src[0]; v[1] = src[jb.sb]; v[2] = src[2 * jb.sb]; v[3] = src[3 * jb.sb]; }
    v *= scale;
    *(bf16x4*)(jb.w_folded + i) = __builtin_convertvector(v, bf16x4);      // round to nearest even
  }
}

extern "C" int64_t u3d_bn_fold_job_bytes(void) { return (int64_t)sizeof(u3d_bn_fold_job); }
extern "C" int32_t u3d_bn_fold_job_blocks(int32_t kvol, int32_t cout, int32_t cin) {
  const long long n = (long long)kvol * cout * cin;
  return (int32_t)((n + BNFOLD_EPB - 1) / BNFOLD_EPB);
}
// jobs: DEVICE array of njobs u3d_bn_fold_job records, first_block ascending from 0 (the sum of u3d_bn_fold_job_blocks over the jobs
// before); total_blocks = that sum over all jobs.  Every job: cin % 4 == 0, w_folded 8-byte aligned (the caller's side of the contract:
// the table is on the device and is not read here).
extern "C" int32_t u3d_bn_fold_batched(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s) {
  U3D_REQUIRE(jobs && njobs > 0 && total_blocks > 0, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_bn_fold_batched, dim3(total_blocks), dim3(256), 0, s, (const u3d_bn_fold_job*)jobs, njobs);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
