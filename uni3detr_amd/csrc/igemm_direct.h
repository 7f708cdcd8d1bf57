// Launch plan of the direct-operand implicit-GEMM kernels (igemm_direct.hip), shared with the forward plan (fwd_plan) of igemm_bf16.hip.
#pragma once
#include "common.h"

enum DirEpi { DIR_BF16, DIR_STATS, DIR_F32 };   // bf16 output (+ bf16 addend) / + BatchNorm statistics / F32 output (split-bf16)

struct DirectPlan {
  int slot = -1;        // kernel (igemm_direct.hip's table); -1: shape not served
  int waves = 0;        // per workgroup
  int grid = 0;         // persistent workgroups; 0: empty output, nothing to launch
  size_t lds = 0;       // dynamic LDS (all 27 offsets' weights)
  int partials = 0;     // statistics partials a DIR_STATS launch writes: one per wave (grid * waves)
};

// Kernel and grid for a shape: 27 offsets with a neighbour table, cin and cout in {16, 32, 64}, not 64 -> 64; DIR_STATS: n-major
// weights and cout <= 32; DIR_F32: n-major weights.  No HIP call but the (cached) CU-count query.
DirectPlan u3d_plan_igemm_direct(int n_out_cap, int cin, int cout, int kvol, bool has_nbr, bool nmajor, DirEpi epi);
// addend: DIR_BF16 - NULL or a bf16 addend of out's shape; DIR_F32 - non-NULL: accumulate into what `out` holds.  stats: DIR_STATS only.
int u3d_launch_igemm_direct(const DirectPlan& p, const void* in, const void* w, const int32_t* nbr, int ld, void* out,
                            const int32_t* n_out_dev, int n_out_cap, int cin, int cout, hipStream_t s, const void* addend, double* stats);
