// bf16 implicit-GEMM weight-gradient kernels and their launch plan (the forward / input-gradient half: igemm_bf16.hip).
//
//   dW[kappa](ci, co) = sum_m in[nbr[kappa][m], ci] * dout[m, co]
//
// MFMA: v_mfma_f32_16x16x32_bf16, f32 accumulation.  The reduction index is the LDS row of BOTH operands, so both are fetched with
// ds_read_b64_tr_b16.  Every kernel writes f32 partials per row split into the workspace; a second launch sums them in a fixed order.
#include "igemm_common.h"
#include "conv_in.h"

#ifndef WGRAD_DMA_SPREAD
#define WGRAD_DMA_SPREAD 1   /* 1: the next stage's LDS-DMA instructions go out behind the MFMA groups of the first k-step (256 x 256 two-phase tile only), 0: at the top of the stage */
#endif

// =============================================================================================
// weight gradient: workgroup (split, kappa, block) accumulates dW[kappa][ci0:+TM][co0:+TN] over its slice of output rows.
// stage = 64 output rows: A tile [64][TM] (gathered input rows), D tile [64][TN] (dout rows), both row-major with the
// reduction index as the LDS row -> both MFMA operands come from transpose reads.
// =============================================================================================
template <int WAVES_M, int WAVES_N, int WM, int WN>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void k_igemm_wgrad(const u16* __restrict__ in, const u16* __restrict__ dout,
                                                                        const int* __restrict__ nbr, int ld, float* __restrict__ partial,
                                                                        const int* __restrict__ n_out_dev, int n_out_cap, int cin,
                                                                        int cout, int kvol, int co_blocks) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int TM = WAVES_M * WM * 16, TN = WAVES_N * WN * 16, RK = 64;
  constexpr int LDA = TM + 16, LDD = TN + 16;
  constexpr int A_ELEMS = RK * LDA, D_ELEMS = RK * LDD;
  constexpr int A_SEGS = RK * TM / 8 / NT, D_SEGS = RK * TN / 8 / NT;
  static_assert(RK * TM / 8 % NT == 0 && RK * TN / 8 % NT == 0, "tile/thread mismatch");
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  constexpr int STAGE_ELEMS = A_ELEMS + D_ELEMS;

  const int n_out = min(*n_out_dev, n_out_cap);
  const int nsplit = gridDim.x, split = blockIdx.x, kap = blockIdx.y;
  const int ci0 = (blockIdx.z / co_blocks) * TM, co0 = (blockIdx.z % co_blocks) * TN;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (n_out + RK - 1) / RK;
  const int per = (ntiles + nsplit - 1) / nsplit;
  const int t_begin = split * per, t_end = min(ntiles, t_begin + per);

  // Two operand-fetch variants (measured, tools/conv_bench.py): raw buffer loads + branch-free stage body win for the 128 / 64 /
  // 32 / 16 tiles (+35...65 %), the 256 x 256 tile schedules better with the plain predicated loads (879 vs 707 TFLOP/s).
  if constexpr (TM < 256) {
    // operand fetch as in k_igemm_fwd: raw buffer loads, missing rows = out-of-range offset (hardware zero fill), one branch-free
    // stage body, gather indices consumed one stage after they were requested
    const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
    const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc((void*)dout, 0, -1, 0x00020000);
    const unsigned in_row_bytes = (unsigned)cin * 2u, d_row_bytes = (unsigned)cout * 2u;
    int a_row[A_SEGS], d_row[D_SEGS];
    unsigned a_col[A_SEGS], d_col[D_SEGS];
  #pragma unroll
    for (int u = 0; u < A_SEGS; ++u) {
      int sgi = tid + u * NT;
      a_row[u] = sgi / (TM / 8);
      int c = ci0 + (sgi % (TM / 8)) * 8;
      a_col[u] = c < cin ? (unsigned)c * 2u : 0xFFFFFFFFu;
    }
  #pragma unroll
    for (int u = 0; u < D_SEGS; ++u) {
      int sgi = tid + u * NT;
      d_row[u] = sgi / (TN / 8);
      int c = co0 + (sgi % (TN / 8)) * 8;
      d_col[u] = c < cout ? (unsigned)c * 2u : 0xFFFFFFFFu;
    }
    u32x4 ra[A_SEGS], rd[D_SEGS];
    int src_nxt[A_SEGS];
    auto load_src_next = [&](int t) {                     // gather indices of stage t, fetched one stage early (raw: masked at use)
      const int r0 = t * RK;
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) {
        int m = r0 + a_row[u];
        int mc = m < n_out ? m : n_out - 1;
        src_nxt[u] = nbr ? nbr[(long long)kap * ld + mc] : mc;
      }
    };
    auto issue_loads = [&](int t) {
      const int r0 = t * RK;
      const bool live = t < t_end;
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) {
        const bool ok = live && (r0 + a_row[u] < n_out) && src_nxt[u] >= 0 && a_col[u] != 0xFFFFFFFFu;
        unsigned voff = ok ? (unsigned)src_nxt[u] * in_row_bytes + a_col[u] : 0xFFFFFFFFu;
        ra[u] = __builtin_amdgcn_raw_buffer_load_b128(in_rs, voff, 0, 0);
      }
  #pragma unroll
      for (int u = 0; u < D_SEGS; ++u) {
        const int m = r0 + d_row[u];
        const bool ok = live && m < n_out && d_col[u] != 0xFFFFFFFFu;
        unsigned voff = ok ? (unsigned)m * d_row_bytes + d_col[u] : 0xFFFFFFFFu;
        rd[u] = __builtin_amdgcn_raw_buffer_load_b128(d_rs, voff, 0, 0);
      }
      load_src_next(t + 1);
    };
    auto store_lds = [&](int buf) {
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) { int sgi = tid + u * NT; *(u32x4*)(smem + buf * STAGE_ELEMS + a_row[u] * LDA + (sgi % (TM / 8)) * 8) = ra[u]; }
  #pragma unroll
      for (int u = 0; u < D_SEGS; ++u) { int sgi = tid + u * NT; *(u32x4*)(smem + buf * STAGE_ELEMS + A_ELEMS + d_row[u] * LDD + (sgi % (TN / 8)) * 8) = rd[u]; }
    };

    if (t_begin < t_end) {
      load_src_next(t_begin);
      issue_loads(t_begin);
      store_lds(0);
      __syncthreads();
      for (int t = t_begin; t < t_end; ++t) {
        const int buf = (t - t_begin) & 1;
        issue_loads(t + 1);                               // past the last stage: all offsets out of range -> zeros into the idle buffer
        const u16* A = smem + buf * STAGE_ELEMS;
        const u16* D = A + A_ELEMS;
  #pragma unroll
        for (int ks = 0; ks < RK / 32; ++ks) {
          bf16x8 bfr[WN];
  #pragma unroll
          for (int b = 0; b < WN; ++b) bfr[b] = tr_frag(D, LDD, ks * 32, (wn * WN + b) * 16, lane);
  #pragma unroll
          for (int a = 0; a < WM; ++a) {
            bf16x8 af = tr_frag(A, LDA, ks * 32, (wm * WM + a) * 16, lane);
  #pragma unroll
            for (int b = 0; b < WN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[b], acc[a][b], 0, 0, 0);
          }
          if (ks == 0) store_lds(buf ^ 1);                // under the second k-step's MFMAs (see k_igemm_fwd)
        }
        __syncthreads();
      }
    }
  } else {
    uint4 ra[A_SEGS], rd[D_SEGS];
    int src_cur[A_SEGS], src_nxt[A_SEGS];
    auto load_src_next = [&](int t) {                     // gather indices of stage t, fetched one stage early
      const int r0 = t * RK;
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) {
        int m = r0 + (tid + u * NT) / (TM / 8);
        src_nxt[u] = (t < t_end && m < n_out) ? (nbr ? nbr[(long long)kap * ld + m] : m) : -1;
      }
    };
    auto issue_loads = [&](int t) {
      const int r0 = t * RK;
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) src_cur[u] = src_nxt[u];
      load_src_next(t + 1);
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) {
        int sgi = tid + u * NT;
        int part = sgi % (TM / 8);
        int src = src_cur[u];
        int c = ci0 + part * 8;
        ra[u] = (src >= 0 && c < cin) ? *(const uint4*)(in + (long long)src * cin + c) : make_uint4(0, 0, 0, 0);
      }
  #pragma unroll
      for (int u = 0; u < D_SEGS; ++u) {
        int sgi = tid + u * NT;
        int row = sgi / (TN / 8), part = sgi % (TN / 8);
        int m = r0 + row;
        int c = co0 + part * 8;
        rd[u] = (m < n_out && c < cout) ? *(const uint4*)(dout + (long long)m * cout + c) : make_uint4(0, 0, 0, 0);
      }
    };
    auto store_lds = [&](int buf) {
  #pragma unroll
      for (int u = 0; u < A_SEGS; ++u) { int sgi = tid + u * NT; *(uint4*)(smem + buf * STAGE_ELEMS + (sgi / (TM / 8)) * LDA + (sgi % (TM / 8)) * 8) = ra[u]; }
  #pragma unroll
      for (int u = 0; u < D_SEGS; ++u) { int sgi = tid + u * NT; *(uint4*)(smem + buf * STAGE_ELEMS + A_ELEMS + (sgi / (TN / 8)) * LDD + (sgi % (TN / 8)) * 8) = rd[u]; }
    };

    if (t_begin < t_end) {
      load_src_next(t_begin);
      issue_loads(t_begin);
      store_lds(0);
      __syncthreads();
      for (int t = t_begin; t < t_end; ++t) {
        const int buf = (t - t_begin) & 1;
        if (t + 1 < t_end) issue_loads(t + 1);
        const u16* A = smem + buf * STAGE_ELEMS;
        const u16* D = A + A_ELEMS;
  #pragma unroll
        for (int ks = 0; ks < RK / 32; ++ks) {
          bf16x8 bfr[WN];
  #pragma unroll
          for (int b = 0; b < WN; ++b) bfr[b] = tr_frag(D, LDD, ks * 32, (wn * WN + b) * 16, lane);
  #pragma unroll
          for (int a = 0; a < WM; ++a) {
            bf16x8 af = tr_frag(A, LDA, ks * 32, (wm * WM + a) * 16, lane);
  #pragma unroll
            for (int b = 0; b < WN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[b], acc[a][b], 0, 0, 0);
          }
          if (ks == 0 && t + 1 < t_end) store_lds(buf ^ 1);     // under the second k-step's MFMAs (see k_igemm_fwd)
        }
        __syncthreads();
      }
    }
  }
  float* p = partial + ((long long)split * kvol + kap) * cin * cout;
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        int ci = ci0 + (wm * WM + a) * 16 + g * 4 + r;
        int co = co0 + (wn * WN + b) * 16 + li;
        if (ci < cin && co < cout) p[(long long)ci * cout + co] = acc[a][b][r];
      }
}

// Workgroup (blockIdx.x, blockIdx.y) -> the (row split, offset) it works on.  The `kvol` workgroups of one row split read the
// same `dout` rows and (offset-shifted) the same input rows, at about the same time: on ONE XCD they are fetched into that L2 once
// and hit by the other offsets; dealt round-robin over the XCDs (hardware order: linear id % 8) every L2 streams the whole of both
// tensors.  XCD x takes the splits x, x + 8, ... of the first 8 * floor(nsplit / 8); the workgroups of the remaining splits are
// dealt round-robin (they keep every CU busy: 27 offsets x 9 splits = 243 workgroups, 8 of the 9 splits L2-local).
#ifndef WGRAD_XCD_SPLITS
#define WGRAD_XCD_SPLITS 1
#endif
__device__ __forceinline__ void wgrad_xcd_remap(int& split, int& kap, int nsplit, int kvol) {
#if WGRAD_XCD_SPLITS
  if (nsplit >= 8 && gridDim.z == 1) {
    const int lin = blockIdx.x + gridDim.x * blockIdx.y, xcd = lin & 7, slot = lin >> 3;
    const int q8 = nsplit >> 3, aligned = q8 * kvol;      // slots of the XCD-local part
    if (slot < aligned) {
      split = xcd + 8 * (slot / kvol);
      kap = slot % kvol;
    } else {
      const int rem = (slot - aligned) * 8 + xcd;
      split = 8 * q8 + rem / kvol;
      kap = rem % kvol;
    }
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// weight gradient with LDS-DMA staging: both stage tiles ([64 rows][TM] gathered input rows, [64 rows][TN] dout rows) go global ->
// LDS with `buffer_load_dwordx4 ... lds`, lane-linear, unpadded.  Transpose reads of an unpadded tile would put the 8 rows of a
// 32-lane group on the same banks (row stride = multiple of 256 B), so 16-column tile T of row r is stored at tile position
// T ^ (r & 7) (source-side swizzle; r & 7 is a per-lane constant of the reading lane: its rows are k0 + 4g + j (+16)).
// Requires cin % TM == 0 and cout % TN == 0 (dispatch), TM, TN in {64, 128, 256}.
// ---------------------------------------------------------------------------------------------
template <int WAVES_M, int WAVES_N, int WM, int WN>
__device__ __forceinline__ void igemm_wgrad_glds_body(const u16* __restrict__ in, const u16* __restrict__ dout,
                                                      const int* __restrict__ nbr, int ld, float* __restrict__ partial,
                                                      const int* __restrict__ n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                      int co_blocks, int kap_override = -1) {
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int TM = WAVES_M * WM * 16, TN = WAVES_N * WN * 16, RK = 64;
  constexpr int A_ELEMS = RK * TM, D_ELEMS = RK * TN, STAGE_ELEMS = A_ELEMS + D_ELEMS;
  constexpr int A_LPR = TM / 8, D_LPR = TN / 8;                  // lanes (16-byte slots) per row
  constexpr int A_RPI = 64 / A_LPR, D_RPI = 64 / D_LPR;          // rows per wave-instruction (1 KiB)
  constexpr int A_SEGS = RK / A_RPI / NW, D_SEGS = RK / D_RPI / NW;
  constexpr int A_YMASK = (TM / 16 >= 8) ? 7 : (TM / 16 - 1), D_YMASK = (TN / 16 >= 8) ? 7 : (TN / 16 - 1);
  static_assert(RK % (A_RPI * NW) == 0 && RK % (D_RPI * NW) == 0, "tile/wave mismatch");
  extern __shared__ __attribute__((aligned(16))) u16 smem[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int nsplit = gridDim.x;
  int split = blockIdx.x, kap = kap_override >= 0 ? kap_override : (int)blockIdx.y;
  if (kap_override < 0) wgrad_xcd_remap(split, kap, nsplit, kvol);
  const int ci0 = (blockIdx.z / co_blocks) * TM, co0 = (blockIdx.z % co_blocks) * TN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (n_out + RK - 1) / RK;
  const int per = (ntiles + nsplit - 1) / nsplit;
  const int t_begin = split * per, t_end = min(ntiles, t_begin + per);

  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc((void*)dout, 0, -1, 0x00020000);
  const unsigned in_row_bytes = (unsigned)cin * 2u, d_row_bytes = (unsigned)cout * 2u;
  // loader role
  int a_row[A_SEGS], d_row[D_SEGS];
  unsigned a_col[A_SEGS], d_col[D_SEGS];
#pragma unroll
  for (int u = 0; u < A_SEGS; ++u) {
    const int r = (wv * A_SEGS + u) * A_RPI + lane / A_LPR, slot = lane % A_LPR;
    const int chunk = slot ^ (((r & 7) & A_YMASK) << 1);         // 16-column tile T = chunk >> 1 is XORed with r & 7
    a_row[u] = r;
    a_col[u] = (unsigned)(ci0 + chunk * 8) * 2u;
  }
#pragma unroll
  for (int u = 0; u < D_SEGS; ++u) {
    const int r = (wv * D_SEGS + u) * D_RPI + lane / D_LPR, slot = lane % D_LPR;
    const int chunk = slot ^ (((r & 7) & D_YMASK) << 1);
    d_row[u] = r;
    d_col[u] = (unsigned)(co0 + chunk * 8) * 2u;
  }
  int src_nxt[A_SEGS];
  auto load_src_next = [&](int t) {
    const int r0 = t * RK;
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) {
      int m = r0 + a_row[u];
      int mc = m < n_out ? m : n_out - 1;
      src_nxt[u] = nbr ? nbr[(long long)kap * ld + mc] : mc;
    }
  };
  auto issue = [&](int t, int buf) {
    const int r0 = t * RK;
    const bool live = t < t_end;
    u16* Ab = smem + buf * STAGE_ELEMS + wv * (A_SEGS * 512);
    u16* Db = smem + buf * STAGE_ELEMS + A_ELEMS + wv * (D_SEGS * 512);
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) {
      const bool ok = live && (r0 + a_row[u] < n_out) && src_nxt[u] >= 0;
      unsigned voff = ok ? (unsigned)src_nxt[u] * in_row_bytes + a_col[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(Ab + u * 512), 16, voff, 0, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < D_SEGS; ++u) {
      const int m = r0 + d_row[u];
      unsigned voff = (live && m < n_out) ? (unsigned)m * d_row_bytes + d_col[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(d_rs, (lds_void_ptr)(Db + u * 512), 16, voff, 0, 0, 0);
    }
    load_src_next(t + 1);
  };
  // one LDS-DMA instruction of stage t (q < A_SEGS: gathered input rows, else gradient rows), dealt out behind MFMA groups (see
  // GLDS_DMA_SPREAD in the forward kernel: a stage's loads queued in front of its MFMAs hold the waves at the address unit)
  auto issue_one = [&](int t, int buf, int q) {
    const int r0 = t * RK;
    const bool live = t < t_end;
    if (q < A_SEGS) {
      u16* Ab = smem + buf * STAGE_ELEMS + wv * (A_SEGS * 512);
      const bool ok = live && (r0 + a_row[q] < n_out) && src_nxt[q] >= 0;
      unsigned voff = ok ? (unsigned)src_nxt[q] * in_row_bytes + a_col[q] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(Ab + q * 512), 16, voff, 0, 0, 0);
    } else {
      const int u = q - A_SEGS;
      u16* Db = smem + buf * STAGE_ELEMS + A_ELEMS + wv * (D_SEGS * 512);
      const int m = r0 + d_row[u];
      unsigned voff = (live && m < n_out) ? (unsigned)m * d_row_bytes + d_col[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(d_rs, (lds_void_ptr)(Db + u * 512), 16, voff, 0, 0, 0);
    }
  };
  // reader role: transpose-read fragments; this lane's rows are k0 + 4g + j (+16): y = (4g + j) & 7
  const int g = lane >> 4, L = lane & 15, j = L >> 2, q = L & 3;
  const int ya = ((4 * g + j) & 7) & A_YMASK, yd = ((4 * g + j) & 7) & D_YMASK;
  auto trf = [&](const u16* tile, int stride, int k0, int T, int y) {
    const u16* p0 = tile + (k0 + 4 * g + j) * stride + ((T ^ y) << 4) + 4 * q;
    s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0));
    s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0 + 16 * stride));
    s16x8 v = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

  if (t_begin < t_end) {
    load_src_next(t_begin);
    issue(t_begin, 0);
    __syncthreads();
    for (int t = t_begin; t < t_end; ++t) {
      const int buf = (t - t_begin) & 1;
      // spreading pays on the 256 x 256 tile only (measured per tile size: +4.5 % there, a loss at step level when applied to all)
      constexpr bool SPREAD = WGRAD_DMA_SPREAD && TM >= 256 && TN >= 256;
      int src_nn[A_SEGS];                               // gather indices of stage t+2: requested now, moved into src_nxt at the end of the stage
      if constexpr (!SPREAD) {
        issue(t + 1, buf ^ 1);                          // past the last stage: all offsets out of range -> zeros into the idle buffer
      } else {
        const int r0n = (t + 2) * RK;
#pragma unroll
        for (int u = 0; u < A_SEGS; ++u) {
          int m = r0n + a_row[u];
          int mc = m < n_out ? m : n_out - 1;
          src_nn[u] = nbr ? nbr[(long long)kap * ld + mc] : mc;
        }
      }
      const u16* A = smem + buf * STAGE_ELEMS;
      const u16* D = A + A_ELEMS;
#pragma unroll
      for (int ks = 0; ks < RK / 32; ++ks) {
        bf16x8 bfr[WN];
#pragma unroll
        for (int b = 0; b < WN; ++b) bfr[b] = trf(D, TN, ks * 32, wn * WN + b, yd);
#pragma unroll
        for (int a = 0; a < WM; ++a) {
          bf16x8 af = trf(A, TM, ks * 32, wm * WM + a, ya);
#pragma unroll
          for (int b = 0; b < WN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[b], af, acc[a][b], 0, 0, 0);   // transposed block
          if constexpr (SPREAD) if (ks == 0) {            // the next stage's loads behind the MFMA groups of the first k-step
            constexpr int NQ = A_SEGS + D_SEGS, PER = (NQ + WM - 1) / WM;
#pragma unroll
            for (int jq = 0; jq < PER; ++jq)
              if (a * PER + jq < NQ) issue_one(t + 1, buf ^ 1, a * PER + jq);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      }
      if constexpr (SPREAD) {
#pragma unroll
        for (int u = 0; u < A_SEGS; ++u) src_nxt[u] = src_nn[u];
      }
      __syncthreads();
    }
  }
  // acc[a][b][r] = dW[ci (wm*WM+a)*16 + li][co (wn*WN+b)*16 + 4g + r]: one 16-byte store per block
  float* p = partial + ((long long)split * kvol + kap) * cin * cout;
  const int li = lane & 15;
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) {
      const int ci = ci0 + (wm * WM + a) * 16 + li;
      const int co = co0 + (wn * WN + b) * 16 + 4 * g;
      *(f32x4*)(p + (long long)ci * cout + co) = acc[a][b];
    }
}
// ---------------------------------------------------------------------------------------------
// 256 x 256 weight-gradient tile on the EIGHT-PHASE schedule of igemm_glds8_body (same segments, counts and barriers; read that
// comment first).  What differs: the reduction index is the output ROW (64 per k-tile), both operands are [64 rows][256 channels]
// tiles read with transpose reads, and a k-tile's four 16 KiB pieces are COLUMN ranges: A0 / A1 = the first / second 64 input
// channels of both wave rows (128 columns, 256 B per row), D0 / D1 = the first / second 32 output channels of all four wave
// columns.  One LDS-DMA instruction = 4 rows x 256 B; 16-column tile T of piece row r sits at position T ^ (r & 7).  The two A
// pieces gather the SAME 64 rows: two index registers per lane.  Needs a neighbour table (the batched linear-layer form stays on
// igemm_wgrad_glds_body).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void igemm_wgrad_glds8_body(const u16* __restrict__ in, const u16* __restrict__ dout,
                                                       const int* __restrict__ nbr, int ld, float* __restrict__ partial,
                                                       const int* __restrict__ n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                       int co_blocks) {
  constexpr int WAVES_N = 4, WM = 8, WN = 4, RK = 64;
  constexpr int PC = 128;                                  // columns of a piece
  constexpr int PIECE = RK * PC, STAGE_ELEMS = 4 * PIECE;  // A0 | A1 | D0 | D1
  extern __shared__ __attribute__((aligned(16))) u16 smem[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int nsplit = gridDim.x;
  int split = blockIdx.x, kap = (int)blockIdx.y;
  wgrad_xcd_remap(split, kap, nsplit, kvol);
  const int ci0 = (blockIdx.z / co_blocks) * 256, co0 = (blockIdx.z % co_blocks) * 256;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const int ntiles = (n_out + RK - 1) / RK;
  const int per = (ntiles + nsplit - 1) / nsplit;
  const int t_begin = split * per, t_end = min(ntiles, t_begin + per);
  const int nstage = t_end - t_begin;

  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t d_rs = __builtin_amdgcn_make_buffer_rsrc((void*)dout, 0, -1, 0x00020000);
  const unsigned in_row_bytes = (unsigned)cin * 2u, d_row_bytes = (unsigned)cout * 2u;
  // loader role: instruction u (0 / 1) of this wave fills piece rows (wv*2+u)*4 .. +3; lane = (row in group, 16-byte slot of 16)
  const int lrow = lane >> 4, lslot = lane & 15;
  int prow[2];
  unsigned a_col[2][2], d_col[2][2];                       // [piece][u]: byte offset of this lane's 16 bytes inside a source row
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (wv * 2 + u) * 4 + lrow;
    prow[u] = r;
    const int chunk = lslot ^ ((r & 7) << 1);              // 8-column chunk of the piece this slot receives (tile T = chunk >> 1 swizzled)
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      const int ca = (chunk < 8) ? sp * 64 + chunk * 8 : 128 + sp * 64 + (chunk - 8) * 8;          // piece column -> input channel
      a_col[sp][u] = (unsigned)(ci0 + ca) * 2u;
      const int pc = chunk * 8;                                                                     // piece column 0..127
      const int cd = (pc >> 5) * 64 + sp * 32 + (pc & 31);                                          // -> output channel
      d_col[sp][u] = (unsigned)(co0 + cd) * 2u;
    }
  }
  const int* nrow = nbr + (long long)kap * ld;
  int idx_cur[2], idx_nxt[2];
  auto load_idx_next = [&](int t) {                        // t: row tile (clamped by the caller)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = t * RK + prow[u];
      idx_nxt[u] = nrow[m < n_out ? m : n_out - 1];
    }
  };
  auto advance_idx = [&](int t) {                          // indices of row tile t; -1 = zero row (past the end / missing neighbour)
#pragma unroll
    for (int u = 0; u < 2; ++u) idx_cur[u] = (t < t_end && t * RK + prow[u] < n_out) ? idx_nxt[u] : -1;
  };
  auto issue_a = [&](int buf, int sp) {                    // piece A_sp of the row tile idx_cur describes
    u16* dst = smem + buf * STAGE_ELEMS + sp * PIECE + wv * 1024;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned voff = idx_cur[u] >= 0 ? (unsigned)idx_cur[u] * in_row_bytes + a_col[sp][u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(dst + u * 512), 16, voff, 0, 0, 0);
    }
  };
  auto issue_d = [&](int t, int buf, int sp) {
    u16* dst = smem + buf * STAGE_ELEMS + (2 + sp) * PIECE + wv * 1024;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = t * RK + prow[u];
      const unsigned voff = (t < t_end && m < n_out) ? (unsigned)m * d_row_bytes + d_col[sp][u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(d_rs, (lds_void_ptr)(dst + u * 512), 16, voff, 0, 0, 0);
    }
  };
  // reader role: transpose-read fragments; this lane's rows are k0 + 4g + j (+16): y = (4g + j) & 7
  const int g = lane >> 4, L = lane & 15, j = L >> 2, q = L & 3;
  const int y = (4 * g + j) & 7;
  auto trf = [&](const u16* piece, int k0, int T) {
    const u16* p0 = piece + (k0 + 4 * g + j) * PC + ((T ^ y) << 4) + 4 * q;
    s16x4 x0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0));
    s16x4 x1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0 + 16 * PC));
    s16x8 v = {x0[0], x0[1], x0[2], x0[3], x1[0], x1[1], x1[2], x1[3]};
    return __builtin_bit_cast(bf16x8, v);
  };
  bf16x8 af[2][4][2], df[2][2][2];                         // A: [half][ci block][k-step]; D: [half][co block][k-step]
#define W8_READ_A(BUF, SP)                                                                       \
  {                                                                                              \
    const u16* A_ = smem + (BUF) * STAGE_ELEMS + (SP) * PIECE;                                   \
    _Pragma("unroll") for (int a = 0; a < 4; ++a) {                                              \
      af[SP][a][0] = trf(A_, 0, wm * 4 + a);                                                     \
      af[SP][a][1] = trf(A_, 32, wm * 4 + a);                                                    \
    }                                                                                            \
  }
#define W8_READ_D(BUF, SP)                                                                       \
  {                                                                                              \
    const u16* D_ = smem + (BUF) * STAGE_ELEMS + (2 + (SP)) * PIECE;                             \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) {                                              \
      df[SP][b][0] = trf(D_, 0, wn * 2 + b);                                                     \
      df[SP][b][1] = trf(D_, 32, wn * 2 + b);                                                    \
    }                                                                                            \
  }
#define W8_MMA(SA, SB)                                                                           \
  {                                                                                              \
    __builtin_amdgcn_s_setprio(1);                                                               \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                             \
      _Pragma("unroll") for (int b = 0; b < 2; ++b)                                              \
        _Pragma("unroll") for (int a = 0; a < 4; ++a)                                            \
          acc[(SA) * 4 + a][(SB) * 2 + b] =                                                      \
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(df[SB][b][ks], af[SA][a][ks], acc[(SA) * 4 + a][(SB) * 2 + b], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                               \
  }
#define W8_BAR()                                  \
  {                                               \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);            \
  }
  if (nstage > 0) {
    // prologue: row tile t_begin complete in buffer 0, its first A half in registers, indices of t_begin + 1 current
    load_idx_next(t_begin);
    advance_idx(t_begin);
    issue_a(0, 0); issue_d(t_begin, 0, 0); issue_d(t_begin, 0, 1); issue_a(0, 1);
    load_idx_next(t_begin + 1);
    advance_idx(t_begin + 1);
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0)
    W8_BAR();
    W8_READ_A(0, 0)
    if (wm == 1) W8_BAR();                                // the second wave row runs one barrier behind the first
    for (int st = 0; st < nstage; ++st) {
      const int buf = st & 1, t = t_begin + st;
      // ---- phase 1: (ci 0-63, co 0-31); requests: indices of t + 2, piece A0 of t + 1
      load_idx_next(t + 2);
      __builtin_amdgcn_sched_barrier(0);
      W8_READ_D(buf, 0)
      issue_a(buf ^ 1, 0);
      __builtin_amdgcn_s_waitcnt(0x0F76);                  // vmcnt(6) = A1 + 2 indices + A0': D1 of this row tile has landed
      W8_BAR();
      W8_MMA(0, 0)
      W8_BAR();
      // ---- phase 2: (ci 0-63, co 32-63)
      W8_READ_D(buf, 1)
      issue_d(t + 1, buf ^ 1, 0);
      __builtin_amdgcn_s_waitcnt(0x0F76);                  // vmcnt(6) = 2 indices + A0' + D0': A1 of this row tile
      W8_BAR();
      W8_MMA(0, 1)
      W8_BAR();
      // ---- phase 3: (ci 64-127, co 32-63)
      W8_READ_A(buf, 1)
      issue_d(t + 1, buf ^ 1, 1);
      __builtin_amdgcn_s_waitcnt(0x0F74);                  // vmcnt(4): the indices and A0 of the next row tile
      W8_BAR();
      W8_MMA(1, 1)
      W8_BAR();
      // ---- phase 4: (ci 64-127, co 0-31): D0 is still in registers; the next row tile's first A half is read here
      W8_READ_A(buf ^ 1, 0)
      issue_a(buf ^ 1, 1);
      __builtin_amdgcn_sched_barrier(0);
      advance_idx(t + 2);
      __builtin_amdgcn_s_waitcnt(0x0F74);                  // vmcnt(4): D0 of the next row tile
      W8_BAR();
      W8_MMA(1, 0)
      W8_BAR();
    }
    if (wm == 0) W8_BAR();
    __builtin_amdgcn_s_waitcnt(0x0F70);                    // the tail's zero-fill requests
  }
#undef W8_READ_A
#undef W8_READ_D
#undef W8_MMA
#undef W8_BAR
  float* p = partial + ((long long)split * kvol + kap) * cin * cout;
  const int li = lane & 15;
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) {
      const int ci = ci0 + (wm * WM + a) * 16 + li;
      const int co = co0 + (wn * WN + b) * 16 + 4 * g;
      *(f32x4*)(p + (long long)ci * cout + co) = acc[a][b];
    }
}
__global__ __launch_bounds__(512) void k_igemm_wgrad_glds8_256(const u16* in, const u16* dout, const int* nbr, int ld, float* partial,
                                                               const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                               int co_blocks) {
  igemm_wgrad_glds8_body(in, dout, nbr, ld, partial, n_out_dev, n_out_cap, cin, cout, kvol, co_blocks);
}

#define U3D_WGRAD_GLDS_KERNEL(NAME, A, B, C, D)                                                                                   \
  __global__ __launch_bounds__(A* B * 64) void NAME(const u16* in, const u16* dout, const int* nbr, int ld, float* partial,        \
                                                    const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol, int co_blocks) { \
    igemm_wgrad_glds_body<A, B, C, D>(in, dout, nbr, ld, partial, n_out_dev, n_out_cap, cin, cout, kvol, co_blocks);               \
  }
U3D_WGRAD_GLDS_KERNEL(k_igemm_wgrad_glds_256, 2, 4, 8, 4)
U3D_WGRAD_GLDS_KERNEL(k_igemm_wgrad_glds_128, 2, 2, 4, 4)
U3D_WGRAD_GLDS_KERNEL(k_igemm_wgrad_glds_64, 2, 2, 2, 2)
// (32- and 16-channel tiles were tried on this kernel too: correct, but no faster than k_igemm_wgrad - those layers are bound by
//  the L2 gather, not by staging - so they stay on the buffer-load kernel)
#undef U3D_WGRAD_GLDS_KERNEL
// ---- batched form for the decoder / head linears: `count` independent products dW_b = in_b^T @ dout_b of ONE shape in one launch
//      (grid.y = batch index; pointers arrive by value in the kernel arguments - no device-side table, capturable as is)
#define U3D_WGRAD_BATCH_MAX 48
struct WgradBatch {
  const u16* in[U3D_WGRAD_BATCH_MAX];
  const u16* dout[U3D_WGRAD_BATCH_MAX];
  float* dw[U3D_WGRAD_BATCH_MAX];
};
#define U3D_WGRAD_BATCH_KERNEL(NAME, A, B, C, D)                                                                                    \
  __global__ __launch_bounds__(A* B * 64) void NAME(WgradBatch bt, float* partial, const int* n_dev, int n_cap, int cin, int cout,   \
                                                    int co_blocks, long long partial_stride) {                                      \
    const int b = blockIdx.y;                                                                                                        \
    igemm_wgrad_glds_body<A, B, C, D>(bt.in[b], bt.dout[b], nullptr, 0, partial + (long long)b * partial_stride, n_dev, n_cap, cin,   \
                                      cout, 1, co_blocks, 0);                                                                         \
  }
U3D_WGRAD_BATCH_KERNEL(k_wgrad_batch_256, 2, 4, 8, 4)
U3D_WGRAD_BATCH_KERNEL(k_wgrad_batch_128, 2, 2, 4, 4)
U3D_WGRAD_BATCH_KERNEL(k_wgrad_batch_64, 2, 2, 2, 2)
#undef U3D_WGRAD_BATCH_KERNEL
// sum of the `nsplit` partials of one f32x4 in a FIXED order, as four independent chains: eight loads in flight per pass instead of
// one (the reductions were latency chains: 20 us for 16 MB of partials)
__device__ __forceinline__ f32x4 wgrad_sum_splits(const float* __restrict__ p, long long stride, int nsplit) {
  f32x4 a = (f32x4){0.f, 0.f, 0.f, 0.f}, b = a, c = a, d = a;
  int k = 0;
  for (; k + 8 <= nsplit; k += 8) {
    const f32x4 v0 = *(const f32x4*)(p + (long long)k * stride), v1 = *(const f32x4*)(p + (long long)(k + 1) * stride);
    const f32x4 v2 = *(const f32x4*)(p + (long long)(k + 2) * stride), v3 = *(const f32x4*)(p + (long long)(k + 3) * stride);
    const f32x4 v4 = *(const f32x4*)(p + (long long)(k + 4) * stride), v5 = *(const f32x4*)(p + (long long)(k + 5) * stride);
    const f32x4 v6 = *(const f32x4*)(p + (long long)(k + 6) * stride), v7 = *(const f32x4*)(p + (long long)(k + 7) * stride);
    a += v0; b += v1; c += v2; d += v3; a += v4; b += v5; c += v6; d += v7;
  }
  for (; k < nsplit; ++k) a += *(const f32x4*)(p + (long long)k * stride);
  return (a + b) + (c + d);
}

// Products that name the SAME output in consecutive batch slots (a weight shared by several decoder layers: dW = sum over its uses)
// are summed here: the group's first slot reduces the nsplit partials of all its members (contiguous in the workspace), the others
// have no output (mult 0).  One fixed order, no separate accumulate launches.
struct WgradGroups { unsigned char mult[U3D_WGRAD_BATCH_MAX]; };
__global__ void k_wgrad_batch_reduce(WgradBatch bt, WgradGroups gr, const float* __restrict__ partial, long long n, int nsplit,
                                     long long partial_stride) {
  const int b = blockIdx.y;
  const int g = gr.mult[b];
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n || g == 0) return;
  *(f32x4*)(bt.dw[b] + i) = wgrad_sum_splits(partial + (long long)b * partial_stride + i, n, nsplit * g);
}

__global__ void k_igemm_wgrad_reduce(const float* __restrict__ partial, float* __restrict__ dw, long long n, int nsplit) {
  long long i = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i >= n) return;
  *(f32x4*)(dw + i) = wgrad_sum_splits(partial + i, n, nsplit);
}

// (shared by the two transposing reductions below: partial [nsplit][K][ca][cb]; the workgroup = (row a of ca, 64 columns of cb, a third
//  of the offsets) sums the splits in a fixed order reading along cb, coalesced, and leaves its [column][k] tile in LDS)
__device__ __forceinline__ void wgrad_reduce_tile(const float* __restrict__ partial, long long n, int nsplit, int ca, int cb, int a,
                                                  int b0, int k0, int k1, float (&tile)[64][10]) {
  const int t = threadIdx.x, col = t & 63;
  for (int k = k0 + (t >> 6); k < k1; k += 4) {
    float s = 0.f;
    if (b0 + col < cb) {
      const float* p = partial + ((long long)k * ca + a) * cb + b0 + col;
      float acc[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] = 0.f;
      int sp = 0;
      for (; sp + 8 <= nsplit; sp += 8) {            // eight independent loads in flight, fixed summation order
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += p[(long long)(sp + j) * n];
      }
      for (; sp < nsplit; ++sp) acc[0] += p[(long long)sp * n];
      s = ((acc[0] + acc[1]) + (acc[2] + acc[3])) + ((acc[4] + acc[5]) + (acc[6] + acc[7]));
    }
    tile[col][k - k0] = s;
  }
  __syncthreads();
}
// same reduction, result written as [Cout][Cin][K] (nn.Conv3d's checkpoint layout): the gradient lands in the parameter's own
// layout and autograd keeps it as is (a permuted view would be cloned into a contiguous tensor by AccumulateGrad: one more launch)
__global__ __launch_bounds__(256) void k_igemm_wgrad_reduce_oik(const float* __restrict__ partial, float* __restrict__ dw, long long n,
                                                                int nsplit, int kvol, int cin, int cout) {
  // workgroup = (ci, 64 output channels, a third of the offsets): reads run along co (coalesced; splits summed in a fixed order), the
  // [co][k] tile is turned in LDS, writes run along k (the innermost dimension of [Cout][Cin][K])
  __shared__ float tile[64][10];
  const int ci = blockIdx.x, co0 = blockIdx.y * 64;
  const int kper = (kvol + gridDim.z - 1) / gridDim.z, k0 = blockIdx.z * kper, k1 = min(kvol, k0 + kper);
  wgrad_reduce_tile(partial, n, nsplit, cin, cout, ci, co0, k0, k1, tile);
  const int nk = k1 - k0;
  for (int idx = threadIdx.x; idx < 64 * nk; idx += 256) {
    const int cl = idx / nk, k = idx % nk;
    if (co0 + cl < cout) dw[((long long)(co0 + cl) * cin + ci) * kvol + k0 + k] = tile[cl][k];
  }
}
// same reduction for out_layout 2: partial [nsplit][K][ca][cb] -> dw [ca][cb][K] (the call with the operands exchanged: ca = the
// convolution's Cout, cb = its Cin, so this too is nn.Conv3d's layout); a workgroup's writes are one contiguous run of 64 * nk floats
__global__ __launch_bounds__(256) void k_igemm_wgrad_reduce_abk(const float* __restrict__ partial, float* __restrict__ dw, long long n,
                                                                int nsplit, int kvol, int ca, int cb) {
  __shared__ float tile[64][10];
  const int a = blockIdx.x, b0 = blockIdx.y * 64;
  const int kper = (kvol + gridDim.z - 1) / gridDim.z, k0 = blockIdx.z * kper, k1 = min(kvol, k0 + kper);
  wgrad_reduce_tile(partial, n, nsplit, ca, cb, a, b0, k0, k1, tile);
  const int nk = k1 - k0;
  for (int idx = threadIdx.x; idx < 64 * nk; idx += 256) {
    const int cl = idx / nk, k = idx % nk;
    if (b0 + cl < cb) dw[((long long)a * cb + b0 + cl) * kvol + k0 + k] = tile[cl][k];
  }
}

// =============================================================================================
// ONE launch plan for the weight-gradient launches: wgrad_plan() decides the kernel family, tile, row split, grid, workspace and
// reduction of u3d_igemm_wgrad_bf16, u3d_igemm_wgrad_bf16_workspace sizes the buffer from that same plan and u3d_igemm_wgrad_plan
// reports it; wgrad_plan_batched() fills the same struct for u3d_wgrad_batched_bf16.
// =============================================================================================
typedef void (*wgrad_kernel_t)(const u16*, const u16*, const int*, int, float*, const int*, int, int, int, int, int);
typedef void (*wgrad_batch_kernel_t)(WgradBatch, float*, const int*, int, int, int, int, long long);
// The kernel families (u3d_igemm_wgrad_plan reports the index).  CONVIN (conv_in.hip) and NARROW (wgrad_narrow.hip) launch and reduce
// themselves; the others are the rows of WGRAD_KERNELS: single-product kernel, batched form (nullptr: none), square tile, threads,
// dynamic LDS (LDS-DMA: two unpadded stages of 64 rows x 2 tiles; register-staged: rows padded by 16 elements).
enum { WG_NONE, WG_CONVIN, WG_NARROW, WG_GLDS8_256, WG_GLDS_256, WG_GLDS_128, WG_GLDS_64, WG_REG_32, WG_REG_16, WG_COUNT };
struct WgradKernel {
  wgrad_kernel_t fn;
  wgrad_batch_kernel_t batch;
  int tile, threads;
  size_t lds;
};
static const WgradKernel WGRAD_KERNELS[WG_COUNT] = {
    {}, {}, {},
    {k_igemm_wgrad_glds8_256, nullptr, 256, 512, 4 * 64 * 256 * 2},               // eight-phase, 128 KiB: needs a neighbour table
    {k_igemm_wgrad_glds_256, k_wgrad_batch_256, 256, 512, 4 * 64 * 256 * 2},      // two-phase
    {k_igemm_wgrad_glds_128, k_wgrad_batch_128, 128, 256, 4 * 64 * 128 * 2},
    {k_igemm_wgrad_glds_64, k_wgrad_batch_64, 64, 256, 4 * 64 * 64 * 2},
    {k_igemm_wgrad<2, 2, 1, 1>, nullptr, 32, 256, 4 * 64 * (32 + 16) * 2},        // register-staged: the 16/32-channel sparse levels,
    {k_igemm_wgrad<1, 1, 1, 1>, nullptr, 16, 64, 4 * 64 * (16 + 16) * 2},         // load/latency bound
};
enum WgReduce { WG_RED_OWN, WG_RED_KIO, WG_RED_OIK, WG_RED_ABK };     // done by the family's own launch / k_igemm_wgrad_reduce / _reduce_oik / _reduce_abk

struct WgradPlan {
  int family = WG_NONE;          // WG_NONE: no kernel serves the shape
  int tile = 0;                  // square channel tile (0: CONVIN / NARROW)
  int ci_blocks = 0, co_blocks = 0;
  int nsplit = 0;                // f32 partials [nsplit][kvol][cin][cout] in the workspace (batched: per product)
  dim3 grid;
  int threads = 0;
  size_t lds = 0;
  int64_t workspace = 0;         // bytes
  WgReduce reduce = WG_RED_OWN;
  bool served() const { return family != WG_NONE; }
};

#ifndef IGEMM_WGRAD_MIN_STAGES_K1
#define IGEMM_WGRAD_MIN_STAGES_K1 8   /* 4 and 2 measured slower end-to-end (33.4 / 33.9 vs 33.3 ms per step) */
#endif
// row split of a single product on `tile`: enough workgroups for the tile's target (256 / 512 / 2048), yet at least 8 stages (64 rows
// each) per split so the prologue is amortised (IGEMM_WGRAD_MIN_STAGES_K1 for the single-offset products of the decoder / head
// linears: ~113 stages in all, latency-bound - more, shorter workgroups finish sooner)
static void wgrad_split_rows(WgradPlan& p, int tile, int n_out_cap, int cin, int cout, int kvol) {
  p.tile = tile;
  p.ci_blocks = u3d_cdiv(cin, tile);
  p.co_blocks = u3d_cdiv(cout, tile);
  const int ntiles = u3d_cdiv(n_out_cap > 0 ? n_out_cap : 1, 64);
  const int wgs_per_split = kvol * p.ci_blocks * p.co_blocks;
  int target = (tile == 256 ? 256 : (tile >= 64 ? 512 : 2048)) / wgs_per_split;
  if (target < 1) target = 1;
  int ns = ntiles < target ? ntiles : target;
  const int min_stages = (kvol == 1 && ntiles <= 256) ? IGEMM_WGRAD_MIN_STAGES_K1 : 8;
  while (ns > 1 && ntiles / ns < min_stages) --ns;
  p.nsplit = ns < 1 ? 1 : ns;
}
// family of a square LDS-DMA / register-staged tile, and the launch geometry its WGRAD_KERNELS row gives (grid.y = kvol or batch size)
static void wgrad_fill_tile(WgradPlan& p, bool table, int grid_y) {
  p.family = p.tile == 256 ? (table ? WG_GLDS8_256 : WG_GLDS_256)
             : p.tile == 128 ? WG_GLDS_128 : p.tile == 64 ? WG_GLDS_64 : p.tile == 32 ? WG_REG_32 : WG_REG_16;
  p.grid = dim3(p.nsplit, grid_y, p.ci_blocks * p.co_blocks);
  p.threads = WGRAD_KERNELS[p.family].threads;
  p.lds = WGRAD_KERNELS[p.family].lds;
}

// 16/32-channel 27-offset weight gradients: wgrad_narrow.hip
bool u3d_wgrad_narrow_shape(int cin, int cout, int kvol);
int64_t u3d_wgrad_narrow_workspace(int n_out_cap, int cin, int cout);
int u3d_launch_wgrad_narrow(const void* in, const void* dout, const int32_t* nbr, int ld, float* dw, const int32_t* n_out_dev, int n_out_cap,
                            int cin, int cout, int kvol, int out_oik, void* workspace, int64_t workspace_bytes, hipStream_t s);

// The rules, first match wins (n = n_out_cap; "table": a neighbour table is passed - the launch refuses kvol > 1 without one, so the
// plan of such a shape is the plan with a table; out_layout 0: dW [K][Cin][Cout], 1: [Cout][Cin][K], 2: [Cin][Cout][K] - the call with
// the operands exchanged, see u3d_hip.h):
//   1. CONVIN: 8 -> 16, 1 <= kvol <= 27, out_layout 0.  One partial per 128 rows.
//   2. cin % 16 != 0 or cout % 16 != 0: none.
//   3. NARROW: a table, kvol 27 and (cin, cout) in 16 -> 16, 16 -> 32, 32 -> 32, 32 -> 64; none of them for out_layout 2.  32 -> 16, which wgrad_narrow.hip claims
//      without having a kernel for it, is none for n > 0 and takes the family's zero fill for n <= 0.
//   4. out_layout 1 or 2 and kvol > 27: none (k_igemm_wgrad_reduce_oik / _abk turn at most 27 offsets).
//   5. the largest square tile of 256 / 128 / 64 / 32 that divides both channel counts, else 16, with wgrad_split_rows(); while the tile
//      is above 64 and nsplit * kvol * ci_blocks * co_blocks < 192 workgroups (few rows: the decoder / head linears), half the tile.
//      256: eight-phase with a table, two-phase without; 128 / 64: LDS-DMA; 32 / 16: register-staged.
static WgradPlan wgrad_plan(int n_out_cap, int cin, int cout, int kvol, bool has_nbr, int out_layout) {
  WgradPlan p;
  if (cin <= 0 || cout <= 0 || kvol <= 0 || out_layout < 0 || out_layout > 2) return p;
  const bool table = has_nbr || kvol > 1;
  const int64_t nw_bytes = (int64_t)kvol * cin * cout * 4;
  if (convin_shape(cin, cout, kvol) && out_layout == 0) {
    p.family = WG_CONVIN;
    p.nsplit = convin_wgrad_blocks(n_out_cap);
    p.workspace = p.nsplit * nw_bytes;
    return p;
  }
  if (cin % 16 != 0 || cout % 16 != 0) return p;
  if (table && u3d_wgrad_narrow_shape(cin, cout, kvol)) {
    if ((n_out_cap > 0 && cin == 32 && cout == 16) || out_layout == 2) return p;
    p.family = WG_NARROW;
    p.workspace = u3d_wgrad_narrow_workspace(n_out_cap, cin, cout);
    p.nsplit = (int)(p.workspace / nw_bytes);
    return p;
  }
  if (out_layout != 0 && kvol > 27) return p;
  const int mn = cin < cout ? cin : cout;
  int tile;
  if (mn >= 256 && cin % 256 == 0 && cout % 256 == 0) tile = 256;
  else if (mn >= 128 && cin % 128 == 0 && cout % 128 == 0) tile = 128;
  else if (cin % 64 == 0 && cout % 64 == 0) tile = 64;
  else if (cin % 32 == 0 && cout % 32 == 0) tile = 32;
  else tile = 16;
  wgrad_split_rows(p, tile, n_out_cap, cin, cout, kvol);
  while (p.tile > 64 && (long long)p.nsplit * kvol * p.ci_blocks * p.co_blocks < 192) wgrad_split_rows(p, p.tile / 2, n_out_cap, cin, cout, kvol);
  wgrad_fill_tile(p, table, kvol);
  p.workspace = p.nsplit * nw_bytes;
  p.reduce = out_layout == 1 ? WG_RED_OIK : (out_layout == 2 ? WG_RED_ABK : WG_RED_KIO);
  return p;
}

// (no has_nbr / out_layout here: neither changes the workspace of a shape the launch serves)
extern "C" int64_t u3d_igemm_wgrad_bf16_workspace(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol) {
  return wgrad_plan(n_out_cap, cin, cout, kvol, kvol > 1, 0).workspace;
}
// The plan of u3d_igemm_wgrad_bf16 for a shape: *kernel = the family (0 none - never reported -, 1 conv-in, 2 narrow, 3 / 4 eight- /
// two-phase LDS-DMA 256, 5 / 6 LDS-DMA 128 / 64, 7 / 8 register-staged 32 / 16), its *tile (0: conv-in, narrow), the *nsplit partials
// and the *workspace bytes that hold them.  U3D_ERR_UNSUPPORTED where the launch returns it.  Host only.
extern "C" int32_t u3d_igemm_wgrad_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr, int32_t out_layout,
                                        int32_t* kernel, int32_t* tile, int32_t* nsplit, int64_t* workspace) {
  U3D_REQUIRE(kernel && tile && nsplit && workspace, U3D_ERR_ARG);
  const WgradPlan p = wgrad_plan(n_out_cap, cin, cout, kvol, has_nbr != 0, out_layout);
  if (!p.served()) return U3D_ERR_UNSUPPORTED;
  *kernel = p.family;
  *tile = p.tile;
  *nsplit = p.nsplit;
  *workspace = p.workspace;
  return U3D_OK;
}

static unsigned long long wgrad_lds_mask[WG_COUNT][2] = {};     // U3D_ALLOW_LDS's per-device mask, one per kernel ([1]: batched form)

extern "C" int32_t u3d_igemm_wgrad_bf16(const void* in, const void* dout, const int32_t* nbr, int32_t ld, float* dw,
                                        const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                                        int32_t out_layout, void* workspace, int64_t workspace_bytes, u3d_stream s) {
  U3D_REQUIRE(in && dout && dw && n_out_dev && workspace && (nbr || kvol == 1), U3D_ERR_ARG);
  const WgradPlan p = wgrad_plan(n_out_cap, cin, cout, kvol, nbr != nullptr, out_layout);
  if (!p.served()) return U3D_ERR_UNSUPPORTED;
  if (p.family == WG_NARROW) {
    if (n_out_cap <= 0) { hipMemsetAsync(dw, 0, sizeof(float) * kvol * cin * cout, s); return U3D_OK; }
    return u3d_launch_wgrad_narrow(in, dout, nbr, ld, dw, n_out_dev, n_out_cap, cin, cout, kvol, out_layout, workspace, workspace_bytes, s);
  }
  U3D_REQUIRE(workspace_bytes >= p.workspace, U3D_ERR_WORKSPACE);
  if (p.family == WG_CONVIN) return u3d_launch_conv_in_wgrad(in, dout, nbr, ld, dw, n_out_dev, n_out_cap, kvol, (float*)workspace, s);
  const WgradKernel& k = WGRAD_KERNELS[p.family];
  if (p.lds > 64 * 1024) u3d_allow_lds_impl((const void*)k.fn, (int)p.lds, &wgrad_lds_mask[p.family][0]);
  hipLaunchKernelGGL(k.fn, p.grid, dim3(p.threads), p.lds, s, (const u16*)in, (const u16*)dout, nbr, ld, (float*)workspace, n_out_dev, n_out_cap,
                     cin, cout, kvol, p.co_blocks);
  if (hipGetLastError() != hipSuccess) return U3D_ERR_LAUNCH;
  const long long n = (long long)kvol * cin * cout;
  if (p.reduce == WG_RED_ABK)
    hipLaunchKernelGGL(k_igemm_wgrad_reduce_abk, dim3(cin, u3d_cdiv(cout, 64), kvol > 9 ? 3 : 1), dim3(256), 0, s, (const float*)workspace, dw, n, p.nsplit, kvol, cin, cout);
  else if (p.reduce == WG_RED_OIK)
    hipLaunchKernelGGL(k_igemm_wgrad_reduce_oik, dim3(cin, u3d_cdiv(cout, 64), kvol > 9 ? 3 : 1), dim3(256), 0, s, (const float*)workspace, dw, n, p.nsplit, kvol, cin, cout);
  else
    hipLaunchKernelGGL(k_igemm_wgrad_reduce, dim3(u3d_cdiv(n / 4, 256)), dim3(256), 0, s, (const float*)workspace, dw, n, p.nsplit);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// dW_b = in_b^T @ dout_b for b < count, all [n_rows, cin] x [n_rows, cout] bf16 -> f32 [cin, cout] (deterministic row split + ordered
// reduce, as u3d_igemm_wgrad_bf16 with kvol = 1).  Two launches for the whole batch.
// plan for `count` same-shape products in one launch (the batched column of WGRAD_KERNELS; cin % 64 == 0 and cout % 64 == 0: the
// launch checks): the batch itself fills the chip, so prefer big tiles and few, long row splits - ceil(768 / workgroups per split)
// splits of at least 8 stages; below 192 workgroups half the tile, down to 64
static WgradPlan wgrad_plan_batched(int count, int n_rows, int cin, int cout) {
  const int mn = cin < cout ? cin : cout;
  int tile = (mn >= 256 && cin % 256 == 0 && cout % 256 == 0) ? 256 : ((mn >= 128 && cin % 128 == 0 && cout % 128 == 0) ? 128 : 64);
  const int ntiles = u3d_cdiv(n_rows > 0 ? n_rows : 1, 64);
  WgradPlan p;
  for (;;) {
    p.tile = tile;
    p.ci_blocks = u3d_cdiv(cin, tile);
    p.co_blocks = u3d_cdiv(cout, tile);
    const int per = (count > 0 ? count : 1) * p.ci_blocks * p.co_blocks;
    int ns = u3d_cdiv(768, per);
    int max_ns = ntiles / 8 > 0 ? ntiles / 8 : 1;
    if (ns > max_ns) ns = max_ns;
    if (ns < 1) ns = 1;
    p.nsplit = ns;
    if (tile == 64 || (long long)per * ns >= 192) break;
    tile /= 2;
  }
  wgrad_fill_tile(p, false, count);
  p.workspace = (int64_t)count * p.nsplit * cin * cout * 4;
  p.reduce = WG_RED_KIO;
  return p;
}
extern "C" int64_t u3d_wgrad_batched_workspace(int32_t count, int32_t n_rows, int32_t cin, int32_t cout) {
  return wgrad_plan_batched(count, n_rows, cin, cout).workspace;
}
extern "C" int32_t u3d_wgrad_batched_bf16(const void* const* in, const void* const* dout, float* const* dw, int32_t count,
                                          const int32_t* n_dev, int32_t n_rows, int32_t cin, int32_t cout, void* workspace,
                                          int64_t workspace_bytes, u3d_stream s) {
  U3D_REQUIRE(in && dout && dw && n_dev && workspace && count >= 0 && count <= U3D_WGRAD_BATCH_MAX, U3D_ERR_ARG);
  if (count == 0) return U3D_OK;
  if (cin % 64 != 0 || cout % 64 != 0) return U3D_ERR_UNSUPPORTED;
  const WgradPlan p = wgrad_plan_batched(count, n_rows, cin, cout);
  U3D_REQUIRE(workspace_bytes >= p.workspace, U3D_ERR_WORKSPACE);
  WgradBatch bt;
  for (int i = 0; i < count; ++i) { bt.in[i] = (const u16*)in[i]; bt.dout[i] = (const u16*)dout[i]; bt.dw[i] = dw[i]; }
  for (int i = count; i < U3D_WGRAD_BATCH_MAX; ++i) { bt.in[i] = nullptr; bt.dout[i] = nullptr; bt.dw[i] = nullptr; }
  const long long n = (long long)cin * cout, stride = (long long)p.nsplit * n;
  const wgrad_batch_kernel_t fn = WGRAD_KERNELS[p.family].batch;
  if (p.lds > 64 * 1024) u3d_allow_lds_impl((const void*)fn, (int)p.lds, &wgrad_lds_mask[p.family][1]);
  hipLaunchKernelGGL(fn, p.grid, dim3(p.threads), p.lds, s, bt, (float*)workspace, n_dev, n_rows, cin, cout, p.co_blocks, stride);
  WgradGroups gr;
  for (int i = 0; i < U3D_WGRAD_BATCH_MAX; ++i) gr.mult[i] = 0;
  for (int i = 0, lead = 0; i < count; ++i) {
    if (i > 0 && dw[i] == dw[i - 1]) { gr.mult[lead]++; } else { lead = i; gr.mult[i] = 1; }
  }
  hipLaunchKernelGGL(k_wgrad_batch_reduce, dim3(u3d_cdiv(n / 4, 256), count), dim3(256), 0, s, bt, gr, (const float*)workspace, n, p.nsplit, stride);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
