// =============================================================================================
// The encoder's input convolution: 4 point features (padded to 8) -> 16 channels, 27 offsets, ~128 k rows
// (ref: sparse_encoder_hd.py:80-88).  0.9 GFLOP: far too small for a tiled MFMA kernel (the first-generation kernel spent 166 us on
// it, its weight gradient 126 us) - plain VALU, one thread per output row, weights (27 x 8 x 16 f32 = 13.5 KB) in LDS read by
// broadcast; rows without a neighbour at an offset skip it (6 % of the (offset,row) pairs exist at this level).
// =============================================================================================
#include "conv_in.h"
#include "igemm_common.h"

__device__ __forceinline__ float convin_bf(u16 v) { return __uint_as_float((unsigned)v << 16); }

__global__ __launch_bounds__(256) void k_conv_in_fwd(const u16* __restrict__ in, const u16* __restrict__ w, const int* __restrict__ nbr,
                                                     int ld, u16* __restrict__ out, const int* __restrict__ n_out_dev, int n_out_cap,
                                                     int kvol) {
  __shared__ __attribute__((aligned(16))) float ws[CONVIN_MAXK * CONVIN_CIN * CONVIN_COUT];
  for (int i = threadIdx.x; i < kvol * CONVIN_CIN * CONVIN_COUT; i += 256) ws[i] = convin_bf(w[i]);
  __syncthreads();
  const int n = min(*n_out_dev, n_out_cap);
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= n) return;
  float acc[CONVIN_COUT];
#pragma unroll
  for (int co = 0; co < CONVIN_COUT; ++co) acc[co] = 0.f;
  int idxs[CONVIN_MAXK];                       // all offsets' indices first: 27 independent loads in flight, not 27 round trips
#pragma unroll
  for (int k = 0; k < CONVIN_MAXK; ++k) idxs[k] = k < kvol ? (nbr ? nbr[(long long)k * ld + m] : m) : -1;
#pragma unroll
  for (int k = 0; k < CONVIN_MAXK; ++k) {
    const int idx = idxs[k];
    if (idx < 0) continue;
    const uint4 xv = *(const uint4*)(in + (long long)idx * CONVIN_CIN);
    const unsigned xw[4] = {xv.x, xv.y, xv.z, xv.w};
    const float* wk = ws + k * CONVIN_CIN * CONVIN_COUT;
#pragma unroll
    for (int ci = 0; ci < CONVIN_CIN; ++ci) {
      const float x = (ci & 1) ? __uint_as_float(xw[ci >> 1] & 0xffff0000u) : __uint_as_float(xw[ci >> 1] << 16);
#pragma unroll
      for (int q = 0; q < CONVIN_COUT / 4; ++q) {
        const float4 wv = *(const float4*)(wk + ci * CONVIN_COUT + q * 4);
        acc[q * 4 + 0] += x * wv.x; acc[q * 4 + 1] += x * wv.y; acc[q * 4 + 2] += x * wv.z; acc[q * 4 + 3] += x * wv.w;
      }
    }
  }
  typedef float f32x8_t __attribute__((ext_vector_type(8)));
  typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    f32x8_t f = {acc[h * 8], acc[h * 8 + 1], acc[h * 8 + 2], acc[h * 8 + 3], acc[h * 8 + 4], acc[h * 8 + 5], acc[h * 8 + 6], acc[h * 8 + 7]};
    *(bf16x8_t*)(out + (long long)m * CONVIN_COUT + h * 8) = __builtin_convertvector(f, bf16x8_t);
  }
}

// weight gradient: dW[k][ci][:] = sum_rows in[nbr[k][row]][ci] * dout[row][:].  A workgroup owns CONVIN_WG_ROWS output rows (their
// dout staged in LDS), thread (k, ci) walks them branch-free (absent neighbour -> factor 0) with the index and input loads of
// several rows in flight; per-workgroup partials [blocks][K*8*16] are summed in order by k_conv_in_reduce.
__global__ __launch_bounds__(256) void k_conv_in_wgrad(const u16* __restrict__ in, const u16* __restrict__ dout, const int* __restrict__ nbr,
                                                       int ld, float* __restrict__ partial, const int* __restrict__ n_out_dev,
                                                       int n_out_cap, int kvol) {
  __shared__ __attribute__((aligned(16))) u16 dys[CONVIN_WG_ROWS * CONVIN_COUT];
  const int n = min(*n_out_dev, n_out_cap);
  const int r0 = blockIdx.x * CONVIN_WG_ROWS;
  const int r1 = min(n, r0 + CONVIN_WG_ROWS);
  for (int i = threadIdx.x; i < CONVIN_WG_ROWS * 2; i += 256) {
    const int row = r0 + (i >> 1);
    uint4 v = {0u, 0u, 0u, 0u};
    if (row < r1) v = *(const uint4*)(dout + (long long)row * CONVIN_COUT + (i & 1) * 8);
    *(uint4*)(dys + (i >> 1) * CONVIN_COUT + (i & 1) * 8) = v;
  }
  __syncthreads();
  const int k = threadIdx.x >> 3, ci = threadIdx.x & 7;
  if (k >= kvol) return;
  float acc[CONVIN_COUT];
#pragma unroll
  for (int co = 0; co < CONVIN_COUT; ++co) acc[co] = 0.f;
  const int* nk = nbr ? nbr + (long long)k * ld : nullptr;
  for (int rb = r0; rb < r1; rb += 8) {
    int idx8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) idx8[j] = (rb + j < r1) ? (nk ? nk[rb + j] : rb + j) : -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
    const int r = rb + j, idx = idx8[j];
    if (__builtin_amdgcn_ballot_w64(idx >= 0) == 0) continue;       // none of this wave's 8 offsets has a neighbour for row r (most rows)
    const float x = idx >= 0 ? convin_bf(in[(long long)idx * CONVIN_CIN + ci]) : 0.f;
    const uint4 a = *(const uint4*)(dys + (r - r0) * CONVIN_COUT), b = *(const uint4*)(dys + (r - r0) * CONVIN_COUT + 8);
    const unsigned dw_[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      acc[2 * q] += x * __uint_as_float(dw_[q] << 16);
      acc[2 * q + 1] += x * __uint_as_float(dw_[q] & 0xffff0000u);
    }
    }
  }
  float* p = partial + (long long)blockIdx.x * (kvol * CONVIN_CIN * CONVIN_COUT) + (k * CONVIN_CIN + ci) * CONVIN_COUT;
#pragma unroll
  for (int q = 0; q < 4; ++q) *(float4*)(p + q * 4) = make_float4(acc[q * 4], acc[q * 4 + 1], acc[q * 4 + 2], acc[q * 4 + 3]);
}
// few outputs (K*8*16 = 3456), many partials (one per 128 rows): 64 columns x 16 partial-lanes per workgroup, fixed order
__global__ __launch_bounds__(1024) void k_conv_in_reduce(const float* __restrict__ partial, float* __restrict__ dw, int n, int nsplit) {
  __shared__ float red[16][64];
  const int c = threadIdx.x & 63, lane = threadIdx.x >> 6, col = blockIdx.x * 64 + c;
  float a = 0.f, b = 0.f, cc = 0.f, d = 0.f;
  if (col < n) {
    const float* p = partial + col;
    int k = lane;
    for (; k + 48 < nsplit; k += 64) {
      a += p[(long long)k * n]; b += p[(long long)(k + 16) * n]; cc += p[(long long)(k + 32) * n]; d += p[(long long)(k + 48) * n];
    }
    for (; k < nsplit; k += 16) a += p[(long long)k * n];
  }
  red[lane][c] = (a + b) + (cc + d);
  __syncthreads();
  if (threadIdx.x < 64 && col < n) {
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 16; ++j) s += red[j][threadIdx.x];
    dw[col] = s;
  }
}

int u3d_launch_conv_in_fwd(const void* in, const void* w, const int32_t* nbr, int ld, void* out, const int32_t* n_out_dev, int n_out_cap,
                           int kvol, hipStream_t s) {
  if (n_out_cap <= 0) return U3D_OK;
  hipLaunchKernelGGL(k_conv_in_fwd, dim3(u3d_cdiv(n_out_cap, 256)), dim3(256), 0, s, (const u16*)in, (const u16*)w, nbr, ld, (u16*)out, n_out_dev,
                     n_out_cap, kvol);
  return hipGetLastError() == hipSuccess ? U3D_OK : U3D_ERR_LAUNCH;
}

int u3d_launch_conv_in_wgrad(const void* in, const void* dout, const int32_t* nbr, int ld, float* dw, const int32_t* n_out_dev, int n_out_cap,
                             int kvol, float* workspace, hipStream_t s) {
  const int nb = convin_wgrad_blocks(n_out_cap), nw = kvol * CONVIN_CIN * CONVIN_COUT;
  hipLaunchKernelGGL(k_conv_in_wgrad, dim3(nb), dim3(256), 0, s, (const u16*)in, (const u16*)dout, nbr, ld, workspace, n_out_dev, n_out_cap, kvol);
  hipLaunchKernelGGL(k_conv_in_reduce, dim3(u3d_cdiv(nw, 64)), dim3(1024), 0, s, (const float*)workspace, dw, nw, nb);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
