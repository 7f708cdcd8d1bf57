// Vector types and LDS fragment helpers shared by the bf16 implicit-GEMM units (igemm_bf16.hip: forward / input gradient,
// igemm_wgrad.hip: weight gradient, split_bf16.hip, conv_in.hip).
#pragma once
#include "common.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef unsigned short u16;
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

typedef __attribute__((address_space(3))) void* lds_void_ptr;   // destination of an LDS-DMA load (buffer_load ... lds)
#define LDS_PTR(p) ((s16x4 __attribute__((address_space(3)))*)(p))

// f32 -> bf16, round to nearest even (NaN stays NaN)
__device__ __forceinline__ u16 f2bf(float f) {
  unsigned u = __float_as_uint(f);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (u16)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (u16)(u >> 16);
}

// 8 reduction-index values for one MFMA operand, reduction index = LDS row.  tile: row-major, `stride` elements per
// row; returns values (rows k0 + r(g,e), column c0 + (lane&15)), r(g,e) = e<4 ? 4g+e : 16+4g+(e-4), g = lane>>4.
__device__ __forceinline__ bf16x8 tr_frag(const u16* tile, int stride, int k0, int c0, int lane) {
  const int g = lane >> 4, L = lane & 15, j = L >> 2, q = L & 3;
  const u16* p0 = tile + (k0 + 4 * g + j) * stride + c0 + 4 * q;
  s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0));
  s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16(LDS_PTR(p0 + 16 * stride));
  s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}
