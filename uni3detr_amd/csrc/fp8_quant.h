// f32 -> OCP e4m3fn (gfx950's fp8; never the fnuz encoding), saturating, round to nearest even.  Plain integer code, host and device:
// the quantiser of the fp8 inference path (fp8.hip) is this one function, so a CPU program can walk it against a reference bit for bit.
//   |v| >= 448 (Inf included) -> +-448 (0x7e / 0xfe);  NaN -> 0x7f / 0xff;  +-0 -> 0x00 / 0x80;
//   |v| <  2^-6: subnormal codes, step 2^-9 (2^-10 ties to 0, 2^-9 is code 1);  else 3 mantissa bits, ties to even.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define U3D_HD __host__ __device__ __forceinline__
#else
#define U3D_HD static inline
#endif

U3D_HD uint32_t u3d_e4m3_from_bits(uint32_t u) {
  const uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7fffffffu;
  if (a > 0x7f800000u) return sign | 0x7fu;               // NaN
  if (a >= 0x43e00000u) return sign | 0x7eu;              // >= 448: saturate
  if (a < 0x3c800000u) {                                  // < 2^-6: code = rne(|v| * 2^9), 0 .. 8 (8 = 0x08 = 2^-6, the first normal)
    if (a < 0x3a800000u) return sign;                     // < 2^-10: below half a step
    // |v| = sig * 2^(E - 150) with the biased exponent E in [117, 120]
    const uint32_t sig = (a & 0x007fffffu) | 0x00800000u; // 1.m as a 24-bit integer, weight 2^(E - 150)
    const int sh = 141 - (int)(a >> 23);                  // |v| * 2^9 = sig * 2^(E - 141): shift right by 141 - E = 21 .. 24
    const uint32_t q = sig >> sh, rem = sig & ((1u << sh) - 1u), half = 1u << (sh - 1);
    return sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));
  }
  a += 0x7ffffu + ((a >> 20) & 1u);                       // round the 23-bit mantissa to 3 bits, ties to even (a carry moves the exponent)
  return sign | ((a >> 20) - ((127u - 7u) << 3));         // rebias 127 -> 7; at most 0x7e: everything >= 448 left above
}

U3D_HD uint32_t u3d_e4m3_from_f32(float v) {
  uint32_t u;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(v);
#else
  memcpy(&u, &v, 4);
#endif
  return u3d_e4m3_from_bits(u);
}
