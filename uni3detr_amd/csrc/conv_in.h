// The encoder's 8 -> 16 input convolution (conv_in.hip): shape test and launches, shared with the forward entry of igemm_bf16.hip and
// the weight-gradient plan of igemm_wgrad.hip.
#pragma once
#include "common.h"

#define CONVIN_CIN 8
#define CONVIN_COUT 16
#define CONVIN_MAXK 27
#define CONVIN_WG_ROWS 128          /* rows per workgroup of the weight-gradient kernel */

static inline bool convin_shape(int cin, int cout, int kvol) { return cin == CONVIN_CIN && cout == CONVIN_COUT && kvol >= 1 && kvol <= CONVIN_MAXK; }
// partials of the weight gradient (one per workgroup): workspace f32 [blocks][kvol * 8 * 16]
static inline int convin_wgrad_blocks(int n_out_cap) { return u3d_cdiv(n_out_cap > 0 ? n_out_cap : 1, CONVIN_WG_ROWS); }

// out bf16 [n_out_cap][16] = conv(in bf16 [.][8]; w bf16 [kvol][8][16]); nbr NULL: kvol == 1, row m reads row m
int u3d_launch_conv_in_fwd(const void* in, const void* w, const int32_t* nbr, int ld, void* out, const int32_t* n_out_dev, int n_out_cap,
                           int kvol, hipStream_t s);
// dw f32 [kvol][8][16]; workspace: convin_wgrad_blocks(n_out_cap) partials
int u3d_launch_conv_in_wgrad(const void* in, const void* dout, const int32_t* nbr, int ld, float* dw, const int32_t* n_out_dev, int n_out_cap,
                             int kvol, float* workspace, hipStream_t s);
