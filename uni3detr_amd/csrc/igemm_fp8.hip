// FP8 (OCP e4m3fn) implicit-GEMM convolution for inference: e4m3 activations and weights, f32 accumulation, bf16 output.
//
//   out[m, n] = act( (sum_kappa sum_k  qa[nbr[kappa][m], k] * qw[kappa][n][k]) * colscale[n] + shift[n] )
//
// The schedule is igemm_glds8_body's (igemm_bf16.hip: 256 x 256 tile, eight phases, LDS-DMA staging, counted vmcnt waits, two wave
// rows one barrier apart) with a k-tile of 128 BYTES of channels: 128 e4m3 channels are byte for byte the 64 bf16 channels of that
// kernel's k-tile, so the LDS image (four 16 KiB pieces per k-tile, 128-byte rows), the source-side XOR swizzle, the LDS-DMA
// addressing and the fragment reads (two conflict-free ds_read_b128 per 16-row block) are unchanged.  What changes is the MFMA: ONE
// v_mfma_scale_f32_16x16x128_f8f6f4 consumes both 16-byte reads of a row (a lane's 32 bytes) where the bf16 kernel issued two
// 16x16x32 - it takes twice the cycles and covers four times the channels, so a k-tile costs the matrix pipe what it cost before and
// a layer has half as many k-tiles.  The block scales are E8M0 127 (= 1.0) in every byte: the non-scaled fp8 MFMA runs at the bf16
// rate and would buy nothing.  A and B fragments go through the same read function, so which channel sits in which (lane group,
// byte) is the same for both operands and the instruction's nominal k order does not matter (all block scales are equal).
#include "igemm_common.h"

typedef unsigned char u8;
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x8 __attribute__((ext_vector_type(8)));

#define F8_UNIT_SCALE 0x7f7f7f7f

// RB = 16-row blocks per wave and row half: 4 = the 256-row tile, 3 = a 192-row tile in the same LDS image (igemm_glds8_body).
// NBR = false: kvol == 1 without a neighbour table (row m reads row m); no index loads in the loop.
template <int RB, bool NBR>
__device__ __forceinline__ void igemm_fp8_glds8_body(const u8* __restrict__ in, const u8* __restrict__ w, const int* __restrict__ nbr,
                                                     int ld, u16* __restrict__ out, const int* __restrict__ n_out_dev, int n_out_cap,
                                                     int cin, int cout, int kvol, const float* __restrict__ colscale,
                                                     const float* __restrict__ shift, int relu) {
  constexpr int WAVES_N = 4, WM = 2 * RB, WN = 4;
  constexpr int BM = 64 * RB, BN = 256, BK = 128;         // BK: bytes = e4m3 channels per k-tile
  constexpr int PIECE = 128 * BK;                         // bytes of one piece (16 KiB)
  constexpr int STAGE = 4 * PIECE;                        // A0 | A1 | B0 | B1
  extern __shared__ __attribute__((aligned(16))) u8 smem8[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int tile = u3d_xcd_tile(blockIdx.x, (n_out + BM - 1) / BM);      // XCD-contiguous ranges of the LIVE tiles
  if (tile < 0) return;
  const int m0 = tile * BM;
  const int col0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;
  const int nstage = kvol * (cin / BK);

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, -1, 0x00020000);
  const unsigned row_bytes = (unsigned)cin;
  // loader role: LDS-DMA instruction u (0 / 1) of this wave fills piece rows (wv*2+u)*8 .. +7; lane = (row in group, 16-byte slot)
  const int lrow = lane >> 3, lslot = lane & 7;
  unsigned a_part16[2], w_voff[2][2];                     // [u], [piece t][u]
  int arow[2][2];                                         // tile row of (piece s, u); -1: a dead row of the 192-row tile
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (wv * 2 + u) * 8 + lrow;                // piece row 0..127
    a_part16[u] = (unsigned)(lslot ^ ((r >> 1) & 7)) * 16u;
#pragma unroll
    for (int sp = 0; sp < 2; ++sp) {
      arow[sp][u] = ((r & 63) < 16 * RB) ? (r >> 6) * (32 * RB) + sp * (16 * RB) + (r & 63) : -1;
      const int tc = (r >> 5) * 64 + sp * 32 + (r & 31);  // piece B_sp row r = tile column tc
      w_voff[sp][u] = (col0 + tc < cout) ? (unsigned)((col0 + tc) * cin) + a_part16[u] : 0xFFFFFFFFu;
    }
  }
  int idx_cur[2][2], idx_nxt[2][2];
  int mcl[2][2];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + (arow[sp][u] < 0 ? 0 : arow[sp][u]);
      mcl[sp][u] = m < n_out ? m : n_out - 1;
      idx_nxt[sp][u] = mcl[sp][u];
    }
  // (the index loads land in the loop-carried registers themselves and are requested and consumed within one loop trip: see
  //  igemm_glds8_body for what either mistake costs)
  auto load_idx_next = [&](int stage) {
    if constexpr (NBR) {
      const int* row = nbr + (long long)(stage % kvol) * ld;
#pragma unroll
      for (int sp = 0; sp < 2; ++sp)
#pragma unroll
        for (int u = 0; u < 2; ++u) idx_nxt[sp][u] = row[mcl[sp][u]];
    }
  };
  auto advance_idx = [&]() {
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
      for (int u = 0; u < 2; ++u) idx_cur[sp][u] = (arow[sp][u] >= 0 && m0 + arow[sp][u] < n_out) ? idx_nxt[sp][u] : -1;
  };
  auto issue_a = [&](int st, int buf, int sp) {           // piece A_sp of k-tile st
    const unsigned soff = (unsigned)((st / kvol) * BK);
    u8* dst = smem8 + buf * STAGE + sp * PIECE + wv * 2048;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned voff = idx_cur[sp][u] >= 0 ? (unsigned)idx_cur[sp][u] * row_bytes + a_part16[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(dst + u * 1024), 16, voff, soff, 0, 0);
    }
  };
  auto issue_b = [&](int st, int buf, int sp) {           // piece B_sp of k-tile st
    const unsigned soff = (unsigned)((st % kvol) * cin * cout + (st / kvol) * BK);
    u8* dst = smem8 + buf * STAGE + (2 + sp) * PIECE + wv * 2048;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_void_ptr)(dst + u * 1024), 16, w_voff[sp][u], soff, 0, 0);
  };
  // fragment of a 16-row block = the lane's 32 bytes of the MFMA operand: 16-byte parts g and 4 + g of row li (g = lane >> 4), each one
  // conflict-free ds_read_b128 under the source-side swizzle (a 16-lane group covers every bank once)
  const int g = lane >> 4, li = lane & 15, fsw = (lane >> 1) & 7;
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) foff[ks] = ((ks * 4 + g) ^ fsw) << 4;
  typedef const volatile i32x4 __attribute__((address_space(3))) * lds_vptr;
  auto frag = [&](const u8* rowp) {
    const i32x4 lo = *(lds_vptr)(rowp + foff[0]);
    const i32x4 hi = *(lds_vptr)(rowp + foff[1]);
    return (i32x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };
  i32x8 af[2][RB], bf[2][2];                              // A: [half][row block]; B: [half][col block]
#define F8_READ_A(BUF, SP)                                                                                   \
  {                                                                                                          \
    const u8* A_ = smem8 + (BUF) * STAGE + (SP) * PIECE + (wm * 64 + li) * BK;                               \
    _Pragma("unroll") for (int a = 0; a < RB; ++a) af[SP][a] = frag(A_ + a * 16 * BK);                       \
  }
#define F8_READ_B(BUF, SP)                                                                                   \
  {                                                                                                          \
    const u8* B_ = smem8 + (BUF) * STAGE + (2 + (SP)) * PIECE + (wn * 32 + li) * BK;                         \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) bf[SP][b] = frag(B_ + b * 16 * BK);                        \
  }
  // operands swapped as in the bf16 kernels: the MFMA produces the transposed 16 x 16 block, this lane ends up with 4 consecutive
  // output COLUMNS (4g .. 4g+3) of row li
#define F8_MMA(SA, SB)                                                                                       \
  {                                                                                                          \
    __builtin_amdgcn_s_setprio(1);                                                                           \
    _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                            \
      _Pragma("unroll") for (int a = 0; a < RB; ++a)                                                         \
        acc[(SA) * RB + a][(SB) * 2 + b] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(                 \
            bf[SB][b], af[SA][a], acc[(SA) * RB + a][(SB) * 2 + b], 0, 0, 0, F8_UNIT_SCALE, 0, F8_UNIT_SCALE); \
    __builtin_amdgcn_s_setprio(0);                                                                           \
  }
#define F8_BAR()                                  \
  {                                               \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);            \
  }
  // counted waits: the trip's index loads (NBR) sit between its first request and the end of phase 4, so the counts that let
  // "8 younger requests" pass in the table kernel are 4 lower without a table in phases 1 and 2
#define F8_VMCNT(N) __builtin_amdgcn_s_waitcnt(0x0F70 | (N))    /* vmcnt(N), N < 16: expcnt / lgkmcnt untouched */
  constexpr int VM12 = NBR ? 8 : 4;

  // prologue: indices of k-tiles 0, 1; all four pieces of k-tile 0; everything landed before the first read
  load_idx_next(0);
  advance_idx();
  issue_a(0, 0, 0); issue_b(0, 0, 0); issue_b(0, 0, 1); issue_a(0, 0, 1);
  load_idx_next(1 < nstage ? 1 : 0);
  advance_idx();
  F8_VMCNT(0);
  F8_BAR();
  F8_READ_A(0, 0)                                         // phase 4 reads the NEXT k-tile's first row half: the first one here
  if (wm == 1) F8_BAR();                                  // the second wave row runs one barrier behind the first
  for (int st = 0; st < nstage; ++st) {
    const int buf = st & 1;
    const int nx = st + 1 < nstage ? st + 1 : st;         // past the end: a harmless re-fetch into the buffer nobody reads again
    // ---- phase 1: quadrant (rows 0-63, cols 0-31)
    load_idx_next(st + 2 < nstage ? st + 2 : nstage - 1);
    __builtin_amdgcn_sched_barrier(0);
    F8_READ_B(buf, 0)
    issue_a(nx, buf ^ 1, 0);
    F8_VMCNT(VM12);                                       // B1 of this k-tile has landed (every wave's share after the barrier)
    F8_BAR();
    F8_MMA(0, 0)
    F8_BAR();
    // ---- phase 2: (rows 0-63, cols 32-63)
    F8_READ_B(buf, 1)
    issue_b(nx, buf ^ 1, 0);
    F8_VMCNT(VM12);                                       // A1 of this k-tile
    F8_BAR();
    F8_MMA(0, 1)
    F8_BAR();
    // ---- phase 3: (rows 64-127, cols 32-63)
    F8_READ_A(buf, 1)
    issue_b(nx, buf ^ 1, 1);
    F8_VMCNT(4);                                          // A0 of the next k-tile (read in phase 4)
    F8_BAR();
    F8_MMA(1, 1)
    F8_BAR();
    // ---- phase 4: (rows 64-127, cols 0-31): B0 is still in registers
    F8_READ_A(buf ^ 1, 0)
    issue_a(nx, buf ^ 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    advance_idx();                                        // (NBR: hipcc waits here for the indices requested in phase 1)
    F8_VMCNT(4);                                          // A0 and B0 of the next k-tile
    F8_BAR();
    F8_MMA(1, 0)
    F8_BAR();
  }
  if (wm == 0) F8_BAR();                                  // same number of barriers for both wave rows
  F8_VMCNT(0);                                            // the tail's re-fetch requests
  __syncthreads();
#undef F8_READ_A
#undef F8_READ_B
#undef F8_MMA
#undef F8_BAR
#undef F8_VMCNT

  // epilogue: acc[a][b][r] = C[row (wm*WM+a)*16 + li][col (wn*WN+b)*16 + 4g + r]; column scale, shift, ReLU, one rounding to bf16
#pragma unroll
  for (int b = 0; b < WN; ++b) {
    const int col = col0 + (wn * WN + b) * 16 + 4 * g;
    if (col >= cout) continue;                            // cout % 4 == 0: the 4-column group is in or out as a whole
    const f32x4 sc = *(const f32x4*)(colscale + col), sh = *(const f32x4*)(shift + col);
#pragma unroll
    for (int a = 0; a < WM; ++a) {
      const int m = m0 + (wm * WM + a) * 16 + li;
      if (m >= n_out) continue;
      f32x4 v = acc[a][b] * sc + sh;
      if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
      *(bf16x4*)(out + (long long)m * cout + col) = __builtin_convertvector(v, bf16x4);
    }
  }
}

#define U3D_FP8_KERNEL(NAME, RB, NBR)                                                                                           \
  __global__ __launch_bounds__(512) void NAME(const u8* in, const u8* w, const int* nbr, int ld, u16* out, const int* n_out_dev, \
                                              int n_out_cap, int cin, int cout, int kvol, const float* colscale,               \
                                              const float* shift, int relu) {                                                   \
    igemm_fp8_glds8_body<RB, NBR>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, colscale, shift, relu);           \
  }
U3D_FP8_KERNEL(k_igemm_fp8_glds8_256x256, 4, true)
U3D_FP8_KERNEL(k_igemm_fp8_glds8_192x256, 3, true)
U3D_FP8_KERNEL(k_igemm_fp8_glds8_256x256_rows, 4, false)
#undef U3D_FP8_KERNEL
typedef void (*fp8_kernel_t)(const u8*, const u8*, const int*, int, u16*, const int*, int, int, int, int, const float*, const float*, int);

// ---------------------------------------------------------------------------------------------
// The launch plan: which kernel serves a shape, asked (u3d_igemm_fwd_fp8_plan, host only) or followed (u3d_igemm_fwd_affine_fp8).
//   cin % 128 == 0 (a k-tile is 128 channels), cout % 128 == 0, and either kvol > 1 with a table or kvol == 1 without one.
//   0: 256 x 256 with a table, 1: 192 x 256 where 192-row tiles finish sooner on 256 CUs (the rule of the bf16 kernels), 2: 256 x 256
//   without a table.  A 128-column layer runs on the 256-column tile with its second half masked.
// ---------------------------------------------------------------------------------------------
struct Fp8Plan {
  int kernel = -1, rows = 0, cols = 256;
};
static const fp8_kernel_t FP8_KERNELS[U3D_FWD_FP8_K_COUNT] = {k_igemm_fp8_glds8_256x256, k_igemm_fp8_glds8_192x256,
                                                                  k_igemm_fp8_glds8_256x256_rows};

static Fp8Plan fp8_plan(int n_out_cap, int cin, int cout, int kvol, bool has_nbr) {
  Fp8Plan p;
  if (n_out_cap <= 0 || cin <= 0 || cout <= 0 || cin % 128 != 0 || cout % 128 != 0) return p;
  if (!((has_nbr && kvol > 1) || (!has_nbr && kvol == 1))) return p;
  if (!has_nbr) { p.kernel = U3D_FWD_FP8_K_256X256_ROWS, p.rows = 256; return p; }
  const int cb = u3d_cdiv(cout, 256);
  const long long w256 = (long long)u3d_cdiv(n_out_cap, 256) * cb, w192 = (long long)u3d_cdiv(n_out_cap, 192) * cb;
  const bool r192 = (double)u3d_cdiv(w192, 256) * 192.0 * 1.05 < (double)u3d_cdiv(w256, 256) * 256.0;    // igemm_rows192 of igemm_bf16.hip
  p.kernel = r192 ? U3D_FWD_FP8_K_192X256 : U3D_FWD_FP8_K_256X256, p.rows = r192 ? 192 : 256;
  return p;
}

extern "C" int32_t u3d_igemm_fwd_fp8_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr,
                                          int32_t* kernel, int32_t* rows, int32_t* cols) {
  U3D_REQUIRE(kernel && rows && cols, U3D_ERR_ARG);
  const Fp8Plan p = fp8_plan(n_out_cap, cin, cout, kvol, has_nbr != 0);
  if (p.kernel < 0) return U3D_ERR_UNSUPPORTED;
  *kernel = p.kernel, *rows = p.rows, *cols = p.cols;
  return U3D_OK;
}

extern "C" int32_t u3d_igemm_fwd_affine_fp8(const void* in, const void* qw, const int32_t* nbr, int32_t ld, const float* colscale,
                                            const float* shift, int32_t relu, void* out, const int32_t* n_out_dev, int32_t n_out_cap,
                                            int32_t cin, int32_t cout, int32_t kvol, u3d_stream s) {
  U3D_REQUIRE(in && qw && out && n_out_dev && colscale && shift && kvol > 0, U3D_ERR_ARG);
  if (n_out_cap <= 0) return (cin > 0 && cout > 0 && cin % 128 == 0 && cout % 128 == 0) ? U3D_OK : U3D_ERR_UNSUPPORTED;
  const Fp8Plan p = fp8_plan(n_out_cap, cin, cout, kvol, nbr != nullptr);
  if (p.kernel < 0) return U3D_ERR_UNSUPPORTED;
  static unsigned long long lds_mask[U3D_FWD_FP8_K_COUNT] = {};
  constexpr int LDS = 2 * 4 * 128 * 128;                  // two k-tiles of four 16 KiB pieces
  u3d_allow_lds_impl((const void*)FP8_KERNELS[p.kernel], LDS, &lds_mask[p.kernel]);
  hipLaunchKernelGGL(FP8_KERNELS[p.kernel], dim3(u3d_cdiv(n_out_cap, p.rows), u3d_cdiv(cout, p.cols)), dim3(512), LDS, (hipStream_t)s,
                     (const u8*)in, (const u8*)qw, nbr, ld, (u16*)out, n_out_dev, n_out_cap, cin, cout, kvol, colscale, shift,
                     relu ? 1 : 0);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
