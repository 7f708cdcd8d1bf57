// bf16 implicit-GEMM convolution kernels, second generation (large tiles, double-buffered LDS, register-staged
// prefetch, LDS transpose reads): the forward / input-gradient half and its launch plan.  The weight gradient is igemm_wgrad.hip,
// the encoder's 8 -> 16 input convolution conv_in.hip, the split-bf16 operand helpers split_bf16.hip.  The kernels serve BOTH the
// sparse levels and the dense SECOND3D/FPN lattice: the only difference is where the neighbour table comes from.
//
//   forward / dgrad :  out[m, n] = sum_kappa sum_k  in[nbr[kappa][m], k] * W[kappa](k, n)
//
// MFMA: v_mfma_f32_16x16x32_bf16, f32 accumulation.  Tiles up to 256x256 per workgroup (8 waves) so that the
// L2->CU traffic per MFMA cycle stays below ~36 B/clk (a 128x128 tile would need ~64 B/clk: DESIGN.md §kernels).
// Operands whose reduction index is the LDS row (the k-major W[k][n]) are fetched with
// ds_read_b64_tr_b16; rows are padded by 16 elements so that those reads are bank-conflict free.
#include "igemm_common.h"
#include "conv_in.h"
#include "igemm_direct.h"

#ifndef IGEMM_SMALL_WM
#define IGEMM_SMALL_WM 4   /* 16-row blocks per wave: 4 waves x 4 = 256-row tiles */
#endif
#ifndef GLDS256_CFG
#define GLDS256_CFG 2, 4, 8, 4   /* waves (rows x cols) and 16x16 blocks per wave (rows x cols) of the 256x256-tile LDS-DMA kernel */
#endif
#ifndef GLDS_DMA_SPREAD
#define GLDS_DMA_SPREAD 2   /* 1: one LDS-DMA instruction behind each MFMA group of the stage, 2: all of them within the first k-step */
#endif
#ifndef GLDS_FRAG_B128
#define GLDS_FRAG_B128 1   /* fragments as one ds_read_b128 per lane (0: two ds_read_b64 in the instruction's nominal k-order) */
#endif
#ifndef IGEMM_STORE_KS
#define IGEMM_STORE_KS 0   /* k-step after which the next stage's registers are written to LDS (0: mid-stage, 1: end of stage) */
#endif

// 8 reduction-index values, reduction index contiguous in the LDS row: row r0 + (lane&15), elements k0 + kmap(g,e) with the
// SAME r(g,e) permutation as tr_frag (so a tr operand and a direct operand can be paired in one MFMA).
__device__ __forceinline__ bf16x8 direct_frag(const u16* tile, int stride, int r0, int k0, int lane) {
  const int g = lane >> 4, i = lane & 15;
  const u16* p = tile + (r0 + i) * stride + k0 + 4 * g;
  // two SEPARATE ds_read_b64 (volatile keeps hipcc from fusing them into ds_read2_b64, whose 16-lane groups / mod-32 banking
  // put rows r and r+8 of the 36-dword-stride tile on the same banks: PMC showed SQ_LDS_BANK_CONFLICT = 36 % of LDS cycles)
  typedef const volatile s16x4 __attribute__((address_space(3))) * lds_vptr;
  s16x4 a = *(lds_vptr)(p);
  s16x4 b = *(lds_vptr)(p + 16);
  s16x8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
  return __builtin_bit_cast(bf16x8, v);
}

// =============================================================================================
// forward / dgrad
//   tile BM x BN, BM = WAVES_M*WM*16, BN = WAVES_N*WN*16, BK = 64 reduction elements per stage.
//   W_KMAJOR = true : global W[kappa][k][n]  (forward; staged row-major [k][n], fetched with transpose reads)
//   W_KMAJOR = false: global W[kappa][n][k]  (dgrad: the forward weight read transposed; staged [n][k], direct reads)
// =============================================================================================
template <int WAVES_M, int WAVES_N, int WM, int WN, bool W_KMAJOR, int BK = 64>
__global__ __launch_bounds__(WAVES_M* WAVES_N * 64) void k_igemm_fwd(const u16* __restrict__ in, const u16* __restrict__ w,
                                                                      const int* __restrict__ nbr, int ld, u16* __restrict__ out,
                                                                      const int* __restrict__ n_out_dev, int n_out_cap, int cin,
                                                                      int cout, int kvol, const float* __restrict__ bias, int relu) {
  constexpr int NT = WAVES_M * WAVES_N * 64;
  constexpr int BM = WAVES_M * WM * 16, BN = WAVES_N * WN * 16;   // BK = 64, or 32 for the 16/32-channel sparse levels (one MFMA k-step)
  constexpr int LDA = BK + 8;                           // A tile [BM][BK] (k contiguous): 36- / 20-dword stride -> conflict-free b64 reads
  constexpr int LDW = W_KMAJOR ? BN + 16 : BK + 8;      // W tile [BK][BN] (transpose reads: +16) or [BN][BK] (direct: +8)
  constexpr int A_ELEMS = BM * LDA;
  constexpr int W_ELEMS = W_KMAJOR ? BK * LDW : BN * LDW;
  constexpr int A_SEGS = BM * (BK / 8) / NT;            // 16-byte segments per thread per stage
  constexpr int W_TOTAL = BK * BN / 8;                  // 16-byte segments of the W tile; small tiles leave some threads without one
  constexpr int W_SEGS = (W_TOTAL + NT - 1) / NT;
  static_assert(BM * (BK / 8) % NT == 0 && (BK == 64 || BK == 32), "tile/thread mismatch");
  extern __shared__ __attribute__((aligned(16))) u16 smem[];
  constexpr int STAGE_ELEMS = A_ELEMS + W_ELEMS;        // buffer b: A at smem + b*STAGE_ELEMS, W right behind it

  const int n_out = min(*n_out_dev, n_out_cap);
  // XCD-aware tile order: workgroup b runs on XCD b % 8 (observed dispatch rule; used for speed only).  Every XCD gets one
  // CONTIGUOUS slab of row tiles, so the halo rows a tile re-gathers for its 27 offsets are shared through that XCD's L2
  // instead of being pulled into all eight L2s.  (Measured: time-neutral on the 3x3x3 layers — they are MFMA-pipeline bound.)
  const int tile = u3d_xcd_tile(blockIdx.x, (n_out + BM - 1) / BM);      // XCD-contiguous ranges of the LIVE tiles (capacity-sized grids)
  if (tile < 0) return;
  const int m0 = tile * BM;
  const int col0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;
  const int kchunks = (cin + BK - 1) / BK;              // cin % 16 == 0 (dispatch); a short last chunk is zero-filled
  const int nstage = kvol * kchunks;

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  // Operand fetch = raw buffer loads (32-bit byte offsets, scalar stage offset, hardware zero fill for out-of-range offsets):
  // a missing neighbour is the offset 0xFFFFFFFF, so the whole stage body is ONE branch-free basic block and the scheduler can
  // interleave the next stage's address arithmetic / loads with this stage's MFMAs (with per-load `if (idx >= 0)` branches the
  // ~230 VALU/SALU instructions of the load section ran with the matrix pipe idle: ISA + SQ counters in DESIGN.md §kernels).
  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, -1, 0x00020000);
  const unsigned row_bytes = (unsigned)cin * 2u;
  const unsigned a_part16 = (unsigned)(tid % (BK / 8)) * 16u;          // NT % (BK/8) == 0: the same 16-byte part for every segment
  const int a_row0 = tid / (BK / 8);                                   // segment u covers row a_row0 + u * (NT / (BK/8))
  constexpr int A_ROW_STEP = NT / (BK / 8);
  unsigned w_voff[W_SEGS];
  int w_k[W_SEGS];                                      // reduction index (within the chunk) of the segment's first element
#pragma unroll
  for (int u = 0; u < W_SEGS; ++u) {
    int sgi = tid + u * NT;
    const bool live = sgi < W_TOTAL;
    if (W_KMAJOR) {
      int k = sgi / (BN / 8), part = sgi % (BN / 8);
      int n = col0 + part * 8;
      w_k[u] = k;
      w_voff[u] = (live && n < cout) ? (unsigned)(k * cout + n) * 2u : 0xFFFFFFFFu;
    } else {
      int n = sgi / (BK / 8), part = sgi % (BK / 8);
      w_k[u] = part * 8;
      w_voff[u] = (live && col0 + n < cout) ? (unsigned)((col0 + n) * cin + part * 8) * 2u : 0xFFFFFFFFu;
    }
  }

  u32x4 ra[A_SEGS], rw[W_SEGS];
  int idx_cur[A_SEGS], idx_nxt[A_SEGS];

  // Stage order: channel chunk OUTER, kernel offset INNER (stage st = chunk st / kvol, offset st % kvol).  Within one chunk
  // round a tile re-reads the same 128-byte row pieces for all kvol offsets (its 3x3x3 halo window, ~130 KB), so the window of
  // the ~32 tiles an XCD runs at a time (~1.5 MB) stays in that XCD's 4 MB L2; with the offset outer, the re-reads of a row
  // for the next dy / dz offsets came 12 / 36 stages (12 / 37 MB of other traffic per XCD) later and went back to MALL/HBM.
  // The neighbour indices of stage st+2 are fetched while stage st computes: the idx -> row gather chain (two dependent
  // L2 round trips) must never sit in front of a stage.
  auto load_idx_next = [&](int stage) {
    const int kap = stage % kvol;
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) {
      int m = m0 + a_row0 + u * A_ROW_STEP;
      int mc = m < n_out ? m : n_out - 1;                              // clamped, branch-free (n_out >= 1 here)
      // the loaded value is NOT touched here: any use (even a select) makes the compiler wait for it on the spot, and
      // vmcnt is in-order - that wait would also cover the stage loads issued just before it (measured: the whole L2
      // latency exposed once per stage).  Rows past n_out are masked when the index is consumed (advance_idx).
      idx_nxt[u] = nbr ? nbr[(long long)kap * ld + mc] : mc;
    }
  };
  auto advance_idx = [&]() {
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) idx_cur[u] = (m0 + a_row0 + u * A_ROW_STEP < n_out) ? idx_nxt[u] : -1;
  };
  auto issue_loads = [&](int st) {
    const int kap = st % kvol, c0 = (st / kvol) * BK;
    const unsigned a_soff = (unsigned)c0 * 2u;
    const bool a_in = BK == 64 || (c0 + (int)(a_part16 >> 1) < cin);   // BK = 32 with cin = 16: the upper half of the chunk is zero
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) {
      unsigned voff = (idx_cur[u] >= 0 && a_in) ? (unsigned)idx_cur[u] * row_bytes + a_part16 : 0xFFFFFFFFu;
#ifdef IGEMM_EXP_SKIP_A
      if (st > 0) continue;
#endif
      ra[u] = __builtin_amdgcn_raw_buffer_load_b128(in_rs, voff, a_soff, 0);
    }
    const unsigned w_soff = W_KMAJOR ? (unsigned)((kap * cin + c0) * cout) * 2u : (unsigned)(kap * cin * cout + c0) * 2u;
#ifdef IGEMM_EXP_SKIP_W
    if (st > 0) return;
#endif
#pragma unroll
    for (int u = 0; u < W_SEGS; ++u) {
      const unsigned vo = (BK == 64 || c0 + w_k[u] < cin) ? w_voff[u] : 0xFFFFFFFFu;
      rw[u] = __builtin_amdgcn_raw_buffer_load_b128(w_rs, vo, w_soff, 0);
    }
  };
  auto store_lds = [&](int buf) {
    u16* Ab = smem + buf * STAGE_ELEMS;
    u16* Wb = Ab + A_ELEMS;
#pragma unroll
    for (int u = 0; u < A_SEGS; ++u) *(u32x4*)(Ab + (a_row0 + u * A_ROW_STEP) * LDA + (tid % (BK / 8)) * 8) = ra[u];
#pragma unroll
    for (int u = 0; u < W_SEGS; ++u) {
      int sgi = tid + u * NT;
      if (sgi >= W_TOTAL) continue;
      if (W_KMAJOR) { int k = sgi / (BN / 8), part = sgi % (BN / 8); *(u32x4*)(Wb + k * LDW + part * 8) = rw[u]; }
      else { int n = sgi / (BK / 8), part = sgi % (BK / 8); *(u32x4*)(Wb + n * LDW + part * 8) = rw[u]; }
    }
  };

  load_idx_next(0);
  advance_idx();
  load_idx_next(1);
  issue_loads(0);
  store_lds(0);
  __syncthreads();
  for (int st = 0; st < nstage; ++st) {
    const int buf = st & 1;
    // the last stage re-fetches itself into the idle buffer (never read): no "is there a next stage" branch in the body
    const int nx = st + 1 < nstage ? st + 1 : st;
    advance_idx();                                      // indices of stage st+1 (fetched a whole stage ago)
    load_idx_next(st + 2 < nstage ? st + 2 : nstage - 1);
    issue_loads(nx);                                    // global loads in flight while this stage computes
    const u16* A = smem + buf * STAGE_ELEMS;
    const u16* W = A + A_ELEMS;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      bf16x8 af[WM];
#pragma unroll
      for (int a = 0; a < WM; ++a) af[a] = direct_frag(A, LDA, (wm * WM + a) * 16, ks * 32, lane);
#pragma unroll
      for (int b = 0; b < WN; ++b) {
        bf16x8 bfr = W_KMAJOR ? tr_frag(W, LDW, ks * 32, (wn * WN + b) * 16, lane)
                              : direct_frag(W, LDW, (wn * WN + b) * 16, ks * 32, lane);
#pragma unroll
        for (int a = 0; a < WM; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bfr, acc[a][b], 0, 0, 0);
      }
      // the next stage's tile goes to the OTHER buffer (free since the previous barrier)
#ifndef IGEMM_EXP_SKIP_STORE
      if (ks == IGEMM_STORE_KS) store_lds(buf ^ 1);
#endif
    }
    __syncthreads();
  }
  // epilogue: C/D layout col = lane&15, row = (lane>>4)*4 + r
  const int li = lane & 15, g = lane >> 4;
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      int m = m0 + (wm * WM + a) * 16 + g * 4 + r;
      if (m >= n_out) continue;
#pragma unroll
      for (int b = 0; b < WN; ++b) {
        int col = col0 + (wn * WN + b) * 16 + li;
        if (col < cout) {
          float v = acc[a][b][r];
          if (bias) v += bias[col];
          if (relu) v = fmaxf(v, 0.f);
          out[(long long)m * cout + col] = f2bf(v);
        }
      }
    }
}

// The instantiations fwd_plan launches: kernel, tile BM x BN, threads, and the dynamic LDS of the kernel's two stages of
// (A tile [BM][BK + 8]) + (W tile [BK][BN + 16] k-major or [BN][BK + 8] n-major).
typedef void (*reg_kernel_t)(const u16*, const u16*, const int*, int, u16*, const int*, int, int, int, int, const float*, int);
struct RegKernel {
  reg_kernel_t fn;
  int rows, cols, threads;
  size_t lds;
};
#define REG_KERNEL(A, B, C, D, WK, BK)                                      \
  {k_igemm_fwd<A, B, C, D, WK, BK>, A * C * 16, B * D * 16, A * B * 64,     \
   (size_t)2 * (A * C * 16 * (BK + 8) + (WK ? BK * (B * D * 16 + 16) : B * D * 16 * (BK + 8))) * 2}
// R_N<cout>_<K|N>: the 16/32-channel sparse levels (and the 32 -> 64 transition), 256-row tiles, one MFMA k-step per stage (BK = 32),
// k-major / n-major weights; R_<tile>: the k-major wide layers
enum { R_N16_K, R_N16_N, R_N32_K, R_N32_N, R_N64_K, R_N64_N, R_256x256, R_256x128, R_128x64, R_COUNT };
static const RegKernel REG_KERNELS[R_COUNT] = {
    REG_KERNEL(4, 1, IGEMM_SMALL_WM, 1, true, 32), REG_KERNEL(4, 1, IGEMM_SMALL_WM, 1, false, 32),
    REG_KERNEL(4, 1, IGEMM_SMALL_WM, 2, true, 32), REG_KERNEL(4, 1, IGEMM_SMALL_WM, 2, false, 32),
    REG_KERNEL(4, 1, IGEMM_SMALL_WM, 4, true, 32), REG_KERNEL(4, 1, IGEMM_SMALL_WM, 4, false, 32),
    REG_KERNEL(2, 4, 8, 4, true, 64),
    REG_KERNEL(4, 2, 4, 4, true, 64),
    REG_KERNEL(4, 1, 2, 4, true, 64),      // 128 x 64: 57 KB LDS -> 2 workgroups per CU hide the gather latency
};
#undef REG_KERNEL

// =============================================================================================
// forward / dgrad with LDS-DMA staging (256 x 256 tile, n-major weights w[kappa][n][k]).
//
// Ablation of k_igemm_fwd (tools/conv_bench.py): without the register->LDS stores of the next stage it runs at 1.2-1.4 PFLOP/s
// instead of 0.9 - the ds_write_b128 stream (13 clk each on the shared VGPR->LDS path, behind a vmcnt wait) is its largest
// overhead; and the k-major weight tile (transpose reads) costs another ~15 % against the n-major one.  Here both operand tiles go
// global -> LDS with `buffer_load_dwordx4 ... lds` (no staging registers, no ds_write, zero fill for missing neighbours by an
// out-of-range offset), issued at the top of a stage into the idle buffer and in flight during the whole stage.  LDS-DMA writes
// lane-linearly (1 KiB per wave-instruction = 8 rows x 128 B), so the tiles are unpadded [256][64] and bank conflicts are avoided
// by an XOR swizzle applied on the SOURCE side: 16-byte part p of row r is stored in slot p ^ ((r >> 1) & 7); a fragment read
// (16 rows x 8 B per k-group) then covers all 64 banks exactly once.
// =============================================================================================

template <int WAVES_M, int WAVES_N, int WM, int WN, bool F32OUT = false>
__device__ __forceinline__ void igemm_glds_body(const u16* __restrict__ in, const u16* __restrict__ w, const int* __restrict__ nbr,
                                                int ld, u16* __restrict__ out, const int* __restrict__ n_out_dev, int n_out_cap,
                                                int cin, int cout, int kvol, const float* __restrict__ bias, int relu,
                                                double* __restrict__ stats) {
  constexpr int NW = WAVES_M * WAVES_N;
  constexpr int BM = WAVES_M * WM * 16, BN = WAVES_N * WN * 16, BK = 64;
  constexpr int A_ELEMS = BM * BK, W_ELEMS = BN * BK;   // unpadded tiles, 128 B per row
  constexpr int STAGE_ELEMS = A_ELEMS + W_ELEMS;
  constexpr int SEGS_A = BM / 8 / NW, SEGS_W = BN / 8 / NW;   // wave-instructions (8 rows x 128 B = 1 KiB) per wave per tile
  static_assert(BM % (8 * NW) == 0 && BN % (8 * NW) == 0, "tile/wave mismatch");
  extern __shared__ __attribute__((aligned(16))) u16 smem[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int tile = u3d_xcd_tile(blockIdx.x, (n_out + BM - 1) / BM);      // XCD-contiguous ranges of the LIVE tiles (capacity-sized grids)
  if (tile < 0) return;
  const int m0 = tile * BM;
  const int col0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wv / WAVES_N, wn = wv % WAVES_N;
  const int kchunks = cin / BK;
  const int nstage = kvol * kchunks;

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, -1, 0x00020000);
  const unsigned row_bytes = (unsigned)cin * 2u;
  // loader role: wave-instruction u of this wave fills rows (wv*4+u)*8 .. +7 of a tile; lane = (row in group, 16-byte slot)
  const int lrow = lane >> 3, lslot = lane & 7;
  unsigned a_part16[SEGS_A], w_voff[SEGS_W];
  int arow[SEGS_A];
#pragma unroll
  for (int u = 0; u < SEGS_A; ++u) {
    const int r = (wv * SEGS_A + u) * 8 + lrow;
    arow[u] = r;
    a_part16[u] = (unsigned)(lslot ^ ((r >> 1) & 7)) * 16u;
  }
#pragma unroll
  for (int u = 0; u < SEGS_W; ++u) {
    const int r = (wv * SEGS_W + u) * 8 + lrow;
    const int part = lslot ^ ((r >> 1) & 7);
    w_voff[u] = (col0 + r < cout) ? (unsigned)((col0 + r) * cin + part * 8) * 2u : 0xFFFFFFFFu;
  }
  int idx_cur[SEGS_A], idx_nxt[SEGS_A];
  auto load_idx_next = [&](int stage) {
    const int kap = stage % kvol;
#pragma unroll
    for (int u = 0; u < SEGS_A; ++u) {
      int m = m0 + arow[u];
      int mc = m < n_out ? m : n_out - 1;
      idx_nxt[u] = nbr ? nbr[(long long)kap * ld + mc] : mc;           // raw: masked when consumed (see k_igemm_fwd)
    }
  };
  auto advance_idx = [&]() {
#pragma unroll
    for (int u = 0; u < SEGS_A; ++u) idx_cur[u] = (m0 + arow[u] < n_out) ? idx_nxt[u] : -1;
  };
  auto issue = [&](int st, int buf) {
    const int kap = st % kvol, c0 = (st / kvol) * BK;
    u16* Ab = smem + buf * STAGE_ELEMS + wv * (SEGS_A * 512);
    u16* Wb = smem + buf * STAGE_ELEMS + A_ELEMS + wv * (SEGS_W * 512);
    const unsigned a_soff = (unsigned)c0 * 2u;
    const unsigned w_soff = (unsigned)(kap * cin * cout + c0) * 2u;
#pragma unroll
    for (int u = 0; u < SEGS_A; ++u) {
      unsigned voff = idx_cur[u] >= 0 ? (unsigned)idx_cur[u] * row_bytes + a_part16[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(Ab + u * 512), 16, voff, a_soff, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < SEGS_W; ++u)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_void_ptr)(Wb + u * 512), 16, w_voff[u], w_soff, 0, 0);
  };
#if GLDS_FRAG_B128
  // one LDS-DMA instruction of stage `st` (q < SEGS_A: activation rows, else weight rows): lets the stage loop feed the address unit
  // between MFMA groups instead of queueing all of a stage's loads in front of them
  auto issue_one = [&](int st, int buf, int q) {
    const int kap = st % kvol, c0 = (st / kvol) * BK;
    if (q < SEGS_A) {
      u16* Ab = smem + buf * STAGE_ELEMS + wv * (SEGS_A * 512);
      unsigned voff = idx_cur[q] >= 0 ? (unsigned)idx_cur[q] * row_bytes + a_part16[q] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(Ab + q * 512), 16, voff, (unsigned)c0 * 2u, 0, 0);
    } else {
      const int u = q - SEGS_A;
      u16* Wb = smem + buf * STAGE_ELEMS + A_ELEMS + wv * (SEGS_W * 512);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_void_ptr)(Wb + u * 512), 16, w_voff[u], (unsigned)(kap * cin * cout + c0) * 2u, 0, 0);
    }
  };
  // fragment = ONE 16-byte LDS read: lane (g, row li) takes the 8 consecutive reduction elements of part ks*4+g of its row.  The MFMA
  // only needs A and B to agree on which reduction element sits in which (lane group, position) - both go through this function -
  // so the nominal k-order of the instruction does not matter.  Conflict-free under the source-side swizzle: in a 16-lane group
  // (one g, rows 0..15) the slots (ks*4+g) ^ ((row>>1)&7) take all 8 values per row parity = every bank once.
  const int g = lane >> 4, li = lane & 15, fsw = (lane >> 1) & 7;
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) foff[ks] = ((ks * 4 + g) ^ fsw) << 3;
  typedef const volatile s16x8 __attribute__((address_space(3))) * lds_vptr;
  auto frag = [&](const u16* rowp, int ks) {
    s16x8 v = *(lds_vptr)(rowp + foff[ks]);
    return __builtin_bit_cast(bf16x8, v);
  };
#else
  // fragment offsets inside a 64-element row: slot of part (ks*4 + g/2 [+2]) under this lane's row swizzle, plus the 8-byte half
  const int g = lane >> 4, li = lane & 15, fsw = (lane >> 1) & 7;
  int foff[2][2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks)
#pragma unroll
    for (int j = 0; j < 2; ++j) foff[ks][j] = (((ks * 4 + (g >> 1) + 2 * j) ^ fsw) << 3) + (g & 1) * 4;
  typedef const volatile s16x4 __attribute__((address_space(3))) * lds_vptr;
  auto frag = [&](const u16* rowp, int ks) {
    s16x4 x = *(lds_vptr)(rowp + foff[ks][0]);
    s16x4 y = *(lds_vptr)(rowp + foff[ks][1]);
    s16x8 v = {x[0], x[1], x[2], x[3], y[0], y[1], y[2], y[3]};
    return __builtin_bit_cast(bf16x8, v);
  };

#endif
  load_idx_next(0);
  advance_idx();
  load_idx_next(1 < nstage ? 1 : 0);
  issue(0, 0);
  __syncthreads();
  for (int st = 0; st < nstage; ++st) {
    const int buf = st & 1;
    const int nx = st + 1 < nstage ? st + 1 : st;       // the last stage re-fetches itself into the idle buffer: branch-free body
    advance_idx();
    load_idx_next(st + 2 < nstage ? st + 2 : nstage - 1);
#if !GLDS_DMA_SPREAD
    issue(nx, buf ^ 1);                                 // in flight during the whole stage; buffer free since the last barrier
#endif
    const u16* A = smem + buf * STAGE_ELEMS + (wm * WM * 16 + li) * BK;
    const u16* W = smem + buf * STAGE_ELEMS + A_ELEMS + (wn * WN * 16 + li) * BK;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 af[WM];
#pragma unroll
      for (int a = 0; a < WM; ++a) af[a] = frag(A + a * 16 * BK, ks);
#pragma unroll
      for (int b = 0; b < WN; ++b) {
        bf16x8 bfr = frag(W + b * 16 * BK, ks);
#pragma unroll
        // operands swapped: the MFMA produces the TRANSPOSED 16x16 block, i.e. this lane ends up with 4 consecutive output
        // COLUMNS (4g..4g+3) of row li - one 8-byte store per block in the epilogue instead of four 2-byte ones
        for (int a = 0; a < WM; ++a) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr, af[a], acc[a][b], 0, 0, 0);
#if GLDS_DMA_SPREAD
        {   // the next stage's LDS-DMA instructions, dealt out behind the MFMA groups of the first part of this stage
          constexpr int NQ = SEGS_A + SEGS_W, NG = (GLDS_DMA_SPREAD == 1) ? 2 * WN : (GLDS_DMA_SPREAD == 3 ? (WN > 1 ? WN / 2 : 1) : (GLDS_DMA_SPREAD == 4 ? WN + WN / 2 : WN));      // groups that carry loads
          constexpr int PER = (NQ + NG - 1) / NG;
          const int grp = ks * WN + b;
          if (grp < NG) {
#pragma unroll
            for (int j = 0; j < PER; ++j)
              if (grp * PER + j < NQ) issue_one(nx, buf ^ 1, grp * PER + j);
          }
          __builtin_amdgcn_sched_barrier(0);
        }
#endif
      }
    }
    __syncthreads();                                    // also drains this wave's LDS-DMA (vmcnt) before anyone reads the next buffer
  }
#define GLDS_EPI_ADDEND (BM != 256 || BN != 256)
#include "glds_epilogue.inc"
#undef GLDS_EPI_ADDEND
}

// =============================================================================================
// 256 x 256 tile, EIGHT-PHASE schedule (two k-tiles of 64 = one trip through both LDS buffers; 4 phases per k-tile).
//
// igemm_glds_body walks all eight waves through a k-tile together: 24 fragment reads, 8 LDS-DMA instructions and 64 MFMAs per wave
// between two __syncthreads() that drain vmcnt - the two waves of a SIMD are always in the same part of the stage, and the LDS-DMA
// instructions (the 35 % its ablation prices) sit among the MFMAs of the wave that issues them.  Here (the schedule the CDNA4
// guide's 256^2 template describes) a k-tile is four PHASES of 16 MFMAs (one 64 x 32 quadrant of the wave's 128 x 64 block, both
// k-steps), each phase = a LOAD segment (the phase's fragment reads + 2 LDS-DMA instructions of the next k-tile + a COUNTED vmcnt
// wait) | s_barrier | an MFMA segment (16 MFMAs at raised priority) | s_barrier, and the two wave rows (wm = 0 / 1: one wave of
// each per SIMD) run ONE barrier apart: while one wave of a SIMD is in its MFMA segment its partner is in its load segment.
//
// LDS image of a k-tile = four 16 KiB pieces, each exactly what one load segment reads: A0 / A1 = the first / second 64 rows of
// BOTH wave rows, B0 / B1 = the first / second 32 columns of all four wave columns.  Phase p reads: 1: A0 + B0, 2: B1, 3: A1, 4: -
// (B0 stays in registers for the last quadrant) and requests for the NEXT k-tile: 1: A0, 2: B0, 3: B1, 4: A1 (+ the gather
// indices two k-tiles ahead, requested first thing in phase 1 and consumed at the end of phase 4).  vmcnt is in order, so
// "everything up to piece X has landed" is one count: at the end of the load segments 1 and 2 exactly 8 younger requests are
// allowed in flight (2 pieces x 2 + 4 index loads), at the end of segment 4 four (B1, A1) - which retires B1 / A1 /
// A0 + B0 one barrier before their first reader - two barriers for the wave row that runs behind.  Nothing waits for vmcnt(0)
// inside the loop.  Rows / swizzle / fragment layout / epilogue as igemm_glds_body.
// =============================================================================================
#ifndef GLDS8_PRIO
#define GLDS8_PRIO 1
#endif
#ifndef GLDS8_BALANCE
#define GLDS8_BALANCE 1     /* the next k-tile's first A half is read in phase 4 (second register set): 4 / 4 / 8 / 8 fragment reads per segment */
#endif
#ifndef GLDS8_STAGGER
#define GLDS8_STAGGER 1     /* 0 (experiment): both wave rows in the same segment at the same time */
#endif
// RB = 16-row blocks per wave and row half: 4 = the 256-row tile; 3 = a 192-row tile in the SAME LDS image and schedule (the last
// 16 rows of every 64-row piece quarter are dead: never requested - their LDS-DMA lanes carry the "no row" offset -, never read,
// never multiplied).  For row counts where 256-row tiles leave a quarter of the CUs without a workgroup (48 000 rows x 256 columns:
// 188 tiles for 256 CUs; 192-row tiles: 250) - see igemm_rows192() and fwd_plan().
template <bool F32OUT = false, int RB = 4>
__device__ __forceinline__ void igemm_glds8_body(const u16* __restrict__ in, const u16* __restrict__ w, const int* __restrict__ nbr,
                                                 int ld, u16* __restrict__ out, const int* __restrict__ n_out_dev, int n_out_cap,
                                                 int cin, int cout, int kvol, const float* __restrict__ bias, int relu,
                                                 double* __restrict__ stats) {
  constexpr int WAVES_M = 2, WAVES_N = 4, WM = 2 * RB, WN = 4, NW = 8;
  constexpr int BM = 64 * RB, BN = 256, BK = 64;
  constexpr int PIECE = 128 * BK;                         // elements of one piece (16 KiB)
  constexpr int STAGE_ELEMS = 4 * PIECE;                  // A0 | A1 | B0 | B1
  extern __shared__ __attribute__((aligned(16))) u16 smem[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int tile = u3d_xcd_tile(blockIdx.x, (n_out + BM - 1) / BM);      // XCD-contiguous ranges of the LIVE tiles (capacity-sized grids)
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
  const unsigned row_bytes = (unsigned)cin * 2u;
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
      w_voff[sp][u] = (col0 + tc < cout) ? (unsigned)((col0 + tc) * cin + (lslot ^ ((r >> 1) & 7)) * 8) * 2u : 0xFFFFFFFFu;
    }
  }
  int idx_cur[2][2], idx_nxt[2][2];
  // (needs a neighbour table: the plain GEMM callers, nbr == nullptr, stay on igemm_glds_body)
  int mcl[2][2];
#pragma unroll
  for (int sp = 0; sp < 2; ++sp)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + (arow[sp][u] < 0 ? 0 : arow[sp][u]);
      mcl[sp][u] = m < n_out ? m : n_out - 1;
      idx_nxt[sp][u] = mcl[sp][u];
    }
  // the loads must land in the loop-carried registers themselves: a copy at the loop's back edge needs the value, i.e. a
  // vmcnt(0) per k-tile (what hipcc emitted with a select or a branch "nbr ? load : m" between the load and the variable)
  // Requested at the top of phase 1 and consumed at the end of phase 4 of the SAME loop trip: a load pending across the back
  // edge made hipcc copy the register there, i.e. wait vmcnt(0) once per k-tile.  Between the request and advance_idx() lie
  // exactly the 8 LDS-DMA requests of the trip: the wait hipcc inserts for the indices is the vmcnt(8) the schedule wants.
  auto load_idx_next = [&](int stage) {
    const int* row = nbr + (long long)(stage % kvol) * ld;
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
      for (int u = 0; u < 2; ++u) idx_nxt[sp][u] = row[mcl[sp][u]];
  };
  auto advance_idx = [&]() {
#pragma unroll
    for (int sp = 0; sp < 2; ++sp)
#pragma unroll
      for (int u = 0; u < 2; ++u) idx_cur[sp][u] = (arow[sp][u] >= 0 && m0 + arow[sp][u] < n_out) ? idx_nxt[sp][u] : -1;
  };
  auto issue_a = [&](int st, int buf, int sp) {           // piece A_sp of k-tile st
    const unsigned soff = (unsigned)((st / kvol) * BK) * 2u;
    u16* dst = smem + buf * STAGE_ELEMS + sp * PIECE + wv * 1024;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const unsigned voff = idx_cur[sp][u] >= 0 ? (unsigned)idx_cur[sp][u] * row_bytes + a_part16[u] : 0xFFFFFFFFu;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(dst + u * 512), 16, voff, soff, 0, 0);
    }
  };
  auto issue_b = [&](int st, int buf, int sp) {           // piece B_sp of k-tile st
    const unsigned soff = (unsigned)((st % kvol) * cin * cout + (st / kvol) * BK) * 2u;
    u16* dst = smem + buf * STAGE_ELEMS + (2 + sp) * PIECE + wv * 1024;
#pragma unroll
    for (int u = 0; u < 2; ++u)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_void_ptr)(dst + u * 512), 16, w_voff[sp][u], soff, 0, 0);
  };
  const int g = lane >> 4, li = lane & 15, fsw = (lane >> 1) & 7;
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) foff[ks] = ((ks * 4 + g) ^ fsw) << 3;
  typedef const volatile s16x8 __attribute__((address_space(3))) * lds_vptr;
  auto frag = [&](const u16* rowp, int ks) {
    s16x8 v = *(lds_vptr)(rowp + foff[ks]);
    return __builtin_bit_cast(bf16x8, v);
  };
#if GLDS8_BALANCE
  bf16x8 af2[2][RB][2], bf[2][2][2];                      // A: [half][row block][k-step]; B: [half][col block][k-step]
#define G8_AF(SP) af2[SP]
#else
  bf16x8 af1[RB][2], bf[2][2][2];                         // A: [row block][k-step] of the current half; B: [half][col block][k-step]
#define G8_AF(SP) af1
#endif
#define G8_READ_A(BUF, SP)                                                                                   \
  {                                                                                                          \
    const u16* A_ = smem + (BUF) * STAGE_ELEMS + (SP) * PIECE + (wm * 64 + li) * BK;                         \
    _Pragma("unroll") for (int a = 0; a < RB; ++a) {                                                         \
      G8_AF(SP)[a][0] = frag(A_ + a * 16 * BK, 0);                                                           \
      G8_AF(SP)[a][1] = frag(A_ + a * 16 * BK, 1);                                                           \
    }                                                                                                        \
  }
#define G8_READ_B(BUF, SP)                                                                                   \
  {                                                                                                          \
    const u16* B_ = smem + (BUF) * STAGE_ELEMS + (2 + (SP)) * PIECE + (wn * 32 + li) * BK;                   \
    _Pragma("unroll") for (int b = 0; b < 2; ++b) {                                                          \
      bf[SP][b][0] = frag(B_ + b * 16 * BK, 0);                                                              \
      bf[SP][b][1] = frag(B_ + b * 16 * BK, 1);                                                              \
    }                                                                                                        \
  }
#define G8_MMA(SA, SB)                                                                                       \
  {                                                                                                          \
    __builtin_amdgcn_s_setprio(GLDS8_PRIO);                                                                  \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                         \
      _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                          \
        _Pragma("unroll") for (int a = 0; a < RB; ++a)                                                       \
          acc[(SA) * RB + a][(SB) * 2 + b] =                                                                 \
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[SB][b][ks], G8_AF(SA)[a][ks], acc[(SA) * RB + a][(SB) * 2 + b], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                           \
  }
#define G8_BAR()                                  \
  {                                               \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);            \
  }
#define G8_VMCNT8() __builtin_amdgcn_s_waitcnt(0x0F78)    /* vmcnt(8): expcnt / lgkmcnt untouched */

  // prologue: indices of k-tiles 0, 1, 2; all four pieces of k-tile 0; everything landed before the first read
  load_idx_next(0);
  advance_idx();
  issue_a(0, 0, 0); issue_b(0, 0, 0); issue_b(0, 0, 1); issue_a(0, 0, 1);
  load_idx_next(1 < nstage ? 1 : 0);
  advance_idx();
  __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
  G8_BAR();
#if GLDS8_BALANCE
  G8_READ_A(0, 0)                                         // phase 4 reads the NEXT k-tile's first row half: the first one here
#endif
  if (GLDS8_STAGGER && wm == 1) G8_BAR();                 // the second wave row runs one barrier behind the first
  for (int st = 0; st < nstage; ++st) {
    const int buf = st & 1;
    const int nx = st + 1 < nstage ? st + 1 : st;         // past the end: a harmless re-fetch into the buffer nobody reads again
    // ---- phase 1: quadrant (rows 0-63, cols 0-31)
    load_idx_next(st + 2 < nstage ? st + 2 : nstage - 1);
    __builtin_amdgcn_sched_barrier(0);
    G8_READ_B(buf, 0)
#if !GLDS8_BALANCE
    __builtin_amdgcn_sched_barrier(0);
    G8_READ_A(buf, 0)
#endif
    issue_a(nx, buf ^ 1, 0);
    G8_VMCNT8();                                          // B1 of this k-tile has landed (every wave's share after the barrier)
    G8_BAR();
    G8_MMA(0, 0)
    G8_BAR();
    // ---- phase 2: (rows 0-63, cols 32-63)
    G8_READ_B(buf, 1)
    issue_b(nx, buf ^ 1, 0);
    G8_VMCNT8();                                          // A1 of this k-tile
    G8_BAR();
    G8_MMA(0, 1)
    G8_BAR();
    // ---- phase 3: (rows 64-127, cols 32-63)
    G8_READ_A(buf, 1)
    issue_b(nx, buf ^ 1, 1);
#if GLDS8_BALANCE
    __builtin_amdgcn_s_waitcnt(0x0F74);                   // vmcnt(4): A0 of the next k-tile (read in phase 4)
#endif
    G8_BAR();
    G8_MMA(1, 1)
    G8_BAR();
    // ---- phase 4: (rows 64-127, cols 0-31): B0 is still in registers
#if GLDS8_BALANCE
    G8_READ_A(buf ^ 1, 0)                                 // 12 / 4 / 8 / 0 reads per segment -> 4 / 4 / 8 / 8
#endif
    issue_a(nx, buf ^ 1, 1);
    __builtin_amdgcn_sched_barrier(0);
    advance_idx();                                        // (hipcc waits vmcnt(8) here: the indices requested in phase 1)
    __builtin_amdgcn_s_waitcnt(0x0F74);                   // vmcnt(4): A0 and B0 of the next k-tile
    G8_BAR();
    G8_MMA(1, 0)
    G8_BAR();
  }
  if (GLDS8_STAGGER && wm == 0) G8_BAR();                 // same number of barriers for both wave rows
  __builtin_amdgcn_s_waitcnt(0x0F70);                     // the tail's re-fetch requests: landed before the epilogue reuses the buffers
  __syncthreads();
#undef G8_AF
#undef G8_READ_A
#undef G8_READ_B
#undef G8_MMA
#undef G8_BAR
#undef G8_VMCNT8
#define GLDS_EPI_ADDEND 1
#include "glds_epilogue.inc"
#undef GLDS_EPI_ADDEND
}
__global__ __launch_bounds__(512) void k_igemm_glds8_256x256(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                             const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                             const float* bias, int relu, double* stats) {
  igemm_glds8_body(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_256x256_f32o(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                                  const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                                  const float* bias, int relu, double* stats) {
  igemm_glds8_body<true>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_192x256(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                             const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                             const float* bias, int relu, double* stats) {
  igemm_glds8_body<false, 3>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_192x256_f32o(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                                  const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                                  const float* bias, int relu, double* stats) {
  igemm_glds8_body<true, 3>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
// 192-row tiles instead of 256-row ones when they finish sooner on 256 CUs with one workgroup each (time ~ rounds x tile rows): the
// mid-size layers of the dense stack (48 000 rows x 256 columns: 188 -> 250 workgroups, 12 000 rows x 512 columns in 128-column
// tiles: 188 -> 252).  Where fwd_plan() asks.
static inline bool igemm_rows192(int n_out_cap, int col_blocks) {
  const long long w256 = (long long)u3d_cdiv(n_out_cap, 256) * col_blocks, w192 = (long long)u3d_cdiv(n_out_cap, 192) * col_blocks;
  return (double)u3d_cdiv(w192, 256) * 192.0 * 1.05 < (double)u3d_cdiv(w256, 256) * 256.0;
}

// =============================================================================================
// 256 x 128 tile on the same idea, for LONG reductions with 128-column output tiles (the 12 000-row 512-channel layers: 72 k-tiles per
// tile; they ran on 128 x 128 tiles, two independent workgroups per CU whose relative phase nobody controls).  Eight waves = two
// GROUPS of four (waves w and w + 4 share a SIMD): group g owns rows g*128 .. +127 as 2 x 2 waves of 64 x 64, both groups share the
// weight tile (1.5 x the LDS-DMA bytes per MFMA of the 256 x 256 tile instead of 2 x) and run one barrier apart.  A k-tile is only
// TWO phases of 16 MFMAs here (column halves of the wave's block), so two stage buffers would leave a request one phase to land:
// THREE buffers (3 x 48 KiB), k-tile st + 2 requested during k-tile st.  Pieces: A0 / A1 = the rows of group 0 / 1 (16 KiB),
// B0 / B1 = the first / second 32 columns of both wave columns (8 KiB).  Per trip: segment 1 reads B0 + B1 and requests A(st+2)
// (+ the gather indices of st + 3), segment 2 reads the NEXT k-tile's A (second register set) and requests B(st+2); one counted
// wait per segment, vmcnt(10) both times (what is younger than the piece that must have landed: 2 + 4 + 4 and 4 + 4 + 2 requests).
// Not for short reductions: with 18 k-tiles per tile a quarter of a workgroup's life is prologue + epilogue, which a second
// resident workgroup hides and this 144 KiB one cannot (measured on par there).
// =============================================================================================
template <bool F32OUT = false, int RB = 4>      // RB = 3: 192-row tiles (48 live rows per wave), see igemm_glds8_body
__device__ __forceinline__ void igemm_glds8n_body(const u16* __restrict__ in, const u16* __restrict__ w, const int* __restrict__ nbr,
                                                  int ld, u16* __restrict__ out, const int* __restrict__ n_out_dev, int n_out_cap,
                                                  int cin, int cout, int kvol, const float* __restrict__ bias, int relu,
                                                  double* __restrict__ stats) {
  constexpr int WAVES_M = 4, WAVES_N = 2, WM = RB, WN = 4, NW = 8;
  constexpr int BM = 64 * RB, BN = 128, BK = 64;
  constexpr int APIECE = 128 * BK, BPIECE = 64 * BK;
  constexpr int STAGE_ELEMS = 2 * APIECE + 2 * BPIECE;    // A0 | A1 | B0 | B1 = 48 KiB
  extern __shared__ __attribute__((aligned(16))) u16 smem[];

  const int n_out = min(*n_out_dev, n_out_cap);
  const int tile = u3d_xcd_tile(blockIdx.x, (n_out + BM - 1) / BM);      // XCD-contiguous ranges of the LIVE tiles (capacity-sized grids)
  if (tile < 0) return;
  const int m0 = tile * BM;
  const int col0 = blockIdx.y * BN;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int grp = wv >> 2, wm = wv >> 1, wn = wv & 1;     // wm = grp*2 + (row half inside the group): the epilogue's row-block index
  const int nstage = kvol * (cin / BK);

  f32x4 acc[WM][WN];
#pragma unroll
  for (int a = 0; a < WM; ++a)
#pragma unroll
    for (int b = 0; b < WN; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

  const __amdgpu_buffer_rsrc_t in_rs = __builtin_amdgcn_make_buffer_rsrc((void*)in, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t w_rs = __builtin_amdgcn_make_buffer_rsrc((void*)w, 0, -1, 0x00020000);
  const unsigned row_bytes = (unsigned)cin * 2u;
  const int lrow = lane >> 3, lslot = lane & 7;
  // A piece g: 16 instructions, this wave issues u = 0 / 1: piece rows (wv*2+u)*8 + lrow = tile rows g*128 + ...
  // B piece t:  8 instructions, this wave issues one: piece row wv*8 + lrow = tile column (r>>5)*64 + t*32 + (r&31)
  unsigned a_part16[2], w_voff[2];
  int arow[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int r = (wv * 2 + u) * 8 + lrow;
    a_part16[u] = (unsigned)(lslot ^ ((r >> 1) & 7)) * 16u;
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) arow[gp][u] = ((r & 63) < 16 * RB) ? gp * (32 * RB) + (r >> 6) * (16 * RB) + (r & 63) : -1;
  }
  {
    const int r = wv * 8 + lrow;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const int tc = (r >> 5) * 64 + t * 32 + (r & 31);
      w_voff[t] = (col0 + tc < cout) ? (unsigned)((col0 + tc) * cin + (lslot ^ ((r >> 1) & 7)) * 8) * 2u : 0xFFFFFFFFu;
    }
  }
  int idx_cur[2][2], idx_nxt[2][2], mcl[2][2];
#pragma unroll
  for (int gp = 0; gp < 2; ++gp)
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int m = m0 + (arow[gp][u] < 0 ? 0 : arow[gp][u]);
      mcl[gp][u] = m < n_out ? m : n_out - 1;
      idx_nxt[gp][u] = mcl[gp][u];
    }
  auto load_idx_next = [&](int stage) {                   // requested and consumed inside one loop trip (see igemm_glds8_body)
    const int* row = nbr + (long long)(stage % kvol) * ld;
#pragma unroll
    for (int gp = 0; gp < 2; ++gp)
#pragma unroll
      for (int u = 0; u < 2; ++u) idx_nxt[gp][u] = row[mcl[gp][u]];
  };
  auto advance_idx = [&]() {
#pragma unroll
    for (int gp = 0; gp < 2; ++gp)
#pragma unroll
      for (int u = 0; u < 2; ++u) idx_cur[gp][u] = (arow[gp][u] >= 0 && m0 + arow[gp][u] < n_out) ? idx_nxt[gp][u] : -1;
  };
  auto issue_a = [&](int st, int sl) {                    // both A pieces of k-tile st into stage slot sl (rows idx_cur describes)
    const unsigned soff = (unsigned)((st / kvol) * BK) * 2u;
#pragma unroll
    for (int gp = 0; gp < 2; ++gp) {
      u16* dst = smem + sl * STAGE_ELEMS + gp * APIECE + wv * 1024;
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const unsigned voff = idx_cur[gp][u] >= 0 ? (unsigned)idx_cur[gp][u] * row_bytes + a_part16[u] : 0xFFFFFFFFu;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(in_rs, (lds_void_ptr)(dst + u * 512), 16, voff, soff, 0, 0);
      }
    }
  };
  auto issue_b = [&](int st, int sl) {                    // both B pieces of k-tile st
    const unsigned soff = (unsigned)((st % kvol) * cin * cout + (st / kvol) * BK) * 2u;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      u16* dst = smem + sl * STAGE_ELEMS + 2 * APIECE + t * BPIECE + wv * 512;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(w_rs, (lds_void_ptr)dst, 16, w_voff[t], soff, 0, 0);
    }
  };
  const int g = lane >> 4, li = lane & 15, fsw = (lane >> 1) & 7;
  int foff[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) foff[ks] = ((ks * 4 + g) ^ fsw) << 3;
  typedef const volatile s16x8 __attribute__((address_space(3))) * lds_vptr;
  auto frag = [&](const u16* rowp, int ks) {
    s16x8 v = *(lds_vptr)(rowp + foff[ks]);
    return __builtin_bit_cast(bf16x8, v);
  };
  bf16x8 af[2][RB][2], bf[2][2][2];                       // A: [register set][row block][k-step]; B: [column half][col block][k-step]
#define N8_READ_A(SL, SET)                                                                                   \
  {                                                                                                          \
    const u16* A_ = smem + (SL) * STAGE_ELEMS + grp * APIECE + (((wv >> 1) & 1) * 64 + li) * BK;             \
    _Pragma("unroll") for (int a = 0; a < RB; ++a) {                                                         \
      af[SET][a][0] = frag(A_ + a * 16 * BK, 0);                                                             \
      af[SET][a][1] = frag(A_ + a * 16 * BK, 1);                                                             \
    }                                                                                                        \
  }
#define N8_READ_B(SL)                                                                                        \
  {                                                                                                          \
    _Pragma("unroll") for (int t = 0; t < 2; ++t) {                                                          \
      const u16* B_ = smem + (SL) * STAGE_ELEMS + 2 * APIECE + t * BPIECE + (wn * 32 + li) * BK;             \
      _Pragma("unroll") for (int b = 0; b < 2; ++b) {                                                        \
        bf[t][b][0] = frag(B_ + b * 16 * BK, 0);                                                             \
        bf[t][b][1] = frag(B_ + b * 16 * BK, 1);                                                             \
      }                                                                                                      \
    }                                                                                                        \
  }
#define N8_MMA(SET, T)                                                                                       \
  {                                                                                                          \
    __builtin_amdgcn_s_setprio(1);                                                                           \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                         \
      _Pragma("unroll") for (int b = 0; b < 2; ++b)                                                          \
        _Pragma("unroll") for (int a = 0; a < RB; ++a)                                                       \
          acc[a][(T) * 2 + b] =                                                                              \
              __builtin_amdgcn_mfma_f32_16x16x32_bf16(bf[T][b][ks], af[SET][a][ks], acc[a][(T) * 2 + b], 0, 0, 0); \
    __builtin_amdgcn_s_setprio(0);                                                                           \
  }
#define N8_BAR()                                  \
  {                                               \
    __builtin_amdgcn_sched_barrier(0);            \
    __builtin_amdgcn_s_barrier();                 \
    __builtin_amdgcn_sched_barrier(0);            \
  }
  // one k-tile: SET = the A register set holding k-tile st (the other one receives k-tile st + 1)
#define N8_TRIP(SET)                                                                                         \
  {                                                                                                          \
    const int s2 = st + 2 < nstage ? st + 2 : nstage - 1;                                                    \
    load_idx_next(st + 3 < nstage ? st + 3 : nstage - 1);                                                    \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    N8_READ_B(sl0)                                                                                           \
    issue_a(s2, sl2);                                                                                        \
    __builtin_amdgcn_s_waitcnt(0x0F7A);                   /* vmcnt(10): A of k-tile st + 1 */                \
    N8_BAR();                                                                                                \
    N8_MMA(SET, 0)                                                                                           \
    N8_BAR();                                                                                                \
    N8_READ_A(sl1, (SET) ^ 1)                                                                                \
    issue_b(s2, sl2);                                                                                        \
    __builtin_amdgcn_sched_barrier(0);                                                                       \
    advance_idx();                                                                                           \
    __builtin_amdgcn_s_waitcnt(0x0F7A);                   /* vmcnt(10): B of k-tile st + 1 */                \
    N8_BAR();                                                                                                \
    N8_MMA(SET, 1)                                                                                           \
    N8_BAR();                                                                                                \
    { const int t_ = sl0; sl0 = sl1; sl1 = sl2; sl2 = t_; }                                                  \
    ++st;                                                                                                    \
  }
  // prologue: k-tiles 0 and 1 requested (slots 0, 1), indices of k-tile 2 current, A of k-tile 0 in register set 0
  load_idx_next(0);
  advance_idx();
  issue_a(0, 0); issue_b(0, 0);
  load_idx_next(1 < nstage ? 1 : 0);
  advance_idx();
  issue_a(1 < nstage ? 1 : 0, 1); issue_b(1 < nstage ? 1 : 0, 1);
  load_idx_next(2 < nstage ? 2 : nstage - 1);
  advance_idx();
  __builtin_amdgcn_s_waitcnt(0x0F70);                     // vmcnt(0)
  N8_BAR();
  N8_READ_A(0, 0)
  if (grp == 1) N8_BAR();                                 // the second group runs one barrier behind the first
  int st = 0, sl0 = 0, sl1 = 1, sl2 = 2;
  while (st + 1 < nstage) {
    N8_TRIP(0)
    N8_TRIP(1)
  }
  if (st < nstage) N8_TRIP(0)
  if (grp == 0) N8_BAR();
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
#undef N8_READ_A
#undef N8_READ_B
#undef N8_MMA
#undef N8_BAR
#undef N8_TRIP
#define GLDS_EPI_ADDEND 1
#include "glds_epilogue.inc"
#undef GLDS_EPI_ADDEND
}
__global__ __launch_bounds__(512) void k_igemm_glds8_256x128(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                             const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                             const float* bias, int relu, double* stats) {
  igemm_glds8n_body(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_256x128_f32o(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                                  const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                                  const float* bias, int relu, double* stats) {
  igemm_glds8n_body<true>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_192x128(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                             const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                             const float* bias, int relu, double* stats) {
  igemm_glds8n_body<false, 3>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
__global__ __launch_bounds__(512) void k_igemm_glds8_192x128_f32o(const u16* in, const u16* w, const int* nbr, int ld, u16* out,
                                                                  const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,
                                                                  const float* bias, int relu, double* stats) {
  igemm_glds8n_body<true, 3>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);
}
// concrete kernels (a __global__ TEMPLATE with this body lost its host stub under hipcc 7.2: undefined symbol at load time)
#define U3D_GLDS_KERNEL(NAME, A, B, C, D)                                                                                        \
  __global__ __launch_bounds__(A* B * 64) void NAME(const u16* in, const u16* w, const int* nbr, int ld, u16* out,               \
                                                    const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,            \
                                                    const float* bias, int relu, double* stats) {                                \
    igemm_glds_body<A, B, C, D>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);                   \
  }
#define U3D_GLDS_KERNEL_X(NAME, ...) U3D_GLDS_KERNEL(NAME, __VA_ARGS__)
U3D_GLDS_KERNEL_X(k_igemm_glds_256x256, GLDS256_CFG)
// (a 4-wave variant with 128 x 128 per wave - 1.5x fewer LDS fragment bytes per MFMA - compiled to 512 VGPRs + spills and ran at
//  877 vs 1076 TFLOP/s: it needs a hand-scheduled fragment pipeline, not another template instance)
U3D_GLDS_KERNEL(k_igemm_glds_256x128, 4, 2, 4, 4)
U3D_GLDS_KERNEL(k_igemm_glds_128x64, 4, 1, 2, 4)
U3D_GLDS_KERNEL(k_igemm_glds_128x128, 2, 2, 4, 4)      /* 4 waves, 64 KiB LDS: two workgroups per CU run out of phase */
#undef U3D_GLDS_KERNEL
// f32-output instantiations of the two small tiles (split-bf16 products, u3d_igemm_fwd_split_bf16)
#define U3D_GLDS_KERNEL_F32O(NAME, A, B, C, D)                                                                                   \
  __global__ __launch_bounds__(A* B * 64) void NAME(const u16* in, const u16* w, const int* nbr, int ld, u16* out,               \
                                                    const int* n_out_dev, int n_out_cap, int cin, int cout, int kvol,            \
                                                    const float* bias, int relu, double* stats) {                                \
    igemm_glds_body<A, B, C, D, true>(in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, bias, relu, stats);             \
  }
U3D_GLDS_KERNEL_F32O(k_igemm_glds_128x64_f32o, 4, 1, 2, 4)
U3D_GLDS_KERNEL_F32O(k_igemm_glds_128x128_f32o, 2, 2, 4, 4)
#undef U3D_GLDS_KERNEL_F32O
typedef void (*glds_kernel_t)(const u16*, const u16*, const int*, int, u16*, const int*, int, int, int, int, const float*, int, double*);

// (The register-staged "ping-pong" kernel of round 1 - two wave groups in opposite phases, measured on par with k_igemm_fwd -
//  was removed when igemm_glds8_body took that idea to the LDS-DMA kernels; DESIGN.md 3.1 keeps its numbers.)

// =============================================================================================
// ONE launch plan for every forward / input-gradient launch: fwd_plan() decides the kernel, tile, grid and statistics layout of
// u3d_igemm_fwd_bf16 / _fwd_affine_bf16 / _fwd_split_bf16 and u3d_linear_bf16, and u3d_igemm_fwd_plan reports that same plan, so
// that a caller asks which kernel serves a shape instead of trying launches.
// =============================================================================================
// The LDS-DMA kernels: bf16- and f32-output instantiations (nullptr: none), tile, threads, dynamic LDS, and whether the epilogue
// takes an addend (relu & 2; GLDS_EPI_ADDEND).
struct GldsKernel {
  glds_kernel_t bf16, f32;
  int rows, cols, threads;
  size_t lds;
  bool addend;
};
#define GLDS_GEOM(A, B, C, D) A * C * 16, B * D * 16, A * B * 64, (size_t)2 * (A * C * 16 + B * D * 16) * 64 * 2     /* U3D_GLDS_KERNEL(A, B, C, D) */
#define GLDS_GEOM_X(...) GLDS_GEOM(__VA_ARGS__)
enum { G_256x256, G8_256x256, G8_192x256, G8_256x128, G8_192x128, G_256x128, G_128x128, G_128x64, G_COUNT };
static const GldsKernel GLDS_KERNELS[G_COUNT] = {
    {k_igemm_glds_256x256, nullptr, GLDS_GEOM_X(GLDS256_CFG), false},                                   // two-phase
    {k_igemm_glds8_256x256, k_igemm_glds8_256x256_f32o, 256, 256, 512, 2 * (256 + 256) * 64 * 2, true},      // eight-phase, 128 KiB
    {k_igemm_glds8_192x256, k_igemm_glds8_192x256_f32o, 192, 256, 512, 2 * (256 + 256) * 64 * 2, true},      // (same LDS image)
    {k_igemm_glds8_256x128, k_igemm_glds8_256x128_f32o, 256, 128, 512, 3 * (256 + 128) * 64 * 2, true},      // eight-phase, 144 KiB
    {k_igemm_glds8_192x128, k_igemm_glds8_192x128_f32o, 192, 128, 512, 3 * (256 + 128) * 64 * 2, true},
    {k_igemm_glds_256x128, nullptr, GLDS_GEOM(4, 2, 4, 4), true},
    {k_igemm_glds_128x128, k_igemm_glds_128x128_f32o, GLDS_GEOM(2, 2, 4, 4), true},
    {k_igemm_glds_128x64, k_igemm_glds_128x64_f32o, GLDS_GEOM(4, 1, 2, 4), true},
};
#undef GLDS_GEOM_X
#undef GLDS_GEOM

// what the launch must do besides the convolution.  The first four are the header's U3D_FWD_EPI_*: PLAIN; ADD = + bf16 addend;
// STATS = + BatchNorm statistics; AFFINE = + per-column f32 shift and optional ReLU on a CONVOLUTION (u3d_igemm_fwd_affine_bf16: an
// eval-mode BatchNorm folded into the weights, bn_fold.hip).  BIAS_RELU: u3d_linear_bf16.  F32 / F32_ADD = f32 output without / with
// an f32 addend (u3d_igemm_fwd_split_bf16; its statistics do not change the kernel).
enum FwdEpi { EPI_PLAIN = U3D_FWD_EPI_PLAIN, EPI_ADD = U3D_FWD_EPI_ADD, EPI_STATS = U3D_FWD_EPI_STATS, EPI_AFFINE = U3D_FWD_EPI_AFFINE,
              EPI_BIAS_RELU, EPI_F32, EPI_F32_ADD };

struct FwdPlan {
  int family = U3D_FWD_FAM_NONE;   // U3D_FWD_FAM_*; NONE: no implicit-GEMM kernel serves the shape
  int kernel = 0;                  // within the family: the direct-operand slot, the index into GLDS_KERNELS / REG_KERNELS
  DirectPlan direct;               // DIRECT: its own plan (igemm_direct.hip)
  glds_kernel_t fn = nullptr;      // GLDS: the bf16- or f32-output instantiation
  int rows = 0, cols = 0;          // tile
  dim3 grid;
  int threads = 0;
  size_t lds = 0;
  int partials = 0, part_rows = 0; // statistics a STATS launch writes: [partials][2][cout], one per part_rows rows (0: one per wave)
  bool addend = false;             // the kernel's epilogue takes an addend
  bool served() const { return family != U3D_FWD_FAM_NONE; }
};

constexpr int GLDS8N_MIN_KTILES = 48;     // 256 x 128 eight-phase tiles: long reductions only (k-tiles of 64 = kvol * cin / 64) ...
constexpr int GLDS8N_MIN_WGS = 160;       // ... and enough 256-row workgroups to keep most CUs busy with ONE per CU

// The rules, first match wins (n = n_out_cap; "table": a neighbour table is passed; tiles = ceil(n / 256)):
//   1. PLAIN / ADD, k-major weights, 8 -> 16 with at most 27 offsets: the encoder's input convolution (conv_in.hip, w = [K][8][16]).
//   2. PLAIN / ADD / STATS: the direct-operand kernels wherever u3d_plan_igemm_direct serves the shape (its rule: igemm_direct.h):
//      the narrow sparse levels, activations gathered straight into the MFMA operand registers.  Statistics: one partial per wave.
//   3. The LDS-DMA kernels, for n-major weights, cin % 64 == 0, cout % 64 == 0 and n > 0 only:
//      BIAS_RELU (plain GEMM, its own thresholds): 256 x 256 two-phase if cout % 256 == 0 and tiles * cout / 256 >= 128,
//         256 x 128 two-phase if cout % 128 == 0 and tiles * cout / 128 >= 128, else 128 x 64.
//      a. cout % 256 == 0 and tiles * cout / 256 >= 128: with a table 256 x 256 eight-phase (192 x 256 when R192(cout / 256));
//         without one the two-phase 256 x 256, which has no addend or f32-output epilogue (F32*: none).
//      b. a table, cout % 128 == 0, kvol * cin / 64 >= GLDS8N_MIN_KTILES k-tiles, tiles * cout / 128 >= GLDS8N_MIN_WGS:
//         256 x 128 eight-phase (192 x 128 when R192(cout / 128)).
//      c. cout % 128 == 0: 128 x 128.
//      d. 128 x 64.
//      AFFINE never takes rule 2 (the direct-operand kernels read `bias` as an addend); the two-phase 256 x 256 kernel serves it (the
//         shift is the per-column bias, not the addend epilogue it lacks).
//      F32 / F32_ADD take the tile's f32-output instantiation.  R192(c): a table, kvol > 1 and igemm_rows192(n, c).
//      Statistics partials: one per row tile, ceil(n / rows).
//   The register-staged kernels (k_igemm_fwd), PLAIN / ADD and n > 0 only:
//   4. cin in {16, 32} and cout in {16, 32, 64}: 256 x cout tiles in the weights' layout.  (cin = 64 -> cout 32 / 16, the dgrad of
//      the 32 -> 64 transition, measured slower here than on the first-generation kernel: 212 vs 170 us.  Not served.)
//   5. k-major weights, cin % 64 == 0, cout % 64 == 0: 256 x 256 if cout % 256 == 0 and tiles * cout / 256 >= 128 (few row tiles -
//      the stride-4 branch of SECOND3D, 12000 rows - would leave most CUs idle; measured: 94 workgroups (N = 12000, 512 ch) 0.136 ->
//      0.100 ms on 256 x 128, 188 workgroups (N = 48000, 256 ch) stay faster on 256 x 256), else 256 x 128 if cout % 128 == 0, else
//      128 x 64.  (A 128 x 128 tile for layers with few rows was measured SLOWER: 285 vs 512 TF/s at N = 48000 - the L2->CU traffic
//      of the smaller tile outweighs the better CU fill.)
//   6. No implicit-GEMM kernel: the caller takes the first-generation u3d_spconv_fwd.
//   ADD on a kernel without an addend epilogue (rules 1, 4, 5, the table-free 256 x 256 of 3a) is that kernel's PLAIN plan with
//   addend = false: the caller adds afterwards.
static FwdPlan fwd_plan(int n_out_cap, int cin, int cout, int kvol, bool has_nbr, bool nmajor, FwdEpi epi) {
  FwdPlan p;
  const bool plain = epi == EPI_PLAIN || epi == EPI_ADD;
  auto tiled = [&](int family, int kernel, int rows, int cols, int threads, size_t lds) {
    p.family = family, p.kernel = kernel, p.rows = rows, p.cols = cols, p.threads = threads, p.lds = lds;
    p.grid = dim3(u3d_cdiv(n_out_cap, rows), u3d_cdiv(cout, cols));
  };
  if (plain && !nmajor && convin_shape(cin, cout, kvol)) {
    tiled(U3D_FWD_FAM_CONV_IN, 0, 256, CONVIN_COUT, 256, 0);
    return p;
  }
  if (plain || epi == EPI_STATS) {
    p.direct = u3d_plan_igemm_direct(n_out_cap, cin, cout, kvol, has_nbr, nmajor, epi == EPI_STATS ? DIR_STATS : DIR_BF16);
    if (p.direct.slot >= 0) {
      p.family = U3D_FWD_FAM_DIRECT, p.kernel = p.direct.slot, p.rows = 64, p.cols = cout;
      p.partials = p.direct.partials;
      p.addend = plain;            // (the statistics variants are never launched with one)
      return p;
    }
  }
  if (n_out_cap <= 0 || cin <= 0 || cout <= 0) return p;
  const long long tiles256 = u3d_cdiv(n_out_cap, 256);
  if (nmajor && cin % 64 == 0 && cout % 64 == 0) {
    const bool r192 = has_nbr && kvol > 1;
    int g;
    if (epi == EPI_BIAS_RELU)
      g = (cout % 256 == 0 && tiles256 * (cout / 256) >= 128) ? G_256x256
          : (cout % 128 == 0 && tiles256 * (cout / 128) >= 128) ? G_256x128 : G_128x64;
    else if (cout % 256 == 0 && tiles256 * (cout / 256) >= 128)
      g = !has_nbr ? G_256x256 : (r192 && igemm_rows192(n_out_cap, cout / 256)) ? G8_192x256 : G8_256x256;
    else if (has_nbr && cout % 128 == 0 && kvol * (cin / 64) >= GLDS8N_MIN_KTILES && tiles256 * (cout / 128) >= GLDS8N_MIN_WGS)
      g = (r192 && igemm_rows192(n_out_cap, cout / 128)) ? G8_192x128 : G8_256x128;
    else
      g = cout % 128 == 0 ? G_128x128 : G_128x64;
    const GldsKernel& k = GLDS_KERNELS[g];
    p.fn = (epi == EPI_F32 || epi == EPI_F32_ADD) ? k.f32 : k.bf16;
    if (!p.fn) return p;
    tiled(U3D_FWD_FAM_GLDS, g, k.rows, k.cols, k.threads, k.lds);
    p.partials = (int)p.grid.x;
    p.part_rows = k.rows;
    p.addend = k.addend;
    return p;
  }
  if (!plain) return p;
  int r = -1;
  if ((cin == 16 || cin == 32) && (cout == 16 || cout == 32 || cout == 64))
    r = (cout == 16 ? R_N16_K : cout == 32 ? R_N32_K : R_N64_K) + (nmajor ? 1 : 0);
  else if (!nmajor && cin % 64 == 0 && cout % 64 == 0)
    r = cout % 256 == 0 ? (tiles256 * (cout / 256) < 128 ? R_256x128 : R_256x256) : cout % 128 == 0 ? R_256x128 : R_128x64;
  if (r >= 0) tiled(U3D_FWD_FAM_REG, r, REG_KERNELS[r].rows, REG_KERNELS[r].cols, REG_KERNELS[r].threads, REG_KERNELS[r].lds);
  return p;
}

// bias: f32 bias (relu & 1: ReLU after it), or with relu & 2 the addend (bf16, or f32 for the f32-output kernels; the direct-operand
// kernels take a bf16 addend here); stats: the statistics epilogue of the plan's epilogue kind
static int fwd_launch(const FwdPlan& p, const void* in, const void* w, const int32_t* nbr, int ld, void* out, const int32_t* n_out_dev,
                      int n_out_cap, int cin, int cout, int kvol, hipStream_t s, const void* bias = nullptr, int relu = 0,
                      double* stats = nullptr) {
  static unsigned long long glds_mask[G_COUNT][2] = {}, reg_mask[R_COUNT] = {};      // U3D_ALLOW_LDS's per-device mask, one per kernel
  switch (p.family) {
    case U3D_FWD_FAM_CONV_IN: return u3d_launch_conv_in_fwd(in, w, nbr, ld, out, n_out_dev, n_out_cap, kvol, s);
    case U3D_FWD_FAM_DIRECT: return u3d_launch_igemm_direct(p.direct, in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, s, bias, stats);
    case U3D_FWD_FAM_GLDS:
      if (p.lds > 64 * 1024) u3d_allow_lds_impl((const void*)p.fn, (int)p.lds, &glds_mask[p.kernel][p.fn == GLDS_KERNELS[p.kernel].f32]);
      hipLaunchKernelGGL(p.fn, p.grid, dim3(p.threads), p.lds, s, (const u16*)in, (const u16*)w, nbr, ld, (u16*)out, n_out_dev, n_out_cap,
                         cin, cout, kvol, (const float*)bias, relu, stats);
      break;
    case U3D_FWD_FAM_REG:
      if (p.lds > 64 * 1024) u3d_allow_lds_impl((const void*)REG_KERNELS[p.kernel].fn, (int)p.lds, &reg_mask[p.kernel]);
      hipLaunchKernelGGL(REG_KERNELS[p.kernel].fn, p.grid, dim3(p.threads), p.lds, s, (const u16*)in, (const u16*)w, nbr, ld, (u16*)out,
                         n_out_dev, n_out_cap, cin, cout, kvol, (const float*)nullptr, 0);
      break;
    default: return U3D_ERR_UNSUPPORTED;
  }
  return hipGetLastError() == hipSuccess ? U3D_OK : U3D_ERR_LAUNCH;
}

// Dense layer on rows: out[M,N] = act(x[M,K] @ W[N,K]^T + bias) — nn.Linear layout, bf16 in/out, f32 accumulate/bias.
// Small M (decoder: B*900 rows): 128x64 tiles so that a few hundred workgroups exist.
extern "C" int32_t u3d_linear_bf16(const void* x, const void* w, const float* bias, int32_t relu, void* out,
                                   const int32_t* m_dev, int32_t m_cap, int32_t k, int32_t n, u3d_stream s) {
  U3D_REQUIRE(x && w && out && m_dev, U3D_ERR_ARG);
  if (k % 64 != 0 || n % 64 != 0) return U3D_ERR_UNSUPPORTED;
  if (m_cap <= 0) return U3D_OK;
  // nn.Linear's [N, K] weight IS the n-major layout of the LDS-DMA kernels
  const FwdPlan p = fwd_plan(m_cap, k, n, 1, false, true, EPI_BIAS_RELU);
  if (!p.served()) return U3D_ERR_UNSUPPORTED;
  return fwd_launch(p, x, w, nullptr, 0, out, m_dev, m_cap, k, n, 1, s, bias, relu ? 1 : 0);
}

// Convolution + per-column f32 shift (+ ReLU) in one pass: conv -> eval-mode BatchNorm -> ReLU with the BatchNorm's scale folded into
// the n-major weights w_folded[kvol][cout][cin] and its shift passed here (u3d_bn_fold_batched, bn_fold.hip).  The kernels and their
// epilogue are those of u3d_igemm_fwd_bf16 / u3d_linear_bf16, unchanged: the plan only keeps the launch off the direct-operand kernels.
// Rows at or past *n_out_dev are left untouched, as u3d_igemm_fwd_bf16 leaves them.
extern "C" int32_t u3d_igemm_fwd_affine_bf16(const void* in, const void* w_folded, const int32_t* nbr, int32_t ld, const float* shift,
                                             int32_t relu, void* out, const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin,
                                             int32_t cout, int32_t kvol, u3d_stream s) {
  U3D_REQUIRE(in && w_folded && out && n_out_dev && shift && kvol > 0 && (nbr || kvol == 1), U3D_ERR_ARG);
  if (cin <= 0 || cout <= 0 || cin % 64 != 0 || cout % 64 != 0) return U3D_ERR_UNSUPPORTED;
  if (n_out_cap <= 0) return U3D_OK;
  const FwdPlan p = fwd_plan(n_out_cap, cin, cout, kvol, nbr != nullptr, true, EPI_AFFINE);
  if (!p.served()) return U3D_ERR_UNSUPPORTED;
  return fwd_launch(p, in, w_folded, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, s, shift, relu ? 1 : 0);
}

// The plan u3d_igemm_fwd_bf16 (PLAIN / ADD / STATS) and u3d_igemm_fwd_affine_bf16 (AFFINE) follow for a shape; host only.
// u3d_igemm_fwd_split_bf16 writes the STATS plan's statistics layout wherever it serves a shape: there the plan never picks a
// direct-operand kernel.
extern "C" int32_t u3d_igemm_fwd_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr, int32_t nmajor,
                                      int32_t epi, u3d_fwd_plan_info* info) {
  U3D_REQUIRE(info && epi >= 0 && epi < U3D_FWD_EPI_COUNT, U3D_ERR_ARG);
  const FwdPlan p = fwd_plan(n_out_cap, cin, cout, kvol, has_nbr != 0, nmajor != 0, (FwdEpi)epi);
  if (!p.served()) return U3D_ERR_UNSUPPORTED;
  *info = {p.family, p.kernel, p.rows, p.cols, p.partials, p.part_rows, p.addend ? 1 : 0};
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------
// Split-bf16 convolution: f32-grade products on the bf16 matrix pipe (the reference keeps SparseEncoderHD and SECOND3D in fp32 - ref:
// sparse_encoder_hd.py:62-64, uni3detr.py:150-151 - and the exact f32 MFMA runs at 1/16 of the bf16 rate).  An f32 tensor x is held
// as two bf16 planes, hi = bf16(x) and lo = bf16(x - hi) (16 mantissa bits together), and x.w ~ hi.wh + hi.wl + lo.wh with f32
// accumulation (the dropped lo.wl term is 2^-16 of a 2^-8 term).  The kernels are the LDS-DMA implicit-GEMM kernels above, UNCHANGED:
// the three products are three sets of "offsets" - the caller stacks the planes as rows [hi ; lo] of one matrix, triples the
// neighbour table (nbr, nbr, nbr + plane stride) and the weights (wh, wl, wh) - and this entry only picks the f32-output instantiations.
//   in   bf16 [2 * n_in_cap][cin] (u3d_split_rows_f32), w bf16 [kvol3][cout][cin] (n-major, kvol3 = 3 * offsets), nbr int32 [kvol3][ld],
//   out  f32 [n_out_cap][cout]; stats (optional) f64 [partials][2][cout] of the f32 output (the STATS plan of u3d_igemm_fwd_plan(.., kvol3, 1, 1, ..))
extern "C" int32_t u3d_igemm_fwd_split_bf16(const void* in, const void* w, const int32_t* nbr, int32_t ld, float* out,
                                            const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol3,
                                            double* stats, const float* addend, u3d_stream s) {
  U3D_REQUIRE(in && w && out && n_out_dev && nbr && kvol3 > 0, U3D_ERR_ARG);
  if (cin % 64 != 0 || cout % 64 != 0) return U3D_ERR_UNSUPPORTED;
  if (n_out_cap <= 0) return U3D_OK;
  const FwdPlan p = fwd_plan(n_out_cap, cin, cout, kvol3, true, true, addend ? EPI_F32_ADD : EPI_F32);
  if (!p.served() || (addend && !p.addend)) return U3D_ERR_UNSUPPORTED;
  return fwd_launch(p, in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol3, s, addend, addend ? 2 : 0, stats);
}

// The convolution itself (forward with transpose_w = 0 / 1 for k- / n-major weights, input gradients), optionally with a bf16 addend
// of out's shape summed in before the one rounding (the input gradient of a residual block's first conv with the residual branch's
// gradient), or with the BatchNorm statistics of the bf16-rounded output: stats f64 [partials][2][cout] = (sum, sum of squares) per
// row tile (or per wave) and column, in the STATS plan's layout.  The caller has asked u3d_igemm_fwd_plan: a shape, an addend or
// statistics the plan does not serve are its error - an empty output (n_out_cap <= 0) included, which launches nothing where the plan
// serves it (rules 1, 2) and is unsupported, as the query says, elsewhere.
extern "C" int32_t u3d_igemm_fwd_bf16(const void* in, const void* w, const int32_t* nbr, int32_t ld, void* out,
                                      const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                                      int32_t transpose_w, const void* addend, double* stats, u3d_stream s) {
  U3D_REQUIRE(in && w && out && n_out_dev && (nbr || (kvol == 1 && !addend)) && !(addend && stats), U3D_ERR_ARG);
  const FwdPlan p = fwd_plan(n_out_cap, cin, cout, kvol, nbr != nullptr, transpose_w != 0, stats ? EPI_STATS : addend ? EPI_ADD : EPI_PLAIN);
  if (!p.served() || (addend && !p.addend)) return U3D_ERR_UNSUPPORTED;
  return fwd_launch(p, in, w, nbr, ld, out, n_out_dev, n_out_cap, cin, cout, kvol, s, addend, addend ? 2 : 0, stats);
}
