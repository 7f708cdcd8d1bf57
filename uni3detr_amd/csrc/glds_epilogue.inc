// Epilogue of the LDS-DMA forward/dgrad kernels, included textually into each kernel body (a helper taking the accumulator
// array by reference cost the 256x256 kernel its register allocation: 256 VGPRs + spills, 25.4 -> 27.5 ms per step).
// Expects in scope: acc, smem, m0, col0, tile, n_out, cout, out, bias, relu, stats, wm, wn, g, li, tid, NW, BN, WAVES_M, WM, WN, F32OUT.
// bias / ReLU, bf16 store (transposed accumulator: 4 consecutive columns per lane), optional per-tile BatchNorm statistics.
  // epilogue: acc[a][b][r] = C[row (wm*WM+a)*16 + li][col (wn*WN+b)*16 + 4g + r]; v_cvt_pk_bf16_f32 (RNE) via convertvector
  f32x4 cs[WN], cq[WN];                                 // BatchNorm statistics of this wave's rows: column sums / sums of squares
#pragma unroll
  for (int b = 0; b < WN; ++b) { cs[b] = (f32x4){0.f, 0.f, 0.f, 0.f}; cq[b] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
#pragma unroll
  for (int a = 0; a < WM; ++a) {
    const int m = m0 + (wm * WM + a) * 16 + li;
    if (m >= n_out) continue;
#pragma unroll
    for (int b = 0; b < WN; ++b) {
      const int col = col0 + (wn * WN + b) * 16 + 4 * g;
      if (col < cout) {                                 // cout % 8 == 0: the 4-column group is in or out as a whole
        f32x4 v = acc[a][b];
        // relu bit 1 (kernels that define GLDS_EPI_ADDEND 1: all but the two-phase 256 x 256 one, which it cost its register
        // allocation): `bias` is not a per-column f32 vector but a bf16 ADDEND of out's shape - the
        // residual branch's gradient summed into the input gradient of a block's first conv (sparse.ResidualToken) instead of
        // by a separate element-wise pass over both tensors
        if (bias) {
          if (GLDS_EPI_ADDEND && (relu & 2)) {
            // (F32OUT instantiations: the addend is f32 like the output - the split-bf16 input gradients of `mixed` mode)
            if constexpr (F32OUT) v += *(const f32x4*)(bias + (long long)m * cout + col);
            else v += __builtin_convertvector(*(const bf16x4*)((const u16*)bias + (long long)m * cout + col), f32x4);
          } else { const f32x4 bv = *(const f32x4*)(bias + col); v += bv; }
        }
        if (relu & 1) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        if constexpr (F32OUT) {
          // F32OUT instantiations (k_*_f32o): `out` is an f32 matrix - the accumulators leave unrounded (split-bf16 products,
          // u3d_igemm_fwd_split_bf16: the operands are hi / lo bf16 planes of f32 tensors, the result is f32-grade and must not be cut
          // back to 8 mantissa bits).  A template parameter, not a run-time flag: the bf16 kernels' code is byte-identical to before
          *(f32x4*)((float*)out + (long long)m * cout + col) = v;
          if (stats) { cs[b] += v; cq[b] += v * v; }
          continue;
        }
        const bf16x4 o = __builtin_convertvector(v, bf16x4);
        *(bf16x4*)(out + (long long)m * cout + col) = o;
        if (stats) {                                    // statistics of the ROUNDED values: what the BatchNorm that follows reads
          const f32x4 vr = __builtin_convertvector(o, f32x4);
          cs[b] += vr;
          cq[b] += vr * vr;
        }
      }
    }
  }
  if (stats) {
    // the BatchNorm behind this conv needs per-column sum / sum of squares over ALL rows: reduce this tile here (16 lanes of a
    // column group by shuffles, the row waves through LDS) and leave one f64 partial per (row tile, column) - the separate
    // statistics pass over the output (one full read of the tensor) disappears
    float* red = (float*)smem;                          // [WAVES_M][2][BN] floats; the stage buffers are dead after the last barrier
#pragma unroll
    for (int b = 0; b < WN; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float s1 = cs[b][r], s2 = cq[b][r];
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
        if (li == 0) {
          const int cl = (wn * WN + b) * 16 + 4 * g + r;
          red[(wm * 2 + 0) * BN + cl] = s1;
          red[(wm * 2 + 1) * BN + cl] = s2;
        }
      }
    __syncthreads();
    for (int t = tid; t < 2 * BN; t += NW * 64) {
      const int which = t / BN, cl = t % BN;
      if (col0 + cl < cout) {
        double a = 0.0;
#pragma unroll
        for (int k = 0; k < WAVES_M; ++k) a += (double)red[(k * 2 + which) * BN + cl];
        stats[((long long)tile * 2 + which) * cout + col0 + cl] = a;
      }
    }
  }
