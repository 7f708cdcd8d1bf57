/*
 * libu3d_hip.so — C ABI of the MI355X-native Uni3DETR detection hot path.
 *
 * Every entry point: plain device pointers + explicit sizes + a hipStream_t; returns 0 or a negative
 * U3D_ERR_* code (u3d_strerror); never throws, never allocates device memory, never synchronises the
 * stream, keeps no global mutable state.  The caller (the ctypes host layer in uni3detr_amd/native.py,
 * or any other FFI) owns every buffer.  Citations `ref:` are paths under the reference repository
 * (zhenyuw16/Uni3DETR) naming the Python call site / upstream op each function replaces.
 *
 * Target: gfx950 only.
 */
#ifndef U3D_HIP_H_
#define U3D_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* u3d_stream;   /* == hipStream_t */

enum {
  U3D_OK = 0,
  U3D_ERR_ARG = -1,        /* bad argument (null pointer, size out of range)        */
  U3D_ERR_UNSUPPORTED = -2,/* shape / dtype combination not compiled in              */
  U3D_ERR_LAUNCH = -3,     /* hipGetLastError() != hipSuccess after a launch         */
  U3D_ERR_WORKSPACE = -4   /* workspace too small                                    */
};

enum { U3D_F32 = 0, U3D_BF16 = 1 };

int32_t u3d_version(void);
const char* u3d_strerror(int32_t code);

/* Measurement helpers (bench.py's roofline block): HIP events on the stream the kernels run on.  external != 0 records with
 * hipEventRecordExternal: inside a stream capture the record becomes an event-record NODE of the graph, so a pair of them brackets
 * one kernel as it runs inside every replay (elapsed time read after the replay).  Not part of the reference's interface. */
int32_t u3d_event_create(void** event);
int32_t u3d_event_record(void* event, int32_t external, u3d_stream s);
int32_t u3d_event_elapsed_ms(void* start, void* stop, float* ms);     /* both events must have completed */
int32_t u3d_event_destroy(void* event);

/* ------------------------------------------------------------------------------------------------
 * Occupancy lattice ("BitGrid").  One 64-bit word per 4x4x4 block of cells, bit = (z&3)*16+(y&3)*4+(x&3),
 * word = ((b*bz + z/4)*by + y/4)*bx + x/4 with bz=ceil(dz/4) etc.  `prefix` = exclusive popcount scan
 * (nwords+1 entries).  The rank of a set bit is the row index of that voxel at this sparse level.
 * Replaces the hash-table indice-pair builder of spconv (ref: models/pts_encoder/sparse_encoder_hd.py:9-12,
 * upstream ext.get_indice_pairs_*).
 * ---------------------------------------------------------------------------------------------- */
typedef struct u3d_bitgrid {
  void* words;      /* uint64 [nwords]   */
  void* prefix;     /* uint32 [nwords+1] */
  int32_t batch, dz, dy, dx;
  int32_t layout;   /* 0: 4x4x4-block words (rank = block-major order, used by the conv levels);
                       1: linear, one bit per cell in (b,z,y,x) order (rank = lexicographic = torch.unique(dim=0) order) */
  int32_t row_capacity; /* > 0: static-shape mode — rows are stored in buffers of this many rows; lookups (rank, neighbour
                           tables) return -1 for any row id >= row_capacity, so an overflowing level degrades to dropped
                           voxels instead of out-of-bounds gathers; 0: unlimited */
} u3d_bitgrid;

/* number of 64-bit words of a lattice: layout 0 batch * ceil(dz/4) * ceil(dy/4) * ceil(dx/4), layout 1 ceil(batch*dz*dy*dx / 64) */
int64_t u3d_bitgrid_nwords_layout(int32_t batch, int32_t dz, int32_t dy, int32_t dx, int32_t layout);

/* words must be zeroed by the caller (hipMemsetAsync) before marking. coors: int32 [n,4] (b,z,y,x);
 * rows with b < 0 are ignored. */
int32_t u3d_bitgrid_mark(const u3d_bitgrid* g, const int32_t* coors, int32_t n, u3d_stream s);

/* Mark every output site of a strided sparse conv whose window touches an active input:
 * o = (i + pad - kappa) / stride when divisible and inside `g` (ref: SURVEY.md App. A4 active-set rule;
 * sparse_encoder_hd.py:181-192).  n_dev: device int32 count of valid rows in `in_coors` (<= n_cap). */
int32_t u3d_bitgrid_mark_strided(const u3d_bitgrid* g, const int32_t* in_coors, const int32_t* n_dev,
                                 int32_t n_cap, const int32_t ksize[3], const int32_t stride[3],
                                 const int32_t pad[3], u3d_stream s);

/* prefix[] from words[]; scratch: uint32 [u3d_bitgrid_scan_scratch(nwords)] ; total count lands in
 * prefix[nwords] (device). */
int64_t u3d_bitgrid_scan_scratch(int64_t nwords);
int32_t u3d_bitgrid_scan(const u3d_bitgrid* g, void* scratch, u3d_stream s);

/* rank[i] = row index of coors[i] in g (or -1). */
int32_t u3d_bitgrid_rank(const u3d_bitgrid* g, const int32_t* coors, int32_t n, int32_t* rank, u3d_stream s);

/* Enumerate occupied cells in rank order: coors_out int32 [cap,4] (b,z,y,x); cap = rows available; rows [count, cap) = (-1,-1,-1,-1). */
int32_t u3d_bitgrid_coords(const u3d_bitgrid* g, int32_t* coors_out, int32_t cap, u3d_stream s);

/* u3d_bitgrid_scan followed by u3d_bitgrid_coords, with the same results.  Block-major grids of up to 2048 scan chunks take two
 * launches (chunk sums; then every workgroup sums the chunk sums in front of it itself, writes its prefixes and emits the
 * coordinates of its own words); the linear layout and larger grids run the two calls above. */
int32_t u3d_bitgrid_scan_coords(const u3d_bitgrid* g, void* scratch, int32_t* coors_out, int32_t cap, u3d_stream s);

/* Neighbour table ("rulebook") nbr[kappa][ld] int32, kappa = (kz*k1 + ky)*k2 + kx, -1 = no partner.
 *   mode 0 (gather/forward): partner of query q at kappa = target cell  q*stride - pad + kappa
 *       (SubMConv3d: stride 1, pad (k-1)/2, target == query grid; SparseConv3d forward: query = output sites).
 *   mode 1 (transposed/dgrad): partner = (q + pad - kappa)/stride when divisible (query = input sites,
 *       target = output grid).
 * n_dev: device count of valid query rows; rows >= *n_dev get -1.  ld >= n_cap.
 * Replaces upstream indice_pairs (ref: SURVEY.md §8a a-4; sparse_encoder_hd.py:195-199 builds them per conv). */
int32_t u3d_nbr_table(const u3d_bitgrid* target, const int32_t* q_coors, const int32_t* n_dev, int32_t n_cap,
                      const int32_t ksize[3], const int32_t stride[3], const int32_t pad[3], int32_t mode,
                      int32_t* nbr, int32_t ld, u3d_stream s);

/* The same table for ksize (3,3,3) on a block-major grid (layout 0), any stride, pad >= 0, both modes: the 27 targets of a row lie
 * in at most 2 x 2 x 2 words, which the row loads at once (u3d_nbr_table: 54 dependent loads).  U3D_ERR_UNSUPPORTED for the linear
 * layout, a negative pad, or a grid / table beyond 32-bit indices: the caller takes u3d_nbr_table. */
int32_t u3d_nbr_table_k3(const u3d_bitgrid* target, const int32_t* q_coors, const int32_t* n_dev, int32_t n_cap,
                         const int32_t stride[3], const int32_t pad[3], int32_t mode, int32_t* nbr, int32_t ld, u3d_stream s);

/* Same table for a DENSE lattice (every cell of [batch, dims] is a row; row id = lexicographic (b,z,y,x) index, i.e. the
 * memory order of a channels-last volume): lets the dense SECOND3D / SECOND3DFPN convolutions run on the same
 * implicit-GEMM kernels (ref: models/backbones/second_3d.py:52-76, models/necks/second3d_fpn.py:48-104). */
int32_t u3d_dense_nbr_table(int32_t batch, const int32_t q_dims[3], const int32_t t_dims[3], const int32_t ksize[3],
                            const int32_t stride[3], const int32_t pad[3], int32_t mode, int32_t* nbr, int32_t ld,
                            u3d_stream s);

/* Tables of a dense lattice restricted to the active rows of a sparse level that lives on it: for each of `count` (<= 4) source
 * tables src[b] int32 [kvol][ld_src] over the lattice [batch, dims] (u3d_dense_nbr_table; ld_src >= batch*dims), writes
 *   out[b][k][i] = src[b][k][lattice row of coords[i]]  for level rows i < min(*n_dev, n_cap),  -1 for n <= i < ld_out.
 * coords int32 [n_cap,4] (b,z,y,x); out int32 [count][kvol][ld_out], ld_out >= n_cap; src: HOST array of device pointers.  One
 * launch, integer only, no host read: shapes follow the capacity.  With the transposed tables of the convolutions that read the
 * level's dense() volume, their input and weight gradients run over the active rows only (ref: sparse_encoder_hd.py:133 feeding
 * models/backbones/second_3d.py:52-76). */
int32_t u3d_active_nbr_table(const int32_t* coords, const int32_t* n_dev, int32_t n_cap, int32_t batch, const int32_t dims[3],
                             const int32_t* const* src, int32_t count, int32_t ld_src, int32_t kvol, int32_t* out, int32_t ld_out,
                             u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Hard voxelization + mean VFE (ref: models/detectors/uni3detr.py:148-149; upstream mmcv Voxelization
 * hard mode + HardSimpleVFE).  Sequential semantics reproduced exactly: voxels in
 * first-appearance point order, first `max_points` points per voxel in point order, at most `max_voxels`
 * voxels per scene.
 *   points      f32 [n_total, nfeat], scenes concatenated; scene_off int32 [B+1] (device).  n_total and max_pts_per_scene are
 *               upper bounds: rows at or past scene_off[B] (read on the device) are spare capacity and never become points
 *   voxel_size/pc_range: host arrays (x,y,z) / (x0,y0,z0,x1,y1,z1)
 *   outputs (capacity B*max_voxels rows, scene-major, compacted):
 *     voxels  f32 [cap, max_points, nfeat] or NULL, coors int32 [cap,4] (b,z,y,x), num_points int32 [cap],
 *     mean    f32 [cap, nfeat] or NULL (sum of kept points / count),
 *     voxel_off int32 [B+1] device (row offsets per scene; voxel_off[B] = total)
 *   workspace: u3d_voxelize_hard_workspace(n_total, B) bytes, caller-zeroing NOT required.
 * ---------------------------------------------------------------------------------------------- */
int64_t u3d_voxelize_hard_workspace(int32_t n_total, int32_t batch, int32_t max_pts_per_scene);
int32_t u3d_voxelize_hard(const float* points, const int32_t* scene_off, int32_t batch, int32_t n_total,
                          int32_t max_pts_per_scene, int32_t nfeat, const float voxel_size[3],
                          const float pc_range[6], int32_t max_points, int32_t max_voxels,
                          float* voxels, int32_t* coors, int32_t* num_points, float* mean,
                          int32_t* voxel_off, void* workspace, int64_t workspace_bytes, u3d_stream s);
/* Same arguments, workspace and results; the first-appearance ranks are built in two levels over (scene, 1024-point chunk)
 * workgroups instead of by one workgroup per scene, and the scene offsets by the same launch. */
int32_t u3d_voxelize_hard_chunked(const float* points, const int32_t* scene_off, int32_t batch, int32_t n_total,
                                  int32_t max_pts_per_scene, int32_t nfeat, const float voxel_size[3],
                                  const float pc_range[6], int32_t max_points, int32_t max_voxels,
                                  float* voxels, int32_t* coors, int32_t* num_points, float* mean,
                                  int32_t* voxel_off, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Dynamic voxelization + DynamicSimpleVFE (ref: models/detectors/uni3detr.py:155-171; upstream mmcv Voxelization with
 * max_num_points=-1 and DynamicScatter(average_points=True)).
 *   u3d_voxelize_dynamic: per point (b, z, y, x) int32, or (b,-1,-1,-1) when out of range (same floor formula as hard mode).
 *   n_total is an upper bound, as for u3d_voxelize_hard: rows at or past scene_off[B] (read on the device) are spare capacity, never
 *   become points and get (-1,-1,-1,-1), which u3d_bitgrid_mark / u3d_bitgrid_rank skip; with scene_off[B] == n_total no such row exists.
 *   u3d_scatter_mean: feats[rank[i], :] = mean of points with that rank (rank < 0 skipped); sums f32 [V,nfeat] and
 *   counts int32 [V] must be zeroed by the caller; f32 atomics (as the upstream kernel), then an in-place divide: the bits of a
 *   mean follow the order in which its points arrive.
 *   u3d_scatter_mean_exact: the same mean and counts with bits that do NOT depend on that order - any permutation of the rows (with
 *   their ranks) and any two calls give identical bytes.  Per (voxel, feature): e = exponent of the largest |v| (integer atomicMax on
 *   the bit patterns), every v rounded once to the integer rint(v * 2^(shift - e)) and summed with 64-bit integer atomics (exact), the
 *   sum scaled back and divided by the count in f64, rounded once to f32.  shift = min(40, 61 - ceil(log2(n_total))), from the host's
 *   n_total (40 below 2^21 rows): n_total values below 2^(e+1) cannot overflow 63 bits.  Against the exact mean m of values v_i:
 *   |mean - m| <= 2^-23 |m| + 2^-shift max|v_i|.  A voxel with one point returns that point's bits (-0 as +0), a row without points 0
 *   and count 0; ranks < 0 or >= n_voxels are skipped.  mean f32 [V,nfeat] and counts int32 [V] are written in full, and neither
 *   they nor the workspace (u3d_scatter_mean_exact_workspace(V, nfeat) bytes, 8-byte aligned) need zeroing.  Four launches, one thread
 *   per (row, feature), no host read.  Non-finite values are out of contract: they are dropped or give any value, never a fault.
 *   U3D_ERR_ARG: a null pointer (points / rank may be null when n_total == 0), n_total < 0, nfeat <= 0, n_voxels <= 0;
 *   U3D_ERR_WORKSPACE: workspace_bytes below the query.  Both before any launch.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_voxelize_dynamic(const float* points, const int32_t* scene_off, int32_t batch, int32_t n_total, int32_t nfeat,
                             const float voxel_size[3], const float pc_range[6], int32_t* coors, u3d_stream s);
int32_t u3d_scatter_mean(const float* points, const int32_t* rank, int32_t n_total, int32_t nfeat, float* sums,
                         int32_t* counts, int32_t n_voxels, u3d_stream s);
int64_t u3d_scatter_mean_exact_workspace(int32_t n_voxels, int32_t nfeat);
int32_t u3d_scatter_mean_exact(const float* points, const int32_t* rank, int32_t n_total, int32_t nfeat, float* mean,
                               int32_t* counts, int32_t n_voxels, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Sparse convolution as output-stationary implicit GEMM over the neighbour table
 *   out[m,:] = sum_kappa  in[nbr[kappa][m], :] @ W[kappa]        (W: [K, Cin, Cout], K = 27 or 1)
 * Covers SubMConv3d, SparseConv3d forward (nbr mode 0) and both dgrads (nbr mode 1 + transpose_w=1,
 * which reads W[kappa] as [Cout_of_fwd x Cin_of_fwd]^T).  nbr == NULL means identity (1x1x1 conv).
 * (ref: sparse_encoder_hd.py:71-104,181-199; upstream ext.indice_conv_forward/backward.)
 * dtype U3D_F32: exact-f32 MFMA (v_mfma_f32_16x16x4_f32); U3D_BF16: bf16 operands, f32 accumulate.
 * n_out_dev: device count of valid output rows (<= n_out_cap).
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_spconv_fwd(const void* in, const void* w, const int32_t* nbr, int32_t ld, void* out,
                       const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                       int32_t transpose_w, int32_t dtype, u3d_stream s);

/* Second-generation bf16 implicit-GEMM kernels: same contract as u3d_spconv_fwd with dtype U3D_BF16.  Which kernel serves a shape is
 * ONE decision, the launch plan, and a caller ASKS for it (u3d_igemm_fwd_plan, host only: no launch, no device access beyond a
 * cached CU-count query) instead of trying launches: U3D_ERR_UNSUPPORTED there = no implicit-GEMM kernel serves the shape, take
 * u3d_spconv_fwd.  nmajor: the weights are [K][Cout][Cin] (transpose_w = 1 of the launch); epi: what the launch does besides the
 * convolution.  Asked with U3D_FWD_EPI_ADD for a shape whose kernel has no addend epilogue, the answer is the PLAIN plan with
 * takes_addend = 0 (the caller adds afterwards); U3D_FWD_EPI_STATS is U3D_ERR_UNSUPPORTED where no kernel with a statistics epilogue
 * serves the shape (use the PLAIN launch + u3d_bn_stats); U3D_FWD_EPI_AFFINE is the plan of u3d_igemm_fwd_affine_bf16.
 *   family   U3D_FWD_FAM_CONV_IN the encoder's 8 -> 16 input convolution; DIRECT the direct-operand kernels of the narrow 27-offset
 *            levels; GLDS the LDS-DMA kernels (n-major weights, channel counts % 64); REG the register-staged kernels
 *   kernel   index within the family.  DIRECT: shape * 4 + variant, shapes 16/32 -> 16, 16/32 -> 32, 16/32 -> 64, 64 -> 16, 64 -> 32,
 *            variants k-major, n-major, n-major + statistics, n-major f32 output.  GLDS: 0 two-phase 256 x 256, 1 / 2 eight-phase
 *            256 / 192 x 256, 3 / 4 eight-phase 256 / 192 x 128, 5 two-phase 256 x 128, 6 128 x 128, 7 128 x 64.  REG: 0 / 1 k- / n-major
 *            256 x 16, 2 / 3 256 x 32, 4 / 5 256 x 64 (cin 16 / 32), then k-major 6 256 x 256, 7 256 x 128, 8 128 x 64
 *   rows, cols  its tile
 *   partials, rows_per_partial  the statistics a STATS launch writes: [partials][2][Cout], one per rows_per_partial rows (=
 *            rows_per_block of u3d_bn_finalize_partials), or with rows_per_partial = 0 one per WAVE of the direct-operand kernels
 *            (every partial counts).  u3d_igemm_fwd_split_bf16 writes the same row-tile layout wherever it serves a shape. */
enum { U3D_FWD_EPI_PLAIN, U3D_FWD_EPI_ADD, U3D_FWD_EPI_STATS, U3D_FWD_EPI_AFFINE, U3D_FWD_EPI_COUNT };
enum { U3D_FWD_FAM_NONE, U3D_FWD_FAM_CONV_IN, U3D_FWD_FAM_DIRECT, U3D_FWD_FAM_GLDS, U3D_FWD_FAM_REG, U3D_FWD_FAM_COUNT };
typedef struct u3d_fwd_plan_info {
  int32_t family, kernel, rows, cols, partials, rows_per_partial, takes_addend;
} u3d_fwd_plan_info;
int32_t u3d_igemm_fwd_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr, int32_t nmajor, int32_t epi,
                           u3d_fwd_plan_info* info);
/* The launch that follows the PLAIN / ADD / STATS plan.  addend: NULL or bf16 [n_out_cap][Cout], summed in by the epilogue before
 * the one rounding (the input gradient of a residual block's first conv with the residual branch's gradient; ref: SparseBasicBlock's
 * `out += identity`, mmdet3d - autograd adds the two gradients with a separate element-wise kernel); needs a table.  stats: NULL or
 * f64 [partials][2][Cout], the BatchNorm statistics of the (bf16-rounded) output in the STATS plan's layout: feeds
 * u3d_bn_finalize_partials and saves the separate statistics pass over the conv output (ref: conv -> BatchNorm pairs of
 * sparse_encoder_hd.py:71-104 and second_3d.py:52-76).  Both: U3D_ERR_ARG.  U3D_ERR_UNSUPPORTED: the plan does not serve the shape,
 * or not with that epilogue - the caller did not ask.  The entry and the query agree for every argument, n_out_cap <= 0 included. */
int32_t u3d_igemm_fwd_bf16(const void* in, const void* w, const int32_t* nbr, int32_t ld, void* out,
                           const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                           int32_t transpose_w, const void* addend, double* stats, u3d_stream s);
/* nn.Linear on rows with the same kernel: out[M,N] = act(x[M,K] @ W[N,K]^T + bias); bf16 x/W/out, f32 bias (may be NULL),
 * relu != 0 applies max(.,0).  (ref: the Linear layers of models/utils/uni3detr_transformer.py:18-30,142-143,248-260 and
 * models/dense_heads/uni3detr_head.py:365-387.)  U3D_ERR_UNSUPPORTED unless K % 64 == 0 and N % 64 == 0. */
int32_t u3d_linear_bf16(const void* x, const void* w, const float* bias, int32_t relu, void* out, const int32_t* m_dev,
                        int32_t m_cap, int32_t k, int32_t n, u3d_stream s);
/* Inference: eval-mode BatchNorm folded into the convolution in front of it.  In eval mode BatchNorm is y = x * scale + shift per
 * channel, scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale (ref: the conv -> BatchNorm -> ReLU chains of
 * sparse_encoder_hd.py:71-104, second_3d.py:52-76, second3d_fpn.py:60-90 under model.eval()).
 *
 * u3d_bn_fold_batched folds every pair of a model in ONE launch.  jobs: DEVICE array of njobs u3d_bn_fold_job records
 * (u3d_bn_fold_job_bytes() = its size), total_blocks = the sum of u3d_bn_fold_job_blocks(kvol, cout, cin) over all jobs. */
typedef struct u3d_bn_fold_job {
  const float* w;          /* the f32 master weight, element (k, co, ci) at w[k * sk + co * sa + ci * sb] (element strides: the
                              checkpoint layouts [kD,kH,kW,Cin,Cout] and [Cout,Cin,kD,kH,kW] are read in place) */
  const float* gamma;      /* gamma / beta / mean / var: f32 [cout] */
  const float* beta;
  const float* mean;
  const float* var;
  uint16_t* w_folded;      /* written: bf16 [kvol][cout][cin] (the n-major layout of the LDS-DMA kernels) = bf16_rne(w * scale[co]),
                              scale computed in f32; 8-byte aligned */
  float* shift;            /* written: f32 [cout]; may be NULL with scale_only */
  int64_t sk, sa, sb;
  float eps;
  int32_t kvol, cout, cin; /* cin % 4 == 0 */
  int32_t scale_only;      /* != 0: only w_folded is written (a second copy of a layer's weights whose shift another job leaves) */
  int32_t first_block;     /* the sum of u3d_bn_fold_job_blocks(kvol, cout, cin) over the jobs before this one */
} u3d_bn_fold_job;
int64_t u3d_bn_fold_job_bytes(void);
int32_t u3d_bn_fold_job_blocks(int32_t kvol, int32_t cout, int32_t cin);
int32_t u3d_bn_fold_batched(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s);
/* out = act(conv(in; w_folded) + shift[col]) in one pass: bf16 in / w_folded / out, f32 shift [cout] (required), relu != 0 applies
 * max(., 0).  w_folded is n-major [kvol][Cout][Cin] (u3d_bn_fold_batched); nbr / ld as u3d_igemm_fwd_bf16 (NULL for kvol == 1).  The
 * kernels are the LDS-DMA kernels of u3d_igemm_fwd_bf16 with the epilogue u3d_linear_bf16 uses; a direct-operand kernel is never
 * picked.  Rows at or past *n_out_dev are left untouched.  With shift == 0 and relu == 0 the result equals u3d_igemm_fwd_bf16
 * (transpose_w = 1) on the same weights bit for bit.  U3D_ERR_UNSUPPORTED unless Cin % 64 == 0 and Cout % 64 == 0. */
int32_t u3d_igemm_fwd_affine_bf16(const void* in, const void* w_folded, const int32_t* nbr, int32_t ld, const float* shift, int32_t relu,
                                  void* out, const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                                  u3d_stream s);
/* FP8 inference of the wide dense convolutions (fp8.hip, igemm_fp8.hip).  Format: OCP e4m3fn.  Every scale is a power of two.
 * Quantiser q(x, e) = e4m3_rne(clamp(x * 2^-e, -448, 448)): saturating, ties to even, NaN -> a NaN code, +-0 -> 0x00 / 0x80.
 *
 * u3d_quant_rows_e4m3: q bytes [n_cap][c] = q(x bf16 [n_cap][c], *e_dev) for the first min(*n_dev, n_cap) rows; the other rows are not
 * written.  c % 8 == 0 (else U3D_ERR_UNSUPPORTED), x 16-byte and q 8-byte aligned.
 * u3d_absmax_rows: *slot = max(*slot, max |x|) over the first min(*n_dev, n_cap) rows of x bf16 [n_cap][c] - an unsigned integer
 * atomicMax on the bit pattern: exact, order independent, no host sync.  A NaN or Inf input leaves +Inf.  The caller zeroes the slot.
 * c % 8 == 0.
 * u3d_bn_fold_fp8_batched: u3d_bn_fold_batched's job-table shape, ONE launch for all pairs, one workgroup per (pair, output channel).
 * jobs: DEVICE array of njobs u3d_bn_fold_fp8_job records (below; u3d_bn_fold_fp8_job_bytes() = its size), total_blocks = the sum of
 * cout over all jobs.  wf = w * gamma / sqrt(var + eps) in f32 is the product u3d_bn_fold_batched rounds to bf16.
 * u3d_igemm_fwd_affine_fp8: out bf16 = bf16_rne(act(conv(in; qw) * colscale[col] + shift[col])), e4m3 in [n_in][cin] and qw
 * [kvol][cout][cin], f32 accumulation on the block-scaled MFMA with unit block scales, colscale / shift f32 [cout] (16-byte aligned),
 * the other arguments as u3d_igemm_fwd_affine_bf16.  An absent neighbour (-1) contributes exact zeros.  Rows at or past *n_out_dev are
 * left untouched.  Serves what u3d_igemm_fwd_fp8_plan serves, else U3D_ERR_UNSUPPORTED.
 * u3d_igemm_fwd_fp8_plan (host only): the kernel (U3D_FWD_FP8_K_*) and its tile (*rows x *cols) for a shape - cin % 128 == 0,
 * cout % 128 == 0, kvol > 1 with a table or kvol == 1 without one - or U3D_ERR_UNSUPPORTED.  u3d_igemm_fwd_plan and its epi values know nothing of it. */
enum { U3D_FWD_FP8_K_256X256, U3D_FWD_FP8_K_192X256, U3D_FWD_FP8_K_256X256_ROWS, U3D_FWD_FP8_K_COUNT };
int32_t u3d_quant_rows_e4m3(const void* x, void* q, const int32_t* n_dev, int32_t n_cap, int32_t c, const int32_t* e_dev, u3d_stream s);
int32_t u3d_absmax_rows(const void* x, const int32_t* n_dev, int32_t n_cap, int32_t c, float* slot, u3d_stream s);
typedef struct u3d_bn_fold_fp8_job {
  const float* w;          /* w, sk / sa / sb, gamma .. var, eps: as in u3d_bn_fold_job */
  const float* gamma;
  const float* beta;
  const float* mean;
  const float* var;
  uint8_t* qw;             /* written: e4m3 [kvol][cout][cin] = q(wf, e_w[co]), rounded ONCE from f32 */
  int32_t* e_w;            /* written: int32 [cout], the smallest e with max |wf[:, co, :]| <= 448 * 2^e (0 for an all-zero channel) */
  float* shift;            /* written: f32 [cout] = beta - mean * scale */
  int64_t sk, sa, sb;
  float eps;
  int32_t kvol, cout, cin;
  int32_t first_block;     /* the sum of cout over the jobs before this one */
} u3d_bn_fold_fp8_job;
int64_t u3d_bn_fold_fp8_job_bytes(void);
int32_t u3d_bn_fold_fp8_batched(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s);
int32_t u3d_igemm_fwd_affine_fp8(const void* in, const void* qw, const int32_t* nbr, int32_t ld, const float* colscale,
                                 const float* shift, int32_t relu, void* out, const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin,
                                 int32_t cout, int32_t kvol, u3d_stream s);
int32_t u3d_igemm_fwd_fp8_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr, int32_t* kernel, int32_t* rows,
                               int32_t* cols);
/* Split-bf16 convolution: f32-grade products on the bf16 matrix pipe, for the modules the reference keeps in fp32 (ref:
 * models/pts_encoder/sparse_encoder_hd.py:62-64 fp16_enabled=False, models/detectors/uni3detr.py:150-151; SECOND3D is never wrapped in
 * auto_fp16).  An f32 row matrix x travels as two bf16 planes (u3d_split_rows_f32: hi = bf16(x), lo = bf16(x - hi), stacked as rows
 * [hi ; lo] with a plane stride of n_cap rows) and x.w ~ hi.wh + hi.wl + lo.wh with f32 accumulation.  The caller passes the three
 * products as three sets of offsets: nbr int32 [kvol3][ld] = (nbr, nbr, nbr + n_in_cap), w bf16 [kvol3][Cout][Cin] = (wh, wl, wh),
 * kvol3 = 3 x offsets.  out is F32 [n_out_cap][Cout]; stats: NULL or f64 [partials][2][Cout] (the STATS plan of u3d_igemm_fwd_plan(.., kvol3, 1, 1,
 * ..)) per-tile BatchNorm sums of the f32 output; addend: NULL or f32 [n_out_cap][Cout] summed into the result in the epilogue (the
 * residual / fan-out gradient sums of the input gradients, as the addend of u3d_igemm_fwd_bf16).  U3D_ERR_UNSUPPORTED unless Cin % 64 == 0 and
 * Cout % 64 == 0. */
int32_t u3d_igemm_fwd_split_bf16(const void* in, const void* w, const int32_t* nbr, int32_t ld, float* out, const int32_t* n_out_dev,
                                 int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol3, double* stats, const float* addend, u3d_stream s);
/* The same product on the NARROW 27-offset sparse levels (cin, cout in {16, 32, 64}, not 64 -> 64; the encoder's stride-1 / stride-2
 * stages, ref: sparse_encoder_hd.py:140-214): three launches of the direct-operand kernel (igemm_direct.hip) accumulating into one f32
 * output - no tripled table: in = the bf16 planes [2 * n_in_cap][cin], w3 = (wh, wl, wh) n-major [3 * 27][cout][cin], nbr / ld as
 * u3d_igemm_fwd_bf16 (ld < 0: the forward table read reversed = the SubM input gradient), out f32 [n_out_cap][cout]. */
int32_t u3d_igemm_direct_split_bf16(const void* in, const void* w3, const int32_t* nbr, int32_t ld, float* out, const int32_t* n_out_dev,
                                    int32_t n_out_cap, int32_t n_in_cap, int32_t cin, int32_t cout, u3d_stream s);
/* conv -> eval-mode BatchNorm (-> + residual) (-> ReLU) on the same narrow levels in one launch of the direct-operand kernel (the
 * inference path; what u3d_igemm_fwd_affine_bf16 is for the wide ones): out = bf16_rne(act(conv(in; w_folded) + shift[col] +
 * addend[m][col])), f32 until the one rounding, in that order.  w_folded bf16 n-major [27][cout][cin] (u3d_bn_fold_batched), shift f32
 * [cout] (required, 16-byte aligned), addend NULL or bf16 [n_out_cap][cout], relu != 0 applies max(., 0); nbr / ld as
 * u3d_igemm_fwd_bf16.  Rows at or past *n_out_dev are left untouched.  With shift == 0 and relu == 0 the result equals
 * u3d_igemm_fwd_bf16 (transpose_w = 1, without / with the addend) on the same weights.  U3D_ERR_UNSUPPORTED unless cin, cout in
 * {16, 32, 64} and not 64 -> 64 (27 offsets are implied). */
int32_t u3d_igemm_direct_affine_bf16(const void* in, const void* w_folded, const int32_t* nbr, int32_t ld, const float* shift,
                                     int32_t relu, const void* addend, void* out, const int32_t* n_out_dev, int32_t n_out_cap,
                                     int32_t cin, int32_t cout, u3d_stream s);
/* The weight side of the same product: dst bf16 [3][k][a][b] = (hi, lo, hi) of the f32 element src[ik * sk + ia * sa + ib * sb]
 * (element strides: the checkpoint layouts [kD,kH,kW,Cin,Cout] and [Cout,Cin,kD,kH,kW] are read in place). */
int32_t u3d_split3_weights(const float* src, int64_t sk, int64_t sa, int64_t sb, int32_t k, int32_t a, int32_t b, void* dst, u3d_stream s);
/* hi / lo bf16 planes (as u3d_split_rows_f32, all rows live) of up to 32 strided f32 row matrices in one launch; `jobs` is a HOST
 * structure (its contents travel in the kernel arguments; first_block is filled by the call). */
typedef struct U3dSplitRowsJobs {
  const float* src[32];
  void* dst[32];
  int32_t ld[32], rows[32], cols[32];
  int32_t first_block[33];
  int32_t njobs;
} U3dSplitRowsJobs;
int32_t u3d_split_rows_batch(const U3dSplitRowsJobs* jobs, u3d_stream s);
/* out = (a + b) + c over n f32 elements (n % 4 == 0, 16-byte aligned): the three partial weight gradients of a split-bf16 product. */
int32_t u3d_sum3_f32(const float* a, const float* b, const float* c, float* out, int64_t n, u3d_stream s);
/* u3d_split3_weights for every convolution weight of a step in ONE launch.  jobs: DEVICE array of njobs u3d_split3_job records
 * (u3d_split3_job_bytes() = its size); total_blocks = the sum of u3d_split3_job_blocks(K, A, B) over all jobs. */
typedef struct u3d_split3_job {
  const float* src;        /* src, sk / sa / sb, K / A / B and dst: u3d_split3_weights' src, strides, k / a / b and dst */
  uint16_t* dst;
  int64_t sk, sa, sb;
  int32_t K, A, B;
  int32_t first_block;     /* the sum of u3d_split3_job_blocks(K, A, B) over the jobs before this one */
} u3d_split3_job;
int64_t u3d_split3_job_bytes(void);
int32_t u3d_split3_job_blocks(int32_t k, int32_t a, int32_t b);
int32_t u3d_split3_weights_batch(const void* jobs, int32_t njobs, int32_t total_blocks, u3d_stream s);
/* dst bf16 [2 * n_cap][c]: rows [0, n) = bf16(x), rows [n_cap, n_cap + n) = bf16(x - hi), n = min(*n_dev, n_cap); c % 4 == 0. */
int32_t u3d_split_rows_f32(const float* x, const int32_t* n_dev, int32_t n_cap, int32_t c, void* dst, u3d_stream s);
/* Output-stationary path of the 27-offset submanifold convs at 64 -> 64 channels (the stride-4 stage's SparseBasicBlocks, ref:
 * sparse_encoder_hd.py:106-138) and of the <= 27-offset convs at 128 -> 128 (the stride-8 stage; with 9 offsets the stride-1 (1,3,3)
 * convs of the dense stack, SECOND3D's 128-channel branch, ref: second_3d.py:52-76, whose tables are static).  Rows are numbered in
 * 4x4x4-block-major order, so the 27 x 128 table entries of a 128-row tile name only a few hundred DISTINCT rows.
 * Tables.  u3d_subm_halo_build (once per level and step) leaves, per tile, the sorted distinct rows tile_rows int32 [tiles][3460]
 * (slot 0 = the all-zero row), their number tile_cnt int32 [tiles] and the table rewritten as 16-bit slots loc u16 [tiles][27][128]
 * (within a (tile, offset): entry (r % 16) * 8 + r / 16 for row r; 27 slots per tile whatever kvol).  They do not depend on the
 * channel count.  u3d_subm_halo_sizes gives the element counts for n_cap rows (the build returns U3D_ERR_UNSUPPORTED above 869 k
 * rows: its per-tile row bitmap lives in LDS).  u3d_halo_tables names them for the entries that read them.
 * Weights.  u3d_subm_halo_wpack: n-major bf16 [kvol][c][c] -> MFMA fragment order, same size; _batched packs n weights in one launch
 * from device arrays of n source / destination pointers (the per-step shadow refresh packs every SubM weight of a width, forward and
 * transposed, at once).
 * Shapes (every entry with a c): c == 64 with kvol == 27, or c == 128 with 1 <= kvol <= 27; anything else U3D_ERR_UNSUPPORTED.
 * u3d_subm_halo_conv_bf16: in / out / addend bf16 [n][c], addend nullable, stats nullable f64 [tiles][2][c] (128 rows per partial,
 * as u3d_bn_finalize_partials takes them).
 *   shift == NULL: what u3d_igemm_fwd_bf16 (transpose_w = 1; plain, with an addend, with statistics) computes from the table.
 *     krev != 0 reads the offsets reversed (the transposed table of a SubM layer, or of a stride-1 "same" conv on a lattice: input
 *     gradients, pass [K][Cin][Cout]).  relu must be 0.
 *   shift != NULL (f32 [c], 16-byte aligned): the forward with an eval-mode BatchNorm folded in (the inference path).  w_packed = the
 *     pack of the FOLDED weights (u3d_bn_fold_batched), out = bf16_rne(act(conv + shift[col] + addend[m][col])) - f32 until the one
 *     rounding, in that order; the addend is the residual block's identity; relu != 0 applies max(., 0).  Rows at or past *n_dev are
 *     left untouched.  Forward only and without statistics: krev != 0 or stats != NULL is U3D_ERR_ARG.  With a zero shift and relu == 0
 *     the result equals the shift == NULL call on the same packed weights.  The epilogue is a compile-time variant of the kernels:
 *     shift == NULL runs the code it ran without it.
 * u3d_subm_halo_wgrad64_bf16: weight gradient of the 64 -> 64 layers from the same tables (kvol == 27): dw f32 [27][64][64]
 * (spconv-1.x layout) = sum over rows m of x[nbr_k(m)]^T dy[m]; x / dy bf16 [n][64].  Persistent workgroups, both MFMA operands by
 * transpose reads out of the staged distinct rows / the dy tile, offsets split over four workgroup groups, one f32 partial per
 * workgroup summed in a fixed order (deterministic).  workspace: u3d_subm_halo_wgrad64_workspace() bytes.  Replaces
 * u3d_igemm_wgrad_bf16 for this shape (ref: the weight half of spconv's indice_conv_backward for sparse_encoder_hd.py:106-138).
 * max_slots (conv and wgrad): 0 = the stage buffer's capacity; a lower value only forces the fall-back paths for tiles with more
 * distinct rows (test hook). */
typedef struct u3d_halo_tables {      /* HOST structure, read during the call */
  const int32_t* tile_rows;
  const uint16_t* loc;
  const int32_t* tile_cnt;
  const int32_t* n_dev;
  int32_t n_cap, kvol;
} u3d_halo_tables;
int32_t u3d_subm_halo_sizes(int32_t n_cap, int64_t* tile_rows_elems, int64_t* loc_elems, int32_t* tiles);
int32_t u3d_subm_halo_build(const int32_t* nbr, int32_t ld, const int32_t* n_dev, int32_t n_cap, int32_t* tile_rows,
                            uint16_t* loc, int32_t* tile_cnt, int32_t kvol, u3d_stream s);
int32_t u3d_subm_halo_wpack(const void* w_nmajor, void* w_packed, int32_t c, int32_t kvol, u3d_stream s);
int32_t u3d_subm_halo_wpack_batched(const void* const* srcs_dev, void* const* dsts_dev, int32_t n, int32_t c, int32_t kvol, u3d_stream s);
int32_t u3d_subm_halo_conv_bf16(const void* in, const void* w_packed, const u3d_halo_tables* t, int32_t c, int32_t krev,
                                const void* addend, void* out, double* stats, const float* shift, int32_t relu,
                                int32_t max_slots, u3d_stream s);
int64_t u3d_subm_halo_wgrad64_workspace(void);
int32_t u3d_subm_halo_wgrad64_bf16(const void* x, const void* dy, const u3d_halo_tables* t, float* dw, void* workspace,
                                   int64_t workspace_bytes, int32_t max_slots, u3d_stream s);
int64_t u3d_igemm_wgrad_bf16_workspace(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol);
/* out_layout 0: dw [K][Cin][Cout] (spconv-1.x / this library's layout); 1: dw [Cout][Cin][K] (nn.Conv3d's [Cout,Cin,kD,kH,kW]);
 * 2: dw [Cin][Cout][K] - for a call with the operands' roles exchanged (in = dy gathered through a transposed table restricted to
 * the active input rows, u3d_active_nbr_table; dout = those rows' features; n_out = their count; cin / cout = the convolution's
 * Cout / Cin), which again lands in nn.Conv3d's layout.  LDS-DMA / register-staged families only, kvol <= 27. */
int32_t u3d_igemm_wgrad_bf16(const void* in, const void* dout, const int32_t* nbr, int32_t ld, float* dw,
                             const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                             int32_t out_layout, void* workspace, int64_t workspace_bytes, u3d_stream s);
/* The launch plan of u3d_igemm_wgrad_bf16 for a shape (host only; the counterpart of u3d_igemm_fwd_plan): *kernel = the kernel
 * family (1 conv-in 8 -> 16, 2 narrow 16/32-channel, 3 / 4 eight- / two-phase LDS-DMA 256, 5 / 6 LDS-DMA 128 / 64, 7 / 8 register-staged
 * 32 / 16), *tile its square channel tile (0: conv-in, narrow), *nsplit the f32 partials it sums, *workspace their bytes (what
 * u3d_igemm_wgrad_bf16_workspace returns).  U3D_ERR_UNSUPPORTED where the launch returns it. */
int32_t u3d_igemm_wgrad_plan(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol, int32_t has_nbr, int32_t out_layout,
                             int32_t* kernel, int32_t* tile, int32_t* nsplit, int64_t* workspace);

/* dW[kappa] = sum_m in[nbr[kappa][m],:]^T @ dout[m,:]   (f32 accumulate, dW f32 [K,Cin,Cout], overwritten).
 * workspace: u3d_spconv_wgrad_workspace() bytes. */
int64_t u3d_spconv_wgrad_workspace(int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol);
int32_t u3d_spconv_wgrad(const void* in, const void* dout, const int32_t* nbr, int32_t ld, float* dw,
                         const int32_t* n_out_dev, int32_t n_out_cap, int32_t cin, int32_t cout, int32_t kvol,
                         int32_t dtype, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* out[c] = sum_r x[r, c] over a dense [n, C] matrix (f32 or bf16 in, f32 out, fixed summation order): the bias gradient of every
 * nn.Linear of the decoder / head (ref: uni3detr_transformer.py:93-214, uni3detr_head.py:95-125 — autograd's sum-to-size there). */
int64_t u3d_colsum_workspace(int32_t n, int32_t c);
int32_t u3d_colsum(const void* x, int32_t n, int32_t c, int32_t dtype, float* out, void* workspace,
                   int64_t workspace_bytes, u3d_stream s);

/* Batched forms for the parameter gradients of the decoder / head linears (one shape per call, count <= 48 / 64): all weight
 * gradients dW_b = in_b^T @ dout_b (bf16 [n_rows, cin] x [n_rows, cout] -> f32 [cin, cout]) in two launches, all bias gradients
 * in two launches; pointer arrays are HOST arrays of device pointers (they travel in the kernel arguments).  CONSECUTIVE batch
 * slots that name the same output are SUMMED into it in a fixed order (a linear shared by several decoder layers: ref
 * models/utils/uni3detr_transformer.py:276-283 ref_point_head / query_scale) - no separate accumulate launches. */
int64_t u3d_wgrad_batched_workspace(int32_t count, int32_t n_rows, int32_t cin, int32_t cout);
int32_t u3d_wgrad_batched_bf16(const void* const* in, const void* const* dout, float* const* dw, int32_t count,
                               const int32_t* n_dev, int32_t n_rows, int32_t cin, int32_t cout, void* workspace,
                               int64_t workspace_bytes, u3d_stream s);
int64_t u3d_colsum_batched_workspace(int32_t count, int32_t n, int32_t c);
int32_t u3d_colsum_batched(const void* const* x, float* const* out, int32_t count, int32_t n, int32_t c, int32_t dtype,
                           void* workspace, int64_t workspace_bytes, u3d_stream s);

/* Weight gradient of a linear layer with <= 16 input or output features (bf16 dy [m, n], x [m, k]): partial f32
 * [u3d_skinny_wgrad_chunks(m)][n*k]; the column sums over the chunks are dW [n][k] (u3d_colsum / u3d_colsum_batched). */
int32_t u3d_skinny_wgrad_chunks(int32_t m);
int32_t u3d_skinny_wgrad_bf16(const void* dy, const void* x, int32_t m, int32_t n, int32_t k, float* partial, u3d_stream s);
/* `count` (<= 32) such products over the same m rows in one launch; dy / x / partial / n / k are HOST arrays of length count;
 * dy_skinny != 0: every n[i] <= 32 (thread = column of x), else every k[i] <= 32 (thread = column of dy). */
int32_t u3d_skinny_wgrad_batched(const void* const* dy, const void* const* x, float* const* partial, const int32_t* n, const int32_t* k,
                                 int32_t count, int32_t m, int32_t dy_skinny, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * BatchNorm1d over sparse rows [n, C] (training statistics) with optional residual add and ReLU
 * (ref: sparse_encoder_hd.py:40; upstream make_sparse_convmodule / SparseBasicBlock).
 * stats: sums f64 [2*C] = (sum x, sum x^2), deterministic two-stage reduction.
 * ---------------------------------------------------------------------------------------------- */
int64_t u3d_bn_stats_workspace(int32_t n_cap, int32_t c);
int32_t u3d_bn_stats(const void* x, const int32_t* n_dev, int32_t n_cap, int32_t c, int32_t dtype,
                     double* sums, void* workspace, int64_t workspace_bytes, u3d_stream s);
/* sums -> mean, invstd = 1/sqrt(biased var + eps); optional nn.BatchNorm1d running-stat update
 * (running = (1-m)*running + m*batch, unbiased variance) and num_batches_tracked += 1. */
int32_t u3d_bn_finalize(const double* sums, const int32_t* n_dev, int32_t n_cap, int32_t c, float eps, float momentum,
                        float* running_mean, float* running_var, int64_t* num_batches, float* mean, float* invstd,
                        u3d_stream s);
/* u3d_bn_stats + u3d_bn_finalize in two launches (stage 2 of the reduction fused with the finalisation); same results. */
int32_t u3d_bn_forward_stats(const void* x, const int32_t* n_dev, int32_t n_cap, int32_t c, int32_t dtype, float eps,
                             float momentum, float* running_mean, float* running_var, int64_t* num_batches, float* mean,
                             float* invstd, void* workspace, int64_t workspace_bytes, u3d_stream s);
/* Same finalisation from statistics the producing convolution already reduced per row tile (u3d_igemm_fwd_bf16 with stats):
 * partial f64 [nblocks][2][C], tile b = rows [b*rows_per_block, (b+1)*rows_per_block). */
int32_t u3d_bn_finalize_partials(const double* partial, int32_t nblocks, int32_t rows_per_block, const int32_t* n_dev,
                                 int32_t n_cap, int32_t c, float eps, float momentum, float* running_mean, float* running_var,
                                 int64_t* num_batches, float* mean, float* invstd, u3d_stream s);
/* y = relu?( (x-mean)*invstd*gamma + beta (+ residual) ); mean/invstd/gamma/beta f32 [C].
 * row_map (nullable; all three functions): y / dy are stored in a permuted row order, row r of x <-> row row_map[r] of y / dy
 * (a bijection of [0, n)).  The (1,s,s)/(1,s,s) transposed convolutions of the FPN (ref: second3d_fpn.py:60-75) produce their
 * rows tap-major; their BatchNorm writes the lattice order directly instead of a separate row gather.  Requires no residual /
 * dres and C % 8 == 0 (bf16) or C % 4 == 0 (f32).
 * post_add (nullable, u3d_bn_apply): a tensor of y's shape and row order added AFTER the activation, y = act(..) + post_add - the
 * running sum of the FPN's upsampled levels (ref: second3d_fpn.py:131-134) without a separate add pass.
 * planes (nullable; u3d_bn_apply and u3d_bn_bwd_apply, F32 rows): the pass ALSO leaves its output (y / dx) as the hi / lo bf16 planes
 * of a split-bf16 product (planes: bf16 [2 * n_cap][C] in the output's row order, rows n .. n_cap of both planes zero - exactly what
 * u3d_split_rows_f32 of the output would hold): the BatchNorm of the fp32 modules (ref: sparse_encoder_hd.py:62-64, second_3d.py:52-76
 * - kept in fp32 by the reference) hands its consumer convolution the planes without a further pass over the tensor; the backward
 * hands the producer convolution the planes of dy.  With planes, U3D_ERR_UNSUPPORTED and nothing launched when the dtype is not
 * U3D_F32, C does not fit the vector kernels (C % 4, (C / 4) | 256), a column parameter is not 16-byte aligned, or row_map comes with
 * a residual / dres: run the plain pass + the split. */
int32_t u3d_bn_apply(const void* x, const float* mean, const float* invstd, const float* gamma,
                     const float* beta, const void* residual, int32_t relu, void* y, void* planes,
                     const int32_t* n_dev, int32_t n_cap, int32_t c, int32_t dtype, const int32_t* row_map, const void* post_add,
                     u3d_stream s);
/* backward: given dy (grad wrt y), y (for relu mask), x: sums f64 [2*C] = (sum g, sum g*xhat) where
 * g = dy * (y>0 if relu).  y may be NULL when relu is set and the forward had NO residual: the mask is then recomputed as
 * (x-mean)*invstd*gamma+beta > 0 (the forward's own expression; gamma/beta required) - one tensor less to stream.
 * sums_f32 (nullable, f32 [2*C]): the same sums rounded to f32 = (d beta, d gamma), the parameter gradients as torch stores them. */
int32_t u3d_bn_bwd_stats(const void* dy, const void* y, const void* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, int32_t relu, const int32_t* n_dev, int32_t n_cap,
                         int32_t c, int32_t dtype, double* sums, void* workspace, int64_t workspace_bytes,
                         const int32_t* row_map, float* sums_f32, u3d_stream s);
/* dx = gamma*invstd*( g - sum_g/n - xhat*sum_gx/n ); dres = g (optional, may be NULL).  y NULL: as above (beta required). */
int32_t u3d_bn_bwd_apply(const void* dy, const void* y, const void* x, const float* mean, const float* invstd,
                         const float* gamma, const float* beta, const double* sums, int32_t relu, void* dx, void* dres, void* planes,
                         const int32_t* n_dev, int32_t n_cap, int32_t c, int32_t dtype, const int32_t* row_map, u3d_stream s);
/* The FPN's level sum (ref: second3d_fpn.py:131-134) in one pass over its output, U3D_BF16 rows: out[o] = sum over the levels i <
 * levels (1 .. 4, in the order given) of relu(bn_i(x_i[idx_i[o]])), every partial sum rounded to bf16 - bit for bit what the chain of
 * u3d_bn_apply launches with relu, row_map and post_add leaves, without writing and re-reading the partial sums.  The per-level
 * arguments are HOST arrays of `levels` device pointers (they travel in the kernel arguments); idx[i] (int32 [n_cap], entries may be
 * NULL = the identity) maps an OUTPUT row to the row of x_i - the inverse of u3d_bn_apply's row_map.
 * u3d_bn_bwd_apply_sum: reads dout [n_cap][C] once and writes dx_i[idx_i[o]] of every level - u3d_bn_bwd_apply with relu, y NULL
 * (mask recomputed from x_i) and that level's sums (u3d_bn_bwd_stats, still one call per level).
 * U3D_ERR_UNSUPPORTED and nothing launched when dtype is not U3D_BF16, C does not fit the vector kernels (C % 8, (C / 8) | 256), the
 * backward's staged parameters exceed 64 KiB of LDS (levels * C * 24 bytes; both entries) or a column parameter is not 16-byte
 * aligned: the caller then runs the chain. */
int32_t u3d_bn_apply_sum(const void* const* x, const float* const* mean, const float* const* invstd, const float* const* gamma,
                         const float* const* beta, const int32_t* const* idx, int32_t levels, void* out, const int32_t* n_dev,
                         int32_t n_cap, int32_t c, int32_t dtype, u3d_stream s);
int32_t u3d_bn_bwd_apply_sum(const void* dout, const void* const* x, const float* const* mean, const float* const* invstd,
                             const float* const* gamma, const float* const* beta, const double* const* sums,
                             const int32_t* const* idx, void* const* dx, int32_t levels, const int32_t* n_dev, int32_t n_cap,
                             int32_t c, int32_t dtype, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * SparseConvTensor.dense() (ref: sparse_encoder_hd.py:133): rows -> channels-last dense volume
 * dense[b, z, y, x, :] (= a torch channels_last_3d tensor of logical shape [B,C,D,H,W]); caller zeroes it.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_to_dense(const void* feat, const int32_t* coors, const int32_t* n_dev, int32_t n_cap, int32_t c,
                     void* dense, int32_t dz, int32_t dy, int32_t dx, int32_t dtype, u3d_stream s);
int32_t u3d_from_dense(const void* dense, const int32_t* coors, const int32_t* n_dev, int32_t n_cap, int32_t c,
                       void* feat, int32_t dz, int32_t dy, int32_t dx, int32_t dtype, u3d_stream s);

/* row gather / permutation: out[i,:] = in[idx[i],:] (idx<0 -> zeros). elem_bytes*c must be a multiple of 4 */
int32_t u3d_gather_rows(const void* in, const int32_t* idx, int32_t n, int32_t row_bytes, void* out, u3d_stream s);
/* out[idx[i],:] = in[i,:]  (idx<0 skipped; idx must be injective) */
int32_t u3d_scatter_rows(const void* in, const int32_t* idx, int32_t n, int32_t row_bytes, void* out, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * D-FPS (ref: models/detectors/uni3detr.py:138,178-187; upstream mmcv PointsSampler / furthest_point_sample,
 * SURVEY.md App. A5).  nsets independent point sets; point k of set s is the float triple base[set_off[s]+3k..+2]
 * (the packed-triple view the upstream kernel takes of whatever buffer it is handed).  idx[0]=0; squared-L2 running
 * minimum; arg-max ties resolved as the upstream 2^k-thread block reduction does: smallest (k mod T, k),
 * T = min(1024, 2^floor(log2 n)).  out_idx int32 [nsets, m].  temp: f32 [nsets, temp_stride >= max_n] workspace, only needed
 * when max_n > 20480: such sets run either on ceil(n / 20480) <= 16 resident workgroups per set that exchange their round
 * winners through the head of temp (sets go out in launches of at most max_wg workgroups; max_wg = 0: 3/4 of the device's CUs,
 * hipDeviceAttributeMultiprocessorCount), or - beyond 16 x 20480 points, or when one set needs more than max_wg workgroups
 * (max_wg = 1: always) - on one workgroup streaming the running minima through temp.  Same indices either way.
 * err: int32 [2], device; REQUIRED for the several-workgroup form, optional otherwise.  err[0] is written by the call: 0, or 1
 * when a workgroup waited longer than poll_ticks (100 MHz ticks of the constant clock; 0 = 0.5 s) for a sibling's round winner -
 * then every workgroup of the call leaves at once, unfinished rounds hold index 0 and the samples of this call MUST NOT be
 * used (the training step ORs err[0] into its collective hold flag).  err[1] += 1 per call that timed out (the caller clears it).
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_fps(const float* base, const int64_t* set_off, const int32_t* set_n, int32_t nsets, int32_t max_n,
                int32_t m, int32_t* out_idx, float* temp, int64_t temp_stride, int32_t* err, int64_t poll_ticks, int32_t max_wg,
                u3d_stream s);
/* the same over two buffers: sets [0, split) are offsets into base, sets [split, nsets) into base2 */
int32_t u3d_fps2(const float* base, const float* base2, int32_t split, const int64_t* set_off, const int32_t* set_n,
                 int32_t nsets, int32_t max_n, int32_t m, int32_t* out_idx, float* temp, int64_t temp_stride, int32_t* err,
                 int64_t poll_ticks, int32_t max_wg, u3d_stream s);
/* The detector's glue around its two FPS passes (ref: models/detectors/uni3detr.py:178-189), one launch each side.
 *   u3d_fps_prep: vox f32 [v_rows,3] = float (z,y,x) of coors int32 [v_rows,4] (b,z,y,x); set descriptors for u3d_fps2 with
 *     split = batch: sets 0..B-1 = the packed-triple view of the [N,nfeat] point buffer from row scene_off[b] (offset
 *     scene_off[b]*nfeat, n = scene_off[b+1]-scene_off[b]); sets B..2B-1 = the voxel rows voxel_off[b]..voxel_off[b+1]
 *     (offset voxel_off[b]*3 into vox).  set_off int64 [2B], set_n int32 [2B].
 *   u3d_fps_points: idx int32 [2B,m] (u3d_fps2's output) -> out f32 [B,2m,3]: rows 0..m-1 = the sampled points' (x,y,z),
 *     rows m..2m-1 = the sampled voxel coordinates as (x,y,z), each group mapped to the unit cube by its per-scene
 *     min / max over the m samples (shift_scale_points, ref :18-46: (x - lo) / (hi - lo)). */
int32_t u3d_fps_prep(const int32_t* coors, int32_t v_rows, const int32_t* scene_off, const int32_t* voxel_off, int32_t batch,
                     int32_t nfeat, float* vox, int64_t* set_off, int32_t* set_n, u3d_stream s);
int32_t u3d_fps_points(const float* pts, int32_t nfeat, const float* vox, const int32_t* idx, const int32_t* scene_off,
                       const int32_t* voxel_off, int32_t batch, int32_t m, float* out, u3d_stream s);
/* Query assembly of Uni3DETRHead.forward (ref: dense_heads/uni3detr_head.py:436-455) in one launch: `groups` query groups of nq
 * queries; group 0 = (tgt[:nq], anchor), group g >= 1 = (tgt[nq:], inverse_sigmoid(points of group g)) with the points of
 * groups 1, 2 in fps f32 [B,2nq,3] and of group 3 (eval layout) in rnd f32 [B,nq,3].  tgt f32 [2nq,c], anchor f32 [nq,3].
 * Outputs: query_embeds f32 [B,G*nq,c+3] and its two column blocks as contiguous tensors, query [B,G*nq,c], ref [B,G*nq,3];
 * ref_sig (nullable) [B,G*nq,3] = sigmoid(ref), the transformer's init_reference.
 * _bwd: d_tgt [2nq,c], d_anchor [nq,3] = sums over scenes (and sharing groups) of the output gradients (each may be null;
 *   d_ref_sig reaches the anchor through the sigmoid, which is why `anchor` is passed). */
int32_t u3d_query_embed_fwd(const float* tgt, const float* anchor, const float* fps, const float* rnd, int32_t batch, int32_t nq,
                            int32_t groups, int32_t c, float* query_embeds, float* query, float* ref, float* ref_sig, u3d_stream s);
int32_t u3d_query_embed_bwd(const float* d_query_embeds, const float* d_query, const float* d_ref, const float* d_ref_sig,
                            const float* anchor, int32_t batch, int32_t nq, int32_t groups, int32_t c, float* d_tgt, float* d_anchor,
                            u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Matching (ref: core/bbox/assigners/hungarian_assigner_3d.py:53-151; match_costs/match_cost.py:19-30,91-97; upstream
 * FocalLossCost; scipy.optimize.linear_sum_assignment).
 *   cls f32 [L,B,Q,C] logits, box f32 [L,B,Q,code] codes, gt f32 [sumG,7] gravity-centre boxes, labels int32 [sumG],
 *   gt_off int32 [B+1] (device).  cost f32 [L*B, gmax, Q] (GT-major) = w_cls*focal + w_reg*L1(8 code dims) +
 *   w_iou*(1 - nearest-BEV IoU).  u3d_lsa solves one problem per (layer, scene, query group of nq) on one wavefront
 *   in float64 with scipy's scan order and tie rule; assigned int32 [L,B,Q]: 0 background, else 1-based GT index.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_match_cost(const float* cls, const float* box, const float* gt, const int32_t* labels,
                       const int32_t* gt_off, int32_t nlayers, int32_t batch, int32_t nq_total, int32_t ncls,
                       int32_t code_size, int32_t gmax, float w_cls, float w_reg, float w_iou, float alpha,
                       float gamma, float* cost, u3d_stream s);
int32_t u3d_lsa(const float* cost, const int32_t* gt_off, int32_t nlayers, int32_t batch, int32_t nq_total,
                int32_t nq, int32_t gmax, int32_t* assigned, u3d_stream s);

/* Trilinear sampling of a channels-last volume at query points = UniCrossAtten's F.grid_sample (mode bilinear, zeros padding,
 * align_corners=False; ref: models/utils/uni3detr_transformer.py:342-345).  value: rows [batch*dz*dy*dx, c] (f32|bf16),
 * grid f32 [batch,nq,3] (x,y,z) in [-1,1], out [batch,nq,c].  Backward: dvalue f32 [rows,c] accumulated with atomics
 * (caller zeroes; may be NULL), dgrid f32 [batch,nq,3] (may be NULL). */
int32_t u3d_trilinear_fwd(const void* value, const float* grid, int32_t batch, int32_t nq, int32_t dz, int32_t dy, int32_t dx,
                          int32_t c, void* out, int32_t dtype, u3d_stream s);
int32_t u3d_trilinear_bwd(const void* value, const float* grid, const void* dout, int32_t batch, int32_t nq, int32_t dz,
                          int32_t dy, int32_t dx, int32_t c, float* dvalue, float* dgrid, int32_t dtype, u3d_stream s);

/* diag(bbox_overlaps_3d(a,b)) for a,b f32 [n,7] (ref: models/dense_heads/uni3detr_head.py:695). */
int32_t u3d_iou3d_rotated_aligned(const float* a, const float* b, int32_t n, float* out, u3d_stream s);

/* Class-aware rotated-BEV NMS (ref: models/dense_heads/uni3detr_head.py:849-865 -> mmcv.ops.nms3d applied per class).
 * boxes f32 [n,7] sorted by descending score, labels int32 [n]; keep uint8 [n] (1 = survives).  A box is suppressed by a
 * kept earlier box of the same label with BEV rotated IoU > thr (height ignored). */
int64_t u3d_nms3d_workspace(int32_t n);
int32_t u3d_nms3d(const float* boxes, const int32_t* labels, int32_t n, float thr, uint8_t* keep, void* workspace,
                  int64_t workspace_bytes, u3d_stream s);

/* The inference tail for every scene of a batch in one call: NMSFreeCoder.decode_single's selection and Uni3DETRHead.get_bboxes'
 * post-processing for post_processing None / 'nms' (ref: core/bbox/coders/nms_free_coder.py:42-100,
 * models/dense_heads/uni3detr_head.py:827-918), bit for bit what the per-scene host loop gives (csrc/det_tail.hip).
 * prob f32 [B,Q,C] sigmoid class scores, fused f32 [B,Q,C] = prob^alpha * iou^(1-alpha) (what is reported), boxes f32 [B,Q,box_dim]
 * denormalised, gravity centre, box_dim 7 or 9; center_range f32 [6] on the device; K = min(max_num, Q*C).  Per scene:
 *   1. the K largest of prob, ordered by descending score, then ascending flat (query, class) index; label = idx % C, query = idx / C;
 *   2. kept if the three centre coordinates lie within center_range (inclusive) and, when score_threshold > 0, prob > score_threshold;
 *      stable compaction; the reported score is fused[query, class];
 *   3. z -= dz * 0.5 in two rounded f32 steps (bottom centre), except in mode U3D_DET_TAIL_DECODE;
 *   4. U3D_DET_TAIL_NONE / _DECODE: that list; U3D_DET_TAIL_NMS: greedy same-label rotated-BEV NMS in (fused score descending, compacted
 *      position ascending) order with u3d_nms3d's IoU, suppression at IoU > nms_thr; survivors by label ascending, inside a label
 *      by descending score, stable;
 *   5. score_thr (f32 [C] on the device, or NULL): keep fused > score_thr[label]; num_thr > 0: the first num_thr by descending fused
 *      score, ties by the order of step 4 (the per-scene path's argsort leaves those ties open: this is the pin).
 * Outputs: out_boxes [B,K,box_dim], out_scores [B,K], out_labels int32 [B,K] with the rows past out_count[b] zeroed, out_count int32
 * [B], out_off int32 [B+1] = exclusive scan of out_count (the det_off layout of u3d_eval_* / u3d_tta_merge).  No atomics on global
 * memory: equal inputs give equal bytes.  U3D_ERR_UNSUPPORTED for K > U3D_DET_TAIL_MAX_K, Q*C >= 2^31, C > 65536, B > 65535.  NMS
 * segments (one scene, one class) of more than U3D_DET_TAIL_LDS_CAP candidates read their BEV rows from the workspace instead of LDS. */
#define U3D_DET_TAIL_NONE 0
#define U3D_DET_TAIL_NMS 1
#define U3D_DET_TAIL_DECODE 2    /* as NONE with the boxes left gravity-centre: what NMSFreeCoder.decode returns */
#define U3D_DET_TAIL_MAX_K 8192
#define U3D_DET_TAIL_LDS_CAP 2048
int64_t u3d_det_tail_workspace(int32_t batch, int32_t nq, int32_t num_classes, int32_t max_num, int32_t box_dim);
int32_t u3d_det_tail(const float* prob, const float* fused, const float* boxes, int32_t batch, int32_t nq, int32_t num_classes,
                     int32_t box_dim, int32_t max_num, const float* center_range, float score_threshold, int32_t mode, float nms_thr,
                     const float* score_thr, int32_t num_thr, float* out_boxes, float* out_scores, int32_t* out_labels,
                     int32_t* out_count, int32_t* out_off, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* u3d_det_tail with get_bboxes' other two post-processing types: every argument of u3d_det_tail, soft_sigma / soft_prune after num_thr.
 * All five modes are accepted (NONE / NMS / DECODE as above, u3d_det_tail forwards here); steps 1-3 and 5 are those of u3d_det_tail,
 * step 4 becomes
 *   U3D_DET_TAIL_SOFT_NMS  per label the Gaussian soft-NMS of u3d_soft_nms on the bottom-centre boxes (first 7 columns, rotated 3-D
 *      IoU): select the highest current score, ties to the lowest compacted position; every other live box of the label is decayed by
 *      exp(-iou^2 / soft_sigma) and dies when its score is <= soft_prune.  Output by label ascending, inside a label in selection
 *      order; the REPORTED SCORE IS THE DECAYED ONE, and step 5 (score_thr, num_thr with ties by this order) works on it.
 *      soft_sigma <= 0 is U3D_ERR_ARG.
 *   U3D_DET_TAIL_MERGE  the KITTI box merging of u3d_box_merge: the candidates in (fused score descending, compacted position
 *      ascending) order - the stable argsort(-scores) -; a live box is kept and absorbs every later live box of its label with
 *      overlap > nms_thr (the reference's overlap with its camera-axis reading of the LiDAR columns, on the un-merged bottom-centre
 *      boxes).  A kept box takes in its first 7 columns the per-column median of {absorbed boxes in that order, itself last}: numpy's
 *      median, the mean of the two middle values for an even count, equal values ranked by that position; columns 7 and up are its
 *      own, the reported score is its fused score.  Output in that scene-wide order, NOT by label; step 5 keeps it (num_thr ties
 *      by compacted position).
 * Limits as for u3d_det_tail, K = U3D_DET_TAIL_MAX_K served in every mode, checked before any launch (U3D_ERR_UNSUPPORTED); a
 * workspace below u3d_det_tail_pp_workspace(..., mode) is U3D_ERR_WORKSPACE.  A (scene, label) segment keeps its scores, its sweep
 * flags and its member list in LDS for any size, its boxes too up to U3D_DET_TAIL_LDS_CAP candidates (read from the workspace above
 * that); the merge needs no mask matrix, so the workspace stays linear in B * K.  No atomics on global memory, no synchronisation,
 * no allocation. */
#define U3D_DET_TAIL_SOFT_NMS 3
#define U3D_DET_TAIL_MERGE 4
int64_t u3d_det_tail_pp_workspace(int32_t batch, int32_t nq, int32_t num_classes, int32_t max_num, int32_t box_dim, int32_t mode);
int32_t u3d_det_tail_pp(const float* prob, const float* fused, const float* boxes, int32_t batch, int32_t nq, int32_t num_classes,
                        int32_t box_dim, int32_t max_num, const float* center_range, float score_threshold, int32_t mode, float nms_thr,
                        const float* score_thr, int32_t num_thr, float soft_sigma, float soft_prune, float* out_boxes, float* out_scores,
                        int32_t* out_labels, int32_t* out_count, int32_t* out_off, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* The validity gate of a captured inference step, applied in place to the outputs of u3d_det_tail_pp (boxes f32 [B,max_num,box_dim],
 * scores f32 [B,max_num], labels int32 [B,max_num], count int32 [B], off int32 [B+1]; max_num is the padded row count K of those
 * tensors).  flag: one device float, non-zero when the forward behind the detections must not be trusted (a sparse level over its
 * capacity, an FPS time-out, a scene cut by u3d_batch_ingest: what u3d_capacity_flag and the ingest leave); n_live: one device int32,
 * the number of leading scenes that carry real data (the rest are padding).
 *   valid[0] = (flag[0] == 0), int32;
 *   scene b is dead when flag[0] != 0 (a NaN counts as raised) or b >= n_live[0]: its rows [0, count[b]) are zeroed, count[b] = 0;
 *   off = exclusive scan of the gated counts.
 * Rows past count[b] are zero on input and stay so: the gated bytes are a function of the inputs alone.  A count outside
 * [0, max_num] is read as clamped to it.  Two launches, no atomics on global memory, no allocation, no synchronisation.
 * U3D_ERR_ARG: a null pointer, batch or max_num <= 0, box_dim not 7 or 9; U3D_ERR_UNSUPPORTED: batch > 65535 or
 * max_num > U3D_DET_TAIL_MAX_K. */
int32_t u3d_det_gate(const float* flag, const int32_t* n_live, float* boxes, float* scores, int32_t* labels, int32_t* count, int32_t* off,
                     int32_t batch, int32_t max_num, int32_t box_dim, int32_t* valid, u3d_stream s);

/* A device-resident store for the detections of a whole dataset (csrc/det_store.hip): finished DetBatches are appended stream-ordered,
 * with no host read, and packed once into the flat layout of u3d_eval_* (the counterpart of the result list the reference's
 * extra_tools/test.py collects on the host).  The store is caller-owned memory, zeroed cursor to start with:
 *   st_boxes f32 [R, box_dim], st_scores f32 [R], st_labels int32 [R]     R = row_capacity
 *   table int32 [S, 2] = (first row, count) per scene                     S = scene_capacity
 *   cursor int32 [4] = (scenes recorded, rows used, invalid calls, refused calls)
 *   invalid int32 [M, 2] = (first scene, scenes) per invalid call         M = invalid_capacity (0: invalid may be NULL)
 * u3d_det_store_append takes the tensors of a DetBatch (boxes [batch, max_num, box_dim], scores / labels [batch, max_num] with the rows
 * past count[b] zero, count int32 [batch]; a count outside [0, max_num] is read as clamped, as in u3d_det_gate), n_live (one device
 * int32, NULL = batch; clamped to [0, batch]), valid (one device int32, NULL = 1) and scene_ids (int32 [batch] or NULL).
 *   scene_ids NULL: the leading n_live scenes become scenes cursor[0] .. cursor[0] + n_live - 1, their live rows go to rows cursor[1] ..
 *     in scene order, table and cursor advance; scenes at or past n_live are padding and are not recorded.  With valid[0] == 0 the
 *     scenes are recorded with count 0 (numbering stays aligned with the dataset), (first scene, n_live) is written to
 *     invalid[cursor[2]] if cursor[2] < M, and cursor[2] is incremented in any case (n_live == 0: nothing to record, nothing counted).
 *     The call is REFUSED AS A WHOLE when the scenes would pass S or the rows would pass R: it writes nothing and increments cursor[3].
 *   scene_ids given (the repair of scenes recorded empty): the rows are appended at cursor[1] and table[scene_ids[b]] is overwritten for
 *     b < n_live; cursor[0] does not move.  A scene id outside [0, cursor[0]), rows that would pass R, or valid[0] == 0 refuse the call
 *     as above.  An id named twice: the last one wins.  The rows an overwritten entry pointed to stay where they are, unreferenced.
 * A cursor outside the store refuses the call too.  Two launches, no atomics on global memory, no allocation, no synchronisation; it can
 * be captured in a graph, and then every replay appends.  The bytes written are a function of the inputs alone: nothing at or past the
 * used rows of the store is ever read.  Every workgroup re-derives the call's plan from count: O(batch) reads each.
 * U3D_ERR_ARG: a null pointer (other than n_live / valid / scene_ids, and invalid with M == 0), batch, max_num, R or S <= 0, M < 0,
 * box_dim not 7 or 9; U3D_ERR_UNSUPPORTED: batch > 65535, max_num > U3D_DET_TAIL_MAX_K, R * box_dim >= 2^31.  Checked before any launch. */
int32_t u3d_det_store_append(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int32_t batch,
                             int32_t max_num, int32_t box_dim, const int32_t* n_live, const int32_t* valid, const int32_t* scene_ids,
                             float* st_boxes, float* st_scores, int32_t* st_labels, int32_t* table, int32_t* cursor, int32_t* invalid,
                             int32_t row_capacity, int32_t scene_capacity, int32_t invalid_capacity, u3d_stream s);

/* The first n_scenes scenes of a store (n_scenes <= cursor[0], which the host has read) in the evaluators' layout, in scene index order:
 * out_boxes f32 [out_rows, box_dim], out_scores f32 [out_rows], out_labels int32 [out_rows], out_off int32 [n_scenes + 1] = exclusive
 * scan of the table's counts (the det_off of u3d_eval_*).  Rows a repair left unreferenced do not appear.  out_off is always the full
 * scan; a row whose place lies at or past out_rows is not written, so out_off[n_scenes] > out_rows tells a too small output.  A table
 * entry is read as clamped to a run inside [0, R).  bad int32 [2]: bad[0] = 1 when a packed score is not finite, bad[1] = 1 when a
 * packed label lies outside [0, num_classes) (num_classes <= 0: not checked), else 0.  At most two launches (one for n_scenes == 0), no
 * atomics on global memory, no allocation, no synchronisation; equal inputs give equal bytes.
 * U3D_ERR_ARG: a null pointer, n_scenes or out_rows < 0, R <= 0, box_dim not 7 or 9; U3D_ERR_UNSUPPORTED: R * box_dim or
 * out_rows * box_dim >= 2^31. */
int32_t u3d_det_store_pack(const float* st_boxes, const float* st_scores, const int32_t* st_labels, const int32_t* table, int32_t n_scenes,
                           int32_t row_capacity, int32_t box_dim, int32_t num_classes, float* out_boxes, float* out_scores,
                           int32_t* out_labels, int32_t out_rows, int32_t* out_off, int32_t* bad, u3d_stream s);

/* The stores of several ranks merged into one, in dataset order (csrc/det_store.hip; det_store.gather_stores: the counterpart of the
 * reference's collect_results behind multi_gpu_test).  The W shards come in wire form - every rank's u3d_det_store_pack output padded
 * to common sizes and stacked, as an all-gather leaves them:
 *   sh_boxes f32 [W, Nmax, box_dim], sh_scores f32 [W, Nmax], sh_labels int32 [W, Nmax]
 *   sh_off int32 [W, Smax + 1]       shard w's det_off: its local scene l holds the shard's rows sh_off[w][l] .. sh_off[w][l + 1] - 1
 *   sh_head int32 [W, 2] = (scenes, rows) of every shard, on the device
 *   scene_map int32 [n_scenes, 2] = (shard, local scene) of every scene to merge, in the order they are to appear
 * and the destination is a store as u3d_det_store_append describes it (st_boxes .. invalid, R, S, M; invalid is not touched).
 *   The n_scenes mapped scenes become scenes cursor[0] .. cursor[0] + n_scenes - 1 of the destination; their rows are written
 *   compactly, in map order, from row cursor[1] on; table gets (first row, count) per scene, cursor[0] += n_scenes, cursor[1] += the
 *   rows written.  A shard's offsets are read clamped into [0, rows of that shard] (a = clamp(sh_off[w][l]), b = clamp(sh_off[w][l + 1]):
 *   the scene is the run of max(b - a, 0) rows from a), so no row outside the shard's own is read whatever sh_off holds.  A map entry
 *   named twice is copied twice.
 *   The call is REFUSED AS A WHOLE - it writes nothing to the store and increments cursor[3] - when the scenes would pass S or the
 *   rows would pass R, when a cursor lies outside the store (cursor[0] outside [0, S], cursor[1] < 0), when a map entry names a shard
 *   outside [0, W) or a local scene outside [0, scenes of that shard), or when a shard head lies outside [0, Smax] x [0, Nmax].
 * Two launches: one workgroup validates, decides the refusal and scans the mapped counts into the workspace (u3d_det_store_merge_workspace
 * (n_scenes) bytes, no contents required), O(n_scenes + W) reads in all; then one workgroup per scene copies its run and writes its
 * table entry, and the first of them the cursor - the only writer of table / cursor, stream-ordered behind the only reader of the
 * cursor.  No atomics on global memory, no allocation, no synchronisation, no host read; the bytes written are a function of the inputs
 * alone: nothing at or past the used rows of the destination is read.  n_scenes == 0 validates the heads and the cursor and moves nothing.
 * U3D_ERR_ARG: a null pointer (other than invalid with M == 0), W, Nmax, R or S <= 0, n_scenes, Smax or M < 0, box_dim not 7 or 9;
 * U3D_ERR_UNSUPPORTED: R * box_dim or W * Nmax * box_dim >= 2^31; U3D_ERR_WORKSPACE: a workspace below
 * u3d_det_store_merge_workspace(n_scenes).  Checked before any launch, in that order. */
int64_t u3d_det_store_merge_workspace(int32_t n_scenes);
int32_t u3d_det_store_merge(const float* sh_boxes, const float* sh_scores, const int32_t* sh_labels, const int32_t* sh_off,
                            const int32_t* sh_head, int32_t n_shards, int32_t shard_rows, int32_t shard_scenes, int32_t box_dim,
                            const int32_t* scene_map, int32_t n_scenes, float* st_boxes, float* st_scores, int32_t* st_labels,
                            int32_t* table, int32_t* cursor, int32_t* invalid, int32_t row_capacity, int32_t scene_capacity,
                            int32_t invalid_capacity, void* workspace, int64_t workspace_bytes, u3d_stream s);

/* Second half of the strided-convolution input gradient (first half: P = dout @ [W_0^T | ... | W_{K-1}^T] with u3d_linear_bf16 on
 * the weight viewed as [K*Cin, Cout]): din[i][c] = sum_kappa P[nbr[kappa][i]][kappa*C + c], nbr = transposed table (mode 1 of
 * u3d_nbr_table / u3d_dense_nbr_table), f32 accumulation.  Replaces the dgrad half of spconv's indice_conv_backward / cuDNN dgrad
 * for stride > 1 (ref: models/backbones/second_3d.py:52-76 first conv of each block).
 * addend (nullable; out's shape and dtype) is added to the sum: the input gradients the other branches of a shared input already summed
 * (SECOND3D with is_cascade=False, ref: second_3d.py:89-114) - autograd's separate element-wise add over the full tensor disappears. */
int32_t u3d_tap_gather_sum(const void* p, const int32_t* nbr, int32_t ld, const int32_t* n_dev, int32_t n_cap, int32_t c,
                           int32_t kvol, int32_t dtype, const void* addend, void* out, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * LayerNorm over the last dimension of a row matrix [n, C] (C <= 1024) with optional fused ReLU; input and output dtypes are
 * independent (f32 / bf16).  Replaces nn.LayerNorm (+ nn.ReLU) of the decoder layers, the position encoder and the head branches
 * (ref: models/utils/uni3detr_transformer.py:232-236, models/dense_heads/uni3detr_head.py:95-125, mmcv BaseTransformerLayer).
 * fwd: y = relu?((x-mean)*rstd*gamma+beta); mean/rstd f32 [n] are saved for the backward.
 * bwd: dx (dtype of x) and partial f32 [2][u3d_layernorm_blocks(n)][C] = per-workgroup sums of (dgamma, dbeta) terms; the caller
 *      column-sums them (u3d_colsum / u3d_colsum_batched).  With relu the mask is recomputed from x.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_layernorm_blocks(int32_t n);
int32_t u3d_layernorm_fwd(const void* x, int32_t x_dtype, int32_t n, int32_t c, const float* gamma, const float* beta,
                          float eps, int32_t relu, void* y, int32_t y_dtype, float* mean, float* rstd, u3d_stream s);
int32_t u3d_layernorm_bwd(const void* dy, int32_t y_dtype, const void* x, int32_t x_dtype, int32_t n, int32_t c,
                          const float* gamma, const float* beta, const float* mean, const float* rstd, int32_t relu,
                          void* dx, float* partial, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Detection losses of Uni3DETRHead for all L decoder layers at once (ref: models/dense_heads/uni3detr_head.py:579-720 loss_single /
 * loss, models/losses/rdiouloss.py:93-223, core/bbox/util.py:8-80).  m = B*Q elements per layer, tensors [L, m, *] contiguous f32:
 * cls [L,m,C] logits, box [L,m,code] codes (code 8 or 10), iou_logit [L,m], tgt [L,m,code-1] assigned GT boxes (zeros for
 * background), lab int64 [L,m] (C = background), w [L,m] (1 for matched), iou_true [L,m] rotated 3-D IoU targets, cls_avg / npos [L]
 * avg factors (already clamped to >= 1), code_w [code].  out [L][4] = (loss_cls, loss_bbox, loss_iou, loss_iou_pred) per layer.
 * bwd: gout [L][4] = incoming gradients of those scalars; dcls / dbox / diou have the shapes of cls / box / iou_logit.
 * The quality (soft) target of the focal loss is NOT detached; gamma of the focal weight is 2.
 * ---------------------------------------------------------------------------------------------- */
int64_t u3d_det_loss_workspace(int32_t L, int32_t m);
int32_t u3d_det_loss_fwd(const float* cls, const float* box, const float* iou_logit, const float* tgt, const int64_t* lab,
                         const float* w, const float* iou_true, const float* cls_avg, const float* npos, const float* code_w,
                         int32_t L, int32_t m, int32_t c, int32_t code, int32_t tdim, float alpha, float w_cls, float w_box,
                         float w_iou, float eps, float* out, void* workspace, int64_t workspace_bytes, u3d_stream s);
int32_t u3d_det_loss_bwd(const float* cls, const float* box, const float* iou_logit, const float* tgt, const int64_t* lab,
                         const float* w, const float* iou_true, const float* cls_avg, const float* npos, const float* code_w,
                         const float* gout, int32_t L, int32_t m, int32_t c, int32_t code, int32_t tdim, float alpha, float w_cls,
                         float w_box, float w_iou, float eps, float* dcls, float* dbox, float* diou, u3d_stream s);
/* Target construction behind the assignment (ref: dense_heads/uni3detr_head.py:510-570), all layers and scenes in one launch:
 * asg int32 [L,B,Q] (u3d_lsa: 0 background, else 1-based GT of the scene), gt f32 [sumG,gd], labels int32 [sumG], gt_off int32 [B+1] ->
 * asg64 int64 [L,B,Q], w f32 [L,B,Q] (1 on matched queries), tgt f32 [L,B,Q,gd] (matched GT row, zeros for background),
 * lab int64 [L,B,Q] (GT label, ncls for background), num_pos f32 [L] (matched queries per layer). */
int32_t u3d_loss_targets(const int32_t* asg, const float* gt, const int32_t* labels, const int32_t* gt_off, int32_t L, int32_t B,
                         int32_t Q, int32_t gd, int32_t ncls, int64_t* asg64, float* w, float* tgt, int64_t* lab, float* num_pos,
                         u3d_stream s);
/* codes [n, code] -> boxes [n, 7] (cx, cy, cz, dx, dy, dz, yaw) (ref: core/bbox/util.py denormalize_bbox). */
int32_t u3d_denormalize_boxes(const float* codes, int32_t n, int32_t code, float* boxes, u3d_stream s);
/* Box decode of the head (ref: dense_heads/uni3detr_head.py:475-490): out = tmp with columns 0,1,4 replaced by
 * sigmoid(tmp + inverse_sigmoid(ref)[x,y,z]) * (pc_range hi - lo) + lo.  tmp [n, code] f32 or bf16 (dtype), ref [n, 3] f32 in
 * sigmoid space (inverse_sigmoid clamps at eps, 1e-5 upstream), pc_range 6 host floats, out f32 [n, code].  The backward returns
 * dtmp in tmp's dtype and, when dref != NULL, the gradient w.r.t. ref (layer 0's reference points depend on learned anchors). */
int32_t u3d_box_decode_fwd(const void* tmp, int32_t dtype, const float* ref, int32_t n, int32_t code, const float* pc_range,
                           float eps, float* out, u3d_stream s);
int32_t u3d_box_decode_bwd(const void* tmp, int32_t dtype, const float* ref, const float* dout, int32_t n, int32_t code,
                           const float* pc_range, float eps, void* dtmp, float* dref, u3d_stream s);
/* Reference-point refinement + box decode of one decoder layer in one launch (ref: models/utils/uni3detr_transformer.py:194-202,
 * dense_heads/uni3detr_head.py:463-490): tmp f32 [n,code] (regression branch), ref_in f32 [n,3] (the layer's input reference
 * logits), ref_s f32 [n,3] (the same in sigmoid space) -> out [n,code] (= u3d_box_decode_fwd(tmp, ref_s)), ref_out [n,3] =
 * ref_in + tmp[:,(0,1,4)], ref_sig [n,3] = sigmoid(ref_out).  Backward w.r.t. tmp: u3d_box_decode_bwd(tmp, ref_s, dout). */
int32_t u3d_refine_decode_fwd(const float* tmp, const float* ref_in, const float* ref_s, int32_t n, int32_t code,
                              const float* pc_range, float eps, float* out, float* ref_out, float* ref_sig, u3d_stream s);
/* Sine position embedding of the decoder's reference points (ref: models/utils/uni3detr_transformer.py:33-65,181):
 * out[n][j*nfeat + f] = (f even ? sin : cos)(sigmoid(logits[n][j]) * 2*pi / dim_t[f]); logits f32 [n, nc], dim_t f32 [nfeat] (host
 * table T^(2*(f/2)/nfeat)), out f32 or bf16 [n, nc*nfeat].  Backward: dlogits f32 [n, nc] from dout (f32 or bf16). */
int32_t u3d_sine_embed_fwd(const float* logits, const float* dim_t, int32_t n, int32_t nc, int32_t nfeat, int32_t out_dtype,
                           void* out, u3d_stream s);
int32_t u3d_sine_embed_bwd(const float* logits, const float* dim_t, const void* dout, int32_t dout_dtype, int32_t n, int32_t nc,
                           int32_t nfeat, float* dlogits, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Parameter update of the training step: global-norm gradient clipping + AdamW over FLAT f32 buffers
 * (ref: projects/configs/uni3detr/uni3detr_sunrgbd.py:234-235 — AdamW(lr, weight_decay=0.01), grad_clip max_norm=10; upstream
 * torch.optim.AdamW + torch.nn.utils.clip_grad_norm_, same arithmetic: coef = min(1, max_norm/(||g||+1e-6)), decoupled decay,
 * bias-corrected moments).  state: 16 floats of device memory, zero-initialised by the caller: [0] step count (incremented here),
 * [1] clip coefficient, [2] 1-beta1^t, [3] 1-beta2^t, [4] ||g||, [5..10] lr, beta1, beta2, eps, weight_decay, max_norm (<= 0: no
 * clipping).  The kernels read the hyper-parameters from the state vector at run time: u3d_adamw_set_hyper (a one-thread launch,
 * issued between hipGraph replays) makes a captured u3d_adamw_step_hold follow a learning-rate / momentum schedule (ref: the
 * `step` lr policy of uni3detr_sunrgbd.py:236-241 and the `cyclic` lr + momentum policies of the KITTI / nuScenes configs).
 * skip (optional): uint8 per 64-element chunk, 1 = parameter chunk received no gradient and is left untouched (torch.optim.AdamW
 * skips parameters whose .grad is None).  u3d_adamw_step = set_hyper + step_hold (hold = NULL) with host scalars.  All pointers 16-byte aligned.
 * ---------------------------------------------------------------------------------------------- */
int64_t u3d_adamw_workspace(int64_t n);
int32_t u3d_adamw_set_hyper(float* state, float lr, float beta1, float beta2, float eps, float weight_decay, float max_norm,
                            u3d_stream s);
/* The step from the state vector.  HOLD flag: hold (nullable) -> one device float; > 0 makes this step a no-op (parameters, moments and
 * the step count untouched; state[11] = 1, state[12] += 1 = held steps so far).  Static-shape training (hipGraph replay over
 * capacity-sized sparse levels) uses it so that a batch that overflowed a level - on ANY rank: the flag rides in the job's
 * positive-count all-reduce - never trains on truncated levels; the host reads state[12] now and then and re-captures. */
int32_t u3d_adamw_step_hold(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float* state,
                            const uint8_t* skip, const float* hold, void* workspace, int64_t workspace_bytes, u3d_stream s);
/* u3d_adamw_step_hold with gradient accumulation, a non-finite skip and EMA weights, all decided on the device (no host read, no
 * allocation, capturable; three launches).  One call is a MICRO-step: unless held, acc += grad; every k-th such call applies clip +
 * AdamW with the window's mean gradient gbar = acc / k (mmcv GradientCumulativeOptimizerHook's arithmetic; k = 1: u3d_adamw_step_hold
 * bit for bit) and clears acc.  A window whose gbar has a NaN / Inf norm is DROPPED instead: acc is cleared, param, moments,
 * state[0..4] and ema keep their bits (what the reference's fp16 loss scaler does with such a step).  After an applied update, if ema
 * is non-null and d > 0: ema += (1 - d) * (param_new - ema).  A held call (hold non-null, *hold > 0) is exactly u3d_adamw_step_hold's:
 * state[11] = 1, state[12] += 1, acc and the window counter untouched (the held batch's gradient is discarded, the window stays open).
 * state: the 16 floats described above, unchanged in meaning.  acc_state: 8 floats of device memory, zero-initialised by the caller:
 * [0] k = accum_steps (u3d_adamw_set_accum; < 1 reads as 1), [1] micro-steps accumulated in the open window, [2] applied updates so
 * far, [3] windows dropped as non-finite so far, [4] EMA decay d (<= 0: no EMA even if ema is given), [5] outcome of THIS call:
 * 0 accumulated, 1 applied, 2 dropped, 3 held, [6] norm of gbar at the last apply or drop, [7] reserved.
 * acc, ema (nullable): n floats, 16-byte aligned; acc zero-initialised.  skip == 1 chunks are left untouched in param, moments, acc
 * and ema; to the norm they contribute this call's grad / k (as they contribute grad to u3d_adamw_step_hold's norm).  The sum of
 * squares is taken over float squares accumulated in double: |gbar| above ~1.8e19 reads as non-finite.
 * workspace: u3d_adamw_workspace(n) bytes. */
int32_t u3d_adamw_step_accum(float* param, const float* grad, float* acc, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n,
                             float* state, float* acc_state, const uint8_t* skip, const float* hold, void* workspace,
                             int64_t workspace_bytes, u3d_stream s);
/* acc_state[0] = accum_steps (>= 1), acc_state[4] = ema_decay (< 1; <= 0: no EMA): a one-thread launch, stream-ordered */
int32_t u3d_adamw_set_accum(float* acc_state, int32_t accum_steps, float ema_decay, u3d_stream s);
/* flag[0] = number of i < n (n <= 8) with *counts[i] > caps[i]; counts: HOST array of device pointers, caps: HOST array */
int32_t u3d_capacity_flag(const int32_t* const* counts, const int32_t* caps, int32_t n, float* flag, u3d_stream s);
int32_t u3d_adamw_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1,
                       float beta2, float eps, float weight_decay, float max_norm, float* state, void* workspace,
                       int64_t workspace_bytes, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Device-resident step log (csrc/step_log.hip; upstream reads every loss on the host per iteration: mmcv's TextLoggerHook behind
 * extra_tools/train.py).  A ring of `capacity` rows of U3D_STEP_LOG_FIXED + n_terms 32-bit columns plus one int64 cursor, both in
 * device memory and zero-initialised by the caller.  The cursor counts the rows appended so far; row k lives in slot k % capacity.
 * Columns: [0] step number = the cursor before the append (int32 bits), [1] outcome (int32 bits) in the coding of acc_state[5] - 0
 * accumulated, 1 applied, 2 dropped, 3 held; without acc_state: 3 if opt_state[11] > 0, else 1 -, [2] total loss, [3] gradient norm
 * (acc_state[6], without acc_state opt_state[4]), [4] clip coefficient opt_state[1], [5] lr opt_state[5], [6] beta1 opt_state[6],
 * [7] 0 (reserved), [8 + i] *terms[i].  Floats are stored as their bits.
 * u3d_step_log_bytes: bytes of the row ring (0 for capacity <= 0 or n_terms outside [0, U3D_STEP_LOG_MAX_TERMS]).
 * u3d_step_log_append: terms is a HOST array of n_terms device pointers to one f32 each (they travel as kernel arguments: a captured
 *   launch keeps them); total one device f32; opt_state / acc_state (nullable) the vectors of u3d_adamw_step_hold / _accum, read
 *   AFTER that call on the same stream.  One launch of one workgroup: reads the cursor, writes the row, advances the cursor.  No host
 *   read, no allocation, no atomics, capturable; the only writer of rows and cursor.
 * u3d_step_log_window: statistics of the latest n = min(last, cursor, capacity) rows taken in ascending step order.  out f32
 *   [U3D_STEP_LOG_FIXED + n_terms][4] = (mean, min, max, rows used) per column, zeros for columns 0 and 1 and wherever no row is used.
 *   A held row (outcome 3) is used by no column, columns 3 and 4 use applied rows (outcome 1) only, a NaN / Inf value is skipped.  The
 *   mean is a float64 sum in that order, divided and rounded once to f32.  counts int32 [4] = (n, held rows, dropped rows, non-finite
 *   totals among the rows not held).  One workgroup per column, no atomics: two calls give the same bytes.
 * U3D_ERR_ARG: a null pointer (acc_state excepted), capacity <= 0, n_terms outside [0, U3D_STEP_LOG_MAX_TERMS], last < 0; nothing is
 * launched or written then.
 * ---------------------------------------------------------------------------------------------- */
#define U3D_STEP_LOG_FIXED 8
#define U3D_STEP_LOG_MAX_TERMS 64
int64_t u3d_step_log_bytes(int64_t capacity, int32_t n_terms);
int32_t u3d_step_log_append(const float* const* terms, int32_t n_terms, const float* total, const float* opt_state,
                            const float* acc_state, void* rows, int64_t* cursor, int64_t capacity, u3d_stream s);
int32_t u3d_step_log_window(const void* rows, const int64_t* cursor, int64_t capacity, int32_t n_terms, int64_t last, float* out,
                            int32_t* counts, u3d_stream s);

/* bf16 shadows of the flat f32 parameter buffer, refreshed once per training step (bf16 mode; upstream has no counterpart: its
 * fp32 run reads the parameters directly).  u3d_cast_bf16: dst[i] = bf16(src[i]) (round to nearest even), 16-byte aligned pointers.
 * u3d_permute_bf16_batched: for every descriptor, dst[dst_off + (k*rows + r)*cols + c] = src[src_off + k*stride_k + r*stride_r +
 * c*stride_c] for k < n/(rows*cols): the conv-weight layouts the implicit-GEMM kernels stage row-linearly, i.e. [K,Cout,Cin] from
 * spconv's [K,Cin,Cout] and both [K,Cin,Cout] / [K,Cout,Cin] from nn.Conv3d's [Cout,Cin,K].  blocks_dev: int32 pairs (descriptor
 * index, first element) - one per u3d_permute_block_elems() output elements; dst_off multiples of 8; descriptors in device memory. */
typedef struct u3d_permute_desc {
  int64_t src_off, dst_off;
  int32_t n, rows, cols, reserved;
  int64_t stride_k, stride_r, stride_c;
} u3d_permute_desc;
int32_t u3d_cast_bf16(const float* src, void* dst, int64_t n, u3d_stream s);
int32_t u3d_permute_block_elems(void);
int32_t u3d_permute_bf16_batched(const void* src, void* dst, const u3d_permute_desc* descs_dev, const int32_t* blocks_dev,
                                 int32_t nblocks, u3d_stream s);
/* The same re-layout through a 32 x 32 x K LDS tile for descriptors whose source is contiguous along k (stride_k == 1, one of
 * stride_r / stride_c == K = n / (rows * cols) <= max_k <= 32, rows % 32 == cols % 32 == 0, even src_off): coalesced reads of
 * nn.Conv3d's [Cout][Cin][K] weights.  tiles_dev: int32 [ntiles][4] = (descriptor index, first row, first column, 0). */
int32_t u3d_permute_bf16_tiled(const void* src, void* dst, const u3d_permute_desc* descs_dev, const int32_t* tiles_dev,
                               int32_t ntiles, int32_t max_k, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Test-time post-processing.
 * u3d_soft_nms: class-wise Gaussian soft-NMS with the rotated 3-D IoU (ref: models/dense_heads/uni3detr_head.py:796-823, per-class loop
 *   :849-880).  boxes f32 [n,7] bottom-centre LiDAR boxes, scores f32 [n], labels int32 [n].  One workgroup per class; outputs
 *   out_idx int32 / out_score f32 [num_classes][n] = indices into the input and decayed scores in selection order, out_cnt [num_classes].
 * u3d_box_merge: the KITTI configs' `box_merging` (ref: core/bbox/bbox_merging.py:112-158 as called from uni3detr_head.py:881-891).
 *   boxes f32 [n,7] / labels sorted by DESCENDING score (the caller sorts); keep[i] = survives the greedy sweep, merged [n,7] = for
 *   kept boxes the per-coordinate median over itself and the same-class boxes it absorbed (overlap > thr), else a copy.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_soft_nms(const float* boxes, const float* scores, const int32_t* labels, int32_t n, int32_t num_classes, float sigma,
                     float prune, int32_t* out_idx, float* out_score, int32_t* out_cnt, u3d_stream s);
int64_t u3d_box_merge_workspace(int32_t n);
int32_t u3d_box_merge(const float* boxes, const int32_t* labels, int32_t n, float thr, float* merged, uint8_t* keep, void* workspace,
                      int64_t workspace_bytes, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Indoor 3-D detection evaluation: per-class AP ('area' mode) and recall at 3-D IoU thresholds (ref:
 * projects/mmdet3d_plugin/core/indoor_eval.py eval_det_cls :58-140 and average_precision :7-55, as called by indoor_eval_ov :168-303;
 * the reference loops over every detection in Python).  Detections and GT are concatenated over scenes: det_off / gt_off int32 [n_scene+1]
 * (CSR), boxes f32 [.,7] bottom-centre (x, y, z, dx, dy, dz, yaw), labels int32 in [0, num_classes), scores finite f32.
 * u3d_eval_iou_argmax: per detection, over the GT of its scene and class (rotated 3-D IoU of mmdet3d's DepthInstance3DBoxes.overlaps):
 *   iou_max f32 [n_det] (-inf without such GT) and jmax int32 [n_det] (global GT index of the FIRST maximal IoU, -1 without), and
 *   sort_key int64 [n_det] = (label << 32) | descending-orderable score bits.  The caller sorts the keys STABLY (perm int64 [n_det]):
 *   ties keep (scene, position in the scene).  n_det == 0 (n_scene == 0 included) is a no-op.
 * u3d_eval_segments: seg int32 [2*num_classes] = [lo, hi) of each class in the sorted keys; npos int32 [num_classes] = GT per class.
 * u3d_eval_first_hit: first int32 [n_thr][n_gt] = lowest rank r (position in perm) with iou_max > thr[t] and jmax == GT (0x7f7f7f7f if
 *   none); thr f32 [n_thr] on the device.  u3d_eval_tp: tp uint8 [n_thr][n_det] in rank order = the reference's greedy TP flags.
 * u3d_eval_ap: ap f32 [n_thr][num_classes] (float64 sum rounded to float32), rec f64 [n_thr][num_classes] (final recall); NaN for a
 *   class that is predicted but has no GT; prec_ws f64 [n_thr][n_gt] workspace.
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_eval_iou_argmax(const float* det_boxes, const float* det_scores, const int32_t* det_labels, const int32_t* det_off,
                            const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_off, int32_t n_scene, int32_t n_det,
                            float* iou_max, int32_t* jmax, int64_t* sort_key, u3d_stream s);
int32_t u3d_eval_segments(const int64_t* sorted_key, int32_t n_det, const int32_t* gt_labels, int32_t n_gt, int32_t num_classes,
                          int32_t* seg, int32_t* npos, u3d_stream s);
int32_t u3d_eval_first_hit(const int64_t* perm, int32_t n_det, const float* iou_max, const int32_t* jmax, const float* thr, int32_t n_thr,
                           int32_t n_gt, int32_t* first, u3d_stream s);
int32_t u3d_eval_tp(const int64_t* perm, int32_t n_det, const float* iou_max, const int32_t* jmax, const float* thr, int32_t n_thr,
                    int32_t n_gt, const int32_t* first, uint8_t* tp, u3d_stream s);
int32_t u3d_eval_ap(const uint8_t* tp, int32_t n_det, const int32_t* seg, const int32_t* npos, int32_t num_classes, int32_t n_thr,
                    int32_t n_gt, double* prec_ws, float* ap, double* rec, u3d_stream s);

/* u3d_compact_rows: out[pos[d]] = rec[d] where valid[d], for n rows of row_bytes bytes each (a positive multiple of 4, else
 * U3D_ERR_ARG; rows move as 32-bit words); pos int32 [n] = exclusive scan of valid int32 [n].  One launch, none for n == 0. */
int32_t u3d_compact_rows(const void* rec, const int32_t* valid, const int32_t* pos, int32_t n, int32_t row_bytes, void* out, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * KITTI 3-D detection evaluation (mmdet3d's kitti_eval: clean_data, compute_statistics, get_thresholds, eval_class; semantics in
 * uni3detr_amd/kitti_eval.py).  Records are f32 [., 16]: camera box (x, y, z bottom centre, l, h, w, ry), 2-D box (x1, y1, x2, y2),
 * alpha, score (detections) / ignore bits of the three difficulties (GT), class code (0 Car, 1 Pedestrian, 2 Cyclist, 3 Van,
 * 4 Person_sitting, 5 DontCare, 6 other), 2 unused.  Scenes are CSR: dt_off / gt_off int32 [n_scene+1]; ov_off int64 [n_scene+1] =
 * exclusive scan of nd * ng, ov f32 [3][n_pairs] = bbox / bev / 3d overlap matrices [dt][gt] per scene.
 * u3d_kitti_convert: LiDAR bottom-centre boxes [n,7] + scores + labels -> rec [n,16] and valid int32 [n] (inside the image and strictly
 *   inside lim = pcd_limit_range); calib f32 [n_scene][32] = R0_rect @ Tr_velo_to_cam then P2 (row-major 4x4), img f32 [n_scene][2] = (H, W).
 *   The valid rows are then kept with u3d_compact_rows.
 * u3d_kitti_flags: for the K <= 3 class codes cls, flag index f = class slot * 3 + difficulty: gt_flag / dt_flag int8 [3K][n] in
 *   {-1, 0, 1}, nvalid int32 [3K] = GT with flag 0, dc_iof f32 [n_dt] = max DontCare intersection over the detection's area.
 * Groups g (n_group): flag index gfid, metric gmet (0 bbox, 1 bev, 2 3d), min overlap gmin.
 * u3d_kitti_pass1: TP scores of compute_statistics(compute_fp = False) at tp_sc f32 [n_group][n_gt] (scene s's TPs from gt_off[s] on,
 *   -inf after them).  U3D_ERR_UNSUPPORTED above 4096 detections in a scene (max_dt).
 * u3d_kitti_thresholds: get_thresholds over rows of tp_sc sorted descending -> thr f32 [n_group][41], nthr int32 [n_group].
 * u3d_kitti_pass2: per (group, scene, threshold) tp / fp / fn int32 and similarity f64 [n_group][n_scene][41] of
 *   compute_statistics(compute_fp = True) (similarity only for bbox groups when aos, -1 = not accumulated); lds_bytes = max over the
 *   scenes of u3d_kitti_pass2_lds(nd, ng), at most 160 KiB (else U3D_ERR_UNSUPPORTED).
 * u3d_kitti_reduce: tot int32 [n_group][3][41], sim_tot f64 [n_group][41], ap f64 [n_group][4] = (AP11, AP40, AOS AP11, AOS AP40).
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_kitti_convert(const float* boxes, const float* scores, const int32_t* labels, const int32_t* off, int32_t n_scene, int32_t n,
                          const float* calib, const float* img, const int32_t* label_code, int32_t n_label, const float* lim, float* rec,
                          int32_t* valid, u3d_stream s);
int32_t u3d_kitti_overlaps(const float* dt, const int32_t* dt_off, const float* gt, const int32_t* gt_off, const int64_t* ov_off,
                           int32_t n_scene, int64_t n_pairs, float* ov, u3d_stream s);
int32_t u3d_kitti_flags(const float* dt, const int32_t* dt_off, int32_t n_scene, int32_t n_dt, const float* gt, const int32_t* gt_off,
                        int32_t n_gt, const int32_t* cls, int32_t K, int8_t* gt_flag, int32_t* nvalid, int8_t* dt_flag, float* dc_iof,
                        u3d_stream s);
int32_t u3d_kitti_pass1(const float* dt, const int32_t* dt_off, int32_t n_dt, const int32_t* gt_off, int32_t n_gt, int32_t n_scene,
                        const int64_t* ov_off, int64_t n_pairs, const float* ov, const int8_t* gt_flag, const int8_t* dt_flag,
                        const int32_t* gfid, const int32_t* gmet, const float* gmin, int32_t n_group, int32_t max_dt, float* tp_sc,
                        u3d_stream s);
int32_t u3d_kitti_thresholds(const float* sorted, int32_t n_gt, int32_t n_group, const int32_t* gfid, const int32_t* nvalid, float* thr,
                             int32_t* nthr, u3d_stream s);
int64_t u3d_kitti_pass2_lds(int32_t nd, int32_t ng);
int32_t u3d_kitti_pass2(const float* dt, const int32_t* dt_off, int32_t n_dt, const float* gt, const int32_t* gt_off, int32_t n_gt,
                        int32_t n_scene, const int64_t* ov_off, int64_t n_pairs, const float* ov, const int8_t* gt_flag, const int8_t* dt_flag,
                        const float* dc_iof, const int32_t* gfid, const int32_t* gmet, const float* gmin, const float* thr, const int32_t* nthr,
                        int32_t n_group, int32_t aos, int64_t lds_bytes, int32_t* st_tp, int32_t* st_fp, int32_t* st_fn, double* st_sim,
                        u3d_stream s);
int32_t u3d_kitti_reduce(const int32_t* st_tp, const int32_t* st_fp, const int32_t* st_fn, const double* st_sim, int32_t n_scene,
                         const int32_t* nthr, int32_t n_group, int32_t* tot, double* sim_tot, double* ap, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * nuScenes detection evaluation (the nuscenes-devkit's detection_cvpr_2019: filter_eval_boxes, accumulate, calc_ap, calc_tp; semantics
 * in uni3detr_amd/nuscenes_eval.py).  Records are f64 [., 12]: global centre (gravity), size (w, l, h), global yaw, global velocity
 * (x, y), score (predictions) / num_lidar_pts + num_radar_pts (GT), class (0..n_cls-1, -1 other, -2 bicycle rack), attribute code
 * (-1 = ''; a rack row holds its LiDAR-frame yaw there).  Samples are CSR: off int32 [n_sample+1]; calib f64 [n_sample][24] =
 * lidar2ego rotation (3x3 row-major), translation, ego2global rotation, translation.  Thresholds: ths f64 [4], tp_th = the index of
 * the TP-error threshold.
 * u3d_nusc_convert: LiDAR rows f64 [n][9] (x, y, z, l, w, h, yaw, vx, vy; z is the bottom for predictions, the gravity centre for GT),
 *   cls int32 [n], attr int32 [n] (GT), aux f64 [n] (score / points) -> rec [n][12], valid int32 [n] (predictions: a label in range
 *   and ego-frame xy radius <= cls_range; GT: an evaluated class or a rack).  attr_moving / attr_still int32 [n_cls]: the prediction
 *   attribute codes by |global v_xy| > 0.2.
 * u3d_nusc_filter: valid &= ego_dist < cls_range, GT points != 0, not (bike[class] and centre inside a rack row of gt / gt_off).
 *   The valid rows are then kept with u3d_compact_rows.
 * u3d_nusc_rank_keys: key int64 [n] / idx int32 [n]: key[n-1-i] = descending-orderable score of row i, idx[n-1-i] = i.
 * u3d_nusc_match: one wave per segment (class * n_sample + sample): rank int32 [n] = prediction rows in rank order, mperm int32 [n] =
 *   rank positions grouped by segment, mseg [n_seg+1]; gord = GT rows grouped by segment, gseg [n_seg+1]; max_gt = the largest GT
 *   segment (U3D_ERR_UNSUPPORTED above 2048; dynamic LDS 16 * max_gt bytes: the segment's GT xy as f64) -> tp int8 [4][n], match int32 [n] (GT row at
 *   tp_th, -1 = none), by rank position.
 * u3d_nusc_accumulate: one workgroup per (class, threshold).  cseg [n_cls+1] = class segments of the rank order, npos [n_cls],
 *   gcoff [n_cls] = exclusive scan of npos, rec_interp f64 [101], period f64 [n_cls]; ws of u3d_nusc_accumulate_workspace(n, n_gt)
 *   bytes -> prec / conf f64 [n_cls][4][101], err f64 [n_cls][5][101] (trans, scale, orient, vel, attr), ap f64 [n_cls][4],
 *   tp_err f64 [n_cls][5] (calc_tp), mri int32 [n_cls][4] (max_recall_ind).
 * ---------------------------------------------------------------------------------------------- */
int32_t u3d_nusc_convert(const double* rows, const int32_t* cls, const int32_t* attr, const double* aux, const int32_t* off, int32_t n_sample,
                         int32_t n, const double* calib, int32_t is_pred, const double* cls_range, const int32_t* attr_moving,
                         const int32_t* attr_still, int32_t n_cls, double* rec, int32_t* valid, u3d_stream s);
int32_t u3d_nusc_filter(const double* rec, const int32_t* off, int32_t n_sample, int32_t n, int32_t is_pred, const double* calib,
                        const double* gt, const int32_t* gt_off, const double* cls_range, const int32_t* bike, int32_t n_cls, int32_t* valid,
                        u3d_stream s);
int32_t u3d_nusc_rank_keys(const double* rec, int32_t n, int64_t* key, int32_t* idx, u3d_stream s);
int32_t u3d_nusc_match(const double* pred, const int32_t* rank, const int32_t* mperm, const int32_t* mseg, int32_t n_seg, int32_t n,
                       const double* gt, const int32_t* gord, const int32_t* gseg, int32_t max_gt, const double* ths, int32_t tp_th, int8_t* tp,
                       int32_t* match, u3d_stream s);
int64_t u3d_nusc_accumulate_workspace(int32_t n, int32_t n_gt);
int32_t u3d_nusc_accumulate(const double* pred, const double* gt, const int32_t* rank, const int32_t* cseg, const int32_t* npos,
                            const int32_t* gcoff, int32_t n_cls, int32_t n, int32_t n_gt, const int8_t* tp, const int32_t* match,
                            const double* rec_interp, const double* period, int32_t tp_th, void* ws, int64_t ws_bytes, double* prec,
                            double* conf, double* err, double* ap, double* tp_err, int32_t* mri, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * Fused decoder layer (bf16 MFMA, f32 accumulation / residual stream / LayerNorm statistics / softmax statistics).
 * One call = one Uni3DETRTransformerDecoder layer over ALL query groups of all scenes, plus everything the decoder loop and the head
 * hang on that layer's state (ref: models/utils/uni3detr_transformer.py:145-212 decoder loop, :33-65 sine embedding, :271-360
 * UniCrossAtten; mmcv BaseTransformerLayer / MultiheadAttention / FFN as configured in the "transformer" section of the shipped configs;
 * models/dense_heads/uni3detr_head.py:367-387 cls / reg / iou branches):
 *
 *   pos   = ref_point_head(sine(sigmoid(ref))) [* query_scale(x) for layers > 0]
 *   x1    = LN1(x + dropout(out_proj(MHA(q = k = x + pos, v = x))))            attention inside each group of nq queries
 *   x2    = LN2(x1 + dropout(output_proj(trilinear(value, ref) * sigmoid(attention_weights(x1 + pos)))) + position_encoder(ref))
 *   x3    = LN3(x2 + dropout(W2 dropout(relu(W1 x2))))
 *   reg   = reg_branch(x3), cls = cls_branch(x3), iou = iou_branch(x3)
 *
 * Rows are [B, G*nq] (scene-major), M = B*G*nq; embed dim 256, 8 heads, FFN 512, num_points 1 (every shipped config).
 * Launches: forward 3 (row-chain kernel | attention | row-chain kernel), backward 4; the row-chain kernels keep a 32-row block of
 * the layer state in LDS through the whole chain of GEMMs / LayerNorms and stream the bf16 weights from L2 straight into MFMA
 * fragments.  Weight / bias gradients are NOT computed here: the backward leaves every linear's dY (bf16) and every LayerNorm's
 * per-workgroup (dgamma, dbeta) partial sums in the gradient workspace; the caller batches dW = dY^T X over layers
 * (u3d_wgrad_batched_bf16 / u3d_skinny_wgrad_bf16 / u3d_colsum_batched).  Slot offsets: u3d_decoder_layer_slots().
 * Dropout: counter-based (hash of seed, layer, site, element index); the backward regenerates the masks from the same seed.
 * ---------------------------------------------------------------------------------------------- */
enum {  /* wide linears: w = [N(pad)][K] (nn.Linear's matrix) and wt = [K][N(pad)] (dgrad), both in u3d_wpack's fragment order; b f32 [N] */
  U3D_DL_RPH0, U3D_DL_RPH1, U3D_DL_RPH2,      /* ref_point_head 384->256->256->256 */
  U3D_DL_QS0, U3D_DL_QS1, U3D_DL_QS2,         /* query_scale 256->256->256->256 (layers > 0) */
  U3D_DL_INQK, U3D_DL_INV,                    /* in_proj rows [0,512) and [512,768) */
  U3D_DL_OUTP,                                /* attn.out_proj */
  U3D_DL_OPROJ,                               /* UniCrossAtten.output_proj */
  U3D_DL_PE1,                                 /* position_encoder[3] */
  U3D_DL_FFN0, U3D_DL_FFN1,                   /* 256->512, 512->256 */
  U3D_DL_REG0, U3D_DL_REG1, U3D_DL_REG2,      /* REG2 / CLS2 / IOU2: N <= 32, w padded to 64 rows, wt = ROW-MAJOR [K][32] (t_plain) */
  U3D_DL_CLS0, U3D_DL_CLS1, U3D_DL_CLS2,
  U3D_DL_IOU0, U3D_DL_IOU1, U3D_DL_IOU2,
  U3D_DL_NLIN
};
enum { U3D_DLN_1, U3D_DLN_2, U3D_DLN_3, U3D_DLN_PE0, U3D_DLN_PE1, U3D_DLN_C1, U3D_DLN_C2, U3D_DL_NLN };
typedef struct u3d_declayer_params {
  const void* w[U3D_DL_NLIN];
  const void* wt[U3D_DL_NLIN];
  const float* b[U3D_DL_NLIN];
  const float* ln_g[U3D_DL_NLN];
  const float* ln_b[U3D_DL_NLN];
  const float* attw_w; const float* attw_b;   /* attention_weights: f32 [256], [1] */
  const float* pe0_w;  const float* pe0_b;    /* position_encoder[0]: f32 [256,3], [256] */
  const float* dim_t;                         /* f32 [128]: T^(2*(f/2)/128) */
} u3d_declayer_params;
typedef struct u3d_declayer_dims {
  int32_t m;            /* rows = batch * queries_per_scene */
  int32_t nq;           /* queries per attention group */
  int32_t qps;          /* queries per scene (groups * nq) */
  int32_t batch, dz, dy, dx;   /* value volume: rows [(b*dz+z)*dy+y)*dx+x][256] bf16 */
  int32_t ncls, code;   /* widths of the cls / reg outputs (<= 32) */
  int32_t has_qs;       /* 0: first layer (pos = ref_point_head output) */
  int32_t need_dref;    /* backward: also produce the gradient w.r.t. the reference-point logits */
  int32_t layer;        /* dropout stream id */
  float p_attn, p_drop; /* dropout probabilities: attention weights | the four residual / FFN sites (0 = off) */
  float ln_eps;
  int32_t dtype;        /* U3D_BF16: bf16 activations / weights / slots, v_mfma_f32_16x16x32_bf16 (throughput mode);
                           U3D_F32: f32 everywhere, exact v_mfma_f32_16x16x4_f32 (parity mode) - the SAME kernels, instantiated on the
                           element type; every `void*` operand / slot below then holds f32 and xc may alias x */
  int32_t reserved;     /* 0 */
} u3d_declayer_dims;
/* forward-save slots (row matrices [m, cols]); u3d_decoder_layer_slots fills byte offsets (U3D_DS_COUNT + 1 entries, last = total) */
enum {
  U3D_DS_SINE, U3D_DS_RPH1, U3D_DS_RPH2, U3D_DS_RAW, U3D_DS_QS1, U3D_DS_QS2, U3D_DS_QS, U3D_DS_POS, U3D_DS_QKIN,
  U3D_DS_QK, U3D_DS_V, U3D_DS_LSE, U3D_DS_O, U3D_DS_U1, U3D_DS_MR, U3D_DS_QP, U3D_DS_SAMP, U3D_DS_GATED, U3D_DS_PEH0,
  U3D_DS_UPE1, U3D_DS_U2, U3D_DS_X2C, U3D_DS_FFH, U3D_DS_U3, U3D_DS_R1, U3D_DS_R2, U3D_DS_I1, U3D_DS_I2, U3D_DS_UC1,
  U3D_DS_C1, U3D_DS_UC2, U3D_DS_C2,
  U3D_DS_AMASK,   /* uint32 [m*8][10]: attention-dropout keep bits, row (group*8 + head)*nq + query, bit b of word w = key 32w + b; written by the
                     fused in-projection + attention launch (bf16, nq <= 320, p_attn > 0), read by the layer's backward */
  U3D_DS_COUNT
};
/* backward-workspace slots: dY of every linear (bf16), LayerNorm partials, intermediate f32 gradients */
enum {
  U3D_DG_CLSO, U3D_DG_C2U, U3D_DG_C1U, U3D_DG_IOUO, U3D_DG_I2, U3D_DG_I1, U3D_DG_REGO, U3D_DG_R2, U3D_DG_R1, U3D_DG_F,
  U3D_DG_FFH, U3D_DG_OUT, U3D_DG_UPE1, U3D_DG_P0, U3D_DG_WL, U3D_DG_O2, U3D_DG_DO, U3D_DG_DQK, U3D_DG_DV, U3D_DG_QS,
  U3D_DG_QS2, U3D_DG_QS1, U3D_DG_RAW, U3D_DG_RPH2, U3D_DG_RPH1, U3D_DG_LNP, U3D_DG_DU1, U3D_DG_DPOSA, U3D_DG_SINE,
  U3D_DG_COUNT
};
int32_t u3d_decoder_layer_slots(int32_t m, int32_t ncls, int32_t code, int32_t dtype, int64_t* save_off, int64_t* grad_off);
/* workgroups of the row-chain kernels = rows of every U3D_DG_LNP partial matrix; rows per workgroup: 32 (U3D_BF16) / 16 (U3D_F32) */
int32_t u3d_decoder_layer_blocks(int32_t m, int32_t dtype);
/* ROW PADDING: every row matrix this layer WRITES (x_out, xc_out, reg_out, cls_out, iou_out, dx, dref and all slots) must hold
 * u3d_decoder_layer_blocks(m, dtype) * (32 | 16) rows; rows >= m receive values nobody reads.  Matrices it only READS (x, xc, ref, dx_out, dreg,
 * dcls, diou) have m rows.  (The row kernels contain no branch on the row index: see csrc/decoder_common.h.) */
/* x f32 [m,256] layer input, xc its bf16 copy, ref f32 [m,3] logits, value bf16 rows, rng: device uint64 seed.
 * Outputs: x_out f32 / xc_out bf16 [m,256], reg_out f32 [m,code], cls_out f32 [m,ncls], iou_out f32 [m]; save: the slot buffer.
 * row_waves (both calls): the wave count of the row-chain launches = 8 (bf16 only: two waves per SIMD, the default of bf16), 4 (one
 * wave per SIMD: the f32 kernels, and the bf16 comparison partner), 0 = the element type's default.  Results are bit-identical for
 * either count; forward and backward of one layer may use different ones. */
int32_t u3d_decoder_layer_fwd(const u3d_declayer_params* p, const u3d_declayer_dims* d, const float* x, const void* xc,
                              const float* ref, const void* value, const uint64_t* rng, float* x_out, void* xc_out,
                              float* reg_out, float* cls_out, float* iou_out, void* save, int64_t save_bytes, int32_t row_waves,
                              u3d_stream s);
/* Gradients in: dx_out f32 [m,256] (NULL = zero), dreg f32 [m,code], dcls f32 [m,ncls], diou f32 [m].
 * Out: dx f32 [m,256] (w.r.t. the layer input x), vrec: the value-gradient records (u3d_value_records_bytes(m) bytes: d(sample) f32
 * [m][256], trilinear corner cells int32 [m][8] (-1 = outside the volume), corner weights f32 [m][8]) that u3d_value_scatter adds into
 * the volume gradient, dref f32 [m,3] (only when need_dref), and the gradient workspace `grad` (dY slots for the weight-gradient pass). */
int32_t u3d_decoder_layer_bwd(const u3d_declayer_params* p, const u3d_declayer_dims* d, const float* x, const void* xc,
                              const float* ref, const void* value, const uint64_t* rng, const void* xc_out, const void* save,
                              const float* dx_out, const float* dreg, const float* dcls, const float* diou, float* dx,
                              void* vrec, float* dref, void* grad, int64_t grad_bytes, int32_t row_waves, u3d_stream s);
int64_t u3d_value_records_bytes(int32_t m);
/* Adds the records of one u3d_decoder_layer_bwd call into dvalue [n_cells][256] (f32, or bf16 when dvalue_bf16): per cell the sum over
 * its (row, corner) entries in ascending entry order, in f32, added once - bitwise reproducible.  work: u3d_value_scatter_workspace
 * bytes of scratch (no contents required; initialised by the call, on stream s). */
int64_t u3d_value_scatter_workspace(int32_t n_cells);
int32_t u3d_value_scatter(const void* records, int32_t m, int32_t n_cells, void* dvalue, int32_t dvalue_bf16, void* work,
                          int64_t work_bytes, u3d_stream s);
/* The records of `layers` (1 .. 4) u3d_decoder_layer_bwd calls into ONE bf16 dvalue [n_cells][256] in three launches: records and m are
 * HOST arrays (device pointers / row counts per layer), order (host, a permutation of 0 .. layers-1) names the layers in the order
 * their per-cell sums are added.  A touched cell receives bf16(+0.0f + sum_order[0] + sum_order[1] + ...), each sum formed as
 * u3d_value_scatter forms it and only the layers that touch the cell taking part - bit for bit what one u3d_value_scatter call per
 * layer, in that order, into a zeroed f32 volume followed by a cast to bf16 leaves.  Cells no layer touches are not written: the
 * caller zero-fills dvalue.  work: u3d_value_scatter_layers_workspace bytes of scratch, initialised by the call. */
int64_t u3d_value_scatter_layers_workspace(int32_t layers, int32_t n_cells);
int32_t u3d_value_scatter_layers(const void* const* records, const int32_t* m, const int32_t* order, int32_t layers, int32_t n_cells,
                                 void* dvalue, void* work, int64_t work_bytes, u3d_stream s);
/* Self-attention over groups on its own (the middle launch of the layer): q,k rows of qk [m,512] (q | k), v [m,256], 8 heads x 32;
 * o bf16 [m,256], lse f32 [m,8].  Backward: dqk [m,512], dv [m,256] bf16.  dtype U3D_BF16 | U3D_F32 (the same kernels on either
 * element type; U3D_F32: all matrices then f32, exact-f32 MFMA). */
int32_t u3d_mha_fwd(const void* qk, const void* v, int32_t m, int32_t nq, float p_attn, int32_t layer, const uint64_t* rng, void* o,
                    float* lse, int32_t dtype, u3d_stream s);
int32_t u3d_mha_bwd(const void* qk, const void* v, const void* o, const void* d_o, const float* lse, int32_t m, int32_t nq,
                    float p_attn, int32_t layer, const uint64_t* rng, void* dqk, void* dv, int32_t dtype, u3d_stream s);
/* Refresh of the weight copies the fused layer reads: for each descriptor dst = bf16(src [n][k]) (rows n >= N zero up to n_pad) and
 * dst_t = its transpose [k][n_pad_t], both stored in MFMA FRAGMENT ORDER: block (16-row tile, 32-element k-step) = 64 x 16 bytes in
 * lane order (lane = kq * 16 + row, 8 consecutive k each), blocks of a tile consecutive - one wave load of a weight fragment is
 * 1 KiB contiguous.  descs in device memory; one launch for all linears of all layers.  dtype U3D_F32: the same copies in f32
 * (zero-padded rows / transposes of the f32 masters) for the parity-mode instantiation. */
typedef struct u3d_wpack_desc {
  const float* src; void* dst; void* dst_t;
  int32_t n, k, n_pad, n_pad_t;   /* n_pad % 16 == 0, k % 32 == 0 (bf16) / % 16 (f32); packed transposes: k % 16 == 0, n_pad_t % 32 == 0 */
  int32_t t_plain;                /* 1: dst_t stays row-major [k][n_pad_t] (the <= 32-column final layers); 0: fragment order */
  int32_t reserved;
} u3d_wpack_desc;
int32_t u3d_wpack(const u3d_wpack_desc* descs_dev, int32_t count, int32_t max_elems, int32_t dtype, u3d_stream s);
/* keep-mask of the layer's dropout sites as bytes (testing aid): site 0..3 = out_proj, output_proj, FFN hidden, FFN out over
 * [m, 256 | 512], linear element index (cols = 0); site 4 = attention weights over [m*8, nq] (row = (group*8 + head)*nq + query):
 * pass cols = nq (rows are padded to an even length in the generator's index space).  p is honoured to 2^-16. */
int32_t u3d_dropout_mask(const uint64_t* rng, int32_t layer, int32_t site, int64_t n, float p, int32_t cols, uint8_t* keep, u3d_stream s);

/* ------------------------------------------------------------------------------------------------
 * On-device training data path.  Replaces, for a packed batch that already sits in HBM, the DataLoader-worker
 * transforms of the shipped train pipelines (ref: projects/configs/uni3detr/uni3detr_sunrgbd.py:150-174: RandomFlip3D ->
 * GlobalRotScaleTrans -> PointsRangeFilter -> PointSample; the plugin's own UnifiedRandomFlip3D / UnifiedRotScaleTrans,
 * projects/mmdet3d_plugin/datasets/pipelines/transform_3d.py:325-589, apply the same geometry).  The random DRAWS stay with the
 * caller (host RNG, as in the reference): per-scene parameters arrive as f32 [batch][U3D_AUG_NPARAM] =
 * (flip_horizontal, flip_vertical, sin(angle), cos(angle), angle, scale, tx, ty, tz): flip -> rotate -> scale -> translate.  coord: 0 = Depth boxes/points (SUN RGB-D, ScanNet),
 * 1 = LiDAR (KITTI, nuScenes) - it selects which axis a horizontal / vertical flip mirrors.
 * ------------------------------------------------------------------------------------------------ */
#define U3D_AUG_NPARAM 9
/* in place: points [n_total, feat] f32 (x, y, z, ...), scene b = rows scene_off[b] .. scene_off[b+1]); height_dim >= 3 scales that
 * attribute with the scene (shift_height=True), -1 = none */
int32_t u3d_points_augment(float* points, const int32_t* scene_off, int32_t batch, int32_t n_total, int32_t feat, const float* params,
                           int32_t coord, int32_t height_dim, u3d_stream s);
/* in place: boxes [n, box_dim] f32 (x, y, z, dx, dy, dz, yaw [, vx, vy]), box_dim 7 or 9, scene b = rows gt_off[b] .. gt_off[b+1]);
 * velocities flip, rotate and scale with the frame */
int32_t u3d_boxes_augment(float* boxes, const int32_t* gt_off, int32_t batch, int32_t n, int32_t box_dim, const float* params, int32_t coord,
                          u3d_stream s);
/* PointsRangeFilter: the points of scene b with lo < (x, y, z) < hi (strict), in their original order, compacted to the front of the
 * scene's own segment of `out` (same offsets as the input; out may alias points); count[b] = survivors.  range6 is a HOST array
 * (x0, y0, z0, x1, y1, z1); feat <= 8. */
int32_t u3d_points_range_filter(const float* points, const int32_t* scene_off, int32_t batch, int32_t feat, const float* range6, float* out,
                                int32_t* count, u3d_stream s);
/* PointSample: out [batch * num_points, feat], scene b = rows b*num_points ...: num_points rows of the first count[b] rows of the
 * scene's segment (count NULL = the whole segment) - distinct rows (a keyed pseudo-random permutation) when count[b] >= num_points,
 * uniform draws with replacement otherwise, zeros for an empty scene.  seed: device u64 (advance it per step); idx_out (nullable)
 * int32 [batch * num_points] = the chosen row within the scene (-1 for an empty scene). */
int32_t u3d_point_sample(const float* points, const int32_t* scene_off, const int32_t* count, int32_t batch, int32_t feat, int32_t num_points,
                         const uint64_t* seed, float* out, int32_t* idx_out, u3d_stream s);

/* ObjectRangeFilter (KITTI / nuScenes train pipelines; ref: projects/configs/uni3detr/uni3detr_kitti_3classes.py train_pipeline):
 * in place, per scene, order kept: boxes whose BEV centre lies strictly inside bev_range4 = (x0, y0, x1, y1) (HOST array) move to the
 * front of the scene's segment (labels int32, nullable, move with them), yaw wrapped into [-pi, pi); count[b] = survivors. */
int32_t u3d_boxes_range_filter(float* boxes, int32_t* labels, const int32_t* gt_off, int32_t batch, int32_t box_dim,
                               const float* bev_range4, int32_t* count, u3d_stream s);
/* PointShuffle: out [n_total, feat] f32, written out of place (out must not alias points): the first count[b] rows of scene b's
 * segment (count NULL = the whole segment) permuted by a keyed pseudo-random permutation (the PointSample one), every other row copied
 * as it is; seed: device u64, the scene index goes into the key (advance it per call). */
int32_t u3d_point_shuffle(const float* points, const int32_t* scene_off, const int32_t* count, int32_t batch, int32_t n_total, int32_t feat,
                          const uint64_t* seed, float* out, u3d_stream s);
/* ObjectNameFilter: in place, per scene, order kept: of the first gt_count[b] rows of scene b's segment (gt_count NULL = the whole
 * segment), the boxes whose label lies in [0, num_classes) move to the front (labels int32 move with them); count[b] = survivors
 * (count must not alias gt_count). */
int32_t u3d_boxes_label_filter(float* boxes, int32_t* labels, const int32_t* gt_off, const int32_t* gt_count, int32_t batch, int32_t box_dim,
                               int32_t num_classes, int32_t* count, u3d_stream s);

/* Batch ingest (uni3detr_amd/csrc/ingest.hip): a packed pipeline batch -> the static input buffers of a capacity-mode training step,
 * two launches, no allocation, no synchronisation (capturable).  In: points f32 [n_src, feat], scene_off int32 [batch + 1], count
 * int32 [batch] (nullable: live prefix of every segment); gt f32 [g_src, box_dim] bottom-centre (nullable / g_src 0: no boxes),
 * gt_labels int32 [g_src], gt_off int32 [batch + 1], gt_count (nullable).  Out (caller-owned, addresses kept): cat f32
 * [batch * point_cap, feat] exactly packed - scene b = rows dst_off[b] .. dst_off[b + 1], live rows only, order kept, rows past
 * dst_off[batch] untouched - and dst_off int32 [batch + 1]; gt_out f32 [batch * gt_cap, gt_dim] (gravity centre z + dz / 2, gt_dim 7 or
 * 9: a 7-column input gets zero velocities, a 9-column input is cut to 7), labels_out int32, gt_off_out int32 [batch + 1] (the three
 * nullable together).  A scene with more than point_cap live rows or more than gt_cap live boxes is cut to the capacity; then
 * flag[0] (one device float) is incremented by 1 and overflow (nullable int32 [2]) counts the call: [0] points, [1] boxes.
 * 16-byte copies when feat % 4 == 0 and both point buffers are 16-byte aligned; batch <= 4096. */
int32_t u3d_batch_ingest(const float* points, int32_t n_src, int32_t feat, const int32_t* scene_off, const int32_t* count, int32_t batch,
                         int32_t point_cap, const float* gt, int32_t g_src, int32_t box_dim, const int32_t* gt_labels, const int32_t* gt_off,
                         const int32_t* gt_count, int32_t gt_cap, int32_t gt_dim, float* cat, int32_t* dst_off, float* gt_out,
                         int32_t* labels_out, int32_t* gt_off_out, float* flag, int32_t* overflow, u3d_stream s);

/* GT-paste (mmdet3d ObjectSample / the plugin's UnifiedObjectSample, ref: projects/mmdet3d_plugin/datasets/pipelines/dbsampler.py,
 * transform_3d.py:591-786) and ObjectNoise (global_rot_range = 0) on a packed batch: uni3detr_amd/csrc/objaug.hip.  The random draws
 * stay with the caller (uni3detr_amd/datapath.py).  Boxes are bottom-centre (x, y, z, dx, dy, dz, yaw [, vx, vy]), box_dim 7 or 9.
 * count / gt_count / n_live / g_live (nullable where noted) give the live rows at the front of every scene's segment. */
/* stats [2*batch + batch*ncls] = live points per scene | live GT rows per scene | GT rows per (scene, label in [0, ncls)); ncls <= 64 */
int32_t u3d_objaug_stats(const int32_t* scene_off, const int32_t* count, const int32_t* gt_off, const int32_t* gt_count,
                         const int32_t* labels, int32_t batch, int32_t ncls, int32_t* stats, u3d_stream s);
/* candidates (database rows cand_ids, scene b = cand_off[b] .. cand_off[b+1], classes contiguous and labelled by cand_grp): BEV
 * collision against the scene's live GT and each other, then sample_class_v2's greedy rule -> acc[k] = 1 accepted / 0 rejected.
 * Every scene holds at most 32 * words <= 1024 candidates; hit_ws int32 [K], cc_ws uint32 [K * words]. */
int32_t u3d_objaug_accept(const float* gt, const int32_t* gt_off, const int32_t* g_live, int32_t box_dim, const float* db_boxes,
                          const int32_t* cand_ids, const int32_t* cand_off, const int32_t* cand_grp, int32_t batch, int32_t words,
                          int32_t* hit_ws, uint32_t* cc_ws, int32_t* acc, u3d_stream s);
/* points of scene b (first n_live[b] rows, n_live nullable) vs the boxes of scene b (box_live nullable, box_active nullable int32 per
 * box row): first[row] = scene-local index of the lowest box that holds the point strictly inside all six faces, -1 none;
 * bits (nullable) [rows][words] one bit per (point, box); tile_free (nullable) [batch][tiles] = points of each 256-row tile inside
 * no box.  tiles = ceil(max live points / 256). */
int32_t u3d_points_in_boxes(const float* points, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat,
                            int32_t tiles, const float* boxes, const int32_t* box_off, const int32_t* box_live, const int32_t* box_active,
                            int32_t box_dim, int32_t words, int32_t* first, uint32_t* bits, int32_t* tile_free, u3d_stream s);
/* the paste after u3d_points_in_boxes(box_active = acc): out_points / out_scene_off get, per scene, the accepted candidates' database
 * points translated by their box (candidate order) and the kept scene points (scene order) - sampled first when sampled_first
 * (mmdet3d ObjectSample), after them otherwise (UnifiedObjectSample); out_boxes / out_labels / out_gt_off (out_boxes nullable) the
 * live GT rows followed by the accepted boxes.  Rows past out_scene_off[batch] / out_gt_off[batch] are untouched.  Workspaces:
 * tile_base_ws int32 [batch * tiles], cand_base_ws / cand_row_ws int32 [n_cand]. */
int32_t u3d_objaug_paste(const float* points, const int32_t* scene_off, const int32_t* n_live, int32_t feat, const int32_t* first,
                         const int32_t* tile_free, int32_t tiles, const float* gt, const int32_t* labels, const int32_t* gt_off,
                         const int32_t* g_live, int32_t box_dim, const float* db_points, const int32_t* db_obj_off, const float* db_boxes,
                         const int32_t* db_labels, const int32_t* cand_ids, const int32_t* cand_off, const int32_t* acc, int32_t n_cand,
                         int32_t max_obj_points, int32_t batch, int32_t sampled_first, int32_t* tile_base_ws, int32_t* cand_base_ws,
                         int32_t* cand_row_ws, float* out_points, int32_t* out_scene_off, float* out_boxes, int32_t* out_labels,
                         int32_t* out_gt_off, u3d_stream s);
/* ObjectNoise in place: per scene (at most 1024 live boxes), box by box in index order, the lowest try j of loc [rows][num_try][3] /
 * rot [rows][num_try] whose moved BEV rectangle collides with no other box's current one (chosen[row] = j, -1 = none: the box stays);
 * then every point moves with the lowest-index original box holding it.  first_ws int32 [point rows], sel_ws f32 [box rows * 8]. */
int32_t u3d_object_noise(float* points, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat, int32_t tiles,
                         float* boxes, const int32_t* gt_off, const int32_t* g_live, int32_t box_dim, int32_t num_try, const float* loc,
                         const float* rot, int32_t* first_ws, float* sel_ws, int32_t* chosen, u3d_stream s);

/* Test-time augmentation: the multi-view box merge (ref: projects/mmdet3d_plugin/core/merge_all_augs.py:9-98, core/bbox/util.py:82-102)
 * for all scenes at once: uni3detr_amd/csrc/tta.hip.  Candidates: boxes [n, box_dim] f32 bottom-centre (box_dim 7 or 9), scores [n]
 * f32, labels [n] int32; det_off int32 [batch*views + 1] (device): view v = rows det_off[v] .. det_off[v+1]), scene s = views
 * s*views .. s*views + views - 1; params f32 [batch*views][U3D_AUG_NPARAM]: every view's FORWARD parameters (rotation by angle and
 * scale, then the flips - the inner test pipeline's order; translation ignored).  Per scene: every candidate is mapped back with
 * exactly the arithmetic of u3d_boxes_augment under (fh, fv, -sin, cos, -angle, 1/scale, 0, 0, 0); candidates with a non-finite score
 * or a label outside [0, num_classes) are dropped; per class (ascending; empty classes skipped) greedy rotated-BEV NMS in (score desc,
 * concatenated index asc) order - suppressed iff a kept higher-ranked candidate has BEV IoU > nms_thr, the BEV rows after the f32
 * round trip of xywhr2xyxyr + mmcv nms_bev; the kept ones class-major, stably sorted by descending score, the first max_num:
 * out_boxes [batch][max_num][box_dim], out_scores / out_labels [batch][max_num], out_count [batch] (rows past the count untouched).
 * max_per_scene >= the candidates of every scene: segments of more than U3D_TTA_LDS_CAP candidates take the global-memory path,
 * whose suppression masks the workspace holds when max_per_scene > U3D_TTA_LDS_CAP. */
#define U3D_TTA_LDS_CAP 2048
int64_t u3d_tta_merge_workspace(int32_t n, int32_t box_dim, int32_t batch, int32_t views, int32_t num_classes, int32_t max_per_scene);
int32_t u3d_tta_merge(const float* boxes, const float* scores, const int32_t* labels, int32_t n, int32_t box_dim, const int32_t* det_off,
                      const float* params, int32_t batch, int32_t views, int32_t coord, int32_t num_classes, float nms_thr, int32_t max_num,
                      int32_t max_per_scene, void* workspace, int64_t workspace_bytes, float* out_boxes, float* out_scores,
                      int32_t* out_labels, int32_t* out_count, u3d_stream s);
/* u3d_tta_merge behind the batched detection tail, whose counts exist only on the device: the same merge over the PADDED layout that
 * u3d_det_tail_pp writes for batch*views scenes (views scene-major, view-minor).  boxes f32 [batch*views][max_det][box_dim], scores f32
 * / labels int32 [batch*views][max_det], count int32 [batch*views] on the DEVICE, clamped to [0, max_det]; rows of a view at or past
 * its count are never read and may hold anything; params, coord, num_classes, nms_thr, max_num as u3d_tta_merge takes them.  Scene by
 * scene the result is bit-identical to u3d_tta_merge on rows [v][0 .. count[v]) of every view concatenated in view order: the same
 * kernels, with the candidate's memory row computed from the device scan of the counts.  The outputs form a complete DetBatch:
 * out_boxes [batch][max_num][box_dim], out_scores / out_labels [batch][max_num] with the rows at or past out_count[b] WRITTEN AS ZERO,
 * out_count int32 [batch], out_off int32 [batch+1] = exclusive scan of out_count.  No host-known row count: every grid, the workspace
 * and the choice of the global-memory NMS path (views*max_det > U3D_TTA_LDS_CAP) depend on batch, views, max_det, num_classes only;
 * no allocation, no synchronisation, no blocking copy - the call may be captured into a graph.  No atomics: equal inputs give equal
 * bytes.  Checked before any launch: U3D_ERR_ARG for a null pointer or a bad shape (batch, views, max_det, num_classes, max_num <= 0,
 * box_dim not 7 / 9, coord not 0 / 1); U3D_ERR_UNSUPPORTED for batch > 65535, max_det or max_num > U3D_DET_TAIL_MAX_K, batch*views*max_det
 * >= 2^31, or views*max_det > 524288 (the suppression words of one mask row must fit the sweep's 64 KiB of LDS); U3D_ERR_WORKSPACE
 * for a workspace below u3d_tta_merge_padded_workspace (which returns -1 for a shape the call refuses). */
int64_t u3d_tta_merge_padded_workspace(int32_t batch, int32_t views, int32_t max_det, int32_t box_dim, int32_t num_classes);
int32_t u3d_tta_merge_padded(const float* boxes, const float* scores, const int32_t* labels, const int32_t* count, int32_t batch,
                             int32_t views, int32_t max_det, int32_t box_dim, const float* params, int32_t coord, int32_t num_classes,
                             float nms_thr, int32_t max_num, void* workspace, int64_t workspace_bytes, float* out_boxes, float* out_scores,
                             int32_t* out_labels, int32_t* out_count, int32_t* out_off, u3d_stream s);

/* LoadPointsFromMultiSweeps (mmdet3d, recalled): uni3detr_amd/csrc/sweeps.hip.  Output, scene after scene:
 * the key frame (time column 4 set to 0), then every chosen sweep's rows that survive remove_close (|x| < 1 and |y| < 1 dropped, on
 * the raw coordinates), transformed in float64 as xyz_f32 = f32((r0*x + r1*y) + r2*z), xyz = f32(xyz_f32 + t), column 4 = f32(lag);
 * or the pad copies of the key frame (remove_close applied, untransformed, time 0); then out[:, k] = row[use_dim[k]].
 * Segments (key frame, sweep or pad copy), scene-major in output order: seg_tab int32 [n_seg][U3D_SWEEPS_SEG_FIELDS] = (kind, first
 * source row, rows): a sweep reads raw [n_raw_rows, load_dim], the key frame and pad copies key_points [n_key_rows, load_dim];
 * seg_param f64 [n_seg][U3D_SWEEPS_NPARAM] = (R row-major [9], t [3], lag); seg_chunk0 int32 [n_seg + 1] = the first chunk of
 * U3D_SWEEPS_CHUNK rows of every segment (ceil(rows / U3D_SWEEPS_CHUNK) chunks each, seg_chunk0[n_seg] = n_chunks); scene_chunk0
 * int32 [batch + 1] = the first chunk of every scene (n_chunks past the last).  All of them device arrays; use_dim (n_use <= 8) a HOST
 * array; 5 <= load_dim <= 8.  out [out_rows, n_use] (out_rows >= the sum of all segment rows); out_scene_off int32 [batch + 1]: the
 * output is exactly packed, rows past out_scene_off[batch] are untouched.  workspace: u3d_sweeps_merge_workspace(n_chunks) bytes. */
#define U3D_SWEEPS_CHUNK 256
#define U3D_SWEEPS_NPARAM 13
#define U3D_SWEEPS_SEG_FIELDS 3
#define U3D_SWEEP_SEG_KEY 0
#define U3D_SWEEP_SEG_SWEEP 1
#define U3D_SWEEP_SEG_PAD 2
int64_t u3d_sweeps_merge_workspace(int32_t n_chunks);
int32_t u3d_sweeps_merge(const float* key_points, int64_t n_key_rows, const float* raw, int64_t n_raw_rows, int32_t load_dim,
                         const int32_t* seg_tab, const double* seg_param, int32_t n_seg, const int32_t* seg_chunk0, const int32_t* scene_chunk0,
                         int32_t batch, int32_t n_chunks, const int32_t* use_dim, int32_t n_use, int32_t remove_close, void* workspace,
                         int64_t workspace_bytes, float* out, int64_t out_rows, int32_t* out_scene_off, u3d_stream s);

/* The GT-paste object database cropped on the device (mmdet3d create_groundtruth_database / the plugin's
 * extra_tools/data_converter/create_unified_gt_database.py:85-176 without the image part):
 * uni3detr_amd/csrc/gtdb.hip.  points [n_rows, feat] f32 (3 <= feat <= 8), scene b = rows scene_off[b] .. scene_off[b+1], of which the
 * first n_live[b] are live (n_live nullable); boxes [n_boxes, box_dim] f32 bottom-centre (box_dim 7 or 9), scene b owns box rows
 * box_off[b] .. box_off[b+1] (box_off[batch] == n_boxes); box_valid (nullable) int32 per box row: 0 = the box holds nothing.  Box row j
 * becomes object j: the live points of its scene strictly inside all six faces (the test of u3d_points_in_boxes, csrc/point_box.h), in
 * scene order, all feat columns, columns 0-2 minus the box's (x, y, z) in f32; a point inside two boxes goes to both.  No atomics: the
 * output is the same bytes on every run.  tiles = ceil(max live points of a scene / 256); tile_ws int32 [n_boxes][tiles].
 *   u3d_gtdb_count  tile_ws[j][t] = points of the scene's 256-point tile t inside box j
 *   u3d_gtdb_scan   tile_ws in place to its exclusive scan over t, num_points [n_boxes] = the row sums, obj_off [n_boxes + 1] = their
 *                   exclusive scan, total int64 [1] = their exact sum (device memory: the caller's one read, to size the output)
 *   u3d_gtdb_crop   out [total, feat]: object j = rows obj_off[j] .. obj_off[j+1]; `total` as read back from u3d_gtdb_scan
 * max_boxes: an upper bound of the boxes of one scene, known to the host; more than 1024 is U3D_ERR_UNSUPPORTED, and so is
 * n_boxes * tiles or total above INT32_MAX (the offsets are int32: crop fewer scenes per call) - all checked before any launch. */
int32_t u3d_gtdb_count(const float* points, int64_t n_rows, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat,
                       int32_t tiles, const float* boxes, int32_t n_boxes, const int32_t* box_off, const int32_t* box_valid, int32_t box_dim,
                       int32_t max_boxes, int32_t* tile_ws, u3d_stream s);
int32_t u3d_gtdb_scan(int32_t* tile_ws, int32_t n_boxes, int32_t tiles, int32_t* num_points, int32_t* obj_off, int64_t* total, u3d_stream s);
int32_t u3d_gtdb_crop(const float* points, int64_t n_rows, const int32_t* scene_off, const int32_t* n_live, int32_t batch, int32_t feat,
                      int32_t tiles, const float* boxes, int32_t n_boxes, const int32_t* box_off, const int32_t* box_valid, int32_t box_dim,
                      int32_t max_boxes, const int32_t* tile_ws, const int32_t* obj_off, int64_t total, float* out, u3d_stream s);

/* LoadPointsFromFile / NormalizePointsColor (mmdet3d, recalled): uni3detr_amd/csrc/points_load.hip.
 * raw [n_rows, load_dim] f32, 3 <= load_dim <= 8, n_rows < 2^31: the file rows of all scenes, scene b = rows scene_off[b] ..
 * scene_off[b+1] (exactly packed, device).  out [n_rows, n_use + (shift_height != 0)]: out[:, k] = raw[:, use_dim[k]] (use_dim a HOST
 * array, at most 8 output columns); with shift_height the column z - floor32 goes in after the third selected column, z = the third
 * selected column, and floor_height f32 [batch] gets floor32 per scene: load_table f64 [batch][2] = (i, g) of NumPy's `linear`
 * percentile (pos = (n - 1) * 0.0099, i = floor(pos), g = pos - i, computed by the host in float64); a = z_(i), b = z_(min(i + 1,
 * n - 1)) are the exact order statistics of the scene's float32 z; in float64 without contraction d = b - a, floor = a + d * g when
 * g < 0.5, b - d * (1 - g) otherwise; floor32 = f32(floor), height = z - floor32 in float32.  A NaN z makes the scene's floor and
 * heights NaN; an empty scene's floor is NaN.  workspace: u3d_points_load_workspace(n_rows, shift_height) bytes.  No host read. */
int64_t u3d_points_load_workspace(int64_t n_rows, int32_t shift_height);
int32_t u3d_points_load(const float* raw, int64_t n_rows, int32_t load_dim, const int32_t* scene_off, int32_t batch,
                        const double* load_table, const int32_t* use_dim, int32_t n_use, int32_t shift_height, void* workspace,
                        int64_t workspace_bytes, float* out, float* floor_height, u3d_stream s);
/* points [n_rows, feat] f32 in place: columns col0 .. col0 + 2 become (c - mean) / 255 in float32 (mean 0: only the division) */
int32_t u3d_points_color_norm(float* points, int64_t n_rows, int32_t feat, int32_t col0, float mean0, float mean1, float mean2,
                              u3d_stream s);

#ifdef __cplusplus
}
#endif
#endif /* U3D_HIP_H_ */
