// nuScenes detection evaluation on the device: the semantics of the nuscenes-devkit's detection_cvpr_2019 evaluation (the box
// conversion of upstream `_format_bbox`, filter_eval_boxes, accumulate, calc_ap, calc_tp), restated in uni3detr_amd/nuscenes_eval.py.
// Parity is unpinned: no devkit source is vendored here, the contract is the module docstring.
//
// Records (float64, NU_REC per row): 0-2 global centre (gravity), 3-5 size (w, l, h), 6 global yaw, 7-8 global velocity (x, y),
// 9 score (predictions) / num_lidar_pts + num_radar_pts (GT), 10 class (0..n_cls-1, NU_OTHER, NU_RACK), 11 attribute code (-1 = '';
// the LiDAR-frame yaw for a bicycle-rack row).
//   u3d_nusc_convert      one thread per box: LiDAR -> ego -> global (float64), the prediction attribute, the upstream ego-radius drop
//   u3d_nusc_filter       one thread per box: the devkit filters (ego_dist < class_range, GT points, bicycle / motorcycle in a rack)
//   (the caller scans the flags and keeps the valid rows with u3d_compact_rows, csrc/compact.hip)
//   u3d_nusc_rank_keys    descending-orderable 64-bit score keys in reversed row order (the caller stable-sorts by score, then class)
//   u3d_nusc_match        one wave per (class, sample): the four greedy matchings, the sample's GT of the class in LDS
//   u3d_nusc_accumulate   one workgroup per (class, threshold): tp cumsum, the 101-point interpolation, cummeans, calc_ap / calc_tp
// No float atomics and no order-dependent reductions: any batching of the same samples gives bit-identical results.
#include "common.h"

// The arithmetic below is restated operation by operation from the float64 NumPy path: no contraction into fused multiply-adds.
#pragma clang fp contract(off)

#define NU_REC 12
#define NU_NTH 4
#define NU_NI 101
#define NU_NERR 5
#define NU_THREADS 256
#define NU_ITEMS 8                  // consecutive ranks per thread in the accumulate scan
#define NU_MAX_GT 2048              // GT of one (class, sample) staged in LDS; the taken flags are 32-bit masks per lane
#define NU_OTHER -1
#define NU_RACK -2
#define NU_PI 3.141592653589793

// ---------------------------------------------------------------------------------------------------------------------------
// conversion.  rows f64 [n][9] = x, y, z, l, w, h, yaw, vx, vy in the LiDAR frame (z: bottom for predictions, gravity centre for GT);
// calib f64 [n_sample][24] = lidar2ego rotation (3x3 row-major), translation, ego2global rotation, translation.  valid int32 [n]:
// predictions: label in range and ego-frame xy radius <= class_range (upstream lidar_nusc_box_to_global); GT: an evaluated class or a rack.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NU_THREADS) void k_nusc_convert(const double* __restrict__ rows, const int* __restrict__ cls,
                                                             const int* __restrict__ attr, const double* __restrict__ aux,
                                                             const int* __restrict__ off, int n_sample, int n,
                                                             const double* __restrict__ calib, int is_pred,
                                                             const double* __restrict__ cls_range, const int* __restrict__ attr_moving,
                                                             const int* __restrict__ attr_still, int n_cls, double* __restrict__ rec,
                                                             int* __restrict__ valid) {
  const int d = blockIdx.x * NU_THREADS + threadIdx.x;
  if (d >= n) return;
  const int s = u3d_segment_of(off, n_sample, d);
  const double* R1 = calib + (long long)s * 24;
  const double* t1 = R1 + 9;
  const double* R2 = R1 + 12;
  const double* t2 = R1 + 21;
  const double* b = rows + (long long)d * 9;
  const double x = b[0], y = b[1], l = b[3], w = b[4], h = b[5], yaw = b[6], vx = b[7], vy = b[8];
  const double z = is_pred ? b[2] + h / 2.0 : b[2];
  const double ex = R1[0] * x + R1[1] * y + R1[2] * z + t1[0];
  const double ey = R1[3] * x + R1[4] * y + R1[5] * z + t1[1];
  const double ez = R1[6] * x + R1[7] * y + R1[8] * z + t1[2];
  const double gx = R2[0] * ex + R2[1] * ey + R2[2] * ez + t2[0];
  const double gy = R2[3] * ex + R2[4] * ey + R2[5] * ez + t2[1];
  const double gz = R2[6] * ex + R2[7] * ey + R2[8] * ez + t2[2];
  // first column of R2 R1 Rz(yaw) -> global yaw; the velocity (vx, vy, 0) takes the same two rotations
  const double c = cos(yaw), sn = sin(yaw);
  const double u0 = R1[0] * c + R1[1] * sn, u1 = R1[3] * c + R1[4] * sn, u2 = R1[6] * c + R1[7] * sn;
  const double gyaw = atan2(R2[3] * u0 + R2[4] * u1 + R2[5] * u2, R2[0] * u0 + R2[1] * u1 + R2[2] * u2);
  const double a0 = R1[0] * vx + R1[1] * vy, a1 = R1[3] * vx + R1[4] * vy, a2 = R1[6] * vx + R1[7] * vy;
  const double gvx = R2[0] * a0 + R2[1] * a1 + R2[2] * a2;
  const double gvy = R2[3] * a0 + R2[4] * a1 + R2[5] * a2;
  const int k = cls[d];
  int ok;
  double a11;
  if (is_pred) {
    ok = k >= 0 && k < n_cls;
    if (ok) ok = !(sqrt(ex * ex + ey * ey) > cls_range[k]);
    a11 = ok ? (double)(sqrt(gvx * gvx + gvy * gvy) > 0.2 ? attr_moving[k] : attr_still[k]) : -1.0;
  } else {
    ok = (k >= 0 && k < n_cls) || k == NU_RACK;
    a11 = k == NU_RACK ? yaw : (double)attr[d];
  }
  double* r = rec + (long long)d * NU_REC;
  r[0] = gx; r[1] = gy; r[2] = gz;
  r[3] = w; r[4] = l; r[5] = h;
  r[6] = gyaw; r[7] = gvx; r[8] = gvy;
  r[9] = aux[d];
  r[10] = (double)((k >= 0 && k < n_cls) || k == NU_RACK ? k : NU_OTHER);
  r[11] = a11;
  valid[d] = ok;
}

extern "C" int32_t u3d_nusc_convert(const double* rows, const int32_t* cls, const int32_t* attr, const double* aux, const int32_t* off,
                                    int32_t n_sample, int32_t n, const double* calib, int32_t is_pred, const double* cls_range,
                                    const int32_t* attr_moving, const int32_t* attr_still, int32_t n_cls, double* rec, int32_t* valid,
                                    u3d_stream s) {
  U3D_REQUIRE(n >= 0 && n_sample >= 0 && n_cls > 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(rows && cls && aux && off && n_sample > 0 && calib && cls_range && rec && valid, U3D_ERR_ARG);
  U3D_REQUIRE(is_pred ? (attr_moving && attr_still) : attr != nullptr, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_nusc_convert, dim3(u3d_cdiv(n, NU_THREADS)), dim3(NU_THREADS), 0, s, rows, cls, attr, aux, off, n_sample, n, calib,
                     is_pred, cls_range, attr_moving, attr_still, n_cls, rec, valid);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// devkit filters, valid int32 [n] in / out: ego_dist = |global xy - ego2global translation| < class_range; GT with no lidar / radar
// point; a bicycle or motorcycle whose centre lies inside one of its sample's racks (rack rows of gt / gt_off), bounds inclusive,
// tested in the rack's own frame (R2 R1 Rz(LiDAR yaw)).
// ---------------------------------------------------------------------------------------------------------------------------
__device__ static bool nu_in_rack(const double* __restrict__ p, const double* __restrict__ rk, const double* __restrict__ R1,
                                  const double* __restrict__ R2) {
  const double d0 = p[0] - rk[0], d1 = p[1] - rk[1], d2 = p[2] - rk[2];
  const double a0 = R2[0] * d0 + R2[3] * d1 + R2[6] * d2;
  const double a1 = R2[1] * d0 + R2[4] * d1 + R2[7] * d2;
  const double a2 = R2[2] * d0 + R2[5] * d1 + R2[8] * d2;
  const double b0 = R1[0] * a0 + R1[3] * a1 + R1[6] * a2;
  const double b1 = R1[1] * a0 + R1[4] * a1 + R1[7] * a2;
  const double b2 = R1[2] * a0 + R1[5] * a1 + R1[8] * a2;
  const double c = cos(rk[11]), sn = sin(rk[11]);
  const double lx = c * b0 + sn * b1, ly = c * b1 - sn * b0;
  return fabs(lx) <= rk[4] / 2.0 && fabs(ly) <= rk[3] / 2.0 && fabs(b2) <= rk[5] / 2.0;
}

__global__ __launch_bounds__(NU_THREADS) void k_nusc_filter(const double* __restrict__ rec, const int* __restrict__ off, int n_sample,
                                                            int n, int is_pred, const double* __restrict__ calib,
                                                            const double* __restrict__ gt, const int* __restrict__ gt_off,
                                                            const double* __restrict__ cls_range, const int* __restrict__ bike, int n_cls,
                                                            int* __restrict__ valid) {
  const int d = blockIdx.x * NU_THREADS + threadIdx.x;
  if (d >= n || !valid[d]) return;
  const double* r = rec + (long long)d * NU_REC;
  const int k = (int)r[10];
  if (k < 0 || k >= n_cls) { valid[d] = 0; return; }
  const int s = u3d_segment_of(off, n_sample, d);
  const double* R1 = calib + (long long)s * 24;
  const double* t2 = R1 + 21;
  const double dx = r[0] - t2[0], dy = r[1] - t2[1];
  bool ok = sqrt(dx * dx + dy * dy) < cls_range[k];
  if (!is_pred) ok = ok && r[9] != 0.0;
  if (ok && bike[k]) {
    for (int i = gt_off[s]; i < gt_off[s + 1]; ++i) {
      const double* rk = gt + (long long)i * NU_REC;
      if ((int)rk[10] == NU_RACK && nu_in_rack(r, rk, R1, R1 + 12)) { ok = false; break; }
    }
  }
  valid[d] = ok ? 1 : 0;
}

extern "C" int32_t u3d_nusc_filter(const double* rec, const int32_t* off, int32_t n_sample, int32_t n, int32_t is_pred, const double* calib,
                                   const double* gt, const int32_t* gt_off, const double* cls_range, const int32_t* bike, int32_t n_cls,
                                   int32_t* valid, u3d_stream s) {
  U3D_REQUIRE(n >= 0 && n_sample >= 0 && n_cls > 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(rec && off && n_sample > 0 && calib && gt_off && cls_range && bike && valid, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_nusc_filter, dim3(u3d_cdiv(n, NU_THREADS)), dim3(NU_THREADS), 0, s, rec, off, n_sample, n, is_pred, calib, gt, gt_off,
                     cls_range, bike, n_cls, valid);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// rank keys: key[n-1-i] = descending-orderable bits of score_i (-0.0 folded into +0.0), idx[n-1-i] = i.  A stable ascending sort of
// the keys then orders by (score desc, row desc): the devkit's sorted((score, index))[::-1]; a second stable sort by class keeps it.
// ---------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NU_THREADS) void k_nusc_rank_keys(const double* __restrict__ rec, int n, long long* __restrict__ key,
                                                               int* __restrict__ idx) {
  const int i = blockIdx.x * NU_THREADS + threadIdx.x;
  if (i >= n) return;
  const long long b = __double_as_longlong(rec[(long long)i * NU_REC + 9] + 0.0);
  const long long o = b >= 0 ? b : (b ^ 0x7fffffffffffffffll);
  key[n - 1 - i] = ~o;
  idx[n - 1 - i] = i;
}

extern "C" int32_t u3d_nusc_rank_keys(const double* rec, int32_t n, int64_t* key, int32_t* idx, u3d_stream s) {
  U3D_REQUIRE(n >= 0, U3D_ERR_ARG);
  if (n == 0) return U3D_OK;
  U3D_REQUIRE(rec && key && idx, U3D_ERR_ARG);
  hipLaunchKernelGGL(k_nusc_rank_keys, dim3(u3d_cdiv(n, NU_THREADS)), dim3(NU_THREADS), 0, s, rec, n, (long long*)key, idx);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// matching, one wave per segment q = class * n_sample + sample.  rank int32 [n] = prediction rows in rank order; mperm int32 [n] =
// rank positions grouped by segment (rank order inside a segment), mseg int32 [n_seg+1]; gord int32 = GT rows grouped by segment
// (row order inside), gseg [n_seg+1].  The segment's GT xy sit in LDS (f64); lane L owns GT L + 64 q and keeps one taken bit per
// (threshold, q).  Per prediction, in rank order, each threshold takes the untaken GT at minimum centre distance (strict '<' in index
// order, then a wave argmin with the lowest index on ties); a TP iff that distance < ths[t].  Outputs by rank position r:
// tp int8 [4][n], match int32 [n] = the GT row taken at threshold tp_th (-1: none).
// ---------------------------------------------------------------------------------------------------------------------------
static inline int64_t nusc_match_lds(int32_t max_gt) { return (int64_t)max_gt * 16; }

__global__ __launch_bounds__(64) void k_nusc_match(const double* __restrict__ pred, const int* __restrict__ rank, const int* __restrict__ mperm,
                                                   const int* __restrict__ mseg, const double* __restrict__ gt, const int* __restrict__ gord,
                                                   const int* __restrict__ gseg, const double* __restrict__ ths, int tp_th, int n,
                                                   signed char* __restrict__ tp, int* __restrict__ match) {
  extern __shared__ double nu_gxy[];
  const int q = blockIdx.x, lane = threadIdx.x;
  const int p0 = mseg[q], np_ = mseg[q + 1] - p0, g0 = gseg[q], ng = gseg[q + 1] - g0;
  if (np_ == 0) return;
  double* gx = nu_gxy;
  double* gy = nu_gxy + ng;
  for (int k = lane; k < ng; k += 64) {
    const long long gi = gord[g0 + k];
    gx[k] = gt[gi * NU_REC + 0];
    gy[k] = gt[gi * NU_REC + 1];
  }
  __syncthreads();
  double th[NU_NTH];
#pragma unroll
  for (int t = 0; t < NU_NTH; ++t) th[t] = ths[t];
  unsigned int taken[NU_NTH] = {0u, 0u, 0u, 0u};
  const int nq = (ng + 63) >> 6;
  for (int k = 0; k < np_; ++k) {
    const int r = mperm[p0 + k];
    const double* p = pred + (long long)rank[r] * NU_REC;
    const double px = p[0], py = p[1];
    double best[NU_NTH];
    int bi[NU_NTH];
#pragma unroll
    for (int t = 0; t < NU_NTH; ++t) { best[t] = INFINITY; bi[t] = -1; }
    for (int j = 0; j < nq; ++j) {
      const int g = lane + 64 * j;
      if (g >= ng) break;
      const double dx = px - gx[g], dy = py - gy[g];
      const double dist = sqrt(dx * dx + dy * dy);
#pragma unroll
      for (int t = 0; t < NU_NTH; ++t)
        if (!((taken[t] >> j) & 1u) && dist < best[t]) { best[t] = dist; bi[t] = g; }
    }
#pragma unroll
    for (int t = 0; t < NU_NTH; ++t) {
#pragma unroll
      for (int m = 32; m > 0; m >>= 1) {
        const double ob = __shfl_xor(best[t], m, 64);
        const int oi = __shfl_xor(bi[t], m, 64);
        if (oi >= 0 && (bi[t] < 0 || ob < best[t] || (ob == best[t] && oi < bi[t]))) { best[t] = ob; bi[t] = oi; }
      }
      const bool hit = bi[t] >= 0 && best[t] < th[t];
      if (hit && (bi[t] & 63) == lane) taken[t] |= 1u << (bi[t] >> 6);
      if (lane == 0) tp[(long long)t * n + r] = hit ? 1 : 0;
      if (lane == 0 && t == tp_th) match[r] = hit ? gord[g0 + bi[t]] : -1;
    }
  }
}

extern "C" int32_t u3d_nusc_match(const double* pred, const int32_t* rank, const int32_t* mperm, const int32_t* mseg, int32_t n_seg, int32_t n,
                                  const double* gt, const int32_t* gord, const int32_t* gseg, int32_t max_gt, const double* ths, int32_t tp_th,
                                  int8_t* tp, int32_t* match, u3d_stream s) {
  U3D_REQUIRE(n_seg >= 0 && n >= 0 && max_gt >= 0 && tp_th >= 0 && tp_th < NU_NTH, U3D_ERR_ARG);
  U3D_REQUIRE(max_gt <= NU_MAX_GT, U3D_ERR_UNSUPPORTED);
  if (n_seg == 0 || n == 0) return U3D_OK;
  U3D_REQUIRE(pred && rank && mperm && mseg && gseg && ths && tp && match && (max_gt == 0 || (gt && gord)), U3D_ERR_ARG);
  hipLaunchKernelGGL(k_nusc_match, dim3(n_seg), dim3(64), (size_t)nusc_match_lds(max_gt), s, pred, rank, mperm, mseg, gt, gord, gseg,
                     ths, tp_th, n, (signed char*)tp, match);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// accumulate, one workgroup per (class c, threshold t), block = c * 4 + t.  cseg int32 [n_cls+1] = class segments of the rank order,
// npos int32 [n_cls], gcoff int32 [n_cls] = exclusive scan of npos (each class's TP slots in the workspace: TPs <= npos).
//   1. tp cumsum (integers) -> ctp; at t == tp_th every TP writes its score and five errors (trans, scale, orient, vel, attr) to slot
//      gcoff[c] + ctp - 1;
//   2. prec = ctp / (i + 1), rec = ctp / npos; np.interp(ri, rec, prec | conf, right=0) at the 101 recall points (NumPy's rule: the
//      last index of a run of equal rec, the exact-hit and NaN fallbacks); max_recall_ind = last non-zero interpolated confidence;
//      calc_ap = mean(max(prec[11:] - 0.1, 0)) / 0.9;
//   3. at t == tp_th: five NaN-aware cummeans, each one sequential float64 scan, then np.interp(conf, TP confs ascending, cummean)
//      (default left / right); calc_tp = the mean over [11, max_recall_ind], 1.0 when empty.
//   npos == 0 or no TP: the devkit's no_predictions (precision / confidence 0, errors 1, AP 0, calc_tp 1).
// Outputs: prec / conf f64 [n_cls][4][101], err f64 [n_cls][5][101] (t == tp_th), ap f64 [n_cls][4], tp_err f64 [n_cls][5],
// mri int32 [n_cls][4].
// ---------------------------------------------------------------------------------------------------------------------------
extern "C" int64_t u3d_nusc_accumulate_workspace(int32_t n, int32_t n_gt) {
  return ((int64_t)NU_NTH * n * 4 + 15) / 16 * 16 + (int64_t)(NU_NERR + 1) * n_gt * 8;
}

// numpy.interp(x, xp, fp, left, right) for non-decreasing xp given by index functors (n >= 1)
template <class XP, class FP>
__device__ static double nu_interp(double x, int n, XP xp, FP fp, double left, double right) {
  if (x != x) return x;
  if (x > xp(n - 1)) return right;
  if (x < xp(0)) return left;
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (x >= xp(mid)) lo = mid + 1; else hi = mid;
  }
  const int j = lo - 1;
  const double xj = xp(j), fj = fp(j);
  if (j == n - 1 || xj == x) return fj;
  const double xk = xp(j + 1), fk = fp(j + 1);
  const double slope = (fk - fj) / (xk - xj);
  double r = slope * (x - xj) + fj;
  if (r != r) {
    r = slope * (x - xk) + fk;
    if (r != r && fj == fk) r = fj;
  }
  return r;
}

__device__ static double nu_angle_diff(double x, double y, double period) {
  // (x - y + period / 2) % period - period / 2 with Python's float modulo (the sign of the divisor), then into (-pi, pi]
  const double a = x - y + period / 2.0;
  double m = fmod(a, period);
  if (m != 0.0) {
    if ((period < 0.0) != (m < 0.0)) m += period;
  } else {
    m = copysign(0.0, period);
  }
  double diff = m - period / 2.0;
  if (diff > NU_PI) diff = diff - 2.0 * NU_PI;
  return diff;
}

__global__ __launch_bounds__(NU_THREADS) void k_nusc_accumulate(const double* __restrict__ pred, const double* __restrict__ gt,
                                                                const int* __restrict__ rank, const int* __restrict__ cseg,
                                                                const int* __restrict__ npos_c, const int* __restrict__ gcoff, int n,
                                                                int n_gt, const signed char* __restrict__ tp, const int* __restrict__ match,
                                                                const double* __restrict__ ri, const double* __restrict__ period_c,
                                                                int tp_th, int* __restrict__ ctp, double* __restrict__ ews,
                                                                double* __restrict__ prec_o, double* __restrict__ conf_o,
                                                                double* __restrict__ err_o, double* __restrict__ ap_o,
                                                                double* __restrict__ tperr_o, int* __restrict__ mri_o) {
  __shared__ int wsum[NU_THREADS / 64];
  __shared__ int carry_s;
  __shared__ double prec_s[NU_NI], conf_s[NU_NI];
  __shared__ int mri_s;
  __shared__ int allnan_s[NU_NERR];
  const int c = blockIdx.x / NU_NTH, t = blockIdx.x - c * NU_NTH;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c0 = cseg[c], nc = cseg[c + 1] - c0, npos = npos_c[c];
  const bool tpth = t == tp_th;
  const signed char* tpf = tp + (long long)t * n + c0;
  int* cs = ctp + (long long)t * n + c0;
  double* mconf = ews + (long long)NU_NERR * n_gt + gcoff[c];
  if (tid == 0) carry_s = 0;
  __syncthreads();
  // 1. integer cumsum of the tp flags, NU_ITEMS consecutive ranks per thread
  for (int base = 0; base < nc; base += NU_THREADS * NU_ITEMS) {
    const int i0 = base + tid * NU_ITEMS;
    int f[NU_ITEMS];
    int tot = 0;
#pragma unroll
    for (int u = 0; u < NU_ITEMS; ++u) {
      f[u] = (i0 + u < nc) ? (int)tpf[i0 + u] : 0;
      tot += f[u];
    }
    int incl = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o, 64);
      if (lane >= o) incl += v;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    int pre = carry_s;
    for (int w = 0; w < wv; ++w) pre += wsum[w];
    int run = pre + incl - tot;
#pragma unroll
    for (int u = 0; u < NU_ITEMS; ++u) {
      const int i = i0 + u;
      if (i >= nc) break;
      run += f[u];
      cs[i] = run;
      if (tpth && f[u]) {
        const int k = run - 1;
        const double* p = pred + (long long)rank[c0 + i] * NU_REC;
        const double* g = gt + (long long)match[c0 + i] * NU_REC;
        const double dx = p[0] - g[0], dy = p[1] - g[1];
        const double dvx = p[7] - g[7], dvy = p[8] - g[8];
        const double mw = fmin(g[3], p[3]), ml = fmin(g[4], p[4]), mh = fmin(g[5], p[5]);
        const double va = g[3] * g[4] * g[5], vr = p[3] * p[4] * p[5], inter = mw * ml * mh;
        mconf[k] = p[9];
        ews[(long long)0 * n_gt + gcoff[c] + k] = sqrt(dx * dx + dy * dy);
        ews[(long long)1 * n_gt + gcoff[c] + k] = 1.0 - inter / (va + vr - inter);
        ews[(long long)2 * n_gt + gcoff[c] + k] = fabs(nu_angle_diff(g[6], p[6], period_c[c]));
        ews[(long long)3 * n_gt + gcoff[c] + k] = sqrt(dvx * dvx + dvy * dvy);
        ews[(long long)4 * n_gt + gcoff[c] + k] = g[11] < 0.0 ? (double)NAN : 1.0 - (g[11] == p[11] ? 1.0 : 0.0);
      }
    }
    __syncthreads();
    if (tid == NU_THREADS - 1) carry_s = run;
    __syncthreads();
  }
  const int ntp = carry_s;
  double* po = prec_o + ((long long)c * NU_NTH + t) * NU_NI;
  double* co = conf_o + ((long long)c * NU_NTH + t) * NU_NI;
  double* eo = err_o + (long long)c * NU_NERR * NU_NI;
  if (npos == 0 || ntp == 0) {
    for (int q = tid; q < NU_NI; q += NU_THREADS) { po[q] = 0.0; co[q] = 0.0; }
    if (tpth) {
      for (int q = tid; q < NU_NERR * NU_NI; q += NU_THREADS) eo[q] = 1.0;
      if (tid < NU_NERR) tperr_o[c * NU_NERR + tid] = 1.0;
    }
    if (tid == 0) { ap_o[c * NU_NTH + t] = 0.0; mri_o[c * NU_NTH + t] = 0; }
    return;
  }
  // 2. interpolation at the 101 recall points
  const double dn = (double)npos;
  const int* csv = cs;
  const double* sc = pred;
  const int* rk = rank + c0;
  if (tid < NU_NI) {
    const double x = ri[tid];
    auto rec = [&](int i) { return (double)csv[i] / dn; };
    auto prc = [&](int i) { return (double)csv[i] / (double)(i + 1); };
    auto cnf = [&](int i) { return sc[(long long)rk[i] * NU_REC + 9]; };
    const double pv = nu_interp(x, nc, rec, prc, prc(0), 0.0);
    const double cv = nu_interp(x, nc, rec, cnf, cnf(0), 0.0);
    prec_s[tid] = pv; conf_s[tid] = cv;
    po[tid] = pv; co[tid] = cv;
  }
  __syncthreads();
  if (tid == 0) {
    int m = 0;
    for (int q = 0; q < NU_NI; ++q)
      if (conf_s[q] != 0.0) m = q;
    mri_s = m;
    mri_o[c * NU_NTH + t] = m;
    double s = 0.0;
    for (int q = 11; q < NU_NI; ++q) s += fmax(prec_s[q] - 0.1, 0.0);
    ap_o[c * NU_NTH + t] = s / (double)(NU_NI - 11) / (1.0 - 0.1);
  }
  if (!tpth) return;
  // 3. NaN-aware cummeans (one sequential scan per error), in place
  if (tid < NU_NERR) {
    double* e = ews + (long long)tid * n_gt + gcoff[c];
    double sum = 0.0;
    int cnt = 0;
    for (int k = 0; k < ntp; ++k) {
      const double v = e[k];
      if (v == v) { sum += v; ++cnt; }
      e[k] = cnt ? sum / (double)cnt : 0.0;
    }
    allnan_s[tid] = cnt == 0;
  }
  __syncthreads();
  for (int task = tid; task < NU_NERR * NU_NI; task += NU_THREADS) {
    const int e = task / NU_NI, q = task - e * NU_NI;
    const double* cm = ews + (long long)e * n_gt + gcoff[c];
    double v = 1.0;
    if (!allnan_s[e]) {
      auto xp = [&](int i) { return mconf[ntp - 1 - i]; };
      auto fp = [&](int i) { return cm[ntp - 1 - i]; };
      v = nu_interp(conf_s[q], ntp, xp, fp, fp(0), fp(ntp - 1));
    }
    eo[task] = v;
  }
  __syncthreads();
  if (tid < NU_NERR) {
    const int last = mri_s;
    double r = 1.0;
    if (last >= 11) {
      double s = 0.0;
      for (int q = 11; q <= last; ++q) s += eo[tid * NU_NI + q];
      r = s / (double)(last - 10);
    }
    tperr_o[c * NU_NERR + tid] = r;
  }
}

extern "C" int32_t u3d_nusc_accumulate(const double* pred, const double* gt, const int32_t* rank, const int32_t* cseg, const int32_t* npos,
                                       const int32_t* gcoff, int32_t n_cls, int32_t n, int32_t n_gt, const int8_t* tp, const int32_t* match,
                                       const double* rec_interp, const double* period, int32_t tp_th, void* ws, int64_t ws_bytes,
                                       double* prec, double* conf, double* err, double* ap, double* tp_err, int32_t* mri, u3d_stream s) {
  U3D_REQUIRE(n_cls > 0 && n >= 0 && n_gt >= 0 && tp_th >= 0 && tp_th < NU_NTH, U3D_ERR_ARG);
  U3D_REQUIRE(ws_bytes >= u3d_nusc_accumulate_workspace(n, n_gt), U3D_ERR_WORKSPACE);
  U3D_REQUIRE(cseg && npos && gcoff && rec_interp && period && prec && conf && err && ap && tp_err && mri, U3D_ERR_ARG);
  U3D_REQUIRE(n == 0 || (pred && rank && tp && match && ws), U3D_ERR_ARG);
  U3D_REQUIRE(n_gt == 0 || (gt && ws), U3D_ERR_ARG);
  int* ctp = (int*)ws;
  double* ews = (double*)((char*)ws + ((int64_t)NU_NTH * n * 4 + 15) / 16 * 16);
  hipLaunchKernelGGL(k_nusc_accumulate, dim3(n_cls * NU_NTH), dim3(NU_THREADS), 0, s, pred, gt, rank, cseg, npos, gcoff, n, n_gt,
                     (const signed char*)tp, match, rec_interp, period, tp_th, ctp, ews, prec, conf, err, ap, tp_err, mri);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
