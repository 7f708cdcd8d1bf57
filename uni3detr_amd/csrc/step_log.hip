// Device-resident step log of the training step (include/u3d_hip.h: u3d_step_log_*).
//
// The log is a ring of `capacity` rows of U3D_STEP_LOG_FIXED + n_terms 32-bit columns and one int64 cursor, both in device memory.  The
// cursor counts the rows appended so far; row k lives in slot k % capacity.  u3d_step_log_append is the ring's only writer: one launch
// of one workgroup at the end of the step's last captured stage, plain loads and stores, no atomics - launches on one stream run one
// after the other, so the cursor needs none.  u3d_step_log_window reduces the latest rows column by column for the line a trainer
// prints: one workgroup per column, the rows taken in ascending step order by ONE thread (the float64 sum has a fixed order: two calls
// give the same bytes, a numpy loop gives the same bits); the other threads only stage the column through LDS.
// Neither kernel is throughput work: a row is at most 72 words, a window at most `capacity` values per column.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "u3d_hip.h"

#define SL_FIXED U3D_STEP_LOG_FIXED
#define SL_MAX_TERMS U3D_STEP_LOG_MAX_TERMS
#define SL_APPEND_BLOCK 128             // >= SL_FIXED + SL_MAX_TERMS: one thread per column
#define SL_WINDOW_BLOCK 256

static_assert(SL_FIXED + SL_MAX_TERMS <= SL_APPEND_BLOCK, "one thread per column of a row");

struct StepLogTerms { const float* t[SL_MAX_TERMS]; };     // by value: a captured launch keeps the pointers

__global__ __launch_bounds__(SL_APPEND_BLOCK) void k_step_log_append(StepLogTerms terms, int n_terms, const float* __restrict__ total,
                                                                     const float* __restrict__ state, const float* __restrict__ acc_state,
                                                                     uint32_t* __restrict__ rows, long long* __restrict__ cursor,
                                                                     long long capacity) {
  __shared__ long long s_k;
  long long k = 0;
  if (threadIdx.x == 0) {
    k = *cursor;
    s_k = k;
  }
  __syncthreads();
  const long long row = s_k;
  const int c = threadIdx.x, ncols = SL_FIXED + n_terms;
  if (c < ncols) {
    uint32_t w = 0u;
    switch (c) {
      case 0: w = (uint32_t)(int32_t)row; break;
      case 1: w = (uint32_t)(acc_state ? (int32_t)acc_state[5] : (state[11] > 0.f ? 3 : 1)); break;
      case 2: w = __float_as_uint(*total); break;
      case 3: w = __float_as_uint(acc_state ? acc_state[6] : state[4]); break;
      case 4: w = __float_as_uint(state[1]); break;
      case 5: w = __float_as_uint(state[5]); break;
      case 6: w = __float_as_uint(state[6]); break;
      case 7: w = 0u; break;
      default: w = __float_as_uint(*terms.t[c - SL_FIXED]); break;
    }
    rows[(row >= 0 ? row % capacity : 0) * ncols + c] = w;
  }
  if (threadIdx.x == 0) *cursor = k + 1;      // (k is this thread's own load: the store cannot pass it)
}

extern "C" int64_t u3d_step_log_bytes(int64_t capacity, int32_t n_terms) {
  if (capacity <= 0 || n_terms < 0 || n_terms > SL_MAX_TERMS) return 0;
  return capacity * (int64_t)(SL_FIXED + n_terms) * 4;
}

extern "C" int32_t u3d_step_log_append(const float* const* terms, int32_t n_terms, const float* total, const float* opt_state,
                                       const float* acc_state, void* rows, int64_t* cursor, int64_t capacity, u3d_stream s) {
  U3D_REQUIRE(n_terms >= 0 && n_terms <= SL_MAX_TERMS && capacity > 0, U3D_ERR_ARG);
  U3D_REQUIRE(total && opt_state && rows && cursor && (n_terms == 0 || terms), U3D_ERR_ARG);
  StepLogTerms a;
  for (int i = 0; i < SL_MAX_TERMS; ++i) a.t[i] = i < n_terms ? terms[i] : nullptr;
  for (int i = 0; i < n_terms; ++i) U3D_REQUIRE(a.t[i], U3D_ERR_ARG);
  hipLaunchKernelGGL(k_step_log_append, dim3(1), dim3(SL_APPEND_BLOCK), 0, s, a, (int)n_terms, total, opt_state, acc_state,
                     (uint32_t*)rows, (long long*)cursor, (long long)capacity);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}

// Block c reduces column c over the rows [cursor - n, cursor), n = min(last, cursor, capacity), oldest first.  A held row (outcome 3)
// is used by no column; columns 3 and 4 (gradient norm, clip coefficient) exist only where an update was applied (outcome 1); a NaN /
// Inf is skipped.  Block 0 writes the counts, blocks 0 and 1 (step number, outcome: no statistics) write zeros.
__global__ __launch_bounds__(SL_WINDOW_BLOCK) void k_step_log_window(const uint32_t* __restrict__ rows, const long long* __restrict__ cursor,
                                                                     long long capacity, int ncols, long long last,
                                                                     float* __restrict__ out, int32_t* __restrict__ counts) {
  __shared__ float s_v[SL_WINDOW_BLOCK];
  __shared__ int s_o[SL_WINDOW_BLOCK];
  const int c = blockIdx.x;
  const long long cur = *cursor;
  long long n = last < cur ? last : cur;
  n = n < capacity ? n : capacity;
  n = n > 0 ? n : 0;
  const long long first = cur - n;
  double sum = 0.0;
  float lo = 0.f, hi = 0.f;
  int used = 0, held = 0, dropped = 0, bad_total = 0;
  for (long long base = 0; base < n; base += SL_WINDOW_BLOCK) {
    const long long i = base + threadIdx.x;
    if (i < n) {
      const uint32_t* r = rows + ((first + i) % capacity) * ncols;
      s_o[threadIdx.x] = (int)r[1];
      s_v[threadIdx.x] = __uint_as_float(r[c]);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const int m = (int)((n - base) < SL_WINDOW_BLOCK ? (n - base) : SL_WINDOW_BLOCK);
      for (int j = 0; j < m; ++j) {
        const int o = s_o[j];
        held += o == 3;
        dropped += o == 2;
        if (o == 3) continue;
        const float v = s_v[j];
        const bool finite = fabsf(v) <= 3.402823466e38f;      // false for NaN and +-Inf
        if (c == 2 && !finite) ++bad_total;
        if (!finite || ((c == 3 || c == 4) && o != 1)) continue;
        sum += (double)v;
        lo = used ? fminf(lo, v) : v;
        hi = used ? fmaxf(hi, v) : v;
        ++used;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const bool stat = c >= 2;
    out[4 * c + 0] = stat && used ? (float)(sum / (double)used) : 0.f;
    out[4 * c + 1] = stat ? lo : 0.f;
    out[4 * c + 2] = stat ? hi : 0.f;
    out[4 * c + 3] = stat ? (float)used : 0.f;
    if (c == 0) {
      counts[0] = (int32_t)n;
      counts[1] = held;
      counts[2] = dropped;
    }
    if (c == 2) counts[3] = bad_total;
  }
}

extern "C" int32_t u3d_step_log_window(const void* rows, const int64_t* cursor, int64_t capacity, int32_t n_terms, int64_t last,
                                       float* out, int32_t* counts, u3d_stream s) {
  U3D_REQUIRE(n_terms >= 0 && n_terms <= SL_MAX_TERMS && capacity > 0 && last >= 0, U3D_ERR_ARG);
  U3D_REQUIRE(rows && cursor && out && counts, U3D_ERR_ARG);
  const int ncols = SL_FIXED + n_terms;
  hipLaunchKernelGGL(k_step_log_window, dim3(ncols), dim3(SL_WINDOW_BLOCK), 0, s, (const uint32_t*)rows, (const long long*)cursor,
                     (long long)capacity, ncols, (long long)last, out, counts);
  U3D_CHECK_LAUNCH();
  return U3D_OK;
}
