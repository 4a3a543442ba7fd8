// block_primitives.h -- the wave and workgroup building blocks shared by the refiner and evaluation kernels (device only, wave64).
//
// Determinism.  Every reduction here has ONE order, whatever the data: a butterfly inside the wave (__shfl_xor with offsets 32, 16, .. 1,
// v = op(v, other lane's v), after which every lane holds the same bits), then the waves' results folded in ascending wave order,
// s = op(s, red[w]).  A sum starts from 0 and adds the waves 0, 1, 2, ..; every other operator starts from red[0].  The kernels that promise
// bit-reproducible results, and the host emulations that pin them, rest on exactly this order.
//
// Barrier contract of block_reduce_all and block_compact.  Each holds two barriers: one BEFORE lane 0 of every wave writes its LDS
// entry (every thread has finished reading the array from an earlier call), one before the entries are read.  So
//   * the helpers may be called back to back on the same array, and on an array that the caller read before the call;
//   * there is NO trailing barrier: LDS that the caller writes after the call is not ordered against other threads' reads of it
//     before the call -- the caller places that barrier itself where it needs one;
//   * every thread of the workgroup must reach the call (a call under divergent control flow hangs the workgroup);
//   * WAVES is the workgroup's wave count, a compile-time fact at every call site (its __launch_bounds__ / 64).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mp {

// ---- shuffles of any value made of 32-bit words (float, double, 64-bit integers, small structs) --------------------------------------------
template <typename T, typename F>
__device__ __forceinline__ T shfl_words(T v, F shfl) {
  static_assert(sizeof(T) % 4 == 0, "a value of whole 32-bit words");
  uint32_t w[sizeof(T) / 4];
  __builtin_memcpy(w, &v, sizeof(T));
#pragma unroll
  for (int k = 0; k < (int)(sizeof(T) / 4); ++k) w[k] = shfl(w[k]);
  __builtin_memcpy(&v, w, sizeof(T));
  return v;
}
template <typename T>
__device__ __forceinline__ T shfl_xor_any(T v, int off) {
  return shfl_words(v, [off](uint32_t w) { return (uint32_t)__shfl_xor(w, off); });
}
template <typename T>
__device__ __forceinline__ T shfl_up_any(T v, int d) {
  return shfl_words(v, [d](uint32_t w) { return (uint32_t)__shfl_up(w, d); });
}

// ---- operators: the floating-point ones are fmaxf / fmax / fminf / fmin (a NaN loses to a number), the integer ones plain comparisons ------
struct SumOp {
  static constexpr bool kFromZero = true;
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct OrOp {
  static constexpr bool kFromZero = false;
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a | b; }
};
struct MaxOp {
  static constexpr bool kFromZero = false;
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b > a ? b : a; }
};
struct MinOp {
  static constexpr bool kFromZero = false;
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
  template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return b < a ? b : a; }
};

// ---- wave butterfly: every lane ends with the same bits ------------------------------------------------------------------------------------
template <typename T, typename Op>
__device__ __forceinline__ T wave_reduce_all(T v, Op op) {
  for (int off = 32; off > 0; off >>= 1) v = op(v, shfl_xor_any(v, off));
  return v;
}
template <typename T> __device__ __forceinline__ T wave_sum_all(T v) { return wave_reduce_all(v, SumOp()); }
template <typename T> __device__ __forceinline__ T wave_max_all(T v) { return wave_reduce_all(v, MaxOp()); }
template <typename T> __device__ __forceinline__ T wave_min_all(T v) { return wave_reduce_all(v, MinOp()); }

// ---- workgroup reduction: every thread returns the result; red holds WAVES entries (contract above) ----------------------------------------
template <int WAVES, typename T, typename Op>
__device__ __forceinline__ T block_reduce_all(T v, T* red, Op op) {
  v = wave_reduce_all(v, op);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[wave] = v;
  __syncthreads();
  T s = red[0];
  if constexpr (Op::kFromZero) s = op(T(0), s);
  for (int w = 1; w < WAVES; ++w) s = op(s, red[w]);
  return s;
}
template <int WAVES, typename T> __device__ __forceinline__ T block_sum_all(T v, T* red) { return block_reduce_all<WAVES>(v, red, SumOp()); }
template <int WAVES, typename T> __device__ __forceinline__ T block_max_all(T v, T* red) { return block_reduce_all<WAVES>(v, red, MaxOp()); }
template <int WAVES, typename T> __device__ __forceinline__ T block_min_all(T v, T* red) { return block_reduce_all<WAVES>(v, red, MinOp()); }

// ---- ordered compaction of one step (one element per thread): returns this thread's position among the step's kept elements, in thread
// order, and *total = how many the step kept (the same in every thread; the caller keeps the running base).  wave_count holds WAVES entries.
template <int WAVES>
__device__ __forceinline__ int block_compact(bool keep, int* wave_count, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long votes = __ballot(keep);
  __syncthreads();
  if (lane == 0) wave_count[wave] = __popcll(votes);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_count[w];
  int all = before;
  for (int w = wave; w < WAVES; ++w) all += wave_count[w];
  *total = all;
  return before + __popcll(votes & ((1ull << lane) - 1ull));
}

// ---- exclusive sum over the workgroup in thread order, and the workgroup's total (the same in every thread); wave_tot holds WAVES entries.
// The barrier contract of block_compact: one barrier before the entries are written, one before they are read, none after.
template <int WAVES>
__device__ __forceinline__ int block_exclusive_sum(int v, int* wave_tot, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int inc = v;
  for (int d = 1; d < 64; d <<= 1) {
    const int o = __shfl_up(inc, d);
    if (lane >= d) inc += o;
  }
  __syncthreads();
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wave; ++w) before += wave_tot[w];
  int all = before;
  for (int w = wave; w < WAVES; ++w) all += wave_tot[w];
  *total = all;
  return before + inc - v;
}

// ---- the object of a job: the largest o with job_off[o] <= job, job_off being the prefix array of the objects' job counts (n_obj + 1
// entries, job_off[0] = 0); at most 31 halvings of n_obj
__device__ __forceinline__ int object_of(const int32_t* __restrict__ job_off, int n_obj, int job) {
  int lo = 0, hi = n_obj;
  for (int s = 0; s < 31 && hi - lo > 1; ++s) {
    const int mid = (lo + hi) >> 1;
    if (job_off[mid] <= job) lo = mid; else hi = mid;
  }
  return lo;
}

}  // namespace mp
