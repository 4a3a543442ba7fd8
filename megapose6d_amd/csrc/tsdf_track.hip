// tsdf_track.hip -- the device side of tracking the camera against the TSDF: the pose of an unposed depth frame by Gauss-Newton on the
// signed distances the volume holds at the frame's own back-projected pixels.
//
// The rules are tsdf_track_core.h, shared with the host emulation of the tests; the volume is tsdf_core.h's descriptor with const
// planes (tsdf::TrackVolume), and the entry's volume and frames are checked by tsdf_views.h's require_volume / require_views; this file
// adds the work distribution.  Every fp32 term of a pixel is produced by one lane from those rules, every fp64 sum has one owner and one
// order (lane, butterfly, waves, groups), so no grid can change a result.  No atomics, no workgroup waits on another, nothing is read back
// inside a call: 1 + 2 * iters launches.
//
//   tsdf_track_init_kernel        one lane per frame: the input pose copied to the output, status 0 or -2 [tsdf::load_view], used and rms 0.
//   tsdf_track_accumulate_kernel  grid (groups, n), one workgroup of 256 lanes per group of 1024 pixels of a frame.  It returns at once
//                                 for a frame whose status is not 0.  The frame's K and current pose are read through addresses that are
//                                 the same in every lane, so they sit in scalar registers.  Per used pixel 16 gathered words (eight
//                                 corners' sum and count); neighbouring pixels hit neighbouring cells.  29 fp64 sums per lane in registers
//                                 (passed and returned by value, as tsdf.hip's Node: an array handed down by pointer would live in
//                                 scratch); the wave butterfly, the four waves through LDS, and one record of 32 doubles per (frame, group)
//                                 written by 32 lanes with plain vector stores.
//   tsdf_track_solve_kernel       one wave per frame: lane k < 32 adds entry k of the frame's records in group order, lane 0 then solves
//                                 [tsdf::track_solve] and writes pose, status, used and rms.  It returns at once for a frame whose status is
//                                 not 0; a lost frame gets its input pose back.
#include "common.h"
#include "tsdf_track_core.h"
#include "tsdf_views.h"

namespace mp {

constexpr int kTrackWaves = tsdf::kTrackBlock / 64;
constexpr int kTrackSolveBlock = 64;

__global__ __launch_bounds__(64) void tsdf_track_init_kernel(const float* __restrict__ K, const float* __restrict__ TCO_in, int n,
                                                             float* __restrict__ TCO_out, int32_t* __restrict__ status,
                                                             int32_t* __restrict__ used, float* __restrict__ rms) {
  const int v = blockIdx.x * 64 + threadIdx.x;
  if (v >= n) return;
  float view[tsdf::kViewFloats];
  const bool ok = tsdf::load_view(K + (size_t)v * 9, TCO_in + (size_t)v * 16, view);
  for (int k = 0; k < 16; ++k) TCO_out[(size_t)v * 16 + k] = TCO_in[(size_t)v * 16 + k];
  status[v] = ok ? tsdf::kTrackRan : tsdf::kTrackBadView;
  used[v] = 0;
  rms[v] = 0.f;
}

__global__ __launch_bounds__(tsdf::kTrackBlock) void tsdf_track_accumulate_kernel(tsdf::TrackVolume vol, const float* __restrict__ depth,
                                                                                  const uint8_t* __restrict__ masks, const float* __restrict__ K,
                                                                                  const float* __restrict__ TCO, const int32_t* __restrict__ status,
                                                                                  int h, int w, float mu, int min_views, int groups,
                                                                                  double* __restrict__ partials) {
  __shared__ double red[kTrackWaves][tsdf::kTrackRecord];
  const int v = blockIdx.y, G = blockIdx.x;
  if (status[v] != tsdf::kTrackRan) return;   // the same in every lane of the workgroup
  float view[tsdf::kViewFloats];
  tsdf::load_view(K + (size_t)v * 9, TCO + (size_t)v * 16, view);
  const int hw = h * w;   // at most 2^26
  const float* __restrict__ d_frame = depth + (size_t)v * hw;
  const uint8_t* __restrict__ m_frame = masks ? masks + (size_t)v * hw : nullptr;
  tsdf::TrackSums acc = tsdf::track_zero();
#pragma unroll
  for (int q = 0; q < tsdf::kTrackPixelsPerLane; ++q) {
    const int pix = G * tsdf::kTrackGroupPixels + q * tsdf::kTrackBlock + (int)threadIdx.x;
    if (pix >= hw) continue;
    if (m_frame && m_frame[pix] == 0) continue;
    float row[tsdf::kTrackRowFloats];
    if (tsdf::track_row(pix % w, pix / w, d_frame[pix], view, vol, mu, min_views, row)) acc = tsdf::track_add(acc, row);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < tsdf::kTrackSums; ++k) {
    const double s = wave_sum_all(acc.s[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < tsdf::kTrackRecord) {
    double s = 0.0;
    if (threadIdx.x < tsdf::kTrackSums)
      for (int wv = 0; wv < kTrackWaves; ++wv) s = s + red[wv][threadIdx.x];
    partials[((size_t)v * groups + G) * tsdf::kTrackRecord + threadIdx.x] = s;
  }
}

__global__ __launch_bounds__(kTrackSolveBlock) void tsdf_track_solve_kernel(const double* __restrict__ partials, int groups,
                                                                            const float* __restrict__ TCO_in, int min_pixels, float eps_rot,
                                                                            float eps_trans, float* __restrict__ TCO_out,
                                                                            int32_t* __restrict__ status, int32_t* __restrict__ used,
                                                                            float* __restrict__ rms) {
  __shared__ double S[tsdf::kTrackRecord];
  const int v = blockIdx.x;
  if (status[v] != tsdf::kTrackRan) return;   // the same in every lane of the workgroup
  if (threadIdx.x < tsdf::kTrackRecord) {
    const double* __restrict__ rec = partials + (size_t)v * groups * tsdf::kTrackRecord + threadIdx.x;
    double s = 0.0;
    for (int G = 0; G < groups; ++G) s = s + rec[(size_t)G * tsdf::kTrackRecord];
    S[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  float T[12], out[12];
  for (int k = 0; k < 12; ++k) T[k] = TCO_out[(size_t)v * 16 + k];
  int32_t n_used;
  float r;
  const int st = tsdf::track_solve(S, T, min_pixels, eps_rot, eps_trans, out, &n_used, &r);
  if (st == tsdf::kTrackLost) {
    for (int k = 0; k < 16; ++k) TCO_out[(size_t)v * 16 + k] = TCO_in[(size_t)v * 16 + k];
  } else {
    for (int k = 0; k < 12; ++k) TCO_out[(size_t)v * 16 + k] = out[k];
  }
  status[v] = st;
  used[v] = n_used;
  rms[v] = r;
}

}  // namespace mp

using namespace mp;

extern "C" int mp_tsdf_track_groups(int h, int w) { return tsdf::track_groups(h, w); }

extern "C" int mp_tsdf_track(const void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel, const float* d_depth,
                             const uint8_t* d_masks, const float* d_K, const float* d_TCO_in, int n, int h, int w, float mu, int min_views,
                             int min_pixels, int iters, float eps_rot, float eps_trans, float* d_TCO_out, int32_t* d_status, int32_t* d_used,
                             float* d_rms, double* d_partials, long long partials_capacity, mp_stream stream) {
  const PosedViews vw = {d_depth, d_masks, nullptr, d_K, d_TCO_in, 16, n, h, w};   // poses of 16 floats, no colour frames
  if (int rc = require_volume("mp_tsdf_track", nx, ny, nz, ox, oy, oz, voxel)) return rc;
  MP_REQUIRE(tsdf::track_params_ok(mu, min_views, min_pixels, iters, eps_rot, eps_trans),
             "mp_tsdf_track: mu finite and > 0, min_views %d >= 1, min_pixels %d >= 1, iters %d in 1 .. %d, eps_rot and eps_trans finite and >= 0",
             min_views, min_pixels, iters, tsdf::kTrackMaxIters);
  const int rc = require_views("mp_tsdf_track", vw, false, tsdf::kTrackMaxFrames);
  if (rc != MP_OK || n == 0) return rc;
  const int groups = tsdf::track_groups(h, w);
  MP_REQUIRE(d_volume && d_TCO_out && d_status && d_used && d_rms && d_partials, "mp_tsdf_track: null pointer");
  MP_REQUIRE(d_TCO_in != d_TCO_out, "mp_tsdf_track: the output poses must not be the input poses (a lost frame returns its input)");
  MP_REQUIRE(partials_capacity >= (long long)n * groups, "mp_tsdf_track: partials of %lld records, %lld needed (%d frames of %d groups)",
             partials_capacity, (long long)n * groups, n, groups);
  MP_REQUIRE((uintptr_t)d_volume % 4 == 0 && (uintptr_t)d_partials % 8 == 0, "mp_tsdf_track: volume not 4-byte aligned or partials not 8-byte aligned");
  const tsdf::TrackVolume vol = tsdf::volume_of<const float, const int32_t>(d_volume, nx, ny, nz, color, ox, oy, oz, voxel);   // (the colour planes are not read)
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tsdf_track", 0.0, (double)iters * n * ((double)h * w * 69.0 + (double)groups * 512.0), s);
  hipLaunchKernelGGL(tsdf_track_init_kernel, dim3((unsigned)ceil_div(n, 64)), dim3(64), 0, s, d_K, d_TCO_in, n, d_TCO_out, d_status, d_used, d_rms);
  MP_CHECK_HIP(hipGetLastError());
  for (int it = 0; it < iters; ++it) {
    hipLaunchKernelGGL(tsdf_track_accumulate_kernel, dim3((unsigned)groups, (unsigned)n), dim3(tsdf::kTrackBlock), 0, s, vol, d_depth, d_masks, d_K,
                       (const float*)d_TCO_out, (const int32_t*)d_status, h, w, mu, min_views, groups, d_partials);
    MP_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(tsdf_track_solve_kernel, dim3((unsigned)n), dim3(kTrackSolveBlock), 0, s, (const double*)d_partials, groups, d_TCO_in, min_pixels,
                       eps_rot, eps_trans, d_TCO_out, d_status, d_used, d_rms);
    MP_CHECK_HIP(hipGetLastError());
  }
  return MP_OK;
}
