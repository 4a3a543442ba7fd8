// vsd.hip -- BOP's Visible Surface Discrepancy between rendered depth maps and an observed frame, as counts per row.
//
// The definition (BOP 2019: visibility "bop19", step cost) and its fp32 arithmetic are vsd_core.h, shared with the host emulation of
// the tests; this file adds the work distribution.  Every per-row result but the final division is an integer count, so neither the
// grid nor the order in which workgroups arrive can change a bit.
//
//   vsd_count_kernel     grid (row, strip of image rows), 4 waves, the walk of depth_walk.h (shared with gt_info.hip): strips, the v*v
//                        table, the u*u registers, the four-pixel loads (16-byte when the width and the bases allow, else guarded
//                        scalar loads with the same counts).  A chunk in which neither render has a positive depth is skipped (it
//                        cannot be visible).  The 2 + n_tau predicates are reduced per wave by ballot + population count, per
//                        workgroup through LDS, then one integer atomicAdd per counter.
//   vsd_finalize_kernel  one thread per row: counts -> errs (NaN / -1 for an invalid row)
#include "common.h"
#include "depth_walk.h"
#include "vsd_core.h"

namespace mp {

using vsd::kMaxSide;
using vsd::kMaxTau;

struct VsdTaus { float v[kMaxTau]; };

template <int NT, bool VEC>
__global__ __launch_bounds__(256) void vsd_count_kernel(const float* __restrict__ depth_est, const int32_t* __restrict__ est_ids,
                                                        const float* __restrict__ depth_gt, const int32_t* __restrict__ gt_ids,
                                                        const float* __restrict__ depth_test, const int32_t* __restrict__ im_ids,
                                                        const float* __restrict__ K, const float* __restrict__ diameter, int h, int w,
                                                        int rows_per_strip, float delta, VsdTaus taus, int n_tau, int normalized,
                                                        int32_t* __restrict__ counters) {
  __shared__ float vv_s[kMaxSide];
  __shared__ int32_t red[4][2 + NT];
  const int row = blockIdx.x;
  float Kr[9];
  for (int k = 0; k < 9; ++k) Kr[k] = K[(size_t)row * 9 + k];
  const float diam = diameter[row];
  if (!vsd::row_valid(Kr, diam)) return;   // uniform over the workgroup; the finalize kernel writes NaN / -1
  const int y0 = blockIdx.y * rows_per_strip, y1 = min(h, y0 + rows_per_strip);
  dw::fill_vv(Kr, y0, y1, vv_s);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float thr[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) thr[t] = t < n_tau ? vsd::threshold(taus.v[t], diam, normalized) : vsd::quiet_nan();   // NaN: never far
  float uu[dw::kChunks][4];
  dw::fill_uu(Kr, lane, uu);
  const size_t hw = (size_t)h * w;
  const float* E = depth_est + (size_t)(est_ids ? est_ids[row] : row) * hw;
  const float* G = depth_gt + (size_t)(gt_ids ? gt_ids[row] : row) * hw;
  const float* T = depth_test + (size_t)(im_ids ? im_ids[row] : row) * hw;
  int n_union = 0, n_inter = 0, n_far[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) n_far[t] = 0;
  for (int y = y0 + wave; y < y1; y += 4) {
    const float vv = vv_s[y - y0];
    const size_t off = (size_t)y * w;
#pragma unroll
    for (int c = 0; c < dw::kChunks; ++c) {
      if (c * 256 >= w) break;   // uniform
      const int x0 = c * 256 + lane * 4;
      float e[4], g[4], t[4];
      dw::load4<VEC>(E, off, x0, w, e);
      dw::load4<VEC>(G, off, x0, w, g);
      dw::load4<VEC>(T, off, x0, w, t);
      // a depth that is not > 0 gives a distance that is not > 0: such a pixel is in neither mask
      const bool any = e[0] > 0.f || e[1] > 0.f || e[2] > 0.f || e[3] > 0.f || g[0] > 0.f || g[1] > 0.f || g[2] > 0.f || g[3] > 0.f;
      if (__ballot(any) == 0) continue;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float r = vsd::ray_factor(uu[c][k], vv);
        const vsd::Pixel p = vsd::classify(e[k], g[k], t[k], r, delta);
        const bool in = p.vis_gt && p.vis_est;
        n_union += __popcll(__ballot(p.vis_gt || p.vis_est));
        n_inter += __popcll(__ballot(in));
        const float key = in ? p.far_key : vsd::quiet_nan();   // key >= thr is vsd::is_far
#pragma unroll
        for (int q = 0; q < NT; ++q) n_far[q] += __popcll(__ballot(key >= thr[q]));
      }
    }
  }
  if (lane == 0) {
    red[wave][0] = n_union;
    red[wave][1] = n_inter;
#pragma unroll
    for (int q = 0; q < NT; ++q) red[wave][2 + q] = n_far[q];
  }
  __syncthreads();
  if ((int)threadIdx.x < 2 + n_tau) {
    const int32_t s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (s != 0) atomicAdd(counters + (size_t)row * (2 + n_tau) + threadIdx.x, s);
  }
}

__global__ __launch_bounds__(256) void vsd_finalize_kernel(const float* __restrict__ K, const float* __restrict__ diameter, int b, int n_tau,
                                                           const int32_t* __restrict__ counters, float* __restrict__ errs,
                                                           int32_t* __restrict__ counts) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= b) return;
  const bool ok = vsd::row_valid(K + (size_t)row * 9, diameter[row]);
  const int32_t* c = counters + (size_t)row * (2 + n_tau);
  for (int t = 0; t < n_tau; ++t) errs[(size_t)row * n_tau + t] = ok ? vsd::error(c[0], c[1], c[2 + t]) : vsd::quiet_nan();
  if (counts)
    for (int k = 0; k < 2 + n_tau; ++k) counts[(size_t)row * (2 + n_tau) + k] = ok ? c[k] : -1;
}

template <int NT>
static void vsd_launch(bool vec, dim3 grid, hipStream_t s, const float* e, const int32_t* ei, const float* g, const int32_t* gi, const float* t,
                       const int32_t* ti, const float* K, const float* diam, int h, int w, int rps, float delta, const VsdTaus& taus, int n_tau,
                       int normalized, int32_t* counters) {
  if (vec)
    hipLaunchKernelGGL((vsd_count_kernel<NT, true>), grid, dim3(256), 0, s, e, ei, g, gi, t, ti, K, diam, h, w, rps, delta, taus, n_tau, normalized,
                       counters);
  else
    hipLaunchKernelGGL((vsd_count_kernel<NT, false>), grid, dim3(256), 0, s, e, ei, g, gi, t, ti, K, diam, h, w, rps, delta, taus, n_tau, normalized,
                       counters);
}

}  // namespace mp

using namespace mp;

extern "C" size_t mp_vsd_workspace_bytes(int b, int n_tau) {
  if (b < 0 || n_tau < 1 || n_tau > kMaxTau) return 0;
  return align256((size_t)b * (2 + n_tau) * sizeof(int32_t)) + 256;
}

extern "C" int mp_vsd(const float* d_depth_est, const int32_t* d_est_ids, const float* d_depth_gt, const int32_t* d_gt_ids,
                      const float* d_depth_test, const int32_t* d_im_ids, int n_est, int n_gt, int n_im, const float* d_K, const float* d_diameter,
                      int b, int h, int w, float delta, const float* h_taus, int n_tau, int normalized, int split, float* d_errs,
                      int32_t* d_counts, void* d_workspace, size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(b >= 0, "mp_vsd: b %d < 0", b);
  MP_REQUIRE(h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide, "mp_vsd: map %d x %d outside [1, %d]", h, w, kMaxSide);
  MP_REQUIRE(n_tau >= 1 && n_tau <= kMaxTau, "mp_vsd: n_tau %d outside [1, %d]", n_tau, kMaxTau);
  MP_REQUIRE(h_taus, "mp_vsd: null taus");
  MP_REQUIRE(split >= 0, "mp_vsd: split < 0");
  MP_REQUIRE(n_est >= 0 && n_gt >= 0 && n_im >= 0, "mp_vsd: negative map count");
  if (b == 0) return MP_OK;
  MP_REQUIRE(d_depth_est && d_depth_gt && d_depth_test && d_K && d_diameter && d_errs && d_workspace, "mp_vsd: null pointer");
  MP_REQUIRE(n_est >= 1 && n_gt >= 1 && n_im >= 1, "mp_vsd: no depth maps");
  // without ids the maps are row-aligned: there must be one per row
  MP_REQUIRE((d_est_ids || n_est >= b) && (d_gt_ids || n_gt >= b) && (d_im_ids || n_im >= b), "mp_vsd: fewer maps than rows and no ids");
  MP_REQUIRE(workspace_bytes >= mp_vsd_workspace_bytes(b, n_tau), "mp_vsd: workspace too small");
  const dw::Strips st = dw::strips_of(split, 4096, b, h);   // a few thousand workgroups when the rows alone cannot give them
  VsdTaus taus;
  for (int t = 0; t < kMaxTau; ++t) taus.v[t] = t < n_tau ? h_taus[t] : 0.f;
  const bool vec = dw::vec_ok(w, {d_depth_est, d_depth_gt, d_depth_test});
  int32_t* counters = (int32_t*)d_workspace;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("vsd", 0.0, (double)b * h * w * 12.0, s);
  MP_CHECK_HIP(hipMemsetAsync(counters, 0, (size_t)b * (2 + n_tau) * sizeof(int32_t), s));
  const dim3 grid(b, st.strips);
#define MP_VSD_ARGS vec, grid, s, d_depth_est, d_est_ids, d_depth_gt, d_gt_ids, d_depth_test, d_im_ids, d_K, d_diameter, h, w, st.rows_per_strip, delta, taus, n_tau, \
                    normalized ? 1 : 0, counters
  if (n_tau <= 1) vsd_launch<1>(MP_VSD_ARGS);
  else if (n_tau <= 4) vsd_launch<4>(MP_VSD_ARGS);
  else if (n_tau <= 10) vsd_launch<10>(MP_VSD_ARGS);
  else vsd_launch<16>(MP_VSD_ARGS);
#undef MP_VSD_ARGS
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(vsd_finalize_kernel, dim3(ceil_div(b, 256)), dim3(256), 0, s, d_K, d_diameter, b, n_tau, counters, d_errs, d_counts);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
