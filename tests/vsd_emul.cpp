// TEST SUPPORT: host emulation of the VSD kernels (megapose6d_amd/csrc/vsd.hip), built from the same arithmetic header (vsd_core.h).
// Same arguments as the C ABI, on host arrays: one plain loop over pixels per row, no strips, no chunks, no ballots.  The counts are
// integers, so the kernels are held to these results bit for bit.  Built by tests/support/vsd.py with -ffp-contract=off.
#include <cmath>
#include <cstdint>

#include "vsd_core.h"

using namespace mp;

extern "C" void vsd_emul(const float* depth_est, const int32_t* est_ids, const float* depth_gt, const int32_t* gt_ids, const float* depth_test,
                         const int32_t* im_ids, const float* K, const float* diameter, int b, int h, int w, float delta, const float* taus,
                         int n_tau, int normalized, float* errs, int32_t* counts) {
  const size_t hw = (size_t)h * w;
  for (int row = 0; row < b; ++row) {
    const float* Kr = K + (size_t)row * 9;
    int32_t* c = counts + (size_t)row * (2 + n_tau);
    if (!vsd::row_valid(Kr, diameter[row])) {
      for (int t = 0; t < n_tau; ++t) errs[(size_t)row * n_tau + t] = vsd::quiet_nan();
      for (int k = 0; k < 2 + n_tau; ++k) c[k] = -1;
      continue;
    }
    const float* E = depth_est + (size_t)(est_ids ? est_ids[row] : row) * hw;
    const float* G = depth_gt + (size_t)(gt_ids ? gt_ids[row] : row) * hw;
    const float* T = depth_test + (size_t)(im_ids ? im_ids[row] : row) * hw;
    for (int k = 0; k < 2 + n_tau; ++k) c[k] = 0;
    for (int y = 0; y < h; ++y) {
      const float v = vsd::ray_v(Kr, y);
      for (int x = 0; x < w; ++x) {
        const float u = vsd::ray_u(Kr, x);
        const float r = vsd::ray_factor(u * u, v * v);
        const vsd::Pixel p = vsd::classify(E[(size_t)y * w + x], G[(size_t)y * w + x], T[(size_t)y * w + x], r, delta);
        c[0] += (p.vis_gt || p.vis_est) ? 1 : 0;
        c[1] += (p.vis_gt && p.vis_est) ? 1 : 0;
        for (int t = 0; t < n_tau; ++t) c[2 + t] += vsd::is_far(p, vsd::threshold(taus[t], diameter[row], normalized)) ? 1 : 0;
      }
    }
    for (int t = 0; t < n_tau; ++t) errs[(size_t)row * n_tau + t] = vsd::error(c[0], c[1], c[2 + t]);
  }
}
