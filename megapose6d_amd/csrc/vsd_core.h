// vsd_core.h -- per-pixel arithmetic of the VSD kernels (vsd.hip), shared with the host emulation (tests/vsd_emul.cpp) the way
// pose_error_core.h is shared with tests/pose_error_emul.cpp.
//
// CONTRACT OF THE ARITHMETIC (BOP 2019 VSD: visibility mode "bop19", step cost; all fp32, compiled with -ffp-contract=off, every
// operation below a separate correctly rounded one, in the order written; lengths in metres)
//   * pixel (x, y) covers [x, x+1) x [y, y+1), its ray passes through the centre:
//       u = ((x + 0.5) - cx) / fx    v = ((y + 0.5) - cy) / fy    r = sqrtf((u*u + v*v) + 1)                    [ray_u, ray_v, ray_factor]
//   * dist = depth * r for the estimate's render, the ground truth's render and the observed frame; an observed depth that is not
//     finite or < 0 counts as 0                                                                                  [test_depth, Pixel]
//   * vis_gt  = dist_gt  > 0 and (dist_test == 0 or dist_gt  - dist_test <= delta)
//     vis_est = dist_est > 0 and (dist_test == 0 or dist_est - dist_test <= delta or vis_gt)                      [classify]
//     inter = vis_gt and vis_est, union = vis_gt or vis_est, far_t = inter and |dist_gt - dist_est| >= thr_t      [far_key, is_far]
//   * thr_t = tau_t * diameter (one product; tau_t itself when not normalised)                                    [threshold]
//   * err_t = (n_far_t + (n_union - n_inter)) / n_union as one division of two counts (each < 2^24: exact in fp32), 1.0 on an empty
//     union; a row whose K has a non-finite entry or whose diameter is not positive and finite: NaN and counts of -1   [row_valid, error]
// Everything but err_t is an integer count, so no grid or reduction order can change a result.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define VSD_HD __host__ __device__ __forceinline__
#else
#define VSD_HD static inline
#endif

namespace mp {
namespace vsd {

constexpr int kMaxTau = 16;
constexpr int kMaxSide = 1024;      // h, w <= 1024: every count <= 2^20

VSD_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

// K [3x3] row-major: fx = K[0], cx = K[2], fy = K[4], cy = K[5]
VSD_HD float ray_u(const float* K, int x) { return (((float)x + 0.5f) - K[2]) / K[0]; }
VSD_HD float ray_v(const float* K, int y) { return (((float)y + 0.5f) - K[5]) / K[4]; }
VSD_HD float ray_factor(float uu, float vv) { return sqrtf((uu + vv) + 1.0f); }

VSD_HD float test_depth(float d) { return (finite_f(d) && d >= 0.f) ? d : 0.f; }

VSD_HD bool row_valid(const float* K, float diameter) {
  bool ok = finite_f(diameter) && diameter > 0.f;
  for (int k = 0; k < 9; ++k) ok = ok && finite_f(K[k]);
  return ok;
}

VSD_HD float threshold(float tau, float diameter, int normalized) { return normalized ? tau * diameter : tau; }

struct Pixel {
  bool vis_gt, vis_est;
  float far_key;      // |dist_gt - dist_est|; it counts only on the intersection (is_far)
};

// r = ray_factor of the pixel; depths as stored (the observed one not yet sanitised)
VSD_HD Pixel classify(float depth_est, float depth_gt, float depth_test, float r, float delta) {
  const float de = depth_est * r, dg = depth_gt * r, dt = test_depth(depth_test) * r;
  Pixel p;
  p.vis_gt = dg > 0.f && (dt == 0.f || dg - dt <= delta);
  p.vis_est = de > 0.f && (dt == 0.f || de - dt <= delta || p.vis_gt);
  p.far_key = fabsf(dg - de);
  return p;
}

VSD_HD bool is_far(const Pixel& p, float thr) { return p.vis_gt && p.vis_est && p.far_key >= thr; }

VSD_HD float quiet_nan() { return nanf(""); }

VSD_HD float error(int32_t n_union, int32_t n_inter, int32_t n_far) {
  if (n_union == 0) return 1.0f;
  return (float)(n_far + (n_union - n_inter)) / (float)n_union;
}

}  // namespace vsd
}  // namespace mp
