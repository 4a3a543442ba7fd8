// TEST SUPPORT: host emulation of the VSD kernels (megapose6d_amd/csrc/vsd.hip) and of the projected symmetry-set error (MSPD,
// mspd_partial_kernel in pose_error.hip), built from the same arithmetic headers (vsd_core.h, pose_error_core.h).  Same arguments as the
// C ABI, on host arrays: one plain loop over pixels / points per row, no strips, no chunks, no ballots.  The counts are integers and a
// maximum has no order, so the kernels are held to these results bit for bit; only the mean form of the projected error accumulates in
// double here and is compared with a tolerance.  Built by tests/support/vsd.py with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <limits>

#include "pose_error_core.h"
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

extern "C" void mspd_emul(const float* T_pred, const float* T_gt, const float* syms, const int32_t* n_sym, int S_max, const float* points,
                          int n_pts_stride, const int32_t* mesh_ids, const int32_t* n_points, int n_pts, int b, int reduce_max, const float* K,
                          float* err, float* err_alt, int32_t* idx, float* T_gt_sym, float* errs) {
  const float inf = std::numeric_limits<float>::infinity();
  for (int row = 0; row < b; ++row) {
    const int mesh = mesh_ids[row];
    const int ns = syms ? (n_sym ? (n_sym[mesh] < S_max ? n_sym[mesh] : S_max) : S_max) : S_max;
    const int nv = n_points ? (n_points[mesh] < n_pts ? n_points[mesh] : n_pts) : n_pts;
    const float* Tp = T_pred + (size_t)row * 16;
    const float* P = points + (size_t)mesh * n_pts_stride * 3;
    bool ok = pe::pose_finite(Tp);
    if (syms) ok = ok && pe::pose_finite(T_gt + (size_t)row * 16);
    float Pp[12];
    pe::proj_matrix(K + (size_t)row * 9, Tp, Pp);
    float best = inf, best_alt = inf, Tw[16];
    int bi = -1;
    for (int s = 0; s < S_max; ++s) {
      float e = inf, e_alt = inf;
      if (s < ns) {
        float G[16], Pg[12];
        if (syms) {
          pe::compose(T_gt + (size_t)row * 16, syms + ((size_t)mesh * S_max + s) * 16, G);
        } else {
          for (int k = 0; k < 16; ++k) G[k] = T_gt[((size_t)row * S_max + s) * 16 + k];
        }
        pe::proj_matrix(K + (size_t)row * 9, G, Pg);
        const bool ok_s = ok && (syms || pe::pose_finite(G));
        double sum = 0.0;
        float mx = 0.f;
        for (int j = 0; j < nv; ++j) {
          const float n = pe::proj_dist(Pp, Pg, P[3 * j], P[3 * j + 1], P[3 * j + 2]);
          sum += (double)n;
          mx = fmaxf(mx, n);
        }
        const float mean = ok_s ? (float)(sum / (double)nv) : pe::quiet_nan();
        const float mxv = (ok_s && mean == mean) ? mx : pe::quiet_nan();
        e = reduce_max ? mxv : mean;
        e_alt = reduce_max ? mean : mxv;
        if (e < best) { best = e; bi = s; for (int k = 0; k < 16; ++k) Tw[k] = G[k]; }
        if (e_alt < best_alt) best_alt = e_alt;
      }
      if (errs) errs[(size_t)row * S_max + s] = e;
    }
    err[row] = bi >= 0 ? best : pe::quiet_nan();
    if (err_alt) err_alt[row] = (bi >= 0 && best_alt < inf) ? best_alt : pe::quiet_nan();
    idx[row] = bi;
    if (bi < 0) for (int k = 0; k < 16; ++k) Tw[k] = pe::quiet_nan();
    if (T_gt_sym) for (int k = 0; k < 16; ++k) T_gt_sym[(size_t)row * 16 + k] = Tw[k];
  }
}
