// TEST SUPPORT: host emulation of the pose-error kernels (megapose6d_amd/csrc/pose_error.hip) built from the same per-element arithmetic
// (pose_error_core.h).  Same arguments as the C ABI, on host arrays; the reductions over points accumulate in double and round once
// (the kernels' own order is compared with a tolerance); a maximum has no order, so the max forms are held bit for bit.  Built by
// tests/support/pose_error.py with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "pose_error_core.h"

using namespace mp;

static inline int valid_points(const int32_t* n_points, int mesh, int n_pts) {
  return n_points ? (n_points[mesh] < n_pts ? n_points[mesh] : n_pts) : n_pts;
}

// the distance of one point under the prediction and under a candidate ground truth: in space (ADD, MSSD) or between projections (MSPD)
struct SpaceDist {
  const float* Tp;
  float G[16];
  SpaceDist(const float*, const float* T_pred) : Tp(T_pred) {}
  void candidate(const float* Gs) { for (int k = 0; k < 16; ++k) G[k] = Gs[k]; }
  float operator()(float x, float y, float z) const {
    float qx, qy, qz, gx, gy, gz;
    pe::apply(Tp, x, y, z, qx, qy, qz);
    pe::apply(G, x, y, z, gx, gy, gz);
    return sqrtf(pe::norm2(gx - qx, gy - qy, gz - qz));
  }
};
struct PixelDist {
  const float* K;
  float Pp[12], Pg[12];
  PixelDist(const float* K_row, const float* T_pred) : K(K_row) { pe::proj_matrix(K, T_pred, Pp); }
  void candidate(const float* Gs) { pe::proj_matrix(K, Gs, Pg); }
  float operator()(float x, float y, float z) const { return pe::proj_dist(Pp, Pg, x, y, z); }
};

// one row loop for both: the symmetry set, the mean (accumulated in double) and the maximum over the points, the arg-min
template <class Dist>
static void sym_rows(const float* T_pred, const float* T_gt, const float* syms, const int32_t* n_sym, int S_max, const float* points,
                     int n_pts_stride, const int32_t* mesh_ids, const int32_t* n_points, int n_pts, int b, int reduce_max, const float* K,
                     float* err, float* err_alt, int32_t* idx, float* T_gt_sym, float* errs, float* diffs) {
  const float inf = std::numeric_limits<float>::infinity();
  for (int row = 0; row < b; ++row) {
    const int mesh = mesh_ids[row];
    const int ns = syms ? (n_sym ? (n_sym[mesh] < S_max ? n_sym[mesh] : S_max) : S_max) : S_max;
    const int nv = valid_points(n_points, mesh, n_pts);
    const float* Tp = T_pred + (size_t)row * 16;
    const float* P = points + (size_t)mesh * n_pts_stride * 3;
    bool ok = pe::pose_finite(Tp);
    if (syms) ok = ok && pe::pose_finite(T_gt + (size_t)row * 16);
    Dist dist(K ? K + (size_t)row * 9 : nullptr, Tp);
    float best = inf, best_alt = inf;
    int bi = -1;
    float Tw[16];
    for (int s = 0; s < S_max; ++s) {
      float e = inf, e_alt = inf;
      if (s < ns) {
        float G[16];
        if (syms) {
          pe::compose(T_gt + (size_t)row * 16, syms + ((size_t)mesh * S_max + s) * 16, G);
        } else {
          for (int k = 0; k < 16; ++k) G[k] = T_gt[((size_t)row * S_max + s) * 16 + k];
        }
        dist.candidate(G);
        const bool ok_s = ok && (syms || pe::pose_finite(G));
        double sum = 0.0;
        float mx = 0.f;
        for (int j = 0; j < nv; ++j) {
          const float n = dist(P[3 * j], P[3 * j + 1], P[3 * j + 2]);
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
    if (diffs) {
      float* D = diffs + (size_t)row * n_pts * 3;
      for (int j = 0; j < n_pts; ++j) {
        float dx = 0.f, dy = 0.f, dz = 0.f;
        if (j < nv) {
          float qx, qy, qz, gx, gy, gz;
          pe::apply(Tp, P[3 * j], P[3 * j + 1], P[3 * j + 2], qx, qy, qz);
          pe::apply(Tw, P[3 * j], P[3 * j + 1], P[3 * j + 2], gx, gy, gz);
          dx = gx - qx; dy = gy - qy; dz = gz - qz;
        }
        D[3 * j] = dx; D[3 * j + 1] = dy; D[3 * j + 2] = dz;
      }
    }
  }
}

extern "C" void pose_error_emul_sym(const float* T_pred, const float* T_gt, const float* syms, const int32_t* n_sym, int S_max,
                                    const float* points, int n_pts_stride, const int32_t* mesh_ids, const int32_t* n_points, int n_pts, int b,
                                    int reduce_max, float* err, float* err_alt, int32_t* idx, float* T_gt_sym, float* errs, float* diffs) {
  sym_rows<SpaceDist>(T_pred, T_gt, syms, n_sym, S_max, points, n_pts_stride, mesh_ids, n_points, n_pts, b, reduce_max, nullptr, err, err_alt,
                      idx, T_gt_sym, errs, diffs);
}

// the projected form (MSPD; mp_pose_error_mspd): no difference vectors
extern "C" void mspd_emul(const float* T_pred, const float* T_gt, const float* syms, const int32_t* n_sym, int S_max, const float* points,
                          int n_pts_stride, const int32_t* mesh_ids, const int32_t* n_points, int n_pts, int b, int reduce_max, const float* K,
                          float* err, float* err_alt, int32_t* idx, float* T_gt_sym, float* errs) {
  sym_rows<PixelDist>(T_pred, T_gt, syms, n_sym, S_max, points, n_pts_stride, mesh_ids, n_points, n_pts, b, reduce_max, K, err, err_alt, idx,
                      T_gt_sym, errs, nullptr);
}

extern "C" void pose_error_emul_nn(const float* T_pred, const float* T_gt, const float* points, int n_pts_stride, const int32_t* mesh_ids,
                                   const int32_t* n_points, int n_pts, int b, float* diffs, int32_t* assign, float* mean_out, float* max_out) {
  std::vector<float> q;
  for (int row = 0; row < b; ++row) {
    const int mesh = mesh_ids[row];
    const int nv = valid_points(n_points, mesh, n_pts);
    const float* Tp = T_pred + (size_t)row * 16;
    const float* Tg = T_gt + (size_t)row * 16;
    const float* P = points + (size_t)mesh * n_pts_stride * 3;
    const bool ok = pe::pose_finite(Tp) && pe::pose_finite(Tg);
    q.resize((size_t)nv * 3);
    for (int k = 0; k < nv; ++k) pe::apply(Tp, P[3 * k], P[3 * k + 1], P[3 * k + 2], q[3 * k], q[3 * k + 1], q[3 * k + 2]);
    double sum = 0.0;
    float mx = 0.f;
    for (int j = 0; j < n_pts; ++j) {
      float dx = 0.f, dy = 0.f, dz = 0.f;
      int bk = -1;
      if (j < nv) {
        float gx, gy, gz;
        pe::apply(Tg, P[3 * j], P[3 * j + 1], P[3 * j + 2], gx, gy, gz);
        uint64_t key = ~(uint64_t)0;
        float best = std::numeric_limits<float>::infinity();
        for (int k = 0; k < nv; ++k) {
          const float d2 = pe::norm2(gx - q[3 * k], gy - q[3 * k + 1], gz - q[3 * k + 2]);
          if (d2 < best) { best = d2; bk = k; }
        }
        key = pe::nn_key(best, bk);
        bk = (int)(uint32_t)(key & 0xffffffffull);
        if (!ok || bk < 0 || bk >= nv) {
          bk = -1;
          dx = dy = dz = pe::quiet_nan();
        } else {
          dx = gx - q[3 * bk]; dy = gy - q[3 * bk + 1]; dz = gz - q[3 * bk + 2];
        }
        const float n = sqrtf(pe::norm2(dx, dy, dz));
        sum += (double)n;
        mx = fmaxf(mx, n);
      }
      if (diffs) { float* D = diffs + ((size_t)row * n_pts + j) * 3; D[0] = dx; D[1] = dy; D[2] = dz; }
      if (assign) assign[(size_t)row * n_pts + j] = bk;
    }
    const float mean = (float)(sum / (double)nv);
    mean_out[row] = mean;
    max_out[row] = mean == mean ? mx : pe::quiet_nan();
  }
}

extern "C" void pose_error_emul_rigid(const float* T_a, const float* T_b, int b, const float* K, const float* points, int n_pts_stride,
                                      const int32_t* mesh_ids, const int32_t* n_points, int n_pts, float* trans, float* rot, float* proj) {
  for (int row = 0; row < b; ++row) {
    const float* Ta = T_a + (size_t)row * 16;
    const float* Tb = T_b + (size_t)row * 16;
    pe::rigid(Ta, Tb, trans[row], rot[row]);
    if (!proj) continue;
    const int mesh = mesh_ids[row];
    const int nv = valid_points(n_points, mesh, n_pts);
    const float* P = points + (size_t)mesh * n_pts_stride * 3;
    float Pa[12], Pb[12];
    pe::proj_matrix(K + (size_t)row * 9, Ta, Pa);
    pe::proj_matrix(K + (size_t)row * 9, Tb, Pb);
    double sum = 0.0;
    for (int j = 0; j < nv; ++j) sum += (double)pe::proj_dist(Pa, Pb, P[3 * j], P[3 * j + 1], P[3 * j + 2]);
    const bool ok = pe::pose_finite(Ta) && pe::pose_finite(Tb);
    proj[row] = ok ? (float)(sum / (double)nv) : pe::quiet_nan();
  }
}
