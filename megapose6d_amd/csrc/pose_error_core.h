// pose_error_core.h -- per-element arithmetic of the pose-error kernels (pose_error.hip), shared with the host emulation
// (tests/pose_error_emul.cpp) the way raster_scene_core.h is shared with tests/raster_scene_emul.cpp.
//
// CONTRACT OF THE ARITHMETIC (all fp32, compiled with -ffp-contract=off: every fused operation below is an explicit fmaf)
//   * point transform q = R p + t: each coordinate fmaf(r2, z, fmaf(r1, y, fmaf(r0, x, t)))                          [apply]
//   * a symmetric ground-truth pose is composed FIRST, T_gt_s = T_gt * Sym_s: entry (r, c) = fmaf(g2, s2c, fmaf(g1, s1c, g0 * s0c)) for
//     c < 3 and fmaf(g2, s23, fmaf(g1, s13, fmaf(g0, s03, g3))) for the translation column; last row 0 0 0 1          [compose]
//     -- then applied as above (affine maps are never subtracted before they are applied: the cancellation would change with |t|)
//   * difference d = q_gt - q_pred (the reference's sign), squared norm fmaf(dz, dz, fmaf(dy, dy, dx * dx)), norm sqrtf   [norm2]
//   * arg-min: ascending scan with a strict <, so the lowest index wins an exact tie (symmetry index, neighbour index); a pose with a
//     non-finite entry gives NaN errors and index -1 (NaN never compares <), never a fault                       [pose_finite, nn_key]
//   * reductions over points (mean, max) are deterministic -- the same bits on every launch, whatever the grid -- but their ORDER is
//     the kernel's own: 4 terms per lane, a 64-lane butterfly per 256-point chunk, a lane-strided sum + butterfly over the chunks
//     (<= ~20 roundings for any point count); the emulation accumulates in double and rounds once.  They are compared with a tolerance.
//   * rotation error = angle of dR = R_b R_a^T as atan2f(|(dR - dR^T)^v| / 2, (tr dR - 1) / 2) * (180 / pi)             [rigid]
//   * projection: P = K T[:3] (fmaf chain over k = 0..2), suv = P (x y z 1) as `apply`, (u, v) = (su / sw, sv / sw)    [proj_matrix, project]
//     and the distance of two projections sqrtf(fmaf(dv, dv, du * du)): its mean over the points is proj_error, its maximum over the
//     points, minimised over the symmetry set as in `arg-min` above, is MSPD                                     [pixel_dist, proj_dist]
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define PE_HD __host__ __device__ __forceinline__
#else
#define PE_HD static inline
#endif

namespace mp {
namespace pe {

constexpr int kChunk = 256;        // points per reduction chunk: one wave, 4 points per lane (point c*256 + p*64 + lane)
constexpr int kPerLane = 4;
constexpr int kMaxSym = 512;       // symmetry poses of a row kept in LDS (12 floats each)

// T: 4x4 row-major, rows 0..2 are read
PE_HD void apply(const float* T, float x, float y, float z, float& qx, float& qy, float& qz) {
  qx = fmaf(T[2], z, fmaf(T[1], y, fmaf(T[0], x, T[3])));
  qy = fmaf(T[6], z, fmaf(T[5], y, fmaf(T[4], x, T[7])));
  qz = fmaf(T[10], z, fmaf(T[9], y, fmaf(T[8], x, T[11])));
}

// O = G * S (rigid 4x4, row-major); O may not alias G or S
PE_HD void compose(const float* G, const float* S, float* O) {
  for (int r = 0; r < 3; ++r) {
    const float g0 = G[4 * r], g1 = G[4 * r + 1], g2 = G[4 * r + 2], g3 = G[4 * r + 3];
    for (int c = 0; c < 3; ++c) O[4 * r + c] = fmaf(g2, S[8 + c], fmaf(g1, S[4 + c], g0 * S[c]));
    O[4 * r + 3] = fmaf(g2, S[11], fmaf(g1, S[7], fmaf(g0, S[3], g3)));
  }
  O[12] = 0.f; O[13] = 0.f; O[14] = 0.f; O[15] = 1.f;
}

PE_HD float norm2(float dx, float dy, float dz) { return fmaf(dz, dz, fmaf(dy, dy, dx * dx)); }

PE_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

PE_HD bool pose_finite(const float* T) {
  bool ok = true;
  for (int k = 0; k < 12; ++k) ok = ok && finite_f(T[k]);
  return ok;
}

PE_HD float quiet_nan() { return nanf(""); }

// key of the nearest-neighbour merge: the bits of a non-negative float order as an unsigned integer, low word = neighbour index, so
// the minimum over any partition of the neighbours is the contract's winner (lowest index among equal distances)
PE_HD uint64_t nn_key(float d2, int k) {
  uint32_t u;
  memcpy(&u, &d2, 4);
  return ((uint64_t)u << 32) | (uint32_t)k;
}

// trans = |t_a - t_b|, rot_deg = angle of R_b R_a^T
PE_HD void rigid(const float* Ta, const float* Tb, float& trans, float& rot_deg) {
  if (!pose_finite(Ta) || !pose_finite(Tb)) {
    trans = quiet_nan();
    rot_deg = quiet_nan();
    return;
  }
  trans = sqrtf(norm2(Ta[3] - Tb[3], Ta[7] - Tb[7], Ta[11] - Tb[11]));
  float d[9];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) d[3 * i + j] = fmaf(Tb[4 * i + 2], Ta[4 * j + 2], fmaf(Tb[4 * i + 1], Ta[4 * j + 1], Tb[4 * i] * Ta[4 * j]));
  const float s = sqrtf(norm2(d[7] - d[5], d[2] - d[6], d[3] - d[1])) * 0.5f;
  const float c = (((d[0] + d[4]) + d[8]) - 1.0f) * 0.5f;
  rot_deg = atan2f(s, c) * 57.29577951308232f;
}

// P [3x4] = K [3x3] * T[:3]
PE_HD void proj_matrix(const float* K, const float* T, float* P) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 4; ++j) P[4 * i + j] = fmaf(K[3 * i + 2], T[8 + j], fmaf(K[3 * i + 1], T[4 + j], K[3 * i] * T[j]));
}

PE_HD void project(const float* P, float x, float y, float z, float& u, float& v) {
  float su, sv, sw;
  apply(P, x, y, z, su, sv, sw);
  u = su / sw;
  v = sv / sw;
}

// distance between two pixel positions
PE_HD float pixel_dist(float ua, float va, float ub, float vb) {
  const float du = ua - ub, dv = va - vb;
  return sqrtf(fmaf(dv, dv, du * du));
}

// 2D distance between the projections of one point under two projection matrices (the mean of it is proj_error, the maximum MSPD)
PE_HD float proj_dist(const float* Pa, const float* Pb, float x, float y, float z) {
  float ua, va, ub, vb;
  project(Pa, x, y, z, ua, va);
  project(Pb, x, y, z, ub, vb);
  return pixel_dist(ua, va, ub, vb);
}

}  // namespace pe
}  // namespace mp
