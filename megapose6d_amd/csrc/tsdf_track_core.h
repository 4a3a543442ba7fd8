// tsdf_track_core.h -- the rules of tracking the camera against the TSDF: the pose of an unposed depth frame found by aligning the
// frame's own back-projected pixels directly to the signed distance field the volume holds (Gauss-Newton on sum f(T^-1 pc)^2, "direct SDF
// alignment"), as it runs on the device (tsdf_track.hip), shared with the host emulation (tests/tsdf_track_emul.cpp) the way tsdf_core.h
// is shared with tests/tsdf_emul.cpp.  No raycast, no vertex or normal maps, no projective association: one gather per pixel.
//
// CONTRACT (compiled with -ffp-contract=off; every fp32 and every fp64 operation a separate correctly rounded one in the order written;
// fp64 uses only + - * / and sqrt, no sin / cos / exp, so the device and the host agree bit for bit; lengths in metres; the volume, a
// view's K and TCO and the pixel convention are tsdf_core.h's)
//   * PER PIXEL (x, y) of a frame, pixel index y * w + x [track_row], all fp32.  (R, t) is the CURRENT TCO, object to camera.
//       1. Skip unless the mask (when given) is non-zero and the depth d is finite and > 0.
//       2. pc = ((((float)x + 0.5) - cx) / fx) * d, likewise y, and d: the pixel's centre, as onboarding.volume_for_views takes it.
//       3. e = pc - t per component; p = R^T e, p[c] = (R[0][c] * e0 + R[1][c] * e1) + R[2][c] * e2: the point in the object's frame.
//       4. q[c] = (p[c] - origin[c]) / voxel, i0[c] = floorf(q[c]), u[c] = q[c] - i0[c].  Skip unless 0 <= i0[c] < dims[c] - 1 on every
//          axis (tested on the floats: a NaN or an overflow skips).
//       5. The eight corners i0 + {0,1}^3, corner code = dx + 2 dy + 4 dz: skip unless every count >= min_views.  F[code] =
//          field(sum, count) = sum / (float)count.  (16 gathered words.)
//       6. Trilinear, x then y then z, each step lerp(a, b, t) = a + t * (b - a):  c00 = lerp(F0, F1, ux), c10 = lerp(F2, F3, ux),
//          c01 = lerp(F4, F5, ux), c11 = lerp(F6, F7, ux); c0 = lerp(c00, c10, uy), c1 = lerp(c01, c11, uy); f = lerp(c0, c1, uz).
//          Skip unless fabsf(f) < 1 (beyond the truncation band the field is flat; a NaN skips).
//       7. The analytic gradient of that form per voxel:  dx = lerp(lerp(F1 - F0, F3 - F2, uy), lerp(F5 - F4, F7 - F6, uy), uz),
//          dy = lerp(c10 - c00, c11 - c01, uz), dz = c1 - c0;  g[c] = d[c] / voxel (per metre).
//       8. Residual r = f * mu (metres).  gm[c] = g[c] * mu.  Jacobian row J = [p x gm, gm] for the increment p <- p + w x p + v in the
//          object's frame: J0 = p1 * gm2 - p2 * gm1, J1 = p2 * gm0 - p0 * gm2, J2 = p0 * gm1 - p1 * gm0, J3..5 = gm.
//   * SUMS, fp64 [track_add].  J and r are widened to double, so every product is exact.  A used pixel's record is kTrackSums = 29
//     doubles: the 21 entries J_i * J_j, i <= j, of the upper triangle of J^T J row by row (00 01 .. 05 11 12 .. 55), the 6 entries
//     J_i * r, then r * r, then 1.  A skipped pixel adds nothing.  Ownership is fixed, so no grid changes a bit: group G of
//     kTrackGroupPixels = 1024 consecutive pixels belongs to one workgroup of kTrackBlock = 256 lanes; lane t adds, from 0, the pixels
//     1024 G + t, + 256, + 512, + 768 in that order (those below h * w); the 64 lanes of a wave add in the butterfly of block_primitives.h
//     (xor 32, 16, .. 1: s = s + other lane's s); the four waves add in ascending order from 0 ((((0 + w0) + w1) + w2) + w3); that is the
//     group's RECORD of kTrackRecord = 32 doubles (29 + 3 zeros).  The groups add in ascending order from 0 in the solve.  (The scheme
//     teaser_core.h states for its float64 sums.)
//   * SOLVE, fp64, per frame and iteration [track_solve].  S = the summed record.
//       1. used = (int)S[28]; rms = (float)sqrt(S[27] / S[28]), 0 when used = 0.  used < min_pixels -> LOST.
//       2. A = the symmetric 6 x 6 of S[0..20], with 1e-9 * S[28] added to the diagonal (the damping of icp_solve); b = S[21..26].
//          Cholesky A = L L^T, column by column: d = A[j][j] - L[j][0]^2 - .. - L[j][j-1]^2 (subtracted in that order); d not > 0 ->
//          LOST; L[j][j] = sqrt(d); L[i][j] = (A[i][j] - L[i][0] L[j][0] - .. - L[i][j-1] L[j][j-1]) / L[j][j] for i > j.
//          Forward: y[i] = (b[i] - L[i][0] y[0] - .. - L[i][i-1] y[i-1]) / L[i][i]; back: z[i] = (y[i] - L[i+1][i] z[i+1] - .. -
//          L[5][i] z[5]) / L[i][i], i = 5 .. 0.  x = -z; w = x[0..2] (rad), v = x[3..5] (metres).
//       3. The rotation of w by the CAYLEY MAP, a = w * 0.5, aa = (a0 a0 + a1 a1) + a2 a2, s = 1 + aa, c = 1 - aa:  Rc[i][i] = (c + 2 * (a_i *
//          a_i)) / s, Rc[i][j] = (2 * (a_i * a_j) + 2 * K[i][j]) / s with K = [a]x = ((0, -a2, a1), (a2, 0, -a0), (-a1, a0, 0)): rational, and
//          exactly orthogonal in exact arithmetic.
//       4. TCO <- TCO * D^-1 with D = [Rc | v], D^-1 = [Rc^T | -Rc^T v]:  Rn[i][j] = (R[i][0] Rc[j][0] + R[i][1] Rc[j][1]) + R[i][2]
//          Rc[j][2];  m[k] = (Rc[0][k] v0 + Rc[1][k] v1) + Rc[2][k] v2;  tn[i] = t[i] - ((R[i][0] m0 + R[i][1] m1) + R[i][2] m2), R and t
//          the fp32 pose widened.
//       5. Gram-Schmidt on the rows of Rn: r0 = row0 / |row0|; e = row1 - (row1 . r0) r0, r1 = e / |e|; r2 = r0 x r1 (|a| = sqrt((a0 a0 +
//          a1 a1) + a2 a2), a . b likewise).  The nine entries and tn are rounded to fp32: the pose the next iteration reads.
//          Any non-finite entry -> LOST.
//       6. CONVERGED when sqrt((w0 w0 + w1 w1) + w2 w2) < eps_rot and the same of v < eps_trans; the pose of step 5 is still written.
//   * STATUS per frame: 0 ran all iterations, 1 converged (later iterations skip it), -1 lost, -2 the frame's K or the first 12
//     entries of its pose hold a non-finite value.  A frame of status 0 or 1 returns the tracked pose (the input's last row copied); a
//     frame of status -1 or -2 returns its INPUT pose bit for bit.  `used` and `rms` are those of the last iteration that ran for the
//     frame (the sums at the pose that iteration started from); 0 and 0 for status -2.
//   * Frames are independent: n frames in one call equal n calls of one.
//
// LIMITS.  The volume's and the frame's of tsdf_core.h (dims 2 .. 512 a side, at most 2^27 nodes, 1 <= h, w <= 8192; origin finite,
// voxel and mu finite and > 0); 1 <= iters <= kTrackMaxIters = 64; 1 <= min_views; 1 <= min_pixels; eps_rot, eps_trans finite and >= 0;
// 0 <= n <= kTrackMaxFrames = 65535 frames per call, each with its own K, pose, depth and mask against the same volume.
#pragma once
#include "tsdf_core.h"

namespace mp {
namespace tsdf {

constexpr int kTrackGroupPixels = 1024;
constexpr int kTrackBlock = 256;
constexpr int kTrackPixelsPerLane = kTrackGroupPixels / kTrackBlock;
constexpr int kTrackSums = 29;
constexpr int kTrackRecord = 32;
constexpr int kTrackMaxIters = 64;
constexpr int kTrackMaxFrames = 65535;
constexpr int kTrackRowFloats = 11;   // what track_row states about a used pixel: f, g [3], r, J [6]

constexpr int kTrackRan = 0, kTrackConverged = 1, kTrackLost = -1, kTrackBadView = -2;

// records per frame; 0 for a refused frame size
TSDF_HD int track_groups(int h, int w) {
  return frame_ok(h, w) ? (int)(((long long)h * w + kTrackGroupPixels - 1) / kTrackGroupPixels) : 0;
}

TSDF_HD bool track_params_ok(float mu, int min_views, int min_pixels, int iters, float eps_rot, float eps_trans) {
  return finite_f(mu) && mu > 0.f && min_views >= 1 && min_pixels >= 1 && iters >= 1 && iters <= kTrackMaxIters && finite_f(eps_rot) &&
         eps_rot >= 0.f && finite_f(eps_trans) && eps_trans >= 0.f;
}

using TrackVolume = VolumeOf<const float, const int32_t>;   // the tracker only reads the volume

// steps 2 .. 8 for the pixel (x, y) of depth d (step 1's mask is the caller's) under the loaded view v [kViewFloats]: false when the
// pixel is skipped, else row = f, g [3], r, J [6]
TSDF_HD bool track_row(int x, int y, float d, const float* v, const TrackVolume& vol, float mu, int min_views, float* row) {
  if (!(finite_f(d) && d > 0.f)) return false;
  const Grid& gr = vol;
  const float pcx = ((((float)x + 0.5f) - v[14]) / v[12]) * d;
  const float pcy = ((((float)y + 0.5f) - v[15]) / v[13]) * d;
  const float e0 = pcx - v[9], e1 = pcy - v[10], e2 = d - v[11];
  const float p0 = (v[0] * e0 + v[3] * e1) + v[6] * e2;
  const float p1 = (v[1] * e0 + v[4] * e1) + v[7] * e2;
  const float p2 = (v[2] * e0 + v[5] * e1) + v[8] * e2;
  const float qx = (p0 - gr.ox) / gr.voxel, qy = (p1 - gr.oy) / gr.voxel, qz = (p2 - gr.oz) / gr.voxel;
  const float ix = floorf(qx), iy = floorf(qy), iz = floorf(qz);
  if (!(ix >= 0.f && ix < (float)(gr.nx - 1) && iy >= 0.f && iy < (float)(gr.ny - 1) && iz >= 0.f && iz < (float)(gr.nz - 1))) return false;
  const float ux = qx - ix, uy = qy - iy, uz = qz - iz;
  const size_t base = ((size_t)(int)iz * gr.ny + (size_t)(int)iy) * gr.nx + (size_t)(int)ix;
  const int nxy = gr.nx * gr.ny;
  float F[8];
  bool seen = true;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int c = 0; c < 8; ++c) {
    const size_t g = corner_node(base, c, gr.nx, nxy);
    const int32_t cnt = vol.count[g];
    seen = seen && cnt >= min_views;
    F[c] = field(vol.sum[g], cnt);
  }
  if (!seen) return false;
  const float c00 = lerp(F[0], F[1], ux), c10 = lerp(F[2], F[3], ux), c01 = lerp(F[4], F[5], ux), c11 = lerp(F[6], F[7], ux);
  const float c0 = lerp(c00, c10, uy), c1 = lerp(c01, c11, uy);
  const float f = lerp(c0, c1, uz);
  if (!(fabsf(f) < 1.0f)) return false;
  const float dx = lerp(lerp(F[1] - F[0], F[3] - F[2], uy), lerp(F[5] - F[4], F[7] - F[6], uy), uz);
  const float dy = lerp(c10 - c00, c11 - c01, uz);
  const float dz = c1 - c0;
  const float g0 = dx / gr.voxel, g1 = dy / gr.voxel, g2 = dz / gr.voxel;
  const float m0 = g0 * mu, m1 = g1 * mu, m2 = g2 * mu;
  row[0] = f;
  row[1] = g0;
  row[2] = g1;
  row[3] = g2;
  row[4] = f * mu;
  row[5] = p1 * m2 - p2 * m1;
  row[6] = p2 * m0 - p0 * m2;
  row[7] = p0 * m1 - p1 * m0;
  row[8] = m0;
  row[9] = m1;
  row[10] = m2;
  return true;
}

// the 29 sums (by value in, by value out: they stay in registers over a lane's pixels)
struct TrackSums {
  double s[kTrackSums];
};

TSDF_HD TrackSums track_zero() {
  TrackSums a;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < kTrackSums; ++k) a.s[k] = 0.0;
  return a;
}

// one used pixel's record added to the sums
TSDF_HD TrackSums track_add(TrackSums a, const float* row) {
  double J[6];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int k = 0; k < 6; ++k) J[k] = (double)row[5 + k];
  const double r = (double)row[4];
  int at = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int j = i; j < 6; ++j) {
      a.s[at] = a.s[at] + J[i] * J[j];
      ++at;
    }
  }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
  for (int i = 0; i < 6; ++i) a.s[21 + i] = a.s[21 + i] + J[i] * r;
  a.s[27] = a.s[27] + r * r;
  a.s[28] = a.s[28] + 1.0;
  return a;
}

TSDF_HD bool finite_d(double v) { return fabs(v) <= 1.7976931348623157e308; }
TSDF_HD double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// one Gauss-Newton step from the summed record S [kTrackSums] at the fp32 pose T [12 ..] (rows of 4): the new pose's first 12 entries
// into out [12] and the status kTrackRan / kTrackConverged, or kTrackLost with out untouched
TSDF_HD int track_solve(const double* S, const float* T, int min_pixels, float eps_rot, float eps_trans, float* out, int32_t* used, float* rms) {
  const double cnt = S[28];
  *used = (int32_t)cnt;
  *rms = *used > 0 ? (float)sqrt(S[27] / cnt) : 0.f;
  if (*used < min_pixels) return kTrackLost;
  double A[6][6], L[6][6], b[6], y[6], z[6];
  int at = 0;
  for (int i = 0; i < 6; ++i)
    for (int j = i; j < 6; ++j) {
      A[i][j] = S[at];
      A[j][i] = S[at];
      ++at;
    }
  const double damp = 1e-9 * cnt;
  for (int i = 0; i < 6; ++i) {
    A[i][i] = A[i][i] + damp;
    b[i] = S[21 + i];
  }
  for (int j = 0; j < 6; ++j) {
    double d = A[j][j];
    for (int k = 0; k < j; ++k) d = d - L[j][k] * L[j][k];
    if (!(d > 0.0)) return kTrackLost;
    L[j][j] = sqrt(d);
    for (int i = j + 1; i < 6; ++i) {
      double s = A[i][j];
      for (int k = 0; k < j; ++k) s = s - L[i][k] * L[j][k];
      L[i][j] = s / L[j][j];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double s = b[i];
    for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double s = y[i];
    for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * z[k];
    z[i] = s / L[i][i];
  }
  const double w[3] = {-z[0], -z[1], -z[2]}, v[3] = {-z[3], -z[4], -z[5]};
  const double a[3] = {w[0] * 0.5, w[1] * 0.5, w[2] * 0.5};
  const double aa = dot3(a, a), s1 = 1.0 + aa, c1 = 1.0 - aa;
  const double K[3][3] = {{0.0, -a[2], a[1]}, {a[2], 0.0, -a[0]}, {-a[1], a[0], 0.0}};
  double Rc[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rc[i][j] = i == j ? (c1 + 2.0 * (a[i] * a[i])) / s1 : (2.0 * (a[i] * a[j]) + 2.0 * K[i][j]) / s1;
  double R[3][3], t[3], Rn[3][3], tn[3], m[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) R[i][j] = (double)T[4 * i + j];
    t[i] = (double)T[4 * i + 3];
  }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) Rn[i][j] = dot3(R[i], Rc[j]);
  for (int k = 0; k < 3; ++k) m[k] = (Rc[0][k] * v[0] + Rc[1][k] * v[1]) + Rc[2][k] * v[2];
  for (int i = 0; i < 3; ++i) tn[i] = t[i] - dot3(R[i], m);
  double r0[3], e[3], r1[3], r2[3];
  const double n0 = sqrt(dot3(Rn[0], Rn[0]));
  for (int k = 0; k < 3; ++k) r0[k] = Rn[0][k] / n0;
  const double pr = dot3(Rn[1], r0);
  for (int k = 0; k < 3; ++k) e[k] = Rn[1][k] - pr * r0[k];
  const double n1 = sqrt(dot3(e, e));
  for (int k = 0; k < 3; ++k) r1[k] = e[k] / n1;
  r2[0] = r0[1] * r1[2] - r0[2] * r1[1];
  r2[1] = r0[2] * r1[0] - r0[0] * r1[2];
  r2[2] = r0[0] * r1[1] - r0[1] * r1[0];
  float res[12];
  bool fin = true;
  for (int k = 0; k < 3; ++k) {
    res[k] = (float)r0[k];
    res[4 + k] = (float)r1[k];
    res[8 + k] = (float)r2[k];
    res[4 * k + 3] = (float)tn[k];
  }
  for (int k = 0; k < 12; ++k) fin = fin && finite_f(res[k]);
  if (!fin) return kTrackLost;
  for (int k = 0; k < 12; ++k) out[k] = res[k];
  return sqrt(dot3(w, w)) < (double)eps_rot && sqrt(dot3(v, v)) < (double)eps_trans ? kTrackConverged : kTrackRan;
}

}  // namespace tsdf
}  // namespace mp
