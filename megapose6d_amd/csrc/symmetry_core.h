// symmetry_core.h -- the rules of the symmetry check that runs on the device (symmetry.hip), shared with the host emulation
// (tests/symmetry_emul.cpp) the way model_info_core.h and surface_sample_core.h are shared with theirs.
//
// CONTRACT (mp_symmetry_check)
//   * SYMMETRY.  A candidate is a proper rotation R (row-major 3x3, fp32) about the object's centre c: g(p) = R (p - c) + c [apply].  It is
//     a symmetry of the object at tolerance tol when every test point p has dist(g(p), surface) <= tol.  One direction suffices: a rigid
//     map that carries the surface into itself carries it onto itself.  Reflections are not candidates (BOP's symmetries are rigid).
//   * SURFACE.  The union of the object's triangles.  A triangle is held as A, E1 = B - A, E2 = C - A (fp32 differences) and its sliver flag.
//   * DISTANCE.  The exact point-to-triangle distance by the closest-point case analysis on the vertex, edge and face regions (C. Ericson,
//     Real-Time Collision Detection, 5.1.5), in fp32 with every fused operation spelled out [tri_dist2]; it returns the SQUARED distance,
//     which is compared against tol^2.  A degenerate (zero-area) triangle goes through the same analysis, which then acts as a segment
//     or a point distance: every quotient has a guarded denominator [ratio], and a triangle with (2 area)^2 <= kSliver |E1|^2 |E2|^2
//     (the sine of its angle at A at most 2^-10: its region tests and barycentric coordinates would be rounding noise) [is_sliver,
//     decided once per triangle when it is staged] is the nearest of its three edges [seg_dist2], which is off by less than the
//     sliver's width, 2^-10 of an edge.  Nothing is skipped, nothing divides by zero.
//   * DEVIATION.  dev2 = max over test points of min over triangles of d2.  The inner minimum is that of the total order (d2, triangle
//     index) and the outer maximum that of (d2, lower point index first) [Worst, worse]: lanes walk triangles and their own points in
//     ascending order with strict comparisons, and the workgroup folds its lanes under `worse`.  A maximum of a total order does not depend
//     on the tile, the grid or the order in which the pieces arrive, so accept, dev2 and the worst point cannot change with them.
//   * NON-FINITE.  A d2 that is NaN never wins the inner minimum: a lane without any comparable triangle keeps +inf, the candidate's dev2
//     is +inf and it is rejected.  The early-out screen agrees: such a lane is never satisfied.
//   * ACCEPT.  accept = dev2 <= tol2, tol2 = tol * tol in fp32.  The screen stops a lane at its first triangle with d2 <= tol2 and a
//     candidate at its first block of kBlock test points that leaves a lane unsatisfied; "some triangle is within tol2" is "the minimum is
//     within tol2", so the screen's flag is the measured one bit for bit.
//
// LIMITS.  At most kMaxCandidates candidates in one call (one workgroup each); a triangle tile is 0 (kDefaultTile) or a multiple of kTileStep
// up to kMaxTile (three float4 per triangle in LDS: 24 KiB at the largest).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SYMM_HD __host__ __device__ __forceinline__
#else
#define SYMM_HD inline
#endif

namespace mp {
namespace symm {

constexpr int kBlock = 256;              // test points of a block, one per lane
constexpr int kTileStep = 64;            // a forced tile is a multiple of this
constexpr int kMaxTile = 512;            // triangles of one LDS stage, at most (24 KiB)
constexpr int kDefaultTile = 256;        // tile == 0
constexpr int kMaxCandidates = 1 << 20;  // candidates of one call
constexpr int kNone = 2147483647;        // the point index of "no point yet"
constexpr float kSliver = 9.5367431640625e-07f;   // 2^-20: a triangle with sin^2 of the angle at A at or below this has no face region

SYMM_HD bool tile_ok(int tile) { return tile == 0 || (tile >= kTileStep && tile <= kMaxTile && tile % kTileStep == 0); }
SYMM_HD int tile_of(int tile) { return tile == 0 ? kDefaultTile : tile; }

// the prefix arrays and tolerances of a call, one block of 32-bit words that the entry point copies to the device: four prefix arrays of
// n_obj + 1 entries (vertices, faces, test points, candidates), then tol2 [n_obj]
SYMM_HD size_t meta_words(int n_obj) { return 4 * ((size_t)n_obj + 1) + (size_t)n_obj; }

SYMM_HD float dot3(float ax, float ay, float az, float bx, float by, float bz) { return fmaf(az, bz, fmaf(ay, by, ax * bx)); }

// g(p) = R (p - c) + c
SYMM_HD void apply(const float* R, const float* c, float px, float py, float pz, float* gx, float* gy, float* gz) {
  const float qx = px - c[0], qy = py - c[1], qz = pz - c[2];
  *gx = dot3(R[0], R[1], R[2], qx, qy, qz) + c[0];
  *gy = dot3(R[3], R[4], R[5], qx, qy, qz) + c[1];
  *gz = dot3(R[6], R[7], R[8], qx, qy, qz) + c[2];
}

// n / d for a parameter in [0, 1]; a segment of no length (d == 0, or d not positive through rounding) has its one point at 0
SYMM_HD float ratio(float n, float d) { return d > 0.0f ? n / d : 0.0f; }

// squared distance of the point at offset (px, py, pz) from the segment's start to the segment 0 .. (ex, ey, ez)
SYMM_HD float seg_dist2(float px, float py, float pz, float ex, float ey, float ez) {
  float t = ratio(dot3(px, py, pz, ex, ey, ez), dot3(ex, ey, ez, ex, ey, ez));
  t = t < 0.0f ? 0.0f : (t > 1.0f ? 1.0f : t);
  const float rx = fmaf(-t, ex, px), ry = fmaf(-t, ey, py), rz = fmaf(-t, ez, pz);
  return dot3(rx, ry, rz, rx, ry, rz);
}

// squared distance of the point at offset r = (rx, ry, rz) from A to the point A + v E1 + w E2
SYMM_HD float offset_dist2(float rx, float ry, float rz, float v, float e1x, float e1y, float e1z, float w, float e2x, float e2y, float e2z) {
  const float x = fmaf(-w, e2x, fmaf(-v, e1x, rx)), y = fmaf(-w, e2y, fmaf(-v, e1y, ry)), z = fmaf(-w, e2z, fmaf(-v, e1z, rz));
  return dot3(x, y, z, x, y, z);
}

// has the triangle with the edges E1, E2 from A no face region worth the name?  (2 area)^2 = |E1|^2 |E2|^2 - (E1 . E2)^2 against
// kSliver |E1|^2 |E2|^2; a property of the triangle alone, taken once when it is staged.  A NaN edge counts as a sliver (and gives NaN).
SYMM_HD bool is_sliver(float e1x, float e1y, float e1z, float e2x, float e2y, float e2z) {
  const float l1 = dot3(e1x, e1y, e1z, e1x, e1y, e1z), l2 = dot3(e2x, e2y, e2z, e2x, e2y, e2z), l12 = dot3(e1x, e1y, e1z, e2x, e2y, e2z);
  return !(fmaf(l1, l2, -(l12 * l12)) > kSliver * (l1 * l2));
}

// the squared distance of p to the triangle A, A + E1, A + E2; sliver = is_sliver(E1, E2)
SYMM_HD float tri_dist2(float ax, float ay, float az, float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, bool sliver, float px,
                        float py, float pz) {
  const float apx = px - ax, apy = py - ay, apz = pz - az;
  const float bpx = apx - e1x, bpy = apy - e1y, bpz = apz - e1z;
  if (!sliver) {
    const float d1 = dot3(e1x, e1y, e1z, apx, apy, apz), d2 = dot3(e2x, e2y, e2z, apx, apy, apz);
    if (d1 <= 0.0f && d2 <= 0.0f) return dot3(apx, apy, apz, apx, apy, apz);                       // vertex A
    const float d3 = dot3(e1x, e1y, e1z, bpx, bpy, bpz), d4 = dot3(e2x, e2y, e2z, bpx, bpy, bpz);
    if (d3 >= 0.0f && d4 <= d3) return dot3(bpx, bpy, bpz, bpx, bpy, bpz);                         // vertex B
    const float vc = fmaf(d1, d4, -(d3 * d2));
    if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f)                                                    // edge AB
      return offset_dist2(apx, apy, apz, ratio(d1, d1 - d3), e1x, e1y, e1z, 0.0f, e2x, e2y, e2z);
    const float cpx = apx - e2x, cpy = apy - e2y, cpz = apz - e2z;
    const float d5 = dot3(e1x, e1y, e1z, cpx, cpy, cpz), d6 = dot3(e2x, e2y, e2z, cpx, cpy, cpz);
    if (d6 >= 0.0f && d5 <= d6) return dot3(cpx, cpy, cpz, cpx, cpy, cpz);                         // vertex C
    const float vb = fmaf(d5, d2, -(d1 * d6));
    if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f)                                                    // edge AC
      return offset_dist2(apx, apy, apz, 0.0f, e1x, e1y, e1z, ratio(d2, d2 - d6), e2x, e2y, e2z);
    const float va = fmaf(d3, d6, -(d5 * d4));
    const float s43 = d4 - d3, s56 = d5 - d6;
    if (va <= 0.0f && s43 >= 0.0f && s56 >= 0.0f) {                                                // edge BC
      const float w = ratio(s43, s43 + s56);
      return offset_dist2(apx, apy, apz, 1.0f - w, e1x, e1y, e1z, w, e2x, e2y, e2z);
    }
    const float sum = va + vb + vc;
    if (sum > 0.0f) {                                                                              // face
      const float inv = 1.0f / sum;
      return offset_dist2(apx, apy, apz, vb * inv, e1x, e1y, e1z, vc * inv, e2x, e2y, e2z);
    }
  }
  // a sliver (or a face case that rounding left without a positive barycentric sum): the nearest of the three edges
  const float ab = seg_dist2(apx, apy, apz, e1x, e1y, e1z), ac = seg_dist2(apx, apy, apz, e2x, e2y, e2z);
  const float bc = seg_dist2(bpx, bpy, bpz, e2x - e1x, e2y - e1y, e2z - e1z);
  return fminf(ab, fminf(ac, bc));
}

// one lane's look at a triangle (ascending triangle index per lane, so a strict comparison keeps the lowest index of equal distances;
// a NaN never wins)
SYMM_HD void lane_min(float d2, float* best) {
  if (d2 < *best) *best = d2;
}

// the worst test point so far: (d2, point index)
struct Worst {
  float d2;
  int32_t i;
};

SYMM_HD Worst none() { return Worst{-1.0f, kNone}; }   // loses against every point (their d2 >= 0 or +inf)

SYMM_HD bool worse(const Worst& a, const Worst& b) { return a.d2 > b.d2 || (a.d2 == b.d2 && a.i < b.i); }

SYMM_HD bool accepted(float dev2, float tol2) { return dev2 <= tol2; }

}  // namespace symm
}  // namespace mp
