// texture_bake_core.h -- the rules of baking a texture atlas for a triangle mesh from posed colour + depth views: every triangle gets a
// chart in a square atlas, every texel of a chart gathers its colour from the views that see its surface point.  As they run on the
// device (texture_bake.hip), shared with the host emulation (tests/texture_bake_emul.cpp) the way tsdf_core.h is shared with
// tests/tsdf_emul.cpp.
//
// CONTRACT (all arithmetic fp32, compiled with -ffp-contract=off, every operation a separate correctly rounded one in the order written,
// no sqrt; lengths in metres; pixel (x, y) covers [x, x+1) x [y, y+1) as in tsdf_core.h, so a pixel's value sits at (x + 0.5, y + 0.5))
//   * ATLAS.  S x S texels, S a power of two, kMinSize = 64 .. kMaxSize = 8192; array row 0 is v = 0 (the engine's convention:
//     mesh_io.load_texture flips the picture).  Texel (i, j) -- column i, row j -- has its centre at ((i + 0.5) / S, (j + 0.5) / S).  The
//     atlas is cut into square blocks of B x B texels, B in {4, 8, 16, 32, 64}, in row-major block order: block k has its origin texel
//     (X, Y) = ((k % (S / B)) * B, (k / (S / B)) * B).  Block k holds triangle 2k (the LOWER chart) and triangle 2k + 1 (the UPPER chart).
//     [atlas_block] (T, S) is the largest allowed B with ceil(T / 2) <= (S / B)^2, 0 if none.  S and B are powers of two, so mip levels
//     up to log2 B average inside one block.
//   * CHART.  Leg c = B - 3.  Lower chart: corners 0, 1, 2 at the local texels (0, 0), (c, 0), (0, c); upper chart: at (B-1, B-1),
//     (B-1-c, B-1), (B-1, B-1-c) -- the lower chart turned by 180 degrees, so the winding is kept.  A corner's UV is its texel's centre
//     [corner_uv].  Local texel (i, j) belongs to the lower chart when i + j <= B - 1, else to the upper one; the diagonal
//     i + j = B - 1, the gutter, is baked as the lower chart's.
//   * SURFACE POINT [chart_point].  a = (float)(i - i0) / (float)c, b = (float)(j - j0) / (float)c from the chart's corner 0 at (i0, j0)
//     -- for the upper chart along its mirrored axes: (float)(i0 - i) / (float)c, (float)(j0 - j) / (float)c.  Both are clamped at 0
//     (fmaxf).  If a + b > 1, with s = a + b: a = a / s, b = b / s.  So the spill and gutter texels bake a point of their own triangle's
//     hypotenuse.  p = (v0 + a * (v1 - v0)) + b * (v2 - v0) per component; the face normal n = (v1 - v0) x (v2 - v0), each component
//     (e1[y] * e2[z]) - (e1[z] * e2[y]) in cyclic order, not normalised; |n|^2 = (nx nx + ny ny) + nz nz.
//   * A VIEW is loaded as tsdf::load_view does: K [9], TCO object to camera, rows of 4 (12 or 16 floats).  A view whose K or first 12
//     TCO entries hold a non-finite value contributes nothing.  Views are taken in ascending order.
//   * PER VIEW AND TEXEL [visit]:
//       1. pc = R p + t, each component ((R0 * px + R1 * py) + R2 * pz) + t, as tsdf::visit.  Skip unless pc.z > z_min.
//       2. xf = (fx * pc.x) / pc.z + cx, yf likewise.
//       3. The nearest pixel is (floorf(xf), floorf(yf)); skip unless 0 <= floorf(xf) < w and 0 <= floorf(yf) < h, tested on the floats
//          (a NaN or an overflow skips).
//       4. Facing.  Rn = R n, each component (R0 * nx + R1 * ny) + R2 * nz; g = -((Rn.x * pc.x + Rn.y * pc.y) + Rn.z * pc.z);
//          |pc|^2 = (pc.x pc.x + pc.y pc.y) + pc.z pc.z; den = |n|^2 * |pc|^2.  Skip unless g > 0 and g * g > (cos_min * cos_min) * den.
//          The weight is wgt = (g * g) / den: cos^2 of the angle between the normal and the ray, with one division.
//       5. A tap (a pixel (x, y), integers) passes when it is in the frame, its mask is non-zero where masks are given, its depth d is
//          finite and > 0, and fabsf(d - pc.z) <= depth_tol -- the occlusion test against the view's own depth [tap].
//       6. Colour.  tx = xf - 0.5, ty = yf - 0.5; the four taps are (floorf(tx) + {0, 1}, floorf(ty) + {0, 1}); ax = tx - floorf(tx),
//          ay likewise.  If all four pass, per channel top = c00 + ax * (c01 - c00), bot = c10 + ax * (c11 - c10) (first index y),
//          colour = top + ay * (bot - top); no fmaf.  Otherwise, if the nearest pixel passes, the colour is its bytes.  Otherwise the
//          view is skipped.
//   * RESULT [Accum, finish].  Blend (the default): per channel (sum of wgt * colour) / (sum of wgt), both sums in view order.
//     best_view: the colour of the view with the largest wgt, ties to the lower index.  Then q255 (clamp to 0 .. 255, round half up, as
//     raster_core.h) gives the byte.  seen = the number of contributing views, capped at 255.  A texel with seen == 0 takes the
//     triangle's interpolated vertex colours, q255(((((1 - a) - b) * c0 + a * c1) + b * c2) * 255) per channel, when colours ([V,3] floats
//     in 0 .. 1) are given, else white.  Alpha is 255 for every texel of a triangle.  Texels of blocks past the last triangle, and the
//     upper half of the last block when T is odd, are four zero bytes with seen 0.
//   * SAFETY [load_tri].  A face with an index outside [0, V) bakes as unseen and white (its colours cannot be addressed either); a face
//     with a non-finite vertex bakes as unseen (no view is visited); a zero-area triangle has n = 0, so g > 0 never holds and it bakes
//     as unseen.  None of them ever causes an access out of range.
// Every float is produced by one thread from the rules above: no grid shape or block size can change a bit.
//
// LIMITS.  1 <= T <= 2^29, 0 <= V <= 2^29, atlas_block(T, S) > 0; frames 1 <= h, w <= tsdf::kMaxSide = 8192; n >= 0 views; depth_tol
// finite and > 0; 0 <= cos_min < 1; z_min finite and >= 0.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "tsdf_core.h"

namespace mp {
namespace texbake {

constexpr int kMinSize = 64, kMaxSize = 8192;
constexpr int kMinBlock = 4, kMaxBlock = 64;
constexpr int kMaxCount = 1 << 29;   // triangles, vertices

TSDF_HD bool size_ok(int S) { return S >= kMinSize && S <= kMaxSize && (S & (S - 1)) == 0; }

// the largest B in {64, 32, 16, 8, 4} whose blocks hold T triangles two by two in an S x S atlas; 0 if none (or a bad S, T)
TSDF_HD int atlas_block(long long T, int S) {
  if (!size_ok(S) || T < 1) return 0;
  const long long pairs = (T + 1) / 2;
  for (int B = kMaxBlock; B >= kMinBlock; B >>= 1) {
    const long long side = S / B;
    if (pairs <= side * side) return B;
  }
  return 0;
}

TSDF_HD bool params_ok(float depth_tol, float cos_min, float z_min) {
  return tsdf::finite_f(depth_tol) && depth_tol > 0.f && cos_min >= 0.f && cos_min < 1.f && tsdf::finite_f(z_min) && z_min >= 0.f;
}

// the local texel of corner `k` (0 .. 2) of the lower / upper chart of a block of B
TSDF_HD void corner_texel(int B, int upper, int k, int* i, int* j) {
  const int c = B - 3;
  const int di = k == 1 ? c : 0, dj = k == 2 ? c : 0;
  *i = upper ? B - 1 - di : di;
  *j = upper ? B - 1 - dj : dj;
}

// UV of corner k of triangle t: its texel's centre
TSDF_HD void corner_uv(int t, int k, int S, int B, float* u, float* v) {
  const int blk = t >> 1, side = S / B;
  int i, j;
  corner_texel(B, t & 1, k, &i, &j);
  *u = ((float)((blk % side) * B + i) + 0.5f) / (float)S;
  *v = ((float)((blk / side) * B + j) + 0.5f) / (float)S;
}

// local texel (i, j) of a block -> its chart (0 lower, 1 upper) and the chart coordinates of the point it bakes
TSDF_HD int chart_point(int B, int i, int j, float* a_out, float* b_out) {
  const int c = B - 3;
  const int upper = i + j > B - 1;
  float a = (float)(upper ? B - 1 - i : i) / (float)c;
  float b = (float)(upper ? B - 1 - j : j) / (float)c;
  a = fmaxf(a, 0.f);
  b = fmaxf(b, 0.f);
  const float s = a + b;
  if (s > 1.f) {
    a = a / s;
    b = b / s;
  }
  *a_out = a;
  *b_out = b;
  return upper;
}

constexpr int kTriFloats = 22;   // v0 [3], e1 [3], e2 [3], n [3], |n|^2, colours of the corners [9]
constexpr int kTriIndexed = 1, kTriFinite = 2;   // flags of a triangle: its indices are in range; its vertices are finite

// triangle t -> tri [kTriFloats] and its flags.  Nothing is read through an index outside [0, V); without colours the corners are white.
TSDF_HD int load_tri(const float* vertices, int V, const int32_t* faces, int t, const float* colors, float* tri) {
  for (int k = 0; k < kTriFloats; ++k) tri[k] = k < 13 ? 0.f : 1.f;
  const int32_t i0 = faces[3 * (size_t)t + 0], i1 = faces[3 * (size_t)t + 1], i2 = faces[3 * (size_t)t + 2];
  if (i0 < 0 || i1 < 0 || i2 < 0 || i0 >= V || i1 >= V || i2 >= V) return 0;
  const float* v0 = vertices + 3 * (size_t)i0;
  const float* v1 = vertices + 3 * (size_t)i1;
  const float* v2 = vertices + 3 * (size_t)i2;
  bool fin = true;
  for (int k = 0; k < 3; ++k) {
    fin = fin && tsdf::finite_f(v0[k]) && tsdf::finite_f(v1[k]) && tsdf::finite_f(v2[k]);
    tri[k] = v0[k];
    tri[3 + k] = v1[k] - v0[k];
    tri[6 + k] = v2[k] - v0[k];
  }
  const float* e1 = tri + 3;
  const float* e2 = tri + 6;
  tri[9] = (e1[1] * e2[2]) - (e1[2] * e2[1]);
  tri[10] = (e1[2] * e2[0]) - (e1[0] * e2[2]);
  tri[11] = (e1[0] * e2[1]) - (e1[1] * e2[0]);
  tri[12] = (tri[9] * tri[9] + tri[10] * tri[10]) + tri[11] * tri[11];
  if (colors)
    for (int k = 0; k < 3; ++k) {
      tri[13 + k] = colors[3 * (size_t)i0 + k];
      tri[16 + k] = colors[3 * (size_t)i1 + k];
      tri[19 + k] = colors[3 * (size_t)i2 + k];
    }
  return kTriIndexed | (fin ? kTriFinite : 0);
}

TSDF_HD void surface_point(const float* tri, float a, float b, float* p) {
  for (int k = 0; k < 3; ++k) p[k] = (tri[k] + a * tri[3 + k]) + b * tri[6 + k];
}

struct Tap {
  bool ok;
  float c[3];
};

// pixel (x, y) of a view's frame against the camera-space depth cz of the point
TSDF_HD Tap tap(int x, int y, const float* depth, const uint8_t* mask, const uint8_t* rgb, int h, int w, float cz, float depth_tol) {
  Tap t = {false, {0.f, 0.f, 0.f}};
  if (x < 0 || y < 0 || x >= w || y >= h) return t;
  const size_t at = (size_t)y * w + x;
  if (mask && mask[at] == 0) return t;
  const float d = depth[at];
  if (!(tsdf::finite_f(d) && d > 0.f)) return t;
  if (!(fabsf(d - cz) <= depth_tol)) return t;
  t.ok = true;
  t.c[0] = (float)rgb[3 * at + 0];
  t.c[1] = (float)rgb[3 * at + 1];
  t.c[2] = (float)rgb[3 * at + 2];
  return t;
}

struct Visit {
  bool hit;
  float wgt;
  float c[3];
};

// what view v [tsdf::kViewFloats] says about the point p of a triangle with normal n (tri + 9) and |n|^2 (tri[12])
TSDF_HD Visit visit(const float* p, const float* tri, const float* v, const float* depth, const uint8_t* mask, const uint8_t* rgb, int h, int w,
                    float depth_tol, float cos_min2, float z_min) {
  Visit s = {false, 0.f, {0.f, 0.f, 0.f}};
  const float cz = ((v[6] * p[0] + v[7] * p[1]) + v[8] * p[2]) + v[11];
  if (!(cz > z_min)) return s;
  const float cxm = ((v[0] * p[0] + v[1] * p[1]) + v[2] * p[2]) + v[9];
  const float cym = ((v[3] * p[0] + v[4] * p[1]) + v[5] * p[2]) + v[10];
  const float xf = (v[12] * cxm) / cz + v[14];
  const float yf = (v[13] * cym) / cz + v[15];
  const float xn = floorf(xf), yn = floorf(yf);
  if (!(xn >= 0.f && xn < (float)w && yn >= 0.f && yn < (float)h)) return s;
  const float* n = tri + 9;
  const float rx = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
  const float ry = (v[3] * n[0] + v[4] * n[1]) + v[5] * n[2];
  const float rz = (v[6] * n[0] + v[7] * n[1]) + v[8] * n[2];
  const float g = -((rx * cxm + ry * cym) + rz * cz);
  const float pp = (cxm * cxm + cym * cym) + cz * cz;
  const float den = tri[12] * pp;
  const float gg = g * g;
  if (!(g > 0.f && gg > cos_min2 * den)) return s;
  s.wgt = gg / den;
  const float tx = xf - 0.5f, ty = yf - 0.5f;
  const float fx = floorf(tx), fy = floorf(ty);
  const float ax = tx - fx, ay = ty - fy;
  const int x0 = (int)fx, y0 = (int)fy;   // (-1 .. w - 1, -1 .. h - 1: the nearest pixel is in the frame)
  const Tap t00 = tap(x0, y0, depth, mask, rgb, h, w, cz, depth_tol);
  const Tap t01 = tap(x0 + 1, y0, depth, mask, rgb, h, w, cz, depth_tol);
  const Tap t10 = tap(x0, y0 + 1, depth, mask, rgb, h, w, cz, depth_tol);
  const Tap t11 = tap(x0 + 1, y0 + 1, depth, mask, rgb, h, w, cz, depth_tol);
  if (t00.ok && t01.ok && t10.ok && t11.ok) {
    for (int k = 0; k < 3; ++k) {
      const float top = t00.c[k] + ax * (t01.c[k] - t00.c[k]);
      const float bot = t10.c[k] + ax * (t11.c[k] - t10.c[k]);
      s.c[k] = top + ay * (bot - top);
    }
    s.hit = true;
    return s;
  }
  const Tap tn = tap((int)xn, (int)yn, depth, mask, rgb, h, w, cz, depth_tol);
  if (!tn.ok) return s;
  for (int k = 0; k < 3; ++k) s.c[k] = tn.c[k];
  s.hit = true;
  return s;
}

// a texel's state over the views
struct Accum {
  float sum[3];   // blend: the sums of wgt * colour; best_view: the best colour
  float w;        // blend: the sum of wgt; best_view: the best wgt
  int seen;
};

TSDF_HD Accum accum_init() {
  Accum a = {{0.f, 0.f, 0.f}, 0.f, 0};
  return a;
}

TSDF_HD Accum accumulate(Accum a, const Visit& s, bool best_view) {
  if (!s.hit) return a;
  if (best_view) {
    if (a.seen == 0 || s.wgt > a.w) {
      a.w = s.wgt;
      for (int k = 0; k < 3; ++k) a.sum[k] = s.c[k];
    }
  } else {
    for (int k = 0; k < 3; ++k) a.sum[k] = a.sum[k] + s.wgt * s.c[k];
    a.w = a.w + s.wgt;
  }
  a.seen += 1;
  return a;
}

// clamp to [0, 255] and round half up, as raster_core.h's q255; NaN -> 0
TSDF_HD float q255(float v255) { return floorf(fminf(fmaxf(v255, 0.f), 255.f) + 0.5f); }

// the texel's four bytes (R in the low byte, alpha 255) and its `seen`
TSDF_HD uint32_t finish(const Accum& acc, const float* tri, float a, float b, bool best_view, uint8_t* seen) {
  float c[3];
  if (acc.seen > 0) {
    for (int k = 0; k < 3; ++k) c[k] = best_view ? acc.sum[k] : acc.sum[k] / acc.w;
  } else {
    const float w0 = (1.f - a) - b;
    for (int k = 0; k < 3; ++k) c[k] = (((w0 * tri[13 + k]) + a * tri[16 + k]) + b * tri[19 + k]) * 255.f;
  }
  *seen = (uint8_t)(acc.seen > 255 ? 255 : acc.seen);
  return (uint32_t)q255(c[0]) | ((uint32_t)q255(c[1]) << 8) | ((uint32_t)q255(c[2]) << 16) | 0xFF000000u;
}

}  // namespace texbake
}  // namespace mp
