// tsdf_core.h -- the rules of onboarding an object without a CAD model: fusing posed depth views into a truncated signed distance
// field (TSDF) on a voxel grid in the object's frame, and the welded triangle mesh of its zero level (marching tetrahedra), as they run
// on the device (tsdf.hip), shared with the host emulation (tests/tsdf_emul.cpp) the way vsd_core.h is shared with tests/vsd_emul.cpp.
// It also states the volume once [VolumeOf, Grid, volume_of, corner_node]: tsdf.hip, tsdf_track.hip and both emulations take that descriptor.
//
// CONTRACT (all arithmetic fp32, compiled with -ffp-contract=off, every operation a separate correctly rounded one in the order written;
// lengths in metres; pixel (x, y) covers [x, x+1) x [y, y+1) as in vsd_core.h)
//   * VOLUME.  Nodes p(i,j,k) = origin + voxel * (i,j,k), component by component origin[c] + voxel * (float)i  [node_coord], i < nx,
//     j < ny, k < nz, linear index (k * ny + j) * nx + i (x fastest).  The volume is 2 planes of N = nx*ny*nz 32-bit words, or 6 with
//     colours: the fp32 SUM of truncated distances, the int32 COUNT of contributing views, then the fp32 sums of red, green and blue
//     (bytes 0 .. 255 as they come) and the int32 colour count.  Sums and counts, never a running average: a call continues exactly
//     where the one before stopped, so views 0-3 then 4-7 leave the bits of 0-7 in one call.
//   * A VIEW [load_view] is K [9] row-major (fx = K[0], cx = K[2], fy = K[4], cy = K[5]) and TCO, object to camera, rows of 4 (R = the
//     3 x 3 block, t = the last column; 12 or 16 floats).  A view whose K or first 12 TCO entries hold a non-finite value contributes
//     nothing.  Views are taken in ascending order.
//   * INTEGRATING view v into a node [visit, integrate]:
//       1. pc = R p + t, each component ((R0 * px + R1 * py) + R2 * pz) + t.  Skip unless pc.z > z_min.
//       2. xf = floorf((fx * pc.x) / pc.z + cx), yf likewise.  Skip unless 0 <= xf < w and 0 <= yf < h (tested on the floats: a NaN or
//          an overflow skips).
//       3. d = the pixel's depth; a d that is not finite or <= 0 is "no measurement".  With a mask given and mask == 0 at the pixel: if
//          `carve`, the node is free space -- add +1 to the sum and 1 to the count (this carves the visual hull: a rendered or
//          segmented frame says nothing about depth outside the object) -- else skip.  Otherwise, with no measurement, skip.
//       4. sd = d - pc.z (along z, not along the ray).  Skip unless sd >= -mu (behind the surface).  Else add fminf(1, sd / mu) to the
//          sum and 1 to the count.
//       5. With colours in the volume and rgb given, and fabsf(sd) <= mu: add the pixel's three bytes to the colour sums, 1 to the
//          colour count.
//     mu is the truncation distance in metres (the Python layer passes trunc_voxels * voxel, 3 voxels by default).
//   * FIELD [field].  f = sum / (float)count.  A node with count < min_views (min_views >= 1) is unobserved.  A node is inside when
//     it is observed and f < 0; a zero is outside.
//   * SURFACE: marching tetrahedra.  Cell (i,j,k), i < nx - 1 .., has the corners c0 + {0,1}^3, corner code = dx + 2 dy + 4 dz.  It is
//     split into the six tetrahedra around its main diagonal, tetrahedron T = 0 .. 5 of the axis order (a,b,c) = xyz, xzy, yxz, yzx, zxy, zyx:
//     v0 = c0, v1 = c0 + e_a, v2 = c0 + e_a + e_b, v3 = c0 + (1,1,1)  [kTetCorner].  Its orientation det[v1-v0, v2-v0, v3-v0] is the sign
//     of the permutation: T = 0, 3, 4 are positive.  The split is the same in every cell, so faces match between neighbours.
//   * EDGES.  The six edges of a tetrahedron (0-1, 0-2, 0-3, 1-2, 1-3, 2-3: tet edge 0 .. 5) run from a lower to a higher corner in every
//     component, so each is one of the seven edge KINDS of its lower node, the owner: +x 0, +y 1, +z 2, +x+y 3, +y+z 4, +x+z 5, +x+y+z 6
//     [kKindDiff, kKindOfDiff].  An edge carries a vertex iff both ends are observed, exactly one end is inside, and the edge belongs
//     to at least one COMPLETE cell (all eight corners observed) [the cells of edge (owner o, difference d): c0 = o or, on an axis with
//     d = 0, o - 1].  Only complete cells emit triangles.
//   * VERTEX [edge_t, lerp].  With a the owner and b the far node, t = fa / (fa - fb), position pa + t * (pb - pa) per component:
//     every cell that shares the edge computes the same bits.  Colour: the node's mean colour (sum / (float)count) / 255 per channel,
//     white (1) for a node without colour or a volume without colours, interpolated the same way.
//   * ORDER.  Vertex index = the rank of (node linear index * 7 + kind) among the vertex-carrying edges.  Triangle index = the rank of
//     (cell's linear node index, tetrahedron, triangle within the case).
//   * CASES [kTetCount, kTetTri].  The case of a tetrahedron is the 4-bit mask of its inside corners (bit q: v_q inside).  One corner a
//     on its own side, the others b < c < d: the triangle (ab, ac, ad); two inside a < b, two outside c < d: the quad ac, ad, bd, bc
//     as (ac, ad, bd) and (ac, bd, bc).  Winding: normals point towards positive f, out of the object -- for a positive tetrahedron as
//     the table lists them, for a negative one with the second and third corner swapped.  (Case 0001 by hand: v0 = 0, v1 = e1, v2 = e2,
//     v3 = e3, the midpoints give (e2 - e1) x (e3 - e1) / 4 = (1,1,1) / 4, away from v0.)  Zero-area triangles are kept: they appear when
//     an f is exactly 0.
// Every count, rank and index is an integer; every float is produced by one thread from the rules above: no grid can change a result.
//
// LIMITS.  2 <= nx, ny, nz <= kMaxDim = 512, nx * ny * nz <= kMaxNodes = 2^27 (so node * 7 + kind, 7 N vertices and 12 N triangles
// fit an int32); 1 <= h, w <= kMaxSide = 8192; n >= 0 views per call; voxel, mu finite and > 0; z_min finite and >= 0; origin finite;
// 1 <= min_views.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TSDF_HD __host__ __device__ __forceinline__
#else
#define TSDF_HD static inline
#endif

namespace mp {
namespace tsdf {

constexpr int kMinDim = 2, kMaxDim = 512;
constexpr long long kMaxNodes = 1LL << 27;
constexpr int kMaxSide = 8192;
constexpr int kEdgeKinds = 7;
constexpr int kTets = 6;
constexpr int kViewFloats = 16;   // a loaded view: R [9], t [3], fx, fy, cx, cy

// flags of a node (extraction)
constexpr int kObserved = 1, kInside = 2;

TSDF_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

TSDF_HD bool dims_ok(int nx, int ny, int nz) {
  return nx >= kMinDim && ny >= kMinDim && nz >= kMinDim && nx <= kMaxDim && ny <= kMaxDim && nz <= kMaxDim &&
         (long long)nx * ny * nz <= kMaxNodes;
}
TSDF_HD bool frame_ok(int h, int w) { return h >= 1 && w >= 1 && h <= kMaxSide && w <= kMaxSide; }
TSDF_HD bool grid_ok(const float* origin, float voxel) {
  return finite_f(origin[0]) && finite_f(origin[1]) && finite_f(origin[2]) && finite_f(voxel) && voxel > 0.f;
}
TSDF_HD int planes(int color) { return color ? 6 : 2; }

TSDF_HD float node_coord(float origin, float voxel, int i) { return origin + voxel * (float)i; }

// ---- the volume, as every kernel, entry and emulation that touches one takes it -------------------------------------------------
struct Grid {
  int nx, ny, nz, N;   // N = nx * ny * nz
  float ox, oy, oz, voxel;
};

// the planes of the CONTRACT over their grid, F and I = float and int32_t, or both const for an entry that only reads.  (Planes first, the
// grid as a base of its own: a kernel that reads no plane takes the `Grid` alone.)
template <class F, class I>
struct Planes {
  F* sum;
  I* count;
  F* c[3];      // null without colours
  I* c_count;   // null without colours
};
template <class F, class I>
struct VolumeOf : Planes<F, I>, Grid {};
using Volume = VolumeOf<float, int32_t>;

// `volume` must not be null; an entry that takes the volume const asks for const planes, or casts the const away here and stores nothing
template <class F = float, class I = int32_t, class P>
TSDF_HD VolumeOf<F, I> volume_of(P* volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel) {
  F* f = static_cast<F*>(volume);
  const size_t N = (size_t)nx * ny * nz;
  VolumeOf<F, I> v;
  v.sum = f;
  v.count = (I*)(f + N);
  for (int k = 0; k < 3; ++k) v.c[k] = color ? f + (2 + k) * N : nullptr;
  v.c_count = color ? (I*)(f + 5 * N) : nullptr;
  (Grid&)v = {nx, ny, nz, (int)N, ox, oy, oz, voxel};
  return v;
}

// the linear index of the corner `code` = dx + 2 dy + 4 dz of the cell at node g (nxy = nx * ny; I is int, or size_t where the caller
// indexes in it)
template <class I>
TSDF_HD I corner_node(I g, int code, int nx, int nxy) {
  return g + (I)(code & 1) + (I)((code >> 1) & 1) * (I)nx + (I)((code >> 2) & 1) * (I)nxy;
}

// K [9], T [12 ..] -> v [kViewFloats]; false when an entry is not finite (the view then contributes nothing)
TSDF_HD bool load_view(const float* K, const float* T, float* v) {
  bool ok = true;
  for (int k = 0; k < 9; ++k) ok = ok && finite_f(K[k]);
  for (int k = 0; k < 12; ++k) ok = ok && finite_f(T[k]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) v[3 * r + c] = T[4 * r + c];
    v[9 + r] = T[4 * r + 3];
  }
  v[12] = K[0];
  v[13] = K[4];
  v[14] = K[2];
  v[15] = K[5];
  return ok;
}

struct Node {
  float sum;
  int32_t count;
  float c0, c1, c2;
  int32_t c_count;
};

// what one view adds to one node at (px, py, pz); depth / mask / rgb are the view's frame (mask, rgb may be null)
struct Visit {
  bool hit;        // `add` joins the sum, 1 the count
  float add;
  bool colored;    // r, g, b join the colour sums, 1 the colour count
  float r, g, b;
};

TSDF_HD Visit visit(float px, float py, float pz, const float* v, const float* depth, const uint8_t* mask, const uint8_t* rgb, int h, int w,
                    float mu, float z_min, bool carve, bool color) {
  Visit s = {false, 0.f, false, 0.f, 0.f, 0.f};
  const float cz = ((v[6] * px + v[7] * py) + v[8] * pz) + v[11];
  if (!(cz > z_min)) return s;
  const float cxm = ((v[0] * px + v[1] * py) + v[2] * pz) + v[9];
  const float cym = ((v[3] * px + v[4] * py) + v[5] * pz) + v[10];
  const float xf = floorf((v[12] * cxm) / cz + v[14]);
  const float yf = floorf((v[13] * cym) / cz + v[15]);
  if (!(xf >= 0.f && xf < (float)w && yf >= 0.f && yf < (float)h)) return s;
  const size_t at = (size_t)(int)yf * w + (int)xf;
  if (mask && mask[at] == 0) {
    s.hit = carve;
    s.add = 1.0f;
    return s;
  }
  const float d = depth[at];
  if (!(finite_f(d) && d > 0.f)) return s;
  const float sd = d - cz;
  if (!(sd >= -mu)) return s;
  s.hit = true;
  s.add = fminf(1.0f, sd / mu);
  if (color && rgb && fabsf(sd) <= mu) {
    s.colored = true;
    s.r = (float)rgb[3 * at + 0];
    s.g = (float)rgb[3 * at + 1];
    s.b = (float)rgb[3 * at + 2];
  }
  return s;
}

// one view into one node (the node's words by value in, by value out: they stay in registers over the views of a call)
TSDF_HD Node integrate(Node nd, const Visit& s) {
  if (s.hit) {
    nd.sum = nd.sum + s.add;
    nd.count += 1;
  }
  if (s.colored) {
    nd.c0 = nd.c0 + s.r;
    nd.c1 = nd.c1 + s.g;
    nd.c2 = nd.c2 + s.b;
    nd.c_count += 1;
  }
  return nd;
}

// ---- the field -------------------------------------------------------------------------------------------------------------------
TSDF_HD float field(float sum, int32_t count) { return sum / (float)count; }
TSDF_HD int node_flags(float sum, int32_t count, int min_views) {
  if (count < min_views) return 0;
  return kObserved | (field(sum, count) < 0.f ? kInside : 0);
}
TSDF_HD float edge_t(float fa, float fb) { return fa / (fa - fb); }
TSDF_HD float lerp(float a, float b, float t) { return a + t * (b - a); }
TSDF_HD float node_color(float sum, int32_t count) { return count > 0 ? (sum / (float)count) / 255.0f : 1.0f; }

// ---- the tetrahedra --------------------------------------------------------------------------------------------------------------
struct Tables {
  int8_t corner[kTets][4];     // corner codes (dx + 2 dy + 4 dz) of v0 .. v3
  int8_t positive[kTets];
  int8_t kind_diff[kEdgeKinds];   // the difference code of each edge kind
  int8_t kind_of_diff[8];
  int8_t edge_end[6][2];          // tet edge -> its two tet corners, lower first
  int8_t count[16];
  int8_t tri[16][2][3];           // tet edges of the triangles of a case, positive orientation
};

// one initialiser, two objects: the host's, and the device's in constant memory (a by-value table would live in scratch: its entries are
// indexed at run time)
#define MP_TSDF_TABLES \
{ \
      {{0, 1, 3, 7}, {0, 1, 5, 7}, {0, 2, 3, 7}, {0, 2, 6, 7}, {0, 4, 5, 7}, {0, 4, 6, 7}}, \
      {1, 0, 0, 1, 1, 0}, \
      {1, 2, 4, 3, 6, 5, 7}, \
      {-1, 0, 1, 3, 2, 5, 4, 6}, \
      {{0, 1}, {0, 2}, {0, 3}, {1, 2}, {1, 3}, {2, 3}}, \
      {0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0}, \
      {{{0, 0, 0}, {0, 0, 0}}, \
       {{0, 1, 2}, {0, 0, 0}}, \
       {{0, 4, 3}, {0, 0, 0}}, \
       {{1, 2, 4}, {1, 4, 3}}, \
       {{1, 3, 5}, {0, 0, 0}}, \
       {{0, 5, 2}, {0, 3, 5}}, \
       {{0, 4, 5}, {0, 5, 1}}, \
       {{2, 4, 5}, {0, 0, 0}}, \
       {{2, 5, 4}, {0, 0, 0}}, \
       {{0, 1, 5}, {0, 5, 4}}, \
       {{0, 5, 3}, {0, 2, 5}}, \
       {{1, 5, 3}, {0, 0, 0}}, \
       {{1, 3, 4}, {1, 4, 2}}, \
       {{0, 3, 4}, {0, 0, 0}}, \
       {{0, 2, 1}, {0, 0, 0}}, \
       {{0, 0, 0}, {0, 0, 0}}}}
static const Tables kHostTables = MP_TSDF_TABLES;
#if defined(__HIPCC__)
static __device__ __constant__ const Tables kDeviceTables = MP_TSDF_TABLES;
#endif
#undef MP_TSDF_TABLES

TSDF_HD const Tables& tables() {
#if defined(__HIP_DEVICE_COMPILE__)
  return kDeviceTables;
#else
  return kHostTables;
#endif
}

// the case of tetrahedron T from the inside bits of the cell's eight corners (bit = corner code)
TSDF_HD int tet_case(const Tables& tb, int T, int inside8) {
  int m = 0;
  for (int q = 0; q < 4; ++q) m |= ((inside8 >> tb.corner[T][q]) & 1) << q;
  return m;
}

// triangles of a complete cell
TSDF_HD int cell_triangles(const Tables& tb, int inside8) {
  int n = 0;
  for (int T = 0; T < kTets; ++T) n += tb.count[tet_case(tb, T, inside8)];
  return n;
}

// corner `s` (0 .. 2) of triangle `tri` of tetrahedron T in case m -> the corner code of the edge's owner and the edge's kind
TSDF_HD void tri_edge(const Tables& tb, int T, int m, int tri, int s, int* owner_code, int* kind) {
  const int slot = tb.positive[T] ? s : (s == 0 ? 0 : 3 - s);
  const int e = tb.tri[m][tri][slot];
  const int lo = tb.corner[T][tb.edge_end[e][0]], hi = tb.corner[T][tb.edge_end[e][1]];
  *owner_code = lo;
  *kind = tb.kind_of_diff[hi - lo];
}

}  // namespace tsdf
}  // namespace mp
