// mesh_cleanup_core.h -- the rules of cleaning up a triangle mesh on the device (mesh_cleanup.hip): its connected components, the
// selection of faces with the vertices they reference, and decimation by vertex clustering (Rossignac-Borrel).  Shared with the host
// emulation (tests/mesh_cleanup_emul.cpp) the way tsdf_core.h is shared with tests/tsdf_emul.cpp.
//
// CONTRACT (float arithmetic fp32 unless a double is written, compiled with -ffp-contract=off, every operation a separate correctly
// rounded one in the order written).  A mesh is V vertices [V,3] fp32, F faces [F,3] int32 and optionally colours [V,3] fp32.
//   * BAD FACES [face_good].  A face with an index outside [0, V) is bad: it joins nothing, is never emitted, and its index is never
//     used as an address.  The number of bad faces comes back with the totals.
//   * COMPONENTS.  label[v] = the smallest vertex index of v's connected component (two vertices are connected when a chain of good
//     faces joins them; a vertex on no good face is its own label).  face_label[f] = label[faces[f][0]], -1 for a bad face.
//     face_count[l] = the number of good faces of label l, 0 where l is not a label.  totals [kComponentTotals]: the components that
//     own at least one face; the label of the one with the most faces, the smaller label on equal counts, -1 when there is none; the
//     bad faces; a status (0, or kStatusCap when a loop of the device's union-find ran into its cap: the labels are then not to be
//     used).  The result is unique, whatever union-find produces it.
//   * SELECT.  keep[f] != 0 keeps face f.  Out: the kept good faces in input order, the vertices they reference in input order,
//     renumbered; vertices and colours are copied bit for bit.  totals [kTotals]: vertices out, faces out, bad faces (kept or not).
//   * CLUSTER.  Grid: origin o (finite), cell size c (finite, > 0), dims g (1 .. kMaxDim a side, at most kMaxCells cells).
//       Per vertex and axis [cell_axis]: u = (p - o) / c, i = floorf(u).  The vertex is bad when on any axis !(i >= 0 && i < (float)g),
//       tested on the floats, so that a NaN, an infinity and an overflow fail; a bad vertex belongs to no cell.
//       Cell id = i.x + g.x * (i.y + g.y * i.z).
//       A face is kept iff it is good, none of its vertices is bad, and its three cell ids differ pairwise.  A cell is used iff a kept
//       face references it.  Output vertex = the rank of the used cell in cell-id order; output face = the rank of the kept face in
//       input order; the corner order is unchanged.  Duplicate and opposite triangles are kept.
//       Position of an output vertex: the mean over ALL good vertices of its cell (on a kept face or not), exact: each coordinate
//       contributes the integer t = (int64)(u * 65536.0f), truncated [fixed_of; u < 512, so t < 2^25 and the product is exact]; sums
//       int64, count int32; p' = (float)((double)o + (double)c * ((double)sum / ((double)count * 65536.0)))  [mean_coord].
//       Colours: each channel contributes (int)(fminf(fmaxf(col, 0), 1) * 65535.0f + 0.5f) [color_of; a NaN counts as 0]; sums int64;
//       out = (float)((double)sum / ((double)count * 65535.0))  [mean_color].  Without colours nothing is computed.
//       totals [kTotals]: vertices out, faces out, bad faces + faces dropped for a bad vertex.
// Integer sums do not depend on the order of their terms, every float is produced by one thread from finished integers: no grid, no
// arrival order of an atomic and no order of the faces or vertices can change a bit of a result.
//
// LIMITS.  0 <= V, F <= kMaxCount = 2^29 (3 F fits an int32; addresses are 64-bit anyway); 1 <= g <= kMaxDim = 512 a side,
// g.x g.y g.z <= kMaxCells = 2^27.  V = 0 or F = 0 is a success with zero totals (the faces of a mesh without vertices are not
// counted as bad; components then still writes label[v] = v, face_count 0, face_label -1 and the largest label -1).
//
// LOOP CAP of the device's union-find [loop_cap]: parent[v] <= v always and only ever decreases, so a walk towards the root visits
// strictly decreasing indices: at most V - 1 steps.  A union retries only when its atomicMin found the word already lowered by another
// lane; every such event is one of at most V - 1 successful hooks or follows one, so no correct run retries more than V times.  Both
// loops stop after V + 1 rounds and raise kStatusCap: a bug or a corrupted array costs a status, never a hang.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MESHC_HD __host__ __device__ __forceinline__
#else
#define MESHC_HD static inline
#endif

namespace mp {
namespace meshc {

constexpr int kMaxCount = 1 << 29;
constexpr int kMaxDim = 512;
constexpr long long kMaxCells = 1LL << 27;
constexpr int kTotals = 3;             // select, cluster: vertices out, faces out, bad (+ dropped) faces
constexpr int kComponentTotals = 4;    // components, largest label, bad faces, status
constexpr int kStatusCap = 1;
constexpr float kFixedOne = 65536.0f;
constexpr float kColorOne = 65535.0f;

MESHC_HD bool finite_f(float v) { return fabsf(v) <= 3.402823466e38f; }   // false for NaN and +-inf

MESHC_HD bool counts_ok(long long V, long long F) { return V >= 0 && F >= 0 && V <= kMaxCount && F <= kMaxCount; }
MESHC_HD bool dims_ok(int gx, int gy, int gz) {
  return gx >= 1 && gy >= 1 && gz >= 1 && gx <= kMaxDim && gy <= kMaxDim && gz <= kMaxDim && (long long)gx * gy * gz <= kMaxCells;
}
MESHC_HD bool grid_ok(float ox, float oy, float oz, float cell) { return finite_f(ox) && finite_f(oy) && finite_f(oz) && finite_f(cell) && cell > 0.f; }
MESHC_HD long long loop_cap(int V) { return (long long)V + 1; }

MESHC_HD bool face_good(int a, int b, int c, int V) { return (unsigned)a < (unsigned)V && (unsigned)b < (unsigned)V && (unsigned)c < (unsigned)V; }

// one axis of a vertex: u in cells from the origin, *i its cell; false when the vertex is bad on this axis
MESHC_HD bool cell_axis(float p, float o, float c, int g, float* u, int* i) {
  *u = (p - o) / c;
  const float fl = floorf(*u);
  const bool ok = fl >= 0.f && fl < (float)g;
  *i = ok ? (int)fl : 0;
  return ok;
}

// the cell id of a vertex or -1; u [3] is meaningful only with a cell
MESHC_HD int cell_of(const float* p, const float* o, float c, const int* g, float* u) {
  int i[3];
  bool ok = true;
  for (int k = 0; k < 3; ++k) ok = cell_axis(p[k], o[k], c, g[k], &u[k], &i[k]) && ok;
  return ok ? i[0] + g[0] * (i[1] + g[1] * i[2]) : -1;
}

MESHC_HD long long fixed_of(float u) { return (long long)(u * kFixedOne); }
MESHC_HD int color_of(float col) { return (int)(fminf(fmaxf(col, 0.f), 1.f) * kColorOne + 0.5f); }

MESHC_HD float mean_coord(float o, float c, long long sum, int count) {
  return (float)((double)o + (double)c * ((double)sum / ((double)count * 65536.0)));
}
MESHC_HD float mean_color(long long sum, int count) { return (float)((double)sum / ((double)count * 65535.0)); }

}  // namespace meshc
}  // namespace mp
