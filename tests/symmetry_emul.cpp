// TEST SUPPORT: host emulation of the symmetry kernels (megapose6d_amd/csrc/symmetry.hip), built from the same rules header
// (symmetry_core.h).  Same arguments as the C ABI, on host arrays: the candidates one after the other (in the order the caller gives, to
// show that the order does not matter), each as its workgroup does it -- block by block, lane by lane, tile by tile, with the screen's two
// early outs in mode 0 -- then a plain fold of the lanes.  No LDS, no shuffles.  Built by tests/support/symmetry.py.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "symmetry_core.h"

using namespace mp;
using symm::Worst;

namespace {

struct Obj {
  int n_vert, n_face, n_test;
  const float* V;
  const int32_t* F;
  const float* T;
  float tol2;
};

// triangle f of the object as the kernel stages it: A, B - A, C - A
void triangle(const Obj& o, int f, float* t) {
  const float* A = o.V + 3 * (size_t)o.F[3 * f];
  const float* B = o.V + 3 * (size_t)o.F[3 * f + 1];
  const float* C = o.V + 3 * (size_t)o.F[3 * f + 2];
  for (int a = 0; a < 3; ++a) {
    t[a] = A[a];
    t[3 + a] = B[a] - A[a];
    t[6 + a] = C[a] - A[a];
  }
}

float dist2(const Obj& o, int f, const float* g) {
  float t[9];
  triangle(o, f, t);
  return symm::tri_dist2(t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8], symm::is_sliver(t[3], t[4], t[5], t[6], t[7], t[8]), g[0], g[1], g[2]);
}

// the screen: 1 = accepted
int screen(const Obj& o, const float* R, const float* c, int tile) {
  for (int i0 = 0; i0 < o.n_test; i0 += symm::kBlock) {
    bool any = false;   // a lane of this block still searches after the last tile
    for (int lane = 0; lane < symm::kBlock; ++lane) {
      const int i = i0 + lane;
      if (i >= o.n_test) continue;
      float g[3];
      symm::apply(R, c, o.T[3 * (size_t)i], o.T[3 * (size_t)i + 1], o.T[3 * (size_t)i + 2], &g[0], &g[1], &g[2]);
      bool searching = true;
      for (int f0 = 0; f0 < o.n_face && searching; f0 += tile) {
        const int n_stage = o.n_face - f0 < tile ? o.n_face - f0 : tile;
        for (int t = 0; t < n_stage; ++t)
          if (dist2(o, f0 + t, g) <= o.tol2) {
            searching = false;
            break;
          }
      }
      any = any || searching;
    }
    if (any) return 0;
  }
  return 1;
}

Worst measure(const Obj& o, const float* R, const float* c, int tile) {
  Worst all = symm::none();
  for (int lane = 0; lane < symm::kBlock; ++lane) {   // a lane's points in ascending order, then the fold of the lanes
    Worst mine = symm::none();
    for (int i = lane; i < o.n_test; i += symm::kBlock) {
      float g[3];
      symm::apply(R, c, o.T[3 * (size_t)i], o.T[3 * (size_t)i + 1], o.T[3 * (size_t)i + 2], &g[0], &g[1], &g[2]);
      float best = INFINITY;
      for (int f0 = 0; f0 < o.n_face; f0 += tile) {
        const int n_stage = o.n_face - f0 < tile ? o.n_face - f0 : tile;
        for (int t = 0; t < n_stage; ++t) symm::lane_min(dist2(o, f0 + t, g), &best);
      }
      const Worst w{best, i};
      if (symm::worse(w, mine)) mine = w;
    }
    if (symm::worse(mine, all)) all = mine;
  }
  return all;
}

}  // namespace

// 0, or the number of the first rule of mp_symmetry_check that the arguments break
extern "C" int symmetry_emul_check(const int32_t* faces, const int32_t* vert_off, const int32_t* face_off, const int32_t* test_off,
                                   const int32_t* cand_off, const float* tol, int n_obj, int tile, int mode) {
  if (n_obj < 1) return 1;
  if (mode != 0 && mode != 1) return 2;
  if (!symm::tile_ok(tile)) return 3;
  if (vert_off[0] != 0 || face_off[0] != 0 || test_off[0] != 0 || cand_off[0] != 0) return 4;
  for (int o = 0; o < n_obj; ++o) {
    const long long n_vert = (long long)vert_off[o + 1] - vert_off[o];
    if (n_vert < 1) return 5;
    if (face_off[o + 1] <= face_off[o]) return 6;
    if (test_off[o + 1] <= test_off[o]) return 7;
    if (cand_off[o + 1] < cand_off[o]) return 8;
    if (!std::isfinite(tol[o]) || tol[o] < 0.0f) return 9;
    for (long long f = 3LL * face_off[o]; f < 3LL * face_off[o + 1]; ++f)
      if (faces[f] < 0 || faces[f] >= n_vert) return 10;
  }
  if (cand_off[n_obj] > symm::kMaxCandidates) return 11;
  return 0;
}

extern "C" int symmetry_emul(const float* vertices, const int32_t* faces, const float* tests, const float* cand_R, const float* centers,
                             const int32_t* vert_off, const int32_t* face_off, const int32_t* test_off, const int32_t* cand_off,
                             const float* tol, int n_obj, int tile_arg, int mode, const int64_t* cand_order /*a permutation, or NULL*/,
                             uint8_t* accept, float* dev2, int32_t* worst) {
  const int rc = symmetry_emul_check(faces, vert_off, face_off, test_off, cand_off, tol, n_obj, tile_arg, mode);
  if (rc) return rc;
  const int tile = symm::tile_of(tile_arg), n_cand = cand_off[n_obj];
  for (int k = 0; k < n_cand; ++k) {
    const int cand = cand_order ? (int)cand_order[k] : k;
    int obj = 0;
    while (cand_off[obj + 1] <= cand) ++obj;
    Obj o;
    o.n_vert = vert_off[obj + 1] - vert_off[obj];
    o.n_face = face_off[obj + 1] - face_off[obj];
    o.n_test = test_off[obj + 1] - test_off[obj];
    o.V = vertices + 3 * (size_t)vert_off[obj];
    o.F = faces + 3 * (size_t)face_off[obj];
    o.T = tests + 3 * (size_t)test_off[obj];
    o.tol2 = tol[obj] * tol[obj];
    const float* R = cand_R + 9 * (size_t)cand;
    const float* c = centers + 3 * (size_t)obj;
    if (mode == 0) {
      accept[cand] = (uint8_t)screen(o, R, c, tile);
      if (!accept[cand]) {
        dev2[cand] = NAN;
        worst[cand] = -1;
        continue;
      }
    }
    const Worst w = measure(o, R, c, tile);
    dev2[cand] = w.d2;
    worst[cand] = w.i == symm::kNone ? -1 : w.i;
    if (mode != 0) accept[cand] = symm::accepted(w.d2, o.tol2) ? 1 : 0;
  }
  return 0;
}

// the squared distance of p to the triangle a b c, as the kernel takes it
extern "C" float symmetry_emul_tri_dist2(const float* a, const float* b, const float* c, const float* p) {
  const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  return symm::tri_dist2(a[0], a[1], a[2], e1[0], e1[1], e1[2], e2[0], e2[1], e2[2], symm::is_sliver(e1[0], e1[1], e1[2], e2[0], e2[1], e2[2]), p[0],
                         p[1], p[2]);
}

extern "C" void symmetry_emul_limits(int* v) {
  v[0] = symm::kBlock;
  v[1] = symm::kTileStep;
  v[2] = symm::kMaxTile;
  v[3] = symm::kDefaultTile;
  v[4] = symm::kMaxCandidates;
}
