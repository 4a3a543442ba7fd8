// TEST SUPPORT: host emulation of the mesh clean-up kernels (megapose6d_amd/csrc/mesh_cleanup.hip), built from the same rules header
// (mesh_cleanup_core.h).  Same arguments as the C ABI, on host arrays, as plain loops: a sequential union-find with the smaller root on
// top, indices handed out as the walk meets a kept face, a referenced vertex or a used cell (no flags passes, no ranks, no scans, no
// workspace, no atomics).  Compiled with -ffp-contract=off, so the kernels are held to these results bit for bit.  Built by
// tests/support/mesh_cleanup.py; tests/mesh_cleanup_asan_main.cpp includes this file.
#include <cstdint>
#include <cstring>
#include <vector>

#include "mesh_cleanup_core.h"

using namespace mp;

namespace {

int find_root(std::vector<int32_t>& parent, int v) {
  int r = v;
  while (parent[r] != r) r = parent[r];
  while (parent[v] != r) {
    const int next = parent[v];
    parent[v] = r;
    v = next;
  }
  return r;
}

void join(std::vector<int32_t>& parent, int a, int b) {
  a = find_root(parent, a);
  b = find_root(parent, b);
  if (a == b) return;
  if (a < b) parent[b] = a; else parent[a] = b;
}

struct Clusters {
  std::vector<int32_t> vcell;      // per vertex: cell or -1
  std::vector<float> u;            // per vertex: the three grid coordinates
  std::vector<uint8_t> fkeep;
  std::vector<int32_t> cell_rank;  // per cell: output vertex or -1
  int32_t nv = 0, nf = 0, dropped = 0;
};

void walk_clusters(const float* vertices, int V, const int32_t* faces, int F, const float* o, float c, const int* g, Clusters* s) {
  const size_t cells = (size_t)g[0] * g[1] * g[2];
  s->vcell.assign((size_t)V, -1);
  s->u.assign((size_t)V * 3, 0.f);
  s->fkeep.assign((size_t)F, 0);
  s->cell_rank.assign(cells, -1);
  for (int v = 0; v < V; ++v) s->vcell[v] = meshc::cell_of(vertices + (size_t)v * 3, o, c, g, &s->u[(size_t)v * 3]);
  std::vector<uint8_t> used(cells, 0);
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    if (!meshc::face_good(t[0], t[1], t[2], V)) { ++s->dropped; continue; }
    const int ca = s->vcell[t[0]], cb = s->vcell[t[1]], cc = s->vcell[t[2]];
    if (ca < 0 || cb < 0 || cc < 0) { ++s->dropped; continue; }
    if (ca == cb || cb == cc || ca == cc) continue;
    s->fkeep[f] = 1;
    used[ca] = used[cb] = used[cc] = 1;
    ++s->nf;
  }
  for (size_t k = 0; k < cells; ++k)
    if (used[k]) s->cell_rank[k] = s->nv++;
}

bool cluster_args_ok(long long V, long long F, float ox, float oy, float oz, float c, int gx, int gy, int gz) {
  return meshc::counts_ok(V, F) && meshc::dims_ok(gx, gy, gz) && meshc::grid_ok(ox, oy, oz, c);
}

}  // namespace

extern "C" int mesh_components_emul(int V, const int32_t* faces, int F, int32_t* labels, int32_t* face_labels, int32_t* face_count, int32_t* totals) {
  if (!meshc::counts_ok(V, F) || !totals) return 1;
  if ((V && (!labels || !face_count)) || (F && (!faces || !face_labels))) return 1;
  if (V == 0 || F == 0) {   // an empty input: zero totals, every vertex its own label, every face without one
    for (int v = 0; v < V; ++v) { labels[v] = v; face_count[v] = 0; }
    for (int f = 0; f < F; ++f) face_labels[f] = -1;
    totals[0] = totals[2] = totals[3] = 0;
    totals[1] = -1;
    return 0;
  }
  std::vector<int32_t> parent((size_t)V);
  for (int v = 0; v < V; ++v) parent[v] = v;
  int32_t bad = 0;
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    if (!meshc::face_good(t[0], t[1], t[2], V)) { ++bad; continue; }
    join(parent, t[0], t[1]);
    join(parent, t[1], t[2]);
  }
  for (int v = 0; v < V; ++v) {
    labels[v] = find_root(parent, v);
    face_count[v] = 0;
  }
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    const bool good = meshc::face_good(t[0], t[1], t[2], V);
    face_labels[f] = good ? labels[t[0]] : -1;
    if (good) ++face_count[labels[t[0]]];
  }
  int32_t n = 0, best = -1, best_count = 0;
  for (int v = 0; v < V; ++v) {
    if (face_count[v] == 0) continue;
    ++n;
    if (face_count[v] > best_count) { best_count = face_count[v]; best = v; }
  }
  totals[0] = n;
  totals[1] = best;
  totals[2] = bad;
  totals[3] = 0;
  return 0;
}

extern "C" int mesh_select_count_emul(int V, const int32_t* faces, int F, const uint8_t* keep, int32_t* totals) {
  if (!meshc::counts_ok(V, F) || !totals || (F && (!faces || !keep))) return 1;
  totals[0] = totals[1] = totals[2] = 0;
  if (V == 0 || F == 0) return 0;
  std::vector<uint8_t> ref((size_t)V, 0);
  int32_t nv = 0, nf = 0, bad = 0;
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    if (!meshc::face_good(t[0], t[1], t[2], V)) { ++bad; continue; }
    if (!keep[f]) continue;
    ++nf;
    for (int k = 0; k < 3; ++k) ref[t[k]] = 1;
  }
  for (int v = 0; v < V; ++v) nv += ref[v];
  totals[0] = nv;
  totals[1] = nf;
  totals[2] = bad;
  return 0;
}

extern "C" int mesh_select_emul(const float* vertices, const float* colors, int V, const int32_t* faces, int F, const uint8_t* keep, int n_vertices,
                                int n_faces, float* out_vertices, float* out_colors, int32_t* out_faces, long long cap_vertices, long long cap_faces) {
  if (!meshc::counts_ok(V, F)) return 1;
  if (n_vertices < 0 || n_faces < 0 || cap_vertices < n_vertices || cap_faces < n_faces) return 1;
  if (V == 0 || F == 0 || (n_vertices == 0 && n_faces == 0)) return 0;
  if (!vertices || !faces || !keep || (n_vertices && (!out_vertices || (colors && !out_colors))) || (n_faces && !out_faces)) return 1;
  std::vector<int32_t> new_index((size_t)V, -1);
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    if (keep[f] && meshc::face_good(t[0], t[1], t[2], V))
      for (int k = 0; k < 3; ++k) new_index[t[k]] = 0;
  }
  int32_t nv = 0, nf = 0;
  for (int v = 0; v < V; ++v) {
    if (new_index[v] < 0) continue;
    new_index[v] = nv;
    if (nv < n_vertices) {
      std::memcpy(out_vertices + (size_t)nv * 3, vertices + (size_t)v * 3, 12);
      if (colors) std::memcpy(out_colors + (size_t)nv * 3, colors + (size_t)v * 3, 12);
    }
    ++nv;
  }
  for (int f = 0; f < F; ++f) {
    const int32_t* t = faces + (size_t)f * 3;
    if (!keep[f] || !meshc::face_good(t[0], t[1], t[2], V)) continue;
    if (nf < n_faces)
      for (int k = 0; k < 3; ++k) out_faces[(size_t)nf * 3 + k] = new_index[t[k]];
    ++nf;
  }
  return 0;
}

extern "C" int mesh_cluster_count_emul(const float* vertices, int V, const int32_t* faces, int F, float ox, float oy, float oz, float cell, int gx,
                                       int gy, int gz, int32_t* totals) {
  if (!cluster_args_ok(V, F, ox, oy, oz, cell, gx, gy, gz) || !totals || (V && !vertices) || (F && !faces)) return 1;
  const float o[3] = {ox, oy, oz};
  const int g[3] = {gx, gy, gz};
  Clusters s;
  if (V && F) walk_clusters(vertices, V, faces, F, o, cell, g, &s);
  totals[0] = s.nv;
  totals[1] = s.nf;
  totals[2] = s.dropped;
  return 0;
}

extern "C" int mesh_cluster_emul(const float* vertices, const float* colors, int V, const int32_t* faces, int F, float ox, float oy, float oz,
                                 float cell, int gx, int gy, int gz, int n_vertices, int n_faces, float* out_vertices, float* out_colors,
                                 int32_t* out_faces, long long cap_vertices, long long cap_faces) {
  if (!cluster_args_ok(V, F, ox, oy, oz, cell, gx, gy, gz)) return 1;
  if (n_vertices < 0 || n_faces < 0 || cap_vertices < n_vertices || cap_faces < n_faces) return 1;
  if (V == 0 || F == 0 || (n_vertices == 0 && n_faces == 0)) return 0;
  if (!vertices || !faces || (n_vertices && (!out_vertices || (colors && !out_colors))) || (n_faces && !out_faces)) return 1;
  const float o[3] = {ox, oy, oz};
  const int g[3] = {gx, gy, gz};
  Clusters s;
  walk_clusters(vertices, V, faces, F, o, cell, g, &s);
  std::vector<long long> sum((size_t)s.nv * 6, 0);
  std::vector<int32_t> count((size_t)s.nv, 0);
  for (int v = 0; v < V; ++v) {
    const int r = s.vcell[v] < 0 ? -1 : s.cell_rank[s.vcell[v]];
    if (r < 0) continue;
    ++count[r];
    for (int k = 0; k < 3; ++k) {
      sum[(size_t)r * 6 + k] += meshc::fixed_of(s.u[(size_t)v * 3 + k]);
      if (colors) sum[(size_t)r * 6 + 3 + k] += meshc::color_of(colors[(size_t)v * 3 + k]);
    }
  }
  for (int r = 0; r < s.nv && r < n_vertices; ++r)
    for (int k = 0; k < 3; ++k) {
      out_vertices[(size_t)r * 3 + k] = meshc::mean_coord(o[k], cell, sum[(size_t)r * 6 + k], count[r]);
      if (colors) out_colors[(size_t)r * 3 + k] = meshc::mean_color(sum[(size_t)r * 6 + 3 + k], count[r]);
    }
  int32_t nf = 0;
  for (int f = 0; f < F; ++f) {
    if (!s.fkeep[f]) continue;
    if (nf < n_faces)
      for (int k = 0; k < 3; ++k) out_faces[(size_t)nf * 3 + k] = s.cell_rank[s.vcell[faces[(size_t)f * 3 + k]]];
    ++nf;
  }
  return 0;
}

extern "C" void mesh_cleanup_emul_limits(long long* v) {
  v[0] = meshc::kMaxCount;
  v[1] = meshc::kMaxDim;
  v[2] = meshc::kMaxCells;
}
