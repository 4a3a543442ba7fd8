// raster_db.hip -- the rasteriser's mesh database (host code only): the meshes and textures of a dataset uploaded once, the device tables
// (rc::MeshRef / rc::TexRef per mesh id) the raster kernels index, and the layout and size of the workspace raster_bin fills.  Contract:
// include/mp_engine.h (mp_mesh_db_*, mp_raster_workspace_bytes); private interface to the kernels' translation units: raster_bin.h.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "raster_bin.h"

using namespace mp;

typedef rc::MeshRef MeshDev;
typedef rc::TexRef TexDev;

extern "C" int mp_mesh_db_create(const mp_mesh_desc* hm, int n, mp_mesh_db** out) {
  MP_REQUIRE(hm && out && n > 0, "mp_mesh_db_create: bad arguments");
  mp_mesh_db* db = new mp_mesh_db();
  db->n = n;
  db->max_verts = db->max_faces = 0;
  db->any_texture = false;
  db->d_meshes = nullptr;
  db->d_texs = nullptr;
  for (int i = 0; i < n; ++i) {
    const mp_mesh_desc& d = hm[i];
    MP_REQUIRE(d.h_vertices && d.h_normals && d.h_colors && d.h_faces && d.n_vertices > 0 && d.n_faces > 0,
               "mp_mesh_db_create: mesh %d incomplete", i);
    MP_REQUIRE(d.n_faces < (1 << 22), "mp_mesh_db_create: mesh %d has %d faces (limit 4 194 303: piece ids are packed in 24 bits)", i, d.n_faces);
    for (int f = 0; f < 3 * d.n_faces; ++f)
      MP_REQUIRE(d.h_faces[f] >= 0 && d.h_faces[f] < d.n_vertices, "mp_mesh_db_create: mesh %d face index out of range", i);
    MeshDev m;
    float *dv, *dn, *dc;
    int32_t* df;
    const size_t vb = (size_t)d.n_vertices * 3 * sizeof(float);
    MP_CHECK_HIP(hipMalloc(&dv, vb));
    MP_CHECK_HIP(hipMalloc(&dn, vb));
    MP_CHECK_HIP(hipMalloc(&dc, vb));
    MP_CHECK_HIP(hipMalloc(&df, (size_t)d.n_faces * 3 * sizeof(int32_t)));
    MP_CHECK_HIP(hipMemcpy(dv, d.h_vertices, vb, hipMemcpyHostToDevice));
    MP_CHECK_HIP(hipMemcpy(dn, d.h_normals, vb, hipMemcpyHostToDevice));
    MP_CHECK_HIP(hipMemcpy(dc, d.h_colors, vb, hipMemcpyHostToDevice));
    MP_CHECK_HIP(hipMemcpy(df, d.h_faces, (size_t)d.n_faces * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
    db->allocs.push_back(dv); db->allocs.push_back(dn); db->allocs.push_back(dc); db->allocs.push_back(df);
    m.verts = dv; m.normals = dn; m.colors = dc; m.faces = df;
    m.n_verts = d.n_vertices; m.n_faces = d.n_faces;
    m.uvs = nullptr;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int v = 0; v < d.n_vertices; ++v)
      for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(lo[k], d.h_vertices[3 * v + k]);
        hi[k] = fmaxf(hi[k], d.h_vertices[3 * v + k]);
      }
    float center[3];
    for (int k = 0; k < 3; ++k) center[k] = 0.5f * (lo[k] + hi[k]);
    float r2 = 0.f;
    for (int v = 0; v < d.n_vertices; ++v) {
      float s = 0.f;
      for (int k = 0; k < 3; ++k) {
        const float dd = d.h_vertices[3 * v + k] - center[k];
        s += dd * dd;
      }
      r2 = fmaxf(r2, s);
    }
    m.radius = sqrtf(r2);
    db->h_meshes.push_back(m);
    db->max_verts = std::max(db->max_verts, d.n_vertices);
    db->max_faces = std::max(db->max_faces, d.n_faces);
  }
  MP_CHECK_HIP(hipMalloc(&db->d_meshes, n * sizeof(MeshDev)));
  MP_CHECK_HIP(hipMemcpy(db->d_meshes, db->h_meshes.data(), n * sizeof(MeshDev), hipMemcpyHostToDevice));
  db->h_texs.assign(n, TexDev{});
  MP_CHECK_HIP(hipMalloc(&db->d_texs, n * sizeof(TexDev)));
  MP_CHECK_HIP(hipMemcpy(db->d_texs, db->h_texs.data(), n * sizeof(TexDev), hipMemcpyHostToDevice));
  *out = db;
  return MP_OK;
}

extern "C" int mp_mesh_db_set_texture(mp_mesh_db* db, int mesh_id, const float* h_uvs, const uint32_t* h_texels, int tex_w, int tex_h,
                                      int n_levels) {
  MP_REQUIRE(db && mesh_id >= 0 && mesh_id < db->n && h_uvs && h_texels, "mp_mesh_db_set_texture: bad arguments");
  MP_REQUIRE(tex_w > 0 && tex_h > 0 && tex_w <= 16384 && tex_h <= 16384 && n_levels >= 1 && n_levels <= MP_TEX_MAX_LEVELS,
             "mp_mesh_db_set_texture: bad texture size %dx%d / %d levels", tex_w, tex_h, n_levels);
  MeshDev& m = db->h_meshes[mesh_id];
  TexDev& tx = db->h_texs[mesh_id];
  size_t total = 0;
  for (int l = 0; l < n_levels; ++l) {
    tx.tex_off[l] = (int)total;
    total += (size_t)std::max(1, tex_w >> l) * std::max(1, tex_h >> l);
  }
  float* duv;
  uint32_t* dtex;
  MP_CHECK_HIP(hipMalloc(&duv, (size_t)m.n_faces * 6 * sizeof(float)));
  MP_CHECK_HIP(hipMalloc(&dtex, total * sizeof(uint32_t)));
  MP_CHECK_HIP(hipMemcpy(duv, h_uvs, (size_t)m.n_faces * 6 * sizeof(float), hipMemcpyHostToDevice));
  MP_CHECK_HIP(hipMemcpy(dtex, h_texels, total * sizeof(uint32_t), hipMemcpyHostToDevice));
  db->allocs.push_back(duv); db->allocs.push_back(dtex);
  m.uvs = duv;
  db->any_texture = true;
  tx.texels = dtex; tx.tex_w = tex_w; tx.tex_h = tex_h; tx.tex_levels = n_levels;
  MP_CHECK_HIP(hipMemcpy(db->d_texs + mesh_id, &tx, sizeof(TexDev), hipMemcpyHostToDevice));
  MP_CHECK_HIP(hipMemcpy(db->d_meshes + mesh_id, &m, sizeof(MeshDev), hipMemcpyHostToDevice));
  return MP_OK;
}

extern "C" int mp_mesh_db_destroy(mp_mesh_db* db) {
  if (!db) return MP_OK;
  for (void* p : db->allocs) (void)hipFree(p);
  if (db->d_meshes) (void)hipFree(db->d_meshes);
  if (db->d_texs) (void)hipFree(db->d_texs);
  delete db;
  return MP_OK;
}

extern "C" int mp_mesh_db_max_vertices(const mp_mesh_db* db) { return db ? db->max_verts : 0; }
extern "C" float mp_mesh_db_radius(const mp_mesh_db* db, int i) {
  return (db && i >= 0 && i < db->n) ? db->h_meshes[i].radius : 0.f;
}

namespace mp {

BinLayout raster_bin_layout(const mp_mesh_db* db, int h, int w) {
  BinLayout lay;
  lay.tiles_x = ceil_div(w, rc::TILE);
  lay.tiles_y = ceil_div(h, rc::TILE);
  lay.n_tiles = lay.tiles_x * lay.tiles_y;
  lay.max_faces = db->max_faces;
  lay.cap_list = 3 * db->max_faces + 2048;
  lay.cap_large = 4 * db->max_faces + 4096;
  lay.off_tl = (RASTER_BIN_HDR_INTS + lay.n_tiles + 1 + 3) & ~3;
  lay.off_large = (lay.off_tl + lay.n_tiles + 1 + 3) & ~3;
  lay.off_list = (lay.off_large + lay.cap_large + 3) & ~3;
  lay.view_ints = (long long)lay.off_list + (long long)lay.cap_list * (long long)(sizeof(rc::TileRec) / sizeof(int));
  return lay;
}

}  // namespace mp

extern "C" size_t mp_raster_workspace_bytes(const mp_mesh_db* db, int n_views, int h, int w) {
  if (!db || n_views <= 0 || h <= 0 || w <= 0) return 0;
  const BinLayout lay = raster_bin_layout(db, h, w);
  const size_t pairs = (size_t)n_views * lay.n_tiles;
  return (raster_job_tail_offset_ints(lay, n_views) + 4 + pairs) * sizeof(int) + 2 * ((pairs + 15) & ~(size_t)15);   // + job flags + per-view tile flags
}
