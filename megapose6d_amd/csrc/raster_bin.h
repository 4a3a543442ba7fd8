// raster_bin.h -- PRIVATE interface between the rasteriser's translation units: raster_db.hip (the mesh database and the workspace
// layout), raster.hip (the binning kernel raster_bin and the batch renderer) and raster_scene.hip (the scene renderer).  Not part of the
// C-ABI: nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "mp_engine.h"
#include "raster_core.h"

struct mp_mesh_db {   // (the C-ABI's opaque handle; written by raster_db.hip only)
  int n;
  int max_verts, max_faces;
  bool any_texture;   // some mesh has uvs + a texture: raster_tiles needs its FULL instance
  mp::rc::MeshRef* d_meshes;   // device tables: MeshRef / TexRef per mesh id
  mp::rc::TexRef* d_texs;
  std::vector<mp::rc::MeshRef> h_meshes;
  std::vector<mp::rc::TexRef> h_texs;
  std::vector<void*> allocs;
};

namespace mp {

constexpr int RASTER_BIN_HDR_INTS = 4;   // per-view header: n_large, n_entries, overflow, front-orientation hint

// per-view workspace of raster_bin, in ints (every section starts 16-byte aligned):
//   [hdr HDR_INTS][tile_off n_tiles + 1][tile_off_l n_tiles + 1][list_l: cap_large piece indices][list: cap_list TileRec records of 8 ints]
// tile_off / list: the binned (small) pieces of every tile as 32-byte records; tile_off_l / list_l: the indices of the LARGE pieces
// (too big for the 32-bit edge functions or touching > LARGE_TILES tiles) per tile they can own a sample in -- recomputed from the mesh
// by the tile kernel, but only by the tiles they touch.
struct BinLayout {
  long long view_ints;
  int n_tiles, tiles_x, tiles_y, cap_list, cap_large, max_faces;
  int off_tl, off_large, off_list;   // int offsets of tile_off_l / list_l / list inside a view's block
};

// the layout raster_bin uses for this database at h x w (what mp_raster_workspace_bytes sizes per view)
BinLayout raster_bin_layout(const mp_mesh_db* db, int h, int w);

// behind the per-view blocks (batch renderer only): [4 counters: light pairs, heavy pairs, -, -][pair list: one int per (view, tile)][job
// flags: one byte per (item, tile), sized for items = views][per-view tile flags: one byte per (view, tile)].  The first n_items * n_tiles
// ints of the pair list hold both lists of raster_classify, which partition the pairs: the light ones from the start, the heavy ones from the
// far end (heavy entry k at index n_items * n_tiles - 1 - k).
inline size_t raster_job_tail_offset_ints(const BinLayout& lay, int n_views) { return ((size_t)n_views * (size_t)lay.view_ints + 3) & ~(size_t)3; }

// Enqueue raster_bin for n_views views (one workgroup each): view v = mesh d_mesh_ids[v] under pose d_TCO[v] and intrinsics d_K[v]
// (a non-finite pose or K gives empty lists), binned for `ns` samples per pixel into the view blocks of d_ws (n_views * lay.view_ints ints).
// counters (4 ints, or NULL): the light-job counters of the compacted launch form, zeroed here; view_flags (one byte per (view, tile), or
// NULL): whether the view reaches the tile, what raster_classify reads.
int raster_bin_launch(const mp_mesh_db* db, const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, int n_views, int h, int w,
                      int ns, int* d_ws, const BinLayout& lay, int* counters, unsigned char* view_flags, hipStream_t stream);

}  // namespace mp
