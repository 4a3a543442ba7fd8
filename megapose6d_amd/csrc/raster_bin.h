// raster_bin.h -- PRIVATE interface between raster.hip (which owns the mesh database and the binning kernel raster_bin) and the other
// rasteriser translation units (raster_scene.hip).  Not part of the C-ABI: nothing here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mp_engine.h"
#include "raster_core.h"

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

// device tables of the database: MeshRef / TexRef per mesh id, and whether some mesh carries a texture
const rc::MeshRef* raster_db_meshes(const mp_mesh_db* db);
const rc::TexRef* raster_db_textures(const mp_mesh_db* db);

// Enqueue raster_bin for n_views views (one workgroup each): view v = mesh d_mesh_ids[v] under pose d_TCO[v] and intrinsics d_K[v]
// (a non-finite pose or K gives empty lists), binned for `ns` samples per pixel into the view blocks of d_ws (n_views * lay.view_ints ints).
// No light-job counters, no per-view tile flags.
int raster_bin_launch(const mp_mesh_db* db, const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, int n_views, int h, int w,
                      int ns, int* d_ws, const BinLayout& lay, hipStream_t stream);

}  // namespace mp
