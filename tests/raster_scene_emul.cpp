// tests/raster_scene_emul.cpp -- HOST emulation of the scene rasteriser (megapose6d_amd/csrc/raster_scene.hip), TEST INFRASTRUCTURE ONLY.
// The same algorithm in the same order, serially: the camera's K next to every object, raster_bin's binning of every (camera, object)
// view (raster_emul.cpp's bin_view: tile lists, the large list, the overflow fallback), then per (camera, 8x8 tile) one depth state per
// sample across all of the camera's objects (raster_scene_core.h: scene_cover) and the per-pixel shading + resolve of the device code
// (scene_shade_resolve).  The CPU tests compare it with the independent oracle (oracle/raster.c); the -m gpu tests compare the kernel
// with it bit for bit.
// Build: g++ -O2 -std=c++17 -ffp-contract=off -mfma -shared -fPIC -I megapose6d_amd/csrc -I tests tests/raster_scene_emul.cpp
#include "raster_emul.cpp"
#include "raster_scene_core.h"

namespace {

template <int NS>
void render_scene(const MeshRef* meshes, const TexRef* texs, int n_cams, const int32_t* obj_off, const int32_t* mesh_ids, const float* TCO,
                  const float* K, const float* radius, const Lights* lights_in, int h, int w, uint32_t flags, float* out, long long stride_v,
                  long long stride_y, long long stride_x, int c_rgb, int c_normals, int c_depth, int32_t* inst, int cap_list, int reverse_lists) {
  const bool do_norm = (flags & 1u) && c_normals >= 0, do_depth = (flags & 2u) && c_depth >= 0, gl_eye = (flags & 4u) != 0;
  if (!do_norm) c_normals = -1;
  if (!do_depth) c_depth = -1;
  const int tiles_x = (w + TILE - 1) / TILE, tiles_y = (h + TILE - 1) / TILE;
  const int n_obj = obj_off[n_cams];
  std::vector<float> K_obj((size_t)9 * n_obj);
  std::vector<Lights> lights(lights_in, lights_in + n_obj);
  for (int c = 0; c < n_cams; ++c)
    for (int o = obj_off[c]; o < obj_off[c + 1]; ++o) std::copy(K + 9 * c, K + 9 * c + 9, K_obj.begin() + 9 * o);
  for (Lights& L : lights) L.n_point = imin(imax(L.n_point, 0), 8);
  std::vector<Lists> lists(n_obj);
  for (int o = 0; o < n_obj; ++o) {
    const MeshRef& m = meshes[mesh_ids[o]];
    lists[o] = bin_view(m, TCO + 16 * o, K_obj.data() + 9 * o, h, w, NS, cap_list > 0 ? cap_list : 3 * m.n_faces + 2048);
    Lists& L = lists[o];
    if (reverse_lists) {   // the fill order of the device lists is not deterministic: the result must not depend on it
      std::reverse(L.large.begin(), L.large.end());
      for (int t = 0; t + 1 < (int)L.tile_off.size() && !L.overflow; ++t) std::reverse(L.list.begin() + L.tile_off[t], L.list.begin() + L.tile_off[t + 1]);
    }
  }
  SceneObjects so;
  so.meshes = meshes; so.texs = texs; so.mesh_ids = mesh_ids; so.TCO = TCO; so.K = K_obj.data(); so.lights = lights.data();
  for (int c = 0; c < n_cams; ++c) {
    const int o0 = obj_off[c], o1 = obj_off[c + 1];
    for (int ty = 0; ty < tiles_y; ++ty)
      for (int tx = 0; tx < tiles_x; ++tx) {
        const int tile = ty * tiles_x + tx, tile_x0 = tx * TILE, tile_y0 = ty * TILE;
        unsigned long long key[64][NS];
        for (int l = 0; l < 64; ++l)
          for (int s = 0; s < NS; ++s) key[l][s] = 0ull;
        for (int o = o0; o < o1; ++o) {
          const Lists& L = lists[o];
          const MeshRef& m = meshes[mesh_ids[o]];
          const float* T = TCO + 16 * o;
          const float* Kv = K_obj.data() + 9 * o;
          std::vector<Piece> pieces;   // the tile's binned records, then the large pieces that can own a sample in it (all pieces on overflow)
          if (L.overflow) {
            for (int i = 0; i < 2 * m.n_faces; ++i) { Piece q; piece_from_index<false>(m, T, Kv, i, q); pieces.push_back(q); }
          } else {
            for (int e = L.tile_off[tile]; e < L.tile_off[tile + 1]; ++e) { Piece q; unpack_tile_rec(L.list[e], tile_x0, tile_y0, q); pieces.push_back(q); }
            for (int idx : L.large) {
              Piece q;
              piece_from_index<false>(m, T, Kv, idx, q);
              if (q.id >= 0 && tile_touched(tile_test_setup(q, NS), tx, ty)) pieces.push_back(q);
            }
          }
          for (const Piece& p : pieces) {
            if (p.id < 0) continue;
            int x0, y0, x1, y1;
            piece_pixel_bbox(p, NS, w, h, x0, y0, x1, y1);
            if (imax(x0, tile_x0) > imin(x1, tile_x0 + TILE - 1) || imax(y0, tile_y0) > imin(y1, tile_y0 + TILE - 1)) continue;
            for (int l = 0; l < 64; ++l) scene_cover<NS>(p, o - o0, tile_x0, tile_y0, tile_x0 + (l & 7), tile_y0 + (l >> 3), key[l]);
          }
        }
        for (int l = 0; l < 64; ++l) {
          const int px = tile_x0 + (l & 7), py = tile_y0 + (l >> 3);
          if (px >= w || py >= h) continue;
          float rgb[3], nrm[3], depth;
          int slot;
          scene_shade_resolve<NS>(so, o0, radius[c], gl_eye, c_normals >= 0, key[l], px, py, rgb, nrm, depth, slot);
          float* dst = out + (size_t)c * stride_v + (size_t)py * stride_y + (size_t)px * stride_x;
          if (c_rgb >= 0) for (int k = 0; k < 3; ++k) dst[c_rgb + k] = rgb[k];
          if (c_normals >= 0) for (int k = 0; k < 3; ++k) dst[c_normals + k] = nrm[k];
          if (c_depth >= 0) dst[c_depth] = depth;
          if (inst) inst[((size_t)c * h + py) * w + px] = slot;
        }
      }
  }
}

}  // namespace

// meshes: arrays of n_meshes pointers / sizes (uvs / texels NULL = vertex-coloured); lights: n_obj object-frame rigs (mp_lights layout)
extern "C" void raster_scene_emul_render(int n_meshes, const float* const* verts, const float* const* normals, const float* const* colors,
                                         const int32_t* const* faces, const int* n_verts, const int* n_faces, const float* const* uvs,
                                         const uint32_t* const* texels, const int* tex_w, const int* tex_h, const int* tex_levels, int n_cams,
                                         const int32_t* obj_off, const int32_t* mesh_ids, const float* TCO, const float* K, const float* radius,
                                         const Lights* lights, int h, int w, uint32_t flags, float* out, long long stride_v, long long stride_y,
                                         long long stride_x, int c_rgb, int c_normals, int c_depth, int32_t* inst, int cap_list, int reverse_lists) {
  std::vector<MeshRef> ms(n_meshes);
  std::vector<TexRef> txs(n_meshes);
  for (int i = 0; i < n_meshes; ++i) {
    MeshRef& m = ms[i];
    m.verts = verts[i]; m.normals = normals[i]; m.colors = colors[i]; m.faces = faces[i]; m.n_verts = n_verts[i]; m.n_faces = n_faces[i];
    m.radius = 0.f;   // (the scene radius replaces it)
    m.uvs = (uvs[i] && texels[i]) ? uvs[i] : nullptr;
    TexRef& tx = txs[i];
    memset(&tx, 0, sizeof(tx));
    tx.texels = texels[i]; tx.tex_w = tex_w[i]; tx.tex_h = tex_h[i]; tx.tex_levels = tex_levels[i];
    int off = 0;
    for (int l = 0; l < tex_levels[i] && l < MP_TEX_MAX_LEVELS; ++l) {
      tx.tex_off[l] = off;
      off += std::max(1, tex_w[i] >> l) * std::max(1, tex_h[i] >> l);
    }
  }
  if (flags & 16u)
    render_scene<4>(ms.data(), txs.data(), n_cams, obj_off, mesh_ids, TCO, K, radius, lights, h, w, flags, out, stride_v, stride_y, stride_x, c_rgb,
                    c_normals, c_depth, inst, cap_list, reverse_lists);
  else
    render_scene<1>(ms.data(), txs.data(), n_cams, obj_off, mesh_ids, TCO, K, radius, lights, h, w, flags, out, stride_v, stride_y, stride_x, c_rgb,
                    c_normals, c_depth, inst, cap_list, reverse_lists);
}
