// raster_scene_core.h -- the per-pixel arithmetic of the multi-object scene renderer (raster_scene.hip), shared with its host
// emulation (tests/raster_scene_emul.cpp).  It only composes the single-object contract of raster_core.h: coverage and depth per
// sample with the same edge functions and depth rule, one shading per (pixel, winning piece) with rc::shade, the same 8-bit
// multisample resolve.  What is new is the depth state: it is kept across ALL objects of a camera, and a sample's winner is the pair
// (object slot, piece id).  Contract: include/mp_engine.h, mp_raster_render_scene.
#pragma once
#include "raster_core.h"

namespace mp {
namespace rc {

constexpr int SCENE_MAX_OBJECTS = 256;   // objects per camera: the slot takes 8 bits of the scene key

// 64-bit scene key of a covered sample: [63:32] wsum bits (nearer = larger), [30:23] 255 - object slot, [22:0] 0x7FFFFF - piece id;
// bit 31 stays 0.  The larger key wins, so on exactly equal depth the object listed first wins (draw order under a less-than depth
// test) and within one object the lower piece id wins, as in the single-object rule.  0 = empty (wsum > 0 inside the depth range).
// The maximum over a set of keys does not depend on the order they are visited in.
MP_HD unsigned long long scene_key(float wsum, int slot, int id) {
  uint32_t wb;
  memcpy(&wb, &wsum, 4);
  return ((unsigned long long)wb << 32) | ((unsigned long long)(255u - (uint32_t)slot) << 23) | (unsigned long long)(0x7FFFFFu - (uint32_t)id);
}
MP_HD float scene_key_wsum(unsigned long long key) {
  const uint32_t wb = (uint32_t)(key >> 32);
  float f;
  memcpy(&f, &wb, 4);
  return f;
}
MP_HD int scene_key_slot(unsigned long long key) { return key ? 255 - (int)((key >> 23) & 255u) : -1; }
MP_HD int scene_key_id(unsigned long long key) { return key ? 0x7FFFFF - (int)(key & 0x7FFFFFu) : -1; }
MP_HD uint32_t scene_key_owner(unsigned long long key) { return (uint32_t)(key & 0x7FFFFFFFu); }   // (slot, id) of the winner

// one piece of the object in `slot` against the NS samples of pixel (px, py) of the tile at (tile_x0, tile_y0): every covered sample
// inside the depth range keeps the larger key.  The 32-bit edge functions where the piece is small for the tile, else the 64-bit form
// (the same integers, raster_core.h).
template <int NS>
MP_HD void scene_cover(const Piece& p, int slot, int tile_x0, int tile_y0, int px, int py, unsigned long long (&key)[NS]) {
  auto emit = [&](int s, float wsum) {
    const unsigned long long k = scene_key(wsum, slot, p.id);
    if (k > key[s]) key[s] = k;
  };
  if (piece_is_small(p, tile_x0, tile_y0)) {
    Edges32 e;
    piece_edges32(p, e);
    cover_pixel32<NS>(p, e, px, py, emit);
  } else {
    Edges e;
    piece_edges(p, e);
    cover_pixel64<NS>(p, e, px, py, emit);
  }
}

// What one scene object needs for shading: the camera's objects are o0 .. o0 + n - 1 of these arrays.
struct SceneObjects {
  const MeshRef* meshes;    // per mesh id
  const TexRef* texs;       // per mesh id
  const int32_t* mesh_ids;  // per object
  const float* TCO;         // per object [4][4]
  const float* K;           // per object [3][3] (the camera's K)
  const Lights* lights;     // per object, rig in the object's frame: position = dir * 10 * scene radius + offset
};

// Shading + resolve of pixel (px, py) from the final keys of its NS samples: one rc::shade per (pixel, distinct winner) with the
// winner's mesh (radius replaced by the scene radius), texture, pose and light rig; the 8-bit values of the samples are averaged.
// Outputs: rgb / nrm = resolved channels (0 = background), depth = metric z of sample 0 (0 = background), slot = object slot of
// sample 0's winner (-1 = background).
template <int NS>
MP_HD void scene_shade_resolve(const SceneObjects& so, int o0, float scene_radius, bool gl_eye, bool want_normals,
                               const unsigned long long (&key)[NS], int px, int py, float rgb[3], float nrm[3], float& depth, int& slot) {
  unsigned fresh = 0;   // samples whose winner no earlier sample of the pixel holds: one shading each
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    bool f = key[s] != 0ull;
#pragma unroll
    for (int k = 0; k < s; ++k) f = f && !(key[k] != 0ull && scene_key_owner(key[k]) == scene_key_owner(key[s]));
    fresh |= (f ? 1u : 0u) << s;
  }
  uint32_t qc[NS], qn[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) qc[s] = qn[s] = 0u;
  for (unsigned m = fresh; m != 0u; m &= m - 1u) {   // (not unrolled: one copy of the shading code)
    const int s = __builtin_ctz(m);
    unsigned long long k = key[0];
#pragma unroll
    for (int j = 1; j < NS; ++j) k = s == j ? key[j] : k;
    const int o = o0 + scene_key_slot(k), id = scene_key_id(k);
    const int mid = so.mesh_ids[o];
    MeshRef mesh = so.meshes[mid];
    mesh.radius = scene_radius;
    const TexRef* tex = mesh.uvs ? &so.texs[mid] : nullptr;
    const float* T = so.TCO + (size_t)o * 16;
    Piece pf;
    piece_from_index<true>(mesh, T, so.K + (size_t)o * 9, id, pf);
    float c255[3], n255[3];
    shade<true>(mesh, tex, so.lights[o], T, gl_eye, want_normals, pf, px, py, c255, n255);
    const uint32_t c = (uint32_t)q255(c255[0]) | ((uint32_t)q255(c255[1]) << 8) | ((uint32_t)q255(c255[2]) << 16);
    const uint32_t n = (uint32_t)q255(n255[0]) | ((uint32_t)q255(n255[1]) << 8) | ((uint32_t)q255(n255[2]) << 16);
#pragma unroll
    for (int j = 0; j < NS; ++j) {
      qc[j] = s == j ? c : qc[j];
      qn[j] = s == j ? n : qn[j];
    }
  }
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (key[s] == 0ull) continue;
    uint32_t c = qc[s], n = qn[s];
#pragma unroll
    for (int k = s - 1; k >= 0; --k)   // ends at the first sample holding this winner (the one that was shaded)
      if (key[k] != 0ull && scene_key_owner(key[k]) == scene_key_owner(key[s])) { c = qc[k]; n = qn[k]; }
    acc[0] += (float)(c & 255u); acc[1] += (float)((c >> 8) & 255u); acc[2] += (float)((c >> 16) & 255u);
    acc[3] += (float)(n & 255u); acc[4] += (float)((n >> 8) & 255u); acc[5] += (float)((n >> 16) & 255u);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    rgb[c] = resolve_channel(acc[c], NS, false);
    nrm[c] = resolve_channel(acc[3 + c], NS, false);
  }
  depth = key[0] ? 1.0f / scene_key_wsum(key[0]) : 0.f;
  slot = scene_key_slot(key[0]);
}

}  // namespace rc
}  // namespace mp
