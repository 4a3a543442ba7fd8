// TEST SUPPORT: host emulation of the texture-atlas kernels (megapose6d_amd/csrc/texture_bake.hip), built from the same rules header
// (texture_bake_core.h).  Same arguments as the C ABI, on host arrays, as plain loops: texels in row order, each one loading its own
// triangle, views in ascending order (no tiles, no staging).  Compiled with -ffp-contract=off, so the kernels are held to these results
// byte for byte.  Built by tests/support/texture_bake.py.
#include <cstdint>

#include "texture_bake_core.h"

using namespace mp;

extern "C" int texture_atlas_block_emul(long long n_triangles, int size) { return texbake::atlas_block(n_triangles, size); }

extern "C" int texture_atlas_uvs_emul(int n_triangles, int size, float* uvs) {
  if (n_triangles < 1 || n_triangles > texbake::kMaxCount || !texbake::size_ok(size) || !uvs) return 1;
  const int B = texbake::atlas_block(n_triangles, size);
  if (B == 0) return 1;
  for (int t = 0; t < n_triangles; ++t)
    for (int k = 0; k < 3; ++k) texbake::corner_uv(t, k, size, B, uvs + 6 * (size_t)t + 2 * k, uvs + 6 * (size_t)t + 2 * k + 1);
  return 0;
}

extern "C" int texture_bake_emul(const float* vertices, int n_vertices, const int32_t* faces, int n_triangles, const float* colors, const float* depth,
                                 const uint8_t* masks, const uint8_t* rgb, const float* K, const float* TCO, int tco_floats, int n, int h, int w,
                                 int size, float depth_tol, float cos_min, float z_min, int best_view, uint8_t* texels, uint8_t* seen) {
  if (n_triangles < 1 || n_triangles > texbake::kMaxCount || n_vertices < 0 || n_vertices > texbake::kMaxCount || !texbake::size_ok(size)) return 1;
  const int B = texbake::atlas_block(n_triangles, size);
  if (B == 0 || !texbake::params_ok(depth_tol, cos_min, z_min)) return 1;
  if (n < 0 || (tco_floats != 12 && tco_floats != 16) || (n > 0 && !tsdf::frame_ok(h, w))) return 1;
  if (!faces || !texels || !seen || (!vertices && n_vertices) || (n > 0 && (!depth || !rgb || !K || !TCO))) return 1;
  const size_t hw = n ? (size_t)h * w : 0;
  const float cos_min2 = cos_min * cos_min;
  const int side = size / B;
  uint32_t* out = (uint32_t*)texels;
  for (int gj = 0; gj < size; ++gj)
    for (int gi = 0; gi < size; ++gi) {
      const size_t at = (size_t)gj * size + gi;
      float a, b;
      const int upper = texbake::chart_point(B, gi % B, gj % B, &a, &b);
      const long long t = 2LL * ((long long)(gj / B) * side + gi / B) + upper;
      if (t >= n_triangles) {
        out[at] = 0u;
        seen[at] = 0;
        continue;
      }
      float tri[texbake::kTriFloats];
      const int flags = texbake::load_tri(vertices, n_vertices, faces, (int)t, colors, tri);
      texbake::Accum acc = texbake::accum_init();
      if ((flags & texbake::kTriIndexed) && (flags & texbake::kTriFinite)) {
        float p[3];
        texbake::surface_point(tri, a, b, p);
        for (int q = 0; q < n; ++q) {
          float view[tsdf::kViewFloats];
          if (!tsdf::load_view(K + (size_t)q * 9, TCO + (size_t)q * tco_floats, view)) continue;
          acc = texbake::accumulate(acc, texbake::visit(p, tri, view, depth + q * hw, masks ? masks + q * hw : nullptr, rgb + q * hw * 3, h, w,
                                                        depth_tol, cos_min2, z_min),
                                    best_view != 0);
        }
      }
      out[at] = texbake::finish(acc, tri, a, b, best_view != 0, &seen[at]);
    }
  return 0;
}

extern "C" void texture_bake_emul_limits(long long* v) {
  v[0] = texbake::kMinSize;
  v[1] = texbake::kMaxSize;
  v[2] = texbake::kMinBlock;
  v[3] = texbake::kMaxBlock;
  v[4] = texbake::kMaxCount;
}
