// texture_bake.hip -- the device side of giving a reconstructed mesh a texture: every triangle gets a chart in a square atlas, every
// texel of a chart gathers its colour from the posed colour + depth views that see its surface point.
//
// The rules are texture_bake_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Every float
// of a texel is produced by one lane from those rules, so no grid or block size can change a result.  No atomics, no workgroup waits on
// another, no workspace.
//
//   texture_uvs_kernel   one lane per triangle corner: the centre of its chart's corner texel [texbake::corner_uv].
//   texture_bake_kernel  one lane per texel, one workgroup per tile of kBakeTile x kBakeTile = 256 texels of the atlas.  Blocks are powers
//                        of two, so a tile is (16 / B)^2 whole blocks (B <= 16: at most 32 triangles) or a part of one block (2
//                        triangles).  The tile's triangles -- corner 0, the two edges, the normal, |n|^2, the corner colours
//                        [texbake::load_tri] -- are staged in LDS by the first lanes, one triangle each; a lane computes its surface
//                        point once and keeps it, and reads the normal from LDS (lanes of one chart read one address).  The views come as
//                        the PosedViews descriptor and are walked by walk_views (tsdf_views.h: the walk of tsdf_integrate_kernel, the
//                        views staged in LDS kViewChunk at a time), so their number is not limited.  The depth, mask and colour reads
//                        are gathers: neighbouring texels of a chart project to neighbouring pixels.  The texel's four bytes are one
//                        32-bit store, rows of 16 texels = 64 B segments.  Tiles past the last triangle store zeros and return.
#include "common.h"
#include "texture_bake_core.h"
#include "tsdf_views.h"

namespace mp {

constexpr int kBakeTile = 16;
constexpr int kBakeBlock = kBakeTile * kBakeTile;
constexpr int kBakeMaxTris = 2 * (kBakeTile / texbake::kMinBlock) * (kBakeTile / texbake::kMinBlock);   // 32: a tile of 4 x 4 blocks of 4
constexpr int kBakeTriStride = texbake::kTriFloats + 1;   // 23 words: odd, so the triangles of a tile start on different banks
constexpr int kUvBlock = 256;

__global__ __launch_bounds__(kUvBlock) void texture_uvs_kernel(int T, int S, int B, float* __restrict__ uvs) {
  const long long g = (long long)blockIdx.x * kUvBlock + threadIdx.x;
  if (g >= 3LL * T) return;
  float u, v;
  texbake::corner_uv((int)(g / 3), (int)(g % 3), S, B, &u, &v);
  uvs[2 * g + 0] = u;
  uvs[2 * g + 1] = v;
}

__global__ __launch_bounds__(kBakeBlock) void texture_bake_kernel(const float* __restrict__ vertices, int V, const int32_t* __restrict__ faces, int T,
                                                                  const float* __restrict__ colors, PosedViews vw, int S, int B, float depth_tol,
                                                                  float cos_min2, float z_min, int best_view, uint32_t* __restrict__ texels,
                                                                  uint8_t* __restrict__ seen) {
  __shared__ float tris[kBakeMaxTris * kBakeTriStride];
  __shared__ int tri_flags[kBakeMaxTris];   // texbake::kTri* flags, -1 for a slot past the last triangle
  __shared__ float views[kViewChunk][tsdf::kViewFloats];
  __shared__ int view_ok[kViewChunk];
  const int tiles = S / kBakeTile;
  const int tile_x = blockIdx.x % tiles, tile_y = blockIdx.x / tiles;
  const int lx = threadIdx.x % kBakeTile, ly = threadIdx.x / kBakeTile;
  const int gi = tile_x * kBakeTile + lx, gj = tile_y * kBakeTile + ly;
  const size_t out = (size_t)gj * S + gi;
  const int side = S / B;                                   // blocks a row
  const int per = B < kBakeTile ? kBakeTile / B : 1;        // blocks a tile side
  const int bx0 = (tile_x * kBakeTile) / B, by0 = (tile_y * kBakeTile) / B;
  // the tile's blocks ascend from (bx0, by0): nothing to bake when that one lies past the last triangle (the same for every lane)
  if (2LL * ((long long)by0 * side + bx0) >= T) {
    texels[out] = 0u;
    seen[out] = 0;
    return;
  }
  if ((int)threadIdx.x < 2 * per * per) {
    const int s = threadIdx.x, sb = s >> 1;
    const long long t = 2LL * ((long long)(by0 + sb / per) * side + (bx0 + sb % per)) + (s & 1);
    tri_flags[s] = t < T ? texbake::load_tri(vertices, V, faces, (int)t, colors, tris + s * kBakeTriStride) : -1;
  }
  __syncthreads();
  float a, b;
  const int upper = texbake::chart_point(B, gi % B, gj % B, &a, &b);
  const int slot = (((gj / B) - by0) * per + ((gi / B) - bx0)) * 2 + upper;
  const float* tri = tris + slot * kBakeTriStride;
  const int flags = tri_flags[slot];
  const bool visits = flags >= 0 && (flags & texbake::kTriIndexed) && (flags & texbake::kTriFinite);
  float p[3] = {0.f, 0.f, 0.f};
  if (visits) texbake::surface_point(tri, a, b, p);
  texbake::Accum acc = texbake::accum_init();
  walk_views(vw, visits, views, view_ok, [&](const float* view, const float* depth, const uint8_t* mask, const uint8_t* rgb) {
    acc = texbake::accumulate(acc, texbake::visit(p, tri, view, depth, mask, rgb, vw.h, vw.w, depth_tol, cos_min2, z_min), best_view != 0);
  });
  if (flags < 0) {
    texels[out] = 0u;
    seen[out] = 0;
    return;
  }
  uint8_t sn;
  texels[out] = texbake::finish(acc, tri, a, b, best_view != 0, &sn);
  seen[out] = sn;
}

}  // namespace mp

using namespace mp;

extern "C" int mp_texture_atlas_block(long long n_triangles, int size) { return texbake::atlas_block(n_triangles, size); }

extern "C" int mp_texture_atlas_uvs(int n_triangles, int size, float* d_uvs, mp_stream stream) {
  MP_REQUIRE(n_triangles >= 1 && n_triangles <= texbake::kMaxCount, "mp_texture_atlas_uvs: %d triangles: 1 .. 2^29", n_triangles);
  MP_REQUIRE(texbake::size_ok(size), "mp_texture_atlas_uvs: an atlas of %d texels a side: a power of two, 64 .. 8192", size);
  const int B = texbake::atlas_block(n_triangles, size);
  MP_REQUIRE(B > 0, "mp_texture_atlas_uvs: %d triangles do not fit an atlas of %d x %d texels in blocks of 4 x 4", n_triangles, size, size);
  MP_REQUIRE(d_uvs, "mp_texture_atlas_uvs: null pointer");
  MP_REQUIRE((uintptr_t)d_uvs % 4 == 0, "mp_texture_atlas_uvs: uvs not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("texture_atlas_uvs", 0.0, 24.0 * (double)n_triangles, s);
  hipLaunchKernelGGL(texture_uvs_kernel, dim3((unsigned)ceil_div(3L * n_triangles, kUvBlock)), dim3(kUvBlock), 0, s, n_triangles, size, B, d_uvs);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_texture_bake(const float* d_vertices, int n_vertices, const int32_t* d_faces, int n_triangles, const float* d_colors,
                               const float* d_depth, const uint8_t* d_masks, const uint8_t* d_rgb, const float* d_K, const float* d_TCO, int tco_floats,
                               int n, int h, int w, int size, float depth_tol, float cos_min, float z_min, int best_view, uint8_t* d_texels,
                               uint8_t* d_seen, mp_stream stream) {
  MP_REQUIRE(n_triangles >= 1 && n_triangles <= texbake::kMaxCount && n_vertices >= 0 && n_vertices <= texbake::kMaxCount,
             "mp_texture_bake: %d triangles (1 .. 2^29) of %d vertices (0 .. 2^29)", n_triangles, n_vertices);
  MP_REQUIRE(texbake::size_ok(size), "mp_texture_bake: an atlas of %d texels a side: a power of two, 64 .. 8192", size);
  const int B = texbake::atlas_block(n_triangles, size);
  MP_REQUIRE(B > 0, "mp_texture_bake: %d triangles do not fit an atlas of %d x %d texels in blocks of 4 x 4", n_triangles, size, size);
  MP_REQUIRE(texbake::params_ok(depth_tol, cos_min, z_min),
             "mp_texture_bake: depth_tol must be finite and > 0, cos_min in [0, 1), z_min finite and >= 0");
  PosedViews vw = {d_depth, d_masks, d_rgb, d_K, d_TCO, tco_floats, n, h, w};
  if (int rc = require_views("mp_texture_bake", vw, true, INT32_MAX)) return rc;
  if (n == 0) vw.h = vw.w = 1;   // no view: the fallback colours are still written
  MP_REQUIRE(d_faces && d_texels && d_seen && (d_vertices || n_vertices == 0), "mp_texture_bake: null pointer");
  MP_REQUIRE((uintptr_t)d_texels % 4 == 0 && (uintptr_t)d_vertices % 4 == 0 && (uintptr_t)d_faces % 4 == 0 && (uintptr_t)d_colors % 4 == 0,
             "mp_texture_bake: texels or a 32-bit input not 4-byte aligned");
  const int tiles = size / kBakeTile;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("texture_bake", 0.0, 5.0 * (double)size * size, s);
  hipLaunchKernelGGL(texture_bake_kernel, dim3((unsigned)(tiles * tiles)), dim3(kBakeBlock), 0, s, d_vertices, n_vertices, d_faces, n_triangles, d_colors, vw,
                     size, B, depth_tol, cos_min * cos_min, z_min, best_view, (uint32_t*)d_texels, d_seen);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
