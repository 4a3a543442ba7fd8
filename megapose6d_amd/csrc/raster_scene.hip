// raster_scene.hip -- multi-object scene renderer for gfx950: several objects drawn into one camera image with depth testing between
// them (replaces Panda3dSceneRenderer.render_scene, the reference's src/megapose/panda3d_renderer/panda3d_scene_renderer.py:298-358).
//
// Contract: include/mp_engine.h (mp_raster_render_scene); per-pixel arithmetic: raster_scene_core.h on top of raster_core.h, which
// tests/raster_scene_emul.cpp also compiles for the host so that the kernel's contract is checked against the oracle without a GPU.
//
// Structure:
//   (0) raster_scene_prep   one thread per object: the camera's K copied next to the object (what raster_bin reads per view) and the
//                           object's light rig copied with its point-light count clamped to 8.
//   (1) raster_bin          (raster.hip, launched through raster_bin.h) one "view" per (camera, object): the object's pieces binned into 8x8-pixel tiles.
//   (2) raster_scene_tiles  one wave per (camera, 8x8 tile), four tiles per workgroup.  The lane owns one pixel and keeps the scene keys
//                           of its NS samples in registers across ALL objects of the camera.  Per object the wave walks the tile's
//                           binned records, then the object's large list (or, if its lists overflowed, every piece), 64 pieces at a
//                           time: each lane turns one into a Piece in the wave's LDS slice, and the wave visits those whose snapped
//                           bounding box reaches the tile (broadcast LDS reads).  Then each lane shades its pixel's distinct winners and
//                           writes the resolved pixel once.  (Record decode and the intra-wave LDS fence: raster_tile_io.h.)
// Roofline: bound by the output writes, (3 + 3 + 1) fp32 channels + one int32 instance id per pixel, ONCE per camera.
#include "common.h"
#include "raster_bin.h"
#include "raster_core.h"
#include "raster_scene_core.h"
#include "raster_tile_io.h"

namespace mp {
namespace {

using rc::Piece;
using rc::SUBPIX;
using rc::TILE;

constexpr int SCENE_WAVES = 4;   // tiles (waves) per workgroup of raster_scene_tiles: a 32 x 8 pixel strip

static_assert(sizeof(mp_lights) == sizeof(rc::Lights), "mp_lights and rc::Lights share one layout");

struct __attribute__((aligned(16))) LdsPiece {   // a piece as the visits need it (absolute snapped coordinates)
  int X[3], Y[3];
  float iz[3];
  int id;
  int pad[2];
};
static_assert(sizeof(LdsPiece) == 48, "three 16-byte words");

__global__ __launch_bounds__(256) void raster_scene_prep(const float* __restrict__ K, const int32_t* __restrict__ obj_off, int n_cams, int n_obj,
                                                         const rc::Lights* __restrict__ lights_in, float* __restrict__ K_obj,
                                                         rc::Lights* __restrict__ lights_out) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= n_obj) return;
  int lo = 0, hi = n_cams - 1;   // the camera of object o: the largest c with obj_off[c] <= o (empty cameras have no object)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (obj_off[mid] <= o) lo = mid;
    else hi = mid - 1;
  }
  for (int k = 0; k < 9; ++k) K_obj[(size_t)o * 9 + k] = K[(size_t)lo * 9 + k];
  rc::Lights L = lights_in[o];
  L.n_point = min(max(L.n_point, 0), 8);
  lights_out[o] = L;
}

template <int NS>
__global__ __launch_bounds__(64 * SCENE_WAVES) void raster_scene_tiles(rc::SceneObjects so, const int32_t* __restrict__ obj_off,
                                                                       const float* __restrict__ radius, const int* __restrict__ ws, BinLayout lay,
                                                                       int h, int w, uint32_t flags, float* __restrict__ out, long long stride_v,
                                                                       long long stride_y, long long stride_x, int c_rgb, int c_normals, int c_depth,
                                                                       int32_t* __restrict__ inst) {
  __shared__ LdsPiece batch[SCENE_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int groups_x = (lay.tiles_x + SCENE_WAVES - 1) / SCENE_WAVES;
  int b = blockIdx.x;
  const int gx = b % groups_x;
  b /= groups_x;
  const int ty = b % lay.tiles_y;
  const int cam = b / lay.tiles_y;
  const int tx = gx * SCENE_WAVES + wave;
  if (tx >= lay.tiles_x) return;   // (no workgroup barrier below: the waves are independent)
  const int tile = ty * lay.tiles_x + tx, tile_x0 = tx * TILE, tile_y0 = ty * TILE;
  const int px = tile_x0 + (lane & 7), py = tile_y0 + (lane >> 3);
  LdsPiece* mine = batch[wave];
  unsigned long long key[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) key[s] = 0ull;
  const int o0 = obj_off[cam], o1 = obj_off[cam + 1];
  for (int o = o0; o < o1; ++o) {
    const int slot = o - o0;
    const int* hdr = ws + (size_t)o * lay.view_ints;
    const rc::MeshRef m = so.meshes[so.mesh_ids[o]];
    const float* T = so.TCO + (size_t)o * 16;
    const float* Kv = so.K + (size_t)o * 9;
    const bool overflow = hdr[2] != 0;
    // the object's pieces for this tile: [0, n_list) binned records, then [n_list, n_list + n_large) large-list indices; an overflowed
    // object walks all 2F piece indices instead
    const int begin = overflow ? 0 : hdr[RASTER_BIN_HDR_INTS + tile];
    const int n_list = overflow ? 0 : hdr[RASTER_BIN_HDR_INTS + tile + 1] - begin;
    const int begin_l = overflow ? 0 : hdr[lay.off_tl + tile];
    const int n_large = overflow ? 2 * m.n_faces : hdr[lay.off_tl + tile + 1] - begin_l;
    const rc::TileRec* list = reinterpret_cast<const rc::TileRec*>(hdr + lay.off_list);
    const int* large = hdr + lay.off_large;
    const int n_total = n_list + n_large;
    for (int base = 0; base < n_total; base += 64) {
      const int e = base + lane;
      Piece p;
      p.id = -1;
      if (e < n_list) {
        rc::unpack_tile_rec(load_tile_rec(list + begin + e), tile_x0, tile_y0, p);
      } else if (e < n_total) {
        rc::piece_from_index<false>(m, T, Kv, overflow ? e - n_list : large[begin_l + e - n_list], p);
      }
      bool reach = false;
      if (p.id >= 0) {
        int x0, y0, x1, y1;
        rc::piece_pixel_bbox(p, NS, w, h, x0, y0, x1, y1);
        reach = max(x0, tile_x0) <= min(x1, tile_x0 + TILE - 1) && max(y0, tile_y0) <= min(y1, tile_y0 + TILE - 1);
      }
      if (reach) {
        LdsPiece& d = mine[lane];
        d.X[0] = p.X[0]; d.X[1] = p.X[1]; d.X[2] = p.X[2];
        d.Y[0] = p.Y[0]; d.Y[1] = p.Y[1]; d.Y[2] = p.Y[2];
        d.iz[0] = p.iz[0]; d.iz[1] = p.iz[1]; d.iz[2] = p.iz[2];
        d.id = p.id;
      }
      unsigned long long todo = __ballot(reach);
      wave_lds_fence();
      while (todo) {
        const int j = __ffsll((long long)todo) - 1;
        todo &= todo - 1ull;
        const LdsPiece& q = mine[j];   // wave-uniform address: broadcast reads
        Piece v;
        v.X[0] = q.X[0]; v.X[1] = q.X[1]; v.X[2] = q.X[2];
        v.Y[0] = q.Y[0]; v.Y[1] = q.Y[1]; v.Y[2] = q.Y[2];
        v.iz[0] = q.iz[0]; v.iz[1] = q.iz[1]; v.iz[2] = q.iz[2];
        v.id = q.id;
        v.tri = -1;
        v.flags = 0;
        rc::scene_cover<NS>(v, slot, tile_x0, tile_y0, px, py, key);
      }
      wave_lds_fence();   // the next batch rewrites the slice
    }
  }
  if (px >= w || py >= h) return;
  float rgb[3], nrm[3], depth;
  int winner;
  rc::scene_shade_resolve<NS>(so, o0, radius[cam], (flags & MP_RASTER_NORMALS_GL) != 0, c_normals >= 0, key, px, py, rgb, nrm, depth, winner);
  float* dst = out + (size_t)cam * stride_v + (size_t)py * stride_y + (size_t)px * stride_x;
  if (c_rgb >= 0) { dst[c_rgb] = rgb[0]; dst[c_rgb + 1] = rgb[1]; dst[c_rgb + 2] = rgb[2]; }
  if (c_normals >= 0) { dst[c_normals] = nrm[0]; dst[c_normals + 1] = nrm[1]; dst[c_normals + 2] = nrm[2]; }
  if (c_depth >= 0) dst[c_depth] = depth;
  if (inst) inst[((size_t)cam * h + py) * w + px] = winner;
}

// workspace: [n_obj view blocks of raster_bin][K per object: 9 floats, padded to 4][light rig per object: rc::Lights]
size_t scene_k_offset_ints(const BinLayout& lay, int n_obj) { return (size_t)n_obj * (size_t)lay.view_ints; }
size_t scene_lights_offset_ints(const BinLayout& lay, int n_obj) { return scene_k_offset_ints(lay, n_obj) + (((size_t)9 * n_obj + 3) & ~(size_t)3); }

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" size_t mp_raster_scene_workspace_bytes(const mp_mesh_db* db, int n_objects, int h, int w) {
  if (!db || n_objects < 0 || h <= 0 || w <= 0) return 0;
  const BinLayout lay = raster_bin_layout(db, h, w);
  return (scene_lights_offset_ints(lay, n_objects) + (size_t)n_objects * (sizeof(rc::Lights) / sizeof(int))) * sizeof(int) + 16;
}

extern "C" int mp_raster_render_scene(const mp_mesh_db* db, int n_cams, const int32_t* h_obj_off, const int32_t* d_obj_off,
                                      const int32_t* d_mesh_ids, const float* d_TCO, const float* d_K, const float* d_radius,
                                      const mp_lights* d_lights, int h, int w, uint32_t flags, float* d_out, int64_t stride_v, int64_t stride_y,
                                      int64_t stride_x, int c_rgb, int c_normals, int c_depth, int32_t* d_instance, void* d_ws, size_t ws_bytes,
                                      mp_stream stream) {
  MP_REQUIRE(db && h_obj_off && d_obj_off && d_K && d_radius && d_ws, "mp_raster_render_scene: null pointer");
  MP_REQUIRE(n_cams >= 0 && h > 0 && w > 0 && w <= 1024 && h <= 1024, "mp_raster_render_scene: bad size (h, w <= 1024)");
  MP_REQUIRE((flags & ~(MP_RASTER_NORMALS | MP_RASTER_DEPTH | MP_RASTER_NORMALS_GL | MP_RASTER_MSAA4)) == 0,
             "mp_raster_render_scene: unsupported flag bits 0x%x (fp32 output only)", flags);
  if (!(flags & MP_RASTER_NORMALS)) c_normals = -1;
  if (!(flags & MP_RASTER_DEPTH)) c_depth = -1;
  MP_REQUIRE(c_rgb >= 0 || c_normals >= 0 || c_depth >= 0 || d_instance, "mp_raster_render_scene: nothing to write");
  MP_REQUIRE(d_out || (c_rgb < 0 && c_normals < 0 && c_depth < 0), "mp_raster_render_scene: null d_out");
  MP_REQUIRE(h_obj_off[0] == 0, "mp_raster_render_scene: obj_off[0] must be 0");
  for (int c = 0; c < n_cams; ++c) {
    const int n = h_obj_off[c + 1] - h_obj_off[c];
    MP_REQUIRE(n >= 0, "mp_raster_render_scene: obj_off must be non-decreasing (camera %d)", c);
    MP_REQUIRE(n <= rc::SCENE_MAX_OBJECTS, "mp_raster_render_scene: camera %d has %d objects (at most %d)", c, n, rc::SCENE_MAX_OBJECTS);
  }
  if (n_cams == 0) return MP_OK;
  const int n_obj = h_obj_off[n_cams];
  MP_REQUIRE(n_obj == 0 || (d_mesh_ids && d_TCO && d_lights), "mp_raster_render_scene: null object arrays");
  MP_REQUIRE(ws_bytes >= mp_raster_scene_workspace_bytes(db, n_obj, h, w), "mp_raster_render_scene: workspace too small");
  hipStream_t s = (hipStream_t)stream;
  const BinLayout lay = raster_bin_layout(db, h, w);
  const int ns = (flags & MP_RASTER_MSAA4) ? 4 : 1;
  int* ws = (int*)d_ws;
  float* K_obj = (float*)(ws + scene_k_offset_ints(lay, n_obj));
  rc::Lights* lights = (rc::Lights*)(ws + scene_lights_offset_ints(lay, n_obj));
  if (n_obj > 0) {
    {
      ProfScope prof("raster_scene_prep", 0.0, (double)n_obj * 2.0 * (36.0 + sizeof(rc::Lights)), s);
      hipLaunchKernelGGL(raster_scene_prep, dim3((unsigned)ceil_div(n_obj, 256)), dim3(256), 0, s, d_K, d_obj_off, n_cams, n_obj,
                         (const rc::Lights*)d_lights, K_obj, lights);
    }
    const int rc_bin = raster_bin_launch(db, d_mesh_ids, d_TCO, K_obj, n_obj, h, w, ns, ws, lay, nullptr, nullptr, s);
    if (rc_bin != MP_OK) return rc_bin;
  }
  const int groups_x = ceil_div(lay.tiles_x, SCENE_WAVES);
  const long long n_wg = (long long)n_cams * lay.tiles_y * groups_x;
  MP_REQUIRE(n_wg < (1LL << 31), "mp_raster_render_scene: grid too large");
  rc::SceneObjects so;
  so.meshes = db->d_meshes;
  so.texs = db->d_texs;
  so.mesh_ids = d_mesh_ids;
  so.TCO = d_TCO;
  so.K = K_obj;
  so.lights = lights;
  const int n_ch = (c_rgb >= 0 ? 3 : 0) + (c_normals >= 0 ? 3 : 0) + (c_depth >= 0 ? 1 : 0) + (d_instance ? 1 : 0);
  // algorithmic bytes: every output channel written once per camera pixel + each object's mesh read once (32 B/vertex, 12 B/triangle)
  const double alg_bytes = (double)n_cams * n_ch * 4.0 * h * w + (double)n_obj * (32.0 * mp_mesh_db_max_vertices(db) + 12.0 * lay.max_faces);
  ProfScope prof("raster_scene_tiles", 0.0, alg_bytes, s);
  if (ns == 4)
    hipLaunchKernelGGL(raster_scene_tiles<4>, dim3((unsigned)n_wg), dim3(64 * SCENE_WAVES), 0, s, so, d_obj_off, d_radius, (const int*)ws, lay, h, w,
                       flags, d_out, (long long)stride_v, (long long)stride_y, (long long)stride_x, c_rgb, c_normals, c_depth, d_instance);
  else
    hipLaunchKernelGGL(raster_scene_tiles<1>, dim3((unsigned)n_wg), dim3(64 * SCENE_WAVES), 0, s, so, d_obj_off, d_radius, (const int*)ws, lay, h, w,
                       flags, d_out, (long long)stride_v, (long long)stride_y, (long long)stride_x, c_rgb, c_normals, c_depth, d_instance);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
