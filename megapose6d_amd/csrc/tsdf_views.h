// tsdf_views.h -- a set of posed views as the onboarding kernels take it (tsdf.hip, texture_bake.hip, tsdf_track.hip): the descriptor, the
// one walk over it with the views staged in LDS, and what the C entries require of a views argument set and of a volume.  Device side
// only; the rules of a view are tsdf_core.h's [load_view], and the emulations of the tests walk their views in plain loops.
#pragma once
#include "common.h"
#include "tsdf_core.h"

namespace mp {

constexpr int kViewChunk = 32;   // views staged in LDS at a time: 2 KB of tables

struct PosedViews {
  const float* depth;     // [n, h, w]
  const uint8_t* masks;   // [n, h, w] or null
  const uint8_t* rgb;     // [n, h, w, 3] or null
  const float* K;         // [n, 9]
  const float* TCO;       // [n, tco_floats]
  int tco_floats, n, h, w;
};

// Every lane of the workgroup calls this: the views (R, t, fx, fy, cx, cy and whether K and TCO are finite) are loaded into `views` /
// `view_ok` kViewChunk at a time by the first lanes, so their number is not limited; a lane that takes part then calls
// per_view(view [kViewFloats], depth frame, mask frame or null, rgb frame or null) for every finite view, in ascending order.
template <class F>
__device__ __forceinline__ void walk_views(const PosedViews& vw, bool takes_part, float (*views)[tsdf::kViewFloats], int* view_ok, F&& per_view) {
  const size_t hw = (size_t)vw.h * vw.w;
  for (int v0 = 0; v0 < vw.n; v0 += kViewChunk) {
    const int m = vw.n - v0 < kViewChunk ? vw.n - v0 : kViewChunk;
    __syncthreads();   // every lane has left the chunk before
    if ((int)threadIdx.x < m)
      view_ok[threadIdx.x] = tsdf::load_view(vw.K + (size_t)(v0 + threadIdx.x) * 9, vw.TCO + (size_t)(v0 + threadIdx.x) * vw.tco_floats, views[threadIdx.x]);
    __syncthreads();
    if (!takes_part) continue;
    for (int q = 0; q < m; ++q) {
      if (!view_ok[q]) continue;
      const size_t v = (size_t)(v0 + q);
      per_view(views[q], vw.depth + v * hw, vw.masks ? vw.masks + v * hw : nullptr, vw.rgb ? vw.rgb + v * hw * 3 : nullptr);
    }
  }
}

// what `entry` requires of its volume arguments
inline int require_volume(const char* entry, int nx, int ny, int nz, float ox, float oy, float oz, float voxel) {
  const float origin[3] = {ox, oy, oz};
  MP_REQUIRE(tsdf::dims_ok(nx, ny, nz), "%s: volume of %d x %d x %d: each side 2 .. 512, at most 2^27 nodes", entry, nx, ny, nz);
  MP_REQUIRE(tsdf::grid_ok(origin, voxel), "%s: origin must be finite, voxel finite and > 0", entry);
  return MP_OK;
}

// what `entry` requires of its views arguments.  n = 0 passes before frames and pointers are looked at: the caller returns or goes on.
inline int require_views(const char* entry, const PosedViews& vw, bool needs_rgb, int max_n) {
  MP_REQUIRE(vw.n >= 0 && vw.n <= max_n && (vw.tco_floats == 12 || vw.tco_floats == 16), "%s: n %d in 0 .. %d, TCO rows of 12 or 16 floats (got %d)",
             entry, vw.n, max_n, vw.tco_floats);
  if (vw.n == 0) return MP_OK;
  MP_REQUIRE(tsdf::frame_ok(vw.h, vw.w), "%s: frames of %d x %d: 1 .. 8192 a side", entry, vw.h, vw.w);
  MP_REQUIRE(vw.depth && vw.K && vw.TCO && (vw.rgb || !needs_rgb), "%s: null pointer among the views", entry);
  MP_REQUIRE((uintptr_t)vw.depth % 4 == 0 && (uintptr_t)vw.K % 4 == 0 && (uintptr_t)vw.TCO % 4 == 0, "%s: depth, K or TCO not 4-byte aligned", entry);
  return MP_OK;
}

}  // namespace mp
