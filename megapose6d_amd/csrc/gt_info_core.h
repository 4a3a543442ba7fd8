// gt_info_core.h -- per-pixel arithmetic and row rules of the ground-truth-info kernels (gt_info.hip), shared with the host emulation
// (tests/gt_info_emul.cpp) the way vsd_core.h is shared with tests/vsd_emul.cpp.  What BOP calls "gt info": per object the visible mask,
// the visibility fraction, the modal (visible-part) box and the amodal (whole-object) box.
//
// CONTRACT (all fp32, compiled with -ffp-contract=off, every operation a separate correctly rounded one, in the order written)
//   * THE CANVAS.  The object's depth is rendered on canvas x canvas tiles of the image's size, canvas in {1, 3}; tiles are row-major,
//     t = ty * canvas + tx, c = (canvas - 1) / 2.  Tile (ty, tx) is the render of the same pose under K with cx' = cx - (tx - c) * w and
//     cy' = cy - (ty - c) * h (one fp32 subtraction each, made by the caller), so tile pixel (x, y) is image pixel (x + (tx - c) * w,
//     y + (ty - c) * h) [tile_shift].  The centre tile is the render under K itself and the only one compared with the observed frame.
//   * obj = depth_gt > 0 [is_obj].  On the centre tile, with r, dist and test_depth of vsd_core.h:
//       valid  = obj and dist_test > 0
//       vis_gt = vsd::classify(0, depth_gt, depth_test, r, delta).vis_gt  (bop19: dist_gt > 0 and (dist_test == 0 or dist_gt - dist_test <= delta))
//                                                                                                                          [classify]
//   * per row: px_count_all = #obj over all tiles, px_count_image = #obj, px_count_valid = #valid, px_count_visib = #vis_gt on the centre
//     tile; visib_fract = (float)px_count_visib / (float)px_count_all as one division of two counts (each < 2^24: exact in fp32), 0 when
//     px_count_all == 0 [visib_fract]; bbox_obj = inclusive extents [xmin, ymin, xmax, ymax] of the obj pixels over all tiles in image
//     coordinates (-w .. 2w - 1: can be negative), bbox_visib the same over the vis_gt pixels; a box over no pixel is -1 -1 -1 -1 [box]
//   * a row whose K has a non-finite entry: counts and boxes of -1, visib_fract NaN, zero masks                             [row_valid]
// Everything but visib_fract is an integer count or a minimum / maximum, so no grid, split or arrival order can change a bit.
#pragma once
#include "vsd_core.h"

namespace mp {
namespace gti {

constexpr int kNumCounts = 4;                 // all, image, valid, visib
constexpr int kAll = 0, kImage = 1, kValid = 2, kVisib = 3;
constexpr int kNumExtents = 8;                // obj: xmin ymin xmax ymax, visib: xmin ymin xmax ymax
constexpr int kRowInts = kNumCounts + kNumExtents;
constexpr int32_t kMinInit = 2147483647, kMaxInit = -2147483647 - 1;   // an extent no pixel has touched

VSD_HD bool canvas_ok(int canvas) { return canvas == 1 || canvas == 3; }

VSD_HD bool row_valid(const float* K) {
  bool ok = true;
  for (int k = 0; k < 9; ++k) ok = ok && vsd::finite_f(K[k]);
  return ok;
}

// image coordinate of tile coordinate 0 along one axis: (t - c) * side
VSD_HD int tile_shift(int t, int canvas, int side) { return (t - (canvas - 1) / 2) * side; }

VSD_HD bool is_obj(float depth_gt) { return depth_gt > 0.f; }

struct Pixel {
  bool obj, valid, vis;
};

// centre tile; r = vsd::ray_factor of the pixel, depths as stored
VSD_HD Pixel classify(float depth_gt, float depth_test, float r, float delta) {
  Pixel p;
  p.obj = is_obj(depth_gt);
  p.valid = p.obj && vsd::test_depth(depth_test) * r > 0.f;
  p.vis = vsd::classify(0.f, depth_gt, depth_test, r, delta).vis_gt;
  return p;
}

VSD_HD float visib_fract(int32_t n_visib, int32_t n_all) {
  if (n_all == 0) return 0.f;
  return (float)n_visib / (float)n_all;
}

VSD_HD bool is_min_extent(int k) { return (k & 3) < 2; }   // xmin, ymin of either box

// ext = xmin ymin xmax ymax as reduced from kMinInit / kMaxInit
VSD_HD void box(const int32_t* ext, int32_t* out) {
  const bool blank = ext[0] > ext[2];
  for (int k = 0; k < 4; ++k) out[k] = blank ? -1 : ext[k];
}

}  // namespace gti
}  // namespace mp
