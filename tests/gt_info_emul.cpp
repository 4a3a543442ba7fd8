// TEST SUPPORT: host emulation of the ground-truth-info kernels (megapose6d_amd/csrc/gt_info.hip), built from the same arithmetic
// headers (gt_info_core.h on top of vsd_core.h).  Same arguments as the C ABI, on host arrays: one plain loop over tiles and pixels per
// row, no strips, no chunks, no ballots.  Counts are integers and extents minima / maxima, so the kernels are held to these results bit
// for bit.  Built by tests/support/gt_info.py with -ffp-contract=off.
#include <cstdint>

#include "gt_info_core.h"

using namespace mp;

extern "C" void gt_info_emul(const float* depth_gt, const int32_t* gt_ids, const float* depth_test, const int32_t* im_ids, const float* K, int b,
                             int h, int w, int canvas, float delta, int32_t* counts, int32_t* boxes, float* fract, uint8_t* mask,
                             uint8_t* mask_visib) {
  const size_t hw = (size_t)h * w;
  const int n_tiles = canvas * canvas, centre = (n_tiles - 1) / 2;
  for (int row = 0; row < b; ++row) {
    const float* Kr = K + (size_t)row * 9;
    int32_t* c = counts + (size_t)row * gti::kNumCounts;
    int32_t* bx = boxes + (size_t)row * gti::kNumExtents;
    uint8_t* M = mask ? mask + (size_t)row * hw : nullptr;
    uint8_t* MV = mask_visib ? mask_visib + (size_t)row * hw : nullptr;
    if (!gti::row_valid(Kr)) {
      for (int k = 0; k < gti::kNumCounts; ++k) c[k] = -1;
      for (int k = 0; k < gti::kNumExtents; ++k) bx[k] = -1;
      fract[row] = vsd::quiet_nan();
      for (size_t i = 0; i < hw; ++i) {
        if (M) M[i] = 0;
        if (MV) MV[i] = 0;
      }
      continue;
    }
    const float* G = depth_gt + (size_t)(gt_ids ? gt_ids[row] : row) * n_tiles * hw;
    const float* T = depth_test + (size_t)(im_ids ? im_ids[row] : row) * hw;
    for (int k = 0; k < gti::kNumCounts; ++k) c[k] = 0;
    int32_t ext[gti::kNumExtents];
    for (int k = 0; k < gti::kNumExtents; ++k) ext[k] = gti::is_min_extent(k) ? gti::kMinInit : gti::kMaxInit;
    auto touch = [&](int q, int X, int Y) {
      int32_t* e = ext + 4 * q;
      if (X < e[0]) e[0] = X;
      if (Y < e[1]) e[1] = Y;
      if (X > e[2]) e[2] = X;
      if (Y > e[3]) e[3] = Y;
    };
    for (int tile = 0; tile < n_tiles; ++tile) {
      const int ox = gti::tile_shift(tile % canvas, canvas, w), oy = gti::tile_shift(tile / canvas, canvas, h);
      const float* Gt = G + (size_t)tile * hw;
      for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x) {
          const float g = Gt[(size_t)y * w + x];
          if (tile != centre) {
            if (gti::is_obj(g)) {
              c[gti::kAll] += 1;
              touch(0, x + ox, y + oy);
            }
            continue;
          }
          const float u = vsd::ray_u(Kr, x), v = vsd::ray_v(Kr, y);
          const gti::Pixel p = gti::classify(g, T[(size_t)y * w + x], vsd::ray_factor(u * u, v * v), delta);
          c[gti::kAll] += p.obj ? 1 : 0;
          c[gti::kImage] += p.obj ? 1 : 0;
          c[gti::kValid] += p.valid ? 1 : 0;
          c[gti::kVisib] += p.vis ? 1 : 0;
          if (p.obj) touch(0, x + ox, y + oy);
          if (p.vis) touch(1, x + ox, y + oy);
          if (M) M[(size_t)y * w + x] = p.obj ? 255 : 0;
          if (MV) MV[(size_t)y * w + x] = p.vis ? 255 : 0;
        }
    }
    gti::box(ext, bx);
    gti::box(ext + 4, bx + 4);
    fract[row] = gti::visib_fract(c[gti::kVisib], c[gti::kAll]);
  }
}
