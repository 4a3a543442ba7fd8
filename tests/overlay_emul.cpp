// TEST SUPPORT: host emulation of the overlay kernels (megapose6d_amd/csrc/overlay.hip), built from the same rules header
// (overlay_core.h).  Same arguments as the C ABI, on host arrays, plus the tile size: the image is walked tile by tile as the workgroups do
// it -- labels with a halo of k + 2 staged with clamped coordinates, e(q) on the tile plus a halo of k, the window maximum rows first, then
// columns -- with plain loops: no lanes, no LDS, no wide accesses.  Any tile size >= 1 must give the same bytes.  Built by
// tests/support/overlay.py; tests/overlay_asan_main.cpp drives it under the sanitizers.
#include <algorithm>
#include <cstdint>
#include <vector>

#include "overlay_core.h"

using namespace mp;

static constexpr ovl::BlendTables kBlend = ovl::make_blend_tables();

extern "C" void overlay_emul_tables(uint8_t* obj, uint8_t* bg) {
  for (int v = 0; v < 256; ++v) {
    obj[v] = kBlend.obj[v];
    bg[v] = kBlend.bg[v];
  }
}

extern "C" void overlay_emul_limits(int* v) {
  v[0] = ovl::kTileW;
  v[1] = ovl::kTileH;
  v[2] = ovl::kMaxDilate;
  v[3] = ovl::kMaxThickness;
  v[4] = ovl::kMaxSide;
}

extern "C" int overlay_emul(const uint8_t* images, const uint8_t* render, const int32_t* labels, const uint8_t* colors, int n_colors, int n, int h,
                            int w, int k, int tile_w, int tile_h, uint8_t* contour, uint8_t* canny, uint8_t* mask, uint8_t* mesh) {
  if (n == 0) return 0;
  if (!ovl::overlay_args_ok(images != nullptr, render != nullptr, labels != nullptr, colors != nullptr, n_colors, n, h, w, k, mesh != nullptr))
    return 1;
  if (tile_w < 1 || tile_h < 1) return 1;
  const int halo = k + 2;
  const int lw = tile_w + 2 * halo, lh = tile_h + 2 * halo, ew = tile_w + 2 * k, eh = tile_h + 2 * k;
  std::vector<int32_t> lab((size_t)lw * lh), edge((size_t)ew * eh), rowmax((size_t)eh * tile_w);
  for (int img = 0; img < n; ++img) {
    const size_t base = (size_t)img * h * w;
    for (int y0 = 0; y0 < h; y0 += tile_h)
      for (int x0 = 0; x0 < w; x0 += tile_w) {
        for (int r = 0; r < lh; ++r)
          for (int c = 0; c < lw; ++c) {
            const int x = ovl::clampi(x0 - halo + c, 0, w - 1), y = ovl::clampi(y0 - halo + r, 0, h - 1);
            const size_t p = base + (size_t)y * w + x;
            lab[(size_t)r * lw + c] = labels ? labels[p] : ovl::label_of_render(render[3 * p], render[3 * p + 1], render[3 * p + 2]);
          }
        for (int r = 0; r < eh; ++r)
          for (int c = 0; c < ew; ++c) {
            const int x = x0 - k + c, y = y0 - k + r;
            int32_t e = -1;
            if (x >= 0 && x < w && y >= 0 && y < h) e = ovl::edge_label(&lab[(size_t)(r + 2) * lw + c + 2], lw, x, y, w, h);
            edge[(size_t)r * ew + c] = e;
          }
        for (int r = 0; r < eh; ++r)
          for (int c = 0; c < tile_w; ++c) {
            int32_t m = edge[(size_t)r * ew + c];
            for (int d = 1; d <= 2 * k; ++d) m = std::max(m, edge[(size_t)r * ew + c + d]);
            rowmax[(size_t)r * tile_w + c] = m;
          }
        for (int row = 0; row < tile_h && y0 + row < h; ++row)
          for (int col = 0; col < tile_w && x0 + col < w; ++col) {
            const size_t p = base + (size_t)(y0 + row) * w + x0 + col;
            const int32_t l = lab[(size_t)(row + halo) * lw + col + halo];
            int32_t out = -1;
            for (int d = 0; d <= 2 * k; ++d) out = std::max(out, rowmax[(size_t)(row + d) * tile_w + col]);
            for (int ch = 0; ch < 3; ++ch) {
              if (contour) contour[3 * p + ch] = out >= 0 ? colors[3 * ovl::color_of(out, n_colors) + ch] : images[3 * p + ch];
              if (mesh) mesh[3 * p + ch] = l >= 0 ? kBlend.obj[render[3 * p + ch]] : kBlend.bg[images[3 * p + ch]];
            }
            if (canny) canny[p] = out >= 0 ? 255 : 0;
            if (mask) mask[p] = l >= 0 ? 255 : 0;
          }
      }
  }
  return 0;
}

// the highest box of image `img` whose frame holds (x, y), or -1
static int box_at(const float* boxes, const int32_t* image_ids, int n_boxes, int img, int x, int y, int t) {
  for (int j = n_boxes - 1; j >= 0; --j) {
    if (image_ids[j] != img) continue;
    bool ok = true;
    const int x1 = ovl::box_corner(boxes[4 * j], &ok), y1 = ovl::box_corner(boxes[4 * j + 1], &ok);
    const int x2 = ovl::box_corner(boxes[4 * j + 2], &ok), y2 = ovl::box_corner(boxes[4 * j + 3], &ok);
    if (ok && ovl::on_frame(x, y, x1, y1, x2, y2, t)) return j;
  }
  return -1;
}

extern "C" int overlay_emul_boxes(const uint8_t* images, const float* boxes, const int32_t* image_ids, int n_boxes, const uint8_t* colors,
                                  int n_colors, int n, int h, int w, int t, uint8_t* out) {
  if (n == 0) return 0;
  if (!ovl::boxes_args_ok(images != nullptr, boxes != nullptr, image_ids != nullptr, colors != nullptr, out != nullptr, n_boxes, n_colors, n, h, w,
                          t))
    return 1;
  for (int img = 0; img < n; ++img)
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        const size_t p = ((size_t)img * h + y) * w + x;
        const int j = box_at(boxes, image_ids, n_boxes, img, x, y, t);
        for (int ch = 0; ch < 3; ++ch) out[3 * p + ch] = j >= 0 ? colors[3 * (j % n_colors) + ch] : images[3 * p + ch];
      }
  return 0;
}
