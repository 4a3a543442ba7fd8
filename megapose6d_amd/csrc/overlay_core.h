// overlay_core.h -- the rules of the prediction overlays (contour overlay, mesh blend, box frames) that run on the device (overlay.hip),
// shared with the host emulation (tests/overlay_emul.cpp) the way model_info_core.h and vsd_core.h are shared with theirs.
//
// CONTRACT (mp_overlay)
//   * INPUTS.  n images of h x w: the observed image uint8 [n,h,w,3]; optionally a render uint8 [n,h,w,3]; optionally a label map int32
//     [n,h,w] (< 0 background, l >= 0 an instance).  Without a label map the label is 0 where any channel of the render is > 0 and -1
//     elsewhere [label_of_render: the reference's get_mask_from_rgb].  A colour table uint8 [n_colors,3]; label l is drawn in colour
//     l mod n_colors (the reference's plotter cycles its palette).
//   * EDGE of label l at pixel q: OpenCV's Canny(mask, 30, 100) with the L1 norm and aperture 3, restated for the 0 / 1 mask
//     m = [label == l].  Every gradient of a 0 / 255 mask is a multiple of 255, so every non-zero magnitude is above the high threshold
//     and hysteresis changes nothing.  gx, gy = the 3x3 Sobel responses of m with the border REPLICATED [sobel: the tile holds the label
//     of the clamped coordinate]; mag = |gx| + |gy| inside the image and ZERO outside [mag_at].  q is an edge when mag != 0 and
//     [is_edge], with ax = |gx|, ay = |gy| << 15, t = ax * 13573 (tan 22.5 deg in 15 fractional bits):
//         ay < t               (horizontal gradient)  mag >  mag(x-1, y)    and  mag >= mag(x+1, y)
//         ay > t + (ax << 16)  (vertical gradient)    mag >  mag(x, y-1)    and  mag >= mag(x, y+1)
//         otherwise            (diagonal)             mag >  mag(x-s, y-1)  and  mag >  mag(x+s, y+1),  s = -1 when (gx ^ gy) < 0 else +1
//     The mix of > and >= is OpenCV's: it decides which side of a one-pixel step keeps the edge.
//   * e(q) = the largest label with an edge at q, or -1 [edge_label].  Only labels present in the 3x3 around q can have an edge there
//     (at most 9 candidates); their magnitudes at q's neighbours need the labels in the 5x5 around q.
//   * out(p) = the largest e(q) over the q OF THE IMAGE within Chebyshev distance k = dilate_iterations of p: k rounds of a 3x3 dilation
//     per label, painted in ascending label order with later overwriting earlier.  The maximum over a square window is taken rows first,
//     then columns; a maximum does not depend on that order.
//   * OUTPUTS.  contour [n,h,w,3] = colour (out mod n_colors) where out >= 0, else the observed pixel; canny [n,h,w] = 255 where out >= 0,
//     else 0; mask [n,h,w] = 255 where label >= 0, else 0; mesh [n,h,w,3] per channel = kBlend.obj[render] where label >= 0, else
//     kBlend.bg[image]: the two tables hold trunc((float)(v * 0.8 + 255 * 0.2)) and trunc((float)(v * 0.6 + 255 * 0.4)) with the sum in
//     float64, which is numpy's evaluation of the reference's plot_overlay.
//   * Integer arithmetic throughout; no atomics; every output byte is written by exactly one thread; the result does not depend on grid,
//     block or tile size.
//   * LIMITS [sizes_ok, overlay_args_ok].  h, w in 1 .. 8192, n * h * w * 3 < 2^31, k in 0 .. 8 (the halo of a tile is k + 2), n_colors >= 1.
//
// CONTRACT (mp_draw_boxes)
//   * Box j = (x1, y1, x2, y2) fp32, truncated to integers [box_corner]; a NaN coordinate draws nothing, the others are clamped to
//     +-2^20 first.  Corners are not reordered: a box with x1 > x2 + 2 (t / 2) covers no pixel.
//   * A pixel is on frame j when it lies inside the box grown by t / 2 and outside the box shrunk by (t + 1) / 2, t = thickness in
//     1 .. 8 [on_frame].  The highest j of the pixel's image wins; the colour is j mod n_colors.  A gather per pixel, not a scatter.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OVL_HD __host__ __device__ __forceinline__
#else
#define OVL_HD inline
#endif

namespace mp {
namespace ovl {

constexpr int kMaxDilate = 8;            // k
constexpr int kMaxThickness = 8;         // t
constexpr int kMaxSide = 8192;           // h, w
constexpr int kTileW = 64;               // the kernel's tile: 64 x 16 pixels, 4 consecutive pixels of a row per lane of 256
constexpr int kTileH = 16;
constexpr int kBlock = 256;
constexpr int kGroup = 4;                // pixels per lane: 12 bytes of a 3-byte image, 4 of a 1-byte one
constexpr int kCornerLimit = 1 << 20;    // box corners are clamped to +- this

OVL_HD bool sizes_ok(int n, int h, int w) {
  return n >= 0 && h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide && (long long)n * h * w * 3 < 2147483648LL;
}

// the argument rules of mp_overlay that do not look at output pointers
OVL_HD bool overlay_args_ok(bool has_images, bool has_render, bool has_labels, bool has_colors, int n_colors, int n, int h, int w, int k,
                            bool want_mesh) {
  return sizes_ok(n, h, w) && has_images && has_colors && (has_render || has_labels) && n_colors >= 1 && k >= 0 && k <= kMaxDilate &&
         (!want_mesh || has_render);
}

OVL_HD bool boxes_args_ok(bool has_images, bool has_boxes, bool has_ids, bool has_colors, bool has_out, int n_boxes, int n_colors, int n,
                          int h, int w, int t) {
  return sizes_ok(n, h, w) && has_images && has_colors && has_out && n_boxes >= 0 && (n_boxes == 0 || (has_boxes && has_ids)) &&
         n_colors >= 1 && t >= 1 && t <= kMaxThickness;
}

OVL_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
OVL_HD int absi(int v) { return v < 0 ? -v : v; }

OVL_HD int32_t label_of_render(uint8_t r, uint8_t g, uint8_t b) { return (r | g | b) ? 0 : -1; }

// the non-negative remainder of a label >= 0
OVL_HD int color_of(int32_t label, int n_colors) { return (int)(label % n_colors); }

// L points at the tile entry of a pixel; L[dy * stride + dx] is the label at the CLAMPED image coordinate (x + dx, y + dy)
OVL_HD void sobel(const int32_t* L, int stride, int32_t l, int* gx, int* gy) {
  const int a = L[-stride - 1] == l, b = L[-stride] == l, c = L[-stride + 1] == l;
  const int d = L[-1] == l, f = L[1] == l;
  const int g = L[stride - 1] == l, hh = L[stride] == l, i = L[stride + 1] == l;
  *gx = (c + 2 * f + i) - (a + 2 * d + g);
  *gy = (g + 2 * hh + i) - (a + 2 * b + c);
}

// the magnitude of label l's mask at image pixel (x, y), whose tile entry L points at: zero outside the image
OVL_HD int mag_at(const int32_t* L, int stride, int32_t l, int x, int y, int w, int h) {
  if (x < 0 || x >= w || y < 0 || y >= h) return 0;
  int gx, gy;
  sobel(L, stride, l, &gx, &gy);
  return absi(gx) + absi(gy);
}

// is image pixel (x, y) an edge of label l?  L points at its tile entry; the 5x5 around it is read
OVL_HD bool is_edge(const int32_t* L, int stride, int32_t l, int x, int y, int w, int h) {
  int gx, gy;
  sobel(L, stride, l, &gx, &gy);
  const int ax = absi(gx), ayi = absi(gy), mag = ax + ayi;
  if (mag == 0) return false;
  const int ay = ayi << 15, t = ax * 13573;
  if (ay < t) return mag > mag_at(L - 1, stride, l, x - 1, y, w, h) && mag >= mag_at(L + 1, stride, l, x + 1, y, w, h);
  if (ay > t + (ax << 16)) return mag > mag_at(L - stride, stride, l, x, y - 1, w, h) && mag >= mag_at(L + stride, stride, l, x, y + 1, w, h);
  const int s = (gx ^ gy) < 0 ? -1 : 1;
  return mag > mag_at(L - stride - s, stride, l, x - s, y - 1, w, h) && mag > mag_at(L + stride + s, stride, l, x + s, y + 1, w, h);
}

// e(q): the largest label with an edge at image pixel (x, y), or -1
OVL_HD int32_t edge_label(const int32_t* L, int stride, int x, int y, int w, int h) {
  int32_t v[9];
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) v[3 * dy + dx + 4] = L[dy * stride + dx];
  bool flat = true;
  for (int i = 0; i < 9; ++i) flat = flat && v[i] == v[4];
  if (flat) return -1;   // one label over the 3x3: every mask is constant there, every gradient zero
  // the labels of the 3x3 in descending order, each tried once; the first with an edge is the largest
  int32_t bound = 0;
  for (bool first = true;; first = false) {
    int32_t cand = -1;
    for (int i = 0; i < 9; ++i)
      if ((first || v[i] < bound) && v[i] > cand) cand = v[i];
    if (cand < 0) return -1;
    if (is_edge(L, stride, cand, x, y, w, h)) return cand;
    bound = cand;
  }
}

// the mesh blend's tables, built by the host compiler from the reference's expression (float64 sum -> float32 -> truncation)
struct BlendTables {
  uint8_t obj[256], bg[256];
};

constexpr BlendTables make_blend_tables() {
  BlendTables t{};
  for (int v = 0; v < 256; ++v) {
    t.obj[v] = (uint8_t)(float)((double)v * 0.8 + 255 * 0.2);
    t.bg[v] = (uint8_t)(float)((double)v * 0.6 + 255 * 0.4);
  }
  return t;
}

// a box corner: NaN -> *ok = false; else clamped to +-kCornerLimit and truncated toward zero
OVL_HD int box_corner(float v, bool* ok) {
  if (!(v == v)) {
    *ok = false;
    return 0;
  }
  const float lim = (float)kCornerLimit;
  return (int)(v < -lim ? -lim : (v > lim ? lim : v));
}

OVL_HD bool on_frame(int x, int y, int x1, int y1, int x2, int y2, int t) {
  const int g = t / 2, s = (t + 1) / 2;
  const bool in_grown = x >= x1 - g && x <= x2 + g && y >= y1 - g && y <= y2 + g;
  const bool in_shrunk = x >= x1 + s && x <= x2 - s && y >= y1 + s && y <= y2 - s;
  return in_grown && !in_shrunk;
}

}  // namespace ovl
}  // namespace mp
