// overlay.hip -- prediction overlays on the device: per-instance Canny contours painted on the observed image, the mesh blend, the mask,
// and box frames (the reference's make_contour_overlay, plot_overlay and draw_bounding_box on uint8 images).
//
// The rules are overlay_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Everything is integer
// arithmetic and a maximum over a window, so neither the grid nor the tile can change a bit.  No atomics: every output byte is written by
// exactly one lane.
//
//   overlay_kernel     one workgroup of 256 lanes per tile of 64 x 16 pixels of one image (a 1-D grid: image, tile row, tile column).
//                        1. the tile's labels plus a halo of k + 2 go to LDS (int32; from the label map, or from the render's bytes through
//                           label_of_render); an entry outside the image holds the label of the clamped coordinate, which is the
//                           replicated border of the Sobel;
//                        2. e(q) [edge_label] for the tile plus a halo of k goes to a second LDS tile, -1 outside the image;
//                        3. the maximum over the (2k + 1)^2 window is taken separably: rows into a third LDS tile, columns in registers;
//                        4. lane l owns 4 consecutive pixels of row l / 16: it reads 12 image (and render) bytes and writes 12 + 12 + 4 + 4.
//                           When w is a multiple of 4 and the tensors are 4-byte aligned these are dword accesses (a wave then covers 4 rows
//                           of 192 contiguous bytes); otherwise byte accesses with the same results.
//                      One instantiation per k: tile sizes and window loops are compile-time constants.  LDS at k = 1: 70 x 22 + 66 x 18 +
//                      64 x 18 int32 + the blend tables (512 bytes, filled only when the mesh is asked for) = 15.7 KiB; at k = 8: 30.3 KiB.
//   draw_boxes_kernel  the same lane-to-pixel map; the boxes that meet the tile are listed in LDS in ascending order, every pixel walks the
//                      list from the last to the first [on_frame].
#include "common.h"
#include "overlay_core.h"

namespace mp {

__constant__ ovl::BlendTables d_blend = ovl::make_blend_tables();

struct OverlayArgs {
  const uint8_t* images;
  const uint8_t* render;
  const int32_t* labels;
  const uint8_t* colors;
  uint8_t* contour;
  uint8_t* canny;
  uint8_t* mask;
  uint8_t* mesh;
  int n_colors, h, w, tiles_x, tiles_y, wide;
};

// 4 pixels of a 3-byte image at byte offset `off`, one byte value per element of b: three dwords when `wide`, else the bytes of the
// `n_px` pixels that exist
__device__ __forceinline__ void load_px3(const uint8_t* __restrict__ p, size_t off, bool wide, int n_px, uint32_t* b) {
  if (wide) {
    const uint32_t* q = (const uint32_t*)(p + off);
    for (int d = 0; d < 3; ++d) {
      const uint32_t v = q[d];
      for (int s = 0; s < 4; ++s) b[4 * d + s] = (v >> (8 * s)) & 0xffu;
    }
  } else {
    for (int s = 0; s < 12; ++s) b[s] = s < 3 * n_px ? p[off + s] : 0;
  }
}

__device__ __forceinline__ void store_px3(uint8_t* __restrict__ p, size_t off, bool wide, int n_px, const uint32_t* b) {
  if (wide) {
    uint32_t* q = (uint32_t*)(p + off);
    for (int d = 0; d < 3; ++d)
      q[d] = b[4 * d] | (b[4 * d + 1] << 8) | (b[4 * d + 2] << 16) | (b[4 * d + 3] << 24);
  } else {
    for (int s = 0; s < 12; ++s)   // a fixed trip count keeps b in registers
      if (s < 3 * n_px) p[off + s] = (uint8_t)b[s];
  }
}

__device__ __forceinline__ void store_px1(uint8_t* __restrict__ p, size_t off, bool wide, int n_px, const uint32_t* b) {
  if (wide) {
    *(uint32_t*)(p + off) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
  } else {
    for (int s = 0; s < 4; ++s)
      if (s < n_px) p[off + s] = (uint8_t)b[s];
  }
}

// K = dilate_iterations: the tile sizes, the index arithmetic and the window loops are constants of the instantiation
template <int K>
__global__ __launch_bounds__(256) void overlay_kernel(OverlayArgs a) {
  constexpr int k = K, halo = K + 2;
  constexpr int lw = ovl::kTileW + 2 * halo, lh = ovl::kTileH + 2 * halo;   // labels:  70 x 22 at K = 1, 84 x 36 at K = 8
  constexpr int ew = ovl::kTileW + 2 * k, eh = ovl::kTileH + 2 * k;         // e(q):    66 x 18 at K = 1, 80 x 32 at K = 8
  constexpr int kLabW = lw, kEdgeW = ew;
  __shared__ int32_t lab[lh * lw];
  __shared__ int32_t edge[eh * ew];
  __shared__ int32_t rowmax[eh * ovl::kTileW];
  __shared__ ovl::BlendTables blend;
  const int tid = threadIdx.x;
  const int per_image = a.tiles_x * a.tiles_y;
  const int img = blockIdx.x / per_image, rest = blockIdx.x - img * per_image;
  const int ty = rest / a.tiles_x, tx = rest - ty * a.tiles_x;
  const int x0 = tx * ovl::kTileW, y0 = ty * ovl::kTileH;
  const int w = a.w, h = a.h;
  const size_t base = (size_t)img * h * w;   // pixels before this image

  if (a.mesh) {
    blend.obj[tid] = d_blend.obj[tid];
    blend.bg[tid] = d_blend.bg[tid];
  }
  // 1. labels of [x0 - halo, x0 + 64 + halo) x [y0 - halo, y0 + 16 + halo), clamped into the image
  for (int t = tid; t < lw * lh; t += ovl::kBlock) {
    const int r = t / lw, c = t - r * lw;
    const int x = ovl::clampi(x0 - halo + c, 0, w - 1), y = ovl::clampi(y0 - halo + r, 0, h - 1);
    const size_t p = base + (size_t)y * w + x;
    int32_t l;
    if (a.labels) {
      l = a.labels[p];
    } else {
      const uint8_t* q = a.render + 3 * p;
      l = ovl::label_of_render(q[0], q[1], q[2]);
    }
    lab[r * kLabW + c] = l;
  }
  __syncthreads();
  const bool want_edges = a.contour || a.canny;
  if (want_edges) {
    // 2. e(q) on [x0 - k, x0 + 64 + k) x [y0 - k, y0 + 16 + k)
    for (int t = tid; t < ew * eh; t += ovl::kBlock) {
      const int r = t / ew, c = t - r * ew;
      const int x = x0 - k + c, y = y0 - k + r;
      int32_t e = -1;
      if (x >= 0 && x < w && y >= 0 && y < h) e = ovl::edge_label(&lab[(r + 2) * kLabW + c + 2], kLabW, x, y, w, h);
      edge[r * kEdgeW + c] = e;
    }
    __syncthreads();
    // 3a. rows: rowmax[r][c] = max of edge[r][c .. c + 2k]
    for (int t = tid; t < eh * ovl::kTileW; t += ovl::kBlock) {
      const int r = t / ovl::kTileW, c = t - r * ovl::kTileW;
      int32_t m = edge[r * kEdgeW + c];
#pragma unroll
      for (int d = 1; d <= 2 * k; ++d) m = max(m, edge[r * kEdgeW + c + d]);
      rowmax[r * ovl::kTileW + c] = m;
    }
  }
  __syncthreads();
  // 4. lane -> 4 pixels of one row
  const int row = tid >> 4, col = (tid & 15) * ovl::kGroup;
  const int x = x0 + col, y = y0 + row;
  if (x >= w || y >= h) return;
  const int n_px = min(ovl::kGroup, w - x);
  const bool wide = a.wide != 0;   // then w % 4 == 0 and n_px == 4
  const size_t p = base + (size_t)y * w + x;
  int32_t out[ovl::kGroup], l[ovl::kGroup];
#pragma unroll
  for (int s = 0; s < ovl::kGroup; ++s) {
    l[s] = lab[(row + halo) * kLabW + col + s + halo];
    int32_t m = -1;
    if (want_edges)   // 3b. columns
#pragma unroll
      for (int d = 0; d <= 2 * k; ++d) m = max(m, rowmax[(row + d) * ovl::kTileW + col + s]);
    out[s] = m;
  }
  uint32_t im[12], b3[12], b1[4];   // one byte value per element
  if (a.contour || a.mesh) load_px3(a.images, 3 * p, wide, n_px, im);
  if (a.contour) {
    for (int s = 0; s < ovl::kGroup; ++s) {
      if (s < n_px && out[s] >= 0) {
        const uint8_t* c = a.colors + 3 * ovl::color_of(out[s], a.n_colors);
        b3[3 * s] = c[0]; b3[3 * s + 1] = c[1]; b3[3 * s + 2] = c[2];
      } else {
        b3[3 * s] = im[3 * s]; b3[3 * s + 1] = im[3 * s + 1]; b3[3 * s + 2] = im[3 * s + 2];
      }
    }
    store_px3(a.contour, 3 * p, wide, n_px, b3);
  }
  if (a.canny) {
    for (int s = 0; s < ovl::kGroup; ++s) b1[s] = out[s] >= 0 ? 255 : 0;
    store_px1(a.canny, p, wide, n_px, b1);
  }
  if (a.mask) {
    for (int s = 0; s < ovl::kGroup; ++s) b1[s] = l[s] >= 0 ? 255 : 0;
    store_px1(a.mask, p, wide, n_px, b1);
  }
  if (a.mesh) {
    uint32_t rn[12];
    load_px3(a.render, 3 * p, wide, n_px, rn);
    for (int s = 0; s < ovl::kGroup; ++s)
      for (int ch = 0; ch < 3; ++ch) b3[3 * s + ch] = l[s] >= 0 ? blend.obj[rn[3 * s + ch]] : blend.bg[im[3 * s + ch]];
    store_px3(a.mesh, 3 * p, wide, n_px, b3);
  }
}

// Boxes are taken 256 at a time: lane l looks at box j0 + l and keeps it when it belongs to the tile's image, has no NaN corner and its
// grown rectangle meets the tile; the kept boxes are compacted in ascending j into LDS (block_compact: no atomics, a
// fixed order), and every pixel walks that list from the last to the first under on_frame.  A later chunk holds higher j and overrides.
__global__ __launch_bounds__(256) void draw_boxes_kernel(const uint8_t* __restrict__ images, const float* __restrict__ boxes,
                                                         const int32_t* __restrict__ image_ids, int n_boxes,
                                                         const uint8_t* __restrict__ colors, int n_colors, int h, int w, int tiles_x,
                                                         int tiles_y, int thickness, int wide_i, uint8_t* __restrict__ out) {
  __shared__ int4 corners[ovl::kBlock];
  __shared__ int32_t index[ovl::kBlock];
  __shared__ int32_t wave_count[ovl::kBlock / 64];
  const int tid = threadIdx.x;
  const int per_image = tiles_x * tiles_y;
  const int img = blockIdx.x / per_image, rest = blockIdx.x - img * per_image;
  const int ty = rest / tiles_x, tx = rest - ty * tiles_x;
  const int x0 = tx * ovl::kTileW, y0 = ty * ovl::kTileH;
  const int x = x0 + (tid & 15) * ovl::kGroup, y = y0 + (tid >> 4);
  const bool live = x < w && y < h;   // every lane stays for the barriers
  const int n_px = min(ovl::kGroup, w - x);
  const int grow = thickness / 2;
  int best[ovl::kGroup] = {-1, -1, -1, -1};
  for (int j0 = 0; j0 < n_boxes; j0 += ovl::kBlock) {
    const int j = j0 + tid;
    bool keep = false;
    int4 c = make_int4(0, 0, 0, 0);
    if (j < n_boxes && image_ids[j] == img) {
      keep = true;
      c.x = ovl::box_corner(boxes[4 * j], &keep); c.y = ovl::box_corner(boxes[4 * j + 1], &keep);
      c.z = ovl::box_corner(boxes[4 * j + 2], &keep); c.w = ovl::box_corner(boxes[4 * j + 3], &keep);
      keep = keep && c.x - grow < x0 + ovl::kTileW && c.z + grow >= x0 && c.y - grow < y0 + ovl::kTileH && c.w + grow >= y0;
    }
    int total;
    const int slot = block_compact<ovl::kBlock / 64>(keep, wave_count, &total);   // (its first barrier: the walk of the chunk before is over)
    if (keep) {
      corners[slot] = c;
      index[slot] = j;
    }
    __syncthreads();
    if (live)
#pragma unroll
      for (int s = 0; s < ovl::kGroup; ++s)
        for (int i = total - 1; i >= 0; --i) {
          const int4 b = corners[i];
          if (ovl::on_frame(x + s, y, b.x, b.y, b.z, b.w, thickness)) {
            best[s] = index[i];
            break;
          }
        }
  }
  if (!live) return;
  const bool wide = wide_i != 0;
  const size_t p = ((size_t)img * h + y) * w + x;
  uint32_t b[12];
  load_px3(images, 3 * p, wide, n_px, b);
#pragma unroll
  for (int s = 0; s < ovl::kGroup; ++s)
    if (s < n_px && best[s] >= 0) {
      const uint8_t* c = colors + 3 * (best[s] % n_colors);
      b[3 * s] = c[0]; b[3 * s + 1] = c[1]; b[3 * s + 2] = c[2];
    }
  store_px3(out, 3 * p, wide, n_px, b);
}

static bool aligned4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace mp

using namespace mp;

extern "C" int mp_overlay(const uint8_t* d_images, const uint8_t* d_render, const int32_t* d_labels, const uint8_t* d_colors, int n_colors,
                          int n, int h, int w, int dilate_iterations, uint8_t* d_contour, uint8_t* d_canny, uint8_t* d_mask,
                          uint8_t* d_mesh, mp_stream stream) {
  if (n == 0) return MP_OK;
  MP_REQUIRE(ovl::overlay_args_ok(d_images != nullptr, d_render != nullptr, d_labels != nullptr, d_colors != nullptr, n_colors, n, h, w,
                                  dilate_iterations, d_mesh != nullptr),
             "mp_overlay: needs images, colors and a render or labels (a render for the mesh); n %d >= 0, h %d and w %d in 1 .. %d, "
             "n * h * w * 3 < 2^31, dilate_iterations %d in 0 .. %d, n_colors %d >= 1",
             n, h, w, ovl::kMaxSide, dilate_iterations, ovl::kMaxDilate, n_colors);
  if (!(d_contour || d_canny || d_mask || d_mesh)) return MP_OK;
  OverlayArgs a;
  a.images = d_images; a.render = d_render; a.labels = d_labels; a.colors = d_colors;
  a.contour = d_contour; a.canny = d_canny; a.mask = d_mask; a.mesh = d_mesh;
  a.n_colors = n_colors; a.h = h; a.w = w;
  a.tiles_x = ceil_div(w, ovl::kTileW);
  a.tiles_y = ceil_div(h, ovl::kTileH);
  a.wide = w % 4 == 0 && aligned4(d_images) && aligned4(d_render) && aligned4(d_contour) && aligned4(d_canny) && aligned4(d_mask) && aligned4(d_mesh);
  const long long blocks = (long long)n * a.tiles_x * a.tiles_y;   // at most n * h * w < 2^31 / 3
  hipStream_t s = (hipStream_t)stream;
  const double px = (double)n * h * w;
  ProfScope prof("overlay", 0.0, px * ((d_labels ? 4.0 : 3.0) + (d_contour || d_mesh ? 3.0 : 0.0) + (d_mesh ? 6.0 : 0.0) + (d_contour ? 3.0 : 0.0) +
                                       (d_canny ? 1.0 : 0.0) + (d_mask ? 1.0 : 0.0)), s);
  static_assert(ovl::kMaxDilate == 8, "one instantiation per dilate_iterations");
  void (*const kernels[ovl::kMaxDilate + 1])(OverlayArgs) = {overlay_kernel<0>, overlay_kernel<1>, overlay_kernel<2>, overlay_kernel<3>, overlay_kernel<4>,
                                                             overlay_kernel<5>, overlay_kernel<6>, overlay_kernel<7>, overlay_kernel<8>};
  hipLaunchKernelGGL(kernels[dilate_iterations], dim3((unsigned)blocks), dim3(ovl::kBlock), 0, s, a);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_draw_boxes(const uint8_t* d_images, const float* d_boxes, const int32_t* d_image_ids, int n_boxes, const uint8_t* d_colors,
                             int n_colors, int n, int h, int w, int thickness, uint8_t* d_out, mp_stream stream) {
  if (n == 0) return MP_OK;
  MP_REQUIRE(ovl::boxes_args_ok(d_images != nullptr, d_boxes != nullptr, d_image_ids != nullptr, d_colors != nullptr, d_out != nullptr, n_boxes,
                                n_colors, n, h, w, thickness),
             "mp_draw_boxes: null pointer, or n %d < 0, h %d or w %d outside 1 .. %d, n * h * w * 3 >= 2^31, n_boxes %d < 0, thickness %d "
             "outside 1 .. %d, n_colors %d < 1",
             n, h, w, ovl::kMaxSide, n_boxes, thickness, ovl::kMaxThickness, n_colors);
  const int tiles_x = ceil_div(w, ovl::kTileW), tiles_y = ceil_div(h, ovl::kTileH);
  const int wide = w % 4 == 0 && aligned4(d_images) && aligned4(d_out);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("draw_boxes", 0.0, (double)n * h * w * 6.0, s);
  hipLaunchKernelGGL(draw_boxes_kernel, dim3((unsigned)((long long)n * tiles_x * tiles_y)), dim3(ovl::kBlock), 0, s, d_images, d_boxes, d_image_ids,
                     n_boxes, d_colors, n_colors, h, w, tiles_x, tiles_y, thickness, wide, d_out);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
