// gt_info.hip -- BOP's ground-truth info of rendered objects under an observed frame: pixel counts, visibility fraction, the amodal and
// the modal box and the two masks, per row.
//
// The definition and its fp32 arithmetic are gt_info_core.h (on top of vsd_core.h), shared with the host emulation of the tests; this
// file adds the work distribution, on the walk of depth_walk.h that vsd.hip uses too.  Every per-row result but the final division is an integer count or a
// minimum / maximum, so neither the grid nor the order in which workgroups arrive can change a bit.
//
//   gt_info_init_kernel      the row's accumulators in the workspace: counters 0, extents "untouched"
//   gt_info_count_kernel     grid (row, tile of the canvas, strip of image rows), 4 waves, the walk of depth_walk.h: a wave walks image
//                            rows, a lane owns four consecutive x of each 256-pixel chunk; 16-byte loads (and 4-byte mask stores) when
//                            the width and the bases allow, else guarded scalar accesses with the same results.  A chunk in which no
//                            lane has a positive depth is skipped after its load.  An OUTER tile takes only the > 0 test and the
//                            extents: no ray, no square root, no read of the frame.  The CENTRE tile has the walk's v*v table and u*u
//                            registers.
//                            Predicates are reduced per wave by ballot + population count, x extents from the first / last set bit of the
//                            same ballots (scalar registers), per workgroup through LDS, then one integer atomicAdd per non-zero counter
//                            and one atomicMin / atomicMax per touched bound.
//   gt_info_finalize_kernel  one thread per row: accumulators -> counts, boxes, visib_fract (-1 / NaN for an invalid row)
#include "common.h"
#include "depth_walk.h"
#include "gt_info_core.h"

namespace mp {

using gti::kRowInts;
using vsd::kMaxSide;

__global__ __launch_bounds__(256) void gt_info_init_kernel(int32_t* __restrict__ acc, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int k = i % kRowInts;
  acc[i] = k < gti::kNumCounts ? 0 : (gti::is_min_extent(k - gti::kNumCounts) ? gti::kMinInit : gti::kMaxInit);
}

// x extents of the pixels of ballot m, lane l holding x = x_lane0 + 4 l
__device__ __forceinline__ void gti_extend_x(uint64_t m, int x_lane0, int& lo, int& hi) {
  if (m == 0) return;   // uniform
  lo = min(lo, x_lane0 + 4 * (int)__builtin_ctzll(m));
  hi = max(hi, x_lane0 + 4 * (63 - (int)__builtin_clzll(m)));
}

// four mask bytes (0 / 255) of the pixels x0 .. x0 + 3 of element `at` of M; VEC: at + x0 is a multiple of 4 and M 4-byte aligned
template <bool VEC>
__device__ __forceinline__ void gti_store_mask(uint8_t* __restrict__ M, size_t at, int x0, int w, bool v0, bool v1, bool v2, bool v3) {
  if (VEC) {
    if (x0 < w)
      *reinterpret_cast<uint32_t*>(M + at + x0) = (v0 ? 0xffu : 0u) | (v1 ? 0xff00u : 0u) | (v2 ? 0xff0000u : 0u) | (v3 ? 0xff000000u : 0u);
  } else {
    const bool v[4] = {v0, v1, v2, v3};
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < w) M[at + x0 + k] = v[k] ? 255 : 0;
  }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gt_info_count_kernel(const float* __restrict__ depth_gt, const int32_t* __restrict__ gt_ids,
                                                            const float* __restrict__ depth_test, const int32_t* __restrict__ im_ids,
                                                            const float* __restrict__ K, int h, int w, int canvas, int rows_per_strip,
                                                            float delta, int32_t* __restrict__ acc, uint8_t* __restrict__ mask,
                                                            uint8_t* __restrict__ mask_visib) {
  __shared__ float vv_s[kMaxSide];
  __shared__ int32_t red[4][kRowInts];
  const int row = blockIdx.x, tile = blockIdx.y, n_tiles = canvas * canvas;
  const bool centre = tile == (n_tiles - 1) / 2;
  float Kr[9];
  for (int k = 0; k < 9; ++k) Kr[k] = K[(size_t)row * 9 + k];
  const int y0 = blockIdx.z * rows_per_strip, y1 = min(h, y0 + rows_per_strip);
  const size_t hw = (size_t)h * w;
  uint8_t* M = mask ? mask + (size_t)row * hw : nullptr;
  uint8_t* MV = mask_visib ? mask_visib + (size_t)row * hw : nullptr;
  if (!gti::row_valid(Kr)) {   // uniform over the workgroup; the finalize kernel writes -1 / NaN, the masks of the row are zero
    if (centre)
      for (size_t i = (size_t)y0 * w + threadIdx.x; i < (size_t)y1 * w; i += 256) {
        if (M) M[i] = 0;
        if (MV) MV[i] = 0;
      }
    return;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* G = depth_gt + ((size_t)(gt_ids ? gt_ids[row] : row) * n_tiles + tile) * hw;
  int32_t cnt[gti::kNumCounts] = {0, 0, 0, 0};
  int32_t ext[gti::kNumExtents] = {gti::kMinInit, gti::kMinInit, gti::kMaxInit, gti::kMaxInit, gti::kMinInit, gti::kMinInit, gti::kMaxInit, gti::kMaxInit};
  if (!centre) {
    for (int y = y0 + wave; y < y1; y += 4) {
      const size_t off = (size_t)y * w;
#pragma unroll
      for (int c = 0; c < dw::kChunks; ++c) {
        if (c * 256 >= w) break;   // uniform
        float g[4];
        dw::load4<VEC>(G, off, c * 256 + lane * 4, w, g);
        if (__ballot(gti::is_obj(g[0]) || gti::is_obj(g[1]) || gti::is_obj(g[2]) || gti::is_obj(g[3])) == 0) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const uint64_t m = __ballot(gti::is_obj(g[k]));
          cnt[gti::kAll] += __popcll(m);
          gti_extend_x(m, c * 256 + k, ext[0], ext[2]);
        }
        ext[1] = min(ext[1], y);
        ext[3] = max(ext[3], y);
      }
    }
  } else {
    dw::fill_vv(Kr, y0, y1, vv_s);
    __syncthreads();
    float uu[dw::kChunks][4];
    dw::fill_uu(Kr, lane, uu);
    const float* T = depth_test + (size_t)(im_ids ? im_ids[row] : row) * hw;
    for (int y = y0 + wave; y < y1; y += 4) {
      const float vv = vv_s[y - y0];
      const size_t off = (size_t)y * w;
#pragma unroll
      for (int c = 0; c < dw::kChunks; ++c) {
        if (c * 256 >= w) break;   // uniform
        const int x0 = c * 256 + lane * 4;
        float g[4], t[4];
        dw::load4<VEC>(G, off, x0, w, g);
        if (__ballot(gti::is_obj(g[0]) || gti::is_obj(g[1]) || gti::is_obj(g[2]) || gti::is_obj(g[3])) == 0) {   // in neither mask
          if (M) gti_store_mask<VEC>(M, off, x0, w, false, false, false, false);
          if (MV) gti_store_mask<VEC>(MV, off, x0, w, false, false, false, false);
          continue;
        }
        dw::load4<VEC>(T, off, x0, w, t);
        bool obj[4], vis[4];
        bool any_vis = false;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const gti::Pixel p = gti::classify(g[k], t[k], vsd::ray_factor(uu[c][k], vv), delta);
          obj[k] = p.obj;
          vis[k] = p.vis;
          const uint64_t m_obj = __ballot(p.obj), m_vis = __ballot(p.vis);
          cnt[gti::kImage] += __popcll(m_obj);
          cnt[gti::kValid] += __popcll(__ballot(p.valid));
          cnt[gti::kVisib] += __popcll(m_vis);
          gti_extend_x(m_obj, c * 256 + k, ext[0], ext[2]);
          gti_extend_x(m_vis, c * 256 + k, ext[4], ext[6]);
          any_vis = any_vis || m_vis != 0;
        }
        ext[1] = min(ext[1], y);
        ext[3] = max(ext[3], y);
        if (any_vis) {   // uniform
          ext[5] = min(ext[5], y);
          ext[7] = max(ext[7], y);
        }
        if (M) gti_store_mask<VEC>(M, off, x0, w, obj[0], obj[1], obj[2], obj[3]);
        if (MV) gti_store_mask<VEC>(MV, off, x0, w, vis[0], vis[1], vis[2], vis[3]);
      }
    }
    cnt[gti::kAll] = cnt[gti::kImage];
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < gti::kNumCounts; ++k) red[wave][k] = cnt[k];
#pragma unroll
    for (int k = 0; k < gti::kNumExtents; ++k) red[wave][gti::kNumCounts + k] = ext[k];
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= kRowInts) return;
  int32_t* dst = acc + (size_t)row * kRowInts + k;
  if (k < gti::kNumCounts) {
    const int32_t s = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
    if (s != 0) atomicAdd(dst, s);
    return;
  }
  const int e = k - gti::kNumCounts;
  // tile coordinates -> image coordinates: x extents are the even entries of a box, y extents the odd ones
  const int shift = (e & 1) ? gti::tile_shift(tile / canvas, canvas, h) : gti::tile_shift(tile % canvas, canvas, w);
  if (gti::is_min_extent(e)) {
    const int32_t v = min(min(red[0][k], red[1][k]), min(red[2][k], red[3][k]));
    if (v != gti::kMinInit) atomicMin(dst, v + shift);
  } else {
    const int32_t v = max(max(red[0][k], red[1][k]), max(red[2][k], red[3][k]));
    if (v != gti::kMaxInit) atomicMax(dst, v + shift);
  }
}

__global__ __launch_bounds__(256) void gt_info_finalize_kernel(const float* __restrict__ K, int b, const int32_t* __restrict__ acc,
                                                               int32_t* __restrict__ counts, int32_t* __restrict__ boxes,
                                                               float* __restrict__ fract) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= b) return;
  const bool ok = gti::row_valid(K + (size_t)row * 9);
  const int32_t* a = acc + (size_t)row * kRowInts;
  for (int k = 0; k < gti::kNumCounts; ++k) counts[(size_t)row * gti::kNumCounts + k] = ok ? a[k] : -1;
  for (int q = 0; q < 2; ++q) {
    int32_t out[4] = {-1, -1, -1, -1};
    if (ok) gti::box(a + gti::kNumCounts + 4 * q, out);
    for (int k = 0; k < 4; ++k) boxes[(size_t)row * gti::kNumExtents + 4 * q + k] = out[k];
  }
  fract[row] = ok ? gti::visib_fract(a[gti::kVisib], a[gti::kAll]) : vsd::quiet_nan();
}

}  // namespace mp

using namespace mp;

extern "C" size_t mp_gt_info_workspace_bytes(int b) {
  if (b < 0) return 0;
  return align256((size_t)b * kRowInts * sizeof(int32_t)) + 256;
}

extern "C" int mp_gt_info(const float* d_depth_gt, const int32_t* d_gt_ids, const float* d_depth_test, const int32_t* d_im_ids, int n_gt, int n_im,
                          const float* d_K, int b, int h, int w, int canvas, float delta, int split, int32_t* d_counts, int32_t* d_boxes,
                          float* d_visib_fract, uint8_t* d_mask, uint8_t* d_mask_visib, void* d_workspace, size_t workspace_bytes,
                          mp_stream stream) {
  MP_REQUIRE(b >= 0, "mp_gt_info: b %d < 0", b);
  MP_REQUIRE(h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide, "mp_gt_info: map %d x %d outside [1, %d]", h, w, kMaxSide);
  MP_REQUIRE(gti::canvas_ok(canvas), "mp_gt_info: canvas %d is not 1 or 3", canvas);
  MP_REQUIRE(split >= 0, "mp_gt_info: split < 0");
  MP_REQUIRE(n_gt >= 0 && n_im >= 0, "mp_gt_info: negative map count");
  if (b == 0) return MP_OK;
  MP_REQUIRE(d_depth_gt && d_depth_test && d_K && d_counts && d_boxes && d_visib_fract && d_workspace, "mp_gt_info: null pointer");
  MP_REQUIRE(n_gt >= 1 && n_im >= 1, "mp_gt_info: no depth maps");
  // without ids the maps are row-aligned: there must be one per row
  MP_REQUIRE((d_gt_ids || n_gt >= b) && (d_im_ids || n_im >= b), "mp_gt_info: fewer maps than rows and no ids");
  MP_REQUIRE(workspace_bytes >= mp_gt_info_workspace_bytes(b), "mp_gt_info: workspace too small");
  const int n_tiles = canvas * canvas;
  const dw::Strips st = dw::strips_of(split, 4096, (long)b * n_tiles, h);   // a few thousand workgroups when rows and tiles cannot give them
  const bool vec = dw::vec_ok(w, {d_depth_gt, d_depth_test}, {d_mask, d_mask_visib});
  int32_t* acc = (int32_t*)d_workspace;
  hipStream_t s = (hipStream_t)stream;
  const double n_masks = (d_mask ? 1.0 : 0.0) + (d_mask_visib ? 1.0 : 0.0);
  ProfScope prof("gt_info", 0.0, (double)b * h * w * (4.0 * n_tiles + 4.0 + n_masks), s);
  hipLaunchKernelGGL(gt_info_init_kernel, dim3(ceil_div((long)b * kRowInts, 256)), dim3(256), 0, s, acc, b * kRowInts);
  MP_CHECK_HIP(hipGetLastError());
  const dim3 grid(b, n_tiles, st.strips);
  if (vec)
    hipLaunchKernelGGL(gt_info_count_kernel<true>, grid, dim3(256), 0, s, d_depth_gt, d_gt_ids, d_depth_test, d_im_ids, d_K, h, w, canvas, st.rows_per_strip, delta,
                       acc, d_mask, d_mask_visib);
  else
    hipLaunchKernelGGL(gt_info_count_kernel<false>, grid, dim3(256), 0, s, d_depth_gt, d_gt_ids, d_depth_test, d_im_ids, d_K, h, w, canvas, st.rows_per_strip, delta,
                       acc, d_mask, d_mask_visib);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(gt_info_finalize_kernel, dim3(ceil_div(b, 256)), dim3(256), 0, s, d_K, b, acc, d_counts, d_boxes, d_visib_fract);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
