// depth_walk.h -- the walk over depth maps that vsd.hip and gt_info.hip share.  A workgroup (4 waves) owns a strip of image rows of one
// row of the batch; a wave walks the strip's image rows; a lane owns four consecutive x of each 256-pixel chunk of an image row.  v*v of
// the strip's image rows is an LDS table, u*u of a lane's pixels stays in registers (vsd_core.h: ray_v, ray_u).  What a kernel does with
// the pixels (which chunks it skips, what it counts and stores) is its own.
#pragma once
#include <initializer_list>

#include "common.h"
#include "vsd_core.h"

namespace mp {
namespace dw {

constexpr int kChunks = vsd::kMaxSide / 256;   // 256-pixel chunks of an image row

// the pixels x0 .. x0 + 3 of the image row at element `off` of P (0 outside the width); VEC: off + x0 is a multiple of 4, P 16-byte aligned
template <bool VEC>
__device__ __forceinline__ void load4(const float* __restrict__ P, size_t off, int x0, int w, float (&d)[4]) {
  d[0] = d[1] = d[2] = d[3] = 0.f;
  if (VEC) {
    if (x0 < w) {   // w % 4 == 0: the four pixels are inside together
      const float4 q = *reinterpret_cast<const float4*>(P + off + x0);
      d[0] = q.x; d[1] = q.y; d[2] = q.z; d[3] = q.w;
    }
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (x0 + k < w) d[k] = P[off + x0 + k];
  }
}

// v*v of the image rows y0 .. y1 - 1 into the workgroup's table; the caller puts the barrier before the first read
__device__ __forceinline__ void fill_vv(const float* Kr, int y0, int y1, float* __restrict__ vv_s) {
  for (int i = threadIdx.x; i < y1 - y0; i += 256) {
    const float v = vsd::ray_v(Kr, y0 + i);
    vv_s[i] = v * v;
  }
}

// u*u of the pixels of `lane`: uu[c][k] belongs to x = 256 c + 4 lane + k
__device__ __forceinline__ void fill_uu(const float* Kr, int lane, float (&uu)[kChunks][4]) {
#pragma unroll
  for (int c = 0; c < kChunks; ++c)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const float u = vsd::ray_u(Kr, c * 256 + lane * 4 + k);
      uu[c][k] = u * u;
    }
}

// Strips of image rows: `split` of them when it is > 0, else enough for `wanted` workgroups given the `given` ones of the other grid
// dimensions; at least one image row per wave, and no empty strip.
struct Strips { int rows_per_strip, strips; };
static inline Strips strips_of(int split, int wanted, long given, int h) {
  int strips = split > 0 ? split : ceil_div(wanted, given);
  const int max_strips = ceil_div(h, 4);
  strips = strips < 1 ? 1 : (strips > max_strips ? max_strips : strips);
  const int rps = ceil_div(h, strips);
  return {rps, ceil_div(h, rps)};
}

// whether the VEC path may run: every image row starts on a 16-byte boundary of every map (and on a 4-byte one of every mask)
static inline bool vec_ok(int w, std::initializer_list<const void*> maps, std::initializer_list<const void*> masks = {}) {
  uintptr_t m16 = 0, m4 = 0;
  for (const void* p : maps) m16 |= (uintptr_t)p;
  for (const void* p : masks) m4 |= (uintptr_t)p;
  return w % 4 == 0 && m16 % 16 == 0 && m4 % 4 == 0;
}

}  // namespace dw
}  // namespace mp
