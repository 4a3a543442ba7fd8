// surface_sample_core.h -- the rules of sampling points uniformly over the surface of triangle meshes (the reference's
// MeshDataBase.batched(resample_n_points=n), trimesh.sample.sample_surface: a face drawn with probability proportional to its area, then
// a point uniform in that face) that run on the device (surface_sample.hip), shared with the host emulation
// (tests/surface_sample_emul.cpp) the way model_info_core.h is shared with its own.  Randomness comes in as an input: the engine draws
// nothing, and no grid, block size or arrival order changes a bit of the result.
//
// CONTRACT (mp_surface_sample)
//   * INPUTS.  vertices [V_total,3] fp32; faces [F_total,3] int32, indices local to the object; vert_off, face_off [n_obj + 1] int32
//     prefix arrays (object o owns vertices vert_off[o] .. vert_off[o+1] - 1 and faces face_off[o] .. face_off[o+1] - 1); u
//     [n_obj,count,3] fp32 uniforms; 1 <= count; 1 <= F_o <= 2^22 faces per object.
//   * WEIGHT.  For face (a, b, c): e1 = b - a, e2 = c - a in fp32; the cross product with every component one fmaf on one product,
//     cx = fmaf(e1y, e2z, -(e1z * e2y)), cy = fmaf(e1z, e2x, -(e1x * e2z)), cz = fmaf(e1x, e2y, -(e1y * e2x)) [cross];
//     n2 = fmaf(cz, cz, fmaf(cy, cy, cx * cx)); w = sqrtf(n2), correctly rounded on both sides [weight].  Twice the area: only ratios
//     matter.
//   * FAILED OBJECT.  A non-finite coordinate of a referenced vertex, an index outside 0 .. V_o - 1, a weight that is not finite (the
//     fp32 edges or their product overflowed), or every weight zero: all points of that object NaN, all its face ids -1 (the convention
//     of mp_model_info / mp_vsd).  Other objects of the launch are unaffected, bit for bit.  An index is tested BEFORE the vertex is
//     loaded [face_ok], and a failed object's vertices are never gathered.
//   * QUANTISE.  wmax = the object's largest weight (a maximum is order-free) = m * 2^e, m in [0.5, 1) [exponent_of];
//     q_f = (uint64) floor(ldexp((double) w_f, 40 - e)) < 2^40 [quantise], so the total stays below 2^62 at 2^22 faces.  A face more
//     than 2^40 times smaller than the largest gets weight 0 and is never drawn.
//   * SCAN.  C_f = the inclusive prefix sum of q over the object's faces, uint64: integer sums are exact, any scan order gives the same.
//   * PICK.  k = min((uint32)(u0 * 2^24), 2^24 - 1), 0 for a negative or NaN u0 [pick_k] (torch.rand fp32 values are multiples of
//     2^-24, so this is exact); t = floor(total * k / 2^24) = hi * k + ((lo * k) >> 24) with hi = total >> 24, lo = total & (2^24 - 1)
//     [pick_t]; the face is the LOWEST f with C_f > t: a zero-weight face is never picked, and t < total always finds one.  The search
//     counts the entries <= t in a fixed number of steps [count_le]: first over the prefix of the blocks, then inside one block.
//   * POINT.  r1 = u1, r2 = u2, each clamped to [0, 1], NaN -> 0; if r1 + r2 > 1.0f (the fp32 sum) then r1 = 1 - r1, r2 = 1 - r2
//     (trimesh's reflection); p = fmaf(e2, r2, fmaf(e1, r1, a)) per component [barycentric, point_axis].
//   * OUTPUTS.  points [n_obj,count,3] fp32, face [n_obj,count] int32 (local to the object).
//
// WORK.  An object's faces are cut into blocks of `block` faces (kDefaultBlock, or a forced multiple of 64 for tests, so that a few hundred
// faces make several blocks); a job is one block, and one prefix array of n_obj + 1 job counts is the only index.  An object has at most
// kMaxBlocks blocks, so that its block prefix fits the LDS of the pick pass and one workgroup scans it in one pass.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define SSAMP_HD __host__ __device__ __forceinline__
#else
#define SSAMP_HD inline
#endif

namespace mp {
namespace ssamp {

constexpr int kThreads = 256;            // lanes of a workgroup
constexpr int kBlockStep = 64;           // a forced block is a multiple of this
constexpr int kMaxBlock = 2048;          // faces of a job, at most (and the library's choice)
constexpr int kDefaultBlock = 2048;      // block == 0
constexpr int kMaxBlocks = 2048;         // blocks of one object: 16 KiB of uint64 prefix in LDS
constexpr int kMaxFaces = 1 << 22;       // faces of one object
constexpr int kSearchSteps = 11;         // ceil(log2) of both search ranges (kMaxBlocks entries, kMaxBlock entries)
constexpr int kWeightBits = 40;          // q < 2^40
constexpr int kFailed = -2147483647 - 1; // the exponent slot of a failed object
constexpr long long kMaxJobs = 2147483647LL;

static_assert((1 << kSearchSteps) == kMaxBlocks && (1 << kSearchSteps) == kMaxBlock, "count_le covers ranges of at most 2^kSearchSteps");

SSAMP_HD bool block_ok(int block) { return block == 0 || (block >= kBlockStep && block <= kMaxBlock && block % kBlockStep == 0); }

SSAMP_HD int block_of(int block) { return block == 0 ? kDefaultBlock : block; }

SSAMP_HD long long n_blocks(int n_faces, int block) { return ((long long)n_faces + block - 1) / block; }

// faces of an object the launch takes at this block size
SSAMP_HD bool faces_ok(long long n_faces, int block) { return n_faces >= 1 && n_faces <= kMaxFaces && n_blocks((int)n_faces, block) <= kMaxBlocks; }

SSAMP_HD bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

// the three indices of a face against the object's vertex count: tested before any vertex is loaded
SSAMP_HD bool face_ok(int32_t ia, int32_t ib, int32_t ic, int32_t n_vert) {
  return ia >= 0 && ia < n_vert && ib >= 0 && ib < n_vert && ic >= 0 && ic < n_vert;
}

SSAMP_HD void cross(float e1x, float e1y, float e1z, float e2x, float e2y, float e2z, float* cx, float* cy, float* cz) {
  *cx = fmaf(e1y, e2z, -(e1z * e2y));
  *cy = fmaf(e1z, e2x, -(e1x * e2z));
  *cz = fmaf(e1x, e2y, -(e1y * e2x));
}

// twice the area of triangle (a, b, c)
SSAMP_HD float weight(const float* a, const float* b, const float* c) {
  float cx, cy, cz;
  cross(b[0] - a[0], b[1] - a[1], b[2] - a[2], c[0] - a[0], c[1] - a[1], c[2] - a[2], &cx, &cy, &cz);
  return sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));
}

// e of wmax = m * 2^e, m in [0.5, 1); wmax is finite and positive
SSAMP_HD int exponent_of(float wmax) {
  int e;
  frexpf(wmax, &e);
  return e;
}

SSAMP_HD uint64_t quantise(float w, int e) { return (uint64_t)floor(ldexp((double)w, kWeightBits - e)); }

SSAMP_HD uint32_t pick_k(float u0) {
  if (!(u0 > 0.0f)) return 0u;                 // negative, zero, NaN
  if (u0 >= 1.0f) return (1u << 24) - 1u;
  const uint32_t k = (uint32_t)(u0 * 16777216.0f);
  return k < (1u << 24) - 1u ? k : (1u << 24) - 1u;
}

SSAMP_HD uint64_t pick_t(uint64_t total, uint32_t k) {
  const uint64_t hi = total >> 24, lo = total & ((1ull << 24) - 1ull);
  return hi * k + ((lo * k) >> 24);
}

// the number of entries of the non-decreasing a[0 .. n - 1] that are <= t, for n <= 2^kSearchSteps and a[n - 1] > t (so the answer is
// at most n - 1 = the index of the lowest entry > t): kSearchSteps steps whatever the data
SSAMP_HD int count_le(const uint64_t* a, int n, uint64_t t) {
  int pos = 0;
#pragma unroll
  for (int s = kSearchSteps - 1; s >= 0; --s) {
    const int next = pos + (1 << s);
    if (next <= n && a[next - 1] <= t) pos = next;
  }
  return pos < n - 1 ? pos : n - 1;
}

SSAMP_HD float clamp01(float r) { return r > 0.0f ? (r < 1.0f ? r : 1.0f) : 0.0f; }   // NaN -> 0

SSAMP_HD void barycentric(float u1, float u2, float* r1, float* r2) {
  float a = clamp01(u1), b = clamp01(u2);
  if (a + b > 1.0f) {
    a = 1.0f - a;
    b = 1.0f - b;
  }
  *r1 = a;
  *r2 = b;
}

SSAMP_HD float point_axis(float a, float b, float c, float r1, float r2) { return fmaf(c - a, r2, fmaf(b - a, r1, a)); }

}  // namespace ssamp
}  // namespace mp
