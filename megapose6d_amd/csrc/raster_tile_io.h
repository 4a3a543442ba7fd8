// raster_tile_io.h -- PRIVATE, device-only: how the tile kernels (raster.hip, raster_scene.hip) read a binned record and how a wave files,
// stages and stores the pixels of its 8x8 tile: "which kernel writes a tile does not change a bit" holds because there is ONE writer.
// Everything is __forceinline__ and small state travels by value: a reference to an aggregate across a real call boundary is built in
// scratch memory, and raster_tiles is compiled for three waves per SIMD with no register to spare.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

#include "raster_core.h"

namespace mp {

// Intra-wave LDS hand-off: the LDS unit executes one wave's DS operations in issue order, so all that is needed for lane A's write
// to be seen by lane B's later read is that the compiler keeps the program order (the asm is a compiler barrier) and that pending DS
// results have landed.  Unlike a workgroup-scope fence this does NOT wait for vmcnt: global loads issued as prefetches for the next
// view stay in flight across it.
__device__ __forceinline__ void wave_lds_fence() {
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_wave_barrier();
}

// a TileRec as two 16-byte loads (a struct copy is split into six ushort + four dword loads by the compiler)
__device__ __forceinline__ rc::TileRec load_tile_rec(const rc::TileRec* __restrict__ p) {
  const int4 a = reinterpret_cast<const int4*>(p)[0], b = reinterpret_cast<const int4*>(p)[1];
  rc::TileRec r;
  r.rx0 = (short)(a.x & 0xFFFF); r.ry0 = (short)(a.x >> 16);
  r.rx1 = (short)(a.y & 0xFFFF); r.ry1 = (short)(a.y >> 16);
  r.rx2 = (short)(a.z & 0xFFFF); r.ry2 = (short)(a.z >> 16);
  r.pad0 = (short)(a.w & 0xFFFF);   // flags (orientation swap / clipped)
  r.pad1 = 0;
  r.iz0 = __int_as_float(b.x); r.iz1 = __int_as_float(b.y); r.iz2 = __int_as_float(b.z);
  r.id = b.w;
  return r;
}

// OUT = OUT_F16 (MP_RASTER_F16, the "fp16 renders" mode of BASELINE.json configs[4]): `out` holds IEEE binary16 elements -- same element
// strides, every written channel (renders and the fused crop) is rounded to nearest-even on its way out; nothing else changes.
// OUT = OUT_XREC (MP_RASTER_XREC): `out` holds the bf16 pixel RECORDS the exact-piece stem convolution consumes (conv_stem.hip):
// [x1,x2,x3 of every crop channel | the 8-bit integer k of every render channel | zero padding], stride_x = record length; the
// record is staged in LDS in that form and leaves as 16-byte chunks.  Channel numbers (c_rgb, c_normals, stride_view, crop.c0) stay
// logical channel numbers; stride_v / stride_y / stride_x count bf16 elements.
constexpr int OUT_F32 = 0, OUT_F16 = 1, OUT_XREC = 2;

// The writer of one wave's tile.  LDS staging area of the wave: [64 pixels][run] floats, lane = pixel (lane & 7, lane >> 3) of the tile --
// or (OUT_XREC) the pixel records themselves, [64][stride_x] bf16 (never larger than [64][run] floats: the launcher checks).
// DEPTHREC (OUT_XREC only): the record's fp32-kind channels are a general mask and depth channels are normalised here (RGBD models); false =
// the fp32-kind channels are the crop's leading ones, no depth channel (the RGB models: free of the extra arithmetic -- raster_tiles sits
// exactly at its register budget).
template <int OUT, bool DEPTHREC>
struct TileWriter {
  float* stage;             // the wave's staging area
  float* my_stage;          // the lane's pixel in it (fp32 / binary16 forms)
  unsigned short* my_rec;   // the lane's pixel record in it (OUT_XREC)
  int c_lo, run;            // the channel run [c_lo, c_lo + run) one launch stages
  long long stride_x;
  // (OUT_XREC) logical channel c is fp32-kind (three record slots) iff bit c of xrec_mask is set -- the crop's channels and, for RGBD
  // models, every depth channel --; the fp32-kind channels come first in the record, in channel order, then the integer channels
  uint32_t xrec_mask;
  int xrec_nf, depth_mode;
  float depth_zr;

  __device__ __forceinline__ TileWriter(float* stage_, int lane, int c_lo_, int run_, long long stride_x_, uint32_t xrec_mask_, int crop_C,
                                        int depth_mode_)
      : stage(stage_), my_stage(stage_ + (size_t)lane * run_), my_rec(reinterpret_cast<unsigned short*>(stage_) + (size_t)lane * (int)stride_x_),
        c_lo(c_lo_), run(run_), stride_x(stride_x_), xrec_mask(xrec_mask_), xrec_nf(DEPTHREC ? __builtin_popcount(xrec_mask_) : crop_C),
        depth_mode(depth_mode_), depth_zr(1.f) {}

  // file a channel value into the lane's pixel in whichever form the launch stages; ch = logical channel number
  __device__ __forceinline__ void put(int ch, float v) const {
    if constexpr (OUT == OUT_XREC) {
      const int f_below = DEPTHREC ? __builtin_popcount(xrec_mask & ((1u << ch) - 1u)) : min(ch, xrec_nf);   // fp32-kind channels in front of ch (ch < 32)
      if (DEPTHREC ? (bool)((xrec_mask >> ch) & 1u) : ch < xrec_nf) {   // exact truncation split x = x1 + x2 + x3 (three bf16 pieces)
        const unsigned b1 = __float_as_uint(v) & 0xFFFF0000u;
        const float r1 = v - __uint_as_float(b1);
        const unsigned b2 = __float_as_uint(r1) & 0xFFFF0000u;
        const float r2 = r1 - __uint_as_float(b2);
        my_rec[3 * f_below] = (unsigned short)(b1 >> 16); my_rec[3 * f_below + 1] = (unsigned short)(b2 >> 16);
        my_rec[3 * f_below + 2] = (unsigned short)(__float_as_uint(r2) >> 16);
      } else {              // an integer 0..255: one bf16, exactly
        my_rec[3 * xrec_nf + (ch - f_below)] = (unsigned short)(__float_as_uint(v) >> 16);
      }
    } else {
      my_stage[ch - c_lo] = v;
    }
  }

  // (OUT_XREC, DEPTHREC) depth channels enter the record NORMALISED, with the operations of normalize_depth_kernel (crop.hip; reference
  // models/pose_rigid.py:466-496) in the same order, so that the three pieces add up to the fp32 tensor path's value bit for bit
  __device__ __forceinline__ void set_item(const float* __restrict__ depth_tcr, int item) {
    if constexpr (OUT == OUT_XREC && DEPTHREC) {
      if (depth_mode != 0 && depth_tcr) depth_zr = depth_tcr[3 * (size_t)item + 2];
    }
  }
  __device__ __forceinline__ float nd(float d) const {
    if constexpr (OUT == OUT_XREC && DEPTHREC) {
      if (depth_mode == 1) d = d / depth_zr;
      else if (depth_mode == 2) d = fminf(fmaxf(d / depth_zr, 0.f), 2.f) - 1.f;
      else if (depth_mode == 3) d = fminf(fmaxf(d - depth_zr, -2.f), 2.f);
    }
    return d;
  }

  // (OUT_XREC) zero the lane's whole record (the padding slots are never written again)
  __device__ __forceinline__ void clear_record() const {
    if constexpr (OUT == OUT_XREC) {
      uint4* z = reinterpret_cast<uint4*>(my_rec);
      for (int q = 0; q < (int)stride_x / 8; ++q) z[q] = make_uint4(0u, 0u, 0u, 0u);
    }
  }

  // nothing of a view reaches the tile: its channels (at channel offset cv) are background
  __device__ __forceinline__ void background(int cv, int c_rgb, int c_normals, int c_depth, bool do_norm, bool do_depth) const {
    if constexpr (OUT != OUT_XREC) {   // (a stem record is cleared as a whole)
      if (c_rgb >= 0) { put(c_rgb + cv, 0.f); put(c_rgb + cv + 1, 0.f); put(c_rgb + cv + 2, 0.f); }
      if (do_norm) { put(c_normals + cv, 0.f); put(c_normals + cv + 1, 0.f); put(c_normals + cv + 2, 0.f); }
      if (do_depth) put(c_depth + cv, 0.f);
    } else {
      if (do_depth) put(c_depth + cv, nd(0.f));   // background depth 0 is normalised like any other value (e.g. to -1)
    }
  }

  // the crop role's result for the lane's pixel: C = 3 | 4 channels from c0 (the observation's depth channel is normalised like the rendered ones)
  __device__ __forceinline__ void put_crop(int c0, int C, float4 v) const {
    put(c0, v.x); put(c0 + 1, v.y); put(c0 + 2, v.z);
    if (C == 4) put(c0 + 3, nd(v.w));
  }

  // store the staged tile (after a wave_lds_fence): each of the tile's 8 rows leaves as one contiguous run of 8 pixels x `run` channels
  // (only the channels of run_mask); tiles on the right / bottom image edge are cut to cols x rows pixels
  __device__ __forceinline__ void store(float* __restrict__ out, int item, long long stride_v, long long stride_y, int tile_x0, int tile_y0,
                                        int w, int h, int lane, uint32_t run_mask) const {
    const int cols = min(rc::TILE, w - tile_x0), rows = min(rc::TILE, h - tile_y0);
    const int per_row = cols * run;   // <= 256 floats
    if constexpr (OUT == OUT_XREC) {
      // the tile's records sit in LDS as [8 rows][8 pixels][stride_x bf16]; a tile row = cols * stride_x / 8 contiguous 16-byte chunks
      const int rowlen = cols * ((int)stride_x / 8);   // <= 40 chunks
      unsigned short* out_item = reinterpret_cast<unsigned short*>(out) + (size_t)item * stride_v;
      const uint4* recs = reinterpret_cast<const uint4*>(stage);
      if (lane < rowlen)
        for (int row = 0; row < rows; ++row)
          *reinterpret_cast<uint4*>(out_item + (size_t)(tile_y0 + row) * stride_y + (size_t)tile_x0 * stride_x + (size_t)lane * 8) =
              recs[row * 8 * ((int)stride_x / 8) + lane];
    } else {
      typedef typename std::conditional<OUT == OUT_F16, _Float16, float>::type Elem;   // (_Float16)x = v_cvt_f16_f32: round to nearest even
      Elem* out_item = reinterpret_cast<Elem*>(out) + (size_t)item * stride_v + c_lo;
      for (int i = lane; i < per_row; i += 64) {
        const int x = i / run, c = i - x * run;   // once per lane and 64-float slice, reused for all 8 rows
        if (!((run_mask >> c) & 1u)) continue;
        Elem* o = out_item + (size_t)tile_y0 * stride_y + (size_t)(tile_x0 + x) * stride_x + c;
        const float* sp = stage + (size_t)x * run + c;
        for (int row = 0; row < rows; ++row) o[(size_t)row * stride_y] = (Elem)sp[(size_t)row * 8 * run];
      }
    }
  }
};

}  // namespace mp
