// conv.hip -- fp32 implicit-GEMM convolution on MFMA (v_mfma_f32_32x32x2_f32) for gfx950.
//
// Replaces the cuDNN convolutions behind `self.backbone(x)`
// (reference: src/megapose/models/pose_rigid.py:323; layers in
//  src/megapose/models/torchvision_resnet.py:74-120,181-316 and src/megapose/models/wide_resnet.py:29-111).
//
// Formulation ("row-run implicit GEMM"): activations are padded NHWC, so for a fixed kernel row kh the
// (kw, c) taps of one output pixel are ONE contiguous run of KW*C floats in memory, and the zero border
// makes bounds checks unnecessary.  GEMM view:  M = N*Ho*Wo output pixels, N = Cout, K = KH * (KW*C).
// The K loop walks (kh, 32-float chunk of the run); A tiles are gathered row-by-row (128-B contiguous
// pieces), B tiles come from a pre-packed weight blob laid out in exactly the loop order.  Both are
// staged through LDS (double-buffered, register prefetch), read back as 16-B fragments, and fed to the
// 32x32x2 fp32 MFMA, whose k-order within a 8-float group is permuted identically for A and B (free).
// Epilogue fuses bias (folded eval-BN), residual add, ReLU and an optional second "pre-activated"
// output relu(y*s+t) for pre-activation (WideResNet) blocks.
//
// Roofline: MFMA-bound (fp32 matrix peak 157.3 TFLOP/s, MI355X_MICROARCH.md).
#include <cstdlib>

#include <algorithm>
#include <string>
#include <vector>

#include "conv_common.h"

namespace mp {

// Clock telemetry (always on, ~free): every 64th workgroup adds the shader cycles (s_memtime) and the 100 MHz real-time ticks
// (s_memrealtime) it spent in its K loop; mp_conv_clock_read turns the sums into the effective shader clock the convolutions ran at.
// The fp32-MFMA peak scales with that clock, and under real (bit-toggling) operands this part sustains ~2.15 GHz, not 2.4.
__device__ unsigned long long g_conv_clk[2];
#ifdef MP_RASTER_PROF   // scripts/microbench build only: where a wave's cycles go inside one K-loop iteration: 0 load issue,
// 1 MFMA groups 0-1, 2 wait for the global loads + LDS writes, 3 MFMA groups 2-3, 4 barrier
__device__ unsigned long long g_conv_seg[8];
#define CPROF(slot)                                                    \
  {                                                                    \
    const unsigned long long cprof_n = __builtin_readcyclecounter();   \
    cprof_acc[slot] += cprof_n - cprof_t;                              \
    cprof_t = cprof_n;                                                 \
  }
#else
#define CPROF(slot)
#endif

constexpr int CONV_BM = 128;   // output pixels per tile; the tile width BN (64 or 128 output channels) is the one the weights are packed for

// Tile: CONV_BM x BN, four waves of 64 x BN/2 (2 x BN/64 accumulators of 32 x 32).  A and B come through buffer_load_dwordx4: one scalar
// resource per operand (A: based at the tile's first pixel -- addresses ascend with the row index, the tile spans a few image rows; B: at
// this n-block's packed weights; neither range check can trigger, num_records = 2^32 - 1), a loop-invariant 32-bit lane offset and the
// chunk position in the scalar offset.  K loop: one 32-float chunk and one barrier per iteration; chunk c+1 is requested at the top and
// written to the other LDS buffer under an MFMA group.
// waves_per_eu(2,2): LDS already limits residency to 2 workgroups per CU (= 2 waves per SIMD); telling the compiler so lets it
// keep the prefetch registers live across the MFMA block instead of spilling them to scratch to chase a higher occupancy.
// RAGGED: K runs that are not a multiple of 32 (the 7x7 / 5x5 stems): per-lane run position.  SPLITK: blockIdx.y owns a range of chunks
// and writes raw partial sums (conv_splitk_reduce applies the epilogue).
// AHALF: the INPUT tensor holds IEEE binary16 values (the "fp16 renders" CNN input the rasteriser writes with MP_RASTER_F16): the A
// tile is fetched as 8-byte pieces (4 halves), stays packed in registers across the MFMA block and is widened to fp32 on its way
// into LDS -- everything after the LDS store (fragments, MFMA, epilogue) is the fp32 path unchanged.
// (Measured against this schedule, bit-identical and within +-1 %, and dropped: persistent workgroups, a 16-byte LDS-transposed epilogue,
//  global_load addressing, a two-chunks-ahead pipeline -- profiles/r03_conv_ab_epilogue_persistent.txt, docs/history.md section 3.1.)
template <int BN, bool RAGGED, bool SPLITK, bool AHALF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_nhwc_f32_mfma(ConvParams p) {
  constexpr int BM = CONV_BM, WM = 64, WN = BN / 2;
  constexpr int NBUF = 2;
  constexpr int LDT = LDS_LD;
  constexpr int TM = WM / 32, TN = WN / 32;
  constexpr int A_LD4 = BM / 32;  // float4 loads per thread for the A tile
  constexpr int B_LD4 = BN / 32;
  static_assert(BN == 64 || BN == 128, "staging code is written for BM = 128, BN in {64, 128}");

  const bool clk_sample = threadIdx.x == 0 && (blockIdx.x & 63) == 0;
  unsigned long long clk_c0 = 0, clk_r0 = 0;
  if (clk_sample) { clk_c0 = __builtin_readcyclecounter(); clk_r0 = __builtin_amdgcn_s_memrealtime(); }
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* As = smem;                          // [NBUF][BM][LDT]
  float* Bs = smem + NBUF * BM * LDT;        // [NBUF][BN][LDT]
  int* row_off = (int*)(Bs + NBUF * BN * LDT);  // [BM] output element offset of each tile row (-1: none)

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / (BN / WN);
  const int wn = wave % (BN / WN);

  const int lb = xcd_remap(blockIdx.x, gridDim.x) + p.tile_begin;
  const int nblk = lb % p.n_nblocks;
  const int mblk = lb / p.n_nblocks;
  const int m0 = mblk * BM;
  const int n0 = nblk * BN;

  // ---- per-thread A row pointers (one output pixel per row) -------------------------------
  const int a_c4 = tid & 7;   // which float4 of the 32-float chunk
  const int a_r0 = tid >> 3;  // 0..31
  const float* a_ptr[A_LD4];
#pragma unroll
  for (int i = 0; i < A_LD4; ++i) {
    int m = m0 + a_r0 + 32 * i;
    m = m < p.M ? m : p.M - 1;
    const int wo = m % p.Wo;
    const int t = m / p.Wo;
    const int ho = t % p.Ho;
    const int n = t / p.Ho;
    const size_t pix = ((size_t)n * p.Hp + (size_t)(ho * p.stride + p.in_off)) * p.Wp + (size_t)(wo * p.stride + p.in_off);
    a_ptr[i] = p.x + pix * p.C;
  }
  // output offsets of this tile's rows
  for (int r = tid; r < BM; r += 256) {
    const int m = m0 + r;
    int off = -1;
    if (m < p.M) {
      const int wo = m % p.Wo;
      const int t = m / p.Wo;
      const int ho = t % p.Ho;
      const int n = t / p.Ho;
      off = (((n * p.Hop) + ho + p.out_border) * p.Wop + wo + p.out_border) * p.Cout;
    }
    row_off[r] = off;
  }

  const int a_col = a_c4 * 4;  // this thread's float offset in a chunk row
  // b_ptr / bp: this thread's B position as a pointer.  No load reads it (they use b_rsrc + b_su), but the compiler's instruction order
  // in the prologue, and so every instance's machine code, depends on it being there (scripts/isa_digest.py).
  const float* b_ptr = p.w + (size_t)nblk * p.n_chunks * (BN * BK) + (tid >> 3) * BK + a_col;
  constexpr int A_ES = AHALF ? 2 : 4;   // bytes per input element
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
  typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
  int a_voff[A_LD4];
  int b_voff;
  __amdgpu_buffer_rsrc_t a_rsrc, b_rsrc;
  {
    const int mb = m0 < p.M ? m0 : p.M - 1;
    const int wo = mb % p.Wo;
    const int t = mb / p.Wo;
    const int ho = t % p.Ho;
    const int n = t / p.Ho;
    const size_t pix = ((size_t)n * p.Hp + (size_t)(ho * p.stride + p.in_off)) * p.Wp + (size_t)(wo * p.stride + p.in_off);
    const float* a_base = p.x + pix * p.C;   // (AHALF: p.x really points at halves; a_ptr / a_base only serve as element counters)
    if constexpr (AHALF)
      a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(reinterpret_cast<const _Float16*>(p.x) + pix * p.C), 0, -1, 0x00020000);
    else
      a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)a_base, 0, -1, 0x00020000);
    b_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.w + (size_t)nblk * p.n_chunks * (BN * BK)), 0, -1, 0x00020000);
#pragma unroll
    for (int i = 0; i < A_LD4; ++i) a_voff[i] = (int)((a_ptr[i] - a_base) * A_ES);
    b_voff = ((tid >> 3) * BK + a_col) * 4;
  }
  const int row_stride = p.Wp * p.C;  // floats between successive kh rows

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // Straight-line software pipeline (no lambdas / no conditional loads: hipcc otherwise parks the prefetch registers in
  // scratch and waits for the loads right away).  The loads of chunk c+1 are issued before the MFMAs of chunk c and written
  // to the other LDS buffer under them; the last iteration harmlessly re-loads the last chunk.
// (explicit scalars, not arrays: the arrays only become registers after loop unrolling, and the sched_barrier intrinsic
//  that pins the prefetch is a memory barrier to the optimiser, which would leave them in scratch)
#define MP_BUF4(R, V, S) ([&] { const u32x4 v_ = __builtin_amdgcn_raw_buffer_load_b128(R, V, S, 0);              \
    return make_float4(__uint_as_float(v_.x), __uint_as_float(v_.y), __uint_as_float(v_.z), __uint_as_float(v_.w)); }())
#define MP_CONV_LOAD()                                                                                             \
  {                                                                                                                \
    /* RAGGED: the run position is per lane (vector offset); otherwise only a_col is, the rest rides in the scalar offset */ \
    const int av_ = RAGGED ? aoff * A_ES : a_col * A_ES;                                                           \
    const int as_ = RAGGED ? 0 : a_su * A_ES;   /* a_su / b_su: the wave-uniform chunk positions (A: non-RAGGED only) */ \
    const int bs_ = b_su * 4;                                                                                      \
    if constexpr (AHALF) {   /* 4 halves per lane and tile row: widened when they are written to LDS */            \
      ah0 = __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, a_voff[0] + av_, as_, 0);                                 \
      ah1 = __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, a_voff[1] + av_, as_, 0);                                 \
      ah2 = __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, a_voff[2] + av_, as_, 0);                                 \
      ah3 = __builtin_amdgcn_raw_buffer_load_b64(a_rsrc, a_voff[3] + av_, as_, 0);                                 \
    } else {                                                                                                       \
      a0 = MP_BUF4(a_rsrc, a_voff[0] + av_, as_);                                                                  \
      a1 = MP_BUF4(a_rsrc, a_voff[1] + av_, as_);                                                                  \
      a2 = MP_BUF4(a_rsrc, a_voff[2] + av_, as_);                                                                  \
      a3 = MP_BUF4(a_rsrc, a_voff[3] + av_, as_);                                                                  \
    }                                                                                                              \
    b0 = MP_BUF4(b_rsrc, b_voff, bs_);                                                                             \
    b1 = MP_BUF4(b_rsrc, b_voff, bs_ + 4096);                                                                      \
    if constexpr (B_LD4 > 2) {                                                                                     \
      b2 = MP_BUF4(b_rsrc, b_voff, bs_ + 8192);                                                                    \
      b3 = MP_BUF4(b_rsrc, b_voff, bs_ + 12288);                                                                   \
    }                                                                                                              \
  }
#define MP_ST4(P, V) (*reinterpret_cast<float4*>(P) = (V))
#define MP_H4(V) ([&] { const f16x4 h_ = __builtin_bit_cast(f16x4, V);                                             \
    return make_float4((float)h_.x, (float)h_.y, (float)h_.z, (float)h_.w); }())
#define MP_CONV_STORE(BUF)                                                        \
  {                                                                               \
    float* as_w = As + (BUF) * BM * LDT + a_r0 * LDT + a_c4 * 4;            \
    float* bs_w = Bs + (BUF) * BN * LDT + (tid >> 3) * LDT + (tid & 7) * 4; \
    if constexpr (AHALF) {                                                        \
      a0 = MP_H4(ah0);                                                            \
      a1 = MP_H4(ah1);                                                            \
      a2 = MP_H4(ah2);                                                            \
      a3 = MP_H4(ah3);                                                            \
    }                                                                             \
    MP_ST4(as_w, a0);                                                             \
    MP_ST4(as_w + 32 * LDT, a1);                                               \
    MP_ST4(as_w + 64 * LDT, a2);                                               \
    MP_ST4(as_w + 96 * LDT, a3);                                               \
    MP_ST4(bs_w, b0);                                                             \
    MP_ST4(bs_w + 32 * LDT, b1);                                               \
    if constexpr (B_LD4 > 2) {                                                    \
      MP_ST4(bs_w + 64 * LDT, b2);                                             \
      MP_ST4(bs_w + 96 * LDT, b3);                                             \
    }                                                                             \
  }
  float4 a0, a1, a2, a3, b0, b1, b2, b3;
  u32x2 ah0, ah1, ah2, ah3;   // AHALF: the packed halves of the prefetched A pieces

  // per-thread position of its float4 inside the concatenated K axis: j = offset in the current kernel row's run,
  // aoff = element offset from the pixel's first tap (run % 4 == 0, so a float4 never straddles two rows)
  // RAGGED (run % 32 != 0, the 7x7 / 5x5 stems): per-lane bookkeeping.  Otherwise chunks never straddle kernel rows and
  // the bump is wave-uniform (scalar registers), which is what the 3x3 / 1x1 layers use.
  int j = a_col, aoff = a_col;
  int ju = 0;  // uniform run position (non-RAGGED)
  int a_su = 0, b_su = 0;  // uniform float offsets of the current chunk (A: non-RAGGED only)
  [[maybe_unused]] const float* bp = b_ptr;
  int c_begin = 0, c_end = p.n_chunks;
  if constexpr (SPLITK) {
    c_begin = blockIdx.y * p.chunks_per_split;
    c_end = min(p.n_chunks, c_begin + p.chunks_per_split);
    b_su = c_begin * (BN * BK);
    if constexpr (RAGGED) {
      const int jj = a_col + c_begin * BK;
      const int kh = jj / p.run;
      j = jj - kh * p.run;
      aoff = kh * row_stride + j;
    } else {
      const int kh = (c_begin * BK) / p.run;
      ju = c_begin * BK - kh * p.run;
      a_su = kh * row_stride + ju;
    }
  } else if constexpr (RAGGED) {
    while (j >= p.run) { j -= p.run; aoff += row_stride - p.run; }
  }
  MP_CONV_LOAD()
  MP_CONV_STORE(0)
  __syncthreads();

  const int frag_row = lane & 31;
  const int frag_k = (lane >> 5) * 4;
  const int row_wrap = row_stride - p.run;
#ifdef MP_RASTER_PROF
  unsigned long long cprof_acc[5] = {0, 0, 0, 0, 0};
  unsigned long long cprof_t = __builtin_readcyclecounter();
#endif
  // The LDS store of the next chunk sits under the 3rd of the 4 MFMA groups in the single pass, under the last one in a split-K pass.
  constexpr int STORE_KK = SPLITK ? BK / 8 - 1 : 2;
  for (int chunk = c_begin; chunk < c_end; ++chunk) {
    const int buf = (chunk - c_begin) & 1;
    if (chunk + 1 < c_end) {   // advance the load position to the next chunk (the last one is loaded again)
      bp += BN * BK;
      b_su += BN * BK;
      if constexpr (RAGGED) {
        aoff += BK;
        j += BK;
        while (j >= p.run) {   // crossed into the next kernel row(s) (runs shorter than BK wrap more than once)
          j -= p.run;
          aoff += row_wrap;
        }
      } else {
        a_su += BK;
        ju += BK;
        if (ju == p.run) {
          ju = 0;
          a_su += row_wrap;
        }
      }
    }
    MP_CONV_LOAD()
    __builtin_amdgcn_sched_barrier(0);  // keep the prefetch ahead of the MFMA block (the scheduler otherwise sinks it to the end)
    CPROF(0)
    const float* as = As + buf * BM * LDT + (wm * WM + frag_row) * LDT + frag_k;
    const float* bs = Bs + buf * BN * LDT + (wn * WN + frag_row) * LDT + frag_k;
#pragma unroll
    for (int kk = 0; kk < BK / 8; ++kk) {
      float4 af[TM], bf[TN];
#pragma unroll
      for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const float4*>(as + i * 32 * LDT + kk * 8);
#pragma unroll
      for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const float4*>(bs + j * 32 * LDT + kk * 8);
      if (kk == STORE_KK) {  // write the prefetched chunk to the other buffer UNDER an MFMA group
        __builtin_amdgcn_sched_barrier(0);
        CPROF(1)
        MP_CONV_STORE(buf ^ 1)
        __builtin_amdgcn_sched_barrier(0);
        CPROF(2)
      }
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].x, bf[j].x, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].y, bf[j].y, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].z, bf[j].z, acc[i][j], 0, 0, 0);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i].w, bf[j].w, acc[i][j], 0, 0, 0);
        }
    }
    CPROF(3)
    __syncthreads();
    CPROF(4)
  }
#ifdef MP_RASTER_PROF
  if (lane == 0 && (blockIdx.x & 15) == 0)
    for (int k = 0; k < 5; ++k) atomicAdd(&g_conv_seg[k], cprof_acc[k]);
#endif
#undef MP_CONV_LOAD
#undef MP_BUF4
#undef MP_CONV_STORE
#undef MP_H4
#undef MP_ST4

  if (clk_sample) {   // prologue + K loop of this workgroup
    atomicAdd(&g_conv_clk[0], __builtin_readcyclecounter() - clk_c0);
    atomicAdd(&g_conv_clk[1], __builtin_amdgcn_s_memrealtime() - clk_r0);
  }
  // ---- epilogue: C/D layout of 32x32 MFMA: col = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) ----
  // (compile-time flags: one straight-line store loop per fused mode instead of four data-dependent branches per element)
  const int erow0 = wm * WM + (lane >> 5) * 4, en0 = n0 + wn * WN + (lane & 31);
  if constexpr (SPLITK) {
    float* part = p.partial + (size_t)blockIdx.y * (p.M - p.m_part_begin) * p.Cout;
#pragma unroll
    for (int jn = 0; jn < TN; ++jn) {
      const int n = en0 + jn * 32;
      if (n >= p.Cout) continue;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int m = m0 + erow0 + i * 32 + (r & 3) + 8 * (r >> 2);
          if (m < p.M) part[(size_t)(m - p.m_part_begin) * p.Cout + n] = acc[i][jn][r];
        }
    }
    return;
  }
  const int emode = (p.residual ? 1 : 0) | (p.relu ? 2 : 0) | (p.y_act ? 4 : 0);
  switch (emode) {
    case 0: conv_epilogue<TM, TN, false, false, false>(p, acc, row_off, erow0, en0); break;
    case 1: conv_epilogue<TM, TN, true, false, false>(p, acc, row_off, erow0, en0); break;
    case 2: conv_epilogue<TM, TN, false, true, false>(p, acc, row_off, erow0, en0); break;
    case 3: conv_epilogue<TM, TN, true, true, false>(p, acc, row_off, erow0, en0); break;
    case 4: conv_epilogue<TM, TN, false, false, true>(p, acc, row_off, erow0, en0); break;
    case 5: conv_epilogue<TM, TN, true, false, true>(p, acc, row_off, erow0, en0); break;
    case 6: conv_epilogue<TM, TN, false, true, true>(p, acc, row_off, erow0, en0); break;
    default: conv_epilogue<TM, TN, true, true, true>(p, acc, row_off, erow0, en0); break;
  }
}

// sum of the k_split partial tiles in ascending split order + the fused epilogue (bias, residual, ReLU, pre-activation output)
__global__ __launch_bounds__(256) void conv_splitk_reduce(ConvParams p) {
  const int c4 = p.Cout >> 2;
  const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int m_part = p.M - p.m_part_begin;
  if (idx >= (long)m_part * c4) return;
  const int mi = (int)(idx / c4), n = (int)(idx % c4) * 4;
  const int m = p.m_part_begin + mi;
  float4 v = *reinterpret_cast<const float4*>(p.partial + (size_t)mi * p.Cout + n);
  for (int z = 1; z < p.k_split; ++z) {
    const float4 q = *reinterpret_cast<const float4*>(p.partial + ((size_t)z * m_part + mi) * p.Cout + n);
    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
  }
  const int wo = m % p.Wo;
  const int t = m / p.Wo;
  const int ho = t % p.Ho;
  const int nn = t / p.Ho;
  const size_t off = ((((size_t)nn * p.Hop) + ho + p.out_border) * p.Wop + wo + p.out_border) * p.Cout + n;
  if (p.bias) {
    const float4 b = *reinterpret_cast<const float4*>(p.bias + n);
    v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
  }
  if (p.residual) {
    const float4 r = *reinterpret_cast<const float4*>(p.residual + off);
    v.x += r.x; v.y += r.y; v.z += r.z; v.w += r.w;
  }
  if (p.relu) { v.x = fmaxf(v.x, 0.f); v.y = fmaxf(v.y, 0.f); v.z = fmaxf(v.z, 0.f); v.w = fmaxf(v.w, 0.f); }
  if (p.y) *reinterpret_cast<float4*>(p.y + off) = v;
  if (p.y_act) {
    const float4 sc = *reinterpret_cast<const float4*>(p.act_scale + n), sh = *reinterpret_cast<const float4*>(p.act_shift + n);
    float4 a;
    a.x = fmaxf(fmaf(v.x, sc.x, sh.x), 0.f); a.y = fmaxf(fmaf(v.y, sc.y, sh.y), 0.f);
    a.z = fmaxf(fmaf(v.z, sc.z, sh.z), 0.f); a.w = fmaxf(fmaf(v.w, sc.w, sh.w), 0.f);
    *reinterpret_cast<float4*>(p.y_act + off) = a;
  }
}

static size_t conv_lds_bytes(int BN) { return (size_t)(2 * CONV_BM * LDS_LD + 2 * BN * LDS_LD) * sizeof(float) + CONV_BM * sizeof(int); }

template <int BN, bool RAGGED = false>
static int launch_splitk(const ConvParams& p, hipStream_t s, double alg_k) {
  ConvParams q = p;
  q.n_mblocks = ceil_div(p.M, CONV_BM);
  q.n_nblocks = ceil_div(p.Cout, BN);
  const size_t lds = conv_lds_bytes(BN);
  static bool attr_set = false;
  if (!attr_set) {
    MP_CHECK_HIP(hipFuncSetAttribute((const void*)conv_nhwc_f32_mfma<BN, RAGGED, true, false>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  const double m_part = (double)(p.M - p.m_part_begin);
  {
    ProfScope prof(BN == 64 ? "conv_nhwc_f32_mfma<128,64,64,32>/splitk" : "conv_nhwc_f32_mfma<128,128,64,64>/splitk",
                   2.0 * m_part * p.Cout * alg_k,
                   4.0 * (m_part * p.stride * p.stride * p.C + (double)p.n_chunks * BK * p.Cout + m_part * p.Cout), s);
    hipLaunchKernelGGL((conv_nhwc_f32_mfma<BN, RAGGED, true, false>),
                       dim3(q.n_mblocks * q.n_nblocks - q.tile_begin, q.k_split), dim3(256), lds, s, q);
  }
  ProfScope prof("conv_splitk_reduce", 0.0, 4.0 * m_part * p.Cout * (q.k_split + 1), s);
  hipLaunchKernelGGL(conv_splitk_reduce, dim3(ceil_div((long)m_part * (p.Cout / 4), 256L)), dim3(256), 0, s, q);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

template <int BN, bool RAGGED = false, bool AHALF = false>
static int launch(const ConvParams& p, hipStream_t s, double alg_k, int n_tiles_main = 0) {
  ConvParams q = p;
  q.n_mblocks = ceil_div(p.M, CONV_BM);
  q.n_nblocks = ceil_div(p.Cout, BN);
  const size_t lds = conv_lds_bytes(BN);
  static bool attr_set = false;
  if (!attr_set) {
    MP_CHECK_HIP(hipFuncSetAttribute((const void*)conv_nhwc_f32_mfma<BN, RAGGED, false, AHALF>,
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    attr_set = true;
  }
  // n_tiles_main > 0: only the first n_tiles_main tiles (whole rounds of resident workgroups); a split-K launch covers the rest
  const int n_tiles = n_tiles_main > 0 ? n_tiles_main : q.n_mblocks * q.n_nblocks;
  const double m_here = n_tiles_main > 0 ? (double)(n_tiles_main / q.n_nblocks) * CONV_BM : (double)p.M;
  // algorithmic work of this launch: 2*MACs over the REAL (unpadded) reduction length; bytes = input + weights + output once
  static const bool detail = getenv("MP_PROF_DETAIL") != nullptr;  // tuning aid: one profiler row per layer shape
  const char* pname = BN == 64 ? "conv_nhwc_f32_mfma<128,64,64,32>" : "conv_nhwc_f32_mfma<128,128,64,64>";
  if (AHALF) pname = "conv_nhwc_f32_mfma<128,64,64,32>/x_f16";   // own profiler row: never mixed into the fp32 kernels' roofline figures
  if (detail) {
    static std::vector<std::string> names;  // stable storage for the profiler's name pointers
    char buf[96];
    snprintf(buf, sizeof(buf), "%s/k%d_c%d_s%d_n%d", pname, p.KH, p.C, p.stride, p.Cout);
    bool found = false;
    for (auto& n : names) if (n == buf) { pname = n.c_str(); found = true; break; }
    if (!found) { names.reserve(64); names.emplace_back(buf); pname = names.back().c_str(); }
  }
  ProfScope prof(pname, 2.0 * m_here * p.Cout * alg_k,
                 (AHALF ? 2.0 : 4.0) * m_here * p.stride * p.stride * p.C + 4.0 * ((double)p.n_chunks * BK * p.Cout + m_here * p.Cout), s);
  hipLaunchKernelGGL((conv_nhwc_f32_mfma<BN, RAGGED, false, AHALF>), dim3(n_tiles), dim3(256), lds, s, q);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

// The packed weight blob is tiled for a fixed BN per layer: BN = 64 when Cout == 64, else 128.
static inline int conv_bn_tile(int Cout) { return Cout <= 64 ? 64 : 128; }

}  // namespace mp

using namespace mp;

extern "C" int mp_conv_clock_read(double* shader_mhz, int reset) {
  MP_REQUIRE(shader_mhz != nullptr, "mp_conv_clock_read: null output");
  unsigned long long h[2] = {0, 0};
  MP_CHECK_HIP(hipDeviceSynchronize());
  MP_CHECK_HIP(hipMemcpyFromSymbol(h, HIP_SYMBOL(g_conv_clk), sizeof(h)));
  *shader_mhz = h[1] ? 100.0 * (double)h[0] / (double)h[1] : 0.0;
  if (reset) {
    const unsigned long long z[2] = {0, 0};
    MP_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_conv_clk), z, sizeof(z)));
  }
  return MP_OK;
}

#ifdef MP_RASTER_PROF
extern "C" int mp_conv_prof_read(unsigned long long* out2, int reset) {
  MP_CHECK_HIP(hipDeviceSynchronize());
  MP_CHECK_HIP(hipMemcpyFromSymbol(out2, HIP_SYMBOL(g_conv_clk), 2 * sizeof(unsigned long long)));
  MP_CHECK_HIP(hipMemcpyFromSymbol(out2 + 2, HIP_SYMBOL(g_conv_seg), 8 * sizeof(unsigned long long)));   // out2 holds 10 words
  if (reset) {
    unsigned long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    MP_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_conv_clk), z, 2 * sizeof(unsigned long long)));
    MP_CHECK_HIP(hipMemcpyToSymbol(HIP_SYMBOL(g_conv_seg), z, sizeof(z)));
  }
  return MP_OK;
}
#endif

extern "C" size_t mp_conv_packed_floats(int Cin_p, int Cout, int KH, int KW) {
  const int BN = conv_bn_tile(Cout);
  const int nblk = ceil_div(Cout, BN);
  const int n_chunks = ceil_div((long)KH * KW * Cin_p, BK);
  return (size_t)nblk * n_chunks * BN * BK;
}

// packed[nb][chunk][n_local][k], K index = kh*(KW*Cin_p) + kw*Cin_p + c over the concatenated row runs (zero padded)
extern "C" int mp_conv_pack_weights(const float* w, int Cout, int Cin, int KH, int KW, int Cin_p,
                                    const float* scale, float* packed) {
  MP_REQUIRE(w && packed && Cin_p >= Cin && (Cin_p % 4) == 0, "mp_conv_pack_weights: bad arguments");
  const int BN = conv_bn_tile(Cout);
  const int nblk = ceil_div(Cout, BN);
  const int run = KW * Cin_p;
  const int k_total = KH * run;
  const int n_chunks = ceil_div(k_total, BK);
  const size_t total = mp_conv_packed_floats(Cin_p, Cout, KH, KW);
  memset(packed, 0, total * sizeof(float));
  for (int nb = 0; nb < nblk; ++nb)
    for (int ch = 0; ch < n_chunks; ++ch) {
      float* tile = packed + ((size_t)nb * n_chunks + ch) * BN * BK;
      for (int nl = 0; nl < BN; ++nl) {
        const int n = nb * BN + nl;
        if (n >= Cout) continue;
        const float s = scale ? scale[n] : 1.f;
        for (int k = 0; k < BK; ++k) {
          const int kidx = ch * BK + k;
          if (kidx >= k_total) continue;
          const int kh = kidx / run, jj = kidx % run;
          const int kw = jj / Cin_p, c = jj % Cin_p;
          if (c >= Cin) continue;
          tile[nl * BK + k] = w[(((size_t)n * Cin + c) * KH + kh) * KW + kw] * s;
        }
      }
    }
  return MP_OK;
}

// How a conv launch is laid out on the chip (host-side decision, exposed through mp_conv2d_plan for the CPU tests):
//   mode 0: one single-pass launch;
//   mode 1: small grid (< 192 tiles: the released K = 1 / K = 5 refiner passes) -- every tile's K loop is split over k_split
//           workgroups and reduced deterministically;
//   mode 2: full rounds + split-K tail -- with `resident` workgroups (2 per CU) a grid of n_tiles runs ceil(n_tiles / resident)
//           rounds; when the last round is less than half full, its tiles are split along K over the idle slots instead
//           (layer 3 at 576 rows: 2700 tiles = 5.27 rounds -> 5 rounds + a third of a round).
struct ConvPlan {
  int mode, k_split, chunks_per_split, n_main, m_begin;
};

static ConvPlan plan_conv(const ConvParams& p, bool small, long ws_floats, int resident, bool splitk_on, bool tail_on) {
  ConvPlan pl = {0, 1, p.n_chunks, 0, 0};
  const int n_nb = ceil_div(p.Cout, small ? 64 : 128);
  const int n_tiles = ceil_div(p.M, 128) * n_nb;
  if (!splitk_on || ws_floats <= 0 || (p.Cout % 4) != 0) return pl;
  if (n_tiles < 192 && p.n_chunks >= 8) {
    long S = std::min<long>(ceil_div(512, n_tiles), p.n_chunks / 4);
    S = std::min<long>(S, ws_floats / ((long)p.M * p.Cout));
    if (S >= 2) {
      pl.mode = 1;
      pl.chunks_per_split = ceil_div(p.n_chunks, (int)S);
      pl.k_split = ceil_div(p.n_chunks, pl.chunks_per_split);
      return pl;
    }
  }
  const int n_tail = n_tiles % resident;
  if (tail_on && n_tiles > resident && n_tail > 0 && 2 * n_tail <= resident && p.run % BK == 0 && resident % n_nb == 0) {
    const int n_main = n_tiles - n_tail;
    const int m_begin = (n_main / n_nb) * 128;
    long S = std::min<long>(resident / n_tail, p.n_chunks / 6);
    S = std::min<long>(S, ws_floats / ((long)(p.M - m_begin) * p.Cout));
    if (S >= 2) {
      pl.mode = 2;
      pl.chunks_per_split = ceil_div(p.n_chunks, (int)S);
      pl.k_split = ceil_div(p.n_chunks, pl.chunks_per_split);
      pl.n_main = n_main;
      pl.m_begin = m_begin;
    }
  }
  return pl;
}

static int make_params(const mp_conv_desc* d, ConvParams* p) {
  MP_REQUIRE(d && d->d_x && d->d_w && (d->d_y || d->d_y_act), "mp_conv2d_nhwc: null pointer");
  MP_REQUIRE(d->C % 4 == 0, "mp_conv2d_nhwc: C (%d) must be a multiple of 4", d->C);
  MP_REQUIRE(d->in_border >= d->pad, "mp_conv2d_nhwc: in_border %d < pad %d", d->in_border, d->pad);
  MP_REQUIRE(d->stride >= 1 && d->KH >= 1 && d->KW >= 1 && d->Cout >= 1, "mp_conv2d_nhwc: bad geometry");
  MP_REQUIRE(!d->d_y_act || (d->d_act_scale && d->d_act_shift), "mp_conv2d_nhwc: y_act needs scale/shift");
  const int Ho = (d->H + 2 * d->pad - d->KH) / d->stride + 1;
  const int Wo = (d->W + 2 * d->pad - d->KW) / d->stride + 1;
  const long M = (long)d->N * Ho * Wo;
  MP_REQUIRE(M > 0 && M < (1L << 31), "mp_conv2d_nhwc: M out of range");
  const long out_elems = (long)d->N * (Ho + 2 * d->out_border) * (Wo + 2 * d->out_border) * d->Cout;
  MP_REQUIRE(out_elems < (1L << 31), "mp_conv2d_nhwc: output too large for 32-bit offsets (%ld)", out_elems);
  p->x = d->d_x;
  p->w = d->d_w;
  p->bias = d->d_bias;
  p->residual = d->d_residual;
  p->act_scale = d->d_act_scale;
  p->act_shift = d->d_act_shift;
  p->y = d->d_y;
  p->y_act = d->d_y_act;
  p->M = (int)M;
  p->Ho = Ho;
  p->Wo = Wo;
  p->Hp = d->H + 2 * d->in_border;
  p->Wp = d->W + 2 * d->in_border;
  p->C = d->C;
  p->in_off = d->in_border - d->pad;
  p->stride = d->stride;
  p->Cout = d->Cout;
  p->Hop = Ho + 2 * d->out_border;
  p->Wop = Wo + 2 * d->out_border;
  p->out_border = d->out_border;
  p->KH = d->KH;
  p->run = d->KW * d->C;
  p->n_chunks = ceil_div((long)d->KH * p->run, BK);
  p->relu = d->relu;
  p->partial = nullptr;
  p->k_split = 1;
  p->chunks_per_split = p->n_chunks;
  p->tile_begin = 0;
  p->m_part_begin = 0;
  return MP_OK;
}

int mp::conv_make_params(const mp_conv_desc* d, ConvParams* p) { return make_params(d, p); }

extern "C" int mp_conv2d_nhwc(const mp_conv_desc* d, mp_stream stream) {
  ConvParams p;
  int rc = make_params(d, &p);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  const double alg_k = (double)d->KH * d->KW * (d->c_real > 0 ? d->c_real : d->C);
  const bool small = conv_bn_tile(d->Cout) == 64;
  if (d->x_f16) {   // half-precision input (the stems of the "fp16 renders" mode): single-pass launches of the 128x64 tile only
    MP_REQUIRE(small, "mp_conv2d_nhwc: x_f16 is implemented for Cout <= 64 (the stem convolutions), got Cout = %d", d->Cout);
    return p.run % BK != 0 ? launch<64, true, true>(p, s, alg_k) : launch<64, false, true>(p, s, alg_k);
  }
  static const int splitk_on = getenv("MP_CONV_SPLITK") ? atoi(getenv("MP_CONV_SPLITK")) : 1;
  static const int tail_on = getenv("MP_CONV_TAIL") ? atoi(getenv("MP_CONV_TAIL")) : 1;
  const ConvPlan plan = plan_conv(p, small, d->d_splitk_ws ? d->splitk_ws_floats : 0, 2 * device_cu_count(), splitk_on != 0, tail_on != 0);
  if (plan.mode == 1) {  // small grid: every tile split along K
    p.chunks_per_split = plan.chunks_per_split;
    p.k_split = plan.k_split;
    p.partial = d->d_splitk_ws;
    if (p.run % BK != 0) return small ? launch_splitk<64, true>(p, s, alg_k) : launch_splitk<128, true>(p, s, alg_k);
    return small ? launch_splitk<64>(p, s, alg_k) : launch_splitk<128>(p, s, alg_k);
  }
  // One schedule per pass (conv_nhwc_f32_mfma); its measured alternatives are recorded in profiles/r03_conv_ab_epilogue_persistent.txt
  // and docs/history.md section 3.1.
  if (plan.mode == 2) {  // whole rounds single-pass, the tiles of the half-empty last round split along K
    const int rc2 = small ? launch<64>(p, s, alg_k, plan.n_main) : launch<128>(p, s, alg_k, plan.n_main);
    if (rc2) return rc2;
    p.chunks_per_split = plan.chunks_per_split;
    p.k_split = plan.k_split;
    p.partial = d->d_splitk_ws;
    p.tile_begin = plan.n_main;
    p.m_part_begin = plan.m_begin;
    return small ? launch_splitk<64>(p, s, alg_k) : launch_splitk<128>(p, s, alg_k);
  }
  if (p.run % BK != 0)  // ragged K (stems): per-lane K bookkeeping
    return small ? launch<64, true>(p, s, alg_k) : launch<128, true>(p, s, alg_k);
  return small ? launch<64>(p, s, alg_k) : launch<128>(p, s, alg_k);
}

extern "C" int mp_conv2d_plan(const mp_conv_desc* d, int n_cu, int32_t* out5) {
  MP_REQUIRE(out5 && n_cu > 0, "mp_conv2d_plan: bad arguments");
  ConvParams p;
  int rc = make_params(d, &p);
  if (rc) return rc;
  ConvPlan pl = plan_conv(p, conv_bn_tile(d->Cout) == 64, d->d_splitk_ws ? d->splitk_ws_floats : 0, 2 * n_cu, true, true);
  if (d->x_f16) pl = ConvPlan{0, 1, p.n_chunks, 0, 0};   // half-precision inputs always run as one single-pass launch
  out5[0] = pl.mode; out5[1] = pl.k_split; out5[2] = pl.chunks_per_split; out5[3] = pl.n_main; out5[4] = pl.m_begin;
  return MP_OK;
}

extern "C" const char* mp_conv2d_kernel_name(const mp_conv_desc* d) {
  return conv_bn_tile(d->Cout) == 64 ? "conv_nhwc_f32_mfma<128,64,64,32>" : "conv_nhwc_f32_mfma<128,128,64,64>";
}
