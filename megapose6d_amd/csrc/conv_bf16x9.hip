// conv_bf16x9.hip -- direct (implicit-GEMM) convolution on the bf16 MFMA through EXACT operand pieces (v_mfma_f32_32x32x16_bf16), gfx950.
//
// Same formulation and launch parameters as conv.hip (row-run implicit GEMM over padded NHWC: M = N*Ho*Wo, N = Cout, K = KH * (KW*C),
// zero border instead of bounds checks, the same fused epilogue: bias, residual, ReLU, the pre-activated second output, border untouched);
// reference layers: src/megapose/models/torchvision_resnet.py:74-120 (BasicBlock conv1 at stride 2 + downsample), wide_resnet.py:29-56.
// What changes is the multiplication (the scheme of conv_wino_bf16.hip, applied to the direct convolution):
//   * weights (eval-BN scale folded in fp32, exactly the values mp_conv_pack_weights packs) are split on the host into three bf16 pieces
//     W = W1 + W2 + W3 EXACTLY (bf16x9_split.h) and packed in MFMA fragment order (mp_conv_bf16x9_pack_weights);
//   * activations are staged as fp32 through LDS (double-buffered, as conv.hip), read back as the 8-element fragments of the bf16 MFMA
//     and split the same way in registers (bf16x9_split8: 4 VALU per element + the packing);
//   * all nine piece products are evaluated, each exact in the fp32 accumulator: the result differs from the fp32-MFMA kernel only in the
//     ORDER of fp32 additions (no product rounded, none dropped).
// Tile: 128 x 128 per workgroup, four waves of 64 x 64 (2 x 2 accumulators of 32 x 32).  Per 16-deep K slice a wave issues 36 MFMAs of 32
// cycles = 1152 cycles, against 32 v_mfma_f32_32x32x2_f32 of 64 cycles = 2048 for the same work on the fp32 pipe (0.56).
// K loop: one 32-float chunk per iteration (two K slices, one barrier): the A chunk c+1 is requested at the top and written to the other
// LDS buffer at the bottom; the weight fragments come straight from L2 into registers one slice ahead (6 x 1 KB per wave and slice).
// Roofline: bf16 MFMA (2.5 PFLOP/s dense); algorithmic work = 2 * MACs of the convolution; executed = 9 x that (padded K) in bf16 FLOPs.
#include <cstdlib>

#include "bf16x9_split.h"
#include "conv_common.h"

namespace mp {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef bf16x9_u32x4 db_u32x4;

constexpr int DB_BM = 128, DB_BN = 128;
constexpr int DB_SLICE_BYTES = (DB_BN / 32) * 3 * 1024;   // one 16-deep K slice of one n block: [32-column block j][piece][lane][8 bf16]
// the nine (activation piece, weight piece) pairs, small terms first
__device__ constexpr int DB_PA[9] = {2, 1, 2, 0, 1, 2, 0, 1, 0}, DB_PB[9] = {2, 2, 1, 2, 1, 0, 1, 0, 0};

// waves_per_eu(2, 2): two workgroups per CU (one wave of each per SIMD) -- while one wave splits fragments or waits at the barrier, the
// other keeps the SIMD's matrix pipe busy; the register budget is 256 per wave.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) void conv_nhwc_bf16x9(ConvParams p) {
  __shared__ __attribute__((aligned(16))) float As[2 * DB_BM * LDS_LD];   // [buffer][tile row][36 floats]: the A chunk, fp32
  __shared__ int row_off[DB_BM];                                          // output element offset of each tile row (-1: none)
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int nblk = lb % p.n_nblocks, mblk = lb / p.n_nblocks;
  const int m0 = mblk * DB_BM, n0 = nblk * DB_BN;

  if (tid < DB_BM) {
    const int m = m0 + tid;
    int off = -1;
    if (m < p.M) {
      const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, n = t / p.Ho;
      off = (((n * p.Hop) + ho + p.out_border) * p.Wop + wo + p.out_border) * p.Cout;
    }
    row_off[tid] = off;
  }
  // A: thread -> float4 (tid & 7) of the 32-float chunk in tile rows (tid >> 3) + 32 i; one buffer resource based at the tile's first
  // pixel (rows ascend with the pixel index), 32-bit lane offsets, the chunk position as a wave-uniform scalar offset
  const int a_c4 = tid & 7, a_r0 = tid >> 3;
  size_t pix[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int m = i < 4 ? m0 + a_r0 + 32 * i : m0;
    m = m < p.M ? m : p.M - 1;
    const int wo = m % p.Wo, t = m / p.Wo, ho = t % p.Ho, n = t / p.Ho;
    pix[i] = ((size_t)n * p.Hp + (size_t)(ho * p.stride + p.in_off)) * p.Wp + (size_t)(wo * p.stride + p.in_off);
  }
  const __amdgpu_buffer_rsrc_t a_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)(p.x + pix[4] * p.C), 0, -1, 0x00020000);
  int a_voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) a_voff[i] = (int)(((pix[i] - pix[4]) * p.C + a_c4 * 4) * 4);
  // B: the pieces of this n block; the wave reads its two 32-column blocks (j = 2 wn, 2 wn + 1), 1 KB per (j, piece) and slice
  const __amdgpu_buffer_rsrc_t b_rsrc = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(reinterpret_cast<const char*>(p.w) + (size_t)nblk * (2 * p.n_chunks) * DB_SLICE_BYTES), 0, -1, 0x00020000);
  const int b_voff = (2 * wn) * 3 * 1024 + lane * 16;

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  float4 a0, a1, a2, a3;
  db_u32x4 bA[2][3], bB[2][3];
#define DB_BUF4(V, S) ([&] { const db_u32x4 v_ = __builtin_amdgcn_raw_buffer_load_b128(a_rsrc, V, S, 0);                  \
    return make_float4(__uint_as_float(v_.x), __uint_as_float(v_.y), __uint_as_float(v_.z), __uint_as_float(v_.w)); }())
#define DB_LOAD_A(SU)                       \
  a0 = DB_BUF4(a_voff[0], (SU) * 4);        \
  a1 = DB_BUF4(a_voff[1], (SU) * 4);        \
  a2 = DB_BUF4(a_voff[2], (SU) * 4);        \
  a3 = DB_BUF4(a_voff[3], (SU) * 4);
#define DB_LOAD_B(DST, SLICE)                                                                                       \
  _Pragma("unroll") for (int jl = 0; jl < 2; ++jl)                                                                  \
    _Pragma("unroll") for (int pc = 0; pc < 3; ++pc)                                                                \
      DST[jl][pc] = __builtin_amdgcn_raw_buffer_load_b128(b_rsrc, b_voff, (SLICE) * DB_SLICE_BYTES + (jl * 3 + pc) * 1024, 0);
#define DB_STORE_A(BUF)                                                            \
  {                                                                                \
    float* as_w = As + (BUF) * DB_BM * LDS_LD + a_r0 * LDS_LD + a_c4 * 4;          \
    *reinterpret_cast<float4*>(as_w) = a0;                                         \
    *reinterpret_cast<float4*>(as_w + 32 * LDS_LD) = a1;                           \
    *reinterpret_cast<float4*>(as_w + 64 * LDS_LD) = a2;                           \
    *reinterpret_cast<float4*>(as_w + 96 * LDS_LD) = a3;                           \
  }
// the 36 MFMAs of one K slice: piece pair outermost, so that four independent accumulators separate two products of one chain
#define DB_MFMA_SLICE(PA_, BB_)                                                                                     \
  _Pragma("unroll") for (int pr = 0; pr < 9; ++pr)                                                                  \
    _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                                   \
      _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                                 \
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, PA_[i][DB_PA[pr]]),          \
                                                            __builtin_bit_cast(bf16x8, BB_[j][DB_PB[pr]]), acc[i][j], 0, 0, 0);

  // K position of the chunk being requested: a_su = its float offset from the pixel's first tap (kh rows apart by Wp*C), ju = its offset
  // inside the current kernel row's run (run % 32 == 0: a chunk never straddles two kernel rows)
  int a_su = 0, ju = 0;
  const int row_wrap = p.Wp * p.C - p.run;
  const int n_ch = p.n_chunks, last_slice = 2 * p.n_chunks - 1;
  DB_LOAD_A(0)
  DB_LOAD_B(bA, 0)
  DB_STORE_A(0)
  __syncthreads();

  // fragment read position: tile row wm*64 + 32 i + (lane & 31), K elements 8 (lane >> 5) .. +7 of the slice (two 16-byte reads)
  const float* fr = As + (wm * 64 + (lane & 31)) * LDS_LD + (lane >> 5) * 8;
  for (int c = 0; c < n_ch; ++c) {
    const int buf = c & 1;
    if (c + 1 < n_ch) {   // (the last iteration harmlessly re-requests the last chunk)
      a_su += BK;
      ju += BK;
      if (ju == p.run) { ju = 0; a_su += row_wrap; }
    }
    DB_LOAD_A(a_su)
    DB_LOAD_B(bB, 2 * c + 1)
    __builtin_amdgcn_sched_barrier(0);   // keep the requests ahead of the MFMA block
    const float* fb = fr + buf * DB_BM * LDS_LD;
    float4 raw[2][2][2];   // [slice][i][elements 0..3 | 4..7]
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      raw[0][i][0] = *reinterpret_cast<const float4*>(fb + i * 32 * LDS_LD);
      raw[0][i][1] = *reinterpret_cast<const float4*>(fb + i * 32 * LDS_LD + 4);
    }
    db_u32x4 pa0[2][3], pa1[2][3];
    bf16x9_split8(raw[0][0][0], raw[0][0][1], pa0[0]);
    bf16x9_split8(raw[0][1][0], raw[0][1][1], pa0[1]);
    __builtin_amdgcn_sched_barrier(0);
    // slice 0, with the fragment reads and the split of slice 1 in its MFMA gaps (left to the scheduler, the 88 VALU of a split form one
    // block in front of the MFMAs): 4 LDS reads, 2 MFMAs, then 22 x (4 VALU, 1 MFMA), the remaining 12 MFMAs
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      raw[1][i][0] = *reinterpret_cast<const float4*>(fb + i * 32 * LDS_LD + 16);
      raw[1][i][1] = *reinterpret_cast<const float4*>(fb + i * 32 * LDS_LD + 16 + 4);
    }
    DB_MFMA_SLICE(pa0, bA)
    bf16x9_split8(raw[1][0][0], raw[1][0][1], pa1[0]);
    bf16x9_split8(raw[1][1][0], raw[1][1][1], pa1[1]);
    __builtin_amdgcn_sched_group_barrier(0x100, 4, 0);   // DS read
    __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);   // MFMA
#pragma unroll
    for (int g = 0; g < 22; ++g) {
      __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);   // VALU
      __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 12, 0);
    __builtin_amdgcn_sched_barrier(0);
    DB_LOAD_B(bA, (2 * c + 2 <= last_slice ? 2 * c + 2 : last_slice))
    // slice 1
    DB_MFMA_SLICE(pa1, bB)
    DB_STORE_A(buf ^ 1)
    __syncthreads();
  }
#undef DB_BUF4
#undef DB_LOAD_A
#undef DB_LOAD_B
#undef DB_STORE_A
#undef DB_MFMA_SLICE

  // epilogue (conv_common.h): C/D layout of the 32x32 MFMAs -- col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
  const int erow0 = wm * 64 + (lane >> 5) * 4, en0 = n0 + wn * 64 + (lane & 31);
  const int emode = (p.residual ? 1 : 0) | (p.relu ? 2 : 0) | (p.y_act ? 4 : 0);
  switch (emode) {
    case 0: conv_epilogue<2, 2, false, false, false>(p, acc, row_off, erow0, en0); break;
    case 1: conv_epilogue<2, 2, true, false, false>(p, acc, row_off, erow0, en0); break;
    case 2: conv_epilogue<2, 2, false, true, false>(p, acc, row_off, erow0, en0); break;
    case 3: conv_epilogue<2, 2, true, true, false>(p, acc, row_off, erow0, en0); break;
    case 4: conv_epilogue<2, 2, false, false, true>(p, acc, row_off, erow0, en0); break;
    case 5: conv_epilogue<2, 2, true, false, true>(p, acc, row_off, erow0, en0); break;
    case 6: conv_epilogue<2, 2, false, true, true>(p, acc, row_off, erow0, en0); break;
    default: conv_epilogue<2, 2, true, true, true>(p, acc, row_off, erow0, en0); break;
  }
}

static int packed_slices(int Cin_p, int KH, int KW) { return 2 * ceil_div((long)KH * KW * Cin_p, BK); }

}  // namespace mp

using namespace mp;

extern "C" size_t mp_conv_bf16x9_packed_bytes(int Cin_p, int Cout, int KH, int KW) {
  return (size_t)ceil_div(Cout, DB_BN) * packed_slices(Cin_p, KH, KW) * DB_SLICE_BYTES;
}

// packed[n block][K slice t][32-column block j][piece][lane][e] = piece of w[n][c][kh][kw] * scale[n] (one fp32 multiplication, as
// mp_conv_pack_weights), n = 128 nb + 32 j + (lane & 31), K index k = 16 t + 8 (lane >> 5) + e = kh*(KW*Cin_p) + kw*Cin_p + c; zero padded
// (c >= Cin, n >= Cout, k past the end of the last 32-float chunk)
extern "C" int mp_conv_bf16x9_pack_weights(const float* w, int Cout, int Cin, int KH, int KW, int Cin_p, const float* scale, void* packed) {
  MP_REQUIRE(w && packed && Cout >= 1 && Cin >= 1 && KH >= 1 && KW >= 1 && Cin_p >= Cin && Cin_p % 16 == 0,
             "mp_conv_bf16x9_pack_weights: bad arguments (Cin_p %% 16 == 0, Cin_p >= Cin)");
  const int run = KW * Cin_p, k_total = KH * run, n_sl = packed_slices(Cin_p, KH, KW);
  unsigned short* out = (unsigned short*)packed;
  memset(out, 0, mp_conv_bf16x9_packed_bytes(Cin_p, Cout, KH, KW));
  for (int n = 0; n < Cout; ++n) {
    const float s = scale ? scale[n] : 1.f;
    const int nb = n / DB_BN, j = (n % DB_BN) / 32, nl = n % 32;
    for (int k = 0; k < k_total; ++k) {
      const int kh = k / run, jj = k % run, kw = jj / Cin_p, c = jj % Cin_p;
      if (c >= Cin) continue;
      unsigned short pc[3];
      bf16x9_split3(w[(((size_t)n * Cin + c) * KH + kh) * KW + kw] * s, pc);
      const int t = k / 16, lane = ((k % 16) / 8) * 32 + nl, e = k % 8;
      for (int piece = 0; piece < 3; ++piece)
        out[(((((size_t)nb * n_sl + t) * 4 + j) * 3 + piece) * 64 + lane) * 8 + e] = pc[piece];
    }
  }
  return MP_OK;
}

// One single-pass launch (no split-K: the caller keeps small grids on mp_conv2d_nhwc); d->d_w is ignored, the pieces come from d_w_pieces.
extern "C" int mp_conv2d_bf16x9_nhwc(const mp_conv_desc* desc, const void* d_w_pieces, mp_stream stream) {
  MP_REQUIRE(desc && d_w_pieces, "mp_conv2d_bf16x9_nhwc: null pointer");
  MP_REQUIRE(!desc->x_f16, "mp_conv2d_bf16x9_nhwc: fp32 input only");
  mp_conv_desc d = *desc;
  d.d_w = (const float*)d_w_pieces;
  ConvParams p;
  const int rc = conv_make_params(&d, &p);
  if (rc) return rc;
  MP_REQUIRE(d.C % 16 == 0 && p.run % BK == 0, "mp_conv2d_bf16x9_nhwc: needs C %% 16 == 0 and KW * C %% 32 == 0 (C = %d, KW = %d)", d.C, d.KW);
  p.n_mblocks = ceil_div(p.M, DB_BM);
  p.n_nblocks = ceil_div(p.Cout, DB_BN);
  const long n_tiles = (long)p.n_mblocks * p.n_nblocks;
  MP_REQUIRE(n_tiles < (1L << 31), "mp_conv2d_bf16x9_nhwc: grid too large");
  hipStream_t s = (hipStream_t)stream;
  const double M = p.M, alg_k = (double)d.KH * d.KW * (d.c_real > 0 ? d.c_real : d.C);
  ProfScope prof("conv_nhwc_bf16x9<128,128,64,64>", 2.0 * M * p.Cout * alg_k,
                 4.0 * (M * p.stride * p.stride * p.C + M * p.Cout) + 6.0 * (double)p.n_chunks * BK * p.n_nblocks * DB_BN, s,
                 9.0 * 2.0 * M * p.Cout * (double)p.n_chunks * BK, 2500.0);
  hipLaunchKernelGGL(conv_nhwc_bf16x9, dim3((unsigned)n_tiles), dim3(256), 0, s, p);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
