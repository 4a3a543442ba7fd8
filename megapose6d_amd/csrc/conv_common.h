// Shared declarations of the implicit-GEMM convolutions on padded NHWC (conv.hip: fp32 MFMA; conv_bf16x9.hip: exact bf16 pieces):
// the launch parameters, the descriptor -> parameter translation and the fused dword epilogue.
#pragma once
#include "common.h"

namespace mp {

constexpr int BK = 32;        // floats of K per chunk
constexpr int LDS_LD = BK + 4;  // padded LDS row (36 floats): conflict-free 16-B fragment reads

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct ConvParams {
  const float* __restrict__ x;
  const float* __restrict__ w;
  const float* __restrict__ bias;
  const float* __restrict__ residual;
  const float* __restrict__ act_scale;
  const float* __restrict__ act_shift;
  float* __restrict__ y;
  float* __restrict__ y_act;
  int M;               // N*Ho*Wo
  int Ho, Wo;
  int Hp, Wp, C;       // padded input geometry
  int in_off;          // in_border - pad
  int stride;
  int Cout;
  int Hop, Wop, out_border;
  int KH;
  int run;             // KW*C floats: contiguous (kw, c) taps of one kernel row
  int n_chunks;        // ceil(KH*run / BK): the K loop walks the concatenated row runs
  int relu;
  int n_mblocks, n_nblocks;
  // split-K (small M: too few tiles to fill 256 CUs): blockIdx.y owns chunks [y*chunks_per_split, ...) and writes raw partial
  // sums to partial[y][M][Cout]; conv_splitk_reduce adds them in a fixed order and applies the epilogue (deterministic)
  float* partial;
  int k_split, chunks_per_split;
  int tile_begin;    // first linear tile id of this launch (the tail launch of a "full rounds + split-K tail" pair starts later)
  int m_part_begin;  // first output row held by `partial` (rows before it belong to the single-pass launch)
};

// mp_conv_desc -> ConvParams (validation, output geometry, K-loop length in BK chunks); defined in conv.hip
int conv_make_params(const mp_conv_desc* d, ConvParams* p);

// Fused epilogue through buffer instructions: one scalar resource per tensor based at the tile's first output row, one 32-bit
// byte offset per (lane, tile row); rows past M and channels past Cout get an offset beyond num_records, which the hardware's range
// check turns into "load 0 / drop the store" -- no per-element branches, no 64-bit lane addresses.
// (Requesting the residual tile before the K loop, to hide its latency, was measured: 2 % slower -- the loads compete with the first
// chunks and 32-64 registers stay live across the loop.)
constexpr unsigned EPI_WINDOW = 0x40000000u;   // 1 GB window from the tile's first row: a tile spans a few image rows

template <int TM>
__device__ __forceinline__ void conv_row_offsets(const int* row_off, int row0, int n_first, int base, unsigned (&voff)[TM][16]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int o = row_off[row0 + i * 32 + (r & 3) + 8 * (r >> 2)];
      voff[i][r] = o >= 0 ? (unsigned)(o - base + n_first) * 4u : EPI_WINDOW;
    }
}

template <int TM, int TN, bool RES, bool RELU, bool ACT>
__device__ __forceinline__ void conv_epilogue(const ConvParams& p, const f32x16 (&acc)[TM][TN], const int* row_off, int row0, int n_first) {
  const int base = __builtin_amdgcn_readfirstlane(row_off[0]);   // row 0 of a launched tile always exists
  unsigned voff[TM][16];
  conv_row_offsets<TM>(row_off, row0, n_first, base, voff);
  float res[TM][TN][16];
  if (RES) {   // every residual value of the wave's tile is requested before the first one is used: one exposed latency per tile
    const __amdgpu_buffer_rsrc_t r_res = __builtin_amdgcn_make_buffer_rsrc((void*)(p.residual + base), 0, (int)EPI_WINDOW, 0x00020000);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const bool n_ok = n_first + j * 32 < p.Cout;
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          res[i][j][r] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r_res, n_ok ? voff[i][r] + j * 128 : EPI_WINDOW, 0, 0));
    }
  }
  const __amdgpu_buffer_rsrc_t r_y = __builtin_amdgcn_make_buffer_rsrc((void*)(p.y ? p.y + base : nullptr), 0, p.y ? (int)EPI_WINDOW : 0, 0x00020000);
  const __amdgpu_buffer_rsrc_t r_act =
      __builtin_amdgcn_make_buffer_rsrc((void*)(ACT ? p.y_act + base : nullptr), 0, ACT ? (int)EPI_WINDOW : 0, 0x00020000);
#pragma unroll
  for (int j = 0; j < TN; ++j) {
    const int n = n_first + j * 32;
    const bool n_ok = n < p.Cout;
    const float bias = (p.bias && n_ok) ? p.bias[n] : 0.f;
    float sc = 1.f, sh = 0.f;
    if (ACT && n_ok) {
      sc = p.act_scale[n];
      sh = p.act_shift[n];
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const unsigned vo = n_ok ? voff[i][r] + j * 128 : EPI_WINDOW;
        float v = acc[i][j][r] + bias;
        if (RES) v += res[i][j][r];
        if (RELU) v = fmaxf(v, 0.f);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r_y, vo, 0, 0);   // (a null y has num_records = 0: dropped)
        if (ACT) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(fmaxf(fmaf(v, sc, sh), 0.f)), r_act, vo, 0, 0);
      }
    }
  }
}

}  // namespace mp
