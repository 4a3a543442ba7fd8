// The exact three-piece bf16 split of an fp32 value, shared by the exact-piece kernels (conv_stem.hip, conv_wino_bf16.hip,
// conv_bf16x9.hip): v = v1 + v2 + v3 with v1 = v truncated to bf16, v2 = (v - v1) truncated, v3 = v - v1 - v2.  Both differences are exact
// fp32 subtractions and 24 = 3 x 8 significant bits, so the three pieces are bf16 numbers that add back to v bit for bit; the nine piece
// products of two split operands are each exact in an fp32 accumulator.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

namespace mp {

// host: the three pieces of v as bf16 bit patterns (hi, mid, lo)
static inline void bf16x9_split3(float v, unsigned short out[3]) {
  unsigned vb, rb, qb;
  memcpy(&vb, &v, 4);
  const unsigned h = vb & 0xFFFF0000u;
  float hf; memcpy(&hf, &h, 4);
  const float r = v - hf;
  memcpy(&rb, &r, 4);
  const unsigned m = rb & 0xFFFF0000u;
  float mf; memcpy(&mf, &m, 4);
  const float q = r - mf;
  memcpy(&qb, &q, 4);
  out[0] = (unsigned short)(h >> 16); out[1] = (unsigned short)(m >> 16); out[2] = (unsigned short)(qb >> 16);
}

typedef unsigned bf16x9_u32x4 __attribute__((ext_vector_type(4)));

// device: the eight fp32 values of one MFMA operand fragment (lo = elements 0..3, hi = 4..7) -> three bf16x8 fragments, piece 1 | 2 | 3
// (element 2j in the low half of dword j).  Four VALU per element (and, sub, and, sub) + three v_perm_b32 per element pair.
__device__ __forceinline__ void bf16x9_split8(const float4& lo, const float4& hi, bf16x9_u32x4 (&pc)[3]) {
  const float v[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  unsigned vb[8], rb[8], qb[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    vb[e] = __float_as_uint(v[e]);
    const float r = v[e] - __uint_as_float(vb[e] & 0xFFFF0000u);
    rb[e] = __float_as_uint(r);
    qb[e] = __float_as_uint(r - __uint_as_float(rb[e] & 0xFFFF0000u));
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) {   // v_perm_b32 selector 0x07060302: {hi16(second arg) low, hi16(first arg) high}
    pc[0][j] = __builtin_amdgcn_perm(vb[2 * j + 1], vb[2 * j], 0x07060302u);
    pc[1][j] = __builtin_amdgcn_perm(rb[2 * j + 1], rb[2 * j], 0x07060302u);
    pc[2][j] = __builtin_amdgcn_perm(qb[2 * j + 1], qb[2 * j], 0x07060302u);
  }
}

}  // namespace mp
