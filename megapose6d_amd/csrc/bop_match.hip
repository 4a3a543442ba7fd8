// bop_match.hip -- BOP's greedy matching of pose estimates to ground truths, every (group, error column, threshold) problem at once.
//
// The rules are bop_match_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Every result is
// an integer picked by comparisons and no two problems share state, so neither the grid nor the path that handled a group can change it.
//
//   bop_match_kernel   one workgroup per group, one lane per (e, k) problem (E * n_theta <= 256 lanes; BOP's 12 x 10 = 120: two waves).
//                      All problems of a group walk the same estimates and the same candidates in the same order, so the loops are
//                      uniform over the workgroup and only the predicates differ between lanes.
//                      FAST PATH (the group has <= 64 ground truths and its walked candidates * E <= 4096 floats): the candidates'
//                      errors and local ground-truth numbers are staged in LDS once (lanes of one error column read one address: a
//                      broadcast; columns are consecutive floats: no bank conflict), the taken set is a 64-bit mask in the lane's
//                      registers.  20 KiB of LDS per workgroup: 8 workgroups per CU.
//                      GENERAL PATH (any other group): the same walk on the candidates where they lie in global memory, the taken set
//                      as bits in the workspace, word w of problem p at [taken_off + w][p] (consecutive lanes, consecutive words),
//                      zeroed by the workgroup itself.  No size is refused.
//   The match table is set to -1 by a memset on the stream (0xff bytes) before the kernel, which stores matches only.
#include "common.h"
#include "bop_match_core.h"

namespace mp {

using bopm::kStageFloats;

template <class Lgt, class Taken>
__device__ __forceinline__ void bopm_walk(const float* errs, const Lgt* lgt, int c_shift, const int32_t* __restrict__ cand_gt,
                                          const int32_t* __restrict__ est_row, const int32_t* __restrict__ est_off, int e0, int nw,
                                          int c_base, int E, int e, int p, int n_prob, double thr, Taken taken,
                                          int32_t* __restrict__ match) {
  // errs / lgt are addressed by (candidate - c_shift): c_shift = c_base for the staged copy, 0 in place
  int c0 = c_base;
  for (int i = 0; i < nw; ++i) {
    const int c1 = est_off[e0 + i + 1];
    const int best = bopm::best_candidate(errs, E, e, lgt, c0 - c_shift, c1 - c_shift, thr, taken);
    if (best >= 0) {
      taken.set((int)lgt[best]);
      match[(size_t)est_row[e0 + i] * n_prob + p] = cand_gt[c_shift + best];
    }
    c0 = c1;
  }
}

__global__ __launch_bounds__(256) void bop_match_kernel(const float* __restrict__ errs, const int32_t* __restrict__ cand_gt,
                                                        const int32_t* __restrict__ cand_lgt, const int32_t* __restrict__ est_row,
                                                        const int32_t* __restrict__ est_off, const int32_t* __restrict__ group_est_off,
                                                        const int32_t* __restrict__ group_n_gt,
                                                        const int32_t* __restrict__ group_taken_off, const int32_t* __restrict__ n_top,
                                                        const double* __restrict__ thr, int E, int n_theta, int32_t* __restrict__ match,
                                                        uint32_t* __restrict__ taken_ws) {
  __shared__ float errs_s[kStageFloats];
  __shared__ uint8_t lgt_s[kStageFloats];
  const int g = blockIdx.x;
  const int e0 = group_est_off[g];
  const int nw = bopm::n_walk(group_est_off[g + 1] - e0, n_top ? n_top[g] : 0);
  if (nw <= 0) return;   // uniform
  const int c_base = est_off[e0], n_cand = est_off[e0 + nw] - c_base;
  const int n_gt = group_n_gt[g];
  const int n_prob = E * n_theta, p = threadIdx.x;
  if (bopm::fast_path(n_gt, n_cand, E)) {   // uniform
    const float* src = errs + (size_t)c_base * E;
    for (int i = threadIdx.x; i < n_cand * E; i += blockDim.x) errs_s[i] = src[i];
    for (int i = threadIdx.x; i < n_cand; i += blockDim.x) lgt_s[i] = (uint8_t)cand_lgt[c_base + i];
    __syncthreads();
    if (p >= n_prob) return;
    bopm_walk(errs_s, lgt_s, c_base, cand_gt, est_row, est_off, e0, nw, c_base, E, p / n_theta, p, n_prob, thr[(size_t)g * n_prob + p],
              bopm::Mask64{0}, match);
  } else {
    if (p >= n_prob) return;
    bopm::BitsMem taken{taken_ws + (size_t)group_taken_off[g] * n_prob + p, (size_t)n_prob};
    for (int w = 0; w < bopm::taken_words(n_gt); ++w) taken.word[(size_t)w * n_prob] = 0u;
    bopm_walk(errs, cand_lgt, 0, cand_gt, est_row, est_off, e0, nw, c_base, E, p / n_theta, p, n_prob, thr[(size_t)g * n_prob + p], taken,
              match);
  }
}

}  // namespace mp

using namespace mp;

extern "C" int mp_bop_match_limits(int* max_errors, int* max_thetas, int* mask_bits, int* stage_floats) {
  if (max_errors) *max_errors = bopm::kMaxErrors;
  if (max_thetas) *max_thetas = bopm::kMaxThetas;
  if (mask_bits) *mask_bits = bopm::kMaskBits;
  if (stage_floats) *stage_floats = bopm::kStageFloats;
  return MP_OK;
}

extern "C" size_t mp_bop_match_workspace_bytes(int n_taken_words, int E, int n_theta) {
  if (n_taken_words < 0 || !bopm::sizes_ok(E, n_theta)) return 0;
  return (size_t)n_taken_words * E * n_theta * sizeof(uint32_t) + 256;
}

extern "C" int mp_bop_match(const float* d_errs, const int32_t* d_cand_gt, const int32_t* d_cand_lgt, const int32_t* d_est_row,
                            const int32_t* d_est_off, const int32_t* d_group_est_off, const int32_t* d_group_n_gt,
                            const int32_t* d_group_taken_off, const int32_t* d_n_top, const double* d_thr, int P, int C, int n_est,
                            int n_groups, int n_taken_words, int E, int n_theta, int32_t* d_match, void* d_workspace,
                            size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(P >= 0 && C >= 0 && n_est >= 0 && n_groups >= 0 && n_taken_words >= 0, "mp_bop_match: negative count");
  MP_REQUIRE(bopm::sizes_ok(E, n_theta), "mp_bop_match: E %d or n_theta %d outside [1, %d] x [1, %d]", E, n_theta, bopm::kMaxErrors,
             bopm::kMaxThetas);
  if (P == 0) return MP_OK;
  MP_REQUIRE(d_match, "mp_bop_match: null match table");
  hipStream_t s = (hipStream_t)stream;
  const size_t n_prob = (size_t)E * n_theta;
  const bool empty = C == 0 || n_est == 0 || n_groups == 0;
  if (!empty) {
    MP_REQUIRE(d_errs && d_cand_gt && d_cand_lgt && d_est_row && d_est_off && d_group_est_off && d_group_n_gt && d_group_taken_off &&
                   d_thr && d_workspace,
               "mp_bop_match: null pointer");
    MP_REQUIRE(n_est <= C, "mp_bop_match: %d listed estimates for %d candidates: each needs a candidate", n_est, C);
    MP_REQUIRE(workspace_bytes >= mp_bop_match_workspace_bytes(n_taken_words, E, n_theta), "mp_bop_match: workspace too small");
  }
  ProfScope prof("bop_match", 0.0, (double)C * (E * 4.0 + 8.0) + (double)P * n_prob * 4.0, s);
  MP_CHECK_HIP(hipMemsetAsync(d_match, 0xff, (size_t)P * n_prob * sizeof(int32_t), s));   // -1 everywhere
  if (empty) return MP_OK;
  const int threads = 64 * ceil_div((long)n_prob, 64);
  hipLaunchKernelGGL(bop_match_kernel, dim3(n_groups), dim3(threads), 0, s, d_errs, d_cand_gt, d_cand_lgt, d_est_row, d_est_off,
                     d_group_est_off, d_group_n_gt, d_group_taken_off, d_n_top, d_thr, E, n_theta, d_match, (uint32_t*)d_workspace);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
