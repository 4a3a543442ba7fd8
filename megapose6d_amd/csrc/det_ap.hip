// det_ap.hip -- the device side of BOP's 2D detection / segmentation scores (COCO average precision): the pixel counts of every
// (detection mask, ground-truth mask) candidate, and COCO's greedy matching of detections to ground truths at every IoU threshold.
//
// The rules are det_ap_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Every result is an
// integer (a sum of integers, or picked by comparisons), so neither the grid, the split nor the arrival order can change a bit.
//
//   mask_pair_counts_kernel  grid (candidate, slice of the mask), 4 waves.  The two masks are read where they lie, as bytes: nothing is
//                            packed first and there is no scratch (the byte accounting of that choice is DESIGN.md 3.11).  VEC (H * W a
//                            multiple of 16 and both tensors 16-byte aligned, so every mask starts on a 16-byte boundary): a lane loads
//                            16 bytes of each mask per step, marks the non-zero bytes of each 8-byte half in their high bits
//                            [dap::nonzero_bytes] and takes three population counts (a & b, a, b).  Otherwise one byte per lane and
//                            step, the same sums.  Lane sums -> wave butterfly -> LDS -> one integer atomicAdd per non-zero counter and
//                            workgroup, on counts the entry point zeroed on the stream.  A candidate whose index is out of range reads
//                            nothing: its first slice stores -1 -1 -1.
//   det_match_kernel         16 groups per workgroup, 16 lanes per group, lane k < n_theta owns problem (group, k): a private walk over
//                            the group's estimates and candidates where they lie in global memory, the taken set as bits in the
//                            workspace (word w of problem k at [taken_off + w][k]), zeroed by the lane itself.  One path, any group
//                            size.  The launch is tiny next to the pair counts and is not tuned.
//   The match table is set to -1 by a memset on the stream (0xff bytes) before the kernel, which stores matches only.
#include "common.h"
#include "det_ap_core.h"

namespace mp {

constexpr int kDetLanesPerGroup = dap::kMaxThetas;            // 16
constexpr int kDetGroupsPerBlock = 256 / kDetLanesPerGroup;   // 16

// units [blockIdx.y * per_block, + per_block) of the n_units of candidate blockIdx.x; a unit is 16 bytes (VEC) or one
template <bool VEC>
__global__ __launch_bounds__(256) void mask_pair_counts_kernel(const uint8_t* __restrict__ pred, const uint8_t* __restrict__ gt,
                                                               const int32_t* __restrict__ cand_pred, const int32_t* __restrict__ cand_gt,
                                                               int P, int G, size_t hw, size_t n_units, size_t per_block,
                                                               int32_t* __restrict__ counts) {
  __shared__ int32_t red[4][3];
  const size_t c = blockIdx.x;
  const int ip = cand_pred[c], ig = cand_gt[c];
  int32_t* out = counts + c * 3;
  if (ip < 0 || ip >= P || ig < 0 || ig >= G) {   // uniform
    if (blockIdx.y == 0 && threadIdx.x < 3) out[threadIdx.x] = -1;
    return;
  }
  const uint8_t* A = pred + (size_t)ip * hw;
  const uint8_t* B = gt + (size_t)ig * hw;
  const size_t start = (size_t)blockIdx.y * per_block;
  const size_t end = start + per_block < n_units ? start + per_block : n_units;
  int32_t inter = 0, area_a = 0, area_b = 0;
  if (VEC) {
    const uint4* A16 = reinterpret_cast<const uint4*>(A);
    const uint4* B16 = reinterpret_cast<const uint4*>(B);
#pragma unroll 4
    for (size_t i = start + threadIdx.x; i < end; i += 256) {
      const uint4 a = A16[i], b = B16[i];
      const uint64_t a0 = dap::nonzero_bytes((uint64_t)a.x | ((uint64_t)a.y << 32)), a1 = dap::nonzero_bytes((uint64_t)a.z | ((uint64_t)a.w << 32));
      const uint64_t b0 = dap::nonzero_bytes((uint64_t)b.x | ((uint64_t)b.y << 32)), b1 = dap::nonzero_bytes((uint64_t)b.z | ((uint64_t)b.w << 32));
      inter += __popcll(a0 & b0) + __popcll(a1 & b1);
      area_a += __popcll(a0) + __popcll(a1);
      area_b += __popcll(b0) + __popcll(b1);
    }
  } else {
    for (size_t i = start + threadIdx.x; i < end; i += 256) {
      const bool a = A[i] != 0, b = B[i] != 0;
      inter += a && b;
      area_a += a;
      area_b += b;
    }
  }
  inter = wave_sum_all(inter);
  area_a = wave_sum_all(area_a);
  area_b = wave_sum_all(area_b);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) {
    red[wave][0] = inter;
    red[wave][1] = area_a;
    red[wave][2] = area_b;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k >= 3) return;
  const int32_t s = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
  if (s != 0) atomicAdd(out + k, s);
}

__global__ __launch_bounds__(256) void det_match_kernel(const double* __restrict__ iou, const int32_t* __restrict__ cand_gt,
                                                        const int32_t* __restrict__ cand_lgt, const int32_t* __restrict__ est_row,
                                                        const int32_t* __restrict__ est_off, const int32_t* __restrict__ group_est_off,
                                                        const int32_t* __restrict__ group_n_gt, const int32_t* __restrict__ group_taken_off,
                                                        const int32_t* __restrict__ n_top, const uint8_t* __restrict__ gt_ignore,
                                                        const double* __restrict__ thr, int n_groups, int n_theta,
                                                        int32_t* __restrict__ match, uint32_t* __restrict__ taken_ws) {
  const int g = blockIdx.x * kDetGroupsPerBlock + threadIdx.x / kDetLanesPerGroup, k = threadIdx.x % kDetLanesPerGroup;
  if (g >= n_groups || k >= n_theta) return;
  const int e0 = group_est_off[g];
  const int nw = bopm::n_walk(group_est_off[g + 1] - e0, n_top ? n_top[g] : 0);
  bopm::BitsMem taken{taken_ws + (size_t)group_taken_off[g] * n_theta + k, (size_t)n_theta};
  for (int w = 0; w < bopm::taken_words(group_n_gt[g]); ++w) taken.word[(size_t)w * n_theta] = 0u;
  const double bar = dap::bar(thr[k]);
  for (int i = 0; i < nw; ++i) {
    const int best = dap::best_candidate(iou, cand_gt, cand_lgt, gt_ignore, est_off[e0 + i], est_off[e0 + i + 1], bar, taken);
    if (best < 0) continue;
    taken.set(cand_lgt[best]);
    match[(size_t)est_row[e0 + i] * n_theta + k] = cand_gt[best];
  }
}

}  // namespace mp

using namespace mp;

extern "C" int mp_mask_pair_counts(const uint8_t* d_pred_masks, const uint8_t* d_gt_masks, const int32_t* d_cand_pred,
                                   const int32_t* d_cand_gt, int P, int G, int C, int H, int W, int split, int32_t* d_counts,
                                   mp_stream stream) {
  MP_REQUIRE(P >= 0 && G >= 0 && C >= 0 && split >= 0, "mp_mask_pair_counts: negative count");
  MP_REQUIRE(C <= dap::kMaxPairs, "mp_mask_pair_counts: %d candidates in one call, at most %d", C, dap::kMaxPairs);
  MP_REQUIRE(H >= 1 && W >= 1 && dap::pixels_ok((long long)H * W), "mp_mask_pair_counts: H * W of %d x %d outside 1 .. 2^31 - 1", H, W);
  if (C == 0) return MP_OK;
  MP_REQUIRE(d_pred_masks && d_gt_masks && d_cand_pred && d_cand_gt && d_counts, "mp_mask_pair_counts: null pointer");
  MP_REQUIRE(P >= 1 && G >= 1, "mp_mask_pair_counts: candidates but no masks");
  const size_t hw = (size_t)H * W;
  const bool vec = hw % 16 == 0 && (uintptr_t)d_pred_masks % 16 == 0 && (uintptr_t)d_gt_masks % 16 == 0;
  const size_t n_units = vec ? hw / 16 : hw;
  // a slice is a whole number of 256-lane steps; by default enough slices for about 2048 workgroups, and never more than 65535
  const size_t steps = (n_units + 255) / 256;
  size_t slices = split > 0 ? (size_t)split : (size_t)ceil_div(2048, C);
  if (slices > steps) slices = steps;
  if (slices > 65535) slices = 65535;
  const size_t per_block = (steps + slices - 1) / slices * 256;
  slices = (n_units + per_block - 1) / per_block;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("mask_pair_counts", 0.0, (double)C * (2.0 * hw + 20.0), s);
  MP_CHECK_HIP(hipMemsetAsync(d_counts, 0, (size_t)C * 3 * sizeof(int32_t), s));
  const dim3 grid(C, (unsigned)slices);
  if (vec)
    hipLaunchKernelGGL(mask_pair_counts_kernel<true>, grid, dim3(256), 0, s, d_pred_masks, d_gt_masks, d_cand_pred, d_cand_gt, P, G, hw, n_units,
                       per_block, d_counts);
  else
    hipLaunchKernelGGL(mask_pair_counts_kernel<false>, grid, dim3(256), 0, s, d_pred_masks, d_gt_masks, d_cand_pred, d_cand_gt, P, G, hw, n_units,
                       per_block, d_counts);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_det_match_workspace_bytes(int n_taken_words, int n_theta) {
  if (n_taken_words < 0 || !dap::sizes_ok(n_theta)) return 0;
  return (size_t)n_taken_words * n_theta * sizeof(uint32_t) + 256;
}

extern "C" int mp_det_match(const double* d_iou, const int32_t* d_cand_gt, const int32_t* d_cand_lgt, const int32_t* d_est_row,
                            const int32_t* d_est_off, const int32_t* d_group_est_off, const int32_t* d_group_n_gt,
                            const int32_t* d_group_taken_off, const int32_t* d_n_top, const uint8_t* d_gt_ignore, const double* d_thr, int P,
                            int C, int n_est, int n_groups, int n_taken_words, int n_theta, int32_t* d_match, void* d_workspace,
                            size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(P >= 0 && C >= 0 && n_est >= 0 && n_groups >= 0 && n_taken_words >= 0, "mp_det_match: negative count");
  MP_REQUIRE(dap::sizes_ok(n_theta), "mp_det_match: n_theta %d outside [1, %d]", n_theta, dap::kMaxThetas);
  if (P == 0) return MP_OK;
  MP_REQUIRE(d_match, "mp_det_match: null match table");
  hipStream_t s = (hipStream_t)stream;
  const bool empty = C == 0 || n_est == 0 || n_groups == 0;
  if (!empty) {
    MP_REQUIRE(d_iou && d_cand_gt && d_cand_lgt && d_est_row && d_est_off && d_group_est_off && d_group_n_gt && d_group_taken_off &&
                   d_gt_ignore && d_thr && d_workspace,
               "mp_det_match: null pointer");
    MP_REQUIRE(n_est <= C, "mp_det_match: %d listed estimates for %d candidates: each needs a candidate", n_est, C);
    MP_REQUIRE(workspace_bytes >= mp_det_match_workspace_bytes(n_taken_words, n_theta), "mp_det_match: workspace too small");
  }
  ProfScope prof("det_match", 0.0, (double)C * 16.0 + (double)P * n_theta * 4.0, s);
  MP_CHECK_HIP(hipMemsetAsync(d_match, 0xff, (size_t)P * n_theta * sizeof(int32_t), s));   // -1 everywhere
  if (empty) return MP_OK;
  hipLaunchKernelGGL(det_match_kernel, dim3(ceil_div(n_groups, kDetGroupsPerBlock)), dim3(256), 0, s, d_iou, d_cand_gt, d_cand_lgt, d_est_row,
                     d_est_off, d_group_est_off, d_group_n_gt, d_group_taken_off, d_n_top, d_gt_ignore, d_thr, n_groups, n_theta, d_match,
                     (uint32_t*)d_workspace);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
