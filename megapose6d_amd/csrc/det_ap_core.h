// det_ap_core.h -- the rules of BOP's 2D detection / segmentation scores (COCO average precision) that run on the device (det_ap.hip),
// shared with the host emulation (tests/det_ap_emul.cpp) the way bop_match_core.h is shared with tests/bop_match_emul.cpp.
//
// CONTRACT OF THE MATCHING (mp_det_match; equals pycocotools' COCOeval.evaluateImg with iscrowd = 0 and one area range; integers and
// comparisons only)
//   * INPUTS.  P estimates with finite scores, G ground truths each with an ignore flag (a byte, set when non-zero), C candidates
//     (pred_row, gt_row) each with one float64 IoU, grouped as for mp_bop_match: a group is one (image, label), an estimate or a ground
//     truth belongs to one group.  thr[k], k < n_theta, float64: the IoU thresholds, the same for every group.  n_top[group] int32, 0 =
//     every estimate (COCO's maxDets).
//   * ORDER.  A group's estimates are walked by decreasing score, ties by ascending pred_row; the walk is cut to the first n_top[group]
//     estimates (0 means all) [bopm::n_walk].  An estimate's candidates are looked at by ascending gt_row.
//   * ONE PROBLEM = (group, k).  The bar is min(thr[k], 1 - 1e-10) in float64 [bar].  The estimate at hand looks at the ground truths
//     that no earlier estimate of this walk took.  It first looks at those with ignore == 0: it takes the one with the largest IoU that
//     is >= the bar, on an exact tie the LAST in gt_row order (COCO's loop replaces on equality) [best_candidate: a later candidate
//     replaces the best one when its IoU is >= the best one's].  Only if no such ground truth exists does it apply the same rule to
//     those with ignore != 0.  A taken ground truth, ignored or not, stays taken for the rest of the walk.  A NaN IoU never matches
//     (NaN >= bar is false).
//   * OUTPUT.  match[P, n_theta] int32 = the matched gt_row, -1 for no match (also for an estimate without candidates or cut by n_top).
// Nothing is accumulated and no two problems share state, so no grid, arrival order or mapping can change a result.
// Known deviation: stock pycocotools overwrites a ground truth's `ignore` with `iscrowd`; here the caller's flag is honoured.
// THE INDEX is the one of mp_bop_match, unchanged (bop_match_core.h, include/mp_engine.h).
//
// CONTRACT OF THE PAIR COUNTS (mp_mask_pair_counts).  Masks are bytes, a pixel is set when its byte is non-zero (0 / 1 of a bool tensor,
// 0 / 255 of mp_gt_info, anything else).  For candidate c: counts[c] = {pixels set in both masks, pixels set in pred_masks[cand_pred[c]],
// pixels set in gt_masks[cand_gt[c]]}, int32; a candidate whose index is outside [0, P) or [0, G) reads nothing and gives -1 -1 -1.
// H * W is in 1 .. 2^31 - 1, so a count fits an int32; the offset of a mask, row * H * W, is computed in size_t (it passes 2^31 long before
// a test can: at 480 x 640 from mask 6 991 on -- no test reaches it, the arithmetic is stated here instead).  Integer sums: no grid,
// split or arrival order can change a bit.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bop_match_core.h"   // n_walk, taken_words, BitsMem, kMaxThetas: the walk and the taken set are the pose matching's

namespace mp {
namespace dap {

constexpr int kMaxThetas = bopm::kMaxThetas;   // n_theta in 1..16 (COCO: 10)

constexpr int kMaxPairs = 1 << 23;             // candidates of one mp_mask_pair_counts call: one workgroup of 256 each, 2^31 threads along x

BOPM_HD bool sizes_ok(int n_theta) { return n_theta >= 1 && n_theta <= kMaxThetas; }

BOPM_HD bool pixels_ok(long long hw) { return hw >= 1 && hw <= 2147483647LL; }

BOPM_HD double bar(double thr) { return thr < 1.0 - 1e-10 ? thr : 1.0 - 1e-10; }

// the high bit of each byte of x that is non-zero (the SWAR form: the low seven bits carry into the high one, which is then or-ed in)
BOPM_HD uint64_t nonzero_bytes(uint64_t x) {
  const uint64_t low7 = 0x7f7f7f7f7f7f7f7fULL;
  return (((x & low7) + low7) | x) & ~low7;
}

// candidates c0 .. c1 - 1 of one estimate, ascending gt_row; iou[c]; lgt[c] = the ground truth's number inside the group; ignore[gt_row]
// -> the candidate to take, or -1
template <class Taken>
BOPM_HD int best_candidate(const double* iou, const int32_t* cand_gt, const int32_t* lgt, const uint8_t* ignore, int c0, int c1, double bar,
                           const Taken& taken) {
  int best = -1, best_ign = -1;   // among the ground truths with ignore == 0, among the others
  double best_iou = 0.0, best_ign_iou = 0.0;
  for (int c = c0; c < c1; ++c) {
    const double v = iou[c];
    if (!(v >= bar) || taken.test((int)lgt[c])) continue;
    if (ignore[cand_gt[c]] == 0) {
      if (best < 0 || v >= best_iou) {
        best = c;
        best_iou = v;
      }
    } else if (best_ign < 0 || v >= best_ign_iou) {
      best_ign = c;
      best_ign_iou = v;
    }
  }
  return best >= 0 ? best : best_ign;
}

}  // namespace dap
}  // namespace mp
