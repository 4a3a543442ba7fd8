// bop_match_core.h -- the rules of BOP's greedy matching of pose estimates to ground truths (bop_match.hip), shared with the host
// emulation (tests/bop_match_emul.cpp) the way vsd_core.h is shared with tests/vsd_emul.cpp.  What the reference does in pandas
// (evaluation/meters/utils.py: get_top_n_ids, match_poses on cand[cand.error < theta]) and bop_toolkit calls match_poses.
//
// CONTRACT (integers and comparisons only)
//   * INPUTS.  P estimates with finite scores, G ground truths, C candidates (pred_row, gt_row) each with E float32 errors.  Candidates
//     are grouped; a group is one (image, label), and an estimate or a ground truth belongs to one group.  thr[group, e, k], k <
//     n_theta, float64.  n_top[group] int32, 0 = every estimate.
//   * ORDER.  A group's estimates are walked by decreasing score, ties by ascending pred_row; with n_top[group] > 0 only the first
//     n_top[group] of them take part [n_walk].  An estimate's candidates are looked at by ascending gt_row.
//   * ONE PROBLEM = (group, e, k).  For the estimate at hand a candidate is admissible when its ground truth is still free in this
//     problem and (double)err < thr[group, e, k]: strict, made in float64 (the comparison `bop_recall` makes on the host), never true for
//     a NaN error [admissible].  The admissible candidate of the smallest error is taken, on an exact tie the first in gt_row order
//     [best_candidate: a later candidate replaces the best one only when strictly smaller]; its ground truth is then taken for the rest
//     of the walk.
//   * OUTPUT.  match[P, E, n_theta] int32 = the matched gt_row, -1 for no match (also for an estimate without candidates or cut by
//     n_top).
// Nothing is accumulated and no two problems share state, so no grid, arrival order or choice of path can change a result.
//
// THE INDEX the entry point takes (built by the caller, documented in include/mp_engine.h): candidates sorted by (group, walk order of
// their estimate, gt_row); per candidate the gt_row and the ground truth's number inside its group (its bit in the taken set); per
// listed estimate its pred_row and its range of candidates; per group its range of estimates, its count of ground truths and where its
// taken set starts in the scratch of the general path.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define BOPM_HD __host__ __device__ __forceinline__
#define BOPM_HDM __host__ __device__ __forceinline__   // on a member function
#else
#define BOPM_HD static inline
#define BOPM_HDM inline
#endif

namespace mp {
namespace bopm {

constexpr int kMaxErrors = 16;        // E in 1..16 (BOP: 10 VSD taus + MSSD + MSPD = 12)
constexpr int kMaxThetas = 16;        // n_theta in 1..16 (BOP: 10)
// the fast path: a group whose ground truths fit one 64-bit taken mask and whose walked candidates fit the LDS staging
constexpr int kMaskBits = 64;         // ground truths per group
constexpr int kStageFloats = 4096;    // (walked candidates of the group) * E staged errors

BOPM_HD bool sizes_ok(int E, int n_theta) { return E >= 1 && E <= kMaxErrors && n_theta >= 1 && n_theta <= kMaxThetas; }

// estimates of a group that take part
BOPM_HD int n_walk(int n_est, int n_top) { return (n_top > 0 && n_top < n_est) ? n_top : n_est; }

BOPM_HD bool fast_path(int n_gt, long n_cand_walked, int E) { return n_gt <= kMaskBits && n_cand_walked * E <= kStageFloats; }

// a group's taken set starts on a 32-bit word of its own
BOPM_HD int taken_words(int n_gt) { return (n_gt + 31) / 32; }

BOPM_HD bool admissible(float err, double thr) { return (double)err < thr; }

// taken set of the fast path: one bit per ground truth of the group, in the lane's registers
struct Mask64 {
  uint64_t m;
  BOPM_HDM bool test(int l) const { return (m >> l) & 1u; }
  BOPM_HDM void set(int l) { m |= (uint64_t)1 << l; }
};

// taken set of the general path (and of the emulation): bit l lives in word[(l / 32) * stride]
struct BitsMem {
  uint32_t* word;
  size_t stride;
  BOPM_HDM bool test(int l) const { return (word[(size_t)(l >> 5) * stride] >> (l & 31)) & 1u; }
  BOPM_HDM void set(int l) { word[(size_t)(l >> 5) * stride] |= (uint32_t)1 << (l & 31); }
};

// candidates c0 .. c1 - 1 of one estimate, ascending gt_row; errs[c * E + e]; lgt[c] = the ground truth's number inside the group
// -> the candidate to take, or -1.  The loop is the same for every problem; only the predicates differ.
template <class Lgt, class Taken>
BOPM_HD int best_candidate(const float* errs, int E, int e, const Lgt* lgt, int c0, int c1, double thr, const Taken& taken) {
  int best = -1;
  float best_err = 0.f;
  for (int c = c0; c < c1; ++c) {
    const float err = errs[(size_t)c * E + e];
    const bool ok = admissible(err, thr) && !taken.test((int)lgt[c]);
    if (ok && (best < 0 || err < best_err)) {
      best = c;
      best_err = err;
    }
  }
  return best;
}

}  // namespace bopm
}  // namespace mp
