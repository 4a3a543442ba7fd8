// TEST SUPPORT: host emulation of the detection matching kernel (megapose6d_amd/csrc/det_ap.hip), built from the same rules header
// (det_ap_core.h).  Same arguments as the C ABI, on host arrays: one plain loop over groups, thresholds and estimates, the taken set as
// bits in a vector of the group's size -- no lanes, no workspace layout.  Every result is an integer, so the kernel is held to these
// results exactly.  Built by tests/support/det_ap.py.
#include <cstdint>
#include <vector>

#include "det_ap_core.h"

using namespace mp;

extern "C" int det_match_emul(const double* iou, const int32_t* cand_gt, const int32_t* cand_lgt, const int32_t* est_row, const int32_t* est_off,
                              const int32_t* group_est_off, const int32_t* group_n_gt, const int32_t* n_top, const uint8_t* gt_ignore,
                              const double* thr, int P, int n_groups, int n_theta, int32_t* match) {
  if (!dap::sizes_ok(n_theta) || P < 0 || n_groups < 0) return 1;
  for (size_t i = 0; i < (size_t)P * n_theta; ++i) match[i] = -1;
  for (int g = 0; g < n_groups; ++g) {
    const int e0 = group_est_off[g];
    const int nw = bopm::n_walk(group_est_off[g + 1] - e0, n_top ? n_top[g] : 0);
    std::vector<uint32_t> bits((size_t)bopm::taken_words(group_n_gt[g]) + 1);
    for (int k = 0; k < n_theta; ++k) {
      for (auto& w : bits) w = 0u;
      bopm::BitsMem taken{bits.data(), 1};
      const double bar = dap::bar(thr[k]);
      for (int i = 0; i < nw; ++i) {
        const int best = dap::best_candidate(iou, cand_gt, cand_lgt, gt_ignore, est_off[e0 + i], est_off[e0 + i + 1], bar, taken);
        if (best < 0) continue;
        taken.set(cand_lgt[best]);
        match[(size_t)est_row[e0 + i] * n_theta + k] = cand_gt[best];
      }
    }
  }
  return 0;
}

// the counts of one pair of masks of n bytes through the header's word test, eight bytes at a time and the rest bytewise
extern "C" void mask_pair_counts_emul(const uint8_t* a, const uint8_t* b, long long n, int32_t* out) {
  int32_t inter = 0, area_a = 0, area_b = 0;
  long long i = 0;
  for (; i + 8 <= n; i += 8) {
    uint64_t x = 0, y = 0;
    for (int k = 0; k < 8; ++k) {
      x |= (uint64_t)a[i + k] << (8 * k);
      y |= (uint64_t)b[i + k] << (8 * k);
    }
    const uint64_t mx = dap::nonzero_bytes(x), my = dap::nonzero_bytes(y);
    inter += __builtin_popcountll(mx & my);
    area_a += __builtin_popcountll(mx);
    area_b += __builtin_popcountll(my);
  }
  for (; i < n; ++i) {
    inter += a[i] != 0 && b[i] != 0;
    area_a += a[i] != 0;
    area_b += b[i] != 0;
  }
  out[0] = inter;
  out[1] = area_a;
  out[2] = area_b;
}

extern "C" void det_ap_emul_limits(int* v) {
  v[0] = dap::kMaxThetas;
  v[1] = dap::kMaxPairs;
}
