// TEST SUPPORT: host emulation of the BOP matching kernel (megapose6d_amd/csrc/bop_match.hip), built from the same rules header
// (bop_match_core.h).  Same arguments as the C ABI, on host arrays: one plain loop over groups, problems and estimates, the taken set as
// bits in a vector of the group's size -- no staging, no mask, no choice of path.  Every result is an integer, so the kernel is held to
// these results exactly.  Built by tests/support/bop_match.py.
#include <cstdint>
#include <vector>

#include "bop_match_core.h"

using namespace mp;

extern "C" int bop_match_emul(const float* errs, const int32_t* cand_gt, const int32_t* cand_lgt, const int32_t* est_row, const int32_t* est_off,
                              const int32_t* group_est_off, const int32_t* group_n_gt, const int32_t* n_top, const double* thr, int P, int n_groups,
                              int E, int n_theta, int32_t* match) {
  if (!bopm::sizes_ok(E, n_theta) || P < 0 || n_groups < 0) return 1;
  const size_t n_prob = (size_t)E * n_theta;
  for (size_t i = 0; i < (size_t)P * n_prob; ++i) match[i] = -1;
  for (int g = 0; g < n_groups; ++g) {
    const int e0 = group_est_off[g];
    const int nw = bopm::n_walk(group_est_off[g + 1] - e0, n_top ? n_top[g] : 0);
    std::vector<uint32_t> bits((size_t)bopm::taken_words(group_n_gt[g]) + 1);
    for (size_t p = 0; p < n_prob; ++p) {
      for (auto& w : bits) w = 0u;
      bopm::BitsMem taken{bits.data(), 1};
      const double t = thr[(size_t)g * n_prob + p];
      for (int i = 0; i < nw; ++i) {
        const int best = bopm::best_candidate(errs, E, (int)(p / n_theta), cand_lgt, est_off[e0 + i], est_off[e0 + i + 1], t, taken);
        if (best < 0) continue;
        taken.set(cand_lgt[best]);
        match[(size_t)est_row[e0 + i] * n_prob + p] = cand_gt[best];
      }
    }
  }
  return 0;
}

extern "C" void bop_match_emul_limits(int* v) {
  v[0] = bopm::kMaxErrors;
  v[1] = bopm::kMaxThetas;
  v[2] = bopm::kMaskBits;
  v[3] = bopm::kStageFloats;
}
