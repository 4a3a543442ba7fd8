// rle_core.h -- the rules of COCO's run-length encoding (RLE) of binary masks, the form in which BOP's detection and segmentation result
// files carry a mask, as they run on the device (rle.hip), shared with the host emulation (tests/rle_emul.cpp) the way det_ap_core.h is
// shared with tests/det_ap_emul.cpp.  Integers and comparisons only: every result is exact.
//
// CONTRACT OF THE FORMAT
//   * SET PIXELS.  A mask is h x w bytes, row-major in memory.  A pixel is set when its byte is non-zero -- the rule of
//     mp_mask_pair_counts [dap::nonzero_bytes]: 1, 2, 128 and 255 all count.
//   * RUNS.  RLE walks the mask in column-major order, p = x * h + y.  `counts` alternates run lengths of unset and set pixels, starting
//     with unset: counts[0] == 0 when pixel p = 0 is set.  A run continues from the bottom of column x into the top of column x + 1.
//   * SUM AND LENGTH.  sum(counts) == h * w.  An empty mask is [h * w], a full one [0, h * w]; the longest possible list has h * w + 1
//     entries.  Worked example: [[0,1],[1,1],[0,0]] (h = 3, w = 2) gives [1,1,1,2,1].
//   * POSITIONS.  With v[-1] := 0 the transitions are the p with v[p] != v[p - 1] [transition; the pixel before p in walk order is the
//     pixel above it, for row 0 the last row of the previous column, for p = 0 nothing: has_prev, prev_x, prev_y].  counts are the
//     differences of 0, pos..., h * w.
//   * AREA AND BOX.  Area = the sum of the odd entries = the number of set pixels.  The box is (x_min, y_min, x_max, y_max), inclusive; an
//     empty mask has the box (0, 0, -1, -1).
//   * A LIST IS MALFORMED [status_of] when it has no entries (kEmptyList), holds a negative entry (kNegativeEntry) or its sum is not
//     h * w (kBadSum); the status is the OR of these bits, 0 for a well-formed list.  A malformed list decodes to an all-zero mask.
//   * THE RUN OF A PIXEL [run_of].  ends[i] = counts[0] + .. + counts[i]; pixel p lies in run r = the number of ends <= p, and is set when
//     r is odd.  For a well-formed list ends[n_runs - 1] = h * w > p, so r <= n_runs - 1; the search halves [0, n_runs - 1] at most
//     kSearchSteps times whatever the data.
//   The compressed string of pycocotools (rleToString / rleFrString) is host-only Python (megapose6d_amd/bop_files.py).
//
// CONTRACT OF THE DECOMPOSITION (encoding).  A JOB is one (mask, row segment, unit): rows [s * rows, min(h, (s + 1) * rows)) of the
// kUnit = 16 columns [16 u, 16 u + 16).  rows = rows_of(h, rows_per_segment): 0 picks kDefaultRows, any value is cut to h.  An ENTRY is
// one (mask, column x, row segment s); in walk order the entries of a mask are numbered x * S + s.  The rank of a transition in `counts`
// is the number of transitions in the entries before its own plus the number above it inside its entry; the position before the first
// transition of an entry is the largest position of a transition in the entries before it (0 if there is none: the list's differences
// start from 0).  Both are exclusive scans over the entries; neither rows_per_segment nor any grid can change one output integer.
//
// LIMITS.  h, w >= 1; h * w <= 2^31 - 2 (a position, a rank and h * w + 1 fit an int32); n >= 0; at most kMaxJobs jobs and kMaxJobs
// entries per call; offsets are int64.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "det_ap_core.h"   // BOPM_HD, dap::nonzero_bytes: the set-pixel rule is the pair counts'

namespace mp {
namespace rle {

constexpr int kUnit = 16;                        // columns of one job: one 16-byte load per row
constexpr int kDefaultRows = 32;                 // rows of a job when rows_per_segment == 0
constexpr long long kMaxPixels = 2147483646LL;   // h * w
constexpr long long kMaxJobs = 1LL << 30;        // jobs (mask, segment, unit) and entries (mask, column, segment) of one call
constexpr int kSearchSteps = 32;                 // halvings of a list of at most 2^31 - 1 runs

constexpr int kEmptyList = 1, kNegativeEntry = 2, kBadSum = 4;   // status bits of a malformed list
constexpr int kStatsPerJob = 5;                  // area, x_min, x_max, y_min, y_max of a job's pixels
constexpr int kNoMin = 2147483647;               // x_min / y_min of a job without a set pixel (its x_max / y_max are -1)

BOPM_HD bool dims_ok(int h, int w) { return h >= 1 && w >= 1 && (long long)h * w <= kMaxPixels; }

BOPM_HD int rows_of(int h, int rows_per_segment) {
  const int r = rows_per_segment > 0 ? rows_per_segment : kDefaultRows;
  return r < h ? r : h;
}
BOPM_HD int segments(int h, int rows) { return (h + rows - 1) / rows; }
BOPM_HD int units(int w) { return (w + kUnit - 1) / kUnit; }

// the pixel before (x, y) in walk order
BOPM_HD bool has_prev(int x, int y) { return x > 0 || y > 0; }
BOPM_HD int prev_x(int x, int y) { return y > 0 ? x : x - 1; }
BOPM_HD int prev_y(int y, int h) { return y > 0 ? y - 1 : h - 1; }

BOPM_HD bool is_set(uint8_t byte) { return byte != 0; }
BOPM_HD bool transition(bool v, bool v_before) { return v != v_before; }

// the number of entries of the non-decreasing ends[0 .. n_runs - 1] that are <= p, at most n_runs - 1
BOPM_HD int run_of(const int32_t* ends, int n_runs, int p, int from = 0) {
  int lo = from, hi = n_runs - 1;
  for (int s = 0; s < kSearchSteps && lo < hi; ++s) {
    const int mid = lo + ((hi - lo) >> 1);
    if (ends[mid] > p) hi = mid; else lo = mid + 1;
  }
  return lo;
}

BOPM_HD int status_of(long long n_runs, bool any_negative, long long sum, long long hw) {
  return (n_runs < 1 ? kEmptyList : 0) | (any_negative ? kNegativeEntry : 0) | (sum != hw ? kBadSum : 0);
}

}  // namespace rle
}  // namespace mp
