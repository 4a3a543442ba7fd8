// TEST SUPPORT: host emulation of the run-length kernels (megapose6d_amd/csrc/rle.hip), built from the same rules header (rle_core.h).
// Same arguments as the C ABI, on host arrays, and the same three steps per mask -- count the transitions of every entry (column, row
// segment), exclusive scans over the entries in walk order, write the differences -- as plain loops over single pixels: no lanes, no
// 16-byte units, no workspace layout.  Every result is an integer, so the kernels are held to these results exactly.  Built by
// tests/support/rle.py; tests/rle_asan_main.cpp includes this file.
#include <cstdint>
#include <cstring>
#include <vector>

#include "rle_core.h"

using namespace mp;

namespace {

struct Entries {
  int rows, S;
  std::vector<int32_t> count, last;   // per entry x * S + s: before the scan its transitions and the last one's position; after: rank, position before
  int32_t n_trans = 0, last_pos = 0;
};

// the transitions of entry (x, s) in walk order: f(p) for each
template <class F>
void entry_transitions(const uint8_t* mask, int h, int w, int rows, int x, int s, F f) {
  const int y1 = (s + 1) * rows < h ? (s + 1) * rows : h;
  for (int y = s * rows; y < y1; ++y) {
    const bool v = rle::is_set(mask[(size_t)y * w + x]);
    const bool before = rle::has_prev(x, y) && rle::is_set(mask[(size_t)rle::prev_y(y, h) * w + rle::prev_x(x, y)]);
    if (rle::transition(v, before)) f(x * h + y);
  }
}

Entries scan_entries(const uint8_t* mask, int h, int w, int rows_per_segment) {
  Entries e;
  e.rows = rle::rows_of(h, rows_per_segment);
  e.S = rle::segments(h, e.rows);
  e.count.assign((size_t)w * e.S, 0);
  e.last.assign((size_t)w * e.S, 0);
  for (int x = 0; x < w; ++x)
    for (int s = 0; s < e.S; ++s)
      entry_transitions(mask, h, w, e.rows, x, s, [&](int p) {
        ++e.count[(size_t)x * e.S + s];
        e.last[(size_t)x * e.S + s] = p;
      });
  int32_t sum = 0, mx = 0;
  for (size_t i = 0; i < e.count.size(); ++i) {
    const int32_t c = e.count[i], l = e.last[i];
    e.count[i] = sum;
    e.last[i] = mx;
    sum += c;
    mx = l > mx ? l : mx;
  }
  e.n_trans = sum;
  e.last_pos = mx;
  return e;
}

bool offsets_ok(const int64_t* offsets, int n, long long capacity) {
  if (offsets[0] != 0) return false;
  for (int m = 0; m < n; ++m)
    if (offsets[m + 1] < offsets[m] || offsets[m + 1] - offsets[m] > 2147483647LL) return false;
  return offsets[n] <= capacity;
}

}  // namespace

extern "C" int rle_count_emul(const uint8_t* masks, int n, int h, int w, int rows_per_segment, int32_t* n_counts, int32_t* areas, int32_t* boxes) {
  if (n < 0 || rows_per_segment < 0 || !rle::dims_ok(h, w)) return 1;
  for (int m = 0; m < n; ++m) {
    const uint8_t* mask = masks + (size_t)m * h * w;
    n_counts[m] = scan_entries(mask, h, w, rows_per_segment).n_trans + 1;
    int32_t area = 0, x_min = rle::kNoMin, y_min = rle::kNoMin, x_max = -1, y_max = -1;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x)
        if (rle::is_set(mask[(size_t)y * w + x])) {
          ++area;
          x_min = x < x_min ? x : x_min;
          x_max = x > x_max ? x : x_max;
          y_min = y < y_min ? y : y_min;
          y_max = y > y_max ? y : y_max;
        }
    if (areas) areas[m] = area;
    if (boxes) {
      boxes[4 * m + 0] = area ? x_min : 0;
      boxes[4 * m + 1] = area ? y_min : 0;
      boxes[4 * m + 2] = x_max;
      boxes[4 * m + 3] = y_max;
    }
  }
  return 0;
}

extern "C" int rle_encode_emul(const uint8_t* masks, int n, int h, int w, int rows_per_segment, const int64_t* offsets, int32_t* counts,
                               long long capacity) {
  if (n < 0 || rows_per_segment < 0 || !rle::dims_ok(h, w)) return 1;
  if (n == 0) return 0;
  if (capacity < 0 || !offsets_ok(offsets, n, capacity)) return 1;
  for (int m = 0; m < n; ++m) {
    const uint8_t* mask = masks + (size_t)m * h * w;
    const Entries e = scan_entries(mask, h, w, rows_per_segment);
    const int64_t off = offsets[m], n_list = offsets[m + 1] - off;
    for (int x = 0; x < w; ++x)
      for (int s = 0; s < e.S; ++s) {
        int32_t rank = e.count[(size_t)x * e.S + s], before = e.last[(size_t)x * e.S + s];
        entry_transitions(mask, h, w, e.rows, x, s, [&](int p) {
          if (rank < n_list) counts[off + rank] = p - before;
          ++rank;
          before = p;
        });
      }
    if (e.n_trans < n_list) counts[off + e.n_trans] = (int32_t)((long long)h * w) - e.last_pos;
  }
  return 0;
}

extern "C" int rle_decode_emul(const int32_t* counts, const int64_t* offsets, long long capacity, int n, int h, int w, uint8_t* masks,
                               int32_t* status) {
  if (n < 0 || !rle::dims_ok(h, w)) return 1;
  if (n == 0) return 0;
  if (capacity < 0 || !offsets_ok(offsets, n, capacity)) return 1;
  const long long hw = (long long)h * w;
  for (int m = 0; m < n; ++m) {
    uint8_t* mask = masks + (size_t)m * hw;
    const int64_t off = offsets[m], n_runs = offsets[m + 1] - off;
    std::vector<int32_t> ends((size_t)n_runs);
    long long sum = 0;
    bool negative = false;
    for (int64_t i = 0; i < n_runs; ++i) {
      negative = negative || counts[off + i] < 0;
      sum += counts[off + i];
      ends[(size_t)i] = (int32_t)sum;
    }
    status[m] = rle::status_of(n_runs, negative, sum, hw);
    std::memset(mask, 0, (size_t)hw);
    if (status[m] != 0) continue;
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) mask[(size_t)y * w + x] = (uint8_t)(rle::run_of(ends.data(), (int)n_runs, x * h + y) & 1);
  }
  return 0;
}

extern "C" void rle_emul_limits(long long* v) {
  v[0] = rle::kMaxPixels;
  v[1] = rle::kDefaultRows;
  v[2] = rle::kUnit;
}
