// TEST SUPPORT: the host emulation of the run-length kernels (tests/rle_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_rle_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of calls written by that test -- per call: int32 kind, n, h, w, rows_per_segment, total; for kind 0 (encode) the masks,
// the offsets (int64), and the counts, areas and boxes the plain build returned; for kind 1 (decode) the offsets, the counts, and the
// masks and status the plain build returned -- runs each call on arrays of exactly these sizes and compares.  Exit code 0 when
// everything agrees.
#include <cstdio>

#include "rle_emul.cpp"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->assign(n, T());
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s calls.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_calls = 0, bad = 0;
  int32_t head[6];
  while (std::fread(head, sizeof(int32_t), 6, f) == 6) {
    const int kind = head[0], n = head[1], h = head[2], w = head[3], rows = head[4], total = head[5];
    if ((kind != 0 && kind != 1) || n < 1 || h < 1 || w < 1 || total < 0) { std::fprintf(stderr, "call %d: bad header\n", n_calls); return 2; }
    const size_t px = (size_t)n * h * w;
    std::vector<uint8_t> masks, want_masks;
    std::vector<int64_t> offsets;
    std::vector<int32_t> counts, want_counts, want_areas, want_boxes, want_status;
    bool ok, agree;
    int rc;
    if (kind == 0) {
      ok = read_n(f, &masks, px) && read_n(f, &offsets, (size_t)n + 1) && read_n(f, &want_counts, (size_t)total) && read_n(f, &want_areas, (size_t)n) &&
           read_n(f, &want_boxes, (size_t)n * 4);
      if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
      std::vector<int32_t> n_counts((size_t)n), areas((size_t)n), boxes((size_t)n * 4);
      counts.assign((size_t)total, -7);
      rc = rle_count_emul(masks.data(), n, h, w, rows, n_counts.data(), areas.data(), boxes.data());
      agree = rc == 0;
      for (int m = 0; m < n && agree; ++m) agree = n_counts[m] == offsets[m + 1] - offsets[m];
      if (agree) rc = rle_encode_emul(masks.data(), n, h, w, rows, offsets.data(), counts.data(), total);
      agree = agree && rc == 0 && same(counts, want_counts) && same(areas, want_areas) && same(boxes, want_boxes);
    } else {
      ok = read_n(f, &offsets, (size_t)n + 1) && read_n(f, &counts, (size_t)total) && read_n(f, &want_masks, px) && read_n(f, &want_status, (size_t)n);
      if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
      std::vector<int32_t> status((size_t)n);
      masks.assign(px, 9);
      rc = rle_decode_emul(counts.data(), offsets.data(), total, n, h, w, masks.data(), status.data());
      agree = rc == 0 && same(masks, want_masks) && same(status, want_status);
    }
    if (!agree) {
      std::fprintf(stderr, "call %d (kind %d, %d masks of %d x %d, rows %d): rc %d, results differ\n", n_calls, kind, n, h, w, rows, rc);
      ++bad;
    }
    ++n_calls;
  }
  std::fclose(f);
  std::printf("%d calls, %d bad\n", n_calls, bad);
  return bad ? 1 : 0;
}
