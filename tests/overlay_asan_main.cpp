// TEST SUPPORT: the host emulation of the overlay kernels (tests/overlay_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_overlay_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads two files written by that test.  cases.bin, per case: int32 n, h, w, k, tile_w, tile_h, has_labels, n_colors; the colours; images
// and render [n,h,w,3] bytes; labels [n,h,w] int32 when given; then the contour, canny, mask and mesh the plain build returned.  boxes.bin:
// int32 n, h, w, n_boxes, t, n_colors; colours, images, boxes (fp32), image ids (int32), the expected image.  Every buffer is allocated at
// its exact size, so a read or write past an end is caught.  Exit code 0 when everything agrees.
#include <cstdio>
#include <cstring>

#include "overlay_emul.cpp"

template <class T>
static bool read_vec(std::FILE* f, std::vector<T>& v, size_t count) {
  v.resize(count);
  return std::fread(v.data(), sizeof(T), count, f) == count;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s cases.bin boxes.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_cases = 0, bad = 0;
  int32_t head[8];
  while (std::fread(head, sizeof(int32_t), 8, f) == 8) {
    const int n = head[0], h = head[1], w = head[2], k = head[3], tw = head[4], th = head[5], has_labels = head[6], n_colors = head[7];
    if (!ovl::sizes_ok(n, h, w) || n_colors < 1 || n_colors > 1024) { std::fprintf(stderr, "case %d: bad header\n", n_cases); return 2; }
    const size_t px = (size_t)n * h * w;
    std::vector<uint8_t> colors, images, render, want[4], got[4];
    std::vector<int32_t> labels;
    bool ok = read_vec(f, colors, (size_t)n_colors * 3) && read_vec(f, images, px * 3) && read_vec(f, render, px * 3);
    if (has_labels) ok = ok && read_vec(f, labels, px);
    const size_t sizes[4] = {px * 3, px, px, px * 3};   // contour, canny, mask, mesh
    for (int o = 0; o < 4; ++o) ok = ok && read_vec(f, want[o], sizes[o]);
    if (!ok) { std::fprintf(stderr, "case %d: short file\n", n_cases); return 2; }
    for (int o = 0; o < 4; ++o) got[o].assign(sizes[o], 0x5A);
    const int rc = overlay_emul(images.data(), render.data(), has_labels ? labels.data() : nullptr, colors.data(), n_colors, n, h, w, k, tw, th,
                                got[0].data(), got[1].data(), got[2].data(), got[3].data());
    bool same = rc == 0;
    for (int o = 0; o < 4; ++o) same = same && got[o] == want[o];
    if (!same) { std::fprintf(stderr, "case %d (%d x %d x %d, k %d, tile %d x %d): rc %d, outputs differ\n", n_cases, n, h, w, k, tw, th, rc); ++bad; }
    ++n_cases;
  }
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f) { std::perror(argv[2]); return 2; }
  int32_t bh[6];
  if (std::fread(bh, sizeof(int32_t), 6, f) != 6 || !ovl::sizes_ok(bh[0], bh[1], bh[2]) || bh[3] < 0 || bh[3] > 4096 || bh[5] < 1 || bh[5] > 1024) {
    std::fprintf(stderr, "boxes: bad header\n");
    return 2;
  }
  const size_t bytes = (size_t)bh[0] * bh[1] * bh[2] * 3;
  std::vector<uint8_t> colors, images, want, got(bytes, 0x5A);
  std::vector<float> boxes;
  std::vector<int32_t> ids;
  if (!(read_vec(f, colors, (size_t)bh[5] * 3) && read_vec(f, images, bytes) && read_vec(f, boxes, (size_t)bh[3] * 4) && read_vec(f, ids, (size_t)bh[3]) &&
        read_vec(f, want, bytes))) {
    std::fprintf(stderr, "boxes: short file\n");
    return 2;
  }
  std::fclose(f);
  const int rc = overlay_emul_boxes(images.data(), boxes.data(), ids.data(), bh[3], colors.data(), bh[5], bh[0], bh[1], bh[2], bh[4], got.data());
  if (rc != 0 || got != want) { std::fprintf(stderr, "boxes: rc %d, output differs\n", rc); ++bad; }
  std::printf("%d cases, 1 box case, %d bad\n", n_cases, bad);
  return bad ? 1 : 0;
}
