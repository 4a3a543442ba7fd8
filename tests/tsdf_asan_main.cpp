// TEST SUPPORT: the host emulation of the TSDF kernels (tests/tsdf_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_tsdf_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of calls written by that test -- per call: int32 nx, ny, nz, color, n, h, w, tco_floats, carve, with_masks, with_rgb,
// min_views, nv, nt; float32 ox, oy, oz, voxel, mu, z_min; the depth, masks, rgb, K and TCO of the views; then the volume, vertices, colours
// and faces the plain build returned -- integrates the views into a zero volume in two calls (the first half, the rest), extracts, all on
// arrays of exactly the call's sizes, and compares bit for bit.  Exit code 0 when everything agrees.
#include <cstdio>

#include "tsdf_emul.cpp"

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
  int32_t hd[14];
  float fl[6];
  while (std::fread(hd, sizeof(int32_t), 14, f) == 14) {
    if (std::fread(fl, sizeof(float), 6, f) != 6) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    const int nx = hd[0], ny = hd[1], nz = hd[2], color = hd[3], n = hd[4], h = hd[5], w = hd[6], tco = hd[7], carve = hd[8], with_masks = hd[9],
              with_rgb = hd[10], min_views = hd[11], nv = hd[12], nt = hd[13];
    if (!tsdf::dims_ok(nx, ny, nz) || n < 0 || h < 1 || w < 1 || nv < 0 || nt < 0) { std::fprintf(stderr, "call %d: bad header\n", n_calls); return 2; }
    const size_t N = (size_t)nx * ny * nz, hw = (size_t)h * w, words = N * tsdf::planes(color);
    std::vector<float> depth, K, TCO, want_v, want_c;
    std::vector<uint8_t> masks, rgb;
    std::vector<uint32_t> want_vol;
    std::vector<int32_t> want_f;
    const bool ok = read_n(f, &depth, n * hw) && read_n(f, &masks, with_masks ? n * hw : 0) && read_n(f, &rgb, with_rgb ? n * hw * 3 : 0) &&
                    read_n(f, &K, (size_t)n * 9) && read_n(f, &TCO, (size_t)n * tco) && read_n(f, &want_vol, words) && read_n(f, &want_v, (size_t)nv * 3) &&
                    read_n(f, &want_c, (size_t)nv * 3) && read_n(f, &want_f, (size_t)nt * 3);
    if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    std::vector<uint32_t> vol(words, 0u);
    const int n0 = n / 2;
    int rc = tsdf_integrate_emul(vol.data(), nx, ny, nz, color, fl[0], fl[1], fl[2], fl[3], depth.data(), with_masks ? masks.data() : nullptr,
                                 with_rgb ? rgb.data() : nullptr, K.data(), TCO.data(), tco, n0, h, w, fl[4], fl[5], carve);
    if (rc == 0 && n > n0)
      rc = tsdf_integrate_emul(vol.data(), nx, ny, nz, color, fl[0], fl[1], fl[2], fl[3], depth.data() + n0 * hw, with_masks ? masks.data() + n0 * hw : nullptr,
                               with_rgb ? rgb.data() + n0 * hw * 3 : nullptr, K.data() + (size_t)n0 * 9, TCO.data() + (size_t)n0 * tco, tco, n - n0, h, w,
                               fl[4], fl[5], carve);
    bool agree = rc == 0 && same(vol, want_vol);
    int32_t totals[2] = {-1, -1};
    std::vector<float> v((size_t)nv * 3, -7.f), c((size_t)nv * 3, -7.f);
    std::vector<int32_t> faces((size_t)nt * 3, -7);
    if (agree) {
      rc = tsdf_extract_count_emul(vol.data(), nx, ny, nz, color, min_views, totals);
      agree = rc == 0 && totals[0] == nv && totals[1] == nt;
    }
    if (agree) {
      rc = tsdf_extract_emul(vol.data(), nx, ny, nz, color, fl[0], fl[1], fl[2], fl[3], min_views, nv, nt, nv ? v.data() : nullptr, nv ? c.data() : nullptr,
                             nt ? faces.data() : nullptr, nv, nt);
      agree = rc == 0 && same(v, want_v) && same(c, want_c) && same(faces, want_f);
    }
    if (!agree) {
      std::fprintf(stderr, "call %d (%d x %d x %d, %d views of %d x %d): rc %d, totals %d %d, results differ\n", n_calls, nx, ny, nz, n, h, w, rc, totals[0],
                   totals[1]);
      ++bad;
    }
    ++n_calls;
  }
  std::fclose(f);
  std::printf("%d calls, %d bad\n", n_calls, bad);
  return bad ? 1 : 0;
}
