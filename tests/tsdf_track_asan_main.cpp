// TEST SUPPORT: the host emulation of the camera-tracking kernels (tests/tsdf_track_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_tsdf_track_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of calls written by that test -- per call: int32 nx, ny, nz, n, h, w, with_masks, min_views, min_pixels, iters; float32 ox,
// oy, oz, voxel, mu, eps_rot, eps_trans; the volume's two planes, the depth, masks, K and poses of the frames; then the poses, status,
// used, rms and records the plain build returned -- tracks on arrays of exactly the call's sizes and compares bit for bit.  Exit code 0
// when everything agrees.
#include <cstdio>

#include "tsdf_track_emul.cpp"

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
  int32_t hd[10];
  float fl[7];
  while (std::fread(hd, sizeof(int32_t), 10, f) == 10) {
    if (std::fread(fl, sizeof(float), 7, f) != 7) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    const int nx = hd[0], ny = hd[1], nz = hd[2], n = hd[3], h = hd[4], w = hd[5], with_masks = hd[6], min_views = hd[7], min_pixels = hd[8], iters = hd[9];
    const int groups = tsdf::track_groups(h, w);
    if (!tsdf::dims_ok(nx, ny, nz) || n < 1 || groups < 1) { std::fprintf(stderr, "call %d: bad header\n", n_calls); return 2; }
    const size_t N = (size_t)nx * ny * nz, hw = (size_t)h * w, recs = (size_t)n * groups * tsdf::kTrackRecord;
    std::vector<uint32_t> vol, want_T, want_rms;
    std::vector<float> depth, K, T_in;
    std::vector<uint8_t> masks;
    std::vector<int32_t> want_status, want_used;
    std::vector<uint64_t> want_rec;
    const bool ok = read_n(f, &vol, 2 * N) && read_n(f, &depth, n * hw) && read_n(f, &masks, with_masks ? n * hw : 0) && read_n(f, &K, (size_t)n * 9) &&
                    read_n(f, &T_in, (size_t)n * 16) && read_n(f, &want_T, (size_t)n * 16) && read_n(f, &want_status, (size_t)n) &&
                    read_n(f, &want_used, (size_t)n) && read_n(f, &want_rms, (size_t)n) && read_n(f, &want_rec, recs);
    if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    std::vector<uint32_t> T(want_T.size(), 0xdeadbeefu), rms(n, 0xdeadbeefu);
    std::vector<int32_t> status(n, -7), used(n, -7);
    std::vector<uint64_t> rec(want_rec);   // the records of a frame that never ran keep what they held
    const int rc = tsdf_track_emul(vol.data(), nx, ny, nz, 0, fl[0], fl[1], fl[2], fl[3], depth.data(), with_masks ? masks.data() : nullptr, K.data(),
                                   T_in.data(), n, h, w, fl[4], min_views, min_pixels, iters, fl[5], fl[6], (float*)T.data(), status.data(), used.data(),
                                   (float*)rms.data(), (double*)rec.data(), (long long)n * groups);
    if (!(rc == 0 && same(T, want_T) && same(status, want_status) && same(used, want_used) && same(rms, want_rms) && same(rec, want_rec))) {
      std::fprintf(stderr, "call %d (%d x %d x %d, %d frames of %d x %d, %d iterations): rc %d, results differ\n", n_calls, nx, ny, nz, n, h, w, iters, rc);
      ++bad;
    }
    ++n_calls;
  }
  std::fclose(f);
  std::printf("%d calls, %d bad\n", n_calls, bad);
  return bad ? 1 : 0;
}
