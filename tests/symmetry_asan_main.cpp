// TEST SUPPORT: the host emulation of the symmetry kernels (tests/symmetry_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_symmetry_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of calls written by that test -- per call: int32 n_obj, V, F, T, C, tile; the vertices, faces, test points, candidates,
// centres, the four prefix arrays and tol; then for mode 0 and for mode 1 the accept bytes, dev2 and worst points the plain build returned
// -- runs each call in both modes on arrays of exactly these sizes and compares bit for bit.  Exit code 0 when everything agrees.
#include <cstdio>

#include "symmetry_emul.cpp"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->assign(n, T());
  return std::fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s calls.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_calls = 0, bad = 0;
  int32_t head[6];
  while (std::fread(head, sizeof(int32_t), 6, f) == 6) {
    const int n_obj = head[0], V = head[1], F = head[2], T = head[3], C = head[4], tile = head[5];
    if (n_obj < 1 || V < 1 || F < 1 || T < 1 || C < 0) { std::fprintf(stderr, "call %d: bad header\n", n_calls); return 2; }
    std::vector<float> vertices, tests, cand_R, centers, tol;
    std::vector<int32_t> faces, off[4];
    bool ok = read_n(f, &vertices, (size_t)V * 3) && read_n(f, &faces, (size_t)F * 3) && read_n(f, &tests, (size_t)T * 3) &&
              read_n(f, &cand_R, (size_t)C * 9) && read_n(f, &centers, (size_t)n_obj * 3);
    for (int k = 0; k < 4; ++k) ok = ok && read_n(f, &off[k], (size_t)n_obj + 1);
    ok = ok && read_n(f, &tol, (size_t)n_obj);
    for (int mode = 0; mode < 2 && ok; ++mode) {
      std::vector<uint8_t> want_accept, accept((size_t)C);
      std::vector<float> want_dev2, dev2((size_t)C);
      std::vector<int32_t> want_worst, worst((size_t)C);
      ok = read_n(f, &want_accept, (size_t)C) && read_n(f, &want_dev2, (size_t)C) && read_n(f, &want_worst, (size_t)C);
      if (!ok) break;
      const int rc = symmetry_emul(vertices.data(), faces.data(), tests.data(), cand_R.data(), centers.data(), off[0].data(), off[1].data(),
                                   off[2].data(), off[3].data(), tol.data(), n_obj, tile, mode, nullptr, accept.data(), dev2.data(), worst.data());
      const bool same = rc == 0 && std::memcmp(accept.data(), want_accept.data(), (size_t)C) == 0 &&
                        std::memcmp(dev2.data(), want_dev2.data(), (size_t)C * 4) == 0 && std::memcmp(worst.data(), want_worst.data(), (size_t)C * 4) == 0;
      if (!same) {
        std::fprintf(stderr, "call %d (n_obj %d, %d candidates, tile %d), mode %d: rc %d, results differ\n", n_calls, n_obj, C, tile, mode, rc);
        ++bad;
      }
    }
    if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    ++n_calls;
  }
  std::fclose(f);
  std::printf("%d calls, %d bad\n", n_calls, bad);
  return bad ? 1 : 0;
}
