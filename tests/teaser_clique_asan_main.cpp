// TEST SUPPORT: the host emulation of the maximum-clique selection (tests/teaser_clique_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_teaser_clique_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of cases written by that test -- per case: int32 stride, count (INT32_MIN: none given), max_steps, then stride x stride bytes of
// adjacency, then the stride int32 members and the 4 int32 of info the plain build returned -- runs each and compares; then one
// registration in the new mode on correspondences of its own.  Exit code 0 when everything agrees.
#include <cstdio>

#include "teaser_clique_emul.cpp"

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_cases = 0, bad = 0;
  int32_t head[3];
  while (std::fread(head, sizeof(int32_t), 3, f) == 3) {
    const int stride = head[0], max_steps = head[2];
    if (stride < 1 || stride > kMaxPoints) { std::fprintf(stderr, "case %d: bad stride %d\n", n_cases, stride); return 2; }
    std::vector<uint8_t> adj((size_t)stride * stride);
    std::vector<int32_t> want((size_t)stride + kCliqueInfo), members((size_t)stride), info(kCliqueInfo);
    if (std::fread(adj.data(), 1, adj.size(), f) != adj.size() || std::fread(want.data(), sizeof(int32_t), want.size(), f) != want.size()) {
      std::fprintf(stderr, "case %d: short file\n", n_cases);
      return 2;
    }
    const int32_t count = head[1];
    const int rc = teaser_clique_emul_max_clique(adj.data(), count == INT32_MIN ? nullptr : &count, 1, stride, max_steps, members.data(), info.data());
    const bool same = rc == 0 && std::memcmp(members.data(), want.data(), (size_t)stride * 4) == 0 && std::memcmp(info.data(), want.data() + stride, kCliqueInfo * 4) == 0;
    if (!same) {
      std::fprintf(stderr, "case %d (stride %d, count %d, budget %d): rc %d, info %d %d %d %d, want %d %d %d %d\n", n_cases, stride, count, max_steps, rc, info[0],
                   info[1], info[2], info[3], want[stride], want[stride + 1], want[stride + 2], want[stride + 3]);
      ++bad;
    }
    ++n_cases;
  }
  std::fclose(f);
  // the registration in the new mode: 60 points on a helix moved rigidly, every fifth one replaced
  const int n = 60;
  std::vector<float> S((size_t)n * 3), D((size_t)n * 3);
  for (int k = 0; k < n; ++k) {
    const float a = 0.37f * (float)k;
    S[3 * k] = 0.1f * std::cos(a); S[3 * k + 1] = 0.1f * std::sin(a); S[3 * k + 2] = 0.6f + 0.004f * (float)k;
    D[3 * k] = S[3 * k + 1] + 0.02f; D[3 * k + 1] = -S[3 * k] - 0.01f; D[3 * k + 2] = S[3 * k + 2] + 0.03f;   // a quarter turn about z and a shift
    if (k % 5 == 4) D[3 * k] += 0.2f + 0.01f * (float)k;
  }
  const int32_t counts[1] = {n};
  double Rt[12];
  int32_t retval[1], info[kInfo], cinfo[kCliqueInfo];
  std::vector<int32_t> deg((size_t)n), core((size_t)n), sel((size_t)n);
  const int rc = teaser_clique_emul_solve(S.data(), D.data(), counts, 1, n, 0.01f, kTimChain, 10, 1 << 20, Rt, retval, deg.data(), core.data(), sel.data(), info, cinfo);
  const bool ok = rc == 0 && retval[0] == 0 && cinfo[0] == 48 && cinfo[2] == 1 && info[2] == 48 && std::fabs(Rt[1] - 1.0) < 1e-6 && std::fabs(Rt[3] - 0.02) < 1e-6;
  if (!ok) {
    std::fprintf(stderr, "registration: rc %d retval %d clique %d %d %d %d selected %d R01 %.9f tx %.9f\n", rc, retval[0], cinfo[0], cinfo[1], cinfo[2], cinfo[3], info[2],
                 Rt[1], Rt[3]);
    ++bad;
  }
  std::printf("%d cases, %d bad\n", n_cases, bad);
  return bad ? 1 : 0;
}
