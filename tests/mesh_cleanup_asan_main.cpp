// TEST SUPPORT: the host emulation of the mesh clean-up kernels (tests/mesh_cleanup_emul.cpp) as a stand-alone program, to be built with
// -fsanitize=address,undefined and run on the CPU only (tests/test_mesh_cleanup_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads a file of calls written by that test -- per call: int32 op (0 components, 1 select, 2 cluster), V, F, with_colors, gx, gy, gz, nv, nf;
// float32 ox, oy, oz, cell; the vertices, colours, faces and (select) keep bytes; then what the plain build returned: for components
// labels, face labels, face counts and the four totals, else the three totals, vertices, colours and faces -- runs the call on arrays of
// exactly the call's sizes and compares bit for bit.  Exit code 0 when everything agrees.
#include <cstdio>

#include "mesh_cleanup_emul.cpp"

template <typename T>
static bool read_n(std::FILE* f, std::vector<T>* v, size_t n) {
  v->assign(n, T());
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

template <typename T>
static bool same(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T>
static T* ptr(std::vector<T>& v) { return v.empty() ? nullptr : v.data(); }

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s calls.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_calls = 0, bad = 0;
  int32_t hd[9];
  float fl[4];
  while (std::fread(hd, sizeof(int32_t), 9, f) == 9) {
    if (std::fread(fl, sizeof(float), 4, f) != 4) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    const int op = hd[0], V = hd[1], F = hd[2], with_colors = hd[3], gx = hd[4], gy = hd[5], gz = hd[6], nv = hd[7], nf = hd[8];
    if (op < 0 || op > 2 || !meshc::counts_ok(V, F) || nv < 0 || nf < 0) { std::fprintf(stderr, "call %d: bad header\n", n_calls); return 2; }
    std::vector<float> vertices, colors, want_v, want_c;
    std::vector<int32_t> faces, want_f, want_labels, want_flabels, want_fcount, want_totals;
    std::vector<uint8_t> keep;
    bool ok = read_n(f, &vertices, (size_t)V * 3) && read_n(f, &colors, with_colors ? (size_t)V * 3 : 0) && read_n(f, &faces, (size_t)F * 3) &&
              read_n(f, &keep, op == 1 ? (size_t)F : 0);
    if (op == 0)
      ok = ok && read_n(f, &want_labels, (size_t)V) && read_n(f, &want_flabels, (size_t)F) && read_n(f, &want_fcount, (size_t)V) && read_n(f, &want_totals, 4);
    else
      ok = ok && read_n(f, &want_totals, 3) && read_n(f, &want_v, (size_t)nv * 3) && read_n(f, &want_c, with_colors ? (size_t)nv * 3 : 0) &&
           read_n(f, &want_f, (size_t)nf * 3);
    if (!ok) { std::fprintf(stderr, "call %d: short file\n", n_calls); return 2; }
    bool agree = false;
    int rc = -1;
    if (op == 0) {
      std::vector<int32_t> labels((size_t)V, -7), flabels((size_t)F, -7), fcount((size_t)V, -7), totals(4, -7);
      rc = mesh_components_emul(V, ptr(faces), F, ptr(labels), ptr(flabels), ptr(fcount), totals.data());
      agree = rc == 0 && same(labels, want_labels) && same(flabels, want_flabels) && same(fcount, want_fcount) && same(totals, want_totals);
    } else {
      std::vector<int32_t> totals(3, -7), out_f((size_t)nf * 3, -7);
      std::vector<float> out_v((size_t)nv * 3, -7.f), out_c(with_colors ? (size_t)nv * 3 : 0, -7.f);
      if (op == 1) {
        rc = mesh_select_count_emul(V, ptr(faces), F, ptr(keep), totals.data());
        if (rc == 0 && same(totals, want_totals) && totals[0] == nv && totals[1] == nf)
          rc = mesh_select_emul(ptr(vertices), ptr(colors), V, ptr(faces), F, ptr(keep), nv, nf, ptr(out_v), ptr(out_c), ptr(out_f), nv, nf);
        else
          rc = rc ? rc : -2;
      } else {
        rc = mesh_cluster_count_emul(ptr(vertices), V, ptr(faces), F, fl[0], fl[1], fl[2], fl[3], gx, gy, gz, totals.data());
        if (rc == 0 && same(totals, want_totals) && totals[0] == nv && totals[1] == nf)
          rc = mesh_cluster_emul(ptr(vertices), ptr(colors), V, ptr(faces), F, fl[0], fl[1], fl[2], fl[3], gx, gy, gz, nv, nf, ptr(out_v), ptr(out_c),
                                 ptr(out_f), nv, nf);
        else
          rc = rc ? rc : -2;
      }
      agree = rc == 0 && same(out_v, want_v) && same(out_c, want_c) && same(out_f, want_f);
    }
    if (!agree) {
      std::fprintf(stderr, "call %d (op %d, %d vertices, %d faces): rc %d, results differ\n", n_calls, op, V, F, rc);
      ++bad;
    }
    ++n_calls;
  }
  std::fclose(f);
  std::printf("%d calls, %d bad\n", n_calls, bad);
  return bad ? 1 : 0;
}
