// TEST SUPPORT: the host emulation of the template-matching kernels (tests/template_match_emul.cpp) as a stand-alone program, to be built
// with -fsanitize=address,undefined and run on the CPU only (tests/test_template_match_contract_cpu.py::test_emulation_under_the_sanitizers).
// Reads one file written by that test.  Per case: int32 n, h, w, blur, weak, T, the tile (w, h) of the quantise, response and match walks,
// n_templates, n_features, n_objects; the images [n,h,w,3]; the templates (int32 x 5) and features (4 bytes each); then what the plain build
// returned: ori, mag2, resp, best_score, best_f, best_template.  Every buffer is allocated at its exact size, so a read or write past an
// end is caught.  Exit code 0 when everything agrees.
#include <cstdio>
#include <cstring>

#include "template_match_emul.cpp"

template <class V>
static bool read_vec(std::FILE* f, std::vector<V>& v, size_t count) {
  v.resize(count);
  return count == 0 || std::fread(v.data(), sizeof(V), count, f) == count;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  int n_cases = 0, bad = 0;
  int32_t head[15];
  while (std::fread(head, sizeof(int32_t), 15, f) == 15) {
    const int n = head[0], h = head[1], w = head[2], blur = head[3], weak = head[4], T = head[5];
    const int n_templates = head[12], n_features = head[13], n_objects = head[14];
    if (!tmatch::match_args_ok(true, true, true, n, h, w, T, n_templates, n_features, n_objects)) { std::fprintf(stderr, "case %d: bad header\n", n_cases); return 2; }
    const size_t px = (size_t)n * h * w, gh = tmatch::cdiv(h, T), gw = tmatch::cdiv(w, T);
    const size_t resp_bytes = (size_t)n * 8 * T * T * gh * gw, locs = (size_t)n * n_objects * gh * gw;
    std::vector<uint8_t> images, features, want_ori, want_resp, want_score, want_f;
    std::vector<int32_t> templates, want_mag2, want_best;
    const bool ok = read_vec(f, images, px * 3) && read_vec(f, templates, (size_t)n_templates * 5) && read_vec(f, features, (size_t)n_features * 4) &&
                    read_vec(f, want_ori, px) && read_vec(f, want_mag2, px) && read_vec(f, want_resp, resp_bytes) && read_vec(f, want_score, locs) &&
                    read_vec(f, want_f, locs) && read_vec(f, want_best, locs);
    if (!ok) { std::fprintf(stderr, "case %d: short file\n", n_cases); return 2; }
    std::vector<uint8_t> ori(px, 0x5A), resp(resp_bytes, 0x5A), score(locs, 0x5A), fb(locs, 0x5A);
    std::vector<int32_t> mag2(px, 0x5A5A5A5A), best(locs, 0x5A5A5A5A);
    const int rc1 = tm_emul_quantize(images.data(), n, h, w, blur, weak, head[6], head[7], ori.data(), mag2.data());
    const int rc2 = tm_emul_response(ori.data(), n, h, w, T, head[8], head[9], resp.data());
    const int rc3 = tm_emul_match(resp.data(), n, h, w, T, templates.data(), features.data(), n_templates, n_features, n_objects, head[10], head[11],
                                  score.data(), fb.data(), best.data());
    const bool same = rc1 == 0 && rc2 == 0 && rc3 == 0 && ori == want_ori && mag2 == want_mag2 && resp == want_resp && score == want_score &&
                      fb == want_f && best == want_best;
    if (!same) { std::fprintf(stderr, "case %d (%d x %d x %d, T %d): rc %d %d %d, outputs differ\n", n_cases, n, h, w, T, rc1, rc2, rc3); ++bad; }
    ++n_cases;
  }
  std::fclose(f);
  std::printf("%d cases, %d bad\n", n_cases, bad);
  return bad ? 1 : 0;
}
