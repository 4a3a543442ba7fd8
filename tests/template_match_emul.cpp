// TEST SUPPORT: host emulation of the template-matching kernels (megapose6d_amd/csrc/template_match.hip), built from the same rules header
// (template_match_core.h).  Same arguments as the C ABI, on host arrays, plus the tile size: the image (or the location map) is walked tile
// by tile as the workgroups do it -- bytes staged with a halo and clamped coordinates, the blur in two passes, the bins on the tile plus
// a halo of 1, the majority; the orientation bytes with a halo of T - 1, the OR rows first, then columns; the running best per location
// -- with plain loops: no lanes, no LDS, no split of the templates over waves.  Any tile size >= 1 must give the same bytes.  Built by
// tests/support/template_match.py; tests/template_match_asan_main.cpp drives it under the sanitizers.
#include <cstdint>
#include <vector>

#include "template_match_core.h"

using namespace mp;

extern "C" void tm_emul_limits(int* v) {
  v[0] = tmatch::kQuantTileW;
  v[1] = tmatch::kQuantTileH;
  v[2] = tmatch::kRespTileH;
  v[3] = tmatch::kLocW;
  v[4] = tmatch::kLocH;
  v[5] = tmatch::kMaxT;
  v[6] = tmatch::kMaxFeatures;
  v[7] = tmatch::kMaxBox;
  v[8] = tmatch::kMaxWeak;
  v[9] = tmatch::kMaxSide;
}

extern "C" int tm_emul_resp_tile_w(int T) { return T >= 1 && T <= tmatch::kMaxT ? tmatch::resp_tile_w(T) : 0; }

extern "C" int tm_emul_bin(int gx, int gy) { return tmatch::orientation_bin(gx, gy); }

extern "C" int tm_emul_quantize(const uint8_t* images, int n, int h, int w, int blur, int weak, int tile_w, int tile_h, uint8_t* ori, int32_t* mag2) {
  if (n == 0) return 0;
  if (!tmatch::quantize_args_ok(images != nullptr, ori != nullptr, n, h, w, weak) || tile_w < 1 || tile_h < 1) return 1;
  const int rw = tile_w + 2 * tmatch::kRawHalo, rh = tile_h + 2 * tmatch::kRawHalo;
  const int bw = tile_w + 2 * tmatch::kBlurHalo, bh = tile_h + 2 * tmatch::kBlurHalo;
  const int qw = tile_w + 2, qh = tile_h + 2;
  std::vector<uint8_t> raw((size_t)3 * rh * rw), blurred((size_t)3 * bh * bw), bins((size_t)qh * qw);
  std::vector<uint16_t> hsum((size_t)3 * rh * bw);
  for (int img = 0; img < n; ++img) {
    const size_t base = (size_t)img * h * w;
    for (int y0 = 0; y0 < h; y0 += tile_h)
      for (int x0 = 0; x0 < w; x0 += tile_w) {
        for (int ch = 0; ch < 3; ++ch)
          for (int r = 0; r < rh; ++r)
            for (int c = 0; c < rw; ++c) {
              const int x = tmatch::clampi(x0 - tmatch::kRawHalo + c, 0, w - 1), y = tmatch::clampi(y0 - tmatch::kRawHalo + r, 0, h - 1);
              raw[((size_t)ch * rh + r) * rw + c] = images[3 * (base + (size_t)y * w + x) + ch];
            }
        if (blur)
          for (int ch = 0; ch < 3; ++ch)
            for (int r = 0; r < rh; ++r)
              for (int c = 0; c < bw; ++c) {
                const int cx = tmatch::clampi(x0 - tmatch::kBlurHalo + c, 0, w - 1);
                hsum[((size_t)ch * rh + r) * bw + c] = (uint16_t)tmatch::blur_row(&raw[((size_t)ch * rh + r) * rw + (cx - x0 + tmatch::kRawHalo)], 1);
              }
        for (int ch = 0; ch < 3; ++ch)
          for (int r = 0; r < bh; ++r)
            for (int c = 0; c < bw; ++c) {
              const int cy = tmatch::clampi(y0 - tmatch::kBlurHalo + r, 0, h - 1);
              uint8_t v;
              if (blur) {
                v = (uint8_t)tmatch::blur_round(tmatch::blur_row(&hsum[((size_t)ch * rh + (cy - y0 + tmatch::kRawHalo)) * bw + c], bw));
              } else {
                const int cx = tmatch::clampi(x0 - tmatch::kBlurHalo + c, 0, w - 1);
                v = raw[((size_t)ch * rh + (cy - y0 + tmatch::kRawHalo)) * rw + (cx - x0 + tmatch::kRawHalo)];
              }
              blurred[((size_t)ch * bh + r) * bw + c] = v;
            }
        for (int r = 0; r < qh; ++r)
          for (int c = 0; c < qw; ++c) {
            const int x = x0 - 1 + c, y = y0 - 1 + r;
            uint8_t q = tmatch::kNoVote;
            if (x >= 0 && x < w && y >= 0 && y < h) {
              int gx3[3], gy3[3], gx = 0, gy = 0;
              for (int ch = 0; ch < 3; ++ch) tmatch::sobel3(&blurred[((size_t)ch * bh + r + 1) * bw + c + 1], bw, &gx3[ch], &gy3[ch]);
              const int m = tmatch::pick_channel(gx3, gy3, &gx, &gy);
              if (tmatch::is_candidate(m, weak)) q = (uint8_t)tmatch::orientation_bin(gx, gy);
              if (mag2 && r >= 1 && r <= tile_h && c >= 1 && c <= tile_w) mag2[base + (size_t)y * w + x] = m;
            }
            bins[(size_t)r * qw + c] = q;
          }
        for (int r = 0; r < tile_h && y0 + r < h; ++r)
          for (int c = 0; c < tile_w && x0 + c < w; ++c) ori[base + (size_t)(y0 + r) * w + x0 + c] = tmatch::majority(&bins[(size_t)(r + 1) * qw + c + 1], qw);
      }
  }
  return 0;
}

extern "C" int tm_emul_response(const uint8_t* ori, int n, int h, int w, int T, int tile_w, int tile_h, uint8_t* resp) {
  if (n == 0) return 0;
  if (!tmatch::response_args_ok(ori != nullptr, resp != nullptr, n, h, w, T) || tile_w < 1 || tile_h < 1) return 1;
  const int gh = tmatch::cdiv(h, T), gw = tmatch::cdiv(w, T);
  const int ew = tile_w + T - 1, eh = tile_h + T - 1;
  std::vector<uint8_t> bits((size_t)eh * ew), row_or((size_t)eh * tile_w);
  for (int img = 0; img < n; ++img) {
    const uint8_t* ori_n = ori + (size_t)img * h * w;
    uint8_t* resp_n = resp + (size_t)img * 8 * T * T * gh * gw;
    for (int y0 = 0; y0 < gh * T; y0 += tile_h)
      for (int x0 = 0; x0 < gw * T; x0 += tile_w) {
        for (int r = 0; r < eh; ++r)
          for (int c = 0; c < ew; ++c) {
            const int x = x0 + c, y = y0 + r;
            bits[(size_t)r * ew + c] = (x < w && y < h) ? ori_n[(size_t)y * w + x] : 0;
          }
        for (int r = 0; r < eh; ++r)
          for (int c = 0; c < tile_w; ++c) {
            uint32_t s = 0;
            for (int d = 0; d < T; ++d) s |= bits[(size_t)r * ew + c + d];
            row_or[(size_t)r * tile_w + c] = (uint8_t)s;
          }
        for (int r = 0; r < tile_h && y0 + r < gh * T; ++r)
          for (int c = 0; c < tile_w && x0 + c < gw * T; ++c) {
            const int x = x0 + c, y = y0 + r;
            uint32_t s = 0;
            if (x < w && y < h)
              for (int d = 0; d < T; ++d) s |= row_or[(size_t)(r + d) * tile_w + c];
            for (int o = 0; o < 8; ++o) resp_n[tmatch::resp_index(o, x, y, T, gh, gw)] = tmatch::response_of(s, o);
          }
      }
  }
  return 0;
}

extern "C" int tm_emul_match(const uint8_t* resp, int n, int h, int w, int T, const int32_t* templates, const uint8_t* features, int n_templates,
                             int n_features, int n_objects, int tile_w, int tile_h, uint8_t* best_score, uint8_t* best_f, int32_t* best_template) {
  if (n == 0) return 0;
  if (!tmatch::match_args_ok(resp != nullptr, templates != nullptr && (n_features == 0 || features != nullptr), best_score && best_f && best_template, n, h,
                         w, T, n_templates, n_features, n_objects) ||
      tile_w < 1 || tile_h < 1)
    return 1;
  if (n_templates && tmatch::first_bad_template(templates, features, n_templates, n_features, n_objects) >= 0) return 2;
  const int gh = tmatch::cdiv(h, T), gw = tmatch::cdiv(w, T);
  const size_t plane = (size_t)gh * gw;
  std::vector<tmatch::Best> best((size_t)tile_w * tile_h);
  for (int img = 0; img < n; ++img) {
    const uint8_t* resp_n = resp + (size_t)img * 8 * T * T * plane;
    for (int obj = 0; obj < n_objects; ++obj)
      for (int y0 = 0; y0 < gh; y0 += tile_h)
        for (int x0 = 0; x0 < gw; x0 += tile_w) {
          for (auto& b : best) b = tmatch::no_best();
          for (int t = 0; t < n_templates; ++t) {
            const int32_t* e = templates + (size_t)tmatch::kTemplateFields * t;
            if (e[0] != obj) continue;
            for (int r = 0; r < tile_h && y0 + r < gh; ++r)
              for (int c = 0; c < tile_w && x0 + c < gw; ++c) {
                const int gx = x0 + c, gy = y0 + r;
                if (!tmatch::placement_valid(gx, gy, T, e[3], e[4], w, h)) continue;
                const tmatch::Best cand{tmatch::score_at(resp_n, features + 4 * (size_t)e[1], e[2], gx, gy, T, gh, gw), e[2], t};
                if (tmatch::better(cand, best[(size_t)r * tile_w + c])) best[(size_t)r * tile_w + c] = cand;
              }
          }
          for (int r = 0; r < tile_h && y0 + r < gh; ++r)
            for (int c = 0; c < tile_w && x0 + c < gw; ++c) {
              const size_t out = ((size_t)img * n_objects + obj) * plane + (size_t)(y0 + r) * gw + x0 + c;
              const tmatch::Best& b = best[(size_t)r * tile_w + c];
              best_score[out] = (uint8_t)b.score;
              best_f[out] = (uint8_t)b.f;
              best_template[out] = b.t;
            }
        }
  }
  return 0;
}

// the order alone, for the pairs a test states by hand: 1 when (score_a, f_a, t_a) beats (score_b, f_b, t_b)
extern "C" int tm_emul_better(int score_a, int f_a, int t_a, int score_b, int f_b, int t_b) {
  return tmatch::better(tmatch::Best{score_a, f_a, t_a}, tmatch::Best{score_b, f_b, t_b}) ? 1 : 0;
}
