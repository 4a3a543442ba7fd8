// template_match_core.h -- the rules of the training-free detector (LINE-2D: template matching on quantised gradient orientations, the
// colour modality of LINE-MOD, Hinterstoisser et al., PAMI 2012) that runs on the device (template_match.hip), shared with the host
// emulation (tests/template_match_emul.cpp) the way overlay_core.h is shared with its own.
//
// CONTRACT (mp_tm_quantize): image -> one orientation bit per pixel
//   * INPUT.  n images uint8 [n,h,w,3].
//   * BLUR (optional).  Per channel the separable binomial (1 4 6 4 1) / 16 in both directions with the border REPLICATED: the tap of a
//     coordinate outside the image is the pixel of the clamped coordinate.  Integers; rounded to nearest ONCE after both passes:
//     B = (sum of the 25 weighted taps + 128) >> 8 [blur_row, blur_round].  Without blur B is the image.
//   * GRADIENT.  gx, gy = the 3x3 Sobel responses of B per channel, the border of B replicated [sobel3]; |g| <= 1020.  The channel with the
//     largest gx^2 + gy^2 wins, the lowest channel on a tie [pick_channel]; mag2 = that sum (<= 2,080,800).
//   * BIN.  The angle of (gx, gy) modulo 180 degrees falls into one of eight half-open bins [k 22.5, (k + 1) 22.5) [orientation_bin].
//     Integer comparisons only: with (gx, gy) negated when gy < 0 or (gy == 0 and gx < 0), a = |gx|, b = gy >= 0,
//         gx > 0:   b < tan(22.5) a -> 0,  b < a -> 1,  b < tan(67.5) a -> 2,  else 3          gx == 0 -> 4
//         gx < 0:   b <= tan(22.5) a -> 7, b <= a -> 6, b <= tan(67.5) a -> 5, else 4
//     where b < (sqrt2 - 1) a  <=>  (b + a)^2 < 2 a^2  and, for b >= a,  b < (sqrt2 + 1) a  <=>  (b - a)^2 < 2 a^2; neither irrational
//     boundary is ever met by integers, so < and <= agree there.  Everything fits 32 bits.
//   * CANDIDATE.  A pixel whose mag2 >= weak_threshold^2 and mag2 > 0 [is_candidate].
//   * MAJORITY.  A pixel keeps bit o when at least 5 of the 9 pixels of its 3x3 neighbourhood are candidates quantised to o; a neighbour
//     outside the image does not vote [majority].  At most one bit can.
//   * OUTPUTS.  ori uint8 [n,h,w] (0 or one bit set); mag2 int32 [n,h,w] of the pixel itself (optional: NULL is not written).
//
// CONTRACT (mp_tm_response): orientation bits -> linearised response maps
//   * s(x, y) = the OR of ori over [x, x + T) x [y, y + T) clipped to the image, T in 1 .. 8 (rows first, then columns; an OR does not
//     depend on that order).
//   * r_o(x, y) = 4 when bit o is set in s(x, y), else 1 when bit o - 1 or o + 1 (circular over eight) is, else 0 [response_of].
//   * resp uint8 [n][8][T][T][gh][gw], gh = ceil(h / T), gw = ceil(w / T): r_o(x, y) sits at [n][o][y mod T][x mod T][y div T][x div T]
//     [resp_index]; a cell beyond the image holds 0.  Every byte of resp is written.
//
// CONTRACT (mp_tm_match): every template at every grid location
//   * TABLE.  templates int32 [n_templates,5] = (object, first feature, n_features f, width, height); features uint8 [n_features,4] =
//     (dx, dy, orientation index, 0).  0 <= object < n_objects, 1 <= f <= 63, 1 <= width, height <= 256, first + f <= n_features,
//     dx < width, dy < height, index < 8 [template_ok, feature_ok]: checked on the HOST copy of the table before anything is launched.
//   * Template t at grid location (gx, gy) has its top-left corner at pixel (gx T, gy T); the placement is VALID when gx T + width <= w and
//     gy T + height <= h.  score = the sum over its features of r_o(gx T + dx, gy T + dy): one byte per feature, at cell
//     (gy + dy div T, gx + dx div T) of phase (dy mod T, dx mod T), contiguous over consecutive gx.
//   * Per (image, object, location) the best valid template: a beats b when score_a f_b > score_b f_a (the exact ratio score / (4 f) by
//     cross-multiplication), or on equality when its index is lower [better].  This is a total order: the result does not depend on the
//     order in which templates are visited or partial results merged.
//   * OUTPUTS [n, n_objects, gh, gw]: best_score uint8 (<= 252 = 63 x 4), best_f uint8, best_template int32; a location without a valid
//     template gets 0, 0 and -1.
//   * Integers throughout, no atomics, every output byte written by one thread; no result depends on tile, grid or block size.
//   * LIMITS [sizes_ok].  h, w in 1 .. 8192, n * h * w * 3 < 2^31, n * 8 * T * T * gh * gw < 2^31, n * n_objects * gh * gw < 2^31,
//     weak_threshold in 0 .. 1443, n_objects in 1 .. 65535, n_templates in 0 .. 2^20, n_features in 0 .. 2^26.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TM_HD __host__ __device__ __forceinline__
#else
#define TM_HD inline
#endif

namespace mp {
namespace tmatch {

constexpr int kMaxSide = 8192;           // h, w
constexpr int kMaxT = 8;                 // T
constexpr int kMaxWeak = 1443;           // weak_threshold: 1443^2 is above every mag2
constexpr int kMaxFeatures = 63;         // f: 63 x 4 = 252 fits a byte
constexpr int kMaxBox = 256;             // width, height of a template
constexpr int kMaxObjects = 65535;
constexpr int kMaxTemplates = 1 << 20;
constexpr int kMaxTableFeatures = 1 << 26;
constexpr int kBlock = 256;
constexpr int kQuantTileW = 64;          // the quantise kernel's tile: 64 x 16 pixels
constexpr int kQuantTileH = 16;
constexpr int kRespTileH = 8;            // the response kernel's tile: 8 rows of resp_tile_w(T) pixels
constexpr int kLocW = 32;                // the match kernel's location tile: 32 x 2 locations per wave, kMatchWaves waves share the templates
constexpr int kLocH = 2;
constexpr int kMatchWaves = 16;
constexpr int kBlurHalo = 2, kRawHalo = 4;   // halo of the blurred tile (Sobel of the majority's neighbours) and of the raw one (+ the blur)

TM_HD int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
TM_HD int cdiv(int a, int b) { return (a + b - 1) / b; }
TM_HD int resp_tile_w(int T) { return (128 / T) * T; }   // a multiple of T: the lanes of a phase write consecutive cells

TM_HD bool sizes_ok(int n, int h, int w) {
  return n >= 0 && h >= 1 && h <= kMaxSide && w >= 1 && w <= kMaxSide && (long long)n * h * w * 3 < 2147483648LL;
}
TM_HD bool resp_sizes_ok(int n, int h, int w, int T) {
  return sizes_ok(n, h, w) && T >= 1 && T <= kMaxT && (long long)n * 8 * T * T * cdiv(h, T) * cdiv(w, T) < 2147483648LL;
}
TM_HD bool quantize_args_ok(bool has_images, bool has_ori, int n, int h, int w, int weak) {
  return sizes_ok(n, h, w) && has_images && has_ori && weak >= 0 && weak <= kMaxWeak;
}
TM_HD bool response_args_ok(bool has_ori, bool has_resp, int n, int h, int w, int T) { return resp_sizes_ok(n, h, w, T) && has_ori && has_resp; }
TM_HD bool match_args_ok(bool has_resp, bool has_tables, bool has_out, int n, int h, int w, int T, int n_templates, int n_features, int n_objects) {
  return resp_sizes_ok(n, h, w, T) && has_resp && has_out && n_templates >= 0 && n_templates <= kMaxTemplates && n_features >= 0 &&
         n_features <= kMaxTableFeatures && (n_templates == 0 || has_tables) && n_objects >= 1 && n_objects <= kMaxObjects &&
         (long long)n * n_objects * cdiv(h, T) * cdiv(w, T) < 2147483648LL;
}

// ---- quantise ---------------------------------------------------------------------------------------------------------------------------
// one direction of the binomial: p[-2 s] .. p[2 s] are the five taps
template <typename V>
TM_HD int blur_row(const V* p, int s) { return (int)p[-2 * s] + 4 * (int)p[-s] + 6 * (int)p[0] + 4 * (int)p[s] + (int)p[2 * s]; }
TM_HD int blur_round(int sum_of_25) { return (sum_of_25 + 128) >> 8; }

// B points at the tile entry of a pixel; B[dy * stride + dx] is the blurred value at the CLAMPED coordinate (x + dx, y + dy)
TM_HD void sobel3(const uint8_t* B, int stride, int* gx, int* gy) {
  const int a = B[-stride - 1], b = B[-stride], c = B[-stride + 1];
  const int d = B[-1], f = B[1];
  const int g = B[stride - 1], hh = B[stride], i = B[stride + 1];
  *gx = (c + 2 * f + i) - (a + 2 * d + g);
  *gy = (g + 2 * hh + i) - (a + 2 * b + c);
}

// the three channels' gradients -> the winner's; returns its mag2
TM_HD int pick_channel(const int* gx3, const int* gy3, int* gx, int* gy) {
  int best = -1;
  for (int c = 0; c < 3; ++c) {
    const int m = gx3[c] * gx3[c] + gy3[c] * gy3[c];
    if (m > best) {
      best = m;
      *gx = gx3[c];
      *gy = gy3[c];
    }
  }
  return best;
}

TM_HD int orientation_bin(int gx, int gy) {
  if (gy < 0 || (gy == 0 && gx < 0)) {
    gx = -gx;
    gy = -gy;
  }
  const int a = gx < 0 ? -gx : gx, b = gy;
  if (gx == 0) return 4;
  const bool below_22 = (b + a) * (b + a) < 2 * a * a;                  // b < tan(22.5) a
  const bool below_67 = b < a || (b - a) * (b - a) < 2 * a * a;         // b < tan(67.5) a
  if (gx > 0) return below_22 ? 0 : (b < a ? 1 : (below_67 ? 2 : 3));
  return below_22 ? 7 : (b <= a ? 6 : (below_67 ? 5 : 4));
}

TM_HD bool is_candidate(int mag2, int weak) { return mag2 > 0 && mag2 >= weak * weak; }

constexpr uint8_t kNoVote = 0xFF;   // the quantised label of a pixel that is no candidate, or outside the image

// Q points at the tile entry of a pixel: Q[dy * stride + dx] is the bin 0 .. 7 of a candidate, else kNoVote -> the orientation byte
TM_HD uint8_t majority(const uint8_t* Q, int stride) {
  uint32_t count = 0;   // eight 4-bit counters, each at most 9
  for (int dy = -1; dy <= 1; ++dy)
    for (int dx = -1; dx <= 1; ++dx) {
      const uint8_t q = Q[dy * stride + dx];
      if (q != kNoVote) count += 1u << (4 * q);
    }
  for (int o = 0; o < 8; ++o)
    if (((count >> (4 * o)) & 15u) >= 5u) return (uint8_t)(1u << o);
  return 0;
}

// ---- response ---------------------------------------------------------------------------------------------------------------------------
TM_HD uint8_t response_of(uint32_t s, int o) {
  if (s & (1u << o)) return 4;
  return (s & ((1u << ((o + 1) & 7)) | (1u << ((o + 7) & 7)))) ? 1 : 0;
}

// the byte of r_o(x, y) within one image's maps
TM_HD size_t resp_index(int o, int x, int y, int T, int gh, int gw) {
  return ((((size_t)o * T + (size_t)(y % T)) * T + (size_t)(x % T)) * gh + (size_t)(y / T)) * gw + (size_t)(x / T);
}

// ---- match ------------------------------------------------------------------------------------------------------------------------------
constexpr int kTemplateFields = 5;   // object, first feature, f, width, height

TM_HD bool template_ok(const int32_t* t, int n_features, int n_objects) {
  return t[0] >= 0 && t[0] < n_objects && t[2] >= 1 && t[2] <= kMaxFeatures && t[1] >= 0 && t[1] <= n_features - t[2] && t[3] >= 1 && t[3] <= kMaxBox &&
         t[4] >= 1 && t[4] <= kMaxBox;
}
TM_HD bool feature_ok(const uint8_t* f, int width, int height) { return f[0] < width && f[1] < height && f[2] < 8; }

// the whole table, on the host: the index of the first bad template, or -1
inline int first_bad_template(const int32_t* templates, const uint8_t* features, int n_templates, int n_features, int n_objects) {
  for (int t = 0; t < n_templates; ++t) {
    const int32_t* e = templates + (size_t)kTemplateFields * t;
    if (!template_ok(e, n_features, n_objects)) return t;
    for (int i = 0; i < e[2]; ++i)
      if (!feature_ok(features + 4 * ((size_t)e[1] + i), e[3], e[4])) return t;
  }
  return -1;
}

TM_HD bool placement_valid(int gx, int gy, int T, int width, int height, int w, int h) { return gx * T + width <= w && gy * T + height <= h; }

// the running best of a location
struct Best {
  int score, f, t;   // t < 0: none yet
};
TM_HD Best no_best() { return Best{0, 0, -1}; }
// does a beat b?  Either may be "none"
TM_HD bool better(const Best& a, const Best& b) {
  if (a.t < 0) return false;
  if (b.t < 0) return true;
  const int l = a.score * b.f, r = b.score * a.f;
  return l > r || (l == r && a.t < b.t);
}

// the score of one template at one valid placement; resp_n = the maps of the image, feat = the template's first feature
TM_HD int score_at(const uint8_t* resp_n, const uint8_t* feat, int f, int gx, int gy, int T, int gh, int gw) {
  int score = 0;
  for (int i = 0; i < f; ++i) score += resp_n[resp_index(feat[4 * i + 2], gx * T + feat[4 * i], gy * T + feat[4 * i + 1], T, gh, gw)];
  return score;
}

}  // namespace tmatch
}  // namespace mp
