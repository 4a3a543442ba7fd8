// template_match.hip -- the training-free detector's three launches on the device: LINE-2D template matching on quantised gradient
// orientations (the colour modality of LINE-MOD, Hinterstoisser et al., PAMI 2012).
//
// The rules are template_match_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Everything is
// integer arithmetic, maxima, ORs and a total order, so neither the grid nor a tile can change a bit.  No atomics: every output byte is
// written by exactly one lane.
//
//   tm_quantize_kernel  one workgroup of 256 lanes per tile of 64 x 16 pixels of one image.
//                         1. the tile's bytes plus a halo of 4 go to LDS per channel, the entry of a coordinate outside the image holding the
//                            pixel of the clamped coordinate (the replicated border);
//                         2. with blur: the horizontal binomial of the columns within 2 of the tile (uint16), then the vertical one, rounded
//                            once, into the blurred tile (halo 2); an entry outside the image is B at the clamped coordinate;
//                         3. Sobel per channel, the winning channel, its bin when the pixel is a candidate [kNoVote otherwise and outside the
//                            image] for the tile plus a halo of 1; mag2 of the tile's own pixels is written from here;
//                         4. the 3x3 majority, one byte per pixel.
//                       LDS: 3 x 24 x 72 + 3 x 24 x 68 x 2 + 3 x 20 x 68 + 18 x 66 = 20.2 KiB.
//   tm_response_kernel  one workgroup per tile of 8 rows x (128 / T) T pixels of the PADDED domain gh T x gw T: the orientation bytes plus a
//                       halo of T - 1 to the right and below go to LDS (0 outside the image), the OR over the window rows first, then
//                       columns; the lanes then walk (row, phase, cell), so the lanes of one phase write consecutive bytes of a map.
//   tm_match_kernel     one workgroup of 16 waves per (tile of 32 x 2 locations, object, image).  A lane owns one location; the sixteen waves
//                       own the same 64 locations and every sixteenth template each (a 480 x 640 image at T = 8 has 75 tiles: the split
//                       over waves is what fills the chip).  A template's header and feature words are the same for every lane (scalar
//                       loads); per feature a lane reads one byte of the linearised maps, which for the lanes of a location row are
//                       consecutive bytes, eight loads in flight.  The running best stays in registers; the waves' bests are merged
//                       through LDS under the contract's total order [better], which makes the split invisible.
#include "common.h"
#include "template_match_core.h"

namespace mp {

__global__ __launch_bounds__(256) void tm_quantize_kernel(const uint8_t* __restrict__ images, int h, int w, int tiles_x, int tiles_y, int blur,
                                                          int weak, uint8_t* __restrict__ ori, int32_t* __restrict__ mag2) {
  constexpr int TW = tmatch::kQuantTileW, TH = tmatch::kQuantTileH;
  constexpr int rw = TW + 2 * tmatch::kRawHalo, rh = TH + 2 * tmatch::kRawHalo;       // raw:      72 x 24
  constexpr int bw = TW + 2 * tmatch::kBlurHalo, bh = TH + 2 * tmatch::kBlurHalo;     // blurred:  68 x 20
  constexpr int qw = TW + 2, qh = TH + 2;                                     // bins:     66 x 18
  __shared__ uint8_t raw[3 * rh * rw];
  __shared__ uint16_t hsum[3 * rh * bw];
  __shared__ uint8_t blurred[3 * bh * bw];
  __shared__ uint8_t bins[qh * qw];
  const int tid = threadIdx.x;
  const int per_image = tiles_x * tiles_y;
  const int img = blockIdx.x / per_image, rest = blockIdx.x - img * per_image;
  const int ty = rest / tiles_x, tx = rest - ty * tiles_x;
  const int x0 = tx * TW, y0 = ty * TH;
  const size_t base = (size_t)img * h * w;   // pixels before this image

  // 1. raw[c][r][col] = the image at the clamped (x0 - 4 + col, y0 - 4 + r)
  for (int t = tid; t < rh * rw; t += tmatch::kBlock) {
    const int r = t / rw, c = t - r * rw;
    const int x = tmatch::clampi(x0 - tmatch::kRawHalo + c, 0, w - 1), y = tmatch::clampi(y0 - tmatch::kRawHalo + r, 0, h - 1);
    const uint8_t* p = images + 3 * (base + (size_t)y * w + x);
    raw[t] = p[0];
    raw[rh * rw + t] = p[1];
    raw[2 * rh * rw + t] = p[2];
  }
  __syncthreads();
  if (blur) {
    // 2a. hsum[c][r][col]: the horizontal pass at raw row r, around the clamped x of blurred column col
    for (int t = tid; t < 3 * rh * bw; t += tmatch::kBlock) {
      const int ch = t / (rh * bw), rem = t - ch * (rh * bw);
      const int r = rem / bw, c = rem - r * bw;
      const int cx = tmatch::clampi(x0 - tmatch::kBlurHalo + c, 0, w - 1);
      hsum[t] = (uint16_t)tmatch::blur_row(&raw[(ch * rh + r) * rw + (cx - x0 + tmatch::kRawHalo)], 1);
    }
    __syncthreads();
  }
  // 2b. blurred[c][r][col] = B at the clamped (x0 - 2 + col, y0 - 2 + r)
  for (int t = tid; t < 3 * bh * bw; t += tmatch::kBlock) {
    const int ch = t / (bh * bw), rem = t - ch * (bh * bw);
    const int r = rem / bw, c = rem - r * bw;
    const int cy = tmatch::clampi(y0 - tmatch::kBlurHalo + r, 0, h - 1);
    if (blur) {
      blurred[t] = (uint8_t)tmatch::blur_round(tmatch::blur_row(&hsum[(ch * rh + (cy - y0 + tmatch::kRawHalo)) * bw + c], bw));
    } else {
      const int cx = tmatch::clampi(x0 - tmatch::kBlurHalo + c, 0, w - 1);
      blurred[t] = raw[(ch * rh + (cy - y0 + tmatch::kRawHalo)) * rw + (cx - x0 + tmatch::kRawHalo)];
    }
  }
  __syncthreads();
  // 3. bins[r][col] of (x0 - 1 + col, y0 - 1 + r)
  for (int t = tid; t < qh * qw; t += tmatch::kBlock) {
    const int r = t / qw, c = t - r * qw;
    const int x = x0 - 1 + c, y = y0 - 1 + r;
    uint8_t q = tmatch::kNoVote;
    if (x >= 0 && x < w && y >= 0 && y < h) {
      int gx3[3], gy3[3], gx, gy;
      for (int ch = 0; ch < 3; ++ch) tmatch::sobel3(&blurred[(ch * bh + r + 1) * bw + c + 1], bw, &gx3[ch], &gy3[ch]);
      const int m = tmatch::pick_channel(gx3, gy3, &gx, &gy);
      if (tmatch::is_candidate(m, weak)) q = (uint8_t)tmatch::orientation_bin(gx, gy);
      if (mag2 && r >= 1 && r <= TH && c >= 1 && c <= TW) mag2[base + (size_t)y * w + x] = m;
    }
    bins[t] = q;
  }
  __syncthreads();
  // 4. the majority of the tile's own pixels
  for (int t = tid; t < TH * TW; t += tmatch::kBlock) {
    const int r = t / TW, c = t - r * TW;
    const int x = x0 + c, y = y0 + r;
    if (x < w && y < h) ori[base + (size_t)y * w + x] = tmatch::majority(&bins[(r + 1) * qw + c + 1], qw);
  }
}

__global__ __launch_bounds__(256) void tm_response_kernel(const uint8_t* __restrict__ ori, int h, int w, int T, int gh, int gw, int tiles_x,
                                                          int tiles_y, uint8_t* __restrict__ resp) {
  constexpr int TH = tmatch::kRespTileH, halo = tmatch::kMaxT - 1;
  constexpr int lw = 128 + halo, lh = TH + halo;
  __shared__ uint8_t bits[lh * lw];
  __shared__ uint8_t row_or[lh * 128];
  const int tid = threadIdx.x;
  const int TW = tmatch::resp_tile_w(T), cells = TW / T;
  const int per_image = tiles_x * tiles_y;
  const int img = blockIdx.x / per_image, rest = blockIdx.x - img * per_image;
  const int ty = rest / tiles_x, tx = rest - ty * tiles_x;
  const int x0 = tx * TW, y0 = ty * TH;
  const uint8_t* ori_n = ori + (size_t)img * h * w;
  uint8_t* resp_n = resp + (size_t)img * 8 * T * T * gh * gw;
  const int ew = TW + T - 1, eh = TH + T - 1;
  for (int t = tid; t < eh * ew; t += tmatch::kBlock) {
    const int r = t / ew, c = t - r * ew;
    const int x = x0 + c, y = y0 + r;
    bits[r * lw + c] = (x < w && y < h) ? ori_n[(size_t)y * w + x] : 0;
  }
  __syncthreads();
  for (int t = tid; t < eh * TW; t += tmatch::kBlock) {
    const int r = t / TW, c = t - r * TW;
    uint32_t s = 0;
    for (int d = 0; d < T; ++d) s |= bits[r * lw + c + d];
    row_or[r * 128 + c] = (uint8_t)s;
  }
  __syncthreads();
  // (row, phase, cell): consecutive lanes write consecutive cells of one phase
  for (int t = tid; t < TH * TW; t += tmatch::kBlock) {
    const int r = t / TW, rem = t - r * TW;
    const int px = rem / cells, j = rem - px * cells;
    const int c = j * T + px;
    const int x = x0 + c, y = y0 + r;
    if (x >= gw * T || y >= gh * T) continue;
    uint32_t s = 0;
    if (x < w && y < h)
      for (int d = 0; d < T; ++d) s |= row_or[(r + d) * 128 + c];
#pragma unroll
    for (int o = 0; o < 8; ++o) resp_n[tmatch::resp_index(o, x, y, T, gh, gw)] = tmatch::response_of(s, o);
  }
}

// v / T and v mod T for v in 0 .. 255 and T in 1 .. 8 by one multiplication: recip = ceil(65536 / T) is exact there (v (recip T - 65536) < 65536)
__device__ __forceinline__ void divmod_small(int v, int T, int recip, int* q, int* m) {
  *q = (v * recip) >> 16;
  *m = v - *q * T;
}

// feature i of the table as one word (dx | dy << 8 | index << 16); bytes when the table is not dword aligned
template <bool kAligned>
__device__ __forceinline__ uint32_t feature_word(const uint8_t* __restrict__ features, size_t i) {
  const uint8_t* fp = features + 4 * i;
  if (kAligned) return *(const uint32_t*)fp;
  return (uint32_t)fp[0] | ((uint32_t)fp[1] << 8) | ((uint32_t)fp[2] << 16);
}

// the byte of a feature within the maps of an image, for the location at offset 0: phase (dy mod T, dx mod T), cell (dy div T, dx div T).
// The maps of one image have fewer than 2^31 bytes [resp_sizes_ok]: 32 bits hold every offset.
__device__ __forceinline__ uint32_t feature_cell(uint32_t word, int T, int recip, uint32_t plane, int gw) {
  int qx, mx, qy, my;
  divmod_small((int)(word & 255u), T, recip, &qx, &mx);
  divmod_small((int)((word >> 8) & 255u), T, recip, &qy, &my);
  const int o = (int)((word >> 16) & 255u);
  return (uint32_t)((o * T + my) * T + mx) * plane + (uint32_t)(qy * gw + qx);
}

template <bool kAligned>
__global__ __launch_bounds__(tmatch::kMatchWaves * 64) void tm_match_kernel(const uint8_t* __restrict__ resp, int h, int w, int T, int gh, int gw,
                                                                            int tiles_x, const int32_t* __restrict__ templates,
                                                                            const uint8_t* __restrict__ features, int n_templates, int n_objects,
                                                                            uint8_t* __restrict__ best_score, uint8_t* __restrict__ best_f,
                                                                            int32_t* __restrict__ best_template) {
  constexpr int per_wave = tmatch::kLocW * tmatch::kLocH;   // 64
  constexpr int kBatch = 8;                                 // byte loads in flight per lane
  __shared__ int32_t merge[(tmatch::kMatchWaves - 1) * per_wave * 2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // the same for the wave: the table is read with scalar loads
  const int tyi = blockIdx.x / tiles_x, txi = blockIdx.x - tyi * tiles_x;
  const int obj = blockIdx.y, img = blockIdx.z;
  const int gx = txi * tmatch::kLocW + (lane & (tmatch::kLocW - 1)), gy = tyi * tmatch::kLocH + lane / tmatch::kLocW;
  const bool live = gx < gw && gy < gh;
  const uint32_t plane = (uint32_t)gh * gw;
  const uint8_t* resp_n = resp + (size_t)img * 8 * T * T * plane;
  const uint32_t at = live ? (uint32_t)(gy * gw + gx) : 0;
  const int recip = (65536 + T - 1) / T;
  tmatch::Best best = tmatch::no_best();
  for (int t = wave; t < n_templates; t += tmatch::kMatchWaves) {
    const int32_t* e = templates + (size_t)tmatch::kTemplateFields * t;   // the same for every lane
    if (e[0] != obj) continue;
    const size_t first = (size_t)e[1];
    const int f = e[2];
    const bool ok = live && tmatch::placement_valid(gx, gy, T, e[3], e[4], w, h);
    if (!__any(ok)) continue;   // no lane of the wave can place it
    // Every lane walks the features (their words are uniform).  A lane whose placement is valid reads gx T + dx < w and gy T + dy < h, a cell
    // inside the maps; any other lane reads byte 0 of the maps and drops the sum: no branch in the loop, kBatch loads in flight.
    const uint32_t keep = ok ? ~0u : 0u;
    int score = 0, i = 0;
    for (; i + kBatch <= f; i += kBatch) {
      uint32_t v[kBatch];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) v[j] = resp_n[(feature_cell(feature_word<kAligned>(features, first + i + j), T, recip, plane, gw) + at) & keep];
#pragma unroll
      for (int j = 0; j < kBatch; ++j) score += (int)v[j];
    }
    for (; i < f; ++i) score += resp_n[(feature_cell(feature_word<kAligned>(features, first + i), T, recip, plane, gw) + at) & keep];
    const tmatch::Best cand{score, f, t};
    if (ok && tmatch::better(cand, best)) best = cand;
  }
  if (wave > 0) {
    int32_t* m = merge + ((wave - 1) * per_wave + lane) * 2;
    m[0] = best.score | (best.f << 8);
    m[1] = best.t;
  }
  __syncthreads();
  if (wave > 0 || !live) return;
  for (int v = 0; v < tmatch::kMatchWaves - 1; ++v) {
    const int32_t* m = merge + (v * per_wave + lane) * 2;
    const tmatch::Best other{m[0] & 255, (m[0] >> 8) & 255, m[1]};
    if (tmatch::better(other, best)) best = other;
  }
  const size_t out = ((size_t)img * n_objects + obj) * plane + at;
  best_score[out] = (uint8_t)best.score;
  best_f[out] = (uint8_t)best.f;
  best_template[out] = best.t;
}

}  // namespace mp

using namespace mp;

extern "C" int mp_tm_quantize(const uint8_t* d_images, int n, int h, int w, int blur, int weak_threshold, uint8_t* d_ori, int32_t* d_mag2,
                              mp_stream stream) {
  if (n == 0) return MP_OK;
  MP_REQUIRE(tmatch::quantize_args_ok(d_images != nullptr, d_ori != nullptr, n, h, w, weak_threshold),
             "mp_tm_quantize: needs images and ori; n %d >= 0, h %d and w %d in 1 .. %d, n * h * w * 3 < 2^31, weak_threshold %d in 0 .. %d", n, h, w,
             tmatch::kMaxSide, weak_threshold, tmatch::kMaxWeak);
  const int tiles_x = ceil_div(w, tmatch::kQuantTileW), tiles_y = ceil_div(h, tmatch::kQuantTileH);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tm_quantize", 0.0, (double)n * h * w * (3.0 + 1.0 + (d_mag2 ? 4.0 : 0.0)), s);
  hipLaunchKernelGGL(tm_quantize_kernel, dim3((unsigned)((long long)n * tiles_x * tiles_y)), dim3(tmatch::kBlock), 0, s, d_images, h, w, tiles_x, tiles_y,
                     blur != 0, weak_threshold, d_ori, d_mag2);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_tm_response(const uint8_t* d_ori, int n, int h, int w, int T, uint8_t* d_resp, mp_stream stream) {
  if (n == 0) return MP_OK;
  MP_REQUIRE(tmatch::response_args_ok(d_ori != nullptr, d_resp != nullptr, n, h, w, T),
             "mp_tm_response: needs ori and resp; n %d >= 0, h %d and w %d in 1 .. %d, T %d in 1 .. %d, n * 8 * T * T * gh * gw < 2^31", n, h, w,
             tmatch::kMaxSide, T, tmatch::kMaxT);
  const int gh = tmatch::cdiv(h, T), gw = tmatch::cdiv(w, T);
  const int tiles_x = ceil_div(gw * T, tmatch::resp_tile_w(T)), tiles_y = ceil_div(gh * T, tmatch::kRespTileH);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tm_response", 0.0, (double)n * ((double)h * w + 8.0 * T * T * gh * gw), s);
  hipLaunchKernelGGL(tm_response_kernel, dim3((unsigned)((long long)n * tiles_x * tiles_y)), dim3(tmatch::kBlock), 0, s, d_ori, h, w, T, gh, gw, tiles_x,
                     tiles_y, d_resp);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_tm_match(const uint8_t* d_resp, int n, int h, int w, int T, const int32_t* d_templates, const int32_t* h_templates,
                           const uint8_t* d_features, const uint8_t* h_features, int n_templates, int n_features, int n_objects,
                           uint8_t* d_best_score, uint8_t* d_best_f, int32_t* d_best_template, mp_stream stream) {
  if (n == 0) return MP_OK;
  MP_REQUIRE(tmatch::match_args_ok(d_resp != nullptr, d_templates != nullptr && h_templates != nullptr && (n_features == 0 || (d_features && h_features)),
                               d_best_score && d_best_f && d_best_template, n, h, w, T, n_templates, n_features, n_objects),
             "mp_tm_match: null pointer, or n %d < 0, h %d or w %d outside 1 .. %d, T %d outside 1 .. %d, n_templates %d outside 0 .. %d, n_features %d "
             "outside 0 .. %d, n_objects %d outside 1 .. %d, or maps or outputs of 2^31 bytes or more",
             n, h, w, tmatch::kMaxSide, T, tmatch::kMaxT, n_templates, tmatch::kMaxTemplates, n_features, tmatch::kMaxTableFeatures, n_objects, tmatch::kMaxObjects);
  const int bad = n_templates ? tmatch::first_bad_template(h_templates, h_features, n_templates, n_features, n_objects) : -1;
  MP_REQUIRE(bad < 0, "mp_tm_match: template %d: object outside 0 .. %d, n_features outside 1 .. %d, a box side outside 1 .. %d, features outside the "
             "table, or a feature outside the box or with an orientation index above 7", bad, n_objects - 1, tmatch::kMaxFeatures, tmatch::kMaxBox);
  const int gh = tmatch::cdiv(h, T), gw = tmatch::cdiv(w, T);
  const int tiles_x = ceil_div(gw, tmatch::kLocW), tiles_y = ceil_div(gh, tmatch::kLocH);
  MP_REQUIRE(n <= 65535, "mp_tm_match: n %d above 65535 images in one call", n);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tm_match", 0.0, (double)n * 8.0 * T * T * gh * gw + (double)n * n_objects * gh * gw * 6.0, s);
  const auto kernel = ((uintptr_t)d_features & 3) == 0 ? tm_match_kernel<true> : tm_match_kernel<false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_x * tiles_y), (unsigned)n_objects, (unsigned)n), dim3(tmatch::kMatchWaves * 64), 0, s, d_resp, h, w, T,
                     gh, gw, tiles_x, d_templates, d_features, n_templates, n_objects, d_best_score, d_best_f, d_best_template);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
