// TEST SUPPORT: host emulation of the camera-tracking kernels (megapose6d_amd/csrc/tsdf_track.hip), built from the same rules header
// (tsdf_track_core.h).  Same arguments as the C ABI, on host arrays, as plain loops: frames, iterations, groups, the 256 lanes of a group
// with their four pixels each, the wave butterfly as an array of 64 sums, the waves and the groups in ascending order.  Compiled with
// -ffp-contract=off, so the kernels are held to these results bit for bit.  Built by tests/support/tsdf_track.py;
// tests/tsdf_track_asan_main.cpp includes this file.
#include <cstdint>
#include <cstring>
#include <vector>

#include "tsdf_track_core.h"

using namespace mp;

namespace {

// the record of group G of one frame under the loaded view
void group_record(const tsdf::TrackVolume& vol, const float* depth, const uint8_t* mask, const float* view, int h, int w, float mu, int min_views, int G,
                  double* record) {
  const long long hw = (long long)h * w;
  double wave_sum[4][tsdf::kTrackSums];
  for (int wave = 0; wave < 4; ++wave) {
    double lanes[64][tsdf::kTrackSums];
    for (int lane = 0; lane < 64; ++lane) {
      const int t = wave * 64 + lane;
      tsdf::TrackSums acc = tsdf::track_zero();
      for (int q = 0; q < tsdf::kTrackPixelsPerLane; ++q) {
        const long long pix = (long long)G * tsdf::kTrackGroupPixels + (long long)q * tsdf::kTrackBlock + t;
        if (pix >= hw) continue;
        if (mask && mask[pix] == 0) continue;
        float row[tsdf::kTrackRowFloats];
        if (tsdf::track_row((int)(pix % w), (int)(pix / w), depth[pix], view, vol, mu, min_views, row)) acc = tsdf::track_add(acc, row);
      }
      for (int k = 0; k < tsdf::kTrackSums; ++k) lanes[lane][k] = acc.s[k];
    }
    for (int off = 32; off > 0; off >>= 1) {
      double next[64][tsdf::kTrackSums];
      for (int lane = 0; lane < 64; ++lane)
        for (int k = 0; k < tsdf::kTrackSums; ++k) next[lane][k] = lanes[lane][k] + lanes[lane ^ off][k];
      std::memcpy(lanes, next, sizeof(lanes));
    }
    for (int k = 0; k < tsdf::kTrackSums; ++k) wave_sum[wave][k] = lanes[0][k];
  }
  for (int k = 0; k < tsdf::kTrackRecord; ++k) {
    double s = 0.0;
    if (k < tsdf::kTrackSums)
      for (int wave = 0; wave < 4; ++wave) s = s + wave_sum[wave][k];
    record[k] = s;
  }
}

bool track_args_ok(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float mu, int min_views, int min_pixels, int iters,
                   float eps_rot, float eps_trans) {
  const float origin[3] = {ox, oy, oz};
  return tsdf::dims_ok(nx, ny, nz) && tsdf::grid_ok(origin, voxel) && tsdf::track_params_ok(mu, min_views, min_pixels, iters, eps_rot, eps_trans);
}

}  // namespace

extern "C" int tsdf_track_groups_emul(int h, int w) { return tsdf::track_groups(h, w); }

extern "C" int tsdf_track_emul(const void* volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel, const float* depth,
                               const uint8_t* masks, const float* K, const float* TCO_in, int n, int h, int w, float mu, int min_views,
                               int min_pixels, int iters, float eps_rot, float eps_trans, float* TCO_out, int32_t* status, int32_t* used, float* rms,
                               double* partials, long long partials_capacity) {
  (void)color;
  if (!track_args_ok(nx, ny, nz, ox, oy, oz, voxel, mu, min_views, min_pixels, iters, eps_rot, eps_trans)) return 1;
  if (n < 0 || n > tsdf::kTrackMaxFrames) return 1;
  if (n == 0) return 0;
  const int groups = tsdf::track_groups(h, w);
  if (groups == 0 || !volume || !depth || !K || !TCO_in || !TCO_out || !status || !used || !rms || !partials) return 1;
  if (TCO_in == TCO_out || partials_capacity < (long long)n * groups) return 1;
  const tsdf::TrackVolume vol = tsdf::volume_of<const float, const int32_t>(volume, nx, ny, nz, 0, ox, oy, oz, voxel);
  const size_t hw = (size_t)h * w;
  for (int v = 0; v < n; ++v) {
    const float* Tin = TCO_in + (size_t)v * 16;
    float* T = TCO_out + (size_t)v * 16;
    float view[tsdf::kViewFloats];
    const bool ok = tsdf::load_view(K + (size_t)v * 9, Tin, view);
    std::memcpy(T, Tin, 16 * sizeof(float));
    status[v] = ok ? tsdf::kTrackRan : tsdf::kTrackBadView;
    used[v] = 0;
    rms[v] = 0.f;
    double* records = partials + (size_t)v * groups * tsdf::kTrackRecord;
    for (int it = 0; it < iters && status[v] == tsdf::kTrackRan; ++it) {
      tsdf::load_view(K + (size_t)v * 9, T, view);
      for (int G = 0; G < groups; ++G)
        group_record(vol, depth + v * hw, masks ? masks + v * hw : nullptr, view, h, w, mu, min_views, G, records + (size_t)G * tsdf::kTrackRecord);
      double S[tsdf::kTrackRecord];
      for (int k = 0; k < tsdf::kTrackRecord; ++k) {
        double s = 0.0;
        for (int G = 0; G < groups; ++G) s = s + records[(size_t)G * tsdf::kTrackRecord + k];
        S[k] = s;
      }
      float out[12];
      const int st = tsdf::track_solve(S, T, min_pixels, eps_rot, eps_trans, out, &used[v], &rms[v]);
      if (st == tsdf::kTrackLost)
        std::memcpy(T, Tin, 16 * sizeof(float));
      else
        std::memcpy(T, out, 12 * sizeof(float));
      status[v] = st;
    }
  }
  return 0;
}

// the per-pixel terms of one frame under (K, TCO): used_out [h*w] 0 / 1, rows [h*w, kTrackRowFloats] (written for the used pixels only)
extern "C" int tsdf_track_rows_emul(const void* volume, int nx, int ny, int nz, float ox, float oy, float oz, float voxel, const float* depth,
                                    const uint8_t* mask, const float* K, const float* TCO, int h, int w, float mu, int min_views, uint8_t* used_out,
                                    float* rows) {
  if (!track_args_ok(nx, ny, nz, ox, oy, oz, voxel, mu, min_views, 1, 1, 0.f, 0.f) || !tsdf::frame_ok(h, w)) return 1;
  if (!volume || !depth || !K || !TCO || !used_out || !rows) return 1;
  const tsdf::TrackVolume vol = tsdf::volume_of<const float, const int32_t>(volume, nx, ny, nz, 0, ox, oy, oz, voxel);
  float view[tsdf::kViewFloats];
  if (!tsdf::load_view(K, TCO, view)) return 2;
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const size_t pix = (size_t)y * w + x;
      used_out[pix] = 0;
      if (mask && mask[pix] == 0) continue;
      float row[tsdf::kTrackRowFloats];
      if (!tsdf::track_row(x, y, depth[pix], view, vol, mu, min_views, row)) continue;
      used_out[pix] = 1;
      std::memcpy(rows + pix * tsdf::kTrackRowFloats, row, sizeof(row));
    }
  return 0;
}

extern "C" void tsdf_track_emul_limits(long long* v) {
  v[0] = tsdf::kTrackGroupPixels;
  v[1] = tsdf::kTrackBlock;
  v[2] = tsdf::kTrackSums;
  v[3] = tsdf::kTrackRecord;
  v[4] = tsdf::kTrackMaxIters;
  v[5] = tsdf::kTrackMaxFrames;
}
