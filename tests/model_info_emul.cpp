// TEST SUPPORT: host emulation of the model-info kernels (megapose6d_amd/csrc/model_info.hip), built from the same rules header
// (model_info_core.h).  Same arguments as the C ABI, on host arrays: the jobs of the prefix array one after the other (in the order the
// caller gives, to show that the order does not matter), each job as the workgroup does it -- lane by lane, stage by stage -- then a plain
// fold of the partials and a plain loop for the bounds.  No lanes, no LDS, no shuffles.  Built by tests/support/model_info.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "model_info_core.h"

using namespace mp;
using minfo::Cand;

// off [n_obj + 1] = the prefix array of job counts -> the number of jobs, -1 for arguments the launch rejects
extern "C" long long model_info_emul_prefix(int n_obj, const int32_t* n_points, int tile, int32_t* off) {
  if (n_obj < 1 || !minfo::tile_ok(tile)) return -1;
  const int chunk = minfo::chunk_of(tile);
  long long total = 0;
  off[0] = 0;
  for (int o = 0; o < n_obj; ++o) {
    if (n_points[o] < 1) return -1;
    total += minfo::n_jobs(n_points[o], chunk);
    if (total >= minfo::kMaxJobs) return -1;
    off[o + 1] = (int32_t)total;
  }
  return total;
}

// job `local` of an object of n points -> i-block, j-chunk and the j range [j0, j1) it looks at
extern "C" void model_info_emul_decode(long long local, int tile, int n, int32_t* out) {
  int b, c, j0, j1;
  minfo::decode_job(local, minfo::chunk_of(tile), &b, &c);
  minfo::job_range(b, c, minfo::chunk_of(tile), n, &j0, &j1);
  out[0] = b;
  out[1] = c;
  out[2] = j0;
  out[3] = j1;
}

extern "C" int model_info_emul(const float* points, int stride, const int32_t* n_points, int n_obj, int tile_arg,
                               const int64_t* job_order /*a permutation of the jobs, or NULL*/, float* d2, int32_t* pair, float* bounds) {
  std::vector<int32_t> off((size_t)n_obj + 1);
  const long long total = model_info_emul_prefix(n_obj, n_points, tile_arg, off.data());
  if (total < 0) return 1;
  for (int o = 0; o < n_obj; ++o)
    if (n_points[o] > stride) return 1;
  const int tile = minfo::tile_of(tile_arg), chunk = minfo::chunk_of(tile_arg);
  std::vector<Cand> partials((size_t)total, Cand{NAN, -7, -7});
  for (long long k = 0; k < total; ++k) {
    const long long job = job_order ? job_order[k] : k;
    int obj = 0;
    while (off[obj + 1] <= job) ++obj;
    const int n = n_points[obj];
    const float* P = points + (size_t)obj * stride * 3;
    int b, c, j_begin, j_end;
    minfo::decode_job(job - off[obj], chunk, &b, &c);
    minfo::job_range(b, c, chunk, n, &j_begin, &j_end);
    Cand best = minfo::none();
    for (int lane = 0; lane < minfo::kBlock; ++lane) {
      const int i = b * minfo::kBlock + lane;
      if (i >= n) continue;
      float best_d2 = -1.0f;
      int best_j = minfo::kNone;
      for (int j0 = j_begin; j0 < j_end; j0 += tile) {
        const int n_stage = j_end - j0 < tile ? j_end - j0 : tile;
        for (int t = 0; t < n_stage; ++t) {
          const int j = j0 + t;
          if (j < i) continue;
          minfo::lane_update(minfo::dist2(P[3 * i], P[3 * i + 1], P[3 * i + 2], P[3 * j], P[3 * j + 1], P[3 * j + 2]), j, &best_d2, &best_j);
        }
      }
      const Cand mine = best_j == minfo::kNone ? minfo::none() : Cand{best_d2, i, best_j};
      if (minfo::better(mine, best)) best = mine;
    }
    partials[(size_t)job] = best;
  }
  for (int o = 0; o < n_obj; ++o) {
    Cand best = minfo::none();
    for (long long p = off[o]; p < off[o + 1]; ++p)
      if (minfo::better(partials[(size_t)p], best)) best = partials[(size_t)p];
    const float* P = points + (size_t)o * stride * 3;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    bool bad = false;
    for (int r = 0; r < n_points[o]; ++r) {
      bad = bad || !minfo::finite3(P[3 * r], P[3 * r + 1], P[3 * r + 2]);
      for (int a = 0; a < 3; ++a) {
        lo[a] = fminf(lo[a], P[3 * r + a]);
        hi[a] = fmaxf(hi[a], P[3 * r + a]);
      }
    }
    const bool ok = !bad && best.j != minfo::kNone;
    d2[o] = ok ? best.d2 : NAN;
    pair[2 * o] = ok ? best.i : -1;
    pair[2 * o + 1] = ok ? best.j : -1;
    for (int a = 0; a < 3; ++a) {
      bounds[6 * o + a] = ok ? lo[a] : NAN;
      bounds[6 * o + 3 + a] = ok ? hi[a] - lo[a] : NAN;
    }
  }
  return 0;
}

extern "C" void model_info_emul_limits(int* v) {
  v[0] = minfo::kBlock;
  v[1] = minfo::kTileStep;
  v[2] = minfo::kMaxTile;
  v[3] = minfo::kDefaultTile;
  v[4] = minfo::kDefaultChunk;
}
