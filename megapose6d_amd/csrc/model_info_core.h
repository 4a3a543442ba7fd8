// model_info_core.h -- the rules of BOP's model info (the exact diameter of a point set, the largest distance between two of its points,
// and its axis-aligned bounds) that run on the device (model_info.hip), shared with the host emulation (tests/model_info_emul.cpp) the
// way det_ap_core.h and vsd_core.h are shared with theirs.
//
// CONTRACT (mp_model_info)
//   * INPUTS.  points [n_obj, stride, 3] fp32; of object o only rows 0 .. n_points[o] - 1 are points, 1 <= n_points[o] <= stride; the
//     rows beyond hold arbitrary padding and are never read as points.
//   * DISTANCE.  d2(a, b) = fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with dx, dy, dz the fp32 differences a - b [dist2]: one fixed order,
//     no contraction, so device and host give the same bits, and d2(a, b) == d2(b, a) (the differences only change sign).
//   * ORDER.  A candidate is (d2, i, j) with i <= j; the pair (i, i) is one (d2 = 0), so a single point has a result.  A candidate beats
//     another when its d2 is larger; on equal d2 when its i is lower; then when its j is lower [better].  This is a total order on the
//     candidates of one object, the result is its maximum, and a maximum does not depend on how the candidates are split into jobs,
//     stages, lanes and waves, nor on the order the pieces are folded in.
//   * NON-FINITE.  A NaN or an infinite coordinate among an object's points makes that object's d2 NaN, its pair (-1, -1) and its six
//     bounds NaN (the convention of mp_vsd for a bad diameter); other objects of the launch are not affected.
//   * OUTPUTS.  d2 [n_obj] fp32, pair [n_obj, 2] int32, bounds [n_obj, 6] fp32 = min x y z, then size x y z (max - min in fp32).
//
// WORK.  An object's points are cut into blocks of kBlock = 256 (one i point per lane of a workgroup) and into chunks of `chunk` j points
// (a multiple of kBlock), streamed `tile` points at a time.  A job is one (i-block b, j-chunk c) whose chunk does not end before the
// block starts, c >= b / (chunk / kBlock); inside it only j >= i is looked at.  Jobs are numbered chunk by chunk: chunk c has the
// blocks 0 .. min(n_blocks, (c + 1) * chunk / kBlock) - 1, so chunk c starts at job (chunk / kBlock) * c * (c + 1) / 2 [jobs_before,
// decode_job], and the index memory of a launch is one prefix array of n_obj + 1 job counts, whatever the size of an object.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MINFO_HD __host__ __device__ __forceinline__
#else
#define MINFO_HD inline
#endif

namespace mp {
namespace minfo {

constexpr int kBlock = 256;             // i points of a job, one per lane
constexpr int kTileStep = 64;           // a forced tile is a multiple of this
constexpr int kMaxTile = 1024;          // j points of one LDS stage, at most (16 KiB)
constexpr int kDefaultTile = 256;       // tile == 0
constexpr int kDefaultChunk = 8192;     // j points of a job with tile == 0: 2 M pairs per job, 240 k jobs for 10^6 points
constexpr long long kMaxJobs = 2147483647LL;   // jobs of one launch: the grid's x extent, and an int32 prefix
constexpr int kNone = 2147483647;       // the indices of "no candidate yet"

struct Cand {
  float d2;
  int32_t i, j;
};

// loses against every candidate of a finite point (their d2 >= 0)
MINFO_HD Cand none() { return Cand{-1.0f, kNone, kNone}; }

MINFO_HD float dist2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

MINFO_HD bool better(const Cand& a, const Cand& b) {
  return a.d2 > b.d2 || (a.d2 == b.d2 && (a.i < b.i || (a.i == b.i && a.j < b.j)));
}

MINFO_HD bool finite3(float x, float y, float z) { return isfinite(x) && isfinite(y) && isfinite(z); }

MINFO_HD bool tile_ok(int tile) { return tile == 0 || (tile >= kTileStep && tile <= kMaxTile && tile % kTileStep == 0); }

MINFO_HD int tile_of(int tile) { return tile == 0 ? kDefaultTile : tile; }

// j points of a job: the library's choice, or with a forced tile the smallest multiple of kBlock that holds one stage (so that a few
// hundred points already make several chunks)
MINFO_HD int chunk_of(int tile) { return tile == 0 ? kDefaultChunk : (tile + kBlock - 1) / kBlock * kBlock; }

MINFO_HD long long n_blocks(int n_points) { return ((long long)n_points + kBlock - 1) / kBlock; }

MINFO_HD long long n_chunks(int n_points, int chunk) { return ((long long)n_points + chunk - 1) / chunk; }

// jobs of the chunks before chunk c (every one of them is followed by another chunk, so none is cut by n_blocks)
MINFO_HD long long jobs_before(long long c, int chunk) { return (long long)(chunk / kBlock) * (c * (c + 1) / 2); }

MINFO_HD long long n_jobs(int n_points, int chunk) {
  return n_points < 1 ? 0 : jobs_before(n_chunks(n_points, chunk) - 1, chunk) + n_blocks(n_points);
}

// job `local` of an object -> its i-block b and j-chunk c
MINFO_HD void decode_job(long long local, int chunk, int* b, int* c) {
  const double per = (double)(chunk / kBlock);
  long long cc = (long long)((sqrt(8.0 * (double)local / per + 1.0) - 1.0) * 0.5);
  if (cc < 0) cc = 0;
  while (jobs_before(cc, chunk) > local) --cc;
  while (jobs_before(cc + 1, chunk) <= local) ++cc;
  *c = (int)cc;
  *b = (int)(local - jobs_before(cc, chunk));
}

// the j range of job (b, c) of an object of n points: [*j0, *j1), never empty for a job that exists
MINFO_HD void job_range(int b, int c, int chunk, int n, int* j0, int* j1) {
  const long long start = (long long)c * chunk, first = (long long)b * kBlock, end = start + chunk;
  *j0 = (int)(start > first ? start : first);
  *j1 = (int)(end < n ? end : (long long)n);
}

// one lane's look at point j (ascending j per lane, so a strict comparison keeps the lowest j of equal distances)
MINFO_HD void lane_update(float d2, int j, float* best_d2, int* best_j) {
  if (d2 > *best_d2) {
    *best_d2 = d2;
    *best_j = j;
  }
}

}  // namespace minfo
}  // namespace mp
