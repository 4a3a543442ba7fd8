// model_info.hip -- BOP's model info on the device: the exact diameter of each object's point set (the largest distance between two of
// its points, bop_toolkit's calc_pts_diameter: an O(N^2) maximum) and its axis-aligned bounds.
//
// The rules are model_info_core.h, shared with the host emulation of the tests; this file adds the work distribution.  The result is the
// maximum of a total order on the candidates (d2, i, j), so neither the grid, the tile, the chunk nor the order in which workgroups
// finish can change a bit.  No atomics: every job stores one candidate, a second launch folds them.
//
//   model_info_pairs_kernel   one workgroup of 256 lanes per job (i-block, j-chunk).  The workgroup finds its object by a binary search
//                             of the prefix array of job counts (n_obj + 1 entries) and its (block, chunk) in closed form
//                             [minfo::decode_job].  Lane l holds point i = 256 * block + l in registers.  The chunk's j points are
//                             staged `tile` at a time in LDS as float4 (x, y, z, 0): every lane then reads the SAME entry, one 16-byte
//                             read that the LDS broadcasts (identical addresses never conflict), and 16 KiB at the largest tile leave
//                             the workgroups per CU to the registers.  Stages that lie wholly after the block need no per-lane test;
//                             the stages that overlap it look at j >= i only.  Lanes with i >= n_points and stage entries with
//                             j >= n_points are masked out, never clamped: a padding row is not read.  Lane best -> workgroup best
//                             [block_primitives.h] -> one 16-byte vector store to partials[job].
//   model_info_reduce_kernel  one workgroup per object: folds the object's partials under the same order, takes min and max per axis and
//                             the finiteness of rows 0 .. n_points - 1, and stores d2, the pair and the bounds (NaN, -1 -1, NaN for an
//                             object with a non-finite coordinate).
#include <vector>

#include "common.h"
#include "model_info_core.h"

namespace mp {

using minfo::Cand;

constexpr int kWaves = minfo::kBlock / 64;

struct BestOp {   // the better of two candidates under minfo::better's total order
  static constexpr bool kFromZero = false;
  __device__ __forceinline__ Cand operator()(Cand a, Cand b) const { return minfo::better(b, a) ? b : a; }
};

__global__ __launch_bounds__(256) void model_info_pairs_kernel(const float* __restrict__ points, int stride,
                                                               const int32_t* __restrict__ n_points,
                                                               const int32_t* __restrict__ job_off, int n_obj, int tile, int chunk,
                                                               int4* __restrict__ partials) {
  __shared__ float4 stage[minfo::kMaxTile];
  __shared__ Cand red[kWaves];
  const int job = blockIdx.x, tid = threadIdx.x;
  const int obj = object_of(job_off, n_obj, job);
  int n = n_points[obj];
  n = n < stride ? n : stride;   // the entry point checked the host's copy; the device's never reaches past the object's rows
  int b, c, j_begin, j_end;
  minfo::decode_job(job - job_off[obj], chunk, &b, &c);
  minfo::job_range(b, c, chunk, n, &j_begin, &j_end);
  const float* P = points + (size_t)obj * stride * 3;
  const int i = b * minfo::kBlock + tid;
  const bool own = i < n;
  float xi = 0.f, yi = 0.f, zi = 0.f;
  if (own) {
    xi = P[3 * (size_t)i];
    yi = P[3 * (size_t)i + 1];
    zi = P[3 * (size_t)i + 2];
  }
  float best_d2 = -1.0f;
  int best_j = minfo::kNone;
  const int i_last = b * minfo::kBlock + minfo::kBlock - 1;
  for (int j0 = j_begin; j0 < j_end; j0 += tile) {
    const int n_stage = j_end - j0 < tile ? j_end - j0 : tile;
    __syncthreads();
    for (int t = tid; t < n_stage; t += minfo::kBlock) {
      const size_t r = 3 * (size_t)(j0 + t);
      stage[t] = make_float4(P[r], P[r + 1], P[r + 2], 0.f);
    }
    __syncthreads();
    if (own && j0 > i_last) {   // the first test masks a lane, the second is uniform: the stage lies after every i of the block
#pragma unroll 8
      for (int t = 0; t < n_stage; ++t) {
        const float4 q = stage[t];
        minfo::lane_update(minfo::dist2(xi, yi, zi, q.x, q.y, q.z), j0 + t, &best_d2, &best_j);
      }
    } else if (own) {
#pragma unroll 4
      for (int t = 0; t < n_stage; ++t) {
        const float4 q = stage[t];
        if (j0 + t >= i) minfo::lane_update(minfo::dist2(xi, yi, zi, q.x, q.y, q.z), j0 + t, &best_d2, &best_j);
      }
    }
  }
  const Cand mine = best_j == minfo::kNone ? minfo::none() : Cand{best_d2, i, best_j};
  const Cand best = block_reduce_all<kWaves>(mine, red, BestOp());
  if (tid == 0) partials[job] = make_int4(__float_as_int(best.d2), best.i, best.j, 0);
}

__global__ __launch_bounds__(256) void model_info_reduce_kernel(const float* __restrict__ points, int stride,
                                                                const int32_t* __restrict__ n_points,
                                                                const int32_t* __restrict__ job_off, const int4* __restrict__ partials,
                                                                float* __restrict__ d2_out, int32_t* __restrict__ pair_out,
                                                                float* __restrict__ bounds_out) {
  __shared__ Cand red[kWaves];
  __shared__ float red_f[kWaves];
  __shared__ int red_bad[kWaves];
  const int obj = blockIdx.x, tid = threadIdx.x;
  int n = n_points[obj];
  n = n < stride ? n : stride;
  Cand mine = minfo::none();
  for (int p = job_off[obj] + tid; p < job_off[obj + 1]; p += minfo::kBlock) {
    const int4 v = partials[p];
    const Cand o{__int_as_float(v.x), v.y, v.z};
    if (minfo::better(o, mine)) mine = o;
  }
  const Cand best = block_reduce_all<kWaves>(mine, red, BestOp());
  const float* P = points + (size_t)obj * stride * 3;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  int bad = 0;
  for (int r = tid; r < n; r += minfo::kBlock) {
    const float x = P[3 * (size_t)r], y = P[3 * (size_t)r + 1], z = P[3 * (size_t)r + 2];
    bad |= !minfo::finite3(x, y, z);
    lo[0] = fminf(lo[0], x); lo[1] = fminf(lo[1], y); lo[2] = fminf(lo[2], z);
    hi[0] = fmaxf(hi[0], x); hi[1] = fmaxf(hi[1], y); hi[2] = fmaxf(hi[2], z);
  }
  bad = block_reduce_all<kWaves>(bad, red_bad, OrOp());
  for (int a = 0; a < 3; ++a) {
    lo[a] = block_min_all<kWaves>(lo[a], red_f);
    hi[a] = block_max_all<kWaves>(hi[a], red_f);
  }
  if (tid != 0) return;
  const bool ok = !bad && best.j != minfo::kNone;
  d2_out[obj] = ok ? best.d2 : NAN;
  pair_out[2 * obj] = ok ? best.i : -1;
  pair_out[2 * obj + 1] = ok ? best.j : -1;
  for (int a = 0; a < 3; ++a) {
    bounds_out[6 * obj + a] = ok ? lo[a] : NAN;
    bounds_out[6 * obj + 3 + a] = ok ? hi[a] - lo[a] : NAN;
  }
}

// the prefix array of job counts; false for arguments the launch rejects
static bool model_info_jobs(int n_obj, const int32_t* h_n_points, int tile, std::vector<int32_t>* off) {
  if (n_obj < 1 || !h_n_points || !minfo::tile_ok(tile)) return false;
  const int chunk = minfo::chunk_of(tile);
  long long total = 0;
  if (off) off->assign((size_t)n_obj + 1, 0);
  for (int o = 0; o < n_obj; ++o) {
    if (h_n_points[o] < 1) return false;
    total += minfo::n_jobs(h_n_points[o], chunk);
    if (total >= minfo::kMaxJobs) return false;
    if (off) (*off)[o + 1] = (int32_t)total;
  }
  return true;
}

struct ModelInfoWs {
  int32_t* off;      // the prefix array of job counts
  int4* partials;    // one per job; they end the workspace, unpadded
  size_t total;
  ModelInfoWs(void* base, int n_obj, int32_t n_jobs) {
    WsCarver c(base);
    off = c.take<int32_t>((size_t)n_obj + 1);
    partials = c.take<int4>((size_t)n_jobs, false);
    total = c.total();
  }
};

}  // namespace mp

using namespace mp;

extern "C" size_t mp_model_info_scratch_bytes(int n_obj, const int32_t* h_n_points, int tile) {
  std::vector<int32_t> off;
  if (!model_info_jobs(n_obj, h_n_points, tile, &off)) return 0;
  return ModelInfoWs(nullptr, n_obj, off[n_obj]).total;
}

extern "C" int mp_model_info(const float* d_points, int stride, const int32_t* d_n_points, const int32_t* h_n_points, int n_obj, int tile,
                             void* d_scratch, float* d_d2, int32_t* d_pair, float* d_bounds, mp_stream stream) {
  MP_REQUIRE(n_obj >= 1 && stride >= 1, "mp_model_info: n_obj %d, stride %d: both must be at least 1", n_obj, stride);
  MP_REQUIRE(minfo::tile_ok(tile), "mp_model_info: tile %d is not 0 or a multiple of %d in [%d, %d]", tile, minfo::kTileStep, minfo::kTileStep,
             minfo::kMaxTile);
  MP_REQUIRE(d_points && d_n_points && h_n_points && d_scratch && d_d2 && d_pair && d_bounds, "mp_model_info: null pointer");
  for (int o = 0; o < n_obj; ++o)
    MP_REQUIRE(h_n_points[o] >= 1 && h_n_points[o] <= stride, "mp_model_info: object %d has %d points, outside [1, stride = %d]", o,
               h_n_points[o], stride);
  std::vector<int32_t> off;
  MP_REQUIRE(model_info_jobs(n_obj, h_n_points, tile, &off), "mp_model_info: more than 2^31 - 1 jobs in one launch");
  hipStream_t s = (hipStream_t)stream;
  const ModelInfoWs ws(d_scratch, n_obj, off[n_obj]);
  double pairs = 0.0;
  for (int o = 0; o < n_obj; ++o) pairs += 0.5 * (double)h_n_points[o] * ((double)h_n_points[o] + 1.0);
  ProfScope prof("model_info", 8.0 * pairs, (double)n_obj * stride * 12.0, s);
  // pageable host memory: the runtime has taken the bytes when the call returns
  MP_CHECK_HIP(hipMemcpyAsync(ws.off, off.data(), off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(model_info_pairs_kernel, dim3((unsigned)off[n_obj]), dim3(minfo::kBlock), 0, s, d_points, stride, d_n_points, ws.off, n_obj,
                     minfo::tile_of(tile), minfo::chunk_of(tile), ws.partials);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(model_info_reduce_kernel, dim3(n_obj), dim3(minfo::kBlock), 0, s, d_points, stride, d_n_points, ws.off, ws.partials, d_d2,
                     d_pair, d_bounds);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
