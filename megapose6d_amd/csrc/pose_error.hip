// pose_error.hip -- pose errors between two pose tables and a mesh, fused so that no point pair is ever stored.
//
// Reference (paths under src/megapose/):
//   dists_add / dists_add_symmetries / dists_add_symmetric   lib3d/distances.py:26-53
//   mssd_torch, compute_pose_error                           evaluation/utils.py:175-238, :50-66
//   ADD on the valid points, 2D projection error             evaluation/meters/modelnet_meters.py:66-79, lib3d/camera_geometry.py:26-37
// The reference materialises [B,S,N,3] (mssd_torch) and [B,N,N,3] (dists_add_symmetric) tensors; here a row's predicted points are
// transformed once and every pair lives in registers only.  The arithmetic of one element is pose_error_core.h (shared with the host
// emulation of the tests); this file adds the work distribution and the deterministic reductions.
//
//   sym_partial_kernel   (a) one wave per 256-point chunk of a row, all symmetries: per (row, symmetry, chunk) sum and max of the distances;
//                            a template over the distance: SpaceMetric (3D norm: ADD, MSSD) or PixelMetric (between projections: MSPD)
//   sym_finalize_kernel  (a) one workgroup per row: chunk partials -> errs[s], arg-min, T_gt_sym, optional difference vectors
//   nn_pairs_kernel      (b) one workgroup per (row, 1024 ground-truth points, range of predicted points): running (d2, k), merged by
//                            a 64-bit atomic minimum on (bits(d2) << 32 | k)
//   nn_finalize_kernel   (b) one workgroup per row: assignment -> difference vectors, mean and max of their norms
//   rigid_kernel         (c) one workgroup per row: translation / rotation error, mean 2D projection distance
#include "common.h"
#include "pose_error_core.h"

namespace mp {

using pe::kChunk;
using pe::kMaxSym;
using pe::kPerLane;

// lane-strided sum / max of n values, then the butterfly: the one order in which chunk partials are combined
__device__ __forceinline__ float chunks_sum(const float* __restrict__ part, int n, int stride, int lane) {
  float acc = 0.f;
  for (int c = lane; c < n; c += 64) acc = acc + part[(size_t)c * stride];
  return wave_sum_all(acc);
}
__device__ __forceinline__ float chunks_max(const float* __restrict__ part, int n, int stride, int lane) {
  float acc = 0.f;
  for (int c = lane; c < n; c += 64) acc = fmaxf(acc, part[(size_t)c * stride]);
  return wave_max_all(acc);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (a) symmetry-set error
// ---------------------------------------------------------------------------------------------------------------------------------
// What the two forms of the error differ in: the 12 floats kept per pose, what a lane keeps per point, and the distance.
struct SpaceMetric {   // 3D: the pose itself, the transformed point, the norm of the difference
  static constexpr int kKeep = 3;
  __device__ SpaceMetric(const float*, int) {}
  __device__ void matrix(const float* T, float* M) const {
    for (int k = 0; k < 12; ++k) M[k] = T[k];
  }
  __device__ static void point(const float* M, float x, float y, float z, float* q) { pe::apply(M, x, y, z, q[0], q[1], q[2]); }
  __device__ static float dist(const float* q, const float* g) { return sqrtf(pe::norm2(g[0] - q[0], g[1] - q[1], g[2] - q[2])); }
};
struct PixelMetric {   // projected (MSPD): P = K T (the projection of the rigid launch), the pixel position, the pixel distance
  static constexpr int kKeep = 2;
  float Kr[9];
  __device__ PixelMetric(const float* K, int row) {
    for (int k = 0; k < 9; ++k) Kr[k] = K[(size_t)row * 9 + k];
  }
  __device__ void matrix(const float* T, float* M) const { pe::proj_matrix(Kr, T, M); }
  __device__ static void point(const float* M, float x, float y, float z, float* q) { pe::project(M, x, y, z, q[0], q[1]); }
  __device__ static float dist(const float* q, const float* g) { return pe::pixel_dist(q[0], q[1], g[0], g[1]); }
};

// grid (b, wgs_per_row); wave w of workgroup y takes chunks (4y + w), (4y + w) + 4 wgs_per_row, ...: which wave computes a chunk never
// changes the chunk's partial, so every grid gives the same bits.  LDS keeps the metric's matrix of T_gt Sym_s per symmetry.
template <class Metric>
__global__ __launch_bounds__(256) void sym_partial_kernel(const float* __restrict__ T_pred, const float* __restrict__ T_gt,
                                                          const float* __restrict__ syms, const int32_t* __restrict__ n_sym, int S_max,
                                                          const float* __restrict__ K, const float* __restrict__ points, int n_pts_stride,
                                                          const int32_t* __restrict__ mesh_ids, const int32_t* __restrict__ n_points,
                                                          int n_pts, int n_chunks, float* __restrict__ partial) {
  __shared__ float Mgs[kMaxSym * 12];
  const int row = blockIdx.x, mesh = mesh_ids[row];
  const int ns = syms ? (n_sym ? min(n_sym[mesh], S_max) : S_max) : S_max;
  const int nv = n_points ? min(n_points[mesh], n_pts) : n_pts;
  const Metric metric(K, row);
  for (int s = threadIdx.x; s < ns; s += 256) {
    float O[16], Mg[12];
    if (syms) {
      pe::compose(T_gt + (size_t)row * 16, syms + ((size_t)mesh * S_max + s) * 16, O);
    } else {
      for (int k = 0; k < 12; ++k) O[k] = T_gt[((size_t)row * S_max + s) * 16 + k];
    }
    metric.matrix(O, Mg);
    for (int k = 0; k < 12; ++k) Mgs[s * 12 + k] = Mg[k];
  }
  __syncthreads();
  float Mp[12];
  metric.matrix(T_pred + (size_t)row * 16, Mp);
  const float* P = points + (size_t)mesh * n_pts_stride * 3;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = blockIdx.y * 4 + wave; c < n_chunks; c += gridDim.y * 4) {
    float px[kPerLane], py[kPerLane], pz[kPerLane], q[kPerLane][Metric::kKeep];
    bool ok[kPerLane];
#pragma unroll
    for (int p = 0; p < kPerLane; ++p) {
      const int j = c * kChunk + p * 64 + lane;
      ok[p] = j < nv;
      const int jj = ok[p] ? j : 0;
      px[p] = P[3 * jj]; py[p] = P[3 * jj + 1]; pz[p] = P[3 * jj + 2];
      Metric::point(Mp, px[p], py[p], pz[p], q[p]);
    }
    for (int s = 0; s < ns; ++s) {
      const float* G = Mgs + s * 12;
      float sum = 0.f, mx = 0.f;
#pragma unroll
      for (int p = 0; p < kPerLane; ++p) {
        float g[Metric::kKeep];
        Metric::point(G, px[p], py[p], pz[p], g);
        const float n = Metric::dist(q[p], g);
        sum = sum + (ok[p] ? n : 0.f);
        mx = fmaxf(mx, ok[p] ? n : 0.f);
      }
      sum = wave_sum_all(sum);
      mx = wave_max_all(mx);
      if (lane == 0) {
        float* o = partial + (((size_t)row * S_max + s) * n_chunks + c) * 2;
        o[0] = sum;
        o[1] = mx;
      }
    }
  }
}

__global__ __launch_bounds__(256) void sym_finalize_kernel(const float* __restrict__ T_pred, const float* __restrict__ T_gt,
                                                           const float* __restrict__ syms, const int32_t* __restrict__ n_sym, int S_max,
                                                           const float* __restrict__ points, int n_pts_stride,
                                                           const int32_t* __restrict__ mesh_ids, const int32_t* __restrict__ n_points,
                                                           int n_pts, int n_chunks, int reduce_max, const float* __restrict__ partial,
                                                           float* __restrict__ err, float* __restrict__ err_alt, int32_t* __restrict__ idx,
                                                           float* __restrict__ T_gt_sym, float* __restrict__ errs,
                                                           float* __restrict__ diffs) {
  __shared__ float Tw[16];
  const int row = blockIdx.x, mesh = mesh_ids[row];
  const int ns = syms ? (n_sym ? min(n_sym[mesh], S_max) : S_max) : S_max;
  const int nv = n_points ? min(n_points[mesh], n_pts) : n_pts;
  const int lane = threadIdx.x & 63;
  if (threadIdx.x < 64) {
    bool ok = pe::pose_finite(T_pred + (size_t)row * 16);
    if (syms) ok = ok && pe::pose_finite(T_gt + (size_t)row * 16);
    float best = INFINITY, best_alt = INFINITY;
    int bi = -1;
    for (int s = 0; s < S_max; ++s) {
      float e = INFINITY, e_alt = INFINITY;
      if (s < ns) {
        const float* part = partial + ((size_t)row * S_max + s) * n_chunks * 2;
        const float sum = chunks_sum(part, n_chunks, 2, lane);
        const float mx = chunks_max(part + 1, n_chunks, 2, lane);
        const bool ok_s = ok && (syms || pe::pose_finite(T_gt + ((size_t)row * S_max + s) * 16));
        const float mean = ok_s ? sum / (float)nv : pe::quiet_nan();
        const float mxv = (ok_s && mean == mean) ? mx : pe::quiet_nan();   // fmaxf drops a NaN term, the sum keeps it
        e = reduce_max ? mxv : mean;
        e_alt = reduce_max ? mean : mxv;
        if (e < best) { best = e; bi = s; }
        if (e_alt < best_alt) best_alt = e_alt;
      }
      if (errs && lane == 0) errs[(size_t)row * S_max + s] = e;
    }
    if (lane == 0) {
      err[row] = bi >= 0 ? best : pe::quiet_nan();
      if (err_alt) err_alt[row] = bi >= 0 && best_alt < INFINITY ? best_alt : pe::quiet_nan();
      idx[row] = bi;
      float O[16];
      if (bi >= 0) {
        if (syms) {
          pe::compose(T_gt + (size_t)row * 16, syms + ((size_t)mesh * S_max + bi) * 16, O);
        } else {
          for (int k = 0; k < 16; ++k) O[k] = T_gt[((size_t)row * S_max + bi) * 16 + k];
        }
      } else {
        for (int k = 0; k < 16; ++k) O[k] = pe::quiet_nan();
      }
      for (int k = 0; k < 16; ++k) {
        Tw[k] = O[k];
        if (T_gt_sym) T_gt_sym[(size_t)row * 16 + k] = O[k];
      }
    }
  }
  if (!diffs) return;
  __syncthreads();
  float Tp[12], Tg[12];
  for (int k = 0; k < 12; ++k) { Tp[k] = T_pred[(size_t)row * 16 + k]; Tg[k] = Tw[k]; }
  const float* P = points + (size_t)mesh * n_pts_stride * 3;
  float* D = diffs + (size_t)row * n_pts * 3;
  for (int j = threadIdx.x; j < n_pts; j += 256) {
    float dx = 0.f, dy = 0.f, dz = 0.f;
    if (j < nv) {
      float qx, qy, qz, gx, gy, gz;
      pe::apply(Tp, P[3 * j], P[3 * j + 1], P[3 * j + 2], qx, qy, qz);
      pe::apply(Tg, P[3 * j], P[3 * j + 1], P[3 * j + 2], gx, gy, gz);
      dx = gx - qx; dy = gy - qy; dz = gz - qz;
    }
    D[3 * j] = dx; D[3 * j + 1] = dy; D[3 * j + 2] = dz;   // the padded tail is zero
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (b) nearest-neighbour error (ADD-S)
// ---------------------------------------------------------------------------------------------------------------------------------
constexpr int kNnOwn = 4;                 // ground-truth points per lane
constexpr int kNnGt = 256 * kNnOwn;       // ground-truth points per workgroup
constexpr int kNnTile = 1024;             // predicted points per LDS tile (16-byte records)

// grid (gt tiles, pred splits, b).  Every lane keeps kNnOwn ground-truth points in registers; one broadcast 16-byte LDS read of a predicted
// point feeds kNnOwn pairs.  The running (d2, k) scans k ascending with a strict <.
__global__ __launch_bounds__(256) void nn_pairs_kernel(const float* __restrict__ T_pred, const float* __restrict__ T_gt,
                                                       const float* __restrict__ points, int n_pts_stride,
                                                       const int32_t* __restrict__ mesh_ids, const int32_t* __restrict__ n_points,
                                                       int n_pts, int tiles_per_split, unsigned long long* __restrict__ keys) {
  __shared__ float4 tile[kNnTile];
  const int row = blockIdx.z, mesh = mesh_ids[row];
  const int nv = n_points ? min(n_points[mesh], n_pts) : n_pts;
  const int k_begin = blockIdx.y * tiles_per_split * kNnTile;
  const int k_end = min(nv, k_begin + tiles_per_split * kNnTile);
  const int j0 = blockIdx.x * kNnGt;
  if (j0 >= nv || k_begin >= k_end) return;   // uniform over the workgroup
  const float* P = points + (size_t)mesh * n_pts_stride * 3;
  float Tp[12], Tg[12];
  for (int k = 0; k < 12; ++k) { Tp[k] = T_pred[(size_t)row * 16 + k]; Tg[k] = T_gt[(size_t)row * 16 + k]; }
  float gx[kNnOwn], gy[kNnOwn], gz[kNnOwn], best[kNnOwn];
  int bk[kNnOwn];
#pragma unroll
  for (int g = 0; g < kNnOwn; ++g) {
    const int j = j0 + g * 256 + threadIdx.x;
    const int jj = j < nv ? j : 0;
    pe::apply(Tg, P[3 * jj], P[3 * jj + 1], P[3 * jj + 2], gx[g], gy[g], gz[g]);
    best[g] = INFINITY;
    bk[g] = -1;
  }
  for (int t0 = k_begin; t0 < k_end; t0 += kNnTile) {
    const int cnt = min(kNnTile, k_end - t0);
    __syncthreads();
    for (int k = threadIdx.x; k < cnt; k += 256) {
      float qx, qy, qz;
      pe::apply(Tp, P[3 * (t0 + k)], P[3 * (t0 + k) + 1], P[3 * (t0 + k) + 2], qx, qy, qz);
      tile[k] = make_float4(qx, qy, qz, 0.f);
    }
    __syncthreads();
#pragma unroll 4
    for (int k = 0; k < cnt; ++k) {
      const float4 q = tile[k];
#pragma unroll
      for (int g = 0; g < kNnOwn; ++g) {
        const float d2 = pe::norm2(gx[g] - q.x, gy[g] - q.y, gz[g] - q.z);
        const bool lt = d2 < best[g];
        best[g] = lt ? d2 : best[g];
        bk[g] = lt ? t0 + k : bk[g];
      }
    }
  }
#pragma unroll
  for (int g = 0; g < kNnOwn; ++g) {
    const int j = j0 + g * 256 + threadIdx.x;
    if (j < nv) atomicMin(keys + (size_t)row * n_pts + j, (unsigned long long)pe::nn_key(best[g], bk[g]));
  }
}

// one workgroup per row (a fixed grid: the reduction order never changes)
__global__ __launch_bounds__(256) void nn_finalize_kernel(const float* __restrict__ T_pred, const float* __restrict__ T_gt,
                                                          const float* __restrict__ points, int n_pts_stride,
                                                          const int32_t* __restrict__ mesh_ids, const int32_t* __restrict__ n_points,
                                                          int n_pts, const unsigned long long* __restrict__ keys,
                                                          float* __restrict__ diffs, int32_t* __restrict__ assign,
                                                          float* __restrict__ mean_out, float* __restrict__ max_out) {
  __shared__ float red[4][2];
  const int row = blockIdx.x, mesh = mesh_ids[row];
  const int nv = n_points ? min(n_points[mesh], n_pts) : n_pts;
  const float* P = points + (size_t)mesh * n_pts_stride * 3;
  float Tp[12], Tg[12];
  for (int k = 0; k < 12; ++k) { Tp[k] = T_pred[(size_t)row * 16 + k]; Tg[k] = T_gt[(size_t)row * 16 + k]; }
  const bool ok = pe::pose_finite(Tp) && pe::pose_finite(Tg);
  // per-thread compensated sum (a thread owns up to n_pts / 256 terms), then butterfly + 4 waves
  float sum = 0.f, comp = 0.f, mx = 0.f;
  for (int j = threadIdx.x; j < n_pts; j += 256) {
    float dx = 0.f, dy = 0.f, dz = 0.f;
    int k = -1;
    if (j < nv) {
      k = (int)(uint32_t)(keys[(size_t)row * n_pts + j] & 0xffffffffull);
      if (!ok || k < 0 || k >= nv) {
        k = -1;
        dx = dy = dz = pe::quiet_nan();
      } else {
        float qx, qy, qz, gx, gy, gz;
        pe::apply(Tp, P[3 * k], P[3 * k + 1], P[3 * k + 2], qx, qy, qz);
        pe::apply(Tg, P[3 * j], P[3 * j + 1], P[3 * j + 2], gx, gy, gz);
        dx = gx - qx; dy = gy - qy; dz = gz - qz;
      }
      const float n = sqrtf(pe::norm2(dx, dy, dz));
      const float y = n - comp;
      const float t = sum + y;
      comp = (t - sum) - y;
      sum = t;
      mx = fmaxf(mx, n);
    }
    if (diffs) {
      float* D = diffs + ((size_t)row * n_pts + j) * 3;
      D[0] = dx; D[1] = dy; D[2] = dz;
    }
    if (assign) assign[(size_t)row * n_pts + j] = k;
  }
  sum = wave_sum_all(sum);
  mx = wave_max_all(mx);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave][0] = sum; red[wave][1] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float s = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
    const float m = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
    const float mean = s / (float)nv;
    mean_out[row] = mean;
    max_out[row] = mean == mean ? m : pe::quiet_nan();
  }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// (c) rigid / projected errors
// ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rigid_kernel(const float* __restrict__ T_a, const float* __restrict__ T_b, const float* __restrict__ K,
                                                    const float* __restrict__ points, int n_pts_stride, const int32_t* __restrict__ mesh_ids,
                                                    const int32_t* __restrict__ n_points, int n_pts, float* __restrict__ trans,
                                                    float* __restrict__ rot, float* __restrict__ proj) {
  __shared__ float red[4];
  const int row = blockIdx.x;
  const float* Ta = T_a + (size_t)row * 16;
  const float* Tb = T_b + (size_t)row * 16;
  if (threadIdx.x == 0) {
    float tr, rd;
    pe::rigid(Ta, Tb, tr, rd);
    trans[row] = tr;
    rot[row] = rd;
  }
  if (!proj) return;
  const int mesh = mesh_ids[row];
  const int nv = n_points ? min(n_points[mesh], n_pts) : n_pts;
  const float* P = points + (size_t)mesh * n_pts_stride * 3;
  float Pa[12], Pb[12];
  pe::proj_matrix(K + (size_t)row * 9, Ta, Pa);
  pe::proj_matrix(K + (size_t)row * 9, Tb, Pb);
  float sum = 0.f, comp = 0.f;
  for (int j = threadIdx.x; j < nv; j += 256) {
    const float n = pe::proj_dist(Pa, Pb, P[3 * j], P[3 * j + 1], P[3 * j + 2]);
    const float y = n - comp;
    const float t = sum + y;
    comp = (t - sum) - y;
    sum = t;
  }
  sum = wave_sum_all(sum);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[wave] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool ok = pe::pose_finite(Ta) && pe::pose_finite(Tb);
    proj[row] = ok ? ((red[0] + red[1]) + (red[2] + red[3])) / (float)nv : pe::quiet_nan();
  }
}

static inline int n_chunks_of(int n_pts) { return (n_pts + kChunk - 1) / kChunk; }

}  // namespace mp

using namespace mp;

extern "C" size_t mp_pose_error_workspace_bytes(int b, int n_pts, int S_max) {
  if (b < 0 || n_pts < 1 || S_max < 1) return 0;
  const size_t sym = (size_t)b * S_max * n_chunks_of(n_pts) * 2 * sizeof(float);
  const size_t nn = (size_t)b * n_pts * sizeof(unsigned long long);
  return align256(sym > nn ? sym : nn) + 256;
}

// both symmetry-set entries: `name` is the entry's (messages; without its mp_ prefix, the profiler row), d_K null = the 3D form
static int pose_error_sym_launch(const char* name, const float* d_T_pred, const float* d_T_gt, const float* d_symmetries, const int32_t* d_n_sym,
                                 int S_max, const float* d_points, int n_pts_stride, const int32_t* d_mesh_ids, const int32_t* d_n_points,
                                 int n_pts, int b, int reduce, int split, const float* d_K, float* d_err, float* d_err_alt, int32_t* d_idx,
                                 float* d_T_gt_sym, float* d_errs, float* d_diffs, void* d_workspace, size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(d_T_pred && d_T_gt && d_points && d_mesh_ids && d_err && d_idx && d_workspace, "%s: null pointer", name);
  MP_REQUIRE(n_pts >= 1 && n_pts <= n_pts_stride && b >= 0, "%s: bad sizes (n_pts %d, stride %d, b %d)", name, n_pts, n_pts_stride, b);
  MP_REQUIRE(S_max >= 1 && S_max <= kMaxSym, "%s: S_max %d outside [1, %d]", name, S_max, kMaxSym);
  MP_REQUIRE(reduce == MP_POSE_ERROR_MEAN || reduce == MP_POSE_ERROR_MAX, "%s: unknown reduce %d", name, reduce);
  MP_REQUIRE(split >= 0, "%s: split < 0", name);
  MP_REQUIRE(workspace_bytes >= mp_pose_error_workspace_bytes(b, n_pts, S_max), "%s: workspace too small", name);
  if (b == 0) return MP_OK;
  const int nch = n_chunks_of(n_pts);
  const int max_wgs = ceil_div(nch, 4);
  int wgs = split > 0 ? split : ceil_div(1024, b);   // ~4 workgroups per CU when the rows alone cannot give them
  wgs = wgs < 1 ? 1 : (wgs > max_wgs ? max_wgs : wgs);
  MP_REQUIRE(wgs <= 65535, "%s: split too large", name);
  float* part = (float*)d_workspace;
  ProfScope prof(name + 3, 0.0, (double)b * n_pts * 12.0, (hipStream_t)stream);
  if (d_K)
    hipLaunchKernelGGL(sym_partial_kernel<PixelMetric>, dim3(b, wgs), dim3(256), 0, (hipStream_t)stream, d_T_pred, d_T_gt, d_symmetries, d_n_sym,
                       S_max, d_K, d_points, n_pts_stride, d_mesh_ids, d_n_points, n_pts, nch, part);
  else
    hipLaunchKernelGGL(sym_partial_kernel<SpaceMetric>, dim3(b, wgs), dim3(256), 0, (hipStream_t)stream, d_T_pred, d_T_gt, d_symmetries, d_n_sym,
                       S_max, d_K, d_points, n_pts_stride, d_mesh_ids, d_n_points, n_pts, nch, part);
  MP_CHECK_HIP(hipGetLastError());
  // the chunk partials have one layout: the same finalize picks the symmetry
  hipLaunchKernelGGL(sym_finalize_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, d_T_pred, d_T_gt, d_symmetries, d_n_sym, S_max, d_points,
                     n_pts_stride, d_mesh_ids, d_n_points, n_pts, nch, reduce == MP_POSE_ERROR_MAX ? 1 : 0, part, d_err, d_err_alt, d_idx,
                     d_T_gt_sym, d_errs, d_diffs);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_pose_error_sym(const float* d_T_pred, const float* d_T_gt, const float* d_symmetries, const int32_t* d_n_sym, int S_max,
                                 const float* d_points, int n_pts_stride, const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts,
                                 int b, int reduce, int split, float* d_err, float* d_err_alt, int32_t* d_idx, float* d_T_gt_sym,
                                 float* d_errs, float* d_diffs, void* d_workspace, size_t workspace_bytes, mp_stream stream) {
  return pose_error_sym_launch("mp_pose_error_sym", d_T_pred, d_T_gt, d_symmetries, d_n_sym, S_max, d_points, n_pts_stride, d_mesh_ids, d_n_points,
                               n_pts, b, reduce, split, nullptr, d_err, d_err_alt, d_idx, d_T_gt_sym, d_errs, d_diffs, d_workspace,
                               workspace_bytes, stream);
}

extern "C" int mp_pose_error_mspd(const float* d_T_pred, const float* d_T_gt, const float* d_symmetries, const int32_t* d_n_sym, int S_max,
                                  const float* d_points, int n_pts_stride, const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts,
                                  int b, int reduce, int split, const float* d_K, float* d_err, float* d_err_alt, int32_t* d_idx,
                                  float* d_T_gt_sym, float* d_errs, void* d_workspace, size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(d_K, "mp_pose_error_mspd: null pointer");
  return pose_error_sym_launch("mp_pose_error_mspd", d_T_pred, d_T_gt, d_symmetries, d_n_sym, S_max, d_points, n_pts_stride, d_mesh_ids, d_n_points,
                               n_pts, b, reduce, split, d_K, d_err, d_err_alt, d_idx, d_T_gt_sym, d_errs, nullptr, d_workspace, workspace_bytes,
                               stream);
}

extern "C" int mp_pose_error_nn(const float* d_T_pred, const float* d_T_gt, const float* d_points, int n_pts_stride,
                                const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts, int b, int split, float* d_diffs,
                                int32_t* d_assign, float* d_mean, float* d_max, void* d_workspace, size_t workspace_bytes, mp_stream stream) {
  MP_REQUIRE(d_T_pred && d_T_gt && d_points && d_mesh_ids && d_mean && d_max && d_workspace, "mp_pose_error_nn: null pointer");
  MP_REQUIRE(n_pts >= 1 && n_pts <= n_pts_stride && b >= 0 && b <= 65535, "mp_pose_error_nn: bad sizes (n_pts %d, stride %d, b %d)", n_pts,
             n_pts_stride, b);
  MP_REQUIRE(split >= 0, "mp_pose_error_nn: split < 0");
  MP_REQUIRE(workspace_bytes >= mp_pose_error_workspace_bytes(b, n_pts, 1), "mp_pose_error_nn: workspace too small");
  if (b == 0) return MP_OK;
  const int gt_tiles = ceil_div(n_pts, kNnGt), pred_tiles = ceil_div(n_pts, kNnTile);
  int splits = split > 0 ? split : ceil_div(1024, (long)b * gt_tiles);
  splits = splits < 1 ? 1 : (splits > pred_tiles ? pred_tiles : splits);
  const int tiles_per_split = ceil_div(pred_tiles, splits);
  splits = ceil_div(pred_tiles, tiles_per_split);
  MP_REQUIRE(splits <= 65535, "mp_pose_error_nn: split too large");
  unsigned long long* keys = (unsigned long long*)d_workspace;
  ProfScope prof("pose_error_nn", 0.0, (double)b * n_pts * 32.0, (hipStream_t)stream);
  MP_CHECK_HIP(hipMemsetAsync(keys, 0xff, (size_t)b * n_pts * sizeof(unsigned long long), (hipStream_t)stream));
  hipLaunchKernelGGL(nn_pairs_kernel, dim3(gt_tiles, splits, b), dim3(256), 0, (hipStream_t)stream, d_T_pred, d_T_gt, d_points, n_pts_stride,
                     d_mesh_ids, d_n_points, n_pts, tiles_per_split, keys);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(nn_finalize_kernel, dim3(b), dim3(256), 0, (hipStream_t)stream, d_T_pred, d_T_gt, d_points, n_pts_stride, d_mesh_ids,
                     d_n_points, n_pts, keys, d_diffs, d_assign, d_mean, d_max);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_pose_error_rigid(const float* d_T_a, const float* d_T_b, int b, const float* d_K, const float* d_points, int n_pts_stride,
                                   const int32_t* d_mesh_ids, const int32_t* d_n_points, int n_pts, float* d_trans_err, float* d_rot_err_deg,
                                   float* d_proj_err, mp_stream stream) {
  MP_REQUIRE(d_T_a && d_T_b && d_trans_err && d_rot_err_deg && b >= 0, "mp_pose_error_rigid: bad arguments");
  if (d_proj_err)
    MP_REQUIRE(d_K && d_points && d_mesh_ids && n_pts >= 1 && n_pts <= n_pts_stride, "mp_pose_error_rigid: the projection error needs K, points "
               "and mesh ids (n_pts %d, stride %d)", n_pts, n_pts_stride);
  if (b == 0) return MP_OK;
  hipLaunchKernelGGL(rigid_kernel, dim3(b), dim3(d_proj_err ? 256 : 64), 0, (hipStream_t)stream, d_T_a, d_T_b, d_K, d_points, n_pts_stride,
                     d_mesh_ids, d_n_points, n_pts, d_trans_err, d_rot_err_deg, d_proj_err);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
