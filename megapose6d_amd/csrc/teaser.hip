// teaser.hip -- the reference's second depth refiner (inference/teaserpp_refiner.py: TeaserppRefiner) on the device.
//
// Replaces a per-object CPU loop: numpy back-projection of the rendered and the measured depth (meshcat_utils.get_pointcloud), the masks
// of refiner_utils.compute_masks, pytorch3d.ops.sample_farthest_points (n_points sequential argmax passes), teaserpp_python's
// RobustRegistrationSolver (consistency graph, inlier selection, GNC-TLS rotation, component-wise TLS translation) and the inlier-count
// acceptance rule (teaserpp_refiner.py:143-149, :276-284).  teaserpp_python and pytorch3d are third-party code absent from the
// reference tree ("parity unpinned"); the algorithm is the one stated in teaser_core.h, which the host emulation and the float64
// restatement of the tests share.  Inlier selection is the k-core rule (TEASER++'s KCORE_HEU idea) by default; the exact maximum clique
// (TEASER++'s default) is selection 2, searched by teaser_clique.hip under a step budget.
//
// Structure: one train of launches on the caller's stream, no host round trip, no atomics, no workgroup waiting for another.
//   teaser_compact  (row)        ordered compaction of the mask pixels: source points + pixel ids
//   teaser_fps      (row)        farthest point sampling: a slice of the points and their running minima in registers, the rest streamed
//                                from L2; one packed-key argmax per pick (wave butterfly, one LDS step across the waves)
// The reductions and ordered compactions are those of block_primitives.h, which states their order and their barriers once.
//   teaser_gather   (row, k)     the sampled correspondences
//   teaser_graph    (tile, row)  the M x M consistency bit matrix, points in LDS, degrees by popcount
//   teaser_kcore    (row)        k-core peel, one thread per vertex, its matrix row in registers; ordered list of the selected vertices
//   clique_search   (rows)       selection 2 only (teaser_clique.hip): one wave per row replaces that list by the maximum clique's
//   teaser_solve    (row)        GNC-TLS rotation (float64 workgroup sums, 4x4 Jacobi on one lane), TLS translation by voting,
//                                inlier count, pose write
// Roofline: latency-bound tail work (once per detection, after the CNN stages); the sampling kernel is the long pole, a chain of
// n_points dependent argmax steps per row.
#include <algorithm>
#include <cmath>

#include "common.h"
#include "teaser_clique_core.h"
#include "teaser_core.h"

namespace mp {

using namespace teaser;

// ---- compaction ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void teaser_compact(const float* __restrict__ depth_meas, const int32_t* __restrict__ im_ids,
                                                           const float* __restrict__ depth_rend, const float* __restrict__ K_rows, int H, int W,
                                                           int mask_type, float thresh, float* __restrict__ pts, int32_t* __restrict__ pix,
                                                           int32_t* __restrict__ n_out) {
  __shared__ int wave_count[kWaves];
  const int row = blockIdx.x, tid = threadIdx.x;
  const int px = H * W;
  const float* dm = depth_meas + (size_t)im_ids[row] * px;
  const float* dr = depth_rend + (size_t)row * px;
  const float* K = K_rows + (size_t)row * 9;
  float* po = pts + (size_t)row * px * 3;
  int32_t* xo = pix + (size_t)row * px;
  int base = 0;   // points kept so far (the same in every thread)
  for (int start = 0; start < px; start += kThreads) {
    const int idx = start + tid;
    float r = 0.0f;
    bool in = false;
    if (idx < px) {
      r = dr[idx];
      in = mask_pixel(dm[idx], r, mask_type, thresh);
    }
    int kept;
    const int pos = base + block_compact<kWaves>(in, wave_count, &kept);
    if (in) {   // pos < N <= px: inside the row's slice
      float p[3];
      backproject(idx % W, idx / W, r, K, p);
      po[(size_t)pos * 3] = p[0]; po[(size_t)pos * 3 + 1] = p[1]; po[(size_t)pos * 3 + 2] = p[2];
      xo[pos] = idx;
    }
    base += kept;
  }
  if (tid == 0) n_out[row] = base;
}

// ---- farthest point sampling -------------------------------------------------------------------------------------------------------------
// points [row][stride][3]; counts[row] of them are valid (clamped to 0 .. stride).  idx_out [row][n_points] (-1 past M), m_out[row] = M.
// mind [row][stride]: the running minima of the points past the register-resident ones (touched only when N > kFpsResident).
__global__ __launch_bounds__(kThreads) void teaser_fps(const float* __restrict__ points, int stride, const int32_t* __restrict__ counts, int n_points,
                                                       int n_min_points, int use_fps, float* __restrict__ mind, int32_t* __restrict__ idx_out,
                                                       int32_t* __restrict__ m_out) {
  __shared__ unsigned long long wave_best[2][kWaves];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int N = counts[row];
  N = N < 0 ? 0 : (N > stride ? stride : N);
  const int M = n_samples(N, n_points, n_min_points);
  const float* P = points + (size_t)row * stride * 3;
  int32_t* out = idx_out + (size_t)row * n_points;
  if (tid == 0) m_out[row] = M;
  for (int k = tid; k < n_points; k += kThreads) out[k] = (k < M && !use_fps) ? stride_pick(k, N, M) : (k == 0 && M > 0 ? 0 : -1);
  if (M < 2 || !use_fps) return;
  float rp[kFpsReg][3], rmin[kFpsReg];
#pragma unroll
  for (int k = 0; k < kFpsReg; ++k) {
    const int i = tid + k * kThreads;
    const bool ok = i < N;
    rp[k][0] = ok ? P[(size_t)i * 3] : 0.0f;
    rp[k][1] = ok ? P[(size_t)i * 3 + 1] : 0.0f;
    rp[k][2] = ok ? P[(size_t)i * 3 + 2] : 0.0f;
    rmin[k] = INFINITY;
  }
  float* md = mind + (size_t)row * stride;
  for (int i = kFpsResident + tid; i < N; i += kThreads) md[i] = INFINITY;   // (a thread only ever reads the entries it wrote)
  int last = 0;
  for (int pick = 1; pick < M; ++pick) {
    const float q[3] = {P[(size_t)last * 3], P[(size_t)last * 3 + 1], P[(size_t)last * 3 + 2]};
    unsigned long long best = 0ull;
#pragma unroll
    for (int k = 0; k < kFpsReg; ++k) {
      const int i = tid + k * kThreads;
      if (i < N) {
        const float d = dist2(rp[k], q);
        if (d < rmin[k]) rmin[k] = d;
        const unsigned long long key = fps_key(rmin[k], i);
        best = key > best ? key : best;
      }
    }
    for (int i = kFpsResident + tid; i < N; i += kThreads) {
      const float p[3] = {P[(size_t)i * 3], P[(size_t)i * 3 + 1], P[(size_t)i * 3 + 2]};
      const float d = dist2(p, q);
      float mn = md[i];
      if (d < mn) { mn = d; md[i] = d; }
      const unsigned long long key = fps_key(mn, i);
      best = key > best ? key : best;
    }
    // (this argmax stays written out: the sampling chain is the refiner's long pole, and through wave_max_all -- the same instructions
    //  in the reduction -- the kernel came out scheduled 9 % slower)
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off);
      best = o > best ? o : best;
    }
    // (one barrier per pick where block_max_all has two: two buffers by the parity of the pick, and a wave can only overwrite a buffer
    //  after the barrier of the pick between, which every wave passes after it has read)
    if (lane == 0) wave_best[pick & 1][wave] = best;
    __syncthreads();
    best = 0ull;
    for (int w = 0; w < kWaves; ++w) {
      const unsigned long long o = wave_best[pick & 1][w];
      best = o > best ? o : best;
    }
    last = fps_key_index(best);   // < N: the key of point 0 is always a candidate, and every candidate index is < N
    if (tid == 0) out[pick] = last;
  }
}

// the sampled correspondences: source = the compacted point, target = the measured depth back-projected at its pixel
__global__ void teaser_gather(const float* __restrict__ pts, const int32_t* __restrict__ pix, const int32_t* __restrict__ idx, const int32_t* __restrict__ m_arr,
                              const float* __restrict__ depth_meas, const int32_t* __restrict__ im_ids, const float* __restrict__ K_rows, int H, int W,
                              int n_points, float* __restrict__ src_s, float* __restrict__ dst_s) {
  const int row = blockIdx.y, k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_points || k >= m_arr[row]) return;
  const size_t px = (size_t)H * W;
  const int i = idx[(size_t)row * n_points + k];   // 0 <= i < N <= px
  const int p = pix[row * px + i];                 // 0 <= p < px
  const float* s = pts + (row * px + i) * 3;
  float d[3];
  backproject(p % W, p / W, depth_meas[(size_t)im_ids[row] * px + p], K_rows + (size_t)row * 9, d);
  for (int c = 0; c < 3; ++c) {
    src_s[((size_t)row * n_points + k) * 3 + c] = s[c];
    dst_s[((size_t)row * n_points + k) * 3 + c] = d[c];
  }
}

// ---- consistency graph ---------------------------------------------------------------------------------------------------------------------
// adj [row][kMaxPoints][kWords]: vertex j sits at bit (j >> 5) of word (j & 31) of every row, so that the 32 lanes of a half-wave read 32
// consecutive points from LDS (12-byte stride: conflict-free) at every step.  A workgroup = 32 vertices x 32 words.
__global__ __launch_bounds__(kThreads) void teaser_graph(const float* __restrict__ src_s, const float* __restrict__ dst_s, int stride,
                                                         const int32_t* __restrict__ m_arr, float noise_bound, uint32_t* __restrict__ adj,
                                                         int32_t* __restrict__ deg) {
  __shared__ float s[kMaxPoints * 3], d[kMaxPoints * 3];
  const int row = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int M = min(m_arr[row], min(stride, kMaxPoints));
  if (tile * 32 >= M) return;
  for (int k = tid; k < M * 3; k += kThreads) {
    s[k] = src_s[(size_t)row * stride * 3 + k];
    d[k] = dst_s[(size_t)row * stride * 3 + k];
  }
  __syncthreads();
  const int w = tid & 31, i = tile * 32 + (tid >> 5);
  uint32_t word = 0u;
  if (i < M) {
    for (int b = 0; b < 32; ++b) {
      const int j = b * 32 + w;
      if (j < M && j != i && edge(s + 3 * i, d + 3 * i, s + 3 * j, d + 3 * j, noise_bound)) word |= 1u << b;
    }
  }
  adj[((size_t)row * kMaxPoints + i) * kWords + w] = word;   // i < kMaxPoints: tile < 32
  int c = __popc(word);
  for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (w == 0 && i < M) deg[(size_t)row * kMaxPoints + i] = c;
}

// ---- k-core peel + ordered list of the selected vertices -----------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void teaser_kcore(const uint32_t* __restrict__ adj, const int32_t* __restrict__ m_arr, int stride, int selection,
                                                         int32_t* __restrict__ core_out, int32_t* __restrict__ sel_out, int32_t* __restrict__ sel_list,
                                                         int32_t* __restrict__ msel) {
  __shared__ unsigned char alive_b[kMaxPoints];
  __shared__ uint32_t alive_w[kWords];
  __shared__ int wave_v[kWaves];
  const int row = blockIdx.x, v = threadIdx.x;
  const int M = min(m_arr[row], min(stride, kMaxPoints));
  uint32_t nb[kWords];
#pragma unroll
  for (int w = 0; w < kWords; ++w) nb[w] = v < M ? adj[((size_t)row * kMaxPoints + v) * kWords + w] : 0u;
  bool alive = v < M;
  int core = 0, k = 0;
  for (int round = 0; round <= kMaxPoints; ++round) {   // (every round with a vertex alive drops at least one)
    alive_b[v] = alive ? 1 : 0;
    __syncthreads();
    if (v < kWords) {
      uint32_t word = 0u;
      for (int b = 0; b < 32; ++b) word |= (uint32_t)alive_b[b * 32 + v] << b;
      alive_w[v] = word;
    }
    __syncthreads();
    int dg = 0x7FFFFFFF;
    if (alive) {
      dg = 0;
#pragma unroll
      for (int w = 0; w < kWords; ++w) dg += __popc(nb[w] & alive_w[w]);
    }
    const int mn = block_min_all<kWaves>(dg, wave_v);
    if (mn == 0x7FFFFFFF) break;   // (uniform: nobody alive)
    k = max(k, mn);
    if (alive && dg <= k) { core = k; alive = false; }
  }
  const bool sel = v < M && (selection == kSelectNone || core == k);
  if (v < M) {
    if (core_out) core_out[(size_t)row * kMaxPoints + v] = core;
    if (sel_out) sel_out[(size_t)row * kMaxPoints + v] = sel ? 1 : 0;
  }
  int total;
  const int pos = block_compact<kWaves>(sel, wave_v, &total);
  if (sel) sel_list[(size_t)row * kMaxPoints + pos] = v;
  if (v == 0) msel[row] = total;
}

// ---- registration --------------------------------------------------------------------------------------------------------------------------
struct CostAt { unsigned long long bits; int e; };   // a translation candidate: the bits of its cost, its interval
struct LowerCostOp {                                  // the lower (cost, e): a total order, no two candidates share an e
  static constexpr bool kFromZero = false;
  __device__ __forceinline__ CostAt operator()(CostAt a, CostAt b) const { return (b.bits < a.bits || (b.bits == a.bits && b.e < a.e)) ? b : a; }
};

__global__ __launch_bounds__(kThreads) void teaser_solve(const float* __restrict__ src_s, const float* __restrict__ dst_s, int stride,
                                                         const int32_t* __restrict__ n_arr, const int32_t* __restrict__ m_arr,
                                                         const int32_t* __restrict__ sel_list, const int32_t* __restrict__ msel, float noise_bound,
                                                         int tim_graph, int min_num_inliers, const float* __restrict__ TCO, float* __restrict__ TCO_out,
                                                         double* __restrict__ Rt_out, int32_t* __restrict__ retval, int32_t* __restrict__ info) {
  __shared__ float ss[kMaxPoints * 3], ds[kMaxPoints * 3];
  __shared__ double x[kMaxPoints], sorted[2 * kMaxPoints];
  __shared__ double red[kWaves], sums[10], tr[3];
  __shared__ CostAt wbest[kWaves];
  __shared__ int wint[kWaves];
  __shared__ GncState g;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int M = max(0, min(m_arr[row], min(stride, kMaxPoints)));
  const int m = min(msel[row], M);
  const float* S = src_s + (size_t)row * stride * 3;
  const float* D = dst_s + (size_t)row * stride * 3;
  if (M < 1 || m < 3) {   // the row keeps its pose
    if (tid == 0) {
      if (TCO_out) for (int k = 0; k < 16; ++k) TCO_out[(size_t)row * 16 + k] = TCO[(size_t)row * 16 + k];
      if (Rt_out) for (int k = 0; k < 12; ++k) Rt_out[(size_t)row * 12 + k] = (k % 5 == 0) ? 1.0 : 0.0;
      retval[row] = -1;
      if (info) {
        int32_t* f = info + (size_t)row * kInfo;
        f[0] = n_arr[row]; f[1] = M; f[2] = m; f[3] = 0; f[4] = 0;
      }
    }
    return;
  }
  for (int k = tid; k < m; k += kThreads) {
    const int c = sel_list[(size_t)row * kMaxPoints + k];   // 0 <= c < M: written by teaser_kcore
    for (int a = 0; a < 3; ++a) { ss[3 * k + a] = S[(size_t)c * 3 + a]; ds[3 * k + a] = D[(size_t)c * 3 + a]; }
  }
  __syncthreads();
  const double beta = (double)noise_bound, beta2 = beta * beta;
  PairAcc acc;
  // ---- rotation ----
  pair_pass(ss, ds, m, tim_graph, tid, kThreads, g.R, 0.0, true, g.R, 0.0, true, beta2, &acc);
  for (int k = 0; k < 9; ++k) {
    const double s = block_sum_all<kWaves>(acc.h[k], red);
    if (tid == 0) sums[k] = s;
  }
  if (tid == 0) gnc_begin(&g, sums);
  __syncthreads();
  pair_pass(ss, ds, m, tim_graph, tid, kThreads, g.R, 0.0, true, g.R, 0.0, false, beta2, &acc);
  {
    const double mx = block_max_all<kWaves>(acc.max_r2, red);
    if (tid == 0) gnc_set_mu(&g, mx, beta2);
  }
  __syncthreads();
  while (!g.stop) {   // (uniform: g changes only between barriers)
    pair_pass(ss, ds, m, tim_graph, tid, kThreads, g.R_prev, g.mu_prev, g.first_w != 0, g.R, g.mu, false, beta2, &acc);
    for (int k = 0; k < 9; ++k) {
      const double s = block_sum_all<kWaves>(acc.h[k], red);
      if (tid == 0) sums[k] = s;
    }
    const double cost = block_sum_all<kWaves>(acc.cost, red);
    __syncthreads();   // (every thread has read g before one lane rewrites it)
    if (tid == 0) gnc_advance(&g, sums, cost);
    __syncthreads();
  }
  // ---- translation ----
  for (int axis = 0; axis < 3; ++axis) {
    for (int k = tid; k < m; k += kThreads)
      x[k] = (double)ds[3 * k + axis] - ((g.R[3 * axis] * (double)ss[3 * k] + g.R[3 * axis + 1] * (double)ss[3 * k + 1]) + g.R[3 * axis + 2] * (double)ss[3 * k + 2]);
    __syncthreads();
    for (int e = tid; e < 2 * m; e += kThreads) sorted[end_rank(x, m, e, beta)] = end_point(x, e, beta);   // a rank is a permutation of 0 .. 2m - 1
    __syncthreads();
    // the lowest (cost, e): costs are non-negative, so they order like their bits
    double est0 = 0.0, est1 = 0.0;
    unsigned long long kb = ~0ull;
    int be = 0x7FFFFFFF;
    if (tid < 2 * m - 1) {
      kb = cost_bits(tls_candidate(x, m, 0.5 * (sorted[tid] + sorted[tid + 1]), beta, &est0));
      be = tid;
    }
    if (tid + kThreads < 2 * m - 1) {
      const int e = tid + kThreads;
      const unsigned long long ob = cost_bits(tls_candidate(x, m, 0.5 * (sorted[e] + sorted[e + 1]), beta, &est1));
      if (ob < kb) { kb = ob; be = e; }
    }
    const int e_win = block_reduce_all<kWaves>(CostAt{kb, be}, wbest, LowerCostOp()).e;
    if (e_win % kThreads == tid) tr[axis] = e_win < kThreads ? est0 : est1;   // e_win <= 2m - 2 < 2 kThreads
    __syncthreads();
  }
  // ---- acceptance ----
  int cnt = 0;
  for (int k = tid; k < M; k += kThreads) cnt += is_inlier(g.R, tr, S + (size_t)k * 3, D + (size_t)k * 3, beta) ? 1 : 0;
  const int n_in = block_sum_all<kWaves>(cnt, wint);
  if (tid == 0) {
    const bool ok = n_in >= min_num_inliers;
    if (TCO_out) {
      if (ok) compose_pose(g.R, tr, TCO + (size_t)row * 16, TCO_out + (size_t)row * 16);
      else for (int k = 0; k < 16; ++k) TCO_out[(size_t)row * 16 + k] = TCO[(size_t)row * 16 + k];
    }
    if (Rt_out)
      for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) Rt_out[(size_t)row * 12 + 4 * r + c] = g.R[3 * r + c];
        Rt_out[(size_t)row * 12 + 4 * r + 3] = tr[r];
      }
    retval[row] = ok ? 0 : -1;
    if (info) {
      int32_t* f = info + (size_t)row * kInfo;
      f[0] = n_arr[row]; f[1] = M; f[2] = m; f[3] = g.iterations; f[4] = n_in;
    }
  }
}

}  // namespace mp

using namespace mp;

namespace {

struct SolveWs {   // the scratch of graph + cores + solve for n rows
  uint32_t* adj;
  int32_t *deg, *core, *sel;   // three adjacent planes [n][kMaxPoints], cleared by one memset up to sel_list
  int32_t *sel_list, *msel, *m_arr, *n_arr;
  CliqueWs clique = {nullptr, nullptr};   // the search stacks of selection 2 (null otherwise)
  SolveWs(WsCarver& c, int n, int stride, int selection) {
    const size_t r = (size_t)n * kMaxPoints;
    adj = c.take<uint32_t>(r * kWords);
    deg = c.take<int32_t>(r);
    core = c.take<int32_t>(r);
    sel = c.take<int32_t>(r);
    sel_list = c.take<int32_t>(r);
    msel = c.take<int32_t>((size_t)n);
    m_arr = c.take<int32_t>((size_t)n);
    n_arr = c.take<int32_t>((size_t)n);
    if (selection == kSelectMaxClique) clique = clique_search_ws(c, n, stride);
  }
};

struct TeaserWs {   // SolveWs, then the samples and the compacted frame of mp_teaser_refine (mp_teaser_solve: a frame of no pixels)
  WsCarver c;
  SolveWs solve;
  float *src_s, *dst_s, *pts, *mind;
  int32_t *idx, *pix;
  size_t total;
  TeaserWs(void* base, int n_rows, int H, int W, int stride, int selection) : c(base), solve(c, n_rows, stride, selection) {
    const size_t px = (size_t)H * W, n = (size_t)n_rows;
    src_s = c.take<float>(n * kMaxPoints * 3);
    dst_s = c.take<float>(n * kMaxPoints * 3);
    idx = c.take<int32_t>(n * kMaxPoints);
    pts = c.take<float>(n * px * 3);
    pix = c.take<int32_t>(n * px);
    mind = c.take<float>(n * px);
    total = c.total(256);
  }
};

bool solve_args_ok(float noise_bound, int selection, int tim_graph, int min_num_inliers, int max_steps) {
  return std::isfinite(noise_bound) && noise_bound > 0.0f && (selection == kSelectKcore || selection == kSelectNone || selection == kSelectMaxClique) &&
         (tim_graph == kTimChain || tim_graph == kTimComplete) && min_num_inliers >= 0 && clique_steps_ok(max_steps);
}

// graph -> cores (-> maximum clique) -> solve on correspondences [n][stride][3] whose counts sit in ws.m_arr; optional [n][stride] copies of the telemetry
int run_solve(const float* src, const float* dst, int n, int stride, const SolveWs& ws, float noise_bound, int selection, int tim_graph,
              int min_num_inliers, int max_steps, const float* TCO, float* TCO_out, double* Rt, int32_t* retval, int32_t* deg, int32_t* core,
              int32_t* sel, int32_t* info, int32_t* clique_info, hipStream_t s) {
  MP_CHECK_HIP(hipMemsetAsync(ws.deg, 0xFF, (char*)ws.sel_list - (char*)ws.deg, s));   // deg, core, sel (adjacent): -1 past a row's M
  hipLaunchKernelGGL(teaser_graph, dim3(kMaxPoints / 32, n), dim3(kThreads), 0, s, src, dst, stride, ws.m_arr, noise_bound, ws.adj, ws.deg);
  hipLaunchKernelGGL(teaser_kcore, dim3(n), dim3(kThreads), 0, s, ws.adj, ws.m_arr, stride, selection, ws.core, ws.sel, ws.sel_list, ws.msel);
  if (selection == kSelectMaxClique) {   // the clique's members replace the vertices of the largest core number in sel, sel_list and msel
    const int rc = clique_search_launch(ws.adj, ws.core, ws.m_arr, n, stride, max_steps, ws.sel, ws.sel_list, ws.msel, clique_info, ws.clique, s);
    if (rc != MP_OK) return rc;
  }
  hipLaunchKernelGGL(teaser_solve, dim3(n), dim3(kThreads), 0, s, src, dst, stride, ws.n_arr, ws.m_arr, ws.sel_list, ws.msel, noise_bound, tim_graph,
                     min_num_inliers, TCO, TCO_out, Rt, retval, info);
  // telemetry [n][stride] from the [n][kMaxPoints] scratch (-1 past a row's M)
  const int32_t* from[3] = {ws.deg, ws.core, ws.sel};
  int32_t* to[3] = {deg, core, sel};
  for (int k = 0; k < 3; ++k)
    if (to[k])
      MP_CHECK_HIP(hipMemcpy2DAsync(to[k], (size_t)stride * 4, from[k], (size_t)kMaxPoints * 4, (size_t)stride * 4, n, hipMemcpyDeviceToDevice, s));
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

}  // namespace

extern "C" size_t mp_fps_workspace_bytes(int n_rows, int stride) {
  if (n_rows < 0 || stride < 1) return 0;
  return align256((size_t)n_rows * stride * 4) + 256;
}

extern "C" int mp_fps(const float* d_points, const int32_t* d_counts, int n_rows, int stride, int n_points, int use_fps, int32_t* d_idx, int32_t* d_m,
                      void* d_ws, size_t ws_bytes, mp_stream stream) {
  MP_REQUIRE(d_points && d_counts && d_idx && d_m && d_ws, "mp_fps: null pointer");
  MP_REQUIRE(n_rows >= 0 && n_rows <= 65535 && stride >= 1 && (long long)stride * 3 < 2147483647LL && n_points >= 1, "mp_fps: bad size");
  MP_REQUIRE(ws_bytes >= mp_fps_workspace_bytes(n_rows, stride), "mp_fps: workspace too small");
  if (n_rows == 0) return MP_OK;
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("fps", 0.0, (double)n_rows * stride * 12.0, s);
  hipLaunchKernelGGL(teaser_fps, dim3(n_rows), dim3(kThreads), 0, s, d_points, stride, d_counts, n_points, 1, use_fps ? 1 : 0, (float*)d_ws, d_idx, d_m);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_teaser_workspace_bytes_ex(int n_rows, int H, int W, int stride, int inlier_selection) {
  if (n_rows < 0 || H < 0 || W < 0 || (long long)H * W * 3 >= 2147483647LL || stride < 1 || stride > kMaxPoints) return 0;
  if (!(inlier_selection == kSelectKcore || inlier_selection == kSelectNone || inlier_selection == kSelectMaxClique)) return 0;
  return TeaserWs(nullptr, n_rows, H, W, stride, inlier_selection).total;
}

extern "C" size_t mp_teaser_workspace_bytes(int n_rows, int H, int W) { return mp_teaser_workspace_bytes_ex(n_rows, H, W, kMaxPoints, kSelectKcore); }

extern "C" int mp_max_clique_default_steps(void) { return kCliqueDefaultSteps; }

extern "C" size_t mp_max_clique_workspace_bytes(int n_rows, int stride) {
  if (n_rows < 0 || stride < 1 || stride > kMaxPoints) return 0;
  WsCarver c(nullptr);
  const SolveWs measured(c, n_rows, stride, kSelectMaxClique);
  return c.total(256);
}

extern "C" int mp_max_clique(const uint8_t* d_adjacency, const int32_t* d_counts, int n_rows, int stride, int max_steps, int32_t* d_members, int32_t* d_info,
                             void* d_ws, size_t ws_bytes, mp_stream stream) {
  MP_REQUIRE(d_adjacency && d_members && d_info && d_ws, "mp_max_clique: null pointer");
  MP_REQUIRE(n_rows >= 0 && n_rows <= 65535 && stride >= 1 && stride <= kMaxPoints, "mp_max_clique: 0 .. 65535 rows of 1 .. 1024 vertices");
  MP_REQUIRE(clique_steps_ok(max_steps), "mp_max_clique: max_steps must be 0 .. 16 x the default budget");
  MP_REQUIRE(ws_bytes >= mp_max_clique_workspace_bytes(n_rows, stride), "mp_max_clique: workspace too small");
  if (n_rows == 0) return MP_OK;
  hipStream_t s = (hipStream_t)stream;
  WsCarver c(d_ws);
  const SolveWs ws(c, n_rows, stride, kSelectMaxClique);
  ProfScope prof("max_clique", 0.0, (double)n_rows * stride * stride, s);
  int rc = clique_pack_launch(d_adjacency, d_counts, n_rows, stride, ws.adj, ws.deg, ws.m_arr, s);
  if (rc != MP_OK) return rc;
  hipLaunchKernelGGL(teaser_kcore, dim3(n_rows), dim3(kThreads), 0, s, ws.adj, ws.m_arr, stride, kSelectKcore, ws.core, ws.sel, ws.sel_list, ws.msel);
  rc = clique_search_launch(ws.adj, ws.core, ws.m_arr, n_rows, stride, max_steps, ws.sel, ws.sel_list, ws.msel, d_info, ws.clique, s);
  if (rc != MP_OK) return rc;
  MP_CHECK_HIP(hipMemcpy2DAsync(d_members, (size_t)stride * 4, ws.sel_list, (size_t)kMaxPoints * 4, (size_t)stride * 4, n_rows, hipMemcpyDeviceToDevice, s));
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_teaser_solve_ex(const float* d_src, const float* d_dst, const int32_t* d_counts, int n_rows, int stride, float noise_bound,
                                  int inlier_selection, int tim_graph, int min_num_inliers, double* d_Rt, int32_t* d_retval, int32_t* d_degree,
                                  int32_t* d_core, int32_t* d_selected, int32_t* d_info, int max_clique_steps, int32_t* d_clique_info, void* d_ws,
                                  size_t ws_bytes, mp_stream stream) {
  MP_REQUIRE(d_src && d_dst && d_counts && d_Rt && d_retval && d_ws, "mp_teaser_solve: null pointer");
  MP_REQUIRE(n_rows >= 0 && n_rows <= 65535 && stride >= 1 && stride <= kMaxPoints, "mp_teaser_solve: 0 .. 65535 rows of 1 .. 1024 correspondences");
  MP_REQUIRE(solve_args_ok(noise_bound, inlier_selection, tim_graph, min_num_inliers, max_clique_steps),
             "mp_teaser_solve: bad noise bound, selection, graph, inlier count or step budget");
  MP_REQUIRE(ws_bytes >= mp_teaser_workspace_bytes_ex(n_rows, 0, 0, stride, inlier_selection), "mp_teaser_solve: workspace too small");
  if (n_rows == 0) return MP_OK;
  hipStream_t s = (hipStream_t)stream;
  const SolveWs ws = TeaserWs(d_ws, n_rows, 0, 0, stride, inlier_selection).solve;
  ProfScope prof("teaser_solve", 0.0, (double)n_rows * stride * 24.0, s);
  MP_CHECK_HIP(hipMemcpyAsync(ws.m_arr, d_counts, (size_t)n_rows * 4, hipMemcpyDeviceToDevice, s));   // (the kernels clamp a count to 0 .. stride)
  MP_CHECK_HIP(hipMemcpyAsync(ws.n_arr, d_counts, (size_t)n_rows * 4, hipMemcpyDeviceToDevice, s));
  return run_solve(d_src, d_dst, n_rows, stride, ws, noise_bound, inlier_selection, tim_graph, min_num_inliers, max_clique_steps, nullptr, nullptr, d_Rt,
                   d_retval, d_degree, d_core, d_selected, d_info, d_clique_info, s);
}

extern "C" int mp_teaser_solve(const float* d_src, const float* d_dst, const int32_t* d_counts, int n_rows, int stride, float noise_bound,
                               int inlier_selection, int tim_graph, int min_num_inliers, double* d_Rt, int32_t* d_retval, int32_t* d_degree,
                               int32_t* d_core, int32_t* d_selected, int32_t* d_info, void* d_ws, size_t ws_bytes, mp_stream stream) {
  return mp_teaser_solve_ex(d_src, d_dst, d_counts, n_rows, stride, noise_bound, inlier_selection, tim_graph, min_num_inliers, d_Rt, d_retval, d_degree, d_core,
                            d_selected, d_info, kCliqueDefaultSteps, nullptr, d_ws, ws_bytes, stream);
}

extern "C" int mp_teaser_refine_ex(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend, const float* d_K_rows,
                                   const float* d_TCO, int n_rows, int H, int W, int mask_type, float depth_delta_thresh, int n_min_points, int n_points,
                                   float noise_bound, int min_num_inliers, int use_fps, int inlier_selection, int tim_graph, float* d_TCO_out,
                                   int32_t* d_retval, double* d_Rt, int32_t* d_sample_idx, int32_t* d_degree, int32_t* d_core, int32_t* d_selected,
                                   int32_t* d_info, int max_clique_steps, int32_t* d_clique_info, void* d_ws, size_t ws_bytes, mp_stream stream) {
  MP_REQUIRE(d_depth_meas && d_im_ids && d_depth_rend && d_K_rows && d_TCO && d_TCO_out && d_retval && d_ws, "mp_teaser_refine: null pointer");
  MP_REQUIRE(n_images > 0 && n_rows >= 0 && n_rows <= 65535 && H >= 1 && W >= 1 && (long long)H * W * 3 < 2147483647LL, "mp_teaser_refine: bad size");
  MP_REQUIRE(n_points >= 1 && n_points <= kMaxPoints, "mp_teaser_refine: n_points must be 1 .. 1024 (the consistency graph is a 1024 x 1024 bit matrix)");
  MP_REQUIRE((mask_type == kMaskSimple || mask_type == kMaskThreshold) && n_min_points >= 0 && std::isfinite(depth_delta_thresh),
             "mp_teaser_refine: bad mask type, threshold or n_min_points");
  MP_REQUIRE(solve_args_ok(noise_bound, inlier_selection, tim_graph, min_num_inliers, max_clique_steps),
             "mp_teaser_refine: bad noise bound, selection, graph, inlier count or step budget");
  MP_REQUIRE(ws_bytes >= mp_teaser_workspace_bytes_ex(n_rows, H, W, n_points, inlier_selection), "mp_teaser_refine: workspace too small");
  if (n_rows == 0) return MP_OK;
  hipStream_t s = (hipStream_t)stream;
  const size_t px = (size_t)H * W, n = (size_t)n_rows;
  const TeaserWs rw(d_ws, n_rows, H, W, n_points, inlier_selection);
  const SolveWs& ws = rw.solve;
  float *src_s = rw.src_s, *dst_s = rw.dst_s, *pts = rw.pts, *mind = rw.mind;
  int32_t *idx = rw.idx, *pix = rw.pix;
  ProfScope prof("teaser_refine", 0.0, (double)n_rows * px * 8.0, s);
  hipLaunchKernelGGL(teaser_compact, dim3(n_rows), dim3(kThreads), 0, s, d_depth_meas, d_im_ids, d_depth_rend, d_K_rows, H, W, mask_type, depth_delta_thresh,
                     pts, pix, ws.n_arr);
  hipLaunchKernelGGL(teaser_fps, dim3(n_rows), dim3(kThreads), 0, s, pts, (int)px, ws.n_arr, n_points, n_min_points, use_fps ? 1 : 0, mind, idx, ws.m_arr);
  hipLaunchKernelGGL(teaser_gather, dim3(ceil_div(n_points, 256), n_rows), dim3(256), 0, s, pts, pix, idx, ws.m_arr, d_depth_meas, d_im_ids, d_K_rows, H, W,
                     n_points, src_s, dst_s);
  if (d_sample_idx) MP_CHECK_HIP(hipMemcpyAsync(d_sample_idx, idx, n * n_points * 4, hipMemcpyDeviceToDevice, s));
  return run_solve(src_s, dst_s, n_rows, n_points, ws, noise_bound, inlier_selection, tim_graph, min_num_inliers, max_clique_steps, d_TCO, d_TCO_out, d_Rt,
                   d_retval, d_degree, d_core, d_selected, d_info, d_clique_info, s);
}

extern "C" int mp_teaser_refine(const float* d_depth_meas, int n_images, const int32_t* d_im_ids, const float* d_depth_rend, const float* d_K_rows,
                                const float* d_TCO, int n_rows, int H, int W, int mask_type, float depth_delta_thresh, int n_min_points, int n_points,
                                float noise_bound, int min_num_inliers, int use_fps, int inlier_selection, int tim_graph, float* d_TCO_out,
                                int32_t* d_retval, double* d_Rt, int32_t* d_sample_idx, int32_t* d_degree, int32_t* d_core, int32_t* d_selected,
                                int32_t* d_info, void* d_ws, size_t ws_bytes, mp_stream stream) {
  return mp_teaser_refine_ex(d_depth_meas, n_images, d_im_ids, d_depth_rend, d_K_rows, d_TCO, n_rows, H, W, mask_type, depth_delta_thresh, n_min_points,
                             n_points, noise_bound, min_num_inliers, use_fps, inlier_selection, tim_graph, d_TCO_out, d_retval, d_Rt, d_sample_idx, d_degree,
                             d_core, d_selected, d_info, kCliqueDefaultSteps, nullptr, d_ws, ws_bytes, stream);
}
