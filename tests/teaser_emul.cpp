// TEST SUPPORT: host emulation of the TEASER++ refiner kernels (megapose6d_amd/csrc/teaser.hip), built from the same rules header
// (teaser_core.h).  Same arguments as the C ABI, on host arrays, one row after the other, each step as the workgroup does it but with
// plain loops -- no lanes, no LDS, no shuffles -- except where the order of a float64 sum is part of the contract: there the shares of
// the kThreads threads are formed one by one and added in the kernel's tree (tree_sum).  Built by tests/support/teaser.py.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "teaser_core.h"

using namespace mp::teaser;

namespace {

// the kernel's block_sum: a butterfly over the 64 lanes of every wave (xor 32 .. 1), then the waves in ascending order
double tree_sum(const std::vector<double>& part) {
  double s = 0.0;
  for (int w = 0; w < kWaves; ++w) {
    double v[64], n[64];
    for (int l = 0; l < 64; ++l) v[l] = part[(size_t)w * 64 + l];
    for (int off = 32; off > 0; off >>= 1) {
      for (int l = 0; l < 64; ++l) n[l] = v[l] + v[l ^ off];
      std::memcpy(v, n, sizeof v);
    }
    s += v[0];
  }
  return s;
}

void fps_row(const float* P, int N, int M, int use_fps, int n_points, int32_t* out) {
  for (int k = 0; k < n_points; ++k) out[k] = -1;
  if (M < 1) return;
  if (!use_fps) {
    for (int k = 0; k < M; ++k) out[k] = stride_pick(k, N, M);
    return;
  }
  std::vector<float> mn((size_t)N, INFINITY);
  int last = 0;
  out[0] = 0;
  for (int pick = 1; pick < M; ++pick) {
    uint64_t best = 0;
    for (int i = 0; i < N; ++i) {
      const float d = dist2(P + 3 * (size_t)i, P + 3 * (size_t)last);
      if (d < mn[i]) mn[i] = d;
      const uint64_t key = fps_key(mn[i], i);
      best = key > best ? key : best;
    }
    last = fps_key_index(best);
    out[pick] = last;
  }
}

// dense adjacency [M][M] of the sampled correspondences
void graph_row(const float* S, const float* D, int M, float noise_bound, std::vector<uint8_t>& adj) {
  adj.assign((size_t)M * M, 0);
  for (int i = 0; i < M; ++i)
    for (int j = 0; j < M; ++j)
      adj[(size_t)i * M + j] = (i != j && edge(S + 3 * i, D + 3 * i, S + 3 * j, D + 3 * j, noise_bound)) ? 1 : 0;
}

// the kernel's peel: rounds of (smallest alive degree, k = max, drop everything at or below k, recount) -> core numbers, the last k
int cores_of(const uint8_t* adj, int M, int32_t* core) {
  std::vector<char> alive((size_t)M, 1);
  std::vector<int> dg((size_t)M);
  int k = 0;
  for (;;) {
    int mn = 0x7FFFFFFF;
    for (int v = 0; v < M; ++v) {
      if (!alive[v]) continue;
      int d = 0;
      for (int j = 0; j < M; ++j) d += (adj[(size_t)v * M + j] && alive[j]) ? 1 : 0;
      dg[v] = d;
      mn = d < mn ? d : mn;
    }
    if (mn == 0x7FFFFFFF) break;
    k = mn > k ? mn : k;
    for (int v = 0; v < M; ++v)
      if (alive[v] && dg[v] <= k) { core[v] = k; alive[v] = 0; }
  }
  return k;
}

struct RowOut {
  double Rt[12];
  int retval, m, iters, n_in;
  bool accepted;
};

void solve_row(const float* S, const float* D, int M, int stride, float noise_bound, int selection, int tim_graph, int min_num_inliers, int32_t* deg, int32_t* core_o,
               int32_t* sel_o, RowOut* o) {
  for (int k = 0; k < 12; ++k) o->Rt[k] = (k % 5 == 0) ? 1.0 : 0.0;
  o->retval = -1; o->m = 0; o->iters = 0; o->n_in = 0; o->accepted = false;
  if (M < 0) M = 0;
  std::vector<uint8_t> adj;
  graph_row(S, D, M, noise_bound, adj);
  std::vector<int32_t> core((size_t)M, 0);
  const int kmax = cores_of(adj.data(), M, core.data());
  std::vector<int> c;
  for (int v = 0; v < M; ++v) {
    const bool sel = selection == kSelectNone || core[v] == kmax;
    if (sel) c.push_back(v);
    if (deg) { int d = 0; for (int j = 0; j < M; ++j) d += adj[(size_t)v * M + j]; deg[v] = d; }
    if (core_o) core_o[v] = core[v];
    if (sel_o) sel_o[v] = sel ? 1 : 0;
  }
  for (int v = M; v < stride; ++v) {
    if (deg) deg[v] = -1;
    if (core_o) core_o[v] = -1;
    if (sel_o) sel_o[v] = -1;
  }
  const int m = (int)c.size();
  o->m = m;
  if (M < 1 || m < 3) return;
  std::vector<float> ss((size_t)m * 3), ds((size_t)m * 3);
  for (int k = 0; k < m; ++k)
    for (int a = 0; a < 3; ++a) { ss[3 * k + a] = S[3 * c[k] + a]; ds[3 * k + a] = D[3 * c[k] + a]; }
  const double beta = (double)noise_bound, beta2 = beta * beta;
  GncState g;
  std::memset(&g, 0, sizeof g);
  std::vector<PairAcc> acc(kThreads);
  std::vector<double> part(kThreads);
  auto sum_of = [&](int slot) {   // slot 0 .. 8 = h, 9 = cost
    for (int t = 0; t < kThreads; ++t) part[t] = slot < 9 ? acc[t].h[slot] : acc[t].cost;
    return tree_sum(part);
  };
  double sums[9];
  for (int t = 0; t < kThreads; ++t) pair_pass(ss.data(), ds.data(), m, tim_graph, t, kThreads, g.R, 0.0, true, g.R, 0.0, true, beta2, &acc[t]);
  for (int k = 0; k < 9; ++k) sums[k] = sum_of(k);
  gnc_begin(&g, sums);
  for (int t = 0; t < kThreads; ++t) pair_pass(ss.data(), ds.data(), m, tim_graph, t, kThreads, g.R, 0.0, true, g.R, 0.0, false, beta2, &acc[t]);
  double mx = 0.0;
  for (int t = 0; t < kThreads; ++t) mx = fmax(mx, acc[t].max_r2);
  gnc_set_mu(&g, mx, beta2);
  while (!g.stop) {
    for (int t = 0; t < kThreads; ++t)
      pair_pass(ss.data(), ds.data(), m, tim_graph, t, kThreads, g.R_prev, g.mu_prev, g.first_w != 0, g.R, g.mu, false, beta2, &acc[t]);
    for (int k = 0; k < 9; ++k) sums[k] = sum_of(k);
    const double cost = sum_of(9);
    gnc_advance(&g, sums, cost);
  }
  double tr[3];
  std::vector<double> x((size_t)m), sorted((size_t)2 * m);
  for (int axis = 0; axis < 3; ++axis) {
    for (int k = 0; k < m; ++k)
      x[k] = (double)ds[3 * k + axis] - ((g.R[3 * axis] * (double)ss[3 * k] + g.R[3 * axis + 1] * (double)ss[3 * k + 1]) + g.R[3 * axis + 2] * (double)ss[3 * k + 2]);
    for (int e = 0; e < 2 * m; ++e) sorted[end_rank(x.data(), m, e, beta)] = end_point(x.data(), e, beta);
    uint64_t kb = ~0ull;
    double best_est = 0.0;
    for (int e = 0; e < 2 * m - 1; ++e) {   // ascending e and a strict <: a tie stays with the lowest e
      double est;
      const uint64_t b = cost_bits(tls_candidate(x.data(), m, 0.5 * (sorted[e] + sorted[e + 1]), beta, &est));
      if (e == 0 || b < kb) { kb = b; best_est = est; }
    }
    tr[axis] = best_est;
  }
  int n_in = 0;
  for (int k = 0; k < M; ++k) n_in += is_inlier(g.R, tr, S + 3 * k, D + 3 * k, beta) ? 1 : 0;
  for (int r = 0; r < 3; ++r) {
    for (int cc = 0; cc < 3; ++cc) o->Rt[4 * r + cc] = g.R[3 * r + cc];
    o->Rt[4 * r + 3] = tr[r];
  }
  o->iters = g.iterations;
  o->n_in = n_in;
  o->accepted = n_in >= min_num_inliers;
  o->retval = o->accepted ? 0 : -1;
}

bool solve_args_ok(float noise_bound, int selection, int tim_graph, int min_num_inliers) {
  return std::isfinite(noise_bound) && noise_bound > 0.0f && (selection == kSelectKcore || selection == kSelectNone) &&
         (tim_graph == kTimChain || tim_graph == kTimComplete) && min_num_inliers >= 0;
}

}  // namespace

extern "C" void teaser_emul_limits(int* v) {
  v[0] = kThreads;
  v[1] = kMaxPoints;
  v[2] = kFpsResident;
  v[3] = kGncMaxIter;
  v[4] = kInfo;
}

extern "C" int teaser_emul_fps(const float* points, const int32_t* counts, int n_rows, int stride, int n_points, int use_fps, int32_t* idx, int32_t* m_out) {
  if (n_rows < 0 || n_rows > 65535 || stride < 1 || n_points < 1) return 1;
  for (int r = 0; r < n_rows; ++r) {
    const int N = counts[r] < 0 ? 0 : (counts[r] > stride ? stride : counts[r]);
    const int M = n_samples(N, n_points, 1);
    m_out[r] = M;
    fps_row(points + (size_t)r * stride * 3, N, M, use_fps, n_points, idx + (size_t)r * n_points);
  }
  return 0;
}

// dense adjacency [M][M] uint8 of one row's correspondences
extern "C" void teaser_emul_graph(const float* src, const float* dst, int M, float noise_bound, uint8_t* adj_out) {
  std::vector<uint8_t> adj;
  graph_row(src, dst, M, noise_bound, adj);
  std::memcpy(adj_out, adj.data(), adj.size());
}

// core numbers of a given dense adjacency -> the largest
extern "C" int teaser_emul_cores(const uint8_t* adj, int M, int32_t* core) { return cores_of(adj, M, core); }

extern "C" int teaser_emul_solve(const float* src, const float* dst, const int32_t* counts, int n_rows, int stride, float noise_bound, int selection,
                                 int tim_graph, int min_num_inliers, double* Rt, int32_t* retval, int32_t* degree, int32_t* core, int32_t* selected,
                                 int32_t* info) {
  if (n_rows < 0 || n_rows > 65535 || stride < 1 || stride > kMaxPoints || !solve_args_ok(noise_bound, selection, tim_graph, min_num_inliers)) return 1;
  for (int r = 0; r < n_rows; ++r) {
    const int M = counts[r] < 0 ? 0 : (counts[r] < stride ? counts[r] : stride);
    RowOut o;
    const size_t q = (size_t)r * stride;
    solve_row(src + q * 3, dst + q * 3, M, stride, noise_bound, selection, tim_graph, min_num_inliers, degree ? degree + q : nullptr, core ? core + q : nullptr,
              selected ? selected + q : nullptr, &o);
    std::memcpy(Rt + (size_t)r * 12, o.Rt, sizeof o.Rt);
    retval[r] = o.retval;
    if (info) { int32_t* f = info + (size_t)r * kInfo; f[0] = counts[r]; f[1] = M; f[2] = o.m; f[3] = o.iters; f[4] = o.n_in; }
  }
  return 0;
}

extern "C" int teaser_emul_refine(const float* depth_meas, int n_images, const int32_t* im_ids, const float* depth_rend, const float* K_rows, const float* TCO,
                                  int n_rows, int H, int W, int mask_type, float thresh, int n_min_points, int n_points, float noise_bound,
                                  int min_num_inliers, int use_fps, int selection, int tim_graph, float* TCO_out, int32_t* retval, double* Rt,
                                  int32_t* sample_idx, int32_t* degree, int32_t* core, int32_t* selected, int32_t* info) {
  if (n_images < 1 || n_rows < 0 || n_rows > 65535 || H < 1 || W < 1 || n_points < 1 || n_points > kMaxPoints || n_min_points < 0 ||
      !(mask_type == kMaskSimple || mask_type == kMaskThreshold) || !std::isfinite(thresh) || !solve_args_ok(noise_bound, selection, tim_graph, min_num_inliers))
    return 1;
  const size_t px = (size_t)H * W;
  for (int r = 0; r < n_rows; ++r) {
    const float *dm = depth_meas + (size_t)im_ids[r] * px, *dr = depth_rend + (size_t)r * px, *K = K_rows + (size_t)r * 9;
    std::vector<float> pts;
    std::vector<int> pix;
    for (size_t i = 0; i < px; ++i)
      if (mask_pixel(dm[i], dr[i], mask_type, thresh)) {
        float p[3];
        backproject((int)(i % W), (int)(i / W), dr[i], K, p);
        pts.insert(pts.end(), p, p + 3);
        pix.push_back((int)i);
      }
    const int N = (int)pix.size(), M = n_samples(N, n_points, n_min_points);
    std::vector<int32_t> idx((size_t)n_points);
    fps_row(pts.data(), N, M, use_fps, n_points, idx.data());
    std::vector<float> S((size_t)n_points * 3, 0.0f), D((size_t)n_points * 3, 0.0f);
    for (int k = 0; k < M; ++k) {
      const int i = idx[k], p = pix[i];
      for (int a = 0; a < 3; ++a) S[3 * k + a] = pts[3 * (size_t)i + a];
      backproject(p % W, p / W, dm[p], K, &D[3 * k]);
    }
    RowOut o;
    const size_t q = (size_t)r * n_points;
    solve_row(S.data(), D.data(), M, n_points, noise_bound, selection, tim_graph, min_num_inliers, degree ? degree + q : nullptr, core ? core + q : nullptr,
              selected ? selected + q : nullptr, &o);
    if (o.accepted) {
      const double R9[9] = {o.Rt[0], o.Rt[1], o.Rt[2], o.Rt[4], o.Rt[5], o.Rt[6], o.Rt[8], o.Rt[9], o.Rt[10]}, t3[3] = {o.Rt[3], o.Rt[7], o.Rt[11]};
      compose_pose(R9, t3, TCO + (size_t)r * 16, TCO_out + (size_t)r * 16);
    } else std::memcpy(TCO_out + (size_t)r * 16, TCO + (size_t)r * 16, 16 * sizeof(float));
    retval[r] = o.retval;
    if (Rt) std::memcpy(Rt + (size_t)r * 12, o.Rt, sizeof o.Rt);
    if (sample_idx) std::memcpy(sample_idx + q, idx.data(), (size_t)n_points * 4);
    if (info) { int32_t* f = info + (size_t)r * kInfo; f[0] = N; f[1] = M; f[2] = o.m; f[3] = o.iters; f[4] = o.n_in; }
  }
  return 0;
}
