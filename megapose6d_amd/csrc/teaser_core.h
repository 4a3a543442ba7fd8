// teaser_core.h -- the rules of the TEASER++ depth refiner (the reference's inference/teaserpp_refiner.py: correspondences from a rendered
// and a measured depth frame, pytorch3d's farthest point sampling, TEASER++'s robust registration) that run on the device (teaser.hip),
// shared with the host emulation (tests/teaser_emul.cpp) the way surface_sample_core.h is shared with its own.  Every fmaf is spelled
// out; both builds use -ffp-contract=off; the only library calls are sqrtf / sqrt / fabs, correctly rounded on both sides.
//
// CONTRACT
//   * MASK [mask_pixel].  A pixel is used when measured > 0 && rendered > 0 (refiner_utils.compute_masks, "simple"); with mask type
//     "threshold" also !(|measured - rendered| > depth_delta_thresh).  N = the number of such pixels, in row-major order.
//   * POINTS [backproject].  x = (u - cx) * (d / fx), y = (v - cy) * (d / fy), z = d in fp32 (meshcat_utils.get_pointcloud), with the
//     row's K.  Source = the rendered depth, target = the measured depth at the same pixel.  A row with N < n_min_points keeps its pose.
//   * SAMPLING [dist2, fps_key].  M = min(n_points, N) picks on the source points: pick 0 is point 0, every later pick the point with the
//     largest running minimum of dist2 to the picks so far, dist2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)); a tie goes to the lowest index
//     (the maximum of the packed key (bits of the minimum << 32 | ~index): non-negative fp32 orders like its bits).  The minimum is only
//     ever lowered by `d < min`, so a NaN distance never enters it.  Without farthest point sampling: index floor(k * N / M) [stride_pick].
//   * GRAPH [edge].  Vertices = the M sampled correspondences; edge (i, j), i != j, when |‖s_j - s_i‖ - ‖d_j - d_i‖| <= 2 * noise_bound
//     in fp32, the norms sqrtf(dist2): symmetric bit for bit, because a difference and its negative square alike.
//   * CORES.  k = 0; until no vertex is alive: d = the smallest alive degree, k = max(k, d), every alive vertex of degree <= k gets core
//     number k and is dropped, degrees are recounted.  Core numbers are unique, so no order changes them.  Selected = the vertices whose
//     core number is the largest (mode "none": every vertex; mode "max_clique": the members of a maximum clique, by the rule of
//     teaser_clique_core.h), m of them, in ascending order c_0 .. c_{m-1}; m < 3 rejects the row.
//   * ROTATION (GNC-TLS) [PairAcc, pair_pass, rotation_of, gnc_weight].  Float64.  The TIMs are a = s_q - s_p, b = d_q - d_p over the pairs
//     (p, q) = (c_k, c_{k+1}) (graph "chain") or all p < q (graph "complete").  beta = noise_bound; weights start at 1.  Iteration i:
//     R_i = the rotation that maximises trace(R sum w a b^T) (the weighted Kabsch solution with the determinant fixed, here in Horn's
//     quaternion form: the eigenvector of the largest eigenvalue of a symmetric 4x4 matrix, by cyclic Jacobi sweeps [rotation_of]);
//     r2 = ‖b - R_i a‖^2; at i = 0: mu = 1 / (2 max r2 / beta^2 - 1), stop if mu <= 0; cost = sum w r2 with the weights R_i was solved
//     with; then w = 0 if r2 >= (mu + 1) / mu beta^2, 1 if r2 <= mu / (mu + 1) beta^2, else sqrt(beta^2 mu (mu + 1) / r2) - mu; stop if
//     |cost - previous cost| < 1e-12 (the previous cost of iteration 0 is infinite), else mu *= 1.4; at most 100 iterations.  A weight
//     is never stored: it is a function of r2 under the rotation and mu of the iteration before, and is recomputed [pair_pass].
//     Sums: thread t of kThreads adds its pairs in ascending order [for_pairs], the 64 lanes of a wave add in a butterfly (xor 32, 16, ..
//     1), the 16 waves in ascending order [the emulation's tree_sum, the kernel's block_sum].
//   * TRANSLATION [tls_1d].  Per axis: x_k = d_k - (R s_k) (float64) over the selected vertices, beta = noise_bound; the 2m end points
//     x_k -/+ beta sorted (ties by their index 2k, 2k + 1); candidate c_e = the midpoint of sorted entries e, e + 1; consensus set
//     |x_k - c| <= beta; x^ = its mean (summed in ascending k); cost = sum min((x_k - x^)^2, beta^2) (ascending k); an empty consensus set
//     costs infinity; the lowest cost wins, a tie goes to the lowest e.
//   * ACCEPT.  num_inliers = #{k < M : sqrt(‖R s_k + t - d_k‖^2) < noise_bound} (float64) over ALL sampled correspondences; when
//     num_inliers >= min_num_inliers the row's pose becomes [R t] * TCO (float64 products, summed left to right, rounded to fp32) and
//     retval = 0; else the input pose is kept and retval = -1.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define TSR_HD __host__ __device__ __forceinline__
#else
#define TSR_HD inline
#endif

namespace mp {
namespace teaser {

constexpr int kThreads = 1024;                     // lanes of a workgroup of the per-row kernels
constexpr int kWaves = kThreads / 64;
constexpr int kMaxPoints = 1024;                   // n_points, at most: a 1024 x 1024 bit matrix per row
constexpr int kWords = kMaxPoints / 32;            // 32-bit words of one row of the bit matrix
constexpr int kFpsReg = 16;                        // points a thread of the sampling kernel keeps in registers
constexpr int kFpsResident = kFpsReg * kThreads;   // ... so this many points of a row are register-resident, the rest is streamed
constexpr int kGncMaxIter = 100;
constexpr double kGncFactor = 1.4;
constexpr double kGncCostThreshold = 1e-12;
constexpr int kJacobiSweeps = 12;                  // cyclic sweeps of the 4x4 eigen solve (quadratic convergence: 6 reach 1e-16)
constexpr int kInfo = 5;                           // per-row info: N, M, m, GNC iterations, num_inliers

enum { kMaskSimple = 0, kMaskThreshold = 1 };
enum { kSelectKcore = 0, kSelectNone = 1 };
enum { kTimChain = 0, kTimComplete = 1 };

TSR_HD bool mask_pixel(float meas, float rend, int mask_type, float thresh) {
  if (!(meas > 0.0f && rend > 0.0f)) return false;
  return mask_type == kMaskSimple || !(fabsf(meas - rend) > thresh);
}

TSR_HD void backproject(int u, int v, float d, const float* K, float* p) {
  p[0] = ((float)u - K[2]) * (d / K[0]);
  p[1] = ((float)v - K[5]) * (d / K[4]);
  p[2] = d;
}

TSR_HD float dist2(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

TSR_HD uint32_t f32_bits(float v) {
  union { float f; uint32_t u; } c;
  c.f = v;
  return c.u;
}

// the larger key = the larger minimum, then the lower index
TSR_HD uint64_t fps_key(float min_d, int index) { return ((uint64_t)f32_bits(min_d) << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)index); }

TSR_HD int fps_key_index(uint64_t key) { return (int)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull)); }

TSR_HD int n_samples(int N, int n_points, int n_min_points) { return N < n_min_points || N < 1 ? 0 : (n_points < N ? n_points : N); }

TSR_HD int stride_pick(int k, int N, int M) { return (int)(((long long)k * N) / M); }

TSR_HD bool edge(const float* si, const float* di, const float* sj, const float* dj, float noise_bound) {
  return fabsf(sqrtf(dist2(sj, si)) - sqrtf(dist2(dj, di))) <= 2.0f * noise_bound;
}

// ---- rotation -------------------------------------------------------------------------------------------------------------------------
struct PairAcc {
  double h[9];      // sum w_new a b^T (row-major: h[3 r + c] = a_r b_c)
  double cost;      // sum w_old r2
  double max_r2;    // max r2 (a maximum is order-free)
};

TSR_HD double gnc_weight(double r2, double mu, double beta2) {
  if (r2 >= (mu + 1.0) / mu * beta2) return 0.0;
  if (r2 <= mu / (mu + 1.0) * beta2) return 1.0;
  return sqrt(beta2 * mu * (mu + 1.0) / r2) - mu;
}

TSR_HD double residual2(const double* R, const double* a, const double* b) {
  double s = 0.0;
  for (int r = 0; r < 3; ++r) {
    const double e = b[r] - ((R[3 * r] * a[0] + R[3 * r + 1] * a[1]) + R[3 * r + 2] * a[2]);
    s += e * e;
  }
  return s;
}

// the pairs of thread t of T, in the order it adds them
template <class F>
TSR_HD void for_pairs(int graph, int m, int t, int T, F f) {
  if (graph == kTimChain) {
    for (int k = t; k < m - 1; k += T) f(k, k + 1);
  } else {
    for (int p = 0; p < m - 1; ++p)
      for (int q = p + 1 + t; q < m; q += T) f(p, q);
  }
}

// One thread's share of one pass over the TIMs.  src / dst: the selected points [m][3] fp32.  R_cur = this iteration's rotation; the
// weights it was solved with are those of (R_prev, mu_prev) -- or all 1 when first_w -- and give the cost; the new weights under
// (R_cur, mu_cur) give h -- or all 1 when unit_new (the pass that only seeds the first rotation, and the pass that finds max r2).
TSR_HD void pair_pass(const float* src, const float* dst, int m, int graph, int t, int T, const double* R_prev, double mu_prev, bool first_w,
                      const double* R_cur, double mu_cur, bool unit_new, double beta2, PairAcc* acc) {
  for (int k = 0; k < 9; ++k) acc->h[k] = 0.0;
  acc->cost = 0.0;
  acc->max_r2 = 0.0;
  for_pairs(graph, m, t, T, [&](int p, int q) {
    double a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = (double)src[3 * q + k] - (double)src[3 * p + k];
      b[k] = (double)dst[3 * q + k] - (double)dst[3 * p + k];
    }
    double w_new = 1.0;
    if (!unit_new) {
      const double r2 = residual2(R_cur, a, b);
      const double w_old = first_w ? 1.0 : gnc_weight(residual2(R_prev, a, b), mu_prev, beta2);
      acc->cost += w_old * r2;
      acc->max_r2 = r2 > acc->max_r2 ? r2 : acc->max_r2;
      w_new = mu_cur > 0.0 ? gnc_weight(r2, mu_cur, beta2) : 1.0;
    }
    for (int r = 0; r < 3; ++r)
      for (int c = 0; c < 3; ++c) acc->h[3 * r + c] += w_new * (a[r] * b[c]);
  });
}

// R (row-major) maximising trace(R H), H = sum w a b^T: Horn's N matrix, its dominant eigenvector by cyclic Jacobi, the quaternion's
// rotation.  H = 0 gives the identity.
TSR_HD void rotation_of(const double* H, double* R) {
  // (Horn 1987: S = sum a b^T with R a ~ b)
  const double Sxx = H[0], Sxy = H[1], Sxz = H[2], Syx = H[3], Syy = H[4], Syz = H[5], Szx = H[6], Szy = H[7], Szz = H[8];
  double A[4][4] = {{(Sxx + Syy) + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                    {Syz - Szy, (Sxx - Syy) - Szz, Sxy + Syx, Szx + Sxz},
                    {Szx - Sxz, Sxy + Syx, (Syy - Sxx) - Szz, Syz + Szy},
                    {Sxy - Syx, Szx + Sxz, Syz + Szy, (Szz - Sxx) - Syy}};
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep)
    for (int p = 0; p < 3; ++p)
      for (int q = p + 1; q < 4; ++q) {
        const double apq = A[p][q];
        if (apq == 0.0) continue;
        const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
        for (int k = 0; k < 4; ++k) {   // A <- A J (columns p, q)
          const double akp = A[k][p], akq = A[k][q];
          A[k][p] = c * akp - s * akq;
          A[k][q] = s * akp + c * akq;
        }
        for (int k = 0; k < 4; ++k) {   // A <- J^T A (rows p, q)
          const double apk = A[p][k], aqk = A[q][k];
          A[p][k] = c * apk - s * aqk;
          A[q][k] = s * apk + c * aqk;
        }
        A[p][q] = 0.0;
        A[q][p] = 0.0;
        for (int k = 0; k < 4; ++k) {
          const double vkp = V[k][p], vkq = V[k][q];
          V[k][p] = c * vkp - s * vkq;
          V[k][q] = s * vkp + c * vkq;
        }
      }
  int best = 0;
  for (int k = 1; k < 4; ++k)
    if (A[k][k] > A[best][best]) best = k;
  double w = V[0][best], x = V[1][best], y = V[2][best], z = V[3][best];
  const double n = sqrt(((w * w + x * x) + y * y) + z * z);
  w /= n; x /= n; y /= n; z /= n;
  R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - z * w);       R[2] = 2.0 * (x * z + y * w);
  R[3] = 2.0 * (x * y + z * w);       R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - x * w);
  R[6] = 2.0 * (x * z - y * w);       R[7] = 2.0 * (y * z + x * w);       R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// loop state of the GNC iterations of one row, advanced by one lane between the passes
struct GncState {
  double R[9], R_prev[9];
  double mu, mu_prev, prev_cost;
  int iterations;     // rotations solved and scored
  int first_w;        // the weights R was solved with are all 1
  int stop;
};

TSR_HD void gnc_begin(GncState* g, const double* sums /*h of the seeding pass*/) {
  rotation_of(sums, g->R);
  for (int k = 0; k < 9; ++k) g->R_prev[k] = g->R[k];
  g->mu = 0.0;
  g->mu_prev = 0.0;
  g->prev_cost = INFINITY;
  g->iterations = 0;
  g->first_w = 1;
  g->stop = 0;
}

// after the pass that found max r2 under the first rotation: mu of iteration 0
TSR_HD void gnc_set_mu(GncState* g, double max_r2, double beta2) {
  g->mu = 1.0 / (2.0 * max_r2 / beta2 - 1.0);
  if (!(g->mu > 0.0)) g->stop = 1;   // (also a NaN: every residual zero and beta zero)
}

// after a full pass under (R, mu): cost test, mu *= 1.4, the next rotation from the new weights
TSR_HD void gnc_advance(GncState* g, const double* h, double cost) {
  g->iterations += 1;
  const double diff = fabs(cost - g->prev_cost);
  g->prev_cost = cost;
  if (diff < kGncCostThreshold || g->iterations >= kGncMaxIter) {
    g->stop = 1;
    return;
  }
  for (int k = 0; k < 9; ++k) g->R_prev[k] = g->R[k];
  g->mu_prev = g->mu;
  g->first_w = 0;
  g->mu *= kGncFactor;
  rotation_of(h, g->R);
}

// ---- translation ------------------------------------------------------------------------------------------------------------------------
// end point e of 2m: e = 2k -> x_k - beta, e = 2k + 1 -> x_k + beta
TSR_HD double end_point(const double* x, int e, double beta) { return (e & 1) ? x[e >> 1] + beta : x[e >> 1] - beta; }

// the position of end point e in the sorted order (ties by e): a rank, so any order of counting gives it
TSR_HD int end_rank(const double* x, int m, int e, double beta) {
  const double v = end_point(x, e, beta);
  int r = 0;
  for (int f = 0; f < 2 * m; ++f) {
    const double u = end_point(x, f, beta);
    r += (u < v || (u == v && f < e)) ? 1 : 0;
  }
  return r;
}

// the cost and estimate of candidate c over the m values
TSR_HD double tls_candidate(const double* x, int m, double c, double beta, double* est) {
  double s = 0.0;
  int n = 0;
  for (int k = 0; k < m; ++k)
    if (fabs(x[k] - c) <= beta) { s += x[k]; ++n; }
  if (n == 0) { *est = c; return INFINITY; }
  const double xh = s / (double)n;
  const double b2 = beta * beta;
  double cost = 0.0;
  for (int k = 0; k < m; ++k) {
    const double e = x[k] - xh, e2 = e * e;
    cost += e2 < b2 ? e2 : b2;
  }
  *est = xh;
  return cost;
}

// a cost is non-negative, so costs order like their bits; the winner is the lowest (cost_bits, e)
TSR_HD uint64_t cost_bits(double cost) {
  union { double d; uint64_t u; } c;
  c.d = cost;
  return c.u;
}

// ---- acceptance -------------------------------------------------------------------------------------------------------------------------
TSR_HD bool is_inlier(const double* R, const double* t, const float* s, const float* d, double beta) {
  double n2 = 0.0;
  for (int r = 0; r < 3; ++r) {
    const double e = (((R[3 * r] * (double)s[0] + R[3 * r + 1] * (double)s[1]) + R[3 * r + 2] * (double)s[2]) + t[r]) - (double)d[r];
    n2 += e * e;
  }
  return sqrt(n2) < beta;
}

// out = [R t; 0 0 0 1] * TCO, rounded to fp32
TSR_HD void compose_pose(const double* R, const double* t, const float* TCO, float* out) {
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 4; ++c) {
      double s = (R[3 * r] * (double)TCO[c] + R[3 * r + 1] * (double)TCO[4 + c]) + R[3 * r + 2] * (double)TCO[8 + c];
      s += t[r] * (double)TCO[12 + c];
      out[4 * r + c] = (float)s;
    }
  for (int c = 0; c < 4; ++c) out[12 + c] = TCO[12 + c];
}

}  // namespace teaser
}  // namespace mp
