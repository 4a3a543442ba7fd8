// TEST SUPPORT: host emulation of the surface-sampling kernels (megapose6d_amd/csrc/surface_sample.hip), built from the same rules header
// (surface_sample_core.h).  Same arguments as the C ABI, on host arrays: every pass over the jobs of the prefix array one after the
// other (in the order the caller gives, to show that the order does not matter), each job as the workgroup does it but with plain
// loops -- no lanes, no LDS, no shuffles: the sums are integers, so a serial sum is what any scan gives.  Built by
// tests/support/surface_sample.py.
#include <cmath>
#include <cstdint>
#include <vector>

#include "surface_sample_core.h"

using namespace mp;

// job_off [n_obj + 1] = the prefix array of job counts -> the number of jobs, -1 for arguments the launch refuses
extern "C" long long surface_sample_emul_prefix(int n_obj, const int32_t* vert_off, const int32_t* face_off, int count, int block,
                                                int32_t* job_off) {
  if (n_obj < 1 || n_obj > 65535 || count < 1 || !ssamp::block_ok(block) || vert_off[0] != 0 || face_off[0] != 0) return -1;
  const int bs = ssamp::block_of(block);
  long long total = 0;
  job_off[0] = 0;
  for (int o = 0; o < n_obj; ++o) {
    if (vert_off[o + 1] < vert_off[o]) return -1;
    const long long n_faces = (long long)face_off[o + 1] - face_off[o];
    if (!ssamp::faces_ok(n_faces, bs)) return -1;
    total += ssamp::n_blocks((int)n_faces, bs);
    if (total >= ssamp::kMaxJobs) return -1;
    job_off[o + 1] = (int32_t)total;
  }
  return total;
}

// w_out (optional) [F_total] receives the fp32 weights, q_out (optional) [F_total] the quantised ones (0 for a failed object)
extern "C" int surface_sample_emul(const float* vertices, const int32_t* faces, const int32_t* vert_off, const int32_t* face_off, int n_obj,
                                   const float* u, int count, int block_arg, const int64_t* job_order /*a permutation of the jobs, or NULL*/,
                                   float* points, int32_t* face, float* w_out, uint64_t* q_out) {
  std::vector<int32_t> job_off((size_t)n_obj + 1);
  const long long n_jobs = surface_sample_emul_prefix(n_obj, vert_off, face_off, count, block_arg, job_off.data());
  if (n_jobs < 0) return 1;
  const int block = ssamp::block_of(block_arg);
  const size_t f_total = (size_t)face_off[n_obj];
  std::vector<float> w(f_total, NAN), job_max((size_t)n_jobs, NAN);
  std::vector<int32_t> job_bad((size_t)n_jobs, -7), obj_e((size_t)n_obj, 0);
  std::vector<uint64_t> prefix((size_t)n_jobs, ~0ull), C(f_total, ~0ull);
  struct Job {
    int obj, b, n;
    size_t f0;
  };
  auto job_of = [&](long long k) {
    const long long job = job_order ? job_order[k] : k;
    Job j;
    j.obj = 0;
    while (job_off[j.obj + 1] <= job) ++j.obj;
    j.b = (int)(job - job_off[j.obj]);
    const int left = face_off[j.obj + 1] - face_off[j.obj] - j.b * block;
    j.n = left < block ? left : block;
    j.f0 = (size_t)face_off[j.obj] + (size_t)j.b * block;
    return j;
  };
  // the weights pass
  for (long long k = 0; k < n_jobs; ++k) {
    const Job j = job_of(k);
    const int32_t n_vert = vert_off[j.obj + 1] - vert_off[j.obj];
    const float* V = vertices + 3 * (size_t)vert_off[j.obj];
    float mx = 0.0f;
    int bad = 0;
    for (int i = 0; i < j.n; ++i) {
      const size_t f = j.f0 + i;
      const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
      float wf = 0.0f;
      if (!ssamp::face_ok(ia, ib, ic, n_vert)) {
        bad = 1;
      } else {
        const float *a = V + 3 * (size_t)ia, *b = V + 3 * (size_t)ib, *c = V + 3 * (size_t)ic;
        if (!ssamp::finite3(a[0], a[1], a[2]) || !ssamp::finite3(b[0], b[1], b[2]) || !ssamp::finite3(c[0], c[1], c[2])) {
          bad = 1;
        } else {
          wf = ssamp::weight(a, b, c);
          if (!std::isfinite(wf)) {
            bad = 1;
            wf = 0.0f;
          }
        }
      }
      w[f] = wf;
      mx = fmaxf(mx, wf);
    }
    job_max[(size_t)job_off[j.obj] + j.b] = mx;
    job_bad[(size_t)job_off[j.obj] + j.b] = bad;
  }
  // the block-sum pass
  for (long long k = 0; k < n_jobs; ++k) {
    const Job j = job_of(k);
    float wmax = 0.0f;
    int bad = 0;
    for (int p = job_off[j.obj]; p < job_off[j.obj + 1]; ++p) {
      wmax = fmaxf(wmax, job_max[(size_t)p]);
      bad |= job_bad[(size_t)p];
    }
    const bool failed = bad || !(wmax > 0.0f);
    const int e = failed ? ssamp::kFailed : ssamp::exponent_of(wmax);
    uint64_t s = 0;
    if (!failed)
      for (int i = 0; i < j.n; ++i) s += ssamp::quantise(w[j.f0 + i], e);
    prefix[(size_t)job_off[j.obj] + j.b] = s;
    if (j.b == 0) obj_e[(size_t)j.obj] = e;
  }
  // the block-prefix pass
  for (int o = 0; o < n_obj; ++o) {
    uint64_t run = 0;
    for (int p = job_off[o]; p < job_off[o + 1]; ++p) {
      run += prefix[(size_t)p];
      prefix[(size_t)p] = run;
    }
  }
  // the scan pass
  for (long long k = 0; k < n_jobs; ++k) {
    const Job j = job_of(k);
    const int e = obj_e[(size_t)j.obj];
    if (e == ssamp::kFailed) continue;
    uint64_t run = j.b > 0 ? prefix[(size_t)job_off[j.obj] + j.b - 1] : 0ull;
    for (int i = 0; i < j.n; ++i) {
      run += ssamp::quantise(w[j.f0 + i], e);
      C[j.f0 + i] = run;
    }
  }
  // the pick pass
  for (int o = 0; o < n_obj; ++o) {
    const bool failed = obj_e[(size_t)o] == ssamp::kFailed;
    const int n_b = job_off[o + 1] - job_off[o], n_faces = face_off[o + 1] - face_off[o];
    const float* V = vertices + 3 * (size_t)vert_off[o];
    for (int s = 0; s < count; ++s) {
      const size_t row = (size_t)o * count + s;
      if (failed) {
        points[3 * row] = points[3 * row + 1] = points[3 * row + 2] = NAN;
        face[row] = -1;
        continue;
      }
      const uint64_t* P = prefix.data() + job_off[o];
      const uint64_t t = ssamp::pick_t(P[n_b - 1], ssamp::pick_k(u[3 * row]));
      const int bi = ssamp::count_le(P, n_b, t);
      const int base = bi * block, left = n_faces - base;
      const int n = left < block ? left : block;
      const int fi = base + ssamp::count_le(C.data() + face_off[o] + base, n, t);
      const size_t f = (size_t)face_off[o] + fi;
      const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
      float r1, r2;
      ssamp::barycentric(u[3 * row + 1], u[3 * row + 2], &r1, &r2);
      for (int a = 0; a < 3; ++a)
        points[3 * row + a] = ssamp::point_axis(V[3 * (size_t)ia + a], V[3 * (size_t)ib + a], V[3 * (size_t)ic + a], r1, r2);
      face[row] = fi;
    }
  }
  for (int o = 0; o < n_obj; ++o)
    for (int f = face_off[o]; f < face_off[o + 1]; ++f) {
      if (w_out) w_out[f] = w[(size_t)f];
      if (q_out) q_out[f] = obj_e[(size_t)o] == ssamp::kFailed ? 0ull : ssamp::quantise(w[(size_t)f], obj_e[(size_t)o]);
    }
  return 0;
}

extern "C" void surface_sample_emul_limits(int* v) {
  v[0] = ssamp::kBlockStep;
  v[1] = ssamp::kMaxBlock;
  v[2] = ssamp::kDefaultBlock;
  v[3] = ssamp::kMaxBlocks;
  v[4] = ssamp::kMaxFaces;
}
