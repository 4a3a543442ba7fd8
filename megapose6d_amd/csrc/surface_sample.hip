// surface_sample.hip -- points drawn uniformly over the surface of triangle meshes, several objects in one launch: a face with
// probability proportional to its area, then a point uniform in that face (trimesh.sample.sample_surface, what the reference's
// MeshDataBase.batched(resample_n_points=n) calls), on uniforms the caller supplies.
//
// The rules are surface_sample_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Weights are
// quantised to integers on a grid fixed by the object's largest weight, so every sum is exact and neither the grid, the block size nor
// the order in which workgroups finish can change a bit.  No atomics, and no workgroup waits for another: the order of the stages comes
// from the kernel boundaries alone.  A job is one block of `block` faces of one object; a workgroup finds its object by a binary
// search of the prefix array of job counts (n_obj + 1 entries), the only index of the launch.
//
//   surface_weights_kernel       one lane per face: tests the three indices BEFORE it loads a vertex, then the coordinates, computes the
//                                weight [ssamp::weight] and stores it; per job the largest weight and a failed flag.
//   surface_block_sum_kernel     folds the object's largest weight and failed flag from its jobs' partials (at most 2048 of them, a
//                                maximum: every workgroup of the object gets the same), quantises the job's weights and reduces them
//                                to one uint64 sum; the object's first job also stores the exponent (or kFailed).
//   surface_block_prefix_kernel  one workgroup per object: the inclusive prefix of its block sums, in place (at most 2048: eight per
//                                lane, a wave scan on two 32-bit halves, the four wave totals through LDS).
//   surface_scan_kernel          per job: the same scan over the job's quantised weights plus the prefix of the blocks before it -> C.
//   surface_pick_kernel          one lane per sample, the object's block prefix (at most 16 KiB) staged in LDS: counts the blocks whose
//                                prefix is <= t, then the faces of that block whose C is <= t [ssamp::count_le: kSearchSteps steps
//                                each, whatever the data], gathers the three vertices and writes point and face.  A failed object gets
//                                NaN and -1 and gathers nothing.
#include <vector>

#include "common.h"
#include "surface_sample_core.h"

namespace mp {

namespace {

constexpr int kWaves = ssamp::kThreads / 64;

// inclusive scan of one value per lane over the workgroup's 256 lanes; red holds one entry per wave
__device__ __forceinline__ uint64_t block_scan_inclusive(uint64_t v, uint64_t* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t o = shfl_up_any(v, d);
    if (lane >= d) v += o;
  }
  if (lane == 63) red[wave] = v;
  __syncthreads();
  for (int w = 0; w < wave; ++w) v += red[w];
  return v;
}

struct Job {
  int obj, b;        // the object and the block within it
  int n;             // faces of the block
  size_t f0;         // the block's first face in the packed arrays
};

// f_total = the faces of the launch by the host's prefix array, which sized the scratch: a device array that disagrees with it cannot
// carry a store past the end
__device__ __forceinline__ Job job_of(const int32_t* __restrict__ job_off, const int32_t* __restrict__ face_off, int n_obj, int block,
                                      int f_total) {
  Job j;
  j.obj = object_of(job_off, n_obj, blockIdx.x);
  j.b = blockIdx.x - job_off[j.obj];
  const long long begin = face_off[j.obj], first = begin + (long long)j.b * block;
  long long end = face_off[j.obj + 1];
  end = end < f_total ? end : f_total;
  const long long left = begin < 0 ? 0 : end - first;
  j.n = left < block ? (left > 0 ? (int)left : 0) : block;
  j.f0 = (size_t)(first > 0 ? first : 0);
  return j;
}

// the vertices of an object, cut to the v_total of the host's prefix array in the same way
__device__ __forceinline__ int32_t vertices_of(const int32_t* __restrict__ vert_off, int obj, int v_total) {
  const int32_t begin = vert_off[obj];
  int32_t end = vert_off[obj + 1];
  end = end < v_total ? end : v_total;
  return begin < 0 || end < begin ? 0 : end - begin;
}

}  // namespace

__global__ __launch_bounds__(256) void surface_weights_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                              const int32_t* __restrict__ vert_off, const int32_t* __restrict__ face_off,
                                                              const int32_t* __restrict__ job_off, int n_obj, int block,
                                                              int v_total, int f_total, float* __restrict__ w_out, float* __restrict__ job_max,
                                                              int32_t* __restrict__ job_bad) {
  __shared__ float red_mx[kWaves];
  __shared__ int red_bad[kWaves];
  const Job j = job_of(job_off, face_off, n_obj, block, f_total);
  const int32_t n_vert = vertices_of(vert_off, j.obj, v_total);
  const float* V = vertices + 3 * (size_t)vert_off[j.obj];
  float mx = 0.0f;
  int bad = 0;
  for (int i = threadIdx.x; i < j.n; i += ssamp::kThreads) {
    const size_t f = j.f0 + i;
    const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];
    float w = 0.0f;
    if (!ssamp::face_ok(ia, ib, ic, n_vert)) {
      bad = 1;                                   // nothing is loaded through a bad index
    } else {
      const float a[3] = {V[3 * (size_t)ia], V[3 * (size_t)ia + 1], V[3 * (size_t)ia + 2]};
      const float b[3] = {V[3 * (size_t)ib], V[3 * (size_t)ib + 1], V[3 * (size_t)ib + 2]};
      const float c[3] = {V[3 * (size_t)ic], V[3 * (size_t)ic + 1], V[3 * (size_t)ic + 2]};
      if (!ssamp::finite3(a[0], a[1], a[2]) || !ssamp::finite3(b[0], b[1], b[2]) || !ssamp::finite3(c[0], c[1], c[2])) {
        bad = 1;
      } else {
        w = ssamp::weight(a, b, c);
        if (!isfinite(w)) {
          bad = 1;
          w = 0.0f;
        }
      }
    }
    w_out[f] = w;
    mx = fmaxf(mx, w);
  }
  mx = block_max_all<kWaves>(mx, red_mx);
  bad = block_reduce_all<kWaves>(bad, red_bad, OrOp());
  if (threadIdx.x == 0) {
    job_max[blockIdx.x] = mx;
    job_bad[blockIdx.x] = bad;
  }
}

__global__ __launch_bounds__(256) void surface_block_sum_kernel(const int32_t* __restrict__ face_off, const int32_t* __restrict__ job_off,
                                                                int n_obj, int block, int f_total, const float* __restrict__ w,
                                                                const float* __restrict__ job_max, const int32_t* __restrict__ job_bad,
                                                                uint64_t* __restrict__ block_sum, int32_t* __restrict__ obj_e) {
  __shared__ float red_mx[kWaves];
  __shared__ int red_bad[kWaves];
  __shared__ uint64_t red[kWaves];
  const Job j = job_of(job_off, face_off, n_obj, block, f_total);
  float wmax = 0.0f;
  int bad = 0;
  for (int p = job_off[j.obj] + threadIdx.x; p < job_off[j.obj + 1]; p += ssamp::kThreads) {
    wmax = fmaxf(wmax, job_max[p]);
    bad |= job_bad[p];
  }
  wmax = block_max_all<kWaves>(wmax, red_mx);
  bad = block_reduce_all<kWaves>(bad, red_bad, OrOp());
  const bool failed = bad || !(wmax > 0.0f);
  const int e = failed ? ssamp::kFailed : ssamp::exponent_of(wmax);
  uint64_t s = 0;
  if (!failed)
    for (int i = threadIdx.x; i < j.n; i += ssamp::kThreads) s += ssamp::quantise(w[j.f0 + i], e);
  s = block_sum_all<kWaves>(s, red);
  if (threadIdx.x == 0) {
    block_sum[blockIdx.x] = s;
    if (j.b == 0) obj_e[j.obj] = e;
  }
}

__global__ __launch_bounds__(256) void surface_block_prefix_kernel(const int32_t* __restrict__ job_off, uint64_t* __restrict__ block_sum) {
  __shared__ uint64_t red[kWaves];
  constexpr int kPer = ssamp::kMaxBlocks / ssamp::kThreads;
  const int first = job_off[blockIdx.x];
  int n = job_off[blockIdx.x + 1] - first;
  n = n < ssamp::kMaxBlocks ? n : ssamp::kMaxBlocks;          // the entry point refused more
  uint64_t v[kPer];
  uint64_t run = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x * kPer + k;
    run += i < n ? block_sum[first + i] : 0ull;
    v[k] = run;
  }
  const uint64_t before = block_scan_inclusive(run, red) - run;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x * kPer + k;
    if (i < n) block_sum[first + i] = before + v[k];
  }
}

__global__ __launch_bounds__(256) void surface_scan_kernel(const int32_t* __restrict__ face_off, const int32_t* __restrict__ job_off, int n_obj,
                                                           int block, int f_total, const float* __restrict__ w,
                                                           const uint64_t* __restrict__ block_prefix,
                                                           const int32_t* __restrict__ obj_e, uint64_t* __restrict__ C) {
  __shared__ uint64_t red[kWaves];
  constexpr int kPer = ssamp::kMaxBlock / ssamp::kThreads;
  const Job j = job_of(job_off, face_off, n_obj, block, f_total);
  const int e = obj_e[j.obj];
  if (e == ssamp::kFailed) return;                             // the whole workgroup: C of a failed object is never read
  const int per = (block + ssamp::kThreads - 1) / ssamp::kThreads;   // consecutive faces of a lane, at most kPer
  uint64_t v[kPer];
  uint64_t run = 0;
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x * per + k;
    run += (k < per && i < j.n) ? ssamp::quantise(w[j.f0 + i], e) : 0ull;
    v[k] = run;
  }
  const uint64_t before = block_scan_inclusive(run, red) - run + (j.b > 0 ? block_prefix[blockIdx.x - 1] : 0ull);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int i = threadIdx.x * per + k;
    if (k < per && i < j.n) C[j.f0 + i] = before + v[k];
  }
}

__global__ __launch_bounds__(256) void surface_pick_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                           const int32_t* __restrict__ vert_off, const int32_t* __restrict__ face_off,
                                                           const int32_t* __restrict__ job_off, int block, const float* __restrict__ u,
                                                           int count, const uint64_t* __restrict__ block_prefix,
                                                           const uint64_t* __restrict__ C, const int32_t* __restrict__ obj_e,
                                                           float* __restrict__ points, int32_t* __restrict__ face_out) {
  __shared__ uint64_t prefix[ssamp::kMaxBlocks];
  const int obj = blockIdx.y;
  const int s = blockIdx.x * ssamp::kThreads + threadIdx.x;
  const size_t row = (size_t)obj * count + s;
  if (obj_e[obj] == ssamp::kFailed) {                          // the whole workgroup
    if (s < count) {
      points[3 * row] = NAN;
      points[3 * row + 1] = NAN;
      points[3 * row + 2] = NAN;
      face_out[row] = -1;
    }
    return;
  }
  const int first = job_off[obj];
  int n_b = job_off[obj + 1] - first;
  n_b = n_b < ssamp::kMaxBlocks ? n_b : ssamp::kMaxBlocks;   // the entry point refused more
  for (int i = threadIdx.x; i < n_b; i += ssamp::kThreads) prefix[i] = block_prefix[first + i];
  __syncthreads();
  if (s >= count) return;
  const float u0 = u[3 * row], u1 = u[3 * row + 1], u2 = u[3 * row + 2];
  const uint64_t t = ssamp::pick_t(prefix[n_b - 1], ssamp::pick_k(u0));
  const int bi = ssamp::count_le(prefix, n_b, t);
  const int n_faces = face_off[obj + 1] - face_off[obj], base = bi * block;
  const int left = n_faces - base;
  const int n = left < block ? (left > 1 ? left : 1) : block;
  const int fi = base + ssamp::count_le(C + (size_t)face_off[obj] + base, n, t);
  const size_t f = (size_t)face_off[obj] + fi;
  const float* V = vertices + 3 * (size_t)vert_off[obj];
  const int32_t ia = faces[3 * f], ib = faces[3 * f + 1], ic = faces[3 * f + 2];   // the weights pass tested every index of the object
  float r1, r2;
  ssamp::barycentric(u1, u2, &r1, &r2);
#pragma unroll
  for (int a = 0; a < 3; ++a)
    points[3 * row + a] = ssamp::point_axis(V[3 * (size_t)ia + a], V[3 * (size_t)ib + a], V[3 * (size_t)ic + a], r1, r2);
  face_out[row] = fi;
}

namespace {

struct Layout {
  std::vector<int32_t> job_off;   // host: the prefix array of job counts, copied to d_job_off
  int32_t *d_job_off, *d_obj_e, *d_job_bad;
  float *d_job_max, *d_w;
  uint64_t *d_block_sum, *d_C;
  size_t bytes;
};

// the prefix array of job counts and the scratch layout on `base` (null: sizes only); false for arguments the launch refuses
bool surface_layout(void* base, int n_obj, const int32_t* h_face_off, int count, int block, Layout* L) {
  if (n_obj < 1 || !h_face_off || count < 1 || !ssamp::block_ok(block) || h_face_off[0] < 0) return false;
  const int bs = ssamp::block_of(block);
  long long total = 0;
  L->job_off.assign((size_t)n_obj + 1, 0);
  for (int o = 0; o < n_obj; ++o) {
    const long long n_faces = (long long)h_face_off[o + 1] - h_face_off[o];
    if (!ssamp::faces_ok(n_faces, bs)) return false;
    total += ssamp::n_blocks((int)n_faces, bs);
    if (total >= ssamp::kMaxJobs) return false;
    L->job_off[o + 1] = (int32_t)total;
  }
  if ((long long)n_obj > 65535 || ((long long)count + ssamp::kThreads - 1) / ssamp::kThreads >= ssamp::kMaxJobs) return false;   // the pick grid
  const size_t n_jobs = (size_t)total, n_faces = (size_t)h_face_off[n_obj] - (size_t)h_face_off[0];
  WsCarver c(base);
  L->d_job_off = c.take<int32_t>((size_t)n_obj + 1);
  L->d_obj_e = c.take<int32_t>((size_t)n_obj);
  L->d_job_max = c.take<float>(n_jobs);
  L->d_job_bad = c.take<int32_t>(n_jobs);
  L->d_block_sum = c.take<uint64_t>(n_jobs);
  L->d_w = c.take<float>(n_faces);
  L->d_C = c.take<uint64_t>(n_faces);
  L->bytes = c.total();
  return true;
}

}  // namespace

}  // namespace mp

using namespace mp;

extern "C" size_t mp_surface_sample_scratch_bytes(int n_obj, const int32_t* h_face_off, int count, int block) {
  Layout L;
  return surface_layout(nullptr, n_obj, h_face_off, count, block, &L) ? L.bytes : 0;
}

extern "C" int mp_surface_sample(const float* d_vertices, const int32_t* d_faces, const int32_t* d_vert_off, const int32_t* d_face_off,
                                 const int32_t* h_vert_off, const int32_t* h_face_off, int n_obj, const float* d_u, int count, int block,
                                 void* d_workspace, float* d_points, int32_t* d_face, mp_stream stream) {
  MP_REQUIRE(n_obj >= 1 && n_obj <= 65535 && count >= 1, "mp_surface_sample: n_obj %d (1 .. 65535), count %d (at least 1)", n_obj, count);
  MP_REQUIRE(ssamp::block_ok(block), "mp_surface_sample: block %d is not 0 or a multiple of %d in [%d, %d]", block, ssamp::kBlockStep,
             ssamp::kBlockStep, ssamp::kMaxBlock);
  MP_REQUIRE(d_vertices && d_faces && d_vert_off && d_face_off && h_vert_off && h_face_off && d_u && d_workspace && d_points && d_face,
             "mp_surface_sample: null pointer");
  MP_REQUIRE(h_vert_off[0] == 0 && h_face_off[0] == 0, "mp_surface_sample: the prefix arrays start at %d and %d, not at 0", h_vert_off[0],
             h_face_off[0]);
  const int bs = ssamp::block_of(block);
  for (int o = 0; o < n_obj; ++o) {
    MP_REQUIRE(h_vert_off[o + 1] >= h_vert_off[o], "mp_surface_sample: vert_off descends at object %d", o);
    const long long n_faces = (long long)h_face_off[o + 1] - h_face_off[o];
    MP_REQUIRE(n_faces >= 1, "mp_surface_sample: object %d has no faces (face_off must ascend)", o);
    MP_REQUIRE(ssamp::faces_ok(n_faces, bs), "mp_surface_sample: object %d has %lld faces: at most 2^22, and at most %d blocks of %d", o, n_faces,
               ssamp::kMaxBlocks, bs);
  }
  Layout L;
  MP_REQUIRE(surface_layout(d_workspace, n_obj, h_face_off, count, block, &L), "mp_surface_sample: more than 2^31 - 1 jobs in one launch");
  hipStream_t s = (hipStream_t)stream;
  int32_t *d_job_off = L.d_job_off, *d_obj_e = L.d_obj_e, *d_job_bad = L.d_job_bad;
  float *d_job_max = L.d_job_max, *d_w = L.d_w;
  uint64_t *d_block_sum = L.d_block_sum, *d_C = L.d_C;
  const unsigned n_jobs = (unsigned)L.job_off[n_obj];
  const double n_faces = (double)h_face_off[n_obj], n_samples = (double)n_obj * count;
  ProfScope prof("surface_sample", 30.0 * n_faces + 12.0 * n_samples, 80.0 * n_faces + 76.0 * n_samples, s);
  // pageable host memory: the runtime has taken the bytes when the call returns
  MP_CHECK_HIP(hipMemcpyAsync(d_job_off, L.job_off.data(), L.job_off.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const dim3 wg(ssamp::kThreads);
  hipLaunchKernelGGL(surface_weights_kernel, dim3(n_jobs), wg, 0, s, d_vertices, d_faces, d_vert_off, d_face_off, d_job_off, n_obj, bs,
                     h_vert_off[n_obj], h_face_off[n_obj], d_w, d_job_max, d_job_bad);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(surface_block_sum_kernel, dim3(n_jobs), wg, 0, s, d_face_off, d_job_off, n_obj, bs, h_face_off[n_obj], d_w, d_job_max, d_job_bad,
                     d_block_sum, d_obj_e);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(surface_block_prefix_kernel, dim3(n_obj), wg, 0, s, d_job_off, d_block_sum);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(surface_scan_kernel, dim3(n_jobs), wg, 0, s, d_face_off, d_job_off, n_obj, bs, h_face_off[n_obj], d_w, d_block_sum, d_obj_e,
                     d_C);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(surface_pick_kernel, dim3((unsigned)((count + ssamp::kThreads - 1) / ssamp::kThreads), (unsigned)n_obj), wg, 0, s, d_vertices,
                     d_faces, d_vert_off, d_face_off, d_job_off, bs, d_u, count, d_block_sum, d_C, d_obj_e, d_points, d_face);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
