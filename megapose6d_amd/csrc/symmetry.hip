// symmetry.hip -- does a candidate rotation map an object's surface into itself?  For every candidate R about the object's centre c and
// every test point p (the vertices, then points drawn on the surface), the distance of g(p) = R (p - c) + c to the nearest triangle: a
// point-to-triangle search over candidates x test points x triangles, several objects in one call.
//
// The rules are symmetry_core.h, shared with the host emulation of the tests; this file adds the work distribution.  A candidate is
// decided by the maximum of a total order, so neither the tile, the grid nor the order in which workgroups finish can change a bit.  No
// atomics and no workgroup waits for another: every workgroup stores its own candidate's result.
//
//   symmetry_screen_kernel    one workgroup of 256 lanes per candidate.  The workgroup finds its object by a binary search of the prefix
//                             array of candidate counts [object_of] and walks the object's test points in blocks of 256: lane l holds the
//                             transformed point of row 256 * block + l in registers.  The object's triangles are staged `tile` at a time
//                             in LDS as three float4 (A and the sliver flag, B - A, C - A): every lane reads the SAME entry, three
//                             16-byte reads that the LDS broadcasts.  A lane stops at its first triangle within tol2; the tile loop ends when no lane of the
//                             workgroup still searches; the block loop ends at the first block that leaves a lane unsatisfied after
//                             the last tile, and the candidate is rejected.  Every exit is decided on the result of a workgroup
//                             reduction, which every thread holds, so every barrier sits under uniform control flow
//                             [block_primitives.h].  Lanes beyond the object's test points and stage entries beyond its triangles are
//                             masked, never clamped: a padding row is not read.  One accept byte per candidate.
//   symmetry_measure_kernel   the same staging without early outs: every lane takes the minimum over all triangles, keeps the worst of its
//                             own points, and the workgroup folds its lanes [block_reduce_all under symm::worse] -> dev2, the worst
//                             point and (mode 1) the accept byte.  In mode 0 a workgroup whose candidate the screen rejected leaves at
//                             once (a uniform test of one byte) with dev2 = NaN and worst = -1.
#include <vector>

#include "common.h"
#include "symmetry_core.h"

namespace mp {

namespace {

using symm::Worst;

constexpr int kWaves = symm::kBlock / 64;

struct WorstOp {   // the worse of two test points under symm::worse's total order
  static constexpr bool kFromZero = false;
  __device__ __forceinline__ Worst operator()(Worst a, Worst b) const { return symm::worse(b, a) ? b : a; }
};

// what a workgroup knows of its candidate's object, from the prefix arrays that the entry point checked and copied
struct Obj {
  int obj, n_vert, n_face, n_test;
  const float* V;        // the object's vertices
  const int32_t* F;      // its faces
  const float* T;        // its test points
  float tol2;
};

__device__ __forceinline__ Obj object_info(const float* __restrict__ vertices, const int32_t* __restrict__ faces, const float* __restrict__ tests,
                                           const int32_t* __restrict__ meta, int n_obj, int cand) {
  const int32_t* vert_off = meta;
  const int32_t* face_off = meta + (n_obj + 1);
  const int32_t* test_off = meta + 2 * (n_obj + 1);
  const int32_t* cand_off = meta + 3 * (n_obj + 1);
  Obj o;
  o.obj = object_of(cand_off, n_obj, cand);
  o.n_vert = vert_off[o.obj + 1] - vert_off[o.obj];
  o.n_face = face_off[o.obj + 1] - face_off[o.obj];
  o.n_test = test_off[o.obj + 1] - test_off[o.obj];
  o.V = vertices + 3 * (size_t)vert_off[o.obj];
  o.F = faces + 3 * (size_t)face_off[o.obj];
  o.T = tests + 3 * (size_t)test_off[o.obj];
  o.tol2 = __int_as_float(meta[4 * (n_obj + 1) + o.obj]);
  return o;
}

// triangles f0 .. f0 + n_stage - 1 of the object -> LDS.  An index outside the object's vertices is tested BEFORE a vertex is loaded and
// gives a NaN triangle, which no point is ever near (the entry point refused such a face on the host's copy).
__device__ __forceinline__ void stage_tile(const Obj& o, int f0, int n_stage, float4* __restrict__ stage) {
  for (int t = threadIdx.x; t < n_stage; t += symm::kBlock) {
    const size_t f = 3 * (size_t)(f0 + t);
    const int32_t ia = o.F[f], ib = o.F[f + 1], ic = o.F[f + 2];
    float4 a = make_float4(NAN, NAN, NAN, 0.f), e1 = a, e2 = a;
    if ((uint32_t)ia < (uint32_t)o.n_vert && (uint32_t)ib < (uint32_t)o.n_vert && (uint32_t)ic < (uint32_t)o.n_vert) {
      const float* A = o.V + 3 * (size_t)ia;
      const float* B = o.V + 3 * (size_t)ib;
      const float* C = o.V + 3 * (size_t)ic;
      a = make_float4(A[0], A[1], A[2], 0.f);
      e1 = make_float4(B[0] - a.x, B[1] - a.y, B[2] - a.z, 0.f);
      e2 = make_float4(C[0] - a.x, C[1] - a.y, C[2] - a.z, 0.f);
    }
    a.w = symm::is_sliver(e1.x, e1.y, e1.z, e2.x, e2.y, e2.z) ? 1.f : 0.f;   // the same for every lane that reads the entry
    stage[3 * t] = a;
    stage[3 * t + 1] = e1;
    stage[3 * t + 2] = e2;
  }
}

// the lane's transformed test point of block b; false for a lane beyond the object's test points (nothing is read)
__device__ __forceinline__ bool lane_point(const Obj& o, const float* R, const float* c, int i, float* gx, float* gy, float* gz) {
  if (i >= o.n_test) return false;
  const float* p = o.T + 3 * (size_t)i;
  symm::apply(R, c, p[0], p[1], p[2], gx, gy, gz);
  return true;
}

__device__ __forceinline__ float stage_dist2(const float4* __restrict__ stage, int t, float gx, float gy, float gz) {
  const float4 a = stage[3 * t], e1 = stage[3 * t + 1], e2 = stage[3 * t + 2];
  return symm::tri_dist2(a.x, a.y, a.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, a.w != 0.f, gx, gy, gz);
}

__device__ __forceinline__ void load_candidate(const float* __restrict__ cand_R, const float* __restrict__ centers, int cand, int obj, float* R,
                                               float* c) {
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = cand_R[9 * (size_t)cand + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = centers[3 * (size_t)obj + k];
}

}  // namespace

__global__ __launch_bounds__(256) void symmetry_screen_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                              const float* __restrict__ tests, const float* __restrict__ cand_R,
                                                              const float* __restrict__ centers, const int32_t* __restrict__ meta, int n_obj,
                                                              int tile, uint8_t* __restrict__ accept) {
  __shared__ float4 stage[3 * symm::kMaxTile];
  __shared__ int red[kWaves];
  const int cand = blockIdx.x, tid = threadIdx.x;
  const Obj o = object_info(vertices, faces, tests, meta, n_obj, cand);
  float R[9], c[3];
  load_candidate(cand_R, centers, cand, o.obj, R, c);
  int rejected = 0;
  for (int i0 = 0; i0 < o.n_test && !rejected; i0 += symm::kBlock) {      // uniform: n_test and rejected are the same in every thread
    float gx = 0.f, gy = 0.f, gz = 0.f;
    int searching = lane_point(o, R, c, i0 + tid, &gx, &gy, &gz) ? 1 : 0;
    int any = 1;
    for (int f0 = 0; f0 < o.n_face && any; f0 += tile) {                  // uniform: any is the result of the reduction
      const int n_stage = o.n_face - f0 < tile ? o.n_face - f0 : tile;
      stage_tile(o, f0, n_stage, stage);
      __syncthreads();
      if (searching)
        for (int t = 0; t < n_stage; ++t)
          if (stage_dist2(stage, t, gx, gy, gz) <= o.tol2) {
            searching = 0;
            break;
          }
      // the reduction's first barrier also ends every thread's reads of the stage before the next tile overwrites it
      any = block_reduce_all<kWaves>(searching, red, OrOp());
    }
    rejected = any;   // after the last tile (or after the tile that satisfied every lane): a lane still searching found no triangle
  }
  if (tid == 0) accept[cand] = rejected ? 0 : 1;
}

__global__ __launch_bounds__(256) void symmetry_measure_kernel(const float* __restrict__ vertices, const int32_t* __restrict__ faces,
                                                               const float* __restrict__ tests, const float* __restrict__ cand_R,
                                                               const float* __restrict__ centers, const int32_t* __restrict__ meta, int n_obj,
                                                               int tile, int mode, uint8_t* __restrict__ accept, float* __restrict__ dev2,
                                                               int32_t* __restrict__ worst) {
  __shared__ float4 stage[3 * symm::kMaxTile];
  __shared__ Worst red[kWaves];
  const int cand = blockIdx.x, tid = threadIdx.x;
  if (mode == 0 && accept[cand] == 0) {      // the whole workgroup: one byte, the same for every thread
    if (tid == 0) {
      dev2[cand] = NAN;
      worst[cand] = -1;
    }
    return;
  }
  const Obj o = object_info(vertices, faces, tests, meta, n_obj, cand);
  float R[9], c[3];
  load_candidate(cand_R, centers, cand, o.obj, R, c);
  Worst mine = symm::none();
  for (int i0 = 0; i0 < o.n_test; i0 += symm::kBlock) {
    float gx = 0.f, gy = 0.f, gz = 0.f;
    const bool own = lane_point(o, R, c, i0 + tid, &gx, &gy, &gz);
    float best = INFINITY;
    for (int f0 = 0; f0 < o.n_face; f0 += tile) {
      const int n_stage = o.n_face - f0 < tile ? o.n_face - f0 : tile;
      __syncthreads();                       // every thread has finished with the previous stage
      stage_tile(o, f0, n_stage, stage);
      __syncthreads();
      if (own)
        for (int t = 0; t < n_stage; ++t) symm::lane_min(stage_dist2(stage, t, gx, gy, gz), &best);
    }
    const Worst w{best, i0 + tid};
    if (own && symm::worse(w, mine)) mine = w;   // ascending points per lane: only a strictly larger d2 replaces
  }
  const Worst all = block_reduce_all<kWaves>(mine, red, WorstOp());
  if (tid == 0) {
    dev2[cand] = all.d2;
    worst[cand] = all.i == symm::kNone ? -1 : all.i;
    if (mode != 0) accept[cand] = symm::accepted(all.d2, o.tol2) ? 1 : 0;
  }
}

static size_t symmetry_meta_bytes(int n_obj) { return align256(symm::meta_words(n_obj) * sizeof(int32_t)); }

}  // namespace mp

using namespace mp;

extern "C" size_t mp_symmetry_check_scratch_bytes(int n_obj) { return n_obj < 1 ? 0 : symmetry_meta_bytes(n_obj); }

extern "C" int mp_symmetry_check(const float* d_vertices, const int32_t* d_faces, const int32_t* h_faces, const float* d_tests,
                                 const float* d_cand_R, const float* d_centers, const int32_t* h_vert_off, const int32_t* h_face_off,
                                 const int32_t* h_test_off, const int32_t* h_cand_off, const float* h_tol, int n_obj, int tile, int mode,
                                 void* d_scratch, uint8_t* d_accept, float* d_dev2, int32_t* d_worst, mp_stream stream) {
  MP_REQUIRE(n_obj >= 1, "mp_symmetry_check: n_obj %d: at least 1", n_obj);
  MP_REQUIRE(mode == 0 || mode == 1, "mp_symmetry_check: mode %d is not 0 (screen, then measure the accepted) or 1 (measure all)", mode);
  MP_REQUIRE(symm::tile_ok(tile), "mp_symmetry_check: tile %d is not 0 or a multiple of %d in [%d, %d]", tile, symm::kTileStep, symm::kTileStep,
             symm::kMaxTile);
  MP_REQUIRE(h_faces && h_vert_off && h_face_off && h_test_off && h_cand_off && h_tol, "mp_symmetry_check: null host pointer");
  MP_REQUIRE(h_vert_off[0] == 0 && h_face_off[0] == 0 && h_test_off[0] == 0 && h_cand_off[0] == 0,
             "mp_symmetry_check: a prefix array does not start at 0");
  for (int o = 0; o < n_obj; ++o) {
    const long long n_vert = (long long)h_vert_off[o + 1] - h_vert_off[o], n_face = (long long)h_face_off[o + 1] - h_face_off[o];
    MP_REQUIRE(n_vert >= 1, "mp_symmetry_check: object %d has no vertices (vert_off must ascend)", o);
    MP_REQUIRE(n_face >= 1, "mp_symmetry_check: object %d has no triangles (face_off must ascend)", o);
    MP_REQUIRE(h_test_off[o + 1] > h_test_off[o], "mp_symmetry_check: object %d has no test points (test_off must ascend)", o);
    MP_REQUIRE(h_cand_off[o + 1] >= h_cand_off[o], "mp_symmetry_check: cand_off descends at object %d", o);
    MP_REQUIRE(isfinite(h_tol[o]) && h_tol[o] >= 0.0f, "mp_symmetry_check: object %d has tol %g: finite and not negative", o, (double)h_tol[o]);
    for (long long f = 3LL * h_face_off[o]; f < 3LL * h_face_off[o + 1]; ++f)
      MP_REQUIRE(h_faces[f] >= 0 && h_faces[f] < n_vert, "mp_symmetry_check: object %d, face %lld: index %d outside its %lld vertices", o,
                 f / 3 - h_face_off[o], h_faces[f], n_vert);
  }
  const int n_cand = h_cand_off[n_obj];
  MP_REQUIRE(n_cand <= symm::kMaxCandidates, "mp_symmetry_check: %d candidates, more than %d in one call", n_cand, symm::kMaxCandidates);
  if (n_cand == 0) return MP_OK;
  MP_REQUIRE(d_vertices && d_faces && d_tests && d_cand_R && d_centers && d_scratch && d_accept && d_dev2 && d_worst,
             "mp_symmetry_check: null device pointer");
  std::vector<int32_t> meta(symm::meta_words(n_obj));
  const size_t n1 = (size_t)n_obj + 1;
  for (size_t k = 0; k < n1; ++k) {
    meta[k] = h_vert_off[k];
    meta[n1 + k] = h_face_off[k];
    meta[2 * n1 + k] = h_test_off[k];
    meta[3 * n1 + k] = h_cand_off[k];
  }
  for (int o = 0; o < n_obj; ++o) {
    const float tol2 = h_tol[o] * h_tol[o];
    memcpy(&meta[4 * n1 + o], &tol2, sizeof(float));
  }
  hipStream_t s = (hipStream_t)stream;
  int32_t* d_meta = (int32_t*)d_scratch;
  double work = 0.0;
  for (int o = 0; o < n_obj; ++o)
    work += (double)(h_cand_off[o + 1] - h_cand_off[o]) * (h_test_off[o + 1] - h_test_off[o]) * (h_face_off[o + 1] - h_face_off[o]);
  ProfScope prof("symmetry_check", 60.0 * work, 12.0 * ((double)h_vert_off[n_obj] + h_face_off[n_obj] + h_test_off[n_obj]), s);
  // pageable host memory: the runtime has taken the bytes when the call returns
  MP_CHECK_HIP(hipMemcpyAsync(d_meta, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice, s));
  const int t = symm::tile_of(tile);
  if (mode == 0) {
    hipLaunchKernelGGL(symmetry_screen_kernel, dim3((unsigned)n_cand), dim3(symm::kBlock), 0, s, d_vertices, d_faces, d_tests, d_cand_R, d_centers,
                       d_meta, n_obj, t, d_accept);
    MP_CHECK_HIP(hipGetLastError());
  }
  hipLaunchKernelGGL(symmetry_measure_kernel, dim3((unsigned)n_cand), dim3(symm::kBlock), 0, s, d_vertices, d_faces, d_tests, d_cand_R, d_centers,
                     d_meta, n_obj, t, mode, d_accept, d_dev2, d_worst);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
