// tsdf.hip -- the device side of onboarding an object without a CAD model: posed depth views fused into a truncated signed distance
// field on a voxel grid, and the welded, coloured triangle mesh of its zero level by marching tetrahedra.
//
// The rules, the volume descriptor (tsdf::Volume over its tsdf::Grid) and the corner indexing are tsdf_core.h, shared with the host
// emulation of the tests; the views descriptor, the staged walk over the views and the entries' argument checks are tsdf_views.h, shared
// with texture_bake.hip and tsdf_track.hip; this file adds the work distribution.  Every float of a node
// or a vertex is produced by one thread from those rules, every rank is an exclusive sum of integers in one fixed order, so no grid or
// block size can change a result.  No atomics, no workgroup waits on another, no search at all: a triangle finds its vertices from
// the scanned ranks of its edges' owners.
//
//   tsdf_integrate_kernel  one lane per node, x across the lanes: the volume's planes are read once and written once per call, coalesced,
//                          and a node's sums and counts stay in registers over the call's views [walk_views: the views are staged in
//                          LDS kViewChunk at a time; every lane then reads the same entry].  The depth, mask and colour reads are
//                          gathers: neighbouring nodes hit neighbouring pixels.
//   tsdf_flags_kernel      per node: observed, inside [tsdf::node_flags].
//   tsdf_cells_kernel      per cell (the node that is its c0): complete or not, and its number of triangles from the six cases.
//   tsdf_count_kernel      per node: the mask of its seven edges that carry a vertex (the complete cells around an edge come from the
//                          pass before, hence a launch of its own), its exclusive vertex rank inside the workgroup, and the workgroup's
//                          totals of vertices and triangles.
//   tsdf_scan_kernel       one workgroup: the exclusive sums of the workgroups' totals in place (256 at a time with a carry), and the
//                          two grand totals -- the one read-back between mp_tsdf_extract_count and mp_tsdf_extract.
//   tsdf_emit_kernel       per node: its vertices (position and colour interpolated from the owner towards the far node) and its cell's
//                          triangles; every store guarded by the stated number of vertices / triangles.
// (The split of a node index into i, j, k and an edge's far node g + dx + dy * nx + dz * nxy stay written out in the kernels, and the grid
// is copied out of the descriptor, not referenced: behind a function, or through the reference, the cells, count and emit kernels compile
// to other instruction streams than the measured ones.)
// WORKSPACE of mp_tsdf_extract_count / mp_tsdf_extract (the extract reads what the count on the same volume left there): per node the
// flags, the cell byte (0x80 complete | triangles), the edge mask (bytes), the vertex rank inside its workgroup (uint16), per workgroup
// of kTsdfBlock nodes the vertex and triangle bases.
#include "common.h"
#include "tsdf_views.h"

namespace mp {

constexpr int kTsdfBlock = 256;
constexpr int kTsdfWaves = kTsdfBlock / 64;
constexpr int kCellComplete = 0x80;   // the cell byte: complete | its number of triangles (<= 12)

__global__ __launch_bounds__(kTsdfBlock) void tsdf_integrate_kernel(tsdf::Volume vol, PosedViews vw, float mu, float z_min, int carve) {
  __shared__ float views[kViewChunk][tsdf::kViewFloats];
  __shared__ int view_ok[kViewChunk];
  const tsdf::Grid gr = vol;
  const int g = blockIdx.x * kTsdfBlock + threadIdx.x;
  const bool in = g < gr.N;
  const bool color = vol.c_count != nullptr;
  tsdf::Node nd = {0.f, 0, 0.f, 0.f, 0.f, 0};
  float px = 0.f, py = 0.f, pz = 0.f;
  if (in) {
    const int i = g % gr.nx, j = (g / gr.nx) % gr.ny, k = g / (gr.nx * gr.ny);
    px = tsdf::node_coord(gr.ox, gr.voxel, i);
    py = tsdf::node_coord(gr.oy, gr.voxel, j);
    pz = tsdf::node_coord(gr.oz, gr.voxel, k);
    nd.sum = vol.sum[g];
    nd.count = vol.count[g];
    if (color) {
      nd.c0 = vol.c[0][g];
      nd.c1 = vol.c[1][g];
      nd.c2 = vol.c[2][g];
      nd.c_count = vol.c_count[g];
    }
  }
  walk_views(vw, in, views, view_ok, [&](const float* view, const float* depth, const uint8_t* mask, const uint8_t* rgb) {
    nd = tsdf::integrate(nd, tsdf::visit(px, py, pz, view, depth, mask, rgb, vw.h, vw.w, mu, z_min, carve != 0, color));
  });
  if (!in) return;
  vol.sum[g] = nd.sum;
  vol.count[g] = nd.count;
  if (color) {
    vol.c[0][g] = nd.c0;
    vol.c[1][g] = nd.c1;
    vol.c[2][g] = nd.c2;
    vol.c_count[g] = nd.c_count;
  }
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_flags_kernel(const float* __restrict__ sum, const int32_t* __restrict__ count, int N,
                                                                int min_views, uint8_t* __restrict__ flags) {
  const int g = blockIdx.x * kTsdfBlock + threadIdx.x;
  if (g < N) flags[g] = (uint8_t)tsdf::node_flags(sum[g], count[g], min_views);
}

// the flags of the eight corners of cell g = (i, j, k), a cell of the grid: all observed?  *inside8: bit = corner code
__device__ __forceinline__ bool tsdf_cell_corners(const uint8_t* __restrict__ flags, int g, int nx, int nxy, int* inside8) {
  int all = tsdf::kObserved, ins = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int f = flags[tsdf::corner_node(g, c, nx, nxy)];
    all &= f;
    ins |= ((f & tsdf::kInside) ? 1 : 0) << c;
  }
  *inside8 = ins;
  return all != 0;
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_cells_kernel(const uint8_t* __restrict__ flags, tsdf::Grid gr, uint8_t* __restrict__ cell) {
  const int g = blockIdx.x * kTsdfBlock + threadIdx.x;
  if (g >= gr.N) return;
  const int i = g % gr.nx, j = (g / gr.nx) % gr.ny, k = g / (gr.nx * gr.ny);
  int out = 0;
  if (i < gr.nx - 1 && j < gr.ny - 1 && k < gr.nz - 1) {
    int inside8;
    if (tsdf_cell_corners(flags, g, gr.nx, gr.nx * gr.ny, &inside8)) out = kCellComplete | tsdf::cell_triangles(tsdf::tables(), inside8);
  }
  cell[g] = (uint8_t)out;
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_count_kernel(const uint8_t* __restrict__ flags, const uint8_t* __restrict__ cell, tsdf::Grid gr,
                                                                uint8_t* __restrict__ emask, uint16_t* __restrict__ lrank,
                                                                int32_t* __restrict__ block_nv, int32_t* __restrict__ block_nt) {
  __shared__ int wave_tot[kTsdfWaves];
  const int g = blockIdx.x * kTsdfBlock + threadIdx.x;
  const bool in = g < gr.N;
  int mask = 0, nt = 0;
  if (in) {
    const tsdf::Tables& tb = tsdf::tables();
    const int nxy = gr.nx * gr.ny;
    const int i = g % gr.nx, j = (g / gr.nx) % gr.ny, k = g / nxy;
    const int fa = flags[g];
    nt = cell[g] & (kCellComplete - 1);
    if (fa & tsdf::kObserved) {
#pragma unroll
      for (int kind = 0; kind < tsdf::kEdgeKinds; ++kind) {
        const int d = tb.kind_diff[kind], dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
        if (i + dx >= gr.nx || j + dy >= gr.ny || k + dz >= gr.nz) continue;
        const int fb = flags[g + dx + dy * gr.nx + dz * nxy];
        if (!(fb & tsdf::kObserved) || ((fa ^ fb) & tsdf::kInside) == 0) continue;
        // the cells of the edge: c0 = the owner, or one back on an axis along which the edge does not run
        bool any = false;
        for (int s = 0; s < 8; ++s) {
          if ((s & d) != 0) continue;
          const int ci = i - (s & 1), cj = j - ((s >> 1) & 1), ck = k - ((s >> 2) & 1);
          if (ci < 0 || cj < 0 || ck < 0 || ci >= gr.nx - 1 || cj >= gr.ny - 1 || ck >= gr.nz - 1) continue;
          any = any || (cell[(ck * gr.ny + cj) * gr.nx + ci] & kCellComplete) != 0;
        }
        if (any) mask |= 1 << kind;
      }
    }
  }
  int total_v, total_t;
  const int before = block_exclusive_sum<kTsdfWaves>(__popc(mask), wave_tot, &total_v);
  block_exclusive_sum<kTsdfWaves>(nt, wave_tot, &total_t);
  if (in) {
    emask[g] = (uint8_t)mask;
    lrank[g] = (uint16_t)before;   // at most 255 * 7
  }
  if (threadIdx.x == 0) {
    block_nv[blockIdx.x] = total_v;
    block_nt[blockIdx.x] = total_t;
  }
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_scan_kernel(int32_t* __restrict__ block_nv, int32_t* __restrict__ block_nt, int n_blocks,
                                                               int32_t* __restrict__ totals) {
  __shared__ int wave_tot[kTsdfWaves];
  int carry_v = 0, carry_t = 0;
  for (int b0 = 0; b0 < n_blocks; b0 += kTsdfBlock) {
    const int b = b0 + threadIdx.x;
    const bool in = b < n_blocks;
    const int v = in ? block_nv[b] : 0, t = in ? block_nt[b] : 0;
    int tot_v, tot_t;
    const int ev = block_exclusive_sum<kTsdfWaves>(v, wave_tot, &tot_v);
    const int et = block_exclusive_sum<kTsdfWaves>(t, wave_tot, &tot_t);
    if (in) {
      block_nv[b] = carry_v + ev;
      block_nt[b] = carry_t + et;
    }
    carry_v += tot_v;
    carry_t += tot_t;
  }
  if (threadIdx.x == 0) {
    totals[0] = carry_v;
    totals[1] = carry_t;
  }
}

// the vertex index of edge `kind` of node o
__device__ __forceinline__ int tsdf_vertex_index(const int32_t* __restrict__ block_nv, const uint16_t* __restrict__ lrank,
                                                 const uint8_t* __restrict__ emask, int o, int kind) {
  return block_nv[o / kTsdfBlock] + (int)lrank[o] + __popc((int)emask[o] & ((1 << kind) - 1));
}

__global__ __launch_bounds__(kTsdfBlock) void tsdf_emit_kernel(tsdf::Volume vol, const uint8_t* __restrict__ flags,
                                                               const uint8_t* __restrict__ cell, const uint8_t* __restrict__ emask,
                                                               const uint16_t* __restrict__ lrank, const int32_t* __restrict__ block_nv,
                                                               const int32_t* __restrict__ block_nt, int n_vertices, int n_triangles,
                                                               float* __restrict__ vertices, float* __restrict__ colors, int32_t* __restrict__ faces) {
  __shared__ int wave_tot[kTsdfWaves];
  const tsdf::Grid gr = vol;
  const int g = blockIdx.x * kTsdfBlock + threadIdx.x;
  const bool in = g < gr.N;
  const int nxy = gr.nx * gr.ny;
  const int i = g % gr.nx, j = (g / gr.nx) % gr.ny, k = g / nxy;
  // (a workspace that no count left is not trusted with an address: only a cell of the grid has triangles, only an edge inside it a vertex)
  const int nt = in && i < gr.nx - 1 && j < gr.ny - 1 && k < gr.nz - 1 ? cell[g] & (kCellComplete - 1) : 0;
  int unused;
  const int t_before = block_exclusive_sum<kTsdfWaves>(nt, wave_tot, &unused);
  if (!in) return;
  const tsdf::Tables& tb = tsdf::tables();
  const int mask = emask[g];
  if (mask) {
    const float pa[3] = {tsdf::node_coord(gr.ox, gr.voxel, i), tsdf::node_coord(gr.oy, gr.voxel, j), tsdf::node_coord(gr.oz, gr.voxel, k)};
    const float fa = tsdf::field(vol.sum[g], vol.count[g]);
    float ca[3] = {1.f, 1.f, 1.f};
    if (vol.c_count)
      for (int c = 0; c < 3; ++c) ca[c] = tsdf::node_color(vol.c[c][g], vol.c_count[g]);
    int r = block_nv[blockIdx.x] + (int)lrank[g];
    for (int kind = 0; kind < tsdf::kEdgeKinds; ++kind) {
      if (!((mask >> kind) & 1)) continue;
      const int d = tb.kind_diff[kind], dx = d & 1, dy = (d >> 1) & 1, dz = (d >> 2) & 1;
      const int far = g + dx + dy * gr.nx + dz * nxy;
      if ((unsigned)r < (unsigned)n_vertices && i + dx < gr.nx && j + dy < gr.ny && k + dz < gr.nz) {
        const float pb[3] = {tsdf::node_coord(gr.ox, gr.voxel, i + dx), tsdf::node_coord(gr.oy, gr.voxel, j + dy),
                             tsdf::node_coord(gr.oz, gr.voxel, k + dz)};
        const float t = tsdf::edge_t(fa, tsdf::field(vol.sum[far], vol.count[far]));
        for (int c = 0; c < 3; ++c) {
          vertices[(size_t)r * 3 + c] = tsdf::lerp(pa[c], pb[c], t);
          const float cb = vol.c_count ? tsdf::node_color(vol.c[c][far], vol.c_count[far]) : 1.f;
          colors[(size_t)r * 3 + c] = tsdf::lerp(ca[c], cb, t);
        }
      }
      ++r;
    }
  }
  if (nt == 0) return;
  int inside8;
  tsdf_cell_corners(flags, g, gr.nx, nxy, &inside8);   // (nt > 0: the cell is a complete cell of the grid)
  int r = block_nt[blockIdx.x] + t_before;
  for (int T = 0; T < tsdf::kTets; ++T) {
    const int m = tsdf::tet_case(tb, T, inside8);
    for (int tri = 0; tri < tb.count[m]; ++tri) {
      if ((unsigned)r < (unsigned)n_triangles) {
        for (int s = 0; s < 3; ++s) {
          int code, kind;
          tsdf::tri_edge(tb, T, m, tri, s, &code, &kind);
          const int o = tsdf::corner_node(g, code, gr.nx, nxy);
          faces[(size_t)r * 3 + s] = tsdf_vertex_index(block_nv, lrank, emask, o, kind);
        }
      }
      ++r;
    }
  }
}

struct TsdfWs {
  uint8_t *flags, *cell, *emask;
  uint16_t* lrank;
  int32_t *block_nv, *block_nt;
  int n_blocks;
  size_t total;
  TsdfWs(void* base, int N) : n_blocks(ceil_div(N, kTsdfBlock)) {
    WsCarver c(base);
    flags = c.take<uint8_t>((size_t)N);
    cell = c.take<uint8_t>((size_t)N);
    emask = c.take<uint8_t>((size_t)N);
    lrank = c.take<uint16_t>((size_t)N);
    block_nv = c.take<int32_t>((size_t)n_blocks);
    block_nt = c.take<int32_t>((size_t)n_blocks);
    total = c.total();
  }
};

}  // namespace mp

using namespace mp;

extern "C" size_t mp_tsdf_volume_bytes(int nx, int ny, int nz, int color) {
  return tsdf::dims_ok(nx, ny, nz) ? (size_t)nx * ny * nz * 4 * tsdf::planes(color) : 0;
}

extern "C" int mp_tsdf_integrate(void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel, const float* d_depth,
                                 const uint8_t* d_masks, const uint8_t* d_rgb, const float* d_K, const float* d_TCO, int tco_floats, int n, int h,
                                 int w, float mu, float z_min, int carve, mp_stream stream) {
  const PosedViews vw = {d_depth, d_masks, d_rgb, d_K, d_TCO, tco_floats, n, h, w};
  if (int rc = require_volume("mp_tsdf_integrate", nx, ny, nz, ox, oy, oz, voxel)) return rc;
  MP_REQUIRE(tsdf::finite_f(mu) && mu > 0.f && tsdf::finite_f(z_min) && z_min >= 0.f,
             "mp_tsdf_integrate: the truncation distance must be finite and > 0, z_min finite and >= 0");
  const int rc = require_views("mp_tsdf_integrate", vw, false, INT32_MAX);
  if (rc != MP_OK || n == 0) return rc;
  MP_REQUIRE(d_volume, "mp_tsdf_integrate: null pointer");
  MP_REQUIRE((uintptr_t)d_volume % 4 == 0, "mp_tsdf_integrate: volume not 4-byte aligned");
  const tsdf::Volume vol = tsdf::volume_of(d_volume, nx, ny, nz, color, ox, oy, oz, voxel);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tsdf_integrate", 0.0, 8.0 * tsdf::planes(color) * (double)vol.N, s);
  hipLaunchKernelGGL(tsdf_integrate_kernel, dim3((unsigned)ceil_div(vol.N, kTsdfBlock)), dim3(kTsdfBlock), 0, s, vol, vw, mu, z_min, carve);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_tsdf_extract_workspace_bytes(int nx, int ny, int nz) {
  return tsdf::dims_ok(nx, ny, nz) ? TsdfWs(nullptr, nx * ny * nz).total : 0;
}

extern "C" int mp_tsdf_extract_count(const void* d_volume, int nx, int ny, int nz, int color, int min_views, int32_t* d_totals, void* d_ws,
                                     size_t ws_bytes, mp_stream stream) {
  if (int rc = require_volume("mp_tsdf_extract_count", nx, ny, nz, 0.f, 0.f, 0.f, 1.f)) return rc;
  MP_REQUIRE(min_views >= 1, "mp_tsdf_extract_count: min_views %d must be at least 1", min_views);
  MP_REQUIRE(d_volume && d_totals && d_ws, "mp_tsdf_extract_count: null pointer");
  const tsdf::Volume vol = tsdf::volume_of(const_cast<void*>(d_volume), nx, ny, nz, color, 0.f, 0.f, 0.f, 1.f);
  const tsdf::Grid& gr = vol;
  const TsdfWs ws(d_ws, gr.N);
  MP_REQUIRE(ws_bytes >= ws.total, "mp_tsdf_extract_count: workspace of %zu bytes, %zu needed", ws_bytes, ws.total);
  MP_REQUIRE((uintptr_t)d_ws % 16 == 0 && (uintptr_t)d_volume % 4 == 0, "mp_tsdf_extract_count: workspace not 16-byte aligned or volume not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tsdf_extract_count", 0.0, 8.0 * (double)gr.N + 30.0 * (double)gr.N, s);
  const dim3 grid((unsigned)ws.n_blocks), block(kTsdfBlock);
  hipLaunchKernelGGL(tsdf_flags_kernel, grid, block, 0, s, (const float*)vol.sum, (const int32_t*)vol.count, gr.N, min_views, ws.flags);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(tsdf_cells_kernel, grid, block, 0, s, (const uint8_t*)ws.flags, gr, ws.cell);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(tsdf_count_kernel, grid, block, 0, s, (const uint8_t*)ws.flags, (const uint8_t*)ws.cell, gr, ws.emask, ws.lrank, ws.block_nv,
                     ws.block_nt);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(tsdf_scan_kernel, dim3(1), block, 0, s, ws.block_nv, ws.block_nt, ws.n_blocks, d_totals);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_tsdf_extract(const void* d_volume, int nx, int ny, int nz, int color, float ox, float oy, float oz, float voxel, int n_vertices,
                               int n_triangles, float* d_vertices, float* d_colors, int32_t* d_faces, long long cap_vertices,
                               long long cap_triangles, void* d_ws, size_t ws_bytes, mp_stream stream) {
  if (int rc = require_volume("mp_tsdf_extract", nx, ny, nz, ox, oy, oz, voxel)) return rc;
  MP_REQUIRE(n_vertices >= 0 && n_triangles >= 0 && cap_vertices >= n_vertices && cap_triangles >= n_triangles,
             "mp_tsdf_extract: %d vertices and %d triangles must not be negative and must fit the capacity of %lld and %lld", n_vertices, n_triangles,
             cap_vertices, cap_triangles);
  if (n_vertices == 0 && n_triangles == 0) return MP_OK;
  MP_REQUIRE(d_volume && d_ws && (d_vertices || n_vertices == 0) && (d_colors || n_vertices == 0) && (d_faces || n_triangles == 0),
             "mp_tsdf_extract: null pointer");
  const tsdf::Volume vol = tsdf::volume_of(const_cast<void*>(d_volume), nx, ny, nz, color, ox, oy, oz, voxel);
  const TsdfWs ws(d_ws, vol.N);
  MP_REQUIRE(ws_bytes >= ws.total, "mp_tsdf_extract: workspace of %zu bytes, %zu needed", ws_bytes, ws.total);
  MP_REQUIRE((uintptr_t)d_ws % 16 == 0 && (uintptr_t)d_volume % 4 == 0, "mp_tsdf_extract: workspace not 16-byte aligned or volume not 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("tsdf_extract", 0.0, 6.0 * (double)vol.N + 24.0 * (double)n_vertices + 12.0 * (double)n_triangles, s);
  hipLaunchKernelGGL(tsdf_emit_kernel, dim3((unsigned)ws.n_blocks), dim3(kTsdfBlock), 0, s, vol, (const uint8_t*)ws.flags, (const uint8_t*)ws.cell,
                     (const uint8_t*)ws.emask, (const uint16_t*)ws.lrank, (const int32_t*)ws.block_nv, (const int32_t*)ws.block_nt, n_vertices,
                     n_triangles, d_vertices, d_colors, d_faces);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
