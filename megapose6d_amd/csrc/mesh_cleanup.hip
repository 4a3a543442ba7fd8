// mesh_cleanup.hip -- cleaning up a triangle mesh on the device: connected components, selection of faces with the vertices they
// reference, and decimation by vertex clustering.  The rules are mesh_cleanup_core.h, shared with the host emulation of the tests; this
// file adds the work distribution.  Every index is an exclusive sum of integers in one fixed order, every sum that an atomic builds is
// a sum of integers, every float comes from one thread and finished integers: no grid, no arrival order can change a bit.
//
// Ordered ranks (select and cluster).  A flag array of n bytes (non-zero: set) is ranked by mc_rank_kernel: a lane takes 16 bytes with one
// load, a workgroup kRankSpan = 4096 of them; it leaves per lane the exclusive count inside the workgroup (uint16) and per workgroup
// its total, which mc_scan_kernel turns into bases (256 workgroups at a time with a carry) and the grand totals -- the one read-back
// between a count call and its emit call.  mc_rank reads a rank back: base + lane's count + the set bytes before it in its 16.
//
//   mc_select_faces_kernel   per face: kept and good -> its flag, a plain byte store of 1 for its three vertices; bad faces counted
//   mc_select_emit_kernel    per vertex and per face (one index space): copy the referenced vertices, renumber the kept faces
//   mc_cells_kernel          per vertex: its cell id or -1
//   mc_cluster_faces_kernel  per face: kept or not, a plain byte store of 1 into used[cell] for its three cells; dropped faces counted
//   mc_accumulate_kernel     per vertex of a used cell: its fixed-point coordinates, colours and a one are summed over the runs of
//                            neighbouring lanes that share the cell (mesh vertices of a TSDF arrive in node order), then one set of
//                            64-bit integer atomic adds per run into the accumulators of the cell's rank
//   mc_cluster_emit_kernel   per output vertex: the means; per face: the ranks of its cells (one index space)
//   mc_uf_init_kernel        parent[v] = v, face_count[v] = 0
//   mc_uf_union_kernel       per good face two unions of a lock-free union-find: the larger root is hooked under the smaller with atomicMin
//                            and the union retried with the displaced value when the hook raced.  parent[v] <= v always and only ever
//                            decreases, so there is no cycle and the final root is the component's minimum
//   mc_uf_label_kernel       per vertex: parent[v] = its root; per face: its label; one integer atomic add into face_count per label and
//                            wave (one index space)
//   mc_uf_largest_kernel     per vertex: components that own a face counted, the largest (count, -label) by block_reduce_all and one
//                            64-bit atomicMax per workgroup
//   mc_uf_totals_kernel      one lane: the totals
// Every loop of the union-find carries the cap of meshc::loop_cap; a lane that reaches it raises the status word and stops.
#include "common.h"
#include "mesh_cleanup_core.h"

namespace mp {

constexpr int kMcBlock = 256;
constexpr int kMcWaves = kMcBlock / 64;
constexpr int kRankPer = 16;                      // bytes per lane of the rank pass
constexpr int kRankSpan = kMcBlock * kRankPer;    // bytes per workgroup
constexpr size_t kMcCounterBytes = 256;           // the head of every workspace: counters (int32 [0] = bad faces; components: below)

// ---- ordered ranks ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int mc_nonzero_bytes(uint32_t w) { return __popc((((w & 0x7f7f7f7fu) + 0x7f7f7f7fu) | w) & 0x80808080u); }

// the non-zero bytes among the first k (0 .. 16) of the sixteen
__device__ __forceinline__ int mc_nonzero_below(uint4 q, int k) {
  const uint32_t w[4] = {q.x, q.y, q.z, q.w};
  int s = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int m = k - 4 * j;
    const uint32_t mask = m >= 4 ? 0xffffffffu : (m <= 0 ? 0u : ((1u << (8 * m)) - 1u));
    s += mc_nonzero_bytes(w[j] & mask);
  }
  return s;
}

struct RankBuf {
  uint8_t* bytes;      // n_blocks * kRankSpan
  uint16_t* lrank;     // n_blocks * kMcBlock
  int32_t* base;       // n_blocks
  long long n;
  int n_blocks;
};

__global__ __launch_bounds__(kMcBlock) void mc_rank_kernel(RankBuf rb) {
  __shared__ int wave_tot[kMcWaves];
  const long long group = (long long)blockIdx.x * kMcBlock + threadIdx.x;
  const long long e0 = group * kRankPer;
  int cnt = 0;
  if (e0 < rb.n) {
    const uint4 q = *reinterpret_cast<const uint4*>(rb.bytes + e0);
    const long long left = rb.n - e0;
    cnt = mc_nonzero_below(q, left < kRankPer ? (int)left : kRankPer);
  }
  int total;
  const int before = block_exclusive_sum<kMcWaves>(cnt, wave_tot, &total);
  rb.lrank[group] = (uint16_t)before;   // at most 255 * 16
  if (threadIdx.x == 0) rb.base[blockIdx.x] = total;
}

// exclusive sums of two arrays of workgroup totals in place, and the totals: [0], [1] the two sums, [2] the counted faces
__global__ __launch_bounds__(kMcBlock) void mc_scan_kernel(int32_t* __restrict__ a, int na, int32_t* __restrict__ b, int nb,
                                                           const int32_t* __restrict__ counters, int32_t* __restrict__ totals) {
  __shared__ int wave_tot[kMcWaves];
  int carry_a = 0, carry_b = 0;
  const int n = na > nb ? na : nb;
  for (int b0 = 0; b0 < n; b0 += kMcBlock) {
    const int i = b0 + threadIdx.x;
    const int va = i < na ? a[i] : 0, vb = i < nb ? b[i] : 0;
    int tot_a, tot_b;
    const int ea = block_exclusive_sum<kMcWaves>(va, wave_tot, &tot_a);
    const int eb = block_exclusive_sum<kMcWaves>(vb, wave_tot, &tot_b);
    if (i < na) a[i] = carry_a + ea;
    if (i < nb) b[i] = carry_b + eb;
    carry_a += tot_a;
    carry_b += tot_b;
  }
  if (threadIdx.x == 0) {
    totals[0] = carry_a;
    totals[1] = carry_b;
    totals[2] = counters[0];
  }
}

// the rank of element e (e < rb.n) among the set bytes
__device__ __forceinline__ int mc_rank(const RankBuf& rb, long long e) {
  const long long group = e >> 4;
  const uint4 q = *reinterpret_cast<const uint4*>(rb.bytes + (group << 4));
  return rb.base[group >> 8] + (int)rb.lrank[group] + mc_nonzero_below(q, (int)(e & 15));
}

// ---- select ------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kMcBlock) void mc_select_faces_kernel(const int32_t* __restrict__ faces, int F, int V, const uint8_t* __restrict__ keep,
                                                                   uint8_t* __restrict__ fkeep, uint8_t* __restrict__ vflag,
                                                                   int32_t* __restrict__ counters) {
  const int f = blockIdx.x * kMcBlock + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  const bool good = meshc::face_good(a, b, c, V);
  const bool kept = good && keep[f] != 0;
  fkeep[f] = kept ? 1 : 0;
  if (kept) {
    vflag[a] = 1;
    vflag[b] = 1;
    vflag[c] = 1;
  }
  if (!good) atomicAdd(&counters[0], 1);
}

__global__ __launch_bounds__(kMcBlock) void mc_select_emit_kernel(const float* __restrict__ vertices, const float* __restrict__ colors, int V,
                                                                  const int32_t* __restrict__ faces, int F, RankBuf vr, RankBuf fr, int n_vertices,
                                                                  int n_faces, float* __restrict__ out_vertices, float* __restrict__ out_colors,
                                                                  int32_t* __restrict__ out_faces) {
  const int g = blockIdx.x * kMcBlock + threadIdx.x;
  if (g < V && vr.bytes[g]) {
    const int r = mc_rank(vr, g);
    if ((unsigned)r < (unsigned)n_vertices)
      for (int k = 0; k < 3; ++k) {
        out_vertices[(size_t)r * 3 + k] = vertices[(size_t)g * 3 + k];
        if (colors) out_colors[(size_t)r * 3 + k] = colors[(size_t)g * 3 + k];
      }
  }
  if (g < F && fr.bytes[g]) {
    const int r = mc_rank(fr, g);
    const int a = faces[(size_t)g * 3], b = faces[(size_t)g * 3 + 1], c = faces[(size_t)g * 3 + 2];
    // (a workspace that no count left is not trusted with an address)
    if ((unsigned)r < (unsigned)n_faces && meshc::face_good(a, b, c, V)) {
      out_faces[(size_t)r * 3] = mc_rank(vr, a);
      out_faces[(size_t)r * 3 + 1] = mc_rank(vr, b);
      out_faces[(size_t)r * 3 + 2] = mc_rank(vr, c);
    }
  }
}

// ---- cluster -----------------------------------------------------------------------------------------------------------------------------
struct McGrid {
  float o[3], c;
  int g[3], cells;
};

__global__ __launch_bounds__(kMcBlock) void mc_cells_kernel(const float* __restrict__ vertices, int V, McGrid gr, int32_t* __restrict__ vcell) {
  const int v = blockIdx.x * kMcBlock + threadIdx.x;
  if (v >= V) return;
  const float p[3] = {vertices[(size_t)v * 3], vertices[(size_t)v * 3 + 1], vertices[(size_t)v * 3 + 2]};
  float u[3];
  vcell[v] = meshc::cell_of(p, gr.o, gr.c, gr.g, u);
}

__global__ __launch_bounds__(kMcBlock) void mc_cluster_faces_kernel(const int32_t* __restrict__ faces, int F, int V, const int32_t* __restrict__ vcell,
                                                                    int cells, uint8_t* __restrict__ fkeep, uint8_t* __restrict__ used,
                                                                    int32_t* __restrict__ counters) {
  const int f = blockIdx.x * kMcBlock + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  bool kept = false, dropped = true;
  if (meshc::face_good(a, b, c, V)) {
    const int ca = vcell[a], cb = vcell[b], cc = vcell[c];
    if ((unsigned)ca < (unsigned)cells && (unsigned)cb < (unsigned)cells && (unsigned)cc < (unsigned)cells) {
      dropped = false;
      kept = ca != cb && cb != cc && ca != cc;
      if (kept) {
        used[ca] = 1;
        used[cb] = 1;
        used[cc] = 1;
      }
    }
  }
  fkeep[f] = kept ? 1 : 0;
  if (dropped) atomicAdd(&counters[0], 1);
}

// the sum of v over the run of lanes [start, lane] (an inclusive scan that does not cross `start`); every lane of the wave calls it
template <typename T>
__device__ __forceinline__ T mc_run_sum(T v, int lane, int start) {
  for (int d = 1; d < 64; d <<= 1) {
    const T o = shfl_up_any(v, d);
    if (lane - d >= start) v += o;
  }
  return v;
}

// acc: six planes of n_vertices 64-bit sums (x, y, z, red, green, blue) and then n_vertices int32 counts
template <bool COLOR>
__global__ __launch_bounds__(kMcBlock) void mc_accumulate_kernel(const float* __restrict__ vertices, const float* __restrict__ colors, int V, McGrid gr,
                                                                 const int32_t* __restrict__ vcell, RankBuf ur, int n_vertices,
                                                                 unsigned long long* __restrict__ acc, int32_t* __restrict__ acc_count) {
  const int v = blockIdx.x * kMcBlock + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int r = -1;
  unsigned long long t[COLOR ? 6 : 3];
  for (int k = 0; k < (COLOR ? 6 : 3); ++k) t[k] = 0ull;
  if (v < V) {
    const float p[3] = {vertices[(size_t)v * 3], vertices[(size_t)v * 3 + 1], vertices[(size_t)v * 3 + 2]};
    float u[3];
    const int cell = meshc::cell_of(p, gr.o, gr.c, gr.g, u);
    if (cell >= 0 && cell == vcell[v] && ur.bytes[cell]) {
      r = mc_rank(ur, cell);
      if ((unsigned)r >= (unsigned)n_vertices) r = -1;
    }
    if (r >= 0) {
      for (int k = 0; k < 3; ++k) t[k] = (unsigned long long)meshc::fixed_of(u[k]);
      if (COLOR)
        for (int k = 0; k < 3; ++k) t[3 + k] = (unsigned long long)meshc::color_of(colors[(size_t)v * 3 + k]);
    }
  }
  // runs of neighbouring lanes with the same rank: the last lane of a run adds the run's sums
  const int prev = __shfl_up(r, 1);
  const unsigned long long heads = __ballot(lane == 0 || prev != r);
  const int start = 63 - __clzll(heads & (~0ull >> (63 - lane)));
  const bool tail = lane == 63 || ((heads >> (lane + 1)) & 1ull);
  const int n = mc_run_sum(r >= 0 ? 1 : 0, lane, start);
  for (int k = 0; k < (COLOR ? 6 : 3); ++k) t[k] = mc_run_sum(t[k], lane, start);
  if (tail && r >= 0) {
    for (int k = 0; k < (COLOR ? 6 : 3); ++k) atomicAdd(&acc[(size_t)k * n_vertices + r], t[k]);
    atomicAdd(&acc_count[r], n);
  }
}

__global__ __launch_bounds__(kMcBlock) void mc_cluster_emit_kernel(const int32_t* __restrict__ faces, int F, int V, McGrid gr,
                                                                   const int32_t* __restrict__ vcell, RankBuf ur, RankBuf fr, int n_vertices,
                                                                   int n_faces, const unsigned long long* __restrict__ acc,
                                                                   const int32_t* __restrict__ acc_count, bool color, float* __restrict__ out_vertices,
                                                                   float* __restrict__ out_colors, int32_t* __restrict__ out_faces) {
  const int g = blockIdx.x * kMcBlock + threadIdx.x;
  if (g < n_vertices) {
    const int count = acc_count[g];
    for (int k = 0; k < 3; ++k) {
      out_vertices[(size_t)g * 3 + k] = meshc::mean_coord(gr.o[k], gr.c, (long long)acc[(size_t)k * n_vertices + g], count);
      if (color) out_colors[(size_t)g * 3 + k] = meshc::mean_color((long long)acc[(size_t)(3 + k) * n_vertices + g], count);
    }
  }
  if (g < F && fr.bytes[g]) {
    const int r = mc_rank(fr, g);
    const int a = faces[(size_t)g * 3], b = faces[(size_t)g * 3 + 1], c = faces[(size_t)g * 3 + 2];
    if ((unsigned)r < (unsigned)n_faces && meshc::face_good(a, b, c, V)) {
      const int ca = vcell[a], cb = vcell[b], cc = vcell[c];
      if ((unsigned)ca < (unsigned)gr.cells && (unsigned)cb < (unsigned)gr.cells && (unsigned)cc < (unsigned)gr.cells) {
        out_faces[(size_t)r * 3] = mc_rank(ur, ca);
        out_faces[(size_t)r * 3 + 1] = mc_rank(ur, cb);
        out_faces[(size_t)r * 3 + 2] = mc_rank(ur, cc);
      }
    }
  }
}

// ---- components --------------------------------------------------------------------------------------------------------------------------
// counters of the components' workspace: the 64-bit (count << 32 | 0x7fffffff - label) of the largest at byte 0, then int32 [2] the
// components that own a face, [3] the bad faces, [4] the status
constexpr int kUfComps = 2, kUfBad = 3, kUfStatus = 4;

__device__ __forceinline__ int mc_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v, with parent[v] lowered to it; -1 (and the status raised) when the walk reaches the cap or leaves [0, V)
__device__ __forceinline__ int mc_find(int32_t* parent, int V, int v, long long cap, int32_t* status) {
  int r = v;
  for (long long it = 0; it < cap; ++it) {
    const int p = mc_load(&parent[r]);
    if (p == r) {
      if (r != v && mc_load(&parent[v]) > r) atomicMin(&parent[v], r);
      return r;
    }
    if ((unsigned)p >= (unsigned)V) break;
    r = p;
  }
  atomicOr(status, meshc::kStatusCap);
  return -1;
}

__device__ __forceinline__ void mc_union(int32_t* parent, int V, int a, int b, long long cap, int32_t* status) {
  for (long long it = 0; it < cap; ++it) {
    a = mc_find(parent, V, a, cap, status);
    b = mc_find(parent, V, b, cap, status);
    if (a < 0 || b < 0 || a == b) return;
    const int hi = a > b ? a : b, lo = a > b ? b : a;
    const int old = atomicMin(&parent[hi], lo);
    if (old == hi) return;   // hi was still a root: hooked
    a = old;                 // another lane had lowered it: what it pointed to must still meet lo
    b = lo;
  }
  atomicOr(status, meshc::kStatusCap);
}

__global__ __launch_bounds__(kMcBlock) void mc_uf_init_kernel(int32_t* __restrict__ parent, int32_t* __restrict__ face_count, int V) {
  const int v = blockIdx.x * kMcBlock + threadIdx.x;
  if (v >= V) return;
  parent[v] = v;
  face_count[v] = 0;
}

__global__ __launch_bounds__(kMcBlock) void mc_uf_union_kernel(const int32_t* __restrict__ faces, int F, int V, int32_t* parent, long long cap,
                                                               int32_t* counters) {
  const int f = blockIdx.x * kMcBlock + threadIdx.x;
  if (f >= F) return;
  const int a = faces[(size_t)f * 3], b = faces[(size_t)f * 3 + 1], c = faces[(size_t)f * 3 + 2];
  if (!meshc::face_good(a, b, c, V)) return;
  mc_union(parent, V, a, b, cap, &counters[kUfStatus]);
  mc_union(parent, V, b, c, cap, &counters[kUfStatus]);
}

__global__ __launch_bounds__(kMcBlock) void mc_uf_label_kernel(const int32_t* __restrict__ faces, int F, int V, int32_t* parent, long long cap,
                                                               int32_t* __restrict__ face_labels, int32_t* face_count, int32_t* counters) {
  const int g = blockIdx.x * kMcBlock + threadIdx.x;
  if (g < V) mc_find(parent, V, g, cap, &counters[kUfStatus]);   // leaves parent[g] = the root
  int label = -1;
  if (g < F) {
    const int a = faces[(size_t)g * 3], b = faces[(size_t)g * 3 + 1], c = faces[(size_t)g * 3 + 2];
    if (meshc::face_good(a, b, c, V))
      label = mc_find(parent, V, a, cap, &counters[kUfStatus]);
    else
      atomicAdd(&counters[kUfBad], 1);
    face_labels[g] = label;
  }
  // one add per label and wave, not per face: the faces of a wave mostly share a label, and a whole mesh may (one word takes
  // its adds one after another)
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(label >= 0);
  while (todo) {
    const int src = __ffsll(todo) - 1;
    const int l = __shfl(label, src);
    const unsigned long long same = __ballot(label == l) & todo;
    if (lane == src) atomicAdd(&face_count[l], __popcll(same));
    todo &= ~same;
  }
}

__global__ __launch_bounds__(kMcBlock) void mc_uf_largest_kernel(const int32_t* __restrict__ face_count, int V, int32_t* counters) {
  __shared__ unsigned long long red_key[kMcWaves];
  __shared__ int red_n[kMcWaves];
  const int v = blockIdx.x * kMcBlock + threadIdx.x;
  const int c = v < V ? face_count[v] : 0;
  const unsigned long long key = c > 0 ? ((unsigned long long)(unsigned)c << 32) | (unsigned long long)(0x7fffffffu - (unsigned)v) : 0ull;
  const unsigned long long best = block_max_all<kMcWaves>(key, red_key);
  const int n = block_sum_all<kMcWaves>(c > 0 ? 1 : 0, red_n);
  if (threadIdx.x == 0 && n > 0) {
    atomicMax(reinterpret_cast<unsigned long long*>(counters), best);
    atomicAdd(&counters[kUfComps], n);
  }
}

__global__ void mc_uf_totals_kernel(const int32_t* __restrict__ counters, int32_t* __restrict__ totals) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long key = *reinterpret_cast<const unsigned long long*>(counters);
  totals[0] = counters[kUfComps];
  totals[1] = key ? (int32_t)(0x7fffffffu - (uint32_t)(key & 0xffffffffull)) : -1;
  totals[2] = counters[kUfBad];
  totals[3] = counters[kUfStatus];
}

// an empty input (V == 0 or F == 0): every vertex its own label, no face has one
__global__ __launch_bounds__(kMcBlock) void mc_uf_empty_kernel(int32_t* __restrict__ labels, int32_t* __restrict__ face_count, int V,
                                                               int32_t* __restrict__ face_labels, int F, int32_t* __restrict__ totals) {
  const int g = blockIdx.x * kMcBlock + threadIdx.x;
  if (g < V) {
    labels[g] = g;
    face_count[g] = 0;
  }
  if (g < F) face_labels[g] = -1;
  if (g == 0) {
    totals[0] = 0;
    totals[1] = -1;
    totals[2] = 0;
    totals[3] = 0;
  }
}

// ---- workspaces ----------------------------------------------------------------------------------------------------------------------------
static RankBuf rank_buf(WsCarver* c, long long n) {
  RankBuf r;
  r.n = n;
  r.n_blocks = ceil_div(n, kRankSpan);
  r.bytes = c->take<uint8_t>((size_t)r.n_blocks * kRankSpan);
  r.lrank = c->take<uint16_t>((size_t)r.n_blocks * kMcBlock);
  r.base = c->take<int32_t>((size_t)r.n_blocks);
  return r;
}

struct SelectWs {
  int32_t* counters;
  RankBuf v, f;
  size_t total;
  SelectWs(void* base, int V, int F) {
    WsCarver c(base);
    counters = c.take<int32_t>(kMcCounterBytes / sizeof(int32_t));
    v = rank_buf(&c, V);
    f = rank_buf(&c, F);
    total = c.total();
  }
};

struct ClusterWs {
  int32_t *counters, *vcell;
  RankBuf u, f;
  long long max_out;          // an output vertex is a used cell that holds a vertex
  unsigned long long* acc;    // [n_vertices][6] sums, then [n_vertices] int32 counts: at most max_out * 52 bytes
  size_t total;
  ClusterWs(void* base, int V, int F, int gx, int gy, int gz) {
    WsCarver c(base);
    const long long cells = (long long)gx * gy * gz;
    counters = c.take<int32_t>(kMcCounterBytes / sizeof(int32_t));
    vcell = c.take<int32_t>((size_t)V);
    u = rank_buf(&c, cells);
    f = rank_buf(&c, F);
    max_out = cells < V ? cells : V;
    acc = (unsigned long long*)c.take<char>((size_t)max_out * (6 * sizeof(unsigned long long) + sizeof(int32_t)));
    total = c.total();
  }
};

static McGrid mc_grid(float ox, float oy, float oz, float cell, int gx, int gy, int gz) {
  McGrid g;
  g.o[0] = ox;
  g.o[1] = oy;
  g.o[2] = oz;
  g.c = cell;
  g.g[0] = gx;
  g.g[1] = gy;
  g.g[2] = gz;
  g.cells = gx * gy * gz;
  return g;
}

// the two rank passes and the scan that end a count call
static int mc_rank_and_scan(const RankBuf& a, const RankBuf& b, const int32_t* counters, int32_t* d_totals, hipStream_t s) {
  hipLaunchKernelGGL(mc_rank_kernel, dim3((unsigned)a.n_blocks), dim3(kMcBlock), 0, s, a);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_rank_kernel, dim3((unsigned)b.n_blocks), dim3(kMcBlock), 0, s, b);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_scan_kernel, dim3(1), dim3(kMcBlock), 0, s, a.base, a.n_blocks, b.base, b.n_blocks, counters, d_totals);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

}  // namespace mp

using namespace mp;

#define MC_REQUIRE_COUNTS(name) \
  MP_REQUIRE(meshc::counts_ok(V, F), name ": %d vertices and %d faces: each 0 .. 2^29", V, F)
#define MC_REQUIRE_GRID(name)                                                                                                             \
  MP_REQUIRE(meshc::dims_ok(gx, gy, gz), name ": a grid of %d x %d x %d cells: each side 1 .. 512, at most 2^27 cells", gx, gy, gz);     \
  MP_REQUIRE(meshc::grid_ok(ox, oy, oz, cell), name ": origin must be finite, the cell size finite and > 0")
#define MC_REQUIRE_WS(name, need)                                                                              \
  MP_REQUIRE(d_ws && (uintptr_t)d_ws % 16 == 0, name ": workspace null or not 16-byte aligned");              \
  MP_REQUIRE(ws_bytes >= (need), name ": workspace of %zu bytes, %zu needed", ws_bytes, (size_t)(need))
#define MC_REQUIRE_CAPS(name)                                                                                                             \
  MP_REQUIRE(n_vertices >= 0 && n_faces >= 0 && cap_vertices >= n_vertices && cap_faces >= n_faces,                                      \
             name ": %d vertices and %d faces must not be negative and must fit the capacity of %lld and %lld", n_vertices, n_faces,     \
             cap_vertices, cap_faces)

extern "C" size_t mp_mesh_components_workspace_bytes(int V, int F) { return meshc::counts_ok(V, F) ? kMcCounterBytes : 0; }

extern "C" int mp_mesh_components(int V, const int32_t* d_faces, int F, int32_t* d_labels, int32_t* d_face_labels, int32_t* d_face_count,
                                  int32_t* d_totals, void* d_ws, size_t ws_bytes, mp_stream stream) {
  MC_REQUIRE_COUNTS("mp_mesh_components");
  MP_REQUIRE(d_totals && (V == 0 || (d_labels && d_face_count)) && (F == 0 || (d_faces && d_face_labels)), "mp_mesh_components: null pointer");
  MC_REQUIRE_WS("mp_mesh_components", kMcCounterBytes);
  hipStream_t s = (hipStream_t)stream;
  const int n = V > F ? V : F;
  if (V == 0 || F == 0) {
    hipLaunchKernelGGL(mc_uf_empty_kernel, dim3((unsigned)(n ? ceil_div(n, kMcBlock) : 1)), dim3(kMcBlock), 0, s, d_labels, d_face_count, V, d_face_labels,
                       F, d_totals);
    MP_CHECK_HIP(hipGetLastError());
    return MP_OK;
  }
  ProfScope prof("mesh_components", 0.0, 12.0 * (double)V + 28.0 * (double)F, s);
  int32_t* counters = (int32_t*)d_ws;
  const long long cap = meshc::loop_cap(V);
  MP_CHECK_HIP(hipMemsetAsync(counters, 0, kMcCounterBytes, s));
  hipLaunchKernelGGL(mc_uf_init_kernel, dim3((unsigned)ceil_div(V, kMcBlock)), dim3(kMcBlock), 0, s, d_labels, d_face_count, V);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_uf_union_kernel, dim3((unsigned)ceil_div(F, kMcBlock)), dim3(kMcBlock), 0, s, d_faces, F, V, d_labels, cap, counters);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_uf_label_kernel, dim3((unsigned)ceil_div(n, kMcBlock)), dim3(kMcBlock), 0, s, d_faces, F, V, d_labels, cap, d_face_labels,
                     d_face_count, counters);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_uf_largest_kernel, dim3((unsigned)ceil_div(V, kMcBlock)), dim3(kMcBlock), 0, s, (const int32_t*)d_face_count, V, counters);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_uf_totals_kernel, dim3(1), dim3(64), 0, s, (const int32_t*)counters, d_totals);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_mesh_select_workspace_bytes(int V, int F) { return meshc::counts_ok(V, F) ? SelectWs(nullptr, V, F).total : 0; }

extern "C" int mp_mesh_select_count(int V, const int32_t* d_faces, int F, const uint8_t* d_keep, int32_t* d_totals, void* d_ws, size_t ws_bytes,
                                    mp_stream stream) {
  MC_REQUIRE_COUNTS("mp_mesh_select_count");
  MP_REQUIRE(d_totals && (F == 0 || (d_faces && d_keep)), "mp_mesh_select_count: null pointer");
  const SelectWs p(d_ws, V, F);
  MC_REQUIRE_WS("mp_mesh_select_count", p.total);
  hipStream_t s = (hipStream_t)stream;
  if (V == 0 || F == 0) {
    MP_CHECK_HIP(hipMemsetAsync(d_totals, 0, meshc::kTotals * sizeof(int32_t), s));
    return MP_OK;
  }
  ProfScope prof("mesh_select_count", 0.0, 15.0 * (double)F + 3.0 * (double)V, s);
  const RankBuf &vr = p.v, &fr = p.f;
  MP_CHECK_HIP(hipMemsetAsync(p.counters, 0, kMcCounterBytes, s));
  MP_CHECK_HIP(hipMemsetAsync(vr.bytes, 0, (size_t)vr.n_blocks * kRankSpan, s));
  hipLaunchKernelGGL(mc_select_faces_kernel, dim3((unsigned)ceil_div(F, kMcBlock)), dim3(kMcBlock), 0, s, d_faces, F, V, d_keep, fr.bytes, vr.bytes,
                     p.counters);
  MP_CHECK_HIP(hipGetLastError());
  return mc_rank_and_scan(vr, fr, p.counters, d_totals, s);
}

extern "C" int mp_mesh_select(const float* d_vertices, const float* d_colors, int V, const int32_t* d_faces, int F, int n_vertices, int n_faces,
                              float* d_out_vertices, float* d_out_colors, int32_t* d_out_faces, long long cap_vertices, long long cap_faces,
                              void* d_ws, size_t ws_bytes, mp_stream stream) {
  MC_REQUIRE_COUNTS("mp_mesh_select");
  MC_REQUIRE_CAPS("mp_mesh_select");
  if (V == 0 || F == 0 || (n_vertices == 0 && n_faces == 0)) return MP_OK;
  MP_REQUIRE(d_vertices && d_faces && (n_vertices == 0 || (d_out_vertices && (!d_colors || d_out_colors))) && (n_faces == 0 || d_out_faces),
             "mp_mesh_select: null pointer");
  const SelectWs p(d_ws, V, F);
  MC_REQUIRE_WS("mp_mesh_select", p.total);
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("mesh_select", 0.0, 13.0 * (double)F + 1.0 * (double)V + 24.0 * (double)n_vertices + 24.0 * (double)n_faces, s);
  const int n = V > F ? V : F;
  hipLaunchKernelGGL(mc_select_emit_kernel, dim3((unsigned)ceil_div(n, kMcBlock)), dim3(kMcBlock), 0, s, d_vertices, d_colors, V, d_faces, F,
                     p.v, p.f, n_vertices, n_faces, d_out_vertices, d_out_colors, d_out_faces);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_mesh_cluster_workspace_bytes(int V, int F, int gx, int gy, int gz) {
  return meshc::counts_ok(V, F) && meshc::dims_ok(gx, gy, gz) ? ClusterWs(nullptr, V, F, gx, gy, gz).total : 0;
}

extern "C" int mp_mesh_cluster_count(const float* d_vertices, int V, const int32_t* d_faces, int F, float ox, float oy, float oz, float cell, int gx,
                                     int gy, int gz, int32_t* d_totals, void* d_ws, size_t ws_bytes, mp_stream stream) {
  MC_REQUIRE_COUNTS("mp_mesh_cluster_count");
  MC_REQUIRE_GRID("mp_mesh_cluster_count");
  MP_REQUIRE(d_totals && (V == 0 || d_vertices) && (F == 0 || d_faces), "mp_mesh_cluster_count: null pointer");
  const ClusterWs p(d_ws, V, F, gx, gy, gz);
  MC_REQUIRE_WS("mp_mesh_cluster_count", p.total);
  hipStream_t s = (hipStream_t)stream;
  if (V == 0 || F == 0) {
    MP_CHECK_HIP(hipMemsetAsync(d_totals, 0, meshc::kTotals * sizeof(int32_t), s));
    return MP_OK;
  }
  const McGrid gr = mc_grid(ox, oy, oz, cell, gx, gy, gz);
  ProfScope prof("mesh_cluster_count", 0.0, 16.0 * (double)V + 27.0 * (double)F + 2.2 * (double)gr.cells, s);
  int32_t *counters = p.counters, *vcell = p.vcell;
  const RankBuf &ur = p.u, &fr = p.f;
  MP_CHECK_HIP(hipMemsetAsync(counters, 0, kMcCounterBytes, s));
  MP_CHECK_HIP(hipMemsetAsync(ur.bytes, 0, (size_t)ur.n_blocks * kRankSpan, s));
  hipLaunchKernelGGL(mc_cells_kernel, dim3((unsigned)ceil_div(V, kMcBlock)), dim3(kMcBlock), 0, s, d_vertices, V, gr, vcell);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(mc_cluster_faces_kernel, dim3((unsigned)ceil_div(F, kMcBlock)), dim3(kMcBlock), 0, s, d_faces, F, V, (const int32_t*)vcell, gr.cells,
                     fr.bytes, ur.bytes, counters);
  MP_CHECK_HIP(hipGetLastError());
  return mc_rank_and_scan(ur, fr, counters, d_totals, s);
}

extern "C" int mp_mesh_cluster(const float* d_vertices, const float* d_colors, int V, const int32_t* d_faces, int F, float ox, float oy, float oz,
                               float cell, int gx, int gy, int gz, int n_vertices, int n_faces, float* d_out_vertices, float* d_out_colors,
                               int32_t* d_out_faces, long long cap_vertices, long long cap_faces, void* d_ws, size_t ws_bytes, mp_stream stream) {
  MC_REQUIRE_COUNTS("mp_mesh_cluster");
  MC_REQUIRE_GRID("mp_mesh_cluster");
  MC_REQUIRE_CAPS("mp_mesh_cluster");
  if (V == 0 || F == 0 || (n_vertices == 0 && n_faces == 0)) return MP_OK;
  const ClusterWs p(d_ws, V, F, gx, gy, gz);
  MP_REQUIRE(n_vertices <= p.max_out, "mp_mesh_cluster: %d vertices out, but %d vertices in %d x %d x %d cells give at most %lld", n_vertices, V, gx, gy,
             gz, p.max_out);
  MP_REQUIRE(d_vertices && d_faces && (n_vertices == 0 || (d_out_vertices && (!d_colors || d_out_colors))) && (n_faces == 0 || d_out_faces),
             "mp_mesh_cluster: null pointer");
  MC_REQUIRE_WS("mp_mesh_cluster", p.total);
  hipStream_t s = (hipStream_t)stream;
  const McGrid gr = mc_grid(ox, oy, oz, cell, gx, gy, gz);
  ProfScope prof("mesh_cluster", 0.0, (d_colors ? 28.0 : 16.0) * (double)V + 13.0 * (double)F + 76.0 * (double)n_vertices + 24.0 * (double)n_faces, s);
  const int32_t* vcell = p.vcell;
  unsigned long long* acc = p.acc;
  int32_t* acc_count = (int32_t*)(acc + (size_t)6 * n_vertices);
  const RankBuf &ur = p.u, &fr = p.f;
  if (n_vertices > 0) {
    MP_CHECK_HIP(hipMemsetAsync(acc, 0, (size_t)n_vertices * (6 * sizeof(unsigned long long) + sizeof(int32_t)), s));
    const dim3 grid((unsigned)ceil_div(V, kMcBlock)), block(kMcBlock);
    if (d_colors)
      hipLaunchKernelGGL(mc_accumulate_kernel<true>, grid, block, 0, s, d_vertices, d_colors, V, gr, vcell, ur, n_vertices, acc, acc_count);
    else
      hipLaunchKernelGGL(mc_accumulate_kernel<false>, grid, block, 0, s, d_vertices, d_colors, V, gr, vcell, ur, n_vertices, acc, acc_count);
    MP_CHECK_HIP(hipGetLastError());
  }
  const int n = n_vertices > F ? n_vertices : F;
  hipLaunchKernelGGL(mc_cluster_emit_kernel, dim3((unsigned)ceil_div(n, kMcBlock)), dim3(kMcBlock), 0, s, d_faces, F, V, gr, vcell, ur, fr, n_vertices,
                     n_faces, (const unsigned long long*)acc, (const int32_t*)acc_count, d_colors != nullptr, d_out_vertices, d_out_colors, d_out_faces);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
