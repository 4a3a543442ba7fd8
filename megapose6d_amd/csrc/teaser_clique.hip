// teaser_clique.hip -- the exact maximum clique of the consistency graph (TEASER++'s default inlier selection, PMC_EXACT) as a bounded,
// deterministic, batched branch-and-bound on the device.  The rule is the sequential one of teaser_clique_core.h; the kernel reproduces
// its members, flag and step count exactly.
//
// Mapping: one row's search is one sequential walk, so one wave searches one row and the rows are spread over the grid (a workgroup is
// one wave; it takes rows blockIdx.x, blockIdx.x + gridDim.x, ..).  Parallelism lives inside a search node: lane w < words owns word w
// of every live bit set (P, the class candidates Q, the uncoloured U, best), so an intersection with a neighbourhood is one LDS read
// and one AND per lane.  The row's adjacency is repacked on load from teaser_graph's layout (vertex j at bit j >> 5 of word j & 31) to
// vertex j at bit j & 31 of word j >> 5, 32 ballots per pair of vertices, so that "the lowest index in the set" is a ballot of the
// non-zero words, a trailing-zero count, a readlane and another trailing-zero count -- no cross-lane minimum -- and sits in LDS
// (stride x words x 4 B, 128 KiB at stride 1024, requested dynamically): a colouring step never leaves the CU.
// Search stack: the candidate set of every depth and the order lists (vertex, colour) of the nodes on the current path live in the
// workspace, per workgroup, not per row: stride (stride + 1) / 2 entries + (stride + 1) sets.  A list is gathered 64 entries at a time
// (entry k waits on lane k & 63) and stored by the whole wave, read back one entry per branch after a barrier; a set is written and
// read by the lane that owns the word.  Both also go to small direct-mapped LDS windows (the latest 1024 entries by offset, the
// latest 64 sets by depth, each with a tag), which is where the walk near the leaves finds them; the workspace serves the rest.  The
// alternative -- only P per depth, recolouring on return -- would save the 2 MiB per workgroup but colour every node once per child.
// No atomics, no workgroup waits for another, vector stores only.  Every loop is bounded by the step counter or by M.
#include <algorithm>

#include "common.h"
#include "teaser_clique_core.h"

namespace mp {

using namespace teaser;

// ---- a caller's adjacency matrix -> the bit matrix and degrees of teaser_graph -----------------------------------------------------------
// a workgroup = 32 vertices x 32 words; an edge when i != j and a[i][j] | a[j][i]: symmetric by construction
__global__ __launch_bounds__(kThreads) void clique_pack(const uint8_t* __restrict__ a, const int32_t* __restrict__ counts, int stride,
                                                        uint32_t* __restrict__ adj, int32_t* __restrict__ deg, int32_t* __restrict__ m_arr) {
  const int row = blockIdx.y, tile = blockIdx.x, tid = threadIdx.x;
  const int M = counts ? max(0, min(counts[row], stride)) : stride;
  if (tile == 0 && tid == 0) m_arr[row] = M;
  if (tile * 32 >= M) return;
  const uint8_t* A = a + (size_t)row * stride * stride;
  const int w = tid & 31, i = tile * 32 + (tid >> 5);
  uint32_t word = 0u;
  if (i < M) {
    for (int b = 0; b < 32; ++b) {
      const int j = b * 32 + w;
      if (j < M && j != i && (A[(size_t)i * stride + j] | A[(size_t)j * stride + i])) word |= 1u << b;   // i, j < M <= stride
    }
  }
  adj[((size_t)row * kMaxPoints + i) * kWords + w] = word;   // i < kMaxPoints: tile < 32
  int c = __popc(word);
  for (int off = 16; off > 0; off >>= 1) c += __shfl_xor(c, off);
  if (w == 0 && i < M) deg[(size_t)row * kMaxPoints + i] = c;
}

// ---- the search ---------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool any_bit(uint32_t word) { return __ballot(word != 0u) != 0ull; }

// the lowest vertex of a non-empty set (uniform): *lane_of = the lane that owns its word, *bit_of = its bit
__device__ __forceinline__ int lowest_vertex(uint32_t word, unsigned long long nonzero, int* lane_of, int* bit_of) {
  const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)nonzero) - 1);
  const uint32_t wv = (uint32_t)__builtin_amdgcn_readlane((int)word, l);
  const int b = __ffs((int)wv) - 1;
  *lane_of = l;
  *bit_of = b;
  return l * 32 + b;
}

// entries first .. first + n - 1 of the order lists, from lane 0 .. n - 1: to the stack in the workspace and, tagged, to its LDS window
__device__ __forceinline__ void store_entries(uint32_t* __restrict__ order, uint32_t* ocache, int first, int n, int lane, uint32_t e) {
  if (lane < n) {
    const int o = first + lane;
    order[o] = e;
    ocache[o & (kCliqueOrderCache - 1)] = cache_word(e, o);
  }
}

__global__ __launch_bounds__(kCliqueLanes) void clique_search(const uint32_t* __restrict__ adj, const int32_t* __restrict__ core_in,
                                                              const int32_t* __restrict__ m_arr, int n_rows, int stride, int max_steps,
                                                              uint32_t* __restrict__ order_ws, uint32_t* __restrict__ pset_ws,
                                                              int32_t* __restrict__ sel_out, int32_t* __restrict__ sel_list, int32_t* __restrict__ msel,
                                                              int32_t* __restrict__ info_out) {
  extern __shared__ uint32_t lds[];
  const int W = clique_words(stride);
  uint32_t* adjL = lds;                                        // [stride][W]
  int32_t* off = (int32_t*)(adjL + (size_t)stride * W);        // [stride + 1] first entry of the order list of every depth
  int32_t* idx = off + (stride + 1);                           // [stride + 1] entries of it not walked yet
  int32_t* Rv = idx + (stride + 1);                            // [stride + 1] R
  uint32_t* ocache = (uint32_t*)(Rv + (stride + 1));           // [kCliqueOrderCache] the latest order entries, tagged with their offset
  uint32_t* pcache = ocache + kCliqueOrderCache;               // [kCliqueSetCache][W] the latest candidate sets, by depth
  int32_t* ptag = (int32_t*)(pcache + (size_t)kCliqueSetCache * W);   // [kCliqueSetCache] the depth a slot of pcache holds
  uint16_t* coreL = (uint16_t*)(ptag + kCliqueSetCache);       // [stride]
  const int lane = threadIdx.x, half = lane >> 5, l32 = lane & 31;
  const bool own = lane < W;                                   // this lane owns a word
  const int wl = own ? lane : 0;                               // (a lane without a word reads word 0 and holds empty sets: no branch)
  uint32_t* order = order_ws + (size_t)blockIdx.x * clique_order_entries(stride);
  uint32_t* pset = pset_ws + (size_t)blockIdx.x * clique_pset_words(stride);

  for (int row = blockIdx.x; row < n_rows; row += gridDim.x) {
    const int M = max(0, min(m_arr[row], min(stride, kMaxPoints)));
    __syncthreads();   // (the row before is done with the LDS)
    // adjacency: two vertices per pass, one per half-wave; word w of the new layout = bit w of the 32 old words
    for (int v0 = 0; v0 < M; v0 += 2) {
      const int v = v0 + half;
      const uint32_t old = v < M ? adj[((size_t)row * kMaxPoints + v) * kWords + l32] : 0u;
      uint32_t mine = 0u;
      for (int w = 0; w < W; ++w) {
        const unsigned long long ball = __ballot(((old >> w) & 1u) != 0u);
        if (l32 == w) mine = half ? (uint32_t)(ball >> 32) : (uint32_t)ball;
      }
      if (l32 == (v >> 5)) mine &= ~(1u << (v & 31));          // never a loop, whatever the bits say: the stack bound needs it
      if (l32 < W && v < M) adjL[v * W + l32] = mine;          // v < M <= stride
    }
    int kmax = 0;
    for (int v = lane; v < M; v += kCliqueLanes) {
      const int c = core_in[(size_t)row * kMaxPoints + v];
      coreL[v] = (uint16_t)c;
      kmax = max(kmax, c);
    }
    kmax = wave_max_all(kmax);
    for (int k = lane; k < kCliqueOrderCache; k += kCliqueLanes) ocache[k] = 0xFFFFFFFFu;   // (no offset has this tag)
    if (lane < kCliqueSetCache) ptag[lane] = -1;
    __syncthreads();
    const int upper = M > 0 ? kmax + 1 : 0;

    // ---- greedy lower bound ----
    uint32_t Pw = 0u, bestw = 0u;
    if (own) Pw = (lane * 32 + 32 <= M) ? 0xFFFFFFFFu : (lane * 32 < M ? (1u << (M - lane * 32)) - 1u : 0u);
    int bsize = 0;
    for (int it = 0; it < M; ++it) {   // (every pass takes a vertex out of P)
      uint32_t key = 0u;               // (a key is never 0: v < 0xFFFF)
      for (uint32_t t = Pw; t; t &= t - 1u) {
        const int v = lane * 32 + __ffs((int)t) - 1;
        key = max(key, greedy_key(coreL[v], v));
      }
      key = wave_max_all(key);
      if (key == 0u) break;
      const int v = greedy_key_vertex(key);   // in P: v < M
      if (lane == (v >> 5)) bestw |= 1u << (v & 31);
      ++bsize;
      Pw &= adjL[v * W + wl];
    }

    // ---- branch and bound ----
    int steps = 0, exact = 1;
    Pw = 0u;
    if (bsize != upper && own)
      for (int b = 0; b < 32; ++b) {
        const int v = lane * 32 + b;
        if (v < M && (int)coreL[v] >= bsize) Pw |= 1u << b;
      }
    if (any_bit(Pw)) {
      int depth = 0;
      bool colour = true;
      off[0] = 0;
      for (;;) {   // (every pass colours a node, takes a list entry or leaves a node: bounded by the steps, max_steps + M at most)
        if (colour) {
          const int base = off[depth];
          int cnt = 0;
          uint32_t U = Pw, pend = 0u;                    // pend: entry cnt of the list waits on lane cnt & 63 for the next store
          for (int k = 1; any_bit(U); ++k) {           // (a class colours at least one vertex)
            uint32_t Q = U;
            for (;;) {                                   // (a pass takes at least v out of Q)
              const unsigned long long nz = __ballot(Q != 0u);
              if (!nz) break;
              int lo, b;
              const int v = lowest_vertex(Q, nz, &lo, &b);
              if (lane == (cnt & 63)) pend = order_entry(v, k);
              ++cnt;
              if ((cnt & 63) == 0) store_entries(order, ocache, base + cnt - 64, 64, lane, pend);
              const uint32_t keep = lane == lo ? ~(1u << b) : 0xFFFFFFFFu;
              Q &= ~adjL[v * W + wl] & keep;
              U &= keep;
            }
          }
          // base + cnt <= stride (stride + 1) / 2: a child's P is its parent's without v at least, and |P0| <= M <= stride
          store_entries(order, ocache, base + (cnt & ~63), cnt & 63, lane, pend);
          steps += cnt;
          idx[depth] = cnt;
          off[depth + 1] = base + cnt;                   // depth <= M - 1 < stride
          __syncthreads();                               // the list, for every lane
          if (steps > max_steps) { exact = 0; break; }
          colour = false;
        }
        const int i = idx[depth];
        bool leave = i == 0;
        int v = 0;
        if (!leave) {
          const int o = off[depth] + i - 1;
          const uint32_t c = ocache[o & (kCliqueOrderCache - 1)];
          const uint32_t e = cache_tag(c) == order_tag(o) ? cache_entry(c) : order[o];   // (uniform)
          v = entry_vertex(e);
          leave = depth + entry_colour(e) <= bsize;
        }
        if (leave) {
          if (depth == 0) break;
          --depth;
          const int slot = depth & (kCliqueSetCache - 1);
          if (ptag[slot] == depth) Pw = own ? pcache[slot * W + lane] : 0u;   // (uniform)
          else Pw = own ? pset[(size_t)depth * W + lane] : 0u;
          continue;
        }
        idx[depth] = i - 1;
        Rv[depth] = v;
        const uint32_t P2 = Pw & adjL[v * W + wl];
        if (lane == (v >> 5)) Pw &= ~(1u << (v & 31));
        if (!any_bit(P2)) {
          if (depth + 1 > bsize) {                       // strictly larger: the first maximum clique met is kept
            bsize = depth + 1;
            bestw = 0u;
            for (int d = 0; d <= depth; ++d) {
              const int r = Rv[d];
              if (lane == (r >> 5)) bestw |= 1u << (r & 31);
            }
          }
        } else {
          const int slot = depth & (kCliqueSetCache - 1);
          if (own) {                                     // the lane that wrote a word is the one that reads it back
            pset[(size_t)depth * W + lane] = Pw;
            pcache[slot * W + lane] = Pw;
          }
          ptag[slot] = depth;
          ++depth;
          Pw = P2;
          colour = true;
        }
      }
    }

    // ---- the members in ascending order ----
    __syncthreads();
    if (own) off[lane] = (int32_t)bestw;                 // (W <= stride: inside off)
    __syncthreads();
    for (int v = lane; v < M; v += kCliqueLanes) sel_out[(size_t)row * kMaxPoints + v] = (int)(((uint32_t)off[v >> 5] >> (v & 31)) & 1u);
    int before = 0;
    for (int w = 0; w < lane && w < W; ++w) before += __popc((uint32_t)off[w]);
    int32_t* list = sel_list + (size_t)row * kMaxPoints;
    for (uint32_t t = bestw; t; t &= t - 1u) list[before++] = lane * 32 + __ffs((int)t) - 1;   // before < bsize <= M
    for (int k = bsize + lane; k < stride; k += kCliqueLanes) list[k] = -1;
    if (lane == 0) {
      msel[row] = bsize;
      if (info_out) {
        int32_t* f = info_out + (size_t)row * kCliqueInfo;
        f[0] = bsize; f[1] = upper; f[2] = exact; f[3] = steps;
      }
    }
  }
}

CliqueWs clique_search_ws(WsCarver& c, int n_rows, int stride) {
  const size_t blocks = (size_t)std::min(std::max(n_rows, 0), kCliqueMaxBlocks);
  CliqueWs w;
  w.order = c.take<uint32_t>(blocks * clique_order_entries(stride));
  w.pset = c.take<uint32_t>(blocks * clique_pset_words(stride));
  return w;
}

int clique_pack_launch(const uint8_t* adjacency, const int32_t* counts, int n_rows, int stride, uint32_t* adj, int32_t* deg, int32_t* m_arr, hipStream_t s) {
  hipLaunchKernelGGL(clique_pack, dim3(kMaxPoints / 32, n_rows), dim3(kThreads), 0, s, adjacency, counts, stride, adj, deg, m_arr);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

int clique_search_launch(const uint32_t* adj, const int32_t* core, const int32_t* m_arr, int n_rows, int stride, int max_steps, int32_t* sel,
                         int32_t* sel_list, int32_t* msel, int32_t* info, const CliqueWs& ws, hipStream_t s) {
  const int blocks = std::min(n_rows, kCliqueMaxBlocks);
  const size_t lds = clique_lds_bytes(stride);
  if (lds > 64 * 1024) MP_CHECK_HIP(hipFuncSetAttribute((const void*)clique_search, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(clique_search, dim3(blocks), dim3(kCliqueLanes), lds, s, adj, core, m_arr, n_rows, stride, max_steps, ws.order, ws.pset, sel, sel_list,
                     msel, info);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

}  // namespace mp
