// teaser_clique_core.h -- the rule of the exact maximum-clique inlier selection of the TEASER++ refiner (TEASER++'s default PMC_EXACT
// mode; selection "max_clique" of teaser.hip), shared by the device search (teaser_clique.hip) and the host emulation
// (tests/teaser_clique_emul.cpp).  The result is defined by a sequential algorithm, so it is unique: it does not depend on grid, block
// size or arrival order, and the kernel reproduces it exactly -- members, flag and step count.
//
// CONTRACT (per row: M <= 1024 vertices, the symmetric adjacency N(v) without loops, the core numbers core[v] of teaser_core.h CORES)
//   * BOUNDS.  kmax = the largest core number; a clique has at most kmax + 1 members (0 for M = 0): the info's upper bound.
//   * GREEDY [greedy_key].  R = {}, P = every vertex.  Until P is empty: v = the vertex of P with the largest core number, a tie to the
//     lowest index (the largest greedy_key); R += v; P &= N(v).  best = R.
//   * SHORTCUT.  |best| == kmax + 1 (or M == 0): best is a maximum clique, exact = 1, steps = 0, no search.
//   * ROOT.  P0 = {v : core[v] >= |best|}: a clique larger than best only has members of at least that core number.  expand({}, P0).
//   * expand(R, P).  COLOUR: classes k = 1, 2, ..: Q = the uncoloured vertices of P; until Q is empty: v = the lowest index in Q, v gets
//     colour k and is appended to the node's order list [order_entry], Q -= {v} + N(v); the next class starts from what is still
//     uncoloured.  Every colour assignment is one STEP.  BUDGET: after a node's colouring, steps > max_steps ends the whole search: best
//     is returned with exact = 0 (TEASER++'s max_clique_time_limit also returns the best clique so far; steps, unlike time, reproduce).
//     Steps overshoot max_steps by at most M.  BRANCH: walk the order list backwards; at entry (v, colour): |R| + colour <= |best| ends the
//     node.  Else R' = R + v, P' = P & N(v), and v leaves P.  P' empty: |R'| > |best| (strictly: the first maximum clique met is
//     kept) replaces best by R'.  P' not empty: expand(R', P').
//   * OUTPUT.  The members of best in ascending order (the selected set of the refiner: m < 3 still rejects the row), and the info
//     record of kCliqueInfo int32: size, upper bound kmax + 1, exact, steps.
//   Every loop is bounded by the step counter or by M, so a pathological graph ends with exact = 0; it never runs long.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "teaser_core.h"

namespace mp {
namespace teaser {

constexpr int kSelectMaxClique = 2;                // beside kSelectKcore, kSelectNone
constexpr int kCliqueInfo = 4;                     // per-row info: size, upper bound, exact, steps
constexpr int kCliqueDefaultSteps = 1 << 19;       // max_steps when the caller gives none: the measured budget of DESIGN.md 3.14
constexpr int kCliqueStepCeiling = 16 * kCliqueDefaultSteps;   // the largest max_steps an argument may ask for
constexpr int kCliqueLanes = 64;                   // one wave searches one row; lane w < words owns word w of every live bit set
constexpr int kCliqueMaxBlocks = 256;              // rows are spread over at most this many workgroups (one search stack each)

TSR_HD bool clique_steps_ok(int max_steps) { return max_steps >= 0 && max_steps <= kCliqueStepCeiling; }

// the larger key = the larger core number, then the lower index (core, v < 2^15)
TSR_HD uint32_t greedy_key(int core, int v) { return ((uint32_t)core << 16) | (uint32_t)(0xFFFF - v); }
TSR_HD int greedy_key_vertex(uint32_t key) { return 0xFFFF - (int)(key & 0xFFFFu); }

// an entry of a node's order list
TSR_HD uint32_t order_entry(int v, int colour) { return ((uint32_t)colour << 16) | (uint32_t)v; }
TSR_HD int entry_vertex(uint32_t e) { return (int)(e & 0xFFFFu); }
TSR_HD int entry_colour(uint32_t e) { return (int)(e >> 16); }

// the LDS windows of the search stack: the latest kCliqueOrderCache entries by offset, the latest kCliqueSetCache sets by depth
constexpr int kCliqueOrderCache = 1024;
constexpr int kCliqueSetCache = 64;
// a cached entry: vertex (10 bits) | colour (11 bits) | offset >> 10 (11 bits: an offset is under 2^19 + 2^10; 2047 is no offset's tag)
TSR_HD uint32_t order_tag(int offset) { return (uint32_t)offset >> 10; }
TSR_HD uint32_t cache_word(uint32_t entry, int offset) { return (entry & 0x3FFu) | ((entry >> 16) << 10) | (order_tag(offset) << 21); }
TSR_HD uint32_t cache_tag(uint32_t c) { return c >> 21; }
TSR_HD uint32_t cache_entry(uint32_t c) { return order_entry((int)(c & 0x3FFu), (int)((c >> 10) & 0x7FFu)); }

// words of a bit set over `stride` vertices, vertex j at bit (j & 31) of word (j >> 5) (the search's own layout)
TSR_HD int clique_words(int stride) { return (stride + 31) >> 5; }

// the search stack of one workgroup: the order lists of the nodes on the current path (a child's list is shorter than its parent's by
// at least one: stride (stride + 1) / 2 entries) and the candidate set P of every depth
TSR_HD size_t clique_order_entries(int stride) { return (size_t)stride * (size_t)(stride + 1) / 2; }
TSR_HD size_t clique_pset_words(int stride) { return (size_t)(stride + 1) * (size_t)clique_words(stride); }

// LDS of one workgroup: the row's adjacency [stride][words], three int32 per depth (list offset, walk position, the vertex taken), the
// two windows with the sets' tags, and the core numbers as uint16: 157964 B at stride 1024, under the 160 KiB of a gfx950 CU
TSR_HD size_t clique_lds_bytes(int stride) {
  const size_t words = (size_t)stride * (size_t)clique_words(stride) + 3 * (size_t)(stride + 1) + kCliqueOrderCache +
                       (size_t)kCliqueSetCache * (size_t)clique_words(stride) + kCliqueSetCache;
  return words * 4 + (((size_t)stride * 2 + 3) & ~(size_t)3);
}

}  // namespace teaser

#if defined(__HIPCC__)
// teaser_clique.hip, called by the entry points of teaser.hip.  adj [n][kMaxPoints][kWords] in the layout of teaser_graph; core, sel,
// sel_list [n][kMaxPoints]; msel, m_arr [n]; info [n][kCliqueInfo] or null.
struct WsCarver;
struct CliqueWs { uint32_t *order, *pset; };   // the search stacks of min(n_rows, kCliqueMaxBlocks) workgroups
CliqueWs clique_search_ws(WsCarver& c, int n_rows, int stride);
int clique_pack_launch(const uint8_t* adjacency, const int32_t* counts, int n_rows, int stride, uint32_t* adj, int32_t* deg, int32_t* m_arr, hipStream_t s);
int clique_search_launch(const uint32_t* adj, const int32_t* core, const int32_t* m_arr, int n_rows, int stride, int max_steps, int32_t* sel,
                         int32_t* sel_list, int32_t* msel, int32_t* info, const CliqueWs& ws, hipStream_t s);
#endif
}  // namespace mp
