// rle.hip -- the device side of BOP's result files: COCO run-length encoding of binary masks, both ways.
//
// The rules are rle_core.h, shared with the host emulation of the tests; this file adds the work distribution.  Every result is an
// integer picked by comparisons or an exclusive sum of integers in one fixed order, so neither the grid, rows_per_segment nor the
// arrival order can change one.  No atomics, no workgroup waits on another, every search has a fixed number of steps.
//
//   rle_walk_kernel<WRITE>  one lane per job (mask, row segment, unit of 16 columns), the unit fastest: neighbouring lanes read
//                           neighbouring 16 bytes of one row.  A lane walks down its rows: 16 bytes per load when the unit lies inside the
//                           row and its address is 16-byte aligned, else byte loads of the columns inside the row (a width that is no
//                           multiple of 16, a tensor sliced at an odd byte); the non-zero bytes are marked in their high bits
//                           [dap::nonzero_bytes], the row above (for a mask's first row: the last row, one column to the left) is kept in
//                           the same form, and their exclusive-or marks the transitions.  WRITE = false counts them per column and keeps
//                           the last position, and the job's area and extent; WRITE = true starts from the scanned rank and position of
//                           its entries and stores the differences into `counts`, each store guarded by the list's length.
//   rle_scan_kernel         one workgroup per mask: exclusive sum (rank) and exclusive maximum (position before) over the mask's
//                           entries in walk order, in place.  A thread owns a column (its S entries follow each other in walk order, and
//                           a wave reads neighbouring columns), 256 columns at a time with a carry; then the mask's number of counts, its
//                           area and box from the jobs' partial results [block_primitives.h].
//   rle_ends_kernel         one workgroup per list: the cumulative ends of the runs (int64 sums, stored as int32: they are used only
//                           when the list is well formed, and then fit) and the list's status.
//   rle_seek_kernel         one lane per entry (mask, row segment, column): the run of the entry's first pixel [rle::run_of].  The
//                           searches of a job's 16 columns would follow each other in one lane; here they run side by side.
//   rle_fill_kernel         the walk's jobs again: a lane keeps, per column, its run and the row at which the column leaves it (in LDS,
//                           its own slots only) and the earliest such row in a register; a row before that is one 16-byte store of the
//                           pixels at hand (bytes where the walk would load bytes); at that row the columns that left step to the next
//                           run, their loads in flight together, and only a column that stepped into a run of length zero searches
//                           (a chain of dependent loads per column and row was the whole cost of this kernel).  The parity of the run
//                           is the pixel.  A list with a non-zero status is never searched: its mask is zeros.
// WORKSPACE of mp_rle_count / mp_rle_encode (the encode reads what the count of the same masks left there): the offsets [n + 1] int64,
// per entry its count and last position [n, S, w] int32 twice (by segment, then column: every kernel touches them coalesced), per job
// its five partial results, per mask the number of transitions and the last position.  Of mp_rle_decode: the offsets, one int32 per
// count, one per entry.
#include "common.h"
#include "rle_core.h"

namespace mp {

constexpr int kRleBlock = 256;       // the scans and the seek
constexpr int kRleWaves = kRleBlock / 64;
constexpr int kRleWalkBlock = 64;    // the walks and the fill: one wave, so that a few hundred jobs' worth of rows still spread over the CUs
constexpr int kRleAhead = 4;         // rows a walking lane loads before it looks at the first

struct RleUnit {
  uint64_t lo, hi;   // the high bit of byte k of lo: column 16 u + k is set; hi: columns 16 u + 8 ..
};

// columns x0 .. x0 + 15 of one row (row = its first byte); columns outside [0, w) read nothing and are unset
__device__ __forceinline__ RleUnit rle_load_unit(const uint8_t* __restrict__ row, int x0, int w) {
  RleUnit r;
  const uint8_t* p = row + x0;
  if (x0 >= 0 && x0 + rle::kUnit <= w && ((uintptr_t)p & 15) == 0) {
    const uint4 v = *reinterpret_cast<const uint4*>(p);
    r.lo = dap::nonzero_bytes((uint64_t)v.x | ((uint64_t)v.y << 32));
    r.hi = dap::nonzero_bytes((uint64_t)v.z | ((uint64_t)v.w << 32));
    return r;
  }
  uint64_t lo = 0, hi = 0;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int xa = x0 + k, xb = x0 + 8 + k;
    if (xa >= 0 && xa < w && rle::is_set(row[xa])) lo |= 0x80ull << (8 * k);
    if (xb >= 0 && xb < w && rle::is_set(row[xb])) hi |= 0x80ull << (8 * k);
  }
  r.lo = lo;
  r.hi = hi;
  return r;
}

struct RleJob {
  int m, s, u, y0, y1;
};

__device__ __forceinline__ bool rle_job(long long n_jobs, int S, int U, int h, int rows, RleJob* j) {
  const long long g = (long long)blockIdx.x * kRleWalkBlock + threadIdx.x;
  if (g >= n_jobs) return false;
  j->u = (int)(g % U);
  j->s = (int)((g / U) % S);
  j->m = (int)(g / ((long long)U * S));
  j->y0 = j->s * rows;
  j->y1 = j->y0 + rows < h ? j->y0 + rows : h;
  return true;
}

template <bool WRITE>
__global__ __launch_bounds__(kRleWalkBlock) void rle_walk_kernel(const uint8_t* __restrict__ masks, int h, int w, int rows, int S, int U,
                                                             long long n_jobs, int32_t* __restrict__ ent_count, int32_t* __restrict__ ent_last,
                                                             int32_t* __restrict__ job_stats, const int32_t* __restrict__ mask_tot,
                                                             const int64_t* __restrict__ offsets, int32_t* __restrict__ counts) {
  RleJob j;
  if (!rle_job(n_jobs, S, U, h, rows, &j)) return;
  const size_t hw = (size_t)h * w;
  const uint8_t* mask = masks + (size_t)j.m * hw;
  const int x0 = j.u * rle::kUnit;
  const size_t ent0 = ((size_t)j.m * S + j.s) * w + x0;   // the entries of columns x0 ..
  int rank[rle::kUnit], before[rle::kUnit];                // of the next transition of column k: its rank, the position before it
#pragma unroll
  for (int k = 0; k < rle::kUnit; ++k) {
    const bool in = WRITE && x0 + k < w;
    rank[k] = in ? ent_count[ent0 + k] : 0;
    before[k] = in ? ent_last[ent0 + k] : 0;
  }
  int64_t off = 0;
  int n_list = 0;
  if (WRITE) {
    off = offsets[j.m];
    const int64_t len = offsets[j.m + 1] - off;
    n_list = len < 0 ? 0 : (len > 2147483647LL ? 2147483647 : (int)len);
  }
  // the pixels before the first row's in walk order: the row above, or the mask's last row one column to the left (none before p = 0)
  RleUnit above = j.y0 > 0 ? rle_load_unit(mask + (size_t)rle::prev_y(j.y0, h) * w, x0, w)
                           : rle_load_unit(mask + (size_t)rle::prev_y(0, h) * w, rle::prev_x(x0, 0), w);
  if (j.y0 == 0 && x0 + rle::kUnit > w) {   // columns >= w of the last unit have no pixel: keep them unset on both sides
    const int keep = w - x0;                // 1 .. 15 columns
    above.lo &= keep >= 8 ? ~0ull : ((1ull << (8 * keep)) - 1ull);
    above.hi &= keep <= 8 ? 0ull : ((1ull << (8 * (keep - 8))) - 1ull);
  }
  int area = 0, y_min = rle::kNoMin, y_max = -1;
  uint64_t any_lo = 0, any_hi = 0;
  for (int yb = j.y0; yb < j.y1; yb += kRleAhead) {
    RleUnit ahead[kRleAhead];
#pragma unroll
    for (int i = 0; i < kRleAhead; ++i)
      ahead[i] = yb + i < j.y1 ? rle_load_unit(mask + (size_t)(yb + i) * w, x0, w) : RleUnit{0ull, 0ull};
#pragma unroll
    for (int i = 0; i < kRleAhead; ++i) {
      const int y = yb + i;
      if (y >= j.y1) break;
      const RleUnit cur = ahead[i];
      const uint64_t t_lo = cur.lo ^ above.lo, t_hi = cur.hi ^ above.hi;
      above = cur;
      if (!WRITE && (cur.lo | cur.hi)) {
        area += __popcll(cur.lo) + __popcll(cur.hi);
        any_lo |= cur.lo;
        any_hi |= cur.hi;
        y_min = y < y_min ? y : y_min;
        y_max = y;
      }
      if ((t_lo | t_hi) == 0) continue;
#pragma unroll
      for (int k = 0; k < rle::kUnit; ++k) {
        const uint64_t t = k < 8 ? t_lo >> (8 * k + 7) : t_hi >> (8 * (k - 8) + 7);
        if (t & 1) {
          const int p = (x0 + k) * h + y;
          if (WRITE && (unsigned)rank[k] < (unsigned)n_list) counts[off + rank[k]] = p - before[k];   // (unsigned: a rank the count did not leave)
          ++rank[k];
          before[k] = p;
        }
      }
    }
  }
  if (WRITE) {
    if (j.s == 0 && j.u == 0) {   // the list's last entry: from the last transition to h * w
      const int n_trans = mask_tot[2 * j.m];
      if ((unsigned)n_trans < (unsigned)n_list) counts[off + n_trans] = (int32_t)hw - mask_tot[2 * j.m + 1];
    }
    return;
  }
#pragma unroll
  for (int k = 0; k < rle::kUnit; ++k)
    if (x0 + k < w) {
      ent_count[ent0 + k] = rank[k];
      ent_last[ent0 + k] = before[k];
    }
  int x_min = rle::kNoMin, x_max = -1;
  if (any_lo | any_hi) {
    x_min = x0 + (any_lo ? __ffsll((long long)any_lo) - 1 : 64 + __ffsll((long long)any_hi) - 1) / 8;
    x_max = x0 + (any_hi ? 8 + (63 - __clzll((long long)any_hi)) / 8 : (63 - __clzll((long long)any_lo)) / 8);
  }
  int32_t* st = job_stats + (((size_t)j.m * S + j.s) * U + j.u) * rle::kStatsPerJob;
  st[0] = area;
  st[1] = x_min;
  st[2] = x_max;
  st[3] = y_min;
  st[4] = y_max;
}

__global__ __launch_bounds__(kRleBlock) void rle_scan_kernel(int w, int S, int U, int32_t* __restrict__ ent_count, int32_t* __restrict__ ent_last,
                                                             const int32_t* __restrict__ job_stats, int32_t* __restrict__ mask_tot,
                                                             int32_t* __restrict__ n_counts, int32_t* __restrict__ areas,
                                                             int32_t* __restrict__ boxes) {
  __shared__ int wave_sum[kRleWaves], wave_max[kRleWaves], red[kRleWaves];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long n_ent = (long long)w * S;
  int32_t* cnt = ent_count + (size_t)m * n_ent;
  int32_t* last = ent_last + (size_t)m * n_ent;
  int carry_sum = 0, carry_max = 0;
  // a thread owns a column: its S entries follow each other in walk order, and the threads of a wave read neighbouring columns
  for (int xb = 0; xb < w; xb += kRleBlock) {
    const int x = xb + threadIdx.x;
    const bool in = x < w;
    int c = 0, l = 0;                                                   // the column's transitions, its last position
    if (in)
      for (int s = 0; s < S; ++s) {
        const size_t at = (size_t)s * w + x;
        c += cnt[at];
        l = last[at] > l ? last[at] : l;
      }
    int sum = c, mx = l;                                                // inclusive over the wave
    for (int d = 1; d < 64; d <<= 1) {
      const int os = __shfl_up(sum, d), om = __shfl_up(mx, d);
      if (lane >= d) {
        sum += os;
        mx = om > mx ? om : mx;
      }
    }
    int mx_before = __shfl_up(mx, 1);
    if (lane == 0) mx_before = 0;
    __syncthreads();
    if (lane == 63) {
      wave_sum[wave] = sum;
      wave_max[wave] = mx;
    }
    __syncthreads();
    int base_sum = carry_sum, base_max = carry_max;
    for (int k = 0; k < kRleWaves; ++k) {
      if (k == wave && in) {
        int run_sum = base_sum + sum - c, run_max = base_max > mx_before ? base_max : mx_before;   // before the column's first entry
        for (int s = 0; s < S; ++s) {
          const size_t at = (size_t)s * w + x;
          const int cs = cnt[at], ls = last[at];
          cnt[at] = run_sum;
          last[at] = run_max;
          run_sum += cs;
          run_max = ls > run_max ? ls : run_max;
        }
      }
      base_sum += wave_sum[k];
      base_max = wave_max[k] > base_max ? wave_max[k] : base_max;
    }
    carry_sum = base_sum;
    carry_max = base_max;
  }
  // the mask's area and box from its jobs
  int area = 0, x_min = rle::kNoMin, x_max = -1, y_min = rle::kNoMin, y_max = -1;
  const int32_t* st = job_stats + (size_t)m * S * U * rle::kStatsPerJob;
  for (long long k = threadIdx.x; k < (long long)S * U; k += kRleBlock) {
    const int32_t* q = st + k * rle::kStatsPerJob;
    area += q[0];
    x_min = q[1] < x_min ? q[1] : x_min;
    x_max = q[2] > x_max ? q[2] : x_max;
    y_min = q[3] < y_min ? q[3] : y_min;
    y_max = q[4] > y_max ? q[4] : y_max;
  }
  area = block_sum_all<kRleWaves>(area, red);
  x_min = block_min_all<kRleWaves>(x_min, red);
  x_max = block_max_all<kRleWaves>(x_max, red);
  y_min = block_min_all<kRleWaves>(y_min, red);
  y_max = block_max_all<kRleWaves>(y_max, red);
  if (threadIdx.x != 0) return;
  mask_tot[2 * m] = carry_sum;
  mask_tot[2 * m + 1] = carry_max;
  n_counts[m] = carry_sum + 1;
  if (areas) areas[m] = area;
  if (boxes) {
    boxes[4 * m + 0] = area ? x_min : 0;
    boxes[4 * m + 1] = area ? y_min : 0;
    boxes[4 * m + 2] = x_max;
    boxes[4 * m + 3] = y_max;
  }
}

__global__ __launch_bounds__(kRleBlock) void rle_ends_kernel(const int32_t* __restrict__ counts, const int64_t* __restrict__ offsets, long long hw,
                                                             int32_t* __restrict__ ends, int32_t* __restrict__ status) {
  __shared__ long long wave_sum[kRleWaves];
  __shared__ int red[kRleWaves];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t off = offsets[m], n_runs = offsets[m + 1] - off;   // validated on the host: inside the counts, n_runs in 0 .. 2^31 - 1
  long long carry = 0;
  int negative = 0;
  for (int64_t i0 = 0; i0 < n_runs; i0 += kRleBlock) {
    const int64_t i = i0 + threadIdx.x;
    const bool in = i < n_runs;
    const int c = in ? counts[off + i] : 0;
    negative |= c < 0;
    long long sum = c;
    for (int d = 1; d < 64; d <<= 1) {
      const long long o = shfl_up_any(sum, d);
      if (lane >= d) sum += o;
    }
    __syncthreads();
    if (lane == 63) wave_sum[wave] = sum;
    __syncthreads();
    long long base = carry;
    for (int k = 0; k < kRleWaves; ++k) {
      if (k == wave && in) ends[off + i] = (int32_t)(base + sum);
      base += wave_sum[k];
    }
    carry = base;
  }
  negative = block_reduce_all<kRleWaves>(negative, red, OrOp());
  if (threadIdx.x == 0) status[m] = rle::status_of(n_runs, negative != 0, carry, hw);
}

// the run of the first pixel of every entry (mask, row segment s, column x), one lane each: ent_run [n, S, w]
__global__ __launch_bounds__(kRleBlock) void rle_seek_kernel(const int32_t* __restrict__ ends, const int64_t* __restrict__ offsets,
                                                             const int32_t* __restrict__ status, int h, int w, int rows, int S, long long n_ent,
                                                             int32_t* __restrict__ ent_run) {
  const long long g = (long long)blockIdx.x * kRleBlock + threadIdx.x;
  if (g >= n_ent) return;
  const int x = (int)(g % w), s = (int)((g / w) % S), m = (int)(g / ((long long)w * S));
  int run = 0;
  if (status[m] == 0) {   // a well-formed list: its last end is h * w, beyond every pixel
    const int64_t off = offsets[m];
    run = rle::run_of(ends + off, (int)(offsets[m + 1] - off), x * h + s * rows);
  }
  ent_run[g] = run;
}

// bit k of bits -> byte k of four words, 0 / 1 (a nibble times 1 + 2^7 + 2^14 + 2^21 puts its bit i at 8 i; the other copies are masked)
__device__ __forceinline__ uint4 rle_spread(uint32_t bits) {
  const uint32_t m = 0x00204081u, keep = 0x01010101u;
  return make_uint4(((bits & 15u) * m) & keep, (((bits >> 4) & 15u) * m) & keep, (((bits >> 8) & 15u) * m) & keep, (((bits >> 12) & 15u) * m) & keep);
}

__global__ __launch_bounds__(kRleWalkBlock) void rle_fill_kernel(const int32_t* __restrict__ ends, const int64_t* __restrict__ offsets,
                                                                 const int32_t* __restrict__ status, const int32_t* __restrict__ ent_run, int h,
                                                                 int w, int rows, int S, int U, long long n_jobs, uint8_t* __restrict__ masks) {
  // per lane and column: the run at hand and the row at which the column's position reaches its end (a lane touches its own slots only)
  __shared__ int row_run[rle::kUnit][kRleWalkBlock], row_limit[rle::kUnit][kRleWalkBlock];
  RleJob j;
  if (!rle_job(n_jobs, S, U, h, rows, &j)) return;
  const int lane = threadIdx.x;
  uint8_t* mask = masks + (size_t)j.m * h * w;
  const int x0 = j.u * rle::kUnit;
  const bool ok = status[j.m] == 0;
  const int32_t* e = ends + offsets[j.m];
  const int n_runs = ok ? (int)(offsets[j.m + 1] - offsets[j.m]) : 0;
  const size_t ent0 = ((size_t)j.m * S + j.s) * w + x0;
  const int never = 2147483647;   // a column outside the mask, a malformed list: no run to leave
  int run[rle::kUnit];
#pragma unroll
  for (int k = 0; k < rle::kUnit; ++k) run[k] = ok && x0 + k < w ? ent_run[ent0 + k] : -1;
  uint32_t bits = 0;              // bit k: column k's pixel of the row at hand
  int next_y = never;             // the first row at which some column leaves its run
#pragma unroll
  for (int k = 0; k < rle::kUnit; ++k) {
    int limit = never;
    if (run[k] >= 0) {
      limit = e[run[k]] - (x0 + k) * h;   // p = (x0 + k) * h + y >= end  <=>  y >= limit
      bits |= (uint32_t)(run[k] & 1) << k;
    }
    row_run[k][lane] = run[k];
    row_limit[k][lane] = limit;
    next_y = limit < next_y ? limit : next_y;
  }
  uint4 v = rle_spread(bits);
  for (int y = j.y0; y < j.y1; ++y) {
    if (y >= next_y) {
      // the columns that left their run (only columns inside a well-formed mask: p < h * w = the list's last end, so run + 1 is a run
      // of the list) step to the next one, all their loads in flight together ...
      int lim[rle::kUnit], end[rle::kUnit];
#pragma unroll
      for (int k = 0; k < rle::kUnit; ++k) {
        lim[k] = row_limit[k][lane];
        run[k] = row_run[k][lane] + (y >= lim[k] ? 1 : 0);
        end[k] = y >= lim[k] ? e[run[k]] : 0;
      }
      next_y = never;
      bool behind = false;
#pragma unroll
      for (int k = 0; k < rle::kUnit; ++k) {
        if (y >= lim[k]) {
          lim[k] = end[k] - (x0 + k) * h;
          row_run[k][lane] = run[k];
          row_limit[k][lane] = lim[k];
          bits = (bits & ~(1u << k)) | ((uint32_t)(run[k] & 1) << k);
          behind = behind || y >= lim[k];
        }
        next_y = lim[k] < next_y ? lim[k] : next_y;
      }
      if (behind) {   // ... and one that stepped into a run of length zero searches
        next_y = never;
#pragma unroll 1
        for (int k = 0; k < rle::kUnit; ++k) {
          int limit = row_limit[k][lane];
          if (y >= limit) {
            const int r = rle::run_of(e, n_runs, (x0 + k) * h + y, row_run[k][lane]);
            limit = e[r] - (x0 + k) * h;
            row_run[k][lane] = r;
            row_limit[k][lane] = limit;
            bits = (bits & ~(1u << k)) | ((uint32_t)(r & 1) << k);
          }
          next_y = limit < next_y ? limit : next_y;
        }
      }
      v = rle_spread(bits);
    }
    uint8_t* q = mask + (size_t)y * w + x0;
    if (x0 + rle::kUnit <= w && ((uintptr_t)q & 15) == 0) {
      *reinterpret_cast<uint4*>(q) = v;
    } else {
      const uint32_t word[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int k = 0; k < rle::kUnit; ++k)
        if (x0 + k < w) q[k] = (uint8_t)((word[k >> 2] >> (8 * (k & 3))) & 1u);
    }
  }
}

struct RlePlan {
  int rows, S, U;
  long long n_jobs, n_ent;
};

static bool rle_plan(int n, int h, int w, int rows_per_segment, RlePlan* p) {
  if (n < 0 || rows_per_segment < 0 || !rle::dims_ok(h, w)) return false;
  p->rows = rle::rows_of(h, rows_per_segment);
  p->S = rle::segments(h, p->rows);
  p->U = rle::units(w);
  // n <= 2^31, S * U and S * w <= 2^31 * 2^31 / 16: no overflow before the test
  if ((long long)p->S * p->U > rle::kMaxJobs || (long long)p->S * w > rle::kMaxJobs) return false;
  p->n_jobs = (long long)n * p->S * p->U;
  p->n_ent = (long long)n * p->S * w;
  return p->n_jobs <= rle::kMaxJobs && p->n_ent <= rle::kMaxJobs;
}

struct RleWs {   // of mp_rle_count and mp_rle_encode
  int64_t* offsets;
  int32_t *ent_count, *ent_last, *job_stats, *mask_tot;
  size_t total;
  RleWs(void* base, int n, const RlePlan& p) {
    WsCarver c(base);
    offsets = c.take<int64_t>((size_t)n + 1);
    ent_count = c.take<int32_t>((size_t)p.n_ent);
    ent_last = c.take<int32_t>((size_t)p.n_ent);
    job_stats = c.take<int32_t>((size_t)p.n_jobs * rle::kStatsPerJob);
    mask_tot = c.take<int32_t>((size_t)n * 2);
    total = c.total();
  }
};

struct RleDecodeWs {
  int64_t* offsets;
  int32_t *ends, *ent_run;
  size_t total;
  RleDecodeWs(void* base, int n, long long capacity, const RlePlan& p) {
    WsCarver c(base);
    offsets = c.take<int64_t>((size_t)n + 1);
    ends = c.take<int32_t>((size_t)capacity);
    ent_run = c.take<int32_t>((size_t)p.n_ent);
    total = c.total(256);
  }
};

// h_offsets [n + 1]: starts at 0, does not descend, no list longer than an int32, ends within capacity
static bool rle_offsets_ok(const int64_t* h_offsets, int n, long long capacity) {
  if (h_offsets[0] != 0) return false;
  for (int m = 0; m < n; ++m) {
    const int64_t len = h_offsets[m + 1] - h_offsets[m];
    if (len < 0 || len > 2147483647LL) return false;
  }
  return h_offsets[n] <= capacity;
}

}  // namespace mp

using namespace mp;

extern "C" size_t mp_rle_workspace_bytes(int n, int h, int w, int rows_per_segment) {
  RlePlan p;
  return rle_plan(n, h, w, rows_per_segment, &p) ? RleWs(nullptr, n, p).total : 0;
}

extern "C" int mp_rle_count(const uint8_t* d_masks, int n, int h, int w, int rows_per_segment, int32_t* d_n_counts, int32_t* d_areas,
                            int32_t* d_boxes, void* d_ws, size_t ws_bytes, mp_stream stream) {
  RlePlan p;
  MP_REQUIRE(rle_plan(n, h, w, rows_per_segment, &p),
             "mp_rle_count: n %d, h %d, w %d, rows_per_segment %d: h, w >= 1, h * w <= 2^31 - 2, n and rows_per_segment >= 0, at most 2^30 jobs", n,
             h, w, rows_per_segment);
  if (n == 0) return MP_OK;
  MP_REQUIRE(d_masks && d_n_counts && d_ws, "mp_rle_count: null pointer");
  const RleWs ws(d_ws, n, p);
  MP_REQUIRE(ws_bytes >= ws.total, "mp_rle_count: workspace of %zu bytes, %zu needed", ws_bytes, ws.total);
  MP_REQUIRE((uintptr_t)d_ws % 16 == 0, "mp_rle_count: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("rle_count", 0.0, (double)n * h * w + 8.0 * (double)p.n_ent, s);
  hipLaunchKernelGGL(rle_walk_kernel<false>, dim3((unsigned)ceil_div(p.n_jobs, kRleWalkBlock)), dim3(kRleWalkBlock), 0, s, d_masks, h, w, p.rows, p.S, p.U,
                     p.n_jobs, ws.ent_count, ws.ent_last, ws.job_stats, (const int32_t*)nullptr, (const int64_t*)nullptr, (int32_t*)nullptr);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rle_scan_kernel, dim3((unsigned)n), dim3(kRleBlock), 0, s, w, p.S, p.U, ws.ent_count, ws.ent_last, ws.job_stats, ws.mask_tot,
                     d_n_counts, d_areas, d_boxes);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" int mp_rle_encode(const uint8_t* d_masks, int n, int h, int w, int rows_per_segment, const int64_t* h_offsets, int32_t* d_counts,
                             long long capacity, void* d_ws, size_t ws_bytes, mp_stream stream) {
  RlePlan p;
  MP_REQUIRE(rle_plan(n, h, w, rows_per_segment, &p),
             "mp_rle_encode: n %d, h %d, w %d, rows_per_segment %d: h, w >= 1, h * w <= 2^31 - 2, n and rows_per_segment >= 0, at most 2^30 jobs", n,
             h, w, rows_per_segment);
  if (n == 0) return MP_OK;
  MP_REQUIRE(d_masks && h_offsets && d_counts && d_ws, "mp_rle_encode: null pointer");
  MP_REQUIRE(capacity >= 0 && rle_offsets_ok(h_offsets, n, capacity),
             "mp_rle_encode: offsets must start at 0, not descend and end within the capacity of %lld counts", capacity);
  const RleWs ws(d_ws, n, p);
  MP_REQUIRE(ws_bytes >= ws.total, "mp_rle_encode: workspace of %zu bytes, %zu needed", ws_bytes, ws.total);
  MP_REQUIRE((uintptr_t)d_ws % 16 == 0, "mp_rle_encode: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("rle_encode", 0.0, (double)n * h * w + 8.0 * (double)p.n_ent + 4.0 * (double)h_offsets[n], s);
  // pageable host memory: the runtime has taken the bytes when the call returns
  MP_CHECK_HIP(hipMemcpyAsync(ws.offsets, h_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(rle_walk_kernel<true>, dim3((unsigned)ceil_div(p.n_jobs, kRleWalkBlock)), dim3(kRleWalkBlock), 0, s, d_masks, h, w, p.rows, p.S, p.U,
                     p.n_jobs, ws.ent_count, ws.ent_last, ws.job_stats, (const int32_t*)ws.mask_tot, (const int64_t*)ws.offsets, d_counts);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}

extern "C" size_t mp_rle_decode_workspace_bytes(int n, int h, int w, long long capacity) {
  RlePlan p;
  return capacity >= 0 && rle_plan(n, h, w, 0, &p) ? RleDecodeWs(nullptr, n, capacity, p).total : 0;
}

extern "C" int mp_rle_decode(const int32_t* d_counts, const int64_t* h_offsets, long long capacity, int n, int h, int w, uint8_t* d_masks,
                             int32_t* d_status, void* d_ws, size_t ws_bytes, mp_stream stream) {
  RlePlan p;
  MP_REQUIRE(rle_plan(n, h, w, 0, &p), "mp_rle_decode: n %d, h %d, w %d: h, w >= 1, h * w <= 2^31 - 2, n >= 0, at most 2^30 jobs", n, h, w);
  if (n == 0) return MP_OK;
  MP_REQUIRE(h_offsets && d_masks && d_status && d_ws, "mp_rle_decode: null pointer");
  MP_REQUIRE(capacity >= 0 && rle_offsets_ok(h_offsets, n, capacity),
             "mp_rle_decode: offsets must start at 0, not descend and end within the %lld counts", capacity);
  MP_REQUIRE(d_counts || h_offsets[n] == 0, "mp_rle_decode: null pointer");
  const RleDecodeWs ws(d_ws, n, capacity, p);
  MP_REQUIRE(ws_bytes >= ws.total, "mp_rle_decode: workspace of %zu bytes, %zu needed", ws_bytes, ws.total);
  MP_REQUIRE((uintptr_t)d_ws % 16 == 0, "mp_rle_decode: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ProfScope prof("rle_decode", 0.0, (double)n * h * w + 8.0 * (double)h_offsets[n], s);
  // pageable host memory: the runtime has taken the bytes when the call returns
  MP_CHECK_HIP(hipMemcpyAsync(ws.offsets, h_offsets, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
  hipLaunchKernelGGL(rle_ends_kernel, dim3((unsigned)n), dim3(kRleBlock), 0, s, d_counts, (const int64_t*)ws.offsets, (long long)h * w, ws.ends,
                     d_status);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rle_seek_kernel, dim3((unsigned)ceil_div(p.n_ent, kRleBlock)), dim3(kRleBlock), 0, s, (const int32_t*)ws.ends,
                     (const int64_t*)ws.offsets, (const int32_t*)d_status, h, w, p.rows, p.S, p.n_ent, ws.ent_run);
  MP_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(rle_fill_kernel, dim3((unsigned)ceil_div(p.n_jobs, kRleWalkBlock)), dim3(kRleWalkBlock), 0, s, (const int32_t*)ws.ends,
                     (const int64_t*)ws.offsets, (const int32_t*)d_status, (const int32_t*)ws.ent_run, h, w, p.rows, p.S, p.U, p.n_jobs, d_masks);
  MP_CHECK_HIP(hipGetLastError());
  return MP_OK;
}
