// Bucket sort of an MSM's signed digits (msm_sort.hip; rocPRIM's onesweep radix sort until round
// 2: DESIGN.md §5).  It knows scalars, base index maps and window widths, not curves: msm.h's
// msm_sort_multi<F> fills the jobs from its MsmBases<F> / MsmScratch<F> and calls msm_sort_launch.
#pragma once
#include "msm_api.h"

namespace zkfl {

constexpr int MSM_SORT_T = 256;                       // threads per block in count / scatter
constexpr int MSM_SORT_HB = 1 << MSM_SORT_HIGH_BITS;  // high bins (every window width)
constexpr int MSM_SORT_MAXBLK = 32768 / MSM_SORT_HB;  // count/scatter blocks (the scan holds cnt in LDS)
constexpr int MSM_SORT_BT = 1024;                     // threads of the scan workgroup
constexpr int MSM_SORT_BINT = MSM_SORT_BIN_THREADS;   // threads per high-bin workgroup
static_assert(MSM_SORT_HB <= MSM_SORT_T, "bucket sort split");
static_assert(MSM_SORT_HB * MSM_SORT_MAXBLK == 32 * MSM_SORT_BT, "scan: 32 counters per thread");
// per-scratch temporary: cnt[HB][MAXBLK], then bin_start[HB + 1]
constexpr size_t MSM_SORT_TMP_WORDS = MSM_SORT_HB * MSM_SORT_MAXBLK + MSM_SORT_HB + 1;

// One sort of a launch (blockIdx.y): its scalars and base map, its blocking (per_blk bases per
// count / scatter block, nblk blocks) and its scratch.  Every sort launch takes a table of up to
// MSM_TAIL_MAX of them, so independent MSMs of a proof sort in the same four launches.
struct MsmSortJob {
  const uint32_t* scalars;
  const uint32_t* extra;
  const uint32_t* sidx;
  uint32_t extra_start;
  uint32_t n, per_blk, nblk;
  uint32_t* cnt;        // [HB][nblk] counts, then exclusive offsets
  uint32_t* bin_start;  // [HB + 1]
  uint32_t* nnz;
  uint16_t* keys_in;
  uint32_t* vals_in;
  uint16_t* keys_out;
  uint32_t* vals_out;
};
struct MsmSortArgs {
  MsmSortJob j[MSM_TAIL_MAX];
};

// The blocking of a sort of m > 0 bases; false when m is beyond the scan's counters.
inline bool msm_sort_blocking(size_t m, uint32_t& per_blk, uint32_t& nblk) {
  const size_t per = (m + MSM_SORT_MAXBLK - 1) / MSM_SORT_MAXBLK;
  const size_t pb = per < MSM_SORT_T ? (size_t)MSM_SORT_T : (per + MSM_SORT_T - 1) / MSM_SORT_T * MSM_SORT_T;
  per_blk = (uint32_t)pb;
  nblk = (uint32_t)((m + pb - 1) / pb);
  return nblk <= (uint32_t)MSM_SORT_MAXBLK;
}

// The four launches (count, scan, scatter, bins) for the first ny jobs of A at window width c, on
// a grid of gx = max nblk count / scatter blocks.  sorted: every job's scratch holds a sort
// already (the sort knock-out build then skips the last two passes).
hipError_t msm_sort_launch(const MsmSortArgs& A, uint32_t gx, int ny, int c, bool sorted, hipStream_t st);

}  // namespace zkfl
