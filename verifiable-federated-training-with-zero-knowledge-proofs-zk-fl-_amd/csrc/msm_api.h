// MSM plan objects and the engine's entry points (see msm.h for the algorithm).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "curve.h"
#include "prof.h"

namespace zkfl {

// Window width c of the signed-digit decomposition.  Scalars are < r < 2^254; with signed digits
// d in [-(2^(c-1) - 1), 2^(c-1)] the top window absorbs the last carry when c W >= 255, so
// W = ceil(255 / c): 19 windows at c = 14, 16 at c = 16, 15 at c = 17.  Every base is expanded into
// its W window copies at key load, so an MSM accumulates one entry per non-zero digit into ONE set
// of 2^(c-1) buckets: a wider window cuts the entries of a full-width scalar and multiplies the
// buckets the (latency-bound) reduction folds.  Bucket keys are |d| - 1 < 2^(c-1),
// a u16 for c <= 17.
// The width is chosen per MSM base set (per proving key: msm_pick_c): MSM_C for large keys, where
// the accumulation dominates, MSM_C_SMALL for keys of at most MSM_SMALL_C_BASES bases, whose
// proofs are chains of latency-bound reduction launches (config 5: 2,335 vs 2,152 proofs/s at 14
// vs 16 bits, the metric key 388 vs 427 -- profiles/r05_ab_window_bits.log).  17 bits (15 windows,
// 2^16 buckets) was measured and rejected in round 5 (config 5 -11%, M within noise:
// profiles/r05_ab_c17_c5_latency.log, r05_ab_c17_large_keys.log) and is no longer accepted.
//
// The engine's tuning table: every numeric choice, with the measurement that set it (MI355X,
// DESIGN.md §5).  An A/B edits a value here and builds the tree (tools/build_ab.sh).
constexpr int MSM_C = 16;                    // window bits of large keys
constexpr int MSM_C_SMALL = 14;              // window bits of small keys
constexpr int MSM_SMALL_C_BASES = 1 << 16;   // a key of at most this many bases is small
// high key bits of the bucket sort (its high bins, every window width): the low c - 1 - HIGH_BITS
// bits are sorted inside one high bin (6 at c = 14, 8 at c = 16)
constexpr int MSM_SORT_HIGH_BITS = 7;
// threads per high-bin workgroup of the bucket sort's bins pass.  A 256-thread variant for small
// MSMs measured neutral on config 5 (1906.7 vs 1894.0 proofs/s, 3 alternations,
// profiles/r04_ab_c5_small_keys.log).
constexpr int MSM_SORT_BIN_THREADS = 1024;
constexpr int MSM_SG = 8;                    // partial sums per lane in each stitching level
// Minimum chunk length (sorted entries per accumulation lane) of small MSMs (<= 2^16 bases), both
// curves.  Small MSMs (config 5's keys) are latency-bound chains, so they take short chunks: a
// shorter serial walk per lane for a few more stitching items (config 5 1970 vs 1893 proofs/s at
// 8 vs 16, same box).
constexpr int MSM_SMALL_L = 8;

// The per-curve choices, by storage field type S (FqOps: G1, Fq2Ops: G2).
//   Compute      the type the point kernels compute in (field29.h), over Affine/XYZZ<S> memory
//   ACC_WAVES    waves per SIMD the register allocator must allow the accumulation kernels
//   STITCH_WAVES / TAIL_WAVES   the same for the stitching levels / the bucket reduction
//   L            minimum chunk length of large MSMs (msm_chunk_len)
//   WSUM_Q       buckets folded serially per lane at level 0 of the bucket reduction: its waves
//                hold their registers for the whole serial fold, but fewer, longer lanes do less
//                scan/tree work per bucket
struct FqOps29;
struct Fq2Pair29;
template <class S>
struct MsmCurve;
// G1 in 29-bit limbs needs ~140 VGPRs in the accumulation: 3 waves/SIMD without spills measured
// 352.8 proofs/s against 342.9 at 4 waves with 17 spilled VGPRs (32-bit limbs, 4 waves: 331.3).
// Its stitching / reduction kernels run at 2-3 waves/SIMD.
template <>
struct MsmCurve<FqOps> {
  using Compute = FqOps29;
  static constexpr int ACC_WAVES = 3, STITCH_WAVES = 2, TAIL_WAVES = 2;
  static constexpr int L = 16, WSUM_Q = 16;
};
// G2 runs on lane pairs: one lane per G2 point needed > 256 registers, so a single wave owned the
// whole SIMD for the kernel's duration (measured 186 -> 208 proofs/s moving G2 to lane pairs).  In
// 29-bit limbs the accumulation takes 168 VGPRs + 14 spilled at 3 waves/SIMD, 180 without spills
// at 2 -- equal throughput (399.5 vs 400.9 proofs/s, profiles/r02_s5_ab_limb29_g2.log); 2 keeps
// scratch out.  The tails take 179-241 VGPRs (2 waves/SIMD), no spills.
template <>
struct MsmCurve<Fq2Ops> {
  using Compute = Fq2Pair29;
  static constexpr int ACC_WAVES = 2, STITCH_WAVES = 2, TAIL_WAVES = 2;
  static constexpr int L = 16, WSUM_Q = 16;
};

__host__ __device__ constexpr int msm_w_of(int c) { return (255 + c - 1) / c; }  // windows: 254-bit scalars + the last carry
__host__ __device__ constexpr int msm_nb_of(int c) { return 1 << (c - 1); }     // buckets (signed digits)
constexpr int MSM_W = msm_w_of(MSM_C);
constexpr int MSM_NB = msm_nb_of(MSM_C);
constexpr int MSM_W_MAX = msm_w_of(MSM_C < MSM_C_SMALL ? MSM_C : MSM_C_SMALL);
static_assert(MSM_C >= 14 && MSM_C <= 16 && MSM_C_SMALL >= 14 && MSM_C_SMALL <= 16,
              "window width: the widths the GPU parity suite runs (>= 64 low counters per high bin of the bucket sort)");
// Knock-out builds for marginal-cost measurements (tools/ko_probe.py; proofs are WRONG, timing
// only): 1 assembly, 2 digit sort, 4 NTT, 8 stitching, 16 bucket reduction, 32 the G2 MSM,
// 64 the G1 accumulation kernel.  0 in every real build; a non-zero value only compiles together
// with ZK_KNOCKOUT_AB_ONLY (tools/build_ab.sh sets both), so a wrong-proof library cannot be built
// by a stray define.
#ifndef ZK_KNOCKOUT
#define ZK_KNOCKOUT 0
#endif
#if ZK_KNOCKOUT != 0 && !defined(ZK_KNOCKOUT_AB_ONLY)
#error "ZK_KNOCKOUT builds compute wrong proofs: timing A/B only (define ZK_KNOCKOUT_AB_ONLY to acknowledge)"
#endif
constexpr int MSM_RB = 64;                 // items per block (one wave) in the weighted bucket reduction
constexpr uint32_t MSM_ITEM_DUMMY = 0x80000000u;  // stitch item flag: padding (its value is infinity)
// Entries per accumulation lane for an MSM with nnz sorted non-zero digits: the minimum L0, or the
// fewest that keep the lanes within `target` = the lanes the device holds at once for the
// accumulation kernel (0: always the minimum), so that one accumulation launch is ONE full round
// of resident lanes.  The kernel argument carries both: bits 0-23 the lanes, bits 24-31 the
// tail's minimum L0 (0: MsmCurve<S>::L) -- msm_target_arg.  A longer chunk leaves fewer chunk
// edges inside a bucket, and every such edge costs one full point addition in the stitching;
// the launch stays one full round of lanes, so the accumulation's own duration does not change.
// The accumulation and the stitching levels derive the same value from nnz on the device.
template <class S>
__host__ __device__ inline uint32_t msm_chunk_len(uint32_t nnz, uint32_t target) {
  const uint32_t L0 = (target >> 24) ? (target >> 24) : (uint32_t)MsmCurve<S>::L;
  target &= 0xFFFFFFu;
  if (target == 0) return L0;
  const uint32_t l = (uint32_t)(((uint64_t)nnz + target - 1) / target);
  return l > L0 ? l : L0;
}
constexpr int MSM_LIVE_LEVELS = 32;  // stitching levels with a liveness flag (level 0 = accumulation)


// Read-only, per proving key: every base expanded into its W window copies.
// Bases are compacted at key load (infinity points dropped); sidx[i] maps compacted base i to
// its scalar: sidx < extra_start -> scalars_main[sidx], else scalars_extra[sidx - extra_start]
// (the proof's 1 / r / s / -rs blinding slots).  sidx == nullptr means identity.
template <class F>
struct MsmBases {
  size_t n = 0;                  // number of (compacted) bases incl. augmentation slots
  int c = MSM_C;                 // window bits (msm_pick_c)
  Affine<F>* bases_w = nullptr;  // [n][W] expanded affine bases (device)
  uint32_t* sidx = nullptr;      // [n] scalar index map (device) or nullptr
  uint32_t extra_start = 0xFFFFFFFFu;
};

// Mutable, per in-flight proof (one stream at a time): digit/sort scratch shared by the MSMs a
// slot runs one after another.
template <class F>
struct MsmScratch {
  size_t cap = 0;                // max number of bases served
  int c = MSM_C;                 // window bits of the base sets served
  uint16_t* keys_in = nullptr;
  uint16_t* keys_out = nullptr;
  uint32_t* vals_in = nullptr;
  uint32_t* vals_out = nullptr;
  void* sort_tmp = nullptr;
  size_t sort_tmp_bytes = 0;
  int ko_sorted = 0;             // sort knock-out builds only: this scratch holds a sort already
};

// Per MSM of a proof: what the accumulation leaves for the tail (stitching + reduction), so the
// tails of several MSMs can run as one batch (one launch per level for all of them).
template <class F>
struct MsmTail {
  size_t max_chunks = 0;        // ceil(cap * W / L)
  int c = MSM_C;                // window bits of the MSMs it serves
  // stitching items (ping-pong): 2 per chunk / per stitching lane, sorted by bucket
  uint32_t* item_key[2] = {nullptr, nullptr};   // bucket | MSM_ITEM_DUMMY
  XYZZ<F>* item_val[2] = {nullptr, nullptr};
  size_t item_cap[2] = {0, 0};
  XYZZ<F>* buckets = nullptr;   // [NB]
  XYZZ<F>* red_a = nullptr;     // weighted-reduction block outputs
  XYZZ<F>* red_s = nullptr;
  uint32_t* nnz = nullptr;      // number of non-zero digits of the last run (device)
  // live[l] != 0: level l (0 = the accumulation) emitted a real open run, so level l + 1 has
  // something to stitch; a level whose predecessor emitted none returns at once (device)
  uint32_t* live = nullptr;
  uint32_t target = 0;          // accumulation lanes resident at once (msm_chunk_len; 0: fixed L)
  uint32_t l0 = 0;              // minimum entries per accumulation lane (msm_tail_l0)
};

// msm_chunk_len's argument: resident lanes (bits 0-23) | minimum chunk length (bits 24-31)
template <class F>
inline uint32_t msm_target_arg(const MsmTail<F>& t) {
  return (t.l0 << 24) | (t.target & 0xFFFFFFu);
}

// Window bits for a base set of n bases; ZKFL_MSM_C=<MSM_C | MSM_C_SMALL> forces one (tests, A/B)
inline int msm_pick_c(size_t n) {
  if (const char* e = getenv("ZKFL_MSM_C")) {
    const int c = atoi(e);
    if (c == MSM_C || c == MSM_C_SMALL) return c;
  }
  return n <= (size_t)MSM_SMALL_C_BASES ? MSM_C_SMALL : MSM_C;
}
// fn(std::integral_constant<int, C>) for the window width c of a base set (MSM_C or MSM_C_SMALL:
// the widths whose kernels are instantiated)
template <class Fn>
hipError_t msm_with_c(int c, Fn&& fn) {
  if (c == MSM_C) return fn(std::integral_constant<int, MSM_C>());
  if constexpr (MSM_C_SMALL != MSM_C)
    if (c == MSM_C_SMALL) return fn(std::integral_constant<int, MSM_C_SMALL>());
  return hipErrorInvalidValue;
}

constexpr int MSM_TAIL_MAX = 4;  // MSM tails per batched launch (the 4 G1 MSMs of a proof)
constexpr int MSM_TAIL_RED = 4 * MSM_RB;  // reduction block outputs per bucket set (<= 2 level-1 blocks of 128 lanes)

// The engine's entry points, templates over the curve (F = FqOps: G1, Fq2Ops: G2).  msm.h defines
// them; msm_g1.hip and msm_g2.hip hold the two instantiations (ZKFL_MSM_API), every other unit
// links against those.
template <class F>
hipError_t msm_bases_alloc(MsmBases<F>& b, size_t n, int c);
template <class F>
hipError_t msm_bases_set(MsmBases<F>& b, const Affine<F>* src, const uint32_t* h_sidx, uint32_t extra_start,
                         hipStream_t st, bool pairs = false);
template <class F>
void msm_bases_free(MsmBases<F>& b);
template <class F>
hipError_t msm_scratch_alloc(MsmScratch<F>& s, size_t cap, int c, hipStream_t st);
template <class F>
void msm_scratch_free(MsmScratch<F>& s);
template <class F>
hipError_t msm_tail_alloc(MsmTail<F>& t, size_t cap, int c);
template <class F>
void msm_tail_free(MsmTail<F>& t);
// digits -> sort -> accumulation into t (the MSM is finished by msm_tails)
template <class F>
hipError_t msm_accumulate(const MsmBases<F>& b, MsmScratch<F>& s, MsmTail<F>& t, const uint32_t* scalars,
                          const uint32_t* extra, hipStream_t st, Profiler* prof, const char* tag);
// empty buckets + zero nnz of n <= MSM_TAIL_MAX tails (before their accumulations)
template <class F>
hipError_t msm_tails_reset(MsmTail<F>* const* t, int n, hipStream_t st);
template <class F>
hipError_t msm_sort(const MsmBases<F>& b, MsmScratch<F>& s, uint32_t* nnz, const uint32_t* sc, const uint32_t* ex,
                    hipStream_t st);
template <class F>
hipError_t msm_accumulate_sorted(const MsmBases<F>& b, const uint16_t* keys, const uint32_t* vals, MsmTail<F>& t,
                                 hipStream_t st, Profiler* prof, const char* tag);
// stitching + bucket reduction of n <= MSM_TAIL_MAX accumulated MSMs -> outs[i] (device)
template <class F>
hipError_t msm_tails(MsmTail<F>* const* t, XYZZ<F>* const* outs, int n, hipStream_t st, bool fast = false);
template <class F>
hipError_t msm_run(const MsmBases<F>& b, MsmScratch<F>& s, MsmTail<F>& t, const uint32_t* scalars,
                   const uint32_t* extra, XYZZ<F>* out, hipStream_t st, Profiler* prof, const char* tag);
// n <= MSM_TAIL_MAX independent MSMs of one window width: their sorts in the same four launches,
// their accumulations in one launch (blockIdx.y = MSM)
template <class F>
hipError_t msm_sort_multi(const MsmBases<F>* const* b, MsmScratch<F>* const* s, uint32_t* const* nnz,
                          const uint32_t* const* sc, const uint32_t* const* ex, int n, hipStream_t st);
template <class F>
hipError_t msm_accumulate_sorted_multi(const MsmBases<F>* const* b, const uint16_t* const* keys,
                                       const uint32_t* const* vals, MsmTail<F>* const* t, int n, hipStream_t st);

// The entry points above for one curve: X = `extern template` here, `template` in the curve's unit.
#define ZKFL_MSM_API(X, F)                                                                                     \
  X hipError_t msm_bases_alloc<F>(MsmBases<F>&, size_t, int);                                                  \
  X hipError_t msm_bases_set<F>(MsmBases<F>&, const Affine<F>*, const uint32_t*, uint32_t, hipStream_t, bool); \
  X void msm_bases_free<F>(MsmBases<F>&);                                                                      \
  X hipError_t msm_scratch_alloc<F>(MsmScratch<F>&, size_t, int, hipStream_t);                                 \
  X void msm_scratch_free<F>(MsmScratch<F>&);                                                                  \
  X hipError_t msm_tail_alloc<F>(MsmTail<F>&, size_t, int);                                                    \
  X void msm_tail_free<F>(MsmTail<F>&);                                                                        \
  X hipError_t msm_accumulate<F>(const MsmBases<F>&, MsmScratch<F>&, MsmTail<F>&, const uint32_t*,             \
                                 const uint32_t*, hipStream_t, Profiler*, const char*);                        \
  X hipError_t msm_tails_reset<F>(MsmTail<F>* const*, int, hipStream_t);                                       \
  X hipError_t msm_sort<F>(const MsmBases<F>&, MsmScratch<F>&, uint32_t*, const uint32_t*, const uint32_t*,    \
                           hipStream_t);                                                                       \
  X hipError_t msm_accumulate_sorted<F>(const MsmBases<F>&, const uint16_t*, const uint32_t*, MsmTail<F>&,     \
                                        hipStream_t, Profiler*, const char*);                                  \
  X hipError_t msm_tails<F>(MsmTail<F>* const*, XYZZ<F>* const*, int, hipStream_t, bool);                      \
  X hipError_t msm_run<F>(const MsmBases<F>&, MsmScratch<F>&, MsmTail<F>&, const uint32_t*, const uint32_t*,   \
                          XYZZ<F>*, hipStream_t, Profiler*, const char*);                                      \
  X hipError_t msm_sort_multi<F>(const MsmBases<F>* const*, MsmScratch<F>* const*, uint32_t* const*,           \
                                 const uint32_t* const*, const uint32_t* const*, int, hipStream_t);            \
  X hipError_t msm_accumulate_sorted_multi<F>(const MsmBases<F>* const*, const uint16_t* const*,               \
                                              const uint32_t* const*, MsmTail<F>* const*, int, hipStream_t);
ZKFL_MSM_API(extern template, FqOps)
ZKFL_MSM_API(extern template, Fq2Ops)

// The G1 tails and the G2 tail of one proof as ONE launch sequence (msm_joint.hip): stitching and
// reduction of both curves side by side, blockIdx.y over all n1 + n2 MSMs
hipError_t msm_tails_joint(MsmTail<FqOps>* const* t1, XYZZ<FqOps>* const* o1, int n1, MsmTail<Fq2Ops>* const* t2,
                           XYZZ<Fq2Ops>* const* o2, int n2, hipStream_t st, bool fast);

}  // namespace zkfl
