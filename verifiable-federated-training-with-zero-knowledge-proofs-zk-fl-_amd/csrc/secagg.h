// Host interface of the secure-aggregation mask engine (csrc/secagg.hip), behind zkfl_secagg_mask and
// zkfl_secagg_aggregate.  Replaces the reference's derivePairwiseMask and client-side masking
// (tests/full_system_simulation.mjs:181-196, :558-637; PairwiseMaskDerivation and the signs of
// src/circuits/secure_masked_update.circom:55-146) and gives its server half, aggregateUpdates
// (:1137-1199), the correction for excluded clients that it lacks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "field.h"
#include "prof.h"

namespace zkfl {

struct PosTables;  // merkle.h

// One fused evaluation, all pointers on the host:
//   out[row][k] = sum_{m in base rows of row} base[m][k]
//               + sum_{t in [term_ptr[row], term_ptr[row+1])} s_t * Poseidon(key_t, round, lo_t, hi_t, k)
// with lo_t / hi_t the smaller / larger of term_a[t], term_b[t] as unsigned 64-bit integers and
// s_t = -1 when (term_a[t] < term_b[t]) == negate_if_less, else +1.
struct SecaggJob {
  size_t n_rows = 0;
  uint32_t dim = 0;
  const uint64_t* term_ptr = nullptr;  // [n_rows + 1], term_ptr[0] = 0, T = term_ptr[n_rows] < 2^32
  const uint64_t* term_a = nullptr;    // [T]
  const uint64_t* term_b = nullptr;    // [T]
  bool negate_if_less = false;
  const uint8_t* keys = nullptr;       // [T x 32] std
  const uint8_t* round = nullptr;      // [32] std
  const uint64_t* base_ptr = nullptr;  // [n_rows + 1], or null: row's base is base row `row`
  const uint8_t* base = nullptr;       // [n_base x dim x 32] std
  size_t n_base = 0;
  uint8_t* out = nullptr;              // [n_rows x dim x 32] std
  int64_t* signed_out = nullptr;       // [n_rows x dim] or null: value, or value - r above r / 2
  uint8_t* range_out = nullptr;        // [n_rows x dim] or null: 1 where that does not fit an int64
  uint32_t chunk_terms = 0;            // terms one lane walks; 0 = secagg_default_chunk
};

// The default of chunk_terms: hashes / SECAGG_TARGET_LANES, between 1 and SECAGG_MAX_CHUNK.  A hash
// is ~1.5 ms of one lane's time, so short chunks fill the device and keep the last wave's tail short;
// chunks grow only once there are several lanes of work per lane the device holds, and then bound
// the partials' memory (measured: DESIGN.md §18).
constexpr uint64_t SECAGG_TARGET_LANES = 1u << 19;
constexpr uint32_t SECAGG_MAX_CHUNK = 8;
uint32_t secagg_default_chunk(uint64_t terms, uint32_t dim);

// Arguments are the caller's to validate (csrc/secagg.hip's entry points do).  Synchronises st.
int secagg_run(const PosTables* P, const SecaggJob& J, hipStream_t st, Profiler* prof, std::string& err);


// The same evaluation on device buffers, for a unit that has its operands on the device already
// (csrc/prepare.hip): launches only, no copies and no synchronisation.  raw holds the n_terms keys
// and then the round, standard form; key, lo, hi, neg and part are scratch of n_terms + 1, n_terms,
// n_terms, n_terms and n_chunks x dim elements; the chunk arrays are secagg_chunk_layout's, uploaded.
struct SecaggDev {
  size_t n_rows = 0, n_terms = 0, n_chunks = 0;
  uint32_t dim = 0, chunk_terms = 1;
  bool negate_if_less = false;
  const Fr* raw = nullptr;
  const uint64_t *term_a = nullptr, *term_b = nullptr, *term_ptr = nullptr, *chunk_ptr = nullptr;
  const uint32_t* chunk_row = nullptr;
  const uint64_t* base_ptr = nullptr;  // or null, as SecaggJob's
  const Fr* base = nullptr;
  Fr *key = nullptr, *lo = nullptr, *hi = nullptr;
  uint8_t* neg = nullptr;
  Fr* part = nullptr;
  Fr* out = nullptr;
  int64_t* signed_out = nullptr;
  uint8_t* range_out = nullptr;
};
// a row's terms in chunks of ct: chunk_ptr[row] = its first chunk, chunk_row[c] = the chunk's row
void secagg_chunk_layout(const uint64_t* term_ptr, size_t n, uint32_t ct, std::vector<uint64_t>& chunk_ptr,
                         std::vector<uint32_t>& chunk_row);
int secagg_eval_dev(const PosTables* P, const SecaggDev& S, hipStream_t st, Profiler* prof, std::string& err);

}  // namespace zkfl
