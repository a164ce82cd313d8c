// Host interface of the round-admission checks (csrc/admit.hip), behind zkfl_round_admit and
// zkfl_debug_admit_static.  Replaces what the reference's Server does before each `groth16 verify`
// (tests/full_system_simulation.mjs: verifyBalanceProof :848-880, verifyTrainingProof :886-990,
// verifySecureAggregationProof :995-1131): signals against claimed fields, the bindings between a
// client's three packages, the clipping bound, and root_G recomputed from the submitted gradient.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "field.h"
#include "prof.h"

namespace zkfl {

struct PosTables;  // merkle.h

constexpr uint32_t ADMIT_B_FIELDS = 1, ADMIT_T_FIELDS = 4, ADMIT_S_FIELDS = 5;  // claimed fields per client
constexpr uint32_t ADMIT_B_NPUB = 5, ADMIT_T_NPUB = 6, ADMIT_S_NPUB0 = 7;       // secagg: 7 + dim + peers

// One round's static checks, all pointers on the host and validated by the caller (the entry points
// of csrc/admit.hip do): the layout of zkfl_admit_round, with the secagg signal count made explicit.
struct AdmitJob {
  size_t n = 0;
  uint32_t dim = 0, flags = 0, s_npub = 0;
  const uint64_t* ids = nullptr;
  const uint8_t *round = nullptr, *tau = nullptr;
  const uint8_t *b_present = nullptr, *t_present = nullptr, *s_present = nullptr;  // never null here
  const uint8_t *b_claimed = nullptr, *t_claimed = nullptr, *s_claimed = nullptr;
  const uint8_t *b_signals = nullptr, *t_signals = nullptr, *s_signals = nullptr;
  const int64_t* gradients = nullptr;
  const uint8_t* masked = nullptr;
  const uint8_t* weights = nullptr;
  const uint64_t *peer_ptr = nullptr, *peer_ids = nullptr;
  uint32_t* codes = nullptr;  // [3 x n] phase-major static codes
};

// Uploads once, runs the chunk pass (dim > 16) and the one-lane-per-client pass, downloads the
// codes.  Synchronises st.
int admit_static_run(const PosTables* P, const AdmitJob& J, hipStream_t st, Profiler* prof, std::string& err);


// the reference's gradient map (:955), standard form: g >= 0 -> g, g < 0 -> r - |g|, with |g| taken
// in unsigned arithmetic (INT64_MIN has no int64 negation)
ZK_DEV Fr fr_from_i64(int64_t g) {
  const uint64_t u = (uint64_t)g;
  const bool neg = g < 0;
  Fr v = fp_zero<FrP>();
  const uint64_t mag = neg ? 0ull - u : u;
  v.v[0] = (uint32_t)mag;
  v.v[1] = (uint32_t)(mag >> 32);
  return neg ? fp_neg(v) : v;  // |g| > 0 here, so r - |g| is in 1..r-1
}

// The device code of the gradient commitment on device buffers, shared with csrc/prepare.hip.
// out[i] = the reference's gradient map of grad[i] (g >= 0 -> g, g < 0 -> r - |g|), standard form.
hipError_t admit_signed_dev(const int64_t* grad, size_t count, Fr* out, hipStream_t st);
// The chunk pass of a vector hash of len in 17..256 values: rows [n_rows x len] standard form ->
// chunk [n_rows x ceil(len / 16)] Montgomery chunk hashes; all full chunks of all rows in one launch,
// the short last chunk in one launch of the width it has.  The top hash is poseidon_rows over chunk.
hipError_t admit_chunks_dev(const PosTables* P, const Fr* rows, size_t n_rows, uint32_t len, Fr* chunk,
                            hipStream_t st);

}  // namespace zkfl
