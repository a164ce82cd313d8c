// Host interface of the round preparation (csrc/prepare.hip), behind zkfl_round_prepare.  Replaces
// what the reference's clients compute before they prove (tests/full_system_simulation.mjs:
// computeDatasetCommitment :308-335, getMerkleProof :225-238, _computeVerifiedGradient :511-553,
// gradPos / gradNeg and the clipping test :411-431, the commitments and the masked update :433-438,
// :565-609), for every client of a round at once.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "field.h"
#include "prof.h"
#include "zkfl.h"

namespace zkfl {

struct PosTables;  // merkle.h

// the input counts of the three circuits, in declaration order (zkfl/circuits.py)
inline size_t prepare_balance_len(uint32_t samples, uint32_t dim, uint32_t depth) {
  return 5 + (size_t)samples * dim + samples + 2 * (size_t)samples * depth;
}
inline size_t prepare_training_len(uint32_t batch, uint32_t dim, uint32_t depth) {
  return 6 + 5 * (size_t)dim + (size_t)batch * dim + batch + 2 * (size_t)batch * depth;
}
inline size_t prepare_secagg_len(uint32_t dim, uint32_t peers) { return 8 + 2 * (size_t)dim + 2 * (size_t)peers; }

// One round, all pointers on the host and validated by the caller (zkfl_round_prepare does).  One
// upload, the kernels, one copy per requested output, one synchronisation of st.
int prepare_run(const PosTables* P, const zkfl_prepare_round& in, const zkfl_prepare_out& out, hipStream_t st,
                Profiler* prof, std::string& err);

}  // namespace zkfl
