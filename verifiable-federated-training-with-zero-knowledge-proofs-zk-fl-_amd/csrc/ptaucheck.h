// The ptau check (csrc/ptaucheck.hip; zkfl_ptau_check): is a .ptau a well-formed Powers of Tau for
// some tau, alpha and beta, with sections 12-15 the Lagrange form of sections 2-5?  `groth16 setup`
// and the key check read sections 12-15 of whatever pot*_final.ptau they are given
// (tests/full_system_simulation.mjs:677-695); include/zkfl.h has the equations and the bound.
//
// Every section goes through the device in chunks of at most chunk_points points (default
// PTAU_CHUNK_DEFAULT), in file order; device memory is sized by the chunk, never by the file.  One
// chunk pass, on the context's stream (profiler names ptaucheck_points / _scalars / _msm; one record
// per pass):
//   points   the chunk's points without its infinities go up once; k_points_check (pointcheck.h)
//            counts the bad ones and keeps the lowest.  A chunk with a bad point ends its section's
//            part in the later checks: its MSMs stop, the remaining chunks are still counted;
//   scalars  a power section (2-5) takes rho shifted by zero and by one place -- S1(X) = sum rho_i
//            X[i+1] is the MSM of the same points under rho[i-1], so the chain needs one overlapping
//            SCALAR across a chunk boundary and no second base set -- and, in a prepared file,
//            k_ptau_s's s_i; a Lagrange section (12-15) takes k_ptau_lam's lam_p.  Both kernels give a
//            lane a run of PTAU_RUN consecutive positions: one power by square-and-multiply, running
//            products after it, and for lam one Fermat inversion per run (batch inversion of the
//            z - w_k^j, which are non-zero because z^(2n) != 1); a run may cross a level boundary.
//            The per-level factors and their suffix sums are power + 2 host values (PtauLevels);
//   msm      one msm_bases_set of the chunk serves its two or three scalar vectors through msm_run
//            (msm_api.h); k_ptau_add adds each partial result into its accumulator.
// Then, once (ptaucheck_pairing): k_ptau_finish compares the four Lagrange pairs (xyzz_same) and
// writes the ten pairing inputs for verify.h pairing_batch; the GT values are compared pairwise.
#pragma once
#include <stdint.h>

namespace zkfl {

constexpr uint32_t PTAU_CHUNK_DEFAULT = 1u << 20;  // points per chunk pass (the ptau check)
constexpr int PTAU_RUN = 8;                        // consecutive positions per lane of the scalar kernels
constexpr int PTAU_MAX_LEVELS = 30;                // levels 0 .. power + 1, power <= 28

}  // namespace zkfl
