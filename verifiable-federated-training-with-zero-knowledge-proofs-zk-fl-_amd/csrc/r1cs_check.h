// The witness check (csrc/r1cs_check.hip; `snarkjs wtns check`): a circuit's .r1cs made
// device-resident and the kernels that test <A_j, w> * <B_j, w> == <C_j, w> for every constraint j.
//
// Layout: one CSR term array over 3 m rows -- the A rows, then the B rows, then the C rows -- in the
// QAP rows' term encoding (poly.h AbcTerms; csrc/host_parse.cc r1cs_parse), coefficients held as
// coef * R^2 mod r so the ABC stage's term walk runs on it unchanged.
// Two passes per witness, both on the context's stream:
//   terms    k_abc_chunks over the 3 m rows (poly.h abc_chunks: the prover's own launcher), leaving
//            the chunk partials head / tail and the rows inside one chunk in abc;
//   verdict  one lane per constraint: abc_row stitches rows j, m + j, 2 m + j and compares a * b with
//            c; failures are counted and the lowest index kept (wave ballot, LDS, one atomic pair
//            per workgroup that saw one), then one lane converts a, b, c of that constraint.
// The verdicts of a batch stay on the device until one copy at the end.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "objects.h"

namespace zkfl {

// one witness's verdict as the device leaves it
struct R1csVerdict {
  uint32_t n_failed, first, w0_bad, pad;
  Fr a, b, c;  // std form, of constraint `first`
};

}  // namespace zkfl

struct zkfl_r1cs;

namespace zkfl {

// The terms pass alone, on the context's stream: k_abc_chunks over the object's 3 m rows with the
// vector w (device, std form, n_wires long), leaving head / tail / abc for abc_row.  The witness
// check runs it per witness; the key check (csrc/keycheck.hip) runs it on its random vectors.
// Launches nothing when the system has no terms (every row is then zero).
void r1cs_terms(hipStream_t st, const zkfl_r1cs* r, const Fr* w);

}  // namespace zkfl

struct zkfl_r1cs {
  zkfl_ctx* ctx = nullptr;
  zkfl_r1cs_header hdr = {};
  uint32_t m = 0, K = 0;
  uint32_t* rows = nullptr;  // [3m + 1]
  uint32_t* cols = nullptr;  // [K]
  Fr* coefs = nullptr;       // [K] (wide) or the coefficient dictionary (packed), coef * R^2
  uint32_t cshift = 0;       // packed terms: col | dict index << cshift in cols[]; 0 = wide
  // scratch for one check (a check uses the object alone: one check at a time per object)
  Fr* w = nullptr;     // [n_wires] a .wtns image's values on their way through
  Fr* head = nullptr;  // [ceil(K / ABC_L) + 1]
  Fr* tail = nullptr;
  Fr* abc = nullptr;   // [3m]
  mutable R1csVerdict* verdicts = nullptr;  // [verdict_cap], grown to the largest batch seen
  mutable size_t verdict_cap = 0;
};
