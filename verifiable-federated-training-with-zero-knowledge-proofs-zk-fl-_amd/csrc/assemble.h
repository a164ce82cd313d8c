// Proof assembly (csrc/assemble.hip): pi_a, pi_b and pi_c = C' + H + s pi_a + r B1' from a proof's MSM
// results (k_assemble; k_assemble_t + k_assemble_c for the latency schedule), the part encoding of
// split proofs (k_part_out, k_parts_sum) and the parity hooks' outputs (k_debug_glv_mul,
// k_point_out).  Each function below only launches its kernel on st; the callers keep the
// sequencing and the error checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.h"
#include "glv.h"

namespace zkfl {

// Parts of a split proof (zkfl_groth16_prove_part_batch / zkfl_groth16_assemble): a shard's MSM
// results as XYZZ points, every coordinate in standard form (so the parts cross process boundaries
// in a defined encoding without an inversion per point): A' (32 words) | B1' (32) | B2' (64: each
// coordinate c0, c1) | C' (32) | H (32); ZZ = 0 is infinity.
constexpr int PART_WORDS = 192;  // 768 B

// n proofs, one block each: block b reads res[5b..], resB2[b], ks[4b..] and writes proof[64b..]
void assemble(hipStream_t st, uint32_t n, const G1P* res, const G2P* resB2, const GlvScalar* ks, uint32_t* proof);
// the same assembly in two launches: T = s pi_A + r B1 -> res[4] and pi_a; then pi_c and pi_b
void assemble_t(hipStream_t st, G1P* res, const GlvScalar* ks, uint32_t* proof);
void assemble_c(hipStream_t st, const G1P* res, const G2P* resB2, uint32_t* proof);
// a key in D form: res[0] (A' - B1') += res[1] (B1'), before anything reads res[0]
void fold_a(hipStream_t st, G1P* res);
// out[b] = k_b P_b as the assembly computes s pi_A': pts, out affine std (zeros = infinity), ks 2 per point
void debug_glv_mul(hipStream_t st, uint32_t n, const uint32_t* pts, const GlvScalar* ks, uint32_t* out);
// a slot's MSM results -> its part (PART_WORDS words)
void part_out(hipStream_t st, const G1P* res, const G2P* resB2, uint32_t* out);
// block b sums the n_parts parts of proof b into res[5b..5b+3], resB2[b]; *bad set by a point off its curve
void parts_sum(hipStream_t st, uint32_t n, const uint32_t* parts, int n_parts, G1P* res, G2P* resB2, uint32_t* bad);
// n <= 64 MSM results -> std affine bytes
void point_out(hipStream_t st, const G1P* p, int n, uint32_t* out);
void point_out(hipStream_t st, const G2P* p, int n, uint32_t* out);

}  // namespace zkfl
