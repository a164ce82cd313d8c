// Proof assembly (csrc/assemble.hip): pi_a, pi_b and pi_c = C' + H + s pi_a + r B1' from a proof's MSM
// results (k_assemble; k_assemble_t + k_assemble_c for the latency schedule), the part encoding of
// split proofs (k_part_out, k_parts_sum) and the parity hooks' outputs (k_debug_glv_mul,
// k_debug_asm_row / k_debug_asm_quad, k_point_out).  Each function below only launches its kernel on st; the callers keep the
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
// zs: NULL, or one nonzero z (std) per point: the chains start from (x z^2, y z^3, z^2, z^3)
void debug_glv_mul(hipStream_t st, uint32_t n, const uint32_t* pts, const uint32_t* zs, const GlvScalar* ks,
                   uint32_t* out);
// One operation of the assembly's field or point layer on raw 29-bit limbs (k_debug_asm_row /
// k_debug_asm_quad; the operations and layouts: zkfl.h zkfl_debug_asm_ops).  policy 0: RowF<P29>,
// 1: Q29.  in: ASM_DBG_IN words per case (eight operands of nine limbs), out: ASM_DBG_OUT words per case.
enum : int {
  ASM_OP_MUL = 0, ASM_OP_ADD, ASM_OP_DBL, ASM_OP_SUB2, ASM_OP_SUB4, ASM_OP_SUB6, ASM_OP_SUB8,
  ASM_OP_MONT1, ASM_OP_MONT2, ASM_OP_MONT3, ASM_OP_MONT4,
  ASM_OP_BCAST0, ASM_OP_BCAST1, ASM_OP_BCAST2, ASM_OP_BCAST3, ASM_OP_PICK4, ASM_OP_FROM_TO,
  ASM_OP_ONE, ASM_OP_ZERO, ASM_OP_IS_ZERO2, ASM_OP_IS_ZERO4, ASM_OP_CANON,
  ASM_OP_PDBL = 32, ASM_OP_PADD = 33,
};
constexpr int ASM_DBG_IN = 72, ASM_DBG_OUT = 256;
bool debug_asm_op_ok(int policy, int op);
void debug_asm_ops(hipStream_t st, int policy, int op, uint32_t n, const uint32_t* in, uint32_t* out);
// a slot's MSM results -> its part (PART_WORDS words)
void part_out(hipStream_t st, const G1P* res, const G2P* resB2, uint32_t* out);
// block b sums the n_parts parts of proof b into res[5b..5b+3], resB2[b]; *bad set by a point off its curve
void parts_sum(hipStream_t st, uint32_t n, const uint32_t* parts, int n_parts, G1P* res, G2P* resB2, uint32_t* bad);
// n <= 64 MSM results -> std affine bytes
void point_out(hipStream_t st, const G1P* p, int n, uint32_t* out);
void point_out(hipStream_t st, const G2P* p, int n, uint32_t* out);

}  // namespace zkfl
