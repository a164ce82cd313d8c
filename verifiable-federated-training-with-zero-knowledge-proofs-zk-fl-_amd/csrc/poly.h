// The polynomial stage of a proof (csrc/poly.hip): a, b, c on the domain from the QAP's CSR rows
// (k_abc_chunks, k_abc_rows), h = a b - c on the coset (k_join; the coset NTT between them is
// ntt.h's), and the proof chain's first kernel (k_proof_start).  Each function below only launches
// its kernel on st; the scheduler (csrc/prove.hip) keeps the sequencing and the error checks.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "field.h"
#include "glv.h"

namespace zkfl {

// terms per lane of k_abc_chunks (the slot's head / tail partials hold one element per chunk)
constexpr uint32_t ABC_L = 16;

// Terms are either packed (col | coefficient-dictionary index << cshift in one u32: circuits
// with few distinct coefficients, e.g. 1,971 among the 7.0 M A/B terms of the training circuit;
// 4 B per term instead of 36 B, the dictionary stays in cache) or wide (cols[] + coefs[]).
struct AbcTerms {
  const uint32_t* cols;  // packed terms, or column indices (wide)
  const Fr* coefs;       // dictionary (packed) or one coefficient per term (wide)
  uint32_t cshift;       // 0: wide
};

// The tails a proof chain empties at its start (k_proof_start): up to 4 G1 and 1 G2, each as
// its bucket array (16-B vectors), nnz counter and liveness flags.
struct ProofStart {
  uint4* buckets[5];
  uint32_t nvec[5];
  uint32_t* nnz[5];
  uint32_t* live[5];
  int n;
  // graph replay: the proof's witness, copied into the slot's stage (w_dst, w_nvec 16-B vectors)
  // from the device address the host left in the pinned buffer (w_src_host); w_dst null: none
  const uint64_t* w_src_host;
  uint4* w_dst;
  uint32_t w_nvec;
  // grouped ABC: the slot's dirty count, plain flag and constraint bits, zeroed for the proof
  // (gr_words of them; gr_state null: none)
  uint32_t* gr_state;
  uint32_t gr_words;
};

// words of the slot's pinned r | s | GLV halves, copied to the device by k_proof_start
constexpr int RS_WORDS = (64 + 4 * (int)sizeof(GlvScalar)) / 4;

// Row r of a segmented sum left by k_abc_chunks (device code; shared by k_abc_rows and the
// constraint check, csrc/r1cs_check.hip): the chunk partials head / tail and the rows written
// whole to abc, stitched over the chunks the row spans.
__device__ __forceinline__ Fr abc_row(const uint32_t* __restrict__ rp, uint32_t r, uint32_t K,
                                      const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                      const Fr* __restrict__ abc) {
  const uint32_t s = rp[r], e = rp[r + 1];
  if (s == e) return fp_zero<FrP>();
  const uint32_t c0 = s / ABC_L, c1 = (e - 1) / ABC_L;
  const bool starts = (s == c0 * ABC_L);
  if (c0 == c1) {
    const uint32_t cend = (c0 + 1) * ABC_L < K ? (c0 + 1) * ABC_L : K;
    if (starts) return head[c0];
    if (e == cend) return tail[c0];
    return abc[r];  // wholly inside the chunk: written by k_abc_chunks
  }
  Fr acc = starts ? head[c0] : tail[c0];
  for (uint32_t c = c0 + 1; c <= c1; c++) acc = fp_add(acc, head[c]);
  return acc;
}

// k_abc_chunks over the K terms (packed when T.cshift != 0), K > 0
void abc_chunks(hipStream_t st, const uint32_t* rp, uint32_t nrows, const AbcTerms& T, const Fr* w, uint32_t K,
                Fr* head, Fr* tail, Fr* abc);
void abc_rows(hipStream_t st, const uint32_t* rp, size_t n, uint32_t K, const Fr* head, const Fr* tail, Fr* abc);

// The grouped ABC (csrc/groups.h): one row per class of equal mapped rows, then the dirty
// constraints again from the original rows.  Both forms are always enqueued and each reads the
// slot's plain flag on the device, so a captured graph serves a proof that follows the partition
// and one that does not.
struct AbcGrouped {
  const uint32_t* crp;    // [classes + 1] the reduced CSR's row pointers
  uint32_t classes;
  AbcTerms terms;         // its Kd terms, in the key's encoding
  uint32_t Kd;
  const uint32_t* cls;    // [2n] class of A row j, then of B row j
  Fr* cls_val;            // [classes] the slot's class values
  const uint32_t* state;  // the slot's dirty count | plain flag | ... (GroupMark::state)
  const uint32_t* dirty;  // the slot's dirty list
  uint32_t cap;           // its capacity
  uint32_t* report;       // host-coherent: the proof's dirty count and plain flag (k_abc_fix leaves them there)
};
// plain flag down: k_abc_chunks over the reduced CSR, a_j = value of class cls[j], b_j = of class
// cls[n + j], c_j = a_j b_j, then a, b, c of every dirty constraint from the original rows (rp, T,
// K); plain flag up: k_abc_chunks and k_abc_rows over the original rows
void abc_grouped(hipStream_t st, const AbcGrouped& G, const uint32_t* rp, size_t n, const AbcTerms& T, const Fr* w,
                 uint32_t K, Fr* head, Fr* tail, Fr* abc);
void join_h(hipStream_t st, const Fr* abc, size_t n, Fr* h);
void proof_start(hipStream_t st, const uint32_t* rs_host, uint32_t* d_rs, Fr* extra, int plain, uint32_t* res3,
                 const ProofStart& ps);
// in place, n elements (zkfl_ntt_coset's conversions around the transform)
void fr_std_to_mont(hipStream_t st, Fr* a, size_t n);
void fr_mont_to_std(hipStream_t st, Fr* a, size_t n);

}  // namespace zkfl
