// Host interface of the GPU Groth16 verifier / pairing (csrc/verify.hip), used by the C ABI in
// csrc/zkfl.hip.  Replaces `snarkjs groth16 verify` [ext] (tests/full_system_simulation.mjs:865-868).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "prof.h"

namespace zkfl {

struct VkDev;  // prepared verification key (device tables + lines), opaque

// vk image: nPublic u32 | alpha1 (64) | beta2 (128) | gamma2 (128) | delta2 (128) | IC[(nPub+1) x 64],
// standard-form little-endian affine coordinates (the proof's encoding).  Returns a ZKFL_* code.
int vk_prepare(const uint8_t* vk, size_t len, hipStream_t st, VkDev** out, std::string& err);
void vk_free(VkDev* vk);
bool vk_same(const VkDev* vk, const uint8_t* bytes, size_t len);
uint32_t vk_npub(const VkDev* vk);

// results[i] = 1 valid / 0 invalid for n proofs (256 B each) with npub public signals each (32 B).
int verify_batch(const VkDev* vk, size_t n, const uint8_t* pubs, const uint8_t* proofs, int32_t* results,
                 hipStream_t st, std::string& err);

// e(P_i, Q_i) (final_exp != 0) or the bare Miller loop value, 384 B std-form Fq12 each
// (ffjavascript toObject order).  Points that are off-curve / out of G2 -> ZKFL_E_ARG.
int pairing_batch(size_t n, const uint8_t* g1, const uint8_t* g2, int final_exp, uint8_t* out, hipStream_t st,
                  std::string& err);

// ---- one proof per wavefront (csrc/verify_wave.hip) ----
// The wave path's per-key tables d * 16^w * IC_i (64 KB per public signal, device memory); *out
// stays null when the key has no public signal or more than ZKFL_VERIFY_WAVE_MAX_PUBLIC.
int vk_wave_tables(const VkDev* vk, hipStream_t st, void** out, std::string& err);
void vk_wave_tables_free(void* tab);

struct VerifyJob {
  const VkDev* vk;
  const void* wtab;    // vk_wave_tables of vk
  const uint8_t* pub;  // vk_npub(vk) x 32 B
};
// results[i] = 1 / 0 for proof i (256 B each) against jobs[i]: verify_batch's verdicts.  Every
// job's key must be within the wave path's nPublic cap.  prof (nullable): "verify_wave_*" records.
int verify_wave(size_t n, const VerifyJob* jobs, const uint8_t* proofs, int32_t* results, hipStream_t st,
                Profiler* prof, std::string& err);
// pairing_batch on the wave path's tower, Miller loop and final exponentiation.
int pairing_wave_batch(size_t n, const uint8_t* g1, const uint8_t* g2, int final_exp, uint8_t* out, hipStream_t st,
                       Profiler* prof, std::string& err);

// ---- a round as one random combination (csrc/verify_round.hip) ----
// Screens every job by verify_batch's encoding rules (screened[i] = 1: rejected, not combined) and
// forms prod_i e(z_i (-A_i), B_i) prod_k e(S_k, beta_k) e(X_k, gamma_k) e(C_k, delta_k) over the
// others; one final exponentiation.  z: n x 16 B little endian (never null here).  chunk: proofs
// per pass (0 = 4096; at most ROUND_MAX_CHUNK).  gt_out (nullable): the value, 384 B in
// pairing_batch's layout; *passed = (value == 1); *nkeys = distinct keys.  jobs[i].wtab is not read.
// prof (nullable): "verify_round_*" records.
constexpr size_t ROUND_MAX_CHUNK = 65536;
int verify_round(size_t n, const VerifyJob* jobs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                 uint8_t* gt_out, int32_t* screened, int* passed, uint32_t* nkeys, hipStream_t st, Profiler* prof,
                 std::string& err);
// Jobs per pass: min(n, chunk), chunk 0 = 4096 (4096 x 102 lines x 192 B = 80 MB of lines, as
// verify_batch)
inline size_t round_pass_size(size_t n, size_t chunk) {
  if (chunk == 0) chunk = 4096;
  if (chunk > ROUND_MAX_CHUNK) chunk = ROUND_MAX_CHUNK;
  return n < chunk ? n : chunk;
}
// Groups of `group` consecutive jobs (>= 1) of every pass, the last one of a pass may be short
inline size_t round_group_count(size_t n, size_t chunk, size_t group) {
  const size_t pass = round_pass_size(n, chunk);
  if (pass == 0) return 0;
  return (n / pass) * ((pass + group - 1) / group) + (n % pass + group - 1) / group;
}
// verify_round with one value per group: the passes' jobs in verify_round's order (by key,
// stable) are cut into runs of `group` (1 .. round_pass_size), and every group's Miller value --
// its jobs' pairs and the three pairs of each of its key segments' own sums -- is kept on the
// device.  The round's value is the product of the groups' values: *passed as verify_round's.
// The groups' values are exponentiated in one launch, one wavefront each, when the round fails and
// at least narrow_min jobs passed the screening, or always when gt_groups is not null; *narrowed
// says whether they were.  Then group_one[g] = (group g's value == 1) and gt_groups (nullable)
// holds the values, 384 B each.  group_of[i] (n entries): job i's group, counted across passes.
// prof: verify_round's records and "verify_round_groups".
int verify_round_narrow(size_t n, const VerifyJob* jobs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                        size_t group, size_t narrow_min, uint32_t* group_of, std::vector<uint8_t>* group_one,
                        std::vector<uint8_t>* gt_groups, int32_t* screened, int* passed, int* narrowed,
                        uint32_t* nkeys, hipStream_t st, Profiler* prof, std::string& err);

}  // namespace zkfl
