/*
 * zkfl.h — C ABI of the MI355X-native Groth16/BN254 prover (libzkfl.so).
 *
 * Drop-in boundary for the reference's proving path.  The reference never links a prover:
 * it shells out to snarkjs [ext].  Each entry point below replaces one
 * snarkjs operation that a host binding (N-API / ctypes) calls:
 *
 *   zkfl_zkey_load            <- snarkjs reads `<c>_final.zkey` in `groth16 prove`
 *                                (tests/full_system_simulation.mjs:773-776)
 *   zkfl_groth16_prove        <- `npx snarkjs groth16 prove <zkey> <wtns> <proof> <public>`
 *                                (tests/full_system_simulation.mjs:773-776,
 *                                 tests/quick_integration_test.mjs:426-429,
 *                                 tests/test_verified_gradient.mjs:480-483)
 *   zkfl_groth16_prove_batch  <- the sequential per-client loop
 *                                (tests/full_system_simulation.mjs:1298-1343)
 *   zkfl_setup_*              <- the bulk fixed-base work of `snarkjs groth16 setup` +
 *                                `zkey contribute` (tests/full_system_simulation.mjs:713-730)
 *   zkfl_msm_*, zkfl_ntt_*    <- ffjavascript multiExpAffine / fft as used inside
 *                                groth16 prove (exported for parity tests)
 *
 * Conventions (snarkjs/ffjavascript byte conventions):
 *   - Field elements are 32-byte little-endian.  "std" = standard form, "mont" = Montgomery
 *     form (x * 2^256 mod p), as stored in zkey sections 2-9.
 *   - Affine points: G1 = x||y (64 B), G2 = x.c0||x.c1||y.c0||y.c1 (128 B); the point at
 *     infinity is all-zero bytes.
 *   - Proof buffer (256 B): pi_a (G1) || pi_b (G2) || pi_c (G1), affine, std form — exactly
 *     the numbers snarkjs prints in proof.json (pi_a[0..1], pi_b[0..1][0..1], pi_c[0..1]).
 *   - Blinding: rs = 64 bytes (r || s, std form, < r) for deterministic parity mode, or NULL
 *     to draw r, s from the OS CSPRNG (snarkjs draws them with Fr.random()).
 * All functions return 0 on success and a negative ZKFL_E_* code on failure; the message is
 * in zkfl_last_error() (thread-local).  A context is bound to one device and one stream;
 * contexts are independent (multi-GPU = one context per device, one process per GPU).
 */
#ifndef ZKFL_H
#define ZKFL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKFL_OK 0
#define ZKFL_E_ARG -1        /* bad argument / null pointer */
#define ZKFL_E_FORMAT -2     /* malformed zkey / wtns / r1cs bytes */
#define ZKFL_E_PRIME -3      /* file prime is not BN254 r / q */
#define ZKFL_E_MISMATCH -4   /* nWitness != nVars, wrong section sizes */
#define ZKFL_E_DEVICE -5     /* HIP runtime error / no GPU */
#define ZKFL_E_OOM -6        /* device allocation failed */
#define ZKFL_E_CONSTRAINT -7 /* witness does not satisfy the circuit */
#define ZKFL_E_KEY -8        /* proving key is not the circuit's key over the ptau (zkfl_zkey_check) */

typedef struct zkfl_ctx zkfl_ctx;
typedef struct zkfl_key zkfl_key;
typedef struct zkfl_witness zkfl_witness;
typedef struct zkfl_wprog zkfl_wprog;
typedef struct zkfl_vkey zkfl_vkey;

int zkfl_version(void);
/* First 16 hex digits of SHA-256 over the sources this library was built from (the csrc .h, .hip
 * and .cc files sorted by name, then include/zkfl.h; the package Makefile).  bench.py prints it and smoke()
 * checks it against the tree it runs from (zkfl/native.py::source_id). */
const char* zkfl_build_id(void);
const char* zkfl_last_error(void);
int zkfl_device_count(int* count);

int zkfl_ctx_create(int device, zkfl_ctx** out);
int zkfl_ctx_destroy(zkfl_ctx* ctx);
/* Per-kernel timing with HIP events on the stream each kernel runs on (bench.py roofline).
 * enabled: 0 off, 1 on, 2 on + serialized (a proof's G2 and assembly work is put on its main
 * stream, so with one slot every kernel runs alone and its events time it in isolation). */
int zkfl_ctx_set_profiling(zkfl_ctx* ctx, int enabled);
/* name: "msm_accumulate_g1", "msm_accumulate_g2", "ntt", "abc", "prove", "witness" (full-prove
 * slots), "r1cs_terms", "r1cs_verdict" (the witness check's two passes), "verify_wave_g2",
 * "verify_wave_inputs", "verify_wave_pair" (the wave verifier's three kernels; units: proofs),
 * "verify_round_screen", "verify_round_pair", "verify_round_reduce", "verify_round_final" (the
 * combined round check's stages; units: proofs), "verify_round_groups" (the narrow entry's group
 * exponentiations; units: groups),
 * "keycheck_points", "keycheck_rows", "keycheck_msm", "keycheck_pairing" (the key check's stages),
 * "ptaucheck_points", "ptaucheck_scalars", "ptaucheck_msm", "ptaucheck_pairing" (the ptau check's
 * stages, one record per chunk pass; units: points),
 * "secagg_terms", "secagg_fold" (the mask engine's two kernels; units: hashes, output values),
 * "admit_chunks", "admit_clients" (the admission checks' two passes; units: chunk hashes, clients).
 * Synchronises the device.
 * total_ms: summed event time; units: summed algorithmic units (MSM entries, NTT elements...);
 * median_ms (nullable): median single-launch time, robust to a one-off stalled dispatch. */
int zkfl_ctx_profile(zkfl_ctx* ctx, const char* name, double* total_ms, uint64_t* launches, double* units,
                     double* median_ms);
int zkfl_ctx_profile_reset(zkfl_ctx* ctx);
int zkfl_ctx_synchronize(zkfl_ctx* ctx);

/* Parse a snarkjs groth16 .zkey and make it device-resident (bases expanded per window).
 * The caller keeps ownership of buf. */
int zkfl_zkey_load(zkfl_ctx* ctx, const uint8_t* buf, size_t len, zkfl_key** out);
/* The same key by path, in two steps so a host can overlap them with creating its context:
 * zkfl_zkey_file_open maps the file (read-only) and parses it on host threads -- no device work --,
 * zkfl_zkey_load_file makes it device-resident (= zkfl_zkey_load on the file's bytes),
 * zkfl_zkey_file_close unmaps it (any time after the load).  snarkjs reads the key by file name:
 * `snarkjs groth16 prove <zkey> ...` (tests/full_system_simulation.mjs:773-776); node/snarkjs_shim.js
 * maps it while its HIP context comes up.  Errors: ZKFL_E_ARG (open / map failed), as zkfl_zkey_load. */
typedef struct zkfl_zkey_file zkfl_zkey_file;
int zkfl_zkey_file_open(const char* path, zkfl_zkey_file** out);
int zkfl_zkey_load_file(zkfl_ctx* ctx, const zkfl_zkey_file* f, zkfl_key** out);
int zkfl_zkey_file_close(zkfl_zkey_file* f);
int zkfl_key_free(zkfl_key* key);
int zkfl_key_info(const zkfl_key* key, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain_size);
/* How the key holds its A query.  A wire whose A and B1 bases are the same point (the
 * S-box squares of a Poseidon circuit) would be accumulated twice per proof with the same scalar, so
 * a key loads A as the differences D_i = A_i - B1_i wherever that has fewer bases than A itself
 * (compared byte for byte at load; ZKFL_AB_SHARED=0 keeps A) and a proof forms A = B1 + sum w_i D_i.
 * *d_form: 1 in that form; *shared_wires: this shard's wires with one non-zero base in both queries
 * (0 with ZKFL_AB_SHARED=0); *a_bases: the bases of the A slot's MSM, augmentation included.  Any
 * output may be NULL.  Proof bytes are the same in both forms. */
int zkfl_key_ab_shared(const zkfl_key* key, uint32_t* d_form, uint32_t* shared_wires, uint32_t* a_bases);
/* The loader's host-side partition behind it, on caller-supplied records (host only, no device):
 * sec_a / sec_b1 = n x 64 B; counts[4] = D form chosen | shared wires | bases of the A image | bases
 * of the D image (both with shard 0's augmentation slots: 2 and 3); in D form sidx_out (capacity
 * n + 3) and img_out (capacity (n + 3) x 128 B, pairs A_i | B1_i) receive the image, with stand-in
 * augmentation points of bytes 1 | 2, 3 | infinity, infinity | 3 and scalar indices n, n + 1, n + 2. */
int zkfl_debug_ab_partition(const uint8_t* sec_a, const uint8_t* sec_b1, size_t n, uint32_t shard, uint32_t n_shards,
                            uint32_t* counts, uint32_t* sidx_out, uint8_t* img_out);
/* Grouped form of the witness queries.  Wires that carry equal values in every
 * witness of a workload (the twin Poseidon instances of Merkle paths through one tree) need one MSM
 * base per group: for a partition of the wires with rep(i) the first wire of i's group,
 *     sum_i w_i P_i = sum_g w_rep(g) S_g + sum_{i non-rep} (w_i - w_rep(i)) P_i,   S_g = sum_{i in g} P_i,
 * holds for any partition and any witness, and a zero difference costs nothing.  The partition is a
 * speed hint: proof bytes never depend on it.  Whole proofs on an unsharded key run the grouped
 * form once the key holds a partition; the parity hook and split proofs keep the plain form.
 *
 * zkfl_key_set_groups: rep[n_vars] with rep[i] <= i and rep[rep[i]] == rep[i] (else ZKFL_E_ARG, as
 * for n_vars != the key's, a sharded key or a key with a proof in flight); a group is further split
 * so that its first wire has a base in every query in which a member has one.  rep == NULL drops
 * the grouped form.  Builds the group sums and their window copies on the device (one more
 * expanded copy of the A, B1, B2 and C + H queries).
 * zkfl_key_learn_groups: the partition of w's equal values >= 2^128 (host hashing of the
 * downloaded witness), then as the setter.
 * A batch call of at least ZKFL_GROUP_MIN_BATCH proofs (default 8) learns from its first witness
 * when its key is unsharded and holds no partition, and learns again (once per call) when more
 * than half of the non-representative wires missed in the key's last proof and the partition was
 * learned; ZKFL_GROUPS=0 (read when the context is made) turns all of it off.  Each build logs
 * its time to stderr.
 *
 * Grouped ABC: a key that holds a partition also classes its QAP rows (A and B rows together) by
 * their terms mapped through rep -- equal multisets of (rep column, coefficient) evaluate alike when
 * the witness follows -- and keeps one row per class when those hold at most half of the key's
 * terms.  A proof evaluates the class rows, copies the values to the rows and recomputes from the
 * original rows the constraints a missing wire touches (the key's per-wire constraint lists); a
 * wire without a list (more than 256 constraints) that misses, or more than domain / 8 dirty
 * constraints, sends that proof through the plain ABC.  a, b, c are the same for any partition and
 * witness.  ZKFL_GROUP_ROWS=0 (read when the context is made) keeps the plain ABC on grouped keys,
 * and small keys (domain <= 2^ZKFL_SMALL_LOGN) always keep it: their proofs are launch-bound and the
 * grouped form has three more launches.  zkfl_key_group_rows reports it (a struct of its own, so
 * zkfl_groups_info keeps its size). */
typedef struct zkfl_groups_info {
  uint32_t grouped;       /* 1: the key holds a partition */
  uint32_t learned;       /* 1: learned from a witness, 0: set by the caller */
  uint32_t groups;        /* groups of more than one wire */
  uint32_t non_rep;       /* wires that are not their group's first */
  uint32_t bases[4];      /* A, B1, B2, C + H: bases of the plain form (augmentation and H included) */
  uint32_t bases_rep[4];  /* of them, those that carry a scalar when the witness follows the partition */
  uint32_t builds;        /* partitions built on this key so far */
  uint32_t last_miss;     /* non-zero differences in the key's last finished grouped proof */
  double build_ms;        /* the last build: host grouping, group sums, expansion, row classes */
} zkfl_groups_info;
typedef struct zkfl_group_rows_info {
  uint32_t rows_grouped;/* 1: proofs run the grouped ABC (the class rows hold <= half of the terms) */
  uint32_t row_classes;   /* classes of equal mapped rows (the empty class included); 0: not built */
  uint32_t terms;         /* A/B terms of the key (K) */
  uint32_t terms_rep;     /* terms of one row per class (Kd) */
  uint32_t wire_list;     /* entries of the non-representative wires' constraint lists */
  uint32_t wires_over_cap;/* non-representative wires in too many constraints to carry a list */
  uint32_t last_dirty;    /* constraints recomputed in the key's last finished grouped proof */
  uint32_t last_plain;    /* 1: that proof ran the plain ABC (a wire over the cap missed, or the list filled) */
  double rows_build_ms;   /* of build_ms: QAP download, row classes, wire lists, upload */
} zkfl_group_rows_info;
int zkfl_key_set_groups(zkfl_key* key, const uint32_t* rep, size_t n_vars);
int zkfl_key_learn_groups(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w);
int zkfl_key_groups(const zkfl_key* key, zkfl_groups_info* out);
int zkfl_key_group_rows(const zkfl_key* key, zkfl_group_rows_info* out);
/* The host side of it on caller-supplied data (no device): values (n x 32 B, std form) -> rep_out[n]
 * (values NULL: rep_out holds the partition on entry), split by sig (n bytes, nullable), then the
 * grouped form of one query's index map sidx[n_bases] with scalar indices u_base + i:
 * sidx_out[n_bases], start_out[n_bases + 1], members_out[n_bases] (the first start_out[n_bases] used).
 * ZKFL_E_ARG for an invalid partition. */
int zkfl_debug_groups(const uint8_t* values, const uint8_t* sig, size_t n, uint32_t* rep_out, const uint32_t* sidx,
                      size_t n_bases, uint32_t u_base, uint32_t* sidx_out, uint32_t* start_out,
                      uint32_t* members_out);
/* The host side of the grouped ABC on caller-supplied data (no device): rows[2 domain + 1] (A rows
 * then B rows over one term array of K = rows[2 domain] terms), cols[K] (packed: column | coefficient
 * index << cshift; cshift 0: columns, with coefs[K x 8] words), rep[n_vars].  Rows are compared in
 * full after a match of hash_bits (0..64) bits of their hash, so 0 makes every row collide;
 * wire_cap 0 = the library's cap.  Out: cls_out[2 domain], crp_out[2 domain + 1], cterms_out[K],
 * ccoefs_out[K x 8] (cshift 0 only, nullable otherwise), wstart_out[n_vars + 1] (bit 31 of entry i:
 * wire i is over the cap and carries no list), wlist_out[K], info_out[4] = classes | Kd | wire-list
 * entries | 1 when Kd <= K / 2 (the grouped ABC is kept). */
int zkfl_debug_group_rows(const uint32_t* rows, uint32_t domain, const uint32_t* cols, uint32_t cshift,
                          const uint32_t* coefs, const uint32_t* rep, uint32_t n_vars, uint32_t hash_bits,
                          uint32_t wire_cap, uint32_t* cls_out, uint32_t* crp_out, uint32_t* cterms_out,
                          uint32_t* ccoefs_out, uint32_t* wstart_out, uint32_t* wlist_out, uint32_t* info_out);
/* The ABC stage alone on the key's slot 0, as a proof runs it: abc_out = a | b | c on the domain
 * (3 x domain x 32 B, std form) for the resident witness w; grouped != 0 runs the form the key's
 * proofs run (the grouped ABC where the key holds row classes), 0 the plain one.  counts_out[3] =
 * non-zero differences | dirty constraints | plain flag (zeros in the plain form). */
int zkfl_debug_abc(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w, int grouped, uint8_t* abc_out,
                   uint32_t* counts_out);
/* Number of proofs kept in flight by zkfl_groth16_prove_batch (1..32, default 3).  Each slot
 * owns one HIP stream and its own scratch (~0.6 GB for the 2^18 training circuit); proofs in
 * different slots overlap on the GPU.  HIP maps a process's streams onto GPU_MAX_HW_QUEUES
 * hardware queues (HIP default 4, which the GPU boxes export): set it in the environment before
 * the first HIP call to at least the slot count, or the slots serialize.  Measured on MI355X
 * (bench.py's default): 20 slots over 28 queues is the best configuration; 24+
 * slots or 32 queues oversubscribe the hardware queues and lose throughput. */
int zkfl_key_set_slots(zkfl_key* key, int slots);

/* Full prove from a .wtns byte image (host).  pub_out may be NULL; otherwise receives
 * n_public x 32 B std-form public signals (witness[1..n_public]) and *npub their count. */
int zkfl_groth16_prove(zkfl_ctx* ctx, zkfl_key* key, const uint8_t* wtns, size_t wtns_len,
                       const uint8_t* rs, uint8_t proof_out[256], uint8_t* pub_out, size_t* npub);

/* Device-resident witnesses (steady-state proving: input already in HBM). */
int zkfl_witness_upload(zkfl_ctx* ctx, const zkfl_key* key, const uint8_t* wtns, size_t wtns_len,
                        zkfl_witness** out);
int zkfl_witness_free(zkfl_witness* w);
int zkfl_groth16_prove_resident(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w, const uint8_t* rs,
                                uint8_t proof_out[256]);
/* n independent proofs (rs: n x 64 B or NULL); proofs_out: n x 256 B. */
int zkfl_groth16_prove_batch(zkfl_ctx* ctx, zkfl_key* key, size_t n, const zkfl_witness* const* w,
                             const uint8_t* rs, uint8_t* proofs_out);

/* Multi-key batch: proof i uses keys[i] and witness w[i] (uploaded for keys[i]); rs: n x 64 B or
 * NULL; proofs_out: n x 256 B.  Replaces the reference's per-round loop that proves each client's
 * training update and then its secure-aggregation update with two different zkeys
 * (tests/full_system_simulation.mjs:1298-1343: `trainAndGenerateProof` -> groth16 prove of
 * sgd_verified_final.zkey, :773-776; `generateSecureAggregationProof` -> groth16 prove of the
 * secure_masked_update zkey, :1040-1107).  Every key keeps its own proof slots resident; the jobs
 * are issued in order, each on the next slot of its key, so proofs of different circuits
 * overlap on the device. */
int zkfl_groth16_prove_multi(zkfl_ctx* ctx, size_t n, zkfl_key* const* keys, const zkfl_witness* const* w,
                             const uint8_t* rs, uint8_t* proofs_out);

/* One proof split across GPUs (optional row: a proof too large for one device's
 * latency budget).  The reference proves each client on one CPU (`groth16 prove`,
 * tests/full_system_simulation.mjs:773-776); these calls divide that same prove over G processes,
 * one per GPU, with the caller's all-gather in between (zkfl/split.py: torch.distributed; RCCL or gloo):
 *
 *   zkfl_zkey_load_shard   every rank loads the same zkey keeping base i of each query (A, B1, B2,
 *                          C, H) only when i % n_shards == shard, and the alpha/beta/delta
 *                          augmentation bases only on shard 0.  The QAP rows and NTT are whole.
 *   zkfl_groth16_prove_part_batch   per rank, per proof: ABC + coset NTT over the FULL witness
 *                          (h is needed whole; redundant on every rank, ~0.4 ms), then this shard's
 *                          share of the five MSMs.  rs is REQUIRED (n x 64 B, the same r, s on every
 *                          rank: rank 0 draws them and broadcasts).  parts_out: n x 768 B =
 *                          A' (128) | B1' (128) | B2' (256) | C' (128) | H (128), each an XYZZ point
 *                          (x = X/ZZ, y = Y/ZZZ; G1: X|Y|ZZ|ZZZ, G2: the same with c0|c1 per
 *                          coordinate), every coordinate 32 B std-form LE, ZZ = 0 is infinity --
 *                          projective, so a shard pays no inversion; the alpha/beta/delta/r/s terms
 *                          are on shard 0; C' may already include H, then H = infinity.
 *   zkfl_groth16_assemble  after the all_gather: parts = n x n_parts x 768 B (proof-major); the parts
 *                          of each proof are summed and pi_c = C' + H + s pi_a + r B1' is formed on
 *                          the GPU -> n x 256 B proofs, byte-identical to zkfl_groth16_prove_batch
 *                          with the same r, s.  Needs no key.  A coordinate >= q -> ZKFL_E_ARG. */
int zkfl_zkey_load_shard(zkfl_ctx* ctx, const uint8_t* buf, size_t len, uint32_t shard, uint32_t n_shards,
                         zkfl_key** out);
int zkfl_key_shard(const zkfl_key* key, uint32_t* shard, uint32_t* n_shards);
int zkfl_groth16_prove_part_batch(zkfl_ctx* ctx, zkfl_key* key, size_t n, const zkfl_witness* const* w,
                                  const uint8_t* rs, uint8_t* parts_out);
int zkfl_groth16_assemble(zkfl_ctx* ctx, size_t n, size_t n_parts, const uint8_t* parts, const uint8_t* rs,
                          uint8_t* proofs_out);

/* Parity hooks: the deterministic core of one proof.
 * h_out: domain_size x 32 B std (coset evaluations a*b-c, the H-MSM scalars) or NULL;
 * msm_out: A (64) | B1 (64) | B2 (128) | C (64) | H (64) std affine MSM results over the
 * zkey queries *without* the alpha/beta/delta/r/s terms, or NULL. */
int zkfl_debug_prove_parts(zkfl_ctx* ctx, zkfl_key* key, const uint8_t* wtns, size_t wtns_len, uint8_t* h_out,
                           uint8_t* msm_out);

/* GLV split used by the proof assembly (host code, no device): k (32 B std, < r) ->
 * out = k1 || k2, each 20 B: |k_i| (16 B little-endian) then a u32 sign (1 = negative), with
 * k = k1 + k2 * lambda (mod r), |k_i| < 2^128 (csrc/glv.h; tests/test_abi.py checks it). */
int zkfl_debug_glv_split(const uint8_t k[32], uint8_t out[40]);

/* The assembly's scalar multiplication on the device (parity hook): out[i] = k_i * P_i for n pairs,
 * P_i affine std (64 B, (0, 0) = infinity), k_i 32 B std < r, out affine std (infinity = zeros) --
 * the GLV halves of k_i as two row-distributed chains, summed, affine by the divsteps inverse, as
 * k_assemble computes s pi_A + r B1 (no reference counterpart: snarkjs's G1.timesFr inside
 * groth16_prove).  zs: NULL, or one z_i per point (32 B std, 1 <= z_i < q): the chains then start
 * from the XYZZ point (x z^2, y z^3, z^2, z^3), as an MSM result reaches the assembly, instead of
 * (x, y, 1, 1).  The chains test no special case and are only right on points of the prime-order
 * group: a point that is neither (0, 0) nor on y^2 = x^3 + 3 with x, y < q, a z outside [1, q) or a
 * scalar >= r -> ZKFL_E_ARG, the message naming the index. */
int zkfl_debug_g1_glv_mul(zkfl_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* zs, const uint8_t* scalars,
                          uint8_t* out);

/* One operation of the assembly's field or point arithmetic on raw operands (parity hook): the
 * 29-bit engine over Fq (nine 29-bit limbs per value, Montgomery domain 2^261), in the row policy
 * (policy 0: csrc/row29.h RowF<P29>, a value per 16-lane row, what the GLV chains run on) or the quad
 * policy (policy 1: Q29 of csrc/assemble.hip, a value per lane, what sums the parts).  Nothing is
 * normalized or reduced on the way in or out: the caller chooses the lazy limbs and reads the raw
 * result, so the operand bounds of every operation can be tested at their edges.
 * in: n cases x 72 words, eight operands of nine limbs each (u32); out: n cases x 256 words.
 * op (operands a0..a7):
 *    0 mul(a0, a1)   1 add(a0, a1)   2 dbl(a0)   3..6 sub<2 | 4 | 6 | 8>(a0, a1) = a0 + K q - a1
 *    7..10 mont<1..4> (row only): sum_k a_k a_(4+k) 2^-261, a_k replicated, a_(4+k) in row form
 *    11..14 bcast<0..3>   15 pick4(index, a0, a1, a2, a3)   16 to(from(a0)) (row only)
 *    17 one   18 zero   19, 20 is_zero<2 | 4>(a0)   21 canon(a0) (19..21 quad only)
 *    32 quad_dbl(P)   33 quad_add(P, O): P = (a0, a1, a2, a3), O = (a4..a7) as X, Y, ZZ, ZZZ; the row
 *    policy without the special cases (as the chains call them), the quad policy with them.
 * Row policy: a wave takes four field cases, one per row (cases 4g..4g+3 share a wave: bcast<K>
 * returns case 4g+K's operand in each of them, pick4 takes the row as index, op 16 returns row 0's
 * value in all four), out = the row's 16 lanes (lanes 0..8 the limbs as they stand, 9..15); a point
 * operation takes the whole wave, out = [row 0..3][X, Y, ZZ, ZZZ][16 lanes].
 * Quad policy: four lanes per case, each storing its own result: field out = [lane 0..3][9 limbs]
 * (bcast<K>: lane q starts from operand q; pick4 takes the lane as index; is_zero: limb 0 = 0 / 1),
 * point out = [lane 0..3][X, Y, ZZ, ZZZ][9 limbs].  The rest of a case's 256 words is zero.
 * n > 2^14, a null pointer, or an op the policy does not have -> ZKFL_E_ARG. */
int zkfl_debug_asm_ops(zkfl_ctx* ctx, int policy, int op, size_t n, const uint32_t* in, uint32_t* out);

/* The MSM stage of a small key's proof on a caller's sets (parity hook; a test entry: its inputs need
 * not come from a key): n1 (1..4) G1 sets sorted in the same four launches and accumulated in one
 * launch, a G2 set accumulated from set b's sorted pairs with set b's entry count, then the tails --
 * the very function a small key's proofs run (csrc/prove.hip front_msm).  Set i has n[i] bases (mont
 * affine, 64 B, (0, 0) = infinity, as zkfl_msm_g1 takes them) and n_scalars[i] scalars (32 B std, < r).
 * sidx == NULL or sidx[i] == NULL: base j takes scalar j (n_scalars[i] >= n[i]).  Otherwise sidx[i]
 * holds n[i] u32, a key's index map: an entry below extra_start[i] addresses scalars[i], any other
 * entry - extra_start[i] addresses extra[i] (n_extra[i] scalars).  bases_g2: n_b = n[b] G2 bases
 * (mont affine, 128 B), base j riding on set b's base j.  fast: the shorter-chain bucket reduction.
 * joint = 1: the G1 and G2 tails as one batch, as proofs run them; 0: the batched G1 tails, then the
 * G2 tail.  Window width: msm_pick_c of the largest set (ZKFL_MSM_C forces one).  out_g1: n1 x 64 B,
 * out_g2: 128 B, std affine, infinity = zeros.  Sets of more than 2^17 entries, a scalar >= r (the
 * error names its index), an index outside its vector, a null argument or a bad count return
 * ZKFL_E_ARG before any device call. */
int zkfl_debug_msm_front(zkfl_ctx* ctx, uint32_t n1, const size_t* n, const uint8_t* const* bases,
                         const uint8_t* const* scalars, const size_t* n_scalars, const uint32_t* const* sidx,
                         const uint32_t* extra_start, const uint8_t* const* extra, const size_t* n_extra, uint32_t b,
                         const uint8_t* bases_g2, size_t n_b, int fast, int joint, uint8_t* out_g1, uint8_t out_g2[128]);

/* Wave-level kernel timeline (measurement only; libraries built with -DZK_WTRACE=1, otherwise every
 * op returns ZKFL_E_ARG).  op 1: start recording into a fresh device buffer of `cap` records (any
 * earlier one is freed); op 2: wait for the device, stop recording, copy min(count, cap) records of
 * 40 B {u32 kind, u32 HW_ID, u64 start, u64 end (s_memrealtime, 100 MHz), u64 start, u64 end
 * (s_memtime, shader clock cycles)} to out (may be NULL) and the number recorded (possibly > cap) to
 * *count; op 0: free.  tools/wtrace.py reads them. */
int zkfl_debug_wtrace(zkfl_ctx* ctx, int op, uint32_t cap, void* out, uint32_t* count);

/* The proof's coset transform on a caller's batch, under any of its schedules (parity hook):
 * zkfl_ntt_coset on nvec (1..3) vectors of 2^logn (logn 1..27) std-form elements, in place, as one
 * batched call the way the prover makes it.  Vector v starts at element v * vstride (vstride >= 2^logn);
 * data holds ((nvec - 1) * vstride + 2^logn) * 32 bytes, and the elements between the vectors come
 * back unchanged.  col_max: the stages above the 1024-element LDS tile (logn - 10 of them) run as
 * one column pass when there are at most col_max, as radix-2 global passes with unfused LDS
 * passes otherwise; < 0 = the prover's default (10: column passes up to 2^20), 0 = the schedule of
 * the domains above 2^20 at any logn > 10; above 10 is ZKFL_E_ARG.  Every schedule gives the same
 * bytes. */
int zkfl_debug_ntt_coset(zkfl_ctx* ctx, uint8_t* data, uint32_t logn, uint32_t nvec, size_t vstride, int col_max);

/* The polynomial stage's last step on a caller's vectors (parity hook): abc = a | b | c, each 2^logn
 * (logn 1..27) std-form elements on the domain (3 * 2^logn * 32 bytes), to h_out = a b - c on the odd
 * coset, 2^logn std-form elements (2^logn * 32 bytes): the batched transform of the three vectors and
 * the join kernel, the two calls a proof makes, at sizes no proving key has.  col_max: as for
 * zkfl_debug_ntt_coset.  Every schedule gives the same bytes. */
int zkfl_debug_coset_join(zkfl_ctx* ctx, const uint8_t* abc, uint32_t logn, int col_max, uint8_t* h_out);

/* Stand-alone primitives (parity tests).  bases: mont affine; scalars: std, n x 32 B. */
int zkfl_msm_g1(zkfl_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[64]);
int zkfl_msm_g2(zkfl_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[128]);
/* In place: 2^logn std-form evaluations on the domain -> evaluations on the odd coset
 * (snarkjs ifft + batchApplyKey(inc) + fft). */
int zkfl_ntt_coset(zkfl_ctx* ctx, uint8_t* data, uint32_t logn);

/* Witness generation on the GPU (replaces circom's WASM witness calculator:
 * `node <c>_js/generate_witness.cjs <c>.wasm input.json out.wtns`, tests/full_system_simulation.mjs:758-767,
 * and `snarkjs wtns calculate`, tests/test_secureagg.cjs:108-118).  The circuit is a witness
 * program image compiled once per circuit by zkfl/wprog.py (the .wasm's role); inputs are the
 * circuit's input signals in declaration order, flattened, reduced mod r, 32 B std form each
 * (zkfl/wprog.py::input_bytes does the input.json -> bytes step).  An unsatisfied assert returns
 * ZKFL_E_CONSTRAINT (circom: "Assert Failed"); an input >= r returns ZKFL_E_ARG. */
int zkfl_wprog_load(zkfl_ctx* ctx, const uint8_t* prog, size_t len, zkfl_wprog** out);
int zkfl_wprog_free(zkfl_wprog* prog);
int zkfl_wprog_info(const zkfl_wprog* prog, uint32_t* n_wires, uint32_t* n_inputs, uint32_t* n_public);
/* Byte size of one .wtns image for this program (snarkjs wtns v2: 76 + 32 x n_wires). */
size_t zkfl_wtns_size(const zkfl_wprog* prog);
/* circom's input.json (one object of signal name -> number | decimal/0x string | nested arrays;
 * negatives reduced mod r) -> the flattened input vector, using the signal table of a program
 * image.  Host only (no device needed).  inputs_out: room for `cap` values of 32 B; *n_inputs
 * receives the count.  Missing signal / wrong shape / non-integer -> ZKFL_E_ARG. */
int zkfl_wprog_parse_inputs(const uint8_t* prog, size_t len, const char* input_json, uint8_t* inputs_out, size_t cap,
                            size_t* n_inputs);
/* One witness from input.json -> one .wtns image (the generate_witness.cjs call, :758-767). */
int zkfl_witness_compute_json(zkfl_ctx* ctx, const zkfl_wprog* prog, const char* input_json, uint8_t* wtns_out);
/* n witnesses -> n .wtns images at wtns_out + i * zkfl_wtns_size(prog). */
int zkfl_witness_compute(zkfl_ctx* ctx, const zkfl_wprog* prog, size_t n, const uint8_t* inputs, uint8_t* wtns_out);
/* n witnesses computed straight into device-resident witnesses for `key` (no host round trip). */
int zkfl_witness_compute_resident(zkfl_ctx* ctx, const zkfl_wprog* prog, const zkfl_key* key, size_t n,
                                  const uint8_t* inputs, zkfl_witness** out);

/* Full prove, pipelined (snarkjs `groth16.fullProve(input, wasm, zkey)` for a batch; the
 * reference's per-client loop `generate_witness.cjs` + `groth16 prove`,
 * tests/full_system_simulation.mjs:758-776 and :1298-1343).  The witnesses are computed a group
 * of `slots` clients at a time (one batched run of the witness engine on the key's witness
 * stream, straight into HBM), one group ahead of the proof slots that consume them, so witness
 * generation overlaps the MSMs of the previous group; nothing returns to the host but the proofs
 * and the public signals.  inputs: n x n_inputs x 32 B std (zkfl_wprog_parse_inputs per input.json);
 * rs: n x 64 B or NULL (CSPRNG); proofs_out: n x 256 B; pubs_out: n x nPublic x 32 B or NULL.
 * A witness whose asserts fail gives ZKFL_E_CONSTRAINT naming the first such index (its proof
 * bytes are zeroed, the others are valid); an input >= r gives ZKFL_E_ARG before any work. */
int zkfl_groth16_full_prove_batch(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, size_t n,
                                  const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs_out, uint8_t* pubs_out);

/* snarkjs `groth16.fullProve(input, wasm, zkey)` for one input.json text: parsed against the loaded
 * program's signal table, then the full-prove pipeline above with n = 1.  pub_out: nPublic x 32 B
 * or NULL.  Errors as zkfl_wprog_parse_inputs (ZKFL_E_ARG) and zkfl_groth16_full_prove_batch. */
int zkfl_groth16_full_prove_json(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, const char* input_json,
                                 const uint8_t* rs, uint8_t proof_out[256], uint8_t* pub_out);

/* snarkjs `groth16.fullProve` over n input.json texts (the reference runs one fullProve /
 * `generate_witness.cjs` + `groth16 prove` pair per client, tests/full_system_simulation.mjs:758-776):
 * host worker threads parse the texts against the program's signal table ahead of the slot
 * scheduler (at most 64 parsed vectors held), so parsing overlaps the proofs in flight; then the
 * zkfl_groth16_full_prove_batch pipeline.  Errors: a text that does not parse or does not fill
 * the program's inputs gives ZKFL_E_ARG naming its index (proofs of earlier slot groups complete);
 * otherwise as zkfl_groth16_full_prove_batch. */
int zkfl_groth16_full_prove_json_batch(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, size_t n,
                                       const char* const* input_jsons, const uint8_t* rs, uint8_t* proofs_out,
                                       uint8_t* pubs_out);

/* Multi-key full prove: job i = (keys[i], progs[i], inputs[i] = that program's input vector);
 * pubs_out[i] (or pubs_out NULL) receives keys[i]'s nPublic x 32 B.  Same error behaviour as
 * zkfl_groth16_full_prove_batch; the witness index in a ZKFL_E_CONSTRAINT message is the job index. */
int zkfl_groth16_full_prove_multi(zkfl_ctx* ctx, size_t n, zkfl_key* const* keys, const zkfl_wprog* const* progs,
                                  const uint8_t* const* inputs, const uint8_t* rs, uint8_t* proofs_out,
                                  uint8_t* const* pubs_out);

/* Witness check (replaces `snarkjs wtns check <circuit.r1cs> <witness.wtns>`, alias `wchk`): does
 * every constraint <A_j, w> * <B_j, w> == <C_j, w> hold over Fr?  A Groth16 zkey carries no C
 * matrix and the prover forms c as a * b, so zkfl_groth16_prove returns a proof for any witness;
 * this is the call that tells a bad one apart, and names the constraint.  The .r1cs is the file the
 * reference hands to `groth16 setup <c.r1cs> ...` (tests/full_system_simulation.mjs:713-716) and the
 * witness is what its calculator writes (`generate_witness.cjs`, :758-767).
 *
 * zkfl_r1cs_header: the counts of the file's header section; n_terms counts every term of the
 * constraints section.  zkfl_r1cs_report: n_failed = constraints that do not hold, first = the
 * lowest such index, a, b, c = the std-form values of <A, w>, <B, w>, <C, w> at `first` (first, a, b,
 * c are valid when n_failed > 0).  A witness whose wire 0 is not 1 fails as a whole: n_failed = 1,
 * first = 0xFFFFFFFF, a, b, c zero.
 *
 * Parsing validates the whole file (iden3 r1cs v1, BN254 r; ZKFL_E_FORMAT / ZKFL_E_PRIME) and needs
 * no device; loading makes the three matrices device-resident as one CSR term array (A rows, B rows,
 * C rows) with scratch for one check, so one object serves one check at a time.  The check calls
 * take n witnesses -- .wtns images, or the prover's device-resident witnesses, which are never
 * copied to the host -- and return ZKFL_OK when every witness satisfies the system, otherwise
 * ZKFL_E_CONSTRAINT with a message naming the lowest failing witness index and its first
 * constraint; reports (nullable, n entries) is filled in both cases.  A witness of another length
 * than n_wires gives ZKFL_E_MISMATCH, a value >= r ZKFL_E_ARG, both before any check runs. */
typedef struct zkfl_r1cs zkfl_r1cs;
typedef struct {
  uint32_t n_wires, n_pub_out, n_pub_in, n_prv_in, n_constraints;
  uint64_t n_labels, n_terms;
} zkfl_r1cs_header;
typedef struct {
  uint32_t n_failed, first;
  uint8_t a[32], b[32], c[32];
} zkfl_r1cs_report;
int zkfl_r1cs_parse(const uint8_t* buf, size_t len, zkfl_r1cs_header* out);
int zkfl_r1cs_load(zkfl_ctx* ctx, const uint8_t* buf, size_t len, zkfl_r1cs** out);
int zkfl_r1cs_info(const zkfl_r1cs* r1cs, zkfl_r1cs_header* out);
int zkfl_r1cs_free(zkfl_r1cs* r1cs);
int zkfl_r1cs_check(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, size_t n, const uint8_t* const* wtns, const size_t* wtns_len,
                    zkfl_r1cs_report* reports);
int zkfl_r1cs_check_resident(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, size_t n, const zkfl_witness* const* w,
                             zkfl_r1cs_report* reports);

/* Key check: is this .zkey the Groth16 proving key of this .r1cs over this prepared .ptau, for some
 * delta (and gamma)?  The reference proves with whatever `<c>_final.zkey` lies in the circuit
 * directory and skips `groth16 setup` + `zkey contribute` when one is there
 * (tests/full_system_simulation.mjs:713-738), and zkfl_zkey_load validates a key's layout, not its
 * content: a wrong key otherwise shows only as an invalid proof.  No snarkjs command asks this
 * (`zkey verify` asserts a contribution transcript, which this call does not read).
 *
 * With rho (n_wires scalars) and sigma (domainSize scalars) uniform below r, a(rho), b(rho), c(rho) the
 * .r1cs rows evaluated on rho (plus the public rows a[m + s] += rho[s], s <= nPublic) and
 * K(v) = MSM(Lb, a(v)) + MSM(La, b(v)) + MSM(L, c(v)), the checks are, in this order:
 *   HEADER        alpha1, beta1, beta2 are the ptau's; gamma2, delta1, delta2 are proper points;
 *                 e(delta1, G2) == e(G1, delta2)
 *   POINTS        every point of the header and of sections 3, 5, 6, 7, 8, 9 is all-zero (infinity)
 *                 or has coordinates < q and lies on its curve; G2 points lie in the order-r subgroup
 *   COEFFICIENTS  section 4 evaluated on rho equals a(rho), b(rho) row for row (zero elsewhere)
 *   A, B1, B2     MSM(section 5 | 6 | 7, rho) == MSM(L, a(rho)) | MSM(L, b(rho)) | MSM(L2, b(rho))
 *   IC            e(MSM(section 3, rho[0..nPublic]), gamma2) == e(K(rho on the public wires), G2)
 *   C             e(MSM(section 8, rho[nPublic+1..]), delta2) == e(K(rho on the other wires), G2)
 *   H             e(MSM(section 9, sigma), delta2) == e(MSM(H0, sigma), G2)
 * A false accept needs a non-zero linear form to vanish at a uniform point: probability <= 2^-253
 * per check.  A section with a bad point (and IC / C / H under an unusable gamma2 / delta2) takes no
 * part in the later checks, which then read ZKFL_KEYCHECK_NOT_RUN.
 *
 * zkfl_ptau_view: the ptau's Lagrange blocks at the circuit's power (domainSize = 2^power points
 * each, mont affine as the file stores them): L = section 12, L2 = section 13 (G2), La = section
 * 14, Lb = section 15, H0[j] = point 2 j + 1 of section 12's block at power + 1; alpha1 / beta1 /
 * beta2 = alphaTauG1[0], betaTauG1[0], betaG2 (64, 64, 128 B).  *_len are byte lengths.
 *
 * zkfl_zkey_report: status[] per check; point_* = the first section (2 = header, points numbered
 * alpha1, beta1, beta2, gamma2, delta1, delta2) with a bad point, its lowest bad index and how many
 * of its points are bad; coef_* = matrix and row of the lowest differing row and the number of
 * differing rows.
 *
 * rho / sigma NULL: drawn from the OS CSPRNG (as rs == NULL for proofs).  Non-NULL values are for
 * tests and forfeit soundness: a key can be made to pass a vector known in advance.
 * Returns ZKFL_OK when every check holds; ZKFL_E_KEY when one does not (zkfl_last_error names the
 * first in the order above and, for points, section and index; the report is filled);
 * ZKFL_E_MISMATCH when nVars / nPublic / domainSize disagree with the r1cs or the view's power,
 * ZKFL_E_ARG for a short block, a scalar >= r or an r1cs of another context, the parser's codes for
 * a malformed key -- all before any device work. */
#define ZKFL_KEYCHECK_HEADER 0
#define ZKFL_KEYCHECK_POINTS 1
#define ZKFL_KEYCHECK_COEFFICIENTS 2
#define ZKFL_KEYCHECK_A 3
#define ZKFL_KEYCHECK_B1 4
#define ZKFL_KEYCHECK_B2 5
#define ZKFL_KEYCHECK_IC 6
#define ZKFL_KEYCHECK_C 7
#define ZKFL_KEYCHECK_H 8
#define ZKFL_KEYCHECK_N 9
#define ZKFL_KEYCHECK_PASS 0
#define ZKFL_KEYCHECK_FAIL 1
#define ZKFL_KEYCHECK_NOT_RUN 2
typedef struct {
  uint32_t power;
  const uint8_t *L, *L2, *La, *Lb, *H0;
  size_t L_len, L2_len, La_len, Lb_len, H0_len;
  const uint8_t *alpha1, *beta1, *beta2;
} zkfl_ptau_view;
typedef struct {
  uint32_t status[ZKFL_KEYCHECK_N];
  uint32_t point_section, point_index, point_count;
  uint32_t coef_matrix, coef_row, coef_count;
} zkfl_zkey_report;
int zkfl_zkey_check(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, const uint8_t* zkey, size_t zkey_len,
                    const zkfl_ptau_view* ptau, const uint8_t* rho, const uint8_t* sigma, zkfl_zkey_report* report);

/* Ptau check: is this .ptau a well-formed Powers of Tau for SOME tau, alpha and beta, with sections
 * 12-15 the Lagrange form of sections 2-5?  `groth16 setup` and the key check above read sections
 * 12-15 of whatever pot*_final.ptau they are given (tests/full_system_simulation.mjs:677-695), and
 * the key check reads the same blocks on both sides of its equations: a key made from a ptau whose
 * Lagrange blocks are not the Lagrange form of its powers, or whose powers are not the powers of one
 * tau, passes it and is unsound.  This call reads no contribution transcript: it does not establish
 * who knows tau (snarkjs's `powersoftau verify` asserts that, and is not served here).
 *
 * n = 2^power; T, U, A, B = sections 2 (2n-1 points), 3, 4, 5 (n points each), b2 = section 6, points
 * as the file stores them (mont affine, all-zero = infinity).  Randomness: rho (2n-1 scalars, a
 * shorter section uses a prefix), z with z^(2n) != 1, gamma_k for the levels k = 0..power+1.  With
 * S0(X) = sum_{i < len-1} rho_i X[i] and S1(X) = sum_{i < len-1} rho_i X[i+1], in this order:
 *   STRUCTURE   T[0] == G1, U[0] == G2; T[1], A[0], B[0], b2 are not infinity (host)
 *   POINTS      every point of sections 2-6 and 12-15 is all-zero or has coordinates < q and lies on
 *               its curve; G2 points lie in the order-r subgroup
 *   TAU_G1      e(S0(T), U[1]) == e(S1(T), G2)
 *   TAU_G2      e(T[1], S0(U)) == e(G1, S1(U))
 *   ALPHA_G1    e(S0(A), U[1]) == e(S1(A), G2)
 *   BETA_G1     e(S0(B), U[1]) == e(S1(B), G2)
 *   BETA_G2     e(B[0], G2) == e(G1, b2)
 *   L_TAU_G1, L_TAU_G2, L_ALPHA_G1, L_BETA_G1 (section 12 against 2, 13 against 3, 14 against 4, 15
 *               against 5; no pairing):  MSM(Lagrange section, lam) == MSM(power section, s)
 * Position p of a Lagrange section lies in level k = bitlength(p+1) - 1 at index j = p + 1 - 2^k;
 * n_k = 2^k and w_k is the level's domain generator (the one the group iFFT of `prepare phase2`
 * uses).  Levels run to power+1 for section 12, whose top block was made with the absent power
 * T[2n-1] as infinity, and to power for the others.
 *   lam_p = gamma_k w_k^j (z^n_k - 1) / (n_k (z - w_k^j))            = gamma_k L_j^(k) at z
 *   s_0   = sum_k gamma_k / n_k
 *   s_i   = z^-i sum_{k : 2^k > i} gamma_k z^n_k / n_k               (i >= 1)
 * since block k holds (1/n_k) sum_i w_k^(-ij) X[i] and sum_j L_j(z) w_k^(-ij) = z^((n_k - i) mod n_k).
 * A false accept of a chain check needs a non-zero linear form in rho to vanish at a uniform point
 * (<= 2^-253); of a Lagrange check, a non-zero linear form in gamma (<= 2^-253) or a non-zero
 * polynomial of degree < 2n in z (<= 2n / r < 2^-224 at power 28).
 *
 * Every section goes through the device in chunks of at most chunk_points points (0: the default,
 * 2^20), so device memory is bounded by the chunk and the file may be a mapped image of any size.
 * A section with a bad point takes no part in the later checks, which then read
 * ZKFL_PTAUCHECK_NOT_RUN; an unprepared file (no sections 12-15) runs the first seven checks, the
 * Lagrange checks read NOT_RUN, prepared = 0 and the call returns ZKFL_OK when the seven hold.
 *
 * zkfl_ptau_parse validates the layout alone (iden3 binfile "ptau" v1, bn128, power 1..28, every
 * section's byte count, sections 12-15 all present or all absent; ZKFL_E_FORMAT / ZKFL_E_PRIME /
 * ZKFL_E_MISMATCH) and needs no device.
 * rnd: z | gamma[power+2] | rho[2n-1], 32 B std form each, or NULL to draw them from the OS CSPRNG
 * (z redrawn until z^(2n) != 1).  Non-NULL values are for tests and forfeit soundness.  A given
 * scalar >= r or a z on the domain gives ZKFL_E_ARG, a malformed file the parser's codes -- all
 * before any device work.  Returns ZKFL_OK when every check that ran holds, ZKFL_E_KEY when one
 * fails (zkfl_last_error names the first in the order above and, for points, section and index;
 * the report is filled).
 * zkfl_ptau_report: status[] per check (ZKFL_KEYCHECK_PASS / _FAIL / _NOT_RUN's values); point_* =
 * the first section in file order with a bad point, its lowest bad index and how many of its points
 * are bad; chunks = the chunk passes that ran. */
#define ZKFL_PTAUCHECK_STRUCTURE 0
#define ZKFL_PTAUCHECK_POINTS 1
#define ZKFL_PTAUCHECK_TAU_G1 2
#define ZKFL_PTAUCHECK_TAU_G2 3
#define ZKFL_PTAUCHECK_ALPHA_G1 4
#define ZKFL_PTAUCHECK_BETA_G1 5
#define ZKFL_PTAUCHECK_BETA_G2 6
#define ZKFL_PTAUCHECK_L_TAU_G1 7
#define ZKFL_PTAUCHECK_L_TAU_G2 8
#define ZKFL_PTAUCHECK_L_ALPHA_G1 9
#define ZKFL_PTAUCHECK_L_BETA_G1 10
#define ZKFL_PTAUCHECK_N 11
#define ZKFL_PTAUCHECK_PASS 0
#define ZKFL_PTAUCHECK_FAIL 1
#define ZKFL_PTAUCHECK_NOT_RUN 2
typedef struct {
  uint32_t power, ceremony_power, prepared, contributions;
} zkfl_ptau_header;
typedef struct {
  uint32_t status[ZKFL_PTAUCHECK_N];
  uint32_t prepared, power;
  uint32_t point_section, point_index, point_count;
  uint32_t chunks;
} zkfl_ptau_report;
int zkfl_ptau_parse(const uint8_t* buf, size_t len, zkfl_ptau_header* out);
int zkfl_ptau_check(zkfl_ctx* ctx, const uint8_t* ptau, size_t len, const uint8_t* rnd, uint32_t chunk_points,
                    zkfl_ptau_report* report);

/* Verification (replaces `snarkjs groth16 verify <vkey> <public> <proof>`,
 * tests/full_system_simulation.mjs:865-868; snarkjs groth16_verify, restated in
 * oracle/groth16.py::verify).  vk image (see zkfl/groth16.py::vk_bytes for vkey.json -> bytes):
 *   nPublic u32 LE | alpha1 (64) | beta2 (128) | gamma2 (128) | delta2 (128) | IC[nPublic+1] (64 each),
 * standard-form affine LE, G2 as x.c0|x.c1|y.c0|y.c1 (the proof's encoding).  pub: npub x 32 B std.
 * Returns 1 (valid), 0 (invalid: pairing check fails, a public signal >= r, a proof coordinate
 * >= q, a point off its curve, pi_b outside the order-r subgroup) or a negative ZKFL_E_* code
 * (malformed vk, npub != nPublic).  The prepared key is cached in the context. */
int zkfl_groth16_verify(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint8_t* pub, size_t npub,
                        const uint8_t proof[256]);
/* n proofs against one key, one GPU lane each: pubs n x npub x 32 B, proofs n x 256 B,
 * results[i] = 1 / 0.  Returns ZKFL_OK or an error code. */
int zkfl_groth16_verify_batch(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t n, const uint8_t* pubs,
                              size_t npub, const uint8_t* proofs, int32_t* results);
/* Optimal-ate pairing e(P_i, Q_i) for n pairs (g1: n x 64 B, g2: n x 128 B, std affine; all-zero
 * = infinity).  gt_out: n x 384 B, 12 std-form Fq in the ffjavascript Fq12 toObject order
 * (c0.c0.a, c0.c0.b, c0.c1.a, ... c1.c2.b) -- the layout of vkey.json's vk_alphabeta_12. */
int zkfl_pairing(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt_out);
/* Parity hook: the Miller-loop value before the final exponentiation, same layout. */
int zkfl_debug_miller_loop(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out);

/* Resident verification keys and a round's proofs, each against its own key (the reference's
 * server verifies phase by phase with three keys, tests/full_system_simulation.mjs:1298-1343).
 *
 * The load call takes the vk image of zkfl_groth16_verify and keeps the prepared key on the
 * device until it is freed; any number may be resident (the context's one-key cache behind
 * zkfl_groth16_verify and its batch form is separate and untouched).  Errors: ZKFL_E_FORMAT
 * (truncated image, wrong length, a point off its curve / outside its subgroup / at infinity).
 * Keys with at most ZKFL_VERIFY_WAVE_MAX_PUBLIC public signals also get the wave path's
 * per-window tables (64 KB per public signal). */
#define ZKFL_VERIFY_WAVE_MAX_PUBLIC 32
int zkfl_vkey_load(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, zkfl_vkey** out);
int zkfl_vkey_info(const zkfl_vkey* key, uint32_t* n_public);
int zkfl_vkey_free(zkfl_vkey* key);

/* Job i checks proofs + 256 i against vkeys[i] with pubs[i] (npubs[i] x 32 B); results[i] = 1 / 0
 * by the verdict rules of zkfl_groth16_verify_batch.  npubs[i] != the key's nPublic gives
 * ZKFL_E_MISMATCH naming the job before any device work (results untouched); an unknown schedule
 * ZKFL_E_ARG.  The schedules compute the same verdicts:
 *   LANES  one proof per lane: jobs grouped by key, one batch pass per key, verdicts scattered
 *          back to job order (throughput: thousands of proofs);
 *   WAVES  one proof per wavefront (csrc/verify_wave.hip): the latency of one proof or one round;
 *          a job whose key exceeds ZKFL_VERIFY_WAVE_MAX_PUBLIC takes LANES;
 *   AUTO   WAVES up to ZKFL_VERIFY_AUTO_WAVES_MAX jobs, LANES above (the measured crossover,
 *          tools/bench_verify.py --multi). */
#define ZKFL_VERIFY_AUTO 0
#define ZKFL_VERIFY_LANES 1
#define ZKFL_VERIFY_WAVES 2
#define ZKFL_VERIFY_AUTO_WAVES_MAX 4096
int zkfl_groth16_verify_multi(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                              const size_t* npubs, const uint8_t* proofs, int32_t* results, int schedule);
/* The same jobs, verdicts and argument checks as zkfl_groth16_verify_multi (a key above
 * ZKFL_VERIFY_WAVE_MAX_PUBLIC is served like any other), answered for the whole round by one
 * random combination (csrc/verify_round.hip) -- the batched Groth16 verifier:
 *
 *   prod_i e(z_i (-A_i), B_i) * prod_k [ e(Z_k alpha_k, beta_k) e(X_k, gamma_k) e(C_k, delta_k) ] == 1
 *   Z_k = sum z_i mod r,  X_k = sum z_i vk_x_i,  C_k = sum z_i C_i   (sums over key k's jobs)
 *
 * one Miller pair per proof, three per key and one final exponentiation per round, where
 * verify_multi pays three pairs and a final exponentiation per proof.
 *
 * Screening: a job with a public signal >= r, a proof coordinate >= q, pi_a or pi_c off the curve,
 * pi_b off the twist or outside the order-r subgroup gets result 0 and stays out of the
 * combination (the subgroup test is what the bound below rests on).  A pair whose pi_a or pi_b is
 * infinity contributes 1, as in zkfl_groth16_verify_batch.
 * Verdict: when the combination is 1 every combined job gets result 1.  Otherwise the combined jobs
 * are verified one by one as zkfl_groth16_verify_multi does under ZKFL_VERIFY_AUTO and get its
 * verdicts.  If every combined proof is valid the combination is 1; if one is not it is 1 with
 * probability <= 2^-128 over the z_i, so the results equal verify_multi's up to that probability.
 * Cost of a bad proof: a single invalid proof that passes the screening costs the round the
 * combined pass plus the per-proof pass.  zkfl_groth16_verify_round_narrow below narrows the bad
 * jobs down to groups first and re-verifies only those.
 *
 * z NULL: each z_i is drawn uniformly from [0, 2^128) with the OS CSPRNG inside the call (as
 * rs == NULL for proofs).  A caller's z (n x 16 B little endian) is for tests and forfeits
 * soundness: proofs can be made to cancel under values known in advance.
 * report (nullable): filled on ZKFL_OK. */
typedef struct {
  uint32_t keys;     /* distinct keys among the jobs */
  uint32_t screened; /* jobs rejected by the encoding checks (result 0, not combined) */
  uint32_t combined; /* jobs that entered the combination */
  uint32_t passed;   /* 1: the combination equals 1 */
  uint32_t fallback; /* jobs re-verified one by one (0 when passed) */
} zkfl_round_report;
int zkfl_groth16_verify_round(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                              const size_t* npubs, const uint8_t* proofs, const uint8_t* z, int32_t* results,
                              zkfl_round_report* report);
/* Parity hook: the final-exponentiated combination of the jobs that pass the screening, 384 B in
 * zkfl_pairing's layout, and screened_out[i] = 1 for the jobs that do not.  z is required.  chunk:
 * how many proofs one pass holds the lines of pi_b for (0 = the production value, 4096: 80 MB of
 * lines); a small value makes a small round take several passes. */
int zkfl_debug_verify_round(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                            const size_t* npubs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                            uint8_t gt_out[384], int32_t* screened_out);
/* zkfl_groth16_verify_round with a failed round narrowed to its bad groups: the same jobs, z,
 * screening, argument checks and errors, and the same 384 B for the round.  The jobs of a pass (at
 * most 4096), in the order the call sorts them -- by key, stable --, are cut into groups of `group`
 * consecutive jobs; groups never cross a pass border, and the last group of a pass may be short.
 * With the round's z_i every group g has a value of its own,
 *
 *   V_g = FE( prod_{i in g} ML(z_i (-A_i), B_i) * prod_k ML(S_gk, beta_k) ML(X_gk, gamma_k) ML(C_gk, delta_k) )
 *
 * (S, X, C summed over the group's unscreened jobs of key k), the product of its jobs' check values
 * raised to z_i; the round's value is the product of the V_g, formed without exponentiating any of
 * them.  A group holding an invalid job has V_g = 1 with probability <= 2^-128; a group of screened
 * jobs only has V_g = 1.
 * Verdict: when the round's value is 1 every combined job gets result 1 and no group is
 * exponentiated.  Otherwise all V_g are computed in one launch, one wavefront each; the combined
 * jobs of groups with V_g = 1 get result 1, and those of the other groups are verified one by one
 * as zkfl_groth16_verify_multi does under ZKFL_VERIFY_AUTO.  The results equal verify_multi's up
 * to (failing groups) x 2^-128.
 * group: jobs per group, 1 .. the pass size min(n, 4096) (above it: ZKFL_E_ARG).  0 is the
 * production policy: groups of ZKFL_ROUND_GROUP, and a failed round is narrowed only when at least
 * ZKFL_ROUND_NARROW_MIN jobs were combined; below that every combined job is re-verified as by
 * zkfl_groth16_verify_round, and the report shows groups 0 and fallback = combined. */
#define ZKFL_ROUND_GROUP 64
#define ZKFL_ROUND_NARROW_MIN 4096
typedef struct {
  uint32_t keys, screened, combined, passed; /* as zkfl_round_report */
  uint32_t groups;     /* groups formed (0: the call did not narrow, see group == 0) */
  uint32_t bad_groups; /* groups whose value is not 1 (0 when passed) */
  uint32_t fallback;   /* jobs re-verified one by one */
} zkfl_narrow_report;
int zkfl_groth16_verify_round_narrow(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys,
                                     const uint8_t* const* pubs, const size_t* npubs, const uint8_t* proofs,
                                     const uint8_t* z, uint32_t group, int32_t* results, zkfl_narrow_report* report);
/* Parity hook: group_of[i] = job i's group, counted across passes, and every group's V_g, 384 B
 * each in zkfl_pairing's layout (exponentiated whether the round passes or not); *n_groups = how
 * many.  cap: the groups gt_groups has room for; too few gives ZKFL_E_ARG with the count needed in
 * *n_groups, before any device work.  z is required.  chunk as in zkfl_debug_verify_round; group
 * as above, 0 = ZKFL_ROUND_GROUP (at most the pass size). */
int zkfl_debug_verify_round_groups(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                                   const size_t* npubs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                                   uint32_t group, uint32_t* group_of, uint8_t* gt_groups, size_t cap,
                                   uint32_t* n_groups, int32_t* screened_out);
/* Parity hook: zkfl_pairing (final_exp != 0) / zkfl_debug_miller_loop (final_exp == 0) computed by
 * the wave path's tower, Miller loop and final exponentiation; same inputs, layout and errors. */
int zkfl_debug_wave_pairing(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, int final_exp,
                            uint8_t* out);

/* Poseidon hashing and Merkle trees on the GPU: the reference's data/server side
 * (tests/full_system_simulation.mjs:139-238, circomlibjs `poseidon` [ext]), bit-identical to
 * circomlib Poseidon (src/circuits/lib/poseidon.circom:35-96).  Values are 32 B std-form LE, < r
 * (ZKFL_E_ARG otherwise); circomlibjs reduces wider integers mod r, callers do that first.
 *
 * zkfl_poseidon_params (host only, no device): circomlib's constants for width t = 2..17 as the
 * Grain LFSR generates them -- (8 + R_P) * t raw round constants and the 2t Cauchy points x|y of the
 * MDS M[i][j] = 1/(x_i + y_j), std form -- and R_P.  Either output may be NULL. */
int zkfl_poseidon_params(uint32_t t, uint8_t* consts_out, uint8_t* xy_out, uint32_t* rp_out);
/* out[i] = Poseidon(inputs[i*arity .. +arity)), arity 1..16 (circomlibjs poseidon(inputs)). */
int zkfl_poseidon_batch(zkfl_ctx* ctx, uint32_t arity, size_t n, const uint8_t* inputs, uint8_t* out);
/* out[i] = vectorHash(values[i*len .. +len)), len 1..256: Poseidon of <= 16 values, else Poseidon of
 * the 16-value chunk hashes (vectorHash, tests/full_system_simulation.mjs:139-156; VectorHash,
 * src/circuits/training/vector_hash.circom:46-89). */
int zkfl_vector_hash_batch(zkfl_ctx* ctx, uint32_t len, size_t n, const uint8_t* values, uint8_t* out);
/* buildMerkleTree(leafHashes, depth) (tests/full_system_simulation.mjs:198-223): n <= 2^depth leaves
 * padded with Poseidon([0]), depth <= ZKFL_MERKLE_MAX_DEPTH.  tree_out: (2^(depth+1) - 1) x 32 B, the
 * reference's `tree` array flattened -- level 0 (2^depth padded leaves) first, the root last, so
 * getMerkleProof (:225-238) reads tree_out[level_offset(l) + (idx >> l ^ 1)]. */
#define ZKFL_MERKLE_MAX_DEPTH 30
int zkfl_merkle_build(zkfl_ctx* ctx, const uint8_t* leaves, size_t n, uint32_t depth, uint8_t* tree_out);
/* computeDatasetCommitment (tests/full_system_simulation.mjs:309-335) without leaving the device:
 * leaf i = vectorHash(values[i*len .. +len)) (features[i] || label[i]), then buildMerkleTree;
 * root_D = the last 32 B of tree_out. */
int zkfl_dataset_commit(zkfl_ctx* ctx, const uint8_t* values, size_t n, uint32_t len, uint32_t depth,
                        uint8_t* tree_out);

/* Secure aggregation: pairwise masks derived, signed and summed on the GPU (csrc/secagg.hip).
 *
 * The reference's semantics: r_ij[k] = Poseidon(K_ij, round, min(i,j), max(i,j), k) for k < dim
 * (derivePairwiseMask, tests/full_system_simulation.mjs:181-196; PairwiseMaskDerivation,
 * src/circuits/secure_masked_update.circom:55-98), sigma_ij = +1 when i < j, else -1 (:100-146 there;
 * ids compare as unsigned 64-bit integers, the circuit's LessThan(64)), and a client publishes
 * m_i[k] = g_i[k] + sum_p sigma(i, p) r_ip[k] mod r (:558-637 of the harness).  Its server adds the
 * masked updates of the clients whose proofs verified (aggregateUpdates, :1137-1199) and decodes a
 * value above r / 2 as value - r (:1168-1178); the masks cancel only when every client of the group is
 * in that sum.  Values are 32 B std-form LE and < r, as in the Poseidon block above.
 *
 * The mask call: client i has id ids[i], peers peer_ids[t] with keys keys[t] for t in
 * [peer_ptr[i], peer_ptr[i+1]) (CSR, peer_ptr[0] = 0, so one call serves clients of many groups of
 * any sizes) and gradient gradients[i]; masked_out[i] = m_i.  A client without peers gets its gradient.
 *
 * The aggregate call: group g sums the masked updates masked[m], m in
 * [member_ptr[g], member_ptr[g+1]) -- the included clients S_g only -- and takes out what the
 * excluded clients left in them: for every pair t in [pair_ptr[g], pair_ptr[g+1]) of an included
 * client pair_in[t] and an excluded client pair_out[t] with their key pair_keys[t],
 *     sum[k] = sum_{i in S} m_i[k] - sum_t sigma(in_t, out_t) r_t[k] mod r   ( = sum_{i in S} g_i[k] ).
 * Which pairs a group needs, and how their keys come to be revealed, is the caller's protocol
 * (zkfl/secagg.py::close_groups refuses a group whose pairs are not exactly the needed ones).
 * signed_out (nullable): the decode above per coordinate; out_of_range[g] (nullable) = 1 when some
 * coordinate of group g does not fit an int64 -- a mask is still in the sum -- and its signed_out
 * is then all zero.
 *
 * chunk_terms: how many terms (peers / pairs) of a row one GPU lane walks before it writes a
 * partial sum; 0 = the library's choice.  The bytes are the same for every value.
 * Errors, all ZKFL_E_ARG before any device work, the message naming the index: a key, gradient,
 * masked value or round >= r; dim == 0; a *_ptr that does not start at 0 or decreases; a peer equal
 * to its client's id or repeated in one client's list; pair_in == pair_out; 2^32 or more peers or
 * pairs in one call.  n == 0 and n_groups == 0 are valid and do nothing. */
int zkfl_secagg_mask(zkfl_ctx* ctx, size_t n, uint32_t dim, const uint64_t* ids, const uint64_t* peer_ptr,
                     const uint64_t* peer_ids, const uint8_t* keys, const uint8_t round[32], const uint8_t* gradients,
                     uint8_t* masked_out, uint32_t chunk_terms);
int zkfl_secagg_aggregate(zkfl_ctx* ctx, size_t n_groups, uint32_t dim, const uint64_t* member_ptr,
                          const uint8_t* masked, const uint64_t* pair_ptr, const uint64_t* pair_in,
                          const uint64_t* pair_out, const uint8_t* pair_keys, const uint8_t round[32],
                          uint8_t* sum_out, int64_t* signed_out, uint8_t* out_of_range, uint32_t chunk_terms);

/* Admitting a round: the checks the reference's server runs on a client's three packages before
 * each `groth16 verify` (the Server class of tests/full_system_simulation.mjs: verifyBalanceProof
 * :848-880, verifyTrainingProof :886-990, verifySecureAggregationProof :995-1131), the proofs that pass
 * them verified, and one code per client and phase (csrc/admit.hip).  A code is 0 (accepted) or the
 * first failing check in the reference's order, which is the order of the values below.  *_MISSING
 * is for a client whose package of that phase is absent (the reference has no such case: every
 * client sends).  The reference's "no balance proof" test at :1018-1023 cannot fire once the
 * training proof is accepted, so it has no code.  Like the reference, the balance phase does not
 * look at client_id, N_public, c0 or c1, and training signal 0 is not compared with the client id:
 * it is bound through root_G. */
#define ZKFL_ADMIT_OK 0
#define ZKFL_ADMIT_B_MISSING 1         /* no balance package */
#define ZKFL_ADMIT_B_SIG_ROOT_D 2      /* public signal 1 != claimed root_D (:853-858) */
#define ZKFL_ADMIT_B_PROOF 3           /* the proof does not verify (:865-874) */
#define ZKFL_ADMIT_T_MISSING 16        /* no training package */
#define ZKFL_ADMIT_T_NO_BALANCE 17     /* the balance code is not 0 (:895-900) */
#define ZKFL_ADMIT_T_BIND_ROOT_D 18    /* claimed root_D != the balance package's (:902-908) */
#define ZKFL_ADMIT_T_SIG_ROOT_D 19     /* signal 2 != claimed root_D (:920-924) */
#define ZKFL_ADMIT_T_SIG_ROOT_G 20     /* signal 3 != claimed root_G (:926-930) */
#define ZKFL_ADMIT_T_SIG_ROOT_W 21     /* signal 4 != claimed root_W (:932-936) */
#define ZKFL_ADMIT_T_SIG_ROUND 22      /* signal 1 != the package's round (:938-942) */
#define ZKFL_ADMIT_T_ROUND_STALE 23    /* ZKFL_ADMIT_CHECK_ROUND: the package's round != the server's */
#define ZKFL_ADMIT_T_SIG_TAU 24        /* signal 5 != the server's tauSquared (:945-950) */
#define ZKFL_ADMIT_T_ROOT_G_GRADIENT 25 /* gradientCommitment(gradient, id, round) != claimed root_G (:953-965, :139-164) */
#define ZKFL_ADMIT_T_ROOT_W_MODEL 26   /* ZKFL_ADMIT_CHECK_MODEL: claimed root_W != weightCommitment(weights) (:168-170) */
#define ZKFL_ADMIT_T_PROOF 27          /* the proof does not verify (:975-984) */
#define ZKFL_ADMIT_S_MISSING 32        /* no secagg package */
#define ZKFL_ADMIT_S_NO_TRAINING 33    /* the training code is not 0 (:1003-1008) */
#define ZKFL_ADMIT_S_BIND_ROOT_G 34    /* claimed root_G != the training package's (:1010-1014) */
#define ZKFL_ADMIT_S_BIND_ROOT_D 35    /* claimed root_D != the balance package's (:1024-1028) */
#define ZKFL_ADMIT_S_BIND_ROOT_W 36    /* claimed root_W != the training package's (:1032-1036) */
#define ZKFL_ADMIT_S_SIG_CLIENT_ID 37  /* signal 0 != the client's id (:1050-1054) */
#define ZKFL_ADMIT_S_SIG_ROUND 38      /* signal 1 != the package's round (:1057-1061) */
#define ZKFL_ADMIT_S_ROUND_STALE 39    /* ZKFL_ADMIT_CHECK_ROUND: the package's round != the server's */
#define ZKFL_ADMIT_S_SIG_ROOT_D 40     /* signal 2 != claimed root_D (:1065-1069) */
#define ZKFL_ADMIT_S_SIG_ROOT_G 41     /* signal 3 != claimed root_G (:1072-1076) */
#define ZKFL_ADMIT_S_SIG_ROOT_W 42     /* signal 4 != claimed root_W (:1079-1083) */
#define ZKFL_ADMIT_S_SIG_ROOT_K 43     /* signal 5 != claimed root_K (:1086-1090) */
#define ZKFL_ADMIT_S_SIG_TAU 44        /* signal 6 != the server's tauSquared (:1093-1097) */
#define ZKFL_ADMIT_S_SIG_MASKED 45     /* some signal 7 + k != masked_update[k] (:1101-1108) */
#define ZKFL_ADMIT_S_SIG_PEERS 46      /* ZKFL_ADMIT_CHECK_PEERS: signals 7 + dim.. are not the listed peer ids */
#define ZKFL_ADMIT_S_PROOF 47          /* the proof does not verify (:1116-1125) */
/* Flags.  The three checks the reference lacks; with all three clear the verdicts are the
 * reference's exactly.
 *   CHECK_ROUND  a package's round must be the server's (the reference compares a package only with
 *                itself; zkfl's aggregate-round already refuses a disagreeing round);
 *   CHECK_MODEL  the training root_W must be weightCommitment(weights), computed once per call;
 *   CHECK_PEERS  signals 7 + dim.. (peer_ids, public in src/circuits/secure_masked_update.circom:350-360)
 *                must be exactly peer_ids[peer_ptr[i] .. peer_ptr[i+1]), in that order;
 *   COMBINED     the proofs go to zkfl_groth16_verify_round instead of zkfl_groth16_verify_multi. */
#define ZKFL_ADMIT_CHECK_ROUND 1u
#define ZKFL_ADMIT_CHECK_MODEL 2u
#define ZKFL_ADMIT_CHECK_PEERS 4u
#define ZKFL_ADMIT_COMBINED 8u
#define ZKFL_ADMIT_MAX_DIM 256 /* the limit of zkfl_vector_hash_batch */
/* One phase of a round, row i belonging to client i.  The rows of a client whose present byte is 0
 * are ignored (they may hold anything); present NULL: every client sent.
 * claimed: the package's fields, 32 B std-form LE each, `fields` per client:
 *   balance   root_D                                   (1)
 *   training  root_D | root_G | root_W | round         (4)
 *   secagg    root_D | root_G | root_W | root_K | round (5)
 * signals: n x nPublic x 32 B, the proof's public signals (balance 5, training 6, secagg
 * 7 + dim + peers, the peer count of a key being its nPublic - 7 - dim); proofs: n x 256 B. */
typedef struct {
  const uint8_t* present;
  const uint8_t* claimed;
  const uint8_t* signals;
  const uint8_t* proofs;
} zkfl_admit_phase;
typedef struct {
  size_t n;                   /* clients */
  uint32_t dim;               /* 1..ZKFL_ADMIT_MAX_DIM */
  const uint64_t* ids;        /* n client ids */
  const uint8_t* round;       /* 32 B: the server's round */
  const uint8_t* tau_squared; /* 32 B: the server's clipping bound */
  const zkfl_vkey* vkeys[3];  /* balance, training, secagg */
  zkfl_admit_phase balance, training, secagg;
  const int64_t* gradients;     /* n x dim, signed: a negative g stands for r - |g| */
  const uint8_t* masked_update; /* n x dim x 32 B, the secagg package's */
  const uint8_t* weights;       /* dim x 32 B, or NULL without CHECK_MODEL */
  const uint64_t* peer_ptr;     /* n + 1 (CSR, as zkfl_secagg_mask), or NULL without CHECK_PEERS */
  const uint64_t* peer_ids;
} zkfl_admit_round;
/* codes: 3 x n, phase-major (balance, training, secagg).  Everything but the *_PROOF codes and the two
 * *_NO_* rules is decided by one pass on the device (the static codes); the present packages whose
 * static code is 0 are verified in one call; then per client the training code is T_MISSING, else
 * T_NO_BALANCE when the balance code is not 0, else its static code, else the proof's verdict, and
 * secagg likewise over the training code.  A statically rejected proof is not verified, as in the
 * reference; a training proof whose balance proof fails its pairing is verified although the
 * reference would stop before it -- the code is T_NO_BALANCE either way.
 * report (nullable): the round verifier's under COMBINED, else zero but for `combined`, the number
 * of proofs verified.
 * Errors, before any device work, the message naming the index, codes and report untouched:
 * ZKFL_E_ARG for a value >= r in a present row (or in round, tau_squared, weights), dim == 0 or
 * dim > ZKFL_ADMIT_MAX_DIM, a flag whose optional input is NULL, a peer_ptr that does not start at 0
 * or decreases; ZKFL_E_MISMATCH for a key whose nPublic does not fit its phase.  n == 0 is valid. */
int zkfl_round_admit(zkfl_ctx* ctx, const zkfl_admit_round* in, uint32_t flags, uint32_t* codes,
                     zkfl_round_report* report);
/* Parity hook: the static codes alone (3 x n, phase-major; *_PROOF and *_NO_* never appear; a
 * binding check against an absent package is skipped).  vkeys and proofs are not read;
 * secagg_npublic stands for the secagg key's nPublic. */
int zkfl_debug_admit_static(zkfl_ctx* ctx, const zkfl_admit_round* in, uint32_t flags, uint32_t secagg_npublic,
                            uint32_t* codes);

/* Preparing a round: what the reference's clients compute before they prove, for all clients of a
 * round in one call (csrc/prepare.hip) -- the round loop of tests/full_system_simulation.mjs:1278-1343:
 * the dataset tree and its Merkle openings (computeDatasetCommitment :308-335, getMerkleProof :225-238),
 * the fixed-point gradient with its floor division (_computeVerifiedGradient :511-553), gradPos /
 * gradNeg and the clipping test (:411-431), the commitments root_W, root_G, root_K and the masked
 * update (:433-438, :565-609).  The results are the flat input vectors of balance_unified(samples,
 * depth, dim), sgd_verified(batch, dim, depth, precision) and secure_masked_update(dim, peers) in
 * declaration order, 32 B std form -- what zkfl_witness_compute / zkfl_groth16_full_prove_batch take --
 * and the fields a client puts into its packages (zkfl_admit_round reads them back).
 *
 * Semantics, the reference's: leaf i = vectorHash(features[i] || label[i]); the tree is padded with
 * Poseidon([0]); pathIndices[l] = (idx >> l) & 1; summed[j] = sum over the batch rows i of
 * (<f_i, w> - label_i * precision) * f_ij; gradient = floor(summed / (batch * precision)); remainder =
 * summed - gradient * (batch * precision), in [0, batch * precision); root_W = vectorHash(weights);
 * root_G = Poseidon(vectorHash(g), Poseidon(id, round)) over the signed gradient; root_K =
 * Poseidon(master, keys...); masked as zkfl_secagg_mask.  The secagg vector carries the training
 * part's root_D, root_G, root_W and gradient.  Key agreement stays the caller's protocol. */
#define ZKFL_PREPARE_OK 0
#define ZKFL_PREPARE_NORM 1 /* sum g^2 > tau_squared: the reference throws (:428-431); the inputs are still
                               written and the witness engine refuses them */
#define ZKFL_PREPARE_MAX_DIM 255  /* a leaf has dim + 1 <= 256 values */
#define ZKFL_PREPARE_MAX_PEERS 15 /* root_K is one Poseidon of peers + 1 inputs */
typedef struct {
  size_t n;              /* clients */
  const uint64_t* ids;   /* n client ids */
  uint32_t samples;      /* 1..2^depth samples per client */
  uint32_t dim;          /* 1..ZKFL_PREPARE_MAX_DIM */
  uint32_t depth;        /* 1..ZKFL_MERKLE_MAX_DEPTH */
  uint32_t batch;        /* 1..samples */
  uint32_t precision;    /* > 0 */
  uint32_t peers;        /* 0..ZKFL_PREPARE_MAX_PEERS; 0: no secagg part */
  const int64_t* features;  /* n x samples x dim, signed: a negative x stands for r - |x| */
  const uint8_t* labels;    /* n x samples, 0 or 1 */
  const uint32_t* batch_idx; /* n x batch sample indices, or NULL for 0..batch-1 (the reference's choice) */
  const int64_t* weights;   /* dim: the global model, signed */
  const uint8_t* round;     /* 32 B */
  uint64_t tau_squared;     /* < 2^64 - 1: the circuit's LessThan(64) takes tau + 1 */
  const uint64_t* peer_ids; /* n x peers */
  const uint8_t* keys;      /* n x peers x 32 B, aligned with peer_ids */
  const uint8_t* master_keys; /* n x 32 B */
} zkfl_prepare_round;
/* Every pointer nullable: NULL means that part is neither assembled nor copied back. */
typedef struct {
  uint8_t* balance_inputs;  /* n x (5 + samples*dim + samples + 2*samples*depth) x 32 B */
  uint8_t* training_inputs; /* n x (6 + 5*dim + batch*dim + batch + 2*batch*depth) x 32 B */
  uint8_t* secagg_inputs;   /* n x (8 + 2*dim + 2*peers) x 32 B */
  uint8_t* roots;           /* n x 4 x 32 B: root_D, root_G, root_W, root_K (root_K zero when peers == 0) */
  int64_t* gradients;       /* n x dim */
  uint8_t* masked;          /* n x dim x 32 B */
  uint32_t* c1;             /* n: the number of labels that are 1 */
  uint32_t* status;         /* n: ZKFL_PREPARE_* */
} zkfl_prepare_out;
/* The norm is accumulated saturating, so it cannot wrap.  With the overflow bound below in force the
 * device works in plain int64.
 * Errors, all ZKFL_E_ARG before any device work, the message naming the client or index: dim, depth,
 * samples, batch or peers outside the ranges above; a batch_idx >= samples; a label not 0 or 1;
 * precision 0; tau_squared = 2^64 - 1; peers == 0 with secagg_inputs, masked, peer_ids, keys or
 * master_keys non-NULL; a peer equal to its client's id, or repeated in a client's list; a key,
 * master key or round >= r; and, with F = max |feature| and W = max |weight|,
 * batch * F * (dim * F * W + precision) > 2^63 - 1.  n == 0 is valid and does nothing. */
int zkfl_round_prepare(zkfl_ctx* ctx, const zkfl_prepare_round* in, const zkfl_prepare_out* out);

/* Dev-ceremony fixed-base multiplications: out[i] = scalars[i] * generator, mont affine. */
int zkfl_setup_g1_gen_mul(zkfl_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out);
int zkfl_setup_g2_gen_mul(zkfl_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out);

/* Ceremony primitives: the bulk group work of the snarkjs setup commands the reference runs once
 * per circuit (tests/test_secureagg.cjs:25-57: `powersoftau new|contribute|prepare phase2`,
 * `groth16 setup`; tests/full_system_simulation.mjs:713-730: `groth16 setup`, `zkey contribute`).
 * The file handling around them is zkfl/ptau.py.  Points are mont affine
 * (the LEM bytes of ptau / zkey sections; infinity = all zero), scalars std 32 B LE; G2 points are
 * x.c0|x.c1|y.c0|y.c1 (128 B).
 *
 * out[i] = scalars[i] * points[i]: `powersoftau contribute` (tauG1[i] *= tau^i, ...) and
 * `zkey contribute` (delta *= d, C and H *= 1/d). */
int zkfl_setup_g1_scale(zkfl_ctx* ctx, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out);
int zkfl_setup_g2_scale(zkfl_ctx* ctx, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out);
/* out[j] = (1/N) sum_i w^-ij points[i], N = 2^logn (logn <= 28), w = Fr.w[logn] (ffjavascript:
 * nqr = 5): the inverse FFT over the group that `powersoftau prepare phase2` applies to each
 * 2^p prefix of tauG1 / tauG2 / alphaTauG1 / betaTauG1 (ptau sections 12-15), i.e. L_j(tau) G. */
int zkfl_setup_g1_lagrange(zkfl_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out);
int zkfl_setup_g2_lagrange(zkfl_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out);
/* Sparse combinations out[r] = sum_{t in [rowptr[r], rowptr[r+1])} coefs[t] * bases[idx[t]]
 * (rowptr: n_out + 1 entries, rowptr[0] = 0, < 2^32 - 1 terms; idx[t] < n_bases; empty row ->
 * infinity): `groth16 setup`'s A_i, B1_i, B2_i, C_i, IC_i from the Lagrange bases. */
int zkfl_setup_g1_lincomb(zkfl_ctx* ctx, const uint8_t* bases, size_t n_bases, size_t n_out, const uint64_t* rowptr,
                          const uint32_t* idx, const uint8_t* coefs, uint8_t* out);
int zkfl_setup_g2_lincomb(zkfl_ctx* ctx, const uint8_t* bases, size_t n_bases, size_t n_out, const uint64_t* rowptr,
                          const uint32_t* idx, const uint8_t* coefs, uint8_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKFL_H */
