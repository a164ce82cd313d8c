// The C ABI's objects (the opaque handles of include/zkfl.h) and what the library's units share
// around them: error reporting, the context's reference count, and what the scheduler
// (csrc/prove.hip) exposes to the key loader (csrc/key_load.hip).  Internal to the library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <string>
#include <vector>

#include "curve.h"
#include "field.h"
#include "msm_api.h"
#include "ntt.h"
#include "prof.h"
#include "wtrace.h"
#include "zkfl.h"

namespace zkfl {
struct VkDev;      // verify.h
struct PosTables;  // merkle.h
struct WProg;      // witness.h

// Set the calling thread's error string (zkfl_last_error; one definition, csrc/zkfl.hip) and
// return the code.
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* where);
}  // namespace zkfl

#define HIP_TRY(x, where)                              \
  do {                                                 \
    hipError_t _e = (x);                               \
    if (_e != hipSuccess) return ::zkfl::hip_fail(_e, where); \
  } while (0)

// The handle types are global names of the C ABI; what they hold lives in namespace zkfl (every
// unit that includes this header is one of the library's own and uses that namespace).
using namespace zkfl;

struct WitPipe;  // csrc/prove.hip

// The proof scheduler's options: read from the environment once, when the
// context is created (zkfl_ctx_create), and fixed for its keys.  The defaults are the measured
// best; each other value picks another schedule for the same proof bytes (csrc/prove.hip plan_proof).
struct SchedOpts {
  bool graph = true;      // ZKFL_GRAPH: graph replay of the one-stream schedules
  bool stagger = true;    // ZKFL_STAGGER: odd slots run ABC + NTT first
  bool lowlat = true;     // ZKFL_LOWLAT: a batch of one takes the latency schedule
  bool fast_wsum = true;  // ZKFL_FAST_WSUM: shorter-chain bucket reduction (latency schedule, small keys)
  int small_logn = 16;    // ZKFL_SMALL_LOGN: a key with a domain <= 2^small_logn is a small key
  bool ab_shared = true;  // ZKFL_AB_SHARED: keys load their A query in D form where that has fewer bases
  bool groups = true;     // ZKFL_GROUPS: the grouped form of the witness queries (csrc/groups.h)
  int group_min_batch = 8;  // ZKFL_GROUP_MIN_BATCH: a batch call of at least this many proofs learns a partition
  bool group_rows = true;   // ZKFL_GROUP_ROWS: a key that holds a partition also classes its QAP rows (grouped ABC)
  int group_rows_cap = 0;   // ZKFL_GROUP_ROWS_CAP: a lower cap on a wire's constraint list (tests); 0: GROUP_ROWS_WIRE_CAP
};

struct zkfl_ctx {
  int device = 0;
  hipStream_t st = nullptr;  // primitives, key loading, verification
  SchedOpts opts;
  Profiler prof;
  zkfl::VkDev* vk = nullptr;       // last prepared verification key (reused while the vk bytes repeat)
  zkfl::PosTables* pos = nullptr;  // Poseidon constants of every width (first hashing call)
  void* asm_buf = nullptr;   // zkfl_groth16_assemble's device buffers (grown on demand, reused)
  size_t asm_cap = 0;
  WtBuf wt;                  // wave-timeline records (ZK_WTRACE builds, zkfl_debug_wtrace)
  // Lifetime: the caller's handle holds one reference and every key and witness program made on
  // the context holds one more, so zkfl_ctx_destroy and the children's frees may come in any
  // order (the N-API finalizers run in an unspecified order); the device state goes with the last.
  std::atomic<int> refs{1};
};

// One in-flight proof: its own stream, scratch and per-proof vectors.
struct ProofSlot {
  hipStream_t st_main = nullptr;
  hipEvent_t ev_done = nullptr;
  MsmScratch<FqOps> g1s;   // digit/sort scratch shared by the four G1 MSMs
#if ZK_KNOCKOUT & 2
  MsmScratch<FqOps> g1s_ko[3];  // sort knock-out (timing only): A, B, C+H keep their first sort
#endif
  MsmTail<FqOps> g1t[4];   // A, B1, C, H: accumulated, finished by one batched tail
  MsmScratch<Fq2Ops> g2s;
  MsmTail<Fq2Ops> g2t;
  Fr* extra = nullptr;  // [4] blinding scalars 1, r, s, -rs (= h + n: the extra slots follow h)
                        // then, on a key that may hold a partition, u[nVars] (k_group_delta)
  Fr* abc = nullptr;  // [3n]
  Fr* abc_head = nullptr;  // [ceil(K / ABC_L)] ABC segmented-sum partials
  Fr* abc_tail = nullptr;
  Fr* h = nullptr;    // [n], then the extra slots
  uint32_t* grp_cnt = nullptr;  // [2] k_group_delta's counters (left zero by every launch)
  // grouped ABC (csrc/groups.h): the proof's dirty-constraint count | plain flag | one bit per
  // constraint (zeroed by k_proof_start), the dirty list (group_rows_dirty_cap entries) and the
  // class values (sized when a proof first needs them: the class count comes with the partition)
  uint32_t* gr_state = nullptr;
  uint32_t* gr_dirty = nullptr;
  uint32_t* gr_missing = nullptr;  // [group_rows_miss_cap] the proof's missing wires (k_group_delta)
  Fr* cls_val = nullptr;
  size_t cls_cap = 0;
  zkfl_key* key = nullptr;      // the slot's key
  bool grouped_run = false;     // its in-flight proof runs the grouped form (its miss count is read back)
  bool rows_run = false;        // ... and the grouped ABC (its dirty count and plain flag are read back)
  G1P* res = nullptr;     // [5]: A', B1', C', H, T
  G2P* resB2 = nullptr;   // [1]
  Fr* d_rs = nullptr;     // r, s (64 B) | GLV halves s1, s2, r1, r2 (4 x 32 B)
  uint32_t* d_parts = nullptr;  // [96]: this rank's part of a split proof (A'|B1'|B2'|C'|H, std affine)
  uint8_t* pinned = nullptr;    // proof (256) | r, s (64) | GLV halves (128) | witness address (8, at
                                // W_PTR_OFF) | the proof's non-zero u, dirty constraints, plain flag (3 x 4, at MISS_OFF) | pad | part (768 at 512)
  // side resources (slot_side_resources): A's and B's own sort scratch, so C + H can sort in g1s
  // while B2 still reads B's pairs -- a small key's slots hold them from the start (run_front),
  // any other slot from its first proof alone (run_lowlat), which also makes that schedule's two
  // side streams and their events (B sorted | B2 final | T = s pi_A + r B1 final)
  hipStream_t st_lat[2] = {nullptr, nullptr};
  hipEvent_t ev_lat[3] = {nullptr, nullptr, nullptr};
  MsmScratch<FqOps> g1s_b;
  MsmScratch<FqOps> g1s_a;
  // graph replay (the context's SchedOpts::graph, ZKFL_GRAPH when it was created; default on): a
  // slot's one-stream schedule captured once, on its second proof
  hipGraph_t graph = nullptr;
  hipGraphExec_t graph_exec = nullptr;
  // the graph's witness: each graph-replayed proof first copies its witness here (nVars x 32 B,
  // a few us of HBM time), so the slot's one graph serves every witness buffer
  Fr* w_stage = nullptr;
  uint32_t direct_proofs = 0;     // proofs this slot ran kernel by kernel (the first one: no capture)
  // B2 shares B1's digit sort, so its tail counts with B1's nnz (g2t.nnz == g1t[1].nnz, owned
  // by g1t[1]): no copy between them
  bool nnz_alias = false;
  bool busy = false;
  int index = 0;                  // position among its key's slots
  size_t job = 0;                 // index of the in-flight proof in its batch
  uint8_t* out_proof = nullptr;   // where its 256 proof bytes go (nullable)
  uint8_t* out_part = nullptr;    // split proofs: where the 768 part bytes go (nullable)
};

// A key's partition of its wires and what was built from it (csrc/groups.hip).
struct KeyGroups {
  bool on = false;        // the grouped base sets below the key's plain ones are built
  bool learned = false;   // from a witness (zkfl_key_learn_groups, a batch call) and not by the caller
  uint32_t groups = 0;    // groups of more than one wire
  uint32_t non_rep = 0;   // wires that are not their group's first
  uint32_t bases[4] = {0, 0, 0, 0};      // A, B1, B2, C + H: bases of the plain form
  uint32_t bases_rep[4] = {0, 0, 0, 0};  // of them, those that carry a scalar when the witness follows
  double build_ms = 0;    // the last build: host grouping, group sums, expansion
  uint32_t builds = 0;
  uint32_t last_miss = 0;     // non-zero u of the last finished grouped proof
  uint32_t* d_rep = nullptr;  // [nVars] (device)
  // grouped ABC (group_rows_build, csrc/groups.h): kept (rows_on) when the classes' rows hold at
  // most half of the K terms; the device copies of GroupRows
  bool rows_on = false;
  uint32_t row_classes = 0;  // D
  uint32_t terms_rep = 0;    // Kd
  uint32_t wire_list = 0;    // entries of the wire lists
  uint32_t over_cap = 0;     // non-representative wires without a list (GROUP_ROWS_WIRE_CAP)
  double rows_ms = 0;        // QAP download, classes, wire lists, upload (part of build_ms)
  uint32_t last_dirty = 0, last_plain = 0;  // of the last finished grouped proof
  uint32_t *d_cls = nullptr, *d_crp = nullptr, *d_cterms = nullptr, *d_wstart = nullptr, *d_wlist = nullptr;
  Fr* d_ccoefs = nullptr;    // wide terms only
};

struct zkfl_key {
  zkfl_ctx* ctx = nullptr;
  uint32_t nVars = 0, nPub = 0, n = 0;
  int logn = 0;
  size_t nC = 0;  // C query length
  size_t K = 0;
  uint32_t* rows = nullptr;  // [2n+1]: A rows then B rows over one term array
  uint32_t* cols = nullptr;  // [K]
  Fr* coefs = nullptr;       // [K] (wide) or the coefficient dictionary (packed)
  uint32_t cshift = 0;       // packed terms: col | dict index << cshift in cols[]; 0 = wide
  MsmBases<FqOps> bA, bB1;
  MsmBases<Fq2Ops> bB2;
  // C and H as ONE MSM: pi_C only needs their sum, so one sort and one tail serve both queries.
  // Bases: C's (scalars: the private wires) then H's (scalars: h, addressed through the extra
  // pointer = the slot's h vector, whose extra slots 1, r, s, -rs follow it).
  MsmBases<FqOps> bCH;
  // The grouped form of the four sets (csrc/groups.h): same base count and order, a
  // representative's slot holds its group's sum, a non-representative's scalar index points at its
  // u behind the blinding scalars.  Whole proofs on an unsharded key run them (ProofPlan::grouped);
  // the parity hook and split proofs keep the plain sets.  q_sidx: the plain index maps (host).
  MsmBases<FqOps> gA, gB1, gCH;
  MsmBases<Fq2Ops> gB2;
  KeyGroups grp;
  std::vector<uint32_t> q_sidx[4];
  // the parity hook's zeros (zkfl_debug_prove_parts, first call, which returns C and H apart): it
  // runs the C + H MSM twice, once with a zero h (C alone) and once with a zero witness (H alone),
  // so the key holds no separate C and H bases (they were ~0.5 GB of expanded bases per key at 2^18)
  Fr* dbg_zero = nullptr;
  // The A query in D form (ab_partition, host_parse.h): bA holds D_i = A_i - B1_i of the wires whose
  // two bases differ (and alpha1 - beta1, delta1 with r, -delta1 with s), so its MSM yields A - B1
  // and every proof adds B1's result to it (fold_a) before anything reads res[0].  The wires that
  // share a base -- the S-box squares, a third of A on the Poseidon-heavy circuits -- are then
  // accumulated once per proof, in B1, instead of twice.
  bool a_diff = false;
  uint32_t ab_shared = 0;  // this shard's wires with the same non-zero base in A and B1
  bool share_b = false;  // B1 and B2 have the same base index map: one digit sort serves both
  // small keys (domain <= 2^SchedOpts::small_logn, config 5's circuits): a proof sorts A, B1 and
  // C + H in the same four launches and accumulates them in one (msm_sort_multi /
  // msm_accumulate_sorted_multi), after ABC / NTT; the slots hold A's and B's sort scratch for it
  // (g1s_a, g1s_b)
  bool front = false;
  int msm_c = MSM_C;     // window bits of every base set of the key (msm_pick_c of its largest)
  NttPlan ntt;
  std::vector<ProofSlot*> slots;
  int max_slots = 3;
  // Split proofs (zkfl_zkey_load_shard): this key holds base i of every query only when
  // i % nshards == shard, and the alpha/beta/delta augmentation bases only on shard 0, so its
  // MSMs are this shard's share of each proof's sums.
  uint32_t shard = 0, nshards = 1;
  WitPipe* wpipe = nullptr;  // batched witnesses of the single-key full-prove entry points
};

struct zkfl_witness {
  const zkfl_key* key = nullptr;
  Fr* d = nullptr;  // nVars std-form elements
  std::vector<uint8_t> pub;  // nPub x 32 B
};

struct zkfl_wprog {
  zkfl_ctx* ctx = nullptr;
  zkfl::WProg* p = nullptr;
};

// A resident verification key (zkfl_vkey_load): the lane path's prepared key plus the wave
// path's per-window IC tables (csrc/verify_wave.hip).
struct zkfl_vkey {
  zkfl_ctx* ctx = nullptr;
  zkfl::VkDev* vk = nullptr;
  void* wtab = nullptr;   // vk_wave_tables (null without public signals or above the cap)
  bool wave_ok = false;   // nPublic <= ZKFL_VERIFY_WAVE_MAX_PUBLIC
};

namespace zkfl {
void ctx_retain(zkfl_ctx* ctx);
void ctx_release(zkfl_ctx* ctx);  // drops one reference; the last one tears the context down
// csrc/zkfl.hip: the context's Poseidon tables (ctx->pos), built by the first hashing call
int pos_ready(zkfl_ctx* ctx);
// csrc/prove.hip: the key's idx-th slot (idx % max_slots), made on first use; all of its slots and
// its witness pipe released (key_release, csrc/key_load.hip)
int get_slot(zkfl_key* k, size_t idx, ProofSlot** out);
void key_release_slots(zkfl_key* k);
// its slots' captured graphs dropped (the key's base sets changed); fails on a busy slot
int key_reset_graphs(zkfl_key* k);
// csrc/groups.hip: the partition's device state released; a partition learned from the resident
// witness d_w (nVars std-form values) and built
void key_groups_release(zkfl_key* k);
int key_learn_groups(zkfl_ctx* ctx, zkfl_key* k, const Fr* d_w);
// ProofSlot::pinned: the proof's count of non-zero u, then (grouped ABC) its dirty constraints and plain flag
constexpr size_t MISS_OFF = 456;
}  // namespace zkfl
