// The proof scheduler and the prove entry points: a key's proof slots (stream, scratch, MSM tails),
// the plan of a proof (plan_proof: decided once, from the context's SchedOpts) and the schedule it
// picks on its slot (run_lowlat for one proof alone, run_front for small keys, run_chain; the last
// two replayed from a graph), the batch scheduler behind every prove call (run_jobs) and the
// batched full-prove pipe with its witness groups and JSON parse pool (full_prove_piped).  The
// kernels it launches live in poly.hip, assemble.hip, ntt.hip and the MSM units.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "assemble.h"
#include "devbufs.h"
#include "glv.h"
#include "groups.h"
#include "host_parse.h"
#include "objects.h"
#include "poly.h"
#include "witness.h"

using namespace zkfl;

namespace {

constexpr size_t W_PTR_OFF = 448;  // pinned: the graph-replayed proof's witness address

// the proof's 256 bytes go straight into the slot's pinned buffer (k_assemble*)
inline uint32_t* proof_out(ProofSlot* s) { return reinterpret_cast<uint32_t*>(s->pinned); }

// Release a slot's latency-schedule streams and events (made again on its next batch of one).
void slot_drop_lowlat(ProofSlot* s) {
  for (hipStream_t& st : s->st_lat)
    if (st) {
      (void)hipStreamSynchronize(st);
      (void)hipStreamDestroy(st);
      st = nullptr;
    }
  for (hipEvent_t& e : s->ev_lat)
    if (e) {
      (void)hipEventDestroy(e);
      e = nullptr;
    }
}

void slot_release(ProofSlot* s) {
  if (!s) return;
  if (s->st_main) (void)hipStreamSynchronize(s->st_main);
  slot_drop_lowlat(s);
  if (s->nnz_alias) s->g2t.nnz = nullptr;
  msm_scratch_free(s->g1s);
#if ZK_KNOCKOUT & 2
  for (MsmScratch<FqOps>& x : s->g1s_ko) msm_scratch_free(x);
#endif
  for (auto& t : s->g1t) msm_tail_free(t);
  msm_scratch_free(s->g2s);
  msm_tail_free(s->g2t);
  void* ptrs[] = {s->abc, s->abc_head, s->abc_tail, s->h, s->res, s->resB2, s->d_rs, s->d_parts,
                  s->w_stage, s->grp_cnt, s->gr_state, s->gr_dirty, s->gr_missing, s->cls_val};  // extra lives in h
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (s->pinned) (void)hipHostFree(s->pinned);
  msm_scratch_free(s->g1s_b);
  msm_scratch_free(s->g1s_a);
  if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
  if (s->graph) (void)hipGraphDestroy(s->graph);
  if (s->ev_done) (void)hipEventDestroy(s->ev_done);
  if (s->st_main) (void)hipStreamDestroy(s->st_main);
  delete s;
}

// A slot's side resources (ProofSlot::g1s_a): A's and B's own sort scratch and, for the latency
// schedule (need_streams), its two side streams and their three events.  What the slot holds
// already is kept.  slot_release frees all of them, slot_drop_lowlat the streams and events.
hipError_t slot_side_resources(ProofSlot* s, const zkfl_key* k, bool need_streams) {
  if (need_streams) {
    for (hipStream_t& st : s->st_lat)
      if (!st) ZK_CHECK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    for (hipEvent_t& e : s->ev_lat)
      if (!e) ZK_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  if (!s->g1s_a.keys_out) ZK_CHECK(msm_scratch_alloc(s->g1s_a, k->bA.n, k->msm_c, k->ctx->st));
  if (!s->g1s_b.keys_out) ZK_CHECK(msm_scratch_alloc(s->g1s_b, k->bB1.n, k->msm_c, k->ctx->st));
  return hipSuccess;
}

hipError_t slot_create(zkfl_key* k, ProofSlot** out) {
  ProofSlot* s = new ProofSlot();
  *out = s;
  const size_t nV = k->nVars, n = k->n;
  const size_t cap1 = std::max<size_t>({k->bA.n, k->bB1.n, k->bCH.n});
  hipStream_t st = k->ctx->st;
  // One stream per slot: a slot's proof is a serial chain and throughput comes from many slots
  // (measured on MI355X, 24 HW queues: 16 slots x 1 stream 238-241 proofs/s vs 8 slots x 3 streams
  // 216-217).
  ZK_CHECK(hipStreamCreateWithFlags(&s->st_main, hipStreamNonBlocking));
  ZK_CHECK(hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming));
  const int c = k->msm_c;
  ZK_CHECK(msm_scratch_alloc(s->g1s, cap1, c, st));
#if ZK_KNOCKOUT & 2
  for (MsmScratch<FqOps>& x : s->g1s_ko) {  // zeroed: an index past a stale sort is base 0
    ZK_CHECK(msm_scratch_alloc(x, cap1, c, st));
    ZK_CHECK(hipMemsetAsync(x.keys_out, 0, cap1 * msm_w_of(c) * sizeof(uint16_t), st));
    ZK_CHECK(hipMemsetAsync(x.vals_out, 0, cap1 * msm_w_of(c) * sizeof(uint32_t), st));
  }
#endif
  // tail 2 is C + H's; tail 3 only serves the parity hook, which runs the C + H MSM twice (C, then H)
  const size_t caps[4] = {k->bA.n, k->bB1.n, k->bCH.n, k->bCH.n};
  for (int i = 0; i < 4; i++) ZK_CHECK(msm_tail_alloc(s->g1t[i], caps[i], c));
  ZK_CHECK(msm_scratch_alloc(s->g2s, k->bB2.n, c, st));
  ZK_CHECK(msm_tail_alloc(s->g2t, k->bB2.n, c));
  if (k->share_b && !ZK_KNOCKOUT) {
    ZK_CHECK(hipFree(s->g2t.nnz));
    s->g2t.nnz = s->g1t[1].nnz;
    s->nnz_alias = true;
  }
  if (k->ctx->opts.graph) ZK_CHECK(hipMalloc(&s->w_stage, nV * 32));
  if (k->front) ZK_CHECK(slot_side_resources(s, k, false));  // run_front: C + H sorts in g1s
  // h, then the extra slots (the merged C+H MSM's scalars), then u where the key may hold a partition
  const bool may_group = k->ctx->opts.groups && k->nshards == 1;
  ZK_CHECK(hipMalloc(&s->h, (n + 4 + (may_group ? nV : 0)) * 32));
  s->extra = s->h + n;
  ZK_CHECK(hipMalloc(&s->grp_cnt, 2 * sizeof(uint32_t)));
  ZK_CHECK(hipMemsetAsync(s->grp_cnt, 0, 2 * sizeof(uint32_t), st));
  // grouped ABC (large keys only: build_rows, csrc/groups.hip): the proof's missing wires and dirty constraints
  if (may_group && k->ctx->opts.group_rows && k->K && k->logn > k->ctx->opts.small_logn) {
    ZK_CHECK(hipMalloc(&s->gr_state, group_rows_state_words(n) * sizeof(uint32_t)));
    ZK_CHECK(hipMalloc(&s->gr_missing, (size_t)group_rows_miss_cap((uint32_t)n) * sizeof(uint32_t)));
    ZK_CHECK(hipMalloc(&s->gr_dirty, (size_t)group_rows_dirty_cap((uint32_t)n) * sizeof(uint32_t)));
  }
  s->key = k;
  ZK_CHECK(hipMalloc(&s->abc, n * 3 * 32));
  const size_t abc_chunks = (k->K + ABC_L - 1) / ABC_L + 1;
  ZK_CHECK(hipMalloc(&s->abc_head, abc_chunks * 32));
  ZK_CHECK(hipMalloc(&s->abc_tail, abc_chunks * 32));
  ZK_CHECK(hipMalloc(&s->res, 5 * sizeof(G1P)));
  ZK_CHECK(hipMalloc(&s->resB2, sizeof(G2P)));
  ZK_CHECK(hipMalloc(&s->d_rs, 2 * 32 + 4 * sizeof(GlvScalar)));
  ZK_CHECK(hipMalloc(&s->d_parts, PART_WORDS * 4));
  // coherent (fine-grained): the proof chain reads r, s and the GLV halves from it and writes the
  // proof into it directly (k_proof_start, k_assemble*), so no copy launches open or close a proof
  ZK_CHECK(hipHostMalloc(&s->pinned, 2048, hipHostMallocCoherent));
  return hipStreamSynchronize(st);
}

}  // namespace

int zkfl::get_slot(zkfl_key* k, size_t idx, ProofSlot** out) {
  size_t want = idx % (size_t)k->max_slots;
  while (k->slots.size() <= want) {
    ProofSlot* s = nullptr;
    hipError_t e = slot_create(k, &s);
    if (e != hipSuccess) {
      slot_release(s);
      return hip_fail(e, "proof slot allocation");
    }
    s->index = (int)k->slots.size();
    k->slots.push_back(s);
  }
  *out = k->slots[want];
  return ZKFL_OK;
}

// Witnesses of the single-key full-prove entry points, computed G (= the key's slots) jobs at a
// time by ONE batched launch sequence of the witness engine on the key's witness stream, ahead of
// the slots that prove them: group g is computed into buffer set g % 3 while the slots prove
// group g - 1 (when group g + 1 is enqueued, the slots have drained group g - 2, so its set is
// free).  Per-slot witnesses cost ~25 small launches per proof on the slot's stream, each a
// permutation-latency chain; batched, a group's 15 levels cost as much as one witness's.
// Witness sets of a key's pipe: group g uses set g % WIT_SETS; groups run up to WIT_SETS - 2 ahead
// of the group the key's slots start (full_prove_piped)
constexpr int WIT_SETS = 4;
struct WitPipe {
  struct Set {
    Fr* W = nullptr;          // [G][nw] Montgomery scratch
    Fr* d = nullptr;          // [G][nw] std-form witnesses = the proofs' scalars
    uint32_t* in = nullptr;   // [G][n_in x 8]
    uint32_t* fail = nullptr; // [G]
    Fr** outs = nullptr;      // [G] device pointers into d
    uint8_t* pin_in = nullptr;
    hipEvent_t ev = nullptr;  // the group's witnesses are complete
  };
  size_t G = 0, nw = 0, n_in = 0;
  hipStream_t st = nullptr;
  Set set[WIT_SETS];
};

namespace {

void wpipe_release(WitPipe* p) {
  if (!p) return;
  if (p->st) (void)hipStreamSynchronize(p->st);
  for (auto& b : p->set) {
    for (void* q : {(void*)b.W, (void*)b.d, (void*)b.in, (void*)b.fail, (void*)b.outs})
      if (q) (void)hipFree(q);
    if (b.pin_in) (void)hipHostFree(b.pin_in);
    if (b.ev) (void)hipEventDestroy(b.ev);
  }
  if (p->st) (void)hipStreamDestroy(p->st);
  delete p;
}

}  // namespace

int zkfl::key_reset_graphs(zkfl_key* k) {
  for (ProofSlot* s : k->slots)
    if (s->busy) return fail(ZKFL_E_ARG, "slots busy");
  for (ProofSlot* s : k->slots) {
    if (s->st_main) (void)hipStreamSynchronize(s->st_main);
    if (s->graph_exec) (void)hipGraphExecDestroy(s->graph_exec);
    if (s->graph) (void)hipGraphDestroy(s->graph);
    s->graph_exec = nullptr;
    s->graph = nullptr;
  }
  return ZKFL_OK;
}

void zkfl::key_release_slots(zkfl_key* k) {
  wpipe_release(k->wpipe);
  k->wpipe = nullptr;
  for (ProofSlot* s : k->slots) slot_release(s);
  k->slots.clear();
}

namespace {

// The key's pipe for groups of G witnesses of nw wires and n_in inputs (kept between calls).
hipError_t wpipe_get(zkfl_key* k, size_t G, size_t nw, size_t n_in, WitPipe** out) {
  WitPipe* p = k->wpipe;
  if (p && p->G == G && p->nw == nw && p->n_in == n_in) {
    *out = p;
    return hipSuccess;
  }
  wpipe_release(p);
  k->wpipe = p = new WitPipe();
  p->G = G;
  p->nw = nw;
  p->n_in = n_in;
  ZK_CHECK(hipStreamCreateWithFlags(&p->st, hipStreamNonBlocking));
  for (auto& b : p->set) {
    ZK_CHECK(hipMalloc(&b.W, G * nw * 32));
    ZK_CHECK(hipMalloc(&b.d, G * nw * 32));
    ZK_CHECK(hipMalloc(&b.in, G * n_in * 32 + 16));
    ZK_CHECK(hipMalloc(&b.fail, G * 4));
    ZK_CHECK(hipMalloc(&b.outs, G * sizeof(Fr*)));
    ZK_CHECK(hipHostMalloc(&b.pin_in, G * n_in * 32 + 16));
    ZK_CHECK(hipEventCreateWithFlags(&b.ev, hipEventDisableTiming));
    std::vector<Fr*> ptrs(G);
    for (size_t j = 0; j < G; j++) ptrs[j] = b.d + j * nw;
    ZK_CHECK(hipMemcpy(b.outs, ptrs.data(), G * sizeof(Fr*), hipMemcpyHostToDevice));
  }
  *out = p;
  return hipSuccess;
}

int get_rs(const uint8_t* rs, uint32_t out[16]) {
  if (rs) {
    memcpy(out, rs, 64);
    if (!fr_lt_r(out) || !fr_lt_r(out + 8)) return fail(ZKFL_E_ARG, "r/s must be < r");
    return ZKFL_OK;
  }
  // CSPRNG, rejection-sample below r (snarkjs: Fr.random())
  for (int k = 0; k < 2; k++) {
    for (int tries = 0;; tries++) {
      uint8_t b[32];
      if (getrandom(b, 32, 0) != 32) return fail(ZKFL_E_DEVICE, "getrandom failed");
      b[31] &= 0x3f;  // < 2^254
      memcpy(out + 8 * k, b, 32);
      if (fr_lt_r(out + 8 * k)) break;
      if (tries > 64) return fail(ZKFL_E_DEVICE, "rng");
    }
  }
  return ZKFL_OK;
}

// count scalars of 32 B, each < r; the error names the first that is not
int check_fr(const uint8_t* v, size_t count, const std::string& what) {
  for (size_t i = 0; i < count; i++) {
    uint32_t w[8];
    memcpy(w, v + 32 * i, 32);
    if (!fr_lt_r(w)) return fail(ZKFL_E_ARG, what + " " + std::to_string(i) + " is not < r");
  }
  return ZKFL_OK;
}

// What a proof is run for.
enum class ProofMode {
  Proof,      // a whole proof: its 256 bytes assembled into the slot's pinned buffer
  Parts,      // the parity hook: alpha/beta/delta/r/s terms zeroed, C and H apart, nothing assembled
  SplitPart,  // a split proof's shard: the full augmentation (on shard 0's bases), no assembly; the
              // part A' | B1' | B2' | C' + H | infinity goes to pinned + 512
};

enum class Schedule { Lowlat, Front, Chain };  // run_lowlat, run_front, run_chain

// How one proof runs on its slot: decided once (plan_proof), then only read.
struct ProofPlan {
  ProofMode mode;
  Schedule schedule;
  bool share_b_sort;  // B2 accumulates from B1's sorted pairs (b2_from_b1_sort)
  bool light_first;   // run_chain: ABC / NTT ahead of the witness-scalar MSMs (the stagger)
  bool joint_tails;   // the G2 tail joins the G1 tails' launches (msm_tails_joint)
  bool fast_wsum;     // the shorter-chain bucket reduction (msm.h MSM_WSUM_Q_FAST)
  bool graph;         // replayed from the slot's graph (enqueue_proof_graph), witness staged
  bool grouped;       // the key's grouped base sets and the differences u (csrc/groups.h)
  bool group_rows;    // and its row classes: the grouped ABC (grouped, on a key that kept them)
};

// The four base sets a plan's proof runs over.
struct PlanBases {
  const MsmBases<FqOps>&A, &B1, &CH;
  const MsmBases<Fq2Ops>& B2;
};
inline PlanBases plan_bases(const zkfl_key* k, const ProofPlan& p) {
  if (p.grouped) return {k->gA, k->gB1, k->gCH, k->gB2};
  return {k->bA, k->bB1, k->bCH, k->bB2};
}

// The plan of the next proof of key k on slot s; batch_of_one: it is its batch's only proof.
ProofPlan plan_proof(const SchedOpts& o, const zkfl_key* k, const ProofSlot* s, ProofMode mode, bool batch_of_one,
                     const Profiler* prof) {
  ProofPlan p = {};
  p.mode = mode;
  // whole proofs on a key that holds a partition (only unsharded keys do) run the grouped sets
  p.grouped = mode == ProofMode::Proof && k->grp.on && !ZK_KNOCKOUT;
  p.group_rows = p.grouped && k->grp.rows_on && s->gr_state;
  // the latency schedule and graph replay serve whole proofs of the plain build on a key whose B
  // queries share a sort; a serialized profile wants one stream, launch by launch
  const bool plain = mode == ProofMode::Proof && k->share_b && !prof->serialize && !ZK_KNOCKOUT;
  // a batch of one proof runs the latency schedule (ZKFL_LOWLAT=0: a one-stream schedule)
  const bool want_lowlat = batch_of_one && o.lowlat;
  // graph replay from a slot's second proof on (a one-off proof pays no capture); the latency
  // schedule is never captured
  p.graph = o.graph && s->w_stage && !want_lowlat && plain && !prof->on && s->direct_proofs > 0;
  // B1's digit sort also serves B2 (same scalars, same index map).  A key whose two index maps differ
  // runs B2 as an MSM of its own (own sort, own tail).
  p.share_b_sort = k->share_b && !(ZK_KNOCKOUT & 32);
  if (want_lowlat && plain) {
    p.schedule = Schedule::Lowlat;
    p.fast_wsum = o.fast_wsum;  // (ZKFL_FAST_WSUM=0 keeps the throughput reduction: A/B)
    return p;
  }
  // Small keys: the G2 tail joins the G1 tails' launches (msm_tails_joint) instead of running right
  // after B2 -- config 5 2,712 vs 2,385 proofs/s (3 same-box alternations); the metric key keeps the
  // separate tails (M 433 vs 439 and 431 vs 433 with them joint, two boxes:
  // profiles/r06_ab_joint_tails.log, r06_ab_front.log)
  p.joint_tails = p.share_b_sort && k->front;
  // and their three G1 MSMs sort and accumulate together (run_front).  The parity hook keeps the
  // chain, which returns C and H apart; a split proof's shard never has k->front (nshards == 1).
  const bool front = p.joint_tails && mode != ProofMode::Parts && !(ZK_KNOCKOUT & 2);
  p.schedule = front ? Schedule::Front : Schedule::Chain;
  // Stage order of the chain.  Every slot runs the same chain, so under load the slots move as a
  // convoy: the accumulations fill the GPU one at a time, and the slots that leave them together
  // reach ABC + NTT together -- the wave timeline (tools/wtrace.py) showed stretches of ~4 ms with
  // no accumulation resident at all.  Staggered (the default; ZKFL_STAGGER=0 turns it off): odd
  // slots run ABC + NTT before their witness-scalar MSMs instead of after, so their light phase falls
  // beside the others' heavy one (+2.3 %, 407.5 vs 398.6 proofs/s, 3 same-box alternations).
  p.light_first = !front && o.stagger && (s->index & 1) && !prof->serialize;
  // Small keys (domain <= 2^ZKFL_SMALL_LOGN, default 2^16: config 5's circuits) take the
  // shorter-chain reduction in batches too: their proofs are chains of small latency-bound kernels
  // that leave most of the GPU idle (config-5 wave trace: SIMD share 0.135 with a wave resident 99%
  // of the time), so the reduction's extra waves are free and its shorter chain is not.
  p.fast_wsum = o.fast_wsum && k->logn <= o.small_logn;
  return p;
}

inline const GlvScalar* glv_halves(const ProofSlot* s) {  // s1, s2, r1, r2 behind r, s in d_rs
  return reinterpret_cast<const GlvScalar*>(reinterpret_cast<const uint8_t*>(s->d_rs) + 64);
}

// Step: k_proof_start on the slot's stream, after the host has put r, s and the GLV halves into
// the pinned buffer -- r, s and the halves to the device, the blinding scalars behind h, the tails
// this plan accumulates into emptied: G1 A, B1, C + H, [H]; G2 B2 when it shares B1's sort (its own
// msm_run empties its tail itself).  A graph-replayed proof stages its witness here.
void start(zkfl_key* k, ProofSlot* s, const ProofPlan& p) {
  // C + H is one MSM into tail 2 (res[2] = C' + H, res[3] = infinity); the parity hook's are apart
  const bool parts = p.mode == ProofMode::Parts;
  const int ntails = parts ? 4 : 3;
  ProofStart ps = {};
  auto add = [&](void* buckets, size_t bytes, uint32_t* nnz, uint32_t* live) {
    ps.buckets[ps.n] = static_cast<uint4*>(buckets);
    ps.nvec[ps.n] = (uint32_t)(bytes / sizeof(uint4));
    ps.nnz[ps.n] = nnz;
    ps.live[ps.n] = live;
    ps.n++;
  };
  const size_t nb = msm_nb_of(k->msm_c);
  for (int i = 0; i < ntails; i++) add(s->g1t[i].buckets, nb * sizeof(G1P), s->g1t[i].nnz, s->g1t[i].live);
  if (p.share_b_sort) add(s->g2t.buckets, nb * sizeof(G2P), s->g2t.nnz, s->g2t.live);
  uint32_t* res3 = parts ? nullptr : reinterpret_cast<uint32_t*>(s->res + 3);
  if (p.graph) {  // from the address enqueue_proof left in the pinned buffer
    ps.w_src_host = reinterpret_cast<const uint64_t*>(s->pinned + W_PTR_OFF);
    ps.w_dst = reinterpret_cast<uint4*>(s->w_stage);
    ps.w_nvec = (uint32_t)((size_t)k->nVars * 32 / sizeof(uint4));
  }
  if (p.group_rows) {  // a replayed graph starts clean after a dirty proof
    ps.gr_state = s->gr_state;
    ps.gr_words = (uint32_t)group_rows_state_words(k->n);
  }
  proof_start(s->st_main, reinterpret_cast<const uint32_t*>(s->pinned + 256), reinterpret_cast<uint32_t*>(s->d_rs),
              s->extra, parts, res3, ps);
}

// What k_group_delta marks for a plan's proof: the key's wire lists into the slot's state.
inline GroupMark group_mark(const zkfl_key* k, const ProofSlot* s, const ProofPlan& p) {
  if (!p.group_rows) return GroupMark{};
  return {k->grp.d_wstart, k->grp.d_wlist, s->gr_state, s->gr_missing, group_rows_miss_cap(k->n), s->gr_dirty,
          group_rows_dirty_cap(k->n)};
}

// Step: a, b, c on the domain (Montgomery form) into the slot's abc, in the plan's form: the
// grouped ABC reads what start and k_group_delta left in the slot's state.
void abc_stage(zkfl_key* k, ProofSlot* s, const Fr* d_w, hipStream_t st, const ProofPlan& p) {
  const size_t n = k->n;
  const uint32_t K = (uint32_t)k->K;
  const AbcTerms T = {k->cols, k->coefs, k->cshift};
  if (p.group_rows) {
    const KeyGroups& g = k->grp;
    const AbcTerms R = {g.d_cterms, k->cshift ? k->coefs : g.d_ccoefs, k->cshift};
    const AbcGrouped G = {g.d_crp, g.row_classes, R, g.terms_rep, g.d_cls, s->cls_val, s->gr_state, s->gr_dirty,
                          group_rows_dirty_cap(k->n), reinterpret_cast<uint32_t*>(s->pinned + MISS_OFF) + 1};
    abc_grouped(st, G, k->rows, n, T, d_w, K, s->abc_head, s->abc_tail, s->abc);
    return;
  }
  if (K) abc_chunks(st, k->rows, (uint32_t)(2 * n), T, d_w, K, s->abc_head, s->abc_tail, s->abc);
  abc_rows(st, k->rows, n, K, s->abc_head, s->abc_tail, s->abc);
}

// Step: ABC (a, b, c on the domain), the coset NTT of all three and h = a b - c (std form: the H
// MSM's scalars) on stream st.
hipError_t abc_ntt(zkfl_key* k, ProofSlot* s, const Fr* d_w, hipStream_t st, const ProofPlan& p, Profiler* prof) {
  const size_t n = k->n;
  int pi = prof->begin("abc", st);
  abc_stage(k, s, d_w, st, p);
  prof->end(pi, st, (double)k->K);
  pi = prof->begin("ntt", st);
  if (!(ZK_KNOCKOUT & 4)) ZK_CHECK(ntt_coset_shift(k->ntt, s->abc, 3, n, st));
  prof->end(pi, st, 3.0 * (double)n);
  join_h(st, s->abc, n, s->h);
  return hipSuccess;
}

// Step: B2 from B1's sort.  `sorted` holds the pairs of B's digit sort (whoever sorted, on
// whichever stream, ordered before st here); B2 accumulates from them into its tail g2t on st before
// anything reuses that scratch.  Its tail counts with B1's nnz (b1_nnz), copied unless the two alias
// (ProofSlot::nnz_alias).
hipError_t b2_from_b1_sort(const MsmBases<Fq2Ops>& bB2, MsmTail<Fq2Ops>& g2t, const uint32_t* b1_nnz, bool nnz_alias,
                           const MsmScratch<FqOps>& sorted, hipStream_t st, Profiler* prof) {
  if (!nnz_alias) ZK_CHECK(hipMemcpyAsync(g2t.nnz, b1_nnz, sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return msm_accumulate_sorted(bB2, sorted.keys_out, sorted.vals_out, g2t, st, prof, "msm_accumulate_g2");
}

// Step: what leaves a one-stream schedule -- a split proof's part and its download, a proof's
// assembly (pi_a, pi_b, pi_c) into the pinned buffer, nothing for the parity hook (its caller
// reads res, resB2 and h).  A key in D form first turns tail 0's A' - B1' into A' (every mode reads
// res[0]).
int finish(const zkfl_key* k, ProofSlot* s, const ProofPlan& p, Profiler* prof) {
  hipStream_t st = s->st_main;
  if (k->a_diff) fold_a(st, s->res);
  if (p.mode == ProofMode::SplitPart) {
    part_out(st, s->res, s->resB2, s->d_parts);
    HIP_TRY(hipMemcpyAsync(s->pinned + 512, s->d_parts, PART_WORDS * 4, hipMemcpyDeviceToHost, st), "download part");
  }
  if (p.mode == ProofMode::Proof && !(ZK_KNOCKOUT & 1)) {
    const int pa = prof->begin("assemble", st);
    assemble(st, 1, s->res, s->resB2, glv_halves(s), proof_out(s));
    prof->end(pa, st, 1.0);
  }
  return ZKFL_OK;
}

// One proof alone (a batch of one: the CLI's `groth16 prove`, the API's prove): its latency is
// the metric, and the GPU is mostly idle along the one-stream chain, so the two long chains start
// at once on streams of their own:
//   main : [start] [ev ready] ABC, coset NTT, join, C + H (sort + accumulate), its tail,
//          wait(B2, T), k_assemble_c (pi_c, pi_b) into the pinned buffer
//   lat0 : wait(ev ready) B sort (own scratch) [ev B sorted] B2 + its tail [ev B2]
//   lat1 : wait(ev B sorted) B1, A (sort into its own scratch + accumulate), the tails of A and
//          B1, [A' += B1': a key in D form], k_assemble_t (T = s pi_A + r B1, pi_a) [ev T]
// Same proof bytes as the one-stream schedules (k_assemble_t / _c form the same points).  The
// round-4 schedule ran A and B1 on the main stream ahead of ABC / NTT (4.10 vs 4.16 ms then); with
// the row assembly and the divsteps inversions the overlap wins: 3.586 vs 3.712 ms, 3 same-box
// alternations (profiles/r06_ab_lowlat2.log), and the round-4 one was deleted, with its
// per-segment graph replay (ZKFL_GRAPH=2: no gain, profiles/r04_ab_lowlat_seg_graphs.log).
int run_lowlat(zkfl_key* k, ProofSlot* s, const Fr* d_w, const ProofPlan& p, Profiler* prof) {
  HIP_TRY(slot_side_resources(s, k, true), "latency schedule resources");
  hipStream_t st = s->st_main, sb = s->st_lat[0], sa = s->st_lat[1];
  // ev_lat[0] marks "ready" then (re-recorded on lat0) "B sorted": each wait is enqueued before
  // the next record, so every wait sees the record it was meant for
  hipEvent_t ev = s->ev_lat[0], ev_b2 = s->ev_lat[1], ev_t = s->ev_lat[2];
  const uint32_t *W = (const uint32_t*)d_w, *E = (const uint32_t*)s->extra;
  const PlanBases b = plan_bases(k, p);
  MsmTail<FqOps>* tails[3] = {&s->g1t[0], &s->g1t[1], &s->g1t[2]};
  G1P* outs[3] = {s->res + 0, s->res + 1, s->res + 2};
  MsmTail<Fq2Ops>* t2 = &s->g2t;
  G2P* o2 = s->resB2;
  HIP_TRY(hipEventRecord(ev, st), "event");  // (tails emptied by k_proof_start)
  // lat0: B's sort, then B2 and its tail
  HIP_TRY(hipStreamWaitEvent(sb, ev, 0), "wait");
  HIP_TRY(msm_sort(b.B1, s->g1s_b, s->g1t[1].nnz, W, E, sb), "msm B sort");
  HIP_TRY(hipEventRecord(ev, sb), "event");
  HIP_TRY(hipStreamWaitEvent(sa, ev, 0), "wait");
  HIP_TRY(b2_from_b1_sort(b.B2, s->g2t, s->g1t[1].nnz, s->nnz_alias, s->g1s_b, sb, prof), "msm B2");
  HIP_TRY(msm_tails(&t2, &o2, 1, sb, p.fast_wsum), "msm B2 tail");
  HIP_TRY(hipEventRecord(ev_b2, sb), "event");
  // lat1: B1 (B's pairs), A, their tails, then T = s pi_A + r B1 and pi_a
  HIP_TRY(msm_accumulate_sorted(b.B1, s->g1s_b.keys_out, s->g1s_b.vals_out, s->g1t[1], sa, prof,
                                   "msm_accumulate_g1"), "msm B1");
  HIP_TRY(msm_accumulate(b.A, s->g1s_a, s->g1t[0], W, E, sa, prof, "msm_accumulate_g1"), "msm A");
  HIP_TRY(msm_tails(tails, outs, 2, sa, p.fast_wsum), "msm tails A, B1");
  if (k->a_diff) fold_a(sa, s->res);  // D form: A' = (A' - B1') + B1'
  assemble_t(sa, s->res, glv_halves(s), proof_out(s));
  HIP_TRY(hipEventRecord(ev_t, sa), "event");
  // main: ABC / NTT / h, C + H and its tail, then pi_c and pi_b
  HIP_TRY(abc_ntt(k, s, d_w, st, p, prof), "ntt");
  HIP_TRY(msm_accumulate(b.CH, s->g1s, s->g1t[2], W, (const uint32_t*)s->h, st, prof, "msm_accumulate_g1"),
          "msm C+H");
  HIP_TRY(msm_tails(&tails[2], &outs[2], 1, st, p.fast_wsum), "msm tail C+H");
  HIP_TRY(hipStreamWaitEvent(st, ev_b2, 0), "wait");
  HIP_TRY(hipStreamWaitEvent(st, ev_t, 0), "wait");
  const int pa = prof->begin("assemble", st);
  assemble_c(st, s->res, s->resB2, proof_out(s));
  prof->end(pa, st, 1.0);
  return ZKFL_OK;
}

// The MSM stage of a small key's proof (run_front) over n1 G1 sets and the G2 set that rides on
// set ib's sort: the n1 sorts in the same four launches (each in its own scratch), the n1
// accumulations in one launch, B2 from set ib's pairs, then the tails -- joint: G1 and G2 as one
// batch (msm_tails_joint, what proofs run); otherwise the batched G1 tails and the G2 tail after
// them (msm_tails, the form of run_chain and run_lowlat).  Every tail must have been emptied.  The
// parity hook zkfl_debug_msm_front runs this same function on a caller's sets.
struct FrontMsm {
  int n1 = 0;                                    // G1 sets (a proof: A, B1, C + H)
  const MsmBases<FqOps>* bases[MSM_TAIL_MAX] = {};
  MsmScratch<FqOps>* scratch[MSM_TAIL_MAX] = {};
  MsmTail<FqOps>* tails[MSM_TAIL_MAX] = {};
  const uint32_t* scalars[MSM_TAIL_MAX] = {};    // per set: its scalar vector
  const uint32_t* extra[MSM_TAIL_MAX] = {};      // and what its index map's extra slots address
  G1P* outs[MSM_TAIL_MAX] = {};
  int ib = 1;                                    // the set that plays B1
  const MsmBases<Fq2Ops>* b2 = nullptr;
  MsmTail<Fq2Ops>* t2 = nullptr;
  bool nnz_alias = false;                        // t2->nnz is tails[ib]->nnz (no copy)
  G2P* out2 = nullptr;
};
int front_msm(const FrontMsm& m, hipStream_t st, bool fast, bool joint, Profiler* prof) {
  const int n = m.n1;
  uint32_t* nn[MSM_TAIL_MAX] = {};
  const uint16_t* kk[MSM_TAIL_MAX] = {};
  const uint32_t* vv[MSM_TAIL_MAX] = {};
  for (int i = 0; i < n; i++) nn[i] = m.tails[i]->nnz;
  HIP_TRY(msm_sort_multi(m.bases, m.scratch, nn, m.scalars, m.extra, n, st), "msm A, B1, C+H sorts");
  for (int i = 0; i < n; i++) {
    kk[i] = m.scratch[i]->keys_out;
    vv[i] = m.scratch[i]->vals_out;
  }
  HIP_TRY(msm_accumulate_sorted_multi(m.bases, kk, vv, m.tails, n, st), "msm A, B1, C+H");
  HIP_TRY(b2_from_b1_sort(*m.b2, *m.t2, m.tails[m.ib]->nnz, m.nnz_alias, *m.scratch[m.ib], st, prof), "msm B2");
  MsmTail<Fq2Ops>* t2 = m.t2;
  G2P* o2 = m.out2;
  if (joint) {
    HIP_TRY(msm_tails_joint(m.tails, m.outs, n, &t2, &o2, 1, st, fast), "msm tails (G1 + G2)");
  } else {
    HIP_TRY(msm_tails(m.tails, m.outs, n, st, fast), "msm tails");
    HIP_TRY(msm_tails(&t2, &o2, 1, st, fast), "msm B2 tail");
  }
  return ZKFL_OK;
}

// Small keys, one stream:
//   [start] ABC, coset NTT, join, A, B1 and C + H sorted together (each in its own scratch) and
//   accumulated in one launch, B2 from B1's pairs, the G1 and G2 tails as one batch, [finish]
// Their proofs are chains of latency-bound launches: fewer links, shorter chain (config 5 2,802 vs
// 2,748 proofs/s, 3 same-box alternations, profiles/r06_ab_front.log).
int run_front(zkfl_key* k, ProofSlot* s, const Fr* d_w, const ProofPlan& p, Profiler* prof) {
  hipStream_t st = s->st_main;
  const uint32_t *W = (const uint32_t*)d_w, *E = (const uint32_t*)s->extra;
  HIP_TRY(abc_ntt(k, s, d_w, st, p, prof), "ntt");
  const PlanBases b = plan_bases(k, p);
  FrontMsm m;
  m.n1 = 3;
  const MsmBases<FqOps>* bs[3] = {&b.A, &b.B1, &b.CH};
  MsmScratch<FqOps>* ss[3] = {&s->g1s_a, &s->g1s_b, &s->g1s};
  const uint32_t* ex[3] = {E, E, (const uint32_t*)s->h};
  for (int i = 0; i < 3; i++) {
    m.bases[i] = bs[i];
    m.scratch[i] = ss[i];
    m.tails[i] = &s->g1t[i];
    m.scalars[i] = W;
    m.extra[i] = ex[i];
    m.outs[i] = s->res + i;
  }
  m.ib = 1;
  m.b2 = &b.B2;
  m.t2 = &s->g2t;
  m.nnz_alias = s->nnz_alias;
  m.out2 = s->resB2;
  const int rc = front_msm(m, st, p.fast_wsum, true, prof);
  if (rc) return rc;
  return finish(k, s, p, prof);
}

// Every other proof, a serial chain on the slot's one stream:
//   [start] [B2 as an MSM of its own: a key whose B queries do not share a sort]
//   [ABC, coset NTT, join: light_first] A, B sort, B1, B2 from B1's pairs [B2's tail unless joint]
//   [ABC, coset NTT, join: otherwise] C + H, the G1 tails as one batch [with B2's: joint], [finish]
// The parity hook runs the C + H MSM twice over the key's zero vectors and finishes four tails:
// C = over (witness, zero h) in C + H's place before ABC / NTT, H = over (zero witness, h) after.
int run_chain(zkfl_key* k, ProofSlot* s, const Fr* d_w, const ProofPlan& p, Profiler* prof) {
  hipStream_t st = s->st_main;
  const bool parts = p.mode == ProofMode::Parts;
  if (parts && !k->dbg_zero) return fail(ZKFL_E_ARG, "parity hook: zeros not allocated");
  const uint32_t *W = (const uint32_t*)d_w, *E = (const uint32_t*)s->extra, *H = (const uint32_t*)s->h,
                 *Z = (const uint32_t*)k->dbg_zero;
#if ZK_KNOCKOUT & 2
  MsmScratch<FqOps>&sA = s->g1s_ko[0], &sB = s->g1s_ko[1], &sCH = s->g1s_ko[2];
#else
  MsmScratch<FqOps>&sA = s->g1s, &sB = s->g1s, &sCH = s->g1s;
#endif
  const PlanBases b = plan_bases(k, p);
  MsmTail<FqOps>* tails[4] = {&s->g1t[0], &s->g1t[1], &s->g1t[2], &s->g1t[3]};
  G1P* outs[4] = {s->res + 0, s->res + 1, s->res + 2, s->res + 3};
  MsmTail<Fq2Ops>* t2 = &s->g2t;
  G2P* o2 = s->resB2;
  if (!p.share_b_sort && !(ZK_KNOCKOUT & 32))
    HIP_TRY(msm_run(b.B2, s->g2s, s->g2t, W, E, s->resB2, st, prof, "msm_accumulate_g2"), "msm B2");
  if (p.light_first) HIP_TRY(abc_ntt(k, s, d_w, st, p, prof), "ntt");
  HIP_TRY(msm_accumulate(b.A, sA, s->g1t[0], W, E, st, prof, "msm_accumulate_g1"), "msm A");
  if (p.share_b_sort) {  // B2 right after B1, before C + H reuses the sort scratch
    HIP_TRY(msm_sort(b.B1, sB, s->g1t[1].nnz, W, E, st), "msm B1 sort");
    HIP_TRY(msm_accumulate_sorted(b.B1, sB.keys_out, sB.vals_out, s->g1t[1], st, prof, "msm_accumulate_g1"),
            "msm B1");
    HIP_TRY(b2_from_b1_sort(b.B2, s->g2t, s->g1t[1].nnz, s->nnz_alias, sB, st, prof), "msm B2");
    if (!p.joint_tails) HIP_TRY(msm_tails(&t2, &o2, 1, st, p.fast_wsum), "msm B2 tail");
  } else {
    HIP_TRY(msm_accumulate(b.B1, sB, s->g1t[1], W, E, st, prof, "msm_accumulate_g1"), "msm B1");
  }
  if (parts) HIP_TRY(msm_accumulate(b.CH, s->g1s, s->g1t[2], W, Z, st, prof, "msm_accumulate_g1"), "msm C");
  if (!p.light_first) HIP_TRY(abc_ntt(k, s, d_w, st, p, prof), "ntt");
  if (parts)
    HIP_TRY(msm_accumulate(b.CH, s->g1s, s->g1t[3], Z, H, st, prof, "msm_accumulate_g1"), "msm H");
  else
    HIP_TRY(msm_accumulate(b.CH, sCH, s->g1t[2], W, H, st, prof, "msm_accumulate_g1"), "msm C+H");
  const int ntails = parts ? 4 : 3;
  if (p.joint_tails)
    HIP_TRY(msm_tails_joint(tails, outs, ntails, &t2, &o2, 1, st, p.fast_wsum), "msm tails (G1 + G2)");
  else
    HIP_TRY(msm_tails(tails, outs, ntails, st, p.fast_wsum), "msm tails");
  return finish(k, s, p, prof);
}

// The device work of one proof, launch by launch: start, then its plan's schedule.
int run_proof(zkfl_ctx* ctx, zkfl_key* k, ProofSlot* s, const Fr* d_w, const ProofPlan& p) {
  Profiler* prof = &ctx->prof;
  const int pp = prof->begin("prove", s->st_main);
  start(k, s, p);
  // the differences u behind the blinding scalars, from the witness the schedule reads (a
  // graph-replayed proof's stage, just filled by k_proof_start), before any MSM of any stream; with
  // them the dirty constraints of the grouped ABC, before any schedule reaches its ABC
  if (p.grouped)
    group_delta(s->st_main, d_w, k->grp.d_rep, k->nVars, s->extra + 4, s->grp_cnt,
                reinterpret_cast<uint32_t*>(s->pinned + MISS_OFF), group_mark(k, s, p));
  if (p.group_rows) group_mark_rows(s->st_main, group_mark(k, s, p));
  const int rc = p.schedule == Schedule::Lowlat  ? run_lowlat(k, s, d_w, p, prof)
                 : p.schedule == Schedule::Front ? run_front(k, s, d_w, p, prof)
                                                 : run_chain(k, s, d_w, p, prof);
  if (rc) return rc;
  prof->end(pp, s->st_main, 1.0);
  return ZKFL_OK;
}

// Graph replay of the one-stream schedules (the default; ZKFL_GRAPH=0 launches kernel by kernel;
// config 5 +3.5%, 1894 vs 1831 proofs/s, M +0.6% inside the spread, 3 same-box alternations,
// profiles/r04_ab_c5_small_keys.log, r04_ab_m_graph_target.log): a slot captures its proof's ~40
// launches once, over its witness stage, and then launches the graph -- one host call per proof
// instead of one per kernel.  Kernel arguments are the slot's own buffers and the key's, all fixed,
// as is the slot's plan; r and s reach the device through the captured copy from the slot's pinned
// buffer.
int enqueue_proof_graph(zkfl_ctx* ctx, zkfl_key* k, ProofSlot* s, const ProofPlan& p) {
  hipStream_t st = s->st_main;
  if (!s->graph_exec) {
    HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal), "begin capture");
    const int rc = run_proof(ctx, k, s, s->w_stage, p);
    hipError_t e = hipStreamEndCapture(st, &s->graph);
    if (rc == ZKFL_OK && e == hipSuccess) e = hipGraphInstantiate(&s->graph_exec, s->graph, nullptr, nullptr, 0);
    if (rc || e != hipSuccess) {
      if (s->graph) (void)hipGraphDestroy(s->graph);
      s->graph = nullptr;
      s->graph_exec = nullptr;
      return rc ? rc : hip_fail(e, "graph capture");
    }
  }
  HIP_TRY(hipGraphLaunch(s->graph_exec, st), "graph launch");
  return ZKFL_OK;
}

// Enqueue one proof on a slot (asynchronous): r, s and their GLV halves into the pinned buffer,
// the proof's plan, then the plan's graph or its launches [ev_done].
int enqueue_proof(zkfl_ctx* ctx, zkfl_key* k, ProofSlot* s, const Fr* d_w, const uint32_t rs_host[16], ProofMode mode,
                  bool batch_of_one) {
  memcpy(s->pinned + 256, rs_host, 64);
  GlvScalar* ks = reinterpret_cast<GlvScalar*>(s->pinned + 320);
  glv_split(rs_host + 8, ks[0], ks[1]);  // s -> s1, s2 (for pi_A, phi(pi_A))
  glv_split(rs_host, ks[2], ks[3]);      // r -> r1, r2 (for B1, phi(B1))
  const ProofPlan p = plan_proof(ctx->opts, k, s, mode, batch_of_one, &ctx->prof);
  s->grouped_run = p.grouped;
  s->rows_run = p.group_rows;
  // the class values, sized by the partition the key holds now (a new partition drops the slot's
  // graph, so a captured pointer never outlives its buffer)
  if (p.group_rows && s->cls_cap < k->grp.row_classes) {
    if (s->cls_val) (void)hipFree(s->cls_val);
    s->cls_val = nullptr;
    s->cls_cap = 0;
    HIP_TRY(hipMalloc(&s->cls_val, (size_t)k->grp.row_classes * 32), "class values");
    s->cls_cap = k->grp.row_classes;
  }
  int rc;
  if (p.graph) {
    // the witness is staged into the slot's own buffer so the captured kernel arguments hold for
    // every witness: k_proof_start copies it into the stage from the address left here
    const uint64_t src = reinterpret_cast<uint64_t>(d_w);
    memcpy(s->pinned + W_PTR_OFF, &src, sizeof(src));
    rc = enqueue_proof_graph(ctx, k, s, p);
  } else {
    s->direct_proofs++;
    rc = run_proof(ctx, k, s, d_w, p);
  }
  if (rc) return rc;
  HIP_TRY(hipEventRecord(s->ev_done, s->st_main), "event");
  HIP_TRY(hipGetLastError(), "launch");
  return ZKFL_OK;
}

// Host wait for a device event.  hipEventSynchronize on these (non-blocking-sync) events spins a
// host core for the whole wait: it was most of config 5's host CPU per proof (0.55-0.57 ms, 1.2
// cores busy at ~2,100 proofs/s).  A batch (poll = true) polls instead, sleeping WAIT_US
// microseconds between queries: 0.13-0.16 ms per proof, 0.3 cores, throughput within
// the spread (2,091 vs 2,095 proofs/s, 3 same-box alternations, profiles/r05_ab_c5_fold_wait.log,
// which A/Bs the waits beside a since-removed fold knob);
// the scheduler refills a freed slot up to that much later, ~0.1% of an M step.  A proof alone (the
// latency path) keeps the spin.
constexpr int WAIT_US = 50;
static hipError_t host_wait(hipEvent_t ev, bool poll) {
  if (!poll) return hipEventSynchronize(ev);
  for (;;) {
    const hipError_t e = hipEventQuery(ev);
    if (e != hipErrorNotReady) return e;
    std::this_thread::sleep_for(std::chrono::microseconds(WAIT_US));
  }
}

int wait_slot(ProofSlot* s, bool poll = false) {
  HIP_TRY(host_wait(s->ev_done, poll), "sync");
  if (s->out_proof) memcpy(s->out_proof, s->pinned, 256);
  if (s->out_part) memcpy(s->out_part, s->pinned + 512, PART_WORDS * 4);
  if (s->grouped_run) {
    uint32_t c[3];
    memcpy(c, s->pinned + MISS_OFF, sizeof(c));
    KeyGroups& g = s->key->grp;
    g.last_miss = c[0];
    g.last_dirty = s->rows_run ? c[1] : 0;
    g.last_plain = s->rows_run ? c[2] : 0;
  }
  s->rows_run = false;
  s->grouped_run = false;
  s->busy = false;
  return ZKFL_OK;
}

// One proof of a batch: a device-resident witness, complete once w_ready is (nullptr: already).
// Jobs of one batch may use different keys.
struct Job {
  zkfl_key* key = nullptr;
  const Fr* w = nullptr;
  hipEvent_t w_ready = nullptr;  // the witness group of the full-prove pipe (full_prove_piped)
  const uint8_t* rs = nullptr;  // 64 B or nullptr (CSPRNG)
  uint8_t* proof_out = nullptr;
  uint8_t* part_out = nullptr;  // split proof: this shard's part instead of a proof
};

// A batch call of at least SchedOpts::group_min_batch proofs meets key J.key for the first time: an
// unsharded key without a partition learns one from this job's witness, and a key whose learned
// partition missed on more than half of its non-representative wires in its last proof learns
// again (once per call: a key is met once).  A single proof never pays for learning.
int learn_for_batch(zkfl_ctx* ctx, const Job& J, size_t n) {
  zkfl_key* k = J.key;
  if (!ctx->opts.groups || ZK_KNOCKOUT || n < (size_t)ctx->opts.group_min_batch || k->nshards != 1 || J.part_out)
    return ZKFL_OK;
  const KeyGroups& g = k->grp;
  if (g.on && !(g.learned && 2 * (uint64_t)g.last_miss > g.non_rep)) return ZKFL_OK;
  if (J.w_ready) HIP_TRY(hipEventSynchronize(J.w_ready), "wait for the witness group");
  return key_learn_groups(ctx, k, J.w);
}

// The batch scheduler behind every prove entry point: job i goes to the next slot of its key
// (round robin per key), a busy slot is drained first, so up to max_slots proofs per key are in
// flight and proofs of different keys (e.g. the training and secure-aggregation circuits of one
// federated round) overlap on the device.  job(i, Job&) fills the i-th job.
template <class GetJob>
int run_jobs(zkfl_ctx* ctx, size_t n, GetJob job) {
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  struct PerKey {
    zkfl_key* key;
    size_t issued = 0;  // proofs issued in this batch
  };
  std::vector<PerKey> cursor;
  auto issue = [&](PerKey& pk, size_t i, const Job& J, const uint32_t* rsl) -> int {
    ProofSlot* s = nullptr;
    int rc = get_slot(J.key, pk.issued++, &s);
    if (rc) return rc;
    if (s->busy) {
      rc = wait_slot(s, n > 1);
      if (rc) return rc;
    }
    s->job = i;
    s->out_proof = J.part_out ? nullptr : J.proof_out;
    s->out_part = J.part_out;
    if (J.w_ready) {
      hipError_t e = hipStreamWaitEvent(s->st_main, J.w_ready, 0);
      if (e != hipSuccess) return hip_fail(e, "wait for the witness group");
    }
    rc = enqueue_proof(ctx, J.key, s, J.w, rsl, J.part_out ? ProofMode::SplitPart : ProofMode::Proof, n == 1);
    if (rc) return rc;
    s->busy = true;
    return ZKFL_OK;
  };
  int rc = ZKFL_OK;
  for (size_t i = 0; i < n && rc == ZKFL_OK; i++) {
    Job J;
    rc = job(i, J);
    if (rc) break;
    if (J.key->nshards != 1 && !J.part_out) {  // its MSMs are one shard's share: no whole proof
      rc = fail(ZKFL_E_ARG, "this key is shard " + std::to_string(J.key->shard) + " of " +
                                std::to_string(J.key->nshards) +
                                " of a split proof: prove parts (zkfl_groth16_prove_part_batch) and assemble them");
      break;
    }
    uint32_t rsl[16];
    rc = get_rs(J.rs, rsl);
    if (rc) break;
    size_t c = 0;
    while (c < cursor.size() && cursor[c].key != J.key) c++;
    if (c == cursor.size()) {
      cursor.emplace_back();
      cursor.back().key = J.key;
      rc = learn_for_batch(ctx, J, n);  // before the call enqueues anything on this key
      if (rc) break;
    }
    rc = issue(cursor[c], i, J, rsl);
  }
  for (auto& pk : cursor) {
    for (ProofSlot* s : pk.key->slots)
      if (s->busy) {
        int r2 = wait_slot(s, n > 1);
        if (rc == ZKFL_OK) rc = r2;
      }
  }
  return rc;
}

}  // namespace

extern "C" {

int zkfl_groth16_prove_resident(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w, const uint8_t* rs,
                                uint8_t proof_out[256]) {
  return zkfl_groth16_prove_batch(ctx, key, 1, &w, rs, proof_out);
}

int zkfl_key_set_slots(zkfl_key* key, int slots) {
  if (!key || slots < 1 || slots > 32) return fail(ZKFL_E_ARG, "slots must be in 1..32");
  (void)hipSetDevice(key->ctx->device);
  for (ProofSlot* s : key->slots) {
    if (s->busy) return fail(ZKFL_E_ARG, "slots busy");
  }
  while ((int)key->slots.size() > slots) {
    slot_release(key->slots.back());
    key->slots.pop_back();
  }
  // a slot's latency-schedule streams (made by a batch of one) hold HW queues: with many slots
  // they would push the slots' own streams past the ~24 HW queues and make slots share them
  // (a latency pass on a one-slot key before a 20-slot run: 395 vs 415 proofs/s)
  if (slots > 1)
    for (ProofSlot* s : key->slots) slot_drop_lowlat(s);
  key->max_slots = slots;
  return ZKFL_OK;
}

int zkfl_groth16_prove_batch(zkfl_ctx* ctx, zkfl_key* key, size_t n, const zkfl_witness* const* w,
                             const uint8_t* rs, uint8_t* proofs_out) {
  if (!ctx || !key || (!w && n) || (!proofs_out && n)) return fail(ZKFL_E_ARG, "null argument");
  for (size_t i = 0; i < n; i++) {
    if (!w[i] || w[i]->key != key) return fail(ZKFL_E_MISMATCH, "witness uploaded for another key");
  }
  return run_jobs(ctx, n, [&](size_t i, Job& J) {
    J.key = key;
    J.w = w[i]->d;
    J.rs = rs ? rs + 64 * i : nullptr;
    J.proof_out = proofs_out + 256 * i;
    return ZKFL_OK;
  });
}

int zkfl_groth16_prove_part_batch(zkfl_ctx* ctx, zkfl_key* key, size_t n, const zkfl_witness* const* w,
                                  const uint8_t* rs, uint8_t* parts_out) {
  if (!ctx || !key || (n && (!w || !rs || !parts_out))) return fail(ZKFL_E_ARG, "prove_part: null argument");
  for (size_t i = 0; i < n; i++) {
    if (!w[i] || w[i]->key != key) return fail(ZKFL_E_MISMATCH, "witness uploaded for another key");
  }
  return run_jobs(ctx, n, [&](size_t i, Job& J) {
    J.key = key;
    J.w = w[i]->d;
    J.rs = rs + 64 * i;
    J.part_out = parts_out + PART_WORDS * 4 * i;
    return ZKFL_OK;
  });
}

int zkfl_groth16_assemble(zkfl_ctx* ctx, size_t n, size_t n_parts, const uint8_t* parts, const uint8_t* rs,
                          uint8_t* proofs_out) {
  if (!ctx || (n && (!parts || !rs || !proofs_out)) || n_parts < 1 || n_parts > 1024)
    return fail(ZKFL_E_ARG, "assemble: bad arguments");
  if (n == 0) return ZKFL_OK;
  // every coordinate canonical (< q): the parts cross a process boundary
  for (size_t i = 0; i < n * n_parts * (PART_WORDS / 8); i++)
    if (!fq_lt_q(reinterpret_cast<const uint32_t*>(parts + 32 * i)))
      return fail(ZKFL_E_ARG, "assemble: part coordinate " + std::to_string(i) + " is not < q");
  std::vector<uint8_t> ks(n * 4 * sizeof(GlvScalar));
  for (size_t i = 0; i < n; i++) {
    uint32_t rsl[16];
    int rc = get_rs(rs + 64 * i, rsl);
    if (rc) return rc;
    GlvScalar* k = reinterpret_cast<GlvScalar*>(ks.data()) + 4 * i;
    glv_split(rsl + 8, k[0], k[1]);  // s -> pi_A's multiplier
    glv_split(rsl, k[2], k[3]);      // r -> B1's multiplier
  }
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  // one device buffer, carved: parts | res (5 G1P per proof) | resB2 | GLV halves | proofs | bad flag
  auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
  const size_t o_res = up(n * n_parts * PART_WORDS * 4), o_b2 = o_res + up(n * 5 * sizeof(G1P)),
               o_ks = o_b2 + up(n * sizeof(G2P)), o_pf = o_ks + up(ks.size()), o_bad = o_pf + up(n * 256),
               total = o_bad + 4;
  if (total > ctx->asm_cap) {
    if (ctx->asm_buf) (void)hipFree(ctx->asm_buf);
    ctx->asm_buf = nullptr;
    ctx->asm_cap = 0;
    HIP_TRY(hipMalloc(&ctx->asm_buf, total), "assemble buffers");
    ctx->asm_cap = total;
  }
  uint8_t* base = static_cast<uint8_t*>(ctx->asm_buf);
  void *d_parts = base, *d_res = base + o_res, *d_b2 = base + o_b2, *d_ks = base + o_ks, *d_proof = base + o_pf;
  uint32_t* d_bad = reinterpret_cast<uint32_t*>(base + o_bad);
  uint32_t bad = 0;
  hipError_t e = hipMemcpyAsync(d_parts, parts, n * n_parts * PART_WORDS * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(d_ks, ks.data(), ks.size(), hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 4, st);
  if (e == hipSuccess) {
    parts_sum(st, (uint32_t)n, (const uint32_t*)d_parts, (int)n_parts, (G1P*)d_res, (G2P*)d_b2, d_bad);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "assemble");
  if (bad) return fail(ZKFL_E_ARG, "assemble: a part holds a point that is not on its curve");
  assemble(st, (uint32_t)n, (const G1P*)d_res, (const G2P*)d_b2, (const GlvScalar*)d_ks, (uint32_t*)d_proof);
  e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(proofs_out, d_proof, n * 256, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "assemble");
  return ZKFL_OK;
}

int zkfl_groth16_prove_multi(zkfl_ctx* ctx, size_t n, zkfl_key* const* keys, const zkfl_witness* const* w,
                             const uint8_t* rs, uint8_t* proofs_out) {
  if (!ctx || (n && (!keys || !w || !proofs_out))) return fail(ZKFL_E_ARG, "prove_multi: null argument");
  for (size_t i = 0; i < n; i++) {
    if (!keys[i] || keys[i]->ctx != ctx) return fail(ZKFL_E_ARG, "prove_multi: key of another context");
    if (!w[i] || w[i]->key != keys[i]) return fail(ZKFL_E_MISMATCH, "prove_multi: witness uploaded for another key");
  }
  return run_jobs(ctx, n, [&](size_t i, Job& J) {
    J.key = keys[i];
    J.w = w[i]->d;
    J.rs = rs ? rs + 64 * i : nullptr;
    J.proof_out = proofs_out + 256 * i;
    return ZKFL_OK;
  });
}

static int full_prove_check(const zkfl_ctx* ctx, const zkfl_key* key, const zkfl_wprog* prog, size_t n,
                            const uint8_t* inputs, size_t* n_in) {
  if (!key || !prog || (n && !inputs)) return fail(ZKFL_E_ARG, "full_prove: null argument");
  if (key->ctx != ctx || prog->ctx != ctx) return fail(ZKFL_E_ARG, "full_prove: key/program of another context");
  uint32_t nw = 0, n_in32 = 0, npub = 0;
  wprog_info(prog->p, &nw, &n_in32, &npub);
  if (nw != key->nVars || npub != key->nPub)
    return fail(ZKFL_E_MISMATCH, "witness program does not match the proving key (nVars / nPublic)");
  *n_in = n_in32;
  std::string err;
  if (!wprog_inputs_ok(prog->p, n, inputs, err)) return fail(ZKFL_E_ARG, err);
  return ZKFL_OK;
}

// Full prove through the keys' witness pipes: for each key, groups of G = its slots witnesses one
// group ahead of its slots (WitPipe); a proof waits on its group's event.  Job i uses key_of(i),
// program prog_of(i) (nVars / inputs of that key), get_input(i, &ptr) yields its input vector
// (n_in x 32 B std form, < r; called in increasing i per key), pub_of(i) its public-signal
// destination (nullable).
extern "C++" {
template <class KeyOf, class ProgOf, class GetInput, class PubOf>
int full_prove_piped(zkfl_ctx* ctx, size_t n, KeyOf key_of, ProgOf prog_of, GetInput get_input, const uint8_t* rs,
                     uint8_t* proofs_out, PubOf pub_of) {
  if (n == 0) return ZKFL_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  struct PerKey {
    zkfl_key* key;
    const WProg* prog;
    size_t G = 0, n_in = 0, groups = 0;
    WitPipe* pipe = nullptr;
    std::vector<size_t> jobs;  // global indices, in order
  };
  std::vector<PerKey> ks;
  std::vector<size_t> kidx(n), local(n), off(n + 1, 0);
  for (size_t i = 0; i < n; i++) {
    zkfl_key* k = key_of(i);
    size_t c = 0;
    while (c < ks.size() && ks[c].key != k) c++;
    if (c == ks.size()) {
      PerKey pk;
      pk.key = k;
      pk.prog = prog_of(i);
      uint32_t nw = 0, nin = 0, np = 0;
      wprog_info(pk.prog, &nw, &nin, &np);
      pk.n_in = nin;
      // one group = the proofs a key holds in flight: the witness sets' reuse (enqueue_group)
      // relies on a group being no smaller
      pk.G = (size_t)k->max_slots;
      ks.push_back(pk);
    }
    kidx[i] = c;
    local[i] = ks[c].jobs.size();
    ks[c].jobs.push_back(i);
    off[i + 1] = off[i] + 4 + (size_t)k->nPub * 32;  // pinned record: fail flag | public signals
  }
  for (auto& pk : ks) {
    pk.groups = (pk.jobs.size() + pk.G - 1) / pk.G;
    HIP_TRY(wpipe_get(pk.key, pk.G, pk.key->nVars, pk.n_in, &pk.pipe), "witness pipe allocation");
  }
  uint8_t* pin_out = nullptr;
  HIP_TRY(hipHostMalloc(&pin_out, off[n] + 16), "pinned witness outputs");
  // groups enqueued ahead of the one the slots start (1..WIT_SETS - 2): a group is computed
  // while the slots run the `ahead` groups before it
  constexpr size_t ahead = 2;
  static_assert(ahead >= 1 && ahead <= WIT_SETS - 2, "a witness set is reused WIT_SETS groups later");
  auto enqueue_group = [&](PerKey& pk, size_t g) -> int {
    WitPipe* P = pk.pipe;
    WitPipe::Set& b = P->set[g % WIT_SETS];
    const size_t l0 = g * pk.G, m = std::min(pk.G, pk.jobs.size() - l0), nw = pk.key->nVars;
    const size_t npub = pk.key->nPub;
    HIP_TRY(host_wait(b.ev, true), "witness set reuse");  // its group of WIT_SETS groups ago
    for (size_t j = 0; j < m; j++) {
      const uint8_t* in = nullptr;
      int r = get_input(pk.jobs[l0 + j], &in);
      if (r) return r;
      memcpy(b.pin_in + j * pk.n_in * 32, in, pk.n_in * 32);
    }
    if (pk.n_in)
      HIP_TRY(hipMemcpyAsync(b.in, b.pin_in, m * pk.n_in * 32, hipMemcpyHostToDevice, P->st), "upload inputs");
    HIP_TRY(wprog_enqueue(pk.prog, m, b.in, b.W, b.outs, b.fail, P->st), "witness group");
    for (size_t j = 0; j < m; j++) {
      uint8_t* o = pin_out + off[pk.jobs[l0 + j]];
      HIP_TRY(hipMemcpyAsync(o, b.fail + j, 4, hipMemcpyDeviceToHost, P->st), "witness status");
      if (npub) HIP_TRY(hipMemcpyAsync(o + 4, b.d + j * nw + 1, npub * 32, hipMemcpyDeviceToHost, P->st), "publics");
    }
    HIP_TRY(hipEventRecord(b.ev, P->st), "event");
    return ZKFL_OK;
  };
  int rc = ZKFL_OK;
  for (auto& pk : ks)
    for (size_t g = 0; g <= ahead && g < pk.groups && rc == ZKFL_OK; g++) rc = enqueue_group(pk, g);
  if (rc == ZKFL_OK)
    rc = run_jobs(ctx, n, [&](size_t i, Job& J) {
      PerKey& pk = ks[kidx[i]];
      const size_t g = local[i] / pk.G, j = local[i] % pk.G;
      // the key's slots hold its group g - 1 now and have drained group g - 2, whose set (mod
      // WIT_SETS) group g + ahead takes (ahead <= WIT_SETS - 2)
      if (j == 0 && g >= 1 && g + ahead < pk.groups) {
        int r = enqueue_group(pk, g + ahead);
        if (r) return r;
      }
      J.key = pk.key;
      J.w = pk.pipe->set[g % WIT_SETS].d + j * pk.key->nVars;
      J.w_ready = pk.pipe->set[g % WIT_SETS].ev;
      J.rs = rs ? rs + 64 * i : nullptr;
      J.proof_out = proofs_out + 256 * i;
      return ZKFL_OK;
    });
  for (auto& pk : ks) {
    const hipError_t e = hipStreamSynchronize(pk.pipe->st);
    if (rc == ZKFL_OK && e != hipSuccess) rc = hip_fail(e, "witness pipe");
  }
  size_t bad = SIZE_MAX;
  uint32_t bad_assert = 0;
  for (size_t i = 0; rc == ZKFL_OK && i < n; i++) {
    uint32_t f;
    memcpy(&f, pin_out + off[i], 4);
    if (f != 0xFFFFFFFFu) {  // unsatisfied witness: its proof bytes are zeroed
      memset(proofs_out + 256 * i, 0, 256);
      if (bad == SIZE_MAX) {
        bad = i;
        bad_assert = f;
      }
    }
    uint8_t* pub = pub_of(i);
    if (pub) memcpy(pub, pin_out + off[i] + 4, off[i + 1] - off[i] - 4);
  }
  (void)hipHostFree(pin_out);
  if (rc == ZKFL_OK && bad != SIZE_MAX)
    rc = fail(ZKFL_E_CONSTRAINT, "witness " + std::to_string(bad) + ": assert constraint #" +
                                     std::to_string(bad_assert) + " failed (inputs do not satisfy the circuit)");
  return rc;
}
}  // extern "C++"

int zkfl_groth16_full_prove_batch(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, size_t n,
                                  const uint8_t* inputs, const uint8_t* rs, uint8_t* proofs_out, uint8_t* pubs_out) {
  if (!ctx || (n && !proofs_out)) return fail(ZKFL_E_ARG, "full_prove: null argument");
  size_t n_in = 0;
  int rc = full_prove_check(ctx, key, prog, n, inputs, &n_in);
  if (rc) return rc;
  return full_prove_piped(
      ctx, n, [&](size_t) { return key; }, [&](size_t) { return (const WProg*)prog->p; },
      [&](size_t i, const uint8_t** in) {
        *in = inputs + i * n_in * 32;
        return ZKFL_OK;
      },
      rs, proofs_out, [&](size_t i) { return pubs_out ? pubs_out + (size_t)key->nPub * 32 * i : nullptr; });
}

int zkfl_groth16_full_prove_json(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, const char* input_json,
                                 const uint8_t* rs, uint8_t proof_out[256], uint8_t* pub_out) {
  if (!ctx || !key || !prog || !input_json || !proof_out) return fail(ZKFL_E_ARG, "full_prove_json: null argument");
  std::vector<uint32_t> v;
  std::string err;
  int rc = wprog_inputs_json(prog->p, input_json, v, err);  // the loaded program's signal table
  if (rc) return fail(rc, err);
  v.resize(v.size() + 8);  // never empty (a circuit without inputs still proves one witness)
  return zkfl_groth16_full_prove_batch(ctx, key, prog, 1, reinterpret_cast<const uint8_t*>(v.data()), rs, proof_out,
                                       pub_out);
}

// input.json texts -> input vectors on host worker threads, ahead of the slot scheduler that
// consumes them (at most AHEAD parsed vectors held), so parsing overlaps the proofs in flight.
namespace {
struct JsonParsePool {
  static constexpr size_t AHEAD = 64;
  const WProg* prog;
  const char* const* texts;
  size_t n, n_in;
  std::vector<std::vector<uint32_t>> vec;
  std::vector<std::string> err;
  std::vector<int> rc;
  std::vector<uint8_t> done;
  std::atomic<size_t> next{0};
  size_t consumed = 0;
  bool stop = false;
  std::mutex mu;
  std::condition_variable cv;
  std::vector<std::thread> th;

  JsonParsePool(const WProg* p, const char* const* t, size_t count, size_t nin)
      : prog(p), texts(t), n(count), n_in(nin), vec(count), err(count), rc(count, 0), done(count, 0) {
    const unsigned hw = std::max(2u, std::thread::hardware_concurrency());
    const size_t workers = std::min<size_t>({count, (size_t)hw / 2, 8});
    for (size_t w = 0; w < workers; w++) th.emplace_back([this] { work(); });
  }
  ~JsonParsePool() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : th) t.join();
  }
  void work() {
    for (;;) {
      const size_t i = next.fetch_add(1);
      if (i >= n) return;
      {
        std::unique_lock<std::mutex> g(mu);
        cv.wait(g, [&] { return stop || i < consumed + AHEAD; });
        if (stop) return;
      }
      std::vector<uint32_t> v;
      std::string e;
      int r = texts[i] ? wprog_inputs_json(prog, texts[i], v, e) : ZKFL_E_ARG;
      if (!texts[i]) e = "null input json";
      if (r == ZKFL_OK && v.size() != n_in * 8) {
        r = ZKFL_E_ARG;
        e = "input json does not fill the program's inputs";
      }
      v.resize(n_in * 8 + 8);  // never empty
      {
        std::lock_guard<std::mutex> g(mu);
        vec[i] = std::move(v);
        err[i] = std::move(e);
        rc[i] = r;
        done[i] = 1;
      }
      cv.notify_all();
    }
  }
  // Job i's vector (blocks until parsed); job i-1's vector is released (its slot copied it).
  int get(size_t i, const uint8_t** out) {
    std::unique_lock<std::mutex> g(mu);
    if (i > 0) std::vector<uint32_t>().swap(vec[i - 1]);
    consumed = i;
    cv.notify_all();
    cv.wait(g, [&] { return done[i] != 0; });
    if (rc[i]) return fail(rc[i], "input " + std::to_string(i) + ": " + err[i]);
    *out = reinterpret_cast<const uint8_t*>(vec[i].data());
    return ZKFL_OK;
  }
};
}  // namespace

int zkfl_groth16_full_prove_json_batch(zkfl_ctx* ctx, zkfl_key* key, const zkfl_wprog* prog, size_t n,
                                       const char* const* input_jsons, const uint8_t* rs, uint8_t* proofs_out,
                                       uint8_t* pubs_out) {
  if (!ctx || (n && (!input_jsons || !proofs_out))) return fail(ZKFL_E_ARG, "full_prove_json_batch: null argument");
  size_t n_in = 0;
  int rc = full_prove_check(ctx, key, prog, 0, nullptr, &n_in);
  if (rc || n == 0) return rc;
  JsonParsePool pool(prog->p, input_jsons, n, n_in);
  // parsed values are < r by construction
  return full_prove_piped(
      ctx, n, [&](size_t) { return key; }, [&](size_t) { return (const WProg*)prog->p; },
      [&](size_t i, const uint8_t** in) { return pool.get(i, in); }, rs, proofs_out,
      [&](size_t i) { return pubs_out ? pubs_out + (size_t)key->nPub * 32 * i : nullptr; });
}

int zkfl_groth16_full_prove_multi(zkfl_ctx* ctx, size_t n, zkfl_key* const* keys, const zkfl_wprog* const* progs,
                                  const uint8_t* const* inputs, const uint8_t* rs, uint8_t* proofs_out,
                                  uint8_t* const* pubs_out) {
  if (!ctx || (n && (!keys || !progs || !inputs || !proofs_out))) return fail(ZKFL_E_ARG, "full_prove_multi: null argument");
  std::vector<size_t> n_in(n);
  for (size_t i = 0; i < n; i++) {
    int rc = full_prove_check(ctx, keys[i], progs[i], 1, inputs[i], &n_in[i]);
    if (rc) return fail(rc, "job " + std::to_string(i) + ": " + zkfl_last_error());
  }
  std::vector<std::pair<const zkfl_key*, const zkfl_wprog*>> kp;  // a key's jobs share its witness program
  for (size_t i = 0; i < n; i++) {
    size_t c = 0;
    while (c < kp.size() && kp[c].first != keys[i]) c++;
    if (c == kp.size()) kp.push_back({keys[i], progs[i]});
    else if (kp[c].second != progs[i])
      return fail(ZKFL_E_ARG, "full_prove_multi: job " + std::to_string(i) +
                                  " uses its key with another witness program than an earlier job");
  }
  return full_prove_piped(
      ctx, n, [&](size_t i) { return keys[i]; }, [&](size_t i) { return (const WProg*)progs[i]->p; },
      [&](size_t i, const uint8_t** in) {
        *in = inputs[i];
        return ZKFL_OK;
      },
      rs, proofs_out, [&](size_t i) { return pubs_out ? pubs_out[i] : nullptr; });
}

int zkfl_groth16_prove(zkfl_ctx* ctx, zkfl_key* key, const uint8_t* wtns, size_t wtns_len, const uint8_t* rs,
                       uint8_t proof_out[256], uint8_t* pub_out, size_t* npub) {
  zkfl_witness* w = nullptr;
  int rc = zkfl_witness_upload(ctx, key, wtns, wtns_len, &w);
  if (rc) return rc;
  rc = zkfl_groth16_prove_resident(ctx, key, w, rs, proof_out);
  if (rc == ZKFL_OK) {
    if (pub_out) memcpy(pub_out, w->pub.data(), w->pub.size());
    if (npub) *npub = key->nPub;
  }
  zkfl_witness_free(w);
  return rc;
}

int zkfl_debug_prove_parts(zkfl_ctx* ctx, zkfl_key* key, const uint8_t* wtns, size_t wtns_len, uint8_t* h_out,
                           uint8_t* msm_out) {
  zkfl_witness* w = nullptr;
  int rc = zkfl_witness_upload(ctx, key, wtns, wtns_len, &w);
  if (rc) return rc;
  ProofSlot* s = nullptr;
  rc = get_slot(key, 0, &s);
  uint32_t zeros[16] = {0};
  if (rc == ZKFL_OK && !key->dbg_zero) {  // see zkfl_key::dbg_zero
    const size_t bytes = std::max<size_t>(key->nVars, (size_t)key->n + 4) * 32;
    hipError_t e = hipMalloc(&key->dbg_zero, bytes);
    // on the slot's stream and waited for: hipMemset is asynchronous to the host and runs on the
    // null stream, which the slots' non-blocking streams do not wait for -- the MSMs below read
    // the zeros, and a recycled allocation (a freed key's memory) is not zero.  (Found as a
    // parity failure that appeared only after earlier tests had freed large keys.)
    if (e == hipSuccess) e = hipMemsetAsync(key->dbg_zero, 0, bytes, s->st_main);
    if (e == hipSuccess) e = hipStreamSynchronize(s->st_main);
    if (e != hipSuccess) rc = hip_fail(e, "parity hook zeros");
  }
  if (rc == ZKFL_OK && s->busy) rc = wait_slot(s);
  if (rc == ZKFL_OK) {
    s->out_proof = nullptr;
    s->out_part = nullptr;
    rc = enqueue_proof(ctx, key, s, w->d, zeros, ProofMode::Parts, false);
  }
  if (rc == ZKFL_OK) rc = wait_slot(s);
  hipStream_t st = s ? s->st_main : ctx->st;
  uint32_t* d_o = nullptr;
  if (rc == ZKFL_OK && msm_out) {
    hipError_t e = hipMalloc(&d_o, 64 * 4 + 128);
    if (e == hipSuccess) {
      point_out(st, s->res, 4, d_o);
      point_out(st, s->resB2, 1, d_o + 64);
      e = hipGetLastError();
    }
    std::vector<uint8_t> tmp(64 * 4 + 128);
    if (e == hipSuccess) e = hipMemcpyAsync(tmp.data(), d_o, tmp.size(), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, "debug parts");
    if (rc == ZKFL_OK) {
      // res order A, B1, C, H ; output order A | B1 | B2 | C | H
      memcpy(msm_out, tmp.data(), 64);
      memcpy(msm_out + 64, tmp.data() + 64, 64);
      memcpy(msm_out + 128, tmp.data() + 256, 128);
      memcpy(msm_out + 256, tmp.data() + 128, 64);
      memcpy(msm_out + 320, tmp.data() + 192, 64);
    }
  }
  if (rc == ZKFL_OK && h_out) {
    hipError_t e = hipMemcpyAsync(h_out, s->h, (size_t)key->n * 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) rc = hip_fail(e, "debug h");
  }
  if (d_o) (void)hipFree(d_o);
  zkfl_witness_free(w);
  return rc;
}

int zkfl_debug_abc(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w, int grouped, uint8_t* abc_out,
                   uint32_t* counts_out) {
  if (!ctx || !key || !w || !abc_out || !counts_out) return fail(ZKFL_E_ARG, "debug_abc: null argument");
  if (key->ctx != ctx) return fail(ZKFL_E_ARG, "debug_abc: key of another context");
  if (w->key != key) return fail(ZKFL_E_MISMATCH, "witness uploaded for another key");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  ProofSlot* s = nullptr;
  int rc = get_slot(key, 0, &s);
  if (rc) return rc;
  if (s->busy && (rc = wait_slot(s))) return rc;
  // the slot's buffers and the proof's own steps up to ABC: start (which empties the state),
  // the differences with their marks, the ABC stage of the plan
  ProofPlan p = {};
  p.mode = ProofMode::Proof;
  p.grouped = grouped && key->grp.on;
  p.group_rows = p.grouped && key->grp.rows_on && s->gr_state;
  p.share_b_sort = key->share_b;
  if (p.group_rows && s->cls_cap < key->grp.row_classes) {
    if (s->cls_val) (void)hipFree(s->cls_val);
    s->cls_val = nullptr;
    s->cls_cap = 0;
    HIP_TRY(hipMalloc(&s->cls_val, (size_t)key->grp.row_classes * 32), "class values");
    s->cls_cap = key->grp.row_classes;
  }
  memset(s->pinned + 256, 0, 64 + 4 * sizeof(GlvScalar));
  memset(s->pinned + MISS_OFF, 0, 12);
  hipStream_t st = s->st_main;
  start(key, s, p);
  if (p.grouped)
    group_delta(st, w->d, key->grp.d_rep, key->nVars, s->extra + 4, s->grp_cnt,
                reinterpret_cast<uint32_t*>(s->pinned + MISS_OFF), group_mark(key, s, p));
  if (p.group_rows) group_mark_rows(st, group_mark(key, s, p));
  abc_stage(key, s, w->d, st, p);
  const size_t n3 = 3 * (size_t)key->n;
  fr_mont_to_std(st, s->abc, n3);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(abc_out, s->abc, n3 * 32, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  if (e != hipSuccess) return hip_fail(e, "debug abc");
  memcpy(counts_out, s->pinned + MISS_OFF, 12);
  if (!p.group_rows) counts_out[1] = counts_out[2] = 0;
  return ZKFL_OK;
}

int zkfl_debug_msm_front(zkfl_ctx* ctx, uint32_t n1, const size_t* n, const uint8_t* const* bases,
                         const uint8_t* const* scalars, const size_t* n_scalars, const uint32_t* const* sidx,
                         const uint32_t* extra_start, const uint8_t* const* extra, const size_t* n_extra, uint32_t b,
                         const uint8_t* bases_g2, size_t n_b, int fast, int joint, uint8_t* out_g1, uint8_t out_g2[128]) {
  constexpr size_t CAP = (size_t)1 << 17;
  if (!ctx || !n || !bases || !scalars || !n_scalars || !out_g1 || !out_g2)
    return fail(ZKFL_E_ARG, "msm front: null argument");
  if (n1 < 1 || n1 > (uint32_t)MSM_TAIL_MAX || b >= n1 || (fast != 0 && fast != 1) || (joint != 0 && joint != 1))
    return fail(ZKFL_E_ARG, "msm front: 1..4 G1 sets, b one of them, fast and joint 0 or 1");
  // B2 accumulates from set b's sorted pairs, which index set b's bases: one G2 base per G1 base
  if (n_b != n[b] || (n_b && !bases_g2)) return fail(ZKFL_E_ARG, "msm front: the G2 set needs one base per base of set b");
  size_t most = 0;
  for (uint32_t i = 0; i < n1; i++) {
    const std::string set = "msm front: set " + std::to_string(i);
    const bool mapped = sidx && sidx[i];
    const size_t ne = mapped && n_extra ? n_extra[i] : 0;
    if (n[i] > CAP || n_scalars[i] > CAP || ne > CAP) return fail(ZKFL_E_ARG, set + ": more than 2^17 entries");
    if ((n[i] && !bases[i]) || (n_scalars[i] && !scalars[i])) return fail(ZKFL_E_ARG, set + ": null argument");
    if (mapped && (!extra_start || (ne && (!extra || !extra[i])))) return fail(ZKFL_E_ARG, set + ": null argument");
    if (int rc = check_fr(scalars[i], n_scalars[i], set + ": scalar")) return rc;
    if (ne)
      if (int rc = check_fr(extra[i], ne, set + ": extra scalar")) return rc;
    // every scalar a base reads lies inside one of the two vectors (msm_sort.hip msm_for_digits)
    if (!mapped && n_scalars[i] < n[i]) return fail(ZKFL_E_ARG, set + ": fewer scalars than bases");
    for (size_t j = 0; mapped && j < n[i]; j++) {
      const uint32_t si = sidx[i][j];
      if (si < extra_start[i] ? si >= n_scalars[i] : (size_t)(si - extra_start[i]) >= ne)
        return fail(ZKFL_E_ARG, set + ": sidx " + std::to_string(j) + " is out of range");
    }
    most = std::max(most, n[i]);
  }
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  struct Engine {  // released on every exit path
    MsmBases<FqOps> mb[MSM_TAIL_MAX];
    MsmScratch<FqOps> ms[MSM_TAIL_MAX];
    MsmTail<FqOps> mt[MSM_TAIL_MAX];
    MsmBases<Fq2Ops> mb2;
    MsmTail<Fq2Ops> mt2;
    ~Engine() {
      for (auto& x : mb) msm_bases_free(x);
      for (auto& x : ms) msm_scratch_free(x);
      for (auto& x : mt) msm_tail_free(x);
      msm_bases_free(mb2);
      msm_tail_free(mt2);
    }
  } E;
  DevBufs D;
  const char* const where = "msm front";
  const int c = msm_pick_c(most);  // as key load: one width for every set of the key
  FrontMsm m;
  m.n1 = (int)n1;
  G1P* d_r;
  G2P* d_r2;
  uint32_t* d_o;
  HIP_TRY(D.get(&d_r, n1), where);
  HIP_TRY(D.get(&d_r2, 1), where);
  HIP_TRY(D.get(&d_o, n1 * 16 + 32), where);
  for (uint32_t i = 0; i < n1; i++) {
    const bool mapped = sidx && sidx[i];
    const size_t ne = mapped && n_extra ? n_extra[i] : 0;
    G1Aff* d_b;
    uint32_t *d_s, *d_e;
    // scratch and tail by the set's own base count, as a slot's are
    HIP_TRY(msm_bases_alloc(E.mb[i], n[i], c), where);
    HIP_TRY(msm_scratch_alloc(E.ms[i], n[i], c, st), where);
    HIP_TRY(msm_tail_alloc(E.mt[i], n[i], c), where);
    HIP_TRY(D.get(&d_b, n[i]), where);
    HIP_TRY(D.get(&d_s, n_scalars[i] * 8), where);
    HIP_TRY(D.get(&d_e, ne * 8), where);
    if (n[i]) HIP_TRY(hipMemcpyAsync(d_b, bases[i], n[i] * sizeof(G1Aff), hipMemcpyHostToDevice, st), where);
    if (n_scalars[i]) HIP_TRY(hipMemcpyAsync(d_s, scalars[i], n_scalars[i] * 32, hipMemcpyHostToDevice, st), where);
    if (ne) HIP_TRY(hipMemcpyAsync(d_e, extra[i], ne * 32, hipMemcpyHostToDevice, st), where);
    HIP_TRY(msm_bases_set(E.mb[i], d_b, mapped ? sidx[i] : nullptr, mapped ? extra_start[i] : 0xFFFFFFFFu, st), where);
    m.bases[i] = &E.mb[i];
    m.scratch[i] = &E.ms[i];
    m.tails[i] = &E.mt[i];
    m.scalars[i] = d_s;
    m.extra[i] = d_e;
    m.outs[i] = d_r + i;
  }
  G2Aff* d_b2;
  HIP_TRY(msm_bases_alloc(E.mb2, n_b, c), where);
  HIP_TRY(msm_tail_alloc(E.mt2, n_b, c), where);  // its own nnz: the copy of b2_from_b1_sort runs
  HIP_TRY(D.get(&d_b2, n_b), where);
  if (n_b) HIP_TRY(hipMemcpyAsync(d_b2, bases_g2, n_b * sizeof(G2Aff), hipMemcpyHostToDevice, st), where);
  HIP_TRY(msm_bases_set(E.mb2, d_b2, nullptr, 0xFFFFFFFFu, st), where);
  m.ib = (int)b;
  m.b2 = &E.mb2;
  m.t2 = &E.mt2;
  m.nnz_alias = false;
  m.out2 = d_r2;
  // what k_proof_start does for a proof: every tail emptied
  MsmTail<Fq2Ops>* t2 = &E.mt2;
  HIP_TRY(msm_tails_reset(m.tails, m.n1, st), where);
  HIP_TRY(msm_tails_reset(&t2, 1, st), where);
  if (int rc = front_msm(m, st, fast != 0, joint != 0, &ctx->prof)) return rc;
  point_out(st, d_r, (int)n1, d_o);
  point_out(st, d_r2, 1, d_o + n1 * 16);
  HIP_TRY(hipGetLastError(), where);
  HIP_TRY(hipMemcpyAsync(out_g1, d_o, n1 * 64, hipMemcpyDeviceToHost, st), where);
  HIP_TRY(hipMemcpyAsync(out_g2, d_o + n1 * 16, 128, hipMemcpyDeviceToHost, st), where);
  HIP_TRY(hipStreamSynchronize(st), where);
  return ZKFL_OK;
}

}  // extern "C"
