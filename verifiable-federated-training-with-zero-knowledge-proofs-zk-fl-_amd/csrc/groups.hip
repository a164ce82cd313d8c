// The grouped form of a key's witness queries (csrc/groups.h): its two kernels -- the group sums
// behind the grouped base sets (once per partition) and the per-proof differences u -- and the
// key's entry points (set, learn, report).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <cstdio>
#include <vector>

#include "devbufs.h"
#include "groups.h"
#include "objects.h"

using namespace zkfl;

namespace {

// A base coordinate of the window table (the 29-bit engine's Montgomery domain, x 2^261) back to
// the loader's (x 2^256): fp_mul by 2^251 (< q, one bit)
ZK_DEV Fq from_m29(const Fq& a) {
  Fq c = fp_zero<FqP>();
  c.v[7] = 0x08000000u;
  return fp_mul(a, c);
}

template <class F>
ZK_DEV Affine<F> load_base(const Affine<F>* __restrict__ p) {
  Affine<F> a = *p;
  Fq* q = reinterpret_cast<Fq*>(&a);
#pragma unroll
  for (int k = 0; k < (int)(sizeof(Affine<F>) / sizeof(Fq)); k++) q[k] = from_m29(q[k]);
  return a;
}

// One lane per base slot: its own base, plus its members' with complete additions (equal bases and
// sums at infinity occur), back to affine with one inversion where there was anything to add.
template <class F>
__global__ void __launch_bounds__(64) k_group_sums(const Affine<F>* __restrict__ bases_w, int W, size_t n,
                                                   const uint32_t* __restrict__ start,
                                                   const uint32_t* __restrict__ members, Affine<F>* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Affine<F> p = load_base<F>(bases_w + j * W);
  const uint32_t b = start[j], e = start[j + 1];
  if (b == e) {
    out[j] = p;
    return;
  }
  XYZZ<F> acc = xyzz_from_affine<F>(p);
  for (uint32_t m = b; m < e; m++) acc = xyzz_madd<F>(acc, load_base<F>(bases_w + (size_t)members[m] * W));
  out[j] = xyzz_to_affine<F>(acc);
}

constexpr int DELTA_T = 256, DELTA_BLOCKS_MAX = 512;  // at most two blocks per CU of an MI355X

__global__ void __launch_bounds__(DELTA_T) k_group_delta(const Fr* __restrict__ w, const uint32_t* __restrict__ rep,
                                                         uint32_t n, Fr* __restrict__ u, uint32_t* __restrict__ cnt,
                                                         uint32_t* __restrict__ miss_out, const GroupMark M) {
  ZK_LIGHT();
  // grid-stride over whole blocks of wires (b0 is the same in every thread of the block, so its
  // waves enter and leave the loop together): a few hundred blocks end on the two counters below,
  // not one per 256 wires
  int blk = 0;
  for (uint32_t b0 = blockIdx.x * DELTA_T; b0 < n; b0 += gridDim.x * DELTA_T) {
    const uint32_t i = b0 + threadIdx.x;
    int nz = 0;
    if (i < n) {
      const uint32_t r = rep[i];
      Fr v = fp_zero<FrP>();
      if (r != i) {
        v = fp_sub(w[i], w[r]);
#pragma unroll
        for (int k = 0; k < 8; k++) nz |= v.v[k] != 0;
      }
      u[i] = v;
    }
    const unsigned long long m = __ballot(nz);
    if (m && M.wstart) {
      // grouped ABC: the missing wires go to the slot's list, one atomic per wave that has any;
      // k_group_mark walks their constraint lists (or raises the plain flag when there are too many)
      const uint32_t lane = threadIdx.x & (warpSize - 1);
      const int first = __ffsll((long long)m) - 1;
      uint32_t base = 0;
      if ((int)lane == first) base = atomicAdd(&M.state[2], (uint32_t)__popcll(m));
      base = __shfl(base, first);
      const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
      if (nz && at < M.miss_cap) M.missing[at] = i;
    }
    blk += nz;
  }
  // the block's misses: lane sums folded per wave, the waves' sums through LDS
  __shared__ int wave_nz[DELTA_T / 64];
  for (int off = warpSize / 2; off; off >>= 1) blk += __shfl_xor(blk, off);
  if ((threadIdx.x & (warpSize - 1)) == 0) wave_nz[threadIdx.x / warpSize] = blk;
  __syncthreads();
  if (threadIdx.x == 0) {
    blk = 0;
    for (int k = 0; k < DELTA_T / warpSize; k++) blk += wave_nz[k];
    // the last block to arrive publishes the total and leaves both counters zero for the next launch
    if (blk) atomicAdd(&cnt[0], (uint32_t)blk);
    __threadfence();
    if (atomicAdd(&cnt[1], 1u) == gridDim.x - 1) {
      __threadfence();
      miss_out[0] = atomicExch(&cnt[0], 0u);
      cnt[1] = 0;
    }
  }
}

constexpr int MARK_T = 256, MARK_BLOCKS_MAX = 256;

// One wave per missing wire and step, an entry of the wire's list per lane and round: a list of
// 180 constraints is three rounds of atomics.  Too many missing wires: the plain flag, and no walk.
__global__ void __launch_bounds__(MARK_T) k_group_mark(const GroupMark M) {
  ZK_LIGHT();
  const uint32_t n = M.state[2];
  if (n == 0) return;
  if (n > M.miss_cap) {
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicExch(&M.state[1], 1u);
    return;
  }
  const uint32_t lane = threadIdx.x & (warpSize - 1), per = MARK_T / warpSize;
  for (uint32_t k = blockIdx.x * per + threadIdx.x / warpSize; k < n; k += gridDim.x * per) {
    if (__any((int)__atomic_load_n(&M.state[1], __ATOMIC_RELAXED))) return;  // nothing reads the marks now
    const uint32_t i = M.missing[k], s = M.wstart[i], e = M.wstart[i + 1] & ~GROUP_ROWS_OVER;
    if (s & GROUP_ROWS_OVER) {
      if (lane == 0) atomicExch(&M.state[1], 1u);
      return;
    }
    for (uint32_t p = s + lane; p < e; p += warpSize) {
      const uint32_t j = M.wlist[p], bit = 1u << (j & 31);
      if (atomicOr(&M.state[GROUP_ROWS_STATE_BITS + (j >> 5)], bit) & bit) continue;
      const uint32_t at = atomicAdd(&M.state[0], 1u);
      if (at < M.cap) M.dirty[at] = j;
      else atomicExch(&M.state[1], 1u);
    }
  }
}

}  // namespace

namespace zkfl {

template <class F>
void group_sums(hipStream_t st, const Affine<F>* bases_w, int W, size_t n, const uint32_t* start,
                const uint32_t* members, Affine<F>* out) {
  if (n) hipLaunchKernelGGL(k_group_sums<F>, dim3(zk_grid(n, 64)), dim3(64), 0, st, bases_w, W, n, start, members, out);
}
template void group_sums<FqOps>(hipStream_t, const G1Aff*, int, size_t, const uint32_t*, const uint32_t*, G1Aff*);
template void group_sums<Fq2Ops>(hipStream_t, const G2Aff*, int, size_t, const uint32_t*, const uint32_t*, G2Aff*);

void group_delta(hipStream_t st, const Fr* w, const uint32_t* rep, uint32_t n, Fr* u, uint32_t* cnt,
                 uint32_t* miss_out, const GroupMark& mark) {
  const unsigned blocks = std::min<unsigned>(zk_grid(n, DELTA_T), DELTA_BLOCKS_MAX);
  hipLaunchKernelGGL(k_group_delta, dim3(blocks), dim3(DELTA_T), 0, st, w, rep, n, u, cnt, miss_out, mark);
}

void group_mark_rows(hipStream_t st, const GroupMark& mark) {
  const unsigned blocks = std::min<unsigned>(zk_grid((size_t)mark.miss_cap * 64, MARK_T), MARK_BLOCKS_MAX);
  hipLaunchKernelGGL(k_group_mark, dim3(blocks), dim3(MARK_T), 0, st, mark);
}

void key_groups_release(zkfl_key* k) {
  msm_bases_free(k->gA);
  msm_bases_free(k->gB1);
  msm_bases_free(k->gB2);
  msm_bases_free(k->gCH);
  void* ptrs[] = {k->grp.d_rep,    k->grp.d_cls,    k->grp.d_crp,  k->grp.d_cterms,
                  k->grp.d_ccoefs, k->grp.d_wstart, k->grp.d_wlist};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  const uint32_t builds = k->grp.builds;
  k->grp = KeyGroups();
  k->grp.builds = builds;
}

}  // namespace zkfl

namespace {

// One query's grouped base set from its plain one: member lists up, group sums, expansion.
template <class F>
hipError_t build_query(const MsmBases<F>& plain, MsmBases<F>& out, const GroupQuery& q, uint32_t extra_start,
                       DevBufs& D, hipStream_t st) {
  ZK_CHECK(msm_bases_alloc(out, plain.n, plain.c));
  if (plain.n == 0) return hipSuccess;
  uint32_t *d_start, *d_members;
  Affine<F>* d_img;
  ZK_CHECK(D.get(&d_start, q.start.size()));
  ZK_CHECK(D.get(&d_members, q.members.size()));
  ZK_CHECK(D.get(&d_img, plain.n));
  ZK_CHECK(hipMemcpyAsync(d_start, q.start.data(), q.start.size() * 4, hipMemcpyHostToDevice, st));
  if (!q.members.empty())
    ZK_CHECK(hipMemcpyAsync(d_members, q.members.data(), q.members.size() * 4, hipMemcpyHostToDevice, st));
  group_sums<F>(st, plain.bases_w, msm_w_of(plain.c), plain.n, d_start, d_members, d_img);
  ZK_CHECK(hipGetLastError());
  return msm_bases_set(out, d_img, q.sidx.data(), extra_start, st, false);
}

// keys that class their rows: the option on, terms to class, and not a small key (build_rows)
bool group_rows_wanted(const zkfl_key* k) {
  return k->ctx->opts.group_rows && k->K != 0 && k->logn > k->ctx->opts.small_logn;
}

// The key's row classes and wire lists (group_rows_build) under the refined partition rep.  The
// host image of the QAP is dropped after the load, so the build downloads it: 2 MB of row pointers
// and 28 MB of packed terms at the training circuit, a few ms once per partition, against holding
// those 30 MB of host memory per key for as long as the key lives.
hipError_t build_rows(zkfl_key* k, const std::vector<uint32_t>& rep, hipStream_t st) {
  KeyGroups& g = k->grp;
  // Small keys (domain <= 2^SchedOpts::small_logn) keep the plain ABC: their proofs are chains of
  // latency-bound launches, the ABC is a few microseconds of them, and the grouped form's three
  // more launches cost config 5 3.6 % (6.3 % weak) when they ran it (profiles/ab_group_rows.log).
  if (!group_rows_wanted(k)) return hipSuccess;
  const auto t0 = std::chrono::steady_clock::now();
  const uint32_t dom = k->n;
  const size_t K = k->K;
  std::vector<uint32_t> rows(2 * (size_t)dom + 1), cols(K), coefs;
  ZK_CHECK(hipMemcpyAsync(rows.data(), k->rows, rows.size() * 4, hipMemcpyDeviceToHost, st));
  ZK_CHECK(hipMemcpyAsync(cols.data(), k->cols, K * 4, hipMemcpyDeviceToHost, st));
  if (!k->cshift) {
    coefs.resize(K * 8);
    ZK_CHECK(hipMemcpyAsync(coefs.data(), k->coefs, K * 32, hipMemcpyDeviceToHost, st));
  }
  ZK_CHECK(hipStreamSynchronize(st));
  GroupRows R;
  const uint32_t low = (uint32_t)k->ctx->opts.group_rows_cap;
  group_rows_build(rows.data(), dom, cols.data(), k->cshift, coefs.data(), rep.data(), k->nVars, 64,
                   low ? std::min(low, GROUP_ROWS_WIRE_CAP) : GROUP_ROWS_WIRE_CAP, R);
  g.row_classes = R.classes;
  g.terms_rep = (uint32_t)R.cterms.size();
  g.wire_list = (uint32_t)R.wlist.size();
  g.over_cap = R.over_cap;
  if (R.keep && !R.cterms.empty()) {
    auto up = [&](auto*& dst, const std::vector<uint32_t>& v) -> hipError_t {
      ZK_CHECK(hipMalloc(&dst, (v.size() ? v.size() : 1) * 4));
      if (!v.empty()) ZK_CHECK(hipMemcpyAsync(dst, v.data(), v.size() * 4, hipMemcpyHostToDevice, st));
      return hipSuccess;
    };
    ZK_CHECK(up(g.d_cls, R.cls));
    ZK_CHECK(up(g.d_crp, R.crp));
    ZK_CHECK(up(g.d_cterms, R.cterms));
    if (!k->cshift) ZK_CHECK(up(g.d_ccoefs, R.ccoefs));
    ZK_CHECK(up(g.d_wstart, R.wstart));
    ZK_CHECK(up(g.d_wlist, R.wlist));
    ZK_CHECK(hipStreamSynchronize(st));
    g.rows_on = true;
  }
  g.rows_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return hipSuccess;
}

// rep: a valid partition of the key's wires (refined here); builds the grouped sets in place of
// any the key holds.
int key_build_groups(zkfl_key* k, std::vector<uint32_t>& rep, bool learned, double host_ms) {
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(k->ctx->device), "hipSetDevice");
  int rc = key_reset_graphs(k);
  if (rc) return rc;
  key_groups_release(k);
  const uint32_t nV = k->nVars, X = nV, dom = k->n;
  std::vector<uint8_t> sig(nV, 0);
  for (int qi = 0; qi < 4; qi++)
    for (uint32_t i : k->q_sidx[qi])
      if (i < nV) sig[i] |= (uint8_t)(1u << qi);
  groups_refine(rep.data(), sig.data(), nV);
  // u sits behind the four blinding scalars: extra = h + n for A, B1, B2, = h for C + H
  const uint32_t u_base[4] = {X + 4, X + 4, X + 4, X + dom + 4};
  GroupQuery q[4];
  for (int qi = 0; qi < 4; qi++)
    groups_query(rep.data(), nV, k->q_sidx[qi].data(), k->q_sidx[qi].size(), u_base[qi], q[qi]);
  hipStream_t st = k->ctx->st;
  hipError_t e;
  {
    DevBufs D;
    e = hipMalloc(&k->grp.d_rep, (size_t)(nV ? nV : 1) * 4);
    if (e == hipSuccess) e = hipMemcpyAsync(k->grp.d_rep, rep.data(), (size_t)nV * 4, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = build_query(k->bA, k->gA, q[0], X, D, st);
    if (e == hipSuccess) e = build_query(k->bB1, k->gB1, q[1], X, D, st);
    if (e == hipSuccess) e = build_query(k->bB2, k->gB2, q[2], X, D, st);
    if (e == hipSuccess) e = build_query(k->bCH, k->gCH, q[3], X, D, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (e == hipSuccess) e = build_rows(k, rep, st);
  }
  if (e != hipSuccess) {
    key_groups_release(k);
    return hip_fail(e, "grouped base sets");
  }
  KeyGroups& g = k->grp;
  g.on = true;
  g.learned = learned;
  for (uint32_t i = 0; i < nV; i++) g.non_rep += rep[i] != i;
  std::vector<uint8_t> has(nV, 0);
  for (uint32_t i = 0; i < nV; i++)
    if (rep[i] != i && !has[rep[i]]) {
      has[rep[i]] = 1;
      g.groups++;
    }
  for (int qi = 0; qi < 4; qi++) {
    g.bases[qi] = (uint32_t)k->q_sidx[qi].size();
    g.bases_rep[qi] = g.bases[qi] - q[qi].non_rep;
  }
  g.builds++;
  g.build_ms = host_ms + std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  fprintf(stderr,
          "zkfl: key of %u wires: %u groups, %u non-representative wires; bases A %u -> %u, B %u -> %u, C+H %u -> %u; "
          "%s and built in %.1f ms\n",
          nV, g.groups, g.non_rep, g.bases[0], g.bases_rep[0], g.bases[1], g.bases_rep[1], g.bases[3], g.bases_rep[3],
          learned ? "learned" : "set", g.build_ms);
  if (group_rows_wanted(k))
    fprintf(stderr,
            "zkfl: key of %u wires: %u row classes, terms %zu -> %u, wire lists %u entries (%u wires over the cap); "
            "%s ABC, built in %.1f ms of the above\n",
            nV, g.row_classes, k->K, g.terms_rep, g.wire_list, g.over_cap, g.rows_on ? "grouped" : "plain", g.rows_ms);
  return ZKFL_OK;
}

int groups_allowed(const zkfl_key* k) {
  if (k->nshards != 1) return fail(ZKFL_E_ARG, "groups: a sharded key keeps the plain form");
  if (!k->ctx->opts.groups) return fail(ZKFL_E_ARG, "groups: turned off on this context (ZKFL_GROUPS=0)");
  return ZKFL_OK;
}

}  // namespace

int zkfl::key_learn_groups(zkfl_ctx* ctx, zkfl_key* k, const Fr* d_w) {
  const auto t0 = std::chrono::steady_clock::now();
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<uint32_t> w((size_t)k->nVars * 8), rep;
  HIP_TRY(hipMemcpy(w.data(), d_w, w.size() * 4, hipMemcpyDeviceToHost), "download witness");
  groups_learn(w.data(), k->nVars, rep);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return key_build_groups(k, rep, true, ms);
}

extern "C" {

int zkfl_key_set_groups(zkfl_key* key, const uint32_t* rep, size_t n_vars) {
  if (!key) return fail(ZKFL_E_ARG, "null key");
  if (!rep) {
    HIP_TRY(hipSetDevice(key->ctx->device), "hipSetDevice");
    const int rc = key_reset_graphs(key);
    if (rc) return rc;
    key_groups_release(key);
    return ZKFL_OK;
  }
  int rc = groups_allowed(key);
  if (rc) return rc;
  if (n_vars != key->nVars) return fail(ZKFL_E_ARG, "groups: rep must hold one entry per wire of the key");
  if (!groups_valid(rep, n_vars)) return fail(ZKFL_E_ARG, "groups: rep[i] <= i and rep[rep[i]] == rep[i] must hold");
  std::vector<uint32_t> r(rep, rep + n_vars);
  return key_build_groups(key, r, false, 0.0);
}

int zkfl_key_learn_groups(zkfl_ctx* ctx, zkfl_key* key, const zkfl_witness* w) {
  if (!ctx || !key || !w) return fail(ZKFL_E_ARG, "null argument");
  if (key->ctx != ctx) return fail(ZKFL_E_ARG, "groups: key of another context");
  if (w->key != key) return fail(ZKFL_E_MISMATCH, "witness uploaded for another key");
  const int rc = groups_allowed(key);
  if (rc) return rc;
  return key_learn_groups(ctx, key, w->d);
}

int zkfl_key_groups(const zkfl_key* key, zkfl_groups_info* out) {
  if (!key || !out) return fail(ZKFL_E_ARG, "null argument");
  const KeyGroups& g = key->grp;
  *out = zkfl_groups_info();
  out->grouped = g.on;
  out->learned = g.learned;
  out->groups = g.groups;
  out->non_rep = g.non_rep;
  for (int i = 0; i < 4; i++) {
    out->bases[i] = g.on ? g.bases[i] : (uint32_t)key->q_sidx[i].size();
    out->bases_rep[i] = g.on ? g.bases_rep[i] : out->bases[i];
  }
  out->builds = g.builds;
  out->last_miss = g.last_miss;
  out->build_ms = g.build_ms;
  return ZKFL_OK;
}

int zkfl_key_group_rows(const zkfl_key* key, zkfl_group_rows_info* out) {
  if (!key || !out) return fail(ZKFL_E_ARG, "null argument");
  const KeyGroups& g = key->grp;
  *out = zkfl_group_rows_info();
  out->rows_grouped = g.rows_on;
  out->row_classes = g.row_classes;
  out->terms = (uint32_t)key->K;
  out->terms_rep = g.row_classes ? g.terms_rep : out->terms;
  out->wire_list = g.wire_list;
  out->wires_over_cap = g.over_cap;
  out->last_dirty = g.last_dirty;
  out->last_plain = g.last_plain;
  out->rows_build_ms = g.rows_ms;
  return ZKFL_OK;
}

int zkfl_debug_group_rows(const uint32_t* rows, uint32_t domain, const uint32_t* cols, uint32_t cshift,
                          const uint32_t* coefs, const uint32_t* rep, uint32_t n_vars, uint32_t hash_bits,
                          uint32_t wire_cap, uint32_t* cls_out, uint32_t* crp_out, uint32_t* cterms_out,
                          uint32_t* ccoefs_out, uint32_t* wstart_out, uint32_t* wlist_out, uint32_t* info_out) {
  if (!rows || !rep || !cls_out || !crp_out || !cterms_out || !wstart_out || !wlist_out || !info_out ||
      cshift >= 32 || domain > 0x3FFFFFFFu)
    return fail(ZKFL_E_ARG, "debug_group_rows: bad arguments");
  const uint32_t K = rows[2 * (size_t)domain];
  if (K && (!cols || (!cshift && !coefs))) return fail(ZKFL_E_ARG, "debug_group_rows: terms missing");
  for (uint32_t r = 0; r < 2 * domain; r++)
    if (rows[r] > rows[r + 1]) return fail(ZKFL_E_ARG, "debug_group_rows: row pointers must not descend");
  if (!groups_valid(rep, n_vars)) return fail(ZKFL_E_ARG, "debug_group_rows: not a partition");
  const uint32_t cmask = cshift ? (1u << cshift) - 1u : 0xFFFFFFFFu;
  for (uint32_t p = 0; p < K; p++)
    if ((cols[p] & cmask) >= n_vars) return fail(ZKFL_E_ARG, "debug_group_rows: column past the wires");
  GroupRows R;
  group_rows_build(rows, domain, cols, cshift, coefs, rep, n_vars, hash_bits, wire_cap ? wire_cap : GROUP_ROWS_WIRE_CAP,
                   R);
  auto put = [](uint32_t* dst, const std::vector<uint32_t>& v) {
    if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * 4);
  };
  put(cls_out, R.cls);
  put(crp_out, R.crp);
  put(cterms_out, R.cterms);
  put(ccoefs_out, R.ccoefs);
  put(wstart_out, R.wstart);
  put(wlist_out, R.wlist);
  info_out[0] = R.classes;
  info_out[1] = (uint32_t)R.cterms.size();
  info_out[2] = (uint32_t)R.wlist.size();
  info_out[3] = R.keep;
  return ZKFL_OK;
}

int zkfl_debug_groups(const uint8_t* values, const uint8_t* sig, size_t n, uint32_t* rep_out, const uint32_t* sidx,
                      size_t n_bases, uint32_t u_base, uint32_t* sidx_out, uint32_t* start_out,
                      uint32_t* members_out) {
  if (!rep_out || n > 0x7FFFFFF0u || (n_bases && !sidx)) return fail(ZKFL_E_ARG, "debug_groups: bad arguments");
  std::vector<uint32_t> rep;
  if (values) {
    std::vector<uint32_t> w(n * 8);
    memcpy(w.data(), values, n * 32);
    groups_learn(w.data(), n, rep);
  } else {
    rep.assign(rep_out, rep_out + n);
    if (!groups_valid(rep.data(), n)) return fail(ZKFL_E_ARG, "debug_groups: not a partition");
  }
  if (sig) groups_refine(rep.data(), sig, n);
  memcpy(rep_out, rep.data(), n * 4);
  if (sidx_out || start_out || members_out) {
    GroupQuery q;
    groups_query(rep.data(), (uint32_t)n, sidx, n_bases, u_base, q);
    if (sidx_out) memcpy(sidx_out, q.sidx.data(), n_bases * 4);
    if (start_out) memcpy(start_out, q.start.data(), (n_bases + 1) * 4);
    if (members_out && !q.members.empty()) memcpy(members_out, q.members.data(), q.members.size() * 4);
  }
  return ZKFL_OK;
}

}  // extern "C"
