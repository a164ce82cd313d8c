// The witness check: .r1cs -> device, and the check's kernels and entry points (see r1cs_check.h).
// Replaces `snarkjs wtns check <circuit.r1cs> <witness.wtns>`; the .r1cs is what the reference gives
// `snarkjs groth16 setup` (tests/full_system_simulation.mjs:713-716), the witness what its
// calculator writes (:758-767).
#include "r1cs_check.h"

#include <string.h>

#include <string>
#include <vector>

#include "common.h"
#include "host_parse.h"
#include "poly.h"

using namespace zkfl;

namespace {

constexpr uint32_t NO_CONSTRAINT = 0xFFFFFFFFu;

// A witness's verdict, emptied; wire 0 must be the constant 1 (std form).
__global__ void __launch_bounds__(64) k_r1cs_begin(R1csVerdict* __restrict__ v, const Fr* __restrict__ w) {
  if (threadIdx.x != 0) return;
  const Fr w0 = w[0];
  uint32_t rest = w0.v[0] ^ 1u;
#pragma unroll
  for (int i = 1; i < 8; i++) rest |= w0.v[i];
  v->n_failed = 0;
  v->first = NO_CONSTRAINT;
  v->w0_bad = rest != 0;
  v->pad = 0;
  v->a = v->b = v->c = fp_zero<FrP>();
}

// One lane per constraint.  The rows hold Montgomery forms (coef R^2 times a std-form wire), each
// fully reduced (field.h: fp_mul, fp_add return values < r), so a R * b R -> a b R compares with
// c R limb by limb.
__global__ void __launch_bounds__(256) k_r1cs_verdict(const uint32_t* __restrict__ rp, uint32_t m, uint32_t K,
                                                      const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                      const Fr* __restrict__ abc, R1csVerdict* __restrict__ v) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;  // 3 m < 2^32 (zkfl_r1cs_load)
  bool failed = false;
  if (j < m) {
    const Fr a = abc_row(rp, j, K, head, tail, abc);
    const Fr b = abc_row(rp, m + j, K, head, tail, abc);
    const Fr c = abc_row(rp, 2 * m + j, K, head, tail, abc);
    failed = !fp_eq(fp_mul(a, b), c);
  }
  __shared__ uint32_t s_cnt[4], s_first[4];
  const uint64_t bal = __ballot(failed);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_cnt[wave] = (uint32_t)__popcll((unsigned long long)bal);
    s_first[wave] = bal ? blockIdx.x * 256u + wave * 64u + (uint32_t)(__ffsll((unsigned long long)bal) - 1) : NO_CONSTRAINT;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t cnt = 0, first = NO_CONSTRAINT;
    for (int q = 0; q < 4; q++) {
      cnt += s_cnt[q];
      first = s_first[q] < first ? s_first[q] : first;
    }
    if (cnt) {  // sums and minima commute: the outcome does not depend on the workgroups' order
      atomicAdd(&v->n_failed, cnt);
      atomicMin(&v->first, first);
    }
  }
}

// After the verdict pass: a, b, c of the first failing constraint, to std form; a witness without
// the constant wire fails as a whole.
__global__ void __launch_bounds__(64) k_r1cs_values(const uint32_t* __restrict__ rp, uint32_t m, uint32_t K,
                                                    const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                    const Fr* __restrict__ abc, R1csVerdict* __restrict__ v) {
  if (threadIdx.x != 0) return;
  if (v->w0_bad) {
    v->n_failed = 1;
    v->first = NO_CONSTRAINT;
    return;
  }
  if (v->n_failed == 0) return;
  const uint32_t j = v->first;
  if (j >= m) return;
  v->a = fp_from_mont(abc_row(rp, j, K, head, tail, abc));
  v->b = fp_from_mont(abc_row(rp, m + j, K, head, tail, abc));
  v->c = fp_from_mont(abc_row(rp, 2 * m + j, K, head, tail, abc));
}

void r1cs_release(zkfl_r1cs* r) {
  if (!r) return;
  void* ptrs[] = {r->rows, r->cols, r->coefs, r->w, r->head, r->tail, r->abc, r->verdicts};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  zkfl_ctx* ctx = r->ctx;
  delete r;
  if (ctx) ctx_release(ctx);  // the object's reference (taken when it was made)
}

void header_of(const R1csHost& h, zkfl_r1cs_header* out) {
  out->n_wires = h.n_wires;
  out->n_pub_out = h.n_pub_out;
  out->n_pub_in = h.n_pub_in;
  out->n_prv_in = h.n_prv_in;
  out->n_constraints = h.m;
  out->n_labels = h.n_labels;
  out->n_terms = h.n_terms;
}

// The n witnesses d_w[i] (device, std form, n_wires long; null: the .wtns values host_w[i], staged
// through the object's buffer), checked one after the other on the context's stream; the verdicts
// come back in one copy.
int run_checks(zkfl_ctx* ctx, const zkfl_r1cs* r, size_t n, const Fr* const* d_w, const uint8_t* const* host_w,
               zkfl_r1cs_report* reports) {
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  if (n > r->verdict_cap) {
    HIP_TRY(hipStreamSynchronize(st), "sync");
    if (r->verdicts) (void)hipFree(r->verdicts);
    r->verdicts = nullptr;
    r->verdict_cap = 0;
    HIP_TRY(hipMalloc(&r->verdicts, n * sizeof(R1csVerdict)), "alloc verdicts");
    r->verdict_cap = n;
  }
  const uint32_t m = r->m, K = r->K;
  for (size_t i = 0; i < n; i++) {
    const Fr* w = d_w ? d_w[i] : r->w;
    if (!d_w) HIP_TRY(hipMemcpyAsync(r->w, host_w[i], (size_t)r->hdr.n_wires * 32, hipMemcpyHostToDevice, st), "upload");
    R1csVerdict* v = r->verdicts + i;
    hipLaunchKernelGGL(k_r1cs_begin, dim3(1), dim3(64), 0, st, v, w);
    if (m == 0) {
      hipLaunchKernelGGL(k_r1cs_values, dim3(1), dim3(64), 0, st, r->rows, m, K, r->head, r->tail, r->abc, v);
      continue;
    }
    int pi = ctx->prof.begin("r1cs_terms", st);
    r1cs_terms(st, r, w);
    ctx->prof.end(pi, st, (double)K);
    pi = ctx->prof.begin("r1cs_verdict", st);
    hipLaunchKernelGGL(k_r1cs_verdict, dim3(zk_grid(m, 256)), dim3(256), 0, st, r->rows, m, K, r->head, r->tail,
                       r->abc, v);
    hipLaunchKernelGGL(k_r1cs_values, dim3(1), dim3(64), 0, st, r->rows, m, K, r->head, r->tail, r->abc, v);
    ctx->prof.end(pi, st, (double)m);
  }
  HIP_TRY(hipGetLastError(), "r1cs check launch");
  std::vector<R1csVerdict> host(n);
  HIP_TRY(hipMemcpyAsync(host.data(), r->verdicts, n * sizeof(R1csVerdict), hipMemcpyDeviceToHost, st), "verdicts");
  HIP_TRY(hipStreamSynchronize(st), "r1cs check");
  size_t bad = SIZE_MAX;
  for (size_t i = 0; i < n; i++) {
    const R1csVerdict& v = host[i];
    if (v.n_failed && bad == SIZE_MAX) bad = i;
    if (!reports) continue;
    reports[i].n_failed = v.n_failed;
    reports[i].first = v.first;
    memcpy(reports[i].a, v.a.v, 32);
    memcpy(reports[i].b, v.b.v, 32);
    memcpy(reports[i].c, v.c.v, 32);
  }
  if (bad == SIZE_MAX) return ZKFL_OK;
  const R1csVerdict& v = host[bad];
  if (v.first == NO_CONSTRAINT) return fail(ZKFL_E_CONSTRAINT, "witness " + std::to_string(bad) + ": wire 0 is not 1");
  return fail(ZKFL_E_CONSTRAINT, "witness " + std::to_string(bad) + ": constraint #" + std::to_string(v.first) +
                                     " is not satisfied (" + std::to_string(v.n_failed) + " of " +
                                     std::to_string(r->m) + " fail)");
}

}  // namespace

void zkfl::r1cs_terms(hipStream_t st, const zkfl_r1cs* r, const Fr* w) {
  const AbcTerms T = {r->cols, r->coefs, r->cshift};
  if (r->K && r->m) abc_chunks(st, r->rows, 3 * r->m, T, w, r->K, r->head, r->tail, r->abc);  // no terms: every row is zero
}

extern "C" {

int zkfl_r1cs_parse(const uint8_t* buf, size_t len, zkfl_r1cs_header* out) {
  if (!buf || !out) return fail(ZKFL_E_ARG, "null argument");
  R1csHost h;
  std::string err;
  const int rc = r1cs_parse(buf, len, false, h, err);  // csrc/host_parse.cc
  if (rc) return fail(rc, err);
  header_of(h, out);
  return ZKFL_OK;
}

int zkfl_r1cs_load(zkfl_ctx* ctx, const uint8_t* buf, size_t len, zkfl_r1cs** out) {
  if (!ctx || !buf || !out) return fail(ZKFL_E_ARG, "null argument");
  R1csHost h;
  std::string err;
  const int rc = r1cs_parse(buf, len, true, h, err);
  if (rc) return fail(rc, err);
  if (h.m > 0x55555554u) return fail(ZKFL_E_FORMAT, "r1cs: too many constraints for 32-bit row indices");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  zkfl_r1cs* r = new zkfl_r1cs();
  r->ctx = ctx;
  ctx_retain(ctx);  // dropped by r1cs_release
  header_of(h, &r->hdr);
  r->m = h.m;
  r->K = (uint32_t)h.n_terms;
  r->cshift = h.cshift;
  const size_t rows = 3 * (size_t)h.m + 1, K = r->K, ncoefs = h.coefs.size() / 8;
  const size_t chunks = (K + ABC_L - 1) / ABC_L + 1;
  hipError_t e = hipMalloc(&r->rows, rows * 4);
  if (e == hipSuccess) e = hipMalloc(&r->cols, (K ? K : 1) * 4);
  if (e == hipSuccess) e = hipMalloc(&r->coefs, (ncoefs ? ncoefs : 1) * 32);
  if (e == hipSuccess) e = hipMalloc(&r->w, (size_t)(h.n_wires ? h.n_wires : 1) * 32);
  if (e == hipSuccess) e = hipMalloc(&r->head, chunks * 32);
  if (e == hipSuccess) e = hipMalloc(&r->tail, chunks * 32);
  if (e == hipSuccess) e = hipMalloc(&r->abc, (rows - 1 ? rows - 1 : 1) * 32);
  if (e == hipSuccess) e = hipMemcpyAsync(r->rows, h.rowptr.data(), rows * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && K) e = hipMemcpyAsync(r->cols, h.cols.data(), K * 4, hipMemcpyHostToDevice, st);
  if (e == hipSuccess && ncoefs) {
    e = hipMemcpyAsync(r->coefs, h.coefs.data(), ncoefs * 32, hipMemcpyHostToDevice, st);
    // std -> coef R -> coef R^2: the form k_abc_chunks multiplies a std-form wire with
    if (e == hipSuccess) {
      fr_std_to_mont(st, r->coefs, ncoefs);
      fr_std_to_mont(st, r->coefs, ncoefs);
      e = hipGetLastError();
    }
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);  // h's vectors go with this frame
  if (e != hipSuccess) {
    r1cs_release(r);
    return hip_fail(e, "r1cs load");
  }
  *out = r;
  return ZKFL_OK;
}

int zkfl_r1cs_info(const zkfl_r1cs* r1cs, zkfl_r1cs_header* out) {
  if (!r1cs || !out) return fail(ZKFL_E_ARG, "null argument");
  *out = r1cs->hdr;
  return ZKFL_OK;
}

int zkfl_r1cs_free(zkfl_r1cs* r1cs) {
  if (!r1cs) return ZKFL_OK;
  (void)hipSetDevice(r1cs->ctx->device);
  (void)hipStreamSynchronize(r1cs->ctx->st);
  r1cs_release(r1cs);
  return ZKFL_OK;
}

int zkfl_r1cs_check(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, size_t n, const uint8_t* const* wtns, const size_t* wtns_len,
                    zkfl_r1cs_report* reports) {
  if (!ctx || !r1cs || (n && (!wtns || !wtns_len))) return fail(ZKFL_E_ARG, "null argument");
  if (ctx != r1cs->ctx) return fail(ZKFL_E_ARG, "r1cs was loaded on another context");
  std::vector<const uint8_t*> vals(n);
  for (size_t i = 0; i < n; i++) {  // every witness is validated before any check runs
    if (!wtns[i]) return fail(ZKFL_E_ARG, "null witness");
    WtnsView v;
    std::string err;
    const int rc = wtns_parse(wtns[i], wtns_len[i], v, err);
    if (rc) return fail(rc, "witness " + std::to_string(i) + ": " + err);
    if (v.n != r1cs->hdr.n_wires)
      return fail(ZKFL_E_MISMATCH, "witness " + std::to_string(i) + ": nWitness != r1cs nWires");
    for (uint32_t k = 0; k < v.n; k++) {
      uint32_t x[8];
      memcpy(x, v.data + 32 * (size_t)k, 32);
      if (!fr_lt_r(x))
        return fail(ZKFL_E_ARG, "witness " + std::to_string(i) + ": wire " + std::to_string(k) + " is not < r");
    }
    vals[i] = v.data;
  }
  if (n == 0) return ZKFL_OK;
  return run_checks(ctx, r1cs, n, nullptr, vals.data(), reports);
}

// Resident witnesses are std form and nVars long (objects.h); values are the prover's own and are
// taken mod r by the arithmetic.
int zkfl_r1cs_check_resident(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, size_t n, const zkfl_witness* const* w,
                             zkfl_r1cs_report* reports) {
  if (!ctx || !r1cs || (n && !w)) return fail(ZKFL_E_ARG, "null argument");
  if (ctx != r1cs->ctx) return fail(ZKFL_E_ARG, "r1cs was loaded on another context");
  std::vector<const Fr*> d(n);
  for (size_t i = 0; i < n; i++) {
    if (!w[i] || !w[i]->key || !w[i]->d) return fail(ZKFL_E_ARG, "null witness");
    if (w[i]->key->nVars != r1cs->hdr.n_wires)
      return fail(ZKFL_E_MISMATCH, "witness " + std::to_string(i) + ": key nVars != r1cs nWires");
    d[i] = w[i]->d;
  }
  if (n == 0) return ZKFL_OK;
  return run_checks(ctx, r1cs, n, d.data(), nullptr, reports);
}

}  // extern "C"
