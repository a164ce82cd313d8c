// The key check: kernels and the one entry point (see keycheck.h; include/zkfl.h has the
// equations).  The reference proves with whatever `<c>_final.zkey` lies in the circuit directory
// (tests/full_system_simulation.mjs:713-738); this is the call that tests the key first.
#include "keycheck.h"

#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "devbufs.h"
#include "host_parse.h"
#include "objects.h"
#include "pairing.h"
#include "pointcheck.h"
#include "poly.h"
#include "r1cs_check.h"
#include "verify.h"
#include "verify_dev.h"

using namespace zkfl;

namespace {

constexpr uint32_t NONE = VERDICT_NONE;

// Rows a | b | c (n each, Montgomery) of the resident .r1cs on the vector v after r1cs_terms(v):
// row j < m stitched by abc_row, the public rows a[m + s] = v[s] for s <= npub (m + npub + 1 <= n),
// zero elsewhere.
__global__ void __launch_bounds__(256) k_rows_gather(const uint32_t* __restrict__ rp, uint32_t m, uint32_t K,
                                                     const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                     const Fr* __restrict__ abc, const Fr* __restrict__ v, uint32_t npub,
                                                     uint32_t n, Fr* __restrict__ out) {
  const uint32_t j = blockIdx.x * 256u + threadIdx.x;
  if (j >= n) return;
  Fr a = fp_zero<FrP>(), b = a, c = a;
  if (j < m) {
    a = abc_row(rp, j, K, head, tail, abc);
    b = abc_row(rp, m + j, K, head, tail, abc);
    c = abc_row(rp, 2 * m + j, K, head, tail, abc);
  } else if (j - m <= npub) {
    a = fp_to_mont(v[j - m]);
  }
  out[j] = a;
  out[n + j] = b;
  out[2 * (size_t)n + j] = c;
}

__global__ void __launch_bounds__(256) k_fr_sum(const Fr* __restrict__ x, const Fr* __restrict__ y, size_t n,
                                                Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  out[i] = fp_add(x[i], y[i]);
}

// Row i < nrows of the key's section 4 on rho (after abc_chunks over its CSR) against want[i]
// (Montgomery, fully reduced on both sides): the matrices compared as linear maps.
__global__ void __launch_bounds__(256) k_rows_compare(const uint32_t* __restrict__ rp, uint32_t nrows, uint32_t K,
                                                      const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                      const Fr* __restrict__ abc, const Fr* __restrict__ want,
                                                      KeyVerdict* __restrict__ v) {
  const uint32_t i = blockIdx.x * 256u + threadIdx.x;
  bool bad = false;
  if (i < nrows) bad = !fp_eq(abc_row(rp, i, K, head, tail, abc), want[i]);
  verdict_reduce<256>(bad, v);
}

// the MSM results, by slot
enum { R_A, R_B1, R_IC, R_C, R_H, R_LA, R_LB, R_LC_PUB, R_LC_PRV, R_LBA_PUB, R_LBA_PRV, R_LAB_PUB, R_LAB_PRV, R_H0, R_N };
enum { S_B2, S_L2B, S_N };
constexpr int N_PAIRS = 8;

// After the MSMs, one lane per task: lanes 0-2 compare A, B1, B2 with their Lagrange sums; lanes
// 3-10 write pair t - 3 of the pairing batch (std affine; a pair that is not usable is written as
// infinity and its value ignored):
//   0 e(delta1, G2)   1 e(G1, delta2)   2 e(IC, gamma2)   3 e(K_pub, G2)
//   4 e(C, delta2)    5 e(K_prv, G2)    6 e(H, delta2)    7 e(H0, G2)
// hdr1 = delta1, hdr2 = gamma2 | delta2 (Montgomery, zeroed by the host when unusable).
__global__ void __launch_bounds__(64) k_key_finish(const G1P* __restrict__ R, const G2P* __restrict__ S,
                                                   const G1Aff* __restrict__ hdr1, const G2Aff* __restrict__ hdr2,
                                                   uint32_t* __restrict__ same, uint32_t* __restrict__ g1_out,
                                                   uint32_t* __restrict__ g2_out) {
  const int t = threadIdx.x;
  if (t == 0) same[0] = xyzz_same<FqOps>(R[R_A], R[R_LA]);
  if (t == 1) same[1] = xyzz_same<FqOps>(R[R_B1], R[R_LB]);
  if (t == 2) same[2] = xyzz_same<Fq2Ops>(S[S_B2], S[S_L2B]);
  if (t < 3 || t >= 3 + N_PAIRS) return;
  const int p = t - 3;
  const G1Aff g1 = g1_generator();
  const G2Aff g2 = g2_generator();
  G1Aff P;
  G2Aff Q = g2;
  switch (p) {
    case 0: P = hdr1[0]; break;
    case 1: P = g1; Q = hdr2[1]; break;
    case 2: P = xyzz_to_affine<FqOps>(R[R_IC]); Q = hdr2[0]; break;
    case 3: P = xyzz_to_affine<FqOps>(xyzz_add<FqOps>(xyzz_add<FqOps>(R[R_LBA_PUB], R[R_LAB_PUB]), R[R_LC_PUB])); break;
    case 4: P = xyzz_to_affine<FqOps>(R[R_C]); Q = hdr2[1]; break;
    case 5: P = xyzz_to_affine<FqOps>(xyzz_add<FqOps>(xyzz_add<FqOps>(R[R_LBA_PRV], R[R_LAB_PRV]), R[R_LC_PRV])); break;
    case 6: P = xyzz_to_affine<FqOps>(R[R_H]); Q = hdr2[1]; break;
    default: P = xyzz_to_affine<FqOps>(R[R_H0]); break;
  }
  store_std(P, g1_out + p * 16);
  store_std(Q, g2_out + p * 32);
}

bool nonzero(const uint8_t* p, size_t len) {
  for (size_t i = 0; i < len; i++)
    if (p[i]) return true;
  return false;
}

// One base set: the section's points without its infinities (as the key loader keeps them), sidx[i]
// = the scalar of kept point i (its index in the section + off).
template <class F>
struct BaseSet {
  std::vector<uint8_t> img;
  std::vector<uint32_t> sidx;
  Affine<F>* d_img = nullptr;
  MsmBases<F> mb;
  bool expanded = false;
  ~BaseSet() { msm_bases_free(mb); }
  size_t n() const { return sidx.size(); }
  void take(const uint8_t* sec, size_t cnt, uint32_t off) {
    constexpr size_t psz = sizeof(Affine<F>);
    for (size_t i = 0; i < cnt; i++) {
      const uint8_t* q = sec + i * psz;
      if (!nonzero(q, psz)) continue;
      img.insert(img.end(), q, q + psz);
      sidx.push_back(off + (uint32_t)i);
    }
  }
  hipError_t upload(DevBufs& D, hipStream_t st) {
    ZK_CHECK(D.get(&d_img, n()));
    if (n()) ZK_CHECK(hipMemcpyAsync(d_img, img.data(), img.size(), hipMemcpyHostToDevice, st));
    return hipSuccess;
  }
  hipError_t expand(int c, hipStream_t st) {
    ZK_CHECK(msm_bases_alloc(mb, n(), c));
    expanded = true;
    if (!n()) return hipSuccess;
    return msm_bases_set(mb, d_img, sidx.data(), 0xFFFFFFFFu, st);
  }
};

// out = MSM(b, scalars) on st; an empty set leaves out as the host zeroed it (infinity)
template <class F>
hipError_t msm_of(const BaseSet<F>& b, MsmScratch<F>& s, MsmTail<F>& t, const Fr* scalars, XYZZ<F>* out,
                  hipStream_t st) {
  if (!b.n()) return hipSuccess;
  return msm_run(b.mb, s, t, reinterpret_cast<const uint32_t*>(scalars), nullptr, out, st, nullptr, "");
}

int draw_fr(uint8_t* out, size_t count) {
  for (size_t i = 0; i < count; i++) {
    for (int tries = 0;; tries++) {
      uint8_t b[32];
      uint32_t w[8];
      if (getrandom(b, 32, 0) != 32) return fail(ZKFL_E_DEVICE, "getrandom failed");
      b[31] &= 0x3f;  // < 2^254
      memcpy(w, b, 32);
      if (fr_lt_r(w)) {
        memcpy(out + 32 * i, b, 32);
        break;
      }
      if (tries > 64) return fail(ZKFL_E_DEVICE, "rng");
    }
  }
  return ZKFL_OK;
}

int check_scalars(const uint8_t* v, size_t count, const char* what) {
  for (size_t i = 0; i < count; i++) {
    uint32_t w[8];
    memcpy(w, v + 32 * i, 32);
    if (!fr_lt_r(w)) return fail(ZKFL_E_ARG, std::string(what) + " " + std::to_string(i) + " is not < r");
  }
  return ZKFL_OK;
}

const char* const CHECK_NAMES[ZKFL_KEYCHECK_N] = {"header", "points", "coefficients", "A", "B1", "B2", "IC", "C", "H"};

}  // namespace

extern "C" int zkfl_zkey_check(zkfl_ctx* ctx, const zkfl_r1cs* r1cs, const uint8_t* zkey, size_t zkey_len,
                               const zkfl_ptau_view* pt, const uint8_t* rho_in, const uint8_t* sigma_in,
                               zkfl_zkey_report* report) {
  if (!ctx || !r1cs || !zkey || !pt) return fail(ZKFL_E_ARG, "null argument");
  if (ctx != r1cs->ctx) return fail(ZKFL_E_ARG, "r1cs was loaded on another context");
  if (!pt->L || !pt->L2 || !pt->La || !pt->Lb || !pt->H0 || !pt->alpha1 || !pt->beta1 || !pt->beta2)
    return fail(ZKFL_E_ARG, "ptau view: null block");
  ZkeyHost z;
  {
    std::string err;
    const int rc = zkey_parse(zkey, zkey_len, z, err);  // q, r are BN254's; sizes; section 4 -> CSR
    if (rc) return fail(rc, err);
  }
  const zkfl_r1cs_header& rh = r1cs->hdr;
  const uint32_t nv = z.nVars, npub = z.nPub, n = z.dom, m = r1cs->m;
  if (nv != rh.n_wires) return fail(ZKFL_E_MISMATCH, "zkey nVars != r1cs nWires");
  if ((uint64_t)npub != (uint64_t)rh.n_pub_out + rh.n_pub_in) return fail(ZKFL_E_MISMATCH, "zkey nPublic != r1cs public signals");
  {
    uint64_t want = 1;  // zkfl/zkey.py domain_size_for
    while (want < (uint64_t)m + npub + 1) want *= 2;
    if (want != n) return fail(ZKFL_E_MISMATCH, "zkey domainSize is not the r1cs's domain");
  }
  if (pt->power != (uint32_t)z.logn) return fail(ZKFL_E_MISMATCH, "ptau view: power is not the key's domain");
  if (pt->L_len != (size_t)n * 64 || pt->La_len != (size_t)n * 64 || pt->Lb_len != (size_t)n * 64 ||
      pt->H0_len != (size_t)n * 64 || pt->L2_len != (size_t)n * 128)
    return fail(ZKFL_E_ARG, "ptau view: a block is not domainSize points long");
  std::vector<uint8_t> rnd;
  if (!rho_in || !sigma_in) {
    rnd.resize(32 * ((size_t)nv + n));
    const int rc = draw_fr(rnd.data(), (size_t)nv + n);
    if (rc) return rc;
  }
  if (rho_in) {
    const int rc = check_scalars(rho_in, nv, "rho");
    if (rc) return rc;
  }
  if (sigma_in) {
    const int rc = check_scalars(sigma_in, n, "sigma");
    if (rc) return rc;
  }
  const uint8_t* rho = rho_in ? rho_in : rnd.data();
  const uint8_t* sigma = sigma_in ? sigma_in : rnd.data() + 32 * (size_t)nv;

  uint32_t status[ZKFL_KEYCHECK_N];
  for (uint32_t& s : status) s = ZKFL_KEYCHECK_PASS;
  zkfl_zkey_report rep = {};

  // ---- header, host part: the ptau's alpha / beta; gamma2, delta1, delta2 present ----
  const uint8_t *alpha1 = z.pts, *beta1 = z.pts + 64, *beta2 = z.pts + 128, *gamma2 = z.pts + 256,
                *delta1 = z.pts + 384, *delta2 = z.pts + 448;
  std::string header_why;
  if (memcmp(alpha1, pt->alpha1, 64) != 0) header_why = "alpha1 is not the ptau's";
  else if (memcmp(beta1, pt->beta1, 64) != 0) header_why = "beta1 is not the ptau's";
  else if (memcmp(beta2, pt->beta2, 128) != 0) header_why = "beta2 is not the ptau's";
  else if (!nonzero(gamma2, 128)) header_why = "gamma2 is infinity";
  else if (!nonzero(delta1, 64)) header_why = "delta1 is infinity";
  else if (!nonzero(delta2, 128)) header_why = "delta2 is infinity";

  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  DevBufs D;

  // ---- points ----
  // the header's six points one launch each (a verdict per point: which of gamma2, delta1, delta2
  // is usable decides what runs below), then sections 3, 5, 6, 8, 9 (G1) and 7 (G2), compacted
  enum { Q_IC, Q_A, Q_B1, Q_C, Q_H, Q_G1 };
  BaseSet<FqOps> q1[Q_G1];
  BaseSet<Fq2Ops> qB2;
  q1[Q_IC].take(z.secIC, (size_t)npub + 1, 0);
  q1[Q_A].take(z.secA, nv, 0);
  q1[Q_B1].take(z.secB1, nv, 0);
  q1[Q_C].take(z.secC, z.nC, npub + 1);
  q1[Q_H].take(z.secH, n, 0);
  qB2.take(z.secB2, nv, 0);
  uint8_t hdr1_img[3 * 64], hdr2_img[3 * 128];
  memcpy(hdr1_img, alpha1, 64);
  memcpy(hdr1_img + 64, beta1, 64);
  memcpy(hdr1_img + 128, delta1, 64);
  memcpy(hdr2_img, beta2, 128);
  memcpy(hdr2_img + 128, gamma2, 128);
  memcpy(hdr2_img + 256, delta2, 128);
  G1Aff* d_hdr1;
  G2Aff* d_hdr2;
  enum { V_ALPHA1, V_BETA1, V_BETA2, V_GAMMA2, V_DELTA1, V_DELTA2, V_IC, V_A, V_B1, V_B2, V_C, V_H, V_COEF, V_N };
  KeyVerdict* d_v;
  HIP_TRY(D.get(&d_hdr1, 3), "alloc");
  HIP_TRY(D.get(&d_hdr2, 3), "alloc");
  HIP_TRY(D.get(&d_v, V_N), "alloc");
  {
    KeyVerdict init[V_N];
    for (KeyVerdict& v : init) v = {0, NONE};
    HIP_TRY(hipMemcpyAsync(d_v, init, sizeof(init), hipMemcpyHostToDevice, st), "upload");
    HIP_TRY(hipStreamSynchronize(st), "sync");  // init goes with this scope
  }
  HIP_TRY(hipMemcpyAsync(d_hdr1, hdr1_img, sizeof(hdr1_img), hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_hdr2, hdr2_img, sizeof(hdr2_img), hipMemcpyHostToDevice, st), "upload");
  for (auto& q : q1) HIP_TRY(q.upload(D, st), "upload");
  HIP_TRY(qB2.upload(D, st), "upload");
  int pi = ctx->prof.begin("keycheck_points", st);
  {
    auto g1 = [&](const G1Aff* p, size_t cnt, int slot) {
      if (cnt)
        hipLaunchKernelGGL(k_points_check<FqOps>, dim3(zk_grid(cnt, 256)), dim3(256), 0, st, p, (uint32_t)cnt, d_v + slot);
    };
    auto g2 = [&](const G2Aff* p, size_t cnt, int slot) {
      if (cnt)
        hipLaunchKernelGGL(k_points_check<Fq2Ops>, dim3(zk_grid(cnt, 64)), dim3(64), 0, st, p, (uint32_t)cnt, d_v + slot);
    };
    g1(d_hdr1, 1, V_ALPHA1);
    g1(d_hdr1 + 1, 1, V_BETA1);
    g1(d_hdr1 + 2, 1, V_DELTA1);
    g2(d_hdr2, 1, V_BETA2);
    g2(d_hdr2 + 1, 1, V_GAMMA2);
    g2(d_hdr2 + 2, 1, V_DELTA2);
    g1(q1[Q_IC].d_img, q1[Q_IC].n(), V_IC);
    g1(q1[Q_A].d_img, q1[Q_A].n(), V_A);
    g1(q1[Q_B1].d_img, q1[Q_B1].n(), V_B1);
    g2(qB2.d_img, qB2.n(), V_B2);
    g1(q1[Q_C].d_img, q1[Q_C].n(), V_C);
    g1(q1[Q_H].d_img, q1[Q_H].n(), V_H);
  }
  HIP_TRY(hipGetLastError(), "points check launch");
  ctx->prof.end(pi, st, (double)(6 + q1[Q_IC].n() + q1[Q_A].n() + q1[Q_B1].n() + qB2.n() + q1[Q_C].n() + q1[Q_H].n()));
  KeyVerdict pv[V_N];
  HIP_TRY(hipMemcpyAsync(pv, d_v, sizeof(pv), hipMemcpyDeviceToHost, st), "verdicts");
  HIP_TRY(hipStreamSynchronize(st), "points check");
  uint32_t hdr_bad = 0, hdr_first = NONE;  // header points in file order: V_ALPHA1 .. V_DELTA2 = 0 .. 5
  for (int k = V_DELTA2; k >= V_ALPHA1; k--)
    if (pv[k].n_bad) {
      hdr_bad++;
      hdr_first = (uint32_t)k;
    }
  const bool ok_delta1 = !pv[V_DELTA1].n_bad && nonzero(delta1, 64), ok_gamma2 = !pv[V_GAMMA2].n_bad && nonzero(gamma2, 128),
             ok_delta2 = !pv[V_DELTA2].n_bad && nonzero(delta2, 128);
  if (hdr_bad && header_why.empty()) header_why = "a header point is not a point of its group";
  {
    // first bad section in file order; the report's index is the point's index in its section
    struct Sec {
      int slot, section;
      const std::vector<uint32_t>* sidx;
      uint32_t off;
    };
    const Sec order[] = {{V_IC, 3, &q1[Q_IC].sidx, 0},  {V_A, 5, &q1[Q_A].sidx, 0},  {V_B1, 6, &q1[Q_B1].sidx, 0},
                         {V_B2, 7, &qB2.sidx, 0},       {V_C, 8, &q1[Q_C].sidx, npub + 1}, {V_H, 9, &q1[Q_H].sidx, 0}};
    if (hdr_bad) {
      status[ZKFL_KEYCHECK_POINTS] = ZKFL_KEYCHECK_FAIL;
      rep.point_section = 2;
      rep.point_index = hdr_first;
      rep.point_count = hdr_bad;
    }
    for (const Sec& s : order) {
      if (!pv[s.slot].n_bad || status[ZKFL_KEYCHECK_POINTS] == ZKFL_KEYCHECK_FAIL) continue;
      status[ZKFL_KEYCHECK_POINTS] = ZKFL_KEYCHECK_FAIL;
      rep.point_section = (uint32_t)s.section;
      rep.point_index = (*s.sidx)[pv[s.slot].first] - s.off;
      rep.point_count = pv[s.slot].n_bad;
    }
  }
  const bool run_A = !pv[V_A].n_bad, run_B1 = !pv[V_B1].n_bad, run_B2 = !pv[V_B2].n_bad,
             run_IC = !pv[V_IC].n_bad && ok_gamma2, run_C = !pv[V_C].n_bad && ok_delta2,
             run_H = !pv[V_H].n_bad && ok_delta2;

  // ---- rows ----
  // scalars: rho | rho on the public wires | rho on the others | sigma, std form
  Fr *d_rho, *d_pub, *d_prv, *d_sigma, *d_rows_pub, *d_rows_prv, *d_rows;
  HIP_TRY(D.get(&d_rho, 3 * (size_t)nv), "alloc");
  d_pub = d_rho + nv;
  d_prv = d_pub + nv;
  HIP_TRY(D.get(&d_sigma, n), "alloc");
  HIP_TRY(D.get(&d_rows_pub, 3 * (size_t)n), "alloc");
  HIP_TRY(D.get(&d_rows_prv, 3 * (size_t)n), "alloc");
  HIP_TRY(D.get(&d_rows, 2 * (size_t)n), "alloc");
  std::vector<uint8_t> split(64 * (size_t)nv, 0);
  memcpy(split.data(), rho, 32 * ((size_t)npub + 1));
  memcpy(split.data() + 32 * ((size_t)nv + npub + 1), rho + 32 * ((size_t)npub + 1), 32 * ((size_t)nv - npub - 1));
  HIP_TRY(hipMemcpyAsync(d_rho, rho, 32 * (size_t)nv, hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_pub, split.data(), split.size(), hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_sigma, sigma, 32 * (size_t)n, hipMemcpyHostToDevice, st), "upload");
  // the key's section 4 as the loader lays it out: A rows then B rows over one term array
  uint32_t *d_zrows, *d_zcols;
  Fr *d_zcoefs, *d_zhead, *d_ztail, *d_zabc;
  const size_t zK = z.ncoef, zchunks = (zK + ABC_L - 1) / ABC_L + 1, zcoefs = z.coefs.size() / 8;
  HIP_TRY(D.get(&d_zrows, 2 * (size_t)n + 1), "alloc");
  HIP_TRY(D.get(&d_zcols, zK), "alloc");
  HIP_TRY(D.get(&d_zcoefs, zcoefs), "alloc");
  HIP_TRY(D.get(&d_zhead, zchunks), "alloc");
  HIP_TRY(D.get(&d_ztail, zchunks), "alloc");
  HIP_TRY(D.get(&d_zabc, 2 * (size_t)n), "alloc");
  HIP_TRY(hipMemcpyAsync(d_zrows, z.rowptr.data(), (size_t)n * 4, hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_zrows + n, z.rowptr.data() + n + 1, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, st), "upload");
  if (zK) {
    HIP_TRY(hipMemcpyAsync(d_zcols, z.cols.data(), zK * 4, hipMemcpyHostToDevice, st), "upload");
    HIP_TRY(hipMemcpyAsync(d_zcoefs, z.coefs.data(), zcoefs * 32, hipMemcpyHostToDevice, st), "upload");
  }
  pi = ctx->prof.begin("keycheck_rows", st);
  {
    const unsigned g = zk_grid(n, 256);
    r1cs_terms(st, r1cs, d_pub);
    hipLaunchKernelGGL(k_rows_gather, dim3(g), dim3(256), 0, st, r1cs->rows, m, r1cs->K, r1cs->head, r1cs->tail,
                       r1cs->abc, d_pub, npub, n, d_rows_pub);
    r1cs_terms(st, r1cs, d_prv);
    hipLaunchKernelGGL(k_rows_gather, dim3(g), dim3(256), 0, st, r1cs->rows, m, r1cs->K, r1cs->head, r1cs->tail,
                       r1cs->abc, d_prv, npub, n, d_rows_prv);
    hipLaunchKernelGGL(k_fr_sum, dim3(zk_grid(2 * (size_t)n, 256)), dim3(256), 0, st, d_rows_pub, d_rows_prv,
                       2 * (size_t)n, d_rows);
    const AbcTerms T = {d_zcols, d_zcoefs, z.cshift};
    if (zK) abc_chunks(st, d_zrows, 2 * n, T, d_rho, (uint32_t)zK, d_zhead, d_ztail, d_zabc);
    hipLaunchKernelGGL(k_rows_compare, dim3(zk_grid(2 * (size_t)n, 256)), dim3(256), 0, st, d_zrows, 2 * n, (uint32_t)zK,
                       d_zhead, d_ztail, d_zabc, d_rows, d_v + V_COEF);
    // the MSMs take std-form scalars
    fr_mont_to_std(st, d_rows_pub, 3 * (size_t)n);
    fr_mont_to_std(st, d_rows_prv, 3 * (size_t)n);
    fr_mont_to_std(st, d_rows, 2 * (size_t)n);
  }
  HIP_TRY(hipGetLastError(), "row evaluation launch");
  ctx->prof.end(pi, st, (double)(2.0 * r1cs->K + zK));

  // ---- MSMs ----
  BaseSet<FqOps> bL, bLa, bLb, bH0;
  BaseSet<Fq2Ops> bL2;
  bL.take(pt->L, n, 0);
  bLa.take(pt->La, n, 0);
  bLb.take(pt->Lb, n, 0);
  bH0.take(pt->H0, n, 0);
  bL2.take(pt->L2, n, 0);
  size_t most1 = std::max({bL.n(), bLa.n(), bLb.n(), bH0.n()}), most2 = std::max(bL2.n(), qB2.n());
  for (auto& q : q1) most1 = std::max(most1, q.n());
  const int c = msm_pick_c(std::max(most1, most2));
  MsmScratch<FqOps> s1;
  MsmTail<FqOps> t1;
  MsmScratch<Fq2Ops> s2;
  MsmTail<Fq2Ops> t2;
  struct Engines {
    MsmScratch<FqOps>& s1;
    MsmTail<FqOps>& t1;
    MsmScratch<Fq2Ops>& s2;
    MsmTail<Fq2Ops>& t2;
    ~Engines() {
      msm_scratch_free(s1);
      msm_tail_free(t1);
      msm_scratch_free(s2);
      msm_tail_free(t2);
    }
  } engines{s1, t1, s2, t2};
  HIP_TRY(msm_scratch_alloc(s1, std::max<size_t>(most1, 1), c, st), "msm scratch");
  HIP_TRY(msm_tail_alloc(t1, std::max<size_t>(most1, 1), c), "msm tail");
  HIP_TRY(msm_scratch_alloc(s2, std::max<size_t>(most2, 1), c, st), "msm scratch");
  HIP_TRY(msm_tail_alloc(t2, std::max<size_t>(most2, 1), c), "msm tail");
  G1P* d_R;
  G2P* d_S;
  uint32_t *d_same, *d_g1, *d_g2;
  HIP_TRY(D.get(&d_R, R_N), "alloc");
  HIP_TRY(D.get(&d_S, S_N), "alloc");
  HIP_TRY(D.get(&d_same, 4), "alloc");
  HIP_TRY(D.get(&d_g1, N_PAIRS * 16), "alloc");
  HIP_TRY(D.get(&d_g2, N_PAIRS * 32), "alloc");
  HIP_TRY(hipMemsetAsync(d_R, 0, R_N * sizeof(G1P), st), "memset");  // ZZ = 0: infinity
  HIP_TRY(hipMemsetAsync(d_S, 0, S_N * sizeof(G2P), st), "memset");
  for (BaseSet<FqOps>* b : {&bL, &bLa, &bLb, &bH0}) HIP_TRY(b->upload(D, st), "upload");
  HIP_TRY(bL2.upload(D, st), "upload");
  pi = ctx->prof.begin("keycheck_msm", st);
  {
    hipError_t e = hipSuccess;
    auto m1 = [&](BaseSet<FqOps>& b, const Fr* sc, int slot) {
      if (e != hipSuccess) return;
      if (!b.expanded) e = b.expand(c, st);
      if (e == hipSuccess) e = msm_of(b, s1, t1, sc, d_R + slot, st);
    };
    auto m2 = [&](BaseSet<Fq2Ops>& b, const Fr* sc, int slot) {
      if (e != hipSuccess) return;
      if (!b.expanded) e = b.expand(c, st);
      if (e == hipSuccess) e = msm_of(b, s2, t2, sc, d_S + slot, st);
    };
    const Fr *a = d_rows, *b = d_rows + n;
    if (run_A) {
      m1(q1[Q_A], d_rho, R_A);
      m1(bL, a, R_LA);
    }
    if (run_B1) {
      m1(q1[Q_B1], d_rho, R_B1);
      m1(bL, b, R_LB);
    }
    if (run_B2) {
      m2(qB2, d_rho, S_B2);
      m2(bL2, b, S_L2B);
    }
    if (run_IC) {
      m1(q1[Q_IC], d_rho, R_IC);
      m1(bLb, d_rows_pub, R_LBA_PUB);
      m1(bLa, d_rows_pub + n, R_LAB_PUB);
      m1(bL, d_rows_pub + 2 * (size_t)n, R_LC_PUB);
    }
    if (run_C) {
      m1(q1[Q_C], d_rho, R_C);
      m1(bLb, d_rows_prv, R_LBA_PRV);
      m1(bLa, d_rows_prv + n, R_LAB_PRV);
      m1(bL, d_rows_prv + 2 * (size_t)n, R_LC_PRV);
    }
    if (run_H) {
      m1(q1[Q_H], d_sigma, R_H);
      m1(bH0, d_sigma, R_H0);
    }
    if (e != hipSuccess) return hip_fail(e, "key check MSM");
  }
  ctx->prof.end(pi, st, (double)(most1 + most2));

  // ---- pairings ----
  pi = ctx->prof.begin("keycheck_pairing", st);
  if (!ok_delta1) memset(hdr1_img + 128, 0, 64);
  if (!ok_gamma2) memset(hdr2_img + 128, 0, 128);
  if (!ok_delta2) memset(hdr2_img + 256, 0, 128);
  HIP_TRY(hipMemcpyAsync(d_hdr1, hdr1_img + 128, 64, hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_hdr2, hdr2_img + 128, 256, hipMemcpyHostToDevice, st), "upload");
  hipLaunchKernelGGL(k_key_finish, dim3(1), dim3(64), 0, st, (const G1P*)d_R, (const G2P*)d_S, (const G1Aff*)d_hdr1,
                     (const G2Aff*)d_hdr2, d_same, d_g1, d_g2);
  HIP_TRY(hipGetLastError(), "key finish launch");
  uint32_t same[4];
  uint8_t g1b[N_PAIRS * 64], g2b[N_PAIRS * 128];
  KeyVerdict cv;
  HIP_TRY(hipMemcpyAsync(same, d_same, sizeof(same), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipMemcpyAsync(g1b, d_g1, sizeof(g1b), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipMemcpyAsync(g2b, d_g2, sizeof(g2b), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipMemcpyAsync(&cv, d_v + V_COEF, sizeof(cv), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipStreamSynchronize(st), "key check");
  std::vector<uint8_t> gt(N_PAIRS * 384);
  {
    std::string err;
    const int rc = pairing_batch(N_PAIRS, g1b, g2b, 1, gt.data(), st, err);
    if (rc) return fail(rc == ZKFL_E_ARG ? ZKFL_E_DEVICE : rc, "key check pairing: " + err);
  }
  ctx->prof.end(pi, st, (double)N_PAIRS);
  auto gt_same = [&](int i) { return memcmp(gt.data() + 384 * (size_t)(2 * i), gt.data() + 384 * (size_t)(2 * i + 1), 384) == 0; };

  // ---- verdicts ----
  if (header_why.empty() && !gt_same(0)) header_why = "e(delta1, G2) != e(G1, delta2)";
  if (!header_why.empty()) status[ZKFL_KEYCHECK_HEADER] = ZKFL_KEYCHECK_FAIL;
  if (cv.n_bad) {
    status[ZKFL_KEYCHECK_COEFFICIENTS] = ZKFL_KEYCHECK_FAIL;
    rep.coef_matrix = cv.first / n;
    rep.coef_row = cv.first % n;
    rep.coef_count = cv.n_bad;
  }
  auto set = [&](int check, bool ran, bool holds) {
    status[check] = !ran ? ZKFL_KEYCHECK_NOT_RUN : holds ? ZKFL_KEYCHECK_PASS : ZKFL_KEYCHECK_FAIL;
  };
  set(ZKFL_KEYCHECK_A, run_A, same[0] != 0);
  set(ZKFL_KEYCHECK_B1, run_B1, same[1] != 0);
  set(ZKFL_KEYCHECK_B2, run_B2, same[2] != 0);
  set(ZKFL_KEYCHECK_IC, run_IC, gt_same(1));
  set(ZKFL_KEYCHECK_C, run_C, gt_same(2));
  set(ZKFL_KEYCHECK_H, run_H, gt_same(3));
  memcpy(rep.status, status, sizeof(status));
  if (report) *report = rep;
  for (int k = 0; k < ZKFL_KEYCHECK_N; k++) {
    if (status[k] != ZKFL_KEYCHECK_FAIL) continue;
    std::string msg = std::string("zkey check: ") + CHECK_NAMES[k] + " fails";
    if (k == ZKFL_KEYCHECK_HEADER) msg += ": " + header_why;
    if (k == ZKFL_KEYCHECK_POINTS)
      msg += ": section " + std::to_string(rep.point_section) + " point " + std::to_string(rep.point_index) +
             " is not a point of its group (" + std::to_string(rep.point_count) + " in the section)";
    if (k == ZKFL_KEYCHECK_COEFFICIENTS)
      msg += ": matrix " + std::to_string(rep.coef_matrix) + " row " + std::to_string(rep.coef_row) + " differs from the r1cs (" +
             std::to_string(rep.coef_count) + " rows differ)";
    return fail(ZKFL_E_KEY, msg);
  }
  return ZKFL_OK;
}
