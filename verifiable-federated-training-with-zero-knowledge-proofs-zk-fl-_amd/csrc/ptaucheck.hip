// The ptau check: kernels and the two entry points (see ptaucheck.h; include/zkfl.h has the
// equations).  The reference takes whatever pot17_final.ptau / pot14_final.ptau it finds
// (tests/full_system_simulation.mjs:677-695); this is the call that tests such a file first.
#include "ptaucheck.h"

#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <string>
#include <vector>

#include "common.h"
#include "devbufs.h"
#include "fr_consts.h"
#include "host_parse.h"
#include "objects.h"
#include "pairing.h"
#include "pointcheck.h"
#include "verify.h"
#include "verify_dev.h"

using namespace zkfl;

namespace {

// ---------------------------------------------------------------------------
// Host arithmetic mod r and mod q (Montgomery, R = 2^256, 4 x 64-bit limbs: the device's Fp<> bytes).
// A few hundred multiplications per call: the per-level factors and the generators' encodings.
// ---------------------------------------------------------------------------
using u128 = unsigned __int128;

struct HMod {
  uint64_t p[4], inv;  // inv = -p^-1 mod 2^64
  uint64_t r2[4];      // 2^512 mod p
};

HMod hmod_of(const uint32_t P[8], const uint32_t R2[8]) {
  HMod m;
  for (int i = 0; i < 4; i++) {
    m.p[i] = (uint64_t)P[2 * i] | ((uint64_t)P[2 * i + 1] << 32);
    m.r2[i] = (uint64_t)R2[2 * i] | ((uint64_t)R2[2 * i + 1] << 32);
  }
  uint64_t x = 1;  // Newton: x = p^-1 mod 2^64
  for (int i = 0; i < 6; i++) x *= 2 - m.p[0] * x;
  m.inv = ~x + 1;
  return m;
}

struct HF {
  uint64_t w[4];
  bool operator==(const HF& o) const { return memcmp(w, o.w, 32) == 0; }
  bool operator!=(const HF& o) const { return !(*this == o); }
};

bool h_geq(const uint64_t a[4], const uint64_t b[4]) {
  for (int i = 3; i >= 0; i--)
    if (a[i] != b[i]) return a[i] > b[i];
  return true;
}

void h_sub_raw(uint64_t a[4], const uint64_t b[4]) {
  uint64_t borrow = 0;
  for (int i = 0; i < 4; i++) {
    const u128 d = (u128)a[i] - b[i] - borrow;
    a[i] = (uint64_t)d;
    borrow = (uint64_t)(d >> 64) & 1;
  }
}

// a b 2^-256 mod p (CIOS); a, b < p < 2^254, so the result before the last subtraction is < 2p
HF h_mul(const HMod& m, const HF& a, const HF& b) {
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) {
      c += (u128)a.w[j] * b.w[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t q = t[0] * m.inv;
    c = (u128)q * m.p[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; j++) {
      c += (u128)q * m.p[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  HF r = {{t[0], t[1], t[2], t[3]}};
  if (t[4] || h_geq(r.w, m.p)) h_sub_raw(r.w, m.p);
  return r;
}

HF h_add(const HMod& m, const HF& a, const HF& b) {
  HF r;
  u128 c = 0;
  for (int i = 0; i < 4; i++) {
    c += (u128)a.w[i] + b.w[i];
    r.w[i] = (uint64_t)c;
    c >>= 64;
  }
  if (h_geq(r.w, m.p)) h_sub_raw(r.w, m.p);  // a + b < 2^255: no carry out
  return r;
}

HF h_sub(const HMod& m, const HF& a, const HF& b) {
  HF r = a;
  if (!h_geq(a.w, b.w)) {  // a + p - b
    u128 c = 0;
    for (int i = 0; i < 4; i++) {
      c += (u128)r.w[i] + m.p[i];
      r.w[i] = (uint64_t)c;
      c >>= 64;
    }
  }
  h_sub_raw(r.w, b.w);
  return r;
}

HF h_from_std(const HMod& m, const uint8_t* b) {
  HF a, r2;
  memcpy(a.w, b, 32);
  memcpy(r2.w, m.r2, 32);
  return h_mul(m, a, r2);
}

HF h_one(const HMod& m) {
  HF one = {{1, 0, 0, 0}}, r2;
  memcpy(r2.w, m.r2, 32);
  return h_mul(m, one, r2);
}

HF h_inv(const HMod& m, const HF& a) {  // a^(p - 2)
  uint64_t e[4] = {m.p[0] - 2, m.p[1], m.p[2], m.p[3]};  // p is odd and > 2: no borrow
  HF r = h_one(m);
  for (int i = 255; i >= 0; i--) {
    r = h_mul(m, r, r);
    if ((e[i / 64] >> (i % 64)) & 1) r = h_mul(m, r, a);
  }
  return r;
}

// ---------------------------------------------------------------------------
// Device
// ---------------------------------------------------------------------------
// What the scalar kernels read, Montgomery Fr.  c[k] = gamma_k (z^n_k - 1) / n_k, w[k] = the level's
// generator; suf[t][b] = sum_{k >= b} gamma_k z^n_k / n_k and s0[t] = sum_k gamma_k / n_k over the
// levels of table t (0: up to power + 1, sections 2 / 12; 1: up to power, the others), so that
// s_i = zinv^i suf[bitlength(i)]: 2^k > i exactly when k >= bitlength(i).
struct PtauLevels {
  Fr z, zinv;
  Fr c[PTAU_MAX_LEVELS], w[PTAU_MAX_LEVELS];
  Fr suf[2][PTAU_MAX_LEVELS + 2], s0[2];
};

// a^e, e < 2^32
ZK_DEV Fr fr_pow_u32(const Fr& a, uint32_t e) {
  Fr r = fp_one<FrP>();
  if (!e) return r;
#pragma unroll 1
  for (int b = 31 - __clz((int)e); b >= 0; b--) {
    r = fp_sqr(r);
    if ((e >> b) & 1u) r = fp_mul(r, a);
  }
  return r;
}

// out[t] = lam of position q0 + t of a Lagrange section, t < cnt, std form.  A lane owns PTAU_RUN
// consecutive positions: w_k^j by one power and running products (restarting at 1 where the run
// enters the next level), the denominators z - w_k^j inverted together.
__global__ void __launch_bounds__(256) k_ptau_lam(const PtauLevels* __restrict__ L, uint32_t q0, uint32_t cnt,
                                                  Fr* __restrict__ out) {
  const uint32_t t0 = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)PTAU_RUN;
  if (t0 >= cnt) return;
  const uint32_t m = cnt - t0 < (uint32_t)PTAU_RUN ? cnt - t0 : (uint32_t)PTAU_RUN;
  uint32_t q = q0 + t0;
  uint32_t k = 31u - (uint32_t)__clz((int)(q + 1));
  const Fr z = L->z, one = fp_one<FrP>();
  Fr w = L->w[k];
  Fr x = fr_pow_u32(w, q + 1 - (1u << k));
  Fr den[PTAU_RUN], pre[PTAU_RUN];  // the numerator is recomputed from den: c[k] (z - den)
  uint32_t lvl[PTAU_RUN];
  Fr acc = one;
#pragma unroll
  for (int t = 0; t < PTAU_RUN; t++) {
    den[t] = one;
    pre[t] = acc;
    lvl[t] = k;
    if ((uint32_t)t < m) {
      den[t] = fp_sub(z, x);
      acc = fp_mul(acc, den[t]);
      q++;
      if (((q + 1) & q) == 0) {  // q + 1 is a power of two: the next level's first position
        k++;
        x = one;
        if ((uint32_t)t + 1 < m) w = L->w[k];
      } else {
        x = fp_mul(x, w);
      }
    }
  }
  Fr inv = fp_inv(acc);
#pragma unroll
  for (int t = PTAU_RUN - 1; t >= 0; t--) {
    if ((uint32_t)t < m) {
      const Fr dinv = fp_mul(inv, pre[t]);
      inv = fp_mul(inv, den[t]);
      out[t0 + t] = fp_from_mont(fp_mul(fp_mul(L->c[lvl[t]], fp_sub(z, den[t])), dinv));
    }
  }
}

// out[t] = s of index i0 + t of a power section, t < cnt, std form: zinv^i by one power per lane
// and running products, times the host's suffix sum for bitlength(i); s_0 is the table's s0.
__global__ void __launch_bounds__(256) k_ptau_s(const PtauLevels* __restrict__ L, int tab, uint32_t i0, uint32_t cnt,
                                                Fr* __restrict__ out) {
  const uint32_t t0 = (blockIdx.x * 256u + threadIdx.x) * (uint32_t)PTAU_RUN;
  if (t0 >= cnt) return;
  const uint32_t m = cnt - t0 < (uint32_t)PTAU_RUN ? cnt - t0 : (uint32_t)PTAU_RUN;
  const Fr zinv = L->zinv;
  Fr x = fr_pow_u32(zinv, i0 + t0);
#pragma unroll 1
  for (uint32_t t = 0; t < m; t++) {
    const uint32_t i = i0 + t0 + t;
    const Fr v = i ? fp_mul(x, L->suf[tab][32 - __clz((int)i)]) : L->s0[tab];
    out[t0 + t] = fp_from_mont(v);
    x = fp_mul(x, zinv);
  }
}

// acc += part (one chunk's partial MSM result into its combination)
template <class F>
__global__ void __launch_bounds__(64) k_ptau_add(XYZZ<F>* __restrict__ acc, const XYZZ<F>* __restrict__ part) {
  if (threadIdx.x == 0) *acc = xyzz_add<F>(*acc, *part);
}

// the combinations, by slot: X0 = S0(X), X1 = S1(X), LX = MSM(Lagrange section, lam), SX = MSM(X, s)
enum { R_T0, R_T1, R_A0, R_A1, R_B0, R_B1, R_LT, R_ST, R_LA, R_SA, R_LB, R_SB, R_N };
enum { S_U0, S_U1, S_LU, S_SU, S_N };
constexpr int N_PAIRS = 10;

// After the last chunk, one lane per task: lanes 0-3 compare the Lagrange pairs of sections 12, 13,
// 14, 15; lanes 4-13 write pair t - 4 of the pairing batch (std affine):
//   0 e(S0(T), U[1])   1 e(S1(T), G2)    2 e(T[1], S0(U))   3 e(G1, S1(U))
//   4 e(S0(A), U[1])   5 e(S1(A), G2)    6 e(S0(B), U[1])   7 e(S1(B), G2)
//   8 e(B[0], G2)      9 e(G1, b2)
// hdr1 = T[1] | B[0], hdr2 = U[1] | b2 (Montgomery, zeroed by the host when their section is unusable).
__global__ void __launch_bounds__(64) k_ptau_finish(const G1P* __restrict__ R, const G2P* __restrict__ S,
                                                    const G1Aff* __restrict__ hdr1, const G2Aff* __restrict__ hdr2,
                                                    uint32_t* __restrict__ same, uint32_t* __restrict__ g1_out,
                                                    uint32_t* __restrict__ g2_out) {
  const int t = threadIdx.x;
  if (t == 0) same[0] = xyzz_same<FqOps>(R[R_LT], R[R_ST]);
  if (t == 1) same[1] = xyzz_same<Fq2Ops>(S[S_LU], S[S_SU]);
  if (t == 2) same[2] = xyzz_same<FqOps>(R[R_LA], R[R_SA]);
  if (t == 3) same[3] = xyzz_same<FqOps>(R[R_LB], R[R_SB]);
  if (t < 4 || t >= 4 + N_PAIRS) return;
  const int p = t - 4;
  G1Aff P = g1_generator();
  G2Aff Q = g2_generator();
  switch (p) {
    case 0: P = xyzz_to_affine<FqOps>(R[R_T0]); Q = hdr2[0]; break;
    case 1: P = xyzz_to_affine<FqOps>(R[R_T1]); break;
    case 2: P = hdr1[0]; Q = xyzz_to_affine<Fq2Ops>(S[S_U0]); break;
    case 3: Q = xyzz_to_affine<Fq2Ops>(S[S_U1]); break;
    case 4: P = xyzz_to_affine<FqOps>(R[R_A0]); Q = hdr2[0]; break;
    case 5: P = xyzz_to_affine<FqOps>(R[R_A1]); break;
    case 6: P = xyzz_to_affine<FqOps>(R[R_B0]); Q = hdr2[0]; break;
    case 7: P = xyzz_to_affine<FqOps>(R[R_B1]); break;
    case 8: P = hdr1[1]; break;
    default: Q = hdr2[1]; break;
  }
  store_std(P, g1_out + p * 16);
  store_std(Q, g2_out + p * 32);
}

bool nonzero(const uint8_t* p, size_t len) {
  for (size_t i = 0; i < len; i++)
    if (p[i]) return true;
  return false;
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

// One curve's engine, sized for one chunk: the chunk's points, the expanded base set, the MSM
// scratch and the partial result.
template <class F>
struct Engine {
  size_t cap = 0;
  Affine<F>* d_pts = nullptr;
  XYZZ<F>* d_part = nullptr;
  MsmBases<F> mb;
  MsmScratch<F> s;
  MsmTail<F> t;
  ~Engine() {
    msm_bases_free(mb);
    msm_scratch_free(s);
    msm_tail_free(t);
  }
  hipError_t alloc(DevBufs& D, size_t cap_, int c, hipStream_t st) {
    cap = cap_;
    ZK_CHECK(D.get(&d_pts, cap));
    ZK_CHECK(D.get(&d_part, 1));
    ZK_CHECK(msm_bases_alloc(mb, cap, c));
    ZK_CHECK(msm_scratch_alloc(s, cap, c, st));
    ZK_CHECK(msm_tail_alloc(t, cap, c));
    return hipSuccess;
  }
  // the kept points of this chunk as the base set (d_pts holds n of them)
  hipError_t set(size_t n, const uint32_t* h_sidx, hipStream_t st) {
    if (mb.sidx) {
      ZK_CHECK(hipFree(mb.sidx));
      mb.sidx = nullptr;
    }
    mb.n = n;
    return msm_bases_set(mb, d_pts, h_sidx, 0xFFFFFFFFu, st);
  }
  // acc += MSM(base set, scalars)
  hipError_t run(const Fr* scalars, XYZZ<F>* acc, hipStream_t st) {
    ZK_CHECK(msm_run(mb, s, t, reinterpret_cast<const uint32_t*>(scalars), nullptr, d_part, st, nullptr, ""));
    hipLaunchKernelGGL(k_ptau_add<F>, dim3(1), dim3(64), 0, st, acc, (const XYZZ<F>*)d_part);
    return hipGetLastError();
  }
};

const char* const CHECK_NAMES[ZKFL_PTAUCHECK_N] = {"STRUCTURE", "POINTS",  "TAU_G1",   "TAU_G2",   "ALPHA_G1",  "BETA_G1",
                                                   "BETA_G2",   "L_TAU_G1", "L_TAU_G2", "L_ALPHA_G1", "L_BETA_G1"};

// what one section leaves behind
struct SecState {
  bool clean = true;          // no bad point so far
  uint32_t first = 0, n_bad = 0;
};

// The state of one call that the per-section walk shares.
struct Walk {
  zkfl_ctx* ctx;
  hipStream_t st;
  uint32_t chunk;
  const uint8_t* rho;       // 2n - 1 scalars, std
  const PtauLevels* d_lev;
  Fr *d_stage, *d_sl;       // rho[a-1 .. b) of the chunk (chunk + 1 entries) | s or lam (chunk entries)
  KeyVerdict* d_v;
  std::vector<uint8_t> img, stage;
  std::vector<uint32_t> sidx;
  uint32_t chunks = 0;
};

// One section through the device, chunk by chunk.  Power sections (lagrange = false): acc0 += S0
// part, acc1 += S1 part, and with accL (a prepared file) accL += MSM(chunk, s) from table tab.
// Lagrange sections: accL += MSM(chunk, lam).  msm = false (the partner section is unusable): the
// points are still checked.  Returns a ZKFL code; S records the section's bad points.
template <class F>
int walk_section(Walk& W, Engine<F>& E, const uint8_t* sec, size_t cnt, bool lagrange, int tab, bool msm,
                 XYZZ<F>* acc0, XYZZ<F>* acc1, XYZZ<F>* accL, SecState& S) {
  constexpr size_t psz = sizeof(Affine<F>);
  constexpr int PB = PointsBlock<F>::N;
  hipStream_t st = W.st;
  Profiler& prof = W.ctx->prof;
  for (size_t a = 0; a < cnt; a += W.chunk) {
    const size_t m = std::min<size_t>(W.chunk, cnt - a);
    W.chunks++;
    W.img.clear();
    W.sidx.clear();
    for (size_t i = 0; i < m; i++) {
      const uint8_t* q = sec + (a + i) * psz;
      if (!nonzero(q, psz)) continue;
      W.img.insert(W.img.end(), q, q + psz);
      W.sidx.push_back((uint32_t)i);
    }
    const size_t kept = W.sidx.size();
    if (!kept) continue;  // a chunk of infinities adds nothing
    const KeyVerdict init = {0, VERDICT_NONE};
    KeyVerdict v;
    HIP_TRY(hipMemcpyAsync(W.d_v, &init, sizeof(init), hipMemcpyHostToDevice, st), "upload");
    HIP_TRY(hipMemcpyAsync(E.d_pts, W.img.data(), W.img.size(), hipMemcpyHostToDevice, st), "upload");
    int pi = prof.begin("ptaucheck_points", st);
    hipLaunchKernelGGL(k_points_check<F>, dim3(zk_grid(kept, PB)), dim3(PB), 0, st, (const Affine<F>*)E.d_pts,
                       (uint32_t)kept, W.d_v);
    HIP_TRY(hipGetLastError(), "points check launch");
    prof.end(pi, st, (double)kept);
    HIP_TRY(hipMemcpyAsync(&v, W.d_v, sizeof(v), hipMemcpyDeviceToHost, st), "verdict");
    HIP_TRY(hipStreamSynchronize(st), "points check");
    if (v.n_bad) {
      if (S.clean) S.first = (uint32_t)a + W.sidx[v.first];
      S.clean = false;
      S.n_bad += v.n_bad;
    }
    if (!S.clean || !msm) continue;

    // ---- scalars ----
    pi = prof.begin("ptaucheck_scalars", st);
    if (!lagrange) {
      // stage[0] = rho[a - 1] (0 at a = 0), stage[1 + t] = rho[a + t] while a + t < cnt - 1, else 0:
      // S1's scalars are stage[0 .. m), S0's are stage[1 .. m]
      W.stage.assign(32 * (m + 1), 0);
      if (a) memcpy(W.stage.data(), W.rho + 32 * (a - 1), 32);
      const size_t live = std::min(m, cnt - 1 - a);
      memcpy(W.stage.data() + 32, W.rho + 32 * a, 32 * live);
      HIP_TRY(hipMemcpyAsync(W.d_stage, W.stage.data(), W.stage.size(), hipMemcpyHostToDevice, st), "upload");
      if (accL)
        hipLaunchKernelGGL(k_ptau_s, dim3(zk_grid(zk_grid(m, PTAU_RUN), 256)), dim3(256), 0, st, W.d_lev, tab, (uint32_t)a,
                           (uint32_t)m, W.d_sl);
    } else {
      hipLaunchKernelGGL(k_ptau_lam, dim3(zk_grid(zk_grid(m, PTAU_RUN), 256)), dim3(256), 0, st, W.d_lev, (uint32_t)a,
                         (uint32_t)m, W.d_sl);
    }
    HIP_TRY(hipGetLastError(), "scalar kernel launch");
    prof.end(pi, st, (double)m);

    // ---- MSMs: one base set, two or three scalar vectors ----
    pi = prof.begin("ptaucheck_msm", st);
    HIP_TRY(E.set(kept, W.sidx.data(), st), "ptau check bases");
    if (!lagrange) {
      HIP_TRY(E.run(W.d_stage + 1, acc0, st), "ptau check MSM");
      HIP_TRY(E.run(W.d_stage, acc1, st), "ptau check MSM");
    }
    if (accL) HIP_TRY(E.run(W.d_sl, accL, st), "ptau check MSM");
    prof.end(pi, st, (double)kept);
    HIP_TRY(hipStreamSynchronize(st), "ptau check chunk");  // img, sidx and stage are reused by the next chunk
  }
  return ZKFL_OK;
}

}  // namespace

extern "C" int zkfl_ptau_parse(const uint8_t* buf, size_t len, zkfl_ptau_header* out) {
  if (!buf) return fail(ZKFL_E_ARG, "null argument");
  PtauHost p;
  std::string err;
  const int rc = ptau_parse(buf, len, p, err);
  if (rc) return fail(rc, err);
  if (out) {
    out->power = p.power;
    out->ceremony_power = p.ceremony_power;
    out->prepared = p.prepared ? 1 : 0;
    out->contributions = p.contributions;
  }
  return ZKFL_OK;
}

extern "C" int zkfl_ptau_check(zkfl_ctx* ctx, const uint8_t* ptau, size_t len, const uint8_t* rnd_in,
                               uint32_t chunk_points, zkfl_ptau_report* report) {
  if (!ctx || !ptau) return fail(ZKFL_E_ARG, "null argument");
  PtauHost pt;
  {
    std::string err;
    const int rc = ptau_parse(ptau, len, pt, err);
    if (rc) return fail(rc, err);
  }
  const uint32_t power = pt.power;
  const size_t n = (size_t)1 << power;
  if (pt.prepared && power + 1 > 28)
    return fail(ZKFL_E_ARG, "ptau check: a prepared file of power 28 needs a 2^29 domain, which Fr does not have");
  const int top = (int)power + 1;  // levels 0 .. top
  const size_t n_rnd = 1 + (size_t)(top + 1) + (2 * n - 1);

  // ---- randomness: z | gamma[power + 2] | rho[2n - 1] ----
  const HMod MR = hmod_of(FrP::P, FrP::R2), MQ = hmod_of(FqP::P, FqP::R2);
  const HF one = h_one(MR);
  std::vector<uint8_t> rnd;
  HF zp[PTAU_MAX_LEVELS];  // z^(2^k), Montgomery
  auto z_powers = [&](const uint8_t* z) {
    zp[0] = h_from_std(MR, z);
    for (int k = 1; k <= top; k++) zp[k] = h_mul(MR, zp[k - 1], zp[k - 1]);
    return nonzero(z, 32) && zp[top] != one;  // z != 0 and z^(2n) != 1
  };
  if (rnd_in) {
    for (size_t i = 0; i < n_rnd; i++) {
      uint32_t w[8];
      memcpy(w, rnd_in + 32 * i, 32);
      if (!fr_lt_r(w)) return fail(ZKFL_E_ARG, "ptau check: scalar " + std::to_string(i) + " of rnd is not < r");
    }
    if (!z_powers(rnd_in)) return fail(ZKFL_E_ARG, "ptau check: z is zero or lies on the 2n domain");
  } else {
    rnd.resize(32 * n_rnd);
    int rc = draw_fr(rnd.data(), n_rnd);
    if (rc) return rc;
    for (int tries = 0; !z_powers(rnd.data()); tries++) {
      if (tries > 64) return fail(ZKFL_E_DEVICE, "rng");
      rc = draw_fr(rnd.data(), 1);
      if (rc) return rc;
    }
  }
  const uint8_t* rv = rnd_in ? rnd_in : rnd.data();
  const uint8_t *gamma = rv + 32, *rho = rv + 32 * (size_t)(top + 2);

  // ---- the per-level factors and their suffix sums ----
  PtauLevels lev;
  memset(&lev, 0, sizeof(lev));
  {
    auto put = [](Fr& d, const HF& s) { memcpy(d.v, s.w, 32); };
    put(lev.z, zp[0]);
    put(lev.zinv, h_inv(MR, zp[0]));
    HF g[PTAU_MAX_LEVELS], gz[PTAU_MAX_LEVELS];  // gamma_k / n_k, gamma_k z^n_k / n_k
    for (int k = 0; k <= top && k <= 28; k++) {
      const HF ninv = h_from_std(MR, reinterpret_cast<const uint8_t*>(FR_INV_2K[k]));
      g[k] = h_mul(MR, h_from_std(MR, gamma + 32 * k), ninv);
      gz[k] = h_mul(MR, g[k], zp[k]);
      put(lev.c[k], h_sub(MR, gz[k], g[k]));
      put(lev.w[k], h_from_std(MR, reinterpret_cast<const uint8_t*>(FR_ROOT[k])));
    }
    for (int tab = 0; tab < 2; tab++) {
      const int last = std::min(tab == 0 ? top : top - 1, 28);
      HF suf = {{0, 0, 0, 0}}, s0 = suf;
      for (int k = last; k >= 0; k--) {
        suf = h_add(MR, suf, gz[k]);
        s0 = h_add(MR, s0, g[k]);
        put(lev.suf[tab][k], suf);
      }
      put(lev.s0[tab], s0);
    }
  }

  uint32_t status[ZKFL_PTAUCHECK_N];
  for (uint32_t& s : status) s = ZKFL_PTAUCHECK_PASS;
  zkfl_ptau_report rep = {};
  rep.prepared = pt.prepared ? 1 : 0;
  rep.power = power;

  // ---- STRUCTURE (host) ----
  const uint8_t *T = pt.sec[2], *U = pt.sec[3], *A = pt.sec[4], *B = pt.sec[5], *b2 = pt.sec[6];
  std::string structure_why;
  {
    uint8_t g1[64], g2[128];
    const HF q1 = h_one(MQ), q2 = h_add(MQ, q1, q1);
    memcpy(g1, q1.w, 32);
    memcpy(g1 + 32, q2.w, 32);
    static const uint32_t G2_STD[4][8] = {
        {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu},
        {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u},
        {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u},
        {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u}};
    for (int i = 0; i < 4; i++) {
      const HF c = h_from_std(MQ, reinterpret_cast<const uint8_t*>(G2_STD[i]));
      memcpy(g2 + 32 * i, c.w, 32);
    }
    if (memcmp(T, g1, 64) != 0) structure_why = "tauG1[0] is not the G1 generator";
    else if (memcmp(U, g2, 128) != 0) structure_why = "tauG2[0] is not the G2 generator";
    else if (!nonzero(T + 64, 64)) structure_why = "tauG1[1] is infinity";
    else if (!nonzero(A, 64)) structure_why = "alphaTauG1[0] is infinity";
    else if (!nonzero(B, 64)) structure_why = "betaTauG1[0] is infinity";
    else if (!nonzero(b2, 128)) structure_why = "betaG2 is infinity";
  }

  // ---- device ----
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  DevBufs D;
  const uint32_t chunk = chunk_points ? chunk_points : PTAU_CHUNK_DEFAULT;
  const size_t most1 = pt.prepared ? 4 * n - 1 : 2 * n - 1, most2 = pt.prepared ? 2 * n - 1 : n;
  const size_t cap1 = std::min<size_t>(chunk, most1), cap2 = std::min<size_t>(chunk, most2);
  const int c = msm_pick_c(std::max(cap1, cap2));
  Engine<FqOps> E1;
  Engine<Fq2Ops> E2;
  HIP_TRY(E1.alloc(D, cap1, c, st), "ptau check engine");
  HIP_TRY(E2.alloc(D, cap2, c, st), "ptau check engine");
  Walk W;
  W.ctx = ctx;
  W.st = st;
  W.chunk = chunk;
  W.rho = rho;
  PtauLevels* d_lev;
  G1P* d_R;
  G2P* d_S;
  HIP_TRY(D.get(&d_lev, 1), "alloc");
  HIP_TRY(D.get(&W.d_stage, cap1 + 1), "alloc");
  HIP_TRY(D.get(&W.d_sl, cap1), "alloc");
  HIP_TRY(D.get(&W.d_v, 1), "alloc");
  HIP_TRY(D.get(&d_R, R_N), "alloc");
  HIP_TRY(D.get(&d_S, S_N), "alloc");
  W.d_lev = d_lev;
  HIP_TRY(hipMemcpyAsync(d_lev, &lev, sizeof(lev), hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemsetAsync(d_R, 0, R_N * sizeof(G1P), st), "memset");  // ZZ = 0: infinity
  HIP_TRY(hipMemsetAsync(d_S, 0, S_N * sizeof(G2P), st), "memset");
  HIP_TRY(hipStreamSynchronize(st), "sync");

  // the sections in file order; a section whose partner in a Lagrange pair is already known to be
  // unusable keeps its point check and drops its MSMs
  SecState S[16];
  const bool prep = pt.prepared;
  int rc;
  if ((rc = walk_section<FqOps>(W, E1, T, pt.cnt[2], false, 0, true, d_R + R_T0, d_R + R_T1, prep ? d_R + R_ST : nullptr, S[2]))) return rc;
  if ((rc = walk_section<Fq2Ops>(W, E2, U, pt.cnt[3], false, 1, true, d_S + S_U0, d_S + S_U1, prep ? d_S + S_SU : nullptr, S[3]))) return rc;
  if ((rc = walk_section<FqOps>(W, E1, A, pt.cnt[4], false, 1, true, d_R + R_A0, d_R + R_A1, prep ? d_R + R_SA : nullptr, S[4]))) return rc;
  if ((rc = walk_section<FqOps>(W, E1, B, pt.cnt[5], false, 1, true, d_R + R_B0, d_R + R_B1, prep ? d_R + R_SB : nullptr, S[5]))) return rc;
  if ((rc = walk_section<Fq2Ops>(W, E2, b2, 1, true, 0, false, nullptr, nullptr, nullptr, S[6]))) return rc;
  if (prep) {
    if ((rc = walk_section<FqOps>(W, E1, pt.sec[12], pt.cnt[12], true, 0, S[2].clean, nullptr, nullptr, d_R + R_LT, S[12]))) return rc;
    if ((rc = walk_section<Fq2Ops>(W, E2, pt.sec[13], pt.cnt[13], true, 1, S[3].clean, nullptr, nullptr, d_S + S_LU, S[13]))) return rc;
    if ((rc = walk_section<FqOps>(W, E1, pt.sec[14], pt.cnt[14], true, 1, S[4].clean, nullptr, nullptr, d_R + R_LA, S[14]))) return rc;
    if ((rc = walk_section<FqOps>(W, E1, pt.sec[15], pt.cnt[15], true, 1, S[5].clean, nullptr, nullptr, d_R + R_LB, S[15]))) return rc;
  }
  rep.chunks = W.chunks;
  for (int t : {2, 3, 4, 5, 6, 12, 13, 14, 15}) {
    if (S[t].clean) continue;
    status[ZKFL_PTAUCHECK_POINTS] = ZKFL_PTAUCHECK_FAIL;
    rep.point_section = (uint32_t)t;
    rep.point_index = S[t].first;
    rep.point_count = S[t].n_bad;
    break;
  }

  // ---- pairings ----
  int pi = ctx->prof.begin("ptaucheck_pairing", st);
  uint8_t hdr1_img[2 * 64], hdr2_img[2 * 128];
  memset(hdr1_img, 0, sizeof(hdr1_img));
  memset(hdr2_img, 0, sizeof(hdr2_img));
  if (S[2].clean) memcpy(hdr1_img, T + 64, 64);
  if (S[5].clean) memcpy(hdr1_img + 64, B, 64);
  if (S[3].clean) memcpy(hdr2_img, U + 128, 128);
  if (S[6].clean) memcpy(hdr2_img + 128, b2, 128);
  G1Aff* d_hdr1;
  G2Aff* d_hdr2;
  uint32_t *d_same, *d_g1, *d_g2;
  HIP_TRY(D.get(&d_hdr1, 2), "alloc");
  HIP_TRY(D.get(&d_hdr2, 2), "alloc");
  HIP_TRY(D.get(&d_same, 4), "alloc");
  HIP_TRY(D.get(&d_g1, N_PAIRS * 16), "alloc");
  HIP_TRY(D.get(&d_g2, N_PAIRS * 32), "alloc");
  HIP_TRY(hipMemcpyAsync(d_hdr1, hdr1_img, sizeof(hdr1_img), hipMemcpyHostToDevice, st), "upload");
  HIP_TRY(hipMemcpyAsync(d_hdr2, hdr2_img, sizeof(hdr2_img), hipMemcpyHostToDevice, st), "upload");
  hipLaunchKernelGGL(k_ptau_finish, dim3(1), dim3(64), 0, st, (const G1P*)d_R, (const G2P*)d_S, (const G1Aff*)d_hdr1,
                     (const G2Aff*)d_hdr2, d_same, d_g1, d_g2);
  HIP_TRY(hipGetLastError(), "ptau finish launch");
  uint32_t same[4];
  uint8_t g1b[N_PAIRS * 64], g2b[N_PAIRS * 128];
  HIP_TRY(hipMemcpyAsync(same, d_same, sizeof(same), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipMemcpyAsync(g1b, d_g1, sizeof(g1b), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipMemcpyAsync(g2b, d_g2, sizeof(g2b), hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipStreamSynchronize(st), "ptau check");
  std::vector<uint8_t> gt(N_PAIRS * 384);
  {
    std::string err;
    const int prc = pairing_batch(N_PAIRS, g1b, g2b, 1, gt.data(), st, err);
    if (prc) return fail(prc == ZKFL_E_ARG ? ZKFL_E_DEVICE : prc, "ptau check pairing: " + err);
  }
  ctx->prof.end(pi, st, (double)N_PAIRS);
  auto gt_same = [&](int i) { return memcmp(gt.data() + 384 * (size_t)(2 * i), gt.data() + 384 * (size_t)(2 * i + 1), 384) == 0; };

  // ---- verdicts ----
  if (!structure_why.empty()) status[ZKFL_PTAUCHECK_STRUCTURE] = ZKFL_PTAUCHECK_FAIL;
  auto set = [&](int check, bool ran, bool holds) {
    status[check] = !ran ? ZKFL_PTAUCHECK_NOT_RUN : holds ? ZKFL_PTAUCHECK_PASS : ZKFL_PTAUCHECK_FAIL;
  };
  set(ZKFL_PTAUCHECK_TAU_G1, S[2].clean && S[3].clean, gt_same(0));
  set(ZKFL_PTAUCHECK_TAU_G2, S[2].clean && S[3].clean, gt_same(1));
  set(ZKFL_PTAUCHECK_ALPHA_G1, S[4].clean && S[3].clean, gt_same(2));
  set(ZKFL_PTAUCHECK_BETA_G1, S[5].clean && S[3].clean, gt_same(3));
  set(ZKFL_PTAUCHECK_BETA_G2, S[5].clean && S[6].clean, gt_same(4));
  set(ZKFL_PTAUCHECK_L_TAU_G1, prep && S[2].clean && S[12].clean, same[0] != 0);
  set(ZKFL_PTAUCHECK_L_TAU_G2, prep && S[3].clean && S[13].clean, same[1] != 0);
  set(ZKFL_PTAUCHECK_L_ALPHA_G1, prep && S[4].clean && S[14].clean, same[2] != 0);
  set(ZKFL_PTAUCHECK_L_BETA_G1, prep && S[5].clean && S[15].clean, same[3] != 0);
  memcpy(rep.status, status, sizeof(status));
  if (report) *report = rep;
  for (int k = 0; k < ZKFL_PTAUCHECK_N; k++) {
    if (status[k] != ZKFL_PTAUCHECK_FAIL) continue;
    std::string msg = std::string("powersoftau check: ") + CHECK_NAMES[k] + " fails";
    if (k == ZKFL_PTAUCHECK_STRUCTURE) msg += ": " + structure_why;
    if (k == ZKFL_PTAUCHECK_POINTS)
      msg += ": section " + std::to_string(rep.point_section) + " point " + std::to_string(rep.point_index) +
             " is not a point of its group (" + std::to_string(rep.point_count) + " in the section)";
    return fail(ZKFL_E_KEY, msg);
  }
  return ZKFL_OK;
}
