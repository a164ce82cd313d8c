// Device code the file checks share (csrc/keycheck.hip, csrc/ptaucheck.hip): is a stored point a
// point of its group, the counted verdict's reduction, projective equality and the std-form store
// of a pairing input.  Device only; every unit that includes it compiles its own copy.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "curve.h"
#include "field.h"
#include "pairing.h"
#include "verify_dev.h"

namespace zkfl {

// a counted verdict as the device leaves it: how many items failed and the lowest of them
struct KeyVerdict {
  uint32_t n_bad, first;
};

constexpr uint32_t VERDICT_NONE = 0xFFFFFFFFu;

// Failures counted and the lowest index kept: wave ballot, LDS, one atomic pair per workgroup that
// saw one (k_r1cs_verdict's reduction).  Sums and minima commute, so the outcome does not depend on
// the workgroups' order.  Every thread of the block calls it; a lane's item is blockIdx.x * BLOCK +
// threadIdx.x.
template <int BLOCK>
__device__ __forceinline__ void verdict_reduce(bool bad, KeyVerdict* __restrict__ v) {
  constexpr int WAVES = BLOCK / 64;
  __shared__ uint32_t s_cnt[WAVES], s_first[WAVES];
  const uint64_t bal = __ballot(bad);
  const uint32_t wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    s_cnt[wave] = (uint32_t)__popcll((unsigned long long)bal);
    s_first[wave] =
        bal ? blockIdx.x * (uint32_t)BLOCK + wave * 64u + (uint32_t)(__ffsll((unsigned long long)bal) - 1) : VERDICT_NONE;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t cnt = 0, first = VERDICT_NONE;
    for (int q = 0; q < WAVES; q++) {
      cnt += s_cnt[q];
      first = s_first[q] < first ? s_first[q] : first;
    }
    if (cnt) {
      atomicAdd(&v->n_bad, cnt);
      atomicMin(&v->first, first);
    }
  }
}

// A point as a .zkey or .ptau stores it (Montgomery affine): all-zero is infinity; otherwise the
// coordinates must be canonical and satisfy the curve equation -- the MSM formulas never read the
// curve's b, so an off-curve point would be added silently -- and a twist point must lie in the
// order-r subgroup (G2's cofactor is large: a random combination can miss a small-order part).
ZK_DEV bool point_ok(const G1Aff& p) {
  if (aff_is_inf(p)) return true;
  if (!lt_mod(p.x.v, FqP::P) || !lt_mod(p.y.v, FqP::P)) return false;
  return fp_eq(fp_sqr(p.y), fp_add(fp_mul(fp_sqr(p.x), p.x), fq_small(3)));
}

ZK_DEV bool point_ok(const G2Aff& q) {
  if (aff_is_inf(q)) return true;
  if (!lt_mod(q.x.c0.v, FqP::P) || !lt_mod(q.x.c1.v, FqP::P) || !lt_mod(q.y.c0.v, FqP::P) ||
      !lt_mod(q.y.c1.v, FqP::P))
    return false;
  if (!f2_eq(f2_sqr(q.y), f2_add(f2_mul(f2_sqr(q.x), q.x), load_fq2(TWIST_B)))) return false;
  const uint32_t u[8] = {(uint32_t)BN_U, (uint32_t)(BN_U >> 32), 0, 0, 0, 0, 0, 0};
  const G2P p = xyzz_from_affine<Fq2Ops>(q);
  return g2_subgroup_criterion(p, xyzz_scalar_mul<Fq2Ops>(p, u));
}

// threads per workgroup: the G2 body (a 63-bit scalar multiplication on the twist) keeps
// k_g2_prepare's launch bounds
template <class F>
struct PointsBlock {
  static constexpr int N = 256;
};
template <>
struct PointsBlock<Fq2Ops> {
  static constexpr int N = 64;
};

// One lane per point.
template <class F>
__global__ void __launch_bounds__(PointsBlock<F>::N) k_points_check(const Affine<F>* __restrict__ pts, uint32_t n,
                                                                    KeyVerdict* __restrict__ v) {
  const uint32_t i = blockIdx.x * (uint32_t)PointsBlock<F>::N + threadIdx.x;
  bool bad = false;
  if (i < n) bad = !point_ok(pts[i]);
  verdict_reduce<PointsBlock<F>::N>(bad, v);
}

template <class F>
ZK_DEV bool xyzz_same(const XYZZ<F>& a, const XYZZ<F>& b) {
  const bool ia = xyzz_is_inf(a), ib = xyzz_is_inf(b);
  if (ia || ib) return ia && ib;
  return F::is_zero(F::sub(F::mul(a.X, b.ZZ), F::mul(b.X, a.ZZ))) &&
         F::is_zero(F::sub(F::mul(a.Y, b.ZZZ), F::mul(b.Y, a.ZZZ)));
}

ZK_DEV void store_std(const G1Aff& p, uint32_t* out) {
  const Fq x = fp_from_mont(p.x), y = fp_from_mont(p.y);
  for (int l = 0; l < 8; l++) {
    out[l] = x.v[l];
    out[8 + l] = y.v[l];
  }
}

ZK_DEV void store_std(const G2Aff& p, uint32_t* out) {
  const Fq2 x = f2_from_mont(p.x), y = f2_from_mont(p.y);
  for (int l = 0; l < 8; l++) {
    out[l] = x.c0.v[l];
    out[8 + l] = x.c1.v[l];
    out[16 + l] = y.c0.v[l];
    out[24 + l] = y.c1.v[l];
  }
}

// the generators, Montgomery affine (G2: the snarkjs / ethereum bn128 generator)
ZK_DEV G1Aff g1_generator() {
  G1Aff g1;
  g1.x = fq_small(1);
  g1.y = fq_small(2);
  return g1;
}

ZK_DEV G2Aff g2_generator() {
  const uint32_t gx0[8] = {0xd992f6edu, 0x46debd5cu, 0xf75edaddu, 0x674322d4u, 0x5e5c4479u, 0x426a0066u, 0x121f1e76u, 0x1800deefu};
  const uint32_t gx1[8] = {0xaef312c2u, 0x97e485b7u, 0x35a9e712u, 0xf1aa4933u, 0x31fb5d25u, 0x7260bfb7u, 0x920d483au, 0x198e9393u};
  const uint32_t gy0[8] = {0x66fa7daau, 0x4ce6cc01u, 0x0c43d37bu, 0xe3d1e769u, 0x8dcb408fu, 0x4aab7180u, 0xdb8c6debu, 0x12c85ea5u};
  const uint32_t gy1[8] = {0xd122975bu, 0x55acdadcu, 0x70b38ef3u, 0xbc4b3133u, 0x690c3395u, 0xec9e99adu, 0x585ff075u, 0x090689d0u};
  Fq a, b, c, d;
  for (int i = 0; i < 8; i++) {
    a.v[i] = gx0[i];
    b.v[i] = gx1[i];
    c.v[i] = gy0[i];
    d.v[i] = gy1[i];
  }
  G2Aff g2;
  g2.x = {fp_to_mont(a), fp_to_mont(b)};
  g2.y = {fp_to_mont(c), fp_to_mont(d)};
  return g2;
}

}  // namespace zkfl
