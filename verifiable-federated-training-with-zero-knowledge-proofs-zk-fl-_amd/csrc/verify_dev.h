// Device helpers and the prepared-key object shared by the two verifier units: csrc/verify.hip
// (one proof per lane) and csrc/verify_wave.hip (one proof per wavefront).  Point decoding with
// the verdict rules of snarkjs groth16_verify plus the stricter encoding checks both paths apply:
// coordinates canonical (< q), points on their curve, G2 points in the order-r subgroup.
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include "curve.h"
#include "pairing.h"
#include "zkfl.h"

namespace zkfl {

// Prepared verification key (vk_prepare): device tables of the lane path, which the wave path
// reads too (IC0, the lines of gamma2 / delta2, the Miller value of (alpha1, beta2)).
struct VkDev {
  std::vector<uint8_t> bytes;
  uint32_t npub = 0;
  G1Aff* ic_table = nullptr;  // (npub+1) x 16; index 1 of row 0 = IC0
  LineCoef* lines = nullptr;  // [3][ATE_NLINES]: beta2, gamma2, delta2
  Fq12* f_ab = nullptr;       // Miller value of (alpha1, beta2), Montgomery
  G1Aff* alpha = nullptr;
};

constexpr uint32_t ST_INF = 1u, ST_BAD = 2u;

// Host side of the two pairing hooks.  stat: the decode statuses of n G1 points, then of their n G2
// points.  The first point that is not a proper one is named in err (ZKFL_E_ARG).
inline int pairing_points_check(const std::vector<uint32_t>& stat, size_t n, std::string& err) {
  for (size_t i = 0; i < 2 * n; i++)
    if (stat[i] & ST_BAD) {
      err = "pairing: point " + std::to_string(i % n) + (i < n ? " (G1)" : " (G2)") +
            " is not canonical / not on the curve / not in the subgroup";
      return ZKFL_E_ARG;
    }
  return ZKFL_OK;
}

// A G2 point at infinity: its G1 side (d_P[i]) is made infinity too, so the pair contributes 1.
inline hipError_t pairing_fix_infinity(const std::vector<uint32_t>& stat, size_t n, G1Aff* d_P, hipStream_t st) {
  for (size_t i = 0; i < n; i++)
    if (stat[n + i] == ST_INF) {
      const hipError_t e = hipMemsetAsync(d_P + i, 0, sizeof(G1Aff), st);
      if (e != hipSuccess) return e;
    }
  return hipSuccess;
}

ZK_DEV bool lt_mod(const uint32_t* v, const uint32_t* P) {
  for (int i = 7; i >= 0; i--)
    if (v[i] != P[i]) return v[i] < P[i];
  return false;
}

// canonical std-form Fq -> Montgomery; false if >= q
ZK_DEV bool fq_load_std(const uint32_t* s, Fq& out) {
  Fq t;
#pragma unroll
  for (int i = 0; i < 8; i++) t.v[i] = s[i];
  if (!lt_mod(t.v, FqP::P)) return false;
  out = fp_to_mont(t);
  return true;
}

ZK_DEV Fq fq_small(uint32_t x) {  // Montgomery form of a small constant
  Fq t = fp_zero<FqP>();
  t.v[0] = x;
  return fp_to_mont(t);
}

// affine G1 from 16 std u32; status bits
ZK_DEV uint32_t g1_load(const uint32_t* s, G1Aff& p) {
  bool ok = fq_load_std(s, p.x) && fq_load_std(s + 8, p.y);
  if (!ok) return ST_BAD;
  if (aff_is_inf(p)) return ST_INF;
  // y^2 == x^3 + 3
  Fq lhs = fp_sqr(p.y);
  Fq rhs = fp_add(fp_mul(fp_sqr(p.x), p.x), fq_small(3));
  return fp_eq(lhs, rhs) ? 0u : ST_BAD;
}

ZK_DEV uint32_t g2_load(const uint32_t* s, G2Aff& q) {
  bool ok = fq_load_std(s, q.x.c0) && fq_load_std(s + 8, q.x.c1) && fq_load_std(s + 16, q.y.c0) &&
            fq_load_std(s + 24, q.y.c1);
  if (!ok) return ST_BAD;
  if (aff_is_inf(q)) return ST_INF;
  Fq2 lhs = f2_sqr(q.y);
  Fq2 rhs = f2_add(f2_mul(f2_sqr(q.x), q.x), load_fq2(TWIST_B));
  return f2_eq(lhs, rhs) ? 0u : ST_BAD;
}

// psi (untwist-Frobenius-twist) on XYZZ coordinates: conj is a field automorphism, so
// psi(X, Y, ZZ, ZZZ) = (conj(X) gx, conj(Y) gy, conj(ZZ), conj(ZZZ))
ZK_DEV G2P g2_psi(const G2P& p) {
  G2P r;
  r.X = f2_mul(f2_conj(p.X), load_fq2(TWIST_FROB_X));
  r.Y = f2_mul(f2_conj(p.Y), load_fq2(TWIST_FROB_Y));
  r.ZZ = f2_conj(p.ZZ);
  r.ZZZ = f2_conj(p.ZZZ);
  return r;
}

ZK_DEV bool g2_eq(const G2P& a, const G2P& b) {
  const bool ia = xyzz_is_inf(a), ib = xyzz_is_inf(b);
  if (ia || ib) return ia && ib;
  return f2_eq(f2_mul(a.X, b.ZZ), f2_mul(b.X, a.ZZ)) && f2_eq(f2_mul(a.Y, b.ZZZ), f2_mul(b.Y, a.ZZZ));
}

// The BN endomorphism criterion for order-r membership of a twist point p, given xp = [x0]p,
// x0 = u: [x0+1]P + psi([x0]P) + psi^2([x0]P) == psi^3([2 x0]P) (ePrint 2022/348 §5.1).
ZK_DEV bool g2_subgroup_criterion(const G2P& p, const G2P& xp) {
  const G2P pxp = g2_psi(xp);
  G2P lhs = xyzz_add<Fq2Ops>(xyzz_add<Fq2Ops>(xyzz_add<Fq2Ops>(xp, p), pxp), g2_psi(pxp));
  G2P rhs = g2_psi(g2_psi(g2_psi(xyzz_dbl<Fq2Ops>(xp))));
  return g2_eq(lhs, rhs);
}

}  // namespace zkfl
