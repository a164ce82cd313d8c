// Proof assembly kernels (see assemble.h): the affine outputs, the quad / row point arithmetic of
// the 29-bit engine, the GLV chains, k_assemble and its two-launch form, the split proofs' parts.
#include "assemble.h"

#include "common.h"
#include "field29.h"
#include "pairing.h"
#include "row29.h"
#include "wtrace.h"

using namespace zkfl;

namespace {

template <class F>
__device__ void store_affine_std(const Affine<F>& a, uint32_t* out);

template <>
__device__ void store_affine_std<FqOps>(const Affine<FqOps>& a, uint32_t* out) {
  Fq x = fp_from_mont(a.x), y = fp_from_mont(a.y);
  for (int i = 0; i < 8; i++) {
    out[i] = x.v[i];
    out[8 + i] = y.v[i];
  }
}

template <>
__device__ void store_affine_std<Fq2Ops>(const Affine<Fq2Ops>& a, uint32_t* out) {
  Fq2 x = f2_from_mont(a.x), y = f2_from_mont(a.y);
  for (int i = 0; i < 8; i++) {
    out[i] = x.c0.v[i];
    out[8 + i] = x.c1.v[i];
    out[16 + i] = y.c0.v[i];
    out[24 + i] = y.c1.v[i];
  }
}

// ---------------------------------------------------------------------------
// Quad-cooperative G1 point operations (k_assemble): four lanes evaluate one XYZZ doubling or
// addition together.  The products of each dependency level are spread over the quad (lane q
// computes product q) and broadcast by DPP quad_perm moves; every lane keeps the whole point, so all
// control flow stays uniform inside a quad.  A chain of point operations then costs one
// multiply latency per level (doubling 3, addition 4) instead of one per product (9 / 14).
// ---------------------------------------------------------------------------
// The quad operations are written once over a field policy QF (T, mul, add, sub<K>, dbl,
// is_zero<K>, zero, one, bcast<K>, pick4).  k_assemble runs them on Q29: the 29-bit engine's
// limbs and Montgomery domain (field29.h), a product one f29_mul (81 + 81 v_mad_u64_u32, two
// column chains: ~2.5x shorter single-lane latency than the 32-bit fp_mul).  Values are LAZY
// (normalized limbs, below a small multiple of p, tracked per site in the formulas' comments):
//   mul(a, b) < p + a b / 2^261 < 2p whenever a b < 169 p^2 (2^261 ~ 169.3 p);
//   add(a, b) < bound(a) + bound(b);  sub<K>(a, b) = a + K p - b < bound(a) + K p, for b <= a + K p
//   on Q29 but only for a + K p - b >= 2^206 on the row policy (row29.h: its top lane wraps below
//   that), so every site keeps its subtrahend well below K p: a product is < p + a b / 2^261, and
//   the formulas' comments give the bound of each subtrahend (tests/test_row_bounds_cpu.py walks
//   them; the narrowest site keeps 0.87 p);
//   is_zero<K>(a) for a < K p (a == 0, p, .., (K-1) p).
// A quad operation keeps X < 8p, Y < 4p, ZZ, ZZZ < 2p (in and out), so no product or sum is
// brought below p on the chain: the canonical (< p) form is taken once, when a point leaves
// (g1q_to).  The round-4 canonical policy spent a conditional subtraction (~40 VALU) after every
// product, sum and difference of the chain.
// lane K of the caller's quad to all four lanes: DPP quad_perm [K,K,K,K] (a VALU move, no
// LDS-path round trip as with ds_bpermute)
template <int K, int N>
ZK_DEV void quad_bcast_words(const uint32_t (&v)[N], uint32_t (&r)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = (uint32_t)__builtin_amdgcn_mov_dpp((int)v[i], K * 0x55, 0xF, 0xF, false);
}
template <int N>
ZK_DEV void pick4_words(int q, const uint32_t (&a)[N], const uint32_t (&b)[N], const uint32_t (&c)[N],
                        const uint32_t (&d)[N], uint32_t (&r)[N]) {
#pragma unroll
  for (int i = 0; i < N; i++) r[i] = (q & 2) ? ((q & 1) ? d[i] : c[i]) : ((q & 1) ? b[i] : a[i]);
}

struct Q29 {
  using T = F29;
  // two accumulators per product column (four measured 2,075 vs 2,106 config-5 proofs/s and 4.05 vs
  // 4.00 ms alone, profiles/r05_ab_q29_acc.log: the extra joins cost what the shorter spine saves)
  static ZK_DEV T mul(const T& a, const T& b) { return f29_mul_acc<2>(a, b); }
  static ZK_DEV T add(const T& a, const T& b) {
    T r = f29_add_lazy(a, b);
    f29_norm(r);
    return r;
  }
  template <int K>
  static ZK_DEV T sub(const T& a, const T& b) {
    constexpr Limbs9 k = p29_times(K, true);
    T r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = a.v[i] + k.v[i] - b.v[i];
    f29_norm(r);
    return r;
  }
  static ZK_DEV T dbl(const T& a) { return add(a, a); }
  template <int K>
  static ZK_DEV bool is_zero(const T& a) {
    bool z = false;
#pragma unroll
    for (int m = 0; m < K; m++) {
      const Limbs9 mp = p29_times(m, false);
      uint32_t d = 0;
#pragma unroll
      for (int i = 0; i < 9; i++) d |= a.v[i] ^ mp.v[i];
      z = z || d == 0;
    }
    return z;
  }
  // a < 8p -> canonical (< p)
  static ZK_DEV T canon(const T& a) { return f29_canon_sub<7>(a); }
  static ZK_DEV T zero() { return f29_zero(); }
  static ZK_DEV T one() { return f29_const(P29::ONE); }
  template <int K>
  static ZK_DEV T bcast(const T& v) {
    T r;
    quad_bcast_words<K, 9>(v.v, r.v);
    return r;
  }
  // operands by value: over references the select chain becomes a select of addresses, which
  // pins every operand to the stack
  static ZK_DEV T pick4(int q, T a, T b, T c, T d) {
    T r;
    pick4_words<9>(q, a.v, b.v, c.v, d.v, r.v);
    return r;
  }
  // Fq (Montgomery 2^256, canonical) <-> this representation
  static ZK_DEV T from_fq(const Fq& x) {
    Fq c;
#pragma unroll
    for (int i = 0; i < 8; i++) c.v[i] = P29::C261[i];
    return f29_pack(fp_mul(x, c).v);  // X 2^256 -> X 2^261, canonical
  }
  static ZK_DEV Fq to_fq(const T& x) {
    Fq r, k = fp_zero<FqP>();
    f29_unpack(r.v, x);
    k.v[7] = 1u << 27;  // 2^251: X 2^261 -> X 2^256
    return fp_mul(r, k);
  }
};

// The row policy of the GLV chains (glv_row_mul): row29.h over Fq
using Row29 = RowF<P29>;

template <class QF>
struct QPoint {
  typename QF::T X, Y, ZZ, ZZZ;
};
template <class QF>
ZK_DEV bool qp_is_inf(const QPoint<QF>& p) { return QF::template is_zero<2>(p.ZZ); }  // ZZ < 2p
template <class QF>
ZK_DEV QPoint<QF> qp_inf() { return {QF::one(), QF::one(), QF::zero(), QF::zero()}; }
using G1Q = QPoint<Q29>;
ZK_DEV G1Q g1q_from(const G1P& p) {
  return {Q29::from_fq(p.X), Q29::from_fq(p.Y), Q29::from_fq(p.ZZ), Q29::from_fq(p.ZZZ)};
}
ZK_DEV G1P g1q_to(const G1Q& p) {  // canonical coordinates out
  return {Q29::to_fq(Q29::canon(p.X)), Q29::to_fq(Q29::canon(p.Y)), Q29::to_fq(Q29::canon(p.ZZ)),
          Q29::to_fq(Q29::canon(p.ZZZ))};
}

// dbl-2008-s-1 by levels: {U^2, X^2} -> {U V, X V, V ZZ, M^2} -> {M (S - X3), W Y, W ZZZ}
// Bounds (X < 8p, Y < 4p, ZZ, ZZZ < 2p in; 2^261 = 169.3 p): U < 8p; V, X2 < 1.38p (64 p^2);
// M < 4.14p; W, S < 1.07p, ZZ3 < 1.02p, M2 < 1.11p; X3 = M2 + 4p - 2S with 2S < 2.14p, X3 < 5.11p;
// S + 6p - X3 < 5.20p (X3 > 1.86p); Y3's products M (S - X3) < 1.13p and W Y < 1.03p, Y3 < 3.13p;
// ZZZ3 < 1.02p.
// Every difference stays above 0.89p (sub<K>'s precondition on the row policy).
// CHECK = false: the operands are known to be finite and distinct (the row chains of glv_row_mul),
// so the special cases are not tested (the row policy has no is_zero)
template <class QF, bool CHECK = true>
ZK_DEV QPoint<QF> quad_dbl(const QPoint<QF>& p, int q) {
  using T = typename QF::T;
  if constexpr (CHECK) {
    if (qp_is_inf(p)) return p;
  }
  const T U = QF::dbl(p.Y);
  const T a1 = QF::pick4(q & 1, U, p.X, U, p.X);
  T t = QF::mul(a1, a1);
  const T V = QF::template bcast<0>(t), X2 = QF::template bcast<1>(t);
  const T M = QF::add(QF::dbl(X2), X2);
  t = QF::mul(QF::pick4(q, U, p.X, p.ZZ, M), QF::pick4(q, V, V, V, M));
  const T W = QF::template bcast<0>(t), S = QF::template bcast<1>(t), ZZ3 = QF::template bcast<2>(t),
          M2 = QF::template bcast<3>(t);
  QPoint<QF> r;
  r.X = QF::template sub<4>(M2, QF::dbl(S));
  t = QF::mul(QF::pick4(q, M, W, W, W), QF::pick4(q, QF::template sub<6>(S, r.X), p.Y, p.ZZZ, p.ZZZ));
  r.Y = QF::template sub<2>(QF::template bcast<0>(t), QF::template bcast<1>(t));
  r.ZZ = ZZ3;
  r.ZZZ = QF::template bcast<2>(t);
  return r;
}

// add-2008-s by levels: {U1, U2, S1, S2} -> {P^2, R^2, ZZ1 ZZ2, ZZZ1 ZZZ2} -> {P PP, U1 PP, ZZ PP}
// -> {R (Q - X3), S1 PPP, ZZZ PPP}
// Bounds (both points X < 8p, Y < 4p, ZZ, ZZZ < 2p): U1, U2 < 1.10p (16 p^2), S1, S2 < 1.05p;
// P < 3.10p, R < 3.05p; PP, R2 < 1.06p, Z12, ZZZ12 < 1.03p; PPP < 1.02p, Q, ZZ3 < 1.01p;
// R2 + 2p - PPP in (0.98p, 3.06p), X3 = that + 4p - 2Q in (2.96p, 7.06p); Q + 8p - X3 < 6.05p; Y3's
// products R (Q - X3) < 1.11p and S1 PPP < 1.01p, Y3 < 3.11p; ZZZ3 < 1.01p.  Every difference stays above
// 0.90p (sub<K>'s precondition on the row policy).
template <class QF, bool CHECK = true>
ZK_DEV QPoint<QF> quad_add(const QPoint<QF>& p, const QPoint<QF>& o, int q) {
  using T = typename QF::T;
  if constexpr (CHECK) {
    if (qp_is_inf(o)) return p;
    if (qp_is_inf(p)) return o;
  }
  T t = QF::mul(QF::pick4(q, p.X, o.X, p.Y, o.Y), QF::pick4(q, o.ZZ, p.ZZ, o.ZZZ, p.ZZZ));
  const T U1 = QF::template bcast<0>(t), U2 = QF::template bcast<1>(t), S1 = QF::template bcast<2>(t),
          S2 = QF::template bcast<3>(t);
  const T P = QF::template sub<2>(U2, U1), R = QF::template sub<2>(S2, S1);
  if constexpr (CHECK) {
    if (QF::template is_zero<4>(P)) {
      if (QF::template is_zero<4>(R)) return quad_dbl<QF>(p, q);
      return qp_inf<QF>();
    }
  }
  t = QF::mul(QF::pick4(q, P, R, p.ZZ, p.ZZZ), QF::pick4(q, P, R, o.ZZ, o.ZZZ));
  const T PP = QF::template bcast<0>(t), R2 = QF::template bcast<1>(t), Z12 = QF::template bcast<2>(t),
          ZZZ12 = QF::template bcast<3>(t);
  t = QF::mul(QF::pick4(q, P, U1, Z12, P), PP);
  const T PPP = QF::template bcast<0>(t), Q = QF::template bcast<1>(t);
  QPoint<QF> r;
  r.ZZ = QF::template bcast<2>(t);
  r.X = QF::template sub<4>(QF::template sub<2>(R2, PPP), QF::dbl(Q));
  const T QX = QF::template sub<8>(Q, r.X);
  t = QF::mul(QF::pick4(q, R, S1, ZZZ12, R), QF::pick4(q, QX, PPP, PPP, QX));
  r.Y = QF::template sub<2>(QF::template bcast<0>(t), QF::template bcast<1>(t));
  r.ZZZ = QF::template bcast<2>(t);
  return r;
}

// Fq inverse on one lane (f29_inv_divsteps): Montgomery 2^256 form in and out (0 -> 0).  The
// proof's last affine conversion (pi_c) sits on the assembly's critical path.
ZK_DEV Fq fq_inv29(const Fq& a) {
  Fq c, k = fp_zero<FqP>();
#pragma unroll
  for (int i = 0; i < 8; i++) c.v[i] = P29::C261[i];
  const Fq a261 = fp_mul(a, c);  // A 2^256 -> A 2^261 (the 29-bit engine's Montgomery domain)
  Fq r;
  const F29 a29 = f29_pack(a261.v);
  f29_unpack(r.v, f29_inv_divsteps(a29));  // A^-1 2^261, canonical
  k.v[7] = 1u << 27;  // 2^251: x 2^261 -> x 2^256
  return fp_mul(r, k);
}

ZK_DEV Affine<FqOps> g1_to_affine29(const G1P& p) {
  if (xyzz_is_inf<FqOps>(p)) return {fp_zero<FqP>(), fp_zero<FqP>()};
  const Fq iZZZ = fq_inv29(p.ZZZ);
  const Fq iZ = fp_mul(p.ZZ, iZZZ);  // ZZ / ZZZ = 1 / Z
  return {fp_mul(p.X, fp_mul(iZ, iZ)), fp_mul(p.Y, iZZZ)};
}

// G2 likewise: (a0 + a1 u)^-1 = (a0 - a1 u) / (a0^2 + a1^2), one Fq inverse
ZK_DEV Affine<Fq2Ops> g2_to_affine29(const G2P& p) {
  if (xyzz_is_inf<Fq2Ops>(p)) return {f2_zero(), f2_zero()};
  const Fq2& z = p.ZZZ;
  const Fq ni = fq_inv29(fp_add(fp_sqr(z.c0), fp_sqr(z.c1)));
  const Fq2 iZZZ = {fp_mul(z.c0, ni), fp_neg(fp_mul(z.c1, ni))};
  const Fq2 iZ = f2_mul(p.ZZ, iZZZ);
  return {f2_mul(p.X, f2_sqr(iZ)), f2_mul(p.Y, iZZZ)};
}

// One GLV half of the assembly's scalar multiplications, on one whole wave in the row policy (Row29):
// wave g < 4 computes k_g * P_g for (s1, A'), (s2, phi(A')), (r1, B1'), (r2, phi(B1')) (res[0] =
// A', res[1] = B1'), the GLV halves of s and r (glv.h): 128-bit scalars in signed 4-bit windows
// over a table of 1P..8P in LDS, the wave's four rows evaluating each level's products side by
// side (a quad chain in one wave, the round-4..6 form, took 664 us per assembly under config 5's
// load against 405 us: profiles/r06_ab_row_assembly.log).  No special cases are tested, and
// none can occur: P' = +-P or +-phi(P) is finite (checked) of prime order r; the table j P'
// (j <= 8) is built by one doubling and additions (j - 1) P' + P', j >= 3; the accumulator starts
// at the first nonzero window and is then m P' with m >= 1 -- the signed base-16 prefix of a
// non-negative scalar is >= 0, and 16 m' + d >= 9 once m' >= 1 -- so every addition adds
// d P' (|d| <= 8) to 16 m' P' with 16 <= 16 m' < 2^133 < r - 8 (never equal, opposite or
// infinity), and a doubling never meets a point of order 2.  The proof bytes are the quad
// chain's (same integers: the row product is the same Montgomery reduction).
// tab: this wave's LDS table, 8 points x 4 coordinates x 64 lanes.
ZK_DEV G1Q glv_row_mul(const G1P* __restrict__ res, const GlvScalar* __restrict__ ks, uint32_t* tab, int g) {
  using RPt = QPoint<Row29>;
  G1P P = res[g >> 1];
  if (g & 1) {  // phi(X/ZZ, Y/ZZZ) = (beta X/ZZ, Y/ZZZ)
    Fq beta;
#pragma unroll
    for (int i = 0; i < 8; i++) beta.v[i] = GLV_BETA[i];
    P.X = fp_mul(P.X, fp_to_mont(beta));
  }
  const GlvScalar k = ks[g];
  if (k.neg) P = xyzz_neg<FqOps>(P);
  const G1Q P29 = g1q_from(P);
  if (qp_is_inf(P29)) return qp_inf<Q29>();
  const int lane = (int)__lane_id(), q = lane >> 4;
  const RPt Pr = {Row29::from(P29.X), Row29::from(P29.Y), Row29::from(P29.ZZ), Row29::from(P29.ZZZ)};
  auto put = [&](int e, const RPt& t) {
    tab[(4 * e + 0) * 64 + lane] = t.X.v;
    tab[(4 * e + 1) * 64 + lane] = t.Y.v;
    tab[(4 * e + 2) * 64 + lane] = t.ZZ.v;
    tab[(4 * e + 3) * 64 + lane] = t.ZZZ.v;
  };
  put(0, Pr);
  RPt Q = quad_dbl<Row29, false>(Pr, q);
  put(1, Q);
#pragma unroll 1
  for (int e = 2; e < 8; e++) {
    Q = quad_add<Row29, false>(Q, Pr, q);
    put(e, Q);
  }
  // signed base-16 digits d_0..d_32 in [-7, 8], packed as nibbles (d & 15): word i holds
  // d_8i .. d_8i+7, word 4 holds d_32 (the final carry)
  uint32_t dg[5] = {0, 0, 0, 0, 0};
  uint32_t carry = 0;
  for (int w = 0; w < 32; w++) {
    const uint32_t v = ((k.mag[w >> 3] >> (4 * (w & 7))) & 15u) + carry;
    carry = v > 8 ? 1u : 0u;
    dg[w >> 3] |= (carry ? (v - 16) & 15u : v) << (4 * (w & 7));
  }
  dg[4] = carry;
  bool inf = true;
  RPt acc = Pr;
#pragma unroll 1
  for (int w = 32; w >= 0; w--) {
    if (!inf)
      for (int i = 0; i < 4; i++) acc = quad_dbl<Row29, false>(acc, q);
    const int wi = w >> 3;
    const uint32_t word = wi == 0 ? dg[0] : wi == 1 ? dg[1] : wi == 2 ? dg[2] : wi == 3 ? dg[3] : dg[4];
    const uint32_t nib = (word >> (4 * (w & 7))) & 15u;
    if (nib) {
      const int d = nib >= 9 ? (int)nib - 16 : (int)nib;
      const int e = (d < 0 ? -d : d) - 1;
      RPt t = {{tab[(4 * e + 0) * 64 + lane]}, {tab[(4 * e + 1) * 64 + lane]}, {tab[(4 * e + 2) * 64 + lane]},
               {tab[(4 * e + 3) * 64 + lane]}};
      // a table entry's Y is the canonical input or a quad_dbl / quad_add output: 0 < Y < 3.13p, so
      // 4p - Y is in (0.87p, 4p) -- Y < 4p alone would not keep sub<4> above its precondition
      if (d < 0) t.Y = Row29::sub<4>(Row29::zero(), t.Y);
      if (inf)
        acc = t;
      else
        acc = quad_add<Row29, false>(acc, t, q);
      inf = false;
    }
  }
  if (inf) return qp_inf<Q29>();
  return {Row29::to(acc.X), Row29::to(acc.Y), Row29::to(acc.ZZ), Row29::to(acc.ZZZ)};
}

constexpr int ASM_THREADS = 64 * 5;    // k_assemble: four chain waves + the C' + H wave
constexpr int ASM_T_THREADS = 64 * 4;  // k_assemble_t: four chain waves

struct AsmLds {
  uint32_t rtab[4][8 * 4 * 64];  // the chains' tables
  G1Q part[6];                   // the four products, C' + H, then the sum of parts 2 + 3
};

// After the chains (part[0..3] in LDS, a barrier behind): quads 0 and 1 of wave 0 add parts 0 + 1
// and 2 + 3 in one pass (the same instructions, operands by quad); quad 1 leaves its sum in part[5]
// for the caller's next barrier.  -> quad 0's sum of parts 0 + 1.
ZK_DEV G1Q asm_pair_sums(AsmLds& sh, int g, int q) {
  const int h = g & 1;
  const G1Q s = quad_add<Q29>(sh.part[2 * h], sh.part[2 * h + 1], q);
  if (g == 1 && q == 0) sh.part[5] = s;
  return s;
}

// Proof assembly, one block (replaces snarkjs's final
// pi_c = C + H + s*A + r*B1 - rs*delta; the rs*delta term is already in the C MSM):
//   waves 0..3: the four GLV halves (glv_row_mul) -> part[0..3]; wave 4: C' + H meanwhile;
//   then wave 0 sums the parts (asm_pair_sums, then quad 0 adds 2 + 3 and C' + H) and writes pi_c
//   -> proof[48..63], while lane 0 of wave 1 / wave 2 converts pi_a / pi_b -> proof[0..15] /
//   proof[16..47] -- after the chains, so that no inversion shares a SIMD with a chain
// The critical path is 132 doublings + 33 additions on the chains, 3 quad additions and one
// inversion; the quad operations run in the 29-bit engine (Q29), the inversions by divsteps.
__global__ void __launch_bounds__(ASM_THREADS) k_assemble(const G1P* __restrict__ res, const G2P* __restrict__ resB2,
                                                          const GlvScalar* __restrict__ ks, uint32_t* __restrict__ proof) {
  ZK_WT(WT_ASSEMBLE);
  ZK_LIGHT();
  // one block per proof: block b reads res[5b..], resB2[b], ks[4b..] and writes proof[64b..]
  res += 5 * blockIdx.x;
  resB2 += blockIdx.x;
  ks += 4 * blockIdx.x;
  proof += 64 * blockIdx.x;
  __shared__ AsmLds sh;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int g = lane >> 2, q = lane & 3;
  if (wave < 4) {
    const G1Q acc = glv_row_mul(res, ks, sh.rtab[wave], wave);
    if (lane == 0) sh.part[wave] = acc;
  } else if (g == 0) {  // wave 4: C' + H
    const G1Q c = quad_add<Q29>(g1q_from(res[2]), g1q_from(res[3]), q);
    if (q == 0) sh.part[4] = c;
  }
  __syncthreads();
  G1Q t01 = qp_inf<Q29>();
  if (wave == 0) t01 = asm_pair_sums(sh, g, q);
  __syncthreads();
  if (wave == 0 && g == 0) {
    const G1Q C = quad_add<Q29>(quad_add<Q29>(t01, sh.part[5], q), sh.part[4], q);
    if (q == 0) store_affine_std<FqOps>(g1_to_affine29(g1q_to(C)), proof + 48);
  } else if (wave == 1 && lane == 0) {
    store_affine_std<FqOps>(g1_to_affine29(res[0]), proof);
  } else if (wave == 2 && lane == 0) {
    store_affine_std<Fq2Ops>(g2_to_affine29(resB2[0]), proof + 16);
  }
}

// The same assembly in two launches for the low-latency schedule (enqueue_proof, one proof alone):
// k_assemble_t runs as soon as A' and B1' are final, beside the ABC / NTT / C + H chain:
// T = s pi_A + r B1 -> res[4] (XYZZ, Montgomery 2^256) and pi_a -> proof[0..15];
// k_assemble_c at the end: pi_c = (C' + H) + T -> proof[48..63] and pi_b -> proof[16..47].
// pi_c is the same point as k_assemble's (the group sum does not depend on the order), so the
// proof bytes are identical.
__global__ void __launch_bounds__(ASM_T_THREADS) k_assemble_t(G1P* __restrict__ res, const GlvScalar* __restrict__ ks,
                                                              uint32_t* __restrict__ proof) {
  ZK_WT(WT_ASSEMBLE);
  ZK_LIGHT();
  __shared__ AsmLds sh;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int g = lane >> 2, q = lane & 3;
  const G1Q acc = glv_row_mul(res, ks, sh.rtab[wave], wave);
  if (lane == 0) sh.part[wave] = acc;
  __syncthreads();
  G1Q t01 = qp_inf<Q29>();
  if (wave == 0) t01 = asm_pair_sums(sh, g, q);
  __syncthreads();
  if (wave == 0 && g == 0) {
    const G1Q T = quad_add<Q29>(t01, sh.part[5], q);
    if (q == 0) res[4] = g1q_to(T);
  } else if (wave == 1 && lane == 0) {
    store_affine_std<FqOps>(g1_to_affine29(res[0]), proof);
  }
}

// Parity hook for the assembly's scalar multiplications (zkfl_debug_g1_glv_mul): block b computes
// k_b P_b as k_assemble computes s pi_A' -- two row chains (glv_row_mul over (k1, P) and
// (k2, phi(P)), the GLV halves of k), their sum by a quad addition, affine by the divsteps inverse.
// pts: affine std (x, y), (0, 0) = infinity; zs: NULL, or one z (std, nonzero) per point: the
// chains then start from (x z^2, y z^3, z^2, z^3), as an MSM result arrives, instead of (x, y, 1, 1);
// out: affine std, infinity as zeros.
__global__ void __launch_bounds__(128) k_debug_glv_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ zs,
                                                       const GlvScalar* __restrict__ ks, uint32_t* __restrict__ out) {
  const uint32_t* pa = pts + 16 * blockIdx.x;
  ks += 2 * blockIdx.x;
  out += 16 * blockIdx.x;
  __shared__ uint32_t rtab[2][8 * 4 * 64];
  __shared__ G1Q part[2];
  __shared__ G1P P;
  if (threadIdx.x == 0) {
    Fq x, y;
    uint32_t z = 0;
    for (int i = 0; i < 8; i++) {
      x.v[i] = pa[i];
      y.v[i] = pa[8 + i];
      z |= x.v[i] | y.v[i];
    }
    P = z ? G1P{fp_to_mont(x), fp_to_mont(y), fp_one<FqP>(), fp_one<FqP>()} : xyzz_inf<FqOps>();
    if (z && zs) {
      Fq zv;
      for (int i = 0; i < 8; i++) zv.v[i] = zs[8 * blockIdx.x + i];
      zv = fp_to_mont(zv);
      const Fq zz = fp_sqr(zv), zzz = fp_mul(zz, zv);
      P = G1P{fp_mul(P.X, zz), fp_mul(P.Y, zzz), zz, zzz};
    }
  }
  __syncthreads();
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const G1Q acc = glv_row_mul(&P, ks, rtab[wave], wave);
  if (lane == 0) part[wave] = acc;
  __syncthreads();
  if (wave == 0 && lane < 4) {
    const G1Q S = quad_add<Q29>(part[0], part[1], lane & 3);
    if (lane == 0) store_affine_std<FqOps>(g1_to_affine29(g1q_to(S)), out);
  }
}

// Parity hook for the field and point layers of both policies (zkfl_debug_asm_ops): one operation on
// the caller's raw limbs, nothing normalized or reduced on the way in or out.  in: ASM_DBG_IN words
// per case, eight operands of nine limbs (a point is four: X, Y, ZZ, ZZZ); out: ASM_DBG_OUT words
// per case (the layouts: assemble.h).
// Row policy: a wave takes four cases of a field operation, one per row, so the four rows are live at
// once and differ; or one case of a point operation, every row holding the point and computing its
// share of the products, as in glv_row_mul (CHECK = false).  All 64 lanes stay active (a case past n
// computes on zeros and stores nothing): the DPP moves and the row swaps read across lanes.
template <class RF, int K>
ZK_DEV typename RF::T dbg_row_mont(const uint32_t* ci, bool live, uint32_t j) {
  uint32_t a[K][9], b[K];
#pragma unroll
  for (int k = 0; k < K; k++) {
#pragma unroll
    for (int i = 0; i < 9; i++) a[k][i] = live ? ci[9 * k + i] : 0u;
    b[k] = live && j < 9 ? ci[9 * (4 + k) + j] : 0u;
  }
  return RF::template mont<K>(a, b);
}

template <class RF>
__global__ void __launch_bounds__(64) k_debug_asm_row(int op, uint32_t n, const uint32_t* __restrict__ in,
                                                      uint32_t* __restrict__ out) {
  using T = typename RF::T;
  const int lane = threadIdx.x, q = lane >> 4;
  const uint32_t j = lane & 15;
  const bool point = op >= ASM_OP_PDBL;
  const uint32_t c = point ? blockIdx.x : 4 * blockIdx.x + q;
  const bool live = c < n;
  const uint32_t* ci = in + (size_t)ASM_DBG_IN * (live ? c : 0);
  uint32_t* co = out + (size_t)ASM_DBG_OUT * (live ? c : 0);
  auto ld = [&](int k) -> T { return {live && j < 9 ? ci[9 * k + j] : 0u}; };
  if (point) {
    const QPoint<RF> p = {ld(0), ld(1), ld(2), ld(3)}, o = {ld(4), ld(5), ld(6), ld(7)};
    const QPoint<RF> r = op == ASM_OP_PDBL ? quad_dbl<RF, false>(p, q) : quad_add<RF, false>(p, o, q);
    if (live) {
      co[64 * q + j] = r.X.v;
      co[64 * q + 16 + j] = r.Y.v;
      co[64 * q + 32 + j] = r.ZZ.v;
      co[64 * q + 48 + j] = r.ZZZ.v;
    }
    return;
  }
  T r = RF::zero();
  switch (op) {
    case ASM_OP_MUL: r = RF::mul(ld(0), ld(1)); break;
    case ASM_OP_ADD: r = RF::add(ld(0), ld(1)); break;
    case ASM_OP_DBL: r = RF::dbl(ld(0)); break;
    case ASM_OP_SUB2: r = RF::template sub<2>(ld(0), ld(1)); break;
    case ASM_OP_SUB4: r = RF::template sub<4>(ld(0), ld(1)); break;
    case ASM_OP_SUB6: r = RF::template sub<6>(ld(0), ld(1)); break;
    case ASM_OP_SUB8: r = RF::template sub<8>(ld(0), ld(1)); break;
    case ASM_OP_MONT1: r = dbg_row_mont<RF, 1>(ci, live, j); break;
    case ASM_OP_MONT2: r = dbg_row_mont<RF, 2>(ci, live, j); break;
    case ASM_OP_MONT3: r = dbg_row_mont<RF, 3>(ci, live, j); break;
    case ASM_OP_MONT4: r = dbg_row_mont<RF, 4>(ci, live, j); break;
    case ASM_OP_BCAST0: r = RF::template bcast<0>(ld(0)); break;
    case ASM_OP_BCAST1: r = RF::template bcast<1>(ld(0)); break;
    case ASM_OP_BCAST2: r = RF::template bcast<2>(ld(0)); break;
    case ASM_OP_BCAST3: r = RF::template bcast<3>(ld(0)); break;
    case ASM_OP_PICK4: r = RF::pick4(q, ld(0), ld(1), ld(2), ld(3)); break;
    case ASM_OP_FROM_TO: {  // to() reads row 0: every row of the wave returns row 0's value
      F29 x;
#pragma unroll
      for (int i = 0; i < 9; i++) x.v[i] = live ? ci[i] : 0u;
      const F29 y = RF::to(RF::from(x));
#pragma unroll
      for (int i = 0; i < 9; i++) r.v = j == (uint32_t)i ? y.v[i] : r.v;
      break;
    }
    case ASM_OP_ONE: r = RF::one(); break;
    default: break;  // ASM_OP_ZERO
  }
  if (live) co[j] = r.v;
}

// Quad policy: four lanes per case (lane q of the quad is quad index q), sixteen cases per wave; every
// lane stores its own result, so the hook also shows that the four lanes of a quad agree.  Point
// operations run with CHECK = true, as asm_pair_sums and k_assemble call them.
__global__ void __launch_bounds__(64) k_debug_asm_quad(int op, uint32_t n, const uint32_t* __restrict__ in,
                                                       uint32_t* __restrict__ out) {
  const int lane = threadIdx.x, q = lane & 3;
  const uint32_t c = 16 * blockIdx.x + (lane >> 2);
  const bool live = c < n;
  const uint32_t* ci = in + (size_t)ASM_DBG_IN * (live ? c : 0);
  uint32_t* co = out + (size_t)ASM_DBG_OUT * (live ? c : 0);
  auto ld = [&](int k) {
    F29 r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.v[i] = live ? ci[9 * k + i] : 0u;
    return r;
  };
  if (op >= ASM_OP_PDBL) {
    const G1Q p = {ld(0), ld(1), ld(2), ld(3)}, o = {ld(4), ld(5), ld(6), ld(7)};
    const G1Q r = op == ASM_OP_PDBL ? quad_dbl<Q29>(p, q) : quad_add<Q29>(p, o, q);
    if (live) {
      for (int i = 0; i < 9; i++) {
        co[36 * q + i] = r.X.v[i];
        co[36 * q + 9 + i] = r.Y.v[i];
        co[36 * q + 18 + i] = r.ZZ.v[i];
        co[36 * q + 27 + i] = r.ZZZ.v[i];
      }
    }
    return;
  }
  F29 r = f29_zero();
  switch (op) {
    case ASM_OP_MUL: r = Q29::mul(ld(0), ld(1)); break;
    case ASM_OP_ADD: r = Q29::add(ld(0), ld(1)); break;
    case ASM_OP_DBL: r = Q29::dbl(ld(0)); break;
    case ASM_OP_SUB2: r = Q29::sub<2>(ld(0), ld(1)); break;
    case ASM_OP_SUB4: r = Q29::sub<4>(ld(0), ld(1)); break;
    case ASM_OP_SUB6: r = Q29::sub<6>(ld(0), ld(1)); break;
    case ASM_OP_SUB8: r = Q29::sub<8>(ld(0), ld(1)); break;
    case ASM_OP_BCAST0: r = Q29::bcast<0>(ld(q)); break;  // lane q of the quad holds operand q
    case ASM_OP_BCAST1: r = Q29::bcast<1>(ld(q)); break;
    case ASM_OP_BCAST2: r = Q29::bcast<2>(ld(q)); break;
    case ASM_OP_BCAST3: r = Q29::bcast<3>(ld(q)); break;
    case ASM_OP_PICK4: r = Q29::pick4(q, ld(0), ld(1), ld(2), ld(3)); break;
    case ASM_OP_ONE: r = Q29::one(); break;
    case ASM_OP_IS_ZERO2: r.v[0] = Q29::is_zero<2>(ld(0)) ? 1u : 0u; break;
    case ASM_OP_IS_ZERO4: r.v[0] = Q29::is_zero<4>(ld(0)) ? 1u : 0u; break;
    case ASM_OP_CANON: r = Q29::canon(ld(0)); break;
    default: break;  // ASM_OP_ZERO
  }
  if (live)
    for (int i = 0; i < 9; i++) co[9 * q + i] = r.v[i];
}

__global__ void __launch_bounds__(128) k_assemble_c(const G1P* __restrict__ res, const G2P* __restrict__ resB2,
                                                    uint32_t* __restrict__ proof) {
  ZK_WT(WT_ASSEMBLE);
  ZK_LIGHT();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int g = lane >> 2, q = lane & 3;
  if (wave == 0 && g == 0) {
    const G1Q C = quad_add<Q29>(quad_add<Q29>(g1q_from(res[2]), g1q_from(res[3]), q), g1q_from(res[4]), q);
    if (q == 0) store_affine_std<FqOps>(g1_to_affine29(g1q_to(C)), proof + 48);
  } else if (wave == 1 && lane == 0) {
    store_affine_std<Fq2Ops>(g2_to_affine29(resB2[0]), proof + 16);
  }
}

// A key in D form (zkfl_key::a_diff): tail 0 finished with A' - B1', so res[0] += res[1] before
// anything reads it -- one quad addition (complete: either may be infinity, equal or opposite).
__global__ void __launch_bounds__(64) k_fold_a(G1P* __restrict__ res) {
  ZK_WT(WT_ASSEMBLE);
  ZK_LIGHT();
  const int lane = threadIdx.x;
  if (lane >= 4) return;
  const G1Q a = quad_add<Q29>(g1q_from(res[0]), g1q_from(res[1]), lane);
  if (lane == 0) res[0] = g1q_to(a);
}

// word offsets of a part's points (the encoding: assemble.h PART_WORDS)
__device__ constexpr int PART_OFF[5] = {0, 32, 128, 160, 64};  // A', B1', C', H (G1), B2' (G2)

__device__ void st_std(const Fq& a, uint32_t* out) {
  const Fq x = fp_from_mont(a);
  for (int i = 0; i < 8; i++) out[i] = x.v[i];
}
__device__ void st_std(const Fq2& a, uint32_t* out) {
  st_std(a.c0, out);
  st_std(a.c1, out + 8);
}
__device__ void ld_std(Fq& a, const uint32_t* in) {
  for (int i = 0; i < 8; i++) a.v[i] = in[i];
  a = fp_to_mont(a);
}
__device__ void ld_std(Fq2& a, const uint32_t* in) {
  ld_std(a.c0, in);
  ld_std(a.c1, in + 8);
}
template <class F>
__device__ void st_xyzz_std(const XYZZ<F>& p, uint32_t* out) {
  constexpr int w = sizeof(typename F::T) / 4;
  st_std(p.X, out);
  st_std(p.Y, out + w);
  st_std(p.ZZ, out + 2 * w);
  st_std(p.ZZZ, out + 3 * w);
}
template <class F>
__device__ XYZZ<F> ld_xyzz_std(const uint32_t* in) {
  constexpr int w = sizeof(typename F::T) / 4;
  XYZZ<F> p;
  ld_std(p.X, in);
  ld_std(p.Y, in + w);
  ld_std(p.ZZ, in + 2 * w);
  ld_std(p.ZZZ, in + 3 * w);
  return p;
}

// the slot's MSM results -> its part (one lane per point)
__global__ void __launch_bounds__(64) k_part_out(const G1P* __restrict__ res, const G2P* __restrict__ resB2,
                                                 uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  if (lane < 4) st_xyzz_std<FqOps>(res[lane], out + PART_OFF[lane]);
  else if (lane == 4) st_xyzz_std<Fq2Ops>(resB2[0], out + PART_OFF[4]);
}

// A part's point crossed a process boundary: it must be infinity (ZZ = ZZZ = 0) or a well-formed
// XYZZ point of the curve y^2 = x^3 + b: ZZ, ZZZ != 0, ZZ^3 = ZZZ^2 and (with x = X/ZZ, y = Y/ZZZ,
// multiplied through by ZZ^3 = ZZZ^2) Y^2 = X^3 + b ZZ^3.  A malformed one (say ZZ = 1, ZZZ = 0)
// would otherwise reach the assembly's inversions.
template <class F>
ZK_DEV bool xyzz_part_ok(const XYZZ<F>& p, const typename F::T& b) {
  const bool zz0 = F::is_zero(p.ZZ), zzz0 = F::is_zero(p.ZZZ);
  if (zz0 || zzz0) return zz0 && zzz0;
  const typename F::T zz3 = F::mul(F::sqr(p.ZZ), p.ZZ);
  if (!F::eq(zz3, F::sqr(p.ZZZ))) return false;
  return F::eq(F::sqr(p.Y), F::add(F::mul(F::sqr(p.X), p.X), F::mul(b, zz3)));
}

// block b sums the n_parts parts of proof b (parts[b][j]) into res[5b + {0, 1, 2, 3}] (A', B1', C',
// H) and resB2[b]: lanes 0..3 the G1 points, lane 4 the G2 point, a serial sum over the world size.
// A point that is not on its curve sets *bad (and is left out).
__global__ void __launch_bounds__(64) k_parts_sum(const uint32_t* __restrict__ parts, int n_parts,
                                                  G1P* __restrict__ res, G2P* __restrict__ resB2,
                                                  uint32_t* __restrict__ bad) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const uint32_t* p = parts + (size_t)b * n_parts * PART_WORDS;
  if (lane < 4) {
    Fq b3;
#pragma unroll
    for (int i = 0; i < 8; i++) b3.v[i] = FQ_THREE[i];
    G1P acc = xyzz_inf<FqOps>();
    for (int j = 0; j < n_parts; j++) {
      const G1P q = ld_xyzz_std<FqOps>(p + j * PART_WORDS + PART_OFF[lane]);
      if (xyzz_part_ok<FqOps>(q, b3)) acc = xyzz_add<FqOps>(acc, q);
      else *bad = 1u;
    }
    res[5 * b + lane] = acc;
  } else if (lane == 4) {
    const Fq2 bt = load_fq2(TWIST_B);
    G2P acc = xyzz_inf<Fq2Ops>();
    for (int j = 0; j < n_parts; j++) {
      const G2P q = ld_xyzz_std<Fq2Ops>(p + j * PART_WORDS + PART_OFF[4]);
      if (xyzz_part_ok<Fq2Ops>(q, bt)) acc = xyzz_add<Fq2Ops>(acc, q);
      else *bad = 1u;
    }
    resB2[b] = acc;
  }
}

// MSM result(s) -> std affine bytes (parity hooks)
template <class F>
__global__ void __launch_bounds__(64) k_point_out(const XYZZ<F>* __restrict__ p, int n, uint32_t* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int words = sizeof(Affine<F>) / 4;
  store_affine_std<F>(xyzz_to_affine<F>(p[i]), out + i * words);
}

}  // namespace

namespace zkfl {

hipError_t zk_wtrace_bind_asm(const WtBuf& b) { return zk_wtrace_bind_tu(b); }

void assemble(hipStream_t st, uint32_t n, const G1P* res, const G2P* resB2, const GlvScalar* ks, uint32_t* proof) {
  hipLaunchKernelGGL(k_assemble, dim3(n), dim3(ASM_THREADS), 0, st, res, resB2, ks, proof);
}

void assemble_t(hipStream_t st, G1P* res, const GlvScalar* ks, uint32_t* proof) {
  hipLaunchKernelGGL(k_assemble_t, dim3(1), dim3(ASM_T_THREADS), 0, st, res, ks, proof);
}

void assemble_c(hipStream_t st, const G1P* res, const G2P* resB2, uint32_t* proof) {
  hipLaunchKernelGGL(k_assemble_c, dim3(1), dim3(128), 0, st, res, resB2, proof);
}

void fold_a(hipStream_t st, G1P* res) { hipLaunchKernelGGL(k_fold_a, dim3(1), dim3(64), 0, st, res); }

void debug_glv_mul(hipStream_t st, uint32_t n, const uint32_t* pts, const uint32_t* zs, const GlvScalar* ks,
                   uint32_t* out) {
  hipLaunchKernelGGL(k_debug_glv_mul, dim3(n), dim3(128), 0, st, pts, zs, ks, out);
}

bool debug_asm_op_ok(int policy, int op) {
  if (op == ASM_OP_PDBL || op == ASM_OP_PADD) return policy == 0 || policy == 1;
  if (policy == 0) return op >= ASM_OP_MUL && op <= ASM_OP_ZERO;
  if (policy == 1)  // no mont<K> and no row form on one lane
    return op >= ASM_OP_MUL && op <= ASM_OP_CANON && !(op >= ASM_OP_MONT1 && op <= ASM_OP_MONT4) &&
           op != ASM_OP_FROM_TO;
  return false;
}

void debug_asm_ops(hipStream_t st, int policy, int op, uint32_t n, const uint32_t* in, uint32_t* out) {
  const bool point = op >= ASM_OP_PDBL;
  if (policy == 0)
    hipLaunchKernelGGL(k_debug_asm_row<Row29>, dim3(point ? n : (n + 3) / 4), dim3(64), 0, st, op, n, in, out);
  else
    hipLaunchKernelGGL(k_debug_asm_quad, dim3((n + 15) / 16), dim3(64), 0, st, op, n, in, out);
}

void part_out(hipStream_t st, const G1P* res, const G2P* resB2, uint32_t* out) {
  hipLaunchKernelGGL(k_part_out, dim3(1), dim3(64), 0, st, res, resB2, out);
}

void parts_sum(hipStream_t st, uint32_t n, const uint32_t* parts, int n_parts, G1P* res, G2P* resB2, uint32_t* bad) {
  hipLaunchKernelGGL(k_parts_sum, dim3(n), dim3(64), 0, st, parts, n_parts, res, resB2, bad);
}

void point_out(hipStream_t st, const G1P* p, int n, uint32_t* out) {
  hipLaunchKernelGGL(k_point_out<FqOps>, dim3(1), dim3(n), 0, st, p, n, out);
}

void point_out(hipStream_t st, const G2P* p, int n, uint32_t* out) {
  hipLaunchKernelGGL(k_point_out<Fq2Ops>, dim3(1), dim3(n), 0, st, p, n, out);
}

}  // namespace zkfl
