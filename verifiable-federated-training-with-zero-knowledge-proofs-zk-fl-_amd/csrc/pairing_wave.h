// BN254 pairing with one pairing product per WAVEFRONT (csrc/verify_wave.hip): the latency
// counterpart of pairing.h, whose one-lane layout makes a single Groth16 check a serial chain of
// ~40 k Fq products.  Same tower, same Fq2 formulas and constants, same prepared-line format and
// the same exact-exponent hard part as pairing.h; only the mapping to lanes differs.  Every value
// that is stored, compared or exported is a canonical Montgomery element and field arithmetic is
// exact, so the results are the lane path's (and oracle/pairing_tower.py's) byte for byte.
//
// Tower.  Fq12 = Fq2[w]/(w^6 - xi): an element is six Fq2 coefficients of w^k, k = 2i + j for
// pairing.h's c_j.c_i (the indexing f12_frob already uses).  It lives in LDS (384 B).  A product is
// a flat map + reduce:
//   map:    lane (i, j), 36 lanes, forms the one Fq2 product a_i b_j (field.h's 8 x 32-bit
//           Montgomery product; 18 lanes for the sparse "034" line product);
//   reduce: lane k, 6 lanes, sums its column, c_k = sum_{i+j=k} + xi sum_{i+j=k+6}.
// An Fq12 product is one Fq2 product plus six Fq2 additions deep instead of 18 Fq2 products.
// Frobenius maps, conjugation and the comparison with one are per-coefficient (6 lanes).
//
// G2 steps (line preparation, the subgroup test's scalar multiplication): the running point is
// held by every lane; each step's independent Fq2 products go to one lane each, and the lanes
// swap the products through LDS (wv_xchg).  A doubling is 3 products deep instead of 12, a mixed
// addition 4 instead of 13.
//
// Control flow is wave-uniform: loop bits are constants, the skip / invalid flags are per proof.
// A workgroup is exactly one wavefront (64 threads), so every barrier is a wave barrier.
#pragma once
#include "pairing.h"

namespace zkfl {

constexpr int WV_NREG = 16;  // Fq12 registers in LDS (the final exponentiation keeps 14 live)

struct WaveLds {
  Fq2 prod[36];        // map-stage products / the exchange buffer of the G2 steps
  Fq2 r[WV_NREG][6];   // Fq12 registers, coefficient of w^k at [k]
  Fq2 line[4][3];      // this Miller step's lines, scaled by the pair's G1 point: coefficients of w^0, w^1, w^3
  Fq px[4], py[4];
  const LineCoef* lptr[4];
  uint32_t skip[4];
  uint32_t flag;
};

// position of the w^k coefficient inside struct Fq12 (c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2)
ZK_DEV int wv_pos(int k) { return (k & 1) * 3 + (k >> 1); }

ZK_NOINLINE Fq2 wv_f2_mul(const Fq2& a, const Fq2& b) { return f2_mul(a, b); }

// a / 2: a + q when a is odd, then one shift (the value of fp_mul(a, FQ_TWO_INV), without the product)
ZK_DEV Fq fp_half(const Fq& a) {
  const uint32_t m = 0u - (a.v[0] & 1u);
  uint32_t t[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    c += (uint64_t)a.v[i] + (FqP::P[i] & m);
    t[i] = (uint32_t)c;
    c >>= 32;
  }
  Fq r;
#pragma unroll
  for (int i = 0; i < 7; i++) r.v[i] = (t[i] >> 1) | (t[i + 1] << 31);
  r.v[7] = t[7] >> 1;  // a + q < 2^255: no carry out of the top limb
  return r;
}
ZK_DEV Fq2 f2_half(const Fq2& a) { return {fp_half(a.c0), fp_half(a.c1)}; }

// ---------------------------------------------------------------- Fq12 in LDS
// r[d] = r[a] * r[b]; d may alias a or b.
ZK_NOINLINE void wv_mul(WaveLds* s, int d, int a, int b) {
  const int l = threadIdx.x;
  if (l < 36) {
    const int i = l / 6, j = l - 6 * i;
    s->prod[l] = wv_f2_mul(s->r[a][i], s->r[b][j]);
  }
  __syncthreads();
  if (l < 6) {
    Fq2 lo = f2_zero(), hi = f2_zero();
    for (int i = 0; i < 6; i++) {
      const int j = l - i;
      if (j >= 0)
        lo = f2_add(lo, s->prod[i * 6 + j]);
      else
        hi = f2_add(hi, s->prod[i * 6 + j + 6]);
    }
    s->r[d][l] = f2_add(lo, f2_mul_xi(hi));
  }
  __syncthreads();
}

// r[f] *= line[p] (coefficients at w^0, w^1, w^3): 18 products, 3 per column
ZK_NOINLINE void wv_mul_line(WaveLds* s, int f, int p) {
  const int l = threadIdx.x;
  if (l < 18) {
    const int i = l / 3, t = l - 3 * i;
    s->prod[l] = wv_f2_mul(s->r[f][i], s->line[p][t]);
  }
  __syncthreads();
  if (l < 6) {
    Fq2 lo = f2_zero(), hi = f2_zero();
    for (int t = 0; t < 3; t++) {
      const int j = t == 2 ? 3 : t;
      const int i = l - j;
      if (i >= 0)
        lo = f2_add(lo, s->prod[i * 3 + t]);
      else
        hi = f2_add(hi, s->prod[(i + 6) * 3 + t]);
    }
    s->r[f][l] = f2_add(lo, f2_mul_xi(hi));
  }
  __syncthreads();
}

ZK_DEV void wv_set_one(WaveLds* s, int d) {
  const int l = threadIdx.x;
  if (l < 6) s->r[d][l] = l == 0 ? f2_one() : f2_zero();
  __syncthreads();
}

ZK_DEV void wv_copy(WaveLds* s, int d, int a) {
  const int l = threadIdx.x;
  if (l < 6) s->r[d][l] = s->r[a][l];
  __syncthreads();
}

// conjugation over Fq6 (c1 -> -c1): the odd powers of w change sign; d may alias a
ZK_DEV void wv_conj(WaveLds* s, int d, int a) {
  const int l = threadIdx.x;
  if (l < 6) {
    Fq2 x = s->r[a][l];
    s->r[d][l] = (l & 1) ? f2_neg(x) : x;
  }
  __syncthreads();
}

ZK_NOINLINE void wv_frob(WaveLds* s, int d, int a) {
  const int l = threadIdx.x;
  if (l < 6) {
    Fq2 x = f2_conj(s->r[a][l]);
    if (l) x = wv_f2_mul(x, load_fq2(GAMMA1[l]));
    s->r[d][l] = x;
  }
  __syncthreads();
}

ZK_NOINLINE void wv_frob2(WaveLds* s, int d, int a) {
  const int l = threadIdx.x;
  if (l < 6) {
    Fq2 x = s->r[a][l];
    if (l) x = f2_mul_fq(x, load_fq(GAMMA2[l]));
    s->r[d][l] = x;
  }
  __syncthreads();
}

// r[d] = r[a]^u; d != a
ZK_NOINLINE void wv_pow_u(WaveLds* s, int d, int a) {
  wv_copy(s, d, a);  // top bit of u
  for (int b = 61; b >= 0; b--) {
    wv_mul(s, d, d, d);
    if ((BN_U >> b) & 1ull) wv_mul(s, d, d, a);
  }
}

// r[d] = 1 / r[a] through the norm to Fq6: x conj(x) = c0^2 - v c1^2 has even powers only, its
// Fq6 inverse is the one serial piece (pairing.h's f6_inv on lane 0: ~50 Fq products and the
// Fq inversion).  Uses r[t0], r[t1].
ZK_NOINLINE void wv_inv(WaveLds* s, int d, int a, int t0, int t1) {
  wv_conj(s, t0, a);
  wv_mul(s, t1, a, t0);
  if (threadIdx.x == 0) {
    Fq6 n = {s->r[t1][0], s->r[t1][2], s->r[t1][4]};
    Fq6 ni = f6_inv(n);
    s->r[t1][0] = ni.c0;
    s->r[t1][2] = ni.c1;
    s->r[t1][4] = ni.c2;
  }
  __syncthreads();
  wv_mul(s, d, t0, t1);
}

ZK_DEV bool wv_is_one(const WaveLds* s, int a) {  // any lane may ask
  bool ok = f2_eq(s->r[a][0], f2_one());
  for (int k = 1; k < 6; k++) ok = ok && f2_is_zero(s->r[a][k]);
  return ok;
}

// struct Fq12 (global, Montgomery) -> r[d]
ZK_DEV void wv_load_f12(WaveLds* s, int d, const Fq12* src) {
  const int l = threadIdx.x;
  if (l < 6) s->r[d][l] = reinterpret_cast<const Fq2*>(src)[wv_pos(l)];
  __syncthreads();
}

// r[a] -> 96 std-form u32 in the ffjavascript toObject order (one Fq per lane)
ZK_DEV void wv_store_std(const WaveLds* s, int a, uint32_t* out) {
  const int l = threadIdx.x;
  if (l < 12) {
    const int k = l >> 1;
    const Fq2 c = s->r[a][k];
    const Fq x = fp_from_mont((l & 1) ? c.c1 : c.c0);
    uint32_t* o = out + wv_pos(k) * 16 + (l & 1) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = x.v[i];
  }
}

// ---------------------------------------------------------------- Miller loop
// r[f] = product over the pairs of the Miller loop with prepared lines.  P: npairs affine G1
// points (infinity: the pair contributes 1); lines[i]: ATE_NLINES coefficients of pair i.
// Per step the lines of all pairs are scaled by their points in one go (one lane per
// coefficient), then applied one after the other.
ZK_DEV void wv_miller(WaveLds* s, int f, int npairs, const G1Aff* P, const LineCoef* const* lines) {
  const int l = threadIdx.x;
  if (l < npairs) {
    G1Aff p = P[l];
    s->px[l] = p.x;
    s->py[l] = p.y;
    s->skip[l] = aff_is_inf(p) ? 1u : 0u;
    s->lptr[l] = lines[l];
  }
  wv_set_one(s, f);  // also the barrier for the above
  int k = 0;
  for (int b = 63; b >= -1; b--) {
    if (b >= 0 && b < 63) wv_mul(s, f, f, f);
    const int nl = (b < 0) ? 2 : (((ATE_LOW >> b) & 1ull) ? 2 : 1);
    for (int t = 0; t < nl; t++, k++) {
      if (l < 3 * npairs) {
        const int p = l / 3, c = l - 3 * p;
        if (!s->skip[p]) {
          Fq2 v = reinterpret_cast<const Fq2*>(s->lptr[p] + k)[c];
          if (c < 2) v = f2_mul_fq(v, c == 0 ? s->py[p] : s->px[p]);
          s->line[p][c] = v;
        }
      }
      __syncthreads();
      for (int p = 0; p < npairs; p++)
        if (!s->skip[p]) wv_mul_line(s, f, p);
    }
  }
}

// r[0] <- r[0]^((p^12-1)/r): pairing.h's final_exp, register for register (r[1..15] scratch).
ZK_DEV void wv_final_exp(WaveLds* s) {
  wv_inv(s, 1, 0, 14, 15);
  wv_conj(s, 2, 0);
  wv_mul(s, 1, 2, 1);
  wv_frob2(s, 2, 1);
  wv_mul(s, 1, 2, 1);  // t
  wv_frob(s, 2, 1);    // fp
  wv_frob2(s, 3, 1);   // fp2
  wv_frob(s, 4, 3);    // fp3
  wv_pow_u(s, 5, 1);   // fu
  wv_pow_u(s, 6, 5);   // fu2
  wv_pow_u(s, 7, 6);   // fu3
  wv_frob(s, 8, 5);
  wv_conj(s, 8, 8);    // y3
  wv_frob(s, 9, 6);    // fu2p
  wv_frob(s, 10, 7);   // fu3p
  wv_frob2(s, 11, 6);  // y2
  wv_mul(s, 2, 2, 3);
  wv_mul(s, 2, 2, 4);  // y0
  wv_conj(s, 3, 1);    // y1
  wv_conj(s, 4, 6);    // y5
  wv_mul(s, 9, 5, 9);
  wv_conj(s, 9, 9);    // y4
  wv_mul(s, 10, 7, 10);
  wv_conj(s, 10, 10);  // y6
  wv_mul(s, 12, 10, 10);
  wv_mul(s, 12, 12, 9);
  wv_mul(s, 12, 12, 4);  // t0 = y6^2 y4 y5
  wv_mul(s, 13, 8, 4);
  wv_mul(s, 13, 13, 12);  // t1 = y3 y5 t0
  wv_mul(s, 12, 12, 11);  // t0 *= y2
  wv_mul(s, 13, 13, 13);
  wv_mul(s, 13, 13, 12);
  wv_mul(s, 13, 13, 13);  // t1 = (t1^2 t0)^2
  wv_mul(s, 12, 13, 3);   // t0 = t1 y1
  wv_mul(s, 13, 13, 2);   // t1 = t1 y0
  wv_mul(s, 12, 12, 12);
  wv_mul(s, 0, 12, 13);
}

// ---------------------------------------------------------------- G2 steps across lanes
// Every lane multiplies its own operand pair; lanes < n publish the product and all lanes read
// the n products back.
template <int N>
ZK_DEV void wv_xchg(WaveLds* s, const Fq2& a, const Fq2& b, Fq2* out) {
  const int l = threadIdx.x;
  const Fq2 p = wv_f2_mul(a, b);
  if (l < N) s->prod[l] = p;
  __syncthreads();
#pragma unroll
  for (int i = 0; i < N; i++) out[i] = s->prod[i];
  __syncthreads();
}

ZK_DEV Fq2 wv_sel(int l, const Fq2& x0, const Fq2& x1, const Fq2& x2, const Fq2& x3, const Fq2& x4) {
  return l == 0 ? x0 : l == 1 ? x1 : l == 2 ? x2 : l == 3 ? x3 : x4;
}

// pairing.h's g2_dbl_step: {XY, Y^2, Z^2, X^2, (Y+Z)^2} | e = b' 3c | {e^2, a(b-f), g^2, bh}
ZK_NOINLINE LineCoef wv_g2_dbl_step(WaveLds* s, G2Proj& R) {
  const int l = threadIdx.x;
  Fq2 p[5];
  const Fq2 yz = f2_add(R.Y, R.Z);
  wv_xchg<5>(s, wv_sel(l, R.X, R.Y, R.Z, R.X, yz), wv_sel(l, R.Y, R.Y, R.Z, R.X, yz), p);
  const Fq2 a = f2_half(p[0]), b = p[1], c = p[2], j = p[3];
  const Fq2 e = wv_f2_mul(load_fq2(TWIST_B), f2_add(f2_dbl(c), c));
  const Fq2 f = f2_add(f2_dbl(e), e);
  const Fq2 g = f2_half(f2_add(b, f));
  const Fq2 h = f2_sub(p[4], f2_add(b, c));
  const Fq2 i = f2_sub(e, b);
  Fq2 q[4];
  wv_xchg<4>(s, wv_sel(l, e, a, g, b, b), wv_sel(l, e, f2_sub(b, f), g, h, h), q);
  R.X = q[1];
  R.Y = f2_sub(q[2], f2_add(f2_dbl(q[0]), q[0]));
  R.Z = q[3];
  return {f2_neg(h), f2_add(f2_dbl(j), j), i};
}

// pairing.h's g2_add_step: {qy Z, qx Z} | {theta^2, lam^2, theta qx, lam qy} | {lam d, Z c, X d} |
// {theta (g-h), e Y, lam h, Z e}
ZK_DEV LineCoef wv_g2_add_step(WaveLds* s, G2Proj& R, const Fq2& qx, const Fq2& qy) {
  const int l = threadIdx.x;
  Fq2 p[4];
  wv_xchg<2>(s, l == 0 ? qy : qx, R.Z, p);
  const Fq2 theta = f2_sub(R.Y, p[0]);
  const Fq2 lam = f2_sub(R.X, p[1]);
  wv_xchg<4>(s, wv_sel(l, theta, lam, theta, lam, lam), wv_sel(l, theta, lam, qx, qy, qy), p);
  const Fq2 c = p[0], d = p[1];
  const Fq2 j = f2_sub(p[2], p[3]);
  wv_xchg<3>(s, wv_sel(l, lam, R.Z, R.X, R.X, R.X), wv_sel(l, d, c, d, d, d), p);
  const Fq2 e = p[0], f = p[1], g = p[2];
  const Fq2 h = f2_sub(f2_add(e, f), f2_dbl(g));
  wv_xchg<4>(s, wv_sel(l, theta, e, lam, R.Z, R.Z), wv_sel(l, f2_sub(g, h), R.Y, h, e, e), p);
  R.Y = f2_sub(p[0], p[1]);
  R.X = p[2];
  R.Z = p[3];
  return {lam, f2_neg(theta), j};
}

ZK_DEV void wv_put_line(LineCoef* out, const LineCoef& c) {
  if (threadIdx.x == 0) *out = c;
}

// pairing.h's g2_prepare_lines: all ATE_NLINES coefficients for a fixed affine Q (not infinity)
ZK_DEV void wv_g2_prepare_lines(WaveLds* s, const Fq2& qx, const Fq2& qy, LineCoef* out) {
  G2Proj R = {qx, qy, f2_one()};
  int k = 0;
  for (int b = 63; b >= 0; b--) {
    wv_put_line(out + k++, wv_g2_dbl_step(s, R));
    if ((ATE_LOW >> b) & 1ull) wv_put_line(out + k++, wv_g2_add_step(s, R, qx, qy));
  }
  Fq2 q1x = f2_mul(f2_conj(qx), load_fq2(TWIST_FROB_X));
  Fq2 q1y = f2_mul(f2_conj(qy), load_fq2(TWIST_FROB_Y));
  Fq2 q2x = f2_mul(f2_conj(q1x), load_fq2(TWIST_FROB_X));
  Fq2 q2y = f2_mul(f2_conj(q1y), load_fq2(TWIST_FROB_Y));
  wv_put_line(out + k++, wv_g2_add_step(s, R, q1x, q1y));
  wv_put_line(out + k++, wv_g2_add_step(s, R, q2x, f2_neg(q2y)));
}

// [u]Q in homogeneous coordinates by the steps above (their lines are dropped).  The step
// formulas are incomplete: a step that meets R = +-Q or R = O leaves Z = 0, and Z = 0 is kept by
// every later step.  For Q of order r no prefix of u is 0 or +-1 mod r, so Z = 0 at the end means
// that Q is not in the order-r subgroup.
ZK_DEV G2Proj wv_g2_mul_u(WaveLds* s, const Fq2& qx, const Fq2& qy) {
  G2Proj R = {qx, qy, f2_one()};
  for (int b = 61; b >= 0; b--) {
    (void)wv_g2_dbl_step(s, R);
    if ((BN_U >> b) & 1ull) (void)wv_g2_add_step(s, R, qx, qy);
  }
  return R;
}

}  // namespace zkfl
