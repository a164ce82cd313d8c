// A round's Groth16 proofs as one random combination with one final exponentiation (BN254).
//
// The server side of a federated round asks "are all of these proofs valid?" (the reference
// verifies client by client and phase by phase, tests/full_system_simulation.mjs:1298-1343).
// With z_i uniform in [0, 2^128) the n pairing checks collapse into one product (the batched
// Groth16 verifier):
//
//   prod_i e(z_i (-A_i), B_i) * prod_k [ e(S_k, beta_k) e(X_k, gamma_k) e(C_k, delta_k) ] == 1
//   S_k = sum z_i alpha_k = (sum z_i mod r) alpha_k,  X_k = sum z_i vk_x_i,  C_k = sum z_i C_i
//
// (sums over key k's jobs).  If every proof is valid the product is 1; if one is not it is 1 with
// probability <= 2^-128 over the z_i, provided every pi_b is in the order-r subgroup -- the
// screening below is what the bound rests on.
//
// Per pass (at most `chunk` proofs, the lines of pi_b are 19.6 KB each):
//   k_round_screen  one lane per piece of work, blocks are uniform in what they do.  Per proof:
//                   0  pi_b: canonical, on the twist, in the subgroup
//                   1  pi_b's 102 lines
//                   2  pi_a, pi_c: canonical, on the curve; z (-pi_a) (affine), z pi_c
//                   3  z alpha
//                   and per group of ROUND_TERMS terms of vk_x = IC_0 + sum pub_t IC_t: the public
//                   signals < r, and the group's part of z vk_x = z IC_0 + sum (z pub_t mod r) IC_t
//                   from the key's window tables -- z goes into the scalars, so no second
//                   multiplication follows, and a key with many public signals spreads over lanes.
//                   S_k is summed from per-job z_i alpha_k like X_k and C_k: the pieces run side by
//                   side on wavefronts that would idle, where (sum z_i) alpha_k would be one more
//                   serial scalar multiplication on a single lane per key.
//   k_round_sums    per (key, sum): a tree over the block's lanes in LDS by the complete addition
//                   (the sums meet P + P and P + (-P)), added to the key's running sums; block
//                   (key, 0) also writes the pass's screened flags.
//   k_round_pair    two lanes per proof: the two factors (miller_part) of the Miller value of
//                   (z (-pi_a), pi_b) on pi_b's own lines.  In the last pass six more lanes per key
//                   take (S_k, beta), (X_k, gamma), (C_k, delta) on the key's lines.
//   k_round_prod    Fq12 product tree: 64 values per block in LDS, then over the blocks' values;
//                   the running product of earlier passes is one more leaf.
// Last: k_round_final, one wavefront: the final exponentiation on pairing_wave.h's tower (the one
// serial piece of the round), the 384 B value and the comparison with 1.
// All arithmetic is exact, so neither the order of the trees nor the split into passes changes a
// byte of the result.
#include <hip/hip_runtime.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "common.h"
#include "curve.h"
#include "devbufs.h"
#include "pairing.h"
#include "pairing_wave.h"
#include "verify.h"
#include "verify_dev.h"
#include "zkfl.h"

namespace zkfl {

namespace {

struct RoundJobDev {
  const G1Aff* ic_table;  // the key's (npub+1) x 16 window table: row t holds d * IC_t, d = 0..15
  const G1Aff* alpha;
  uint64_t pub_off;  // u32 words into the pass's public signals
  uint32_t npub;
  uint32_t pad;
};

// vk_x = IC_0 + sum pub_t IC_t has npub + 1 terms; a lane takes ROUND_TERMS consecutive ones
constexpr uint32_t ROUND_TERMS = 6;
struct RoundGroup {
  uint32_t job, first_term;
};

struct RoundRange {  // one key's jobs inside the pass, and their term groups
  uint32_t lo, hi, xlo, xhi;
};

constexpr int ROUND_NSUM = 3;     // per key: S (pairs with beta2), X (gamma2), C (delta2): vk->lines' order
constexpr int SUM_THREADS = 256;  // 32 KB of LDS for the tree

// z * p, z = 4 x u32 little endian; complete (p may be infinity, z may be 0)
ZK_DEV G1P g1_mul128(const G1Aff& p, const uint32_t* z) {
  G1P acc = xyzz_inf<FqOps>();
  for (int i = 3; i >= 0; i--) {
    const uint32_t w = z[i];
    for (int b = 31; b >= 0; b--) {
      acc = xyzz_dbl<FqOps>(acc);
      if ((w >> b) & 1u) acc = xyzz_madd<FqOps>(acc, p);
    }
  }
  return acc;
}

// verify.hip's g2_in_subgroup
ZK_DEV bool round_g2_in_subgroup(const G2Aff& q) {
  const uint32_t u[8] = {(uint32_t)BN_U, (uint32_t)(BN_U >> 32), 0, 0, 0, 0, 0, 0};
  const G2P p = xyzz_from_affine<Fq2Ops>(q);
  const G2P xp = xyzz_scalar_mul<Fq2Ops>(p, u);
  return g2_subgroup_criterion(p, xp);
}

// gstat: [m] the public signals' verdicts, then [m] pi_a's and pi_c's
ZK_DEV bool round_screened(size_t i, size_t m, const uint32_t* bstat, const uint32_t* gstat) {
  return ((bstat[i] & ST_BAD) | gstat[i] | gstat[m + i]) != 0;
}

// sums: [m] z alpha | [m] z pi_c | [T] the term groups' parts of z vk_x
__global__ __launch_bounds__(64) void k_round_screen(size_t m, unsigned gb, size_t T, const RoundJobDev* jobs,
                                                     const RoundGroup* groups, const uint32_t* pubs,
                                                     const uint32_t* proofs, const uint32_t* z, LineCoef* lines,
                                                     uint32_t* bstat, uint32_t* gstat, G1Aff* P0, G1P* sums) {
  const unsigned role = blockIdx.x / gb;  // 0..3: per proof; from 4 on: per term group
  if (role >= 4) {
    // z vk_x = z IC_0 + sum (z pub_t mod r) IC_t over this lane's terms, 4-bit windows, MSB first
    // (k_verify_inputs' vk_x with the scalars scaled by z)
    const size_t t = (size_t)(blockIdx.x - 4 * gb) * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const RoundGroup g = groups[t];
    const RoundJobDev jb = jobs[g.job];
    const uint32_t* pub = pubs + jb.pub_off;
    if (g.first_term == 0) {  // the job's first group also answers for its public signals
      uint32_t bad = 0;
      for (uint32_t j = 0; j < jb.npub; j++)
        if (!lt_mod(pub + j * 8, FrP::P)) bad = ST_BAD;
      gstat[g.job] = bad;
    }
    Fr zm = fp_zero<FrP>();
    for (int l = 0; l < 4; l++) zm.v[l] = z[(size_t)g.job * 4 + l];
    const uint32_t nt = min(ROUND_TERMS, jb.npub + 1 - g.first_term);
    Fr sc[ROUND_TERMS];  // standard form; a public signal >= r gives some scalar, and the job is screened
    for (uint32_t c = 0; c < ROUND_TERMS; c++) {
      sc[c] = fp_zero<FrP>();
      if (c >= nt) continue;
      const uint32_t term = g.first_term + c;
      if (term == 0) {
        sc[c] = zm;
      } else {
        Fr x;
        for (int l = 0; l < 8; l++) x.v[l] = pub[(size_t)(term - 1) * 8 + l];
        sc[c] = fp_mul(fp_to_mont(x), zm);  // Montgomery product of x R and z: x z mod r, standard form
      }
    }
    G1P acc = xyzz_inf<FqOps>();
    for (int w = 63; w >= 0; w--) {
      if (w != 63)
        for (int d = 0; d < 4; d++) acc = xyzz_dbl<FqOps>(acc);
      for (uint32_t c = 0; c < nt; c++) {
        const uint32_t dig = (sc[c].v[w >> 3] >> ((w & 7) * 4)) & 15u;
        if (dig) acc = xyzz_madd<FqOps>(acc, jb.ic_table[(size_t)(g.first_term + c) * 16 + dig]);
      }
    }
    sums[2 * m + t] = acc;
    return;
  }
  const size_t i = (size_t)(blockIdx.x - role * gb) * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint32_t* pr = proofs + i * 64;
  const uint32_t* zi = z + i * 4;
  if (role == 0) {  // k_g2_prepare's checks
    G2Aff q;
    uint32_t st = g2_load(pr + 16, q);
    if (st == 0 && !round_g2_in_subgroup(q)) st = ST_BAD;
    bstat[i] = st;
  } else if (role == 1) {  // k_g2_prepare's lines (of any point on the twist: role 0 has the verdict)
    G2Aff q;
    if (g2_load(pr + 16, q) == 0) g2_prepare_lines(q.x, q.y, lines + i * ATE_NLINES);
  } else if (role == 2) {  // pi_a, pi_c
    G1Aff a, c;
    const uint32_t sa = g1_load(pr, a), sc = g1_load(pr + 48, c);
    const uint32_t bad = (sa | sc) & ST_BAD;
    gstat[m + i] = bad;
    const G1Aff zero = {fp_zero<FqP>(), fp_zero<FqP>()};
    if (bad) {
      P0[i] = zero;
      sums[m + i] = xyzz_inf<FqOps>();
      return;
    }
    // z (-A): infinity for A = O or z = 0, and the pair then contributes 1
    P0[i] = xyzz_to_affine<FqOps>(g1_mul128(aff_neg<FqOps>(a), zi));
    sums[m + i] = g1_mul128(c, zi);
  } else {  // z alpha
    sums[i] = g1_mul128(*jobs[i].alpha, zi);
  }
}

// Block (k, y): sum y (0 S, 1 X, 2 C) of key k over the pass's jobs [lo, hi) -- for X their term
// groups [xlo, xhi) -- that passed the screening, added to acc[k][y] (stored when first).  Lanes
// stride over the range, then a tree over the lanes.
// The narrow entry runs it per segment (a group's jobs of one key) with a tree of one wavefront.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void k_round_sums(size_t m, const RoundRange* ranges, const RoundGroup* groups,
                                                        const uint32_t* bstat, const uint32_t* gstat, const G1P* sums,
                                                        int first, G1P* acc, int32_t* screened) {
  constexpr unsigned SUM_THREADS = THREADS;
  __shared__ G1P s[SUM_THREADS];
  const unsigned k = blockIdx.x, y = blockIdx.y, t = threadIdx.x;
  const RoundRange rg = ranges[k];
  const size_t lo = y == 1 ? rg.xlo : rg.lo, hi = y == 1 ? rg.xhi : rg.hi;
  const size_t base = y == 0 ? 0 : (y == 1 ? 2 * m : m);
  G1P a = xyzz_inf<FqOps>();
  for (size_t e = lo + t; e < hi; e += SUM_THREADS) {
    const size_t i = y == 1 ? groups[e].job : e;
    const bool scr = round_screened(i, m, bstat, gstat);
    if (y == 0) screened[i] = scr ? 1 : 0;
    if (!scr) a = xyzz_add<FqOps>(a, sums[base + e]);
  }
  s[t] = a;
  __syncthreads();
  for (unsigned h = SUM_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) {
      const G1P p = s[t], q = s[t + h];
      s[t] = xyzz_add<FqOps>(p, q);
    }
    __syncthreads();
  }
  if (t == 0) {
    G1P* o = acc + (size_t)k * ROUND_NSUM + y;
    const G1P p = s[0];
    *o = first ? p : xyzz_add<FqOps>(*o, p);
  }
}

// The Miller loop of one pair is a serial chain of 63 squarings and 102 line products.  Its value
// is the product of the lines, each raised to 2^(the squarings behind it), so the loop bits
// [b_hi, b_lo] (-1: the two Frobenius lines) give a factor of their own: pairing.h's
// miller_prepared over those bits from f = 1, then the squarings of the bits below.  Two lanes
// take [63, MILLER_SPLIT] and [MILLER_SPLIT - 1, -1]; the product tree multiplies the factors.
// The upper part always pays the 63 squarings, so the lower one takes most of the lines: 38
// balances 63 x 36 + 39 x 45 against 37 x 36 + 63 x 45 Fq products (full loop: 63 x 36 + 102 x 45).
constexpr int MILLER_SPLIT = 38;

ZK_DEV Fq12 miller_part(const Fq& px, const Fq& py, const LineCoef* lines, int b_hi, int b_lo) {
  int k = 0;
  for (int b = 63; b > b_hi; b--) k += ((ATE_LOW >> b) & 1ull) ? 2 : 1;
  Fq12 f = f12_one();
  for (int b = b_hi; b >= b_lo; b--) {
    if (b >= 0 && b < b_hi) f = f12_sqr(f);
    const int nl = (b < 0) ? 2 : (((ATE_LOW >> b) & 1ull) ? 2 : 1);
    for (int t = 0; t < nl; t++, k++) f = ell(f, lines[k], px, py);
  }
  for (int b = b_lo - 1; b >= 0; b--) f = f12_sqr(f);
  return f;
}

// Item i < m: proof i of the pass.  Item m + j, j < nk3 (in blocks of their own): sum j % 3 of key
// j / 3 against that key's beta2 / gamma2 / delta2 lines.  The grid holds the items twice, upper
// parts then lower parts: f[part * (m + nk3) + item] = that part of the pair's Miller value.
__global__ __launch_bounds__(64) void k_round_pair(size_t m, unsigned gb, const G1Aff* P0, const LineCoef* lines,
                                                   const uint32_t* bstat, const uint32_t* gstat, size_t nk3,
                                                   unsigned gk, const G1P* acc, const LineCoef* const* key_lines,
                                                   Fq12* f) {
  const unsigned part = blockIdx.x / (gb + gk), bx = blockIdx.x - part * (gb + gk);
  G1Aff p;
  const LineCoef* ln;
  size_t item;
  bool skip;
  if (bx < gb) {
    const size_t i = (size_t)bx * blockDim.x + threadIdx.x;
    if (i >= m) return;
    p = P0[i];
    ln = lines + i * ATE_NLINES;
    item = i;
    skip = round_screened(i, m, bstat, gstat) || bstat[i] == ST_INF;
  } else {
    const size_t j = (size_t)(bx - gb) * blockDim.x + threadIdx.x;
    if (j >= nk3) return;
    p = xyzz_to_affine<FqOps>(acc[j]);
    ln = key_lines[j / ROUND_NSUM] + (j % ROUND_NSUM) * ATE_NLINES;
    item = m + j;
    skip = false;
  }
  skip = skip || aff_is_inf(p);
  Fq12* out = f + part * (m + nk3) + item;
  if (skip)
    *out = f12_one();
  else
    *out = part == 0 ? miller_part(p.x, p.y, ln, 63, MILLER_SPLIT) : miller_part(p.x, p.y, ln, MILLER_SPLIT - 1, -1);
}

// out[block] = product of in[64 block .. +64) (short tail: ones)
__global__ __launch_bounds__(64) void k_round_prod(size_t cnt, const Fq12* in, Fq12* out) {
  __shared__ Fq12 s[64];
  const unsigned t = threadIdx.x;
  const size_t i = (size_t)blockIdx.x * 64 + t;
  s[t] = i < cnt ? in[i] : f12_one();
  __syncthreads();
  for (unsigned h = 32; h > 0; h >>= 1) {
    if (t < h) {
      const Fq12 a = s[t], b = s[t + h];
      s[t] = f12_mul(a, b);
    }
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = s[0];
}

// One wavefront: gt = f^((p^12-1)/r) (std form, zkfl_pairing's layout), passed = (gt == 1)
__global__ __launch_bounds__(64) void k_round_final(const Fq12* f, uint32_t* gt_std, uint32_t* passed) {
  __shared__ WaveLds s;
  wv_load_f12(&s, 0, f);
  wv_final_exp(&s);
  wv_store_std(&s, 0, gt_std);
  if (threadIdx.x == 0) *passed = wv_is_one(&s, 0) ? 1u : 0u;
}

// ---- narrowing: one value per group of jobs (verify_round_narrow) ----
// A group is a run of jobs of the pass; a segment is a group's jobs of one key, with sums S, X, C
// of its own (k_round_sums over the segment's range) and three pairs against that key's lines
// (k_round_pair's items behind the jobs).  jlo..jhi: the group's jobs, slo..shi: its segments.
struct RoundGrp {
  uint32_t jlo, jhi, slo, shi;
};

// Block g: out[g] = the product of both Miller parts of group g's jobs and of its segments' three
// pairs, f laid out as k_round_pair writes it.  Lanes stride over the 2 (jobs + 3 segments)
// values, then a tree over the lanes.
__global__ __launch_bounds__(64) void k_round_group_prod(size_t m, size_t nk3, const RoundGrp* grps, const Fq12* f,
                                                         Fq12* out) {
  __shared__ Fq12 s[64];
  const unsigned t = threadIdx.x;
  const RoundGrp g = grps[blockIdx.x];
  const size_t nj = g.jhi - g.jlo, per = nj + (size_t)ROUND_NSUM * (g.shi - g.slo);
  Fq12 a = f12_one();
  bool have = false;
  for (size_t e = t; e < 2 * per; e += 64) {
    const size_t part = e >= per ? 1 : 0, r = e - part * per;
    const size_t item = r < nj ? g.jlo + r : m + (size_t)ROUND_NSUM * g.slo + (r - nj);
    const Fq12 v = f[part * (m + nk3) + item];
    a = have ? f12_mul(a, v) : v;
    have = true;
  }
  s[t] = a;
  __syncthreads();
  for (unsigned h = 32; h > 0; h >>= 1) {
    if (t < h) {
      const Fq12 p = s[t], q = s[t + h];
      s[t] = f12_mul(p, q);
    }
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = s[0];
}

// k_round_final, one wavefront per group: gt of group g at gt_std + 96 g, one[g] = (gt == 1)
__global__ __launch_bounds__(64) void k_round_final_groups(const Fq12* f, uint32_t* gt_std, uint32_t* one) {
  __shared__ WaveLds s;
  const size_t g = blockIdx.x;
  wv_load_f12(&s, 0, f + g);
  wv_final_exp(&s);
  wv_store_std(&s, 0, gt_std + 96 * g);
  if (threadIdx.x == 0) one[g] = wv_is_one(&s, 0) ? 1u : 0u;
}

constexpr size_t PAD = 16;  // bytes behind every allocation of this unit

// keys in order of first appearance; jobs ordered by key (stable), so a key's jobs are one range
// [start[k], start[k + 1]) of order
void round_order(size_t n, const VerifyJob* jobs, std::vector<const VkDev*>& keys, std::vector<uint32_t>& key_of,
                 std::vector<size_t>& start, std::vector<size_t>& order) {
  key_of.resize(n);
  std::unordered_map<const VkDev*, uint32_t> seen;
  for (size_t i = 0; i < n; i++) {
    auto it = seen.find(jobs[i].vk);
    if (it == seen.end()) {
      it = seen.emplace(jobs[i].vk, (uint32_t)keys.size()).first;
      keys.push_back(jobs[i].vk);
    }
    key_of[i] = it->second;
  }
  const size_t K = keys.size();
  start.assign(K + 1, 0);
  order.resize(n);
  for (size_t i = 0; i < n; i++) start[key_of[i] + 1]++;
  for (size_t k = 0; k < K; k++) start[k + 1] += start[k];
  std::vector<size_t> fill(start.begin(), start.end() - 1);
  for (size_t i = 0; i < n; i++) order[fill[key_of[i]]++] = i;
}

}  // namespace

int verify_round(size_t n, const VerifyJob* jobs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                 uint8_t* gt_out, int32_t* screened, int* passed, uint32_t* nkeys, hipStream_t st, Profiler* prof,
                 std::string& err) {
  const char* const where = "verify_round";
  std::vector<const VkDev*> keys;
  std::vector<uint32_t> key_of;
  std::vector<size_t> start, order;
  round_order(n, jobs, keys, key_of, start, order);
  const size_t K = keys.size();
  if (nkeys) *nkeys = (uint32_t)K;
  const size_t cap = round_pass_size(n, chunk);
  size_t pub_words = 0, tcap = 0;  // the largest pass: public signals, term groups
  for (size_t off = 0; off < n; off += cap) {
    size_t w = 0, t = 0;
    for (size_t j = off; j < n && j < off + cap; j++) {
      const size_t np = jobs[order[j]].vk->npub;
      w += 8 * np;
      t += (np + 1 + ROUND_TERMS - 1) / ROUND_TERMS;
    }
    if (w > pub_words) pub_words = w;
    if (t > tcap) tcap = t;
  }
  const size_t nk3 = ROUND_NSUM * K;
  const size_t fcap = 2 * (cap + nk3) + 1;  // two parts per pair, and the earlier passes' product

  DevBufs D;
  RoundJobDev* d_jobs;
  RoundRange* d_ranges;
  RoundGroup* d_groups;
  const LineCoef** d_klines;
  uint32_t *d_pub, *d_proof, *d_z, *d_bstat, *d_gstat, *d_gt, *d_pass;
  LineCoef* d_lines;
  G1Aff* d_P0;
  G1P *d_sums, *d_acc;
  int32_t* d_scr;
  Fq12 *d_fa, *d_fb, *d_facc;
  HIP_TRY_ERR(D.get(&d_jobs, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_ranges, K, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_groups, tcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_klines, K, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_pub, pub_words, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_proof, cap * 64, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_z, cap * 4, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_bstat, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gstat, 2 * cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gt, 96, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_pass, 1, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_lines, cap * ATE_NLINES, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_P0, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_sums, 2 * cap + tcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_acc, nk3, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_scr, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_fa, fcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_fb, (fcap + 63) / 64, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_facc, 1, PAD), where, err);

  std::vector<const LineCoef*> klines(K);
  for (size_t k = 0; k < K; k++) klines[k] = keys[k]->lines;
  HIP_TRY_ERR(hipMemcpyAsync(d_klines, klines.data(), K * sizeof(LineCoef*), hipMemcpyHostToDevice, st), where, err);

  std::vector<RoundJobDev> hj(cap);
  std::vector<RoundRange> hr(K);
  std::vector<RoundGroup> hg(tcap);
  std::vector<size_t> gfirst(cap + 1);  // job j's first term group
  std::vector<uint32_t> hpub(pub_words + 1), hproof(cap * 64), hz(cap * 4);
  std::vector<int32_t> hscr(cap);
  for (size_t off = 0; off < n; off += cap) {
    const size_t m = (n - off < cap) ? n - off : cap;
    const bool first = off == 0, last = off + m == n;
    size_t w = 0, T = 0;
    for (size_t j = 0; j < m; j++) {
      const size_t i = order[off + j];
      const VkDev* vk = jobs[i].vk;
      hj[j] = {vk->ic_table, vk->alpha, (uint64_t)w, vk->npub, 0};
      gfirst[j] = T;
      for (uint32_t t0 = 0; t0 < vk->npub + 1; t0 += ROUND_TERMS) hg[T++] = {(uint32_t)j, t0};
      if (vk->npub) memcpy(hpub.data() + w, jobs[i].pub, 32 * (size_t)vk->npub);
      w += 8 * (size_t)vk->npub;
      memcpy(hproof.data() + 64 * j, proofs + 256 * i, 256);
      memcpy(hz.data() + 4 * j, z + 16 * i, 16);
    }
    gfirst[m] = T;
    for (size_t k = 0; k < K; k++) {  // [start[k], start[k+1]) cut to [off, off + m)
      const size_t lo = start[k] > off ? start[k] : off, hi = start[k + 1] < off + m ? start[k + 1] : off + m;
      hr[k] = lo < hi ? RoundRange{(uint32_t)(lo - off), (uint32_t)(hi - off), (uint32_t)gfirst[lo - off],
                                   (uint32_t)gfirst[hi - off]}
                      : RoundRange{0, 0, 0, 0};
    }
    HIP_TRY_ERR(hipMemcpyAsync(d_jobs, hj.data(), m * sizeof(RoundJobDev), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_ranges, hr.data(), K * sizeof(RoundRange), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_groups, hg.data(), T * sizeof(RoundGroup), hipMemcpyHostToDevice, st), where, err);
    if (w) HIP_TRY_ERR(hipMemcpyAsync(d_pub, hpub.data(), w * 4, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_proof, hproof.data(), m * 256, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_z, hz.data(), m * 16, hipMemcpyHostToDevice, st), where, err);

    const unsigned gb = zk_grid(m, 64);
    int pi = prof ? prof->begin("verify_round_screen", st) : -1;
    hipLaunchKernelGGL(k_round_screen, dim3(4 * gb + zk_grid(T, 64)), dim3(64), 0, st, m, gb, T,
                       (const RoundJobDev*)d_jobs, (const RoundGroup*)d_groups, (const uint32_t*)d_pub,
                       (const uint32_t*)d_proof, (const uint32_t*)d_z, d_lines, d_bstat, d_gstat, d_P0, d_sums);
    if (prof) prof->end(pi, st, (double)m);
    pi = prof ? prof->begin("verify_round_reduce", st) : -1;
    hipLaunchKernelGGL(k_round_sums<SUM_THREADS>, dim3((unsigned)K, ROUND_NSUM), dim3(SUM_THREADS), 0, st, m,
                       (const RoundRange*)d_ranges, (const RoundGroup*)d_groups, (const uint32_t*)d_bstat, (const uint32_t*)d_gstat,
                       (const G1P*)d_sums, first ? 1 : 0, d_acc, d_scr);
    if (prof) prof->end(pi, st, (double)m);
    const size_t nk = last ? nk3 : 0;
    pi = prof ? prof->begin("verify_round_pair", st) : -1;
    const unsigned gk = zk_grid(nk, 64);
    hipLaunchKernelGGL(k_round_pair, dim3(2 * (gb + gk)), dim3(64), 0, st, m, gb, (const G1Aff*)d_P0,
                       (const LineCoef*)d_lines, (const uint32_t*)d_bstat, (const uint32_t*)d_gstat, nk, gk,
                       (const G1P*)d_acc, (const LineCoef* const*)d_klines, d_fa);
    if (prof) prof->end(pi, st, (double)m);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    // the product of this pass's values and of the passes before it
    size_t cnt = 2 * (m + nk);
    if (!first) {
      HIP_TRY_ERR(hipMemcpyAsync(d_fa + cnt, d_facc, sizeof(Fq12), hipMemcpyDeviceToDevice, st), where, err);
      cnt++;
    }
    Fq12 *in = d_fa, *out = d_fb;
    pi = prof ? prof->begin("verify_round_reduce", st) : -1;
    while (cnt > 1) {
      const unsigned g = zk_grid(cnt, 64);
      hipLaunchKernelGGL(k_round_prod, dim3(g), dim3(64), 0, st, cnt, (const Fq12*)in, out);
      cnt = g;
      Fq12* t = in;
      in = out;
      out = t;
    }
    if (prof) prof->end(pi, st, 0.0);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_facc, in, sizeof(Fq12), hipMemcpyDeviceToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(hscr.data(), d_scr, m * 4, hipMemcpyDeviceToHost, st), where, err);
    HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
    for (size_t j = 0; j < m; j++) screened[order[off + j]] = hscr[j];
  }
  int pi = prof ? prof->begin("verify_round_final", st) : -1;
  hipLaunchKernelGGL(k_round_final, dim3(1), dim3(64), 0, st, (const Fq12*)d_facc, d_gt, d_pass);
  if (prof) prof->end(pi, st, (double)n);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  uint32_t hpass = 0, hgt[96];
  HIP_TRY_ERR(hipMemcpyAsync(&hpass, d_pass, 4, hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(hgt, d_gt, 384, hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  if (gt_out) memcpy(gt_out, hgt, 384);
  if (passed) *passed = (int)hpass;
  return ZKFL_OK;
}

// verify_round's passes with the sums and the three pairs per segment instead of per key: the
// pairs ride in every pass's own pair launch, k_round_group_prod forms the groups' values and the
// round's value is their product, so a passing round launches what verify_round launches plus
// nothing of length, and a failing one only adds k_round_final_groups.  FE(prod ML(S_g, beta)) =
// FE(ML(sum S_g, beta)) and all arithmetic is exact: the round's 384 B are verify_round's.
int verify_round_narrow(size_t n, const VerifyJob* jobs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                        size_t group, size_t narrow_min, uint32_t* group_of, std::vector<uint8_t>* group_one,
                        std::vector<uint8_t>* gt_groups, int32_t* screened, int* passed, int* narrowed,
                        uint32_t* nkeys, hipStream_t st, Profiler* prof, std::string& err) {
  const char* const where = "verify_round_narrow";
  std::vector<const VkDev*> keys;
  std::vector<uint32_t> key_of;
  std::vector<size_t> start, order;
  round_order(n, jobs, keys, key_of, start, order);
  if (nkeys) *nkeys = (uint32_t)keys.size();
  const size_t cap = round_pass_size(n, chunk);
  if (group == 0 || group > cap) {
    err = std::string(where) + ": group size outside 1 .. the pass size";
    return ZKFL_E_ARG;
  }
  const size_t G = round_group_count(n, chunk, group), gcap = (cap + group - 1) / group;
  // a segment starts with every group and at every change of key inside one
  auto seg_starts = [&](size_t off, size_t j) {
    return j % group == 0 || key_of[order[off + j]] != key_of[order[off + j - 1]];
  };
  size_t pub_words = 0, tcap = 0, scap = 0;  // the largest pass: public signals, term groups, segments
  for (size_t off = 0; off < n; off += cap) {
    size_t w = 0, t = 0, s = 0;
    for (size_t j = 0; off + j < n && j < cap; j++) {
      const size_t np = jobs[order[off + j]].vk->npub;
      w += 8 * np;
      t += (np + 1 + ROUND_TERMS - 1) / ROUND_TERMS;
      if (seg_starts(off, j)) s++;
    }
    if (w > pub_words) pub_words = w;
    if (t > tcap) tcap = t;
    if (s > scap) scap = s;
  }
  const size_t tree = (G + 63) / 64;  // the first level of the product over the groups' values

  DevBufs D;
  RoundJobDev* d_jobs;
  RoundRange* d_segs;
  RoundGroup* d_groups;
  RoundGrp* d_grps;
  const LineCoef** d_slines;
  uint32_t *d_pub, *d_proof, *d_z, *d_bstat, *d_gstat, *d_gt, *d_pass, *d_ggt, *d_gone;
  LineCoef* d_lines;
  G1Aff* d_P0;
  G1P *d_sums, *d_acc;
  int32_t* d_scr;
  Fq12 *d_f, *d_gval, *d_fa, *d_fb;
  HIP_TRY_ERR(D.get(&d_jobs, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_segs, scap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_groups, tcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_grps, gcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_slines, scap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_pub, pub_words, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_proof, cap * 64, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_z, cap * 4, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_bstat, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gstat, 2 * cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gt, 96, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_pass, 1, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_ggt, 96 * G, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gone, G, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_lines, cap * ATE_NLINES, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_P0, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_sums, 2 * cap + tcap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_acc, ROUND_NSUM * scap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_scr, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_f, 2 * (cap + ROUND_NSUM * scap), PAD), where, err);
  HIP_TRY_ERR(D.get(&d_gval, G, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_fa, tree, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_fb, (tree + 63) / 64, PAD), where, err);

  std::vector<RoundJobDev> hj(cap);
  std::vector<RoundRange> hs(scap);
  std::vector<const LineCoef*> hsl(scap);
  std::vector<RoundGrp> hgr(gcap);
  std::vector<RoundGroup> hg(tcap);
  std::vector<size_t> gfirst(cap + 1);  // job j's first term group
  std::vector<uint32_t> hpub(pub_words + 1), hproof(cap * 64), hz(cap * 4);
  std::vector<int32_t> hscr(cap);
  size_t gbase = 0, combined = 0;  // the groups of earlier passes; jobs that passed the screening
  for (size_t off = 0; off < n; off += cap) {
    const size_t m = (n - off < cap) ? n - off : cap;
    const size_t ng = (m + group - 1) / group;
    size_t w = 0, T = 0, S = 0;
    for (size_t j = 0; j < m; j++) {
      const size_t i = order[off + j];
      const VkDev* vk = jobs[i].vk;
      hj[j] = {vk->ic_table, vk->alpha, (uint64_t)w, vk->npub, 0};
      gfirst[j] = T;
      for (uint32_t t0 = 0; t0 < vk->npub + 1; t0 += ROUND_TERMS) hg[T++] = {(uint32_t)j, t0};
      if (vk->npub) memcpy(hpub.data() + w, jobs[i].pub, 32 * (size_t)vk->npub);
      w += 8 * (size_t)vk->npub;
      memcpy(hproof.data() + 64 * j, proofs + 256 * i, 256);
      memcpy(hz.data() + 4 * j, z + 16 * i, 16);
      if (j % group == 0) hgr[j / group] = {(uint32_t)j, (uint32_t)j, (uint32_t)S, (uint32_t)S};
      if (seg_starts(off, j)) {
        hs[S] = {(uint32_t)j, (uint32_t)j, 0, 0};  // the term groups' range follows below
        hsl[S] = vk->lines;
        S++;
        hgr[j / group].shi = (uint32_t)S;
      }
      hs[S - 1].hi = (uint32_t)(j + 1);
      hgr[j / group].jhi = (uint32_t)(j + 1);
      group_of[i] = (uint32_t)(gbase + j / group);
    }
    gfirst[m] = T;
    for (size_t s = 0; s < S; s++) {
      hs[s].xlo = (uint32_t)gfirst[hs[s].lo];
      hs[s].xhi = (uint32_t)gfirst[hs[s].hi];
    }
    HIP_TRY_ERR(hipMemcpyAsync(d_jobs, hj.data(), m * sizeof(RoundJobDev), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_segs, hs.data(), S * sizeof(RoundRange), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_slines, hsl.data(), S * sizeof(LineCoef*), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_grps, hgr.data(), ng * sizeof(RoundGrp), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_groups, hg.data(), T * sizeof(RoundGroup), hipMemcpyHostToDevice, st), where, err);
    if (w) HIP_TRY_ERR(hipMemcpyAsync(d_pub, hpub.data(), w * 4, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_proof, hproof.data(), m * 256, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_z, hz.data(), m * 16, hipMemcpyHostToDevice, st), where, err);

    const unsigned gb = zk_grid(m, 64);
    int pi = prof ? prof->begin("verify_round_screen", st) : -1;
    hipLaunchKernelGGL(k_round_screen, dim3(4 * gb + zk_grid(T, 64)), dim3(64), 0, st, m, gb, T,
                       (const RoundJobDev*)d_jobs, (const RoundGroup*)d_groups, (const uint32_t*)d_pub,
                       (const uint32_t*)d_proof, (const uint32_t*)d_z, d_lines, d_bstat, d_gstat, d_P0, d_sums);
    if (prof) prof->end(pi, st, (double)m);
    pi = prof ? prof->begin("verify_round_reduce", st) : -1;
    hipLaunchKernelGGL(k_round_sums<64>, dim3((unsigned)S, ROUND_NSUM), dim3(64), 0, st, m, (const RoundRange*)d_segs,
                       (const RoundGroup*)d_groups, (const uint32_t*)d_bstat, (const uint32_t*)d_gstat,
                       (const G1P*)d_sums, 1, d_acc, d_scr);
    if (prof) prof->end(pi, st, (double)m);
    const size_t nk3 = ROUND_NSUM * S;
    pi = prof ? prof->begin("verify_round_pair", st) : -1;
    const unsigned gk = zk_grid(nk3, 64);
    hipLaunchKernelGGL(k_round_pair, dim3(2 * (gb + gk)), dim3(64), 0, st, m, gb, (const G1Aff*)d_P0,
                       (const LineCoef*)d_lines, (const uint32_t*)d_bstat, (const uint32_t*)d_gstat, nk3, gk,
                       (const G1P*)d_acc, (const LineCoef* const*)d_slines, d_f);
    if (prof) prof->end(pi, st, (double)m);
    pi = prof ? prof->begin("verify_round_reduce", st) : -1;
    hipLaunchKernelGGL(k_round_group_prod, dim3((unsigned)ng), dim3(64), 0, st, m, nk3, (const RoundGrp*)d_grps,
                       (const Fq12*)d_f, d_gval + gbase);
    if (prof) prof->end(pi, st, 0.0);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(hscr.data(), d_scr, m * 4, hipMemcpyDeviceToHost, st), where, err);
    HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
    for (size_t j = 0; j < m; j++) {
      screened[order[off + j]] = hscr[j];
      if (!hscr[j]) combined++;
    }
    gbase += ng;
  }
  // the round's value: the product of the groups' values, which stay where they are
  const Fq12* in = d_gval;
  Fq12 *out = d_fa, *other = d_fb;
  int pi = prof ? prof->begin("verify_round_reduce", st) : -1;
  for (size_t cnt = G; cnt > 1;) {
    const unsigned g = zk_grid(cnt, 64);
    hipLaunchKernelGGL(k_round_prod, dim3(g), dim3(64), 0, st, cnt, in, out);
    cnt = g;
    in = out;
    out = other;
    other = const_cast<Fq12*>(in);
  }
  if (prof) prof->end(pi, st, 0.0);
  pi = prof ? prof->begin("verify_round_final", st) : -1;
  hipLaunchKernelGGL(k_round_final, dim3(1), dim3(64), 0, st, in, d_gt, d_pass);
  if (prof) prof->end(pi, st, (double)n);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  uint32_t hpass = 0;
  HIP_TRY_ERR(hipMemcpyAsync(&hpass, d_pass, 4, hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  if (passed) *passed = (int)hpass;
  const bool narrow = gt_groups || (!hpass && combined >= narrow_min);
  if (narrowed) *narrowed = narrow ? 1 : 0;
  if (!narrow) return ZKFL_OK;
  pi = prof ? prof->begin("verify_round_groups", st) : -1;
  hipLaunchKernelGGL(k_round_final_groups, dim3((unsigned)G), dim3(64), 0, st, (const Fq12*)d_gval, d_ggt, d_gone);
  if (prof) prof->end(pi, st, (double)G);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  std::vector<uint32_t> hone(G);
  HIP_TRY_ERR(hipMemcpyAsync(hone.data(), d_gone, G * 4, hipMemcpyDeviceToHost, st), where, err);
  if (gt_groups) {
    gt_groups->resize(384 * G);
    HIP_TRY_ERR(hipMemcpyAsync(gt_groups->data(), d_ggt, 384 * G, hipMemcpyDeviceToHost, st), where, err);
  }
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  group_one->assign(hone.begin(), hone.end());
  return ZKFL_OK;
}

}  // namespace zkfl
