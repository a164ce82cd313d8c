// GPU Groth16 verification, one proof per WAVEFRONT: the latency path behind
// zkfl_groth16_verify_multi (ZKFL_VERIFY_WAVES) and zkfl_debug_wave_pairing.
//
// csrc/verify.hip puts a proof in one lane: right for thousands of proofs, but one proof -- or a
// federated round's 16 -- is then one lane's serial chain.  The reference's server verifies each
// proof as its client produces it, phase by phase with three different keys
// (tests/full_system_simulation.mjs:1298-1343).  Here a workgroup is one wavefront and the wave
// shares one proof (csrc/pairing_wave.h).  Verdict rules are verify.hip's, decided by the same
// helpers (csrc/verify_dev.h).
//
// Kernels per call, each job with its own key:
//   k_wave_g2_prepare ("verify_wave_g2")     pi_b: decoding, subgroup test, 102 line coefficients;
//   k_wave_inputs     ("verify_wave_inputs") pi_a / pi_c / public-signal checks; vk_x with one lane
//                                            per 4-bit window over per-key tables d 16^w IC_i,
//                                            a tree sum over the wave, one inversion;
//   k_wave_miller     ("verify_wave_pair")   3-pair Miller loop, times the key's Miller value of
//                                            (alpha1, beta2), final exponentiation, compare with 1.
#include <hip/hip_runtime.h>
#include <string.h>

#include "common.h"
#include "curve.h"
#include "devbufs.h"
#include "pairing_wave.h"
#include "verify.h"
#include "verify_dev.h"
#include "zkfl.h"

namespace zkfl {

namespace {

// what a job's kernels read of its key
struct WaveJob {
  const G1Aff* wtab;       // [npub][64][16]: d * 16^w * IC_{i+1}
  const G1Aff* ic_table;   // the lane path's table; entry 1 = IC0
  const LineCoef* lines;   // [3][ATE_NLINES]: beta2, gamma2, delta2
  const Fq12* f_ab;
  uint32_t npub;
  uint32_t pub_off;        // first public signal of the job, in signals
};

// Order-r membership of a twist point: [u]Q across the wave, then the endomorphism criterion of
// verify.hip on lane 0 (complete XYZZ formulas; ~60 Fq2 products out of the test's ~1300).
ZK_DEV bool wv_g2_in_subgroup(WaveLds* s, const G2Aff& q) {
  const G2Proj R = wv_g2_mul_u(s, q.x, q.y);
  if (threadIdx.x == 0) {
    uint32_t ok = 0;
    if (!f2_is_zero(R.Z)) {
      // (X/Z, Y/Z) as XYZZ with ZZ = Z^2, ZZZ = Z^3
      G2P xp;
      xp.ZZ = f2_sqr(R.Z);
      xp.ZZZ = f2_mul(xp.ZZ, R.Z);
      xp.X = f2_mul(R.X, R.Z);
      xp.Y = f2_mul(R.Y, xp.ZZ);
      ok = g2_subgroup_criterion(xyzz_from_affine<Fq2Ops>(q), xp) ? 1u : 0u;
    }
    s->flag = ok;
  }
  __syncthreads();
  const bool r = s->flag != 0;
  __syncthreads();
  return r;
}

// Two workgroups per G2 point, since its two chains are independent: the even one writes the
// ATE_NLINES line coefficients of a point that is on the twist (whatever the subgroup test will
// say: nobody reads the lines of a point whose status is not 0), the odd one runs the subgroup
// test and writes the status.  p_std (nullable): the pair's G1 point is decoded alongside (the
// pairing hook).
__global__ __launch_bounds__(64) void k_wave_g2_prepare(const uint32_t* q_std, size_t q_stride, LineCoef* lines,
                                                        uint32_t* qstat, const uint32_t* p_std, G1Aff* p_out,
                                                        uint32_t* pstat) {
  __shared__ WaveLds s;
  const size_t i = blockIdx.x >> 1;
  G2Aff q;
  uint32_t st = g2_load(q_std + i * q_stride, q);  // every lane: the wave holds the point
  if ((blockIdx.x & 1) == 0) {
    if (p_std && threadIdx.x == 0) {
      G1Aff p;
      uint32_t pst = g1_load(p_std + i * 16, p);
      if (pst) p.x = p.y = fp_zero<FqP>();
      p_out[i] = p;
      pstat[i] = pst;
    }
    if (st == 0) wv_g2_prepare_lines(&s, q.x, q.y, lines + i * ATE_NLINES);
  } else {
    if (st == 0 && !wv_g2_in_subgroup(&s, q)) st = ST_BAD;
    if (threadIdx.x == 0) qstat[i] = st;
  }
}

// d * 16^w * IC_i, d = 0..15, affine Montgomery: one thread per (i, w), i = 1..npub
__global__ __launch_bounds__(64) void k_wave_ic_tables(uint32_t npub, const uint32_t* ic_std, G1Aff* table) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= npub * 64) return;
  const uint32_t i = t >> 6, w = t & 63;
  G1Aff p;
  const uint32_t st = g1_load(ic_std + (size_t)(i + 1) * 16, p);
  G1Aff* row = table + (size_t)t * 16;
  const G1Aff zero = {fp_zero<FqP>(), fp_zero<FqP>()};
  row[0] = zero;
  if (st) {  // infinity (an invalid point never gets here: vk_prepare rejected the key)
    for (int j = 1; j < 16; j++) row[j] = zero;
    return;
  }
  G1P b = xyzz_from_affine<FqOps>(p);
  for (uint32_t k = 0; k < 4 * w; k++) b = xyzz_dbl<FqOps>(b);
  p = xyzz_to_affine<FqOps>(b);  // never infinity: 16^w is not a multiple of r
  G1P m[16];
  m[1] = xyzz_from_affine<FqOps>(p);
  for (int j = 2; j < 16; j++) m[j] = xyzz_madd<FqOps>(m[j - 1], p);
  Fq pre[16];
  pre[1] = m[1].ZZZ;
  for (int j = 2; j < 16; j++) pre[j] = fp_mul(pre[j - 1], m[j].ZZZ);
  Fq inv = fp_inv(pre[15]);
  for (int j = 15; j >= 1; j--) {
    Fq iZZZ = (j > 1) ? fp_mul(inv, pre[j - 1]) : inv;
    if (j > 1) inv = fp_mul(inv, m[j].ZZZ);
    Fq iZ = fp_mul(m[j].ZZ, iZZZ);
    row[j].x = fp_mul(m[j].X, fp_sqr(iZ));
    row[j].y = fp_mul(m[j].Y, iZZZ);
  }
}

// Per proof (workgroup): public-signal range, pi_a / pi_c checks, vk_x; writes the 3 G1 points of
// the pairing product (-pi_a, vk_x, pi_c) and a status (0 ok, else invalid) -- k_verify_inputs'
// outputs.
__global__ __launch_bounds__(64) void k_wave_inputs(const WaveJob* jobs, const uint32_t* pubs, const uint32_t* proofs,
                                                    const uint32_t* bstat, G1Aff* P, uint32_t* status) {
  __shared__ G1P part[64];
  __shared__ G1Aff ac[2];
  __shared__ uint32_t st_ac[2], bad_s;
  const size_t k = blockIdx.x;
  const uint32_t l = threadIdx.x;
  const WaveJob J = jobs[k];
  const uint32_t* pub = pubs + (size_t)J.pub_off * 8;
  const uint32_t* pr = proofs + k * 64;
  const uint32_t bst = bstat[k];
  if (l == 0) bad_s = (bst & ST_BAD) ? 1u : 0u;
  __syncthreads();
  uint32_t bad = 0;
  for (uint32_t i = l; i < J.npub; i += 64)
    if (!lt_mod(pub + i * 8, FrP::P)) bad |= 2u;
  if (l < 2) {
    G1Aff p;
    const uint32_t st = g1_load(pr + (l ? 48 : 0), p);
    ac[l] = p;
    st_ac[l] = st;
    if (st & ST_BAD) bad |= 4u;
  }
  if (bad) atomicOr(&bad_s, bad);
  __syncthreads();
  bad = bad_s;
  G1Aff* out = P + k * 3;
  const G1Aff zero = {fp_zero<FqP>(), fp_zero<FqP>()};
  if (bad) {
    if (l == 0) {
      status[k] = bad;
      out[0] = out[1] = out[2] = zero;
    }
    return;
  }
  // lane w: sum over the signals of digit_w(pub_i) * 16^w * IC_i
  G1P acc = xyzz_inf<FqOps>();
  for (uint32_t i = 0; i < J.npub; i++) {
    const uint32_t dig = (pub[i * 8 + (l >> 3)] >> ((l & 7) * 4)) & 15u;
    if (dig) acc = xyzz_madd<FqOps>(acc, J.wtab[((size_t)i * 64 + l) * 16 + dig]);
  }
  part[l] = acc;
  __syncthreads();
  for (uint32_t h = 32; h >= 1; h >>= 1) {
    if (l < h) {
      acc = xyzz_add<FqOps>(acc, part[l + h]);
      part[l] = acc;
    }
    __syncthreads();
  }
  if (l == 0) {
    acc = xyzz_madd<FqOps>(acc, J.ic_table[1]);  // 1 * IC0
    // pair (-A, B) vanishes when either is infinity
    out[0] = (st_ac[0] == ST_INF || bst == ST_INF) ? zero : aff_neg<FqOps>(ac[0]);
    out[1] = xyzz_to_affine<FqOps>(acc);
    out[2] = ac[1];
    status[k] = 0;
  }
}

// Per item (workgroup): f = Miller loop over npairs pairs.  Pair 0 uses the item's own lines;
// with jobs, pairs 1 and 2 use the key's gamma2 / delta2 lines and f is multiplied by the key's
// Miller value of (alpha1, beta2).  Optionally the final exponentiation; writes f (std form)
// and/or result = (status ok && f == 1).
__global__ __launch_bounds__(64) void k_wave_miller(int npairs, const G1Aff* P, const LineCoef* own_lines,
                                                    const WaveJob* jobs, const uint32_t* status, int do_final,
                                                    uint32_t* f_std, int32_t* result) {
  __shared__ WaveLds s;
  const size_t k = blockIdx.x;
  if (status && status[k]) {
    if (result && threadIdx.x == 0) result[k] = 0;
    return;
  }
  const LineCoef* lines[3] = {own_lines + k * ATE_NLINES, nullptr, nullptr};
  if (jobs) {
    lines[1] = jobs[k].lines + ATE_NLINES;      // gamma2
    lines[2] = jobs[k].lines + 2 * ATE_NLINES;  // delta2
  }
  wv_miller(&s, 0, npairs, P + k * npairs, lines);
  if (jobs) {
    wv_load_f12(&s, 1, jobs[k].f_ab);
    wv_mul(&s, 0, 0, 1);
  }
  if (do_final) wv_final_exp(&s);
  if (f_std) wv_store_std(&s, 0, f_std + k * 96);
  if (result && threadIdx.x == 0) result[k] = wv_is_one(&s, 0) ? 1 : 0;
}

constexpr size_t PAD = 16;  // bytes behind every allocation of this unit

}  // namespace

int vk_wave_tables(const VkDev* vk, hipStream_t st, void** out, std::string& err) {
  *out = nullptr;
  const uint32_t npub = vk->npub;
  if (npub == 0 || npub > ZKFL_VERIFY_WAVE_MAX_PUBLIC) return ZKFL_OK;
  DevBufs D;
  uint32_t* d_ic;
  G1Aff* tab;
  const size_t ic_bytes = 64ull * (npub + 1);
  const char* const where = "vk_wave_tables";
  HIP_TRY_ERR(D.get(&d_ic, ic_bytes / 4, PAD), where, err);
  HIP_TRY_ERR(D.get(&tab, (size_t)npub * 64 * 16, PAD), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_ic, vk->bytes.data() + 4 + 448, ic_bytes, hipMemcpyHostToDevice, st), where, err);
  hipLaunchKernelGGL(k_wave_ic_tables, dim3(npub), dim3(64), 0, st, npub, (const uint32_t*)d_ic, tab);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  *out = D.keep(tab);  // vk_wave_tables_free's from here on
  return ZKFL_OK;
}

void vk_wave_tables_free(void* tab) {
  if (tab) (void)hipFree(tab);
}

int verify_wave(size_t n, const VerifyJob* jobs, const uint8_t* proofs, int32_t* results, hipStream_t st,
                Profiler* prof, std::string& err) {
  if (n == 0) return ZKFL_OK;
  const size_t CH = 4096;  // proofs per chunk: 4096 x 102 lines x 192 B = 80 MB of lines
  const size_t cap = n < CH ? n : CH;
  // job descriptors and public signals, packed in job order
  std::vector<WaveJob> hj(n);
  std::vector<uint8_t> hpub;
  size_t max_pub = 1;
  for (size_t i = 0; i < n; i++) {
    const VkDev* vk = jobs[i].vk;
    hj[i] = {(const G1Aff*)jobs[i].wtab, vk->ic_table, vk->lines, vk->f_ab, vk->npub, 0};
  }
  for (size_t off = 0; off < n; off += cap) {  // offsets restart in every chunk
    size_t m = (n - off < cap) ? n - off : cap, words = 0;
    for (size_t i = off; i < off + m; i++) {
      hj[i].pub_off = (uint32_t)words;
      words += hj[i].npub;
    }
    if (words > max_pub) max_pub = words;
  }
  DevBufs D;
  WaveJob* d_jobs;
  uint32_t *d_pub, *d_proof, *d_bstat, *d_status;
  LineCoef* d_lines;
  G1Aff* d_P;
  int32_t* d_res;
  const char* const where = "verify_wave";
  HIP_TRY_ERR(D.get(&d_jobs, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_pub, max_pub * 8, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_proof, cap * 64, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_bstat, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_status, cap, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_lines, cap * ATE_NLINES, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_P, cap * 3, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_res, cap, PAD), where, err);
  for (size_t off = 0; off < n; off += cap) {
    const size_t m = (n - off < cap) ? n - off : cap;
    hpub.clear();
    for (size_t i = off; i < off + m; i++) hpub.insert(hpub.end(), jobs[i].pub, jobs[i].pub + 32ull * hj[i].npub);
    HIP_TRY_ERR(hipMemcpyAsync(d_jobs, hj.data() + off, m * sizeof(WaveJob), hipMemcpyHostToDevice, st), where, err);
    if (!hpub.empty())
      HIP_TRY_ERR(hipMemcpyAsync(d_pub, hpub.data(), hpub.size(), hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_proof, proofs + off * 256, m * 256, hipMemcpyHostToDevice, st), where, err);
    const dim3 g((unsigned)m), b(64);
    int pi = prof ? prof->begin("verify_wave_g2", st) : -1;
    hipLaunchKernelGGL(k_wave_g2_prepare, dim3(2 * g.x), b, 0, st, (const uint32_t*)(d_proof + 16), (size_t)64, d_lines, d_bstat,
                       (const uint32_t*)nullptr, (G1Aff*)nullptr, (uint32_t*)nullptr);
    if (prof) prof->end(pi, st, (double)m);
    pi = prof ? prof->begin("verify_wave_inputs", st) : -1;
    hipLaunchKernelGGL(k_wave_inputs, g, b, 0, st, (const WaveJob*)d_jobs, (const uint32_t*)d_pub,
                       (const uint32_t*)d_proof, (const uint32_t*)d_bstat, d_P, d_status);
    if (prof) prof->end(pi, st, (double)m);
    pi = prof ? prof->begin("verify_wave_pair", st) : -1;
    hipLaunchKernelGGL(k_wave_miller, g, b, 0, st, 3, (const G1Aff*)d_P, (const LineCoef*)d_lines,
                       (const WaveJob*)d_jobs, (const uint32_t*)d_status, 1, (uint32_t*)nullptr, d_res);
    if (prof) prof->end(pi, st, (double)m);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(results + off, d_res, m * 4, hipMemcpyDeviceToHost, st), where, err);
    HIP_TRY_ERR(hipStreamSynchronize(st), where, err);  // hpub is reused by the next chunk
  }
  return ZKFL_OK;
}

int pairing_wave_batch(size_t n, const uint8_t* g1, const uint8_t* g2, int final_exp, uint8_t* out, hipStream_t st,
                       Profiler* prof, std::string& err) {
  if (n == 0) return ZKFL_OK;
  DevBufs D;
  uint32_t *d_g1, *d_g2, *d_stat, *d_out;
  LineCoef* d_lines;
  G1Aff* d_P;
  const char* const where = "pairing_wave_batch";
  HIP_TRY_ERR(D.get(&d_g1, n * 16, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_g2, n * 32, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_stat, 2 * n, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_lines, n * ATE_NLINES, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_P, n, PAD), where, err);
  HIP_TRY_ERR(D.get(&d_out, n * 96, PAD), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_g1, g1, n * 64, hipMemcpyHostToDevice, st), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_g2, g2, n * 128, hipMemcpyHostToDevice, st), where, err);
  std::vector<uint32_t> stat(2 * n);
  const dim3 g((unsigned)n), b(64);
  int pi = prof ? prof->begin("verify_wave_g2", st) : -1;
  hipLaunchKernelGGL(k_wave_g2_prepare, dim3(2 * g.x), b, 0, st, (const uint32_t*)d_g2, (size_t)32, d_lines, d_stat + n,
                     (const uint32_t*)d_g1, d_P, d_stat);
  if (prof) prof->end(pi, st, (double)n);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(stat.data(), d_stat, 2 * n * 4, hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  if (const int rc = pairing_points_check(stat, n, err)) return rc;
  HIP_TRY_ERR(pairing_fix_infinity(stat, n, d_P, st), where, err);
  pi = prof ? prof->begin("verify_wave_pair", st) : -1;
  hipLaunchKernelGGL(k_wave_miller, g, b, 0, st, 1, (const G1Aff*)d_P, (const LineCoef*)d_lines,
                     (const WaveJob*)nullptr, (const uint32_t*)nullptr, final_exp, d_out, (int32_t*)nullptr);
  if (prof) prof->end(pi, st, (double)n);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(out, d_out, n * 384, hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  return ZKFL_OK;
}

}  // namespace zkfl
