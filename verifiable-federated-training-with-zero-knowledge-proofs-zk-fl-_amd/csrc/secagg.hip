// Secure aggregation on the GPU: pairwise masks derived, signed and summed in one kernel.
//
// Reference behaviour: derivePairwiseMask (tests/full_system_simulation.mjs:181-196) and the client's
// masking loop (:558-637), r_ij[k] = Poseidon(K_ij, round, min(i,j), max(i,j), k) and
// m_i = g_i + sum_j sigma_ij r_ij with sigma_ij = +1 when i < j, else -1 (PairwiseMaskDerivation and
// the LessThan(64) sign of src/circuits/secure_masked_update.circom:55-146); the server's
// aggregateUpdates (:1137-1199) with its signed decode (:1168-1178).  The reference sums whatever
// updates verified, which leaves sigma_ij r_ij of every excluded j in the sum; zkfl_secagg_aggregate
// takes the revealed keys of the (included, excluded) pairs and subtracts exactly those terms.
// Same values as zkfl/clients.py::pairwise_mask / secagg_input (pinned by the reference fixture).
//
// Layout (MI355X): both entries are one evaluation (csrc/secagg.h),
//     out[row][k] = base[row][k] + sum_{t in row} s_t Poseidon5(key_t, round, lo_t, hi_t, k),
// a row being a client and a term a peer (masking), or a group and an (included, excluded) pair
// (aggregation).  A row's terms are cut into chunks of chunk_terms; one lane owns one (chunk, k): it
// hashes each term of its chunk with poseidon_perm0<6> (state in VGPRs, constants through scalar loads,
// csrc/poseidon.h) and adds or subtracts the hash into an Fr it keeps in registers: the masks are not
// stored, only one partial per (chunk, k) is (with chunks of one term, the default of small jobs, a
// partial is one signed mask; secagg.h).  The lanes run over the flattened
// (chunk, k) index and not over k alone: at dim 4 a wave that spans k would use 4 of its 64 lanes.
// A term's key, ids and sign then differ between the lanes of a wave when dim < 64 and are read with
// vector loads: ~100 B against the ~3000 field multiplications of one t = 6 hash.  k_secagg_fold adds a
// row's partials, leaves Montgomery form, adds the base rows and decodes.  No atomics: modular
// addition is exact, so every chunk_terms gives the same bytes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "common.h"
#include "devbufs.h"
#include "host_parse.h"
#include "merkle.h"
#include "objects.h"
#include "poseidon.h"
#include "secagg.h"
#include "zkfl.h"

namespace zkfl {

namespace {

// a term's hash inputs besides round and k, Montgomery, and its sign
struct SecaggTerms {
  const Fr* key;       // [T], then the round at [T]
  const Fr* lo;        // [T]
  const Fr* hi;        // [T]
  const uint8_t* neg;  // [T] 1: the term is subtracted
};

ZK_DEV Fr fr_from_u64(uint64_t x) {
  Fr v = fp_zero<FrP>();
  v.v[0] = (uint32_t)x;
  v.v[1] = (uint32_t)(x >> 32);
  return fp_to_mont(v);
}

// min / max as unsigned 64-bit integers (LessThan(64)) and the sign, once per term
__global__ __launch_bounds__(256) void k_secagg_prepare(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b,
                                                        size_t n, uint32_t negate_if_less, Fr* __restrict__ lo,
                                                        Fr* __restrict__ hi, uint8_t* __restrict__ neg) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  const uint64_t x = a[t], y = b[t];
  const bool less = x < y;
  lo[t] = fr_from_u64(less ? x : y);
  hi[t] = fr_from_u64(less ? y : x);
  neg[t] = (uint8_t)(less == (negate_if_less != 0));
}

// lane i = (chunk c, coordinate k): part[c][k] = sum over the chunk's terms of +-Poseidon5 (Montgomery)
__global__ __launch_bounds__(256) void k_secagg_terms(PosConsts K, SecaggTerms tm, size_t n_terms,
                                                      const uint64_t* __restrict__ term_ptr,
                                                      const uint64_t* __restrict__ chunk_ptr,
                                                      const uint32_t* __restrict__ chunk_row, size_t n_chunks,
                                                      uint32_t dim, uint32_t chunk_terms, Fr* __restrict__ part) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_chunks * dim) return;
  const size_t c = i / dim;
  const uint32_t k = (uint32_t)(i - c * dim);
  const uint32_t row = chunk_row[c];
  const uint64_t begin = term_ptr[row] + (c - chunk_ptr[row]) * chunk_terms;
  const uint64_t row_end = term_ptr[row + 1];
  const uint64_t end = begin + chunk_terms < row_end ? begin + chunk_terms : row_end;
  const Fr kf = fr_from_u64(k);
  const Fr round = tm.key[n_terms];
  Fr acc = fp_zero<FrP>();
  for (uint64_t t = begin; t < end; t++) {
    Fr st[6];
    st[0] = fp_zero<FrP>();
    st[1] = tm.key[t];
    st[2] = round;
    st[3] = tm.lo[t];
    st[4] = tm.hi[t];
    st[5] = kf;
    const Fr h = poseidon_perm0<6>(st, K);
    acc = tm.neg[t] ? fp_sub(acc, h) : fp_add(acc, h);
  }
  part[i] = acc;
}

// value, or value - r above r / 2, when that fits an int64 (v < r)
ZK_DEV bool fr_signed64(const Fr& v, int64_t* out) {
  uint32_t high = 0;
#pragma unroll
  for (int i = 2; i < 8; i++) high |= v.v[i];
  if (high == 0 && v.v[1] < 0x80000000u) {
    *out = (int64_t)(v.v[0] | ((uint64_t)v.v[1] << 32));
    return true;
  }
  uint32_t m[8];  // r - v, in 1..r
  uint32_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const uint64_t d = (uint64_t)FrP::P[i] - v.v[i] - borrow;
    m[i] = (uint32_t)d;
    borrow = (uint32_t)(d >> 63);
  }
  high = 0;
#pragma unroll
  for (int i = 2; i < 8; i++) high |= m[i];
  const uint64_t m64 = m[0] | ((uint64_t)m[1] << 32);
  if (high == 0 && m64 <= (1ull << 63)) {
    *out = (int64_t)(0 - m64);
    return true;
  }
  *out = 0;
  return false;
}

// lane i = (row, k): out = from_mont(sum of the row's partials) + the row's base rows (std)
__global__ __launch_bounds__(256) void k_secagg_fold(size_t n_rows, uint32_t dim, const uint64_t* __restrict__ chunk_ptr,
                                                     const Fr* __restrict__ part, const uint64_t* __restrict__ base_ptr,
                                                     const Fr* __restrict__ base, Fr* __restrict__ out,
                                                     int64_t* __restrict__ signed_out, uint8_t* __restrict__ range_out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_rows * dim) return;
  const size_t row = i / dim;
  const uint32_t k = (uint32_t)(i - row * dim);
  Fr acc = fp_zero<FrP>();
  for (uint64_t c = chunk_ptr[row]; c < chunk_ptr[row + 1]; c++) acc = fp_add(acc, part[c * dim + k]);
  Fr v = fp_from_mont(acc);
  const uint64_t b0 = base_ptr ? base_ptr[row] : row, b1 = base_ptr ? base_ptr[row + 1] : row + 1;
  for (uint64_t m = b0; m < b1; m++) v = fp_add(v, base[m * dim + k]);
  out[i] = v;
  if (signed_out) {
    int64_t s;
    const bool fits = fr_signed64(v, &s);
    signed_out[i] = s;
    range_out[i] = fits ? 0 : 1;
  }
}

constexpr size_t MAX_GRID = 0x7FFFFFFFull;  // blocks of one launch

}  // namespace

uint32_t secagg_default_chunk(uint64_t terms, uint32_t dim) {
  const uint64_t c = terms * dim / SECAGG_TARGET_LANES;
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c, 1), SECAGG_MAX_CHUNK);
}

void secagg_chunk_layout(const uint64_t* term_ptr, size_t n, uint32_t ct, std::vector<uint64_t>& chunk_ptr,
                         std::vector<uint32_t>& chunk_row) {
  chunk_ptr.assign(n + 1, 0);
  for (size_t r = 0; r < n; r++) chunk_ptr[r + 1] = chunk_ptr[r] + (term_ptr[r + 1] - term_ptr[r] + ct - 1) / ct;
  chunk_row.resize((size_t)chunk_ptr[n]);  // <= T < 2^32
  for (size_t r = 0; r < n; r++)
    for (uint64_t c = chunk_ptr[r]; c < chunk_ptr[r + 1]; c++) chunk_row[c] = (uint32_t)r;
}

int secagg_eval_dev(const PosTables* P, const SecaggDev& S, hipStream_t st, Profiler* prof, std::string& err) {
  const char* const where = "secagg";
  const size_t cells = S.n_rows * S.dim, lanes = S.n_chunks * S.dim;
  if ((cells + 255) / 256 > MAX_GRID || (lanes + 255) / 256 > MAX_GRID) {
    err = "secagg: rows x dim exceeds one launch";
    return ZKFL_E_ARG;
  }
  if (lanes) {
    PosConsts K;
    pos_tables_width(P, 6, &K.C, &K.M, &K.rp);
    HIP_TRY_ERR(fr_to_mont_batch(S.raw, S.n_terms + 1, S.key, st), where, err);  // the keys and the round, once per call
    hipLaunchKernelGGL(k_secagg_prepare, dim3(zk_grid(S.n_terms, 256)), dim3(256), 0, st, S.term_a, S.term_b, S.n_terms,
                       (uint32_t)S.negate_if_less, S.lo, S.hi, S.neg);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    const SecaggTerms tm = {S.key, S.lo, S.hi, S.neg};
    const int pi = prof ? prof->begin("secagg_terms", st) : -1;
    hipLaunchKernelGGL(k_secagg_terms, dim3(zk_grid(lanes, 256)), dim3(256), 0, st, K, tm, S.n_terms, S.term_ptr,
                       S.chunk_ptr, S.chunk_row, S.n_chunks, S.dim, S.chunk_terms, S.part);
    HIP_TRY_ERR(hipGetLastError(), where, err);
    if (prof) prof->end(pi, st, (double)S.n_terms * S.dim);  // units: hashes
  }
  const int pf = prof ? prof->begin("secagg_fold", st) : -1;
  hipLaunchKernelGGL(k_secagg_fold, dim3(zk_grid(cells, 256)), dim3(256), 0, st, S.n_rows, S.dim, S.chunk_ptr, S.part,
                     S.base_ptr, S.base, S.out, S.signed_out, S.range_out);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  if (prof) prof->end(pf, st, (double)cells);
  return ZKFL_OK;
}

int secagg_run(const PosTables* P, const SecaggJob& J, hipStream_t st, Profiler* prof, std::string& err) {
  const char* const where = "secagg";
  const size_t n = J.n_rows, T = (size_t)J.term_ptr[n];
  const uint32_t dim = J.dim;
  const uint32_t ct = J.chunk_terms ? J.chunk_terms : secagg_default_chunk(T, dim);
  // a row's terms in chunks of ct: chunk_ptr[row] = its first chunk, chunk_row[c] = the chunk's row
  std::vector<uint64_t> chunk_ptr;
  std::vector<uint32_t> chunk_row;
  secagg_chunk_layout(J.term_ptr, n, ct, chunk_ptr, chunk_row);
  const size_t n_chunks = chunk_row.size();
  const size_t cells = n * dim, lanes = n_chunks * dim;
  if ((cells + 255) / 256 > MAX_GRID || (lanes + 255) / 256 > MAX_GRID) {
    err = "secagg: rows x dim exceeds one launch";
    return ZKFL_E_ARG;
  }

  DevBufs D;
  Fr *d_raw, *d_key, *d_lo, *d_hi, *d_part, *d_base, *d_out;
  uint64_t *d_a, *d_b, *d_tptr, *d_cptr, *d_bptr = nullptr;
  uint32_t* d_crow;
  uint8_t *d_neg, *d_range = nullptr;
  int64_t* d_signed = nullptr;
  HIP_TRY_ERR(D.get(&d_raw, T + 1), where, err);
  HIP_TRY_ERR(D.get(&d_key, T + 1), where, err);
  HIP_TRY_ERR(D.get(&d_lo, T), where, err);
  HIP_TRY_ERR(D.get(&d_hi, T), where, err);
  HIP_TRY_ERR(D.get(&d_neg, T), where, err);
  HIP_TRY_ERR(D.get(&d_a, T), where, err);
  HIP_TRY_ERR(D.get(&d_b, T), where, err);
  HIP_TRY_ERR(D.get(&d_tptr, n + 1), where, err);
  HIP_TRY_ERR(D.get(&d_cptr, n + 1), where, err);
  HIP_TRY_ERR(D.get(&d_crow, n_chunks), where, err);
  HIP_TRY_ERR(D.get(&d_part, lanes), where, err);
  HIP_TRY_ERR(D.get(&d_base, J.n_base * dim), where, err);
  HIP_TRY_ERR(D.get(&d_out, cells), where, err);
  if (J.base_ptr) HIP_TRY_ERR(D.get(&d_bptr, n + 1), where, err);
  if (J.signed_out) {
    HIP_TRY_ERR(D.get(&d_signed, cells), where, err);
    HIP_TRY_ERR(D.get(&d_range, cells), where, err);
  }
  if (T) {
    HIP_TRY_ERR(hipMemcpyAsync(d_raw, J.keys, T * 32, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_a, J.term_a, T * 8, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_b, J.term_b, T * 8, hipMemcpyHostToDevice, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(d_crow, chunk_row.data(), n_chunks * 4, hipMemcpyHostToDevice, st), where, err);
  }
  HIP_TRY_ERR(hipMemcpyAsync(d_raw + T, J.round, 32, hipMemcpyHostToDevice, st), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_tptr, J.term_ptr, (n + 1) * 8, hipMemcpyHostToDevice, st), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_cptr, chunk_ptr.data(), (n + 1) * 8, hipMemcpyHostToDevice, st), where, err);
  if (J.base_ptr) HIP_TRY_ERR(hipMemcpyAsync(d_bptr, J.base_ptr, (n + 1) * 8, hipMemcpyHostToDevice, st), where, err);
  if (J.n_base)
    HIP_TRY_ERR(hipMemcpyAsync(d_base, J.base, J.n_base * dim * 32, hipMemcpyHostToDevice, st), where, err);

  SecaggDev S;
  S.n_rows = n;
  S.n_terms = T;
  S.n_chunks = n_chunks;
  S.dim = dim;
  S.chunk_terms = ct;
  S.negate_if_less = J.negate_if_less;
  S.raw = d_raw;
  S.term_a = d_a;
  S.term_b = d_b;
  S.term_ptr = d_tptr;
  S.chunk_ptr = d_cptr;
  S.chunk_row = d_crow;
  S.base_ptr = d_bptr;
  S.base = d_base;
  S.key = d_key;
  S.lo = d_lo;
  S.hi = d_hi;
  S.neg = d_neg;
  S.part = d_part;
  S.out = d_out;
  S.signed_out = d_signed;
  S.range_out = d_range;
  if (int rc = secagg_eval_dev(P, S, st, prof, err)) return rc;
  HIP_TRY_ERR(hipMemcpyAsync(J.out, d_out, cells * 32, hipMemcpyDeviceToHost, st), where, err);
  if (J.signed_out) {
    HIP_TRY_ERR(hipMemcpyAsync(J.signed_out, d_signed, cells * 8, hipMemcpyDeviceToHost, st), where, err);
    HIP_TRY_ERR(hipMemcpyAsync(J.range_out, d_range, cells, hipMemcpyDeviceToHost, st), where, err);
  }
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  return ZKFL_OK;
}

}  // namespace zkfl

namespace {

int arg_fail(const char* who, const std::string& msg) { return fail(ZKFL_E_ARG, std::string(who) + ": " + msg); }

int check_lt_r(const char* who, const uint8_t* v, size_t count, const char* what) {
  for (size_t i = 0; i < count; i++) {
    uint32_t w[8];
    memcpy(w, v + 32 * i, 32);
    if (!fr_lt_r(w)) return arg_fail(who, std::string(what) + " " + std::to_string(i) + " is not < r");
  }
  return ZKFL_OK;
}

// ptr[0] = 0, ptr non-decreasing; *total = ptr[n]
int check_csr(const char* who, const char* name, const uint64_t* ptr, size_t n, uint64_t* total) {
  if (ptr[0] != 0) return arg_fail(who, std::string(name) + "[0] must be 0");
  for (size_t i = 0; i < n; i++)
    if (ptr[i + 1] < ptr[i])
      return arg_fail(who, std::string(name) + "[" + std::to_string(i + 1) + "] is below " + name + "[" +
                               std::to_string(i) + "]");
  *total = ptr[n];
  return ZKFL_OK;
}

int run_job(zkfl_ctx* ctx, const SecaggJob& J) {
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = pos_ready(ctx);
  if (rc) return rc;
  std::string err;
  rc = secagg_run(ctx->pos, J, ctx->st, &ctx->prof, err);
  return rc ? fail(rc, err) : ZKFL_OK;
}

}  // namespace

extern "C" int zkfl_secagg_mask(zkfl_ctx* ctx, size_t n, uint32_t dim, const uint64_t* ids, const uint64_t* peer_ptr,
                                const uint64_t* peer_ids, const uint8_t* keys, const uint8_t round[32],
                                const uint8_t* gradients, uint8_t* masked_out, uint32_t chunk_terms) {
  const char* const who = "secagg_mask";
  if (!ctx) return arg_fail(who, "null context");
  if (dim == 0) return arg_fail(who, "dim must be at least 1");
  if (!peer_ptr || !round || (n && (!ids || !gradients || !masked_out))) return arg_fail(who, "null argument");
  if (n >= (1ull << 32)) return arg_fail(who, "n must be < 2^32");
  uint64_t T = 0;
  int rc = check_csr(who, "peer_ptr", peer_ptr, n, &T);
  if (rc) return rc;
  if (T >= (1ull << 32))
    return arg_fail(who, "peer_ptr[" + std::to_string(n) + "] = " + std::to_string(T) + " peers: must be < 2^32");
  if (T && (!peer_ids || !keys)) return arg_fail(who, "null argument");
  if ((rc = check_lt_r(who, round, 1, "round"))) return rc;
  if ((rc = check_lt_r(who, keys, T, "key"))) return rc;
  if ((rc = check_lt_r(who, gradients, n * dim, "gradient value"))) return rc;
  std::vector<uint64_t> own(T);
  std::vector<std::pair<uint64_t, uint64_t>> seen;
  for (size_t i = 0; i < n; i++) {
    seen.clear();
    for (uint64_t t = peer_ptr[i]; t < peer_ptr[i + 1]; t++) {
      if (peer_ids[t] == ids[i])
        return arg_fail(who, "client " + std::to_string(i) + ": peer_ids[" + std::to_string(t) + "] is the client's own id");
      own[t] = ids[i];
      seen.emplace_back(peer_ids[t], t);
    }
    std::sort(seen.begin(), seen.end());
    for (size_t q = 1; q < seen.size(); q++)
      if (seen[q].first == seen[q - 1].first)
        return arg_fail(who, "client " + std::to_string(i) + ": peer_ids[" + std::to_string(seen[q].second) +
                                 "] repeats peer_ids[" + std::to_string(seen[q - 1].second) + "]");
  }
  if (!n) return ZKFL_OK;
  SecaggJob J;
  J.n_rows = n;
  J.dim = dim;
  J.term_ptr = peer_ptr;
  J.term_a = own.data();
  J.term_b = peer_ids;
  J.negate_if_less = false;  // sigma_ij = +1 when i < j
  J.keys = keys;
  J.round = round;
  J.base = gradients;
  J.n_base = n;
  J.out = masked_out;
  J.chunk_terms = chunk_terms;
  return run_job(ctx, J);
}

extern "C" int zkfl_secagg_aggregate(zkfl_ctx* ctx, size_t n_groups, uint32_t dim, const uint64_t* member_ptr,
                                     const uint8_t* masked, const uint64_t* pair_ptr, const uint64_t* pair_in,
                                     const uint64_t* pair_out, const uint8_t* pair_keys, const uint8_t round[32],
                                     uint8_t* sum_out, int64_t* signed_out, uint8_t* out_of_range,
                                     uint32_t chunk_terms) {
  const char* const who = "secagg_aggregate";
  if (!ctx) return arg_fail(who, "null context");
  if (dim == 0) return arg_fail(who, "dim must be at least 1");
  if (!member_ptr || !pair_ptr || !round || (n_groups && !sum_out)) return arg_fail(who, "null argument");
  if (n_groups >= (1ull << 32)) return arg_fail(who, "n_groups must be < 2^32");
  uint64_t M = 0, P = 0;
  int rc = check_csr(who, "member_ptr", member_ptr, n_groups, &M);
  if (rc) return rc;
  if ((rc = check_csr(who, "pair_ptr", pair_ptr, n_groups, &P))) return rc;
  if (P >= (1ull << 32))
    return arg_fail(who, "pair_ptr[" + std::to_string(n_groups) + "] = " + std::to_string(P) + " pairs: must be < 2^32");
  if ((M && !masked) || (P && (!pair_in || !pair_out || !pair_keys))) return arg_fail(who, "null argument");
  if ((rc = check_lt_r(who, round, 1, "round"))) return rc;
  if ((rc = check_lt_r(who, pair_keys, P, "pair key"))) return rc;
  if ((rc = check_lt_r(who, masked, M * dim, "masked value"))) return rc;
  for (uint64_t t = 0; t < P; t++)
    if (pair_in[t] == pair_out[t]) return arg_fail(who, "pair " + std::to_string(t) + ": pair_in equals pair_out");
  if (!n_groups) return ZKFL_OK;
  const size_t cells = n_groups * (size_t)dim;
  std::vector<int64_t> sg((signed_out || out_of_range) ? cells : 0);
  std::vector<uint8_t> rg(sg.size());
  SecaggJob J;
  J.n_rows = n_groups;
  J.dim = dim;
  J.term_ptr = pair_ptr;
  J.term_a = pair_in;
  J.term_b = pair_out;
  J.negate_if_less = true;  // the sum holds +sigma_ij r_ij of each pair: take it out
  J.keys = pair_keys;
  J.round = round;
  J.base_ptr = member_ptr;
  J.base = masked;
  J.n_base = M;
  J.out = sum_out;
  J.signed_out = sg.empty() ? nullptr : sg.data();
  J.range_out = sg.empty() ? nullptr : rg.data();
  J.chunk_terms = chunk_terms;
  if ((rc = run_job(ctx, J))) return rc;
  // a group with a coordinate outside int64 reads all zero and raises its flag
  for (size_t g = 0; g < n_groups && !sg.empty(); g++) {
    bool bad = false;
    for (uint32_t k = 0; k < dim; k++) bad |= rg[g * dim + k] != 0;
    if (out_of_range) out_of_range[g] = bad ? 1 : 0;
    if (signed_out)
      for (uint32_t k = 0; k < dim; k++) signed_out[g * dim + k] = bad ? 0 : sg[g * dim + k];
  }
  return ZKFL_OK;
}
