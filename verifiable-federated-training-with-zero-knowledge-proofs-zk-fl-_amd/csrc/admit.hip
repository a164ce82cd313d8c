// Admitting a round on the GPU: the server's binding and commitment checks, then the proofs.
//
// Reference behaviour: the Server class of tests/full_system_simulation.mjs.  verifyBalanceProof
// (:848-880) compares public signal 1 with the claimed root_D; verifyTrainingProof (:886-990) wants
// an accepted balance proof, the same root_D as that proof's package, signals 2, 3, 4, 1 equal to the
// package's root_D, root_G, root_W and round, signal 5 equal to the server's tauSquared, and root_G
// equal to gradientCommitment(gradient, clientId, round) = Poseidon(vectorHash(g), Poseidon(id, round))
// (:139-164) over the signed gradient (a negative g is r - |g|, :955);
// verifySecureAggregationProof (:995-1131) wants an accepted training proof, root_G, root_D and
// root_W bound to the earlier packages, signals 0..6 equal to the id, the round, the four roots and
// tauSquared, and signals 7.. equal to masked_update.  Each then runs `snarkjs groth16 verify`.
// The codes, their order and the three added checks are in include/zkfl.h.
//
// Layout (MI355X): everything is uploaded once.  All comparisons are between standard-form values
// and are 8-dword equalities; only the gradient commitment needs field work.  For dim > 16
// k_admit_signed maps the gradients into the field and k_admit_chunks hashes their full 16-value
// chunks with lanes over (client, chunk) -- a lane per client alone would run a client's chunk hashes
// one after the other -- in ONE launch, the short last chunk taking one launch of the device Poseidon
// of its width (poseidon_rows, csrc/merkle.h); the chunk hashes stay in Montgomery form.  The global
// model's weights ride along as one more row, so weightCommitment costs no chunk launch of its own.  k_admit_clients then runs one lane per client: the top hash (of the gradient
// itself for dim <= 16, of the chunk hashes above), Poseidon(id, round), the commitment, every
// comparison in the reference's order, and the three static codes.  The hashes are poseidon_perm0<T>
// with the context's tables (csrc/poseidon.h): state in VGPRs, constants through scalar loads.  The
// width T is the same for every lane of a launch, so it is a template parameter and the kernel is
// instantiated for T = 2..17.  No atomics: a lane owns its client's three codes.
//
// The present packages whose static code is 0 go to the multi-key verifier (or the round verifier) in
// one call; the cross-phase rules (T_NO_BALANCE, S_NO_TRAINING) and the proof verdicts are folded on
// the host, n x 3 integers.
#include <hip/hip_runtime.h>
#include <string.h>

#include <string>
#include <vector>

#include "admit.h"
#include "common.h"
#include "devbufs.h"
#include "host_parse.h"
#include "merkle.h"
#include "objects.h"
#include "poseidon.h"
#include "verify.h"
#include "zkfl.h"

namespace zkfl {

namespace {

struct AdmitDev {
  size_t n;
  uint32_t dim, nch, s_npub, flags;
  const uint64_t* ids;
  const Fr* server;  // std: [0] round, [1] tauSquared, [2] weightCommitment(weights)
  const uint8_t *b_present, *t_present, *s_present;
  const Fr *b_claimed, *t_claimed, *s_claimed;  // std
  const Fr *b_sig, *t_sig, *s_sig;              // std
  const int64_t* grad;
  const Fr* masked;  // std
  const Fr* chunk;   // [(n + 1) x nch] Montgomery chunk hashes (dim > 16); row n: the weights'
  const Fr* weights;  // [dim] std (dim <= 16)
  Fr* wc_out;         // = server + 2
  uint32_t weights_pass;
  const uint64_t *peer_ptr, *peer_ids;
  uint32_t* codes;  // [3 x n]
};

ZK_DEV bool fr_same(const Fr& a, const Fr& b) {
  uint32_t d = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) d |= a.v[i] ^ b.v[i];
  return d == 0;
}

// a std-form value against an unsigned 64-bit integer
ZK_DEV bool fr_is_u64(const Fr& a, uint64_t x) {
  uint32_t d = (a.v[0] ^ (uint32_t)x) | (a.v[1] ^ (uint32_t)(x >> 32));
#pragma unroll
  for (int i = 2; i < 8; i++) d |= a.v[i];
  return d == 0;
}

// dim > 16: the gradients as standard-form field elements, the input of the chunk pass
__global__ __launch_bounds__(256) void k_admit_signed(const int64_t* __restrict__ grad, size_t count,
                                                      Fr* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = fr_from_i64(grad[i]);
}

// dim > 16: lane = (row, full chunk c): chunk[row][c] = Poseidon of the row's 16 values of chunk c,
// Montgomery.  One launch for all full chunks of all rows (a launch per chunk, as the device vector
// hash makes them, pays the t = 17 kernel's scratch set-up once per chunk: DESIGN.md).
__global__ __launch_bounds__(256) void k_admit_chunks(PosConsts K, const Fr* __restrict__ rows, size_t n_rows,
                                                      uint32_t dim, uint32_t nch, uint32_t full,
                                                      Fr* __restrict__ chunk) {
  const size_t lane = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (lane >= n_rows * full) return;
  const size_t row = lane / full;
  const uint32_t c = (uint32_t)(lane - row * full);
  const Fr* in = rows + row * dim + (size_t)c * VHASH_CHUNK;  // c < full = dim / 16: 16 values are there
  Fr st[VHASH_CHUNK + 1];
  st[0] = fp_zero<FrP>();
#pragma unroll
  for (int k = 0; k < (int)VHASH_CHUNK; k++) st[k + 1] = fp_to_mont(in[k]);
  chunk[row * nch + c] = poseidon_perm0<VHASH_CHUNK + 1>(st, K);
}

// One lane per client; T - 1 = the inputs of the top hash (dim, or the chunk count above 16).
// With D.weights_pass the launch is one lane that finishes weightCommitment(weights) instead -- the
// same top hash over the weights (dim <= 16) or over their chunk hashes, row n of D.chunk -- and
// writes it to D.wc_out for the launch that follows.
template <int T>
__global__ __launch_bounds__(256) void k_admit_clients(PosConsts K, PosConsts K3, AdmitDev D) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool wpass = D.weights_pass != 0;  // uniform; lane 0 reads client 0's rows below but uses none
  if (wpass ? i != 0 : i >= D.n) return;
  const bool has_b = D.b_present[i] != 0, has_t = D.t_present[i] != 0, has_s = D.s_present[i] != 0;
  const Fr* bc = D.b_claimed + i * ADMIT_B_FIELDS;  // root_D
  const Fr* tc = D.t_claimed + i * ADMIT_T_FIELDS;  // root_D, root_G, root_W, round
  const Fr* sc = D.s_claimed + i * ADMIT_S_FIELDS;  // root_D, root_G, root_W, root_K, round
  const Fr srv_round = D.server[0], tau = D.server[1];

  uint32_t cb = ZKFL_ADMIT_OK;
  if (!has_b) {
    cb = ZKFL_ADMIT_B_MISSING;
  } else if (!fr_same(D.b_sig[i * ADMIT_B_NPUB + 1], bc[0])) {
    cb = ZKFL_ADMIT_B_SIG_ROOT_D;
  }

  uint32_t ct = ZKFL_ADMIT_OK;
  if (wpass) {
    // nothing to compare: straight to the hash
  } else if (!has_t) {
    ct = ZKFL_ADMIT_T_MISSING;
  } else {
    const Fr* sig = D.t_sig + i * ADMIT_T_NPUB;
    if (has_b && !fr_same(tc[0], bc[0])) ct = ZKFL_ADMIT_T_BIND_ROOT_D;
    else if (!fr_same(sig[2], tc[0])) ct = ZKFL_ADMIT_T_SIG_ROOT_D;
    else if (!fr_same(sig[3], tc[1])) ct = ZKFL_ADMIT_T_SIG_ROOT_G;
    else if (!fr_same(sig[4], tc[2])) ct = ZKFL_ADMIT_T_SIG_ROOT_W;
    else if (!fr_same(sig[1], tc[3])) ct = ZKFL_ADMIT_T_SIG_ROUND;
    else if ((D.flags & ZKFL_ADMIT_CHECK_ROUND) && !fr_same(tc[3], srv_round)) ct = ZKFL_ADMIT_T_ROUND_STALE;
    else if (!fr_same(sig[5], tau)) ct = ZKFL_ADMIT_T_SIG_TAU;
  }
  if (ct == ZKFL_ADMIT_OK) {  // root_G from the submitted gradient
    Fr st[T];
    st[0] = fp_zero<FrP>();
    if (D.nch) {  // the client's chunk hashes, or the weights' (row n)
      const Fr* row = D.chunk + (wpass ? D.n : i) * D.nch;
#pragma unroll
      for (int k = 1; k < T; k++) st[k] = row[k - 1];
    } else if (wpass) {
#pragma unroll
      for (int k = 1; k < T; k++) st[k] = fp_to_mont(D.weights[k - 1]);
    } else {
#pragma unroll
      for (int k = 1; k < T; k++) st[k] = fp_to_mont(fr_from_i64(D.grad[i * D.dim + (k - 1)]));
    }
    const Fr grad_hash = poseidon_perm0<T>(st, K);
    if (wpass) {
      *D.wc_out = fp_from_mont(grad_hash);
      return;
    }
    Fr id = fp_zero<FrP>();
    id.v[0] = (uint32_t)D.ids[i];
    id.v[1] = (uint32_t)(D.ids[i] >> 32);
    Fr s3[3] = {fp_zero<FrP>(), fp_to_mont(id), fp_to_mont(tc[3])};
    const Fr meta = poseidon_perm0<3>(s3, K3);
    s3[0] = fp_zero<FrP>();
    s3[1] = grad_hash;
    s3[2] = meta;
    const Fr root_g = fp_from_mont(poseidon_perm0<3>(s3, K3));
    if (!fr_same(root_g, tc[1])) ct = ZKFL_ADMIT_T_ROOT_G_GRADIENT;
    else if ((D.flags & ZKFL_ADMIT_CHECK_MODEL) && !fr_same(tc[2], D.server[2])) ct = ZKFL_ADMIT_T_ROOT_W_MODEL;
  }

  uint32_t cs = ZKFL_ADMIT_OK;
  if (!has_s) {
    cs = ZKFL_ADMIT_S_MISSING;
  } else {
    const Fr* sig = D.s_sig + i * D.s_npub;
    if (has_t && !fr_same(sc[1], tc[1])) cs = ZKFL_ADMIT_S_BIND_ROOT_G;
    else if (has_b && !fr_same(sc[0], bc[0])) cs = ZKFL_ADMIT_S_BIND_ROOT_D;
    else if (has_t && !fr_same(sc[2], tc[2])) cs = ZKFL_ADMIT_S_BIND_ROOT_W;
    else if (!fr_is_u64(sig[0], D.ids[i])) cs = ZKFL_ADMIT_S_SIG_CLIENT_ID;
    else if (!fr_same(sig[1], sc[4])) cs = ZKFL_ADMIT_S_SIG_ROUND;
    else if ((D.flags & ZKFL_ADMIT_CHECK_ROUND) && !fr_same(sc[4], srv_round)) cs = ZKFL_ADMIT_S_ROUND_STALE;
    else if (!fr_same(sig[2], sc[0])) cs = ZKFL_ADMIT_S_SIG_ROOT_D;
    else if (!fr_same(sig[3], sc[1])) cs = ZKFL_ADMIT_S_SIG_ROOT_G;
    else if (!fr_same(sig[4], sc[2])) cs = ZKFL_ADMIT_S_SIG_ROOT_W;
    else if (!fr_same(sig[5], sc[3])) cs = ZKFL_ADMIT_S_SIG_ROOT_K;
    else if (!fr_same(sig[6], tau)) cs = ZKFL_ADMIT_S_SIG_TAU;
    else {
      const Fr* m = D.masked + i * D.dim;
      bool same = true;
      for (uint32_t k = 0; k < D.dim; k++) same = same && fr_same(sig[ADMIT_S_NPUB0 + k], m[k]);
      if (!same) {
        cs = ZKFL_ADMIT_S_SIG_MASKED;
      } else if (D.flags & ZKFL_ADMIT_CHECK_PEERS) {
        const uint32_t slots = D.s_npub - ADMIT_S_NPUB0 - D.dim;
        const uint64_t p0 = D.peer_ptr[i], p1 = D.peer_ptr[i + 1];
        same = p1 - p0 == slots;
        for (uint32_t j = 0; same && j < slots; j++)
          same = fr_is_u64(sig[ADMIT_S_NPUB0 + D.dim + j], D.peer_ids[p0 + j]);
        if (!same) cs = ZKFL_ADMIT_S_SIG_PEERS;
      }
    }
  }
  D.codes[i] = cb;
  D.codes[D.n + i] = ct;
  D.codes[2 * D.n + i] = cs;
}

template <int T>
hipError_t launch_clients(const PosTables* P, const AdmitDev& D, hipStream_t st) {
  PosConsts K, K3;
  pos_tables_width(P, T, &K.C, &K.M, &K.rp);
  pos_tables_width(P, 3, &K3.C, &K3.M, &K3.rp);
  hipLaunchKernelGGL(k_admit_clients<T>, dim3(D.weights_pass ? 1 : zk_grid(D.n, 256)), dim3(256), 0, st, K, K3, D);
  return hipGetLastError();
}

#define ZK_ADMIT_WIDTHS(X) \
  X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16) X(17)

hipError_t clients_of_width(uint32_t t, const PosTables* P, const AdmitDev& D, hipStream_t st) {
  switch (t) {
#define ZK_CASE(T) \
  case T:          \
    return launch_clients<T>(P, D, st);
    ZK_ADMIT_WIDTHS(ZK_CASE)
#undef ZK_CASE
    default:
      return hipErrorInvalidValue;
  }
}

}  // namespace

hipError_t admit_signed_dev(const int64_t* grad, size_t count, Fr* out, hipStream_t st) {
  if (!count) return hipSuccess;
  hipLaunchKernelGGL(k_admit_signed, dim3(zk_grid(count, 256)), dim3(256), 0, st, grad, count, out);
  return hipGetLastError();
}

hipError_t admit_chunks_dev(const PosTables* P, const Fr* rows, size_t n_rows, uint32_t len, Fr* chunk,
                            hipStream_t st) {
  if (len <= VHASH_CHUNK || len > VHASH_CHUNK * VHASH_CHUNK) return hipErrorInvalidValue;
  if (!n_rows) return hipSuccess;
  const uint32_t nch = (len + VHASH_CHUNK - 1) / VHASH_CHUNK, full = len / VHASH_CHUNK, tail = len % VHASH_CHUNK;
  PosConsts K17;
  pos_tables_width(P, VHASH_CHUNK + 1, &K17.C, &K17.M, &K17.rp);
  hipLaunchKernelGGL(k_admit_chunks, dim3(zk_grid(n_rows * full, 256)), dim3(256), 0, st, K17, rows, n_rows, len, nch,
                     full, chunk);
  ZK_CHECK(hipGetLastError());
  if (tail)  // the short last chunk of every row: one launch of the width it has
    ZK_CHECK(poseidon_rows(P, tail, n_rows, rows + (size_t)full * VHASH_CHUNK, len, false, chunk + full, nch, true, st));
  return hipSuccess;
}

int admit_static_run(const PosTables* P, const AdmitJob& J, hipStream_t st, Profiler* prof, std::string& err) {
  const char* const where = "admit";
  const size_t n = J.n;
  const uint32_t dim = J.dim;
  const uint32_t nch = dim > VHASH_CHUNK ? (dim + VHASH_CHUNK - 1) / VHASH_CHUNK : 0;
  const bool peers = (J.flags & ZKFL_ADMIT_CHECK_PEERS) != 0, model = (J.flags & ZKFL_ADMIT_CHECK_MODEL) != 0;
  const size_t n_peer = peers ? (size_t)J.peer_ptr[n] : 0;

  DevBufs B;
  AdmitDev D = {};
  uint8_t *d_bp, *d_tp, *d_sp;
  Fr *d_bc, *d_tc, *d_sc, *d_bs, *d_ts, *d_ss, *d_masked, *d_server, *d_chunk, *d_gfr, *d_w;
  int64_t* d_grad;
  uint64_t *d_ids, *d_pptr, *d_pids;
  uint32_t* d_codes;
  HIP_TRY_ERR(B.get(&d_bp, n), where, err);
  HIP_TRY_ERR(B.get(&d_tp, n), where, err);
  HIP_TRY_ERR(B.get(&d_sp, n), where, err);
  HIP_TRY_ERR(B.get(&d_bc, n * ADMIT_B_FIELDS), where, err);
  HIP_TRY_ERR(B.get(&d_tc, n * ADMIT_T_FIELDS), where, err);
  HIP_TRY_ERR(B.get(&d_sc, n * ADMIT_S_FIELDS), where, err);
  HIP_TRY_ERR(B.get(&d_bs, n * ADMIT_B_NPUB), where, err);
  HIP_TRY_ERR(B.get(&d_ts, n * ADMIT_T_NPUB), where, err);
  HIP_TRY_ERR(B.get(&d_ss, n * J.s_npub), where, err);
  HIP_TRY_ERR(B.get(&d_masked, n * dim), where, err);
  HIP_TRY_ERR(B.get(&d_grad, n * dim), where, err);
  HIP_TRY_ERR(B.get(&d_ids, n), where, err);
  HIP_TRY_ERR(B.get(&d_server, 3), where, err);
  // dim > 16: the gradients as field elements, then the weights as row n; their chunk hashes likewise
  const size_t n_rows = n + (model ? 1 : 0);
  HIP_TRY_ERR(B.get(&d_chunk, n_rows * nch), where, err);
  HIP_TRY_ERR(B.get(&d_gfr, nch ? n_rows * dim : 0), where, err);
  HIP_TRY_ERR(B.get(&d_w, model && !nch ? dim : 0), where, err);
  HIP_TRY_ERR(B.get(&d_pptr, n + 1), where, err);
  HIP_TRY_ERR(B.get(&d_pids, n_peer), where, err);
  HIP_TRY_ERR(B.get(&d_codes, 3 * n), where, err);

  // a phase nobody sent may come without its arrays: those stay unread (every lane sees present = 0)
  auto up = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return (src && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipSuccess;
  };
  HIP_TRY_ERR(up(d_bp, J.b_present, n), where, err);
  HIP_TRY_ERR(up(d_tp, J.t_present, n), where, err);
  HIP_TRY_ERR(up(d_sp, J.s_present, n), where, err);
  HIP_TRY_ERR(up(d_bc, J.b_claimed, n * ADMIT_B_FIELDS * 32), where, err);
  HIP_TRY_ERR(up(d_tc, J.t_claimed, n * ADMIT_T_FIELDS * 32), where, err);
  HIP_TRY_ERR(up(d_sc, J.s_claimed, n * ADMIT_S_FIELDS * 32), where, err);
  HIP_TRY_ERR(up(d_bs, J.b_signals, n * ADMIT_B_NPUB * 32), where, err);
  HIP_TRY_ERR(up(d_ts, J.t_signals, n * ADMIT_T_NPUB * 32), where, err);
  HIP_TRY_ERR(up(d_ss, J.s_signals, n * J.s_npub * 32), where, err);
  HIP_TRY_ERR(up(d_masked, J.masked, n * dim * 32), where, err);
  HIP_TRY_ERR(up(d_grad, J.gradients, n * dim * 8), where, err);
  HIP_TRY_ERR(up(d_ids, J.ids, n * 8), where, err);
  HIP_TRY_ERR(up(d_server, J.round, 32), where, err);
  HIP_TRY_ERR(up(d_server + 1, J.tau, 32), where, err);
  if (peers) {
    HIP_TRY_ERR(up(d_pptr, J.peer_ptr, (n + 1) * 8), where, err);
    HIP_TRY_ERR(up(d_pids, J.peer_ids, n_peer * 8), where, err);
  }
  if (model) HIP_TRY_ERR(up(nch ? d_gfr + n * dim : d_w, J.weights, (size_t)dim * 32), where, err);

  if (nch) {
    const int pc = prof ? prof->begin("admit_chunks", st) : -1;
    HIP_TRY_ERR(admit_signed_dev(d_grad, n * dim, d_gfr, st), where, err);
    HIP_TRY_ERR(admit_chunks_dev(P, d_gfr, n_rows, dim, d_chunk, st), where, err);
    if (prof) prof->end(pc, st, (double)n_rows * nch);  // units: chunk hashes
  }
  D.n = n;
  D.dim = dim;
  D.nch = nch;
  D.s_npub = J.s_npub;
  D.flags = J.flags;
  D.ids = d_ids;
  D.server = d_server;
  D.b_present = d_bp;
  D.t_present = d_tp;
  D.s_present = d_sp;
  D.b_claimed = d_bc;
  D.t_claimed = d_tc;
  D.s_claimed = d_sc;
  D.b_sig = d_bs;
  D.t_sig = d_ts;
  D.s_sig = d_ss;
  D.grad = d_grad;
  D.masked = d_masked;
  D.chunk = d_chunk;
  D.weights = d_w;
  D.wc_out = d_server + 2;
  D.peer_ptr = d_pptr;
  D.peer_ids = d_pids;
  D.codes = d_codes;
  const int pk = prof ? prof->begin("admit_clients", st) : -1;
  if (model) {  // weightCommitment(weights), once per call: one lane of the same kernel
    D.weights_pass = 1;
    HIP_TRY_ERR(clients_of_width((nch ? nch : dim) + 1, P, D, st), where, err);
    D.weights_pass = 0;
  }
  HIP_TRY_ERR(clients_of_width((nch ? nch : dim) + 1, P, D, st), where, err);
  if (prof) prof->end(pk, st, (double)n);  // units: clients
  HIP_TRY_ERR(hipMemcpyAsync(J.codes, d_codes, 3 * n * sizeof(uint32_t), hipMemcpyDeviceToHost, st), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  return ZKFL_OK;
}

}  // namespace zkfl

namespace {

int bad(int code, const char* who, const std::string& msg) { return fail(code, std::string(who) + ": " + msg); }

// rows x per values of 32 B; only the rows of present clients are looked at
int rows_lt_r(const char* who, const char* what, const uint8_t* v, const uint8_t* present, size_t n, size_t per) {
  for (size_t i = 0; i < n; i++) {
    if (!present[i]) continue;
    for (size_t k = 0; k < per; k++) {
      uint32_t w[8];
      memcpy(w, v + 32 * (i * per + k), 32);
      if (!fr_lt_r(w))
        return bad(ZKFL_E_ARG, who, "client " + std::to_string(i) + ": " + what + " " + std::to_string(k) + " is not < r");
    }
  }
  return ZKFL_OK;
}

// The argument checks of both entry points; fills J (but for codes).  all_present backs a NULL
// present array.
int admit_args(const char* who, const zkfl_ctx* ctx, const zkfl_admit_round* in, uint32_t flags, uint32_t s_npub,
               bool proofs, const uint32_t* codes, std::vector<uint8_t>& all_present, AdmitJob& J) {
  if (!ctx || !in) return bad(ZKFL_E_ARG, who, "null argument");
  const size_t n = in->n;
  if (flags & ~(ZKFL_ADMIT_CHECK_ROUND | ZKFL_ADMIT_CHECK_MODEL | ZKFL_ADMIT_CHECK_PEERS | ZKFL_ADMIT_COMBINED))
    return bad(ZKFL_E_ARG, who, "unknown flag in " + std::to_string(flags));
  if (in->dim == 0 || in->dim > ZKFL_ADMIT_MAX_DIM)
    return bad(ZKFL_E_ARG, who, "dim " + std::to_string(in->dim) + " must be in 1.." + std::to_string(ZKFL_ADMIT_MAX_DIM));
  if (n >= (1ull << 32)) return bad(ZKFL_E_ARG, who, "n must be < 2^32");
  if (s_npub < ADMIT_S_NPUB0 + in->dim)
    return bad(ZKFL_E_MISMATCH, who, "key 2 (secagg) has " + std::to_string(s_npub) + " public signals, dim " +
                                         std::to_string(in->dim) + " needs at least " +
                                         std::to_string(ADMIT_S_NPUB0 + in->dim));
  if (!in->round || !in->tau_squared || (n && (!in->ids || !codes))) return bad(ZKFL_E_ARG, who, "null argument");
  if ((flags & ZKFL_ADMIT_CHECK_MODEL) && !in->weights)
    return bad(ZKFL_E_ARG, who, "ZKFL_ADMIT_CHECK_MODEL (flag 2) needs weights");
  if ((flags & ZKFL_ADMIT_CHECK_PEERS) && (!in->peer_ptr || (in->peer_ptr[n] && !in->peer_ids)))
    return bad(ZKFL_E_ARG, who, "ZKFL_ADMIT_CHECK_PEERS (flag 4) needs peer_ptr and peer_ids");
  if (flags & ZKFL_ADMIT_CHECK_PEERS) {
    if (in->peer_ptr[0] != 0) return bad(ZKFL_E_ARG, who, "peer_ptr[0] must be 0");
    for (size_t i = 0; i < n; i++)
      if (in->peer_ptr[i + 1] < in->peer_ptr[i])
        return bad(ZKFL_E_ARG, who, "peer_ptr[" + std::to_string(i + 1) + "] is below peer_ptr[" + std::to_string(i) + "]");
  }
  all_present.assign(n, 1);
  const zkfl_admit_phase* ph[3] = {&in->balance, &in->training, &in->secagg};
  const char* const names[3] = {"balance", "training", "secagg"};
  const size_t fields[3] = {ADMIT_B_FIELDS, ADMIT_T_FIELDS, ADMIT_S_FIELDS};
  const size_t npub[3] = {ADMIT_B_NPUB, ADMIT_T_NPUB, s_npub};
  const uint8_t* present[3];
  for (int p = 0; p < 3; p++) {
    present[p] = ph[p]->present ? ph[p]->present : all_present.data();
    bool any = false;
    for (size_t i = 0; i < n; i++) any |= present[p][i] != 0;
    if (any && (!ph[p]->claimed || !ph[p]->signals || (proofs && !ph[p]->proofs)))
      return bad(ZKFL_E_ARG, who, std::string(names[p]) + ": null array with a package present");
    if (any && p == 1 && !in->gradients) return bad(ZKFL_E_ARG, who, "training: null gradients with a package present");
    if (any && p == 2 && !in->masked_update)
      return bad(ZKFL_E_ARG, who, "secagg: null masked_update with a package present");
  }
  uint32_t w[8];
  memcpy(w, in->round, 32);
  if (!fr_lt_r(w)) return bad(ZKFL_E_ARG, who, "round is not < r");
  memcpy(w, in->tau_squared, 32);
  if (!fr_lt_r(w)) return bad(ZKFL_E_ARG, who, "tau_squared is not < r");
  if (flags & ZKFL_ADMIT_CHECK_MODEL)
    for (uint32_t k = 0; k < in->dim; k++) {
      memcpy(w, in->weights + 32 * k, 32);
      if (!fr_lt_r(w)) return bad(ZKFL_E_ARG, who, "weight " + std::to_string(k) + " is not < r");
    }
  for (int p = 0; p < 3; p++) {
    int rc = rows_lt_r(who, (std::string(names[p]) + " claimed field").c_str(), ph[p]->claimed, present[p], n, fields[p]);
    if (rc) return rc;
    if ((rc = rows_lt_r(who, (std::string(names[p]) + " signal").c_str(), ph[p]->signals, present[p], n, npub[p])))
      return rc;
  }
  if (int rc = rows_lt_r(who, "masked_update value", in->masked_update, present[2], n, in->dim)) return rc;

  J.n = n;
  J.dim = in->dim;
  J.flags = flags;
  J.s_npub = s_npub;
  J.ids = in->ids;
  J.round = in->round;
  J.tau = in->tau_squared;
  J.b_present = present[0];
  J.t_present = present[1];
  J.s_present = present[2];
  J.b_claimed = in->balance.claimed;
  J.t_claimed = in->training.claimed;
  J.s_claimed = in->secagg.claimed;
  J.b_signals = in->balance.signals;
  J.t_signals = in->training.signals;
  J.s_signals = in->secagg.signals;
  J.gradients = in->gradients;
  J.masked = in->masked_update;
  J.weights = in->weights;
  J.peer_ptr = in->peer_ptr;
  J.peer_ids = in->peer_ids;
  return ZKFL_OK;
}

int run_static(zkfl_ctx* ctx, const AdmitJob& J) {
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = pos_ready(ctx);
  if (rc) return rc;
  std::string err;
  rc = admit_static_run(ctx->pos, J, ctx->st, &ctx->prof, err);
  return rc ? fail(rc, err) : ZKFL_OK;
}

}  // namespace

extern "C" int zkfl_debug_admit_static(zkfl_ctx* ctx, const zkfl_admit_round* in, uint32_t flags,
                                       uint32_t secagg_npublic, uint32_t* codes) {
  const char* const who = "debug_admit_static";
  std::vector<uint8_t> ones;
  AdmitJob J;
  int rc = admit_args(who, ctx, in, flags, secagg_npublic, false, codes, ones, J);
  if (rc || !in->n) return rc;
  std::vector<uint32_t> st(3 * in->n);
  J.codes = st.data();
  if ((rc = run_static(ctx, J))) return rc;
  memcpy(codes, st.data(), st.size() * sizeof(uint32_t));
  return ZKFL_OK;
}

extern "C" int zkfl_round_admit(zkfl_ctx* ctx, const zkfl_admit_round* in, uint32_t flags, uint32_t* codes,
                                zkfl_round_report* report) {
  const char* const who = "round_admit";
  if (!ctx || !in) return bad(ZKFL_E_ARG, who, "null argument");
  const uint32_t want[3] = {ADMIT_B_NPUB, ADMIT_T_NPUB, 0};
  uint32_t s_npub = 0;
  for (int p = 0; p < 3; p++) {
    const zkfl_vkey* k = in->vkeys[p];
    if (!k || k->ctx != ctx) return bad(ZKFL_E_ARG, who, "key " + std::to_string(p) + " is not a key of this context");
    const uint32_t np = vk_npub(k->vk);
    if (p == 2) s_npub = np;  // checked against dim below
    else if (np != want[p])
      return bad(ZKFL_E_MISMATCH, who, "key " + std::to_string(p) + " has " + std::to_string(np) +
                                           " public signals, its phase has " + std::to_string(want[p]));
  }
  std::vector<uint8_t> ones;
  AdmitJob J;
  int rc = admit_args(who, ctx, in, flags, s_npub, true, codes, ones, J);
  if (rc) return rc;
  const size_t n = in->n;
  zkfl_round_report rep = {0, 0, 0, 0, 0};
  if (!n) {
    if (report) *report = rep;
    return ZKFL_OK;
  }
  std::vector<uint32_t> st(3 * n);
  J.codes = st.data();
  if ((rc = run_static(ctx, J))) return rc;

  // the present packages whose static code is 0, phase after phase
  const zkfl_admit_phase* ph[3] = {&in->balance, &in->training, &in->secagg};
  const size_t npub[3] = {ADMIT_B_NPUB, ADMIT_T_NPUB, s_npub};
  std::vector<size_t> job_of;
  std::vector<const zkfl_vkey*> keys;
  std::vector<const uint8_t*> pubs;
  std::vector<size_t> npubs;
  std::vector<uint8_t> proofs;
  for (size_t p = 0; p < 3; p++)
    for (size_t i = 0; i < n; i++) {
      if (st[p * n + i] != ZKFL_ADMIT_OK) continue;
      job_of.push_back(p * n + i);
      keys.push_back(in->vkeys[p]);
      pubs.push_back(ph[p]->signals + 32 * npub[p] * i);
      npubs.push_back(npub[p]);
      proofs.insert(proofs.end(), ph[p]->proofs + 256 * i, ph[p]->proofs + 256 * (i + 1));
    }
  const size_t m = job_of.size();
  std::vector<int32_t> ok(m, 0);
  if (m) {
    if (flags & ZKFL_ADMIT_COMBINED)
      rc = zkfl_groth16_verify_round(ctx, m, keys.data(), pubs.data(), npubs.data(), proofs.data(), nullptr, ok.data(),
                                     &rep);
    else
      rc = zkfl_groth16_verify_multi(ctx, m, keys.data(), pubs.data(), npubs.data(), proofs.data(), ok.data(),
                                     ZKFL_VERIFY_AUTO);
    if (rc) return rc;
  }
  if (!(flags & ZKFL_ADMIT_COMBINED)) rep.combined = (uint32_t)m;
  const uint32_t proof_code[3] = {ZKFL_ADMIT_B_PROOF, ZKFL_ADMIT_T_PROOF, ZKFL_ADMIT_S_PROOF};
  for (size_t j = 0; j < m; j++)
    if (!ok[j]) st[job_of[j]] = proof_code[job_of[j] / n];
  // the reference's chain: no training proof without an accepted balance proof, no secagg proof
  // without an accepted training proof
  for (size_t i = 0; i < n; i++) {
    if (st[n + i] != ZKFL_ADMIT_T_MISSING && st[i] != ZKFL_ADMIT_OK) st[n + i] = ZKFL_ADMIT_T_NO_BALANCE;
    if (st[2 * n + i] != ZKFL_ADMIT_S_MISSING && st[n + i] != ZKFL_ADMIT_OK) st[2 * n + i] = ZKFL_ADMIT_S_NO_TRAINING;
  }
  memcpy(codes, st.data(), st.size() * sizeof(uint32_t));
  if (report) *report = rep;
  return ZKFL_OK;
}
