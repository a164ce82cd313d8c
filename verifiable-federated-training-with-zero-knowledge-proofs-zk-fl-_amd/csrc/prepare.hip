// Preparing a round on the GPU: every client's dataset tree, Merkle openings, fixed-point gradient,
// commitments and masked update, written straight into the three circuits' input vectors.
//
// Reference behaviour: the client half of the round loop of tests/full_system_simulation.mjs
// (:1278-1343).  computeDatasetCommitment (:308-335): leaf i = vectorHash(features[i] || label[i]),
// buildMerkleTree over the leaves padded with Poseidon([0]); getMerkleProof (:225-238): the sibling
// of every level and pathIndices[l] = (idx >> l) & 1; _computeVerifiedGradient (:511-553):
// summed[j] = sum_i (<f_i, w> - label_i * PRECISION) * f_ij over the batch rows, gradient =
// Math.floor(summed / (BATCH * PRECISION)), remainder = summed - gradient * (BATCH * PRECISION);
// gradPos / gradNeg and the clipping test (:411-431, the reference throws above tauSquared);
// root_W = vectorHash(weights), root_G = gradientCommitment(gradient, id, round) (:433-438, :139-170),
// root_K = Poseidon(master, keys...) and the masked update (:565-609).  Same values as
// zkfl/clients.py, which stays the model.
//
// Layout (MI355X): one upload of everything, then launches whose number depends on the shape only:
//   rows     lane = (client, sample, k): the leaf's dim + 1 values as standard-form field elements;
//            the input vectors take their features and labels from this buffer, too
//   leaves   lane = (client, sample): one Poseidon of width dim + 2 for dim + 1 <= 16 (poseidon_rows,
//            csrc/merkle.h); else admit's chunk pass (all full chunks of all leaves in one launch,
//            the short last chunk in one more) and the top hash over the chunk hashes
//   levels   one launch per tree level, lane = (client, live node) of all clients together; only
//            nodes above real leaves are hashed, every other node of level l is z_l (PosTables.zeros)
//   open     lane = (client, row, level): the sibling (live node or z_l) and the path bit, standard
//            form, straight to their offsets in the input vectors (all samples for balance, the batch
//            rows for training)
//   gradient lane = (client, j): int64 arithmetic (the host refuses what could overflow), explicit
//            floor for negative sums
//   commit   the gradients through admit's signed map with the weights as one more row, their vector
//            hash (admit's chunk pass above 16), then lane = client: the saturating norm and status,
//            c1, Poseidon(id, round) and root_G; root_K is one Poseidon of width peers + 2
//   masks    secagg's term and fold kernels on the device buffers (secagg_eval_dev)
//   inputs   lane = (client, k) over the part of each input vector that is not an opening
// Node storage is level-major: level l holds n x live[l] Montgomery nodes, client after client, so a
// level's launch reads and writes contiguous memory.  No atomics: a lane owns what it writes.
#include <hip/hip_runtime.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "admit.h"
#include "common.h"
#include "devbufs.h"
#include "host_parse.h"
#include "merkle.h"
#include "objects.h"
#include "poseidon.h"
#include "prepare.h"
#include "secagg.h"
#include "zkfl.h"

namespace zkfl {

namespace {

constexpr uint32_t PREP_LEVELS = ZKFL_MERKLE_MAX_DEPTH + 1;

// per client: the live node count of every level and the level's offset in a client-compact tree
struct PrepMap {
  uint32_t live[PREP_LEVELS];
  uint32_t off[PREP_LEVELS];
};

struct PrepDev {
  size_t n;
  uint32_t samples, dim, depth, batch, precision, peers, leaf_len;
  uint64_t tau;
  size_t nb, nt, ns;  // the input vectors' lengths
  const uint64_t* ids;
  const int64_t* features;  // [n x samples x dim]
  const int64_t* weights;   // [dim]
  const uint8_t* labels;    // [n x samples]
  const uint32_t* idx;      // [n x batch]
  const uint64_t* peer_ids; // [n x peers]
  const Fr* round;          // std
  const Fr* krows;          // [n x (peers + 1)] std: master key, then the keys
  const Fr* rows;           // [n x samples x leaf_len] std
  const Fr* nodes;          // level-major Montgomery nodes, or null without a tree
  size_t root_off;          // the roots' level: nodes[root_off + client]
  int64_t *summed, *grad, *rem;  // [n x dim]
  const Fr* gfr;            // [(n + 1) x dim] std: the gradients, then the weights
  const Fr* vh;             // [n + 1] Montgomery: their vector hashes
  Fr* roots;                // [n x 4] std: D, G, W, K
  const Fr* masked;         // [n x dim] std
  uint32_t *c1, *status;    // [n]
  Fr *bal, *trn, *sec;      // the input vectors (null: not asked for)
};

ZK_DEV Fr fr_std_u64(uint64_t x) {
  Fr v = fp_zero<FrP>();
  v.v[0] = (uint32_t)x;
  v.v[1] = (uint32_t)(x >> 32);
  return v;
}

// lane = (client, sample, k): rows[(client, sample)][k] = features[k] for k < dim, the label at k = dim
__global__ __launch_bounds__(256) void k_prepare_rows(const int64_t* __restrict__ features,
                                                      const uint8_t* __restrict__ labels, size_t n_rows, uint32_t dim,
                                                      Fr* __restrict__ rows) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t len = dim + 1;
  if (i >= n_rows * len) return;
  const size_t row = i / len;
  const uint32_t k = (uint32_t)(i - row * len);
  rows[i] = k < dim ? fr_from_i64(features[row * dim + k]) : fr_std_u64(labels[row]);
}

// lane = (client, parent j): up[client][j] = Poseidon(lvl[client][2j], lvl[client][2j + 1] or z_l)
__global__ __launch_bounds__(256) void k_prepare_level(PosConsts K, const Fr* __restrict__ lvl, uint32_t live,
                                                       const Fr* __restrict__ zero_l, Fr* __restrict__ up,
                                                       uint32_t up_live, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * up_live) return;
  const size_t c = i / up_live;
  const uint32_t j = (uint32_t)(i - c * up_live);
  const Fr* mine = lvl + c * live;
  Fr st[3];
  st[0] = fp_zero<FrP>();
  st[1] = mine[2 * j];
  st[2] = (2 * j + 1 < live) ? mine[2 * j + 1] : *zero_l;
  up[i] = poseidon_perm0<3>(st, K);
}

// lane = (client, row, level): the opening of leaf idx[client][row] (or of leaf `row`), into the
// client's input vector at sib_off / path_off + row * depth + level
__global__ __launch_bounds__(256) void k_prepare_open(PrepMap map, const Fr* __restrict__ nodes,
                                                      const Fr* __restrict__ zeros, size_t n, uint32_t rows_per,
                                                      uint32_t depth, const uint32_t* __restrict__ idx,
                                                      Fr* __restrict__ out, size_t stride, size_t sib_off,
                                                      size_t path_off) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t per = (size_t)rows_per * depth;
  if (i >= n * per) return;
  const size_t c = i / per;
  const uint32_t q = (uint32_t)(i - c * per);
  const uint32_t row = q / depth, l = q - row * depth;
  const uint32_t leaf = idx ? idx[c * rows_per + row] : row;
  const uint32_t at = leaf >> l, sib = at ^ 1u;
  const uint32_t live = map.live[l];
  const Fr v = sib < live ? nodes[n * map.off[l] + c * live + sib] : zeros[l];
  Fr* vec = out + c * stride;
  vec[sib_off + q] = fp_from_mont(v);
  vec[path_off + q] = fr_std_u64(at & 1u);
}

// lane = (client, j): summed, gradient = floor(summed / div), remainder in [0, div)
__global__ __launch_bounds__(256) void k_prepare_gradient(PrepDev D) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n * D.dim) return;
  const size_t c = i / D.dim;
  const uint32_t j = (uint32_t)(i - c * D.dim);
  const int64_t div = (int64_t)D.batch * (int64_t)D.precision;
  int64_t s = 0;
  for (uint32_t b = 0; b < D.batch; b++) {
    const size_t row = c * D.samples + D.idx[c * D.batch + b];
    const int64_t* f = D.features + row * D.dim;
    int64_t pred = 0;
    for (uint32_t k = 0; k < D.dim; k++) pred += f[k] * D.weights[k];
    const int64_t e = pred - (int64_t)D.labels[row] * (int64_t)D.precision;
    s += e * f[j];
  }
  int64_t q = s / div, r = s % div;  // C++ truncates: the floor of a negative sum is one lower
  if (r < 0) {
    q -= 1;
    r += div;
  }
  D.summed[i] = s;
  D.grad[i] = q;
  D.rem[i] = r;
}

// lane = client: norm and status, c1, root_D, root_G, root_W (root_K: the launch that follows)
__global__ __launch_bounds__(256) void k_prepare_clients(PosConsts K3, PrepDev D) {
  const size_t c = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= D.n) return;
  // sum g^2 against tau, saturating: a square or a sum above 2^64 - 1 is over any tau
  uint64_t norm = 0;
  bool over = false;
  for (uint32_t j = 0; j < D.dim; j++) {
    const int64_t g = D.grad[c * D.dim + j];
    const uint64_t a = g < 0 ? 0ull - (uint64_t)g : (uint64_t)g;
    over |= __umul64hi(a, a) != 0;
    const uint64_t sq = a * a, sum = norm + sq;
    over |= sum < norm;
    norm = sum;
  }
  D.status[c] = (over || norm > D.tau) ? ZKFL_PREPARE_NORM : ZKFL_PREPARE_OK;
  uint32_t ones = 0;
  for (uint32_t s = 0; s < D.samples; s++) ones += D.labels[c * D.samples + s];
  D.c1[c] = ones;

  Fr s3[3] = {fp_zero<FrP>(), fp_to_mont(fr_std_u64(D.ids[c])), fp_to_mont(*D.round)};
  const Fr meta = poseidon_perm0<3>(s3, K3);
  s3[0] = fp_zero<FrP>();
  s3[1] = D.vh[c];
  s3[2] = meta;
  Fr* roots = D.roots + 4 * c;
  roots[0] = D.nodes ? fp_from_mont(D.nodes[D.root_off + c]) : fp_zero<FrP>();
  roots[1] = fp_from_mont(poseidon_perm0<3>(s3, K3));
  roots[2] = fp_from_mont(D.vh[D.n]);
  if (!D.peers) roots[3] = fp_zero<FrP>();
}

// lane = (client, k): entry k of the phase's input vector, k below the openings
template <int PHASE>
__global__ __launch_bounds__(256) void k_prepare_inputs(PrepDev D, size_t head) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.n * head) return;
  const size_t c = i / head;
  size_t k = i - c * head;
  const uint32_t dim = D.dim, len = D.leaf_len;
  const Fr* roots = D.roots + 4 * c;
  Fr v;
  if (PHASE == 0) {  // client_id, root, N_public, c0, c1, features, labels
    if (k < 5) {
      v = k == 0 ? fr_std_u64(D.ids[c]) : k == 1 ? roots[0] : k == 2 ? fr_std_u64(D.samples)
          : k == 3 ? fr_std_u64(D.samples - D.c1[c]) : fr_std_u64(D.c1[c]);
    } else if ((k -= 5) < (size_t)D.samples * dim) {
      v = D.rows[(c * D.samples + k / dim) * len + k % dim];
    } else {
      k -= (size_t)D.samples * dim;
      v = D.rows[(c * D.samples + k) * len + dim];
    }
    D.bal[c * D.nb + (i - c * head)] = v;
  } else if (PHASE == 1) {  // client_id, round, root_D, root_G, root_W, tauSquared, weights,
                            // expectedSummedGrad, remainder, gradPos, gradNeg, features, labels
    if (k < 6) {
      v = k == 0 ? fr_std_u64(D.ids[c]) : k == 1 ? *D.round : k == 5 ? fr_std_u64(D.tau) : roots[k - 2];
    } else if ((k -= 6) < 5 * (size_t)dim) {
      const uint32_t what = (uint32_t)(k / dim), j = (uint32_t)(k % dim);
      const int64_t g = D.grad[c * dim + j];
      v = what == 0   ? D.gfr[D.n * dim + j]
          : what == 1 ? fr_from_i64(D.summed[c * dim + j])
          : what == 2 ? fr_std_u64((uint64_t)D.rem[c * dim + j])
          : what == 3 ? fr_std_u64(g > 0 ? (uint64_t)g : 0)
                      : fr_std_u64(g < 0 ? 0ull - (uint64_t)g : 0);
    } else if ((k -= 5 * (size_t)dim) < (size_t)D.batch * dim) {
      const size_t row = c * D.samples + D.idx[c * D.batch + k / dim];
      v = D.rows[row * len + k % dim];
    } else {
      k -= (size_t)D.batch * dim;
      const size_t row = c * D.samples + D.idx[c * D.batch + k];
      v = D.rows[row * len + dim];
    }
    D.trn[c * D.nt + (i - c * head)] = v;
  } else {  // client_id, round, root_D, root_G, root_W, root_K, tauSquared, masked_update, peer_ids,
            // gradient, master_key, shared_keys
    const uint32_t p = D.peers;
    if (k < 7) {
      v = k == 0 ? fr_std_u64(D.ids[c]) : k == 1 ? *D.round : k == 6 ? fr_std_u64(D.tau) : roots[k - 2];
    } else if ((k -= 7) < dim) {
      v = D.masked[c * dim + k];
    } else if ((k -= dim) < p) {
      v = fr_std_u64(D.peer_ids[c * p + k]);
    } else if ((k -= p) < dim) {
      v = D.gfr[c * dim + k];
    } else {
      k -= dim;  // the master key, then the keys: the client's row of krows
      v = D.krows[c * (p + 1) + k];
    }
    D.sec[c * D.ns + (i - c * head)] = v;
  }
}

// vectorHash of n_rows rows of len values (std) -> out[i * out_stride]; chunk: scratch of n_rows x
// ceil(len / 16) above 16 values
hipError_t vhash_dev(const PosTables* P, const Fr* rows, size_t n_rows, uint32_t len, Fr* chunk, Fr* out,
                     size_t out_stride, bool out_mont, hipStream_t st) {
  if (len <= VHASH_CHUNK) return poseidon_rows(P, len, n_rows, rows, len, false, out, out_stride, out_mont, st);
  const uint32_t nch = (len + VHASH_CHUNK - 1) / VHASH_CHUNK;
  ZK_CHECK(admit_chunks_dev(P, rows, n_rows, len, chunk, st));
  return poseidon_rows(P, nch, n_rows, chunk, nch, true, out, out_stride, out_mont, st);
}

// a host staging buffer cut into aligned sections, uploaded in one copy
struct Stage {
  std::vector<uint8_t> host;
  size_t add(size_t bytes) {
    const size_t at = (host.size() + 31) & ~(size_t)31;
    host.resize(at + bytes);
    return at;
  }
};

}  // namespace

int prepare_run(const PosTables* P, const zkfl_prepare_round& in, const zkfl_prepare_out& out, hipStream_t st,
                Profiler* prof, std::string& err) {
  const char* const where = "prepare";
  const size_t n = in.n;
  const uint32_t S = in.samples, dim = in.dim, depth = in.depth, batch = in.batch, peers = in.peers;
  const uint32_t len = dim + 1;
  const size_t T = n * peers;
  const size_t nb = prepare_balance_len(S, dim, depth), nt = prepare_training_len(batch, dim, depth),
               ns = prepare_secagg_len(dim, peers);
  const bool tree = out.balance_inputs || out.training_inputs || out.secagg_inputs || out.roots;
  const bool want_sec = peers && out.secagg_inputs;

  PrepMap map = {};
  uint32_t per_client = 0;
  for (uint32_t l = 0, live = S; l <= depth; l++, live = (live + 1) / 2) {
    map.live[l] = live;
    map.off[l] = per_client;
    per_client += live;
  }

  // the secagg terms: client i's peers are terms [i * peers, (i + 1) * peers)
  const uint32_t ct = secagg_default_chunk(T, dim);
  std::vector<uint64_t> term_ptr(n + 1), chunk_ptr;
  std::vector<uint32_t> chunk_row;
  for (size_t i = 0; i <= n; i++) term_ptr[i] = i * peers;
  secagg_chunk_layout(term_ptr.data(), n, ct, chunk_ptr, chunk_row);
  const size_t n_chunks = chunk_row.size();

  // ---- one upload ----
  Stage G;
  const size_t o_raw = G.add((T + 1) * 32), o_krows = G.add(n * (peers + 1) * 32),
               o_feat = G.add(n * S * dim * 8), o_w = G.add((size_t)dim * 8), o_ids = G.add(n * 8),
               o_peer = G.add(T * 8), o_own = G.add(T * 8), o_tptr = G.add((n + 1) * 8),
               o_cptr = G.add((n + 1) * 8), o_idx = G.add(n * batch * 4), o_crow = G.add(n_chunks * 4),
               o_lab = G.add(n * S);
  uint8_t* h = G.host.data();
  if (T) memcpy(h + o_raw, in.keys, T * 32);
  memcpy(h + o_raw + T * 32, in.round, 32);
  if (peers)
    for (size_t i = 0; i < n; i++) {
      uint8_t* row = h + o_krows + i * (peers + 1) * 32;
      memcpy(row, in.master_keys + 32 * i, 32);
      memcpy(row + 32, in.keys + 32 * i * peers, (size_t)peers * 32);
    }
  memcpy(h + o_feat, in.features, n * S * dim * 8);
  memcpy(h + o_w, in.weights, (size_t)dim * 8);
  memcpy(h + o_ids, in.ids, n * 8);
  if (T) {
    memcpy(h + o_peer, in.peer_ids, T * 8);
    uint64_t* own = (uint64_t*)(h + o_own);
    for (size_t i = 0; i < n; i++)
      for (uint32_t j = 0; j < peers; j++) own[i * peers + j] = in.ids[i];
  }
  memcpy(h + o_tptr, term_ptr.data(), (n + 1) * 8);
  memcpy(h + o_cptr, chunk_ptr.data(), (n + 1) * 8);
  uint32_t* hidx = (uint32_t*)(h + o_idx);
  if (in.batch_idx) {
    memcpy(hidx, in.batch_idx, n * batch * 4);
  } else {
    for (size_t i = 0; i < n; i++)
      for (uint32_t b = 0; b < batch; b++) hidx[i * batch + b] = b;
  }
  if (n_chunks) memcpy(h + o_crow, chunk_row.data(), n_chunks * 4);
  memcpy(h + o_lab, in.labels, n * S);

  DevBufs B;
  uint8_t* d_in;
  HIP_TRY_ERR(B.get(&d_in, G.host.size()), where, err);
  HIP_TRY_ERR(hipMemcpyAsync(d_in, h, G.host.size(), hipMemcpyHostToDevice, st), where, err);

  const uint32_t nch_leaf = len > VHASH_CHUNK ? (len + VHASH_CHUNK - 1) / VHASH_CHUNK : 0;
  const uint32_t nch_g = dim > VHASH_CHUNK ? (dim + VHASH_CHUNK - 1) / VHASH_CHUNK : 0;
  Fr *d_rows, *d_nodes = nullptr, *d_lchunk, *d_gfr, *d_gchunk, *d_vh, *d_roots, *d_masked = nullptr;
  Fr *d_bal = nullptr, *d_trn = nullptr, *d_sec = nullptr;
  Fr *d_key = nullptr, *d_lo = nullptr, *d_hi = nullptr, *d_part = nullptr;
  uint8_t* d_neg = nullptr;
  int64_t* d_g64;
  uint32_t* d_u32;
  HIP_TRY_ERR(B.get(&d_rows, n * S * len), where, err);
  HIP_TRY_ERR(B.get(&d_lchunk, tree ? n * S * nch_leaf : 0), where, err);
  if (tree) HIP_TRY_ERR(B.get(&d_nodes, n * per_client), where, err);
  HIP_TRY_ERR(B.get(&d_g64, 3 * n * dim), where, err);
  HIP_TRY_ERR(B.get(&d_gfr, (n + 1) * dim), where, err);
  HIP_TRY_ERR(B.get(&d_gchunk, (n + 1) * nch_g), where, err);
  HIP_TRY_ERR(B.get(&d_vh, n + 1), where, err);
  HIP_TRY_ERR(B.get(&d_roots, 4 * n), where, err);
  HIP_TRY_ERR(B.get(&d_u32, 2 * n), where, err);
  if (peers) {
    HIP_TRY_ERR(B.get(&d_masked, n * dim), where, err);
    HIP_TRY_ERR(B.get(&d_key, T + 1), where, err);
    HIP_TRY_ERR(B.get(&d_lo, T), where, err);
    HIP_TRY_ERR(B.get(&d_hi, T), where, err);
    HIP_TRY_ERR(B.get(&d_neg, T), where, err);
    HIP_TRY_ERR(B.get(&d_part, n_chunks * dim), where, err);
  }
  if (out.balance_inputs) HIP_TRY_ERR(B.get(&d_bal, n * nb), where, err);
  if (out.training_inputs) HIP_TRY_ERR(B.get(&d_trn, n * nt), where, err);
  if (want_sec) HIP_TRY_ERR(B.get(&d_sec, n * ns), where, err);

  PrepDev D = {};
  D.n = n;
  D.samples = S;
  D.dim = dim;
  D.depth = depth;
  D.batch = batch;
  D.precision = in.precision;
  D.peers = peers;
  D.leaf_len = len;
  D.tau = in.tau_squared;
  D.nb = nb;
  D.nt = nt;
  D.ns = ns;
  D.ids = (const uint64_t*)(d_in + o_ids);
  D.features = (const int64_t*)(d_in + o_feat);
  D.weights = (const int64_t*)(d_in + o_w);
  D.labels = d_in + o_lab;
  D.idx = (const uint32_t*)(d_in + o_idx);
  D.peer_ids = (const uint64_t*)(d_in + o_peer);
  D.round = (const Fr*)(d_in + o_raw) + T;
  D.krows = (const Fr*)(d_in + o_krows);
  D.rows = d_rows;
  D.nodes = d_nodes;
  D.root_off = n * map.off[depth];
  D.summed = d_g64;
  D.grad = d_g64 + n * dim;
  D.rem = d_g64 + 2 * n * dim;
  D.gfr = d_gfr;
  D.vh = d_vh;
  D.roots = d_roots;
  D.masked = d_masked;
  D.c1 = d_u32;
  D.status = d_u32 + n;
  D.bal = d_bal;
  D.trn = d_trn;
  D.sec = d_sec;

  PosConsts K3;
  pos_tables_width(P, 3, &K3.C, &K3.M, &K3.rp);
  const Fr* zeros = pos_tables_zeros(P);

  // ---- leaves ----
  int pe = prof ? prof->begin("prepare_leaves", st) : -1;
  hipLaunchKernelGGL(k_prepare_rows, dim3(zk_grid(n * S * len, 256)), dim3(256), 0, st, D.features, D.labels, n * S,
                     dim, d_rows);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  if (tree) HIP_TRY_ERR(vhash_dev(P, d_rows, n * S, len, d_lchunk, d_nodes, 1, true, st), where, err);
  if (prof) prof->end(pe, st, (double)n * S);  // units: leaves

  if (tree) {
    // ---- levels ----
    for (uint32_t l = 0; l < depth; l++) {
      pe = prof ? prof->begin("prepare_levels", st) : -1;
      const size_t lanes = n * map.live[l + 1];
      hipLaunchKernelGGL(k_prepare_level, dim3(zk_grid(lanes, 256)), dim3(256), 0, st, K3, d_nodes + n * map.off[l],
                         map.live[l], zeros + l, d_nodes + n * map.off[l + 1], map.live[l + 1], n);
      HIP_TRY_ERR(hipGetLastError(), where, err);
      if (prof) prof->end(pe, st, (double)lanes);  // units: node hashes
    }
    // ---- openings ----
    if (d_bal || d_trn) {
      pe = prof ? prof->begin("prepare_open", st) : -1;
      if (d_bal) {
        const size_t sib = 5 + (size_t)S * dim + S;
        hipLaunchKernelGGL(k_prepare_open, dim3(zk_grid(n * S * depth, 256)), dim3(256), 0, st, map, d_nodes, zeros, n,
                           S, depth, (const uint32_t*)nullptr, d_bal, nb, sib, sib + (size_t)S * depth);
        HIP_TRY_ERR(hipGetLastError(), where, err);
      }
      if (d_trn) {
        const size_t sib = 6 + 5 * (size_t)dim + (size_t)batch * dim + batch;
        hipLaunchKernelGGL(k_prepare_open, dim3(zk_grid(n * batch * depth, 256)), dim3(256), 0, st, map, d_nodes,
                           zeros, n, batch, depth, D.idx, d_trn, nt, sib, sib + (size_t)batch * depth);
        HIP_TRY_ERR(hipGetLastError(), where, err);
      }
      if (prof) prof->end(pe, st, (double)n * depth * ((d_bal ? S : 0) + (d_trn ? batch : 0)));  // units: siblings
    }
  }

  // ---- gradient ----
  pe = prof ? prof->begin("prepare_gradient", st) : -1;
  hipLaunchKernelGGL(k_prepare_gradient, dim3(zk_grid(n * dim, 256)), dim3(256), 0, st, D);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  if (prof) prof->end(pe, st, (double)n * dim);  // units: coordinates

  // ---- commitments ----
  pe = prof ? prof->begin("prepare_commit", st) : -1;
  HIP_TRY_ERR(admit_signed_dev(D.grad, n * dim, d_gfr, st), where, err);
  HIP_TRY_ERR(admit_signed_dev(D.weights, dim, d_gfr + n * dim, st), where, err);
  HIP_TRY_ERR(vhash_dev(P, d_gfr, n + 1, dim, d_gchunk, d_vh, 1, true, st), where, err);
  hipLaunchKernelGGL(k_prepare_clients, dim3(zk_grid(n, 256)), dim3(256), 0, st, K3, D);
  HIP_TRY_ERR(hipGetLastError(), where, err);
  if (peers)  // root_K = Poseidon(master, keys...)
    HIP_TRY_ERR(poseidon_rows(P, peers + 1, n, D.krows, peers + 1, false, d_roots + 3, 4, false, st), where, err);
  if (prof) prof->end(pe, st, (double)n);  // units: clients

  // ---- masks ----
  if (peers) {
    pe = prof ? prof->begin("prepare_masks", st) : -1;
    SecaggDev M;
    M.n_rows = n;
    M.n_terms = T;
    M.n_chunks = n_chunks;
    M.dim = dim;
    M.chunk_terms = ct;
    M.negate_if_less = false;  // sigma_ij = +1 when i < j
    M.raw = (const Fr*)(d_in + o_raw);
    M.term_a = (const uint64_t*)(d_in + o_own);
    M.term_b = D.peer_ids;
    M.term_ptr = (const uint64_t*)(d_in + o_tptr);
    M.chunk_ptr = (const uint64_t*)(d_in + o_cptr);
    M.chunk_row = (const uint32_t*)(d_in + o_crow);
    M.base = d_gfr;
    M.key = d_key;
    M.lo = d_lo;
    M.hi = d_hi;
    M.neg = d_neg;
    M.part = d_part;
    M.out = d_masked;
    if (int rc = secagg_eval_dev(P, M, st, prof, err)) return rc;
    if (prof) prof->end(pe, st, (double)T * dim);  // units: mask hashes
  }

  // ---- the input vectors below their openings ----
  if (d_bal || d_trn || d_sec) {
    pe = prof ? prof->begin("prepare_inputs", st) : -1;
    double units = 0;
    if (d_bal) {
      const size_t head = 5 + (size_t)S * dim + S;
      hipLaunchKernelGGL(k_prepare_inputs<0>, dim3(zk_grid(n * head, 256)), dim3(256), 0, st, D, head);
      units += (double)n * head;
    }
    if (d_trn) {
      const size_t head = 6 + 5 * (size_t)dim + (size_t)batch * dim + batch;
      hipLaunchKernelGGL(k_prepare_inputs<1>, dim3(zk_grid(n * head, 256)), dim3(256), 0, st, D, head);
      units += (double)n * head;
    }
    if (d_sec) {
      hipLaunchKernelGGL(k_prepare_inputs<2>, dim3(zk_grid(n * ns, 256)), dim3(256), 0, st, D, ns);
      units += (double)n * ns;
    }
    HIP_TRY_ERR(hipGetLastError(), where, err);
    if (prof) prof->end(pe, st, units);  // units: values
  }

  // ---- the requested outputs, each copied once ----
  auto down = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
    return (dst && bytes) ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st) : hipSuccess;
  };
  HIP_TRY_ERR(down(out.balance_inputs, d_bal, n * nb * 32), where, err);
  HIP_TRY_ERR(down(out.training_inputs, d_trn, n * nt * 32), where, err);
  if (want_sec) HIP_TRY_ERR(down(out.secagg_inputs, d_sec, n * ns * 32), where, err);
  HIP_TRY_ERR(down(out.roots, d_roots, n * 4 * 32), where, err);
  HIP_TRY_ERR(down(out.gradients, D.grad, n * dim * 8), where, err);
  if (peers) HIP_TRY_ERR(down(out.masked, d_masked, n * dim * 32), where, err);
  HIP_TRY_ERR(down(out.c1, D.c1, n * 4), where, err);
  HIP_TRY_ERR(down(out.status, D.status, n * 4), where, err);
  HIP_TRY_ERR(hipStreamSynchronize(st), where, err);
  return ZKFL_OK;
}

}  // namespace zkfl

namespace {

int bad(const std::string& msg) { return zkfl::fail(ZKFL_E_ARG, "round_prepare: " + msg); }

bool lt_r(const uint8_t* v) {
  uint32_t w[8];
  memcpy(w, v, 32);
  return zkfl::fr_lt_r(w);
}

uint64_t mag(int64_t x) { return x < 0 ? 0ull - (uint64_t)x : (uint64_t)x; }

}  // namespace

extern "C" int zkfl_round_prepare(zkfl_ctx* ctx, const zkfl_prepare_round* in, const zkfl_prepare_out* out) {
  using zkfl::fail;
  if (!ctx || !in || !out) return bad("null argument");
  const size_t n = in->n;
  const uint32_t S = in->samples, dim = in->dim, depth = in->depth, batch = in->batch, peers = in->peers;
  if (dim < 1 || dim > ZKFL_PREPARE_MAX_DIM)
    return bad("dim " + std::to_string(dim) + " must be in 1.." + std::to_string(ZKFL_PREPARE_MAX_DIM));
  if (depth < 1 || depth > ZKFL_MERKLE_MAX_DEPTH)
    return bad("depth " + std::to_string(depth) + " must be in 1.." + std::to_string(ZKFL_MERKLE_MAX_DEPTH));
  if (S < 1 || S > (1ull << depth))
    return bad("samples " + std::to_string(S) + " must be in 1..2^depth = " + std::to_string(1ull << depth));
  if (batch < 1 || batch > S) return bad("batch " + std::to_string(batch) + " must be in 1..samples = " + std::to_string(S));
  if (in->precision == 0) return bad("precision must be at least 1");
  if (in->tau_squared == ~0ull) return bad("tau_squared must be below 2^64 - 1: the circuit compares with tau_squared + 1");
  if (peers > ZKFL_PREPARE_MAX_PEERS)
    return bad("peers " + std::to_string(peers) + " must be at most " + std::to_string(ZKFL_PREPARE_MAX_PEERS));
  if (peers == 0 && (out->secagg_inputs || out->masked || in->peer_ids || in->keys || in->master_keys))
    return bad("peers == 0 means no secagg part: secagg_inputs, masked, peer_ids, keys and master_keys must be NULL");
  if (n >= (1ull << 32)) return bad("n must be < 2^32");
  if (n && (!in->round || !in->weights || !in->ids || !in->features || !in->labels)) return bad("null argument");
  if (n && peers && (!in->peer_ids || !in->keys || !in->master_keys))
    return bad("peers > 0 needs peer_ids, keys and master_keys");
  {  // every launch and every buffer of the call within one grid
    const size_t nb = zkfl::prepare_balance_len(S, dim, depth), nt = zkfl::prepare_training_len(batch, dim, depth),
                 ns = zkfl::prepare_secagg_len(dim, peers);
    const unsigned __int128 widest = std::max({nb, nt, ns, (size_t)S * (dim + 1), (size_t)peers * dim});
    if ((unsigned __int128)n * widest > (1ull << 36))
      return bad("n x the longest input vector exceeds 2^36 values: prepare the round in several calls");
  }
  if (in->round && !lt_r(in->round)) return bad("round is not < r");
  for (size_t i = 0; i < n; i++)
    for (uint32_t s = 0; s < S; s++)
      if (in->labels[i * S + s] > 1)
        return bad("client " + std::to_string(i) + ": label " + std::to_string(s) + " is " +
                   std::to_string(in->labels[i * S + s]) + ", not 0 or 1");
  if (in->batch_idx)
    for (size_t i = 0; i < n; i++)
      for (uint32_t b = 0; b < batch; b++)
        if (in->batch_idx[i * batch + b] >= S)
          return bad("client " + std::to_string(i) + ": batch_idx " + std::to_string(b) + " is " +
                     std::to_string(in->batch_idx[i * batch + b]) + ", samples is " + std::to_string(S));
  std::vector<std::pair<uint64_t, uint32_t>> seen;
  for (size_t i = 0; i < n && peers; i++) {
    seen.clear();
    for (uint32_t j = 0; j < peers; j++) {
      const uint64_t p = in->peer_ids[i * peers + j];
      if (p == in->ids[i]) return bad("client " + std::to_string(i) + ": peer " + std::to_string(j) + " is the client's own id");
      seen.emplace_back(p, j);
      if (!lt_r(in->keys + 32 * (i * peers + j)))
        return bad("client " + std::to_string(i) + ": key " + std::to_string(j) + " is not < r");
    }
    std::sort(seen.begin(), seen.end());
    for (size_t q = 1; q < seen.size(); q++)
      if (seen[q].first == seen[q - 1].first)
        return bad("client " + std::to_string(i) + ": peer " + std::to_string(seen[q].second) + " repeats peer " +
                   std::to_string(seen[q - 1].second));
    if (!lt_r(in->master_keys + 32 * i)) return bad("client " + std::to_string(i) + ": master key is not < r");
  }
  // the overflow bound: batch * F * (dim * F * W + precision) <= 2^63 - 1, so that every int64 sum of
  // the gradient kernel is exact; the steps below stay under 2^128
  {
    uint64_t F = 0, W = 0;
    size_t f_at = 0;
    for (size_t i = 0; i < n * S * dim; i++)
      if (mag(in->features[i]) > F) {
        F = mag(in->features[i]);
        f_at = i;
      }
    for (uint32_t k = 0; k < dim && in->weights; k++) W = std::max(W, mag(in->weights[k]));
    const unsigned __int128 lim = (1ull << 63) - 1;
    bool over = false;
    if (F) {
      const unsigned __int128 fw = (unsigned __int128)F * W;  // <= 2^126
      over = fw > lim;
      if (!over) {
        const unsigned __int128 inner = fw * dim + in->precision;  // < 2^72
        over = inner > lim;
        if (!over) {
          const unsigned __int128 x = inner * F;  // < 2^126
          over = x > lim || x * batch > lim;
        }
      }
    }
    if (over)
      return bad("overflow bound: batch * F * (dim * F * W + precision) exceeds 2^63 - 1 with F = " + std::to_string(F) +
                 " (client " + std::to_string(f_at / ((size_t)S * dim)) + ", feature " +
                 std::to_string(f_at % ((size_t)S * dim)) + ") and W = " + std::to_string(W));
  }
  if (!n) return ZKFL_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = pos_ready(ctx);
  if (rc) return rc;
  std::string err;
  rc = zkfl::prepare_run(ctx->pos, *in, *out, ctx->st, &ctx->prof, err);
  return rc ? fail(rc, err) : ZKFL_OK;
}
