// libzkfl: MI355X-native Groth16 prover (BN254) behind the C ABI in include/zkfl.h.
//
// Replaces `snarkjs groth16 prove` [ext] as invoked by the reference harness
// (tests/full_system_simulation.mjs:773-776).  Algorithm per proof (snarkjs groth16_prove,
// restated in oracle/groth16.py::prove):
//   1. buildABC1: a = A.w, b = B.w over the domain rows (zkey section 4 coefficients),
//      c = a o b                                           -> k_abc (CSR rows, Montgomery)
//   2. a,b,c: ifft -> * inc^i -> fft  (odd coset)          -> ntt_coset_shift (3 vectors)
//   3. joinABC: h = a*b - c, from Montgomery               -> k_join
//   4. multiExpAffine A(w), B1(w), B2(w), C(w_priv), H(h)  -> msm_run (G1 x4, G2 x1)
//   5. pi_a = A + alpha1 + r delta1, pi_b = B2 + beta2 + s delta2,
//      pi_c = C + H + s pi_a + r (B1 + beta1 + s delta1) - r s delta1
//      The constant terms are folded into the MSMs as extra bases (alpha1/delta1 on A,
//      beta1/delta1 on B1, beta2/delta2 on B2, delta1 with scalar -rs on C); only
//      s*pi_a + r*B1 remains for k_assemble (GLV halves, windowed, one wave each), then affine.
// Everything from the device-resident witness to the 256-byte proof runs on the GPU; the host
// only parses files, uploads, and launches.
// This unit holds the thread's error string, the context's lifetime and the entry points that
// are glue around the engines' own units (MSM, NTT, setup, verification, witness, Poseidon /
// Merkle).  The proof chain itself: poly.hip (ABC, join), assemble.hip (pi_a, pi_b, pi_c), prove.hip
// (slots, schedules, the prove entry points), key_load.hip (zkey -> device).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <sys/random.h>

#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "assemble.h"
#include "devbufs.h"
#include "field29.h"
#include "glv.h"
#include "host_parse.h"
#include "merkle.h"
#include "objects.h"
#include "poly.h"
#include "setup.h"
#include "verify.h"
#include "witness.h"

using namespace zkfl;

// The calling thread's last error (zkfl_last_error): the library's one definition; every unit
// sets it through fail / hip_fail.
static thread_local std::string g_err;

int zkfl::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

int zkfl::hip_fail(hipError_t e, const char* where) {
  return hip_rc(e, where, g_err);
}

namespace {

int parse_wtns(const uint8_t* buf, size_t len, WtnsView& out) {
  std::string err;
  int rc = wtns_parse(buf, len, out, err);  // csrc/host_parse.cc
  return rc ? fail(rc, err) : ZKFL_OK;
}

template <class F>
int run_msm_primitive(zkfl_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t* out) {
  if (!ctx || !bases || !scalars || !out || n == 0) return fail(ZKFL_E_ARG, "msm: bad args");
  hipStream_t st = ctx->st;
  struct Engine {  // released on every exit path
    MsmBases<F> mb;
    MsmScratch<F> ms;
    MsmTail<F> mt;
    ~Engine() {
      msm_bases_free(mb);
      msm_scratch_free(ms);
      msm_tail_free(mt);
    }
  } E;
  DevBufs D;
  Affine<F>* d_b;
  uint32_t* d_s;
  XYZZ<F>* d_r;
  Affine<F>* d_o;
  const int c = msm_pick_c(n);
  const char* const where = "msm primitive";
  HIP_TRY(msm_bases_alloc(E.mb, n, c), where);
  HIP_TRY(msm_scratch_alloc(E.ms, n, c, st), where);
  HIP_TRY(msm_tail_alloc(E.mt, n, c), where);
  HIP_TRY(D.get(&d_b, n), where);
  HIP_TRY(D.get(&d_s, n * 8), where);
  HIP_TRY(D.get(&d_r, 1), where);
  HIP_TRY(D.get(&d_o, 1), where);
  HIP_TRY(hipMemcpyAsync(d_b, bases, n * sizeof(Affine<F>), hipMemcpyHostToDevice, st), where);
  HIP_TRY(hipMemcpyAsync(d_s, scalars, n * 32, hipMemcpyHostToDevice, st), where);
  HIP_TRY(msm_bases_set(E.mb, d_b, nullptr, 0xFFFFFFFFu, st), where);
  HIP_TRY(msm_run(E.mb, E.ms, E.mt, d_s, nullptr, d_r, st, &ctx->prof,
                  std::is_same<F, FqOps>::value ? "msm_accumulate_g1" : "msm_accumulate_g2"),
          where);
  point_out(st, d_r, 1, reinterpret_cast<uint32_t*>(d_o));
  HIP_TRY(hipGetLastError(), where);
  HIP_TRY(hipMemcpyAsync(out, d_o, sizeof(Affine<F>), hipMemcpyDeviceToHost, st), where);
  HIP_TRY(hipStreamSynchronize(st), where);
  return ZKFL_OK;
}

int check_fr_array(const uint8_t* v, size_t count, const char* what) {
  for (size_t i = 0; i < count; i++) {
    uint32_t w[8];
    memcpy(w, v + 32 * i, 32);
    if (!fr_lt_r(w)) return fail(ZKFL_E_ARG, std::string(what) + " " + std::to_string(i) + " is not < r");
  }
  return ZKFL_OK;
}

// leaves (device, Montgomery) -> full padded tree (host, std)
int tree_from_device_leaves(zkfl_ctx* ctx, DevBufs& B, const Fr* d_leaves, size_t n, uint32_t depth,
                            uint8_t* tree_out) {
  hipStream_t st = ctx->st;
  const size_t nodes = ((size_t)2 << depth) - 1;
  Fr *d_work, *d_tree;
  HIP_TRY(B.get(&d_work, merkle_work_size(n, depth)), "alloc");
  HIP_TRY(B.get(&d_tree, nodes), "alloc");
  int pi = ctx->prof.begin("merkle", st);
  HIP_TRY(merkle_build(ctx->pos, d_leaves, n, depth, d_tree, d_work, st), "merkle");
  ctx->prof.end(pi, st, (double)(merkle_work_size(n, depth) - n));
  HIP_TRY(hipMemcpyAsync(tree_out, d_tree, nodes * 32, hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  return ZKFL_OK;
}

// Host checks of a parity hook's Fq inputs (std, 8 x 32-bit words), on the 29-bit engine's
// host-callable code: w < q
bool fq_words_lt_p(const uint32_t (&w)[8]) {
  const F29 a = f29_pack(w), c = f29_canon_sub<1>(a);  // a < 2^256 < 6q: unchanged exactly when a < q
  uint32_t d = 0;
  for (int i = 0; i < 9; i++) d |= a.v[i] ^ c.v[i];
  return d == 0;
}
// (x, y) is (0, 0), or x, y < q and y^2 = x^3 + 3.  A product is a b 2^-261 mod q, so both sides are
// taken times 2^-522: (y y) 1, (x x) x, (3 1) 1; each < 1.01 q, the right side's sum < 2.02 q.
bool g1_std_ok(const uint32_t (&x)[8], const uint32_t (&y)[8]) {
  uint32_t nz = 0;
  for (int i = 0; i < 8; i++) nz |= x[i] | y[i];
  if (!nz) return true;
  if (!fq_words_lt_p(x) || !fq_words_lt_p(y)) return false;
  const F29 X = f29_pack(x), Y = f29_pack(y);
  F29 one = f29_zero(), three = f29_zero();
  one.v[0] = 1;
  three.v[0] = 3;
  const F29 lhs = f29_canon_sub<1>(f29_mul(f29_mul(Y, Y), one));
  F29 rhs = f29_add_lazy(f29_mul(f29_mul(X, X), X), f29_mul(f29_mul(three, one), one));
  f29_norm(rhs);
  rhs = f29_canon_sub<2>(rhs);
  uint32_t d = 0;
  for (int i = 0; i < 9; i++) d |= lhs.v[i] ^ rhs.v[i];
  return d == 0;
}

int tree_args(zkfl_ctx* ctx, size_t n, uint32_t depth, const void* in, const void* out) {
  if (!ctx || !out || (n && !in)) return fail(ZKFL_E_ARG, "merkle: null argument");
  if (depth > ZKFL_MERKLE_MAX_DEPTH) return fail(ZKFL_E_ARG, "merkle: depth must be <= 30");
  if (n > ((size_t)1 << depth)) return fail(ZKFL_E_ARG, "merkle: more leaves than 2^depth");
  return ZKFL_OK;
}

}  // namespace

int zkfl::pos_ready(zkfl_ctx* ctx) {
  if (ctx->pos) return ZKFL_OK;
  std::string err;
  int rc = pos_tables_create(&ctx->pos, ctx->st, err);
  return rc ? fail(rc, err) : ZKFL_OK;
}

void zkfl::ctx_retain(zkfl_ctx* ctx) { ctx->refs.fetch_add(1, std::memory_order_relaxed); }

// Drops one reference; the last one tears the context down.
void zkfl::ctx_release(zkfl_ctx* ctx) {
  if (ctx->refs.fetch_sub(1, std::memory_order_acq_rel) != 1) return;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->st);
  ctx->prof.reset();
  vk_free(ctx->vk);
  pos_tables_free(ctx->pos);
  if (ctx->asm_buf) (void)hipFree(ctx->asm_buf);
  if (ctx->wt.rec) {  // a wave trace still bound: unbind before its buffer goes
    (void)zkfl_debug_wtrace(ctx, 0, 0, nullptr, nullptr);
  }
  (void)hipStreamDestroy(ctx->st);
  delete ctx;
}

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int zkfl_version(void) { return 1; }

int zkfl_debug_glv_split(const uint8_t k[32], uint8_t out[40]) {
  if (!k || !out) return fail(ZKFL_E_ARG, "null argument");
  uint32_t kk[8];
  memcpy(kk, k, 32);
  if (!fr_lt_r(kk)) return fail(ZKFL_E_ARG, "k must be < r");
  GlvScalar a, b;
  glv_split(kk, a, b);
  memcpy(out, a.mag, 16);
  memcpy(out + 16, &a.neg, 4);
  memcpy(out + 20, b.mag, 16);
  memcpy(out + 36, &b.neg, 4);
  return ZKFL_OK;
}

int zkfl_debug_g1_glv_mul(zkfl_ctx* ctx, size_t n, const uint8_t* points, const uint8_t* zs, const uint8_t* scalars,
                          uint8_t* out) {
  if (!ctx || (n && (!points || !scalars || !out))) return fail(ZKFL_E_ARG, "null argument");
  if (n == 0) return ZKFL_OK;
  if (n > (1u << 20)) return fail(ZKFL_E_ARG, "glv mul: n too large");
  std::vector<GlvScalar> ks(2 * n);
  for (size_t i = 0; i < n; i++) {
    uint32_t kk[8], x[8], y[8];
    memcpy(kk, scalars + 32 * i, 32);
    if (!fr_lt_r(kk)) return fail(ZKFL_E_ARG, "glv mul: scalar " + std::to_string(i) + " is not < r");
    glv_split(kk, ks[2 * i], ks[2 * i + 1]);
    // the chains test no special case: they are only right on the curve's (prime-order) points
    memcpy(x, points + 64 * i, 32);
    memcpy(y, points + 64 * i + 32, 32);
    if (!g1_std_ok(x, y))
      return fail(ZKFL_E_ARG, "glv mul: point " + std::to_string(i) + " is neither (0, 0) nor on the curve");
    if (zs) {
      memcpy(x, zs + 32 * i, 32);
      uint32_t nz = 0;
      for (int k = 0; k < 8; k++) nz |= x[k];
      if (!nz || !fq_words_lt_p(x)) return fail(ZKFL_E_ARG, "glv mul: z " + std::to_string(i) + " is not in [1, q)");
    }
  }
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  DevBufs D;
  uint32_t *d_p, *d_o, *d_z = nullptr;
  GlvScalar* d_k;
  HIP_TRY(D.get(&d_p, n * 16), "glv mul");
  HIP_TRY(D.get(&d_k, ks.size()), "glv mul");
  HIP_TRY(D.get(&d_o, n * 16), "glv mul");
  HIP_TRY(hipMemcpyAsync(d_p, points, n * 64, hipMemcpyHostToDevice, st), "glv mul");
  if (zs) {
    HIP_TRY(D.get(&d_z, n * 8), "glv mul");
    HIP_TRY(hipMemcpyAsync(d_z, zs, n * 32, hipMemcpyHostToDevice, st), "glv mul");
  }
  HIP_TRY(hipMemcpyAsync(d_k, ks.data(), ks.size() * sizeof(GlvScalar), hipMemcpyHostToDevice, st), "glv mul");
  debug_glv_mul(st, (uint32_t)n, d_p, d_z, d_k, d_o);
  HIP_TRY(hipGetLastError(), "glv mul");
  HIP_TRY(hipMemcpyAsync(out, d_o, n * 64, hipMemcpyDeviceToHost, st), "glv mul");
  HIP_TRY(hipStreamSynchronize(st), "glv mul");
  return ZKFL_OK;
}

int zkfl_debug_asm_ops(zkfl_ctx* ctx, int policy, int op, size_t n, const uint32_t* in, uint32_t* out) {
  if (!ctx || (n && (!in || !out))) return fail(ZKFL_E_ARG, "asm ops: null argument");
  if (!debug_asm_op_ok(policy, op))
    return fail(ZKFL_E_ARG, "asm ops: no operation " + std::to_string(op) + " in policy " + std::to_string(policy));
  if (n == 0) return ZKFL_OK;
  if (n > (1u << 14)) return fail(ZKFL_E_ARG, "asm ops: n too large (at most 2^14 cases)");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  DevBufs D;
  uint32_t *d_i, *d_o;
  HIP_TRY(D.get(&d_i, n * ASM_DBG_IN), "asm ops");
  HIP_TRY(D.get(&d_o, n * ASM_DBG_OUT), "asm ops");
  HIP_TRY(hipMemcpyAsync(d_i, in, n * ASM_DBG_IN * 4, hipMemcpyHostToDevice, st), "asm ops");
  HIP_TRY(hipMemsetAsync(d_o, 0, n * ASM_DBG_OUT * 4, st), "asm ops");
  debug_asm_ops(st, policy, op, (uint32_t)n, d_i, d_o);
  HIP_TRY(hipGetLastError(), "asm ops");
  HIP_TRY(hipMemcpyAsync(out, d_o, n * ASM_DBG_OUT * 4, hipMemcpyDeviceToHost, st), "asm ops");
  HIP_TRY(hipStreamSynchronize(st), "asm ops");
  return ZKFL_OK;
}

const char* zkfl_last_error(void) { return g_err.c_str(); }

int zkfl_device_count(int* count) {
  if (!count) return fail(ZKFL_E_ARG, "null");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *count = 0;
    return hip_fail(e, "hipGetDeviceCount");
  }
  *count = c;
  return ZKFL_OK;
}

int zkfl_ctx_create(int device, zkfl_ctx** out) {
  if (!out) return fail(ZKFL_E_ARG, "null out");
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess || c == 0) return fail(ZKFL_E_DEVICE, "no HIP device available");
  if (device < 0 || device >= c) return fail(ZKFL_E_ARG, "device index out of range");
  HIP_TRY(hipSetDevice(device), "hipSetDevice");
  zkfl_ctx* ctx = new zkfl_ctx();
  ctx->device = device;
  // the scheduler's options (SchedOpts): the environment is read here only
  auto env = [](const char* name, int dflt) {
    const char* v = getenv(name);
    return v ? atoi(v) : dflt;
  };
  ctx->opts.graph = env("ZKFL_GRAPH", 1) != 0;
  ctx->opts.stagger = env("ZKFL_STAGGER", 1) != 0;
  ctx->opts.lowlat = env("ZKFL_LOWLAT", 1) != 0;
  ctx->opts.fast_wsum = env("ZKFL_FAST_WSUM", 1) != 0;
  ctx->opts.small_logn = env("ZKFL_SMALL_LOGN", 16);
  ctx->opts.ab_shared = env("ZKFL_AB_SHARED", 1) != 0;
  ctx->opts.groups = env("ZKFL_GROUPS", 1) != 0;
  ctx->opts.group_min_batch = std::max(1, env("ZKFL_GROUP_MIN_BATCH", 8));
  ctx->opts.group_rows = env("ZKFL_GROUP_ROWS", 1) != 0;
  ctx->opts.group_rows_cap = std::max(0, env("ZKFL_GROUP_ROWS_CAP", 0));
  hipError_t e = hipStreamCreateWithFlags(&ctx->st, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete ctx;
    return hip_fail(e, "hipStreamCreate");
  }
  *out = ctx;
  return ZKFL_OK;
}

// The caller's handle: after this call the handle is gone, but keys and witness programs still
// alive keep the device state until they are freed.
int zkfl_ctx_destroy(zkfl_ctx* ctx) {
  if (!ctx) return ZKFL_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->st);
  ctx_release(ctx);
  return ZKFL_OK;
}

int zkfl_ctx_set_profiling(zkfl_ctx* ctx, int enabled) {
  if (!ctx) return fail(ZKFL_E_ARG, "null ctx");
  ctx->prof.on = enabled != 0;
  ctx->prof.serialize = enabled == 2;
  return ZKFL_OK;
}

int zkfl_ctx_profile(zkfl_ctx* ctx, const char* name, double* total_ms, uint64_t* launches, double* units,
                     double* median_ms) {
  if (!ctx || !name || !total_ms || !launches) return fail(ZKFL_E_ARG, "null");
  (void)hipSetDevice(ctx->device);
  HIP_TRY(hipDeviceSynchronize(), "sync");
  ctx->prof.query(name, total_ms, launches, units, median_ms);
  return ZKFL_OK;
}

int zkfl_ctx_profile_reset(zkfl_ctx* ctx) {
  if (!ctx) return fail(ZKFL_E_ARG, "null ctx");
  (void)hipStreamSynchronize(ctx->st);
  ctx->prof.reset();
  return ZKFL_OK;
}

int zkfl_ctx_synchronize(zkfl_ctx* ctx) {
  if (!ctx) return fail(ZKFL_E_ARG, "null ctx");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  HIP_TRY(hipDeviceSynchronize(), "sync");  // every stream of this process: the proof slots' too
  return ZKFL_OK;
}

int zkfl_witness_upload(zkfl_ctx* ctx, const zkfl_key* key, const uint8_t* wtns, size_t wtns_len,
                        zkfl_witness** out) {
  if (!ctx || !key || !wtns || !out) return fail(ZKFL_E_ARG, "null argument");
  WtnsView v;
  int rc = parse_wtns(wtns, wtns_len, v);
  if (rc) return rc;
  if (v.n != key->nVars) return fail(ZKFL_E_MISMATCH, "wtns: nWitness != zkey nVars");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  zkfl_witness* w = new zkfl_witness();
  w->key = key;
  hipError_t e = hipMalloc(&w->d, (size_t)v.n * 32);
  if (e == hipSuccess) e = hipMemcpyAsync(w->d, v.data, (size_t)v.n * 32, hipMemcpyHostToDevice, ctx->st);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
  if (e != hipSuccess) {
    zkfl_witness_free(w);
    return hip_fail(e, "witness upload");
  }
  w->pub.assign(v.data + 32, v.data + 32 + (size_t)key->nPub * 32);
  *out = w;
  return ZKFL_OK;
}

int zkfl_witness_free(zkfl_witness* w) {
  if (!w) return ZKFL_OK;
  if (w->d) (void)hipFree(w->d);
  delete w;
  return ZKFL_OK;
}

int zkfl_debug_wtrace(zkfl_ctx* ctx, int op, uint32_t cap, void* out, uint32_t* count) {
#if !ZK_WTRACE
  (void)ctx;
  (void)op;
  (void)cap;
  (void)out;
  (void)count;
  return fail(ZKFL_E_ARG, "wave trace: this library was built without -DZK_WTRACE=1");
#else
  if (!ctx || op < 0 || op > 2) return fail(ZKFL_E_ARG, "wave trace: bad arguments");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  auto bind_all = [](const WtBuf& b) {
    hipError_t e = zk_wtrace_bind_poly(b);
    if (e == hipSuccess) e = zk_wtrace_bind_asm(b);
    if (e == hipSuccess) e = zk_wtrace_bind_g1(b);
    if (e == hipSuccess) e = zk_wtrace_bind_g2(b);
    if (e == hipSuccess) e = zk_wtrace_bind_sort(b);
    if (e == hipSuccess) e = zk_wtrace_bind_ntt(b);
    if (e == hipSuccess) e = zk_wtrace_bind_wit(b);
    if (e == hipSuccess) e = zk_wtrace_bind_joint(b);
    return e;
  };
  HIP_TRY(hipDeviceSynchronize(), "wave trace: sync");
  if (op == 2) {
    if (!ctx->wt.rec) return fail(ZKFL_E_ARG, "wave trace: not started");
    uint32_t n = 0;
    HIP_TRY(hipMemcpy(&n, ctx->wt.cnt, 4, hipMemcpyDeviceToHost), "wave trace: count");
    HIP_TRY(bind_all(WtBuf()), "wave trace: unbind");
    const uint32_t m = std::min(n, std::min(cap, ctx->wt.cap));
    if (out && m) HIP_TRY(hipMemcpy(out, ctx->wt.rec, (size_t)m * sizeof(WtRec), hipMemcpyDeviceToHost), "wave trace: read");
    if (count) *count = n;
    return ZKFL_OK;
  }
  HIP_TRY(bind_all(WtBuf()), "wave trace: unbind");
  if (ctx->wt.rec) (void)hipFree(ctx->wt.rec);
  if (ctx->wt.cnt) (void)hipFree(ctx->wt.cnt);
  ctx->wt = WtBuf();
  if (op == 0) return ZKFL_OK;
  if (cap == 0) return fail(ZKFL_E_ARG, "wave trace: cap must be > 0");
  HIP_TRY(hipMalloc(&ctx->wt.rec, (size_t)cap * sizeof(WtRec)), "wave trace: alloc");
  HIP_TRY(hipMalloc(&ctx->wt.cnt, 4), "wave trace: alloc");
  HIP_TRY(hipMemset(ctx->wt.cnt, 0, 4), "wave trace: reset");
  ctx->wt.cap = cap;
  HIP_TRY(bind_all(ctx->wt), "wave trace: bind");
  HIP_TRY(hipDeviceSynchronize(), "wave trace: sync");
  return ZKFL_OK;
#endif
}

int zkfl_msm_g1(zkfl_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[64]) {
  return run_msm_primitive<FqOps>(ctx, bases, scalars, n, out);
}

int zkfl_msm_g2(zkfl_ctx* ctx, const uint8_t* bases, const uint8_t* scalars, size_t n, uint8_t out[128]) {
  return run_msm_primitive<Fq2Ops>(ctx, bases, scalars, n, out);
}

int zkfl_debug_ntt_coset(zkfl_ctx* ctx, uint8_t* data, uint32_t logn, uint32_t nvec, size_t vstride, int col_max) {
  if (!ctx || !data || logn < 1 || logn > 27 || nvec < 1 || nvec > 3 || col_max > NTT_COL_TILE_LOG)
    return fail(ZKFL_E_ARG, "ntt: bad args");
  const size_t n = (size_t)1 << logn;
  if (vstride < n || vstride > ((size_t)1 << 32)) return fail(ZKFL_E_ARG, "ntt: bad stride");
  hipStream_t st = ctx->st;
  struct Plan {  // released on every exit path
    NttPlan pl;
    ~Plan() { ntt_plan_free(pl); }
  } P;
  DevBufs D;
  Fr* d;
  const size_t count = (size_t)(nvec - 1) * vstride + n;
  HIP_TRY(ntt_plan_alloc(P.pl, (int)logn, st), "ntt");
  if (col_max >= 0) P.pl.col_max = col_max;
  HIP_TRY(D.get(&d, count), "ntt");
  HIP_TRY(hipMemcpyAsync(d, data, count * 32, hipMemcpyHostToDevice, st), "ntt");
  for (uint32_t v = 0; v < nvec; v++) fr_std_to_mont(st, d + v * vstride, n);  // the gaps stay as they are
  HIP_TRY(ntt_coset_shift(P.pl, d, (int)nvec, vstride, st), "ntt");
  for (uint32_t v = 0; v < nvec; v++) fr_mont_to_std(st, d + v * vstride, n);
  HIP_TRY(hipGetLastError(), "ntt");
  HIP_TRY(hipMemcpyAsync(data, d, count * 32, hipMemcpyDeviceToHost, st), "ntt");
  HIP_TRY(hipStreamSynchronize(st), "ntt");
  return ZKFL_OK;
}

int zkfl_ntt_coset(zkfl_ctx* ctx, uint8_t* data, uint32_t logn) {
  return zkfl_debug_ntt_coset(ctx, data, logn, 1, logn <= 27 ? (size_t)1 << logn : 0, -1);
}

int zkfl_debug_coset_join(zkfl_ctx* ctx, const uint8_t* abc, uint32_t logn, int col_max, uint8_t* h_out) {
  if (!ctx || !abc || !h_out || logn < 1 || logn > 27 || col_max > NTT_COL_TILE_LOG)
    return fail(ZKFL_E_ARG, "coset join: bad args");
  const size_t n = (size_t)1 << logn;
  hipStream_t st = ctx->st;
  struct Plan {  // released on every exit path
    NttPlan pl;
    ~Plan() { ntt_plan_free(pl); }
  } P;
  DevBufs D;
  Fr *d, *h;
  HIP_TRY(ntt_plan_alloc(P.pl, (int)logn, st), "coset join");
  if (col_max >= 0) P.pl.col_max = col_max;
  HIP_TRY(D.get(&d, 3 * n), "coset join");
  HIP_TRY(D.get(&h, n), "coset join");
  HIP_TRY(hipMemcpyAsync(d, abc, 3 * n * 32, hipMemcpyHostToDevice, st), "coset join");
  fr_std_to_mont(st, d, 3 * n);
  // the prover's own two calls (abc_ntt, csrc/prove.hip)
  HIP_TRY(ntt_coset_shift(P.pl, d, 3, n, st), "coset join");
  join_h(st, d, n, h);
  HIP_TRY(hipGetLastError(), "coset join");
  HIP_TRY(hipMemcpyAsync(h_out, h, n * 32, hipMemcpyDeviceToHost, st), "coset join");
  HIP_TRY(hipStreamSynchronize(st), "coset join");
  return ZKFL_OK;
}

// Ceremony primitives (csrc/setup.hip)
static int setup_gen_mul_abi(zkfl_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out, bool g2) {
  if (!ctx || !scalars || !out) return fail(ZKFL_E_ARG, "gen_mul: bad args");
  hipError_t e = setup_gen_mul(g2, ctx->st, scalars, n, out);
  return e == hipSuccess ? ZKFL_OK : hip_fail(e, "gen_mul");
}

int zkfl_setup_g1_gen_mul(zkfl_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out) {
  return setup_gen_mul_abi(ctx, scalars, n, out, false);
}

int zkfl_setup_g2_gen_mul(zkfl_ctx* ctx, const uint8_t* scalars, size_t n, uint8_t* out) {
  return setup_gen_mul_abi(ctx, scalars, n, out, true);
}

static int setup_scale_abi(zkfl_ctx* ctx, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out,
                           bool g2) {
  if (!ctx || (n && (!points || !scalars || !out))) return fail(ZKFL_E_ARG, "setup scale: bad args");
  hipError_t e = setup_scale(g2, ctx->st, points, scalars, n, out);
  return e == hipSuccess ? ZKFL_OK : hip_fail(e, "setup scale");
}

int zkfl_setup_g1_scale(zkfl_ctx* ctx, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out) {
  return setup_scale_abi(ctx, points, scalars, n, out, false);
}

int zkfl_setup_g2_scale(zkfl_ctx* ctx, const uint8_t* points, const uint8_t* scalars, size_t n, uint8_t* out) {
  return setup_scale_abi(ctx, points, scalars, n, out, true);
}

static int setup_lagrange_abi(zkfl_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out, bool g2) {
  if (!ctx || !points || !out) return fail(ZKFL_E_ARG, "setup lagrange: bad args");
  if (logn > 28) return fail(ZKFL_E_ARG, "setup lagrange: logn > 28 (BN254 Fr 2-adicity)");
  hipError_t e = setup_lagrange(g2, ctx->st, points, (int)logn, out);
  return e == hipSuccess ? ZKFL_OK : hip_fail(e, "setup lagrange");
}

int zkfl_setup_g1_lagrange(zkfl_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out) {
  return setup_lagrange_abi(ctx, points, logn, out, false);
}

int zkfl_setup_g2_lagrange(zkfl_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out) {
  return setup_lagrange_abi(ctx, points, logn, out, true);
}

static int setup_lincomb_abi(zkfl_ctx* ctx, const uint8_t* bases, size_t n_bases, size_t n_out,
                             const uint64_t* rowptr, const uint32_t* idx, const uint8_t* coefs, uint8_t* out,
                             bool g2) {
  if (!ctx || !rowptr || (n_out && !out)) return fail(ZKFL_E_ARG, "setup lincomb: bad args");
  if (rowptr[0] != 0) return fail(ZKFL_E_ARG, "setup lincomb: rowptr[0] != 0");
  for (size_t r = 0; r < n_out; r++)
    if (rowptr[r + 1] < rowptr[r]) return fail(ZKFL_E_ARG, "setup lincomb: rowptr not monotonic at " + std::to_string(r));
  const uint64_t nnz = rowptr[n_out];
  if (nnz >= 0xffffffffull) return fail(ZKFL_E_ARG, "setup lincomb: more than 2^32 - 2 terms");
  if (nnz && (!idx || !coefs || !bases)) return fail(ZKFL_E_ARG, "setup lincomb: bad args");
  for (uint64_t t = 0; t < nnz; t++)  // no device access outside the bases
    if (idx[t] >= n_bases) return fail(ZKFL_E_ARG, "setup lincomb: term " + std::to_string(t) + " base index out of range");
  hipError_t e = setup_lincomb(g2, ctx->st, bases, n_bases, n_out, rowptr, idx, coefs, out);
  return e == hipSuccess ? ZKFL_OK : hip_fail(e, "setup lincomb");
}

int zkfl_setup_g1_lincomb(zkfl_ctx* ctx, const uint8_t* bases, size_t n_bases, size_t n_out, const uint64_t* rowptr,
                          const uint32_t* idx, const uint8_t* coefs, uint8_t* out) {
  return setup_lincomb_abi(ctx, bases, n_bases, n_out, rowptr, idx, coefs, out, false);
}

int zkfl_setup_g2_lincomb(zkfl_ctx* ctx, const uint8_t* bases, size_t n_bases, size_t n_out, const uint64_t* rowptr,
                          const uint32_t* idx, const uint8_t* coefs, uint8_t* out) {
  return setup_lincomb_abi(ctx, bases, n_bases, n_out, rowptr, idx, coefs, out, true);
}

// ---------------------------------------------------------------------------
// Verification (csrc/verify.hip)
// ---------------------------------------------------------------------------
static int vk_get(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t npub) {
  if (!vk_same(ctx->vk, vk, vk_len)) {
    vk_free(ctx->vk);
    ctx->vk = nullptr;
    std::string err;
    VkDev* p = nullptr;
    int rc = vk_prepare(vk, vk_len, ctx->st, &p, err);
    if (rc != ZKFL_OK) return fail(rc, err);
    ctx->vk = p;
  }
  if (vk_npub(ctx->vk) != npub)
    return fail(ZKFL_E_MISMATCH, "verify: " + std::to_string(npub) + " public signals, key expects " +
                                     std::to_string(vk_npub(ctx->vk)));
  return ZKFL_OK;
}

int zkfl_groth16_verify_batch(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, size_t n, const uint8_t* pubs,
                              size_t npub, const uint8_t* proofs, int32_t* results) {
  if (!ctx || !vk || (n && (!proofs || !results || (npub && !pubs)))) return fail(ZKFL_E_ARG, "verify: bad args");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  int rc = vk_get(ctx, vk, vk_len, npub);
  if (rc != ZKFL_OK) return rc;
  std::string err;
  rc = verify_batch(ctx->vk, n, pubs, proofs, results, ctx->st, err);
  return rc == ZKFL_OK ? rc : fail(rc, err);
}

int zkfl_groth16_verify(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, const uint8_t* pub, size_t npub,
                        const uint8_t proof[256]) {
  int32_t res = 0;
  int rc = zkfl_groth16_verify_batch(ctx, vk, vk_len, 1, pub, npub, proof, &res);
  return rc == ZKFL_OK ? res : rc;
}

static int pairing_common(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out, int fe) {
  if (!ctx || (n && (!g1 || !g2 || !out))) return fail(ZKFL_E_ARG, "pairing: bad args");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::string err;
  int rc = pairing_batch(n, g1, g2, fe, out, ctx->st, err);
  return rc == ZKFL_OK ? rc : fail(rc, err);
}

int zkfl_pairing(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* gt_out) {
  return pairing_common(ctx, n, g1, g2, gt_out, 1);
}

int zkfl_debug_miller_loop(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, uint8_t* out) {
  return pairing_common(ctx, n, g1, g2, out, 0);
}

int zkfl_debug_wave_pairing(zkfl_ctx* ctx, size_t n, const uint8_t* g1, const uint8_t* g2, int final_exp,
                            uint8_t* out) {
  if (!ctx || (n && (!g1 || !g2 || !out))) return fail(ZKFL_E_ARG, "pairing: bad args");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::string err;
  int rc = pairing_wave_batch(n, g1, g2, final_exp, out, ctx->st, &ctx->prof, err);
  return rc == ZKFL_OK ? rc : fail(rc, err);
}

// Resident verification keys; a round's proofs, each against its own key
int zkfl_vkey_load(zkfl_ctx* ctx, const uint8_t* vk, size_t vk_len, zkfl_vkey** out) {
  if (!ctx || !vk || !out) return fail(ZKFL_E_ARG, "vkey_load: null argument");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::string err;
  VkDev* p = nullptr;
  int rc = vk_prepare(vk, vk_len, ctx->st, &p, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  void* wtab = nullptr;
  rc = vk_wave_tables(p, ctx->st, &wtab, err);
  if (rc != ZKFL_OK) {
    vk_free(p);
    return fail(rc, err);
  }
  zkfl_vkey* k = new zkfl_vkey();
  k->ctx = ctx;
  k->vk = p;
  k->wtab = wtab;
  k->wave_ok = vk_npub(p) <= ZKFL_VERIFY_WAVE_MAX_PUBLIC;
  ctx_retain(ctx);
  *out = k;
  return ZKFL_OK;
}

int zkfl_vkey_info(const zkfl_vkey* key, uint32_t* n_public) {
  if (!key) return fail(ZKFL_E_ARG, "vkey_info: null key");
  if (n_public) *n_public = vk_npub(key->vk);
  return ZKFL_OK;
}

int zkfl_vkey_free(zkfl_vkey* key) {
  if (!key) return fail(ZKFL_E_ARG, "vkey_free: null key");
  zkfl_ctx* ctx = key->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->st);
  vk_wave_tables_free(key->wtab);
  vk_free(key->vk);
  delete key;
  ctx_release(ctx);
  return ZKFL_OK;
}

// The per-job argument checks of the multi-key entry points (fn names the caller in the message)
static int verify_jobs_check(const char* fn, zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys,
                             const uint8_t* const* pubs, const size_t* npubs) {
  const std::string who = std::string(fn) + ": job ";
  for (size_t i = 0; i < n; i++) {
    if (!vkeys[i] || vkeys[i]->ctx != ctx) return fail(ZKFL_E_ARG, who + std::to_string(i) + " has no key of this context");
    const uint32_t want = vk_npub(vkeys[i]->vk);
    if (npubs[i] != want)
      return fail(ZKFL_E_MISMATCH, who + std::to_string(i) + " has " + std::to_string(npubs[i]) +
                                       " public signals, its key expects " + std::to_string(want));
    if (want && !pubs[i]) return fail(ZKFL_E_ARG, who + std::to_string(i) + " has null publics");
  }
  return ZKFL_OK;
}

// n > 0 checked jobs by one of the schedules; the device is set
static int verify_multi_run(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                            const uint8_t* proofs, int32_t* results, int schedule) {
  if (schedule == ZKFL_VERIFY_AUTO)
    schedule = n <= ZKFL_VERIFY_AUTO_WAVES_MAX ? ZKFL_VERIFY_WAVES : ZKFL_VERIFY_LANES;
  // the wave jobs, in job order; every other job by key, in order of first appearance
  std::vector<size_t> wave;
  std::vector<const zkfl_vkey*> lane_keys;
  std::vector<std::vector<size_t>> lane_jobs;
  for (size_t i = 0; i < n; i++) {
    if (schedule == ZKFL_VERIFY_WAVES && vkeys[i]->wave_ok) {
      wave.push_back(i);
      continue;
    }
    size_t g = 0;
    while (g < lane_keys.size() && lane_keys[g] != vkeys[i]) g++;
    if (g == lane_keys.size()) {
      lane_keys.push_back(vkeys[i]);
      lane_jobs.emplace_back();
    }
    lane_jobs[g].push_back(i);
  }
  std::vector<int32_t> res(n, 0), part;
  std::vector<uint8_t> pr, pb;
  std::string err;
  int rc = ZKFL_OK;
  if (!wave.empty()) {
    std::vector<VerifyJob> jobs(wave.size());
    pr.resize(256 * wave.size());
    part.assign(wave.size(), 0);
    for (size_t j = 0; j < wave.size(); j++) {
      const size_t i = wave[j];
      jobs[j] = {vkeys[i]->vk, vkeys[i]->wtab, pubs[i]};
      memcpy(pr.data() + 256 * j, proofs + 256 * i, 256);
    }
    rc = verify_wave(wave.size(), jobs.data(), pr.data(), part.data(), ctx->st, &ctx->prof, err);
    if (rc != ZKFL_OK) return fail(rc, err);
    for (size_t j = 0; j < wave.size(); j++) res[wave[j]] = part[j];
  }
  for (size_t g = 0; g < lane_keys.size(); g++) {
    const std::vector<size_t>& idx = lane_jobs[g];
    const size_t np = vk_npub(lane_keys[g]->vk);
    pr.resize(256 * idx.size());
    pb.resize(32 * np * idx.size() + 1);
    part.assign(idx.size(), 0);
    for (size_t j = 0; j < idx.size(); j++) {
      memcpy(pr.data() + 256 * j, proofs + 256 * idx[j], 256);
      if (np) memcpy(pb.data() + 32 * np * j, pubs[idx[j]], 32 * np);
    }
    rc = verify_batch(lane_keys[g]->vk, idx.size(), pb.data(), pr.data(), part.data(), ctx->st, err);
    if (rc != ZKFL_OK) return fail(rc, err);
    for (size_t j = 0; j < idx.size(); j++) res[idx[j]] = part[j];
  }
  memcpy(results, res.data(), n * sizeof(int32_t));
  return ZKFL_OK;
}

int zkfl_groth16_verify_multi(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                              const size_t* npubs, const uint8_t* proofs, int32_t* results, int schedule) {
  if (!ctx || (n && (!vkeys || !pubs || !npubs || !proofs || !results)))
    return fail(ZKFL_E_ARG, "verify_multi: null argument");
  if (schedule != ZKFL_VERIFY_AUTO && schedule != ZKFL_VERIFY_LANES && schedule != ZKFL_VERIFY_WAVES)
    return fail(ZKFL_E_ARG, "verify_multi: unknown schedule " + std::to_string(schedule));
  if (const int rc = verify_jobs_check("verify_multi", ctx, n, vkeys, pubs, npubs)) return rc;
  if (n == 0) return ZKFL_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  return verify_multi_run(ctx, n, vkeys, pubs, proofs, results, schedule);
}

// z NULL: n x 16 B from the OS CSPRNG into drawn, as rs == NULL for proofs; every 128-bit value is a valid z
static int round_draw_z(size_t n, const uint8_t*& z, std::vector<uint8_t>& drawn) {
  if (z) return ZKFL_OK;
  drawn.resize(16 * n);
  for (size_t got = 0; got < drawn.size();) {
    const size_t want = std::min<size_t>(256, drawn.size() - got);
    if (getrandom(drawn.data() + got, want, 0) != (ssize_t)want) return fail(ZKFL_E_DEVICE, "getrandom failed");
    got += want;
  }
  z = drawn.data();
  return ZKFL_OK;
}

// A round as one random combination (csrc/verify_round.hip).  screened: n flags; *passed: the
// combination is 1.
static int verify_round_combine(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                                const uint8_t* proofs, const uint8_t* z, size_t chunk, uint8_t* gt_out,
                                int32_t* screened, int* passed, uint32_t* nkeys) {
  std::vector<uint8_t> drawn;
  if (const int rc = round_draw_z(n, z, drawn)) return rc;
  std::vector<VerifyJob> jobs(n);
  for (size_t i = 0; i < n; i++) jobs[i] = {vkeys[i]->vk, vkeys[i]->wtab, pubs[i]};
  std::string err;
  const int rc = verify_round(n, jobs.data(), proofs, z, chunk, gt_out, screened, passed, nkeys, ctx->st, &ctx->prof,
                              err);
  return rc == ZKFL_OK ? rc : fail(rc, err);
}

int zkfl_groth16_verify_round(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                              const size_t* npubs, const uint8_t* proofs, const uint8_t* z, int32_t* results,
                              zkfl_round_report* report) {
  if (!ctx || (n && (!vkeys || !pubs || !npubs || !proofs || !results)))
    return fail(ZKFL_E_ARG, "verify_round: null argument");
  if (const int rc = verify_jobs_check("verify_round", ctx, n, vkeys, pubs, npubs)) return rc;
  zkfl_round_report rep = {0, 0, 0, 1, 0};
  if (n == 0) {
    if (report) *report = rep;
    return ZKFL_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<int32_t> screened(n, 0), res(n, 0);
  int passed = 0;
  int rc = verify_round_combine(ctx, n, vkeys, pubs, proofs, z, 0, nullptr, screened.data(), &passed, &rep.keys);
  if (rc != ZKFL_OK) return rc;
  std::vector<size_t> comb;
  for (size_t i = 0; i < n; i++)
    if (!screened[i]) comb.push_back(i);
  rep.screened = (uint32_t)(n - comb.size());
  rep.combined = (uint32_t)comb.size();
  rep.passed = passed ? 1 : 0;
  if (passed) {
    for (size_t i : comb) res[i] = 1;
  } else {  // exact verdicts for the combined jobs, one by one
    const size_t m = comb.size();
    std::vector<const zkfl_vkey*> fk(m);
    std::vector<const uint8_t*> fp(m);
    std::vector<uint8_t> fpr(256 * m);
    std::vector<int32_t> fres(m, 0);
    for (size_t j = 0; j < m; j++) {
      fk[j] = vkeys[comb[j]];
      fp[j] = pubs[comb[j]];
      memcpy(fpr.data() + 256 * j, proofs + 256 * comb[j], 256);
    }
    rc = verify_multi_run(ctx, m, fk.data(), fp.data(), fpr.data(), fres.data(), ZKFL_VERIFY_AUTO);
    if (rc != ZKFL_OK) return rc;
    for (size_t j = 0; j < m; j++) res[comb[j]] = fres[j];
    rep.fallback = (uint32_t)m;
  }
  memcpy(results, res.data(), n * sizeof(int32_t));
  if (report) *report = rep;
  return ZKFL_OK;
}

int zkfl_debug_verify_round(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                            const size_t* npubs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                            uint8_t gt_out[384], int32_t* screened_out) {
  if (!ctx || (n && (!vkeys || !pubs || !npubs || !proofs || !z || !gt_out || !screened_out)))
    return fail(ZKFL_E_ARG, "verify_round: null argument");
  if (const int rc = verify_jobs_check("verify_round", ctx, n, vkeys, pubs, npubs)) return rc;
  if (n == 0) return ZKFL_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<int32_t> screened(n, 0);
  int passed = 0;
  const int rc = verify_round_combine(ctx, n, vkeys, pubs, proofs, z, chunk, gt_out, screened.data(), &passed, nullptr);
  if (rc != ZKFL_OK) return rc;
  memcpy(screened_out, screened.data(), n * sizeof(int32_t));
  return ZKFL_OK;
}

int zkfl_groth16_verify_round_narrow(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys,
                                     const uint8_t* const* pubs, const size_t* npubs, const uint8_t* proofs,
                                     const uint8_t* z, uint32_t group, int32_t* results, zkfl_narrow_report* report) {
  if (!ctx || (n && (!vkeys || !pubs || !npubs || !proofs || !results)))
    return fail(ZKFL_E_ARG, "verify_round_narrow: null argument");
  if (const int rc = verify_jobs_check("verify_round_narrow", ctx, n, vkeys, pubs, npubs)) return rc;
  zkfl_narrow_report rep = {0, 0, 0, 1, 0, 0, 0};
  if (n == 0) {
    if (report) *report = rep;
    return ZKFL_OK;
  }
  const size_t pass = round_pass_size(n, 0);
  if (group > pass)
    return fail(ZKFL_E_ARG, "verify_round_narrow: group " + std::to_string(group) + " exceeds the pass of " +
                                std::to_string(pass) + " jobs");
  if (group == 0 && n < ZKFL_ROUND_NARROW_MIN) {  // too small to narrow, whatever is screened: the plain call
    zkfl_round_report r5;
    const int rc = zkfl_groth16_verify_round(ctx, n, vkeys, pubs, npubs, proofs, z, results, &r5);
    if (rc != ZKFL_OK) return rc;
    rep = {r5.keys, r5.screened, r5.combined, r5.passed, 0, 0, r5.fallback};
    if (report) *report = rep;
    return ZKFL_OK;
  }
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<uint8_t> drawn, group_one;
  if (const int rc = round_draw_z(n, z, drawn)) return rc;
  std::vector<VerifyJob> jobs(n);
  for (size_t i = 0; i < n; i++) jobs[i] = {vkeys[i]->vk, vkeys[i]->wtab, pubs[i]};
  std::vector<int32_t> screened(n, 0), res(n, 0);
  std::vector<uint32_t> group_of(n, 0);
  int passed = 0, narrowed = 0;
  std::string err;
  const size_t gsize = group ? group : std::min<size_t>(ZKFL_ROUND_GROUP, pass);
  int rc = verify_round_narrow(n, jobs.data(), proofs, z, 0, gsize, group ? 0 : ZKFL_ROUND_NARROW_MIN, group_of.data(),
                               &group_one, nullptr, screened.data(), &passed, &narrowed, &rep.keys, ctx->st,
                               &ctx->prof, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  std::vector<size_t> again;  // the jobs to verify one by one
  for (size_t i = 0; i < n; i++) {
    if (screened[i]) continue;
    rep.combined++;
    if (passed || (narrowed && group_one[group_of[i]]))
      res[i] = 1;
    else
      again.push_back(i);
  }
  rep.screened = (uint32_t)n - rep.combined;
  rep.passed = passed ? 1 : 0;
  if (passed || narrowed) rep.groups = (uint32_t)round_group_count(n, 0, gsize);
  if (narrowed)
    for (uint8_t one : group_one) rep.bad_groups += one ? 0 : 1;
  if (!again.empty()) {
    const size_t m = again.size();
    std::vector<const zkfl_vkey*> fk(m);
    std::vector<const uint8_t*> fp(m);
    std::vector<uint8_t> fpr(256 * m);
    std::vector<int32_t> fres(m, 0);
    for (size_t j = 0; j < m; j++) {
      fk[j] = vkeys[again[j]];
      fp[j] = pubs[again[j]];
      memcpy(fpr.data() + 256 * j, proofs + 256 * again[j], 256);
    }
    rc = verify_multi_run(ctx, m, fk.data(), fp.data(), fpr.data(), fres.data(), ZKFL_VERIFY_AUTO);
    if (rc != ZKFL_OK) return rc;
    for (size_t j = 0; j < m; j++) res[again[j]] = fres[j];
    rep.fallback = (uint32_t)m;
  }
  memcpy(results, res.data(), n * sizeof(int32_t));
  if (report) *report = rep;
  return ZKFL_OK;
}

int zkfl_debug_verify_round_groups(zkfl_ctx* ctx, size_t n, const zkfl_vkey* const* vkeys, const uint8_t* const* pubs,
                                   const size_t* npubs, const uint8_t* proofs, const uint8_t* z, size_t chunk,
                                   uint32_t group, uint32_t* group_of, uint8_t* gt_groups, size_t cap,
                                   uint32_t* n_groups, int32_t* screened_out) {
  if (!ctx || !n_groups ||
      (n && (!vkeys || !pubs || !npubs || !proofs || !z || !group_of || !gt_groups || !screened_out)))
    return fail(ZKFL_E_ARG, "verify_round_groups: null argument");
  if (const int rc = verify_jobs_check("verify_round_groups", ctx, n, vkeys, pubs, npubs)) return rc;
  if (n == 0) {
    *n_groups = 0;
    return ZKFL_OK;
  }
  const size_t pass = round_pass_size(n, chunk);
  if (group > pass)
    return fail(ZKFL_E_ARG, "verify_round_groups: group " + std::to_string(group) + " exceeds the pass of " +
                                std::to_string(pass) + " jobs");
  const size_t gsize = group ? group : std::min<size_t>(ZKFL_ROUND_GROUP, pass);
  const size_t G = round_group_count(n, chunk, gsize);
  *n_groups = (uint32_t)G;
  if (cap < G)
    return fail(ZKFL_E_ARG, "verify_round_groups: room for " + std::to_string(cap) + " of " + std::to_string(G) +
                                " groups");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<VerifyJob> jobs(n);
  for (size_t i = 0; i < n; i++) jobs[i] = {vkeys[i]->vk, vkeys[i]->wtab, pubs[i]};
  std::vector<int32_t> screened(n, 0);
  std::vector<uint32_t> gof(n, 0);
  std::vector<uint8_t> group_one, gt;
  int passed = 0, narrowed = 0;
  std::string err;
  const int rc = verify_round_narrow(n, jobs.data(), proofs, z, chunk, gsize, 0, gof.data(), &group_one, &gt,
                                     screened.data(), &passed, &narrowed, nullptr, ctx->st, &ctx->prof, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  memcpy(group_of, gof.data(), n * sizeof(uint32_t));
  memcpy(gt_groups, gt.data(), 384 * G);
  memcpy(screened_out, screened.data(), n * sizeof(int32_t));
  return ZKFL_OK;
}

// ---------------------------------------------------------------------------
// Witness generation (csrc/witness.hip)
// ---------------------------------------------------------------------------
int zkfl_wprog_load(zkfl_ctx* ctx, const uint8_t* prog, size_t len, zkfl_wprog** out) {
  if (!ctx || !prog || !out) return fail(ZKFL_E_ARG, "wprog_load: null argument");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::string err;
  WProg* p = nullptr;
  int rc = wprog_load(prog, len, ctx->st, &p, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  zkfl_wprog* w = new zkfl_wprog();
  w->ctx = ctx;
  ctx_retain(ctx);  // dropped by zkfl_wprog_free
  w->p = p;
  *out = w;
  return ZKFL_OK;
}

int zkfl_wprog_free(zkfl_wprog* prog) {
  if (!prog) return ZKFL_OK;
  zkfl_ctx* ctx = prog->ctx;
  (void)hipSetDevice(ctx->device);
  (void)hipStreamSynchronize(ctx->st);
  wprog_free(prog->p);
  delete prog;
  ctx_release(ctx);
  return ZKFL_OK;
}

int zkfl_wprog_info(const zkfl_wprog* prog, uint32_t* n_wires, uint32_t* n_inputs, uint32_t* n_public) {
  if (!prog) return fail(ZKFL_E_ARG, "null program");
  wprog_info(prog->p, n_wires, n_inputs, n_public);
  return ZKFL_OK;
}

size_t zkfl_wtns_size(const zkfl_wprog* prog) {
  uint32_t nw = 0;
  if (prog) wprog_info(prog->p, &nw, nullptr, nullptr);
  return 76 + 32 * (size_t)nw;
}

static void wtns_header(uint8_t* dst, uint32_t nw) {
  const uint32_t h1[3] = {0x736e7477u /* "wtns" */, 2, 2};
  memcpy(dst, h1, 12);
  uint32_t t = 1;
  uint64_t sz = 40;
  memcpy(dst + 12, &t, 4);
  memcpy(dst + 16, &sz, 8);
  uint32_t n8 = 32;
  memcpy(dst + 24, &n8, 4);
  memcpy(dst + 28, FrP::P, 32);
  memcpy(dst + 60, &nw, 4);
  t = 2;
  sz = 32ull * nw;
  memcpy(dst + 64, &t, 4);
  memcpy(dst + 68, &sz, 8);
}

int zkfl_witness_compute(zkfl_ctx* ctx, const zkfl_wprog* prog, size_t n, const uint8_t* inputs, uint8_t* wtns_out) {
  if (!ctx || !prog || (n && (!wtns_out || !inputs))) return fail(ZKFL_E_ARG, "witness_compute: null argument");
  if (n == 0) return ZKFL_OK;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  uint32_t nw = 0;
  wprog_info(prog->p, &nw, nullptr, nullptr);
  const size_t img = 76 + 32 * (size_t)nw;
  DevBufs D;
  Fr* d;
  HIP_TRY(D.get(&d, n * (size_t)nw), "witness buffer");
  std::vector<Fr*> outs(n);
  for (size_t j = 0; j < n; j++) outs[j] = d + j * nw;
  std::string err;
  const int rc = wprog_run(prog->p, n, inputs, outs.data(), ctx->st, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  for (size_t j = 0; j < n; j++) {
    wtns_header(wtns_out + j * img, nw);
    HIP_TRY(hipMemcpyAsync(wtns_out + j * img + 76, outs[j], 32ull * nw, hipMemcpyDeviceToHost, ctx->st),
            "witness download");
  }
  HIP_TRY(hipStreamSynchronize(ctx->st), "witness download");
  return ZKFL_OK;
}

int zkfl_wprog_parse_inputs(const uint8_t* prog, size_t len, const char* input_json, uint8_t* inputs_out, size_t cap,
                            size_t* n_inputs) {
  if (!prog || !input_json || !n_inputs || (cap && !inputs_out)) return fail(ZKFL_E_ARG, "parse_inputs: null argument");
  std::vector<uint32_t> v;
  std::string err;
  int rc = wprog_image_inputs_json(prog, len, input_json, v, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  *n_inputs = v.size() / 8;
  if (*n_inputs > cap) return fail(ZKFL_E_ARG, "parse_inputs: output buffer too small");
  memcpy(inputs_out, v.data(), v.size() * 4);
  return ZKFL_OK;
}

int zkfl_witness_compute_json(zkfl_ctx* ctx, const zkfl_wprog* prog, const char* input_json, uint8_t* wtns_out) {
  if (!ctx || !prog || !input_json || !wtns_out) return fail(ZKFL_E_ARG, "witness_compute_json: null argument");
  std::vector<uint32_t> v;
  std::string err;
  int rc = wprog_inputs_json(prog->p, input_json, v, err);
  if (rc != ZKFL_OK) return fail(rc, err);
  return zkfl_witness_compute(ctx, prog, 1, reinterpret_cast<const uint8_t*>(v.data()), wtns_out);
}

int zkfl_witness_compute_resident(zkfl_ctx* ctx, const zkfl_wprog* prog, const zkfl_key* key, size_t n,
                                  const uint8_t* inputs, zkfl_witness** out) {
  if (!ctx || !prog || !key || (n && (!out || !inputs))) return fail(ZKFL_E_ARG, "witness_compute: null argument");
  uint32_t nw = 0, npub = 0;
  wprog_info(prog->p, &nw, nullptr, &npub);
  if (nw != key->nVars || npub != key->nPub)
    return fail(ZKFL_E_MISMATCH, "witness program does not match the proving key (nVars / nPublic)");
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  std::vector<zkfl_witness*> ws(n, nullptr);
  std::vector<Fr*> outs(n, nullptr);
  hipError_t e = hipSuccess;
  for (size_t j = 0; j < n && e == hipSuccess; j++) {
    ws[j] = new zkfl_witness();
    ws[j]->key = key;
    e = hipMalloc(&ws[j]->d, 32ull * nw);
    outs[j] = ws[j]->d;
  }
  std::string err;
  int rc = e == hipSuccess ? wprog_run(prog->p, n, inputs, outs.data(), ctx->st, err) : hip_fail(e, "witness alloc");
  if (rc == ZKFL_OK) {
    // public signals (witness[1..nPub]) for the prove call's public.json
    for (size_t j = 0; j < n && e == hipSuccess; j++) {
      ws[j]->pub.resize(32ull * npub);
      if (npub) e = hipMemcpyAsync(ws[j]->pub.data(), ws[j]->d + 1, 32ull * npub, hipMemcpyDeviceToHost, ctx->st);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->st);
    if (e != hipSuccess) rc = hip_fail(e, "public signals");
  } else if (!err.empty()) {
    rc = fail(rc, err);
  }
  if (rc != ZKFL_OK) {
    for (zkfl_witness* w : ws) zkfl_witness_free(w);
    return rc;
  }
  for (size_t j = 0; j < n; j++) out[j] = ws[j];
  return ZKFL_OK;
}


// ---------------------------------------------------------------------------
// Poseidon / vectorHash / Merkle trees (csrc/merkle.hip)
// ---------------------------------------------------------------------------
int zkfl_poseidon_params(uint32_t t, uint8_t* consts_out, uint8_t* xy_out, uint32_t* rp_out) {
  if (t < 2 || t > 17) return fail(ZKFL_E_ARG, "poseidon width t must be in 2..17");
  pos_params_raw(t, consts_out, xy_out);
  if (rp_out) *rp_out = pos_rp(t);
  return ZKFL_OK;
}

int zkfl_poseidon_batch(zkfl_ctx* ctx, uint32_t arity, size_t n, const uint8_t* inputs, uint8_t* out) {
  if (!ctx || (n && (!inputs || !out))) return fail(ZKFL_E_ARG, "poseidon_batch: null argument");
  if (arity < 1 || arity > POS_MAX_ARITY) return fail(ZKFL_E_ARG, "poseidon arity must be in 1..16");
  int rc = check_fr_array(inputs, n * arity, "poseidon input");
  if (rc || !n) return rc;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  if ((rc = pos_ready(ctx))) return rc;
  DevBufs B;
  Fr *d_in, *d_out;
  HIP_TRY(B.get(&d_in, n * arity), "alloc");
  HIP_TRY(B.get(&d_out, n), "alloc");
  hipStream_t st = ctx->st;
  HIP_TRY(hipMemcpyAsync(d_in, inputs, n * arity * 32, hipMemcpyHostToDevice, st), "upload");
  int pi = ctx->prof.begin("poseidon", st);
  HIP_TRY(poseidon_batch(ctx->pos, arity, n, d_in, d_out, st), "poseidon");
  ctx->prof.end(pi, st, (double)n);
  HIP_TRY(hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  return ZKFL_OK;
}

int zkfl_vector_hash_batch(zkfl_ctx* ctx, uint32_t len, size_t n, const uint8_t* values, uint8_t* out) {
  if (!ctx || (n && (!values || !out))) return fail(ZKFL_E_ARG, "vector_hash_batch: null argument");
  if (len < 1 || len > VHASH_CHUNK * VHASH_CHUNK) return fail(ZKFL_E_ARG, "vector length must be in 1..256");
  int rc = check_fr_array(values, n * len, "vector value");
  if (rc || !n) return rc;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  if ((rc = pos_ready(ctx))) return rc;
  DevBufs B;
  Fr *d_in, *d_out, *d_s;
  const size_t nch = (len + VHASH_CHUNK - 1) / VHASH_CHUNK;
  HIP_TRY(B.get(&d_in, n * len), "alloc");
  HIP_TRY(B.get(&d_out, n), "alloc");
  HIP_TRY(B.get(&d_s, n * nch), "alloc");
  hipStream_t st = ctx->st;
  HIP_TRY(hipMemcpyAsync(d_in, values, n * len * 32, hipMemcpyHostToDevice, st), "upload");
  int pi = ctx->prof.begin("vector_hash", st);
  HIP_TRY(vector_hash_batch(ctx->pos, len, n, d_in, d_out, false, d_s, st), "vector hash");
  ctx->prof.end(pi, st, (double)n);
  HIP_TRY(hipMemcpyAsync(out, d_out, n * 32, hipMemcpyDeviceToHost, st), "download");
  HIP_TRY(hipStreamSynchronize(st), "sync");
  return ZKFL_OK;
}

int zkfl_merkle_build(zkfl_ctx* ctx, const uint8_t* leaves, size_t n, uint32_t depth, uint8_t* tree_out) {
  int rc = tree_args(ctx, n, depth, leaves, tree_out);
  if (rc) return rc;
  if ((rc = check_fr_array(leaves, n, "leaf"))) return rc;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  if ((rc = pos_ready(ctx))) return rc;
  DevBufs B;
  Fr *d_raw, *d_leaves;
  HIP_TRY(B.get(&d_raw, n), "alloc");
  HIP_TRY(B.get(&d_leaves, n), "alloc");
  if (n) {
    HIP_TRY(hipMemcpyAsync(d_raw, leaves, n * 32, hipMemcpyHostToDevice, ctx->st), "upload");
    HIP_TRY(fr_to_mont_batch(d_raw, n, d_leaves, ctx->st), "leaves");
  }
  return tree_from_device_leaves(ctx, B, d_leaves, n, depth, tree_out);
}

int zkfl_dataset_commit(zkfl_ctx* ctx, const uint8_t* values, size_t n, uint32_t len, uint32_t depth,
                        uint8_t* tree_out) {
  int rc = tree_args(ctx, n, depth, values, tree_out);
  if (rc) return rc;
  if (len < 1 || len > VHASH_CHUNK * VHASH_CHUNK) return fail(ZKFL_E_ARG, "vector length must be in 1..256");
  if ((rc = check_fr_array(values, n * len, "sample value"))) return rc;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  if ((rc = pos_ready(ctx))) return rc;
  DevBufs B;
  Fr *d_in, *d_leaves, *d_s;
  const size_t nch = (len + VHASH_CHUNK - 1) / VHASH_CHUNK;
  HIP_TRY(B.get(&d_in, n * len), "alloc");
  HIP_TRY(B.get(&d_leaves, n), "alloc");
  HIP_TRY(B.get(&d_s, n * nch), "alloc");
  if (n) {
    HIP_TRY(hipMemcpyAsync(d_in, values, n * len * 32, hipMemcpyHostToDevice, ctx->st), "upload");
    int pi = ctx->prof.begin("vector_hash", ctx->st);
    HIP_TRY(vector_hash_batch(ctx->pos, len, n, d_in, d_leaves, true, d_s, ctx->st), "leaf hashes");
    ctx->prof.end(pi, ctx->st, (double)n);
  }
  return tree_from_device_leaves(ctx, B, d_leaves, n, depth, tree_out);
}

}  // extern "C"
