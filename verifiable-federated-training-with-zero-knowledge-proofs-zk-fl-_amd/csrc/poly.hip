// The polynomial stage's kernels (see poly.h).
#include "poly.h"

#include <algorithm>

#include "common.h"
#include "msm_api.h"
#include "wtrace.h"

using namespace zkfl;

namespace {

// ABC as a segmented sum over the flat term array (A rows then B rows; rp[0..2n] row pointers).
// coef raw = coef * R^2 mod r (snarkjs zkey section 4), w std form, so
// mont_mul(coef_raw, w) = coef * w * R = Montgomery form of coef*w.  Rows range from 1 to ~130
// terms (Poseidon S-box inputs carry ~61-term combinations), so one lane per row leaves ~2/3 of
// the lanes idle; instead lane c takes the ABC_L terms [c*L, c*L+L), emitting the sum of its
// first row segment to head[c], of its last to tail[c], and rows wholly inside the chunk
// straight to abc[row]; k_abc_rows stitches rows j and n+j and forms c = a*b.
// (ABC_L and the term encodings, AbcTerms: poly.h)
// One lane's chunk (the body of k_abc_chunks and of its gated twin below).
template <bool PACKED>
ZK_DEV void abc_chunk(const uint32_t* __restrict__ rp, uint32_t nrows, const AbcTerms& T, const Fr* __restrict__ w,
                      uint32_t K, Fr* __restrict__ head, Fr* __restrict__ tail, Fr* __restrict__ abc) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t p0 = c * ABC_L;
  if (p0 >= K) return;
  const uint32_t p1 = p0 + ABC_L < K ? p0 + ABC_L : K;
  const uint32_t* __restrict__ cols = T.cols;
  const Fr* __restrict__ coefs = T.coefs;
  const uint32_t cmask = PACKED ? (1u << T.cshift) - 1u : 0xFFFFFFFFu;
  auto coef_of = [&](uint32_t t, uint32_t p) { return PACKED ? coefs[t >> T.cshift] : coefs[p]; };
  // row containing p0: largest r with rp[r] <= p0 (empty rows share their start with the next)
  auto row_of = [&](uint32_t p, uint32_t lo) {
    uint32_t hi = nrows - 1;
    while (lo < hi) {
      const uint32_t mid = (lo + hi + 1) >> 1;
      if (rp[mid] <= p) lo = mid;
      else hi = mid - 1;
    }
    return lo;
  };
  uint32_t r = row_of(p0, 0), rend = rp[r + 1];
  Fr acc = fp_zero<FrP>();
  bool first = true;
  // software-pipelined: term p+1's witness gather (and p+2's term word) are in flight while
  // term p is multiplied
  uint32_t t1 = (p0 + 1 < p1) ? cols[p0 + 1] : 0u;
  const uint32_t t0 = cols[p0];
  Fr wv = w[t0 & cmask], cf = coef_of(t0, p0);
  for (uint32_t p = p0; p < p1; p++) {
    Fr wn, cn;
    uint32_t t2 = 0;
    if (p + 1 < p1) {
      wn = w[t1 & cmask];
      cn = coef_of(t1, p + 1);
    }
    if (p + 2 < p1) t2 = cols[p + 2];
    if (p == rend) {  // row boundary inside the chunk
      if (first) head[c] = acc;
      else abc[r] = acc;
      first = false;
      acc = fp_zero<FrP>();
      // next non-empty row: usually r + 1; a run of empty rows (the domain padding after the
      // last constraint: ~241 K rows at 2^19) is skipped by binary search, not walked row by row
      r++;
      rend = rp[r + 1];
      if (rend == p) {
        r = row_of(p, r);
        rend = rp[r + 1];
      }
    }
    acc = fp_add(acc, fp_mul(cf, wv));
    wv = wn;
    cf = cn;
    t1 = t2;
  }
  if (first) head[c] = acc;
  else tail[c] = acc;
}

template <bool PACKED>
__global__ void __launch_bounds__(64) k_abc_chunks(const uint32_t* __restrict__ rp, uint32_t nrows, AbcTerms T,
                                                   const Fr* __restrict__ w, uint32_t K, Fr* __restrict__ head,
                                                   Fr* __restrict__ tail, Fr* __restrict__ abc) {
  ZK_WT(WT_ABC);
  ZK_LIGHT();
  abc_chunk<PACKED>(rp, nrows, T, w, K, head, tail, abc);
}

// (abc_row, the row stitching over head / tail / abc: poly.h)
ZK_DEV void abc_rows_lane(const uint32_t* __restrict__ rp, size_t n, uint32_t K, const Fr* __restrict__ head,
                          const Fr* __restrict__ tail, Fr* __restrict__ abc) {
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Fr a = abc_row(rp, (uint32_t)j, K, head, tail, abc);
  const Fr b = abc_row(rp, (uint32_t)(n + j), K, head, tail, abc);
  abc[j] = a;
  abc[n + j] = b;
  abc[2 * n + j] = fp_mul(a, b);
}

__global__ void __launch_bounds__(256) k_abc_rows(const uint32_t* __restrict__ rp, size_t n, uint32_t K,
                                                  const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                  Fr* __restrict__ abc) {
  ZK_WT(WT_ABC_ROWS);
  ZK_LIGHT();
  abc_rows_lane(rp, n, K, head, tail, abc);
}

// ---- The grouped ABC (poly.h AbcGrouped).  Every kernel reads the slot's plain flag state[1]
// (uniform: one scalar load) and returns at once when the proof runs the other form. ----

// k_abc_chunks and k_abc_rows for a launch that runs only when the plain flag equals `when`: over
// the reduced CSR (when = 0), or over the original rows (when = 1)
template <bool PACKED>
__global__ void __launch_bounds__(64) k_abc_chunks_when(const uint32_t* __restrict__ rp, uint32_t nrows, AbcTerms T,
                                                        const Fr* __restrict__ w, uint32_t K, Fr* __restrict__ head,
                                                        Fr* __restrict__ tail, Fr* __restrict__ abc,
                                                        const uint32_t* __restrict__ state, uint32_t when) {
  if ((state[1] != 0) != (when != 0)) return;
  ZK_WT(WT_ABC);
  ZK_LIGHT();
  abc_chunk<PACKED>(rp, nrows, T, w, K, head, tail, abc);
}

__global__ void __launch_bounds__(256) k_abc_rows_plain(const uint32_t* __restrict__ rp, size_t n, uint32_t K,
                                                        const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                        Fr* __restrict__ abc, const uint32_t* __restrict__ state) {
  if (!state[1]) return;
  ZK_WT(WT_ABC_ROWS);
  ZK_LIGHT();
  abc_rows_lane(rp, n, K, head, tail, abc);
}

// a_j, b_j = the values of the classes of rows j and n + j, stitched over the reduced CSR's chunks
__global__ void __launch_bounds__(256) k_abc_rows_grouped(const uint32_t* __restrict__ crp,
                                                          const uint32_t* __restrict__ cls, size_t n, uint32_t Kd,
                                                          const Fr* __restrict__ head, const Fr* __restrict__ tail,
                                                          const Fr* __restrict__ cls_val, Fr* __restrict__ abc,
                                                          const uint32_t* __restrict__ state) {
  if (state[1]) return;
  ZK_WT(WT_ABC_ROWS);
  ZK_LIGHT();
  const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const Fr a = abc_row(crp, cls[j], Kd, head, tail, cls_val);
  const Fr b = abc_row(crp, cls[n + j], Kd, head, tail, cls_val);
  abc[j] = a;
  abc[n + j] = b;
  abc[2 * n + j] = fp_mul(a, b);
}

// The dirty constraints again, from the original rows: FIX_LANES lanes per constraint stride its A
// row, then its B row, and fold their sums by butterfly, so a and b of one constraint have one
// writer (the group's first lane) whichever of its rows a missing wire sits in.
constexpr int FIX_LANES = 8, FIX_T = 256, FIX_BLOCKS_MAX = 256;
template <bool PACKED>
__global__ void __launch_bounds__(FIX_T) k_abc_fix(const uint32_t* __restrict__ rp, AbcTerms T,
                                                   const Fr* __restrict__ w, size_t n,
                                                   const uint32_t* __restrict__ state,
                                                   const uint32_t* __restrict__ dirty, uint32_t cap,
                                                   Fr* __restrict__ abc, uint32_t* __restrict__ report) {
  // the marking is complete (stream order): the proof's dirty count and plain flag for the host
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    report[0] = state[0];
    report[1] = state[1];
  }
  if (state[1]) return;
  ZK_WT(WT_ABC_ROWS);
  ZK_LIGHT();
  const uint32_t cnt = state[0] < cap ? state[0] : cap;
  const uint32_t lane = threadIdx.x % FIX_LANES;
  const uint32_t cmask = PACKED ? (1u << T.cshift) - 1u : 0xFFFFFFFFu;
  const uint32_t step = gridDim.x * (FIX_T / FIX_LANES);
  // d is the same in the FIX_LANES lanes of a group, so a group enters and leaves the loop together
  for (uint32_t d = (blockIdx.x * FIX_T + threadIdx.x) / FIX_LANES; d < cnt; d += step) {
    const uint32_t j = dirty[d];
    Fr ab[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const uint32_t r = h ? (uint32_t)n + j : j, e = rp[r + 1];
      Fr acc = fp_zero<FrP>();
      for (uint32_t p = rp[r] + lane; p < e; p += FIX_LANES) {
        const uint32_t t = T.cols[p];
        acc = fp_add(acc, fp_mul(PACKED ? T.coefs[t >> T.cshift] : T.coefs[p], w[t & cmask]));
      }
#pragma unroll
      for (int off = FIX_LANES / 2; off; off >>= 1) {
        Fr o;
#pragma unroll
        for (int k = 0; k < 8; k++) o.v[k] = __shfl_xor(acc.v[k], off, FIX_LANES);
        acc = fp_add(acc, o);
      }
      ab[h] = acc;
    }
    if (lane == 0) {
      abc[j] = ab[0];
      abc[n + j] = ab[1];
      abc[2 * n + j] = fp_mul(ab[0], ab[1]);
    }
  }
}

// h = a*b - c (coset evaluations), to standard form for the H MSM.
__global__ void k_join(const Fr* __restrict__ abc, size_t n, Fr* __restrict__ h) {
  ZK_WT(WT_JOIN);
  ZK_LIGHT();
  size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
#if ZK_KNOCKOUT & 4
  // NTT knock-out (timing only): a*b - c vanishes on the domain, so without the coset shift h would
  // be zero and the H MSM would lose its digits too; a*b + c keeps h a full-size scalar vector
  Fr v = fp_add(fp_mul(abc[j], abc[n + j]), abc[2 * n + j]);
#else
  Fr v = fp_sub(fp_mul(abc[j], abc[n + j]), abc[2 * n + j]);
#endif
  h[j] = fp_from_mont(v);
}

// Blinding scalar slots referenced by the compacted bases' index maps (std form):
// extra = [1, r, s, -r*s].  plain -> all zero (parity hook: pure MSMs).
// The tails the chain empties: ProofStart (poly.h).
// A proof chain's first kernel, one launch for what were up to four: the augmentation scalars
// (1, r, s, -rs) of the merged MSMs, res[3] = infinity (the merged C + H leaves the H slot
// empty), and the proof's MSM tails emptied (buckets, nnz, liveness: blockIdx.y = tail).
// rs_host: the slot's pinned r | s | GLV halves (host memory, coherent), copied to d_rs for the
// assembly; the augmentation scalars are computed from the host copy directly.
__global__ void __launch_bounds__(256) k_proof_start(const uint32_t* __restrict__ rs_host, uint32_t* __restrict__ d_rs,
                                                     Fr* __restrict__ extra, int plain, uint32_t* __restrict__ res3,
                                                     const ProofStart ps) {
  ZK_WT(WT_SET_EXTRA);
  ZK_LIGHT();
  const int y = blockIdx.y;
  if (ps.w_dst) {  // uniform per launch
    __shared__ const uint4* src;
    if (threadIdx.x == 0) src = reinterpret_cast<const uint4*>(*ps.w_src_host);
    __syncthreads();
    const size_t nb = (size_t)gridDim.x * gridDim.y * blockDim.x;
    for (size_t i = ((size_t)y * gridDim.x + blockIdx.x) * blockDim.x + threadIdx.x; i < ps.w_nvec; i += nb)
      ps.w_dst[i] = src[i];
  }
  if (y == 0 && ps.gr_state)  // uniform per launch
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < ps.gr_words; i += gridDim.x * blockDim.x)
      ps.gr_state[i] = 0u;
  if (y == 0 && blockIdx.x == 2 && threadIdx.x < RS_WORDS) d_rs[threadIdx.x] = rs_host[threadIdx.x];
  if (y == 0 && blockIdx.x == 0 && threadIdx.x == 0) {
    const Fr* rs = reinterpret_cast<const Fr*>(rs_host);
    Fr one = fp_zero<FrP>();
    one.v[0] = plain ? 0u : 1u;
    Fr r = plain ? fp_zero<FrP>() : rs[0];
    Fr s = plain ? fp_zero<FrP>() : rs[1];
    extra[0] = one;
    extra[1] = r;
    extra[2] = s;
    extra[3] = fp_from_mont(fp_neg(fp_mul(fp_to_mont(r), fp_to_mont(s))));
  }
  if (y == 0 && blockIdx.x == 1 && res3 && threadIdx.x < sizeof(G1P) / 4) res3[threadIdx.x] = 0u;  // ZZ = 0
  if (y >= ps.n) return;
  uint4* b = ps.buckets[y];
  const size_t nv = ps.nvec[y];
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x)
    b[i] = make_uint4(0, 0, 0, 0);
  if (blockIdx.x == 0 && threadIdx.x == 0) *ps.nnz[y] = 0;
  if (blockIdx.x == 0 && threadIdx.x < MSM_LIVE_LEVELS) ps.live[y][threadIdx.x] = 0;
}

__global__ void k_fr_std_to_mont(Fr* __restrict__ a, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a[i] = fp_to_mont(a[i]);
}

__global__ void k_fr_mont_to_std(Fr* __restrict__ a, size_t n) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  a[i] = fp_from_mont(a[i]);
}

}  // namespace

namespace zkfl {

hipError_t zk_wtrace_bind_poly(const WtBuf& b) { return zk_wtrace_bind_tu(b); }

void abc_chunks(hipStream_t st, const uint32_t* rp, uint32_t nrows, const AbcTerms& T, const Fr* w, uint32_t K,
                Fr* head, Fr* tail, Fr* abc) {
  if (T.cshift)
    hipLaunchKernelGGL(k_abc_chunks<true>, dim3(zk_grid((K + ABC_L - 1) / ABC_L, 64)), dim3(64), 0, st, rp, nrows, T, w,
                       K, head, tail, abc);
  else
    hipLaunchKernelGGL(k_abc_chunks<false>, dim3(zk_grid((K + ABC_L - 1) / ABC_L, 64)), dim3(64), 0, st, rp, nrows, T, w,
                       K, head, tail, abc);
}

void abc_rows(hipStream_t st, const uint32_t* rp, size_t n, uint32_t K, const Fr* head, const Fr* tail, Fr* abc) {
  hipLaunchKernelGGL(k_abc_rows, dim3(zk_grid(n, 256)), dim3(256), 0, st, rp, n, K, head, tail, abc);
}

void abc_grouped(hipStream_t st, const AbcGrouped& G, const uint32_t* rp, size_t n, const AbcTerms& T, const Fr* w,
                 uint32_t K, Fr* head, Fr* tail, Fr* abc) {
  auto chunks = [&](const uint32_t* rows, uint32_t nrows, const AbcTerms& terms, uint32_t k, Fr* whole, uint32_t when) {
    const dim3 grid(zk_grid((k + ABC_L - 1) / ABC_L, 64));
    if (terms.cshift)
      hipLaunchKernelGGL(k_abc_chunks_when<true>, grid, dim3(64), 0, st, rows, nrows, terms, w, k, head, tail, whole,
                         G.state, when);
    else
      hipLaunchKernelGGL(k_abc_chunks_when<false>, grid, dim3(64), 0, st, rows, nrows, terms, w, k, head, tail, whole,
                         G.state, when);
  };
  chunks(G.crp, G.classes, G.terms, G.Kd, G.cls_val, 0);
  hipLaunchKernelGGL(k_abc_rows_grouped, dim3(zk_grid(n, 256)), dim3(256), 0, st, G.crp, G.cls, n, G.Kd, head, tail,
                     G.cls_val, abc, G.state);
  const dim3 fix_grid(std::min<unsigned>(zk_grid((size_t)G.cap * FIX_LANES, FIX_T), FIX_BLOCKS_MAX));
  if (T.cshift)
    hipLaunchKernelGGL(k_abc_fix<true>, fix_grid, dim3(FIX_T), 0, st, rp, T, w, n, G.state, G.dirty, G.cap, abc, G.report);
  else
    hipLaunchKernelGGL(k_abc_fix<false>, fix_grid, dim3(FIX_T), 0, st, rp, T, w, n, G.state, G.dirty, G.cap, abc, G.report);
  chunks(rp, (uint32_t)(2 * n), T, K, abc, 1);
  hipLaunchKernelGGL(k_abc_rows_plain, dim3(zk_grid(n, 256)), dim3(256), 0, st, rp, n, K, head, tail, abc, G.state);
}

void join_h(hipStream_t st, const Fr* abc, size_t n, Fr* h) {
  hipLaunchKernelGGL(k_join, dim3(zk_grid(n, 256)), dim3(256), 0, st, abc, n, h);
}

void proof_start(hipStream_t st, const uint32_t* rs_host, uint32_t* d_rs, Fr* extra, int plain, uint32_t* res3,
                 const ProofStart& ps) {
  hipLaunchKernelGGL(k_proof_start, dim3(128, ps.n), dim3(256), 0, st, rs_host, d_rs, extra, plain, res3, ps);
}

void fr_std_to_mont(hipStream_t st, Fr* a, size_t n) {
  hipLaunchKernelGGL(k_fr_std_to_mont, dim3(zk_grid(n, 256)), dim3(256), 0, st, a, n);
}

void fr_mont_to_std(hipStream_t st, Fr* a, size_t n) {
  hipLaunchKernelGGL(k_fr_mont_to_std, dim3(zk_grid(n, 256)), dim3(256), 0, st, a, n);
}

}  // namespace zkfl
