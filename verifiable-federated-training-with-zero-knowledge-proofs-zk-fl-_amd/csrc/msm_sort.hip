// Bucket sort of the MSM digits, one translation unit for both curves (msm_sort.h).
// Keys are (c-1)-bit bucket numbers, so two counting passes put every non-zero digit in bucket
// order with no look-back and no memsets:
//   count   per block of bases: digits -> LDS histogram of the high key bits -> cnt[bin][block]
//   scan    one workgroup: cnt (bin-major) -> exclusive offsets, bin starts, nnz
//   scatter per block: digits again (the scalars are 2 B per entry, the pairs 6) -> each pair
//           to its high bin at an LDS-atomic cursor
//   bins    one workgroup per high bin: LDS histogram of the low bits, then each pair to its
//           bucket at an LDS-atomic cursor
// Zero digits are dropped (the accumulation reads only the first nnz pairs).  The order inside
// a bucket is arbitrary: a bucket's sum does not depend on it, and the proof is affine.
#include "msm_sort.h"
#include "wtrace.h"

namespace zkfl {

hipError_t zk_wtrace_bind_sort(const WtBuf& b) { return zk_wtrace_bind_tu(b); }

// key bits sorted inside a high bin at window width C, and its low counters
template <int C>
constexpr int msm_sort_lb() {
  return C - 1 - MSM_SORT_HIGH_BITS;
}
template <int C>
constexpr int msm_sort_nl() {
  return 1 << msm_sort_lb<C>();
}

// Window j of a 256-bit scalar (8 x 32-bit words): bits [c j, c j + c) (j is unrolled, so the
// word index and shifts are constants).
template <int C>
ZK_DEV uint32_t msm_window(const uint32_t (&s)[8], int j) {
  const int b = C * j, w = b >> 5, sh = b & 31;
  uint32_t x = s[w] >> sh;
  if (sh + C > 32 && w + 1 < 8) x |= s[w + 1] << (32 - sh);
  return x & ((1u << C) - 1u);
}

// Signed digits of base i: fn(key, val) for every non-zero digit d of its scalar (window j),
// key = |d| - 1 (the bucket), val = (i W + j) | sign << 31
template <int C, class Fn>
ZK_DEV void msm_for_digits(const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ extra,
                           const uint32_t* __restrict__ sidx, uint32_t extra_start, size_t i, Fn&& fn) {
  constexpr int W = msm_w_of(C), NB = msm_nb_of(C);
  const uint32_t si = sidx ? sidx[i] : (uint32_t)i;
  const uint32_t* src = si < extra_start ? scalars + (size_t)si * 8 : extra + (size_t)(si - extra_start) * 8;
  const uint4* sp = reinterpret_cast<const uint4*>(src);
  const uint4 a = sp[0], b = sp[1];
  const uint32_t s[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  uint32_t carry = 0;
#pragma unroll
  for (int j = 0; j < W; j++) {
    const uint32_t raw = msm_window<C>(s, j);
    int32_t d = (int32_t)(raw + carry);
    carry = d > NB ? 1u : 0u;
    if (carry) d -= (1 << C);
    if (d != 0) {
      const uint32_t mag = (uint32_t)(d < 0 ? -d : d);
      fn(mag - 1, (uint32_t)(i * W + j) | (d < 0 ? 0x80000000u : 0u));
    }
  }
}

template <int C>
__global__ void __launch_bounds__(MSM_SORT_T) k_msm_bin_count(const MsmSortArgs A) {
  ZK_WT(WT_SORT_COUNT);
  ZK_LIGHT();
  constexpr int LB = msm_sort_lb<C>();
  const MsmSortJob& J = A.j[blockIdx.y];
  if (blockIdx.x >= J.nblk) return;
  __shared__ uint32_t h[MSM_SORT_HB];
  if (threadIdx.x < MSM_SORT_HB) h[threadIdx.x] = 0;
  __syncthreads();
  const size_t i0 = (size_t)blockIdx.x * J.per_blk, i1 = i0 + J.per_blk < J.n ? i0 + J.per_blk : J.n;
  for (size_t i = i0 + threadIdx.x; i < i1; i += MSM_SORT_T)
    msm_for_digits<C>(J.scalars, J.extra, J.sidx, J.extra_start, i,
                      [&](uint32_t key, uint32_t) { atomicAdd(&h[key >> LB], 1u); });
  __syncthreads();
  if (threadIdx.x < MSM_SORT_HB) J.cnt[(size_t)threadIdx.x * J.nblk + blockIdx.x] = h[threadIdx.x];
}

// cnt[HB * nblk] (bin-major) -> exclusive offsets in place; bin_start[HB + 1]; *nnz.
// The scan keeps all 32 K counters in LDS (~139 KB): gfx950's 160 KB per workgroup.
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "the bucket sort's scan needs gfx950's 160 KB of LDS"
#endif
static __global__ void __launch_bounds__(MSM_SORT_BT) k_msm_bin_scan(const MsmSortArgs A) {
  ZK_WT(WT_SORT_SCAN);
  ZK_LIGHT();
  const MsmSortJob& J = A.j[blockIdx.y];
  uint32_t* __restrict__ cnt = J.cnt;
  uint32_t* __restrict__ bin_start = J.bin_start;
  const uint32_t nblk = J.nblk;
  __shared__ uint32_t c[MSM_SORT_HB * MSM_SORT_MAXBLK + MSM_SORT_BT];  // +1 word per 32: no bank conflicts
  __shared__ uint32_t part[MSM_SORT_BT];
  const uint32_t total = MSM_SORT_HB * nblk, t = threadIdx.x;
  for (uint32_t k = t; k < total; k += MSM_SORT_BT) c[k + (k >> 5)] = cnt[k];
  __syncthreads();
  uint32_t s = 0;
  for (uint32_t q = 0; q < 32; q++) {
    const uint32_t k = t * 32 + q;
    if (k < total) s += c[k + (k >> 5)];
  }
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < MSM_SORT_BT; off <<= 1) {
    const uint32_t v = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  uint32_t run = part[t] - s;
  for (uint32_t q = 0; q < 32; q++) {
    const uint32_t k = t * 32 + q;
    if (k < total) {
      const uint32_t v = c[k + (k >> 5)];
      c[k + (k >> 5)] = run;
      run += v;
    }
  }
  __syncthreads();
  for (uint32_t k = t; k < total; k += MSM_SORT_BT) {
    const uint32_t v = c[k + (k >> 5)];
    cnt[k] = v;
    if (k % nblk == 0) bin_start[k / nblk] = v;
  }
  if (t == MSM_SORT_BT - 1) {
    bin_start[MSM_SORT_HB] = part[t];
    *J.nnz = part[t];
  }
}

template <int C>
__global__ void __launch_bounds__(MSM_SORT_T) k_msm_bin_scatter(const MsmSortArgs A) {
  ZK_WT(WT_SORT_SCATTER);
  ZK_LIGHT();
  constexpr int LB = msm_sort_lb<C>();
  const MsmSortJob& J = A.j[blockIdx.y];
  if (blockIdx.x >= J.nblk) return;
  __shared__ uint32_t cur[MSM_SORT_HB];
  if (threadIdx.x < MSM_SORT_HB) cur[threadIdx.x] = J.cnt[(size_t)threadIdx.x * J.nblk + blockIdx.x];
  __syncthreads();
  uint16_t* __restrict__ keys = J.keys_in;
  uint32_t* __restrict__ vals = J.vals_in;
  const size_t i0 = (size_t)blockIdx.x * J.per_blk, i1 = i0 + J.per_blk < J.n ? i0 + J.per_blk : J.n;
  for (size_t i = i0 + threadIdx.x; i < i1; i += MSM_SORT_T)
    msm_for_digits<C>(J.scalars, J.extra, J.sidx, J.extra_start, i, [&](uint32_t key, uint32_t val) {
      const uint32_t p = atomicAdd(&cur[key >> LB], 1u);
      keys[p] = (uint16_t)key;
      vals[p] = val;
    });
}

// One workgroup per high bin: [bin_start[b], bin_start[b+1]) of (tk, tv) -> buckets in (ko, vo).
// BINT threads per workgroup (MSM_SORT_BINT).  The bin is read from memory twice: once to count
// the low bits, once to place the pairs.
template <int BINT, int NL>
__global__ void __launch_bounds__(BINT) k_msm_bin_sort(const MsmSortArgs A) {
  static_assert(BINT >= NL && BINT <= 1024 && NL >= 64, "bins: one thread per low counter");
  ZK_WT(WT_SORT_BINS);
  ZK_LIGHT();
  const MsmSortJob& J = A.j[blockIdx.y];
  const uint32_t* __restrict__ bin_start = J.bin_start;
  const uint16_t* __restrict__ tk = J.keys_in;
  const uint32_t* __restrict__ tv = J.vals_in;
  uint16_t* __restrict__ ko = J.keys_out;
  uint32_t* __restrict__ vo = J.vals_out;
  __shared__ uint32_t c[NL];
  const uint32_t b0 = bin_start[blockIdx.x], b1 = bin_start[blockIdx.x + 1], t = threadIdx.x;
  if (b0 == b1) return;
  if (t < NL) c[t] = 0;
  __syncthreads();
  for (uint32_t p = b0 + t; p < b1; p += BINT) atomicAdd(&c[tk[p] & (NL - 1)], 1u);
  __syncthreads();
  // exclusive scan of the low counters by the first waves (wave scan + wave totals)
  uint32_t v = 0, x = 0;
  if (t < NL) {
    v = c[t];
    x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t y = __shfl_up(x, o);
      if ((t & 63) >= (uint32_t)o) x += y;
    }
  }
  __shared__ uint32_t wt[NL / 64];
  if (t < NL && (t & 63) == 63) wt[t >> 6] = x;
  __syncthreads();
  if (t < NL) {
    uint32_t base = b0;
    for (uint32_t w = 0; w < (t >> 6); w++) base += wt[w];
    c[t] = base + x - v;
  }
  __syncthreads();
  for (uint32_t p = b0 + t; p < b1; p += BINT) {
    const uint16_t key = tk[p];
    const uint32_t val = tv[p];
    const uint32_t q = atomicAdd(&c[key & (NL - 1)], 1u);
    ko[q] = key;
    vo[q] = val;
  }
}

hipError_t msm_sort_launch(const MsmSortArgs& A, uint32_t gx, int ny, int c, bool sorted, hipStream_t st) {
  return msm_with_c(c, [&](auto cc) {
    constexpr int C = decltype(cc)::value;
    constexpr int NL = msm_sort_nl<C>();
    static_assert(NL >= 64 && NL <= 1024 && MSM_SORT_BINT >= NL, "bins: one thread per low counter");
    hipLaunchKernelGGL((k_msm_bin_count<C>), dim3(gx, ny), dim3(MSM_SORT_T), 0, st, A);
    hipLaunchKernelGGL(k_msm_bin_scan, dim3(1, ny), dim3(MSM_SORT_BT), 0, st, A);
    if (!(ZK_KNOCKOUT & 2) || !sorted) {  // knock-out: an MSM's own scratch keeps its first sort
      hipLaunchKernelGGL((k_msm_bin_scatter<C>), dim3(gx, ny), dim3(MSM_SORT_T), 0, st, A);
      hipLaunchKernelGGL((k_msm_bin_sort<MSM_SORT_BINT, NL>), dim3(MSM_SORT_HB, ny), dim3(MSM_SORT_BINT), 0, st, A);
    }
    return hipGetLastError();
  });
}

}  // namespace zkfl
