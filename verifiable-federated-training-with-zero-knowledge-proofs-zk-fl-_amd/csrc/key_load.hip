// Proving keys: a parsed .zkey (csrc/host_parse.cc) made device-resident -- the QAP's CSR rows, the
// compacted and window-expanded MSM bases of every query, the NTT plan and the first proof slot --
// and the key's entry points (load, shard load, file handles, free, info).
#include <hip/hip_runtime.h>
#include <fcntl.h>
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "devbufs.h"
#include "host_parse.h"
#include "objects.h"

using namespace zkfl;

namespace {

void key_release(zkfl_key* k) {
  if (!k) return;
  key_release_slots(k);  // and its witness pipe (csrc/prove.hip)
  msm_bases_free(k->bA);
  msm_bases_free(k->bB1);
  msm_bases_free(k->bCH);
  msm_bases_free(k->bB2);
  key_groups_release(k);
  if (k->dbg_zero) (void)hipFree(k->dbg_zero);
  ntt_plan_free(k->ntt);
  void* ptrs[] = {k->rows, k->cols, k->coefs};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  zkfl_ctx* ctx = k->ctx;
  delete k;
  if (ctx) ctx_release(ctx);  // the key's reference (taken when it was made)
}

// Make a parsed key device-resident.  z's pointers address the key bytes (len of them), which
// stay valid for the call; parse_ms: the parse's duration for the load timing.
int zkey_load_parsed(zkfl_ctx* ctx, const ZkeyHost& z, size_t len, double parse_ms, uint32_t shard, uint32_t nshards,
                     zkfl_key** out) {
  if (!ctx || !out) return fail(ZKFL_E_ARG, "null argument");
  if (nshards < 1 || nshards > 1024 || shard >= nshards) return fail(ZKFL_E_ARG, "shard must be < n_shards <= 1024");
  // ZKFL_LOAD_TIMING=<file>: one JSON line per load with the host-side stages (bench.py cli_prove)
  const char* timing_path = getenv("ZKFL_LOAD_TIMING");
  std::vector<std::pair<std::string, double>> marks;
  auto t_last = std::chrono::steady_clock::now();
  auto mark = [&](const char* what) {
    if (!timing_path) return;
    const auto t = std::chrono::steady_clock::now();
    marks.emplace_back(what, std::chrono::duration<double, std::milli>(t - t_last).count());
    t_last = t;
  };
  if (timing_path) marks.emplace_back("parse", parse_ms);
  const uint32_t nVars = z.nVars, nPub = z.nPub, dom = z.dom;
  const int logn = z.logn;
  const size_t nC = z.nC;
  const size_t ncoef = z.ncoef;
  const uint32_t cshift = z.cshift;
  const std::vector<uint32_t>& rowptr = z.rowptr;
  const std::vector<uint32_t>& cols = z.cols;
  const std::vector<uint32_t>& coefs = z.coefs;
  const uint8_t* pts = z.pts;
  HIP_TRY(hipSetDevice(ctx->device), "hipSetDevice");
  hipStream_t st = ctx->st;
  zkfl_key* k = new zkfl_key();
  k->ctx = ctx;
  ctx_retain(ctx);  // dropped by key_release
  k->nVars = nVars;
  k->nPub = nPub;
  k->n = dom;
  k->logn = logn;
  k->nC = nC;
  k->K = ncoef;
  k->shard = shard;
  k->nshards = nshards;
  auto cleanup = [&](int code) {
    key_release(k);
    return code;
  };
#define KTRY(x, where)                                  \
  do {                                                  \
    hipError_t _e = (x);                                \
    if (_e != hipSuccess) return cleanup(hip_fail(_e, where)); \
  } while (0)
  KTRY(hipMalloc(&k->rows, (2 * (size_t)dom + 1) * 4), "alloc rows");
  KTRY(hipMalloc(&k->cols, (size_t)(ncoef ? ncoef : 1) * 4), "alloc cols");
  k->cshift = cshift;
  const size_t ncoefs_dev = coefs.size() / 8;
  KTRY(hipMalloc(&k->coefs, (ncoefs_dev ? ncoefs_dev : 1) * 32), "alloc coefs");
  // combined row pointers: A rows [0, dom), B rows [dom, 2 dom) over one term array (rowA[dom] == rowB[0])
  KTRY(hipMemcpyAsync(k->rows, rowptr.data(), (size_t)dom * 4, hipMemcpyHostToDevice, st), "upload");
  KTRY(hipMemcpyAsync(k->rows + dom, rowptr.data() + dom + 1, ((size_t)dom + 1) * 4, hipMemcpyHostToDevice, st),
       "upload");
  if (ncoef) {
    KTRY(hipMemcpyAsync(k->cols, cols.data(), (size_t)ncoef * 4, hipMemcpyHostToDevice, st), "upload");
    KTRY(hipMemcpyAsync(k->coefs, coefs.data(), ncoefs_dev * 32, hipMemcpyHostToDevice, st), "upload");
  }
  if (timing_path) KTRY(hipStreamSynchronize(st), "sync");
  mark("qap_upload");
  // MSM bases: infinity points dropped (e.g. ~1/3 of B1/B2 for Poseidon-heavy circuits: x^4
  // wires never appear in B), plus augmentation slots alpha1/delta1 (A), beta1/delta1 (B1),
  // beta2/delta2 (B2), delta1 (C) whose scalars are the proof's extra = [1, r, s, -rs]
  // (index map: extra_start = nVars).
  {
    const uint8_t* alpha1 = pts;
    const uint8_t* beta1 = pts + 64;
    const uint8_t* beta2 = pts + 128;
    const uint8_t* delta1 = pts + 384;
    const uint8_t* delta2 = pts + 448;
    const uint32_t X = nVars;  // extra_start
    auto nonzero = [](const uint8_t* p, size_t len) {
      for (size_t i = 0; i < len; i++)
        if (p[i]) return true;
      return false;
    };
    struct Aug {
      const uint8_t* pt;
      uint32_t sidx;
    };
    // this shard's share of a query: element i when i % nshards == shard; the augmentation
    // bases once, on shard 0
    auto mine = [&](size_t i) { return nshards == 1 || i % nshards == shard; };
    const bool aug_here = shard == 0;
    // The compacted (host) base images + index maps of every query are built on host threads at
    // once (they only read the key bytes), then uploaded and expanded back to back on the stream
    // with one synchronisation at the end (the images stay alive until then).
    struct Img {
      std::vector<uint8_t> img;
      std::vector<uint32_t> sidx;
    };
    auto image = [&](Img& o, size_t psz, const uint8_t* sec, size_t cnt, uint32_t scalar_off,
                     std::vector<Aug> aug) {
      size_t kept = 0;
      for (size_t i = 0; i < cnt; i++) kept += mine(i) && nonzero(sec + i * psz, psz);
      o.img.resize((kept + aug.size()) * psz);
      o.sidx.reserve(kept + aug.size());
      uint8_t* w = o.img.data();
      for (size_t i = 0; i < cnt; i++) {
        const uint8_t* p = sec + i * psz;
        if (!mine(i) || !nonzero(p, psz)) continue;
        memcpy(w, p, psz);
        w += psz;
        o.sidx.push_back(scalar_off + (uint32_t)i);
      }
      if (aug_here)
        for (const Aug& x : aug) {
          memcpy(w, x.pt, psz);
          w += psz;
          o.sidx.push_back(x.sidx);
        }
      o.img.resize((size_t)(w - o.img.data()));
    };
    // C (private wires -> the witness) then H (h_j -> extra[j], the slot's h vector), then delta1
    // with -rs (extra[dom + 3]: the extra slots sit behind h)
    auto image_ch = [&](Img& o) {
      Img c, h;
      image(c, 64, z.secC, nC, nPub + 1, {});
      image(h, 64, z.secH, dom, X, {{delta1, (uint32_t)(X + dom + 3)}});
      o.img.swap(c.img);
      o.img.insert(o.img.end(), h.img.begin(), h.img.end());
      o.sidx.swap(c.sidx);
      o.sidx.insert(o.sidx.end(), h.sidx.begin(), h.sidx.end());
    };
    enum { QA, QB1, QB2, QCH, NQ };
    std::vector<Img> im(NQ);
    // A in D form where that has fewer bases (ab_partition: D_i = A_i - B1_i; A - B1 also holds
    // (alpha1 - beta1) + r delta1 - s delta1), else as it is
    AbPartition ab;
    auto image_a = [&] {
      if (ctx->opts.ab_shared) {
        const AbAug aug[3] = {{alpha1, beta1, X + 0}, {delta1, nullptr, X + 1}, {nullptr, delta1, X + 2}};
        ab_partition(z.secA, z.secB1, nVars, shard, nshards, aug, 3, 2, ab);
      }
      if (ab.d_form) {
        im[QA].img.swap(ab.img);
        im[QA].sidx.swap(ab.sidx);
      } else {
        image(im[QA], 64, z.secA, nVars, 0, {{alpha1, X + 0}, {delta1, X + 1}});
      }
    };
    {
      std::vector<std::thread> th;
      th.emplace_back(image_a);
      th.emplace_back([&] { image(im[QB1], 64, z.secB1, nVars, 0, {{beta1, X + 0}, {delta1, X + 2}}); });
      th.emplace_back([&] { image(im[QB2], 128, z.secB2, nVars, 0, {{beta2, X + 0}, {delta2, X + 2}}); });
      th.emplace_back([&] { image_ch(im[QCH]); });
      for (auto& t : th) t.join();
    }
    mark("bases_host");
    size_t most = 0;
    for (const Img& o : im) most = std::max(most, o.sidx.size());
    k->msm_c = msm_pick_c(most);
    k->a_diff = ab.d_form;
    k->ab_shared = (uint32_t)ab.shared;
    // B_i(tau) G1 and B_i(tau) G2 vanish together in an honest zkey; the sort is shared only when
    // the two index maps really are equal
    k->share_b = im[QB1].sidx == im[QB2].sidx && !im[QB1].sidx.empty();
    k->front = k->share_b && nshards == 1 && logn <= ctx->opts.small_logn;
    hipError_t e;
    {
      DevBufs D;  // the images' device copies: freed once the expansions are done
      auto upload = [&](auto& mb, Img& o, bool pairs) -> hipError_t {
        ZK_CHECK(msm_bases_alloc(mb, o.sidx.size(), k->msm_c));
        if (o.sidx.empty()) return hipSuccess;
        uint8_t* d_img;
        ZK_CHECK(D.get(&d_img, o.img.size()));
        ZK_CHECK(hipMemcpyAsync(d_img, o.img.data(), o.img.size(), hipMemcpyHostToDevice, st));
        return msm_bases_set(mb, reinterpret_cast<decltype(mb.bases_w)>(d_img), o.sidx.data(), X, st, pairs);
      };
      e = upload(k->bA, im[QA], k->a_diff);
      if (e == hipSuccess) e = upload(k->bB1, im[QB1], false);
      if (e == hipSuccess) e = upload(k->bB2, im[QB2], false);
      if (e == hipSuccess) e = upload(k->bCH, im[QCH], false);
      const hipError_t es = hipStreamSynchronize(st);
      if (e == hipSuccess) e = es;
    }
    mark("bases_upload");
    if (e != hipSuccess) return cleanup(hip_fail(e, "base expansion"));
    // the index maps stay on the host: a partition's grouped sets are built from them (csrc/groups.hip)
    if (nshards == 1 && ctx->opts.groups)
      for (int q = 0; q < NQ; q++) k->q_sidx[q].swap(im[q].sidx);
  }
  KTRY(ntt_plan_alloc(k->ntt, logn, st), "ntt plan");
  if (timing_path) KTRY(hipStreamSynchronize(st), "sync");
  mark("ntt_plan");
  {
    ProofSlot* s0 = nullptr;
    int rc0 = get_slot(k, 0, &s0);  // first slot eagerly: surfaces OOM at load time
    if (rc0) return cleanup(rc0);
  }
  KTRY(hipStreamSynchronize(st), "sync");
  mark("first_slot");
  if (timing_path) {
    if (FILE* f = fopen(timing_path, "a")) {
      double total = 0;
      fprintf(f, "{\"bytes\": %zu", len);
      for (auto& m : marks) {
        fprintf(f, ", \"%s_ms\": %.3f", m.first.c_str(), m.second);
        total += m.second;
      }
      fprintf(f, ", \"a_form\": \"%s\", \"ab_shared\": %u, \"a_bases\": %zu", k->a_diff ? "D" : "A", k->ab_shared,
              k->bA.n);
      fprintf(f, ", \"total_ms\": %.3f}\n", total);
      fclose(f);
    }
  }
#undef KTRY
  *out = k;
  return ZKFL_OK;
}

int zkey_load_impl(zkfl_ctx* ctx, const uint8_t* buf, size_t len, uint32_t shard, uint32_t nshards,
                   zkfl_key** out) {
  if (!ctx || !buf || !out) return fail(ZKFL_E_ARG, "null argument");
  if (nshards < 1 || nshards > 1024 || shard >= nshards) return fail(ZKFL_E_ARG, "shard must be < n_shards <= 1024");
  const auto t0 = std::chrono::steady_clock::now();
  ZkeyHost z;
  std::string err;
  const int rc = zkey_parse(buf, len, z, err);  // csrc/host_parse.cc: header, sections, CSR + dictionary
  if (rc) return fail(rc, err);
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return zkey_load_parsed(ctx, z, len, ms, shard, nshards, out);
}
}  // namespace

extern "C" {

struct zkfl_zkey_file {
  int fd = -1;
  void* map = nullptr;
  size_t len = 0;
  ZkeyHost z;
  double parse_ms = 0;
};

int zkfl_zkey_load(zkfl_ctx* ctx, const uint8_t* buf, size_t len, zkfl_key** out) {
  return zkey_load_impl(ctx, buf, len, 0, 1, out);
}

int zkfl_zkey_file_open(const char* path, zkfl_zkey_file** out) {
  if (!path || !out) return fail(ZKFL_E_ARG, "null argument");
  *out = nullptr;
  const auto t0 = std::chrono::steady_clock::now();
  zkfl_zkey_file* f = new zkfl_zkey_file();
  f->fd = open(path, O_RDONLY | O_CLOEXEC);
  struct stat stt;
  if (f->fd < 0 || fstat(f->fd, &stt) != 0) {
    zkfl_zkey_file_close(f);
    return fail(ZKFL_E_ARG, std::string("cannot open ") + path);
  }
  f->len = (size_t)stt.st_size;
  if (f->len) {
    f->map = mmap(nullptr, f->len, PROT_READ, MAP_PRIVATE, f->fd, 0);
    if (f->map == MAP_FAILED) {
      f->map = nullptr;
      zkfl_zkey_file_close(f);
      return fail(ZKFL_E_ARG, std::string("cannot map ") + path);
    }
    (void)madvise(f->map, f->len, MADV_WILLNEED);
  }
  std::string err;
  const int rc = zkey_parse(static_cast<const uint8_t*>(f->map), f->len, f->z, err);
  if (rc) {
    zkfl_zkey_file_close(f);
    return fail(rc, err);
  }
  f->parse_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  *out = f;
  return ZKFL_OK;
}

int zkfl_zkey_load_file(zkfl_ctx* ctx, const zkfl_zkey_file* f, zkfl_key** out) {
  if (!f) return fail(ZKFL_E_ARG, "null argument");
  return zkey_load_parsed(ctx, f->z, f->len, f->parse_ms, 0, 1, out);
}

int zkfl_zkey_file_close(zkfl_zkey_file* f) {
  if (!f) return ZKFL_OK;
  if (f->map) munmap(f->map, f->len);
  if (f->fd >= 0) close(f->fd);
  delete f;
  return ZKFL_OK;
}

int zkfl_zkey_load_shard(zkfl_ctx* ctx, const uint8_t* buf, size_t len, uint32_t shard, uint32_t n_shards,
                         zkfl_key** out) {
  return zkey_load_impl(ctx, buf, len, shard, n_shards, out);
}

int zkfl_key_free(zkfl_key* key) {
  if (!key) return ZKFL_OK;
  (void)hipSetDevice(key->ctx->device);
  (void)hipStreamSynchronize(key->ctx->st);
  key_release(key);
  return ZKFL_OK;
}

int zkfl_key_info(const zkfl_key* key, uint32_t* n_vars, uint32_t* n_public, uint32_t* domain_size) {
  if (!key) return fail(ZKFL_E_ARG, "null key");
  if (n_vars) *n_vars = key->nVars;
  if (n_public) *n_public = key->nPub;
  if (domain_size) *domain_size = key->n;
  return ZKFL_OK;
}

int zkfl_key_ab_shared(const zkfl_key* key, uint32_t* d_form, uint32_t* shared_wires, uint32_t* a_bases) {
  if (!key) return fail(ZKFL_E_ARG, "null key");
  if (d_form) *d_form = key->a_diff ? 1u : 0u;
  if (shared_wires) *shared_wires = key->ab_shared;
  if (a_bases) *a_bases = (uint32_t)key->bA.n;
  return ZKFL_OK;
}

int zkfl_debug_ab_partition(const uint8_t* sec_a, const uint8_t* sec_b1, size_t n, uint32_t shard, uint32_t n_shards,
                            uint32_t* counts, uint32_t* sidx_out, uint8_t* img_out) {
  if ((n && (!sec_a || !sec_b1)) || !counts || n_shards < 1 || shard >= n_shards || n > 0x7FFFFFF0u)
    return fail(ZKFL_E_ARG, "ab_partition: bad arguments");
  // the loader's augmentation slots, with recognisable points: (1.., 2..), (3.., inf), (inf, 3..)
  uint8_t pt[3][64];
  for (int j = 0; j < 3; j++) memset(pt[j], j + 1, 64);
  const AbAug aug[3] = {{pt[0], pt[1], (uint32_t)n}, {pt[2], nullptr, (uint32_t)n + 1}, {nullptr, pt[2], (uint32_t)n + 2}};
  AbPartition ab;
  ab_partition(sec_a, sec_b1, n, shard, n_shards, aug, 3, 2, ab);
  counts[0] = ab.d_form ? 1u : 0u;
  counts[1] = (uint32_t)ab.shared;
  counts[2] = (uint32_t)ab.n_a;
  counts[3] = (uint32_t)ab.n_d;
  if (ab.d_form) {
    if (sidx_out) memcpy(sidx_out, ab.sidx.data(), ab.sidx.size() * 4);
    if (img_out) memcpy(img_out, ab.img.data(), ab.img.size());
  }
  return ZKFL_OK;
}

int zkfl_key_shard(const zkfl_key* key, uint32_t* shard, uint32_t* n_shards) {
  if (!key) return fail(ZKFL_E_ARG, "null key");
  if (shard) *shard = key->shard;
  if (n_shards) *n_shards = key->nshards;
  return ZKFL_OK;
}

}  // extern "C"
