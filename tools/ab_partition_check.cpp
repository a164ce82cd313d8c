// Stand-alone check of the loader's A / B1 partition (csrc/host_parse.cc ab_partition) against a
// naive model on random 64-byte records, every shard of 1..5; meant to be built with
// -fsanitize=address,undefined (tests/test_ab_shared_cpu.py does), host code only:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I include -I <pkg>/csrc
//       tools/ab_partition_check.cpp <pkg>/csrc/host_parse.cc -o ab_partition_check && ./ab_partition_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "host_parse.h"

using namespace zkfl;

int main() {
  std::mt19937 rng(20261);
  static const uint8_t zero[64] = {0};
  uint8_t pa[64], pb[64], pd[64];
  memset(pa, 1, 64);
  memset(pb, 2, 64);
  memset(pd, 3, 64);
  size_t cases = 0, d_forms = 0;
  for (int round = 0; round < 400; round++) {
    const size_t n = round < 8 ? (size_t)round : rng() % 300;
    std::vector<uint8_t> a(64 * n + 1), b(64 * n + 1);  // + 1: never a null data() at n = 0
    for (size_t i = 0; i < n; i++) {
      const unsigned kind = rng() % 6;  // 0, 1: equal; 2: different; 3: A only; 4: B only; 5: both zero
      const uint8_t va = (uint8_t)(10 + rng() % 200), vb = (uint8_t)(va + 1);
      if (kind <= 3) memset(&a[64 * i], va, 64);
      if (kind <= 1) memset(&b[64 * i], va, 64);
      if (kind == 2 || kind == 4) memset(&b[64 * i], vb, 64);
      if (kind == 2 && rng() % 2) {  // differ in one byte only
        memcpy(&b[64 * i], &a[64 * i], 64);
        b[64 * i + rng() % 64] ^= 0x80;
      }
    }
    for (uint32_t ns = 1; ns <= 5; ns++)
      for (uint32_t sh = 0; sh < ns; sh++) {
        const AbAug aug[3] = {{pa, pb, (uint32_t)n}, {pd, nullptr, (uint32_t)n + 1}, {nullptr, pd, (uint32_t)n + 2}};
        AbPartition ab;
        ab_partition(a.data(), b.data(), n, sh, ns, aug, 3, 2, ab);
        size_t n_a = sh == 0 ? 2 : 0, n_d = sh == 0 ? 3 : 0, shared = 0, k = 0;
        bool ok = true;
        for (size_t i = sh; i < n; i += ns) {
          const bool nza = memcmp(&a[64 * i], zero, 64) != 0, eq = memcmp(&a[64 * i], &b[64 * i], 64) == 0;
          n_a += nza;
          n_d += !eq;
          shared += eq && nza;
        }
        ok = ok && ab.n_a == n_a && ab.n_d == n_d && ab.shared == shared && ab.d_form == (n_d < n_a);
        if (ab.d_form) {
          ok = ok && ab.sidx.size() == n_d && ab.img.size() == 128 * n_d;
          for (size_t i = sh; ok && i < n; i += ns) {
            if (memcmp(&a[64 * i], &b[64 * i], 64) == 0) continue;
            ok = ab.sidx[k] == i && memcmp(&ab.img[128 * k], &a[64 * i], 64) == 0 &&
                 memcmp(&ab.img[128 * k + 64], &b[64 * i], 64) == 0;
            k++;
          }
          if (ok && sh == 0) {
            ok = ab.sidx[k] == n && ab.sidx[k + 1] == n + 1 && ab.sidx[k + 2] == n + 2 &&
                 memcmp(&ab.img[128 * k], pa, 64) == 0 && memcmp(&ab.img[128 * k + 64], pb, 64) == 0 &&
                 memcmp(&ab.img[128 * (k + 1)], pd, 64) == 0 && memcmp(&ab.img[128 * (k + 1) + 64], zero, 64) == 0 &&
                 memcmp(&ab.img[128 * (k + 2)], zero, 64) == 0 && memcmp(&ab.img[128 * (k + 2) + 64], pd, 64) == 0;
          }
          d_forms++;
        } else {
          ok = ok && ab.img.empty() && ab.sidx.empty();
        }
        if (!ok) {
          printf("MISMATCH round %d n %zu shard %u of %u\n", round, n, sh, ns);
          return 1;
        }
        cases++;
      }
  }
  printf("ok %zu cases, %zu in D form, no sanitizer findings\n", cases, d_forms);
  return d_forms > 100 && d_forms < cases ? 0 : 1;
}
