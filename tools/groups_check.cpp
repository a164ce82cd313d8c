// Stand-alone check of the grouped form's host side (csrc/groups.h: values -> partition, the split
// by query signature, one query's index map and member lists) against naive models on random data;
// meant to be built with -fsanitize=address,undefined (tests/test_groups_cpu.py does), host code only:
//   g++ -std=c++17 -g -O1 -fsanitize=address,undefined -I <pkg>/csrc tools/groups_check.cpp -o groups_check
//   ./groups_check
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "groups.h"

using namespace zkfl;

int main() {
  std::mt19937 rng(20262);
  size_t cases = 0, grouped = 0;
  for (int round = 0; round < 300; round++) {
    const size_t n = round < 6 ? (size_t)round : rng() % 500;
    // a pool of large values (word 4..7 set) and small ones; wires draw from it
    const size_t pool = n / 4 + 1;
    std::vector<uint32_t> vals(8 * n + 8), pv(8 * pool);
    for (size_t k = 0; k < pool; k++) {
      for (int j = 0; j < 8; j++) pv[8 * k + j] = (k % 3 == 2 && j >= 4) ? 0u : (uint32_t)rng();
      if (k % 3 != 2) pv[8 * k + 4 + rng() % 4] |= 1u;
    }
    for (size_t i = 0; i < n; i++) memcpy(&vals[8 * i], &pv[8 * (rng() % pool)], 32);
    std::vector<uint32_t> rep;
    groups_learn(vals.data(), n, rep);
    bool ok = rep.size() == n && groups_valid(rep.data(), n);
    for (size_t i = 0; ok && i < n; i++) {  // naive: the first earlier wire with the same large value
      const uint32_t* v = &vals[8 * i];
      size_t want = i;
      if (v[4] | v[5] | v[6] | v[7])
        for (size_t j = 0; j < i; j++)
          if (memcmp(&vals[8 * j], v, 32) == 0) {
            want = j;
            break;
          }
      ok = rep[i] == want;
    }
    std::vector<uint8_t> sig(n + 1);
    for (size_t i = 0; i < n; i++) sig[i] = (uint8_t)(rng() % 16);
    std::vector<uint32_t> ref(rep);
    groups_refine(ref.data(), sig.data(), n);
    ok = ok && groups_valid(ref.data(), n);
    for (size_t i = 0; ok && i < n; i++) ok = rep[ref[i]] == rep[i] && (sig[i] & ~sig[ref[i]]) == 0;
    for (int q = 0; ok && q < 4; q++) {
      std::vector<uint32_t> sidx;
      for (size_t i = 0; i < n; i++)
        if (sig[i] >> q & 1) sidx.push_back((uint32_t)i);
      sidx.push_back((uint32_t)n);  // augmentation slots: groups of their own
      sidx.push_back((uint32_t)n + 3);
      const uint32_t u_base = (uint32_t)n + 4;
      for (const std::vector<uint32_t>* part : {&rep, &ref}) {
        GroupQuery g;
        groups_query(part->data(), (uint32_t)n, sidx.data(), sidx.size(), u_base, g);
        ok = ok && g.sidx.size() == sidx.size() && g.start.size() == sidx.size() + 1 &&
             g.members.size() == g.non_rep && g.start.back() == g.non_rep;
        std::vector<uint8_t> listed(sidx.size(), 0);
        for (size_t r = 0; ok && r < sidx.size(); r++)
          for (uint32_t m = g.start[r]; ok && m < g.start[r + 1]; m++) {
            const uint32_t j = g.members[m];
            ok = j < sidx.size() && sidx[j] < n && sidx[r] < n && (*part)[sidx[j]] == sidx[r] && j != r && !listed[j];
            if (ok) listed[j] = 1;
          }
        for (size_t j = 0; ok && j < sidx.size(); j++) {
          ok = g.sidx[j] == (listed[j] ? u_base + sidx[j] : sidx[j]);
          // after the split every non-representative wire of the query is listed in it
          if (ok && part == &ref && sidx[j] < n && ref[sidx[j]] != sidx[j]) ok = listed[j] != 0;
        }
        grouped += g.non_rep;
        cases++;
      }
    }
    if (!ok) {
      printf("MISMATCH round %d n %zu\n", round, n);
      return 1;
    }
  }
  printf("ok %zu cases, %zu grouped slots, no sanitizer findings\n", cases, grouped);
  return grouped > 1000 ? 0 : 1;
}
