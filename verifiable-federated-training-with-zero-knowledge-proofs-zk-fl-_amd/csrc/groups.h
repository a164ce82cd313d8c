// Wires that carry equal values: one MSM base per group ("grouped form").
//
// For a partition of the wires with rep(i) = the first wire of i's group, S_g = sum of the group's
// bases and u_i = w_i - w_rep(i) mod r,
//     sum_i w_i P_i  =  sum_g w_rep(g) S_g  +  sum_{i non-rep} u_i P_i
// for ANY partition and ANY witness.  Where the witness follows the partition u_i = 0, the digit sort
// drops the wire, and the group costs one base; where it does not, the wire costs what it costs in
// the plain form.  The partition is a speed hint learned from data, never a correctness assumption.
//
// This header holds the host side (plain C++, no device code: values -> partition, partition ->
// per-query member lists) and declares what csrc/groups.hip launches.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <unordered_map>
#include <vector>

namespace zkfl {

// rep describes a partition by its groups' first wires: rep[i] <= i and rep[rep[i]] == rep[i]
inline bool groups_valid(const uint32_t* rep, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (rep[i] > i || rep[rep[i]] != rep[i]) return false;
  return true;
}

// Learn a partition from one witness (w: n values of 8 words, standard form): wires whose values
// are equal and >= 2^128 share a group (below that, equality may be a coincidence of small data).
inline void groups_learn(const uint32_t* w, size_t n, std::vector<uint32_t>& rep) {
  rep.resize(n);
  std::vector<uint32_t> big;
  for (size_t i = 0; i < n; i++) {
    rep[i] = (uint32_t)i;
    const uint32_t* v = w + 8 * i;
    if (v[4] | v[5] | v[6] | v[7]) big.push_back((uint32_t)i);
  }
  std::sort(big.begin(), big.end(), [&](uint32_t a, uint32_t b) {
    const int c = memcmp(w + 8 * (size_t)a, w + 8 * (size_t)b, 32);
    return c ? c < 0 : a < b;
  });
  for (size_t k = 1; k < big.size(); k++)
    if (memcmp(w + 8 * (size_t)big[k], w + 8 * (size_t)big[k - 1], 32) == 0) rep[big[k]] = rep[big[k - 1]];
}

// Split groups by the wires' signatures (sig[i]: bit q set when query q holds a base of wire i),
// in place: afterwards a group's first wire has a base in every query in which any of its members
// has one, so one difference vector u serves all queries.  A member whose queries are among its
// first wire's stays; the others of a group regroup by signature.
inline void groups_refine(uint32_t* rep, const uint8_t* sig, size_t n) {
  std::unordered_map<uint64_t, uint32_t> first;
  for (size_t i = 0; i < n; i++) {
    const uint32_t r = rep[i];  // r <= i: rep[r] is final, and r kept itself (its signature covers its own)
    if ((sig[i] & ~sig[r]) == 0) continue;
    rep[i] = first.emplace((uint64_t)r << 8 | sig[i], (uint32_t)i).first->second;
  }
}

// One query's grouped form over its compacted base list (sidx[j] < n_vars: the wire of base j; any
// other index is an augmentation or H slot, a group of its own).  Base j of a non-representative
// wire i whose representative has a base here keeps P_i and takes the scalar index u_base + i;
// its representative's base becomes the sum over the slots members[start[r] .. start[r + 1]) and
// itself.  A wire whose representative has no base in this query stays as it is.
struct GroupQuery {
  std::vector<uint32_t> sidx;     // [n] the grouped index map
  std::vector<uint32_t> start;    // [n + 1] CSR over the base slots
  std::vector<uint32_t> members;  // slots summed into their representative's
  uint32_t groups = 0;            // slots with members
  uint32_t non_rep = 0;           // == members.size()
};

inline void groups_query(const uint32_t* rep, uint32_t n_vars, const uint32_t* sidx, size_t n, uint32_t u_base,
                         GroupQuery& q) {
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  std::vector<uint32_t> slot_of(n_vars, NONE), to(n, NONE);
  for (size_t j = 0; j < n; j++)
    if (sidx[j] < n_vars) slot_of[sidx[j]] = (uint32_t)j;
  q.sidx.assign(sidx, sidx + n);
  q.start.assign(n + 1, 0);
  q.groups = q.non_rep = 0;
  for (size_t j = 0; j < n; j++) {
    const uint32_t i = sidx[j];
    if (i >= n_vars || rep[i] == i || slot_of[rep[i]] == NONE) continue;
    to[j] = slot_of[rep[i]];
    q.sidx[j] = u_base + i;
    if (q.start[to[j] + 1]++ == 0) q.groups++;
    q.non_rep++;
  }
  for (size_t j = 0; j < n; j++) q.start[j + 1] += q.start[j];
  q.members.resize(q.non_rep);
  std::vector<uint32_t> cur(q.start.begin(), q.start.end() - 1);
  for (size_t j = 0; j < n; j++)
    if (to[j] != NONE) q.members[cur[to[j]]++] = (uint32_t)j;
}

}  // namespace zkfl

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

#include "curve.h"

namespace zkfl {

// out[j] (affine, Montgomery 2^256, zeros = infinity) = base j of the window table bases_w (its
// window-0 copy, [n][W]) plus the bases of the slots members[start[j] .. start[j + 1])
template <class F>
void group_sums(hipStream_t st, const Affine<F>* bases_w, int W, size_t n, const uint32_t* start,
                const uint32_t* members, Affine<F>* out);
// u[i] = w[i] - w[rep[i]] mod r (standard form; 0 for a representative); the count of non-zero u
// goes to *miss_out (host-coherent memory) through the slot's two counters cnt (left zero)
void group_delta(hipStream_t st, const Fr* w, const uint32_t* rep, uint32_t n, Fr* u, uint32_t* cnt,
                 uint32_t* miss_out);

}  // namespace zkfl
#endif
