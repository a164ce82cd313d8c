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

// ---- Grouped ABC: classes of equal QAP rows ("grouped ABC") ----
//
// Map every column of every A and B row through rep.  Rows whose mapped terms are equal as
// multisets of (rep column, coefficient) evaluate to the same field element whenever the witness
// follows the partition, so a proof evaluates one row per class (a reduced CSR over the classes)
// and copies the class value to the class's rows.  Where the witness does not follow, the wire
// lists say which constraints a missing wire touches: those are recomputed from the original rows.
// As for the base sets, the partition is a hint: a, b, c are the same for any partition and witness.

// The longest constraint list a non-representative wire may carry.  A wave of the marking kernel
// walks one wire's list at a time, so the list is bounded: a wire that occurs in more constraints
// carries none and sends the proof to the plain ABC when it misses.  The largest fan-out of a
// learned non-representative wire of the training circuit is 180.
constexpr uint32_t GROUP_ROWS_WIRE_CAP = 256;
// The slot's dirty list holds domain / GROUP_ROWS_DIRTY_DIV constraints (at least 64); a proof
// that dirties more runs the plain ABC.  A dirty constraint costs about a tenth of a class row's
// throughput (8 lanes per constraint, ~27 terms), so at domain / 8 the repair costs about as much
// as the reduced pass and the two together stay well under the plain pass (10 x the reduced one).
constexpr uint32_t GROUP_ROWS_DIRTY_DIV = 8;
inline uint32_t group_rows_dirty_cap(uint32_t domain) { return std::max<uint32_t>(64u, domain / GROUP_ROWS_DIRTY_DIV); }
// The slot's list of missing wires holds domain / GROUP_ROWS_MISS_DIV of them (at least 64); a
// proof with more raises the plain flag from the count alone, before any list is walked.  That
// bound counts the marking, which the one above leaves out: walking the lists of the 31,161 wires
// that miss when the training circuit's samples are rotated cost 1.3 ms per proof, for a repair
// that only just fit.  A missing wire dirties 17 constraints on average there (3.2 M list
// entries over 187 K wires), so past domain / 64 wires the dirty list would be a third full
// or more and the marking alone (4,096 walks) would cost what the reduced pass saves.
constexpr uint32_t GROUP_ROWS_MISS_DIV = 64;
inline uint32_t group_rows_miss_cap(uint32_t domain) { return std::max<uint32_t>(64u, domain / GROUP_ROWS_MISS_DIV); }
// wstart[i] carries this bit when wire i is over GROUP_ROWS_WIRE_CAP (its list is empty)
constexpr uint32_t GROUP_ROWS_OVER = 0x80000000u;

struct GroupRows {
  std::vector<uint32_t> cls;     // [2 domain] class of A row j, then of B row j
  std::vector<uint32_t> crp;     // [classes + 1] reduced CSR: one row per class
  std::vector<uint32_t> cterms;  // [Kd] packed: rep[col] | dictionary index << cshift; wide: rep[col]
  std::vector<uint32_t> ccoefs;  // wide: [Kd x 8] the terms' coefficients
  std::vector<uint32_t> wstart;  // [n_vars + 1] CSR over the wires (low 31 bits; GROUP_ROWS_OVER)
  std::vector<uint32_t> wlist;   // constraints j < domain with the wire in their A or B row, ascending
  uint32_t classes = 0;          // the empty class included, when a row is empty
  uint32_t over_cap = 0;         // non-representative wires over GROUP_ROWS_WIRE_CAP
  bool keep = false;             // Kd <= K / 2: otherwise the key runs the plain ABC
};

// rows[2 domain + 1], cols[K] and cshift as the key holds them (objects.h); coefs: the wide form's
// K x 8 words (unused when cshift != 0).  hash_bits < 64 keeps that many bits of a row's hash
// (tests: 0 makes every row collide); equal hashes are always followed by a full comparison.
inline void group_rows_build(const uint32_t* rows, uint32_t domain, const uint32_t* cols, uint32_t cshift,
                             const uint32_t* coefs, const uint32_t* rep, uint32_t n_vars, uint32_t hash_bits,
                             uint32_t wire_cap, GroupRows& g) {
  const uint32_t nrows = 2 * domain, K = rows[nrows];
  const uint32_t cmask = cshift ? (1u << cshift) - 1u : 0xFFFFFFFFu;
  // a term's key: the mapped term (packed) or rep column | coefficient id << 32 (wide)
  std::vector<uint64_t> key(K);
  std::vector<uint32_t> uniq;  // wide: the first term of each distinct coefficient
  if (cshift) {
    for (uint32_t p = 0; p < K; p++) key[p] = (cols[p] & ~cmask) | rep[cols[p] & cmask];
  } else {
    struct H32 {
      const uint32_t* c;
      size_t operator()(uint32_t p) const {
        uint64_t h = 1469598103934665603ull;
        for (int k = 0; k < 8; k++) h = (h ^ c[8 * (size_t)p + k]) * 1099511628211ull;
        return (size_t)h;
      }
    };
    struct E32 {
      const uint32_t* c;
      bool operator()(uint32_t a, uint32_t b) const { return memcmp(c + 8 * (size_t)a, c + 8 * (size_t)b, 32) == 0; }
    };
    std::unordered_map<uint32_t, uint32_t, H32, E32> ids(16, H32{coefs}, E32{coefs});
    for (uint32_t p = 0; p < K; p++) {
      const auto it = ids.emplace(p, (uint32_t)uniq.size());
      if (it.second) uniq.push_back(p);
      key[p] = (uint64_t)it.first->second << 32 | rep[cols[p]];
    }
  }
  // rows as sorted multisets, hashed
  std::vector<uint64_t> hash(nrows);
  const uint64_t hmask = hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull;
  for (uint32_t r = 0; r < nrows; r++) {
    std::sort(key.begin() + rows[r], key.begin() + rows[r + 1]);
    uint64_t h = 0x9E3779B97F4A7C15ull + (rows[r + 1] - rows[r]);
    for (uint32_t p = rows[r]; p < rows[r + 1]; p++) {
      h = (h ^ key[p]) * 0xFF51AFD7ED558CCDull;
      h ^= h >> 29;
    }
    hash[r] = h & hmask;
  }
  // classes in order of their first row: open addressing over the hashes, full comparison on a match
  uint32_t tbits = 4;
  while ((1ull << tbits) < 2ull * nrows) tbits++;
  std::vector<uint32_t> table((size_t)1 << tbits, 0xFFFFFFFFu), first;  // table: class ids; first[class]: its row
  const size_t tmask = ((size_t)1 << tbits) - 1;
  g.cls.assign(nrows, 0);
  g.crp.assign(1, 0);
  g.cterms.clear();
  g.ccoefs.clear();
  for (uint32_t r = 0; r < nrows; r++) {
    const uint32_t s = rows[r], len = rows[r + 1] - s;
    size_t slot = (size_t)((hash[r] * 0x9E3779B97F4A7C15ull) >> (64 - tbits)) & tmask;
    uint32_t c;
    for (;; slot = (slot + 1) & tmask) {
      c = table[slot];
      if (c == 0xFFFFFFFFu) break;
      const uint32_t f = first[c];
      if (hash[f] == hash[r] && rows[f + 1] - rows[f] == len &&
          std::equal(key.begin() + s, key.begin() + s + len, key.begin() + rows[f]))
        break;
    }
    if (c == 0xFFFFFFFFu) {
      c = table[slot] = (uint32_t)first.size();
      first.push_back(r);
      for (uint32_t p = s; p < s + len; p++) {
        g.cterms.push_back((uint32_t)key[p]);
        if (!cshift) {
          const uint32_t* v = coefs + 8 * (size_t)uniq[key[p] >> 32];
          g.ccoefs.insert(g.ccoefs.end(), v, v + 8);
        }
      }
      g.crp.push_back((uint32_t)g.cterms.size());
    }
    g.cls[r] = c;
  }
  g.classes = (uint32_t)first.size();
  g.keep = 2 * (uint64_t)g.cterms.size() <= K;
  // wire lists: constraint by constraint (A row, then B row), so each list ascends and a wire that
  // sits in both rows of a constraint, or twice in one, is listed once
  constexpr uint32_t NONE = 0xFFFFFFFFu;
  std::vector<uint32_t> last(n_vars, NONE), cnt(n_vars, 0);
  auto walk = [&](auto&& hit) {
    std::fill(last.begin(), last.end(), NONE);
    for (uint32_t j = 0; j < domain; j++)
      for (int ab = 0; ab < 2; ab++)
        for (uint32_t p = rows[ab * domain + j]; p < rows[ab * domain + j + 1]; p++) {
          const uint32_t i = cols[p] & cmask;
          if (rep[i] == i || last[i] == j) continue;
          last[i] = j;
          hit(i, j);
        }
  };
  walk([&](uint32_t i, uint32_t) { cnt[i]++; });
  g.wstart.assign((size_t)n_vars + 1, 0);
  g.over_cap = 0;
  for (uint32_t i = 0; i < n_vars; i++) {
    const bool over = cnt[i] > wire_cap;
    g.over_cap += over;
    if (over) cnt[i] = 0;
    g.wstart[i + 1] = g.wstart[i] + cnt[i];
    cnt[i] = over ? NONE : g.wstart[i];  // now the fill cursor
  }
  g.wlist.assign(g.wstart[n_vars], 0);
  walk([&](uint32_t i, uint32_t j) {
    if (cnt[i] != NONE) g.wlist[cnt[i]++] = j;
  });
  for (uint32_t i = 0; i < n_vars; i++)
    if (cnt[i] == NONE) g.wstart[i] |= GROUP_ROWS_OVER;
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
// The grouped ABC's marking (wstart null: none), in two steps.  k_group_delta appends every wire
// with u != 0 to the slot's list of missing wires (state[2] counts them; wires past the list's
// capacity are only counted).  k_group_mark, right behind it, raises the plain flag state[1] when
// the list overflowed; otherwise a wave takes one missing wire at a time and sets, with all its
// lanes, the bit of every constraint on the wire's list (state[GROUP_ROWS_STATE_BITS + j / 32]),
// appending each constraint it set first to dirty[] (state[0] counts them); a wire over the
// cap, or a full dirty list, raises the plain flag too.  The slot's state is zero when
// k_group_delta starts (k_proof_start).
struct GroupMark {
  const uint32_t* wstart;
  const uint32_t* wlist;
  uint32_t* state;
  uint32_t* missing;  // [miss_cap] the proof's missing wires
  uint32_t miss_cap;
  uint32_t* dirty;    // [cap] its dirty constraints
  uint32_t cap;
};
constexpr uint32_t GROUP_ROWS_STATE_BITS = 3;  // state: dirty count | plain flag | missing wires | bits
// words of a slot's state for a domain of n constraints
inline size_t group_rows_state_words(size_t n) { return GROUP_ROWS_STATE_BITS + (n + 31) / 32; }

// u[i] = w[i] - w[rep[i]] mod r (standard form; 0 for a representative); the count of non-zero u
// goes to miss_out[0] (host-coherent memory) through the slot's two counters cnt (left zero); with
// mark.wstart set, the missing wires go to mark.missing
void group_delta(hipStream_t st, const Fr* w, const uint32_t* rep, uint32_t n, Fr* u, uint32_t* cnt,
                 uint32_t* miss_out, const GroupMark& mark);
// k_group_mark (see GroupMark), behind group_delta on the same stream
void group_mark_rows(hipStream_t st, const GroupMark& mark);

}  // namespace zkfl
#endif
