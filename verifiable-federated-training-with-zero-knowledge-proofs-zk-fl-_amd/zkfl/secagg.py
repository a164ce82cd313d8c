"""Secure aggregation: mask a set of clients' updates and close a round's groups on the GPU.

The reference's clients mask their update with pairwise Poseidon masks
(tests/full_system_simulation.mjs:181-196, :558-637) and its server adds the masked updates of the
clients whose proofs verified (aggregateUpdates, :1137-1199).  The masks cancel only when every
client of a group is in that sum: each excluded client j leaves sigma_ij r_ij in the update of
every included i.  `close_groups` takes the included clients' updates and the revealed keys of the
(included, excluded) pairs and returns the sum of the included gradients -- and refuses, before any
GPU call, a group whose revealed keys are not exactly the ones that sum needs.  How a key comes to
be revealed (key agreement, secret sharing, who reveals what) is the caller's protocol.

Everything here is packing around Context.secagg_mask / Context.secagg_aggregate
(zkfl_secagg_mask, zkfl_secagg_aggregate; csrc/secagg.hip).  Field elements travel as uint8 arrays
of 32 little-endian bytes; `fr_bytes` and `fr_ints` convert.
"""

from __future__ import annotations

import numpy as np

from .field import R

_R_LIMBS = np.array([(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)], dtype=np.uint64)
HARNESS_KEY_SALT = 12345   # K_ij = Poseidon(min, max, 12345), tests/full_system_simulation.mjs:1321-1336


def fr_bytes(values) -> np.ndarray:
    """Integers (any sign, reduced mod r) -> a uint8 array of values.shape + (32,).  A uint8 array
    whose last axis is 32 passes through; an int64 array is packed without a Python loop."""
    if isinstance(values, np.ndarray) and values.dtype == np.uint8:
        if values.shape[-1:] != (32,):
            raise ValueError("a uint8 array of field elements must end in an axis of 32")
        return np.ascontiguousarray(values)
    if isinstance(values, np.ndarray) and values.dtype.kind in "iu" and values.dtype.itemsize <= 8:
        return _pack_small(values)
    arr = np.asarray(values, dtype=object)
    flat = b"".join((int(v) % R).to_bytes(32, "little") for v in arr.reshape(-1))
    return np.frombuffer(flat, dtype=np.uint8).reshape(arr.shape + (32,)).copy()


def _pack_small(v: np.ndarray) -> np.ndarray:
    """int64 / uint64 values -> field elements: x >= 0 is x, x < 0 is r - |x| (limbs with borrow)."""
    neg = (v < 0) if v.dtype.kind == "i" else np.zeros(v.shape, bool)
    mag = np.where(neg, -v, v).astype(np.uint64) if v.dtype.kind == "i" else v.astype(np.uint64)
    limbs = np.zeros(v.shape + (4,), np.uint64)
    limbs[..., 0] = mag
    if neg.any():
        m = mag[neg]                                           # r - m, limb by limb with borrow
        out = np.zeros((m.size, 4), np.uint64)
        borrow = np.zeros(m.size, np.uint64)
        for i in range(4):
            sub = (m if i == 0 else np.zeros_like(m))
            d = _R_LIMBS[i] - sub - borrow                     # wraps mod 2^64
            borrow = ((_R_LIMBS[i] < sub) | ((_R_LIMBS[i] == sub) & (borrow == 1))).astype(np.uint64)
            out[:, i] = d
        limbs[neg] = out
    return limbs.astype("<u8").view(np.uint8).reshape(v.shape + (32,))


def fr_ints(arr) -> list:
    """A uint8 array (..., 32) -> nested lists of integers."""
    arr = np.asarray(arr, dtype=np.uint8)
    if arr.ndim == 1:
        return int.from_bytes(arr.tobytes(), "little")
    return [fr_ints(a) for a in arr]


def signed(value: int) -> int:
    """The server's decode (tests/full_system_simulation.mjs:1168-1178): above r / 2 is negative."""
    return value - R if value > R // 2 else value


def mask_updates(ctx, ids, peers, keys, rnd, gradients, chunk_terms: int = 0) -> np.ndarray:
    """Mask a set of clients: client i has id ids[i], peer ids peers[i] (a list; the lists may differ
    in length, so the clients may come from many groups) with the pairwise keys keys[i] (aligned
    with peers[i]; integers, or a uint8 array (len, 32)) and the update gradients[i] (dim integers of
    any sign, or field-element bytes).  -> m_i = g_i + sum_p sigma(i, p) r_ip mod r as a uint8 array
    (n, dim, 32)."""
    n = len(ids)
    if len(peers) != n or len(keys) != n or len(gradients) != n:
        raise ValueError("ids, peers, keys and gradients must have one entry per client")
    counts = np.fromiter((len(p) for p in peers), dtype=np.uint64, count=n)
    if any(len(k) != c for k, c in zip(keys, counts)):
        raise ValueError("keys[i] must hold one key per peer of client i")
    ptr = np.zeros(n + 1, np.uint64)
    np.cumsum(counts, out=ptr[1:])
    flat_peers = np.concatenate([np.asarray(p, dtype=np.uint64) for p in peers]) if n else np.zeros(0, np.uint64)
    flat_keys = (np.concatenate([fr_bytes(k).reshape(-1, 32) for k in keys]) if n else np.zeros((0, 32), np.uint8))
    g = fr_bytes(gradients if isinstance(gradients, np.ndarray) else np.asarray(gradients, dtype=object))
    if g.ndim != 3:
        raise ValueError("gradients must be n vectors of one length")
    return ctx.secagg_mask(np.asarray(ids, dtype=np.uint64), ptr, flat_peers, flat_keys, rnd, g, g.shape[1],
                           chunk_terms)


def needed_pairs(roster, accepted) -> set:
    """The (included, excluded) pairs whose masks stay in the sum of the accepted clients."""
    acc = set(accepted)
    return {(i, j) for i in acc for j in roster if j not in acc}


def check_group(g: int, roster, accepted, revealed) -> None:
    """ValueError unless the revealed (in, out, key) triples name every needed pair exactly once
    and nothing else.  A sum with a mask left in it, or with a mask taken out that was never in
    it, is a field element of ~250 bits: refusing to produce it is what this module is for."""
    roster = [int(x) for x in roster]
    if len(set(roster)) != len(roster):
        raise ValueError(f"group {g}: an id is repeated in the roster")
    accepted = [int(x) for x in accepted]
    if len(set(accepted)) != len(accepted):
        raise ValueError(f"group {g}: an accepted id is repeated")
    if not accepted:
        raise ValueError(f"group {g}: no accepted client, nothing to aggregate")
    members = set(roster)
    stray = [i for i in accepted if i not in members]
    if stray:
        raise ValueError(f"group {g}: accepted client {stray[0]} is not in the roster")
    need = needed_pairs(roster, accepted)
    seen = set()
    for t, (i, j, _) in enumerate(revealed):
        pair = (int(i), int(j))
        if pair in seen:
            raise ValueError(f"group {g}: revealed key {t} names the pair {pair} a second time")
        if pair not in need:
            raise ValueError(f"group {g}: revealed key {t} names the pair {pair}, which is not an "
                             "(accepted, excluded) pair of the group")
        seen.add(pair)
    missing = sorted(need - seen)
    if missing:
        raise ValueError(f"group {g}: no revealed key for the pair {missing[0]} "
                         f"({len(missing)} of {len(need)} needed keys missing)")


def close_groups(ctx, groups, rnd, chunk_terms: int = 0) -> list:
    """Aggregate a round's groups.  Each group is a dict:
        "roster":   the ids of every client of the group,
        "accepted": {id: masked update} of the clients whose proofs verified (dim integers, or a
                    uint8 array (dim, 32)),
        "revealed": [(in, out, key)] -- the pairwise key of each accepted `in` and excluded `out`.
    Raises ValueError before any GPU call unless every (accepted, excluded) pair of a group has
    exactly one revealed key and no other pair is named.  -> per group {"clients": the number of
    accepted clients, "field": the sum as field elements, "sum": the signed decode (None when
    out of range), "out_of_range": a coordinate does not fit an int64}."""
    for g, grp in enumerate(groups):
        check_group(g, grp["roster"], list(grp["accepted"]), grp["revealed"])
    if not groups:
        return []
    updates = [fr_bytes(np.asarray(u, dtype=object) if not isinstance(u, np.ndarray) else u)
               for grp in groups for u in grp["accepted"].values()]
    dims = {u.shape for u in updates}
    if len(dims) != 1 or len(next(iter(dims))) != 2:
        raise ValueError("every masked update must be one vector of the same length")
    dim = updates[0].shape[0]
    member_ptr = np.zeros(len(groups) + 1, np.uint64)
    np.cumsum([len(grp["accepted"]) for grp in groups], out=member_ptr[1:])
    pair_ptr = np.zeros(len(groups) + 1, np.uint64)
    np.cumsum([len(grp["revealed"]) for grp in groups], out=pair_ptr[1:])
    triples = [t for grp in groups for t in grp["revealed"]]
    pair_in = np.array([int(t[0]) for t in triples], dtype=np.uint64)
    pair_out = np.array([int(t[1]) for t in triples], dtype=np.uint64)
    pair_keys = fr_bytes([t[2] for t in triples]) if triples else np.zeros((0, 32), np.uint8)
    sums, sg, oor = ctx.secagg_aggregate(member_ptr, np.stack(updates), pair_ptr, pair_in, pair_out, pair_keys, rnd,
                                         dim, chunk_terms)
    return [{"clients": len(grp["accepted"]), "field": fr_ints(sums[g]),
             "sum": None if oor[g] else [int(x) for x in sg[g]], "out_of_range": bool(oor[g])}
            for g, grp in enumerate(groups)]


def harness_keys(ctx, pairs) -> np.ndarray:
    """The harness's simulated key agreement, K_ij = Poseidon(min, max, 12345)
    (zkfl/clients.py::shared_key; tests/full_system_simulation.mjs:1321-1336), for an array of id
    pairs (P, 2), hashed on the GPU.  -> uint8 (P, 32)."""
    pairs = np.asarray(pairs, dtype=np.uint64).reshape(-1, 2)
    rows = np.zeros((len(pairs), 3, 4), np.uint64)
    rows[:, 0, 0] = pairs.min(axis=1)
    rows[:, 1, 0] = pairs.max(axis=1)
    rows[:, 2, 0] = HARNESS_KEY_SALT
    return ctx.poseidon_batch_raw(3, rows.astype("<u8").view(np.uint8))


def round_masked_updates(ctx, ids, gradients, rnd, group_size: int | None = None, chunk_terms: int = 0):
    """A round's masked updates under the harness's simulated keys, for rounds of a size that
    clients.federated_round cannot build on the host: ids are cut into consecutive groups of
    group_size (None: one group), every client's peers are the others of its group, and
    gradients is an (n, dim) integer array (or field-element bytes).  -> uint8 (n, dim, 32)."""
    ids = np.asarray(ids, dtype=np.uint64)
    n = len(ids)
    gs = n if group_size is None else int(group_size)
    if n and (gs < 1 or n % gs):
        raise ValueError("group_size must divide the number of clients")
    if n == 0:
        return np.zeros((0, 0, 32), np.uint8)
    grp = ids.reshape(-1, gs)                                        # (G, gs)
    keep = ~np.eye(gs, dtype=bool)
    own = np.repeat(grp[:, :, None], gs, axis=2)[:, keep]            # (G, gs * (gs - 1)), client-major
    peer = np.repeat(grp[:, None, :], gs, axis=1)[:, keep]
    peer_ids = peer.reshape(-1)
    keys = harness_keys(ctx, np.stack([own.reshape(-1), peer_ids], axis=1))
    ptr = np.arange(n + 1, dtype=np.uint64) * np.uint64(gs - 1)
    g = fr_bytes(gradients if isinstance(gradients, np.ndarray) else np.asarray(gradients, dtype=object))
    return ctx.secagg_mask(ids, ptr, peer_ids, keys, rnd, g, g.shape[1], chunk_terms)
