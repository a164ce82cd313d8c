"""Model of the secure-aggregation mask engine (zkfl_secagg_mask, zkfl_secagg_aggregate), on
oracle/poseidon.py only.

    r_ij[k]  = Poseidon(K_ij, round, min(i, j), max(i, j), k)       k < dim
    sigma_ij = +1 if i < j else -1                                   (ids as unsigned integers)
    m_i      = g_i + sum_p sigma(i, p) r_ip                 mod r    (mask)
    sum      = sum_{i in S} m_i - sum_{(i, j)} sigma_ij r_ij mod r   (aggregate; (i, j) the revealed pairs)

Every hash costs milliseconds here, so `pair_mask` caches by its arguments: a pair's mask is
computed once however many clients, sums and tests use it.
"""
from functools import lru_cache

from oracle.poseidon import R, poseidon

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


@lru_cache(maxsize=None)
def pair_mask(key, rnd, lo, hi, dim):
    return tuple(poseidon([key, rnd, lo, hi, k]) for k in range(dim))


def sigma(i, j):
    return 1 if i < j else -1


def mask(cid, peer_ids, keys, rnd, gradient):
    """One client's masked update: field elements."""
    out = [g % R for g in gradient]
    for p, key in zip(peer_ids, keys):
        m = pair_mask(key, rnd, min(cid, p), max(cid, p), len(out))
        out = [(a + sigma(cid, p) * b) % R for a, b in zip(out, m)]
    return out


def aggregate(masked, pairs, rnd):
    """masked: the included clients' updates; pairs: [(in, out, key)] -> the sum, field elements."""
    dim = len(masked[0])
    out = [sum(m[k] for m in masked) % R for k in range(dim)]
    for i, j, key in pairs:
        m = pair_mask(key, rnd, min(i, j), max(i, j), dim)
        out = [(a - sigma(i, j) * b) % R for a, b in zip(out, m)]
    return out


def signed(v):
    """The server's decode: a value above r / 2 is v - r."""
    return v - R if v > R // 2 else v


def decode(values):
    """-> (signed values or all zero, out_of_range) as zkfl_secagg_aggregate reports a group."""
    s = [signed(v) for v in values]
    if all(INT64_MIN <= x <= INT64_MAX for x in s):
        return s, False
    return [0] * len(s), True


def fr_bytes(values):
    """Nested lists of field elements -> their bytes, 32 B little-endian each, in order."""
    if isinstance(values, int):
        return values.to_bytes(32, "little")
    return b"".join(fr_bytes(v) for v in values)
