"""Hand-written .r1cs systems for the witness-check tests (tests/test_r1cs_parse_cpu.py,
tests/test_gpu_r1cs_check.py): a small writer of the iden3 r1cs v1 format, a Python evaluation of a
witness against such a system, and the systems themselves.

A system here is ``(n_wires, cons)`` with ``cons = [(A, B, C)]`` and each linear combination a LIST
of ``(wire, coef)`` -- a list, not a dict, so a row can name a wire twice or carry a zero
coefficient, which the builder's circuits never do.
"""
import random
import struct

from zkfl.field import R


def write_r1cs(n_wires, cons, n_pub_out=0, n_pub_in=0, n_prv_in=0, labels=True, n_labels=None) -> bytes:
    hdr = struct.pack("<I", 32) + R.to_bytes(32, "little")
    hdr += struct.pack("<IIIIQI", n_wires, n_pub_out, n_pub_in, n_prv_in, n_wires if n_labels is None else n_labels,
                       len(cons))
    body = []
    for con in cons:
        for lc in con:
            body.append(struct.pack("<I", len(lc)))
            body.extend(struct.pack("<I", k) + int(v).to_bytes(32, "little") for k, v in lc)
    secs = [(1, hdr), (2, b"".join(body))]
    if labels:
        secs.append((3, b"".join(struct.pack("<Q", i) for i in range(n_wires))))
    out = [b"r1cs", struct.pack("<II", 1, len(secs))]
    for typ, data in secs:
        out.append(struct.pack("<IQ", typ, len(data)))
        out.append(data)
    return b"".join(out)


ROW_LENGTHS = (15, 16, 17, 31, 32, 33)


def row_starts(cons):
    """-> {row length: set of (first term index mod 16)} over the A rows then the B rows, as the
    loader lays them out (C rows follow)."""
    out, pos = {}, 0
    for k in (0, 1):
        for con in cons:
            out.setdefault(len(con[k]), set()).add(pos % 16)
            pos += len(con[k])
    return out


def n_terms(cons) -> int:
    return sum(len(lc) for con in cons for lc in con)


def lists_of(cons_dicts):
    """The builder's / read_r1cs's constraints ({wire: coef} dicts) as term lists in wire order."""
    return [tuple(sorted(lc.items()) for lc in con) for con in cons_dicts]


def evaluate(cons, w):
    """-> [(a, b, c)] per constraint, Python integers mod r."""
    def ev(lc):
        return sum(c * w[k] for k, c in lc) % R
    return [(ev(A), ev(B), ev(C)) for A, B, C in cons]


def expected(cons, w):
    """-> (n_failed, first, a, b, c) as the check reports them (first .. c None when all hold)."""
    vals = evaluate(cons, w)
    bad = [j for j, (a, b, c) in enumerate(vals) if a * b % R != c]
    if not bad:
        return 0, None, None, None, None
    return (len(bad), bad[0]) + vals[bad[0]]


def product_system(m, rng, rows_a=None, rows_b=None, max_terms=40, n_free=48, distinct=False):
    """m constraints satisfied by construction: wires 1..n_free are free values, constraint j has
    random A and B rows over the free wires (their lengths from rows_a / rows_b, default random
    0..max_terms) and C_j = one fresh wire set to a_j * b_j.  distinct: every coefficient a random
    value of its own.  -> (n_wires, cons, witness)."""
    n_wires = 1 + n_free + m
    w = [1] + [rng.randrange(R) for _ in range(n_free)] + [0] * m
    cons = []
    for j in range(m):
        def row(n):
            return [(rng.randrange(0, 1 + n_free),
                     rng.randrange(R) if distinct else rng.choice((1, 2, R - 1, rng.randrange(R)))) for _ in range(n)]
        A = row(rows_a[j] if rows_a else rng.randrange(max_terms + 1))
        B = row(rows_b[j] if rows_b else rng.randrange(max_terms + 1))
        cons.append((A, B, [(1 + n_free + j, 1)]))
    for j, (a, b, _) in enumerate(evaluate(cons, w)):
        w[1 + n_free + j] = a * b % R
    return n_wires, cons, w


def edge_systems():
    """name -> (n_wires, cons, satisfying witness): the shapes the builder's circuits never have."""
    rng = random.Random(1105)
    out = {}
    x, y = rng.randrange(R), rng.randrange(R)
    # an empty A row (0 * b == 0: C must evaluate to 0), an empty B row, both beside a full constraint
    out["empty_a"] = (4, [([], [(1, 1)], []), ([(1, 1)], [(2, 1)], [(3, 1)])], [1, x, y, x * y % R])
    out["empty_b"] = (4, [([(1, 3)], [], [(0, 0)]), ([(1, 1)], [(2, 1)], [(3, 1)])], [1, x, y, x * y % R])
    # a C row of several terms: x * y == 2 z + 5 - t, t chosen to fit
    z = rng.randrange(R)
    out["multi_c"] = (5, [([(1, 1)], [(2, 1)], [(3, 2), (0, 5), (4, R - 1)])], [1, x, y, z, (2 * z + 5 - x * y) % R])
    # every C row empty: each constraint has a zero factor
    out["all_c_empty"] = (3, [([(1, 1), (0, R - 1)], [(2, 1)], []), ([(2, 7)], [(1, 1), (0, R - 1)], [])], [1, 1, y])
    # no terms at all: every witness satisfies it
    out["no_terms"] = (3, [([], [], [])] * 5, [1, x, y])
    # coefficient r - 1 against wire value r - 1, and the same wire twice in one row
    out["r_minus_1"] = (3, [([(1, R - 1)], [(1, R - 1)], [(2, 1)])], [1, R - 1, 1])
    out["wire_twice"] = (4, [([(1, 2), (1, 3), (1, R - 1)], [(2, 1), (2, 1)], [(3, 1)])], [1, x, y, 8 * x * y % R])
    # rows of 15..33 terms, each length once starting on a multiple of 16 terms (the chunk length of
    # the term walk) and once one term past it; the filler rows in between (some empty) restore the
    # alignment, and the A rows end on a multiple of 16, so the B rows repeat the pattern
    seq = []
    for n in ROW_LENGTHS:
        seq += [n, (16 - n % 16) % 16 + 1, n, (16 - (1 + n) % 16) % 16]
    out["rows_16"] = product_system(len(seq), rng, rows_a=seq, rows_b=seq)
    for m in (1, 63, 64, 65, 257):
        out[f"m{m}"] = product_system(m, rng, max_terms=6)
    return out


def wtns_of(w) -> bytes:
    from zkfl import zkey
    return zkey.wtns_bytes(w)
