"""The host side of the grouped ABC (csrc/groups.h group_rows_build through zkfl_debug_group_rows: no
device): row classes, the reduced CSR and the wire lists against a short Python restatement.

Systems are random CSR matrices of up to 64 rows (A rows then B rows) over a handful of wires and
coefficients, seeded with the cases that matter: empty rows, an A and a B row that are equal, rows
that are equal only after the columns are mapped through rep, and rows that differ in one
coefficient.  Partitions: the identity, random ones, and all wires in one group."""
import ctypes as C
import random

import pytest

from zkfl import native

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
OVER = 1 << 31
U32 = C.POINTER(C.c_uint32)


def _arr(xs):
    return (C.c_uint32 * max(1, len(xs)))(*xs)


def build(rows, rep, n_vars, cshift, coefs=None, hash_bits=64, wire_cap=0):
    """rows: 2 * domain lists of (col, coefficient id) -> the builder's output as Python lists.
    cshift != 0: packed terms; cshift == 0: wide, coefs[id] the 256-bit coefficient values."""
    dom = len(rows) // 2
    rp, cols, wide = [0], [], []
    for row in rows:
        for c, k in row:
            cols.append(c | k << cshift if cshift else c)
            if not cshift:
                wide += [coefs[k] >> 32 * i & 0xFFFFFFFF for i in range(8)]
        rp.append(len(cols))
    K = len(cols)
    cls, crp, ct = _arr([0] * 2 * dom), _arr([0] * (2 * dom + 1)), _arr([0] * K)
    cc, ws, wl, info = _arr([0] * 8 * K), _arr([0] * (n_vars + 1)), _arr([0] * K), _arr([0] * 4)
    rc = native.lib().zkfl_debug_group_rows(_arr(rp), dom, _arr(cols), cshift, _arr(wide) if not cshift else None,
                                            _arr(rep), n_vars, hash_bits, wire_cap, cls, crp, ct,
                                            cc if not cshift else None, ws, wl, info)
    if rc:
        return rc
    D, Kd, nl, keep = list(info)
    crp = list(crp)[:D + 1]
    terms = list(ct)[:Kd]
    red = []
    for d in range(D):
        row = []
        for p in range(crp[d], crp[d + 1]):
            if cshift:
                row.append((terms[p] & (1 << cshift) - 1, terms[p] >> cshift))
            else:
                v = sum(cc[8 * p + i] << 32 * i for i in range(8))
                row.append((terms[p], coefs.index(v)))
        red.append(row)
    return {"cls": list(cls)[:2 * dom], "rows": red, "wstart": list(ws)[:n_vars + 1], "wlist": list(wl)[:nl],
            "K": K, "Kd": Kd, "keep": bool(keep)}


def mapped(row, rep):
    return tuple(sorted((rep[c], k) for c, k in row))


def check(rows, rep, n_vars, got, wire_cap):
    dom = len(rows) // 2
    # classes are exactly the equality classes of the mapped multisets, numbered by first row
    seen = {}
    want = [seen.setdefault(mapped(r, rep), len(seen)) for r in rows]
    assert got["cls"] == want
    assert len(got["rows"]) == len(seen)
    for m, d in seen.items():
        assert tuple(sorted(got["rows"][d])) == m
    assert got["Kd"] == sum(len(m) for m in seen) and got["keep"] == (2 * got["Kd"] <= got["K"])
    # wire lists: the constraints with a non-representative wire in their A or B row, ascending
    ws, wl = got["wstart"], got["wlist"]
    assert ws[n_vars] & OVER == 0 and len(wl) == ws[n_vars]
    for i in range(n_vars):
        lst = [j for j in range(dom) if any(c == i for c, _ in rows[j] + rows[dom + j])] if rep[i] != i else []
        start, end = ws[i] & ~OVER, ws[i + 1] & ~OVER
        if len(lst) > wire_cap:
            assert ws[i] & OVER and start == end, f"wire {i} is over the cap and must carry no list"
        else:
            assert not ws[i] & OVER and wl[start:end] == lst, f"wire {i}"


def evaluate(row, w, coef_values):
    return sum(coef_values[k] * w[c] for c, k in row) % R


def random_system(rng, dom, n_vars, n_coef, rep):
    rows = [[(rng.randrange(n_vars), rng.randrange(n_coef)) for _ in range(rng.choice([0, 1, 1, 2, 3, 5, 9]))]
            for _ in range(2 * dom)]
    if dom >= 4:
        rows[1] = []                                           # empty rows (and whatever the draw left empty)
        rows[dom + 2] = list(rows[0])                          # an A row and a B row that are equal
        rows[dom + 3] = list(reversed(rows[0]))                # ... as multisets
        grouped = [i for i in range(n_vars) if rep[i] != i]
        if grouped:                                            # equal only after the map
            i = grouped[0]
            rows[2] = [(i, 1), (rep[i], 0)]
            rows[3] = [(rep[i], 1), (i, 0)]
        base = rows[0] or [(0, 0)]
        c, k = base[0]
        rows[dom] = [(c, (k + 1) % n_coef)] + base[1:]         # differs in one coefficient
    return rows


def partitions(rng, n):
    yield "identity", list(range(n))
    for t in range(2):
        rep = list(range(n))
        for i in range(1, n):
            if rng.random() < 0.6:
                rep[i] = rep[rng.randrange(i)]
        yield f"random{t}", rep
    yield "all", [0] * n


@pytest.mark.parametrize("seed", range(6))
def test_classes_reduced_rows_and_wire_lists(seed):
    rng = random.Random(seed)
    dom = rng.choice([1, 4, 9, 32])
    n_vars, n_coef, cshift = rng.choice([3, 8, 20]), rng.choice([2, 5]), rng.choice([5, 8])
    coef_values = [rng.randrange(1, R) for _ in range(n_coef)]
    for name, rep in partitions(rng, n_vars):
        rows = random_system(rng, dom, n_vars, n_coef, rep)
        for wire_cap in (256, 2):
            for hash_bits in (64, 4, 0):
                got = build(rows, rep, n_vars, cshift, hash_bits=hash_bits, wire_cap=wire_cap)
                check(rows, rep, n_vars, got, wire_cap)
        # the wide form classes the same rows the same way
        wide = build(rows, rep, n_vars, 0, coefs=coef_values)
        check(rows, rep, n_vars, wide, 256)
        assert wide["cls"] == got["cls"]
        # a witness that follows the partition: every row's value is its class's reduced row's
        w = [rng.randrange(R) for _ in range(n_vars)]
        w = [w[rep[i]] for i in range(n_vars)]
        for r, row in enumerate(rows):
            assert evaluate(row, w, coef_values) == evaluate(got["rows"][got["cls"][r]], w, coef_values), (name, r)


def test_hand_made_system():
    # wires 0..5, rep: 3 -> 1, 4 -> 1, 5 -> 2; coefficient ids 0..2; domain 4
    rep = [0, 1, 2, 1, 1, 2]
    A = [[(1, 0), (2, 1)], [], [(3, 0), (5, 1)], [(4, 0), (5, 2)]]
    B = [[(2, 1), (4, 0)], [(0, 0)], [], [(0, 0)]]
    got = build(A + B, rep, 6, 4)
    # A0, A2 and B0 are {(1,0), (2,1)} after the map; A3 differs from them in one coefficient
    assert got["cls"] == [0, 1, 0, 2, 0, 3, 1, 3]
    assert [sorted(r) for r in got["rows"]] == [[(1, 0), (2, 1)], [], [(1, 0), (2, 2)], [(0, 0)]]
    assert got["K"] == 10 and got["Kd"] == 5 and got["keep"]
    # wire 3: constraint 2; wire 4: constraints 0 (B) and 3 (A); wire 5: constraints 2 and 3
    assert got["wstart"] == [0, 0, 0, 0, 1, 3, 5] and got["wlist"] == [2, 0, 3, 2, 3]
    capped = build(A + B, rep, 6, 4, wire_cap=1)
    assert capped["wstart"] == [0, 0, 0, 0, 1 | OVER, 1 | OVER, 1] and capped["wlist"] == [2]


def test_more_than_half_of_the_terms_left_reports_plain():
    # all rows distinct under the identity: Kd == K
    rows = [[(i % 7, 0), (i // 7, 1)] for i in range(16)]
    got = build(rows, list(range(7)), 7, 3)
    assert got["Kd"] == got["K"] == 32 and not got["keep"]
    # two copies of each row: Kd == K / 2 is still kept
    got = build(rows[:8] * 2, list(range(7)), 7, 3)
    assert got["Kd"] == 16 and got["K"] == 32 and got["keep"]
    # one more distinct term and it is not
    got = build(rows[:8] + rows[:7] + [[(6, 1), (6, 1)]], list(range(7)), 7, 3)
    assert got["Kd"] == 18 and not got["keep"]


def test_arguments():
    L = native.lib()
    assert L.zkfl_debug_group_rows(None, 0, None, 0, None, None, 0, 64, 0, None, None, None, None, None, None,
                                   None) == -1
    assert build([[(0, 0)], [(1, 0)]], [0, 0], 2, 4)["cls"] == [0, 0]
    assert build([[(0, 0)], [(2, 0)]], [0, 0], 2, 4) == -1         # column past the wires
    assert build([[(0, 0)], [(1, 0)]], [0, 2], 2, 4) == -1         # not a partition
