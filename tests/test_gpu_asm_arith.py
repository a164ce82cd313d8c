"""The assembly's row and quad arithmetic on the device, operation by operation (zkfl_debug_asm_ops,
zkfl_debug_g1_glv_mul) against Python integers and oracle/bn254.py -- run on an MI355X (-m gpu).

The field layer of both policies (csrc/row29.h RowF<P29>, Q29 of csrc/assemble.hip) on raw lazy
limbs at the edges of their ranges, quad_dbl / quad_add on points lifted to the top of the documented
coordinate ranges, the special cases of the quad policy on lifted inputs, and the GLV chains from
XYZZ points with ZZ != 1.  Every comparison is exact.  The operands of sub<K> stay inside its
precondition (row29.h; tests/test_row_bounds_cpu.py derives it): nothing is asserted outside it.
"""
import random

import pytest

import row_model as M
from oracle import bn254 as bn

pytestmark = pytest.mark.gpu

Q, R = M.Q, bn.R
ROW, QUAD = 0, 1
MUL, ADD, DBL, SUB2, SUB4, SUB6, SUB8, MONT1 = range(8)
BCAST0, PICK4, FROM_TO, ONE, ZERO, IS_ZERO2, IS_ZERO4, CANON = 11, 15, 16, 17, 18, 19, 20, 21
PDBL, PADD = 32, 33
SUB_OP = {2: SUB2, 4: SUB4, 6: SUB6, 8: SUB8}
RANGE = (8 * Q, 4 * Q, 2 * Q, 2 * Q)   # X, Y, ZZ, ZZZ between point operations

EDGE = [0, 1, Q - 1, Q] + [k * Q + d for k in range(1, 9) for d in (-1, 1)]
MAXROW = [M.LAZY - 1] * 9            # every lane at the lazy maximum
MASKROW = [M.MASK] * 9               # normalized, every limb full
ZROW = [0] * 9
SPECIAL = [MAXROW, ZROW, MASKROW] + [M.limbs(v) for v in EDGE]


def _lazy(rnd, top=1 << 29):
    return [M.lazy_limb(rnd) for _ in range(8)] + [rnd.randrange(top)]


def _row_ok(r):
    assert all(v < M.LAZY for v in r[:8]), r
    assert not any(r[9:16]), r


# ---------------------------------------------------------------------------
# field layer, row policy
# ---------------------------------------------------------------------------
def test_row_mul(gpu_ctx):
    rnd = random.Random(1)
    cases = [(a, b) for a in SPECIAL for b in SPECIAL] + [(_lazy(rnd), _lazy(rnd)) for _ in range(120)]
    cases += [(M.lazy_spread(rnd.randrange(8 * Q)), MAXROW) for _ in range(8)]
    out = gpu_ctx.asm_ops(ROW, MUL, cases)
    for (a, b), o in zip(cases, out):
        r = o[:16]
        assert M.value(r) == M.mont_int([(M.value(a), M.value(b))]), (a, b)
        _row_ok(r)
        assert r == M.row_mont([a], [M.row(b)]), (a, b)
        assert not any(o[16:])


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_row_mont(gpu_ctx, k):
    """sum_k a_k b_k 2^-261 with one reduction, a_k replicated; K = 4 at the largest lazy operands is
    the column bound of the static_assert"""
    rnd = random.Random(10 + k)
    cases = [[MAXROW] * 4 + [MAXROW] * 4, [MASKROW] * 8, [ZROW] * 8]
    cases += [[rnd.choice(SPECIAL) for _ in range(8)] for _ in range(60)]
    cases += [[_lazy(rnd) for _ in range(8)] for _ in range(140)]
    out = gpu_ctx.asm_ops(ROW, MONT1 + k - 1, cases)
    for ops, o in zip(cases, out):
        r = o[:16]
        pairs = [(ops[i], ops[4 + i]) for i in range(k)]
        assert M.value(r) == M.mont_int([(M.value(a), M.value(b)) for a, b in pairs]), ops
        _row_ok(r)
        assert r == M.row_mont([a for a, _ in pairs], [M.row(b) for _, b in pairs]), ops


def test_row_add_dbl(gpu_ctx):
    rnd = random.Random(2)
    cases = [(a, b) for a in SPECIAL for b in SPECIAL] + [(_lazy(rnd), _lazy(rnd)) for _ in range(120)]
    for (a, b), o in zip(cases, gpu_ctx.asm_ops(ROW, ADD, cases)):
        r = o[:16]
        assert M.value(r) == M.value(a) + M.value(b), (a, b)
        _row_ok(r)
        assert r == M.row_add(M.row(a), M.row(b))
    ones = SPECIAL + [_lazy(rnd) for _ in range(200)]
    for a, o in zip(ones, gpu_ctx.asm_ops(ROW, DBL, [(a,) for a in ones])):
        r = o[:16]
        assert M.value(r) == 2 * M.value(a), a
        _row_ok(r)


def _sub_cases(k, rnd):
    """operands inside sub<K>'s precondition: the formulas' sites with this K at their worst (the
    least minuend, the largest subtrahend of the interval walk), the threshold itself in its extreme
    limb configuration and from normalized / re-spread operands, edge values, random lazy limbs"""
    t = M.sub_threshold(k)
    w = M.walk()[0]
    cases = []
    for site, (sk, a_lo, b_hi) in w.worst.items():
        if sk == k:
            for f in (M.limbs, M.lazy_spread):
                cases += [(f(a_lo), f(b_hi)), (f(a_lo + 1), f(b_hi - 1))]
    assert cases
    cases.append(tuple(r[:9] for r in M.sub_edge_case(k, True)))
    for d in (t, t + 1, M.SUB_SAFE, 1 << 232):
        for av in (0, 1, Q - 1):
            cases += [(M.limbs(av), M.limbs(av + k * Q - d)), (M.lazy_spread(av), M.lazy_spread(av + k * Q - d))]
    cases += [(M.limbs(a), M.limbs(b)) for a in EDGE for b in EDGE if a + k * Q - b >= t]
    cases += [(MAXROW, ZROW), (MAXROW, MAXROW), (MASKROW, MASKROW), (ZROW, ZROW), (MAXROW, M.limbs(k * Q - Q // 2))]
    top = (k * Q) >> 232
    while len(cases) < 600:
        a, b = _lazy(rnd, 4), _lazy(rnd, top + 2)
        if M.value(a) + k * Q - M.value(b) >= t:
            cases.append((a, b))
    for a, b in cases:
        assert M.value(a) + k * Q - M.value(b) >= t and max(a[:8] + b[:8]) < M.LAZY
    rnd.shuffle(cases)   # the rows of a wave hold unrelated cases
    return cases


@pytest.mark.parametrize("k", [2, 4, 6, 8])
def test_row_sub(gpu_ctx, k):
    cases = _sub_cases(k, random.Random(20 + k))
    for (a, b), o in zip(cases, gpu_ctx.asm_ops(ROW, SUB_OP[k], cases)):
        r = o[:16]
        assert M.value(r) == M.value(a) + k * Q - M.value(b), (a, b)
        _row_ok(r)
        assert r == M.row_sub(k, M.row(a), M.row(b)), (a, b)


def test_row_bcast_pick4_from_to_consts(gpu_ctx):
    rnd = random.Random(3)
    rows = [MAXROW, MASKROW, M.limbs(Q), M.limbs(1)] + [_lazy(rnd, 1 << 32) for _ in range(60)]
    assert all(len({tuple(r) for r in rows[g:g + 4]}) == 4 for g in range(0, len(rows), 4))   # four distinct rows
    for k in range(4):
        out = gpu_ctx.asm_ops(ROW, BCAST0 + k, [(r,) for r in rows])
        for c, o in enumerate(out):
            assert o[:16] == M.row(rows[4 * (c // 4) + k]), (k, c)
    quads = [[rows[(c + i) % len(rows)] for i in (0, 5, 11, 17)] for c in range(64)]
    for c, o in enumerate(gpu_ctx.asm_ops(ROW, PICK4, quads)):
        assert o[:16] == M.row(quads[c][c % 4]), c
    # to(from(x)) == x for normalized x; to() reads row 0, whatever the other rows hold
    xs = [M.limbs(v) for v in EDGE] + [MASKROW] + [M.limbs(rnd.randrange(1 << 261)) for _ in range(43)]
    for c, o in enumerate(gpu_ctx.asm_ops(ROW, FROM_TO, [(x,) for x in xs])):
        assert o[:16] == M.row(xs[4 * (c // 4)]), c
    for o in gpu_ctx.asm_ops(ROW, ONE, [()] * 5):
        assert o[:16] == M.row(M.limbs(M.ONE))
    for o in gpu_ctx.asm_ops(ROW, ZERO, [(MAXROW,)] * 5):
        assert o[:16] == [0] * 16


def test_hook_arguments(gpu_ctx):
    from zkfl import native
    for policy, op in ((ROW, IS_ZERO2), (ROW, CANON), (QUAD, MONT1), (QUAD, FROM_TO), (2, MUL), (ROW, 22), (QUAD, 31),
                       (ROW, -1), (QUAD, 34)):
        with pytest.raises(native.ZkflError) as e:
            gpu_ctx.asm_ops(policy, op, [(ZROW,)])
        assert e.value.code == -1
    assert gpu_ctx.asm_ops(ROW, MUL, []) == []


# ---------------------------------------------------------------------------
# field layer, quad policy: every lane of the quad stores its own result
# ---------------------------------------------------------------------------
def _lanes(o):
    return [o[9 * q:9 * q + 9] for q in range(4)]


def _same(o):
    ls = _lanes(o)
    assert ls[0] == ls[1] == ls[2] == ls[3], ls
    assert not any(o[36:])
    return ls[0]


def test_quad_add_sub_mul(gpu_ctx):
    rnd = random.Random(4)
    vals = EDGE + [M.value(MASKROW), (1 << 232) - 1, 1 << 232] + [rnd.randrange(8 * Q) for _ in range(8)]
    pairs = [(a, b) for a in vals for b in vals]
    for (a, b), o in zip(pairs, gpu_ctx.asm_ops(QUAD, ADD, [(M.limbs(a), M.limbs(b)) for a, b in pairs])):
        assert _same(o) == M.limbs(a + b) == M.q_add(M.limbs(a), M.limbs(b)), (a, b)
    for k in (2, 4, 6, 8):
        ps = [(a, b) for a, b in pairs if a + k * Q - b >= 0]
        assert (0, k * Q - 1) in ps and (1, k * Q + 1) in ps   # the difference 1 and 0: no margin needed here
        for (a, b), o in zip(ps, gpu_ctx.asm_ops(QUAD, SUB_OP[k], [(M.limbs(a), M.limbs(b)) for a, b in ps])):
            assert _same(o) == M.limbs(a + k * Q - b) == M.q_sub(k, M.limbs(a), M.limbs(b)), (k, a, b)
    for (a, b), o in zip(pairs, gpu_ctx.asm_ops(QUAD, MUL, [(M.limbs(a), M.limbs(b)) for a, b in pairs])):
        assert _same(o) == M.limbs(M.mont_int([(a, b)])), (a, b)
    for a, o in zip(vals, gpu_ctx.asm_ops(QUAD, DBL, [(M.limbs(a),) for a in vals])):
        assert _same(o) == M.limbs(2 * a), a


def test_quad_is_zero_canon(gpu_ctx):
    rnd = random.Random(5)
    for k, op in ((2, IS_ZERO2), (4, IS_ZERO4)):
        vals = [j * Q + d for j in range(k + 1) for d in (-1, 0, 1) if j * Q + d >= 0]
        vals += [rnd.randrange(k * Q) for _ in range(20)]
        for v, o in zip(vals, gpu_ctx.asm_ops(QUAD, op, [(M.limbs(v),) for v in vals])):
            want = v % Q == 0 and v < k * Q         # true exactly at 0, p, .., (K - 1) p
            assert _same(o) == [int(want)] + [0] * 8, (k, v)
            assert want == M.q_is_zero(k, M.limbs(v))
    base = [0, 1, 2, Q - 2, Q - 1, (1 << 232) - 1, 1 << 232, (1 << 253) - 1] + [rnd.randrange(Q) for _ in range(24)]
    vals = [(v, k) for v in base for k in range(8)]
    for (v, k), o in zip(vals, gpu_ctx.asm_ops(QUAD, CANON, [(M.limbs(v + k * Q),) for v, k in vals])):
        assert _same(o) == M.limbs(v), (v, k)


def test_quad_bcast_pick4_consts(gpu_ctx):
    rnd = random.Random(6)
    quads = [[M.limbs(rnd.randrange(8 * Q)) for _ in range(4)] for _ in range(40)]
    for k in range(4):
        for ops, o in zip(quads, gpu_ctx.asm_ops(QUAD, BCAST0 + k, quads)):
            assert _same(o) == ops[k], k
    for ops, o in zip(quads, gpu_ctx.asm_ops(QUAD, PICK4, quads)):
        assert _lanes(o) == ops
    assert _same(gpu_ctx.asm_ops(QUAD, ONE, [()])[0]) == M.limbs(M.ONE)
    assert _same(gpu_ctx.asm_ops(QUAD, ZERO, [(MAXROW,)])[0]) == [0] * 9


# ---------------------------------------------------------------------------
# point layer
# ---------------------------------------------------------------------------
TOP = (7, 3, 1, 1)   # the largest multiples of p that keep X < 8p, Y < 4p, ZZ, ZZZ < 2p


def _points():
    rnd = random.Random(40)
    pts = [bn.mul(bn.G1_GEN, rnd.randrange(1, R)) for _ in range(40)]
    zs = [rnd.randrange(1, Q) for _ in pts]
    lifts = [TOP, (0, 0, 0, 0), (7, 0, 0, 0), (0, 3, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1)]
    lifts += [tuple(rnd.randrange(t + 1) for t in TOP) for _ in range(len(pts) - len(lifts))]
    return pts, [_lift(M.xyzz_mont(p, z), l) for p, z, l in zip(pts, zs, lifts)]


def _lift(c, l):
    r = tuple(v + i * Q for v, i in zip(c, l))
    assert all(v < b for v, b in zip(r, RANGE))
    return r


def _row_point(o):
    """-> the four coordinates' integers; the four rows hold the same words"""
    rows = [[o[64 * q + 16 * c:64 * q + 16 * c + 16] for c in range(4)] for q in range(4)]
    assert rows[0] == rows[1] == rows[2] == rows[3]
    for r in rows[0]:
        _row_ok(r)
    return tuple(M.value(r) for r in rows[0])


def _quad_point(o):
    ls = [[o[36 * q + 9 * c:36 * q + 9 * c + 9] for c in range(4)] for q in range(4)]
    assert ls[0] == ls[1] == ls[2] == ls[3]
    assert all(max(c[:8]) <= M.MASK for c in ls[0])   # normalized
    assert not any(o[144:])
    return tuple(M.value(c) for c in ls[0])


def _in(p, f):
    return [f(v) for v in p]


def _lazy_points(rnd, n):
    """XYZZ coordinates as random lazy limbs anywhere inside the documented ranges (no curve point:
    the formulas are integer identities, and their bounds hold for any operands in range)"""
    out = []
    while len(out) < 4 * n:
        b = RANGE[len(out) % 4]
        l = _lazy(rnd, (b >> 232) + 1)
        if M.value(l) < b:
            out.append(l)
    return [out[4 * i:4 * i + 4] for i in range(n)]


def test_point_ops_on_lazy_limbs(gpu_ctx):
    """quad_dbl / quad_add on coordinates whose limbs are lazy throughout (a curve point's limbs
    are almost never above 2^29): the row policy on the lazy limbs, the quad policy on the same
    integers normalized, both against the integer formulas"""
    rnd = random.Random(42)
    ps, os_ = _lazy_points(rnd, 32), _lazy_points(rnd, 32)
    assert sum(max(c[:8]) > M.MASK for p in ps for c in p) > 100   # of 128 coordinates
    ints = lambda p: tuple(M.value(c) for c in p)
    row = gpu_ctx.asm_ops(ROW, PDBL, ps)
    quad = gpu_ctx.asm_ops(QUAD, PDBL, [_in(ints(p), M.limbs) for p in ps])
    for p, ro, qo in zip(ps, row, quad):
        w = M.quad_dbl_int(ints(p))
        assert _row_point(ro) == w and _quad_point(qo) == w
        assert all(v < b for v, b in zip(w, RANGE))
    row = gpu_ctx.asm_ops(ROW, PADD, [p + o for p, o in zip(ps, os_)])
    quad = gpu_ctx.asm_ops(QUAD, PADD, [_in(ints(p) + ints(o), M.limbs) for p, o in zip(ps, os_)])
    for p, o, ro, qo in zip(ps, os_, row, quad):
        w = M.quad_add_int(ints(p), ints(o))
        assert _row_point(ro) == w and _quad_point(qo) == w
        assert all(v < b for v, b in zip(w, RANGE))


def test_point_dbl_add_both_policies(gpu_ctx):
    pts, xs = _points()
    want = [M.quad_dbl_int(x) for x in xs]
    row = gpu_ctx.asm_ops(ROW, PDBL, [_in(x, M.lazy_spread) for x in xs])
    quad = gpu_ctx.asm_ops(QUAD, PDBL, [_in(x, M.limbs) for x in xs])
    for p, w, ro, qo in zip(pts, want, row, quad):
        assert _row_point(ro) == w and _quad_point(qo) == w      # the same integers on both policies
        assert all(v < b for v, b in zip(w, RANGE))
        assert M.xyzz_affine(w) == bn.add(p, p)
    pairs = [(i, (i + 1) % len(pts)) for i in range(len(pts))]
    want = [M.quad_add_int(xs[i], xs[j]) for i, j in pairs]
    row = gpu_ctx.asm_ops(ROW, PADD, [_in(xs[i], M.lazy_spread) + _in(xs[j], M.lazy_spread) for i, j in pairs])
    quad = gpu_ctx.asm_ops(QUAD, PADD, [_in(xs[i], M.limbs) + _in(xs[j], M.limbs) for i, j in pairs])
    for (i, j), w, ro, qo in zip(pairs, want, row, quad):
        assert _row_point(ro) == w and _quad_point(qo) == w
        assert all(v < b for v, b in zip(w, RANGE))
        assert M.xyzz_affine(w) == bn.add(pts[i], pts[j])


def _equal_x_cases():
    """pairs (p, o) of lifted XYZZ forms of one point, or of a point and its negative, such that
    P = U2 + 2p - U1 is p, 2p and 3p: the three values is_zero<4> has to recognise (U1, U2 < 1.1p are
    congruent, so they differ by -p, 0 or p; a U at or above p needs a small canonical value and
    coordinates lifted to the top, hence the search).  -> {(P / p, negated): (p, o, R / p)}"""
    rnd = random.Random(41)
    found = {}
    for _ in range(20000):
        pt = bn.mul(bn.G1_GEN, rnd.randrange(1, R))
        neg = rnd.random() < 0.5
        c1 = M.xyzz_mont(pt, rnd.randrange(1, Q))
        c2 = M.xyzz_mont(bn.neg(pt) if neg else pt, rnd.randrange(1, Q))
        for l1, l2 in ((TOP, (0, 0, 0, 0)), ((0, 0, 0, 0), TOP), (TOP, TOP), ((7, 3, 0, 0), (0, 0, 1, 1)),
                       ((0, 0, 1, 1), (7, 3, 0, 0))):
            p, o = _lift(c1, l1), _lift(c2, l2)
            tr = {}
            M.quad_add_int(p, o, tr)
            assert tr["P"] % Q == 0 and (tr["R"] % Q == 0) == (not neg)
            found.setdefault((tr["P"] // Q, neg), (p, o, tr["R"]))
        if len(found) == 6:
            break
    assert sorted(found) == [(j, n) for j in (1, 2, 3) for n in (False, True)], sorted(found)
    return found


def test_quad_special_cases_on_lifted_inputs(gpu_ctx):
    pts, xs = _points()
    one = M.ONE
    infs = [(one, one, 0, 0), (one, one, Q, 0), (xs[0][0], xs[0][1], Q, Q), (xs[1][0], xs[1][1], 0, Q)]
    # infinity + P, P + infinity, infinity + infinity: the other operand comes back as it is
    cases, want = [], []
    for i, x in enumerate(xs[:8]):
        inf = infs[i % 4]
        cases += [inf + x, x + inf]
        want += [x, x]
    for a in infs:
        for b in infs:
            cases.append(a + b)
            want.append(a)
    out = gpu_ctx.asm_ops(QUAD, PADD, [_in(c, M.limbs) for c in cases])
    for c, w, o in zip(cases, want, out):
        assert _quad_point(o) == w, c
    # doubling infinity
    for a, o in zip(infs, gpu_ctx.asm_ops(QUAD, PDBL, [_in(a, M.limbs) for a in infs])):
        assert _quad_point(o) == a
    # P + P and P + (-P) through every value of U2 + 2p - U1
    found = _equal_x_cases()
    keys = sorted(found)
    out = gpu_ctx.asm_ops(QUAD, PADD, [_in(found[k][0] + found[k][1], M.limbs) for k in keys])
    for (j, neg), o in zip(keys, out):
        p, _, r = found[(j, neg)]
        got = _quad_point(o)
        if neg:
            assert got == (one, one, 0, 0), (j, r // Q)       # infinity, ZZ = 0
        else:
            assert r // Q in (1, 2, 3) and got == M.quad_dbl_int(p), (j, r // Q)
            assert M.xyzz_affine(got) == bn.add(M.xyzz_affine(p), M.xyzz_affine(p))


# ---------------------------------------------------------------------------
# the GLV chains from XYZZ points with ZZ != 1
# ---------------------------------------------------------------------------
def _scal(vals):
    return b"".join(int(v).to_bytes(32, "little") for v in vals)


def _glv(gpu_ctx, pts, ks, zs):
    out = gpu_ctx.g1_glv_mul(b"".join(bn.g1_to_bytes_std(p) for p in pts), _scal(ks), _scal(zs))
    for i, (p, k) in enumerate(zip(pts, ks)):
        want = None if p is None else bn.mul(p, k)
        assert bn.g1_from_bytes_std(out[64 * i:64 * i + 64]) == want, (i, k, zs[i])


def test_glv_mul_from_xyzz_points(gpu_ctx):
    """the edge scalars of tests/test_gpu_parity.py's GLV test, from points with a random z and with
    z = q - 1; then every single-digit scalar d 16^w: each table entry and both signs (d >= 9 is
    d - 16 with a carry into the next window), the accumulator starting at the first nonzero window"""
    rnd = random.Random(23)
    lam = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd
    ks = [0, 1, 2, 3, 8, 9, 16, R - 1, R - 2, lam, R - lam, (1 << 128) - 1, 1 << 128, (1 << 128) + 1,
          int("8" * 32, 16), int("9" * 32, 16) % R, (1 << 253) + 7, R // 2]
    pts = [bn.mul(bn.G1_GEN, rnd.randrange(1, R)) for _ in ks]
    pts[3] = None
    pts[4] = bn.neg(bn.G1_GEN)
    pts[5] = bn.G1_GEN
    _glv(gpu_ctx, pts, ks, [rnd.randrange(2, Q) for _ in ks])
    _glv(gpu_ctx, pts, ks, [Q - 1] * len(ks))
    ks = [d << (4 * w) for w in (0, 1, 30, 31) for d in range(1, 16)]
    pts = [bn.mul(bn.G1_GEN, rnd.randrange(1, R)) for _ in ks]
    _glv(gpu_ctx, pts, ks, [rnd.randrange(2, Q) for _ in ks])


def test_glv_mul_refuses_bad_points(gpu_ctx):
    from zkfl import native
    g = bn.g1_to_bytes_std(bn.G1_GEN)
    off = (1).to_bytes(32, "little") + (3).to_bytes(32, "little")         # 9 != 1 + 3
    big = (1 + Q).to_bytes(32, "little") + (2).to_bytes(32, "little")     # G with x encoded as x + q
    for bad, idx in ((off, 2), (big, 1)):
        pts = [g] * 4
        pts[idx] = bad
        for zs in (None, _scal([5] * 4)):
            with pytest.raises(native.ZkflError) as e:
                gpu_ctx.g1_glv_mul(b"".join(pts), _scal([1, 2, 3, 4]), zs)
            assert e.value.code == -1 and f"point {idx}" in str(e.value)
    for z in (0, Q):
        with pytest.raises(native.ZkflError) as e:
            gpu_ctx.g1_glv_mul(g * 2, _scal([1, 2]), _scal([7, z]))
        assert e.value.code == -1 and "z 1" in str(e.value)
