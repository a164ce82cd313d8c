"""The bound argument behind the assembly's row and quad point arithmetic (csrc/row29.h, csrc/
assemble.hip quad_dbl / quad_add / glv_row_mul), on Python integers: no GPU, no compiler.

1. RowF::sub<K>'s precondition (row29.h's header states it): the threshold is derived in
   row_model.sub_threshold and the model is run on both sides of it.
2. An interval walk of quad_dbl, quad_add and the negation of glv_row_mul from the documented
   ranges (X < 8p, Y < 4p, ZZ, ZZZ < 2p), every product bounded by p + floor(a b / 2^261) + 1:
   every sub<K> site keeps its difference above the precondition, every product its column below
   2^64, and the results land back inside the input ranges.
"""
import random

import pytest

import row_model as M

Q = M.Q
KS = (2, 4, 6, 8)   # the K of the formulas' sub<K> sites


def _exact(k, a, b):
    r = M.row_sub(k, a, b)
    return M.value(r) == M.value(a) + k * Q - M.value(b)


@pytest.mark.parametrize("k", KS)
def test_sub_threshold_both_sides(k):
    t = M.sub_threshold(k)
    # the largest difference that wraps: one below the threshold
    a, b = M.sub_edge_case(k, False)
    r = M.row_sub(k, a, b)
    assert r[8] == M.U32 and M.value(r) == t - 1 + (1 << 264)
    # the threshold itself, in the configuration that reaches it (lane 7 one higher, lanes 0..6 lowered)
    a, b = M.sub_edge_case(k, True)
    assert _exact(k, a, b)
    assert t < M.SUB_SAFE
    # lazy operands at and just above the threshold, whatever their limbs
    rnd = random.Random(k)
    for _ in range(2000):
        d = t + rnd.choice((0, 1, rnd.randrange(1 << 206), rnd.randrange(1 << 232)))
        av = rnd.choice((0, 1, rnd.randrange(Q)))
        bv = av + k * Q - d
        # both in lazy limbs where a limb can be raised
        a, b = M.row(M.lazy_spread(av)), M.row(M.lazy_spread(bv))
        assert M.row_sub_lanes_in_range(k, a, b)
        r = M.row_sub(k, a, b)
        assert M.value(r) == d and all(v < M.LAZY for v in r[:8]) and not any(r[9:])


@pytest.mark.parametrize("k", KS)
def test_sub_table_of_the_issue(k):
    """normalized operands: 0 - (K p - 1) wraps (the limb sum off by 2^264), 0 - (K p - 2^232) and
    0 - 1.3 p are exact"""
    z = M.row([0] * 9)
    r = M.row_sub(k, z, M.row(M.limbs(k * Q - 1)))
    assert r[8] == M.U32 and M.value(r) == 1 + (1 << 264)
    assert _exact(k, z, M.row(M.limbs(k * Q - (1 << 232))))
    assert _exact(k, z, M.row(M.limbs(13 * Q // 10)))


@pytest.mark.parametrize("k", KS)
def test_sub_random_lazy_limbs(k):
    """any lazy limbs: lanes stay inside 32 bits, and the result is exact whenever the difference
    is at or above the threshold"""
    rnd = random.Random(100 + k)
    t = M.sub_threshold(k)
    top = (k * Q) >> 232
    seen = 0
    for _ in range(4000):
        a = M.row([M.lazy_limb(rnd) for _ in range(8)] + [rnd.randrange(4)])
        b = M.row([M.lazy_limb(rnd) for _ in range(8)] + [rnd.randrange(top - 2, top + 2)])
        assert M.row_sub_lanes_in_range(k, a, b)
        d = M.value(a) + k * Q - M.value(b)
        if d >= t:
            seen += 1
            assert _exact(k, a, b), (a, b)
    assert seen > 1000


def test_row_mont_is_the_one_lane_integer():
    """the lane-by-lane row product has the limb sum (sum a b + d p) / 2^261 of f29_mont, lazy limbs
    below 2^29 + 2^7, lanes 9..15 zero -- at the largest lazy operands too (K = 1..4)"""
    rnd = random.Random(5)
    mx = [M.LAZY - 1] * 8 + [M.MASK]
    for kk in (1, 2, 3, 4):
        for it in range(40):
            ops = [(mx, mx) if it == 0 else
                   ([M.lazy_limb(rnd) for _ in range(8)] + [rnd.randrange(1 << 29)],
                    [M.lazy_limb(rnd) for _ in range(8)] + [rnd.randrange(1 << 29)]) for _ in range(kk)]
            r = M.row_mont([a for a, _ in ops], [M.row(b) for _, b in ops])
            assert M.value(r) == M.mont_int([(M.value(a), M.value(b)) for a, b in ops])
            assert all(v < M.LAZY for v in r[:8]) and not any(r[9:])


def test_interval_walk():
    w, d, a, ny = M.walk()
    assert set(w.margin) == set(M.SITE_K) and len(w.margin) == 10
    assert all(m >= 0 for m in w.margin.values())
    assert w.column < 1 << 64
    assert M.inside(d) and M.inside(a)          # the outputs are inputs again
    assert ny[1] - 1 < 4 * Q                    # and so is a negated Y


def test_walk_refuses_what_is_insufficient():
    """the net has no hole: a smaller K at any site, the loose bound Y < 4p at the negation, wider
    input ranges or a smaller bias in row_kp each fail the walk"""
    for site, k in M.SITE_K.items():
        # add.X3 = (R2 + 2p - PPP) + 4p - 2 Q: its minuend is itself a difference of at least 0.98 p,
        # so this one site would also hold with K = 2 (the 4 keeps X3's documented bound simple)
        with pytest.raises(AssertionError):
            M.walk(site_k={**M.SITE_K, site: 0 if site == "add.X3" else k - 2})
    w = M.Walk()
    with pytest.raises(AssertionError):
        w.neg_y((0, 4 * Q))                     # Y < 4p alone does not keep 4p - Y above the precondition
    with pytest.raises(AssertionError):
        M.walk(rng={**M.IN_RANGE, "X": 64, "ZZ": 4})   # U1 = X ZZ 2^-261 can pass 2p: U2 + 2p - U1 wraps
    with pytest.raises(AssertionError):
        M.walk(hi=1 << 29, lo=1)                # a bias below the largest lazy subtrahend limb
    # and the model agrees with the walk at such a site: sub<4> of a 2 S just below 4p + M2 wraps
    z = M.row([0] * 9)
    assert not _exact(4, z, M.row(M.limbs(4 * Q - 1)))
